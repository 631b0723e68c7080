"""Worker of test_two_ranks_give_the_rays_of_one (tests/test_gpu_camera.py): rank r of 2, both on cuda:0, gloo.

Under the default group every rank makes shard_bounds of a view's rays (a 65 x 33 grid in chunks of 500, and 257 pixels given as
arrays, five of them not finite) and the shards are gathered; the same process alone (a group of one) makes the whole view.  The
rays must be the same bits and `skipped` the same number.
"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import camera_cases as M
    from brdf_nerf_amd.camera import Rpc, view_rays

    groups = [dist.new_group([r]) for r in range(world)]      # (every rank must take part in every new_group call)
    lo, hi = M.alt_bounds("z17")
    rpc = Rpc.from_dict(M.make_rpc("z17", 8))
    kw = dict(zone=17, sun=M.SUN, device=dev)
    args = (lo, hi, (431000.0, 3354400.0, 25.0), 250.0)
    bits = lambda t: t.contiguous().view(torch.int32)
    ok = True
    for precision in ("reference", "exact"):
        two, s2 = view_rays(rpc, 65, 33, *args, chunk=500, precision=precision, **kw)
        one, s1 = view_rays(rpc, 65, 33, *args, chunk=500, precision=precision, group=groups[rank], **kw)
        ok = ok and s1 == s2 == 0 and two.shape == (65 * 33, 11) and torch.equal(bits(one), bits(two))
    rng = np.random.default_rng(4)
    cols, rows = rng.uniform(0, 1024, 257), rng.uniform(0, 1024, 257)
    cols[[0, 63, 200]], rows[[100, 256]] = (np.nan, np.inf, -np.inf), (np.inf, np.nan)      # both shards hold some
    two, s2 = view_rays(rpc, 0, 0, *args, rows=rows, cols=cols, **kw)
    one, s1 = view_rays(rpc, 0, 0, *args, rows=rows, cols=cols, group=groups[rank], **kw)
    nan = torch.isnan(one)
    ok = ok and s1 == s2 == 5 and torch.equal(nan, torch.isnan(two)) and torch.equal(bits(one)[~nan], bits(two)[~nan])
    print(f"RESULT rank {rank}: skipped {s2} of {two.shape[0]} -> {'ok' if ok else 'FAIL'}", flush=True)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
