"""Worker of test_two_rank_view_maps_match_one_rank (tests/test_gpu_maps.py): rank r of 2, both on cuda:0, gloo.

Under the default group every rank renders its half of a 12 x 10 view (60 rays: chunks of 50 and 10) after the same seed, the
rows are gathered and the counters merged by one SUM all-reduce.  One rank fed the same per-chunk draws is the same process
alone (a group of one) rendering each half as a 6 x 10 view after that seed: the gathered maps must be the two halves one after
the other and the counters their sums, bit for bit; nr_from_depth is formed from the gathered depth of the whole view.
"""
import os
import sys

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
    from brdf_nerf_amd import depth_normals, view_maps
    from test_gpu_dsm import frame
    from test_gpu_maps import CHUNK, VIEW_H, VIEW_W, view_case

    args, models, rays, fl = view_case("rpv_an")
    H, W, half = VIEW_H, VIEW_W, VIEW_H * VIEW_W // 2
    groups = [dist.new_group([r]) for r in range(world)]      # (every rank must take part in every new_group call)
    torch.manual_seed(31)
    two = view_maps(models, args, rays, H, W, frame=frame(), chunk=CHUNK, cross_rows=5, **fl)
    parts = []
    for a, b in ((0, half), (half, 2 * half)):
        torch.manual_seed(31)
        parts.append(view_maps(models, args, rays[a:b], H // 2, W, chunk=CHUNK, group=groups[rank], **fl))
    bits = lambda t: t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t
    ok = True
    for key in parts[0]["maps"]:
        one = torch.cat([p["maps"][key] for p in parts], 0)
        ok = ok and one.shape == two["maps"][key].shape and torch.equal(bits(one), bits(two["maps"][key]))
    for row in ("an", "lr"):
        ok = ok and torch.equal(parts[0]["counters"][row] + parts[1]["counters"][row], two["counters"][row])
    ok = ok and int(two["counters"]["an"][5]) == H * W * (args.n_samples + args.guided_samples)
    want = depth_normals(rays, two["maps"]["depth"], frame(), H, W)
    ok = ok and torch.equal(bits(want), bits(two["maps"]["nr_from_depth"]))
    # image row 5 ends where rank 1's share begins: its cross-section comes from rank 0's second chunk
    ok = ok and torch.equal(two["cross"]["depth"], two["maps"]["depth"][5 * W:6 * W]) and two["cross"]["z_vals"].shape[0] == W
    print(f"RESULT rank {rank}: depth_std {two['stats']['depth_std']!r} bad_nr_an% {two['stats']['bad_nr_an%']!r} -> "
          f"{'ok' if ok else 'FAIL'}", flush=True)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
