"""Worker of test_two_rank_relight_matches_one_rank (tests/test_gpu_relight_samples.py): rank r of 2, both on cuda:0, gloo.

Each rank renders and shades its contiguous share of the rays inside relight_image(per_sample=True) and the (K, r, 3) results
are all-gathered along the ray axis; the result must equal, bitwise, what the same process computes alone for all rays.  The
draws are served from full-view tensors as in tests/dist_relight_worker.py, whose RowDraws this worker uses.
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
    import relight_cases as RC
    import relight_sample_cases as SC
    from dist_relight_worker import RowDraws
    from test_gpu_parity import make_args
    from brdf_nerf_amd import load_model, relight_image
    from brdf_nerf_amd.distributed import shard_bounds
    from brdf_nerf_amd.raytable import synthetic_table

    name = "rpv111_nlr"
    fl = SC.flags(name)
    cfg = SC.config(name)
    args = make_args(cfg, "fp32")
    model = load_model(args)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in cfg.make_params(RC.MODEL_SEED).items()})
    models = {"coarse": model.to(dev)}
    R, S, G = 257, cfg.n_samples, cfg.guided_samples          # odd: the two shares differ in size
    rays = synthetic_table(R, device=dev, seed=RC.RAYS_SEED).data["rays"]
    g = torch.Generator().manual_seed(23)
    full = [torch.rand(R, S, generator=g), torch.randn(R, S, generator=g), torch.rand(R, G, generator=g), torch.randn(R, S + G, generator=g)]
    suns = RC.sun_directions().to(dev)
    kw = dict(per_sample=True, return_surface=True, **fl)

    lo, hi = shard_bounds(R, rank, world)
    with RowDraws(full, [(lo, hi)], dev):
        two = relight_image(models, args, rays, suns, **kw)            # data parallel: the default group
    # the single-rank result, computed by this process alone: a group of one rank, chunked where the two ranks split (the guided
    # samples' clamp window is the first ray's of each call, see tests/dist_relight_worker.py)
    groups = [dist.new_group([r]) for r in range(world)]           # (every rank must take part in every new_group call)
    cut = shard_bounds(R, 0, world)[1]
    with RowDraws(full, [(0, cut), (cut, R)], dev):
        one = relight_image(models, args, rays, suns, group=groups[rank], chunk=cut, **kw)
    ok = tuple(two["rgb"].shape) == (suns.shape[0], R, 3) and torch.equal(two["rgb"], one["rgb"]) and \
        torch.equal(two["depth"], one["depth"]) and torch.equal(two["surface"].rows, one["surface"].rows) and \
        torch.equal(two["surface"].weights, one["surface"].weights) and tuple(two["surface"].rows.shape[:2]) == (R, S + G)
    print(f"RESULT rank {rank}: rays {lo}:{hi} of {R}, rgb max |two - one| = {float((two['rgb'] - one['rgb']).abs().max()):.3e} -> "
          f"{'ok' if ok else 'FAIL'}", flush=True)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
