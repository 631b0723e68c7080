"""Worker of test_two_ranks_reproduce_their_shards (tests/test_gpu_relight_shadows.py): rank r of 2, both on cuda:0, gloo.

Each rank seeds torch with its own seed, renders and shades its contiguous share of the rays inside relight_image_shadowed,
and rgb / depth / visibility are all-gathered along the ray axis.  Rows [lo, hi) of the gathered result must equal, bitwise, what
a single-process call on rays[lo:hi] gives after that rank's seed - every rank checks both shares.
"""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SEED = 100


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import relight_cases as RC
    import relight_shadow_cases as HC
    from test_gpu_parity import make_args
    from brdf_nerf_amd import load_model, relight_image_shadowed
    from brdf_nerf_amd.distributed import shard_bounds
    from brdf_nerf_amd.raytable import synthetic_table

    name = "rpv111_multi"                                          # per-sample shading: rows and weights are streamed too
    cfg = HC.config(name)
    args = make_args(cfg, "fp32")
    model = load_model(args)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in cfg.make_params(RC.MODEL_SEED).items()})
    models = {"coarse": model.to(dev)}
    R = 257                                                        # odd: the two shares differ in size
    rays = synthetic_table(R, device=dev, seed=RC.RAYS_SEED).data["rays"]
    suns = RC.sun_directions().to(dev)

    torch.manual_seed(SEED + rank)
    two = relight_image_shadowed(models, args, rays, suns, chunk=100)      # data parallel: the default group
    groups = [dist.new_group([r]) for r in range(world)]           # (every rank must take part in every new_group call)
    ok = tuple(two["rgb"].shape) == (suns.shape[0], R, 3) and tuple(two["visibility"].shape) == (suns.shape[0], R) and \
        tuple(two["depth"].shape) == (R,)
    worst = 0.0
    for r in range(world):
        lo, hi = shard_bounds(R, r, world)
        torch.manual_seed(SEED + r)
        one = relight_image_shadowed(models, args, rays[lo:hi], suns, chunk=100, group=groups[rank])
        ok = ok and torch.equal(two["rgb"][:, lo:hi], one["rgb"]) and torch.equal(two["depth"][lo:hi], one["depth"]) and \
            torch.equal(two["visibility"][:, lo:hi], one["visibility"])
        worst = max(worst, float((two["rgb"][:, lo:hi] - one["rgb"]).abs().max()))
    print(f"RESULT rank {rank}: {R} rays in {world} shares, rgb max |two - one| = {worst:.3e} -> {'ok' if ok else 'FAIL'}", flush=True)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
