"""Worker of test_two_rank_dsm_matches_one_rank (tests/test_gpu_dsm.py): rank r of 2, both on cuda:0, gloo.

Each rank renders and splats its contiguous share of the rays inside dsm_image (shard_bounds); the depths are all-gathered and
the integer accumulators summed.  The result must equal, bitwise, what the same process computes alone for all rays - once with
the grid taken from the cloud, once with that grid passed in.  The evaluation draws are served from full-view tensors seeded on
the host (dist_relight_worker.RowDraws), so both runs see the same numbers.
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
    import dsm_cases as D
    import relight_cases as RC
    from dist_relight_worker import RowDraws
    from test_gpu_parity import make_args
    from brdf_nerf_amd import SceneFrame, dsm_image, load_model
    from brdf_nerf_amd.distributed import shard_bounds
    from brdf_nerf_amd.raytable import synthetic_table

    name = "rpv111"
    fl = RC.CASES[name][1]
    cfg = RC.config(name)
    args = make_args(cfg, "fp32")
    model = load_model(args)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in cfg.make_params(RC.MODEL_SEED).items()})
    models = {"coarse": model.to(dev)}
    R, S, G = 257, cfg.n_samples, cfg.guided_samples          # odd: the two shares differ in size
    rays = synthetic_table(R, device=dev, seed=RC.RAYS_SEED).data["rays"]
    g = torch.Generator().manual_seed(23)
    full = [torch.rand(R, S, generator=g), torch.randn(R, S, generator=g), torch.rand(R, G, generator=g), torch.randn(R, S + G, generator=g)]
    frame = SceneFrame(D.CENTER, D.RANGE)
    kw = dict(apply_brdf=fl["apply_brdf"], cos_irra_on=fl["cos_irra_on"])

    lo, hi = shard_bounds(R, rank, world)
    with RowDraws(full, [(lo, hi)], dev):
        two = dsm_image(models, args, rays, frame, **kw)               # data parallel: the default group, grid from the cloud
    with RowDraws(full, [(lo, hi)], dev):
        two_g = dsm_image(models, args, rays, frame, grid=two["grid"], **kw)      # the same grid passed in: splatted chunk by chunk
    # the single-rank result, computed by this process alone: a group of one rank
    groups = [dist.new_group([r]) for r in range(world)]           # (every rank must take part in every new_group call)
    # render_rays clamps the guided samples to the (near, far) of the FIRST ray of each call (kept as upstream), so a view is a
    # function of its chunk boundaries: the one-rank run is chunked where the two ranks split
    cut = shard_bounds(R, 0, world)[1]
    with RowDraws(full, [(0, cut), (cut, R)], dev):
        one = dsm_image(models, args, rays, frame, group=groups[rank], chunk=cut, **kw)
    bits = lambda t: t.contiguous().view(torch.int32)
    ok = True
    for res in (two, two_g):
        ok = ok and res["grid"] == one["grid"] and tuple(res["dsm"].shape) == (one["grid"].height, one["grid"].width) and \
            torch.equal(res["depth"], one["depth"]) and torch.equal(bits(res["dsm"]), bits(one["dsm"])) and \
            torch.equal(res["count"], one["count"]) and torch.equal(res["altitude"], one["altitude"]) and res["skipped"] == one["skipped"]
    ok = ok and int(one["count"].sum()) >= R - one["skipped"] > 0
    print(f"RESULT rank {rank}: rays {lo}:{hi} of {R}, grid {one['grid']}, cells filled {int((one['count'] > 0).sum())}, "
          f"deposits two {int(two['count'].sum())} one {int(one['count'].sum())} -> {'ok' if ok else 'FAIL'}", flush=True)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
