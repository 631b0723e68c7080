"""Worker of test_two_rank_ecef_dsm_matches_one_rank (tests/test_gpu_ecef.py): rank r of 2, both on cuda:0, gloo.

tests/dist_dsm_worker.py with the frame of an ECEF scene: each rank renders and splats its contiguous share of the rays inside
dsm_image (bn_dsm_splat_world), the depths are all-gathered and the integer accumulators and `skipped` summed.  The result must
equal, bitwise, what the same process computes alone for all rays - once with the grid taken from the cloud, once with that grid
passed in.  Two rows of the view are refused (a NaN origin), one in each rank's share.
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
    import ecef_cases as E
    import relight_cases as RC
    from dist_relight_worker import RowDraws
    from test_gpu_parity import make_args
    from brdf_nerf_amd import DsmAccumulator, SceneFrame, dsm_image, load_model
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
    frame = SceneFrame.ecef(E.site_frame("z21s")[0], 40.0, south=True)
    kw = dict(apply_brdf=fl["apply_brdf"], cos_irra_on=fl["cos_irra_on"])

    lo, hi = shard_bounds(R, rank, world)
    with RowDraws(full, [(lo, hi)], dev):
        two = dsm_image(models, args, rays, frame, **kw)               # data parallel: the default group, grid from the cloud
    with RowDraws(full, [(lo, hi)], dev):
        two_g = dsm_image(models, args, rays, frame, grid=two["grid"], **kw)      # the same grid passed in: splatted chunk by chunk
    # the single-rank result, computed by this process alone: a group of one rank, chunked where the two ranks split
    groups = [dist.new_group([r]) for r in range(world)]           # (every rank must take part in every new_group call)
    cut = shard_bounds(R, 0, world)[1]
    with RowDraws(full, [(0, cut), (cut, R)], dev):
        one = dsm_image(models, args, rays, frame, group=groups[rank], chunk=cut, **kw)
    bits = lambda t: t.contiguous().view(torch.int32)
    ok = frame.zone == 21
    for res in (two, two_g):
        ok = ok and res["grid"] == one["grid"] and tuple(res["dsm"].shape) == (one["grid"].height, one["grid"].width) and \
            torch.equal(res["depth"], one["depth"]) and torch.equal(bits(res["dsm"]), bits(one["dsm"])) and \
            torch.equal(res["count"], one["count"]) and torch.equal(res["altitude"], one["altitude"]) and res["skipped"] == one["skipped"]
    ok = ok and int(one["count"].sum()) >= R - one["skipped"] > 0
    # the accumulator and `skipped` themselves, with refused rows in both shares: each rank splats its share of the one-rank
    # depths, the merge is one SUM all-reduce
    depth = one["depth"].clone()
    depth[3], depth[R - 2] = float("nan"), float("inf")
    mine = DsmAccumulator(one["grid"], dev).add(rays[lo:hi], depth[lo:hi], frame).merge()
    alone = DsmAccumulator(one["grid"], dev).add(rays, depth, frame)
    ok = ok and torch.equal(mine.acc, alone.acc) and mine.skipped == alone.skipped == one["skipped"] + 2
    print(f"RESULT rank {rank}: rays {lo}:{hi} of {R}, grid {one['grid']}, cells filled {int((one['count'] > 0).sum())}, "
          f"deposits two {int(two['count'].sum())} one {int(one['count'].sum())}, skipped {mine.skipped} -> {'ok' if ok else 'FAIL'}", flush=True)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
