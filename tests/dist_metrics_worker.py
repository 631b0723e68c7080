"""Worker of test_two_rank_scores_match_one_rank (tests/test_gpu_metrics.py): rank r of 2, both on cuda:0, gloo.

Each rank renders its contiguous share of the rays inside score_view, the rows are all-gathered, each rank scores its own band
of image rows (bn_ssim_map's row range) and splats its own share of the depths; the integer SSIM triples and the DSM
accumulators are summed.  Every integer and every number must equal what the same process computes alone - a group of one
rank - for the whole view.  The evaluation draws are served from full-view tensors seeded on the host
(dist_relight_worker.RowDraws), so both runs see the same numbers.
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
    from brdf_nerf_amd import SceneFrame, load_model, score_view
    from brdf_nerf_amd.distributed import shard_bounds
    from brdf_nerf_amd.raytable import synthetic_table

    name = "rpv111"
    fl = RC.CASES[name][1]
    cfg = RC.config(name)
    args = make_args(cfg, "fp32")
    model = load_model(args)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in cfg.make_params(RC.MODEL_SEED).items()})
    models = {"coarse": model.to(dev)}
    H, W = 15, 17                                             # 255 rays: the shares of rays (128 | 127) and of rows (8 | 7) differ
    R, S, G = H * W, cfg.n_samples, cfg.guided_samples
    rays = synthetic_table(R, device=dev, seed=RC.RAYS_SEED).data["rays"]
    g = torch.Generator().manual_seed(23)
    full = [torch.rand(R, S, generator=g), torch.randn(R, S, generator=g), torch.rand(R, G, generator=g), torch.randn(R, S + G, generator=g)]
    rgbs = torch.rand(R, 3, generator=g).to(dev)
    mask = (torch.rand(H, W, generator=g) < 0.8).to(dev)
    frame = SceneFrame(D.CENTER, D.RANGE)
    kw = dict(apply_brdf=fl["apply_brdf"], cos_irra_on=fl["cos_irra_on"], mask=mask, frame=frame, window=5)

    # the single-rank result, computed by this process alone: a group of one rank
    groups = [dist.new_group([r]) for r in range(world)]           # (every rank must take part in every new_group call)
    # render_rays clamps the guided samples to the (near, far) of the FIRST ray of each call (kept as upstream), so a view is a
    # function of its chunk boundaries: the one-rank run is chunked where the two ranks split
    cut = shard_bounds(R, 0, world)[1]
    with RowDraws(full, [(0, cut), (cut, R)], dev):
        one = score_view(models, args, rays, rgbs, H, W, group=groups[rank], chunk=cut, **kw)
    grid = one["grid"]
    rows, cols = torch.meshgrid(torch.arange(grid.height, device=dev), torch.arange(grid.width, device=dev), indexing="ij")
    gt_dsm = (torch.nan_to_num(one["dsm"], nan=12.0) + 0.25 * torch.sin(0.7 * rows + 0.3 * cols)).float()
    dsm_mask = (rows + cols) % 3 != 0
    kw.update(grid=grid, gt_dsm=gt_dsm, dsm_mask=dsm_mask)
    with RowDraws(full, [(0, cut), (cut, R)], dev):
        one = score_view(models, args, rays, rgbs, H, W, group=groups[rank], chunk=cut, **kw)
    lo, hi = shard_bounds(R, rank, world)
    with RowDraws(full, [(lo, hi)], dev):
        two = score_view(models, args, rays, rgbs, H, W, **kw)         # data parallel: the default group
    bits = lambda t: t.contiguous().view(torch.int32)
    ok = torch.equal(two["ssim_sums"], one["ssim_sums"]) and int(one["ssim_sums"][0, 1]) + int(one["ssim_sums"][0, 2]) == 3 * R
    ok = ok and torch.equal(two["depth"], one["depth"]) and torch.equal(two["rgb"], one["rgb"])
    ok = ok and torch.equal(bits(two["dsm"]), bits(one["dsm"])) and torch.equal(two["count"], one["count"])
    numbers = ("psnr", "psnr_scl", "ssim", "ssim_scl", "ssim_skipped", "mae", "mae_in", "mae_out", "mae_nr", "mae_nr_in", "mae_nr_out")
    ok = ok and all(two[k] == one[k] and one[k] == one[k] for k in numbers)
    print(f"RESULT rank {rank}: rows {shard_bounds(H, rank, world)} of {H}, ssim sums two {two['ssim_sums'].tolist()} one "
          f"{one['ssim_sums'].tolist()}, ssim {one['ssim']:.6f} mae {one['mae']:.4f} mae_nr {one['mae_nr']:.4f} -> {'ok' if ok else 'FAIL'}",
          flush=True)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
