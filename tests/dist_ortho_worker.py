"""Worker of test_two_rank_ortho_matches_one_rank (tests/test_gpu_ortho.py): rank r of 2, both on cuda:0, gloo.

Each rank runs pass 1 on its contiguous share of the block scene's rays, the top grids merge by a MAX all-reduce, each rank runs
pass 2 on its share, and the accumulators and counters merge by a SUM all-reduce.  Top, acc, the counters and the resolved maps
must equal, bitwise, what the same process computes alone for all rays.  Two rows are bad, one in each share: a NaN depth and an
inf feature.
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
    import dsm_cases as D
    import ortho_cases as O
    from brdf_nerf_amd import Grid, OrthoAccumulator, SceneFrame
    from brdf_nerf_amd.distributed import shard_bounds

    s = O.block_scene()
    rays, depth, feats = (torch.from_numpy(np.array(s[k])).to(dev) for k in ("rays", "depth", "features"))
    R = rays.shape[0]
    depth[3] = float("nan")
    feats[R - 2, 1] = float("inf")
    frame, grid = SceneFrame(D.CENTER, D.RANGE), Grid(*s["grid"])
    lo, hi = shard_bounds(R, rank, world)
    ok = True
    for mode in ("top", "mean"):
        mine = OrthoAccumulator(grid, dev, 3, mode=mode, band=O.BLOCK_BAND)
        alone = OrthoAccumulator(grid, dev, 3, mode=mode, band=O.BLOCK_BAND)
        if mode == "top":
            mine.add_top(rays[lo:hi], depth[lo:hi], frame).merge_top()
            alone.add_top(rays, depth, frame)
            ok = ok and torch.equal(mine.top, alone.top)
        mine.add(rays[lo:hi], depth[lo:hi], frame, feats[lo:hi]).merge()
        alone.add(rays, depth, frame, feats)
        ok = ok and torch.equal(mine.acc, alone.acc) and (mine.skipped, mine.bad_features, mine.culled) == (alone.skipped, alone.bad_features, alone.culled)
        ok = ok and mine.skipped == 1 and mine.bad_features == 1 and (mine.culled > 0) == (mode == "top")
        ok = ok and all(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)) for a, b in zip(mine.result(), alone.result()))
    print(f"RESULT rank {rank}: rays {lo}:{hi} of {R}, deposits {int(alone.acc[..., 1].sum())}, culled in top mode > 0 -> {'ok' if ok else 'FAIL'}",
          flush=True)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
