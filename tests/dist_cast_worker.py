"""Worker of test_two_rank_cast_matches_one_rank (tests/test_gpu_cast.py): rank r of 2, both on cuda:0, gloo.

Every rank casts its ViewWalk share of the view's rays over the whole raster (cast_rays' default under a group); the rows are
gathered and the counts merged by one SUM all-reduce.  depth, state, cell, nan_cells and counts must equal what the same process
computes alone - a group of one rank - bit for bit, and the numpy statement; chunks that do not divide a rank's share must give
the same again.
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
    import cast_cases as K
    from brdf_nerf_amd import Grid, SceneFrame, cast_rays

    dsm = K.grid_case((33, 65))                               # NaN, +-inf and -0.0 cells
    xoff, yoff = K.ORIGINS["utm"]
    rays, center, rng = K.scatter_view(257, dsm, xoff, yoff, 45.0, 17.0)      # shares of 129 | 128 rays
    want = K.cast_statement(rays, center, rng, dsm, xoff, yoff, K.RES)
    frame, grid = SceneFrame(center, rng), Grid(xoff, yoff, K.RES, 65, 33)
    r, d = torch.from_numpy(rays).to(dev), torch.from_numpy(dsm).to(dev)
    groups = [dist.new_group([k]) for k in range(world)]      # (every rank must take part in every new_group call)
    one = cast_rays(r, frame, d, grid, group=groups[rank])
    two = cast_rays(r, frame, d, grid)                        # data parallel: the default group
    odd = cast_rays(r, frame, d, grid, chunk=50)
    keys = ("depth", "state", "cell", "nan_cells")
    same = lambda a, b: all(torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in keys) and a["counts"] == b["counts"]
    stated = all(np.array_equal(one[k].cpu().numpy().view(np.uint8), w.view(np.uint8)) for k, w in zip(keys, want)) and \
        one["counts"] == want[4].tolist()
    ok = same(one, two) and same(one, odd) and stated
    print(f"RESULT rank {rank}: counts {two['counts']} (one rank {one['counts']}, statement {want[4].tolist()}) -> "
          f"{'ok' if ok else 'FAIL'}", flush=True)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
