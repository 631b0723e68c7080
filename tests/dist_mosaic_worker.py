"""Worker of test_two_rank_orthomosaic_matches_one_rank (tests/test_gpu_mosaic.py): rank r of 2, both on cuda:0, gloo.

Every rank takes its band of rows through the march towards the three sensors and the fused launch (orthomosaic's default under a
group); the bands are gathered and counts and sums merged by one SUM all-reduce.  Every map, the counts and the consistency must
equal what the same process computes alone - a group of one rank - bit for bit, and uneven explicit bands (rows=) must give the
same again.
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
    import mosaic_cases as M
    import orthophoto_cases as O
    from brdf_nerf_amd import Grid, Rpc, orthomosaic

    ds, dsm, xoff, yoff, res, zone = M.box_views()            # 48 x 40: bands of 24 | 24 rows; the box spans the cut
    H, W = dsm.shape
    Hi, Wi = O.SCENE_IMAGE
    views = [(torch.from_numpy(O.to_layout(O.linear_image(Hi, Wi, 3) + k, "image")).to(dev), Hi, Wi, Rpc.from_dict(d))
             for k, d in enumerate(ds)]
    args = (views, torch.from_numpy(dsm).to(dev), Grid(xoff, yoff, res, W, H), zone)
    groups = [dist.new_group([r]) for r in range(world)]      # (every rank must take part in every new_group call)
    one = orthomosaic(*args, group=groups[rank])
    two = orthomosaic(*args)                                  # data parallel: the default group
    cut = 19                                                  # uneven bands: 19 | 29 rows
    odd = orthomosaic(*args, rows=(0, cut) if rank == 0 else (cut, H))
    bits = lambda t: t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t
    tensors = ("best_rgb", "mean", "std", "count", "best", "visible", "view_dirs")
    plain = ("rank", "counts", "consistency", "cells", "skipped")
    same = lambda a, b: all(torch.equal(bits(a[k]), bits(b[k])) for k in tensors) and all(a[k] == b[k] for k in plain)
    hist = torch.bincount(one["count"].reshape(-1).long(), minlength=4).tolist()
    ok = same(one, two) and same(one, odd) and min(hist) >= 10 and one["cells"] == hist[2] + hist[3] and \
        sum(one["counts"][s][0] for s in M.STATES) == H * W
    print(f"RESULT rank {rank}: seen by 0 to 3 views {hist}, consistency {two['consistency']:.6g} (one rank {one['consistency']:.6g}) -> "
          f"{'ok' if ok else 'FAIL'}", flush=True)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
