"""Worker of test_two_rank_sweep_matches_one_rank (tests/test_gpu_sweep.py): rank r of 2, both on cuda:0, gloo.

Every rank takes its band of rows through the march towards the three sensors and the fused launch (altitude_sweep's default under
a group); the bands are gathered and valid, wins and sums merged by one SUM all-reduce.  Every map, the counters and the mean cost
must equal what the same process computes alone - a group of one rank - bit for bit, and uneven explicit bands (rows=) must give
the same again.
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
    import sweep_cases as S
    from brdf_nerf_amd import Grid, Rpc, altitude_sweep

    ds, planes, dsm, xoff, yoff, res, zone = S.scene()        # 48 x 40: bands of 24 | 24 rows; the box spans the cut
    H, W = dsm.shape
    views = [(torch.from_numpy(p).to(dev), p.shape[1], p.shape[2], Rpc.from_dict(d)) for p, d in zip(planes, ds)]
    args = (views, torch.from_numpy(M.raised(dsm)).to(dev), Grid(xoff, yoff, res, W, H), zone, S.SCENE_OFFSETS)
    kw = dict(layout="planes", want_cost=True)
    groups = [dist.new_group([r]) for r in range(world)]      # (every rank must take part in every new_group call)
    one = altitude_sweep(*args, group=groups[rank], **kw)
    two = altitude_sweep(*args, **kw)                         # data parallel: the default group
    cut = 19                                                  # uneven bands: 19 | 29 rows
    odd = altitude_sweep(*args, rows=(0, cut) if rank == 0 else (cut, H), **kw)
    bits = lambda t: t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t
    same_nan = lambda a, b: torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a[~torch.isnan(a)], b[~torch.isnan(b)])
    tensors = ("level", "altitude", "cost_min", "count", "cost", "visible", "view_dirs", "offsets")
    plain = ("valid", "wins", "mean_cost", "cells", "skipped")
    same = lambda a, b: all(torch.equal(bits(a[k]), bits(b[k])) for k in tensors) and same_nan(a["offset"], b["offset"]) and \
        all(a[k] == b[k] for k in plain)
    want = S.SCENE_RECORD["raised"]
    ok = same(one, two) and same(one, odd) and one["wins"] == want["wins"] and one["valid"] == want["valid"] and one["cells"] == sum(want["wins"])
    print(f"RESULT rank {rank}: wins {two['wins']}, mean cost {two['mean_cost']:.6g} (one rank {one['mean_cost']:.6g}) -> "
          f"{'ok' if ok else 'FAIL'}", flush=True)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
