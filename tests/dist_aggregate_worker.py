"""Worker of test_two_rank_aggregation_matches_one_rank (tests/test_gpu_aggregate.py): rank r of 2, both on cuda:0, gloo.

Rank r runs the directions whose bit index is r modulo 2 - bits 0, 2, 4, 6 or 1, 3, 5, 7; with 4 paths bits 0, 2 or 1, 3 -, one SUM
all-reduce of `sum` merges them, and every rank picks.  Every output must equal what the same process computes alone - a group of
one rank - bit for bit, through aggregate_costs and through altitude_sweep(aggregate=...), whose row bands are gathered first.
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
    import aggregate_cases as A
    import mosaic_cases as M
    import sweep_cases as S
    from brdf_nerf_amd import Grid, Rpc, aggregate_costs, altitude_sweep

    groups = [dist.new_group([r]) for r in range(world)]      # (every rank must take part in every new_group call)
    bits = lambda t: t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t
    same_nan = lambda a, b: torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a[~torch.isnan(a)], b[~torch.isnan(b)])
    ok = True

    H, W, Z = 33, 65, 65                                      # a volume with every special, two levels per lane
    cost = torch.from_numpy(A.random_volume(Z, H, W)).to(dev)
    want = A.aggregate(cost.cpu().numpy(), 0.25, 256, 2048)
    for paths in (8, 4):
        kw = dict(quantum=0.25, paths=paths, want_sum=True)
        one = aggregate_costs(cost, 64.0, 512.0, group=groups[rank], **kw)
        two = aggregate_costs(cost, 64.0, 512.0, **kw)        # the default group: the directions split over the ranks
        ok &= all(torch.equal(one[k], two[k]) for k in ("level", "sum_min", "sum"))
        ok &= all(one[k] == two[k] for k in ("wins", "cells", "sum_total", "valid_pairs", "capped", "quantum", "P1", "P2"))
        if paths == 8:
            ok &= np.array_equal(two["level"].cpu().numpy(), want["level"]) and two["wins"] == want["wins"]
            ok &= np.array_equal(two["sum"].cpu().numpy(), np.moveaxis(want["sum"], -1, 0)) and (two["P1"], two["P2"]) == (256, 2048)

    ds, planes, dsm, xoff, yoff, res, zone = S.scene()        # 48 x 40: bands of 24 | 24 rows, gathered before the paths
    rng = np.random.default_rng(7)
    noisy = [(p + rng.normal(0, A.SCENE_NOISE * float(p.max() - p.min()), p.shape)).astype(np.float32) for p in planes]
    views = [(torch.from_numpy(p).to(dev), p.shape[1], p.shape[2], Rpc.from_dict(d)) for p, d in zip(noisy, ds)]
    args = (views, torch.from_numpy(M.raised(dsm)).to(dev), Grid(xoff, yoff, res, dsm.shape[1], dsm.shape[0]), zone, S.SCENE_OFFSETS)
    kw = dict(layout="planes", want_cost=True, aggregate=dict(p1=A.SCENE_P1, p2=A.SCENE_P2))
    one = altitude_sweep(*args, group=groups[rank], **kw)
    two = altitude_sweep(*args, **kw)
    tensors = ("level", "level_wta", "sum_min", "altitude", "cost_min", "count", "cost", "visible", "view_dirs", "offsets")
    ok &= all(torch.equal(bits(one[k]), bits(two[k])) for k in tensors) and same_nan(one["offset"], two["offset"])
    ok &= all(one[k] == two[k] for k in ("valid", "wins", "mean_cost", "cells", "skipped"))
    roof, ground, astray, none = S.scene_counts({"level": two["level"].cpu().numpy()}, dsm, 2)
    wta = S.scene_counts({"level": two["level_wta"].cpu().numpy()}, dsm, 2)
    ok &= wta[2] >= 500 and astray * 4 <= wta[2] and roof >= wta[0]
    print(f"RESULT rank {rank}: wins {two['wins']}, roof {roof}, astray {astray} of {ground} -> {'ok' if ok else 'FAIL'}", flush=True)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
