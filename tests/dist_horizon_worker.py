"""Worker of test_two_rank_horizon_matches_one_rank (tests/test_gpu_horizon.py): rank r of 2, both on cuda:0, gloo.

Every rank marches the starts of its band of rows over the whole grid (the default under a group); the bands are gathered along
the row axis and the sums merged by one SUM all-reduce.  slope, hit, svf and sums must equal what the same process computes alone -
a group of one rank - bit for bit, and the numpy statement; uneven explicit bands (rows=) must give the same again.
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
    import horizon_cases as Hc
    from brdf_nerf_amd import grid_horizon, sky_view_factor

    dsm = Hc.grid_case((33, 65))                              # bands of 17 | 16 rows: marches cross the cut in both directions
    az = Hc.all_azimuths()
    want = Hc.grid_statement(dsm, Hc.RES, az)
    sky = Hc.sky_statement(want[0])
    u = torch.from_numpy(dsm).to(dev)
    groups = [dist.new_group([r]) for r in range(world)]      # (every rank must take part in every new_group call)
    H, cut = dsm.shape[0], 7                                  # uneven bands: 7 | 26 rows
    rows = (0, cut) if rank == 0 else (cut, H)
    bits = lambda t: t.contiguous().view(torch.int32)          # float32 and int32 alike: NaN payloads included
    same = lambda a, b, keys: all(torch.equal(bits(a[k]), bits(b[k])) if a[k].dtype != torch.int64 else torch.equal(a[k], b[k]) for k in keys)
    h1 = grid_horizon(u, Hc.RES, az, group=groups[rank], want_hit=True)
    h2 = grid_horizon(u, Hc.RES, az, want_hit=True)           # data parallel: the default group
    h3 = grid_horizon(u, Hc.RES, az, rows=rows, want_hit=True)
    s1 = sky_view_factor(u, Hc.RES, az=az, group=groups[rank], want_slope=True)
    s2 = sky_view_factor(u, Hc.RES, az=az, dir_tile=5, want_slope=True)
    s3 = sky_view_factor(u, Hc.RES, az=az, rows=rows, dir_tile=3)
    known = ~np.isnan(want[0])
    stated = np.array_equal(np.isnan(h1["slope"].cpu().numpy()), ~known) and \
        np.array_equal(h1["slope"].cpu().numpy().view(np.uint32)[known], want[0].view(np.uint32)[known]) and \
        np.array_equal(h1["hit"].cpu().numpy(), want[1]) and np.array_equal(s1["sums"].numpy(), sky[2]) and \
        np.array_equal(s1["svf"].cpu().numpy().view(np.uint32)[known[0]], sky[1].view(np.uint32)[known[0]])
    ok = same(h1, h2, ("slope", "hit")) and same(h1, h3, ("slope", "hit")) and same(s1, s2, ("svf", "sums", "slope")) and \
        same(s1, s3, ("svf", "sums")) and same(s1, h1, ("slope",)) and s1["mean"] == s2["mean"] == s3["mean"] and stated
    print(f"RESULT rank {rank}: sums {s2['sums'].tolist()} (one rank {s1['sums'].tolist()}, statement {sky[2].tolist()}) "
          f"-> {'ok' if ok else 'FAIL'}", flush=True)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
