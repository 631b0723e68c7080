"""Worker of test_two_rank_visibility_matches_one_rank (tests/test_gpu_visibility.py): rank r of 2, both on cuda:0, gloo.

Every rank marches the starts of its band of rows over the whole grid (grid_visibility's default under a group); the bands are
gathered and the counts merged by one SUM all-reduce.  visible, hit and counts must equal what the same process computes alone -
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
    import visibility_cases as V
    from brdf_nerf_amd import grid_visibility

    dsm = V.grid_case((33, 65))                               # bands of 17 | 16 rows: marches cross the cut in both directions
    dirs = V.all_dirs()
    want = V.grid_statement(dsm, V.RES, dirs)
    u = torch.from_numpy(dsm).to(dev)
    groups = [dist.new_group([r]) for r in range(world)]      # (every rank must take part in every new_group call)
    one = grid_visibility(u, V.RES, dirs, group=groups[rank], want_hit=True)
    two = grid_visibility(u, V.RES, dirs, want_hit=True, dir_tile=5)      # data parallel: the default group
    H, cut = dsm.shape[0], 7                                  # uneven bands: 7 | 26 rows
    odd = grid_visibility(u, V.RES, dirs, rows=(0, cut) if rank == 0 else (cut, H), want_hit=True)
    same = lambda a, b: torch.equal(a["visible"], b["visible"]) and torch.equal(a["hit"], b["hit"]) and torch.equal(a["counts"], b["counts"])
    stated = np.array_equal(one["visible"].cpu().numpy(), want[0]) and np.array_equal(one["hit"].cpu().numpy(), want[1]) and \
        np.array_equal(one["counts"].numpy(), want[2])
    ok = same(one, two) and same(one, odd) and stated
    print(f"RESULT rank {rank}: blocked {int(two['counts'][:, 0].sum())} visible {int(two['counts'][:, 1].sum())} "
          f"(one rank {int(one['counts'][:, 0].sum())}, statement {int(want[2][:, 0].sum())}) -> {'ok' if ok else 'FAIL'}", flush=True)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
