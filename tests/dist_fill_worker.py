"""Worker of test_two_rank_fill_matches_one_rank (tests/test_gpu_fill.py): rank r of 2, both on cuda:0, gloo.

Every rank runs the column pass on the whole grid and fills its band of rows (fill_holes' default under a group); the bands are
gathered and (holes, largest d2) merged by one SUM and one MAX all-reduce.  filled, source, holes and max_dist must equal what
the same process computes alone - a group of one rank - bit for bit, and uneven explicit bands (rows=) must give the same again.
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
    import fill_cases as F
    from brdf_nerf_amd import fill_holes

    u = torch.from_numpy(F.golden("holes30")["u"]).to(dev)    # 104 x 112: bands of 52 | 52 rows; the NaN patch spans the cut
    groups = [dist.new_group([r]) for r in range(world)]      # (every rank must take part in every new_group call)
    one = fill_holes(u, group=groups[rank], want_source=True)
    two = fill_holes(u, want_source=True)                     # data parallel: the default group
    H, cut = u.shape[0], 37                                   # uneven bands: 37 | 67 rows
    odd = fill_holes(u, rows=(0, cut) if rank == 0 else (cut, H), want_source=True)
    same = lambda a, b: torch.equal(a["filled"].view(torch.int32), b["filled"].view(torch.int32)) and \
        torch.equal(a["source"], b["source"]) and a["holes"] == b["holes"] and a["max_dist"] == b["max_dist"]
    ok = same(one, two) and same(one, odd) and one["holes"] == int(torch.isnan(u).sum()) and not bool(torch.isnan(one["filled"]).any())
    print(f"RESULT rank {rank}: holes {two['holes']} max_dist {two['max_dist']!r} (one rank {one['holes']}, {one['max_dist']!r}) -> "
          f"{'ok' if ok else 'FAIL'}", flush=True)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
