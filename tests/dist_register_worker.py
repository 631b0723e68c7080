"""Worker of test_two_rank_registration_matches_one_rank (tests/test_gpu_register.py): rank r of 2, both on cuda:0, gloo.

Each rank takes its band of the ground truth's rows at every pyramid level (register_xy's default under a group), the integer
moments are summed by one all-reduce per level, and both ranks run the same host-side search.  Every integer, (dx, dy) and b
must equal what the same process computes alone - a group of one rank - bit for bit; so must altitude_mae_xy's numbers, and
uneven explicit bands (rows=) must give the same again.
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
    import register_cases as R
    from brdf_nerf_amd import altitude_mae_xy, register_xy

    g = R.golden("one_level")                                 # 104 x 112: two levels, bands of 52 | 52 rows and 26 | 26
    pred, gt = torch.from_numpy(g["v"]).to(dev), torch.from_numpy(g["u"]).to(dev)
    groups = [dist.new_group([r]) for r in range(world)]      # (every rank must take part in every new_group call)
    one = register_xy(pred, gt, group=groups[rank])
    two = register_xy(pred, gt)                               # data parallel: the default group
    H = gt.shape[0]
    cut = 37                                                  # uneven bands that cut a tile: 37 | 67 rows, 19 | 33 a level up
    odd = register_xy(pred, gt, rows=(0, cut) if rank == 0 else (cut, H))
    same = lambda a, b: all(torch.equal(x, y) for x, y in zip(a["moments"], b["moments"])) and \
        all(a[k] == b[k] for k in ("dx", "dy", "b", "k", "pivot", "levels", "skipped"))
    ok = same(one, two) and same(one, odd) and (one["dx"], one["dy"]) == (8, -4) and len(one["moments"]) == 2
    mask = (torch.arange(gt.numel(), device=dev).reshape(gt.shape) % 7) != 0
    a1, a2 = altitude_mae_xy(pred, gt, mask=mask, group=groups[rank]), altitude_mae_xy(pred, gt, mask=mask)
    ok = ok and all(a1[k] == a2[k] and a1[k] == a1[k] for k in ("mae", "mae_in", "mae_out", "shift", "dx", "dy"))
    ok = ok and torch.equal(a1["rdsm"].view(torch.int32), a2["rdsm"].view(torch.int32))
    print(f"RESULT rank {rank}: levels {two['levels']} b {two['b']!r} (one rank {one['b']!r}), first moments "
          f"{two['moments'][-1][60].tolist()}, mae {a2['mae']:.6f} -> {'ok' if ok else 'FAIL'}", flush=True)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
