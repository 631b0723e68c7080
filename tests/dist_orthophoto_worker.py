"""Worker of test_two_rank_orthophoto_matches_one_rank (tests/test_gpu_orthophoto.py): rank r of 2, both on cuda:0, gloo.

Every rank takes its band of rows through grid_pixels, the march towards the sensor and the gather (orthophoto's default under a
group); the bands are gathered and the counts merged by one SUM all-reduce.  ortho, state, colrow, visible and counts must equal
what the same process computes alone - a group of one rank - bit for bit, and uneven explicit bands (rows=) must give the same again.
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
    import camera_cases as K
    import orthophoto_cases as O
    from brdf_nerf_amd import Grid, Rpc, orthophoto

    d, dsm, xoff, yoff, res = O.box_scene()                   # 48 x 40: bands of 24 | 24 rows; the box spans the cut
    H, W = dsm.shape
    Hi, Wi = O.SCENE_IMAGE
    zone = K.SITES[O.SCENE_SITE][2]
    image = torch.from_numpy(O.to_layout(O.linear_image(Hi, Wi, 3), "image")).to(dev)
    args = (image, Hi, Wi, Rpc.from_dict(d), torch.from_numpy(dsm).to(dev), Grid(xoff, yoff, res, W, H), zone)
    groups = [dist.new_group([r]) for r in range(world)]      # (every rank must take part in every new_group call)
    one = orthophoto(*args, group=groups[rank])
    two = orthophoto(*args)                                   # data parallel: the default group
    cut = 19                                                  # uneven bands: 19 | 29 rows
    odd = orthophoto(*args, rows=(0, cut) if rank == 0 else (cut, H))
    bits = lambda t: t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)
    same = lambda a, b: torch.equal(bits(a["ortho"]), bits(b["ortho"])) and torch.equal(a["state"], b["state"]) and \
        torch.equal(bits(a["colrow"]), bits(b["colrow"])) and torch.equal(a["visible"], b["visible"]) and a["counts"] == b["counts"] and \
        torch.equal(a["view_dir"], b["view_dir"])
    ok = same(one, two) and same(one, odd) and one["counts"]["occluded"] >= 20 and one["counts"]["kept"] >= 200 and \
        sum(one["counts"][k] for k in O.STATES) == H * W
    print(f"RESULT rank {rank}: counts {two['counts']} (one rank {one['counts']}) -> {'ok' if ok else 'FAIL'}", flush=True)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
