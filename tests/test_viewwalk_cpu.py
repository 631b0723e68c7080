"""The view walk (brdf_nerf_amd/viewwalk.py) on the host: the chunk bounds against a written-out range() loop, the join and the
direction-major result on one rank, and both - with distributed.allreduce_ and row_band - under gloo at world 2."""
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT
from brdf_nerf_amd.distributed import shard_bounds
from brdf_nerf_amd.viewwalk import ViewWalk

CASES = [(257, 100, 2), (300, 100, 1), (7, 16, 8), (0, 4, 2), (64, 64, 2), (65, 64, 2)]


@pytest.mark.parametrize("n,chunk,world", CASES)
def test_bounds(n, chunk, world):
    per_rank, expected = [], []
    for r in range(world):
        w = ViewWalk(n, chunk, rank_world=(r, world))
        lo, hi = shard_bounds(n, r, world)
        assert (w.rank, w.world, w.lo, w.hi) == (r, world, lo, hi)
        want = []
        for i in range(lo, hi, chunk):                  # the loop every caller used to write
            want.append((i, min(hi, i + chunk)))
        got = w.chunks()
        assert got == want
        assert all(lo <= i < j <= hi and j - i <= chunk for i, j in got)
        per_rank += got
        expected += want
    # the ranks' chunks tile [0, n) in order, without gap or overlap
    assert [i for i, _ in per_rank] == [0] * bool(per_rank) + [j for _, j in per_rank[:-1]]
    assert (per_rank[-1][1] if per_rank else 0) == n
    for r in range(world):
        assert ViewWalk(n, chunk, rank_world=(r, world)).all_chunks() == expected


def test_join_world1():
    w = ViewWalk(8, 4)
    assert (w.rank, w.world, w.lo, w.hi) == (0, 1, 0, 8)
    rows = torch.arange(32, dtype=torch.float32).reshape(8, 4)
    out = w.join([rows[0:3], rows[3:3], rows[3:8]], (4,))
    assert torch.equal(out, rows) and out.is_contiguous()
    strided = torch.arange(64, dtype=torch.float32).reshape(8, 8)[:, ::2]        # a part that is not contiguous
    out = w.join([strided], (4,))
    assert torch.equal(out, strided) and out.is_contiguous()
    empty = w.join([], (4,), dtype=torch.int32)
    assert tuple(empty.shape) == (0, 4) and empty.dtype == torch.int32
    assert w.join([], ()).dtype == torch.float32 and tuple(w.join([], ()).shape) == (0,)


def test_planes_world1():
    K, R = 3, 10
    w = ViewWalk(R, 4)
    want = torch.arange(K * R * 3, dtype=torch.float32).reshape(K, R, 3)
    p = w.planes(K, (3,))
    for i, j in w.chunks():
        assert tuple(p.chunk(i, j).shape) == (K, j - i, 3)
        p.chunk(i, j).copy_(want[:, i:j])
    assert torch.equal(p.result(), want)
    out = torch.zeros(K, R, 3)
    p = w.planes(K, (3,), out)
    for i, j in w.chunks():
        p.chunk(i, j).copy_(want[:, i:j])
    got = p.result()
    assert got.data_ptr() == out.data_ptr() and torch.equal(out, want)
    vis = w.planes(K, ())                                # the visibility (K, R)
    for i, j in w.chunks():
        vis.chunk(i, j).copy_(want[:, i:j, 0])
    assert torch.equal(vis.result(), want[..., 0])
    for bad in (torch.zeros(K, R + 1, 3), torch.zeros(K, R), torch.zeros(K, R, 3, dtype=torch.float64)):
        with pytest.raises(ValueError, match="out must be float32"):
            w.planes(K, (3,), bad)


_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.environ["BN_ROOT"])
from brdf_nerf_amd.distributed import allreduce_, row_band, shard_bounds
from brdf_nerf_amd.viewwalk import ViewWalk
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
group = dist.group.WORLD
K, bad = 3, []
def check(name, ok):
    if not ok:
        bad.append(name)
for n in (7, 1):                                        # n = 1: rank 1 has no ray
    w = ViewWalk(n, 2, group)
    check(f"bounds {n}", (w.rank, w.world, w.lo, w.hi) == (rank, world) + shard_bounds(n, rank, world))
    table = torch.arange(n * 4, dtype=torch.float32).reshape(n, 4)
    full = torch.arange(K * n * 3, dtype=torch.float32).reshape(K, n, 3)
    got = w.join([table[i:j] for i, j in w.chunks()], (4,))
    check(f"join {n}", torch.equal(got, table) and got.is_contiguous())
    for out in (None, torch.zeros(K, n, 3)):
        p = w.planes(K, (3,), out)
        for i, j in w.chunks():
            p.chunk(i, j).copy_(full[:, i:j])
        got = p.result()
        check(f"planes {n}", torch.equal(got, full) and got.is_contiguous() and (out is None or got.data_ptr() == out.data_ptr()))
    vis = w.planes(K, ())
    for i, j in w.chunks():
        vis.chunk(i, j).copy_(full[:, i:j, 0])
    check(f"vis {n}", torch.equal(vis.result(), full[..., 0]))
t = torch.tensor([rank + 1, 10 * (rank + 1)], dtype=torch.int64)
check("sum", allreduce_(t, group=group) is t and t.tolist() == [3, 30])
t = torch.tensor([rank + 1, 5 - rank], dtype=torch.int64)
check("max", allreduce_(t, dist.ReduceOp.MAX, group).tolist() == [2, 5])
check("band", row_band("x", 5, None, group) == shard_bounds(5, rank, 2))
check("band given", row_band("x", 5, (1, 4), group) == (1, 4))
try:
    row_band("x", 5, (4, 9), None)
    check("band refused", False)
except ValueError as e:
    check("band text", "x: rows (4, 9) outside [0, 5]" in str(e))
print("RESULT", rank, bad)
dist.destroy_process_group()
sys.exit(1 if bad else 0)
"""


def test_world2_gloo(tmp_path):
    script = tmp_path / "viewwalk_worker.py"
    script.write_text(_WORKER)
    env = dict(os.environ, BN_ROOT=ROOT, MASTER_ADDR="127.0.0.1", MASTER_PORT="29547", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(2)]
    try:
        outs = [p.communicate(timeout=120)[0] for p in procs]
    finally:
        for p in procs:
            p.kill()
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
