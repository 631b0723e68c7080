"""The grid walk (brdf_nerf_amd/gridwalk.py) on the host: the band and the lone-band rule against their written-out forms, the
buffers, the join and the merge on one rank, the bands of every rank under rank_world=, and all of it under gloo at world 2."""
import os
import socket
import subprocess
import sys

import pytest
import torch

from conftest import ROOT
from brdf_nerf_amd.distributed import shard_bounds
from brdf_nerf_amd.gridwalk import GridWalk

H, W, K = 5, 3, 2


@pytest.mark.parametrize("rows", [None, (0, 5), (1, 4), (2, 2)])
def test_one_rank(rows, monkeypatch):
    w = GridWalk("x", H, rows)
    want = (0, H) if rows is None else rows
    assert (w.rank, w.world, w.rows) == (0, 1, want)
    assert w.alone == (want != (0, H))                   # world == 1 and rows != (0, H)
    fills, full = [], torch.full
    monkeypatch.setattr(torch, "full", lambda *a, **k: fills.append(a) or full(*a, **k))
    for shape, dtype, unseen in (((K, H, W), torch.uint8, 2), ((H, W), torch.int32, -1), ((H, W, 2), torch.float64, float("nan")),
                                 ((K, H, W), torch.float32, 7.5)):
        del fills[:]
        b = w.buffer(shape, dtype, unseen, "cpu")
        assert tuple(b.shape) == shape and b.dtype == dtype and b.is_contiguous()
        assert len(fills) == w.alone                     # a fill pass exactly for a lone band: otherwise the buffer is torch.empty
        if w.alone:
            assert bool((b.isnan() if unseen != unseen else b == unseen).all())
    monkeypatch.undo()
    for t, axis in ((torch.arange(H * W * 2, dtype=torch.float64).reshape(H, W, 2), 0), (torch.arange(K * H * W).reshape(K, H, W), 1),
                    (torch.arange(H * W).reshape(H, W), 0)):
        got = w.join(t, row_axis=axis)
        assert got is t and got.data_ptr() == t.data_ptr()
    counts = torch.arange(6, dtype=torch.int64)
    keep = counts.clone()
    assert w.merge(counts) is counts and w.merge(counts, torch.distributed.ReduceOp.MAX) is counts and torch.equal(counts, keep)


@pytest.mark.parametrize("rows", [(4, 9), (3, 2)])
def test_band_refused(rows):
    with pytest.raises(ValueError, match=rf"x: rows \({rows[0]}, {rows[1]}\) outside \[0, 5\]"):
        GridWalk("x", H, rows)


@pytest.mark.parametrize("world", [1, 2, 8])
@pytest.mark.parametrize("height", [5, 1, 0])
def test_rank_world(height, world):
    at = 0
    for r in range(world):
        w = GridWalk("x", height, rank_world=(r, world))
        assert (w.rank, w.world) == (r, world) and w.rows == shard_bounds(height, r, world)
        assert w.rows[0] == at and w.rows[1] >= at       # the ranks' bands tile [0, H) in rank order
        assert not w.alone or (world == 1 and w.rows != (0, height))
        at = w.rows[1]
    assert at == height


_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.environ["BN_ROOT"])
from brdf_nerf_amd.distributed import shard_bounds
from brdf_nerf_amd.gridwalk import GridWalk
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
group = dist.group.WORLD
H, W, K, C, bad = 5, 3, 2, 3, []
def check(name, ok):
    if not ok:
        bad.append(name)
wholes = [(torch.arange(H * W * 2, dtype=torch.float64).reshape(H, W, 2), 0, float("nan")),
          (torch.arange(K * H * W, dtype=torch.uint8).reshape(K, H, W), 1, 2),
          (torch.arange(C * H * W, dtype=torch.float32).reshape(C, H, W) + 0.5, 1, float("nan"))]
for tag, bands in (("default", None), ("uneven", ((0, 1), (1, 5))), ("empty", ((0, 0), (0, 5)))):
    w = GridWalk("x", H, None if bands is None else bands[rank], group)
    r0, r1 = w.rows
    check(f"{tag} band", (w.rank, w.world, w.rows) == (rank, world, shard_bounds(H, rank, world) if bands is None else bands[rank]))
    check(f"{tag} alone", not w.alone)
    for whole, axis, unseen in wholes:
        keep = whole.clone()
        buf = w.buffer(tuple(whole.shape), whole.dtype, unseen, "cpu")
        check(f"{tag} buffer {axis}", buf.shape == whole.shape and buf.dtype == whole.dtype)
        buf.narrow(axis, r0, r1 - r0).copy_(whole.narrow(axis, r0, r1 - r0))          # only this rank's band is written
        got = w.join(buf, row_axis=axis)
        check(f"{tag} join {whole.dtype} axis {axis}", torch.equal(got, whole) and got.is_contiguous() and got.dtype == whole.dtype)
        check(f"{tag} whole unchanged", torch.equal(whole, keep))
    t = torch.tensor([rank + 1, 10 * (rank + 1)], dtype=torch.int64)
    check(f"{tag} sum", w.merge(t) is t and t.tolist() == [3, 30])
    t = torch.tensor([rank + 1, 5 - rank], dtype=torch.int64)
    check(f"{tag} max", w.merge(t, dist.ReduceOp.MAX) is t and t.tolist() == [2, 5])
w = GridWalk("x", H, ((0, 2), (3, 5))[rank], group)     # the bands leave row 2 out
for whole, axis, _ in wholes:
    try:
        w.join(whole.clone(), row_axis=axis)
        check(f"cover refused axis {axis}", False)
    except ValueError as e:
        check(f"cover text axis {axis}", "x: the ranks' bands cover 4 rows of 5" in str(e))
print("RESULT", rank, bad)
dist.destroy_process_group()
sys.exit(1 if bad else 0)
"""


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_world2_gloo(tmp_path):
    script = tmp_path / "gridwalk_worker.py"
    script.write_text(_WORKER)
    env = dict(os.environ, BN_ROOT=ROOT, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(2)]
    try:
        outs = [p.communicate(timeout=120)[0] for p in procs]
    finally:
        for p in procs:
            p.kill()
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
