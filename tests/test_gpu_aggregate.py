"""GPU tests of the semi-global aggregation of a cost volume (brdf_nerf_amd/aggregate.py; bn_cost_quanta, bn_cost_paths, bn_cost_pick).
Run on the MI355X box with `pytest -m gpu`.  Cases and the numpy statement they are held to: tests/aggregate_cases.py.

Everything after the one float64 division of the quanta is integer, so every output - quanta, sum, level, sum_min and every counter -
must EQUAL the statement.  The shapes are aggregate_cases.SHAPES: lines of one cell, diagonals shorter than both sides, more lines
than a block holds, and the lane edges of 1, 2, 3 and 4 levels per lane.
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import aggregate_cases as A
import mosaic_cases as M
import sweep_cases as S
from test_gpu_parity import DEV, _free_port

pytestmark = pytest.mark.gpu

QUANTUM = 0.25
# the shapes every direction and every penalty pair run on: Z below, at and above a lane edge, 1 to 3 levels per lane
MASK_SHAPES = ((3, 5, 63), (2, 130, 65), (33, 65, 2), (33, 65, 129))


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype).copy()).to(DEV)


def npy(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(shape, quantum=QUANTUM):
    """The volume of a shape and its quanta by the statement, computed once and left unchanged."""
    H, W, Z = shape
    cost = A.random_volume(Z, H, W, quantum=quantum)
    q, counters = A.quanta(cost, quantum)
    return cost, q, counters


@functools.lru_cache(maxsize=None)
def lines(shape, P1, P2):
    """L_r of the 8 directions by the statement."""
    return [A.line_costs(case(shape)[1], P1, P2, r) for r in A.DIRECTIONS]


def summed(shape, P1, P2, mask):
    return sum(L for b, L in enumerate(lines(shape, P1, P2)) if mask >> b & 1).astype(np.int32)


def check_pick(out, want, where):
    for key in ("level", "sum_min"):
        assert np.array_equal(npy(out[key]), want[key]), f"{where} {key}"
    assert npy(out["wins"]).tolist() == want["wins"] and npy(out["sums"]).tolist() == want["sums"], where


# ------------------------------------------------------------------------------------------------ the three entries
@pytest.mark.parametrize("shape", A.SHAPES)
def test_quanta_equal_the_statement(shape):
    """A dyadic quantum, whose half-quantum costs are exact ties of the rounding, and one that is not."""
    from brdf_nerf_amd import functions as Fn
    for quantum in (QUANTUM, 0.1):
        cost, q, counters = case(shape, quantum)
        got, cnt = Fn.cost_quanta(dev(cost), quantum)
        assert np.array_equal(npy(got), q), (shape, quantum)
        assert npy(cnt).tolist() == counters, (shape, quantum)
    cost, q, counters = case(shape)
    if q.size >= 10000:                                                      # the specials are all there, and all do what the rule says
        assert counters[2] > 0 and (q == -1).any() and (q == A.QINV).any() and (q == A.CAP).any() and (q == 0).any()
        ties = np.moveaxis(cost, 0, -1).astype(np.float64) / QUANTUM
        assert (q[ties == 0.5] == 0).all() and (q[ties == 1.5] == 2).all() and (q[ties == 2.5] == 2).all() and (ties == 2.5).sum() > 10


@pytest.mark.parametrize("shape", A.SHAPES)
def test_paths_and_pick_equal_the_statement(shape):
    from brdf_nerf_amd import functions as Fn
    P1, P2 = 256, 2048
    _, q, _ = case(shape)
    want_sum = summed(shape, P1, P2, 0xFF)
    dq = dev(q)
    total = Fn.cost_paths(dq, P1, P2, 0xFF)
    assert np.array_equal(npy(total), want_sum), shape
    check_pick(Fn.cost_pick(dq, total), A.pick(q, want_sum), shape)
    d = npy(total).astype(np.int64) - 8 * np.maximum(q, 0)
    assert d.min() >= 0 and d.max() <= 8 * P2                                # 0 <= L_r - c <= P2 in every direction


@pytest.mark.parametrize("P1,P2", A.PENALTIES)
@pytest.mark.parametrize("shape", MASK_SHAPES)
def test_every_direction_and_penalty(shape, P1, P2):
    from brdf_nerf_amd import functions as Fn
    _, q, _ = case(shape)
    dq = dev(q)
    for mask in A.MASKS:
        want_sum = summed(shape, P1, P2, mask)
        total = Fn.cost_paths(dq, P1, P2, mask)
        assert np.array_equal(npy(total), want_sum), (shape, P1, P2, hex(mask))
        if mask in (0x01, 0x80, 0x0F, 0xFF):
            check_pick(Fn.cost_pick(dq, total), A.pick(q, want_sum), (shape, P1, P2, hex(mask)))
    if (P1, P2) == (0, 0):                                                   # no smoothing: the paths are the quanta themselves
        assert np.array_equal(summed(shape, 0, 0, 0xFF), 8 * np.maximum(q, 0))


def test_two_launches_into_one_sum():
    """Masks 0x55 and 0xAA into one sum equal one launch of 0xFF; the entry adds into what it is given."""
    from brdf_nerf_amd import functions as Fn
    shape, P1, P2 = (33, 65, 65), 256, 2048
    _, q, _ = case(shape)
    dq = dev(q)
    total = Fn.cost_paths(dq, P1, P2, 0x55)
    assert np.array_equal(npy(total), summed(shape, P1, P2, 0x55))
    assert Fn.cost_paths(dq, P1, P2, 0xAA, total) is total
    assert np.array_equal(npy(total), summed(shape, P1, P2, 0xFF)) and torch.equal(total, Fn.cost_paths(dq, P1, P2, 0xFF))
    start = torch.full_like(total, 7)
    Fn.cost_paths(dq, P1, P2, 0x0F, start)
    assert np.array_equal(npy(start), summed(shape, P1, P2, 0x0F) + 7)


@pytest.mark.parametrize("Z", (1, 3, 64, 65, 256))
def test_constant_volumes_tie_everywhere(Z):
    """A constant volume: every level has the same sum at every cell and level 0 keeps it - or, where level 0 is NaN, level 1."""
    from brdf_nerf_amd import aggregate_costs
    H, W = 7, 9
    cost = np.full((Z, H, W), 2.5, dtype=np.float32)
    if Z > 1:
        cost[0, 2, 3] = np.nan
    cost[:, 4, 4] = np.nan
    for P1, P2 in ((0.0, 0.0), (1.0, 8.0)):
        want = A.aggregate(cost, 0.5, int(P1 * 2), int(P2 * 2))
        got = aggregate_costs(dev(cost), P1, P2, quantum=0.5, want_sum=True)
        assert np.array_equal(npy(got["level"]), want["level"]) and np.array_equal(npy(got["sum_min"]), want["sum_min"])
        assert np.array_equal(npy(got["sum"]), np.moveaxis(want["sum"], -1, 0)) and got["wins"] == want["wins"]
        assert want["level"][4, 4] == -1 and want["level"][2, 3] == (1 if Z > 1 else 0)
        if P2 == 0 or Z == 1:                                                # (with penalties the NaN level costs its lines' level 0 a P1)
            assert want["wins"][0] == H * W - (2 if Z > 1 else 1)
        assert (got["P1"], got["P2"], got["quantum"], got["capped"]) == (int(P1 * 2), int(P2 * 2), 0.5, 0)


def test_an_invalid_level_never_wins():
    """bn_cost_pick on a sum of the caller's: the smallest sum sits on a NaN level or in a cell without a result."""
    from brdf_nerf_amd import functions as Fn
    H, W, Z = 3, 5, 65
    rng = np.random.default_rng(3)
    q = rng.integers(0, 1000, (H, W, Z)).astype(np.int32)
    total = rng.integers(100, 5000, (H, W, Z)).astype(np.int32)
    q[0, 0, 7], total[0, 0, 7] = A.QINV, 0                                   # a NaN level with the smallest sum
    q[1, 1], total[1, 1, 3] = -1, 0                                          # a cell without a result
    q[2, 2, :], q[2, 2, 64], total[2, 2, 64] = A.QINV, 5, 4999               # one valid level, the last, with the largest sum
    total[2, 4, 10], total[2, 4, 40] = 1, 1                                  # a tie: the first
    want = A.pick(q, total)
    assert want["level"][0, 0] != 7 and want["level"][1, 1] == -1 and want["level"][2, 2] == 64 and want["level"][2, 4] == 10
    check_pick(Fn.cost_pick(dev(q), dev(total)), want, "constructed")


# ------------------------------------------------------------------------------------------------ the scene
@pytest.fixture(scope="module")
def scene_volume():
    return A.noisy_scene()


@pytest.mark.parametrize("paths", (8, 4))
def test_aggregate_costs_on_the_scene(scene_volume, paths):
    """The statement's volume through aggregate_costs: the recorded counts of test_aggregate_cpu.py."""
    from brdf_nerf_amd import aggregate_costs
    cost, dsm = scene_volume
    got = aggregate_costs(dev(cost), A.SCENE_P1, A.SCENE_P2, paths=paths, want_sum=True)
    want, rec = A.SCENE_RECORD[paths], A.SCENE_RECORD
    roof, ground, astray, none = S.scene_counts({"level": npy(got["level"])}, dsm, 2)
    print(f"{paths} paths: roof {roof}, astray {astray} of {ground}, none {none}, wins {got['wins']}, largest sum {int(got['sum'].max())}")
    assert (roof, astray, none) == (want["roof"], want["astray"], rec["none"]) and got["wins"] == want["wins"]
    assert (got["cells"], got["valid_pairs"], got["capped"]) == (rec["cells"], rec["valid_pairs"], rec["capped"])
    assert (got["quantum"], got["P1"], got["P2"]) == (A.SCENE_QUANTUM, 256, 2048)
    assert got["sum_total"] == want["sum_total"] and int(got["sum"].max()) == want["max_sum"] and got["sum"].shape == cost.shape
    assert got["sum"].dtype == torch.int32 and got["level"].dtype == torch.int32 and got["sum_min"].dtype == torch.int32
    assert aggregate_costs(dev(cost), A.SCENE_P1, A.SCENE_P2, quantum=A.SCENE_QUANTUM, paths=paths)["sum"] is None


def test_altitude_sweep_with_aggregate():
    """The noisy scene on the device.  Every aggregated output equals the statement applied to the DEVICE's own cost volume (its
    projections may differ from numpy's in a last bit, so the recorded counts are not asserted); the conditions on the inputs hold;
    level_wta and every key the sweep had equal the call without `aggregate` bit for bit."""
    from brdf_nerf_amd import Grid, Rpc, altitude_sweep
    ds, planes, dsm, xoff, yoff, res, zone = S.scene()
    rng = np.random.default_rng(7)
    noisy = [(p + rng.normal(0, A.SCENE_NOISE * float(p.max() - p.min()), p.shape)).astype(np.float32) for p in planes]
    views = [(dev(p), p.shape[1], p.shape[2], Rpc.from_dict(d)) for p, d in zip(noisy, ds)]
    grid, raised = Grid(xoff, yoff, res, dsm.shape[1], dsm.shape[0]), dev(M.raised(dsm))
    plain = altitude_sweep(views, raised, grid, zone, S.SCENE_OFFSETS, layout="planes", want_cost=True)
    wta = S.scene_counts({"level": npy(plain["level"])}, dsm, 2)
    bits = lambda t: t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t
    same_nan = lambda a, b: torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a[~torch.isnan(a)], b[~torch.isnan(b)])
    for paths in (8, 4):
        got = altitude_sweep(views, raised, grid, zone, S.SCENE_OFFSETS, layout="planes", want_cost=paths == 8,
                             aggregate=dict(p1=A.SCENE_P1, p2=A.SCENE_P2, paths=paths))
        want = A.aggregate(npy(plain["cost"]), A.SCENE_QUANTUM, 256, 2048, A.MASKS[8 + (paths == 8)])
        assert np.array_equal(npy(got["level"]), want["level"]) and np.array_equal(npy(got["sum_min"]), want["sum_min"])
        assert got["wins"] == want["wins"]
        has = want["level"] >= 0
        offset = np.where(has, S.SCENE_OFFSETS[np.maximum(want["level"], 0)], np.nan)
        assert same_nan(got["offset"], dev(offset))
        assert same_nan(got["altitude"], dev((M.raised(dsm).astype(np.float64) + offset).astype(np.float32)))
        roof, ground, astray, none = S.scene_counts({"level": npy(got["level"])}, dsm, 2)
        print(f"{paths} paths on the device's volume: roof {roof} (per cell {wta[0]}), astray {astray} (per cell {wta[2]}) of {ground}")
        assert wta[2] >= 500 and astray * 4 <= wta[2] and roof >= wta[0]
        assert torch.equal(got["level_wta"], plain["level"])
        for key in ("cost_min", "count", "visible", "view_dirs", "offsets"):
            assert torch.equal(bits(got[key]), bits(plain[key])), key
        for key in ("valid", "mean_cost", "cells", "skipped"):
            assert got[key] == plain[key], key
        assert torch.equal(bits(got["cost"]), bits(plain["cost"])) if paths == 8 else got["cost"] is None
    again = altitude_sweep(views, raised, grid, zone, S.SCENE_OFFSETS, layout="planes", want_cost=True)
    assert set(again) == set(plain) and "level_wta" not in plain and "sum_min" not in plain


def test_two_rank_aggregation_matches_one_rank():
    """World 2: two ranks on cuda:0 over gloo (tests/dist_aggregate_worker.py), each child under its own time limit and started once."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dist_aggregate_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=_free_port(), WORLD_SIZE="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, worker], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                              text=True) for r in range(2)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=300)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            outs.append("TIMEOUT\n" + p.communicate()[0])
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    assert all("RESULT" in o and "ok" in o for o in outs), "\n".join(outs)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    """BN_EINVAL through the raw ABI, nothing launched, every buffer as it was."""
    from brdf_nerf_amd import _lib as L
    lib = L.lib()
    H, W, Z = 5, 7, 3
    cost = torch.full((Z, H, W), 1.5, device=DEV)
    quanta = torch.full((H, W, Z), -9, dtype=torch.int32, device=DEV)
    total = torch.full((H, W, Z), -7, dtype=torch.int32, device=DEV)
    level, sum_min = (torch.full((H, W), -9, dtype=torch.int32, device=DEV) for _ in range(2))
    counters, wins, sums = (torch.full((n,), -5, dtype=torch.int64, device=DEV) for n in (3, Z, 2))
    p = lambda t: C.c_void_p(t.data_ptr())
    nan, inf = float("nan"), float("inf")

    def to_quanta(c=p(cost), Z=Z, H=H, W=W, quantum=0.5, q=p(quanta), n=p(counters)):
        return lib.bn_cost_quanta(c, Z, H, W, quantum, q, n, None)

    def to_paths(q=p(quanta), Z=Z, H=H, W=W, P1=1, P2=8, mask=0xFF, s=p(total)):
        return lib.bn_cost_paths(q, Z, H, W, P1, P2, mask, s, None)

    def to_pick(q=p(quanta), s=p(total), Z=Z, H=H, W=W, lv=p(level), sm=p(sum_min), w=p(wins), n=p(sums)):
        return lib.bn_cost_pick(q, s, Z, H, W, lv, sm, w, n, None)

    volume = [dict(Z=0), dict(Z=257), dict(Z=-1), dict(H=0), dict(W=0), dict(H=-2), dict(W=-1), dict(H=1 << 15, W=1 << 15, Z=2),
              dict(H=(1 << 20), W=(1 << 11), Z=1), dict(H=(1 << 12), W=(1 << 11), Z=256)]
    for kw in [dict(c=None), dict(q=None), dict(n=None), dict(quantum=0.0), dict(quantum=-0.5), dict(quantum=nan), dict(quantum=inf),
               dict(quantum=-inf)] + volume:
        assert to_quanta(**kw) == -1, kw
        assert b"cost_quanta" in lib.bn_last_error()
    for kw in [dict(q=None), dict(s=None), dict(P1=-1), dict(P1=9, P2=8), dict(P2=(1 << 20) + 1), dict(P1=(1 << 20) + 1, P2=(1 << 20) + 1),
               dict(P1=-2, P2=-1), dict(mask=0), dict(mask=0x100), dict(mask=0x1FF), dict(mask=-1), dict(mask=1 << 30)] + volume:
        assert to_paths(**kw) == -1, kw
        assert b"cost_paths" in lib.bn_last_error()
    for kw in [dict(q=None), dict(s=None), dict(lv=None), dict(sm=None), dict(w=None), dict(n=None)] + volume:
        assert to_pick(**kw) == -1, kw
        assert b"cost_pick" in lib.bn_last_error()
    torch.cuda.synchronize()
    assert (quanta == -9).all() and (total == -7).all() and (level == -9).all() and (sum_min == -9).all() and (cost == 1.5).all()
    assert all((t == -5).all() for t in (counters, wins, sums))
    for t in (counters, wins, sums, total):
        t.zero_()
    assert to_quanta() == 0 and to_paths(P1=0, P2=0, mask=0x01) == 0 and to_paths(P1=1 << 20, P2=1 << 20, mask=0x80) == 0 and to_pick() == 0
    torch.cuda.synchronize()
    assert (quanta == 3).all() and (level == 0).all() and counters.tolist() == [H * W, H * W * Z, 0] and wins.tolist() == [H * W, 0, 0]
    assert sums.tolist() == [H * W, int(sum_min.sum())] and int(total.min()) >= 6


def test_wrapper_refusals_on_the_device():
    from brdf_nerf_amd import aggregate_costs
    from brdf_nerf_amd import functions as Fn
    cost = torch.zeros(3, 4, 5, device=DEV)
    quanta = torch.zeros(4, 5, 3, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="device"):
        aggregate_costs(cost.cpu(), 1.0, 8.0)
    for call, what in ((lambda: Fn.cost_quanta(cost, 0.5, quanta=torch.zeros(4, 5, 4, dtype=torch.int32, device=DEV)), "quanta"),
                       (lambda: Fn.cost_quanta(cost, 0.5, counters=torch.zeros(2, dtype=torch.int64, device=DEV)), "counters"),
                       (lambda: Fn.cost_quanta(cost, 0.5, quanta=quanta.cpu()), "device"),
                       (lambda: Fn.cost_quanta(torch.zeros(257, 2, 2, device=DEV), 0.5), "levels"),
                       (lambda: Fn.cost_quanta(cost, float("nan")), "quantum"),
                       (lambda: Fn.cost_paths(quanta, 1, 8, sum=torch.zeros(4, 5, 3, device=DEV)), "sum"),
                       (lambda: Fn.cost_paths(quanta, 1, 8, sum=quanta.cpu()), "device"),
                       (lambda: Fn.cost_paths(quanta.float(), 1, 8), "quanta"),
                       (lambda: Fn.cost_paths(quanta, 9, 8), "penalties"), (lambda: Fn.cost_paths(quanta, 1.0, 8), "penalties"),
                       (lambda: Fn.cost_paths(quanta, 1, (1 << 20) + 1), "penalties"),
                       (lambda: Fn.cost_paths(quanta, 1, 8, mask=0), "mask"), (lambda: Fn.cost_paths(quanta, 1, 8, mask=0x100), "mask"),
                       (lambda: Fn.cost_pick(quanta, torch.zeros(4, 5, 2, dtype=torch.int32, device=DEV)), "sum"),
                       (lambda: Fn.cost_pick(quanta, quanta, level=torch.zeros(4, 4, dtype=torch.int32, device=DEV)), "level"),
                       (lambda: Fn.cost_pick(quanta, quanta, wins=torch.zeros(4, dtype=torch.int64, device=DEV)), "wins")):
        with pytest.raises(ValueError, match=what):
            call()
