"""Host tests of the semi-global aggregation (no device): the numpy statement of tests/aggregate_cases.py against a brute force over
all level sequences, its bounds, its limits (no penalties; a split of the directions), the neutral cell, the invalid level, the tie
rule, the scene fixture with its recorded counts, the build, and the wrapper refusals that need no device."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

import aggregate_cases as A
import camera_cases as K
import sweep_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute_force(c, P1, P2):
    """best[p][d]: the minimum, over ALL sequences of levels d_0 .. d_p = d along a line of costs c (n, Z), of the sum of c[j][d_j] and
    of V(d_j-1, d_j), V = 0, P1, P2 for a change of 0, 1, more levels.  Shares nothing with the recurrence."""
    n, Z = c.shape
    best = np.full((n, Z), np.iinfo(np.int64).max, dtype=np.int64)
    for p in range(n):
        for seq in itertools.product(range(Z), repeat=p + 1):
            total = sum(int(c[j, d]) for j, d in enumerate(seq))
            total += sum(0 if a == b else (P1 if abs(a - b) == 1 else P2) for a, b in zip(seq[:-1], seq[1:]))
            best[p, seq[-1]] = min(best[p, seq[-1]], total)
    return best


@pytest.mark.parametrize("P1,P2", ((0, 0), (0, 5), (1, 1), (2, 7), (3, 40), (11, 11), (6, 1000)))
def test_the_recurrence_against_brute_force(P1, P2):
    """L_r(p, d) + the sum over j < p of m_j (the minima the recurrence took off) is the cheapest sequence ending in d at p - in every
    direction a 1 x n or n x 1 grid has, forwards and backwards."""
    rng = np.random.default_rng(P1 + 3 * P2)
    for n, Z in ((1, 1), (1, 3), (2, 2), (3, 3), (4, 3), (4, 2), (4, 1)):
        c = rng.integers(0, 30, (n, Z))
        want = brute_force(c, P1, P2)
        for shape, direction, flip in (((1, n, Z), (0, 1), False), ((1, n, Z), (0, -1), True), ((n, 1, Z), (1, 0), False),
                                       ((n, 1, Z), (-1, 0), True)):
            L = A.line_costs((c[::-1] if flip else c).reshape(shape).astype(np.int32), P1, P2, direction).reshape(n, Z)
            L = L[::-1] if flip else L
            taken = np.concatenate([[0], np.cumsum(L.min(1))[:-1]])
            assert np.array_equal(L + taken[:, None], want), (n, Z, direction)


def test_bounds_and_limits():
    """0 <= L_r - c <= P2 in every direction; without penalties sum = paths x c and the pick is the argmin of the quanta; a split of
    the directions adds up."""
    H, W, Z = 9, 11, 7
    cost = A.random_volume(Z, H, W, seed=1)
    q, counters = A.quanta(cost, 0.25)
    c = np.maximum(q, 0).astype(np.int64)
    assert counters[2] > 0 and (q == -1).any() and (q == A.QINV).any() and (q == A.CAP).any()
    for P1, P2 in A.PENALTIES:
        for r in A.DIRECTIONS:
            d = A.line_costs(q, P1, P2, r) - c
            assert d.min() >= 0 and d.max() <= P2, (P1, P2, r)
    for mask, n in ((0x0F, 4), (0xFF, 8)):
        total = A.paths(q, 0, 0, mask)
        assert np.array_equal(total, n * c)
        got = A.pick(q, total)
        valid = (q >= 0) & (q < A.QINV)
        has = valid.any(-1)
        assert np.array_equal(got["level"][has], np.argmin(np.where(valid, q, A.QINV), -1)[has]) and (got["level"][~has] == -1).all()
    whole = A.paths(q, 256, 2048, 0xFF)
    assert np.array_equal(A.paths(q, 256, 2048, 0x55) + A.paths(q, 256, 2048, 0xAA), whole)
    assert np.array_equal(sum(A.paths(q, 256, 2048, 1 << b) for b in range(8)), whole)


def test_quanta_rule():
    quantum = 0.25
    values = np.array([np.nan, np.inf, -np.inf, -3.5, -0.0, 0.0, 1e-42, 0.125, 0.375, 0.625, 0.25, A.CAP * quantum, (A.CAP - 0.5) * quantum,
                       (A.CAP - 1.5) * quantum, A.QINV * quantum, 3e38], dtype=np.float32)
    level0 = np.concatenate([values, np.float32([np.nan])])                  # the last cell has no result either
    cost = np.stack([level0, np.full_like(level0, np.nan)]).reshape(2, 1, -1)
    q, counters = A.quanta(cost, quantum)
    # level 0 of every cell; ties to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 2^20 - 1.5 and 2^20 - 2.5 -> 2^20 - 2
    assert q[0, :, 0].tolist() == [-1, A.CAP, 0, 0, 0, 0, 0, 0, 2, 2, 1, A.CAP, A.CAP - 1, A.CAP - 1, A.CAP, A.CAP, -1]
    assert q[0, 1:-1, 1].tolist() == [A.QINV] * 15 and q[0, 0].tolist() == [-1, -1] and q[0, -1].tolist() == [-1, -1]
    assert counters == [15, 15, 4] and q.dtype == np.int32 and q.shape == (1, 17, 2)


def test_a_cell_without_a_result_is_neutral():
    """It gets -1, costs 0 at every level, passes the message on and does not restart a path.  With P1 = P2 one hop and two hops
    smooth alike, so the other cells are exactly as without it; with P1 < P2 two hops may change two levels for 2 P1."""
    Z = 5
    rng = np.random.default_rng(5)
    line = rng.integers(0, 50, (1, 6, Z)).astype(np.int32)
    holed = np.insert(line, 3, -1, axis=1)                                   # the same line with a neutral cell after cell 2
    free = np.insert(line, 3, 0, axis=1)                                     # and with a cell that costs 0 at every level
    for P1, P2 in ((1, 8), (3, 3), (0, 0)):
        for r in ((0, 1), (0, -1)):
            a, b = A.line_costs(line, P1, P2, r), A.line_costs(holed, P1, P2, r)
            assert np.array_equal(b, A.line_costs(free, P1, P2, r))
            assert (b[0, 3] >= 0).all() and (b[0, 3] <= P2).all() and b[0, 3].min() == 0
            if P1 == P2:
                assert np.array_equal(np.delete(b, 3, axis=1), a), (P1, P2, r)
            if P2:                                                           # a restart would give the next cell its bare costs
                after = 4 if r == (0, 1) else 2
                assert not np.array_equal(b[0, after], np.maximum(holed[0, after], 0))
    got = A.pick(holed, A.paths(holed, 1, 8))
    assert got["level"][0, 3] == -1 and got["sum_min"][0, 3] == -1 and (np.delete(got["level"], 3, axis=1) >= 0).all()
    assert got["sums"][0] == 6 and sum(got["wins"]) == 6


def test_an_invalid_level_never_wins():
    """A NaN level costs 2^20 on the paths, so its sum is large - but the rule does not rest on that: constructed sums whose smallest
    sits on the invalid level still give the best VALID one."""
    cost = np.full((3, 1, 4), 1.0, dtype=np.float32)
    cost[1, 0, 2] = np.nan
    got = A.aggregate(cost, 0.5, 0, 0)
    assert got["quanta"][0, 2].tolist() == [2, A.QINV, 2] and got["level"][0, 2] == 0 and got["sum"][0, 2, 1] == 8 * A.QINV
    q = np.array([[[5, A.QINV, 7, 9], [-1, -1, -1, -1], [A.QINV, A.QINV, A.QINV, 3]]], dtype=np.int32)
    total = np.array([[[40, 0, 30, 30], [0, 1, 2, 3], [0, 0, 0, 99]]], dtype=np.int32)
    got = A.pick(q, total)
    assert got["level"].tolist() == [[2, -1, 3]] and got["sum_min"].tolist() == [[30, -1, 99]]
    assert got["wins"] == [0, 0, 1, 1] and got["sums"] == [2, 129]


def test_a_tie_goes_to_the_first_level():
    cost = np.full((6, 4, 5), 0.75, dtype=np.float32)
    first = A.aggregate(cost, 0.25, 2, 9)
    assert (first["sum"] == first["sum"][..., :1]).all() and (first["level"] == 0).all() and first["wins"] == [20, 0, 0, 0, 0, 0]
    last = A.aggregate(cost, 0.25, 2, 9, strict=False)                       # the comparison the rule does NOT use
    assert (last["level"] == 5).all() and last["wins"] == [0, 0, 0, 0, 0, 20] and np.array_equal(last["sum_min"], first["sum_min"])
    cost[0, 1, 1] = np.nan                                                   # the first VALID level
    assert A.aggregate(cost, 0.25, 0, 0)["level"][1, 1] == 1


@pytest.fixture(scope="module")
def scene_volume():
    return A.noisy_scene()


def test_the_scene_fixture(scene_volume):
    """Conditions on the inputs of the GPU end-to-end test, asserted on the statement alone, and the exact counts, recorded."""
    cost, dsm = scene_volume
    rec = A.SCENE_RECORD
    assert cost.shape == (17, 48, 40) and cost.dtype == np.float32
    wta = S.scene_counts({"level": A.wta_level(cost)}, dsm, 2)
    print(f"per cell: {wta[0]} of the 100 roof cells at -6 m, {wta[2]} of the {wta[1]} ground cells not at 0 m, {wta[3]} cells without a result")
    assert wta[2] >= 500 and (wta[0], wta[2], wta[3]) == (rec["wta"]["roof"], rec["wta"]["astray"], rec["none"])
    P1, P2 = round(A.SCENE_P1 / A.SCENE_QUANTUM), round(A.SCENE_P2 / A.SCENE_QUANTUM)
    assert (P1, P2) == (256, 2048)
    for paths, mask in ((8, 0xFF), (4, 0x0F)):
        got = A.aggregate(cost, A.SCENE_QUANTUM, P1, P2, mask)
        roof, ground, astray, none = S.scene_counts(got, dsm, 2)
        q = got["quanta"]
        print(f"{paths} paths: {roof} roof cells at -6 m, {astray} of the {ground} ground cells not at 0 m; wins {got['wins']}; largest sum "
              f"{int(got['sum'].max())}; largest quantum {int(q[q < A.QINV].max())}; counters {got['counters']}")
        assert astray * 4 <= wta[2] and roof >= wta[0]
        want = rec[paths]
        assert (roof, astray, none) == (want["roof"], want["astray"], rec["none"]) and got["wins"] == want["wins"]
        assert got["sums"] == [rec["cells"], want["sum_total"]] and int(got["sum"].max()) == want["max_sum"]
        assert got["counters"] == [rec["cells"], rec["valid_pairs"], rec["capped"]] and int(q[q < A.QINV].max()) == rec["max_quantum"]


def test_package_surface():
    import brdf_nerf_amd
    from brdf_nerf_amd import _lib
    from brdf_nerf_amd import functions as Fn
    assert "aggregate_costs" in brdf_nerf_amd.__all__ and callable(brdf_nerf_amd.aggregate_costs)
    assert all(callable(getattr(Fn, f)) for f in ("cost_quanta", "cost_paths", "cost_pick"))
    header = open(os.path.join(ROOT, "include", "brdfnerf_hip.h")).read()
    assert "Semi-global aggregation of a cost volume" in header
    declared = set(re.findall(r"\b(bn_[a-z0-9_]+)\s*\(", header))
    lib = open(os.path.join(ROOT, "brdf_nerf_amd", "libbrdfnerf_hip.so"), "rb").read()
    for name, n_args in (("bn_cost_quanta", 8), ("bn_cost_paths", 9), ("bn_cost_pick", 10)):
        assert name in declared and name in _lib.exported_symbols() and len(_lib._SIGS[name][1]) == n_args
        assert name.encode() in lib                                          # exported by the cross-compiled library
    assert re.search(rf"#define BN_AGG_QINV {A.QINV}\b", header) and _lib.BN_AGG_QINV == A.QINV == 1 << 20
    for line in ("(0,+1) (0,-1) (+1,0) (-1,0) (+1,+1) (-1,-1) (+1,-1) (-1,+1)", "The entry ADDS", "a strict <"):
        assert line in header
    assert os.path.exists(os.path.join(ROOT, "brdf_nerf_amd", "csrc", "aggregate.hip"))
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "## Semi-global aggregation of the sweep's cost volume" in readme


def test_wrapper_refusals_without_a_device():
    from brdf_nerf_amd import Grid, Rpc, aggregate_costs, altitude_sweep
    from brdf_nerf_amd import functions as Fn
    cost = torch.zeros(3, 4, 5)
    nan, inf = float("nan"), float("inf")
    for bad in (None, [[[0.0]]], torch.zeros(4, 5), torch.zeros(1, 3, 4, 5)):
        with pytest.raises(ValueError, match="3-D"):
            aggregate_costs(bad, 1.0, 8.0)
    for bad in (cost.double(), cost.int()):
        with pytest.raises(ValueError, match="float32"):
            aggregate_costs(bad, 1.0, 8.0)
    with pytest.raises(ValueError, match="levels"):
        aggregate_costs(torch.zeros(257, 2, 2), 1.0, 8.0)
    for p1, p2 in ((-1.0, 8.0), (9.0, 8.0), (nan, 8.0), (1.0, inf), (1.0, nan), ("1", 8.0), (True, 8.0)):
        with pytest.raises(ValueError, match="p1|p2|penalties"):
            aggregate_costs(cost, p1, p2)
    with pytest.raises(ValueError, match="quantum must be given"):
        aggregate_costs(cost, 0.0, 8.0)
    for bad in (0.0, -1.0, nan, inf, "x"):
        with pytest.raises(ValueError, match="quantum"):
            aggregate_costs(cost, 1.0, 8.0, quantum=bad)
    with pytest.raises(ValueError, match=r"2\^20 quanta"):
        aggregate_costs(cost, 1.0, 8.0, quantum=1e-6)
    for bad in (0, 2, 5, 16, 8.5, "8", None, True):
        with pytest.raises(ValueError, match="paths"):
            aggregate_costs(cost, 1.0, 8.0, paths=bad)
    with pytest.raises(ValueError, match="device"):
        aggregate_costs(cost, 1.0, 8.0)
    with pytest.raises(ValueError, match="device"):
        aggregate_costs(cost, 0.0, 0.0, quantum=0.5, paths=4)
    quanta = torch.zeros(4, 5, 3, dtype=torch.int32)
    for call, what in ((lambda: Fn.cost_quanta(cost, 0.0), "quantum"), (lambda: Fn.cost_quanta(cost[:, :, ::2], 0.5), "contiguous"),
                       (lambda: Fn.cost_paths(quanta, -1, 8), "penalties"), (lambda: Fn.cost_paths(quanta, 1, 8, mask=0x1FF), "mask"),
                       (lambda: Fn.cost_paths(torch.zeros(4, 5, 257, dtype=torch.int32), 1, 8), "levels"),
                       (lambda: Fn.cost_pick(quanta, quanta.long()), "sum"), (lambda: Fn.cost_pick(quanta, quanta), "device")):
        with pytest.raises(ValueError, match=what):
            call()
    # altitude_sweep(aggregate=...): what it refuses before any launch
    rpc = Rpc.from_dict(K.make_rpc("z17", 1))
    grid = Grid(0.0, 0.0, 0.5, 5, 4)
    view, dsm, off = (torch.zeros(6 * 7, 3), 6, 7, rpc), torch.zeros(4, 5), [-1.0, 0.0, 1.0]
    good = dict(p1=1.0, p2=8.0)
    for bad in ({}, dict(p1=1.0), dict(p1=1.0, p2=8.0, window=3), [1.0, 8.0], 8):
        with pytest.raises(ValueError, match="aggregate"):
            altitude_sweep([view], dsm, grid, 17, off, aggregate=bad)
    for bad, what in ((dict(p1=9.0, p2=8.0), "penalties"), (dict(p1=0.0, p2=8.0), "quantum"), (dict(good, paths=6), "paths"),
                      (dict(good, quantum=-1.0), "quantum")):
        with pytest.raises(ValueError, match=what):
            altitude_sweep([view], dsm, grid, 17, off, aggregate=bad)
    with pytest.raises(ValueError, match="rows"):
        altitude_sweep([view], dsm, grid, 17, off, aggregate=good, rows=(0, 2))
    for bad in ([0.0, 0.0, 1.0], [1.0, 0.0, -1.0], [0.0, 2.0, 1.0]):
        with pytest.raises(ValueError, match="strictly increasing"):
            altitude_sweep([view], dsm, grid, 17, bad, aggregate=good)
    with pytest.raises(ValueError, match="device"):
        altitude_sweep([view], dsm, grid, 17, off, aggregate=good)
    with pytest.raises(ValueError, match="device"):
        altitude_sweep([view], dsm, grid, 17, [1.0, 0.0], aggregate=None)   # unsorted offsets stay fine without it
