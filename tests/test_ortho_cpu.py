"""The statement of the orthorectified maps (tests/ortho_cases.py) against what it must reduce to, the conditions on the block
scene, the quantisation bound, and the refusals of OrthoAccumulator that need no device."""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import dsm_cases as D
import ortho_cases as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(D.CASES))
def test_without_channels_and_top_the_statement_is_the_dsm_statement(name):
    """E = 0, top = None: (sum_z, count) and the bad points are dsm_cases' sums, counts and skipped on every one of its cases, and
    the resolved dsm and count are its dsm and count, bit for bit."""
    grid, radius, footprint, rays, depth = D.case(name)
    want = D.expected(name)
    acc, counters = O.splat(rays, depth, np.zeros((len(rays), 0), np.float32), grid, radius, footprint)
    acc = O.as_int64(acc)
    assert acc.shape == want["sums"].shape + (2,)
    assert np.array_equal(acc[..., 0], want["sums"]) and np.array_equal(acc[..., 1], want["counts"])
    assert counters == [want["skipped"], 0, 0]
    maps, dsm, count = O.resolve(acc)
    assert maps.shape == (0,) + want["dsm"].shape
    assert np.array_equal(dsm.view(np.int32), want["dsm"].view(np.int32)) and np.array_equal(count, want["count"])


def test_block_scene_conditions():
    """The scene shows what top mode is for: at least 20 cells where mean and top mode (band 1 m) differ, every roof cell exactly
    the roof colour in top mode, at least 5 cells whose highest point comes in through a neighbour's footprint only - and in mean
    mode the cells along the roof's western edge are NOT the roof colour (the facade is mixed in)."""
    c = O.block_conditions()
    print(c)
    assert c == O.BLOCK_CONDITIONS
    assert c["differ"] >= 20 and c["roof_off_colour"] == 0 and c["neighbour_only"] >= 5 and c["culled"] > 0
    s = O.block_scene()
    roof = np.array(O.BLOCK_COLOURS["roof"], dtype=np.float32)
    west = [np.array_equal(s["mean"]["maps"][:, j, O.ROOF_COLS[0]], roof) for j in O.ROOF_ROWS]
    assert not any(west)
    assert set(s["surface"]) == {"ground", "roof", "facade"} and s["mean"]["counters"] == [0, 0, 0]
    # the altitude of a roof cell: the mean drags it down, top mode leaves 30 m within the 4e-6 m of the fp32 origins
    j, i = O.ROOF_ROWS[3], O.ROOF_COLS[0]
    assert abs(float(s["top"]["dsm"][j, i]) - 30.0) < 1e-5 and float(s["mean"]["dsm"][j, i]) < 29.0
    # the block's shadow stays empty in both modes
    assert np.isnan(s["top"]["dsm"][O.ROOF_ROWS[3], 28]) and s["top"]["count"][O.ROOF_ROWS[3], 28] == 0


def test_a_band_above_the_relief_is_mean_mode():
    """Top mode with a band larger than the relief (20 m) culls nothing: acc, maps, dsm and count of mean mode, bit for bit - and
    so does a top grid left at EMPTY with band 0."""
    s = O.block_scene()
    mean = s["mean"]
    wide = O.statement(s["rays"], s["depth"], s["features"], s["grid"], 1, "disc", "top", 25.0)
    assert wide["counters"] == [0, 0, 0] and np.array_equal(wide["acc"], mean["acc"])
    for k in ("maps", "dsm"):
        assert np.array_equal(wide[k].view(np.int32), mean[k].view(np.int32))
    assert np.array_equal(wide["count"], mean["count"])
    _, _, _, W, H = s["grid"]
    acc, counters = O.splat(s["rays"], s["depth"], s["features"], s["grid"], 1, "disc", np.full((H, W), O.EMPTY, dtype=object), 0)
    assert counters == [0, 0, 0] and np.array_equal(O.as_int64(acc), mean["acc"])
    # and band 0 keeps, per cell, exactly the points at the cell's top
    zero = O.statement(s["rays"], s["depth"], s["features"], s["grid"], 1, "disc", "top", 0.0)
    filled = zero["count"] > 0
    assert np.array_equal(zero["acc"][..., 0][filled], (zero["top"] * zero["acc"][..., 1])[filled])
    assert np.array_equal(filled, mean["count"] > 0)


def test_quantisation_bound():
    """|map - exact mean of the float32 features| <= 2^-25 + one float32 rounding of the result, in every cell and channel of the
    contention case (up to ~200 points per cell, values up to +-300 and the largest accepted magnitude).  Each f_e is within 2^-25
    of x_e, so their mean is; the two float64 operations of the resolve add 2^-52 relative each, counted as |v| 2^-50."""
    grid, rays, depth, feats = O.contention_case()
    radius, footprint = 1, "disc"
    got = O.statement(rays, depth, feats, grid, radius, footprint)
    _, _, _, W, H = grid
    sums = [[[Fraction(0)] * feats.shape[1] for _ in range(W)] for _ in range(H)]
    for cell, x in zip(O._cells(rays, depth, grid, radius, O.CENTER, O.RANGE), feats):
        if cell:
            for row, col in O._footprint(cell[0], cell[1], W, H, radius, footprint):
                for e, v in enumerate(x):
                    sums[row][col][e] += Fraction(float(v))
    worst = 0.0
    for row in range(H):
        for col in range(W):
            n = int(got["count"][row, col])
            assert n > 30
            for e in range(feats.shape[1]):
                exact = sums[row][col][e] / n
                v = float(got["maps"][e, row, col])
                err = abs(Fraction(v) - exact)
                bound = Fraction(1, 2 ** 25) + abs(exact) * Fraction(1, 2 ** 24) + abs(exact) * Fraction(1, 2 ** 50)
                worst = max(worst, float(err / bound))
                assert err <= bound, (row, col, e, float(err), float(bound))
    print(f"quantisation: worst error / bound {worst:.3f}")


def test_abi_and_exports():
    from brdf_nerf_amd import _lib
    header = open(os.path.join(ROOT, "include", "brdfnerf_hip.h")).read()
    declared = set(re.findall(r"\b(bn_\w+)\s*\(", header))
    for name, nargs in (("bn_ortho_top", 19), ("bn_ortho_splat", 24), ("bn_ortho_resolve", 8)):
        assert name in declared and name in _lib.exported_symbols() and len(_lib._SIGS[name][1]) == nargs, name
        assert hasattr(_lib.lib(), name), name
    assert "#define BN_ORTHO_MAX_CHANNELS 32" in header and _lib.BN_ORTHO_MAX_CHANNELS == 32
    assert _lib.BN_ORTHO_EMPTY == O.EMPTY == -(1 << 63) and "Orthorectified maps of a view" in header
    assert "NO upstream counterpart" in header and _lib.BN_ABI_VERSION == 7
    from brdf_nerf_amd.build import FILE_FLAGS
    assert "-ffp-contract=off" in FILE_FLAGS["ortho.hip"]
    csrc = os.path.join(ROOT, "brdf_nerf_amd", "csrc")
    for f in ("ortho.hip", "surface_cell.h"):
        assert "#pragma clang fp contract(off)" in open(os.path.join(csrc, f)).read()
    for f in ("ortho.hip", "world.hip"):                      # one statement of the point, cell and footprint chain, shared
        assert '#include "surface_cell.h"' in open(os.path.join(csrc, f)).read()
    import brdf_nerf_amd
    for name in ("OrthoAccumulator", "ortho_image"):
        assert name in brdf_nerf_amd.__all__ and callable(getattr(brdf_nerf_amd, name))


def test_refusals_that_need_no_device(monkeypatch):
    """ValueError by name from host tensors, before any library call (the loader is replaced by a trap)."""
    from brdf_nerf_amd import Grid, OrthoAccumulator, SceneFrame, _lib
    from brdf_nerf_amd import functions as Fn
    from brdf_nerf_amd.ortho import band_quanta

    def trap():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", trap)
    grid, frame = Grid(*D.SMALL), SceneFrame(D.CENTER, D.RANGE)
    make = lambda **kw: OrthoAccumulator(grid, "cpu", kw.pop("channels", 3), **kw)
    for kw, what in ((dict(mode="max"), "mode"), (dict(band=-0.5), "band"), (dict(band=float("nan")), "band"),
                     (dict(band=float("inf")), "band"), (dict(channels=33), "channels"), (dict(channels=-1), "channels"),
                     (dict(radius=5), "radius"), (dict(footprint="ring"), "footprint")):
        with pytest.raises(ValueError, match=what):
            make(**kw)
    assert band_quanta(0.5) == 1 << 19 and band_quanta(0) == 0 and band_quanta(1e300) == 1 << 62
    top = make()
    assert top.top.dtype == torch.int64 and int(top.top.min()) == int(top.top.max()) == O.EMPTY and tuple(top.acc.shape) == (5, 7, 5)
    assert make(mode="mean").top is None
    rays, depth = torch.zeros(4, 8), torch.ones(4)
    with pytest.raises(ValueError, match="mean"):
        make(mode="mean").add_top(rays, depth, frame)
    with pytest.raises(ValueError, match="mean"):
        make(mode="mean").merge_top()
    for feats in (torch.zeros(4, 3), torch.zeros(4, 2), torch.zeros(4, 3, dtype=torch.float64), None, np.zeros((4, 3), np.float32)):
        with pytest.raises(ValueError, match="features"):
            top.add(rays, depth, frame, feats)                # host tensors, another width, another dtype, none, not a tensor
    # add_top after the first add: pass 1 must be complete before pass 2 starts
    monkeypatch.setattr(Fn, "ortho_splat", lambda *a, **k: None)
    monkeypatch.setattr(Fn, "ortho_top", lambda *a, **k: None)
    plain = make(channels=0)
    plain.add_top(rays, depth, frame).add_top(rays, depth, frame).add(rays, depth, frame)
    with pytest.raises(ValueError, match="pass 1"):
        plain.add_top(rays, depth, frame)
    assert math.isfinite(plain.band) and plain.band_q == 1 << 19
