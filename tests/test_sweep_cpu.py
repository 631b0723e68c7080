"""Host tests of the altitude sweep (no device): the numpy statement of tests/sweep_cases.py against the two-pass float64 variance,
against the orthomosaic's statement at one level, the conditions on the end-to-end inputs with their recorded counts, the tie rule,
min_views, a NaN base cell, the build, and the wrapper refusals that need no device."""
import os
import re

import numpy as np
import pytest
import torch

import camera_cases as K
import mosaic_cases as M
import orthophoto_cases as O
import sweep_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def scene():
    return S.scene()


@pytest.fixture(scope="module")
def raised_sweep(scene):
    ds, planes, dsm, xoff, yoff, res, zone = scene
    return S.sweep(ds, planes, M.raised(dsm), xoff, yoff, res, zone, S.SCENE_OFFSETS)


@pytest.mark.parametrize("Cn", (1, 3, 4))
@pytest.mark.parametrize("views", (2, 5, 32))
def test_cost_against_the_two_pass_variance(views, Cn):
    """Welford's M2 / n against np.var of the used views, summed over the channels: the error of one channel is of order K 2^-53 of
    the largest x^2; K C 2^-50 max(x^2) leaves a margin of 8 for the per-step roundings, as test_mosaic_cpu.py leaves for std."""
    n = 4000
    values, states = M.random_stack(views, Cn, n, specials=False)
    got = S.pick([(values, states)], np.zeros(n, np.float32), [0.0], min_views=1)
    used = states == O.KEPT
    x = values.astype(np.float64)
    want = np.full(n, np.nan)
    for i in np.flatnonzero(used.any(0)):
        want[i] = sum(np.var(x[used[:, i], ch, i]) for ch in range(Cn))
    has = got["level"] == 0
    assert np.array_equal(has, used.any(0)) and has.sum() >= 3000 and np.array_equal(got["count"], used.sum(0))
    bound = views * Cn * 2.0 ** -50 * float((x * x).max())
    err = float(np.abs(got["cost64"][has] - want[has]).max())
    print(f"K={views} C={Cn}: the cost within {err:.3g} of the sum of np.var in float64 (bound {bound:.3g})")
    assert err <= bound
    assert O.same_f32(got["cost_min"], got["cost64"].astype(np.float32)) and O.same_f32(got["cost"][0], got["cost_min"])


def test_one_level_is_the_orthomosaic(scene):
    """offsets = [0]: the sweep's count and validity are the orthomosaic statement's count >= 2, valid[0] its sums[0], and the cost
    the sum of its squared float64 spreads up to their roundings."""
    ds, planes, dsm, xoff, yoff, res, zone = scene
    got = S.sweep(ds, planes, dsm, xoff, yoff, res, zone, [0.0])
    mosaic = M.mosaic(ds, planes, dsm, xoff, yoff, res, zone)
    twice = mosaic["count"] >= 2
    assert np.array_equal(got["level"] == 0, twice) and np.array_equal(got["level"] == -1, ~twice)
    assert np.array_equal(got["count"][twice], mosaic["count"][twice]) and (got["count"][~twice] == 0).all()
    assert got["valid"] == [mosaic["sums"][0]] == got["wins"] and got["sums"][0] == mosaic["sums"][0] >= 1500
    spread = mosaic["std64"].reshape(1, *dsm.shape)[0]
    assert np.allclose(got["cost64"][twice], spread[twice] ** 2, rtol=1e-12, atol=0.0)
    assert np.array_equal(got["altitude"][twice], dsm[twice]) and np.isnan(got["altitude"][~twice]).all()


@pytest.mark.parametrize("which", ("raised", "true", "raised_tenth"))
def test_the_scene_finds_the_planted_error(scene, raised_sweep, which):
    """Conditions on the inputs of the GPU end-to-end test, asserted on the statement alone, and the exact counts, recorded."""
    ds, planes, dsm, xoff, yoff, res, zone = scene
    offsets = S.SCENE_OFFSETS + (0.1 if which == "raised_tenth" else 0.0)
    got = raised_sweep if which == "raised" else S.sweep(ds, planes, dsm if which == "true" else M.raised(dsm), xoff, yoff, res, zone, offsets)
    roof, ground, astray, none = S.scene_counts(got, dsm, 8 if which == "true" else 2)
    print(f"{which}: {roof} of the 100 roof cells at {offsets[8 if which == 'true' else 2]:+.1f} m, {ground} ground cells with a result and "
          f"{astray} of them not at {offsets[8]:+.1f} m, {none} cells without one; valid {got['valid']}; wins {got['wins']}; mean cost "
          f"{got['sums'][1] / (got['sums'][0] * S.Q20):.6g}")
    assert roof >= 80 and astray == 0 and roof + ground >= 1500
    want = S.SCENE_RECORD[which]
    assert (roof, ground, none) == (want["roof"], want["ground"], want["none"])
    assert got["valid"] == want["valid"] and got["wins"] == want["wins"] and got["sums"][0] == sum(want["wins"]) and got["sums"][2] == 0
    has = got["level"] >= 0
    assert np.array_equal(got["altitude"][has], ((M.raised(dsm) if which != "true" else dsm).astype(np.float64)[has]
                                                 + offsets[got["level"][has]]).astype(np.float32))
    if which == "raised":                                                    # the refined model has the true roof back
        assert (np.abs(got["altitude"][S.roof_mask(dsm)] - dsm[S.roof_mask(dsm)]) == 0).sum() == roof


def test_the_scene_without_occlusion(scene):
    ds, planes, dsm, xoff, yoff, res, zone = scene
    got = S.sweep(ds, planes, M.raised(dsm), xoff, yoff, res, zone, S.SCENE_OFFSETS, occlusion=False)
    roof, ground, astray, none = S.scene_counts(got, dsm, 2)
    want = S.SCENE_RECORD["raised_unoccluded"]
    print(f"without occlusion: {roof} roof cells at -6 m, {ground} ground cells with a result, {astray} of them not at 0, wins {got['wins']}")
    assert roof >= 80 and (roof, ground, none) == (want["roof"], want["ground"], want["none"])
    assert got["valid"] == want["valid"] and got["wins"] == want["wins"] and 0 < astray < 100


def test_a_tie_goes_to_the_first_level(scene):
    """Constant images: every level gathers the same values, so every level has the same cost and the strict < keeps level 0; a <=
    comparison would keep the last one."""
    ds, _, dsm, xoff, yoff, res, zone = scene
    planes = [M.planted_image(1, *M.TEXTURE_IMAGE, k) for k in range(len(ds))]
    Z = len(S.SCENE_OFFSETS)
    got = S.sweep(ds, planes, dsm, xoff, yoff, res, zone, S.SCENE_OFFSETS)
    has = got["level"] >= 0
    assert has.sum() >= 1500 and (got["level"][has] == 0).all() and got["wins"] == [got["sums"][0]] + [0] * (Z - 1)
    assert (got["cost"][:, has] == got["cost"][0, has]).all() and (got["cost_min"][has] > 0).all()
    other = S.sweep(ds, planes, dsm, xoff, yoff, res, zone, S.SCENE_OFFSETS, strict=False)
    assert (other["level"][has] == Z - 1).all() and other["wins"][Z - 1] == got["sums"][0]
    twice = S.sweep(ds, planes, dsm, xoff, yoff, res, zone, [3.0, -2.0, 3.0, -2.0])          # unsorted, repeated offsets
    assert (twice["level"][has] == 0).all()


def test_min_views(scene, raised_sweep):
    ds, planes, dsm, xoff, yoff, res, zone = scene
    runs = {2: raised_sweep}
    for mv in (1, 3):
        runs[mv] = S.sweep(ds, planes, M.raised(dsm), xoff, yoff, res, zone, S.SCENE_OFFSETS, min_views=mv)
    for lo, hi in ((1, 2), (2, 3)):
        ok_lo, ok_hi = ~np.isnan(runs[lo]["cost"]), ~np.isnan(runs[hi]["cost"])
        assert not (ok_hi & ~ok_lo).any() and (ok_lo & ~ok_hi).any()                        # never invalid -> valid, and it bites
        assert all(a >= b for a, b in zip(runs[lo]["valid"], runs[hi]["valid"]))
    once = (runs[1]["count"] == 1)
    assert once.sum() >= 10 and (runs[1]["cost_min"][once] == 0.0).all() and not np.signbit(runs[1]["cost_min"][once]).any()
    values = np.array([[[1.5, 2.0]], [[np.nan, 4.0]]], dtype=np.float32)                     # cell 0 seen once, cell 1 twice
    states = np.full((2, 2), O.KEPT)
    assert S.pick([(values, states)], np.zeros(2, np.float32), [1.0], 1)["cost_min"].tolist() == [0.0, 1.0]
    two = S.pick([(values, states)], np.zeros(2, np.float32), [1.0], 2)
    assert two["level"].tolist() == [-1, 0] and np.isnan(two["cost_min"][0]) and two["count"].tolist() == [0, 2] and two["sums"] == [1, 1 << 20, 0]


def test_a_nan_base_cell_has_no_result(scene):
    ds, planes, dsm, xoff, yoff, res, zone = scene
    holed = np.array(dsm)
    holed[5, 7], holed[22, 18] = np.nan, np.inf
    got = S.sweep(ds, planes, holed, xoff, yoff, res, zone, S.SCENE_OFFSETS, occlusion=False, min_views=1)
    for cell in ((5, 7), (22, 18)):
        assert got["level"][cell] == -1 and got["count"][cell] == 0 and np.isnan(got["cost"][(slice(None), *cell)]).all()
        assert np.isnan(got["altitude"][cell]) and np.isnan(got["cost_min"][cell])
    assert (got["level"] >= 0).sum() == dsm.size - 2


def test_package_surface():
    import brdf_nerf_amd
    from brdf_nerf_amd import _lib
    from brdf_nerf_amd.build import FILE_FLAGS
    assert "altitude_sweep" in brdf_nerf_amd.__all__ and callable(brdf_nerf_amd.altitude_sweep)
    assert callable(brdf_nerf_amd.functions.grid_sweep)
    assert "-ffp-contract=off" in FILE_FLAGS["sweep.hip"]
    csrc = os.path.join(ROOT, "brdf_nerf_amd", "csrc")
    for f in ("sweep.hip", "view_step.h"):
        assert "#pragma clang fp contract(off)" in open(os.path.join(csrc, f)).read()
    for f in ("sweep.hip", "mosaic.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "view_step.h"' in text and "view_step::add_view<C>" in text          # one statement of the per-view step, shared
        assert "delta / (double)n" not in text                                               # and no second Welford beside it
    header = open(os.path.join(ROOT, "include", "brdfnerf_hip.h")).read()
    assert "Altitude sweep of a surface model under several observed images" in header
    declared = set(re.findall(r"\b(bn_[a-z0-9_]+)\s*\(", header))
    assert "bn_grid_sweep" in declared and "bn_grid_sweep" in _lib.exported_symbols() and len(_lib._SIGS["bn_grid_sweep"][1]) == 29
    assert re.search(rf"#define BN_SWEEP_MAX_LEVELS {S.MAX_LEVELS}\b", header) and _lib.BN_SWEEP_MAX_LEVELS == S.MAX_LEVELS == 256
    lib = os.path.join(ROOT, "brdf_nerf_amd", "libbrdfnerf_hip.so")
    assert b"bn_grid_sweep" in open(lib, "rb").read()                                        # exported by the cross-compiled library
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "## Altitude sweep of a surface model" in readme


def test_wrapper_refusals_without_a_device():
    from brdf_nerf_amd import Grid, Rpc, altitude_sweep
    rpc = Rpc.from_dict(K.make_rpc("z17", 1))
    grid = Grid(0.0, 0.0, 0.5, 5, 4)
    dsm, img = torch.zeros(4, 5), torch.zeros(6 * 7, 3)
    view = (img, 6, 7, rpc)
    off = [-1.0, 0.0, 1.0]
    with pytest.raises(ValueError, match="0 views"):
        altitude_sweep([], dsm, grid, 17, off)
    with pytest.raises(ValueError, match="33 views"):
        altitude_sweep([view] * 33, dsm, grid, 17, off)
    with pytest.raises(ValueError, match="channels"):
        altitude_sweep([view, (torch.zeros(6 * 7, 2), 6, 7, rpc)], dsm, grid, 17, off)
    with pytest.raises(ValueError, match="view 1"):
        altitude_sweep([view, (img, 6, 7)], dsm, grid, 17, off)
    for bad in ([], [0.0] * 257, torch.zeros(2, 2), 1.0):
        with pytest.raises(ValueError, match="offsets"):
            altitude_sweep([view], dsm, grid, 17, bad)
    for bad in ([0.0, float("nan")], [float("inf")], torch.tensor([0.0, -float("inf")])):
        with pytest.raises(ValueError, match="finite"):
            altitude_sweep([view], dsm, grid, 17, bad)
    for bad in (0, 33, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="min_views"):
            altitude_sweep([view], dsm, grid, 17, off, min_views=bad)
    for vd, what in (([[0.0, 0.0, 1.0]], "view_dirs"), ([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0]], "upwards")):
        with pytest.raises(ValueError, match=what):
            altitude_sweep([view, view], dsm, grid, 17, off, view_dirs=vd)
    for bad, what in ((dsm.double(), "float32"), (dsm[:, ::2], "contiguous"), (torch.zeros(5, 4), "grid")):
        with pytest.raises(ValueError, match=what):
            altitude_sweep([view], bad, grid, 17, off)
    for kw, what in ((dict(mode="cubic"), "mode"), (dict(layout="chw"), "layout"), (dict(rows=(2, 1)), "rows"), (dict(rows=(0, 5)), "rows"),
                     (dict(eps=-1.0), "eps"), (dict(alt_bounds=(5.0, 5.0)), "alt_bounds"), (dict(zone=61), "zone"),
                     (dict(colrow=torch.zeros(3, 1, 4, 5, 2)), "float64"), (dict(colrow=torch.zeros(1, 4, 5, 2, dtype=torch.float64)), "colrow"),
                     (dict(colrow=torch.zeros(2, 1, 4, 5, 2, dtype=torch.float64)), "colrow")):
        kw = dict(dict(zone=17), **kw)
        with pytest.raises(ValueError, match=what):
            altitude_sweep([view], dsm, grid, offsets=off, **kw)
    with pytest.raises(ValueError, match="device"):
        altitude_sweep([view], dsm, grid, 17, off)
