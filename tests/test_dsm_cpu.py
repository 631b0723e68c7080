"""CPU tests of the DSM feature (brdf_nerf_amd/dsm.py): the grid rules and the altitude MAE on hand-worked numbers, the
float64 statement of the rasteriser (tests/dsm_cases.py) checked for the invariances it is about to measure, and the ABI."""
import os
import re

import numpy as np
import pytest
import torch

import dsm_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_grid_from_cloud_follows_the_reference_rule():
    """datasets/satellite_rgb_dep.py:665-671 on hand-worked numbers: x in [10.3, 14.9] at 0.5 m -> xoff 10, 1 + floor(4.9 / 0.5)
    = 10 columns; y in [20.7, 23.2] -> yoff = ceil(46.4) 0.5 = 23.5, 1 - floor((20.7 - 23.5) / 0.5) = 1 + 6 = 7 rows."""
    from brdf_nerf_amd import Grid
    g = Grid.from_cloud((10.3, 20.7), (14.9, 23.2))
    assert (g.xoff, g.yoff, g.resolution, g.width, g.height) == (10.0, 23.5, 0.5, 10, 7)
    # bounds exactly on cell edges: xmax on an edge opens one more column, ymin on an edge one more row
    g = Grid.from_cloud((10.0, 20.0), (12.0, 22.0), resolution=1.0)
    assert (g.xoff, g.yoff, g.width, g.height) == (10.0, 22.0, 1 + 2, 1 + 2)
    # negative coordinates and a coarse resolution: floor, not truncation
    g = Grid.from_cloud((-3.2, -7.9), (-0.1, -4.1), resolution=2.0)
    assert (g.xoff, g.yoff, g.width, g.height) == (-4.0, -4.0, 1 + 1, 1 + 2)      # floor((-7.9 + 4) / 2) = -2
    # a single point: one column, and the row above it too (1 - floor(-0.5) = 2)
    g = Grid.from_cloud((5.25, 5.25), (5.25, 5.25))
    assert (g.xoff, g.yoff, g.width, g.height) == (5.0, 5.5, 1, 2)


def test_grid_from_roi_is_the_ground_truth_grid():
    """:658-663: (x, y, size, resolution) -> a square grid whose upper edge is y + size * resolution."""
    from brdf_nerf_amd import Grid
    g = Grid.from_roi((368000.0, 3359000.0, 512, 0.5))
    assert (g.xoff, g.yoff, g.resolution, g.width, g.height) == (368000.0, 3359256.0, 0.5, 512, 512)
    g = Grid.from_roi(np.array([100.0, 200.0, 8.0, 0.25]))
    assert (g.xoff, g.yoff, g.width, g.height) == (100.0, 202.0, 8, 8)
    with pytest.raises(ValueError):
        Grid(0.0, 0.0, 0.0, 4, 4)
    with pytest.raises(ValueError):
        Grid(0.0, 0.0, 0.5, 0, 4)


def test_altitude_mae_against_numpy():
    """sat_utils.py:235, 246, 340-349 restated in numpy: NaN holes in both images, and a mask (MaskDoD)."""
    from brdf_nerf_amd import altitude_mae
    g = np.random.RandomState(0)
    gt = 20.0 + 5.0 * g.rand(9, 13)
    pred = gt + 1.75 + 0.3 * g.randn(9, 13)               # an offset the z registration removes
    pred[g.rand(9, 13) < 0.2] = np.nan
    gt[g.rand(9, 13) < 0.1] = np.nan
    mask = g.rand(9, 13) < 0.5
    pred_r = pred + np.nanmean((gt - pred).ravel())
    diff = pred_r - gt
    want = np.nanmean(np.abs(diff.ravel()))
    d_in, d_out = diff.copy(), diff.copy()
    d_in[mask == False] = np.nan                          # noqa: E712 (MaskDoD's own statement)
    d_out[mask == True] = np.nan                          # noqa: E712
    got = altitude_mae(torch.from_numpy(pred), torch.from_numpy(gt), torch.from_numpy(mask))
    assert got["mae"] == pytest.approx(want, rel=1e-12) and got["mae"] < 0.5
    assert got["mae_in"] == pytest.approx(np.nanmean(np.abs(d_in.ravel())), rel=1e-12)
    assert got["mae_out"] == pytest.approx(np.nanmean(np.abs(d_out.ravel())), rel=1e-12)
    assert got["shift"] == pytest.approx(np.nanmean((gt - pred).ravel()), rel=1e-12)
    np.testing.assert_allclose(got["diff"].numpy(), diff, rtol=0, atol=1e-12, equal_nan=True)
    plain = altitude_mae(pred, gt)                        # numpy in, no mask
    assert set(plain) == {"mae", "shift", "diff"} and plain["mae"] == got["mae"]
    # hand-worked: pred = gt - 2 on two cells and gt on two -> shift 1 -> |diff| = 1 everywhere
    r = altitude_mae(torch.tensor([[1.0, 2.0], [5.0, 6.0]]), torch.tensor([[3.0, 4.0], [5.0, 6.0]]))
    assert r["shift"] == 1.0 and r["mae"] == 1.0
    with pytest.raises(ValueError):
        altitude_mae(torch.zeros(3, 4), torch.zeros(4, 3))


def test_ecef_is_refused_by_name():
    from brdf_nerf_amd import SceneFrame
    with pytest.raises(NotImplementedError, match="ecef"):
        SceneFrame(D.CENTER, D.RANGE, cs="ecef")
    f = SceneFrame(np.array(D.CENTER), D.RANGE)
    assert f.cs == "utm" and f.center == D.CENTER and f.range == D.RANGE


def test_point_cloud_is_the_statement_on_the_host():
    """point_cloud / altitude_image in torch float64 equal the numpy statement bit for bit (each operation rounded once)."""
    from brdf_nerf_amd import SceneFrame, altitude_image, point_cloud
    _, _, _, rays, depth = D.case("large_R300_r1_disc")
    frame = SceneFrame(D.CENTER, D.RANGE)
    want = D.points(rays, depth)
    got = point_cloud(torch.from_numpy(rays.copy()), torch.from_numpy(depth.copy()), frame)
    assert got.dtype == torch.float64
    np.testing.assert_array_equal(got.numpy(), want)          # NaN rows compare equal here
    np.testing.assert_array_equal(altitude_image(torch.from_numpy(rays.copy()), torch.from_numpy(depth.copy()), frame).numpy(), want[:, 2])


def test_the_cases_hold_what_they_promise():
    """The yardstick before it measures: edge points, clipped footprints, skipped rows, negative altitudes, empty cells, total
    contention - and the fp32-position guard: rounding the positions to fp32 changes the guarded case."""
    one = D.expected("one_point_r1_disc")
    want = np.zeros((5, 7), dtype=np.int64)
    want[2, 3] = want[1, 3] = want[3, 3] = want[2, 2] = want[2, 4] = 1         # a point ON the corner (row 2, column 3): floor puts it there
    assert np.array_equal(one["counts"], want) and one["skipped"] == 0
    assert np.array_equal(one["sums"], want * int(14.0 * 2 ** 20)) and np.all(one["dsm"][want == 1] == np.float32(14.0))
    assert np.isnan(one["dsm"][want == 0]).all()
    seen = {"skipped": 0, "empty": 0, "negative": 0}
    for name in D.CASES:
        grid, radius, footprint, rays, depth = D.case(name)
        e = D.expected(name)
        assert e["sums"].shape == (grid[4], grid[3]) and rays.dtype == np.float32 and depth.dtype == np.float32
        assert np.array_equal(np.isnan(e["dsm"]), e["counts"] == 0)
        seen["skipped"] += e["skipped"]
        seen["empty"] += int((e["counts"] == 0).sum())
        seen["negative"] += int((e["sums"] < 0).sum())
        if "small_R6" in name:
            assert e["skipped"] == 5, name          # NaN, +inf, -inf, |z| == 2^23 exactly, |z| ~ 1.2e7; the row at 8388602 m is kept
            assert int(e["sums"].max()) >= 8388602 * 2 ** 20
    assert all(v > 0 for v in seen.values()), seen
    # the square footprint takes more cells than the disc: 25 against 13 at radius 2, 9 against 5 at radius 1
    assert D.expected("large_R300_r2_square")["counts"].sum() > D.expected("large_R300_r2_disc")["counts"].sum()
    assert D.expected("small_R65_r1_square")["counts"].sum() > D.expected("small_R65_r1_disc")["counts"].sum()
    # a point whose centre cell is outside still reaches inside: x = 0.75 m (column 7 of 7), y = 0.75 m (row 0)
    r, t = D._nadir(np.array([0.75]), np.array([0.75]), np.array([0.0]), 0.5)
    s0, c0, _ = D.splat(r, t, D.SMALL, 0, "square")
    s1, c1, _ = D.splat(r, t, D.SMALL, 1, "disc")
    assert D.as_int64(c0).sum() == 0 and D.as_int64(c1).sum() == 1 and D.as_int64(c1)[0, 6] == 1
    # the south outer edge itself belongs to the row below the grid, the west outer edge to column 0
    r, t = D._nadir(np.array([-3.0, -3.0]), np.array([-1.5, -0.75]), np.array([0.0, 0.0]), 0.5)
    _, c, _ = D.splat(r, t, D.SMALL, 0, "square")
    assert D.as_int64(c).sum() == 1 and D.as_int64(c)[3, 0] == 1
    cont = D.expected("contention_R4096_r1_disc")
    assert cont["counts"][1, 3] == 4096 and cont["counts"].sum() == 5 * 4096 and (cont["counts"] == 0).sum() == 30
    guard, guard32 = D.expected(D.FP32_GUARD_CASE), D.expected(D.FP32_GUARD_CASE, True)
    assert not np.array_equal(guard["counts"], guard32["counts"]), "fp32 positions must move points across cells"


def test_the_statement_is_order_and_chunk_invariant():
    """Integer sums: a permutation of the rows, and the rows added in chunks of 1, 64 and 100, give the same accumulator."""
    name = "large_R300_r2_disc"
    grid, radius, footprint, rays, depth = D.case(name)
    e = D.expected(name)
    perm = np.random.RandomState(3).permutation(rays.shape[0])
    s, c, k = D.splat(rays[perm], depth[perm], grid, radius, footprint)
    assert np.array_equal(D.as_int64(s), e["sums"]) and np.array_equal(D.as_int64(c), e["counts"]) and k == e["skipped"]
    for chunk in (1, 64, 100):
        acc = None
        for i in range(0, rays.shape[0], chunk):
            acc = D.splat(rays[i:i + chunk], depth[i:i + chunk], grid, radius, footprint, acc=acc)
        assert np.array_equal(D.as_int64(acc[0]), e["sums"]) and np.array_equal(D.as_int64(acc[1]), e["counts"]) and acc[2] == e["skipped"], chunk


def test_header_and_binding_carry_both_entries():
    from brdf_nerf_amd import _lib
    header = open(os.path.join(ROOT, "include", "brdfnerf_hip.h")).read()
    declared = set(re.findall(r"\b(bn_[a-z0-9_]+)\s*\(", header))
    for name in ("bn_dsm_splat", "bn_dsm_resolve"):
        assert name in declared and name in _lib._SIGS, name
        assert hasattr(_lib.lib(), name), name
    assert re.search(r"BN_DSM_DISC\s*=\s*0\s*,\s*BN_DSM_SQUARE\s*=\s*1", header) and (_lib.BN_DSM_DISC, _lib.BN_DSM_SQUARE) == (0, 1)
    assert int(re.search(r"#define BN_DSM_MAX_RADIUS (\d+)", header).group(1)) == _lib.BN_DSM_MAX_RADIUS == 4
    assert _lib.BN_ABI_VERSION == 7 and _lib.lib().bn_abi_version() == 7
    assert len(_lib._SIGS["bn_dsm_splat"][1]) == 16 and len(_lib._SIGS["bn_dsm_resolve"][1]) == 6


def test_accumulator_refuses_bad_arguments_before_any_device_work():
    from brdf_nerf_amd import DsmAccumulator, Grid
    g = Grid(*D.SMALL)
    with pytest.raises(ValueError, match="radius"):
        DsmAccumulator(g, "cpu", radius=5)
    with pytest.raises(ValueError, match="radius"):
        DsmAccumulator(g, "cpu", radius=-1)
    with pytest.raises(ValueError, match="footprint"):
        DsmAccumulator(g, "cpu", footprint="gauss")


def test_the_chain_is_stated_once():
    """The point, cell and deposit chain has one statement, csrc/surface_cell.h, which world.hip (every DSM entry) and ortho.hip are
    made of: no second copy of the arithmetic, of its argument struct or of the host checks as macros, and no retired A/B form."""
    from brdf_nerf_amd.build import FILE_FLAGS
    csrc = os.path.join(ROOT, "brdf_nerf_amd", "csrc")
    assert not os.path.exists(os.path.join(csrc, "dsm.hip")) and "dsm.hip" not in FILE_FLAGS
    text = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc))}
    hips = [f for f in text if f.endswith(".hip")]
    assert "world.hip" in hips and "ortho.hip" in hips
    cell_index = re.compile(r"floor\(\([^\n]*/[^\n]*resolution\)")
    assert len(cell_index.findall(text["surface_cell.h"])) == 2          # the column and the row
    for f in text:                                                       # (the headers too)
        assert "struct DsmArgs" not in text[f] and "#define WORLD_REQUIRE_" not in text[f], f
    for f in hips:
        assert not cell_index.search(text[f]), f
    assert '#include "surface_cell.h"' in text["world.hip"] and "#pragma clang fp contract(off)" in text["world.hip"]
    assert "-ffp-contract=off" in FILE_FLAGS["world.hip"]
    for f, s in text.items():
        assert "BN_ORTHO_LANE_PER_RAY" not in s, f
