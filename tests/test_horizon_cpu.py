"""The horizon and sky-view rule's numpy statement on its own cases, its agreement with the shadow march, the package surface and
the wrapper refusals: no GPU, no library."""
import math
import os
import re

import numpy as np
import pytest
import torch

import horizon_cases as Hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

bits = lambda a: a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_floats(a, b):
    """Bit for bit, a NaN being a NaN whatever its payload."""
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(bits(a)[~np.isnan(a)], bits(b)[~np.isnan(b)])


@pytest.mark.parametrize("shape", Hc.GRID_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_zmax_changes_no_bit(shape):
    """The early exit under the grid's maximum against the plain rule (zmax = +inf): slope, hit and acc."""
    dsm = Hc.grid_case(shape)
    az = Hc.all_azimuths()
    plain = Hc.grid_statement(dsm, Hc.RES, az)
    early = Hc.grid_statement(dsm, Hc.RES, az, zmax=Hc.grid_zmax(dsm))
    assert same_floats(plain[0], early[0]) and np.array_equal(plain[1], early[1])
    sparse = Hc.grid_statement(dsm, Hc.RES, az, zmax=Hc.grid_zmax(dsm), exit_every=8)       # the test is valid at any step: the kernels make it once per 8
    assert same_floats(plain[0], sparse[0]) and np.array_equal(plain[1], sparse[1])
    assert same_floats(Hc.sky_statement(plain[0])[0], Hc.sky_statement(early[0])[0])
    if shape[0] * shape[1] >= 8:
        assert (plain[0] > 0).any() and (plain[0] == 0).any()           # a condition on the inputs: both kinds of horizon occur


def test_closed_form_row():
    slope, hit = Hc.grid_statement(Hc.closed_row(), 0.5, Hc.CARDINALS)
    north, east, south, west = slope[:, 0]
    assert np.array_equal(east, np.array(Hc.CLOSED_EAST, dtype=np.float32)) and np.array_equal(west, east[::-1])
    assert (north == 0).all() and (south == 0).all()
    assert hit[1, 0].tolist() == [4, 4, 4, 4, -1, -1, -1, -1, -1] and hit[3, 0].tolist() == [-1, -1, -1, -1, -1, 4, 4, 4, 4]
    acc, svf, sums = Hc.sky_statement(slope)
    want = np.array(Hc.CLOSED_SVF + Hc.CLOSED_SVF[-2::-1], dtype=np.float64)
    assert svf[0, 0] == 0.875 and svf[0, 2] == np.float32(0.8) and svf[0, 4] == 1.0
    assert np.allclose(svf[0], want, rtol=0, atol=2.0 ** -24) and np.array_equal(svf[0], svf[0][::-1])
    assert sums[1:].tolist() == [9, 0]


def test_the_first_cell_keeps_a_tie():
    slope, hit = Hc.grid_statement(Hc.tie_row(), 0.5, [[1.0, 0.0]])
    assert slope[0, 0, 0] == 2.0 and hit[0, 0, 0] == 1
    assert (11.0 - 10.0) / 0.5 == (12.0 - 10.0) / 1.0 == (14.0 - 10.0) / 2.0 == 2.0      # the tie is exact


def test_flat_and_all_nan_grids():
    az = Hc.all_azimuths()
    slope, hit = Hc.grid_statement(np.full((9, 13), 4.0, dtype=np.float32), Hc.RES, az)
    acc, svf, sums = Hc.sky_statement(slope)
    assert (slope == 0).all() and (hit == -1).all() and (svf == 1.0).all() and sums.tolist() == [9 * 13 << 30, 9 * 13, 0]
    slope, hit = Hc.grid_statement(np.full((5, 70), np.nan, dtype=np.float32), Hc.RES, az, zmax=-Hc.INF)
    acc, svf, sums = Hc.sky_statement(slope)
    assert np.isnan(slope).all() and (hit == -1).all() and np.isnan(svf).all() and sums.tolist() == [0, 0, 350]


@pytest.mark.parametrize("D", sorted(Hc.BLOCK_SVF))
def test_block_scene_sky_view(D):
    """The prototype's counts of cells below 1 (asserted by the generator), the recorded integer sums, the means, and the roof:
    nothing on the grid is higher, so every roof cell sees the whole sky."""
    slope, acc, svf, sums = Hc.block_svf(D)
    assert tuple(int(v) for v in sums) == Hc.BLOCK_SVF[D][1]
    mean = int(sums[0]) / (int(sums[1]) * 2 ** 30)
    assert abs(mean - {4: 0.91608, 8: 0.88353, 16: 0.88081, 32: 0.87931}[D]) < 5e-6
    assert (svf[24:40, 24:40] == 1.0).all() and (svf <= 1.0).all() and (svf > 0).all()


@pytest.mark.parametrize("shape", Hc.AGREE_GRIDS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_horizon_agrees_with_the_shadow_march(shape):
    """slope > tan(elevation) is the shadow march's BLOCKED, on every cell with data whose slope is not within 1e-6 (1 + tan) of
    the tangent; at most 1 % of the cells with data may be that close (a condition on the inputs)."""
    dsm = Hc.grid_case(shape)
    for el, azd in Hc.AGREE_DIRS:
        d = Hc.direction(el, azd)
        slope, _ = Hc.grid_statement(dsm, Hc.RES, [d[:2]], zmax=Hc.grid_zmax(dsm))
        compared, data, wrong = Hc.agreement(dsm, slope[0], d)
        assert data - compared <= 0.01 * data, (el, azd, data - compared)
        assert wrong == 0, (el, azd, wrong)


def test_grid_mode_is_point_mode_on_the_cell_centres():
    """On a dyadic origin and resolution the centres and the quotients are exact: both modes give the same bits."""
    xoff, yoff, res = 1024.0, 2048.0, 0.5
    az = Hc.all_azimuths()
    for dsm in (Hc.block_scene(), Hc.relief(33, 65, seed=5)):
        g = Hc.grid_statement(dsm, res, az)
        p = Hc.points_statement(Hc.cell_centres(dsm, xoff, yoff, res), dsm, xoff, yoff, res, az)
        assert same_floats(g[0].reshape(len(az), -1), p[0]) and np.array_equal(g[1].reshape(len(az), -1), p[1])


def test_points_outside_and_without_data():
    dsm = Hc.block_scene()
    pts = np.array([[5.0, -5.0, 25.0], [-0.25, -5.0, 11.0], [5.0, 0.25, 11.0], [32.0, -5.0, 11.0], [5.0, -32.0, 11.0],
                    [np.nan, -5.0, 11.0], [5.0, -5.0, np.inf], [0.0, 0.0, 25.0], [5.0, -16.0, 11.0]])
    slope, hit = Hc.points_statement(pts, dsm, 0.0, 0.0, Hc.RES, [[1.0, 0.0]])
    assert np.isnan(slope[0][1:7]).all() and (hit[0][1:7] == -1).all()
    assert slope[0][0] == 0 and slope[0][7] == 0 and hit[0][7] == -1           # above the ground, east along rows 10 and 0: no roof
    assert slope[0][8] == np.float32(19.0 / 7.0) and hit[0][8] == 32 * 64 + 24  # 14 cells = 7 m to the roof's wall, 19 m up


def test_what_each_perturbation_would_change():
    """The statement's own account of the rule's choices on the 33 x 65 relief: a descending sum moves acc but no svf float32, the
    unrounded best moves svf; max_steps is a prefix of the march."""
    dsm = Hc.grid_case((33, 65))
    az = Hc.azimuths(16, 7.0)
    slope, _ = Hc.grid_statement(dsm, Hc.RES, az)
    acc, svf, _ = Hc.sky_statement(slope)
    acc_d, svf_d, _ = Hc.sky_statement(slope, descending=True)
    data = ~np.isnan(acc)
    assert (acc[data] != acc_d[data]).sum() > 100 and same_floats(svf, svf_d)
    _, svf_b, _ = Hc.sky_statement(slope, stored=Hc.best_statement(dsm, Hc.RES, az))
    assert (svf[data] != svf_b[data]).sum() > 10
    near, _ = Hc.grid_statement(dsm, Hc.RES, az, max_steps=3)
    assert (near[~np.isnan(near)] <= slope[~np.isnan(slope)]).all() and (near != slope)[data[None].repeat(16, 0)].any()


def test_package_surface():
    import brdf_nerf_amd
    from brdf_nerf_amd import _lib, horizon
    from brdf_nerf_amd.build import FILE_FLAGS
    for name in ("azimuths", "grid_horizon", "sky_view_factor", "point_sky_view", "view_sky_view"):
        assert name in brdf_nerf_amd.__all__ and getattr(brdf_nerf_amd, name) is getattr(horizon, name)
    assert "-ffp-contract=off" in FILE_FLAGS["horizon.hip"]
    src = open(os.path.join(ROOT, "brdf_nerf_amd", "csrc", "horizon.hip")).read()
    assert "#pragma clang fp contract(off)" in src
    header = open(os.path.join(ROOT, "include", "brdfnerf_hip.h")).read()
    assert "Horizon and sky view over a surface model" in header and "rounded division by a growing positive run is monotone" in header
    declared = set(re.findall(r"\b(bn_[a-z0-9_]+)\s*\(", header))
    for name, nargs in (("bn_grid_horizon", 13), ("bn_points_horizon", 15), ("bn_sky_view", 10)):
        assert name in declared and name in _lib.exported_symbols() and len(_lib._SIGS[name][1]) == nargs, name
    assert re.search(rf"#define BN_HORIZON_MAX_DIRS {_lib.BN_HORIZON_MAX_DIRS}\b", header) and _lib.BN_HORIZON_MAX_DIRS == 4096
    assert horizon.SVF_FIX == int(Hc.SVF_FIX) == 1 << 30
    fn = open(os.path.join(ROOT, "brdf_nerf_amd", "functions.py")).read()
    assert fn.index("def cast_rays(") < fn.index("def grid_horizon(") < fn.index("def points_horizon(") < fn.index("def sky_view(")


def test_azimuths():
    from brdf_nerf_amd import azimuths
    for n, start in ((1, 0.0), (4, 0.0), (16, 7.0), (32, -11.5)):
        got = azimuths(n, start)
        assert got.dtype == torch.float64 and tuple(got.shape) == (n, 2) and not got.is_cuda
        assert np.array_equal(got.numpy(), Hc.azimuths(n, start))
    four = azimuths(4).numpy()
    assert np.abs(four - Hc.CARDINALS).max() < 2e-16 and four[0].tolist() == [0.0, 1.0]       # north first, then clockwise: east
    with pytest.raises(ValueError, match="azimuths"):
        azimuths(0)


def test_wrapper_refusals_without_a_device():
    from brdf_nerf_amd import Grid, SceneFrame, grid_horizon, point_sky_view, sky_view_factor, view_sky_view
    from brdf_nerf_amd import functions as Fn
    dsm = torch.zeros(4, 5)
    east = [1.0, 0.0]
    grid = Grid(0.0, 0.0, 0.5, 5, 4)
    for bad, what in ((dsm.double(), "float32"), (dsm[:, ::2], "contiguous"), (dsm[0], "2-D"), (dsm.numpy(), "tensor"), (dsm, "device")):
        with pytest.raises(ValueError, match=what):
            grid_horizon(bad, 0.5, east)
        with pytest.raises(ValueError, match=what):
            sky_view_factor(bad, 0.5)
    pts = torch.zeros(3, 3, dtype=torch.float64)
    for az, what in (([0.0, 0.0], r"\(0, 0\)"), ([float("nan"), 1.0], "finite"), ([[0.0, float("inf")]], "finite"),
                     (torch.zeros(2, 3), r"\(D, 2\)"), (torch.zeros(0, 2), r"\(D, 2\)"), (torch.ones(4097, 2), "4096"),
                     (torch.ones(2, dtype=torch.int64), "float")):
        with pytest.raises(ValueError, match=what):
            grid_horizon(dsm, 0.5, az)
        with pytest.raises(ValueError, match=what):
            sky_view_factor(dsm, 0.5, az=az)
        with pytest.raises(ValueError, match=what):
            Fn.points_horizon(pts, dsm, 0.0, 0.0, 0.5, az)
    for kw, what in ((dict(resolution=0.0), "resolution"), (dict(resolution=float("inf")), "resolution"), (dict(max_dist=0.0), "max_dist"),
                     (dict(max_dist=float("nan")), "max_dist"), (dict(rows=(2, 1)), "rows"), (dict(rows=(0, 5)), "rows")):
        with pytest.raises(ValueError, match=what):
            grid_horizon(dsm, **dict(dict(resolution=0.5, az=east), **kw))
        with pytest.raises(ValueError, match=what):
            sky_view_factor(dsm, **dict(dict(resolution=0.5), **kw))
    for kw, what in ((dict(dir_tile=0), "dir_tile"), (dict(n_az=0), "azimuths"), (dict(n_az=4097), "4096")):
        with pytest.raises(ValueError, match=what):
            sky_view_factor(dsm, 0.5, **kw)
    with pytest.raises(ValueError, match="zmax"):
        Fn.grid_horizon(dsm, 0.5, east, zmax=float("nan"))
    with pytest.raises(ValueError, match="max_steps"):
        Fn.grid_horizon(dsm, 0.5, east, max_steps=0)
    with pytest.raises(ValueError, match="origin"):
        Fn.points_horizon(pts, dsm, float("nan"), 0.0, 0.5, east)
    for bad, what in ((pts.float(), "float64"), (pts[:, :2], r"\(R, 3\)"), (pts.numpy(), "tensor"), (pts, "device")):
        with pytest.raises(ValueError, match=what):
            point_sky_view(bad, dsm, grid)
    with pytest.raises(ValueError, match="grid"):
        point_sky_view(pts, torch.zeros(5, 4), grid)
    with pytest.raises(ValueError, match="lift"):
        point_sky_view(pts, dsm, grid, lift=float("inf"))
    with pytest.raises(ValueError, match="ecef"):
        view_sky_view(torch.zeros(12, 11), torch.zeros(12), SceneFrame.ecef((6378137.0, 0.0, 0.0), 100.0), dsm, grid)
    slope, acc = torch.zeros(2, 4, 5), torch.zeros(4, 5, dtype=torch.float64)
    for args, kw, what in (((slope.double(), acc, 2), {}, "float32"), ((slope, acc.float(), 2), {}, "float64"), ((slope[:, :3], acc, 2), {}, "slope"),
                           ((slope, acc, 0), {}, "D"), ((slope, acc, 4097), {}, "D"), ((slope, acc, 2), dict(cells=(3, 2)), "cells"),
                           ((slope, acc, 2), dict(cells=(0, 21)), "cells"), ((slope, acc, 2), dict(last=False, svf=torch.zeros(4, 5)), "last"),
                           ((slope, acc, 2), dict(svf=torch.zeros(4, 4)), "svf"), ((slope, acc, 2), dict(sums=torch.zeros(3)), "int64"),
                           ((slope, acc, 2), {}, "device")):
        with pytest.raises(ValueError, match=what):
            Fn.sky_view(*args, **kw)
    assert math.isnan(Fn.fixed_mean(0, 0, 1 << 30))
