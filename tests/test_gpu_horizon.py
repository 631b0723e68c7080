"""bn_grid_horizon, bn_points_horizon and bn_sky_view against the numpy statement of tests/horizon_cases.py: slope as float32 bits,
hit, acc as float64 bits, svf and sums, on every grid shape, azimuth family, special cell, launch and tile split, band split and
refusal; then the agreement with the shadow march, the wrappers and two ranks.  (A NaN is a NaN whatever its payload.)"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import horizon_cases as Hc
from test_gpu_parity import DEV, _free_port

pytestmark = pytest.mark.gpu

npy = lambda t: None if t is None else t.detach().cpu().numpy()
bits = lambda a: a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(g, w, what=""):
    """Bit for bit: floats by their bits (NaN where NaN), integers by value."""
    assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, g.shape, w.dtype, w.shape)
    if g.dtype.kind == "f":
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, "NaN", int((np.isnan(g) != np.isnan(w)).sum()))
        k = ~np.isnan(w)
        assert np.array_equal(bits(g)[k], bits(w)[k]), (what, int((bits(g)[k] != bits(w)[k]).sum()))
    else:
        assert np.array_equal(g, w), (what, int((g != w).sum()))


def check(got, want, what=""):
    for g, w, name in zip(got, want, ("slope", "hit")):
        same(g, w, f"{what} {name}")


def run_grid(dsm, az, max_steps=None, zmax=Hc.INF, **kw):
    from brdf_nerf_amd import functions as Fn
    slope, hit = Fn.grid_horizon(dev(dsm), Hc.RES, torch.from_numpy(np.asarray(az, dtype=np.float64)), max_steps, zmax, want_hit=True, **kw)
    return npy(slope), npy(hit)


def run_points(pts, dsm, xoff, yoff, res, az, max_steps=None, zmax=Hc.INF, want_hit=True):
    from brdf_nerf_amd import functions as Fn
    slope, hit = Fn.points_horizon(dev(pts), dev(dsm), xoff, yoff, res, torch.from_numpy(np.asarray(az, dtype=np.float64)), max_steps, zmax,
                                   want_hit=want_hit)
    return npy(slope), npy(hit)


def run_sky(slope, tile=None):
    """The sky view of a (D, ...) table in tiles of `tile` planes (None: all D at once) -> acc, svf, sums."""
    from brdf_nerf_amd import functions as Fn
    s = dev(slope)
    D = s.shape[0]
    step = D if tile is None else tile
    acc = torch.zeros(s.shape[1:], dtype=torch.float64, device=DEV)
    svf = sums = None
    for k0 in range(0, D, step):
        k1 = min(D, k0 + step)
        _, svf, sums = Fn.sky_view(s[k0:k1], acc, D, last=k1 == D)
    return npy(acc), npy(svf), npy(sums)


def check_sky(got, want, what=""):
    for g, w, name in zip(got, want, ("acc", "svf", "sums")[-len(got):]):        # (acc, svf, sums), or (svf, sums) of a wrapper
        same(g, w, f"{what} {name}")


@functools.lru_cache(maxsize=None)
def grid_reference(shape):
    """The grid of a shape, the statement under all azimuths (zmax = inf: the plain rule) and its sky view, computed once."""
    dsm = Hc.grid_case(shape)
    az = Hc.all_azimuths()
    want = Hc.grid_statement(dsm, Hc.RES, az)
    return dsm, az, want, Hc.sky_statement(want[0])


@pytest.mark.parametrize("shape", Hc.GRID_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_grid_bit_equal_to_the_statement(shape):
    """Every azimuth family at once (D = 26), then D = 1, 3 and 8 of them, with zmax = +inf and with the computed maximum; the sky
    view of the device's own table."""
    dsm, az, want, sky = grid_reference(shape)
    zmax = Hc.grid_zmax(dsm)
    got = run_grid(dsm, az)
    check(got, want, "all, inf")
    check(run_grid(dsm, az, zmax=zmax), want, "all, zmax")
    for ks in ([8], [0, 5, 25], list(range(4, 12))):
        check(run_grid(dsm, az[ks], zmax=zmax), (want[0][ks], want[1][ks]), f"D={len(ks)}")
    check_sky(run_sky(got[0]), sky)
    if shape[0] * shape[1] >= 8:
        assert (want[0] > 0).any() and (want[0] == 0).any()               # a condition on the inputs: both kinds of horizon occur


def test_launches_max_steps_and_tiles_change_no_bit():
    """D = 70 on 7 x 9 is two launches (64 azimuths travel with one); max_steps 1, 3 and max(W, H); dir_tile 1, 3 and D."""
    dsm = Hc.grid_case((7, 9))
    az = Hc.azimuths(70, 3.0)
    want = Hc.grid_statement(dsm, Hc.RES, az)
    got = run_grid(dsm, az, zmax=Hc.grid_zmax(dsm))
    check(got, want, "D=70")
    pts = Hc.point_case(65, dsm, 0.0, 0.0, Hc.RES)
    check(run_points(pts, dsm, 0.0, 0.0, Hc.RES, az), Hc.points_statement(pts, dsm, 0.0, 0.0, Hc.RES, az), "D=70 points")
    sky = Hc.sky_statement(want[0])
    for tile in (1, 3, None, 64):
        check_sky(run_sky(got[0], tile), sky, f"tile={tile}")
    dsm, az, whole, sky = grid_reference((33, 65))
    for steps in (1, 3, 65, 1 << 30):
        ref = Hc.grid_statement(dsm, Hc.RES, az, max_steps=steps)
        check(run_grid(dsm, az, steps, Hc.grid_zmax(dsm)), ref, f"max_steps={steps}")
        assert (steps >= 65) == all(a.tobytes() == b.tobytes() for a, b in zip(ref, whole))      # a bound below the side is felt
    for tile in (1, 3):
        check_sky(run_sky(whole[0], tile), sky, f"tile={tile}")


def test_special_grids_and_cells():
    """An all-NaN grid is all NaN with sums (0, 0, H W); a flat one has every slope 0 and every svf exactly 1; +inf makes an infinite
    slope that adds exactly 0, -inf and NaN cells never raise a horizon, -0.0 is 0, 1e30 stays finite in float32."""
    az = Hc.all_azimuths()
    nan_grid, flat = np.full((5, 70), np.nan, dtype=np.float32), np.full((9, 13), -3.0, dtype=np.float32)
    for dsm in (nan_grid, flat, np.zeros((3, 3), dtype=np.float32)):
        want = Hc.grid_statement(dsm, Hc.RES, az)
        got = run_grid(dsm, az, zmax=Hc.grid_zmax(dsm))
        check(got, want)
        check(run_grid(dsm, az), want)
        check_sky(run_sky(got[0]), Hc.sky_statement(want[0]))
    acc, svf, sums = run_sky(run_grid(nan_grid, az, zmax=-Hc.INF)[0])
    assert np.isnan(svf).all() and sums.tolist() == [0, 0, 350]
    slope, hit = run_grid(flat, az)
    acc, svf, sums = run_sky(slope)
    assert (slope == 0).all() and (hit == -1).all() and (svf == 1.0).all() and sums.tolist() == [117 << 30, 117, 0]
    row = np.array([[1.0, -0.0, np.nan, -np.inf, 5.0, np.inf, 2.0, 1e30, 3.0]], dtype=np.float32)
    want = Hc.grid_statement(row, Hc.RES, Hc.CARDINALS)
    assert np.isinf(want[0][1, 0, [0, 1, 4]]).all() and want[1][1, 0, :2].tolist() == [5, 5]           # east: the +inf cell
    assert np.isnan(want[0][:, 0, [2, 3, 5]]).all() and want[0][3, 0, 4] == 0      # west of the 5.0 cell: -inf, NaN, -0.0, 1.0
    assert np.isfinite(want[0][1, 0, 6]) and want[0][1, 0, 6] > 1e30
    for zmax in (Hc.INF, Hc.grid_zmax(row)):
        got = run_grid(row, Hc.CARDINALS, zmax=zmax)
        check(got, want, f"specials zmax={zmax}")
    sky = Hc.sky_statement(want[0])
    assert sky[1][0, 0] == 0.75 and sky[2].tolist()[1:] == [6, 3]
    check_sky(run_sky(got[0]), sky)


def test_the_tie_row_and_the_closed_form_row():
    slope, hit = run_grid(Hc.tie_row(), [[1.0, 0.0]])
    assert slope[0, 0, 0] == 2.0 and hit[0, 0, 0] == 1                      # three cells at exactly 2.0: the first keeps the hit
    check((slope, hit), Hc.grid_statement(Hc.tie_row(), Hc.RES, [[1.0, 0.0]]))
    pts = np.array([[0.25, -0.25, 10.0]])
    got = run_points(pts, Hc.tie_row(), 0.0, 0.0, Hc.RES, [[1.0, 0.0]])
    assert got[0][0, 0] == 2.0 and got[1][0, 0] == 1
    slope, hit = run_grid(Hc.closed_row(), Hc.CARDINALS, zmax=12.0)
    assert np.array_equal(slope[1, 0], np.array(Hc.CLOSED_EAST, dtype=np.float32)) and np.array_equal(slope[3, 0], slope[1, 0][::-1])
    assert (slope[[0, 2]] == 0).all() and hit[1, 0].tolist() == [4, 4, 4, 4, -1, -1, -1, -1, -1]
    check((slope, hit), Hc.grid_statement(Hc.closed_row(), Hc.RES, Hc.CARDINALS))
    acc, svf, sums = run_sky(slope)
    assert svf[0, 0] == 0.875 and svf[0, 2] == np.float32(0.8) and svf[0, 4] == 1.0 and np.array_equal(svf[0], svf[0][::-1])
    check_sky((acc, svf, sums), Hc.sky_statement(slope))


@pytest.mark.parametrize("cut", [None, 1, 13])
def test_row_bands_concatenate_to_the_whole(cut):
    """Bands (whole; (0, 1) + (1, H); 13 + 20 rows) written into one pre-filled buffer: the bands' rows are the whole result and
    the rows a call does not own keep their bytes; an empty band writes nothing.  The same for bn_sky_view's [c0, c1)."""
    from brdf_nerf_amd import functions as Fn
    dsm, az, want, sky = grid_reference((33, 65))
    H, W = dsm.shape
    D = len(az)
    d, t = dev(dsm), torch.from_numpy(az)
    slope = torch.full((D, H, W), -77.0, dtype=torch.float32, device=DEV)
    hit = torch.full((D, H, W), -7, dtype=torch.int32, device=DEV)
    acc = torch.zeros((H, W), dtype=torch.float64, device=DEV)
    svf = torch.full((H, W), -77.0, dtype=torch.float32, device=DEV)
    sums = torch.zeros((3,), dtype=torch.int64, device=DEV)
    bands = [(0, H)] if cut is None else [(0, cut), (cut, H)]
    for n, (a, b) in enumerate(bands):
        Fn.grid_horizon(d, Hc.RES, t, None, Hc.grid_zmax(dsm), rows=(a, b), slope=slope, hit=hit)
        Fn.sky_view(slope, acc, D, cells=(a * W, b * W), svf=svf, sums=sums)
        if n == 0 and b < H:
            assert (slope[:, b:] == -77.0).all() and (hit[:, b:] == -7).all() and (svf[b:] == -77.0).all() and (acc[b:] == 0).all()
            check((npy(slope[:, :b]), npy(hit[:, :b])), (want[0][:, :b], want[1][:, :b]), "first band")
            check_sky((npy(acc[:b]), npy(svf[:b]), npy(sums)), Hc.sky_statement(want[0][:, :b]), "first band")
    check((npy(slope), npy(hit)), want)
    check_sky((npy(acc), npy(svf), npy(sums)), sky)
    before = (slope.clone(), acc.clone(), svf.clone(), sums.clone())
    Fn.grid_horizon(d, Hc.RES, t, rows=(5, 5), slope=slope, hit=hit)          # an empty band and an empty range write nothing
    Fn.sky_view(slope, acc, D, cells=(70, 70), svf=svf, sums=sums)
    for a, b in zip(before, (slope, acc, svf, sums)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


GRIDS = {"dyadic": (4.0e5, 3.3e6 + 0.5, 0.5), "utm": (4.0e5 + 0.7, 3.3e6 + 0.4, 0.3)}


@pytest.mark.parametrize("R", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("origin", sorted(GRIDS))
def test_points_bit_equal_to_the_statement(R, origin):
    """Points inside, outside, on cell edges and corners, NaN and inf ones, at UTM-sized coordinates (easting 4.0e5, northing
    3.3e6), on a dyadic and on a non-dyadic origin and resolution."""
    xoff, yoff, res = GRIDS[origin]
    dsm = Hc.grid_case((33, 65))
    az = Hc.all_azimuths()
    pts = Hc.point_case(R, dsm, xoff, yoff, res)
    want = Hc.points_statement(pts, dsm, xoff, yoff, res, az)
    if R >= 63:
        assert np.isnan(want[0]).any() and (want[0] > 0).any() and (want[0] == 0).any()
    got = run_points(pts, dsm, xoff, yoff, res, az)
    check(got, want)
    check(run_points(pts, dsm, xoff, yoff, res, az, zmax=Hc.grid_zmax(dsm)), want, "zmax")
    check(run_points(pts, dsm, xoff, yoff, res, az, 3, Hc.grid_zmax(dsm)), Hc.points_statement(pts, dsm, xoff, yoff, res, az, 3), "3 steps")
    slope, hit = run_points(pts, dsm, xoff, yoff, res, az[[9]], want_hit=False)
    assert hit is None
    same(slope, want[0][[9]])
    check_sky(run_sky(got[0], 8), Hc.sky_statement(want[0]))


def test_grid_mode_is_point_mode_on_the_cell_centres_and_lift():
    from brdf_nerf_amd import Grid, point_sky_view, sky_view_factor
    xoff, yoff, res = GRIDS["dyadic"]
    dsm, az, want, sky = grid_reference((33, 65))
    assert res == Hc.RES
    D = len(az)
    grid = Grid(xoff, yoff, res, 65, 33)
    centres = Hc.cell_centres(dsm, xoff, yoff, res)
    got = point_sky_view(dev(centres), dev(dsm), grid, az=az, want_slope=True, dir_tile=5)
    assert set(got) == {"svf", "mean", "sums", "n_az", "slope"} and got["n_az"] == D and not got["sums"].is_cuda
    same(npy(got["slope"]), want[0].reshape(D, -1))
    check_sky((npy(got["svf"]), npy(got["sums"])), (sky[1].reshape(-1), sky[2]))
    whole = sky_view_factor(dev(dsm), res, az=az)
    assert torch.equal(whole["svf"].reshape(-1).view(torch.int32), got["svf"].view(torch.int32)) and torch.equal(whole["sums"], got["sums"])
    lifted = centres.copy()
    lifted[:, 2] = lifted[:, 2] + 0.75
    ref = Hc.sky_statement(Hc.points_statement(lifted, dsm, xoff, yoff, res, az)[0])
    up = point_sky_view(dev(centres), dev(dsm), grid, az=az, lift=0.75)
    check_sky((npy(up["svf"]), npy(up["sums"])), ref[1:])
    data = ~np.isnan(sky[1].reshape(-1))
    assert (ref[1][data] >= sky[1].reshape(-1)[data]).all() and (ref[1][data] > sky[1].reshape(-1)[data]).any()
    empty = point_sky_view(torch.zeros((0, 3), dtype=torch.float64, device=DEV), dev(dsm), grid, n_az=4)
    assert empty["svf"].shape == (0,) and empty["sums"].tolist() == [0, 0, 0] and empty["mean"] != empty["mean"]


def test_refusals():
    """BN_EINVAL through the raw ABI, nothing launched, every buffer as it was."""
    from brdf_nerf_amd import _lib as L
    lib = L.lib()
    H, W, D, R = 7, 9, 2, 5
    dsm = dev(Hc.grid_case((H, W)))
    slope = torch.full((D, H, W), -77.0, dtype=torch.float32, device=DEV)
    hit = torch.full((D, H, W), -7, dtype=torch.int32, device=DEV)
    acc = torch.full((H * W,), 0.5, dtype=torch.float64, device=DEV)
    svf = torch.full((H * W,), -77.0, dtype=torch.float32, device=DEV)
    sums = torch.full((3,), -5, dtype=torch.int64, device=DEV)
    enz = dev(Hc.point_case(R, npy(dsm), 0.0, 0.0, Hc.RES))
    p = lambda t: C.c_void_p(t.data_ptr())
    nan, inf = float("nan"), float("inf")

    def arr(rows):
        return (C.c_double * (2 * len(rows)))(*[v for r in rows for v in r])

    good = [(0.3, 0.2), (-1.0, 0.0)]
    bad_az = [[(0.3, 0.2), (0.0, 0.0)], [(-0.0, 0.0), good[1]], [(nan, 0.2), good[1]], [good[0], (0.3, inf)], [good[0], (-inf, 0.0)]]

    def grid(s=p(dsm), H=H, W=W, res=Hc.RES, row0=0, row1=H, a=arr(good), D=D, steps=9, zmax=inf, o=p(slope), h=p(hit)):
        return lib.bn_grid_horizon(s, H, W, res, row0, row1, a, D, steps, zmax, o, h, None)

    def points(e=p(enz), R=R, s=p(dsm), H=H, W=W, xoff=0.0, yoff=0.0, res=Hc.RES, a=arr(good), D=D, steps=9, zmax=inf, o=p(slope), h=p(hit)):
        return lib.bn_points_horizon(e, R, s, H, W, xoff, yoff, res, a, D, steps, zmax, o, h, None)

    def sky(s=p(slope), n=D, cells=H * W, c0=0, c1=H * W, a=p(acc), D=D, v=p(svf), q=p(sums)):
        return lib.bn_sky_view(s, n, cells, c0, c1, a, D, v, q, None)

    shared = [dict(s=None), dict(a=None), dict(o=None), dict(H=0), dict(W=0), dict(H=-2), dict(H=1 << 15, W=(1 << 15) + 1),
              dict(D=0), dict(D=-1), dict(D=4097), dict(res=0.0), dict(res=-0.5), dict(res=inf), dict(res=nan), dict(steps=0),
              dict(steps=-3), dict(zmax=nan)] + [dict(a=arr(b)) for b in bad_az]
    for kw in shared + [dict(row0=-1), dict(row1=H + 1), dict(row0=5, row1=4), dict(row0=H + 1, row1=H + 1)]:
        assert grid(**kw) == -1, kw
        assert b"grid_horizon" in lib.bn_last_error()
    for kw in shared + [dict(e=None), dict(R=-1), dict(R=(1 << 30) + 1), dict(xoff=nan), dict(yoff=inf), dict(xoff=-inf)]:
        assert points(**kw) == -1, kw
        assert b"points_horizon" in lib.bn_last_error()
    for kw in [dict(s=None), dict(a=None), dict(q=None), dict(n=0), dict(n=4097), dict(D=0), dict(D=4097), dict(cells=0),
               dict(cells=(1 << 30) + 1, c1=1), dict(c0=-1), dict(c1=H * W + 1), dict(c0=5, c1=4), dict(c0=H * W + 1, c1=H * W + 1)]:
        assert sky(**kw) == -1, kw
        assert b"sky_view" in lib.bn_last_error()
    assert grid(row0=3, row1=3) == 0 and points(R=0) == 0 and sky(c0=4, c1=4) == 0          # accepted, nothing launched
    torch.cuda.synchronize()
    assert (slope == -77.0).all() and (hit == -7).all() and (acc == 0.5).all() and (svf == -77.0).all() and (sums == -5).all()
    assert grid(h=None) == 0                                              # the same arguments, accepted: hit NULL
    torch.cuda.synchronize()
    want = Hc.grid_statement(npy(dsm), Hc.RES, np.array(good), max_steps=9)
    same(npy(slope), want[0])
    assert (hit == -7).all()
    assert grid() == 0
    acc.zero_()
    sums.zero_()
    assert sky(v=None, q=None) == 0                                       # not the last tile: acc alone
    torch.cuda.synchronize()
    assert (svf == -77.0).all() and (sums == 0).all()
    acc.zero_()
    assert sky() == 0
    torch.cuda.synchronize()
    check((npy(slope), npy(hit)), want)
    check_sky((npy(acc).reshape(H, W), npy(svf).reshape(H, W), npy(sums)), Hc.sky_statement(want[0]))


@pytest.mark.parametrize("shape", Hc.AGREE_GRIDS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_device_horizon_agrees_with_the_shadow_march(shape):
    """The device's slope > tan(elevation) is the shadow march's BLOCKED wherever the slope is not within 1e-6 (1 + tan) of it;
    at most 1 % of the cells with data may be that close."""
    dsm = Hc.grid_case(shape)
    dirs = np.stack([Hc.direction(el, azd) for el, azd in Hc.AGREE_DIRS])
    slope, _ = run_grid(dsm, dirs[:, :2], zmax=Hc.grid_zmax(dsm))
    for k, d in enumerate(dirs):
        compared, data, wrong = Hc.agreement(dsm, slope[k], d)
        assert data - compared <= 0.01 * data, (Hc.AGREE_DIRS[k], data - compared)
        assert wrong == 0, (Hc.AGREE_DIRS[k], wrong)


def test_wrappers_grid_horizon_and_sky_view_factor():
    """grid_horizon and sky_view_factor: zmax is computed inside; dir_tile 1, 3 and D, want_slope, max_dist and a lone band."""
    from brdf_nerf_amd import azimuths, grid_horizon, sky_view_factor
    dsm, az, want, sky = grid_reference((33, 65))
    d = dev(dsm)
    D = len(az)
    got = grid_horizon(d, Hc.RES, az.astype(np.float32).astype(np.float64), want_hit=True)
    assert set(got) == {"slope", "hit"}
    f32 = Hc.grid_statement(dsm, Hc.RES, az.astype(np.float32).astype(np.float64))
    check((npy(got["slope"]), npy(got["hit"])), f32)
    plain = grid_horizon(d, Hc.RES, torch.from_numpy(az))
    assert plain["hit"] is None
    same(npy(plain["slope"]), want[0])
    near = grid_horizon(d, Hc.RES, az, max_dist=1.6, want_hit=True)       # floor(1.6 / 0.5) = 3 cells
    check((npy(near["slope"]), npy(near["hit"])), Hc.grid_statement(dsm, Hc.RES, az, max_steps=3))
    band = grid_horizon(d, Hc.RES, az, rows=(7, 20), want_hit=True)
    check((npy(band["slope"][:, 7:20]), npy(band["hit"][:, 7:20])), (want[0][:, 7:20], want[1][:, 7:20]))
    assert torch.isnan(band["slope"][:, :7]).all() and torch.isnan(band["slope"][:, 20:]).all() and (band["hit"][:, 20:] == -1).all()
    for tile in (1, 3, D, 8):
        res = sky_view_factor(d, Hc.RES, az=az, dir_tile=tile, want_slope=tile == 3)
        assert set(res) == {"svf", "mean", "sums", "n_az"} | ({"slope"} if tile == 3 else set()) and res["n_az"] == D
        check_sky((npy(res["svf"]), npy(res["sums"])), sky[1:], f"dir_tile={tile}")
        assert res["mean"] == int(sky[2][0]) / (int(sky[2][1]) * 2 ** 30)
        if tile == 3:
            same(npy(res["slope"]), want[0])
    ring = sky_view_factor(d, Hc.RES, n_az=16, start_deg=7.0)
    assert np.array_equal(azimuths(16, 7.0).numpy(), az[5:21])
    check_sky((npy(ring["svf"]), npy(ring["sums"])), Hc.sky_statement(want[0][5:21])[1:])
    lone = sky_view_factor(d, Hc.RES, az=az, rows=(7, 20))
    part = Hc.sky_statement(want[0][:, 7:20])
    same(npy(lone["svf"][7:20]), part[1])
    assert torch.isnan(lone["svf"][:7]).all() and torch.isnan(lone["svf"][20:]).all() and np.array_equal(npy(lone["sums"]), part[2])
    block = sky_view_factor(dev(Hc.block_scene()), Hc.RES, n_az=16)
    assert tuple(block["sums"].tolist()) == Hc.BLOCK_SVF[16][1] and int((block["svf"] < 1).sum()) == Hc.BLOCK_SVF[16][0]
    assert (block["svf"][24:40, 24:40] == 1.0).all()


def test_view_sky_view_on_a_rendered_view():
    """The 12 x 10 view of test_gpu_maps.py over its own filled DSM: view_sky_view is the statement on point_cloud of the depth,
    with and without lift."""
    from brdf_nerf_amd import fill_holes, point_cloud, score_view, view_sky_view
    from test_gpu_dsm import frame
    from test_gpu_maps import CHUNK, VIEW_H, VIEW_W, view_case
    args, models, rays, fl = view_case("rpv_an")
    H, W = VIEW_H, VIEW_W
    rgbs = torch.rand(H * W, 3, generator=torch.Generator().manual_seed(11)).to(DEV)
    torch.manual_seed(31)
    plain = score_view(models, args, rays, rgbs, H, W, frame=frame(), chunk=CHUNK, **fl)
    grid = plain["grid"]
    filled = fill_holes(plain["dsm"])["filled"]
    pts = npy(point_cloud(rays, plain["depth"], frame()))
    az = Hc.azimuths(8, 7.0)
    for lift in (0.0, 0.5):
        up = pts.copy()
        up[:, 2] = up[:, 2] + lift
        ref = Hc.points_statement(up, npy(filled), grid.xoff, grid.yoff, grid.resolution, az)
        sky = Hc.sky_statement(ref[0])
        got = view_sky_view(rays, plain["depth"], frame(), filled, grid, n_az=8, start_deg=7.0, dir_tile=3, want_slope=True, lift=lift)
        assert got["svf"].shape == (H * W,)
        same(npy(got["slope"]), ref[0], f"lift={lift}")
        check_sky((npy(got["svf"]), npy(got["sums"])), sky[1:], f"lift={lift}")
        if lift == 0.0:
            assert int(sky[2][1]) > 0 and (sky[1][~np.isnan(sky[1])] < 1).any()       # a condition on the inputs: some pixel has a horizon


def test_two_rank_horizon_matches_one_rank():
    """World 2: two ranks on cuda:0 over gloo (tests/dist_horizon_worker.py), each child under its own time limit and started
    once: the gathered row bands and the summed sums are the single process's slope, hit, svf and sums, bitwise."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dist_horizon_worker.py")
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
