"""The orthophoto rule's numpy statement on its own cases, the package surface and the wrapper refusals: no GPU.

The inverse UTM has no upstream counterpart to be held to; its judge is the round trip through camera_cases.utm, the forward series
the project already holds to quadrature and to Snyder's series (tests/test_camera_cpu.py).  The bounds are derived here from 1e-6 m,
the project's bound for world coordinates, never typed in as degrees or pixels.
"""
import os
import re

import numpy as np
import pytest
import torch

import camera_cases as K
import orthophoto_cases as O
import visibility_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (site, south): all three sites, z21 - the southern one - in both settings
SETTINGS = [("z38", False), ("z17", False), ("z21", False), ("z21", True)]


@pytest.mark.parametrize("site,south", SETTINGS)
def test_round_trip_through_the_forward_series(site, south):
    zone = K.SITES[site][2]
    lons, lats, e, n = O.site_points(site, 2000, south)
    lon, lat, bad = O.utm_inverse(e, n, zone, south)
    assert not bad.any()
    e2, n2 = K.utm(lon, lat, zone, south)
    worst = float(np.max(np.hypot(e2 - e, n2 - n)))
    print(f"{site} south={south}: utm(inverse(e, n)) within {worst:.3g} m")
    assert worst <= O.WORLD_BOUND
    blon, blat = O.degree_bounds(site, south)
    dlon, dlat = float(np.max(np.abs(lon - lons))), float(np.max(np.abs(lat - lats)))
    print(f"{site} south={south}: inverse(utm(lon, lat)) within {dlon:.3g} / {dlat:.3g} degrees (bounds {blon:.3g} / {blat:.3g})")
    assert dlon <= blon and dlat <= blat
    # the bound in degrees is what 1e-6 m is at the site: some 1e-11 degrees, five orders above float64's resolution of a longitude
    assert 5e-12 < blat < 2e-11 and blat <= blon < 2e-11


@pytest.mark.parametrize("site,south", SETTINGS)
def test_newton_has_converged_on_the_inputs(site, south):
    """A condition on the inputs, not a tolerance on any code: the relative step of the fourth iteration is rounding noise."""
    _, _, e, n = O.site_points(site, 2000, south)
    steps = []
    O.utm_inverse(e, n, K.SITES[site][2], south, steps)
    print(f"{site} south={south}: relative Newton steps {['%.2g' % s for s in steps]}")
    assert len(steps) == O.NEWTON_ITERS == 4 and steps[3] <= 4 * K.ULP


def test_false_northing_and_the_central_meridian():
    """On the central meridian at the equator the point is (500000, 0) - with south, (500000, 1e7) - and comes back as (lon0, 0)."""
    for south in (False, True):
        lon, lat, bad = O.utm_inverse([500000.0], [10000000.0 if south else 0.0], 21, south)
        assert not bad.any() and lon[0] == -57.0 and lat[0] == 0.0
    lon, lat, bad = O.utm_inverse([np.nan, np.inf, 500000.0], [0.0, 0.0, np.inf], 21)
    assert bad.all() and np.isnan(lon).all() and np.isnan(lat).all()


@pytest.mark.parametrize("site,south", SETTINGS)
def test_cells_come_back_to_the_pixels_they_were_localised_from(site, south):
    zone, alt0 = K.SITES[site][2], K.SITES[site][3]
    d = K.make_rpc(site, 11)
    bound = O.pixel_bound(d, site, south)
    rng = np.random.default_rng(4)
    cols, rows = rng.uniform(0, 1023, 500), rng.uniform(0, 1023, 500)
    for alt in (alt0 - 60.0, alt0, alt0 + 90.0):
        lon, lat, bad = K.localize(d, cols, rows, alt)
        assert not bad.any()
        e, n = K.utm(lon, lat, zone, south)
        colrow, counted = O.world_pixels(d, e, n, np.full(500, alt), zone, south)
        worst = float(np.max(np.abs(colrow - np.stack([cols, rows], -1))))
        print(f"{site} south={south} alt {alt}: pixels within {worst:.3g} (bound {bound:.3g})")
        assert not counted.any() and worst <= bound
    assert 1e-7 < bound < 1e-6                  # some 0.3 pixels per metre on these fixtures


@pytest.mark.parametrize("site,south", SETTINGS)
def test_points_along_the_view_direction_project_to_one_pixel(site, south):
    zone, alt0 = K.SITES[site][2], K.SITES[site][3]
    d = K.make_rpc(site, 12)
    lo, hi = alt0 - 60.0, alt0 + 90.0
    vd = O.view_direction(d, zone, south, lo, hi)
    assert vd[2] == hi - lo
    lon, lat, _ = K.localize(d, [d["col_offset"]], [d["row_offset"]], lo)
    e, n = K.utm(lon, lat, zone, south)
    t = np.linspace(0.0, 1.0, 21)
    colrow, counted = O.world_pixels(d, e[0] + t * vd[0], n[0] + t * vd[1], lo + t * vd[2], zone, south)
    assert not counted.any()
    ends = colrow[[0, -1]] - np.array([d["col_offset"], d["row_offset"]])
    assert float(np.max(np.abs(ends))) <= O.pixel_bound(d, site, south)
    # between the ends the ray of an RPC model is not a straight line in UTM: the 16 monomials that are not linear carry synthetic
    # coefficients of up to 1e-3 in the numerator and the denominator (a real image's are some 1e-6), and |H| <= 0.75 along the
    # ray, so the pixel sags by at most 2 x 16 x 1e-3 x 0.75^2 scales.  Part of what one direction per scene neglects; printed.
    sag = float(np.max(np.abs(colrow - np.array([d["col_offset"], d["row_offset"]]))))
    print(f"{site} south={south}: between the ends the pixel sags by {sag:.3g}")
    assert sag <= 2 * 16 * 1e-3 * 0.75 ** 2 * max(d["col_scale"], d["row_scale"])


def test_bilinear_gather_of_a_linear_image_is_the_linear_function():
    for Hi, Wi in ((2, 2), (5, 7), (33, 65)):
        planes = O.linear_image(Hi, Wi, 3)
        colrow = np.concatenate([O.random_colrow(Hi, Wi, 400, seed=1), O.edge_colrow(Hi, Wi)])
        out, state, counts = O.gather(planes, colrow)
        kept = state == O.KEPT
        assert kept.sum() >= 100 and counts.sum() == len(colrow)
        for ch in range(3):
            assert O.within_one_ulp(out[ch, kept], O.linear_value(colrow[kept], ch))
        assert np.isnan(out[:, ~kept]).all()
        near, nstate, _ = O.gather(planes, np.floor(colrow), mode="nearest")          # on pixel centres nearest is the pixel itself
        k = nstate == O.KEPT
        assert np.array_equal(near[0, k], O.linear_value(np.floor(colrow)[k]))


@pytest.mark.parametrize("shape", O.EDGE_IMAGES)
def test_gather_edge_rules(shape):
    Hi, Wi = shape
    t = 2.0 ** -40
    planes = O.random_image(2, Hi, Wi, seed=7, specials=False)
    last = float(Wi - 1)
    cols = np.array([0.0, -0.0, last, -t, last + t, np.nan, np.inf, -np.inf, float(Wi // 2)])
    colrow = np.stack([cols, np.zeros_like(cols)], -1)
    state = O.gather_state(colrow, Hi, Wi)
    assert state.tolist() == [O.KEPT, O.KEPT, O.KEPT, O.OUTSIDE, O.OUTSIDE, O.NODATA, O.OUTSIDE, O.OUTSIDE, O.KEPT]
    r0, r1, c0, c1, fy, fx = O.gather_taps(colrow, Hi, Wi)
    if Wi == 1:
        assert (c0[[0, 1, 2, 8]] == 0).all() and (c1[[0, 1, 2, 8]] == 0).all() and (fx[[0, 1, 2, 8]] == 0).all()
    else:
        assert (c0[0], c1[0], fx[0]) == (0, 1, 0.0) and (c0[1], c1[1]) == (0, 1) and fx[1] == 0.0
        assert (c0[2], c1[2], fx[2]) == (Wi - 2, Wi - 1, 1.0)              # at col = Wi - 1 the taps are the last two and fx = 1
        m = Wi // 2
        assert (c0[8], c1[8], fx[8]) == ((m, m + 1, 0.0) if m <= Wi - 2 else (Wi - 2, Wi - 1, 1.0))
    assert (r0 == 0).all() and (r1 == min(1, Hi - 1)).all() and (fy == 0.0).all()
    out, _, counts = O.gather(planes, colrow)
    kept = state == O.KEPT
    at = np.where(cols[kept] == last, Wi - 1, np.floor(np.abs(cols[kept])).astype(int))
    assert np.array_equal(out[:, kept], planes[:, 0, at])                 # on a pixel centre the value is the pixel
    assert counts.tolist() == [1, 4, 0, 4]
    # the same on the rows, and occlusion after the first two tests: an occluded cell outside the image is OUTSIDE
    rowcol = colrow[:, ::-1].copy()
    assert O.gather_state(rowcol, Wi, Hi).tolist() == state.tolist()
    vis = np.full(len(cols), V.BLOCKED, dtype=np.uint8)
    assert O.gather_state(colrow, Hi, Wi, vis).tolist() == [O.OCCLUDED, O.OCCLUDED, O.OCCLUDED, O.OUTSIDE, O.OUTSIDE, O.NODATA, O.OUTSIDE,
                                                            O.OUTSIDE, O.OCCLUDED]
    vis[:] = V.NODATA
    assert (O.gather_state(colrow, Hi, Wi, vis)[[0, 1, 2, 8]] == O.OCCLUDED).all()        # anything but VISIBLE
    # nearest: the half-way point goes up, the last pixel is not left
    if Wi > 1:
        n, ns, _ = O.gather(planes, np.array([[0.5, 0.0], [last - 0.5, 0.0], [0.5 - t, 0.0]]), mode="nearest")
        assert np.array_equal(n, planes[:, 0, [1, Wi - 1, 0]])


def test_a_nan_tap_propagates_at_weight_zero_and_nearest_copies_bits():
    planes = O.random_image(1, 5, 7, seed=3, specials=False)
    planes[0, 2, 3] = np.nan
    planes[0, 0, 0], planes[0, 0, 1] = -0.0, np.float32(1e-41)
    out, state, _ = O.gather(planes, np.array([[2.0, 2.0], [3.0, 1.0], [5.0, 4.0]]))
    assert np.isnan(out[0, 0]) and np.isnan(out[0, 1]) and not np.isnan(out[0, 2])      # (2, 2) and (3, 1) have pixel (2, 3) as a tap
    near, _, _ = O.gather(planes, np.array([[0.0, 0.0], [1.0, 0.0], [3.0, 2.0]]), mode="nearest")
    assert O.same_f32(near[0], planes[0, [0, 0, 2], [0, 1, 3]], exact_nan=True)
    assert np.signbit(near[0, 0]) and near[0, 1] == np.float32(1e-41)


def test_end_to_end_scene_has_both_classes():
    """A condition on the input of the GPU end-to-end test, asserted on the statement alone."""
    d, dsm, xoff, yoff, res = O.box_scene()
    zone = K.SITES[O.SCENE_SITE][2]
    planes = O.linear_image(*O.SCENE_IMAGE)
    out, state, colrow, vis, counts = O.orthophoto(d, planes, dsm, xoff, yoff, res, zone)
    print(f"box scene: {counts}")
    assert counts["occluded"] >= 20 and counts["kept"] >= 200 and counts["skipped"] == 0
    assert counts["nodata"] == 0 and counts["outside"] == 0
    kept = state == O.KEPT
    assert O.within_one_ulp(out[0][kept], O.linear_value(colrow[kept]))
    assert np.array_equal(state == O.OCCLUDED, vis != V.VISIBLE)
    free, _, _, _, c2 = O.orthophoto(d, planes, dsm, xoff, yoff, res, zone, occlusion=False)
    assert c2["kept"] == dsm.size and not np.isnan(free).any()


def test_package_surface():
    import brdf_nerf_amd
    from brdf_nerf_amd import _lib, camera
    from brdf_nerf_amd.build import FILE_FLAGS
    for name in ("world_pixels", "grid_pixels", "sample_image", "orthophoto", "ortho_psnr"):
        assert name in brdf_nerf_amd.__all__ and callable(getattr(brdf_nerf_amd, name))
    for name in ("utm_geodetic", "view_direction"):
        assert name in camera.__all__ and callable(getattr(camera, name))
    assert "-ffp-contract=off" in FILE_FLAGS["orthophoto.hip"]
    csrc = os.path.join(ROOT, "brdf_nerf_amd", "csrc")
    for f in ("orthophoto.hip", "rpc_poly.h", "geodesy.h"):
        assert "#pragma clang fp contract(off)" in open(os.path.join(csrc, f)).read()
    src = open(os.path.join(csrc, "orthophoto.hip")).read()
    assert "atomic" not in re.sub(r"//.*", "", src)                       # the counters go out through block_sums.h
    for f in ("camera.hip", "orthophoto.hip"):
        assert '#include "rpc_poly.h"' in open(os.path.join(csrc, f)).read()          # one statement of the polynomials, shared
    assert "struct Mono" not in open(os.path.join(csrc, "camera.hip")).read()
    header = open(os.path.join(ROOT, "include", "brdfnerf_hip.h")).read()
    assert "Orthophoto of an observed image" in header
    declared = set(re.findall(r"\b(bn_[a-z0-9_]+)\s*\(", header))
    for name, nargs in (("bn_utm_geodetic", 7), ("bn_grid_pixels", 14), ("bn_image_gather", 17)):
        assert name in declared and name in _lib.exported_symbols() and len(_lib._SIGS[name][1]) == nargs, name
    assert (_lib.BN_GATHER_NODATA, _lib.BN_GATHER_OUTSIDE, _lib.BN_GATHER_OCCLUDED, _lib.BN_GATHER_KEPT) == \
        (O.NODATA, O.OUTSIDE, O.OCCLUDED, O.KEPT) == (0, 1, 2, 3)
    for name, value in (("BN_UTM_NEWTON_ITERS", O.NEWTON_ITERS), ("BN_GATHER_MAX_CHANNELS", 32)):
        assert re.search(rf"#define {name} {value}\b", header) and getattr(_lib, name) == value, name
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "## Orthophoto of an observed image" in readme and "an inverse UTM" not in readme


def test_wrapper_refusals_without_a_device():
    from brdf_nerf_amd import Grid, Rpc, camera, grid_pixels, ortho_psnr, orthophoto, sample_image, world_pixels
    rpc = Rpc.from_dict(K.make_rpc("z17", 1))
    grid = Grid(0.0, 0.0, 0.5, 5, 4)
    dsm, img = torch.zeros(4, 5), torch.zeros(6 * 7, 3)
    for bad, what in ((dsm.double(), "float32"), (dsm[:, ::2], "contiguous"), (dsm[0], "2-D"), (dsm.numpy(), "tensor"),
                      (torch.zeros(5, 4), "grid"), (dsm, "device")):
        with pytest.raises(ValueError, match=what):
            grid_pixels(bad, grid, rpc, 17)
        with pytest.raises(ValueError, match=what):
            orthophoto(img, 6, 7, rpc, bad, grid, 17)
    for zone in (0, 61, 17.5, None, True):
        with pytest.raises(ValueError, match="zone"):
            grid_pixels(dsm, grid, rpc, zone)
        with pytest.raises(ValueError, match="zone"):
            orthophoto(img, 6, 7, rpc, dsm, grid, zone)
        with pytest.raises(ValueError, match="zone"):
            world_pixels(rpc, torch.zeros(3, 3, dtype=torch.float64), zone)
        with pytest.raises(ValueError, match="zone"):
            camera.utm_geodetic(torch.zeros(3, 2, dtype=torch.float64), zone, device="cpu")
    for bad, what in ((img.double(), "float32"), (img[:, :2], "contiguous"), (img.numpy(), "tensor"), (torch.zeros(6 * 7, 33), "channels")):
        with pytest.raises(ValueError, match=what):
            orthophoto(bad, 6, 7, rpc, dsm, grid, 17)
        with pytest.raises(ValueError, match=what):
            sample_image(bad, 6, 7, torch.zeros(4, 5, 2, dtype=torch.float64))
    for hw in ((6, 8), (5, 7), (0, 7)):
        with pytest.raises(ValueError, match="pixels"):
            orthophoto(img, *hw, rpc, dsm, grid, 17)
        with pytest.raises(ValueError, match="pixels"):
            sample_image(img, *hw, torch.zeros(4, 5, 2, dtype=torch.float64))
    for vd, what in (([0.0, 0.0, float("nan")], "finite"), ([float("inf"), 0.0, 1.0], "finite"), ([0.0, 1.0, 0.0], "upwards"),
                     ([0.0, 1.0], "3 floats"), (torch.ones(3, dtype=torch.int64), "3 floats")):
        with pytest.raises(ValueError, match=what):
            orthophoto(img, 6, 7, rpc, dsm, grid, 17, view_dir=vd)
    for kw, what in ((dict(mode="cubic"), "mode"), (dict(layout="chw"), "layout"), (dict(rows=(2, 1)), "rows"), (dict(rows=(0, 5)), "rows"),
                     (dict(eps=-1.0), "eps"), (dict(alt_bounds=(5.0, 5.0)), "alt_bounds"), (dict(alt_bounds=(0.0, float("inf"))), "alt_bounds")):
        with pytest.raises(ValueError, match=what):
            orthophoto(img, 6, 7, rpc, dsm, grid, 17, **kw)
    cr = torch.zeros(4, 5, 2, dtype=torch.float64)
    for bad, what in ((cr.float(), "float64"), (torch.zeros(4, 5, 3, dtype=torch.float64), r"\(\.\.\., 2\)"), (cr, "device")):
        with pytest.raises(ValueError, match=what):
            sample_image(img, 6, 7, bad)
    with pytest.raises(ValueError, match="visible"):
        sample_image(img, 6, 7, cr, visible=torch.zeros(5, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="mode"):
        sample_image(img, 6, 7, cr, mode="cubic")
    pts = torch.zeros(3, 3, dtype=torch.float64)
    for bad, what in ((pts.float(), "float64"), (pts[:, :2], r"\(R, 3\)"), (pts.numpy(), "tensor"), (pts, "device")):
        with pytest.raises(ValueError, match=what):
            world_pixels(rpc, bad, 17)
    with pytest.raises(ValueError, match=r"\(n, 2\)"):
        camera.utm_geodetic(torch.zeros(3, 3), 17, device="cpu")
    for lo, hi in ((5.0, 5.0), (0.0, float("nan")), (10.0, 0.0)):
        with pytest.raises(ValueError, match="altitudes"):
            camera.view_direction(rpc, 17, False, lo, hi)
    with pytest.raises(ValueError, match="one grid"):
        ortho_psnr(torch.zeros(3, 4, 5), torch.zeros(3, 5, 4))
    with pytest.raises(ValueError, match="mask"):
        ortho_psnr(torch.zeros(3, 4, 5), torch.zeros(3, 4, 5), mask=torch.ones(7))
    # no kernel of its own: on the host it is image_psnr on the cells where both are finite
    a, b = torch.rand(3, 4, 5), torch.rand(3, 4, 5)
    b[:, 1, 2] = float("nan")
    a[0, 3, 3] = float("nan")
    from brdf_nerf_amd import image_psnr
    keep = torch.ones(4, 5, dtype=torch.bool)
    keep[1, 2] = keep[3, 3] = False
    psnr, n = ortho_psnr(a, b)
    assert n == 18 and psnr == image_psnr(a[:, keep].t().contiguous(), b[:, keep].t().contiguous())[0]
    assert ortho_psnr(b, b)[0] == image_psnr(torch.ones(2, 3), torch.ones(2, 3))[0] == float("inf")
