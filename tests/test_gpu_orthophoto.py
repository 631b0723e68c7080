"""GPU tests of the orthophoto of an observed image (brdf_nerf_amd/orthophoto.py; bn_utm_geodetic / bn_grid_pixels /
bn_image_gather).  Run on the MI355X box with `pytest -m gpu`.  Cases and the numpy float64 statement they are held to:
tests/orthophoto_cases.py.

The inverse UTM and the pixels pass through the device's float64 transcendentals, which are not bit-specified: they are held to
the statement within 1e-6 m - the project's bound for world coordinates - carried to degrees and to pixels by orthophoto_cases.  The
gather is fed the STATEMENT's colrow, so no transcendental lies between its inputs and its outputs, and must equal the statement bit
for bit in out, state and counts.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import camera_cases as K
import orthophoto_cases as O
import visibility_cases as V
from test_gpu_parity import DEV, _free_port

pytestmark = pytest.mark.gpu

SETTINGS = [("z38", False), ("z17", False), ("z21", False), ("z21", True)]
LAYOUTS = ("image", "planes")
MODES = ("bilinear", "nearest")


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype).copy()).to(DEV)


def npy(t):
    return t.detach().cpu().numpy()


def bits64(t):
    return t.contiguous().view(torch.int64)


def rpc_of(d):
    from brdf_nerf_amd import Rpc
    return Rpc.from_dict(d)


def site_relief(site, H, W, seed=0):
    """A relief around the site's altitude with NaN cells and, from 8 cells on, one +inf, one -inf and one -0.0 cell."""
    alt = K.SITES[site][3]
    if H * W < 8:
        return V.relief(H, W, seed=seed, nan=0.0, specials=False, low=alt - 20.0)
    return V.relief(H, W, seed=seed, nan=0.1, low=alt - 20.0)


# ------------------------------------------------------------------------------------------------ bn_utm_geodetic
@pytest.mark.parametrize("n", O.GEODETIC_N)
def test_utm_geodetic_within_the_bound_of_the_statement(n):
    from brdf_nerf_amd import camera
    for site, south in SETTINGS:
        zone = K.SITES[site][2]
        _, _, e, nn = O.site_points(site, n, south)
        en = np.stack([e, nn], -1)
        if n >= 63:
            en[5, 0], en[17, 1], en[40, 0], en[41, 1] = np.nan, np.nan, np.inf, -np.inf
        lon, lat, bad = O.utm_inverse(en[:, 0], en[:, 1], zone, south)
        lonlat, skipped = camera.utm_geodetic(dev(en), zone, south)
        got = npy(lonlat)
        assert skipped == int(bad.sum()) == (4 if n >= 63 else 0)
        assert np.array_equal(np.isnan(got), np.stack([bad, bad], -1))
        blon, blat = O.degree_bounds(site, south)
        dlon, dlat = np.abs(got[~bad, 0] - lon[~bad]).max(), np.abs(got[~bad, 1] - lat[~bad]).max()
        print(f"{site} south={south} n={n}: within {dlon:.3g} / {dlat:.3g} degrees (bounds {blon:.3g} / {blat:.3g})")
        assert dlon <= blon and dlat <= blat


# ------------------------------------------------------------------------------------------------ bn_grid_pixels
@pytest.mark.parametrize("site,south", SETTINGS)
@pytest.mark.parametrize("shape", O.PIXEL_GRIDS)
def test_grid_pixels(shape, site, south):
    """Within the bound of the statement; bit for bit the two-launch chain on the same cell centres; the same from every row
    split; counts[0] the statement's."""
    from brdf_nerf_amd import functions as Fn
    from brdf_nerf_amd import world_pixels
    H, W = shape
    zone, res = K.SITES[site][2], 0.5
    d = K.make_rpc(site, 21)
    rpc = rpc_of(d)
    dsm = site_relief(site, H, W, seed=H + W)
    xoff, yoff = O.site_grid(site, H, W, res, south, shift=(137.0, -61.0))
    want, bad = O.grid_pixels(d, dsm, xoff, yoff, res, zone, south)
    colrow, counts = Fn.grid_pixels(rpc, dev(dsm), xoff, yoff, res, zone, south)
    got = npy(colrow)
    assert int(counts.item()) == int(bad.sum())
    assert np.array_equal(np.isnan(got), np.stack([bad, bad], -1))
    if H * W >= 8:
        assert bad.sum() >= 2 and (~bad).sum() >= 8          # NaN and infinite cells are there, and so are cells with a pixel
    bound = O.pixel_bound(d, site, south)
    worst = np.abs(got[~bad] - want[~bad]).max()
    print(f"{site} south={south} {H} x {W}: within {worst:.3g} pixels (bound {bound:.3g})")
    assert worst <= bound
    # the two-launch chain: bn_utm_geodetic, then bn_rpc_project, on the statement's cell centres (the same float64 operations)
    e, n = O.cell_centres(H, W, xoff, yoff, res)
    pts = np.stack([e.ravel(), n.ravel(), dsm.astype(np.float64).ravel()], -1)
    chain, skipped = world_pixels(rpc, dev(pts), zone, south)
    assert skipped == int(bad.sum())
    assert torch.equal(bits64(chain), bits64(colrow.reshape(-1, 2)))
    # row bands into one pre-filled buffer: every split gives the whole, the counts add up, untouched rows keep their bytes
    cuts = sorted({min(c, H) for c in O.ROW_SPLITS} | {H})
    buf = torch.full((H, W, 2), -7.0, dtype=torch.float64, device=DEV)
    total = torch.zeros(1, dtype=torch.int64, device=DEV)
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        assert (buf[r0:] == -7.0).all()
        Fn.grid_pixels(rpc, dev(dsm), xoff, yoff, res, zone, south, rows=(r0, r1), colrow=buf, counts=total)
        assert (buf[r1:] == -7.0).all()
    assert torch.equal(bits64(buf), bits64(colrow)) and int(total.item()) == int(bad.sum())


# ------------------------------------------------------------------------------------------------ bn_image_gather
def run_gather(planes, colrow, vis, mode, layout, cells=None, out=None, state=None, counts=None):
    from brdf_nerf_amd import functions as Fn
    Cn, Hi, Wi = planes.shape
    strides = (Wi * Cn, Cn, 1) if layout == "image" else (Wi, 1, Hi * Wi)
    return Fn.image_gather(dev(O.to_layout(planes, layout)), Hi, Wi, Cn, strides, dev(colrow), None if vis is None else dev(vis),
                           cells=cells, mode=mode, out=out, state=state, counts=counts)


def check_gather(planes, colrow, vis, what):
    n = len(colrow)
    for mode in MODES:
        want, wstate, wcounts = O.gather(planes, colrow, vis, mode)
        for layout in LAYOUTS:
            out, state, counts = run_gather(planes, colrow, vis, mode, layout)
            where = f"{what} {mode} {layout}"
            assert np.array_equal(npy(state), wstate), where
            assert npy(counts).tolist() == wcounts.tolist() and int(counts.sum()) == n, where
            assert O.same_f32(npy(out).reshape(want.shape), want, exact_nan=mode == "nearest"), where


@pytest.mark.parametrize("shape", O.EDGE_IMAGES)
def test_gather_edge_cases_bit_equal_to_the_statement(shape):
    Hi, Wi = shape
    colrow = O.edge_colrow(Hi, Wi)
    state = O.gather_state(colrow, Hi, Wi)
    assert all((state == s).any() for s in (O.NODATA, O.OUTSIDE, O.KEPT))
    rng = np.random.default_rng(Hi * 10 + Wi)
    vis = rng.integers(0, 3, len(colrow)).astype(np.uint8)
    for Cn in (1, 3):
        planes = O.random_image(Cn, Hi, Wi, seed=2)
        check_gather(planes, colrow, None, f"{Hi} x {Wi} C={Cn}")
        check_gather(planes, colrow, vis, f"{Hi} x {Wi} C={Cn} vis")


@pytest.mark.parametrize("Cn", O.GATHER_CHANNELS)
@pytest.mark.parametrize("shape", O.GATHER_IMAGES)
def test_gather_bit_equal_to_the_statement(shape, Cn):
    """Random and edge coordinates over images with NaN, payload-NaN, -0.0, denormal and infinite pixels, with and without vis."""
    Hi, Wi = shape
    planes = O.random_image(Cn, Hi, Wi, seed=5)
    colrow = np.concatenate([O.random_colrow(Hi, Wi, 321, seed=Cn), O.edge_colrow(Hi, Wi)])
    vis = np.random.default_rng(Cn + Hi).integers(0, 3, len(colrow)).astype(np.uint8)
    check_gather(planes, colrow, None, f"{Hi} x {Wi} C={Cn}")
    check_gather(planes, colrow, vis, f"{Hi} x {Wi} C={Cn} vis")
    _, state, _ = O.gather(planes, colrow, vis)
    assert all((state == s).any() for s in (O.NODATA, O.OUTSIDE, O.OCCLUDED, O.KEPT))


def test_gather_of_a_linear_image_and_cell_ranges():
    """The bilinear gather of v = alpha col + beta row + gamma is that function within one float32 ulp; cell ranges cut at 0, 1,
    64 and n into pre-filled buffers give the whole, the counts add up, the cells outside a range keep their bytes."""
    Hi, Wi, Cn = 33, 65, 3
    planes = O.linear_image(Hi, Wi, Cn)
    colrow = np.concatenate([O.random_colrow(Hi, Wi, 200, seed=9), O.edge_colrow(Hi, Wi)])
    n = len(colrow)
    vis = np.random.default_rng(1).integers(0, 3, n).astype(np.uint8)
    for layout in LAYOUTS:
        out, state, _ = run_gather(planes, colrow, None, "bilinear", layout)
        kept = npy(state) == O.KEPT
        assert kept.sum() >= 100
        for ch in range(Cn):
            assert O.within_one_ulp(npy(out)[ch, kept], O.linear_value(colrow[kept], ch))
    for mode in MODES:
        whole, wstate, wcounts = run_gather(planes, colrow, vis, mode, "image")
        out = torch.full((Cn, n), -3.0, dtype=torch.float32, device=DEV)
        state = torch.full((n,), 0xAB, dtype=torch.uint8, device=DEV)
        counts = torch.zeros(4, dtype=torch.int64, device=DEV)
        cuts = list(O.CELL_CUTS) + [n]
        for n0, n1 in zip(cuts[:-1], cuts[1:]):
            assert (state[n0:] == 0xAB).all() and (out[:, n0:] == -3.0).all()
            run_gather(planes, colrow, vis, mode, "image", cells=(n0, n1), out=out, state=state, counts=counts)
            assert (state[n1:] == 0xAB).all() and (out[:, n1:] == -3.0).all()
        assert torch.equal(out.view(torch.int32), whole.view(torch.int32)) and torch.equal(state, wstate) and torch.equal(counts, wcounts)


# ------------------------------------------------------------------------------------------------ end to end
def test_orthophoto_of_the_box_scene():
    """A 48 x 40 flat DSM with a tall box under a tilted RPC: the orthophoto of the linear image is the linear function of the
    returned pixels on the kept cells, `state` is the statement's composed from the visibility statement, both classes are there
    (asserted on the statement alone), ortho_psnr of the orthophoto against itself is image_psnr's identity value."""
    from brdf_nerf_amd import Grid, grid_pixels, image_psnr, ortho_psnr, orthophoto, sample_image
    d, dsm, xoff, yoff, res = O.box_scene()
    zone = K.SITES[O.SCENE_SITE][2]
    H, W = dsm.shape
    Hi, Wi = O.SCENE_IMAGE
    planes = O.linear_image(Hi, Wi, 3)
    lo, hi = float(dsm.min()), float(dsm.max())
    vd = O.view_direction(d, zone, False, lo, hi)
    _, wstate, wcolrow, wvis, wcounts = O.orthophoto(d, planes, dsm, xoff, yoff, res, zone, view_dir=vd)
    assert wcounts["occluded"] >= 20 and wcounts["kept"] >= 200              # a condition on the input
    rpc, grid = rpc_of(d), Grid(xoff, yoff, res, W, H)
    image, ddsm = dev(O.to_layout(planes, "image")), dev(dsm)
    res1 = orthophoto(image, Hi, Wi, rpc, ddsm, grid, zone, view_dir=vd)
    state, colrow = npy(res1["state"]), npy(res1["colrow"])
    assert res1["ortho"].shape == (3, H, W) and np.array_equal(state, wstate) and res1["counts"] == wcounts
    assert np.array_equal(npy(res1["visible"]), wvis)
    assert np.abs(colrow - wcolrow).max() <= O.pixel_bound(d, O.SCENE_SITE)
    kept = state == O.KEPT
    for ch in range(3):
        assert O.within_one_ulp(npy(res1["ortho"])[ch][kept], O.linear_value(colrow[kept], ch))
    assert np.isnan(npy(res1["ortho"])[:, ~kept]).all()
    # the default direction: view_direction between the lowest and the highest cell, each point held to 1e-6 m
    res2 = orthophoto(image, Hi, Wi, rpc, ddsm, grid, zone)
    assert np.abs(res2["view_dir"].numpy() - vd).max() <= 2 * O.WORLD_BOUND and res2["view_dir"][2] == hi - lo
    assert torch.equal(bits64(res2["colrow"]), bits64(res1["colrow"]))
    # the pieces: grid_pixels, then sample_image with the mask, are the whole; the planes layout and no occlusion
    assert torch.equal(bits64(grid_pixels(ddsm, grid, rpc, zone)), bits64(res1["colrow"]))
    piece = sample_image(image, Hi, Wi, res1["colrow"], visible=res1["visible"])
    assert torch.equal(piece["ortho"].view(torch.int32), res1["ortho"].view(torch.int32)) and torch.equal(piece["state"], res1["state"])
    res3 = orthophoto(dev(planes), Hi, Wi, rpc, ddsm, grid, zone, occlusion=False, layout="planes", mode="nearest")
    assert res3["visible"] is None and res3["view_dir"] is None and res3["counts"]["kept"] == H * W
    want, _, _ = O.gather(planes, wcolrow, None, "nearest")
    agree = npy(res3["ortho"]).reshape(3, -1) == want
    assert agree.mean() > 0.99          # (a pixel 1e-9 beside a half-way point may fall either way)
    # a band without a group: the other rows are NODATA and NaN and are not counted
    res4 = orthophoto(image, Hi, Wi, rpc, ddsm, grid, zone, view_dir=vd, rows=(10, 31))
    assert torch.equal(res4["ortho"][:, 10:31].view(torch.int32), res1["ortho"][:, 10:31].view(torch.int32))
    assert torch.isnan(res4["ortho"][:, :10]).all() and torch.isnan(res4["ortho"][:, 31:]).all()
    assert (res4["state"][:10] == O.NODATA).all() and torch.equal(res4["state"][10:31], res1["state"][10:31])
    assert sum(res4["counts"][k] for k in ("nodata", "outside", "occluded", "kept")) == 21 * W
    psnr, n = ortho_psnr(res1["ortho"], res1["ortho"])
    assert n == int(kept.sum()) and psnr == image_psnr(torch.ones(2, 3), torch.ones(2, 3))[0]


def test_two_rank_orthophoto_matches_one_rank():
    """World 2: two ranks on cuda:0 over gloo (tests/dist_orthophoto_worker.py), each child under its own time limit and started
    once: the gathered row bands and the summed counts are the single process's ortho, state and counts, bitwise."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dist_orthophoto_worker.py")
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
    H, W, Hi, Wi, Cn, n = 7, 9, 5, 6, 3, 11
    site, zone = "z17", 17
    d = K.make_rpc(site, 2)
    rpc = rpc_of(d)
    xoff, yoff = O.site_grid(site, H, W)
    dsm = dev(site_relief(site, H, W))
    en = dev(np.stack(O.site_points(site, n)[2:], -1))
    lonlat = torch.full((n, 2), -7.0, dtype=torch.float64, device=DEV)
    colrow = torch.full((H, W, 2), -7.0, dtype=torch.float64, device=DEV)
    counts = torch.full((4,), -5, dtype=torch.int64, device=DEV)
    img = dev(O.random_image(Cn, Hi, Wi))
    cr = dev(O.random_colrow(Hi, Wi, n))
    vis = torch.ones(n, dtype=torch.uint8, device=DEV)
    out = torch.full((Cn, n), -3.0, dtype=torch.float32, device=DEV)
    state = torch.full((n,), 0xAB, dtype=torch.uint8, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    nan, inf = float("nan"), float("inf")

    def geodetic(e=p(en), n=n, zone=zone, south=0, ll=p(lonlat), c=p(counts)):
        return lib.bn_utm_geodetic(e, n, zone, south, ll, c, None)

    def pixels(r=rpc.ref(), s=p(dsm), H=H, W=W, xoff=xoff, yoff=yoff, res=0.5, row0=0, row1=H, zone=zone, south=0, cr=p(colrow), c=p(counts)):
        return lib.bn_grid_pixels(r, s, H, W, xoff, yoff, res, row0, row1, zone, south, cr, c, None)

    def gather(i=p(img), Hi=Hi, Wi=Wi, Cn=Cn, s_row=Wi, s_col=1, s_chan=Hi * Wi, cr=p(cr), v=p(vis), n0=0, n1=n, mode=0, o=p(out), ocs=n,
               st=p(state), c=p(counts)):
        return lib.bn_image_gather(i, Hi, Wi, Cn, s_row, s_col, s_chan, cr, v, n0, n1, mode, o, ocs, st, c, None)

    zones = [dict(zone=0), dict(zone=61), dict(zone=-1), dict(south=2), dict(south=-1)]
    for kw in zones + [dict(e=None), dict(ll=None), dict(c=None), dict(n=-1), dict(n=(1 << 30) + 1)]:
        assert geodetic(**kw) == -1, kw
        assert b"utm_geodetic" in lib.bn_last_error()
    flat = L.Rpc.from_buffer_copy(rpc.struct)
    flat.col_scale = 0.0
    bent = L.Rpc.from_buffer_copy(rpc.struct)
    bent.row_num[7] = nan
    for kw in zones + [dict(r=None), dict(s=None), dict(cr=None), dict(c=None), dict(H=0), dict(W=0), dict(H=-2), dict(H=1 << 15, W=(1 << 15) + 1),
                       dict(row0=-1), dict(row1=H + 1), dict(row0=5, row1=4), dict(res=0.0), dict(res=-0.5), dict(res=inf), dict(res=nan),
                       dict(xoff=nan), dict(yoff=inf), dict(r=C.byref(flat)), dict(r=C.byref(bent))]:
        assert pixels(**kw) == -1, kw
        assert b"grid_pixels" in lib.bn_last_error()
    for kw in [dict(i=None), dict(cr=None), dict(o=None), dict(st=None), dict(c=None), dict(Cn=0), dict(Cn=33), dict(Cn=-1), dict(Hi=0), dict(Wi=0),
               dict(Hi=-3), dict(s_row=-1), dict(s_col=-1), dict(s_chan=-1), dict(ocs=-1), dict(n0=5, n1=4), dict(n0=-1), dict(mode=2),
               dict(mode=-1), dict(n1=(1 << 30) + 1)]:
        assert gather(**kw) == -1, kw
        assert b"image_gather" in lib.bn_last_error()
    assert geodetic(n=0) == 0 and pixels(row0=3, row1=3) == 0 and gather(n0=4, n1=4) == 0          # accepted, nothing launched
    torch.cuda.synchronize()
    assert (lonlat == -7.0).all() and (colrow == -7.0).all() and (counts == -5).all() and (out == -3.0).all() and (state == 0xAB).all()
    counts.zero_()
    assert geodetic() == 0 and pixels() == 0 and gather(v=None) == 0                                # the same arguments, accepted
    torch.cuda.synchronize()
    assert not (lonlat == -7.0).any() and not (colrow == -7.0).any() and not (state == 0xAB).any() and int(counts.sum()) >= n


def test_wrapper_refusals_on_the_device():
    from brdf_nerf_amd import Grid, camera, grid_pixels, orthophoto, sample_image, world_pixels
    from brdf_nerf_amd import functions as Fn
    rpc = rpc_of(K.make_rpc("z17", 1))
    grid = Grid(0.0, 0.0, 0.5, 5, 4)
    dsm, img = torch.zeros(4, 5, device=DEV), torch.zeros(6 * 7, 3, device=DEV)
    cr = torch.zeros(4, 5, 2, dtype=torch.float64, device=DEV)
    for call in (lambda: grid_pixels(dsm.cpu(), grid, rpc, 17), lambda: orthophoto(img.cpu(), 6, 7, rpc, dsm, grid, 17),
                 lambda: orthophoto(img, 6, 7, rpc, dsm.cpu(), grid, 17), lambda: sample_image(img, 6, 7, cr.cpu()),
                 lambda: sample_image(img.cpu(), 6, 7, cr), lambda: world_pixels(rpc, torch.zeros(3, 3, dtype=torch.float64), 17),
                 lambda: sample_image(img, 6, 7, cr, visible=torch.ones(4, 5, dtype=torch.uint8))):
        with pytest.raises(ValueError, match="device"):
            call()
    with pytest.raises(ValueError, match="zone"):
        orthophoto(img, 6, 7, rpc, dsm, grid, 61)
    with pytest.raises(ValueError, match="pixels"):
        orthophoto(img, 7, 7, rpc, dsm, grid, 17)
    with pytest.raises(ValueError, match="upwards"):
        orthophoto(img, 6, 7, rpc, dsm, grid, 17, view_dir=[0.0, 1.0, -1.0])
    with pytest.raises(ValueError, match="no finite cell"):
        orthophoto(img, 6, 7, rpc, torch.full((4, 5), float("nan"), device=DEV), grid, 17)
    with pytest.raises(ValueError, match="strides"):
        Fn.image_gather(img, 6, 7, 3, (7 * 3, 3, 2), cr)
    with pytest.raises(ValueError, match="state"):
        Fn.image_gather(img, 6, 7, 3, (21, 3, 1), cr, state=torch.zeros(19, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="colrow"):
        Fn.grid_pixels(rpc, dsm, 0.0, 0.0, 0.5, 17, 0, colrow=torch.zeros(4, 5, 2, device=DEV))
    with pytest.raises(ValueError, match="altitudes"):
        camera.view_direction(rpc, 17, False, 10.0, 10.0)
