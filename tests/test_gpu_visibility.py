"""bn_grid_visibility and bn_points_visibility against the numpy statement of tests/visibility_cases.py: vis, hit and counts bit
for bit, on every grid shape, direction family, special cell, band split and refusal; then the wrappers, two ranks and score_view."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import visibility_cases as V
from test_gpu_parity import DEV, _free_port

pytestmark = pytest.mark.gpu

npy = lambda t: None if t is None else t.detach().cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_grid(dsm, dirs, eps=0.0, zmax=V.INF, **kw):
    from brdf_nerf_amd import functions as Fn
    vis, hit, counts = Fn.grid_visibility(dev(dsm), V.RES, torch.from_numpy(np.asarray(dirs)), eps, zmax, want_hit=True, **kw)
    return npy(vis), npy(hit), npy(counts)


def run_points(pts, dsm, xoff, yoff, res, dirs, eps=0.0, zmax=V.INF, want_hit=True):
    from brdf_nerf_amd import functions as Fn
    vis, hit, counts = Fn.points_visibility(dev(pts), dev(dsm), xoff, yoff, res, torch.from_numpy(np.asarray(dirs)), eps, zmax, want_hit=want_hit)
    return npy(vis), npy(hit), npy(counts)


def check(got, want, what=""):
    for g, w, name in zip(got, want, ("vis", "hit", "counts")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g, w), (what, name, int((g != w).sum()))


@functools.lru_cache(maxsize=None)
def grid_reference(shape):
    """The grid of a shape and the statement under all directions, computed once (zmax = inf: the plain rule)."""
    dsm = V.grid_case(shape)
    return dsm, V.all_dirs(), V.grid_statement(dsm, V.RES, V.all_dirs())


def pick(ref, ks):
    return ref[0][ks], ref[1][ks], ref[2][ks]


@pytest.mark.parametrize("shape", V.GRID_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_grid_bit_equal_to_the_statement(shape):
    """Every direction family at once (K = 18), then K = 1, 3 and 8 of them, with zmax = +inf and with the computed maximum."""
    dsm, dirs, want = grid_reference(shape)
    zmax = V.grid_zmax(dsm)
    check(run_grid(dsm, dirs), want, "all, inf")
    check(run_grid(dsm, dirs, zmax=zmax), want, "all, zmax")
    for ks in ([8], [0, 5, 17], list(range(4, 12))):
        check(run_grid(dsm, dirs[ks], zmax=zmax), pick(want, ks), f"K={len(ks)}")
    if shape == (64, 64):
        block = V.grid_statement(dsm, V.RES, [V.direction(*d) for d in V.BLOCK_DIRS])
        assert block[2][:, 0].tolist() == V.BLOCK_BLOCKED
        check(run_grid(dsm, [V.direction(*d) for d in V.BLOCK_DIRS], zmax=zmax), block, "block scene")
    if shape[0] * shape[1] >= 8:
        n = want[2].sum(0)
        assert n[0] > 0 and n[1] > 0 and (n[2] > 0 or shape == (64, 64))       # conditions on the inputs: every class occurs


def test_more_directions_than_one_launch_takes():
    """K = 150: three launches of the entry (64 directions travel with one launch), each writing its own planes and counts."""
    rng = np.random.default_rng(3)
    dirs = np.stack([V.direction(el, az) for el, az in zip(rng.uniform(3.0, 80.0, 150), rng.uniform(0.0, 360.0, 150))])
    dsm = V.grid_case((7, 9))
    check(run_grid(dsm, dirs, zmax=V.grid_zmax(dsm)), V.grid_statement(dsm, V.RES, dirs))
    pts = V.point_case(65, dsm, 0.0, 0.0, V.RES)
    check(run_points(pts, dsm, 0.0, 0.0, V.RES, dirs), V.points_statement(pts, dsm, 0.0, 0.0, V.RES, dirs))


def test_special_grids():
    """An all-NaN grid is all nodata; a flat one all visible; the zenith sees every cell with data."""
    dirs = V.all_dirs()
    for dsm in (np.full((5, 70), np.nan, dtype=np.float32), np.full((9, 13), -3.0, dtype=np.float32), np.zeros((3, 3), dtype=np.float32)):
        want = V.grid_statement(dsm, V.RES, dirs)
        check(run_grid(dsm, dirs, zmax=V.grid_zmax(dsm)), want)
        check(run_grid(dsm, dirs), want)
    nan = run_grid(np.full((5, 70), np.nan, dtype=np.float32), dirs, zmax=-V.INF)
    assert (nan[0] == V.NODATA).all() and (nan[1] == -1).all() and (nan[2] == [0, 0, 350]).all()
    rough = V.relief(33, 65, seed=2)
    vis, hit, counts = run_grid(rough, [V.ZENITH, V.ZENITH * 7.5], zmax=V.grid_zmax(rough))
    assert ((vis == V.VISIBLE) == np.isfinite(rough)).all() and ((vis == V.NODATA) == ~np.isfinite(rough)).all() and (hit == -1).all()
    # an +inf cell blocks whatever looks at it, a -inf or NaN cell nothing; -0.0 is 0
    row = np.array([[1.0, -0.0, np.nan, -np.inf, 5.0, np.inf, 2.0, 1e30, 3.0]], dtype=np.float32)
    east, west = np.array([1.0, 0.0, 4.0]), np.array([-1.0, 0.0, 4.0])
    want = V.grid_statement(row, V.RES, [east, west])
    assert want[0][0, 0].tolist() == [0, 0, 2, 2, 0, 2, 0, 1, 1] and want[1][0, 0, :2].tolist() == [5, 5]
    assert want[0][1, 0].tolist() == [1, 1, 2, 2, 1, 2, 0, 0, 0]
    check(run_grid(row, [east, west], zmax=V.grid_zmax(row)), want)
    check(run_grid(row, [east, west]), want)


@pytest.mark.parametrize("eps", [0.0, 0.25])
def test_the_tie_does_not_block_and_the_next_float_does(eps):
    """h == zt + eps exactly at t = 4 from cell 0 (su == 1, sz == 0.5 exactly): visible; nextafter(h): blocked, hit = cell 4."""
    on, over = V.tie_row(eps), V.tie_row(eps, above=True)
    want_on, want_over = V.grid_statement(on, V.RES, V.TIE_DIR, eps), V.grid_statement(over, V.RES, V.TIE_DIR, eps)
    assert want_on[0][0, 0, 0] == V.VISIBLE and want_over[0][0, 0, 0] == V.BLOCKED and want_over[1][0, 0, 0] == 4
    for zmax in (V.INF, 13.0):
        check(run_grid(on, V.TIE_DIR, eps, zmax), want_on, "tie")
        check(run_grid(over, V.TIE_DIR, eps, zmax), want_over, "above the tie")
    # the same pair in point mode, from the centre of cell 0 at its altitude
    pts = np.array([[0.25, -0.25, 10.0]])
    for row, want in ((on, V.VISIBLE), (over, V.BLOCKED)):
        ref = V.points_statement(pts, row, 0.0, 0.0, V.RES, V.TIE_DIR, eps)
        assert ref[0][0, 0] == want
        check(run_points(pts, row, 0.0, 0.0, V.RES, V.TIE_DIR, eps), ref)


def test_raising_eps_on_the_device():
    dsm, dirs, want = grid_reference((33, 65))
    for eps in (0.25, 8.0):
        ref = V.grid_statement(dsm, V.RES, dirs, eps)
        assert not ((want[0] == V.VISIBLE) & (ref[0] == V.BLOCKED)).any() and (ref[0] != want[0]).any()
        check(run_grid(dsm, dirs, eps, V.grid_zmax(dsm)), ref, f"eps={eps}")


@pytest.mark.parametrize("cut", [None, 1, 13])
def test_row_bands_concatenate_to_the_whole(cut):
    """Bands (whole; (0, 1) + (1, H); 13 + 20 rows) written into one pre-filled buffer: the bands' rows are the whole result, the
    counts add up, and the rows a call does not own keep their bytes."""
    from brdf_nerf_amd import functions as Fn
    dsm, dirs, want = grid_reference((33, 65))
    H, W = dsm.shape
    K = len(dirs)
    d, t = dev(dsm), torch.from_numpy(dirs)
    vis = torch.full((K, H, W), 0xAB, dtype=torch.uint8, device=DEV)
    hit = torch.full((K, H, W), -7, dtype=torch.int32, device=DEV)
    counts = torch.zeros((K, 3), dtype=torch.int64, device=DEV)
    bands = [(0, H)] if cut is None else [(0, cut), (cut, H)]
    for n, (a, b) in enumerate(bands):
        Fn.grid_visibility(d, V.RES, t, 0.0, V.grid_zmax(dsm), rows=(a, b), vis=vis, hit=hit, counts=counts)
        if n == 0 and b < H:
            assert (vis[:, b:] == 0xAB).all() and (hit[:, b:] == -7).all()
            assert np.array_equal(npy(vis[:, :b]), want[0][:, :b]) and np.array_equal(npy(hit[:, :b]), want[1][:, :b])
            assert np.array_equal(npy(counts), V._counts(want[0][:, :b].reshape(K, -1)))
    check((npy(vis), npy(hit), npy(counts)), want)
    before = vis.clone()
    Fn.grid_visibility(d, V.RES, t, rows=(5, 5), vis=vis, hit=hit, counts=counts)          # an empty band writes and counts nothing
    assert torch.equal(vis, before) and np.array_equal(npy(counts), want[2])


def test_wrapper_rows_dir_tile_and_hit():
    """grid_visibility: dir_tile 1 and 3 against all K in one call; zmax is computed inside; rows= without a group leaves NODATA
    and -1 outside the band; want_hit=False returns no hit and the same vis."""
    from brdf_nerf_amd import grid_visibility
    dsm, dirs, want = grid_reference((33, 65))
    ks = list(range(4, 12))
    ref = pick(want, ks)
    d = dev(dsm)
    whole = grid_visibility(d, V.RES, dirs[ks].astype(np.float32).astype(np.float64), want_hit=True)
    assert set(whole) == {"visible", "hit", "counts"} and not whole["counts"].is_cuda
    for tile in (None, 1, 3):
        got = grid_visibility(d, V.RES, torch.from_numpy(dirs[ks]), want_hit=True, dir_tile=tile)
        check((npy(got["visible"]), npy(got["hit"]), npy(got["counts"])), ref, f"dir_tile={tile}")
    plain = grid_visibility(d, V.RES, torch.from_numpy(dirs[ks]))
    assert set(plain) == {"visible", "counts"} and np.array_equal(npy(plain["visible"]), ref[0])
    band = grid_visibility(d, V.RES, torch.from_numpy(dirs[ks]), rows=(7, 20), want_hit=True)
    assert np.array_equal(npy(band["visible"][:, 7:20]), ref[0][:, 7:20]) and np.array_equal(npy(band["hit"][:, 7:20]), ref[1][:, 7:20])
    assert (band["visible"][:, :7] == V.NODATA).all() and (band["visible"][:, 20:] == V.NODATA).all() and (band["hit"][:, 20:] == -1).all()
    assert np.array_equal(npy(band["counts"]), V._counts(ref[0][:, 7:20].reshape(len(ks), -1)))
    one = grid_visibility(d, V.RES, dirs[8].astype(np.float32))                              # (3,) float32 directions
    assert np.array_equal(npy(one["visible"]), V.grid_statement(dsm, V.RES, dirs[8].astype(np.float32).astype(np.float64))[0])


GRIDS = {"dyadic": (368640.0, 3301376.5, 0.5), "utm": (367891.7, 3300123.4, 0.3)}


@pytest.mark.parametrize("R", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("origin", sorted(GRIDS))
def test_points_bit_equal_to_the_statement(R, origin):
    """Points inside, outside, on cell edges and corners, NaN and inf ones, at UTM-sized coordinates (northing 3.3e6)."""
    xoff, yoff, res = GRIDS[origin]
    dsm = V.grid_case((33, 65))
    dirs = V.all_dirs()
    pts = V.point_case(R, dsm, xoff, yoff, res)
    want = V.points_statement(pts, dsm, xoff, yoff, res, dirs)
    if R >= 63:
        n = want[2].sum(0)
        assert n[0] > 0 and n[1] > 0 and n[2] > 0
    check(run_points(pts, dsm, xoff, yoff, res, dirs), want)
    check(run_points(pts, dsm, xoff, yoff, res, dirs, zmax=V.grid_zmax(dsm)), want)
    vis, hit, counts = run_points(pts, dsm, xoff, yoff, res, dirs[[9]], want_hit=False)
    assert hit is None and np.array_equal(vis, want[0][[9]]) and np.array_equal(counts, want[2][[9]])


def test_grid_mode_is_point_mode_on_the_cell_centres():
    from brdf_nerf_amd import Grid, point_visibility
    xoff, yoff, res = GRIDS["dyadic"]
    dsm, dirs, want = grid_reference((33, 65))
    assert res == V.RES
    got = point_visibility(dev(V.cell_centres(dsm, xoff, yoff, res)), dev(dsm), Grid(xoff, yoff, res, 65, 33), dirs, want_hit=True)
    K = len(dirs)
    check((npy(got["visible"]), npy(got["hit"]), npy(got["counts"])), (want[0].reshape(K, -1), want[1].reshape(K, -1), want[2]))
    empty = point_visibility(torch.zeros((0, 3), dtype=torch.float64, device=DEV), dev(dsm), Grid(xoff, yoff, res, 65, 33), dirs)
    assert empty["visible"].shape == (K, 0) and int(empty["counts"].sum()) == 0


def test_refusals():
    """BN_EINVAL through the raw ABI, nothing launched, every buffer as it was."""
    from brdf_nerf_amd import _lib as L
    lib = L.lib()
    H, W, K, R = 7, 9, 2, 5
    dsm = dev(V.grid_case((H, W)))
    vis = torch.full((K, H, W), 0xAB, dtype=torch.uint8, device=DEV)
    hit = torch.full((K, H, W), -7, dtype=torch.int32, device=DEV)
    counts = torch.full((K, 3), -5, dtype=torch.int64, device=DEV)
    enz = dev(V.point_case(R, npy(dsm), 0.0, 0.0, V.RES))
    p = lambda t: C.c_void_p(t.data_ptr())
    nan, inf = float("nan"), float("inf")

    def arr(rows):
        return (C.c_double * (3 * len(rows)))(*[v for r in rows for v in r])

    good = [(0.3, 0.2, 0.5), (-1.0, 0.0, 0.1)]
    bad_dirs = [[(0.3, 0.2, 0.5), (0.0, 1.0, 0.0)], [(0.3, 0.2, -0.5), good[1]], [(nan, 0.2, 0.5), good[1]], [good[0], (0.3, inf, 0.5)],
                [good[0], (0.3, 0.2, inf)], [good[0], (0.3, 0.2, nan)]]

    def grid(s=p(dsm), H=H, W=W, res=V.RES, row0=0, row1=H, d=arr(good), K=K, eps=0.0, zmax=inf, v=p(vis), h=p(hit), c=p(counts)):
        return lib.bn_grid_visibility(s, H, W, res, row0, row1, d, K, eps, zmax, v, h, c, None)

    def points(e=p(enz), R=R, s=p(dsm), H=H, W=W, xoff=0.0, yoff=0.0, res=V.RES, d=arr(good), K=K, eps=0.0, zmax=inf, v=p(vis), h=p(hit),
               c=p(counts)):
        return lib.bn_points_visibility(e, R, s, H, W, xoff, yoff, res, d, K, eps, zmax, v, h, c, None)

    shared = [dict(s=None), dict(d=None), dict(v=None), dict(c=None), dict(H=0), dict(W=0), dict(H=-2), dict(H=1 << 15, W=(1 << 15) + 1),
              dict(K=0), dict(K=-1), dict(K=4097), dict(res=0.0), dict(res=-0.5), dict(res=inf), dict(res=nan), dict(eps=-1e-9),
              dict(eps=inf), dict(eps=nan), dict(zmax=nan)] + [dict(d=arr(b)) for b in bad_dirs]
    for kw in shared + [dict(row0=-1), dict(row1=H + 1), dict(row0=5, row1=4), dict(row0=H + 1, row1=H + 1)]:
        assert grid(**kw) == -1, kw
        assert b"grid_visibility" in lib.bn_last_error()
    for kw in shared + [dict(e=None), dict(R=-1), dict(R=(1 << 30) + 1), dict(xoff=nan), dict(yoff=inf), dict(xoff=-inf)]:
        assert points(**kw) == -1, kw
        assert b"points_visibility" in lib.bn_last_error()
    assert grid(row0=3, row1=3) == 0 and points(R=0) == 0                 # accepted, nothing launched
    torch.cuda.synchronize()
    assert (vis == 0xAB).all() and (hit == -7).all() and (counts == -5).all()
    counts.zero_()
    assert grid(h=None, zmax=-inf) == 0                                   # the same arguments, accepted: hit NULL; zmax = -inf: all visible
    torch.cuda.synchronize()
    known = np.isfinite(npy(dsm))
    assert ((npy(vis) == V.VISIBLE) == known[None]).all() and (hit == -7).all() and int(counts.sum()) == K * H * W
    counts.zero_()
    assert grid() == 0
    torch.cuda.synchronize()
    check((npy(vis), npy(hit), npy(counts)), V.grid_statement(npy(dsm), V.RES, np.array(good)))


def test_wrapper_refusals_on_the_device():
    from brdf_nerf_amd import Grid, grid_visibility, point_visibility
    from brdf_nerf_amd import functions as Fn
    dsm = dev(V.grid_case((7, 9)))
    up = [0.0, 0.0, 1.0]
    for bad, what in ((dsm.double(), "float32"), (dsm[:, ::2], "contiguous"), (dsm.cpu(), "device")):
        with pytest.raises(ValueError, match=what):
            grid_visibility(bad, V.RES, up)
    with pytest.raises(ValueError, match="vis"):
        Fn.grid_visibility(dsm, V.RES, up, vis=torch.zeros((1, 7, 9), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="device"):
        Fn.grid_visibility(dsm, V.RES, up, counts=torch.zeros((1, 3), dtype=torch.int64))
    pts = torch.zeros((4, 3), dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="grid"):
        point_visibility(pts, dsm, Grid(0.0, 0.0, 0.5, 7, 9), up)
    with pytest.raises(ValueError, match="device"):
        point_visibility(pts.cpu(), dsm, Grid(0.0, 0.0, 0.5, 9, 7), up)


def test_two_rank_visibility_matches_one_rank():
    """World 2: two ranks on cuda:0 over gloo (tests/dist_visibility_worker.py), each child under its own time limit and started
    once: the gathered row bands and the summed counts are the single process's visible, hit and counts, bitwise."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dist_visibility_worker.py")
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


def test_score_view_splits_the_psnr_by_the_geometric_shadow():
    """The 12 x 10 view of test_gpu_maps.py.  Without sun_dir: exactly the keys and bits of before.  With one: `visibility` is the
    statement on point_cloud of the call's own depth over the raster it names, and psnr_sunlit / psnr_shadow are image_psnr under
    those masks.  The sun is the first of a fixed list under which the statement finds both classes."""
    from brdf_nerf_amd import fill_holes, image_psnr, point_cloud, score_view, view_visibility
    from test_gpu_dsm import frame
    from test_gpu_maps import CHUNK, VIEW_H, VIEW_W, view_case
    args, models, rays, fl = view_case("rpv_an")
    H, W = VIEW_H, VIEW_W
    g = torch.Generator().manual_seed(11)
    rgbs = torch.rand(H * W, 3, generator=g).to(DEV)
    mask = (torch.rand(H, W, generator=g) < 0.85).to(DEV)
    kw = dict(mask=mask, frame=frame(), chunk=CHUNK, **fl)
    torch.manual_seed(31)
    plain = score_view(models, args, rays, rgbs, H, W, **kw)
    assert set(plain) == {"psnr", "psnr_scl", "ssim", "ssim_scl", "ssim_skipped", "ssim_sums", "rgb", "depth", "dsm", "count", "grid", "skipped"}
    torch.manual_seed(31)
    assert set(score_view(models, args, rays, rgbs, H, W, mask=mask, chunk=CHUNK, **fl)) == \
        {"psnr", "psnr_scl", "ssim", "ssim_scl", "ssim_skipped", "ssim_sums", "rgb", "depth"}
    grid = plain["grid"]
    filled = fill_holes(plain["dsm"])["filled"]
    pts = npy(point_cloud(rays, plain["depth"], frame()))
    state = lambda raster, sun, eps=0.0: V.points_statement(pts, npy(raster), grid.xoff, grid.yoff, grid.resolution, sun, eps)[0][0]
    keep = npy(mask).reshape(-1)
    suns = [V.direction(el, az) for el in (25.0, 10.0, 45.0, 4.0, 70.0) for az in (135.0, 17.0, 250.0)]
    both = [s for s in suns if (state(filled, s)[keep] == V.BLOCKED).any() and (state(filled, s)[keep] == V.VISIBLE).any()]
    assert both, "no sun of the list leaves sunlit AND shadowed pixels on this view"      # a condition on the inputs
    sun = both[0]
    want = state(filled, sun)
    torch.manual_seed(31)
    got = score_view(models, args, rays, rgbs, H, W, sun_dir=torch.from_numpy(sun), **kw)
    assert set(got) == set(plain) | {"visibility", "shadow_source", "shadow_fraction", "psnr_sunlit", "psnr_shadow"}
    for k, a in plain.items():                                                             # nothing else moved
        b = got[k]
        if torch.is_tensor(a):
            assert a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), k
        else:
            assert a == b or (a != a and b != b), k
    assert got["shadow_source"] == "dsm" and got["visibility"].dtype == torch.uint8 and got["visibility"].shape == (H * W,)
    assert np.array_equal(npy(got["visibility"]), want)
    lit, dark = keep & (want == V.VISIBLE), keep & (want == V.BLOCKED)
    assert lit.any() and dark.any() and got["shadow_fraction"] == dark.sum() / (lit.sum() + dark.sum())
    assert got["psnr_sunlit"] == float(image_psnr(got["rgb"], rgbs, mask=dev(lit))[0])
    assert got["psnr_shadow"] == float(image_psnr(got["rgb"], rgbs, mask=dev(dark))[0])
    assert np.isfinite(got["psnr_sunlit"]) and np.isfinite(got["psnr_shadow"])
    vv = view_visibility(rays, got["depth"], frame(), filled, grid, sun)
    assert torch.equal(vv["visible"][0], got["visibility"])
    # the raster marched: shadow_dsm before gt_dsm before the view's own filled DSM; eps reaches the march; an empty class gives -1
    gt = (filled + 0.4).contiguous()
    low = torch.full_like(filled, -1e6)                     # a surface far below every pixel shadows none
    for extra, source, raster, eps in ((dict(gt_dsm=gt), "gt_dsm", gt, 0.0), (dict(gt_dsm=gt, shadow_dsm=low), "shadow_dsm", low, 0.0),
                                       (dict(shadow_eps=0.25), "dsm", filled, 0.25)):
        torch.manual_seed(31)
        res = score_view(models, args, rays, rgbs, H, W, sun_dir=sun, grid=grid, **dict(kw, **extra))
        assert res["shadow_source"] == source and np.array_equal(npy(res["visibility"]), state(raster, sun, eps)), source
        if source == "shadow_dsm":
            assert (state(raster, sun) == V.VISIBLE).all() and res["psnr_shadow"] == -1 and res["shadow_fraction"] == 0.0
            assert res["psnr_sunlit"] == float(image_psnr(res["rgb"], rgbs, mask=mask)[0])
