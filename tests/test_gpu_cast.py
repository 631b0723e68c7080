"""bn_cast_rays against the numpy statement of tests/cast_cases.py: depth (NaNs alike), state, cell, nan_cells and counts bit for
bit, on every grid shape, view direction, ray count, chunk cut and refusal; the round trips through point_cloud and the DSM splat;
then the Python surface: cast_rays under two ranks, grid_to_view, surface_priors, ray_table, a training loop and score_view."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cast_cases as K
import visibility_cases as V
from test_gpu_parity import DEV, _free_port

pytestmark = pytest.mark.gpu

npy = lambda t: None if t is None else t.detach().cpu().numpy()
NAMES = ("depth", "state", "cell", "nan_cells", "counts")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(rays, center, rng, dsm, xoff, yoff, zmax=K.INF, **kw):
    from brdf_nerf_amd import functions as Fn
    rays = rays if torch.is_tensor(rays) else dev(rays)
    return tuple(npy(t) for t in Fn.cast_rays(rays, center, rng, dev(dsm), xoff, yoff, K.RES, zmax, **kw))


def check(got, want, what=""):
    """Bitwise: the depths are compared as their 32 bits, so NaN equals NaN.  An output that was not asked for is None."""
    for g, w, name in zip(got, want, NAMES):
        if g is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        a, b = (g.view(np.uint32), w.view(np.uint32)) if name == "depth" else (g, w)
        assert np.array_equal(a, b), (what, name, int((a != b).sum()), np.flatnonzero(a != b)[:4])


def check_all(rays, center, rng, dsm, xoff, yoff, what):
    """The entry under zmax = inf and zmax = the grid's maximum, with and without the two optional outputs."""
    want = K.cast_statement(rays, center, rng, dsm, xoff, yoff, K.RES)
    zmax = V.grid_zmax(dsm)
    check(run(rays, center, rng, dsm, xoff, yoff), want, (what, "inf"))
    check(run(rays, center, rng, dsm, xoff, yoff, zmax), want, (what, "zmax"))
    for z in (K.INF, zmax):
        bare = run(rays, center, rng, dsm, xoff, yoff, z, want_cell=False, want_nan=False)
        assert bare[2] is None and bare[3] is None
        check(bare, want, (what, "bare", z))
    check(run(rays, center, rng, dsm, xoff, yoff, zmax, want_nan=False), want, (what, "cell only"))
    return want


@pytest.mark.parametrize("shape", K.GRID_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bit_equal_to_the_statement(shape):
    """257 rays over and around each grid from every elevation and azimuth of the lists, at a dyadic and at a UTM-sized origin."""
    dsm = K.grid_case(shape)
    seen = np.zeros(5, dtype=np.int64)
    for n, (el, az) in enumerate((el, az) for el in K.ELEVATIONS for az in K.AZIMUTHS):
        xoff, yoff = K.ORIGINS["utm" if n % 2 else "dyadic"]
        rays, center, rng = K.scatter_view(257, dsm, xoff, yoff, el, az, seed=n)
        seen += check_all(rays, center, rng, dsm, xoff, yoff, (shape, el, az))[4]
    assert seen[K.TOP] > 0 and seen[K.WALL] > 0 and seen[K.MISS] > 0 and seen[K.NODATA] > 0      # conditions on the inputs


@pytest.mark.parametrize("R", K.SIZES)
def test_ray_counts_and_strided_rows(R):
    """R around the wave and the block; rows of 8, of 11 and of 11 floats cut out of rows of 13 (read in place, stride 13)."""
    from brdf_nerf_amd import functions as Fn
    if R == 2304:
        dsm, rays, center, rng, xoff, yoff = K.block_view("utm")
        want = check_all(rays, center, rng, dsm, xoff, yoff, "block view")
        assert want[4].tolist() == [K.BLOCK_COUNTS["top"], K.BLOCK_COUNTS["wall"], 0, 0, 0]
    else:
        dsm = K.grid_case((33, 65))
        xoff, yoff = K.ORIGINS["utm"]
        rays, center, rng = K.scatter_view(R, dsm, xoff, yoff, 45.0, 17.0)
        want = check_all(rays, center, rng, dsm, xoff, yoff, R)
    wide = torch.full((R, 13), float("nan"), device=DEV)
    wide[:, :8] = dev(rays)
    for view in (wide[:, :11], wide[:, :8]):
        assert view.stride(0) == 13 and (R == 1 or not view.is_contiguous())
        check(run(view, center, rng, dsm, xoff, yoff), want, ("strided", view.shape[1]))
    eleven = torch.zeros((R, 11), device=DEV)
    eleven[:, :8] = dev(rays)
    check(run(eleven, center, rng, dsm, xoff, yoff), want, "11 columns")
    assert Fn.cast_rays(eleven[:0], center, rng, dev(dsm), xoff, yoff, K.RES)[4].tolist() == [0] * 5      # no ray: nothing launched


def test_engineered_cases():
    """The graze (<=), the corner (both indices move on a tie), the closed forms and every single case, on the device."""
    for case in (K.graze_case(), K.corner_case(), K.closed_form_cases()[:6]):
        dsm, rays, center, rng, xoff, yoff = case
        check_all(rays, center, rng, dsm, xoff, yoff, "engineered")
    dsm, rays, center, rng, xoff, yoff = K.graze_case()
    got = run(rays, center, rng, dsm, xoff, yoff)
    assert (int(got[1][0]), float(got[0][0]), int(got[2][0])) == (K.TOP, 4.5, 4)
    dsm, rays, center, rng, xoff, yoff = K.corner_case()
    got = run(rays, center, rng, dsm, xoff, yoff)
    assert int(got[1][0]) == K.MISS and np.isnan(got[0][0]) and int(got[2][0]) == -1
    dsm, rays, center, rng, xoff, yoff, want = K.closed_form_cases()
    got = run(rays, center, rng, dsm, xoff, yoff)
    assert [(int(s), float(d), int(c)) for s, d, c in zip(got[1], got[0], got[2])] == want
    dsm, cases, center, rng, xoff, yoff = K.single_cases()
    rays = np.concatenate([c[0] for c in cases.values()])
    want = check_all(rays, center, rng, dsm, xoff, yoff, "singles")
    for k, (name, (_, (state, depth, cell, nan_cells))) in enumerate(cases.items()):
        assert (int(want[1][k]), int(want[2][k]), int(want[3][k])) == (state, cell, nan_cells), name
    for special in (np.full((5, 70), np.nan, dtype=np.float32), np.full((3, 3), np.inf, dtype=np.float32),
                    np.full((3, 3), -np.inf, dtype=np.float32)):
        xoff, yoff = K.ORIGINS["dyadic"]
        rays, center, rng = K.scatter_view(65, special, xoff, yoff, 45.0, 135.0)
        check_all(rays, center, rng, special, xoff, yoff, "special grid")


def test_chunks_write_their_slices_and_counts_add_up():
    """The rays cut at 0, 1, 64 and R into caller-owned buffers: every chunk writes its own rows and no other, the counts
    accumulate, and the whole is the one-call result."""
    from brdf_nerf_amd import functions as Fn
    dsm = K.grid_case((33, 65))
    xoff, yoff = K.ORIGINS["utm"]
    R = 257
    rays, center, rng = K.scatter_view(R, dsm, xoff, yoff, 45.0, 263.0)
    want = K.cast_statement(rays, center, rng, dsm, xoff, yoff, K.RES)
    r, d = dev(rays), dev(dsm)
    depth = torch.full((R,), -7.0, device=DEV)
    state = torch.full((R,), 0xAB, dtype=torch.uint8, device=DEV)
    cell = torch.full((R,), -9, dtype=torch.int32, device=DEV)
    nan_cells = torch.full((R,), -9, dtype=torch.int32, device=DEV)
    counts = torch.zeros((5,), dtype=torch.int64, device=DEV)
    cuts = [0, 0, 1, 64, R]
    for a, b in zip(cuts[:-1], cuts[1:]):
        Fn.cast_rays(r[a:b], center, rng, d, xoff, yoff, K.RES, V.grid_zmax(dsm), depth=depth[a:b], state=state[a:b], cell=cell[a:b],
                     nan_cells=nan_cells[a:b], counts=counts)
        assert (depth[b:] == -7.0).all() and (state[b:] == 0xAB).all() and (cell[b:] == -9).all() and (nan_cells[b:] == -9).all()
        part = tuple(w[:b] for w in want[:4]) + (np.array([(want[1][:b] == k).sum() for k in range(5)], dtype=np.int64),)
        check((npy(depth[:b]), npy(state[:b]), npy(cell[:b]), npy(nan_cells[:b]), npy(counts)), part, ("cut", a, b))
    check((npy(depth), npy(state), npy(cell), npy(nan_cells), npy(counts)), want, "whole")


def test_refusals():
    """BN_EINVAL through the raw ABI, nothing launched, every buffer as it was."""
    from brdf_nerf_amd import _lib as L
    lib = L.lib()
    H, W, R = 7, 9, 65
    grid = K.grid_case((H, W))
    xoff, yoff = K.ORIGINS["dyadic"]
    rays_np, center, rng = K.scatter_view(R, grid, xoff, yoff, 45.0, 17.0)
    rays, dsm = dev(rays_np), dev(grid)
    depth = torch.full((R,), -7.0, device=DEV)
    state = torch.full((R,), 0xAB, dtype=torch.uint8, device=DEV)
    cell = torch.full((R,), -9, dtype=torch.int32, device=DEV)
    nan_cells = torch.full((R,), -9, dtype=torch.int32, device=DEV)
    counts = torch.full((5,), -5, dtype=torch.int64, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    nan, inf = float("nan"), float("inf")
    c3 = lambda v: (C.c_double * 3)(*v)

    def call(r=p(rays), stride=8, R=R, c=c3(center), rng=rng, s=p(dsm), H=H, W=W, xoff=xoff, yoff=yoff, res=K.RES, zmax=inf, d=p(depth),
             st=p(state), ce=p(cell), n=p(nan_cells), k=p(counts)):
        return lib.bn_cast_rays(r, stride, R, c, rng, s, H, W, xoff, yoff, res, zmax, d, st, ce, n, k, None)

    bad = [dict(r=None), dict(c=None), dict(s=None), dict(d=None), dict(st=None), dict(k=None), dict(R=-1), dict(R=(1 << 30) + 1),
           dict(H=0), dict(W=0), dict(H=-2), dict(H=1 << 15, W=(1 << 15) + 1), dict(stride=7), dict(stride=0), dict(stride=-8),
           dict(res=0.0), dict(res=-0.5), dict(res=inf), dict(res=nan), dict(rng=0.0), dict(rng=-1.0), dict(rng=inf), dict(rng=nan),
           dict(c=c3((nan, 0.0, 0.0))), dict(c=c3((0.0, inf, 0.0))), dict(c=c3((0.0, 0.0, -inf))), dict(xoff=nan), dict(yoff=inf),
           dict(xoff=-inf), dict(zmax=nan)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"cast_rays" in lib.bn_last_error()
    assert call(R=0) == 0                                                  # accepted, nothing launched
    torch.cuda.synchronize()
    assert (depth == -7.0).all() and (state == 0xAB).all() and (cell == -9).all() and (nan_cells == -9).all() and (counts == -5).all()
    counts.zero_()
    assert call(ce=None, n=None) == 0                                      # the same arguments, accepted, without the optional outputs
    torch.cuda.synchronize()
    want = K.cast_statement(rays_np, center, rng, grid, xoff, yoff, K.RES)
    assert (cell == -9).all() and (nan_cells == -9).all()
    check((npy(depth), npy(state), None, None, npy(counts)), want)
    counts.zero_()
    assert call(zmax=V.grid_zmax(grid)) == 0
    torch.cuda.synchronize()
    check((npy(depth), npy(state), npy(cell), npy(nan_cells), npy(counts)), want)


def test_wrapper_refusals_on_the_device():
    from brdf_nerf_amd import Grid, SceneFrame, cast_rays, surface_priors
    from brdf_nerf_amd import functions as Fn
    dsm = dev(K.grid_case((7, 9)))
    grid = Grid(0.0, 0.0, 0.5, 9, 7)
    utm = SceneFrame((0.0, 0.0, 0.0), 100.0)
    rays = torch.zeros((12, 11), device=DEV)
    for fn in (cast_rays, surface_priors):
        for r, d, g, what in ((rays.cpu(), dsm, grid, "device"), (rays, dsm.cpu(), grid, "device"), (rays, dsm, Grid(0.0, 0.0, 0.5, 7, 9), "grid"),
                              (rays.double(), dsm, grid, "float32"), (rays, dsm[:, ::2], grid, "contiguous")):
            with pytest.raises(ValueError, match=what):
                fn(r, utm, d, g)
        with pytest.raises(ValueError, match="ecef"):
            fn(rays, SceneFrame.ecef((6378137.0, 0.0, 0.0), 100.0), dsm, grid)
    with pytest.raises(ValueError, match="depth"):
        Fn.cast_rays(rays, (0.0, 0.0, 0.0), 1.0, dsm, 0.0, 0.0, 0.5, depth=torch.zeros((11,), device=DEV))
    with pytest.raises(ValueError, match="device"):
        Fn.cast_rays(rays, (0.0, 0.0, 0.0), 1.0, dsm, 0.0, 0.0, 0.5, counts=torch.zeros((5,), dtype=torch.int64))


@functools.lru_cache(maxsize=None)
def block_on_device(origin):
    from brdf_nerf_amd import Grid, SceneFrame, cast_rays
    dsm, rays, center, rng, xoff, yoff = K.block_view(origin)
    frame, grid = SceneFrame(center, rng), Grid(xoff, yoff, K.RES, 64, 64)
    return dsm, rays, frame, grid, cast_rays(dev(rays), frame, dev(dsm), grid)


def test_cast_rays_chunks_and_the_block_view():
    """The public entry: the grid's maximum is found inside, any chunk gives the one-call result, the counts are Python integers."""
    from brdf_nerf_amd import cast_rays
    for origin in K.ORIGINS:
        dsm, rays, frame, grid, whole = block_on_device(origin)
        want = K.cast_statement(rays, frame.center, frame.range, dsm, grid.xoff, grid.yoff, K.RES)
        assert set(whole) == set(NAMES) and whole["counts"] == want[4].tolist() and all(type(v) is int for v in whole["counts"])
        check(tuple(npy(whole[k]) for k in NAMES[:4]), want[:4], origin)
        for chunk in (1000, 64):
            got = cast_rays(dev(rays), frame, dev(dsm), grid, chunk=chunk, want_cell=chunk == 64)
            assert ("cell" in got) == (chunk == 64) and got["counts"] == whole["counts"]
            for k in got:
                assert k == "counts" or torch.equal(got[k].view(torch.uint8), whole[k].view(torch.uint8)), (chunk, k)


def test_top_hits_land_on_the_surface():
    """Round trip: on every TOP hit of the block-scene views point_cloud(rays, depth, frame)[:, 2] is the hit cell's height within
    2^-23 far range metres - one float32 rounding of the depth moves the point by at most 2^-24 far range along the ray; doubled."""
    from brdf_nerf_amd import point_cloud
    for origin in K.ORIGINS:
        dsm, rays, frame, grid, got = block_on_device(origin)
        top = npy(got["state"]) == K.TOP
        z = npy(point_cloud(dev(rays), got["depth"], frame))[:, 2]
        err = np.abs(z[top] - dsm.reshape(-1)[npy(got["cell"])[top]])
        bound = 2.0 ** -23 * float(rays[:, 7].max()) * frame.range
        print(f"{origin}: {int(top.sum())} tops, max |z - h| {err.max():.3e} m, bound {bound:.3e} m")
        assert top.sum() == K.BLOCK_COUNTS["top"] and err.max() <= bound


def test_nadir_depths_splat_back_to_the_raster():
    """One nadir ray through every cell centre: a DsmAccumulator(radius=0) of the cast depths returns the raster within 2^-20 m plus
    the bound above on every cell that received a point (the depth's rounding is half that bound; the splat's quantum adds 2^-21 m
    and the float32 of a height below 32 m 2^-20 m; bound / 2 >= 2^-21 because far range is over 8 m)."""
    from brdf_nerf_amd import DsmAccumulator, Grid, SceneFrame, cast_rays
    dsm = V.relief(33, 65, seed=4, nan=0.0, specials=False)
    assert np.abs(dsm).max() < 32.0
    H, W = dsm.shape
    xoff, yoff = K.ORIGINS["utm"]
    center, rng = K.frame_of(dsm, xoff, yoff)
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    world = np.stack([xoff + (ii.reshape(-1) + 0.5) * K.RES, yoff - (jj.reshape(-1) + 0.5) * K.RES, np.full(H * W, 60.0)], -1)
    rays = np.zeros((H * W, 8), dtype=np.float32)
    rays[:, 0:3] = (world - np.asarray(center)) / rng
    rays[:, 5], rays[:, 6], rays[:, 7] = -1.0, 0.25, 2.5                   # from 50 m down to -40 m
    frame, grid = SceneFrame(center, rng), Grid(xoff, yoff, K.RES, W, H)
    got = cast_rays(dev(rays), frame, dev(dsm), grid)
    check(tuple(npy(got[k]) for k in NAMES[:4]), K.cast_statement(rays, center, rng, dsm, xoff, yoff, K.RES)[:4], "nadir")
    assert got["counts"] == [H * W, 0, 0, 0, 0] and np.array_equal(npy(got["cell"]), np.arange(H * W))
    back, count = DsmAccumulator(grid, DEV, radius=0).add(dev(rays), got["depth"], frame).result()
    back, count = npy(back), npy(count)
    bound = 2.0 ** -20 + 2.0 ** -23 * 2.5 * rng
    assert (count == 1).all() and np.abs(back.astype(np.float64) - dsm).max() <= bound


def test_two_rank_cast_matches_one_rank():
    """World 2: two ranks on cuda:0 over gloo (tests/dist_cast_worker.py), each child under its own time limit and started once:
    the gathered rows and the summed counts are the single process's, bitwise."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dist_cast_worker.py")
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


def test_grid_to_view_and_surface_priors():
    from brdf_nerf_amd import grid_to_view, surface_priors
    dsm, rays, frame, grid, got = block_on_device("utm")
    index = torch.arange(64 * 64, dtype=torch.int32, device=DEV).reshape(64, 64)
    assert torch.equal(grid_to_view(index, got["cell"], fill=-1), got["cell"])
    seen = grid_to_view(dev(dsm), got["cell"])
    hit = got["cell"] >= 0
    assert torch.equal(seen[hit], dev(dsm).reshape(-1)[got["cell"][hit].long()]) and bool(torch.isnan(seen[~hit]).all())
    holes = dsm.copy()
    holes[30:34, :] = np.nan                                               # rays that pass these cells are not valid priors
    want_cast = K.cast_statement(rays, frame.center, frame.range, holes, grid.xoff, grid.yoff, K.RES)
    kw = dict(weight=0.75, stdscale=2.0, margin=0.5, std_span=3.0)
    want = K.surface_prior_statement(want_cast, **kw)
    pr = surface_priors(dev(rays), frame, dev(holes), grid, **kw)
    assert 0 < want[1].sum() < want[1].size and pr["counts"] == want_cast[4].tolist()
    for k, w in zip(("depths", "valid_depth", "depth_std"), want):
        g = npy(pr[k])
        assert g.dtype == np.float32 and g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32)), k


def surface_scene(rays):
    """A surface model under the rays of a view (numpy rows, as ray_table made them): cells of 2 m on the grid of the rays' points
    at mid depth, 40 m wider on every side, an undulating relief a tenth of the rays' own height span about their mid altitude."""
    from brdf_nerf_amd import Grid
    from test_gpu_priors import scene
    sc = scene("z17", 12, 12, 10)
    r = rays.astype(np.float64)
    at = lambda s: (r[:, 0:3] + r[:, 3:6] * s[:, None]) * sc["rng"] + np.asarray(sc["center"])
    mid, top, low = at(0.5 * (r[:, 6] + r[:, 7])), at(r[:, 6]), at(r[:, 7])
    grid = Grid.from_cloud((mid[:, :2].min(0) - 40.0).tolist(), (mid[:, :2].max(0) + 40.0).tolist(), 2.0)
    jj, ii = np.meshgrid(np.arange(grid.height), np.arange(grid.width), indexing="ij")
    span = float(top[:, 2].mean() - low[:, 2].mean())
    dsm = (mid[:, 2].mean() + 0.1 * span * np.sin(0.3 * ii) * np.cos(0.2 * jj)).astype(np.float32)
    return grid, dsm


def test_ray_table_with_a_surface_prior_trains():
    """One view with a surface prior, one with None: the first view's columns are surface_priors of its own rays, the second's are
    zero, the rays are bitwise the table's without priors; three TrainLoop steps with ds_lambda > 0 on it give finite losses that
    differ from the lambda-0 run."""
    from brdf_nerf_amd import SceneFrame, surface_priors
    from brdf_nerf_amd.camera import ray_table
    from brdf_nerf_amd.train import TrainLoop
    from test_gpu_parity import make_args, mini
    import camera_cases as M
    from test_gpu_priors import scene
    sc = scene("z17", 12, 12, 10)
    view = {"rpc": sc["d"], "H": 12, "W": 10, "min_alt": sc["lo"], "max_alt": sc["hi"], "sun": M.SUN}
    n = 120
    g = torch.Generator().manual_seed(5)
    images = [torch.rand(n, 3, generator=g), torch.rand(n, 3, generator=g)]
    make = lambda **kw: ray_table([view, view], images, sc["center"], sc["rng"], zone=17, device=DEV, **kw)
    plain = make()
    grid, dsm = surface_scene(npy(plain.data["rays"][:n]))
    pri = {"dsm": dev(dsm), "grid": grid, "weight": 0.5}
    table = make(priors=[pri, None], std_span=0.25)
    assert "depths" not in plain.data and set(table.data) == set(plain.data) | {"depths", "valid_depth", "depth_std"}
    for k in plain.data:
        assert torch.equal(table.data[k].view(torch.int32), plain.data[k].view(torch.int32)), k
    one = surface_priors(plain.data["rays"][:n], SceneFrame(sc["center"], sc["rng"]), pri["dsm"], grid, weight=0.5, std_span=0.25)
    want = K.surface_prior_statement(K.cast_statement(npy(plain.data["rays"][:n]), sc["center"], sc["rng"], dsm, grid.xoff, grid.yoff,
                                                      grid.resolution), weight=0.5, std_span=0.25)
    for k, w in zip(("depths", "valid_depth", "depth_std"), want):
        assert table.data[k].shape[0] == 2 * n and torch.equal(table.data[k][:n], one[k]) and not table.data[k][n:].any(), k
        assert np.array_equal(npy(one[k]).view(np.uint32), w.view(np.uint32)), k
    assert int(table.data["valid_depth"].sum()) == int(want[1].sum()) >= n // 2               # (>=: a condition on the inputs)
    normal = make(priors=[pri, None], want_normals=True)
    assert (normal.data["normals"] == torch.tensor([0.0, 0.0, 1.0], device=DEV)).all() and not normal.data["valid_normal"].any()
    with pytest.raises(ValueError, match="cs='utm'"):
        ray_table([view], images[:1], sc["center"], sc["rng"], cs="ecef", zone=17, device=DEV, priors=[pri])
    with pytest.raises(ValueError, match="grid"):
        make(priors=[{"dsm": pri["dsm"]}, None])
    cfg = mini()

    def losses_of(lam):
        a = make_args(cfg)
        for k, v in dict(batch_size=64, lr=5e-4, max_train_steps=40, brdf_on=0.0, cos_irra_on=0.0, nrrg_on=0.0, ds_drop=0.5, ds_lambda=lam,
                         gsam_only_on=1.0, nr_reg_lr_lambda=0.0, hs_lambda=0.0, in_ckpts="none").items():
            setattr(a, k, v)
        torch.manual_seed(0)
        loop = TrainLoop(a, make(priors=[pri, None], std_span=0.25), compute_dtype="fp32", near_far=None)
        torch.manual_seed(1)
        return [float(loop.step()["loss"]) for _ in range(3)]

    on, off = losses_of(10.0), losses_of(0.0)
    assert np.isfinite(on).all() and np.isfinite(off).all()
    assert all(abs(a - b) > 1e-5 * abs(b) for a, b in zip(on, off)), (on, off)


def test_score_view_with_a_cast_surface_model():
    """The 12 x 10 view of test_gpu_maps.py.  Without cast_dsm: exactly the keys and bits of before.  With it: depth_gt and
    cast_state are cast_rays' on the same rays, and the two MAEs equal the integer statement - the sum of round(|e| 2^20) over the
    kept pixels that were hit, over their count times 2^20."""
    from brdf_nerf_amd import cast_rays, fill_holes, score_view
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
    grid = plain["grid"]
    gt = (fill_holes(plain["dsm"])["filled"] + 0.4).contiguous()
    torch.manual_seed(31)
    got = score_view(models, args, rays, rgbs, H, W, cast_dsm=gt, grid=grid, **kw)
    assert set(got) == set(plain) | {"depth_gt", "cast_state", "depth_mae", "alt_mae_view"}
    for k, a in plain.items():                                             # nothing else moved
        b = got[k]
        if torch.is_tensor(a):
            assert a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), k
        else:
            assert a == b or (a != a and b != b), k
    cast = cast_rays(rays.float(), frame(), gt, grid)
    assert torch.equal(got["depth_gt"].view(torch.int32), cast["depth"].view(torch.int32)) and torch.equal(got["cast_state"], cast["state"])
    want = K.cast_statement(npy(rays.float()), frame().center, frame().range, npy(gt), grid.xoff, grid.yoff, grid.resolution)
    assert np.array_equal(npy(cast["depth"]).view(np.uint32), want[0].view(np.uint32)) and np.array_equal(npy(cast["state"]), want[1])
    keep = npy(mask).reshape(-1) & (want[2] >= 0)
    assert keep.sum() > 20                                                 # a condition on the inputs: the view sees the raster
    r64, d, d_gt = npy(rays).astype(np.float64), npy(got["depth"]).astype(np.float64).reshape(-1), want[0].astype(np.float64)
    alt = lambda s: (r64[:, 2] + r64[:, 5] * s) * frame().range + frame().center[2]
    with np.errstate(invalid="ignore"):
        errors = {"depth_mae": np.abs(d - d_gt) * frame().range, "alt_mae_view": np.abs(alt(d) - alt(d_gt))}
    for k, e in errors.items():
        sel = keep & np.isfinite(e)
        q = int(np.rint(e[sel] * 2.0 ** 20).astype(np.int64).sum())
        assert got[k] == q / (int(sel.sum()) * 2.0 ** 20) and got[k] > 0, k
