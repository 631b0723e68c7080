"""GPU tests of the camera geometry (brdf_nerf_amd/camera.py, bn_rpc_project / bn_rpc_localize / bn_geo_world / bn_rpc_rays).  Run on
the MI355X box with `pytest -m gpu`.

Up to the geodetic point only + - x / occur, so the kernels are held BIT FOR BIT to the numpy statement of
tests/camera_cases.py.  The device's float64 sin / cos / atanh / sinh / cosh / atan2 are not bit-specified: the world points are
held to the statement within 1e-6 m - 20 times below what a float32 normalised coordinate resolves at a range of 300 m
(6e-8 x 300 m = 2e-5 m): the bound comes from the output's own resolution.  From there:
  precision='exact'      every element within 1 float32 ulp of the statement
  precision='reference'  a 1e-8 m difference can flip the float32 rounding of a world coordinate, so an origin element may differ
                         by at most one float32 ulp of its WORLD coordinate divided by range, and at most 1 element in 10^4 may
                         differ at all (the generator asserts that +-1e-6 m flips fewer in the statement); direction and far
                         within 1 ulp."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import camera_cases as M
from conftest import ROOT
from test_gpu_parity import DEV, _free_port

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden")
WORLD_TOL = 1e-6            # metres


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same64(a, b):
    """Bitwise on float64, NaN positions equal (the payload of an arithmetic NaN is the machine's)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(bits64(a)[~nan], bits64(b)[~nan])


def ulp32(x):
    """The float32 ulp at |x| (float64 array)."""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def rpc_of(d, downscale=1.0):
    from brdf_nerf_amd.camera import Rpc
    return Rpc.from_dict(d, downscale)


def random_pixels(R, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-20.0, 1044.0, R), rng.uniform(-20.0, 1044.0, R)


def localize_split(rpc, cols, rows, W, n, alt, cuts):
    """bn_rpc_localize over [r0, r1) pieces of n rays -> lonlat (n, 2), skipped."""
    from brdf_nerf_amd import _lib
    from brdf_nerf_amd import camera as Cm
    out = torch.full((n, 2), 7.0, dtype=torch.float64, device=DEV)
    counts = torch.zeros(1, dtype=torch.int64, device=DEV)
    cuts = sorted({c for c in cuts if 0 <= c <= n} | {0, n})
    for a, b in zip(cuts[:-1], cuts[1:]):
        _lib.check(_lib.lib().bn_rpc_localize(rpc.ref(), Cm._p(cols), Cm._p(rows), W, a, b, float(alt), Cm._p(out[a:b]), Cm._p(counts),
                                              Cm._stream()), "bn_rpc_localize")
    return out.cpu().numpy(), int(counts.item())


@pytest.mark.parametrize("site", sorted(M.SITES))
def test_project_and_localize_bit_equal_to_the_statement(site):
    """Array mode at R in {1, 63, 64, 65, 257}: pixels -> geodetic points at both altitudes, and back to pixels."""
    from brdf_nerf_amd.camera import localize, project
    d = M.make_rpc(site, 3)
    rpc = rpc_of(d)
    for R in M.RAY_R:
        cols, rows = random_pixels(R, 100 + R)
        for alt in M.alt_bounds(site):
            lon, lat, bad = M.localize(d, cols, rows, alt)
            got, skipped = localize(rpc, cols, rows, alt, device=DEV)
            assert skipped == 0 and not bad.any()
            assert same64(got.cpu().numpy(), np.stack([lon, lat], -1)), (site, R, alt)
            alts = np.random.default_rng(R).uniform(alt - 30, alt + 30, R)
            c, r = project(rpc, lon, lat, alts, device=DEV)
            wc, wr = M.project(d, lon, lat, alts)
            assert same64(c.cpu().numpy(), wc) and same64(r.cpu().numpy(), wr), (site, R, alt)


@pytest.mark.parametrize("H,W", M.GRIDS)
def test_grid_mode_equals_array_mode_under_any_split(H, W):
    """Grids of 1 x 1, 3 x 5 and 65 x 33 with [r0, r1) cut at 0, 1, 64 and R: the statement's bits from every split, from the grid
    rule (col r % W, row r / W) and from the same pixels given as arrays."""
    d = M.rescaled(M.make_rpc("z17", 6), 2.0)
    rpc = rpc_of(M.make_rpc("z17", 6), 2.0)
    cols, rows = M.grid_pixels(H, W)
    n, alt = H * W, M.alt_bounds("z17")[1]
    lon, lat, _ = M.localize(d, cols, rows, alt)
    want = np.stack([lon, lat], -1)
    tc, tr = torch.from_numpy(cols).to(DEV), torch.from_numpy(rows).to(DEV)
    for cuts in ((), (1,), (64,), (1, 64)):
        grid, s1 = localize_split(rpc, None, None, W, n, alt, cuts)
        arr, s2 = localize_split(rpc, tc, tr, 1, n, alt, cuts)
        assert s1 == s2 == 0 and same64(grid, want) and same64(arr, want), (H, W, cuts)


def test_zero_determinant_and_non_finite_pixels_are_counted():
    from brdf_nerf_amd.camera import localize, view_rays
    sing = M.singular_rpc()
    cols, rows = random_pixels(65, 9)
    got, skipped = localize(rpc_of(sing), cols, rows, 10.0, device=DEV)
    assert skipped == 65 and np.isnan(got.cpu().numpy()).all()
    d = M.make_rpc("z38", 3)
    cols, rows = random_pixels(257, 10)
    cols[[0, 63, 64]], rows[[100, 256]] = (np.nan, np.inf, -np.inf), (np.inf, np.nan)
    lon, lat, bad = M.localize(d, cols, rows, 10.0)
    got, skipped = localize(rpc_of(d), cols, rows, 10.0, device=DEV)
    assert skipped == int(bad.sum()) == 5 and same64(got.cpu().numpy(), np.stack([lon, lat], -1))
    lo, hi = M.alt_bounds("z38")
    want = M.rays(d, cols, rows, lo, hi, "utm", 38, False, (290000.0, 1285000.0, 50.0), 300.0, M.sun_direction(*M.SUN))
    rays, skipped = view_rays(rpc_of(d), 0, 0, lo, hi, (290000.0, 1285000.0, 50.0), 300.0, zone=38, sun=M.SUN, rows=rows, cols=cols, device=DEV)
    rays = rays.cpu().numpy()
    assert skipped == want["skipped"] == 5
    assert np.array_equal(np.isnan(rays), np.isnan(want["rays"])) and np.isnan(rays[0, :8]).all() and not np.isnan(rays[:, 8:]).any()


CASES = [("z38", "utm", False), ("z38", "ecef", False), ("z17", "utm", False), ("z17", "ecef", False), ("z21", "utm", False),
         ("z21", "utm", True), ("z21", "ecef", False)]


@pytest.mark.parametrize("site,cs,south", CASES)
def test_geo_world_within_a_micrometre_of_the_statement(site, cs, south):
    from brdf_nerf_amd.camera import geo_world
    lat0, lon0, zone, _ = M.SITES[site]
    rng = np.random.default_rng(zone)
    lon, lat, alt = lon0 + rng.uniform(-0.05, 0.05, 257), lat0 + rng.uniform(-0.05, 0.05, 257), rng.uniform(-100, 500, 257)
    want = M.geo_world(lon, lat, alt, cs, zone, south)
    got = geo_world(np.stack([lon, lat], -1), alt, cs, zone, south, device=DEV).cpu().numpy()
    gap = np.abs(got - want).max()
    print(f"geo_world {site} {cs} south={south}: {gap:.3e} m")
    assert gap <= WORLD_TOL
    if cs == "utm":
        assert np.array_equal(got[:, 2], alt)


def check_rays(got, want, rng, center, precision, what):
    """The module docstring's conditions on rays (n, >= 8) against the statement's dict."""
    w = want["rays"]
    assert got.shape == w.shape and got.dtype == np.float32, what
    g64, w64 = got.astype(np.float64), w.astype(np.float64)
    one = ulp32(np.maximum(np.abs(g64), np.abs(w64)))
    rest = np.abs(g64[:, 3:8] - w64[:, 3:8])
    assert (rest <= one[:, 3:8]).all(), (what, "direction / far", rest.max())
    assert np.array_equal(got[:, 6], np.zeros(len(got), np.float32)), what
    if w.shape[1] > 8:
        assert np.array_equal(got[:, 8:].view(np.int32), w[:, 8:].view(np.int32)), (what, "sun")
    diff = np.abs(g64[:, :3] - w64[:, :3])
    if precision == "exact":
        assert (diff <= one[:, :3]).all(), (what, "origin", diff.max())
        return 0
    bound = ulp32(want["world_near"]) / rng
    changed = int((got[:, :3].view(np.int32) != w[:, :3].view(np.int32)).sum())
    assert (diff <= bound).all(), (what, "origin", diff.max(), bound.max())
    assert changed * 10000 <= got[:, :3].size, (what, f"{changed} origin elements differ")
    return changed


@pytest.mark.parametrize("site,cs,south", CASES)
def test_rays_against_the_statement(site, cs, south):
    """bn_rpc_rays in array mode at R in {1, 63, 64, 65, 257} and on the 65 x 33 grid cut at 1 and 64: lonlat_near / lonlat_far
    bit for bit (no transcendental on that path); the rays under both precisions; the same bits from every split, from chunks and
    from the grid's pixels given as arrays.  The world part of the ray kernel is read where float32 resolves a micrometre:
    pixels within 1 px of one another (4 m on the ground) with the first one's world point as the centre and range 1, so that
    precision='exact' stores near - centre with an ulp below 1e-6 m."""
    from brdf_nerf_amd.camera import geo_world, view_rays
    _, _, zone, _ = M.SITES[site]
    lo, hi = M.alt_bounds(site)
    d = M.make_rpc(site, 8)
    rpc = rpc_of(d)
    sun = M.sun_direction(*M.SUN)
    c0, r0 = M.grid_pixels(33, 65)
    raw = M.rays(d, c0, r0, lo, hi, cs, zone, south, (0.0, 0.0, 0.0), 1.0)
    loc = M.scene_loc([raw["rays"]])
    center = (loc["X_offset"], loc["Y_offset"], loc["Z_offset"])
    rng = max(loc["X_scale"], loc["Y_scale"], loc["Z_scale"])
    kw = dict(cs=cs, zone=zone, south=south, device=DEV)
    for R in M.RAY_R:
        cols, rows = random_pixels(R, 300 + R)
        for precision in ("reference", "exact"):
            want = M.rays(d, cols, rows, lo, hi, cs, zone, south, center, rng, sun, precision)
            rays, skipped, near, far = view_rays(rpc, 0, 0, lo, hi, center, rng, sun=M.SUN, rows=rows, cols=cols, precision=precision,
                                                 want_lonlat=True, **kw)
            assert skipped == 0 and rays.shape == (R, 11)
            assert same64(near.cpu().numpy(), want["lonlat_near"]) and same64(far.cpu().numpy(), want["lonlat_far"]), (R, precision)
            check_rays(rays.cpu().numpy(), want, rng, center, precision, (site, cs, R, precision))
        world = geo_world(near, hi, cs, zone, south).cpu().numpy()
        assert np.abs(world - want["world_near"]).max() <= WORLD_TOL
    pc, pr = 500.0 + np.random.default_rng(1).uniform(-0.5, 0.5, 64), 480.0 + np.random.default_rng(2).uniform(-0.5, 0.5, 64)
    near = M.rays(d, pc, pr, lo, hi, cs, zone, south, (0.0, 0.0, 0.0), 1.0)["world_near"]
    patch, _ = view_rays(rpc, 0, 0, lo, hi, tuple(near[0]), 1.0, rows=pr, cols=pc, precision="exact", **kw)
    local = near - near[0]
    assert np.abs(local).max() < 16.0                        # a condition on the inputs: float32 ulp below 1e-6 m
    gap = np.abs(patch[:, :3].cpu().numpy().astype(np.float64) - local)
    print(f"world part of the rays {site} {cs} south={south}: {gap.max():.3e} m (float32 rounding of up to {ulp32(local).max() / 2:.1e} m included)")
    assert (gap <= WORLD_TOL + ulp32(local) / 2).all()
    H, W = 65, 33
    cols, rows = M.grid_pixels(H, W)
    for precision in ("reference", "exact"):
        want = M.rays(d, cols, rows, lo, hi, cs, zone, south, center, rng, None, precision)
        whole, skipped, near, far = view_rays(rpc, H, W, lo, hi, center, rng, precision=precision, want_lonlat=True, **kw)
        assert skipped == 0 and whole.shape == (H * W, 8)
        assert same64(near.cpu().numpy(), want["lonlat_near"]) and same64(far.cpu().numpy(), want["lonlat_far"])
        changed = check_rays(whole.cpu().numpy(), want, rng, center, precision, (site, cs, "grid", precision))
        print(f"rays {site} {cs} south={south} {precision}: {changed} of {3 * H * W} origin elements differ from the statement")
        pieces = [view_rays(rpc, H, W, lo, hi, center, rng, precision=precision, span=s, **kw)[0] for s in ((0, 1), (1, 64), (64, H * W))]
        chunked = view_rays(rpc, H, W, lo, hi, center, rng, precision=precision, chunk=700, **kw)[0]
        arrays = view_rays(rpc, 0, 0, lo, hi, center, rng, precision=precision, rows=rows, cols=cols, **kw)[0]
        for other in (torch.cat(pieces, 0), chunked, arrays):
            assert torch.equal(other.view(torch.int32), whole.view(torch.int32)), (site, cs, precision)


@pytest.mark.parametrize("name", sorted(M.GOLDENS))
def test_view_rays_and_scene_bounds_reproduce_the_reference(name):
    """Against the goldens recorded from upstream's get_rays / normalize_rays / get_sun_dirs / rpc_scaling_params, under the two
    conditions of 'reference': scene_bounds gives scene.loc (6 values: 1 in 10^4 leaves room for none to differ) and view_rays
    with the recorded centre and range gives the reference's rays."""
    from brdf_nerf_amd.camera import scene_bounds, view_rays
    site, cs, south, ds = M.GOLDENS[name]
    zone = M.SITES[site][2]
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    views = [dict(v, downscale=ds) for v in M.golden_views(name)]
    loc, center, rng = scene_bounds(views, cs=cs, zone=zone, south=south, device=DEV)
    got = np.array([loc[k] for k in ("X_scale", "X_offset", "Y_scale", "Y_offset", "Z_scale", "Z_offset")])
    print(f"{name}: scene.loc differs from the reference in {int((got != g['loc']).sum())} of 6 values, by up to "
          f"{np.abs(got - g['loc']).max():.3e}")
    assert np.array_equal(got, g["loc"]), (got, g["loc"])
    assert center == tuple(g["center"]) and rng == float(g["range"])
    center, rng = tuple(g["center"]), float(g["range"])
    for i, v in enumerate(views):
        d = M.rescaled(v["rpc"], ds)
        rays, skipped = view_rays(rpc_of(v["rpc"], ds), v["H"], v["W"], v["min_alt"], v["max_alt"], center, rng, cs=cs, zone=zone,
                                  south=south, sun=v["sun"], device=DEV)
        c, r = M.grid_pixels(v["H"], v["W"])
        stmt = M.rays(d, c, r, v["min_alt"], v["max_alt"], cs, zone, south, center, rng, M.sun_direction(*v["sun"]))
        want = dict(stmt, rays=g[f"rays{i}"])
        changed = check_rays(rays.cpu().numpy(), want, rng, center, "reference", (name, i))
        print(f"{name} view {i}: {changed} of {3 * v['H'] * v['W']} origin elements differ from the reference")
        assert skipped == 0


def test_float32_world_origins_lose_a_quarter_metre_at_zone_17():
    """The defect, shown on the zone-17 fixture: 'reference' origins are up to 0.125 m / range from the 'exact' ones (northing),
    and the exact rays put altitude_image(rays, 0) on max_alt and altitude_image(rays, far) on min_alt within float32 resolution
    of the normalised coordinates (3 roundings of 2^-24 x range each)."""
    from brdf_nerf_amd import SceneFrame, altitude_image
    from brdf_nerf_amd.camera import view_rays
    name = "camera_z17_utm_d1"
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    v = M.golden_views(name)[1]
    frame = SceneFrame(g["center"], float(g["range"]))
    args = (rpc_of(v["rpc"]), v["H"], v["W"], v["min_alt"], v["max_alt"], frame)
    ref, _ = view_rays(*args, zone=17, precision="reference", device=DEV)
    exact, _ = view_rays(*args, zone=17, precision="exact", device=DEV)
    gap = (ref[:, :3].double() - exact[:, :3].double()).abs().amax(0).cpu().numpy() * frame.range
    top = (altitude_image(exact, torch.zeros(len(exact), device=DEV), frame) - v["max_alt"]).abs().max().item()
    bottom = (altitude_image(exact, exact[:, 7], frame) - v["min_alt"]).abs().max().item()
    print(f"reference - exact origins: {gap} m; exact rays: |altitude - max_alt| {top:.3e} m, |altitude - min_alt| {bottom:.3e} m")
    assert 0.1 < gap[1] <= 0.125 + 1e-3
    res = 2.0 ** -24 * frame.range
    assert top <= res and bottom <= 3 * res


def test_two_ranks_give_the_rays_of_one():
    """World 2: two ranks on cuda:0 over gloo (tests/dist_camera_worker.py), each child under its own time limit and started once."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dist_camera_worker.py")
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


def test_view_rays_go_straight_into_render_image():
    """A 12 x 10 view made by view_rays renders; rendering it in two chunks whose rays are made on the fly (span=) equals rendering
    the stored table, bit for bit; ray_table holds the same rows."""
    from brdf_nerf_amd import render_rays
    from brdf_nerf_amd.camera import ray_table, scene_bounds, view_rays
    from brdf_nerf_amd.evaluate import render_image
    from test_gpu_maps import view_case
    args, models, _, fl = view_case("rpv_an")
    H, W, chunk = 12, 10, 60
    lo, hi = M.alt_bounds("z17")
    view = {"rpc": M.make_rpc("z17", 12), "H": H, "W": W, "min_alt": lo, "max_alt": hi, "sun": M.SUN}
    _, center, rng = scene_bounds([view], zone=17, device=DEV)
    rpc = rpc_of(view["rpc"])
    rays, skipped = view_rays(rpc, H, W, lo, hi, center, rng, zone=17, sun=M.SUN, device=DEV)
    assert skipped == 0 and rays.shape == (H * W, 11) and float(rays[:, :3].abs().max()) <= 1.0 + 1e-6
    torch.manual_seed(5)
    stored = render_image(models, args, rays, chunk=chunk, **fl)
    assert torch.isfinite(stored["rgb"]).all() and stored["rgb"].shape == (H * W, 3)
    torch.manual_seed(5)
    parts = []
    for i in range(0, H * W, chunk):
        piece, _ = view_rays(rpc, H, W, lo, hi, center, rng, zone=17, sun=M.SUN, span=(i, i + chunk), device=DEV)
        out, _ = render_rays(models, args, piece, None, mode="test", **fl)
        parts.append((out["rgb_coarse"], out["depth_coarse"]))
    assert torch.equal(torch.cat([p[0] for p in parts], 0), stored["rgb"])
    assert torch.equal(torch.cat([p[1] for p in parts], 0), stored["depth"])
    table = ray_table([view, view], [torch.rand(H * W, 3), torch.rand(H * W, 3)], center, rng, zone=17, device=DEV)
    assert len(table) == 2 * H * W and torch.equal(table.data["rays"][H * W:], rays) and "depths" not in table.data
