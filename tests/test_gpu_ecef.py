"""ECEF scenes on the device: bn_ecef_geodetic, bn_surface_points, bn_dsm_splat_points and bn_dsm_splat_world (world.hip) against
the numpy statement and the Python-integer splat of tests/ecef_cases.py, and everything behind SceneFrame(cs='ecef').

Bounds.  Points: 1e-6 m per coordinate against the statement (degrees at 111,320 m per degree), the bound bn_geo_world carries -
the device's float64 atan2 / sin / cos are not bit-specified.  Everything that is integer after the point is held to bits:
bn_dsm_splat_points against the Python-integer statement, the fused launch against the two-launch form, cs = utm against
bn_dsm_splat, chunks and ranks against one call.  End to end against the float64 statement the counts are equal (every golden
east and north keeps 1e-4 m from a cell edge) and a cell's mean altitude is within 2e-6 m.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import camera_cases as M
import dsm_cases as D
import ecef_cases as E
from test_gpu_parity import DEV, _free_port

pytestmark = pytest.mark.gpu

I64 = dict(dtype=torch.int64, device=DEV)


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                  # a copy: the shared inputs are read-only


def ecef_frame(name):
    from brdf_nerf_amd import SceneFrame
    center, rng = E.site_frame(name)
    return SceneFrame(center, rng, cs="ecef", zone=E.zone_of(name), south=E.SITES[name][1])


def site_inputs(name, R=None, strided=False):
    rays, depth = E.site_rays(name)
    rays, depth = dev(rays[:R]), dev(depth[:R])
    if strided:                                      # rows of 11 floats: the table's layout with the sun columns
        wide = torch.full((rays.shape[0], 11), float("nan"), device=DEV)
        wide[:, :8] = rays
        rays = wide[:, :8]
        assert rays.stride(0) == 11
    return rays, depth


def fresh(grid, radius=1, footprint="disc"):
    from brdf_nerf_amd import DsmAccumulator, Grid
    return DsmAccumulator(Grid(*grid), DEV, radius=radius, footprint=footprint)


# ------------------------------------------------------------------------------------------------------- points and altitude
@pytest.mark.parametrize("R", M.RAY_R)
def test_points_within_the_bound_of_the_statement(R):
    from brdf_nerf_amd import point_cloud
    from brdf_nerf_amd.camera import ecef_geodetic
    worst = {"lon": 0.0, "lat": 0.0, "alt": 0.0, "east": 0.0, "north": 0.0, "z": 0.0}
    for name in E.SITES:
        st = E.site_statement(name)
        lonlat, alt, skipped = ecef_geodetic(dev(st["xyz"][:R]), want_skipped=True)
        lonlat, alt = lonlat.cpu().numpy(), alt.cpu().numpy()
        assert skipped == 0 and lonlat.shape == (R, 2) and alt.shape == (R,)
        worst["lon"] = max(worst["lon"], np.abs(lonlat[:, 0] - st["lon"][:R]).max() * E.M_PER_DEG)
        worst["lat"] = max(worst["lat"], np.abs(lonlat[:, 1] - st["lat"][:R]).max() * E.M_PER_DEG)
        worst["alt"] = max(worst["alt"], np.abs(alt - st["enz"][:R, 2]).max())
        clouds = []
        for strided in (False, True):
            rays, depth = site_inputs(name, R, strided)
            enz = point_cloud(rays, depth, ecef_frame(name))
            assert enz.dtype == torch.float64 and tuple(enz.shape) == (R, 3)
            clouds.append(enz)
            d = np.abs(enz.cpu().numpy() - st["enz"][:R]).max(0)
            for k, v in zip(("east", "north", "z"), d):
                worst[k] = max(worst[k], float(v))
        assert torch.equal(clouds[0], clouds[1])
    print(f"R={R}: device - statement, metres: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) <= 1e-6


def test_free_points_within_the_bound_of_the_statement():
    """|lat| up to 80 degrees, both hemispheres, the equator, the antimeridian, altitudes -400 to 9000 m."""
    from brdf_nerf_amd.camera import ecef_geodetic, geo_world
    g = E.golden()
    xyz = g["free_xyz"]
    lon, lat, alt, _ = E.ecef_geodetic(xyz[:, 0], xyz[:, 1], xyz[:, 2])
    lonlat_d, alt_d = ecef_geodetic(dev(xyz))
    d_lon = np.abs(lonlat_d[:, 0].cpu().numpy() - lon).max() * E.M_PER_DEG
    d_lat = np.abs(lonlat_d[:, 1].cpu().numpy() - lat).max() * E.M_PER_DEG
    d_alt = np.abs(alt_d.cpu().numpy() - alt).max()
    print(f"free points: device - statement, metres: lon {d_lon:.2e}, lat {d_lat:.2e}, alt {d_alt:.2e}")
    assert max(d_lon, d_lat, d_alt) <= 1e-6
    # the round trip on the device: geo_world(cs='ecef') of the result, within the 2e-6 m of the one-step formula
    back = geo_world(lonlat_d, alt_d, cs="ecef").cpu().numpy()
    assert np.abs(back - xyz).max() <= 2e-6


@pytest.mark.parametrize("name", sorted(E.SITES))
def test_altitude_image_is_the_third_column_of_the_cloud(name):
    from brdf_nerf_amd import altitude_image, point_cloud
    rays, depth = site_inputs(name)
    alt = altitude_image(rays, depth, ecef_frame(name))
    assert alt.dtype == torch.float64 and tuple(alt.shape) == (E.N_RAYS,) and alt.is_contiguous()
    assert torch.equal(alt, point_cloud(rays, depth.reshape(-1, 1), ecef_frame(name))[:, 2])
    lo, hi = M.alt_bounds(E.SITES[name][0])
    assert float(alt.min()) > lo and float(alt.max()) < hi


# ----------------------------------------------------------------------------------------------------------------- the splat
SPLAT_GRIDS = {"1x1": (368412.0, 3359872.0, 2.0, 1, 1), "25x27": (368410.5, 3359880.0, 0.5, 25, 27), "3x300": (368400.3, 3359870.1, 0.3, 300, 3)}


def splat_cloud(grid, seed):
    """Points over and around a grid: random ones up to 6 cells outside on every side, points exactly on cell edges and on the
    outer edges, negative altitudes, NaN / inf coordinates, |altitude| == 2^23 and beyond, and one just inside that bound."""
    xoff, yoff, res, W, H = grid
    g = np.random.RandomState(seed)
    n = 260
    pts = np.stack([xoff + g.uniform(-6 * res, (W + 6) * res, n), yoff - g.uniform(-6 * res, (H + 6) * res, n), g.uniform(-30.0, 60.0, n)], -1)
    k = np.arange(40)
    edges = np.stack([xoff + (k % (W + 3) - 1) * res, yoff - (k % (H + 2) - 1) * res, -5.0 + k], -1)          # on edges; outside by one cell too
    bad = np.array([[np.nan, yoff, 1.0], [xoff, np.inf, 1.0], [xoff, yoff, -np.inf], [xoff, yoff, np.nan], [xoff + res / 2, yoff - res / 2, 2.0 ** 23],
                    [xoff + res / 2, yoff - res / 2, -1.2e7], [xoff + res / 2, yoff - res / 2, 8388602.0], [1e300, yoff, 1.0], [xoff, -1e300, 1.0]])
    pts = np.concatenate([pts, edges, bad])
    return pts[g.permutation(len(pts))]


@pytest.mark.parametrize("gname", list(SPLAT_GRIDS))
def test_splat_points_bit_equal_to_the_integer_statement(gname):
    grid = SPLAT_GRIDS[gname]
    pts = splat_cloud(grid, 3 + len(gname))
    wide = torch.full((len(pts), 5), 7.0, dtype=torch.float64, device=DEV)
    wide[:, :3] = dev(pts)
    for radius in (0, 1, 4):
        for footprint in ("disc", "square"):
            sums, counts, skipped = E.splat_points(pts, grid, radius, footprint)
            for enz in (dev(pts), wide[:, :3]):                         # contiguous rows and rows of 5 doubles
                acc = fresh(grid, radius, footprint).add_points(enz)
                got = acc.acc.cpu().numpy()
                assert np.array_equal(got, E.acc_int64(sums, counts)), (gname, radius, footprint)
                assert acc.skipped == skipped == 6
            assert int(got[..., 1].sum()) > 0
    # in two calls and shuffled: the same accumulator
    whole = fresh(grid, 1).add_points(dev(pts))
    parts = fresh(grid, 1).add_points(dev(pts[100:])).add_points(dev(pts[:100][::-1].copy()))
    assert torch.equal(whole.acc, parts.acc) and whole.skipped == parts.skipped


@pytest.mark.parametrize("name", sorted(E.SITES))
def test_fused_splat_is_the_two_launch_form_bit_for_bit(name):
    """bn_dsm_splat_world(cs = ecef) against bn_dsm_splat_points(bn_surface_points(...)): one device function each for the point
    and the deposit, so equal bits - from every split of the rays at 0, 1, 64 and R, and from a shuffled ray order."""
    from brdf_nerf_amd import point_cloud
    frame = ecef_frame(name)
    rays, depth = site_inputs(name)
    depth = depth.clone()
    depth[5], depth[70] = float("nan"), float("inf")                     # refused rows take part
    grid = E.cloud_grid(E.site_statement(name)["enz"])
    R = rays.shape[0]
    two = fresh(grid).add_points(point_cloud(rays, depth, frame))
    assert two.skipped == 2 and int(two.acc[..., 1].sum()) >= R - 2
    perm = torch.from_numpy(np.random.RandomState(4).permutation(R)).to(DEV)
    for cut in (0, 1, 64, R):
        fused = fresh(grid).add(rays[:cut], depth[:cut], frame).add(rays[cut:], depth[cut:], frame)
        assert torch.equal(fused.acc, two.acc) and fused.skipped == two.skipped, cut
        split = fresh(grid).add_points(point_cloud(rays[cut:], depth[cut:], frame)).add(rays[:cut], depth[:cut], frame)
        assert torch.equal(split.acc, two.acc) and split.skipped == two.skipped, cut
    shuffled = fresh(grid).add(rays[perm].contiguous(), depth[perm].contiguous(), frame)
    assert torch.equal(shuffled.acc, two.acc) and shuffled.skipped == two.skipped


@pytest.mark.parametrize("name", list(D.CASES))
def test_fused_splat_of_a_utm_scene_is_bn_dsm_splat(name):
    """cs = utm: the accumulator and skipped of bn_dsm_splat, bit for bit, on the cases of tests/dsm_cases.py; and so is the
    two-launch form."""
    from brdf_nerf_amd import _lib as L
    from brdf_nerf_amd import functions as Fn
    grid, radius, footprint, rays, depth = D.case(name)
    rays, depth = dev(rays), dev(depth)
    fp = {"disc": L.BN_DSM_DISC, "square": L.BN_DSM_SQUARE}[footprint]
    xoff, yoff, res, W, H = grid
    accs = [torch.zeros((H, W, 2), **I64) for _ in range(3)]
    sk = [torch.zeros((1,), **I64) for _ in range(4)]
    Fn.dsm_splat(rays, depth, D.CENTER, D.RANGE, xoff, yoff, res, radius, fp, accs[0], sk[0])
    Fn.dsm_splat_world(rays, depth, D.CENTER, D.RANGE, xoff, yoff, res, radius, fp, L.BN_CS_UTM, 17, 0, accs[1], sk[1])
    enz = Fn.surface_points(rays, depth, D.CENTER, D.RANGE, L.BN_CS_UTM, 17, 0, sk[3])
    Fn.dsm_splat_points(enz, xoff, yoff, res, radius, fp, accs[2], sk[2])
    assert int(accs[0][..., 1].sum()) > 0
    assert torch.equal(accs[1], accs[0]) and int(sk[1]) == int(sk[0]) == D.expected(name)["skipped"]
    assert torch.equal(accs[2], accs[0]) and int(sk[2]) == int(sk[0])
    p = D.points(rays.cpu().numpy(), depth.cpu().numpy())
    ok, got = np.isfinite(p).all(1), enz.cpu().numpy()
    assert np.array_equal(got[ok].view(np.int64), p[ok].view(np.int64)) and np.isnan(got[~ok]).all() and int(sk[3]) == int((~ok).sum())


@pytest.mark.parametrize("name", sorted(E.SITES))
def test_dsm_of_the_golden_rays_against_the_float64_statement(name):
    """The 257 golden rays splatted at 0.5 m: the counts of the statement, and every cell's mean altitude within 2e-6 m (a
    deposit llrint(alt 2^20) may differ by one unit where the device's altitude differs by up to 1e-6 m)."""
    from brdf_nerf_amd import Grid
    from brdf_nerf_amd.dsm import _cloud_grid
    frame = ecef_frame(name)
    rays, depth = site_inputs(name)
    st = E.site_statement(name)
    grid = E.cloud_grid(st["enz"])
    assert _cloud_grid(rays, depth, frame, E.RESOLUTION) == Grid(*grid)
    sums, counts, skipped = E.splat_points(st["enz"], grid, 1, "disc")
    acc = fresh(grid).add(rays, depth, frame)
    got = acc.acc.cpu().numpy()
    want = E.acc_int64(sums, counts)
    assert acc.skipped == skipped == 0 and np.array_equal(got[..., 1], want[..., 1]) and 4 * E.N_RAYS < int(want[..., 1].sum()) <= 5 * E.N_RAYS
    filled = want[..., 1] > 0
    gap = np.abs((got[..., 0][filled] - want[..., 0][filled]) / want[..., 1][filled]).max() / D.FIX
    print(f"{name}: grid {grid[3]} x {grid[4]}, {int(filled.sum())} cells filled, mean altitude off by at most {gap:.2e} m")
    assert gap <= 2e-6
    dsm, count = acc.result()
    assert np.array_equal(count.cpu().numpy(), want[..., 1].astype(np.int32)) and bool(torch.isfinite(dsm[count > 0]).all())


def test_skipped_points():
    """A point on the axis, a NaN and an inf coordinate: counted, NaN rows, nothing deposited."""
    from brdf_nerf_amd import SceneFrame, point_cloud
    from brdf_nerf_amd import _lib as L
    from brdf_nerf_amd import functions as Fn
    from brdf_nerf_amd.camera import ecef_geodetic
    frame = SceneFrame((0.0, 0.0, 0.0), 1.0e6, cs="ecef", zone=37)
    rays = torch.zeros((70, 8), device=DEV)
    rays[:, 0], rays[:, 1], rays[:, 2], rays[:, 5] = 4.03, 3.02, 3.9, -1.0          # about (4.03e6, 3.02e6, 3.9e6) m: an ordinary point
    depth = torch.zeros((70,), device=DEV)
    rays[3, 0] = rays[3, 1] = 0.0                                                     # on the axis
    depth[40], depth[66] = float("nan"), float("inf")
    rays[67, 1] = float("-inf")
    bad = [3, 40, 66, 67]
    skipped = torch.zeros((1,), **I64)
    enz = Fn.surface_points(rays, depth, frame.center, frame.range, L.BN_CS_ECEF, 37, 0, skipped)
    good = torch.ones(70, dtype=torch.bool, device=DEV)
    good[bad] = False
    assert int(skipped) == 4 and bool(torch.isnan(enz[~good]).all()) and bool(torch.isfinite(enz[good]).all())
    assert torch.equal(point_cloud(rays, depth, frame)[good], enz[good])
    ref = E.world_enz(D.points(rays[:1].cpu().numpy(), depth[:1].cpu().numpy(), frame.center, frame.range), "ecef", 37, False)[0]
    assert abs(ref[0, 2]) < 2.0e4 and 1.0e5 < ref[0, 0] < 9.0e5
    assert np.abs(enz[good].cpu().numpy() - ref).max() <= 1e-6
    grid = E.cloud_grid(ref, 0.5)
    acc = fresh(grid, radius=0).add(rays, depth, frame)
    assert acc.skipped == 4 and int(acc.acc[..., 1].sum()) == 66
    only_bad = fresh(grid, radius=4, footprint="square").add(rays[bad].contiguous(), depth[bad].contiguous(), frame)
    assert only_bad.skipped == 4 and int(only_bad.acc.abs().sum()) == 0
    xyz = torch.tensor([[0.0, 0.0, 6.4e6], [float("nan"), 1.0, 2.0], [1.0, 2.0, float("inf")], [4.0e6, 3.0e6, 3.9e6]], dtype=torch.float64)
    lonlat, alt, n = ecef_geodetic(xyz, device=DEV, want_skipped=True)
    assert n == 3 and bool(torch.isnan(lonlat[:3]).all()) and bool(torch.isnan(alt[:3]).all()) and bool(torch.isfinite(lonlat[3]).all())


def test_refusals():
    """BN_EINVAL, not a launch."""
    import ctypes as C
    from brdf_nerf_amd import _lib as L
    lib = L.lib()
    rays, depth = torch.zeros(4, 8, device=DEV), torch.ones(4, device=DEV)
    enz = torch.zeros(4, 3, dtype=torch.float64, device=DEV)
    acc, skipped = torch.zeros(5, 7, 2, **I64), torch.zeros(1, **I64)
    c = (C.c_double * 3)(0.0, 0.0, 0.0)
    p = lambda t: C.c_void_p(t.data_ptr())

    def world(cs=L.BN_CS_UTM, zone=17, south=0, radius=1, res=0.5, stride=8, acc_p=p(acc)):
        return lib.bn_dsm_splat_world(p(rays), stride, p(depth), 4, c, 1.0, -100.0, 100.0, res, 7, 5, radius, 0, cs, zone, south, acc_p, p(skipped), None)

    def points(stride=3, radius=1, fp=0, n=4, enz_p=p(enz)):
        return lib.bn_dsm_splat_points(enz_p, stride, n, -100.0, 100.0, 0.5, 7, 5, radius, fp, p(acc), p(skipped), None)

    def surface(cs=L.BN_CS_ECEF, zone=17, south=0, stride=8, out=p(enz)):
        return lib.bn_surface_points(p(rays), stride, p(depth), 4, c, 1.0, cs, zone, south, out, p(skipped), None)

    assert world() == 0 and points() == 0
    for kw in (dict(cs=2), dict(zone=0), dict(zone=61), dict(south=2), dict(radius=5), dict(res=0.0), dict(stride=5), dict(acc_p=None)):
        assert world(**kw) == -1 and b"dsm_splat_world" in lib.bn_last_error(), kw
    for kw in (dict(stride=2), dict(radius=-1), dict(fp=2), dict(n=-1), dict(enz_p=None)):
        assert points(**kw) == -1 and b"dsm_splat_points" in lib.bn_last_error(), kw
    for kw in (dict(cs=-1), dict(zone=0), dict(south=-1), dict(stride=5), dict(out=None)):
        assert surface(**kw) == -1 and b"surface_points" in lib.bn_last_error(), kw
    assert lib.bn_ecef_geodetic(None, 4, p(enz), p(enz), p(skipped), None) == -1 and lib.bn_ecef_geodetic(p(enz), -1, p(enz), p(enz), p(skipped), None) == -1
    torch.cuda.synchronize()
    assert int(acc.abs().sum()) == 0 and int(skipped) == 0                # (0, 0, 0) + (0, 0, 1): far outside the grid, and finite


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_a_view_of_an_ecef_scene_end_to_end():
    """A 12 x 10 view: view_rays(cs='ecef') with SceneFrame.ecef in place of center and range, a small RPV model, then dsm_image,
    score_view(frame=, gt_dsm=) and view_maps(frame=).  depth is render_image's bit for bit; the DSM splatted chunk by chunk (50, 50
    and 20 rays) is the DSM of those depths splatted in one call, bit for bit."""
    from brdf_nerf_amd import Rpc, SceneFrame, altitude_image, dsm_image, score_view, view_maps, view_rays
    from brdf_nerf_amd.evaluate import render_image
    from test_gpu_relight import build, flags
    H, W = 10, 12
    site = "z17"
    lo, hi = M.alt_bounds(site)
    center, rng = E.site_frame("z17")
    frame = SceneFrame.ecef(center, rng)
    assert frame.zone == 17
    rpc = Rpc.from_dict(M.make_rpc(site, 31))
    rays, skipped = view_rays(rpc, H, W, lo, hi, frame, cs="ecef", sun=M.SUN, precision="exact", device=DEV)
    same, _ = view_rays(rpc, H, W, lo, hi, center, rng, cs="ecef", sun=M.SUN, precision="exact", device=DEV)
    assert skipped == 0 and tuple(rays.shape) == (H * W, 11) and torch.equal(rays, same)
    cfg, args, models, _ = build("rpv111")
    fl, cosi = flags("rpv111")
    kw = dict(chunk=50, cos_irra_on=cosi, **fl)
    torch.manual_seed(31)
    ref = render_image(models, args, rays, **kw)
    torch.manual_seed(31)
    got = dsm_image(models, args, rays, frame, fill=True, **kw)
    assert torch.equal(got["depth"], ref["depth"])
    grid = got["grid"]
    alt = altitude_image(rays, ref["depth"], frame)
    assert torch.equal(got["altitude"], alt) and bool(torch.isfinite(alt).all()) and got["skipped"] == 0
    assert bool(torch.isfinite(got["dsm"][got["count"] > 0]).all()) and int((got["count"] > 0).sum()) > 0
    assert bool(torch.isfinite(got["dsm_grid"]).all())
    one = fresh((grid.xoff, grid.yoff, grid.resolution, grid.width, grid.height)).add(rays, ref["depth"], frame)
    torch.manual_seed(31)
    chunked = dsm_image(models, args, rays, frame, grid=grid, **kw)                  # splatted as the chunks of 50 are rendered
    for res in (got, chunked):
        assert torch.equal(res["dsm"].view(torch.int32), one.result()[0].view(torch.int32)) and torch.equal(res["count"], one.result()[1])
    gt, rgbs = got["dsm_grid"] + 0.25, torch.rand(H * W, 3, device=DEV)
    torch.manual_seed(31)
    sc = score_view(models, args, rays, rgbs, H, W, frame=frame, gt_dsm=gt, grid=grid, **kw)
    assert torch.equal(sc["depth"], ref["depth"]) and torch.equal(sc["dsm"].view(torch.int32), got["dsm"].view(torch.int32))
    assert np.isfinite(sc["mae"]) and sc["mae"] < 1e-3 and abs(sc["shift"] - 0.25) < 1e-3 and np.isfinite(sc["psnr"])
    torch.manual_seed(31)
    vm = view_maps(models, args, rays, H, W, frame=frame, **kw)["maps"]
    assert torch.equal(vm["depth"], ref["depth"]) and torch.equal(vm["altitude"], alt.float())
    assert tuple(vm["nr_from_depth"].shape) == (H * W, 3) and bool(torch.isfinite(vm["nr_from_depth"]).all())


def test_two_rank_ecef_dsm_matches_one_rank():
    """World 2: two ranks on cuda:0 over gloo (tests/dist_ecef_worker.py), each child under its own time limit and started once."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dist_ecef_worker.py")
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


# ---------------------------------------------------------------------------------------------------------------- tie points
def tie_points(name):
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
    return g["pts3d_mm"] / 1000.0


def test_tie_point_dsm_of_an_ecef_view():
    """The *_3DPts_ecef.txt content of the z38 priors fixture: the DSM equals, bit for bit, the integer statement applied to the
    device's own converted points; those are within 1e-6 m of the statement; the filled grid has no NaN."""
    from brdf_nerf_amd import altitude_mae, tie_point_dsm
    pts = tie_points("priors_z38_ecef")
    res = tie_point_dsm(dev(pts), cs="ecef", zone=38, resolution=2.0)
    enz = res["points"].cpu().numpy()
    want, bad = E.world_enz(pts, "ecef", 38, False)
    assert not bad.any() and np.abs(enz - want).max() <= 1e-6
    g = res["grid"]
    grid = (g.xoff, g.yoff, g.resolution, g.width, g.height)
    assert grid == E.cloud_grid(enz, 2.0) and g.width * g.height < 200000
    sums, counts, skipped = E.splat_points(enz, grid, 1, "disc")
    dsm, count = D.resolve(sums, counts)
    assert res["skipped"] == skipped == 0
    assert np.array_equal(res["count"].cpu().numpy(), count) and np.array_equal(res["dsm"].cpu().numpy().view(np.int32), dsm.view(np.int32))
    assert res["holes"] == int(np.isnan(dsm).sum()) > 0 and bool(torch.isfinite(res["dsm_grid"]).all())
    assert altitude_mae(res["dsm"], res["dsm_grid"])["mae"] == 0.0          # goes straight into the MAE: the filled grid keeps the known cells
    with pytest.raises(NotImplementedError, match="ecef"):
        tie_point_dsm(dev(pts), cs="ecef")


def test_tie_point_dsm_of_a_utm_view():
    from brdf_nerf_amd import tie_point_dsm
    pts = tie_points("priors_z17_utm")
    res = tie_point_dsm(dev(pts), cs="utm")
    assert np.array_equal(res["points"].cpu().numpy(), pts)
    g = res["grid"]
    grid = (g.xoff, g.yoff, g.resolution, g.width, g.height)
    assert grid == E.cloud_grid(pts, 0.5) and g.width * g.height < 400000
    sums, counts, skipped = E.splat_points(pts, grid, 1, "disc")
    assert res["skipped"] == skipped == 0
    nz = np.nonzero(D.as_int64(counts))
    got = fresh(grid).add_points(dev(pts)).acc.cpu().numpy()
    assert np.array_equal(got[..., 0][nz], D.as_int64(sums)[nz]) and np.array_equal(got[..., 1], D.as_int64(counts))
    assert np.array_equal(res["count"].cpu().numpy(), D.as_int64(counts).astype(np.int32))
    filled = res["count"] > 0
    want = (D.as_int64(sums)[nz] / D.as_int64(counts)[nz] * (1.0 / D.FIX)).astype(np.float32)
    assert np.array_equal(res["dsm"][filled].cpu().numpy().view(np.int32), want.view(np.int32))
    assert bool(torch.isfinite(res["dsm_grid"]).all()) and res["holes"] == int((~filled).sum())
    no_fill = tie_point_dsm(dev(pts), cs="utm", grid=g, fill=False)
    assert "dsm_grid" not in no_fill and torch.equal(no_fill["count"], res["count"])
