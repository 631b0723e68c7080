"""CPU tests of the camera geometry: the numpy statement (tests/camera_cases.py) against the goldens recorded from the reference
and against independent formulas, and the host side of brdf_nerf_amd/camera.py (descriptor, zone rule, refusals).  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import camera_cases as M
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
ENTRIES = ("bn_rpc_project", "bn_rpc_localize", "bn_geo_world", "bn_rpc_rays")


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def test_entries_are_declared_bound_and_exported():
    import brdf_nerf_amd
    from brdf_nerf_amd import _lib
    header = open(os.path.join(ROOT, "include", "brdfnerf_hip.h")).read()
    declared = set(re.findall(r"\b(bn_[a-z0-9_]+)\s*\(", header))
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in declared and name in _lib._SIGS and hasattr(raw, name), name
    assert C.sizeof(_lib.Rpc) == 90 * 8 and _lib.BN_RPC_NEWTON_ITERS == M.NEWTON_ITERS == 8
    assert re.search(r"#define BN_RPC_NEWTON_ITERS 8\b", header)
    for name in ("camera", "Rpc", "view_rays", "scene_bounds", "ray_table", "utm_zone", "sun_direction"):
        assert name in brdf_nerf_amd.__all__ and hasattr(brdf_nerf_amd, name), name
    from brdf_nerf_amd.build import FILE_FLAGS
    assert "-ffp-contract=off" in FILE_FLAGS["camera.hip"]


def test_descriptor_from_dict_and_downscale():
    """The 90 doubles in the header's order; downscale multiplies the four image scales and offsets by float(1 / downscale)."""
    from brdf_nerf_amd.camera import Rpc
    d = M.make_rpc("z17", 4)
    for ds in (1.0, 2.0, 3.0):
        rpc = Rpc.from_dict(d, ds)
        got = np.frombuffer(bytes(rpc.struct), dtype=np.float64)
        assert np.array_equal(got, M.flat(M.rescaled(d, ds)))
    as_text = dict(d, row_num=", ".join(repr(v) for v in d["row_num"]))
    assert Rpc.from_dict(as_text).row_num == d["row_num"]


def test_zone_rule_with_its_exceptions():
    from brdf_nerf_amd.camera import utm_zone
    for lat, lon, zone in M.ZONE_TABLE:
        assert utm_zone(lat, lon) == zone, (lat, lon)
    for lat, lon in ((91.0, 0.0), (0.0, 181.0), (float("nan"), 0.0)):
        with pytest.raises(ValueError, match="utm_zone"):
            utm_zone(lat, lon)


def test_sun_direction_is_the_statements():
    from brdf_nerf_amd.camera import sun_direction
    for el, az in ((38.5, 141.0), (90.0, 0.0), (12.25, 359.5)):
        assert np.array_equal(bits(sun_direction(el, az)), bits(M.sun_direction(el, az)))


@pytest.mark.parametrize("site", sorted(M.SITES))
def test_round_trip_of_the_statement(site):
    """project(localize(col, row, alt), alt) == (col, row) within 1e-9 px, and the inputs meet the generator's conditions."""
    _, _, zone, _ = M.SITES[site]
    lo, hi = M.alt_bounds(site)
    d = M.make_rpc(site, 3)
    M.check_rpc(d, 65, 33, lo, hi, "utm", zone, False)
    cols, rows = M.grid_pixels(65, 33)
    for alt in (lo, hi):
        lon, lat, bad = M.localize(d, cols, rows, alt)
        c, r = M.project(d, lon, lat, alt)
        err = max(np.abs(c - cols).max(), np.abs(r - rows).max())
        print(f"{site} alt {alt}: round trip {err:.3e} px")
        assert not bad.any() and err <= 1e-9


def test_zero_determinant_and_non_finite_pixels_are_counted():
    d = M.singular_rpc()
    lon, lat, bad = M.localize(d, [1.0, 2.0], [3.0, 4.0], 10.0)
    assert bad.all() and np.isnan(lon).all() and np.isnan(lat).all()
    lon, lat, bad = M.localize(M.make_rpc("z38", 3), [1.0, np.nan, np.inf, 4.0], [1.0, 2.0, 3.0, -np.inf], 10.0)
    assert bad.tolist() == [False, True, True, True] and np.isfinite(lon[0])


def test_utm_on_the_central_meridian_is_the_meridian_arc():
    """Easting 500000 exactly; northing = k0 x the arc by numerical quadrature within 1e-6 m (measured: 2.8e-9 m)."""
    from scipy.integrate import quad
    worst = 0.0
    for lat in (5.0, 11.6, 30.3, 45.0, 60.0, 70.0):
        arc = quad(M.meridian_integrand, 0.0, np.radians(lat), epsabs=1e-10, epsrel=1e-13, limit=200)[0]
        x, y = M.utm(np.array([-81.0]), np.array([lat]), 17)
        xs, ys = M.utm(np.array([-81.0]), np.array([-lat]), 17, south=True)
        assert x[0] == 500000.0 and xs[0] == 500000.0
        worst = max(worst, abs(y[0] - M.K0 * arc), abs(ys[0] - (10000000.0 - M.K0 * arc)))
    print(f"meridian arc: {worst:.3e} m")
    assert worst <= 1e-6


def test_utm_off_the_meridian_against_snyders_series():
    """200 random points, |lat| <= 60, |dlon| <= 3 degrees: within 1e-3 m of Snyder's truncated series (measured: 7.3e-5 m east,
    3.2e-6 m north; 5.8e-11 m east within |dlon| <= 0.2 degrees)."""
    rng = np.random.default_rng(0)
    lat, dl = rng.uniform(-60, 60, 200), rng.uniform(-3, 3, 200)
    for zone in (17, 38):
        lon0 = 6.0 * zone - 183.0
        x, y = M.utm(lon0 + dl, lat, zone)
        xs, ys = M.snyder_utm(lon0 + dl, lat, zone)
        print(f"zone {zone}: east {np.abs(x - xs).max():.3e} m north {np.abs(y - ys).max():.3e} m")
        assert np.abs(x - xs).max() <= 1e-3 and np.abs(y - ys).max() <= 1e-3


@pytest.mark.parametrize("name", sorted(M.GOLDENS))
def test_statement_reproduces_the_reference(name):
    """precision='reference': the reference's rays (get_rays, normalize_rays, get_sun_dirs) and scene.loc, bit for bit."""
    site, cs, south, ds = M.GOLDENS[name]
    zone = M.SITES[site][2]
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    raw = []
    for i, v in enumerate(M.golden_views(name)):
        d = M.rescaled(v["rpc"], ds)
        c, r = M.grid_pixels(v["H"], v["W"])
        got = M.rays(d, c, r, v["min_alt"], v["max_alt"], cs, zone, south, g["center"], float(g["range"]), M.sun_direction(*v["sun"]))
        assert got["skipped"] == 0 and np.array_equal(bits(got["rays"]), bits(g[f"rays{i}"])), (name, i)
        raw.append(M.rays(d, c, r, v["min_alt"], v["max_alt"], cs, zone, south, (0.0, 0.0, 0.0), 1.0)["rays"])
    loc = M.scene_loc(raw)
    assert [loc[k] for k in ("X_scale", "X_offset", "Y_scale", "Y_offset", "Z_scale", "Z_offset")] == g["loc"].tolist()
    assert max(loc["X_scale"], loc["Y_scale"], loc["Z_scale"]) == float(g["range"])


def test_float32_world_origins_lose_a_quarter_metre_at_zone_17():
    """The defect: at a northing of 3.35e6 m the 'reference' origins sit on a 0.25 m lattice - up to 0.125 m from the 'exact' ones."""
    name = "camera_z17_utm_d1"
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    v = M.golden_views(name)[1]
    c, r = M.grid_pixels(v["H"], v["W"])
    args = (v["rpc"], c, r, v["min_alt"], v["max_alt"], "utm", 17, False, g["center"], float(g["range"]))
    ref, exact = M.rays(*args, precision="reference"), M.rays(*args, precision="exact")
    gap = np.abs(ref["rays"][:, :3].astype(np.float64) - exact["rays"][:, :3].astype(np.float64)).max(0) * float(g["range"])
    print(f"reference - exact origins, metres: {gap}")
    assert 0.1 < gap[1] <= 0.125 + 1e-3 and gap[0] <= 0.03125 / 2 + 1e-3


def test_refusals_by_name():
    from brdf_nerf_amd import SceneFrame
    from brdf_nerf_amd.camera import Rpc, view_rays, scene_bounds, geo_world
    d = M.make_rpc("z38", 3)
    rpc = Rpc.from_dict(d)
    ok = dict(center=(0.0, 0.0, 0.0), range=1.0, device="cpu")
    with pytest.raises(ValueError, match="scale"):
        Rpc.from_dict(dict(d, lon_scale=0.0))
    with pytest.raises(ValueError, match="non-finite"):
        Rpc.from_dict(dict(d, alt_offset=float("inf")))
    with pytest.raises(ValueError, match="20"):
        Rpc.from_dict(dict(d, col_den=[1.0] * 19))
    with pytest.raises(ValueError, match="missing"):
        Rpc.from_dict({k: v for k, v in d.items() if k != "row_num"})
    with pytest.raises(ValueError, match="downscale"):
        Rpc.from_dict(d, 0.0)
    with pytest.raises(ValueError, match="precision"):
        view_rays(rpc, 3, 5, 0.0, 10.0, precision="float16", **ok)
    with pytest.raises(ValueError, match="coordinate system"):
        view_rays(rpc, 3, 5, 0.0, 10.0, cs="enu", **ok)
    with pytest.raises(ValueError, match="zone"):
        view_rays(rpc, 3, 5, 0.0, 10.0, zone=61, **ok)
    with pytest.raises(ValueError, match="zone"):
        geo_world(np.zeros((1, 2)), 0.0, cs="utm", device="cpu")
    with pytest.raises(ValueError, match="range"):
        view_rays(rpc, 3, 5, 0.0, 10.0, (0.0, 0.0, 0.0), 0.0, device="cpu")
    with pytest.raises(ValueError, match="range"):
        view_rays(rpc, 3, 5, 0.0, 10.0, (0.0, 0.0, 0.0), float("inf"), device="cpu")
    with pytest.raises(ValueError, match="center"):
        view_rays(rpc, 3, 5, 0.0, 10.0, (0.0, float("nan"), 0.0), 1.0, device="cpu")
    with pytest.raises(ValueError, match="pixels"):
        view_rays(rpc, 3, 0, 0.0, 10.0, **ok)
    with pytest.raises(ValueError, match="altitudes"):
        view_rays(rpc, 3, 5, float("nan"), 10.0, **ok)
    with pytest.raises(ValueError, match="together"):
        view_rays(rpc, 3, 5, 0.0, 10.0, rows=np.zeros(4), **ok)
    with pytest.raises(ValueError, match="span"):
        view_rays(rpc, 3, 5, 0.0, 10.0, span=(4, 16), **ok)
    with pytest.raises(ValueError, match="SceneFrame"):
        view_rays(rpc, 3, 5, 0.0, 10.0, SceneFrame((0.0, 0.0, 0.0), 1.0), cs="ecef", device="cpu")
    with pytest.raises(ValueError, match="no views"):
        scene_bounds([])
    with pytest.raises(NotImplementedError):
        SceneFrame((0.0, 0.0, 0.0), 1.0, cs="ecef")          # the DSM's frame keeps refusing it; the camera carries its own cs


def test_library_refuses_bad_arguments_without_a_launch():
    """BN_EINVAL before anything touches a device: null pointers, r0 > r1, too many rays, W < 1, cs, zone, range, centre, scale."""
    from brdf_nerf_amd import _lib
    from brdf_nerf_amd.camera import Rpc
    lib = _lib.lib()
    rpc = Rpc.from_dict(M.make_rpc("z38", 3))
    p = C.c_void_p(4096)                                     # never dereferenced: every call below is refused on the host
    c3 = (C.c_double * 3)(0.0, 0.0, 0.0)

    def rays(rpc_ref=rpc.ref(), cols=None, rows=None, W=5, r0=0, r1=15, lo=0.0, hi=10.0, cs=_lib.BN_CS_UTM, zone=38, south=0, center=c3,
             rng=1.0, sun=None, f32=1, out=p, stride=8, counts=p):
        return lib.bn_rpc_rays(rpc_ref, cols, rows, W, r0, r1, lo, hi, cs, zone, south, center, rng, sun, f32, out, stride, None, None,
                               counts, None)
    bad = Rpc.from_dict(M.make_rpc("z38", 3))
    bad.struct.alt_scale = 0.0
    nan_c = (C.c_double * 3)(0.0, float("nan"), 0.0)
    sun = (C.c_float * 3)(0.0, 0.0, 1.0)
    cases = [dict(rpc_ref=None), dict(out=None), dict(counts=None), dict(center=None), dict(r0=3, r1=2), dict(r0=-1), dict(r1=(1 << 30) + 1),
             dict(W=0), dict(cols=p), dict(cs=2), dict(zone=0), dict(zone=61), dict(south=2), dict(rng=0.0), dict(rng=float("inf")),
             dict(rng=float("nan")), dict(center=nan_c), dict(rpc_ref=bad.ref()), dict(f32=2), dict(stride=7), dict(sun=sun, stride=10),
             dict(lo=float("nan"))]
    for kw in cases:
        assert rays(**kw) == -1, kw
        assert lib.bn_last_error()
    assert lib.bn_rpc_localize(rpc.ref(), None, None, 0, 0, 4, 0.0, p, p, None) == -1
    assert lib.bn_rpc_localize(rpc.ref(), None, None, 5, 4, 3, 0.0, p, p, None) == -1
    assert lib.bn_rpc_localize(rpc.ref(), None, None, 5, 0, 4, 0.0, None, p, None) == -1
    assert lib.bn_rpc_localize(bad.ref(), None, None, 5, 0, 4, 0.0, p, p, None) == -1
    assert lib.bn_rpc_project(rpc.ref(), p, p, p, -1, p, p, None) == -1
    assert lib.bn_rpc_project(rpc.ref(), p, None, p, 4, p, p, None) == -1
    assert lib.bn_geo_world(p, p, 4, 5, 17, 0, p, None) == -1
    assert lib.bn_geo_world(p, p, 4, _lib.BN_CS_UTM, 0, 0, p, None) == -1
    assert lib.bn_geo_world(p, p, -1, _lib.BN_CS_ECEF, 17, 0, p, None) == -1
    assert lib.bn_geo_world(None, p, 4, _lib.BN_CS_ECEF, 17, 0, p, None) == -1
    # nothing to do: accepted without a launch
    assert rays(r0=7, r1=7) == 0 and lib.bn_rpc_project(rpc.ref(), p, p, p, 0, p, p, None) == 0
