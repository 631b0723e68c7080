"""The numpy statement of "World points of an ECEF scene" (include/brdfnerf_hip.h), the Python-integer splat of world points, and
the inputs of tests/test_ecef_cpu.py, tests/test_gpu_ecef.py and tests/golden/make_ecef_goldens.py.

The statement is the header's rule written with np.float64 scalars and array expressions, one ufunc per operation, so every
operation is rounded on its own.  It shares no code with brdf_nerf_amd or the kernels.  The UTM series and the surface point are
the statements of tests/camera_cases.py and tests/dsm_cases.py, imported.

  ecef_geodetic    (x, y, z) -> lon_deg, lat_deg, alt, refused
  world_enz        a world point of a scene -> (east, north, altitude), NaN where refused
  surface_points   rays, depth, frame -> (east, north, altitude) of bn_surface_points
  splat_points     (east, north, altitude) -> Python-integer sums and counts, skipped: the cell, footprint and deposit of the DSM

The sites are the three of camera_cases, zone 21 with both `south` settings.  A site's rays are 257 pixels of a synthetic RPC
image of the site, made by camera_cases.rays with cs='ecef' in a frame whose centre is the float32 of the site's ECEF position
(upstream keeps its centre in a float32 tensor), with depths that put the surface points between min_alt and max_alt.
"""
import functools
import os

import numpy as np

import camera_cases as M
import dsm_cases as D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ecef.npz")
M_PER_DEG = 111320.0                        # metres per degree: how a difference in degrees is stated in metres
RANGE = 160.0
N_RAYS = 257
N_FREE = 64
RESOLUTION = 0.5
EDGE_MARGIN = 1e-4                          # metres between every golden east / north and the nearest cell edge

# name: (site of camera_cases, south)
SITES = {"z38": ("z38", False), "z17": ("z17", False), "z21n": ("z21", False), "z21s": ("z21", True)}


def zone_of(name):
    return M.SITES[SITES[name][0]][2]


# ---------------------------------------------------------------------------------------------------------------- the rule
def constants():
    """a, b, esq, k1, k2 as upstream forms them (sat_utils.py:131-137), squares as products."""
    a = np.float64(6378137.0)
    e = np.float64(8.1819190842622e-2)
    asq = a * a
    esq = e * e
    b = np.sqrt(asq * (np.float64(1.0) - esq))
    bsq = b * b
    ep = np.sqrt((asq - bsq) / bsq)
    return a, b, esq, (ep * ep) * b, esq * a


def ecef_geodetic(x, y, z, esq_from_f=False, alt_from_z=False):
    """-> lon_deg, lat_deg, alt (float64 arrays, as computed), refused (bool).  esq_from_f / alt_from_z: the two perturbations
    the tests must catch (e2 = 1 - (1 - f)^2 in place of the truncated e; alt = z / sin(lat) - N (1 - esq))."""
    x, y, z = (np.asarray(v, np.float64) for v in (x, y, z))
    a, b, esq, k1, k2 = constants()
    if esq_from_f:
        f = np.float64(1.0) / np.float64(298.257223563)
        esq = np.float64(1.0) - (np.float64(1.0) - f) * (np.float64(1.0) - f)
        b = np.sqrt((a * a) * (np.float64(1.0) - esq))
        ep = np.sqrt((a * a - b * b) / (b * b))
        k1, k2 = (ep * ep) * b, esq * a
    with np.errstate(all="ignore"):
        p = np.sqrt(x * x + y * y)
        th = np.arctan2(a * z, b * p)
        s, c = np.sin(th), np.cos(th)
        lon = np.arctan2(y, x)
        lat = np.arctan2(z + k1 * ((s * s) * s), p - k2 * ((c * c) * c))
        sl = np.sin(lat)
        N = a / np.sqrt(np.float64(1.0) - esq * (sl * sl))
        alt = z / sl - N * (np.float64(1.0) - esq) if alt_from_z else p / np.cos(lat) - N
        lon_deg = lon * np.float64(180.0) / np.pi
        lat_deg = lat * np.float64(180.0) / np.pi
    bad = (p == 0.0) | ~(np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & np.isfinite(lat) & np.isfinite(alt))
    return lon_deg, lat_deg, alt, bad


def world_enz(xyz, cs, zone=None, south=False, **perturb):
    """World points (n, 3) of a `cs` scene -> (east, north, altitude) float64 (n, 3), NaN rows where refused, refused (bool)."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    if cs == "utm":
        bad = ~np.isfinite(xyz).all(1)
        out = xyz.copy()
    else:
        lon, lat, alt, bad = ecef_geodetic(xyz[:, 0], xyz[:, 1], xyz[:, 2], **perturb)
        with np.errstate(all="ignore"):
            east, north = M.utm(lon, lat, zone, south)
        bad = bad | ~(np.isfinite(east) & np.isfinite(north))
        out = np.stack([east, north, alt], -1)
    out[bad] = np.nan
    return out, bad


def surface_points(rays, depth, center, rng, cs, zone=None, south=False, **perturb):
    """bn_surface_points: -> enz (R, 3) float64, skipped."""
    enz, bad = world_enz(D.points(rays, depth, center, rng), cs, zone, south, **perturb)
    return enz, int(bad.sum())


def splat_points(enz, grid, radius, footprint, acc=None):
    """The DSM deposit of given (east, north, altitude) rows -> (sums, counts) object arrays of Python ints (H, W), skipped.
    grid = (xoff, yoff, res, W, H); acc: an earlier result that is added to."""
    xoff, yoff, res, W, H = grid
    xoff, yoff, res = np.float64(xoff), np.float64(yoff), np.float64(res)
    if acc is None:
        sums, counts, skipped = np.zeros((H, W), dtype=object), np.zeros((H, W), dtype=object), 0
    else:
        sums, counts, skipped = acc[0].copy(), acc[1].copy(), acc[2]
    for px, py, pz in np.asarray(enz, np.float64).reshape(-1, 3):
        if not (np.isfinite(px) and np.isfinite(py) and np.isfinite(pz)) or not abs(pz) < D.ZMAX:
            skipped += 1
            continue
        fi, fj = np.floor((px - xoff) / res), np.floor((yoff - py) / res)
        if not (-radius <= fi <= W - 1 + radius and -radius <= fj <= H - 1 + radius):
            continue
        i, j = int(fi), int(fj)
        q = int(np.rint(pz * D.FIX))
        for k2 in range(-radius, radius + 1):
            for k1 in range(-radius, radius + 1):
                row, col = j + k2, i + k1
                if not (0 <= row < H and 0 <= col < W):
                    continue
                if footprint == "disc" and k1 * k1 + k2 * k2 > radius * radius:
                    continue
                sums[row, col] += q
                counts[row, col] += 1
    return sums, counts, skipped


def acc_int64(sums, counts):
    """(H, W, 2) int64 = (sum, count), the layout of the device accumulator."""
    return np.stack([D.as_int64(sums), D.as_int64(counts)], -1)


def cloud_grid(enz, res=RESOLUTION):
    """Grid.from_cloud (datasets/satellite_rgb_dep.py:665-671) of the finite rows -> (xoff, yoff, res, W, H)."""
    xy = enz[np.isfinite(enz).all(1)][:, :2]
    (xmin, ymin), (xmax, ymax) = xy.min(0), xy.max(0)
    xoff = np.floor(xmin / res) * res
    yoff = np.ceil(ymax / res) * res
    return float(xoff), float(yoff), float(res), int(1 + np.floor((xmax - xoff) / res)), int(1 - np.floor((ymin - yoff) / res))


# ---------------------------------------------------------------------------------------------------------------- inputs
def make_site_frame(name):
    """The generator's: (center (3 floats, float32-representable), range) of a site's ECEF frame."""
    lat, lon, _, alt = M.SITES[SITES[name][0]]
    c = np.array(M.ecef(lon, lat, alt), np.float64).astype(np.float32).astype(np.float64)
    return tuple(float(v) for v in c), RANGE


def edge_distance(v, res=RESOLUTION):
    """Metres from v to the nearest multiple of res."""
    q = np.asarray(v, np.float64) / res
    return np.abs(q - np.rint(q)) * res


def make_site_rays(name):
    """The generator's: -> rays (257, 8) float32, depth (257,) float32 of a site: a 17-column block of pixels around the image's centre, depths
    between 5 % and 95 % of the ray, redrawn until every east and north keeps EDGE_MARGIN from the cell edges of a 0.5 m grid
    (a condition on the inputs: the device's points differ from the statement's by up to 1e-6 m)."""
    site, south = SITES[name]
    zone = M.SITES[site][2]
    lo, hi = M.alt_bounds(site)
    center, rng = make_site_frame(name)
    k = np.arange(N_RAYS)
    cols, rows = 504.0 + (k % 17), 504.0 + (k // 17)
    rays = M.rays(M.make_rpc(site, 900 + sorted(SITES).index(name)), cols, rows, lo, hi, "ecef", None, False, center, rng,
                  precision="exact")["rays"]
    assert np.isfinite(rays).all()
    g = np.random.default_rng(77 + sorted(SITES).index(name))
    depth = (rays[:, 7] * g.uniform(0.05, 0.95, N_RAYS)).astype(np.float32)
    for _ in range(200):
        enz, skipped = surface_points(rays, depth, center, rng, "ecef", zone, south)
        assert skipped == 0
        near = (edge_distance(enz[:, 0]) < EDGE_MARGIN) | (edge_distance(enz[:, 1]) < EDGE_MARGIN)
        if not near.any():
            break
        depth[near] = (rays[near, 7] * g.uniform(0.05, 0.95, int(near.sum()))).astype(np.float32)
    else:
        raise AssertionError(f"{name}: the depths could not be drawn clear of the cell edges")
    return rays, depth


def make_free_points():
    """64 ECEF points with |lat| up to 80 degrees, any longitude, altitudes -400 to 9000 m -> xyz (64, 3), zone (64,) int."""
    g = np.random.default_rng(5)
    lat = np.concatenate([[-80.0, 80.0, 0.0, 1e-9], g.uniform(-80.0, 80.0, N_FREE - 4)])
    lon = np.concatenate([[-179.5, 179.5, 0.0, 90.0], g.uniform(-180.0, 180.0, N_FREE - 4)])
    alt = np.concatenate([[-400.0, 9000.0, 0.0, 0.0], g.uniform(-400.0, 9000.0, N_FREE - 4)])
    xyz = np.stack(M.ecef(lon, lat, alt), -1)
    zone = np.minimum((np.floor((lon + 180.0) / 6.0) + 1).astype(np.int64), 60)
    return xyz, zone, np.stack([lon, lat, alt], -1)


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        out = {k: z[k] for k in z.files}
    for v in out.values():
        v.setflags(write=False)
    return out


def site_rays(name):
    """The golden inputs of a site: rays (257, 8) float32, depth (257,) float32."""
    g = golden()
    return g[name + "_rays"], g[name + "_depth"]


def site_frame(name):
    """The golden frame of a site: (center (3 floats), range)."""
    return tuple(float(v) for v in golden()[name + "_center"]), RANGE


@functools.lru_cache(maxsize=None)
def site_statement(name):
    """The statement on a site's golden rays, computed once: enz (257, 3), lon, lat (degrees)."""
    site, south = SITES[name]
    rays, depth = site_rays(name)
    center, rng = site_frame(name)
    p = D.points(rays, depth, center, rng)
    lon, lat, alt, bad = ecef_geodetic(p[:, 0], p[:, 1], p[:, 2])
    enz, bad2 = world_enz(p, "ecef", M.SITES[site][2], south)
    assert not bad.any() and not bad2.any()
    for v in (enz, lon, lat):
        v.setflags(write=False)
    return {"enz": enz, "lon": lon, "lat": lat, "xyz": p}
