"""The numpy statement of the orthophoto rule (include/brdfnerf_hip.h, "Orthophoto of an observed image") and its cases.

Every function is the rule of the header written with numpy float64 arrays, one ufunc per operation, so every operation is
rounded on its own.  The statement shares no code with brdf_nerf_amd/orthophoto.py or the kernels.  The inverse UTM sums its six
terms with a sin and a cosh PER TERM - not the kernels' angle-addition recurrence - and is itself held to camera_cases.utm, the
forward series the project already holds to quadrature and to Snyder, by the round trip (tests/test_orthophoto_cpu.py).  The
polynomials are camera_cases.project, the march is visibility_cases.grid_statement.

What the device must equal BIT FOR BIT is the gather (gather below: no transcendental lies between its inputs and its outputs);
the inverse UTM and the pixels are held to bounds that the tests derive from 1e-6 m, the project's bound for world coordinates.
"""
import numpy as np

import visibility_cases as V
from camera_cases import SITES, WGS84_A, WGS84_FINV, K0, ULP, localize, make_rpc, project, utm

NEWTON_ITERS = 4
NODATA, OUTSIDE, OCCLUDED, KEPT = 0, 1, 2, 3
STATES = ("nodata", "outside", "occluded", "kept")
WORLD_BOUND = 1e-6                           # metres: the project's bound for world coordinates
GEODETIC_N = (1, 63, 64, 65, 257)
PIXEL_GRIDS = ((1, 1), (3, 5), (33, 65), (65, 33))          # (H, W)
ROW_SPLITS = (0, 1, 32)                      # and H
EDGE_IMAGES = ((1, 1), (1, 4), (2, 2), (5, 7))              # (Hi, Wi)
GATHER_IMAGES = ((1, 1), (1, 4), (2, 2), (5, 7), (33, 65))
GATHER_CHANNELS = (1, 3, 32)
CELL_CUTS = (0, 1, 64)                       # and n


# ------------------------------------------------------------------------------------------------ the inverse UTM
def utm_inverse_constants():
    """e, 1 - e^2, k0 A and beta_1..6 (Karney 2011, eq. 36) on WGS84, as written in the header."""
    f = 1.0 / WGS84_FINV
    n = f / (2.0 - f)
    n2 = n * n
    e = np.sqrt(f * (2.0 - f))
    k0A = K0 * (WGS84_A / (1.0 + n) * (1.0 + n2 / 4.0 + n2 * n2 / 64.0 + n2 * n2 * n2 / 256.0))
    beta = [n * (1 / 2 + n * (-2 / 3 + n * (37 / 96 + n * (-1 / 360 + n * (-81 / 512 + n * (96199 / 604800)))))),
            n2 * (1 / 48 + n * (1 / 15 + n * (-437 / 1440 + n * (46 / 105 + n * (-1118711 / 3870720))))),
            n2 * n * (17 / 480 + n * (-37 / 840 + n * (-209 / 4480 + n * (5569 / 90720)))),
            n2 * n2 * (4397 / 161280 + n * (-11 / 504 + n * (-830251 / 7257600))),
            n2 * n2 * n * (4583 / 161280 + n * (-108847 / 3991680)),
            n2 * n2 * n2 * (20648693 / 638668800)]
    return e, 1.0 - e * e, k0A, beta


def utm_inverse(east, north, zone, south=False, steps=None):
    """-> lon, lat in degrees (NaN where either is not finite), counted (bool).  steps: a list that receives, per Newton iteration,
    max |d tau / tau| over the points (the generator's condition)."""
    e, e2m, k0A, beta = utm_inverse_constants()
    east, north = np.broadcast_arrays(np.asarray(east, np.float64), np.asarray(north, np.float64))
    with np.errstate(all="ignore"):
        xi = (north - (10000000.0 if south else 0.0)) / k0A
        eta = (east - 500000.0) / k0A
        xip, etap = xi, eta
        for j in range(1, 7):
            xip = xip - beta[j - 1] * (np.sin((2.0 * j) * xi) * np.cosh((2.0 * j) * eta))
            etap = etap - beta[j - 1] * (np.cos((2.0 * j) * xi) * np.sinh((2.0 * j) * eta))
        sh, cx = np.sinh(etap), np.cos(xip)
        lon = (6.0 * zone - 183.0) + np.arctan2(sh, cx) * 180.0 / np.pi
        taup = np.sin(xip) / np.sqrt(sh * sh + cx * cx)
        tau = taup
        for _ in range(NEWTON_ITERS):
            r = np.sqrt(1.0 + tau * tau)
            sigma = np.sinh(e * np.arctanh(e * tau / r))
            t = tau * np.sqrt(1.0 + sigma * sigma) - sigma * r
            d = (taup - t) / np.sqrt(1.0 + t * t) * (1.0 + e2m * (tau * tau)) / (e2m * r)
            if steps is not None:
                steps.append(float(np.max(np.abs(d / tau))) if d.size else 0.0)
            tau = tau + d
        lat = np.arctan(tau) * 180.0 / np.pi
    bad = ~(np.isfinite(lon) & np.isfinite(lat))
    return np.where(bad, np.nan, lon), np.where(bad, np.nan, lat), bad


def metres_per_degree(site, south=False):
    """(metres per degree of longitude, of latitude) at a site: central differences of the FORWARD statement over 1e-3 degrees."""
    lat, lon, zone, _ = SITES[site]
    h = 1e-3
    e1, n1 = utm(np.array([lon + h, lon]), np.array([lat, lat + h]), zone, south)
    e0, n0 = utm(np.array([lon - h, lon]), np.array([lat, lat - h]), zone, south)
    d = np.hypot(e1 - e0, n1 - n0) / (2 * h)
    return float(d[0]), float(d[1])


def degree_bounds(site, south=False):
    """WORLD_BOUND carried to degrees of longitude and of latitude at a site."""
    mlon, mlat = metres_per_degree(site, south)
    return WORLD_BOUND / mlon, WORLD_BOUND / mlat


def pixel_bound(d, site, south=False):
    """WORLD_BOUND carried to pixels through the RPC scales of the image d: a displacement of 1e-6 m moves L by at most dL = 1e-6 /
    (lon_scale metres per degree) and P by dP likewise; a pixel coordinate is scale x (a ratio of polynomials whose linear part
    has coefficients 1 and |rot| <= 0.05, every other coefficient at most 1e-3 (0.1 on the altitude, which is not displaced),
    over a denominator within 2 % of 1), so it moves by at most 1.25 scale (dL + dP)."""
    mlon, mlat = metres_per_degree(site, south)
    dL, dP = WORLD_BOUND / (d["lon_scale"] * mlon), WORLD_BOUND / (d["lat_scale"] * mlat)
    return 1.25 * max(d["col_scale"], d["row_scale"]) * (dL + dP)


def site_points(site, n, south=False, seed=0, spread=0.02):
    """n geodetic points around a site (+- spread degrees) and their UTM coordinates by the forward statement."""
    lat, lon, zone, _ = SITES[site]
    rng = np.random.default_rng(seed + n)
    lons, lats = lon + rng.uniform(-spread, spread, n), lat + rng.uniform(-spread, spread, n)
    e, nn = utm(lons, lats, zone, south)
    return lons, lats, e, nn


# ------------------------------------------------------------------------------------------------ cells to pixels
def cell_centres(H, W, xoff, yoff, res):
    """(east, north) of every cell, (H, W) each: row 0 is the northern edge."""
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return xoff + (ii.astype(np.float64) + 0.5) * res, yoff - (jj.astype(np.float64) + 0.5) * res


def world_pixels(d, east, north, alt, zone, south=False):
    """-> colrow float64 (..., 2), NaN in both where alt, lon, lat, col or row is not finite, and that mask."""
    alt = np.asarray(alt, np.float64)
    lon, lat, _ = utm_inverse(east, north, zone, south)
    with np.errstate(all="ignore"):
        col, row = project(d, lon, lat, alt)
    bad = ~(np.isfinite(alt) & np.isfinite(lon) & np.isfinite(lat) & np.isfinite(col) & np.isfinite(row))
    return np.stack([np.where(bad, np.nan, col), np.where(bad, np.nan, row)], -1), bad


def grid_pixels(d, dsm, xoff, yoff, res, zone, south=False):
    """-> colrow float64 (H, W, 2), counted (bool (H, W))."""
    dsm = np.asarray(dsm, np.float32)
    e, n = cell_centres(*dsm.shape, xoff, yoff, res)
    return world_pixels(d, e, n, dsm.astype(np.float64), zone, south)


def site_grid(site, H, W, res=0.5, south=False, shift=(0.0, 0.0)):
    """(xoff, yoff) of an H x W grid whose centre lies at the site (+ shift metres), on a lattice of `res`."""
    lat, lon, zone, _ = SITES[site]
    e, n = utm(lon, lat, zone, south)
    xoff = np.floor((float(e) + shift[0] - 0.5 * W * res) / res) * res
    yoff = np.ceil((float(n) + shift[1] + 0.5 * H * res) / res) * res
    return float(xoff), float(yoff)


def view_direction(d, zone, south, alt_lo, alt_hi, col=None, row=None):
    """P(alt_hi) - P(alt_lo) of one pixel (default: the image's offsets) in (east, north, up)."""
    col = d["col_offset"] if col is None else col
    row = d["row_offset"] if row is None else row
    pts = []
    for a in (alt_lo, alt_hi):
        lon, lat, bad = localize(d, [col], [row], a)
        assert not bad.any()
        e, n = utm(lon, lat, zone, south)
        pts.append(np.array([e[0], n[0], a]))
    return pts[1] - pts[0]


# ------------------------------------------------------------------------------------------------ the gather
def _taps(x, n):
    t0 = np.maximum(np.minimum(np.floor(x).astype(np.int64), n - 2), 0)
    return t0, np.minimum(t0 + 1, n - 1), x - t0.astype(np.float64)


def gather_taps(colrow, Hi, Wi):
    """(r0, r1, c0, c1, fy, fx) of every cell as the bilinear rule forms them (read where the state is KEPT)."""
    colrow = np.asarray(colrow, np.float64).reshape(-1, 2)
    with np.errstate(all="ignore"):
        safe = np.where(np.isfinite(colrow), colrow, 0.0)
        c0, c1, fx = _taps(safe[:, 0], Wi)
        r0, r1, fy = _taps(safe[:, 1], Hi)
    return r0, r1, c0, c1, fy, fx


def gather_state(colrow, Hi, Wi, vis=None):
    colrow = np.asarray(colrow, np.float64).reshape(-1, 2)
    col, row = colrow[:, 0], colrow[:, 1]
    with np.errstate(all="ignore"):
        nodata = np.isnan(col) | np.isnan(row)
        inside = (col >= 0.0) & (col <= float(Wi - 1)) & (row >= 0.0) & (row <= float(Hi - 1))
    state = np.full(col.shape, KEPT, dtype=np.uint8)
    if vis is not None:
        state[np.asarray(vis).reshape(-1) != V.VISIBLE] = OCCLUDED
    state[~inside] = OUTSIDE
    state[nodata] = NODATA
    return state


def gather(planes, colrow, vis=None, mode="bilinear"):
    """planes: float32 (C, Hi, Wi); colrow (..., 2) float64; vis uint8 per cell or None.
    -> out float32 (C, n), state uint8 (n), counts int64 (4)."""
    planes = np.asarray(planes, np.float32)
    C, Hi, Wi = planes.shape
    colrow = np.asarray(colrow, np.float64).reshape(-1, 2)
    state = gather_state(colrow, Hi, Wi, vis)
    out = np.full((C, colrow.shape[0]), np.nan, dtype=np.float32)
    at = np.flatnonzero(state == KEPT)
    col, row = colrow[at, 0], colrow[at, 1]
    if mode == "nearest":
        c = np.minimum(np.floor(col + 0.5).astype(np.int64), Wi - 1)
        r = np.minimum(np.floor(row + 0.5).astype(np.int64), Hi - 1)
        out.view(np.uint32)[:, at] = planes.view(np.uint32)[:, r, c]          # the pixel's 32 bits
    else:
        c0, c1, fx = _taps(col, Wi)
        r0, r1, fy = _taps(row, Hi)
        with np.errstate(all="ignore"):
            p00, p01 = planes[:, r0, c0].astype(np.float64), planes[:, r0, c1].astype(np.float64)
            p10, p11 = planes[:, r1, c0].astype(np.float64), planes[:, r1, c1].astype(np.float64)
            v = (1.0 - fy) * ((1.0 - fx) * p00 + fx * p01) + fy * ((1.0 - fx) * p10 + fx * p11)
            out[:, at] = v.astype(np.float32)
    counts = np.array([(state == s).sum() for s in (NODATA, OUTSIDE, OCCLUDED, KEPT)], dtype=np.int64)
    return out, state, counts


def same_f32(a, b, exact_nan=False):
    """float32 arrays equal bit for bit; unless exact_nan, every NaN counts as one value (the sign and payload of a NaN that
    ARITHMETIC produces - inf x 0 - is the processor's choice: x86 sets the sign bit, the device does not)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    if exact_nan:
        return np.array_equal(a.view(np.uint32), b.view(np.uint32))
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def edge_coordinates(n):
    """The coordinates of one axis of n pixels at which the rule can go wrong: the edges, both sides of them by 2^-40, -0.0, an
    integer and two fractions inside, NaN and both infinities."""
    t = 2.0 ** -40
    last = float(n - 1)
    xs = [0.0, -0.0, last, -t, last + t, t if n > 1 else 0.0, last - t if n > 1 else 0.0, np.nan, np.inf, -np.inf, -1.0, last + 1.0]
    if n > 2:
        xs += [1.0, float(n // 2), 0.5, last - 0.5, 1.25, last - 0.75]
    elif n == 2:
        xs += [0.5, 0.25]
    return np.array(xs, dtype=np.float64)


def edge_colrow(Hi, Wi):
    """Every pair of edge_coordinates of the two axes: (n, 2) = (col, row)."""
    c, r = np.meshgrid(edge_coordinates(Wi), edge_coordinates(Hi))
    return np.stack([c.ravel(), r.ravel()], -1)


def random_colrow(Hi, Wi, n, seed=0):
    """n pixel coordinates over and around an image, some NaN, some exactly on pixel centres."""
    rng = np.random.default_rng(seed + 131 * Hi + Wi + n)
    cr = np.stack([rng.uniform(-0.2 * Wi - 0.5, 1.2 * Wi, n), rng.uniform(-0.2 * Hi - 0.5, 1.2 * Hi, n)], -1)
    inside = rng.random(n) < 0.7
    cr[inside] = np.stack([rng.uniform(0, Wi - 1, n), rng.uniform(0, Hi - 1, n)], -1)[inside]
    whole = rng.random(n) < 0.1
    cr[whole] = np.floor(cr[whole])
    cr[rng.random(n) < 0.05] = np.nan
    return cr


def random_image(C, Hi, Wi, seed=0, specials=True):
    """float32 (C, Hi, Wi) planes; specials: some NaN pixels, a -0.0, a denormal, an infinity."""
    rng = np.random.default_rng(seed + 1000 * C + 31 * Hi + Wi)
    img = rng.uniform(-2.0, 3.0, (C, Hi, Wi)).astype(np.float32)
    flat = img.reshape(-1)
    if specials and flat.size >= 8:
        flat[rng.random(flat.size) < 0.03] = np.nan
        where = rng.choice(flat.size, 4, replace=False)
        flat[where[0]], flat[where[1]], flat[where[2]] = -0.0, np.float32(1e-41), np.inf
        flat[where[3]] = np.frombuffer(np.uint32(0x7FC12345).tobytes(), np.float32)[0]          # a NaN with a payload
    return img


LINEAR = (0.25, -0.5, 3.0)                   # alpha, beta, gamma: dyadic


def linear_image(Hi, Wi, C=1):
    """v = alpha col + beta row + gamma (+ channel) on integer pixels, exact in float32: (C, Hi, Wi)."""
    a, b, g = LINEAR
    rr, cc = np.meshgrid(np.arange(Hi), np.arange(Wi), indexing="ij")
    v = a * cc + b * rr + g
    img = np.stack([v + k for k in range(C)]).astype(np.float32)
    assert np.array_equal(img.astype(np.float64), np.stack([v + k for k in range(C)]))
    return img


def linear_value(colrow, channel=0):
    a, b, g = LINEAR
    colrow = np.asarray(colrow, np.float64)
    return (a * colrow[..., 0] + b * colrow[..., 1] + (g + channel)).astype(np.float32)


def within_one_ulp(got, want):
    """float32 arrays within one unit in the last place of `want`."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return bool(np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)))


def to_layout(planes, layout):
    """(C, Hi, Wi) planes as the buffer of a layout: 'planes' as they are, 'image' (Hi Wi, C)."""
    planes = np.asarray(planes, np.float32)
    return np.ascontiguousarray(planes) if layout == "planes" else np.ascontiguousarray(planes.reshape(planes.shape[0], -1).T)


# ------------------------------------------------------------------------------------------------ end to end
SCENE_SITE, SCENE_SEED, SCENE_IMAGE = "z17", 3, (640, 640)


def box_scene():
    """A 48 x 40 flat DSM at the site's altitude with a tall box, 0.5 m cells, under a tilted make_rpc: -> d, dsm, xoff, yoff, res."""
    d = make_rpc(SCENE_SITE, SCENE_SEED)
    ground = SITES[SCENE_SITE][3]
    dsm = np.full((48, 40), ground, dtype=np.float32)
    dsm[18:28, 14:24] = ground + 18.0
    res = 0.5
    xoff, yoff = site_grid(SCENE_SITE, 48, 40, res)
    return d, dsm, xoff, yoff, res


def orthophoto(d, planes, dsm, xoff, yoff, res, zone, south=False, occlusion=True, eps=0.0, view_dir=None, mode="bilinear"):
    """The whole chain: -> out (C, H, W), state (H, W), colrow (H, W, 2), vis (H, W) or None, counts {skipped + the four states}."""
    dsm = np.asarray(dsm, np.float32)
    H, W = dsm.shape
    colrow, bad = grid_pixels(d, dsm, xoff, yoff, res, zone, south)
    vis = None
    if occlusion:
        if view_dir is None:
            known = dsm[np.isfinite(dsm)]
            lo, hi = float(known.min()), float(known.max())
            view_dir = view_direction(d, zone, south, lo, max(hi, lo + 1.0))
        vis = V.grid_statement(dsm, res, [view_dir], eps, V.grid_zmax(dsm))[0][0]
    out, state, counts = gather(planes, colrow, vis, mode)
    return out.reshape(-1, H, W), state.reshape(H, W), colrow, vis, dict(zip(("nodata", "outside", "occluded", "kept"), counts.tolist()),
                                                                         skipped=int(bad.sum()))
