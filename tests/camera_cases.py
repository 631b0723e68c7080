"""The numpy statement of the camera geometry (include/brdfnerf_hip.h, "The rays of a satellite view") and its synthetic inputs.

Every function is the rule of the header written with numpy float64 arrays, one ufunc per operation, so every operation is
rounded on its own (numpy never fuses a multiply into an add).  The statement shares no code with brdf_nerf_amd/camera.py or
the kernels: project / localize are what bn_rpc_project / bn_rpc_localize must equal bit for bit; geo_world and rays are what
bn_geo_world / bn_rpc_rays must equal within the bounds the tests derive.

The synthetic RPCs (make_rpc) stand at three sites - zone 38 north, zone 17 north at a northing of 3.35e6 m, zone 21 south -
with scales of 0.02 degrees and 200 m over a 1024 px image, a linear part with an off-nadir altitude term and every other
coefficient drawn at relative size 1e-3.  CONDITIONS ON THE INPUTS, asserted by check_rpc (not tolerances on any code): every
denominator stays above 0.5, the Newton steps of iterations 7 and 8 are at most 4 x 2^-52 in normalised units, and len > 0.

Also here, for the CPU tests of the UTM series: Snyder's truncated series (an independent formula) and the meridian arc's
integrand.
"""
import numpy as np

NEWTON_ITERS = 8
KEYS10 = ("row_offset", "col_offset", "lat_offset", "lon_offset", "alt_offset", "row_scale", "col_scale", "lat_scale", "lon_scale",
          "alt_scale")
KEYS20 = ("row_num", "row_den", "col_num", "col_den")
WGS84_A, WGS84_FINV = 6378137.0, 298.257223563
K0 = 0.9996
ULP = 2.0 ** -52

# name: (lat, lon, zone, alt_offset)
SITES = {"z38": (11.6, 43.1, 38, 40.0), "z17": (30.3, -81.7, 17, 10.0), "z21": (-34.5, -58.5, 21, 25.0)}
RAY_R = (1, 63, 64, 65, 257)
GRIDS = ((1, 1), (3, 5), (65, 33))          # (H, W)
SUN = (38.5, 141.0)                         # elevation, azimuth in degrees


def alt_bounds(site):
    """(min_alt, max_alt) of a site's views."""
    off = SITES[site][3]
    return off - 60.0, off + 90.0


def make_rpc(site, seed):
    """The `rpc` dictionary (rpcm's keys, lists of 20 floats) of one synthetic image at a site."""
    lat, lon, _, alt = SITES[site]
    rng = np.random.default_rng(seed)
    d = {"row_offset": 512.0, "col_offset": 512.0, "lat_offset": lat, "lon_offset": lon, "alt_offset": alt, "row_scale": 512.0,
         "col_scale": 512.0, "lat_scale": 0.02, "lon_scale": 0.02, "alt_scale": 200.0}
    for k in KEYS20:
        d[k] = rng.uniform(-1e-3, 1e-3, 20)
    rot = rng.uniform(-0.05, 0.05)
    tilt = rng.uniform(0.03, 0.1, 2) * rng.choice([-1.0, 1.0], 2)
    d["col_num"][1:4] = (1.0, rot, tilt[0])          # columns grow with the longitude
    d["row_num"][1:4] = (rot, -1.0, tilt[1])         # rows grow southwards
    d["col_den"][0] = d["row_den"][0] = 1.0
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def rescaled(d, downscale):
    """sat_utils.rescale_rpc(rpc, 1 / downscale): the four image scales and offsets times float(1 / downscale)."""
    alpha = float(1.0 / downscale)
    out = dict(d)
    for k in ("row_scale", "col_scale", "row_offset", "col_offset"):
        out[k] = d[k] * alpha
    return out


def flat(d):
    """The 90 doubles of bn_rpc."""
    return np.concatenate([[float(d[k]) for k in KEYS10]] + [np.asarray(d[k], dtype=np.float64) for k in KEYS20])


# ------------------------------------------------------------------------------------------------ rules 1-3
def monomials(L, P, H):
    L, P, H = np.broadcast_arrays(np.asarray(L, np.float64), np.asarray(P, np.float64), np.asarray(H, np.float64))
    m4, m5, m6, m7, m8, m9 = L * P, L * H, P * H, L * L, P * P, H * H
    return [np.ones_like(L), L, P, H, m4, m5, m6, m7, m8, m9, (P * L) * H, m7 * L, m4 * P, m5 * H, m7 * P, m8 * P, m6 * H, m7 * H,
            m8 * H, m9 * H]


def poly(c, m):
    s = c[0] * m[0]
    for k in range(1, 20):
        s = s + c[k] * m[k]
    return s


def poly_dL(c, m):
    terms = ((4, m[2]), (5, m[3]), (7, 2.0 * m[1]), (10, m[6]), (11, 3.0 * m[7]), (12, m[8]), (13, m[9]), (14, 2.0 * m[4]),
             (17, 2.0 * m[5]))
    s = c[1] * m[0]
    for k, dm in terms:
        s = s + c[k] * dm
    return s


def poly_dP(c, m):
    terms = ((4, m[1]), (6, m[3]), (8, 2.0 * m[2]), (10, m[5]), (12, 2.0 * m[4]), (14, m[7]), (15, 3.0 * m[8]), (16, m[9]),
             (18, 2.0 * m[6]))
    s = c[2] * m[0]
    for k, dm in terms:
        s = s + c[k] * dm
    return s


def project(d, lon, lat, alt):
    """Rule 3: (col, row) of geodetic points."""
    c = {k: np.asarray(d[k], np.float64) for k in KEYS20}
    L = (np.asarray(lon, np.float64) - d["lon_offset"]) / d["lon_scale"]
    P = (np.asarray(lat, np.float64) - d["lat_offset"]) / d["lat_scale"]
    H = (np.asarray(alt, np.float64) - d["alt_offset"]) / d["alt_scale"]
    m = monomials(L, P, H)
    col = (poly(c["col_num"], m) / poly(c["col_den"], m)) * d["col_scale"] + d["col_offset"]
    row = (poly(c["row_num"], m) / poly(c["row_den"], m)) * d["row_scale"] + d["row_offset"]
    return col, row


def localize(d, cols, rows, alt, steps=None, denominators=None):
    """Rule 4: -> lon, lat (NaN where counted), counted (bool).  steps / denominators: lists that receive max |dL|, |dP| of every
    iteration and the smallest denominator met (the generator's conditions)."""
    c = {k: np.asarray(d[k], np.float64) for k in KEYS20}
    cols, rows, alt = np.broadcast_arrays(np.asarray(cols, np.float64), np.asarray(rows, np.float64), np.asarray(alt, np.float64))
    cn = (cols - d["col_offset"]) / d["col_scale"]
    rn = (rows - d["row_offset"]) / d["row_scale"]
    H = (alt - d["alt_offset"]) / d["alt_scale"]
    L, P = np.zeros_like(cn), np.zeros_like(cn)
    bad = np.zeros(cn.shape, dtype=bool)
    with np.errstate(all="ignore"):
        for _ in range(NEWTON_ITERS):
            m = monomials(L, P, H)
            N, D = poly(c["col_num"], m), poly(c["col_den"], m)
            NL, NP, DL, DP = poly_dL(c["col_num"], m), poly_dP(c["col_num"], m), poly_dL(c["col_den"], m), poly_dP(c["col_den"], m)
            fc = N / D - cn
            a, b = (NL * D - N * DL) / (D * D), (NP * D - N * DP) / (D * D)
            if denominators is not None:
                denominators.append(float(np.min(D)))
            N, D = poly(c["row_num"], m), poly(c["row_den"], m)
            NL, NP, DL, DP = poly_dL(c["row_num"], m), poly_dP(c["row_num"], m), poly_dL(c["row_den"], m), poly_dP(c["row_den"], m)
            fr = N / D - rn
            cc, dd = (NL * D - N * DL) / (D * D), (NP * D - N * DP) / (D * D)
            if denominators is not None:
                denominators.append(float(np.min(D)))
            det = a * dd - b * cc
            bad |= det == 0.0
            dL, dP = (fc * dd - b * fr) / det, (a * fr - fc * cc) / det
            if steps is not None:
                steps.append(float(np.max(np.abs(np.concatenate([dL.ravel(), dP.ravel()])))) if dL.size else 0.0)
            L, P = L - dL, P - dP
        lon = L * d["lon_scale"] + d["lon_offset"]
        lat = P * d["lat_scale"] + d["lat_offset"]
    bad |= ~np.isfinite(lon) | ~np.isfinite(lat)
    return np.where(bad, np.nan, lon), np.where(bad, np.nan, lat), bad


# ------------------------------------------------------------------------------------------------ rule 5
def utm_constants():
    """e, k0 A and alpha_1..6 of the Krueger series to n^6 (Karney 2011, eq. 35) on WGS84."""
    f = 1.0 / WGS84_FINV
    n = f / (2.0 - f)
    n2 = n * n
    e = np.sqrt(f * (2.0 - f))
    k0A = K0 * (WGS84_A / (1.0 + n) * (1.0 + n2 / 4.0 + n2 * n2 / 64.0 + n2 * n2 * n2 / 256.0))
    alpha = [n * (((((31564.0 * n - 66675.0) * n + 34440.0) * n + 47250.0) * n - 100800.0) * n + 75600.0) / 151200.0,
             n2 * ((((-1983433.0 * n + 863232.0) * n + 748608.0) * n - 1161216.0) * n + 524160.0) / 1935360.0,
             n2 * n * (((670412.0 * n + 406647.0) * n - 533952.0) * n + 184464.0) / 725760.0,
             n2 * n2 * ((6601661.0 * n - 7732800.0) * n + 2230245.0) / 7257600.0,
             n2 * n2 * n * (-13675556.0 * n + 3438171.0) / 7983360.0,
             n2 * n2 * n2 * 212378941.0 / 319334400.0]
    return e, k0A, alpha


def utm(lon, lat, zone, south=False):
    """(easting, northing): the central meridian is 6 zone - 183; south adds the false northing of 10,000,000 m."""
    e, k0A, alpha = utm_constants()
    lon, lat = np.asarray(lon, np.float64), np.asarray(lat, np.float64)
    d2r = np.pi / 180.0
    rlat = lat * d2r
    dl = (lon - (6.0 * zone - 183.0)) * d2r
    sp, cp = np.sin(rlat), np.cos(rlat)
    tau = sp / cp
    t = np.sinh(e * np.arctanh(e * sp))
    taup = tau * np.sqrt(1.0 + t * t) - t * np.sqrt(1.0 + tau * tau)
    xip = np.arctan2(taup, np.cos(dl))
    etap = np.arctanh(np.sin(dl) / np.sqrt(1.0 + taup * taup))
    s2, c2, sh2, ch2 = np.sin(2.0 * xip), np.cos(2.0 * xip), np.sinh(2.0 * etap), np.cosh(2.0 * etap)
    z, w = s2 * ch2 + 1j * (c2 * sh2), c2 * ch2 - 1j * (s2 * sh2)        # sin, cos of 2 (xi' + i eta')
    S, Cc = z, w
    xi, eta = xip, etap
    for j in range(6):
        xi = xi + alpha[j] * S.real
        eta = eta + alpha[j] * S.imag
        S, Cc = S * w + Cc * z, Cc * w - S * z
    return 500000.0 + k0A * eta, (10000000.0 if south else 0.0) + k0A * xi


def ecef(lon, lat, alt):
    """sat_utils.latlon_to_ecef_custom, as written there."""
    lon, lat, alt = np.asarray(lon, np.float64), np.asarray(lat, np.float64), np.asarray(alt, np.float64)
    rad_lat = lat * (np.pi / 180.0)
    rad_lon = lon * (np.pi / 180.0)
    f = 1 / WGS84_FINV
    e2 = 1 - (1 - f) * (1 - f)
    v = WGS84_A / np.sqrt(1 - e2 * np.sin(rad_lat) * np.sin(rad_lat))
    x = (v + alt) * np.cos(rad_lat) * np.cos(rad_lon)
    y = (v + alt) * np.cos(rad_lat) * np.sin(rad_lon)
    z = (v * (1 - e2) + alt) * np.sin(rad_lat)
    return x, y, z


def geo_world(lon, lat, alt, cs, zone=None, south=False):
    """-> float64 (n, 3)."""
    alt = np.broadcast_to(np.asarray(alt, np.float64), np.shape(lon))
    with np.errstate(all="ignore"):
        if cs == "ecef":
            return np.stack(ecef(lon, lat, alt), -1)
        x, y = utm(lon, lat, zone, south)
    return np.stack([x, y, alt], -1)


def sun_direction(elevation_deg, azimuth_deg):
    """get_sun_dirs (datasets/satellite_rgb_dep.py:561-576): float32 (3,)."""
    el, az = np.radians(elevation_deg), np.radians(azimuth_deg)
    return np.array([np.sin(az) * np.cos(el), np.cos(az) * np.cos(el), np.sin(el)]).astype(np.float32)


# ------------------------------------------------------------------------------------------------ rule 6
def rays(d, cols, rows, min_alt, max_alt, cs, zone, south, center, rng, sun=None, precision="reference", world_shift=0.0):
    """-> {"rays" float32 (n, 8 or 11), "lonlat_near", "lonlat_far" float64 (n, 2), "world_near" float64 (n, 3), "skipped"}.
    world_shift: metres added to every world coordinate that comes out of a transcendental (the generator's condition on
    the float32 rounding of the origins)."""
    lon_n, lat_n, bad_n = localize(d, cols, rows, max_alt)
    lon_f, lat_f, bad_f = localize(d, cols, rows, min_alt)
    near, far = geo_world(lon_n, lat_n, max_alt, cs, zone, south), geo_world(lon_f, lat_f, min_alt, cs, zone, south)
    if world_shift:
        k = 3 if cs == "ecef" else 2
        near, far = near.copy(), far.copy()
        near[:, :k] += world_shift
        far[:, :k] += world_shift
    with np.errstate(all="ignore"):
        dv = far - near
        ln = np.sqrt((dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2])
        direction = (dv / ln[:, None]).astype(np.float32)
        c64, r64 = np.asarray(center, np.float64), float(rng)
        if precision == "reference":
            o = (near.astype(np.float32) - c64.astype(np.float32)) / np.float32(r64)
            fr = ln.astype(np.float32) / np.float32(r64)
        else:
            o = ((near - c64) / r64).astype(np.float32)
            fr = (ln / r64).astype(np.float32)
    out = np.concatenate([o, direction, np.zeros((len(ln), 1), np.float32), fr[:, None]], 1).astype(np.float32)
    bad = bad_n | bad_f | ~np.isfinite(out).all(1)
    out[bad] = np.nan
    if sun is not None:
        out = np.concatenate([out, np.tile(np.asarray(sun, np.float32), (len(ln), 1))], 1)
    return {"rays": out, "lonlat_near": np.stack([lon_n, lat_n], -1), "lonlat_far": np.stack([lon_f, lat_f], -1), "world_near": near,
            "len": ln, "skipped": int(bad.sum())}


def grid_pixels(H, W):
    """(cols, rows) of an H x W view in row-major order, float64."""
    c, r = np.meshgrid(np.arange(W), np.arange(H))
    return c.ravel().astype(np.float64), r.ravel().astype(np.float64)


def scaling_params(v):
    """sat_utils.rpc_scaling_params on a float32 vector, in float32."""
    v = np.asarray(v, np.float32)
    scale = (v.max() - v.min()) / np.float32(2)
    return scale, v.min() + scale


def scene_loc(ray_tables):
    """init_scaling_params (:238-261) from the un-normalised float32 rays of every view (centre 0, range 1)."""
    allr = np.concatenate(ray_tables, 0)
    pts = np.concatenate([allr[:, :3], allr[:, :3] + allr[:, 7:8] * allr[:, 3:6]], 0)
    loc = {}
    for i, ax in enumerate("XYZ"):
        s, o = scaling_params(pts[:, i])
        loc[ax + "_scale"], loc[ax + "_offset"] = float(s), float(o)
    return loc


def check_rpc(d, H, W, min_alt, max_alt, cs, zone, south):
    """The conditions on a synthetic image (module docstring), on the H x W view it is used for."""
    cols, rows = grid_pixels(H, W)
    for alt in (min_alt, max_alt):
        steps, dens = [], []
        _, _, bad = localize(d, cols, rows, alt, steps, dens)
        assert not bad.any()
        assert min(dens) > 0.5, f"a denominator falls to {min(dens)}"
        assert max(steps[6:]) <= 4 * ULP, f"Newton steps 7, 8: {steps[6:]}"
    r = rays(d, cols, rows, min_alt, max_alt, cs, zone, south, (0.0, 0.0, 0.0), 1.0)
    assert r["skipped"] == 0 and (r["len"] > 0).all()


def singular_rpc():
    """An image whose rows do not depend on (L, P): the Jacobian's determinant is exactly zero in every iteration."""
    d = make_rpc("z38", 5)
    d["row_num"] = [0.25] + [0.0] * 19
    d["row_den"] = [1.0] + [0.0] * 19
    return d


# ------------------------------------------------------------------------------------------------ the UTM series on its own
def meridian_integrand(theta):
    """d (meridian arc) / d (latitude in radians): a (1 - e^2) (1 - e^2 sin^2)^-3/2."""
    f = 1.0 / WGS84_FINV
    e2 = f * (2.0 - f)
    return WGS84_A * (1.0 - e2) / (1.0 - e2 * np.sin(theta) ** 2) ** 1.5


def snyder_utm(lon, lat, zone, south=False):
    """Snyder, Map Projections - A Working Manual (USGS PP 1395), eqs. 8-9, 8-10, 3-21: truncated series in A = dlon cos lat."""
    f = 1.0 / WGS84_FINV
    e2 = f * (2.0 - f)
    ep2 = e2 / (1.0 - e2)
    phi = np.radians(np.asarray(lat, np.float64))
    lam = np.radians(np.asarray(lon, np.float64) - (6.0 * zone - 183.0))
    N = WGS84_A / np.sqrt(1.0 - e2 * np.sin(phi) ** 2)
    T, Cq, A = np.tan(phi) ** 2, ep2 * np.cos(phi) ** 2, lam * np.cos(phi)
    # the meridian arc (3-21) with its e^8 terms kept: truncated at e^6 it is itself 7e-4 m off at 60 degrees
    M = WGS84_A * ((1 - e2 / 4 - 3 * e2 ** 2 / 64 - 5 * e2 ** 3 / 256 - 175 * e2 ** 4 / 16384) * phi
                   - (3 * e2 / 8 + 3 * e2 ** 2 / 32 + 45 * e2 ** 3 / 1024 + 105 * e2 ** 4 / 4096) * np.sin(2 * phi)
                   + (15 * e2 ** 2 / 256 + 45 * e2 ** 3 / 1024 + 525 * e2 ** 4 / 16384) * np.sin(4 * phi)
                   - (35 * e2 ** 3 / 3072 + 175 * e2 ** 4 / 12288) * np.sin(6 * phi) + (315 * e2 ** 4 / 131072) * np.sin(8 * phi))
    x = K0 * N * (A + (1 - T + Cq) * A ** 3 / 6 + (5 - 18 * T + T ** 2 + 72 * Cq - 58 * ep2) * A ** 5 / 120)
    y = K0 * (M + N * np.tan(phi) * (A ** 2 / 2 + (5 - T + 9 * Cq + 4 * Cq ** 2) * A ** 4 / 24
                                     + (61 - 58 * T + T ** 2 + 600 * Cq - 330 * ep2) * A ** 6 / 720))
    return 500000.0 + x, (10000000.0 if south else 0.0) + y


# zone rule: (lat, lon, zone) including the Norway and Svalbard exceptions
ZONE_TABLE = ((11.6, 43.1, 38), (30.3, -81.7, 17), (-34.5, -58.5, 21), (0.0, -180.0, 1), (0.0, 179.9, 60), (0.0, 180.0, 60), (10.0, 5.9, 31),
              (10.0, 6.0, 32), (60.0, 4.0, 32), (55.9, 4.0, 31), (63.9, 3.0, 32), (64.0, 4.0, 31), (60.0, 2.9, 31), (60.0, 12.0, 33),
              (75.0, 8.0, 31), (75.0, 9.0, 33), (75.0, 20.9, 33), (75.0, 21.0, 35), (75.0, 32.9, 35), (75.0, 33.0, 37), (75.0, 41.9, 37),
              (71.9, 8.0, 32), (84.0, 8.0, 31), (72.0, 8.0, 31), (75.0, 42.0, 38), (75.0, -1.0, 30))

# ------------------------------------------------------------------------------------------------ the golden fixtures
# name: (site, cs, south, downscale); every fixture holds two views of 9 x 11 and 33 x 65 (after the downscale)
GOLDENS = {"camera_z38_utm_d1": ("z38", "utm", False, 1), "camera_z38_ecef_d2": ("z38", "ecef", False, 2),
           "camera_z17_utm_d1": ("z17", "utm", False, 1), "camera_z17_utm_d2": ("z17", "utm", False, 2),
           "camera_z17_ecef_d1": ("z17", "ecef", False, 1), "camera_z21_utm_north_d2": ("z21", "utm", False, 2),
           "camera_z21_utm_south_d1": ("z21", "utm", True, 1)}
GOLDEN_VIEWS = ((9, 11), (33, 65))           # (H, W)


def golden_views(name):
    """The views of a fixture: [{"rpc" (the image's dictionary, before the downscale), "H", "W", "min_alt", "max_alt", "sun"}]."""
    site, _, _, _ = GOLDENS[name]
    lo, hi = alt_bounds(site)
    seed0 = sorted(GOLDENS).index(name) * 10
    return [{"rpc": make_rpc(site, seed0 + i), "H": H, "W": W, "min_alt": lo, "max_alt": hi, "sun": (SUN[0] + 7 * i, SUN[1] - 30 * i)}
            for i, (H, W) in enumerate(GOLDEN_VIEWS)]
