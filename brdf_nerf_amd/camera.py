"""The rays of a satellite view from its RPC camera model, on the device.

The reference builds `rays (N, 11)` on the host in its dataset class (datasets/satellite_rgb_dep.py): get_rays localises every
pixel at max_alt and at min_alt through rpcm, projects both points to UTM through pyproj / utm (or to ECEF), and normalize_rays
subtracts the scene's centre.  This project depends on none of those packages; the geometry is stated operation by operation in
include/brdfnerf_hip.h ("The rays of a satellite view") and runs in brdf_nerf_amd/csrc/camera.hip, one lane per ray:

  Rpc.from_dict      the `rpc` dictionary of a scene's JSON (rpcm's keys) -> the 90 doubles of bn_rpc; downscale as
                     sat_utils.rescale_rpc (:90-108)
  project            geodetic points -> pixels (bn_rpc_project)
  localize           pixels at an altitude -> geodetic points (bn_rpc_localize): 8 Newton iterations, no data-dependent exit
  geo_world          geodetic points -> ECEF (sat_utils.latlon_to_ecef_custom) or UTM (Krueger series to n^6) (bn_geo_world)
  ecef_geodetic      ECEF points -> geodetic points (sat_utils.ecef_to_latlon_custom as written) (bn_ecef_geodetic)
  view_rays          get_rays + normalize_rays + get_sun_dirs of one view in one launch per chunk (bn_rpc_rays)
  scene_bounds       init_scaling_params (:238-261): the scene.loc dictionary, the centre and the range
  nearest_lines      the lines scale_depth (:396-399) samples: torch's nearest rule with its float32 scale, and its inverse
  depth_priors       load_depth_data (:401-548) of one view from its tie points, paired by pixel: depths, weights, valid_depth,
                     depth_std, the padded rays and the normals (bn_tie_owner, bn_tie_priors, one lane per tie point)
  ray_table          the views of a scene concatenated into a RayTable (load_data, :311-394, and with priors= load_depth_data:
                     load_train_split without its file readers; a view's priors may also be a surface model, raycast.surface_priors)
  utm_zone           the zone of a point, with the Norway and Svalbard exceptions (utm.latlon_to_zone_number)
  sun_direction      get_sun_dirs (:561-576)

precision="reference" reproduces upstream's rounding: the WORLD origin is cast to float32 (:76-77) before the centre is
subtracted (:550-559), which at a UTM northing of 3.3e6 m puts the origins on a 0.25 m lattice.  precision="exact" subtracts
and divides in float64 and rounds once.  The coordinate system is this module's own parameter (`cs`, 'utm' or 'ecef');
a dsm.SceneFrame given in place of center and range must state the same one (its zone plays no part here).  The UTM zone is
a parameter of the scene, not taken from the first pixel of each call as upstream does (sat_utils.py:156-159); south=False adds
no false northing, which is what upstream's "+proj=utm +zone=17R" does in both hemispheres.

  utm_geodetic       UTM points -> geodetic points (Karney's inverse series and Newton for the latitude) (bn_utm_geodetic)
  view_direction     the direction from the surface towards the sensor at one pixel, in (east, north, up)

Not here: the file readers (JSON, GeoTIFF, the tie-point text files), image scaling, a `group` for depth_priors
(a view's priors are made once), the normals as a table column.
The RPC rule is the public RPC00B definition and the UTM series Karney's; neither was checked against rpcm or pyproj.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L

_CS = {"ecef": L.BN_CS_ECEF, "utm": L.BN_CS_UTM}
_PRECISION = {"reference": 1, "exact": 0}
_KEYS10 = ("row_offset", "col_offset", "lat_offset", "lon_offset", "alt_offset", "row_scale", "col_scale", "lat_scale", "lon_scale",
           "alt_scale")
_KEYS20 = ("row_num", "row_den", "col_num", "col_den")
MAX_RAYS = 1 << 30


class Rpc:
    """One image's RPC model: the 90 doubles of bn_rpc (`struct`) under their names."""

    def __init__(self, values):
        for k in _KEYS10:
            setattr(self, k, float(values[k]))
        for k in _KEYS20:
            c = values[k]
            if isinstance(c, str):                                  # "a, b, ..." as some JSON writers store the lists
                c = c.replace(",", " ").split()
            c = [float(v) for v in c]
            if len(c) != 20:
                raise ValueError(f"Rpc: {k} has {len(c)} coefficients (20)")
            setattr(self, k, c)
        flat = [getattr(self, k) for k in _KEYS10] + [v for k in _KEYS20 for v in getattr(self, k)]
        if not all(math.isfinite(v) for v in flat):
            raise ValueError("Rpc: the descriptor has a non-finite entry")
        for k in _KEYS10[5:]:
            if getattr(self, k) == 0.0:
                raise ValueError(f"Rpc: {k} is zero")
        self.struct = L.Rpc()
        for k in _KEYS10:
            setattr(self.struct, k, getattr(self, k))
        for k in _KEYS20:
            setattr(self.struct, k, (C.c_double * 20)(*getattr(self, k)))

    @classmethod
    def from_dict(cls, d, downscale=1.0):
        """d: the `rpc` dictionary of a scene's JSON (dict_format="rpcm").  downscale: the image was shrunk by this factor
        (sat_utils.rescale_rpc with alpha = 1 / downscale: the row / col scales and offsets times float(1 / downscale))."""
        missing = [k for k in _KEYS10 + _KEYS20 if k not in d]
        if missing:
            raise ValueError(f"Rpc.from_dict: missing keys {missing}")
        if not (float(downscale) > 0 and math.isfinite(float(downscale))):
            raise ValueError(f"Rpc.from_dict: downscale {downscale} must be positive and finite")
        alpha = float(1.0 / downscale)
        v = dict(d)
        for k in ("row_scale", "col_scale", "row_offset", "col_offset"):
            v[k] = float(d[k]) * alpha
        return cls(v)

    def ref(self):
        return C.byref(self.struct)


def utm_zone(lat, lon):
    """The UTM zone number of (lat, lon) in degrees: int((lon + 180) / 6) + 1, 60 at lon == 180, with the exceptions of south-west
    Norway (56 <= lat < 64, 3 <= lon < 12: 32) and Svalbard (72 <= lat <= 84: 31, 33, 35, 37): utm.latlon_to_zone_number."""
    lat, lon = float(lat), float(lon)
    if not (-180.0 <= lon <= 180.0 and -90.0 <= lat <= 90.0):
        raise ValueError(f"utm_zone: ({lat}, {lon}) is not a latitude in [-90, 90] and a longitude in [-180, 180]")
    if 56 <= lat < 64 and 3 <= lon < 12:
        return 32
    if 72 <= lat <= 84 and lon >= 0:
        if lon < 9:
            return 31
        if lon < 21:
            return 33
        if lon < 33:
            return 35
        if lon < 42:
            return 37
    if lon == 180:
        return 60
    return int((lon + 180) / 6) + 1


def sun_direction(elevation_deg, azimuth_deg):
    """get_sun_dirs (datasets/satellite_rgb_dep.py:561-576) in numpy float64, rounded to float32: (3,) numpy array."""
    el, az = np.radians(elevation_deg), np.radians(azimuth_deg)
    return np.array([np.sin(az) * np.cos(el), np.cos(az) * np.cos(el), np.sin(el)]).astype(np.float32)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _device(device, *tensors):
    if device is not None:
        return torch.device(device)
    for t in tensors:
        if torch.is_tensor(t) and t.is_cuda:
            return t.device
    return torch.device("cuda", torch.cuda.current_device())


def _f64(x, dev, what, n=None):
    """A float64 contiguous vector on the device (a scalar with n: repeated)."""
    t = torch.as_tensor(x, dtype=torch.float64).to(dev)
    if t.dim() == 0 and n is not None:
        t = t.expand(n)
    if t.dim() != 1 or (n is not None and t.shape[0] != n):
        raise ValueError(f"{what}: expected a vector" + (f" of {n}" if n is not None else "") + f", got {tuple(t.shape)}")
    return t.contiguous()


def _world_args(cs, zone, south, rpc=None):
    if cs not in _CS:
        raise ValueError(f"camera: unknown coordinate system {cs!r} ('utm' or 'ecef')")
    if cs == "ecef":
        return _CS[cs], 1, 0
    if zone is None:
        if rpc is None:
            raise ValueError("camera: cs='utm' needs the scene's zone")
        zone = utm_zone(rpc.lat_offset, rpc.lon_offset)
    if not 1 <= int(zone) <= 60:
        raise ValueError(f"camera: zone {zone} outside 1-60")
    return _CS[cs], int(zone), int(bool(south))


def _check_count(n, what):
    if n < 0 or n > MAX_RAYS:
        raise ValueError(f"{what}: {n} rays (0 to 2^30)")


@torch.no_grad()
def project(rpc, lon, lat, alt, device=None):
    """Pixels of geodetic points (rule 3): lon, lat in degrees, alt in metres (vectors, alt may be a scalar) -> col, row float64."""
    dev = _device(device, lon, lat, alt)
    lon = _f64(lon, dev, "project: lon")
    n = lon.shape[0]
    _check_count(n, "project")
    lat, alt = _f64(lat, dev, "project: lat", n), _f64(alt, dev, "project: alt", n)
    col, row = torch.empty_like(lon), torch.empty_like(lon)
    with torch.cuda.device(dev):
        L.check(L.lib().bn_rpc_project(rpc.ref(), _p(lon), _p(lat), _p(alt), n, _p(col), _p(row), _stream()), "bn_rpc_project")
    return col, row


@torch.no_grad()
def localize(rpc, cols, rows, alt, device=None):
    """Geodetic points of pixels at the altitude `alt` (rule 4) -> lonlat float64 (n, 2) in degrees (NaN where the Newton
    iteration met a zero determinant or did not stay finite), skipped (their number)."""
    if not math.isfinite(float(alt)):
        raise ValueError(f"localize: alt {alt} must be finite")
    dev = _device(device, cols, rows)
    cols = _f64(cols, dev, "localize: cols")
    n = cols.shape[0]
    _check_count(n, "localize")
    rows = _f64(rows, dev, "localize: rows", n)
    lonlat = torch.empty((n, 2), dtype=torch.float64, device=dev)
    counts = torch.zeros((1,), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().bn_rpc_localize(rpc.ref(), _p(cols), _p(rows), 1, 0, n, float(alt), _p(lonlat), _p(counts), _stream()),
                "bn_rpc_localize")
    return lonlat, int(counts.item())


@torch.no_grad()
def geo_world(lonlat, alt, cs="utm", zone=None, south=False, device=None):
    """World points of geodetic points (rule 5): lonlat (n, 2) degrees, alt (n,) or a scalar -> float64 (n, 3): ECEF, or
    (easting, northing, alt) in the UTM `zone`."""
    code, zone, south = _world_args(cs, zone, south)
    dev = _device(device, lonlat, alt)
    lonlat = torch.as_tensor(lonlat, dtype=torch.float64).to(dev).contiguous()
    if lonlat.dim() != 2 or lonlat.shape[1] != 2:
        raise ValueError(f"geo_world: lonlat must be (n, 2), got {tuple(lonlat.shape)}")
    n = lonlat.shape[0]
    _check_count(n, "geo_world")
    alt = _f64(alt, dev, "geo_world: alt", n)
    xyz = torch.empty((n, 3), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().bn_geo_world(_p(lonlat), _p(alt), n, code, zone, south, _p(xyz), _stream()), "bn_geo_world")
    return xyz


@torch.no_grad()
def ecef_geodetic(xyz, device=None, want_skipped=False):
    """Geodetic points of ECEF points ("World points of an ECEF scene" in the header; the counterpart of geo_world(cs='ecef')):
    xyz (n, 3) metres -> lonlat float64 (n, 2) in degrees, alt float64 (n,); NaN where a point is on the axis or not finite
    (want_skipped: also their number)."""
    from . import functions as Fn
    dev = _device(device, xyz)
    xyz = torch.as_tensor(xyz, dtype=torch.float64).to(dev)
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"ecef_geodetic: xyz must be (n, 3), got {tuple(xyz.shape)}")
    _check_count(xyz.shape[0], "ecef_geodetic")
    skipped = torch.zeros((1,), dtype=torch.int64, device=dev)
    lonlat, alt = Fn.ecef_geodetic(xyz, skipped)
    return (lonlat, alt, int(skipped.item())) if want_skipped else (lonlat, alt)


@torch.no_grad()
def utm_geodetic(en, zone, south=False, device=None):
    """Geodetic points of UTM points ("Orthophoto of an observed image" in the header, step 2; the counterpart of
    geo_world(cs='utm')): en (n, 2) metres = (east, north) in `zone`, south=True taking the false northing off -> lonlat float64
    (n, 2) in degrees (NaN where lon or lat is not finite), skipped (their number)."""
    from . import functions as Fn
    dev = _device(device, en)
    en = torch.as_tensor(en, dtype=torch.float64).to(dev)
    if en.dim() != 2 or en.shape[1] != 2:
        raise ValueError(f"utm_geodetic: en must be (n, 2), got {tuple(en.shape)}")
    _check_count(en.shape[0], "utm_geodetic")
    skipped = torch.zeros((1,), dtype=torch.int64, device=dev)
    lonlat = Fn.utm_geodetic(en, zone, south, skipped)
    return lonlat, int(skipped.item())


@torch.no_grad()
def view_direction(rpc, zone, south, alt_lo, alt_hi, col=None, row=None, device=None):
    """The direction from the surface towards the sensor at one pixel of a view, in (east, north, up) - what grid_visibility
    takes: the pixel (default: the image's col_offset, row_offset) localised at alt_lo and at alt_hi, both points taken to the UTM
    `zone`, P(alt_hi) - P(alt_lo).  Existing entries only (localize, geo_world).  -> float64 (3,) on the host, not normalised."""
    alt_lo, alt_hi = float(alt_lo), float(alt_hi)
    if not (math.isfinite(alt_lo) and math.isfinite(alt_hi) and alt_hi > alt_lo):
        raise ValueError(f"view_direction: altitudes [{alt_lo}, {alt_hi}] must be finite and alt_hi above alt_lo")
    _world_args("utm", zone, south)
    col = rpc.col_offset if col is None else float(col)
    row = rpc.row_offset if row is None else float(row)
    dev = _device(device)
    pts = [geo_world(localize(rpc, [col], [row], a, device=dev)[0], a, "utm", zone, south, device=dev) for a in (alt_lo, alt_hi)]
    d = (pts[1] - pts[0]).reshape(3).cpu()
    if not bool(torch.isfinite(d).all()):
        raise ValueError(f"view_direction: pixel ({col}, {row}) does not localise at [{alt_lo}, {alt_hi}]")
    return d


def _frame(center, range, cs):
    """(center (3 floats), range) from the two values or from a dsm.SceneFrame in place of `center`."""
    from .dsm import SceneFrame
    if isinstance(center, SceneFrame):
        if center.cs != cs:
            raise ValueError(f"camera: the SceneFrame states a {center.cs!r} scene and the call cs={cs!r}")
        center, range = center.center, center.range
    if range is None:
        raise ValueError("camera: range is missing (pass center and range, or a SceneFrame)")
    center = tuple(float(c) for c in (center.tolist() if hasattr(center, "tolist") else center))
    range = float(range)
    if len(center) != 3 or not all(math.isfinite(c) for c in center):
        raise ValueError(f"camera: center {center} must be 3 finite numbers")
    if not (range > 0 and math.isfinite(range)):
        raise ValueError(f"camera: range {range} must be positive and finite")
    return center, range


def rays_launch(rpc, cols, rows, W, r0, r1, min_alt, max_alt, code, zone, south, center, range, sun, round_f32, out, lonlat_near=None,
                lonlat_far=None, counts=None):
    """One bn_rpc_rays launch: rays [r0, r1) of the view into the rows of `out` (float32, r1 - r0 rows), indexed from r0."""
    c = (C.c_double * 3)(*center)
    s = None if sun is None else (C.c_float * 3)(*[float(v) for v in sun])
    with torch.cuda.device(out.device):
        L.check(L.lib().bn_rpc_rays(rpc.ref(), _p(cols), _p(rows), int(W), int(r0), int(r1), float(min_alt), float(max_alt), code, zone,
                                    south, c, float(range), s, round_f32, _p(out), out.stride(0), _p(lonlat_near), _p(lonlat_far),
                                    _p(counts), _stream()), "bn_rpc_rays")


@torch.no_grad()
def view_rays(rpc, H, W, min_alt, max_alt, center, range=None, cs="utm", zone=None, south=False, sun=None, rows=None, cols=None,
              chunk=None, precision="reference", group=None, device=None, span=None, want_lonlat=False):
    """The normalised rays of a view: get_rays + normalize_rays (+ get_sun_dirs) of datasets/satellite_rgb_dep.py.
    Grid mode: ray r is pixel (col r % W, row r / W) of the H x W image, row-major as upstream's meshgrid.  Array mode (rows and
    cols: pixel coordinates, any float64 values): ray r is (cols[r], rows[r]); H and W are not read.
    center, range: the scene's normalisation (scene_bounds, or the scene.loc file), or a dsm.SceneFrame in place of both.
    sun: (elevation_deg, azimuth_deg) -> columns 8-10; None: 8 columns.  precision: 'reference' or 'exact' (module docstring).
    chunk: rays per launch (None: one launch).  span=(r0, r1): only those rays of the view - a chunk made in front of
    render_image.  group: each rank makes shard_bounds of the rays and the shards are gathered in rank order.
    -> rays (R, 11 or 8) float32 on the device, skipped (rays with NaN in columns 0-7: a zero determinant or a non-finite value);
    want_lonlat: also the float64 (R, 2) geodetic near and far points."""
    from .viewwalk import ViewWalk
    if precision not in _PRECISION:
        raise ValueError(f"view_rays: unknown precision {precision!r} ('reference' or 'exact')")
    code, zone, south = _world_args(cs, zone, south, rpc)
    center, range = _frame(center, range, cs)
    if not (math.isfinite(float(min_alt)) and math.isfinite(float(max_alt))):
        raise ValueError(f"view_rays: altitudes [{min_alt}, {max_alt}] must be finite")
    if (rows is None) != (cols is None):
        raise ValueError("view_rays: rows and cols come together")
    dev = _device(device, rows, cols)
    if cols is not None:
        cols = _f64(cols, dev, "view_rays: cols")
        rows = _f64(rows, dev, "view_rays: rows", cols.shape[0])
        n, W = cols.shape[0], 1
    else:
        if int(H) < 1 or int(W) < 1:
            raise ValueError(f"view_rays: a view of {H} x {W} pixels")
        n = int(H) * int(W)
    _check_count(n, "view_rays")
    a, b = (0, n) if span is None else (int(span[0]), int(span[1]))
    if not 0 <= a <= b <= n:
        raise ValueError(f"view_rays: span [{a}, {b}) outside the view's {n} rays")
    sun_v = None if sun is None else sun_direction(*sun)
    width = 8 if sun is None else 11
    walk = ViewWalk(b - a, chunk or max(b - a, 1), group)
    m = walk.hi - walk.lo
    out = torch.empty((m, width), dtype=torch.float32, device=dev)
    counts = torch.zeros((1,), dtype=torch.int64, device=dev)
    near = torch.empty((m, 2), dtype=torch.float64, device=dev) if want_lonlat else None
    far = torch.empty((m, 2), dtype=torch.float64, device=dev) if want_lonlat else None
    for i, j in walk.chunks():
        k0, k1 = i - walk.lo, j - walk.lo
        rays_launch(rpc, cols, rows, W, a + i, a + j, min_alt, max_alt, code, zone, south, center, range, sun_v, _PRECISION[precision],
                    out[k0:k1], None if near is None else near[k0:k1], None if far is None else far[k0:k1], counts)
    if walk.world > 1:
        from .distributed import allreduce_
        out = walk.join([out], (width,), device=dev)
        allreduce_(counts, group=group)
        if want_lonlat:
            near, far = walk.join([near], (2,), torch.float64, dev), walk.join([far], (2,), torch.float64, dev)
    skipped = int(counts.item())
    return (out, skipped, near, far) if want_lonlat else (out, skipped)


def _view_args(v):
    rpc = v["rpc"] if isinstance(v["rpc"], Rpc) else Rpc.from_dict(v["rpc"], v.get("downscale", 1.0))
    return rpc, int(v["H"]), int(v["W"]), float(v["min_alt"]), float(v["max_alt"])


@torch.no_grad()
def scene_bounds(views, cs="utm", zone=None, south=False, device=None, chunk=None):
    """init_scaling_params (datasets/satellite_rgb_dep.py:238-261): the float32 world near and far points of every view (centre 0,
    range 1, precision='reference': get_rays' own rows), amin / amax per axis on the device, sat_utils.rpc_scaling_params in float32.
    views: dictionaries {"rpc": Rpc or its dictionary (+ "downscale"), "H", "W", "min_alt", "max_alt"}.  cs='utm' without a zone:
    the zone of the first view's lat / lon offset, for every view.
    -> loc {"X_scale", "X_offset", ...} (scene.loc), center (3 floats), range = max(scales) (:164-165).  Rays that were skipped
    (NaN) take no part."""
    if not views:
        raise ValueError("scene_bounds: no views")
    lo = hi = None
    for v in views:
        rpc, H, W, min_alt, max_alt = _view_args(v)
        if cs == "utm" and zone is None:
            zone = utm_zone(rpc.lat_offset, rpc.lon_offset)
        rays, skipped = view_rays(rpc, H, W, min_alt, max_alt, (0.0, 0.0, 0.0), 1.0, cs=cs, zone=zone, south=south, chunk=chunk,
                                  device=device)
        if skipped:
            rays = rays[torch.isfinite(rays).all(1)]
        if rays.shape[0] == 0:
            continue
        pts = torch.cat([rays[:, :3], rays[:, :3] + rays[:, 7:8] * rays[:, 3:6]], 0)
        vlo, vhi = pts.amin(0), pts.amax(0)
        lo, hi = (vlo, vhi) if lo is None else (torch.minimum(lo, vlo), torch.maximum(hi, vhi))
    if lo is None:
        raise ValueError("scene_bounds: no view has a finite ray")
    scale = (hi - lo) / 2                                   # float32, as rpc_scaling_params on the float32 points
    offset = lo + scale
    scale, offset = scale.tolist(), offset.tolist()
    loc = {}
    for i, ax in enumerate("XYZ"):
        loc[ax + "_scale"], loc[ax + "_offset"] = scale[i], offset[i]
    return loc, tuple(offset), max(scale)


def nearest_lines(n, downscale):
    """The lines a nearest resize of n lines by `downscale` samples (scale_depth, :396-399: torch's interpolate to the size
    int(n / downscale), whose scale is the float32 quotient n / n_out): -> n_out, src int64 (n_out) with
    src[j] = min(int(floorf((float)j * ((float)n / (float)n_out))), n - 1), dst int32 (n) its inverse, -1 where a line is not sampled."""
    n = int(n)
    if n < 1 or n > 1 << 24:
        raise ValueError(f"nearest_lines: {n} lines (1 to 2^24: the float32 rule is exact in the index up to there)")
    if not (math.isfinite(float(downscale)) and float(downscale) >= 1.0):
        raise ValueError(f"nearest_lines: downscale {downscale} must be finite and at least 1")
    n_out = int(n / downscale)
    if n_out < 1:
        raise ValueError(f"nearest_lines: {n} lines at downscale {downscale} leave none")
    scale = np.float32(n) / np.float32(n_out)
    src = np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), n - 1)
    dst = np.full(n, -1, dtype=np.int32)
    dst[src] = np.arange(n_out, dtype=np.int32)
    return n_out, src, dst


def _tie_inputs(name, pts2d, pts3d, correl, dev):
    px = torch.as_tensor(pts2d)
    if px.is_floating_point() or px.dtype == torch.bool or px.is_complex():
        raise ValueError(f"{name}: pts2d are {px.dtype}: integer (col, row) pixels at full resolution")
    px = px.reshape(-1, 2) if px.dim() == 1 and px.numel() == 2 else px             # one tie point, as np.loadtxt returns it
    if px.dim() != 2 or px.shape[1] != 2:
        raise ValueError(f"{name}: pts2d must be (T, 2), got {tuple(px.shape)}")
    T = px.shape[0]
    _check_count(T, name)
    px = px.to(dev).to(torch.int64).clamp(-(1 << 31), (1 << 31) - 1).to(torch.int32).contiguous()
    pts3d = torch.as_tensor(pts3d, dtype=torch.float64).to(dev).reshape(-1, 3).contiguous()
    correl = torch.as_tensor(correl, dtype=torch.float64).to(dev).reshape(-1).contiguous()
    if pts3d.shape[0] != T or correl.shape[0] != T:
        raise ValueError(f"{name}: {T} pixels, {pts3d.shape[0]} points and {correl.shape[0]} correlations")
    return px, pts3d, correl, T


@torch.no_grad()
def tie_priors(rpc, H, W, pts2d, pts3d, correl, cmin, cmax, min_alt, max_alt, center, range=None, cs="utm", zone=None, south=False,
               downscale=1.0, corrscale=1.0, stdscale=1.0, margin=0.0, std_span=0.0, precision="reference", want_rays=False,
               want_points=True, want_tie_rays=False, device=None):
    """The two launches of the depth priors (bn_tie_owner, bn_tie_priors) with the correlation bounds given: the raw buffers.
    -> {"owner" int32 (H, W), "valid" (Hout Wout), "depths" (Hout Wout, 2), "depth_std", "rays" (Hout Wout, 8) or None, "points"
    (H, W, 3) and "valid_full" (H, W) or None, "tie_rays" (T, 8) or None, "counts" int64 (4) on the device, "shape",
    "src_rows", "src_cols" (int64, on the device)}.  depth_priors is the public form."""
    name = "tie_priors"
    if precision not in _PRECISION:
        raise ValueError(f"{name}: unknown precision {precision!r} ('reference' or 'exact')")
    code, zone, south = _world_args(cs, zone, south, rpc)
    center, range = _frame(center, range, cs)
    H, W = int(H), int(W)
    if H < 1 or W < 1 or H * W > 1 << 30:
        raise ValueError(f"{name}: a view of {H} x {W} pixels (at least 1 x 1, H W at most 2^30)")
    scalars = {"min_alt": min_alt, "max_alt": max_alt, "cmin": cmin, "cmax": cmax, "corrscale": corrscale, "stdscale": stdscale,
               "margin": margin, "std_span": std_span, "downscale": downscale}
    for k, v in scalars.items():
        if not math.isfinite(float(v)):
            raise ValueError(f"{name}: {k} {v} must be finite")
    if not float(cmax) > float(cmin):
        raise ValueError(f"{name}: correlations [{cmin}, {cmax}]: cmax must exceed cmin")
    dev = _device(device, pts2d, pts3d, correl)
    px, pts3d, correl, T = _tie_inputs(name, pts2d, pts3d, correl, dev)
    Hout, src_r, dst_r = nearest_lines(H, downscale)
    Wout, src_c, dst_c = nearest_lines(W, downscale)
    identity = float(downscale) == 1.0
    dst_r, dst_c = (None, None) if identity else (torch.from_numpy(dst_r).to(dev), torch.from_numpy(dst_c).to(dev))
    f32 = dict(dtype=torch.float32, device=dev)
    owner = torch.full((H, W), -1, dtype=torch.int32, device=dev)
    counts = torch.zeros((4,), dtype=torch.int64, device=dev)
    out = {"owner": owner, "counts": counts, "shape": (Hout, Wout), "valid": torch.zeros((Hout * Wout,), **f32),
           "depths": torch.zeros((Hout * Wout, 2), **f32), "depth_std": torch.zeros((Hout * Wout,), **f32),
           "rays": torch.zeros((Hout * Wout, 8), **f32) if want_rays else None,
           "points": torch.zeros((H, W, 3), **f32) if want_points else None,
           "valid_full": torch.zeros((H, W), **f32) if want_points else None,
           "tie_rays": torch.zeros((T, 8), **f32) if want_tie_rays else None,
           "src_rows": torch.from_numpy(src_r).to(dev), "src_cols": torch.from_numpy(src_c).to(dev)}
    c = (C.c_double * 3)(*center)
    with torch.cuda.device(dev):
        L.check(L.lib().bn_tie_owner(_p(px), T, H, W, _p(owner), _p(counts), _stream()), "bn_tie_owner")
        L.check(L.lib().bn_tie_priors(rpc.ref(), _p(px), _p(owner), _p(pts3d), _p(correl), T, H, W, Hout, Wout, _p(dst_r), _p(dst_c),
                                      float(downscale), float(min_alt), float(max_alt), code, zone, south, c, range,
                                      _PRECISION[precision], float(cmin), float(cmax), float(corrscale), float(stdscale), float(margin),
                                      float(std_span), _p(out["valid"]), _p(out["depths"]), _p(out["depth_std"]), _p(out["rays"]),
                                      _p(out["points"]), _p(out["valid_full"]), _p(out["tie_rays"]), _p(counts), _stream()),
                "bn_tie_priors")
    return out


@torch.no_grad()
def depth_priors(rpc, H, W, pts2d, pts3d, correl, min_alt, max_alt, center, range=None, cs="utm", zone=None, south=False, downscale=1.0,
                 corrscale=1.0, stdscale=1.0, margin=0.0, std_span=0.0, precision="reference", want_rays=False, want_normals=True,
                 device=None):
    """The depth priors of one view from its tie points: load_depth_data (datasets/satellite_rgb_dep.py:401-548) without its file
    readers, paired by pixel (include/brdfnerf_hip.h, "The depth priors of a view").
    H, W and pts2d (T, 2) integer (col, row): at FULL resolution; rpc: Rpc.from_dict(d, downscale); pts3d (T, 3) world points,
    correl (T) their correlation scores; center, range: as view_rays.  corrscale, stdscale, margin: upstream's options of those
    names; std_span: upstream's depth_max - depth_min, which is 0 (so its depth_std is identically zero).
    The correlations are normalised by their amin / amax over all T tie points, read from the device as two scalars; a cmax <=
    cmin or a non-finite one is a ValueError (upstream divides by zero).
    -> {"depths" (Hout Wout, 2) = (depth, weight), "valid_depth", "depth_std", "normals" (Hout Wout, 3) and "valid_normal"
    (want_normals), "rays" (Hout Wout, 8) (want_rays: upstream's all_deprays), "shape" (Hout, Wout), "outside", "duplicates",
    "skipped", "unsampled", "kept"}, with kept + outside + duplicates + skipped + unsampled == T.
    Where valid_depth == 0 the depth is the float32 of the float64 mean of the kept depths (padding, no loss reads it), weight
    and std are 0.  Normals: point_normals on the FULL-resolution grid of tie points (calc_normal_from_pts3d with its valid_depth
    rule), (0, 0, 1) where valid_normal == 0 (:511-514), then the lines the resize samples.  At downscale == 1 every output is
    upstream's; at other factors upstream raises (valid_depth.reshape(height, width) after scale_depth) and the outputs are
    this project's reading of it: the resize of the full-resolution maps."""
    from . import functions as Fn
    name = "depth_priors"
    dev = _device(device, pts2d, pts3d, correl)
    pts2d, pts3d, cor, T = _tie_inputs(name, pts2d, pts3d, correl, dev)          # on the device once; tie_priors takes them as they are
    if T == 0:
        raise ValueError(f"{name}: no tie points (a view without priors: ray_table(priors=[..., None, ...]))")
    cmin, cmax = torch.stack([cor.amin(), cor.amax()]).tolist()
    if not (math.isfinite(cmin) and math.isfinite(cmax) and cmax > cmin):
        raise ValueError(f"{name}: correlations in [{cmin}, {cmax}]: they must be finite and not all equal")
    raw = tie_priors(rpc, H, W, pts2d, pts3d, cor, cmin, cmax, min_alt, max_alt, center, range, cs=cs, zone=zone, south=south,
                     downscale=downscale, corrscale=corrscale, stdscale=stdscale, margin=margin, std_span=std_span,
                     precision=precision, want_rays=want_rays, want_points=want_normals, device=dev)
    valid, depths = raw["valid"], raw["depths"]
    kept_t = valid.sum(dtype=torch.float64)
    mean = (depths[:, 0].double().sum() / kept_t.clamp(min=1.0)).float()            # the invalid entries are zero
    depths[:, 0] = torch.where(valid > 0, depths[:, 0], mean)
    outside, duplicates, skipped, unsampled = raw["counts"].tolist()
    res = {"depths": depths, "valid_depth": valid, "depth_std": raw["depth_std"], "shape": raw["shape"], "outside": outside,
           "duplicates": duplicates, "skipped": skipped, "unsampled": unsampled, "kept": int(kept_t.item())}
    if want_rays:
        res["rays"] = raw["rays"]
    if want_normals:
        normals, valid_normal = Fn.point_normals(raw["points"].double(), raw["valid_full"], _PRECISION[precision] == 1)
        up = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float32, device=dev)
        normals = torch.where(valid_normal[..., None] > 0, normals, up)
        rows, cols = raw["src_rows"], raw["src_cols"]
        res["normals"] = normals[rows][:, cols].reshape(-1, 3).contiguous()
        res["valid_normal"] = valid_normal[rows][:, cols].reshape(-1).contiguous()
    return res


@torch.no_grad()
def ray_table(views, images, center, range=None, cs="utm", zone=None, south=False, precision="reference", device=None, seed=0,
              chunk=None, priors=None, corrscale=1.0, stdscale=1.0, margin=1e-4, std_span=0.0, want_normals=False):
    """The views of a scene as one RayTable (load_data, :311-394, and with `priors` load_depth_data, :401-548: the whole of
    load_train_split without the file readers): views as scene_bounds takes them, each with "sun": (elevation_deg, azimuth_deg);
    images: per view the (H W, 3) colours, row-major.  cs='utm' without a zone: the zone of the first view's lat / lon offset.
    priors: per view None or {"pts2d", "pts3d", "correl"} (depth_priors; corrscale, stdscale, margin - upstream's --margin
    1e-4 - and std_span are its parameters): the table gains depths, valid_depth and depth_std, a view with None has
    valid_depth = 0 rows.  A view's "H", "W" are its ray grid - the image AFTER its "downscale"; the tie points of a downscaled
    view are at full resolution, which the view names as "full_H", "full_W" (their resize must be H x W).  priors=None: the
    table without depth columns.  want_normals (with priors): the table also gains depth_priors' normals and valid_normal - what
    FusedTrainer's nr_spv_type 2 / 3 read; a view with None has the normal (0, 0, 1) and valid_normal = 0.
    A view's priors may also be {"dsm": (h, w) float32 on the device, "grid": dsm.Grid} with an optional "weight" (default 1): a
    surface model in place of tie points - its columns are raycast.surface_priors of the view's own rays (stdscale, margin,
    std_span as above).  It needs cs='utm'; with want_normals such a view has the normal (0, 0, 1) and valid_normal = 0."""
    from .raytable import RayTable
    if len(views) != len(images) or not views:
        raise ValueError(f"ray_table: {len(views)} views and {len(images)} images")
    if priors is not None and len(priors) != len(views):
        raise ValueError(f"ray_table: {len(views)} views and {len(priors)} priors")
    if priors is not None and cs != "utm":
        for i, p in enumerate(priors):
            if isinstance(p, dict) and ("dsm" in p or "grid" in p):
                raise ValueError(f"ray_table: the surface prior of view {i} needs cs='utm', not {cs!r}: a surface model is cast in a "
                                 "frame whose world axes are (east, north, up)")
    tables, cols = [], {"depths": [], "valid_depth": [], "depth_std": []}
    if want_normals:
        if priors is None:
            raise ValueError("ray_table: want_normals needs priors (the normals come from the tie points)")
        cols.update(normals=[], valid_normal=[])
    for i, (v, img) in enumerate(zip(views, images)):
        rpc, H, W, min_alt, max_alt = _view_args(v)
        if cs == "utm" and zone is None:
            zone = utm_zone(rpc.lat_offset, rpc.lon_offset)
        if tuple(img.shape) != (H * W, 3):
            raise ValueError(f"ray_table: an image of shape {tuple(img.shape)} for a view of {H} x {W} pixels ({H * W}, 3)")
        rays, _ = view_rays(rpc, H, W, min_alt, max_alt, center, range, cs=cs, zone=zone, south=south, sun=v["sun"], chunk=chunk,
                            precision=precision, device=device)
        tables.append(rays)
        if priors is None:
            continue
        if priors[i] is None:
            pr = {"depths": torch.zeros((H * W, 2), device=rays.device), "valid_depth": torch.zeros((H * W,), device=rays.device),
                  "depth_std": torch.zeros((H * W,), device=rays.device)}
            if want_normals:
                pr["normals"] = torch.tensor([0.0, 0.0, 1.0], device=rays.device).repeat(H * W, 1)
                pr["valid_normal"] = torch.zeros((H * W,), device=rays.device)
        elif "dsm" in priors[i] or "grid" in priors[i]:
            from .dsm import SceneFrame
            from .raycast import surface_priors
            missing = [k for k in ("dsm", "grid") if k not in priors[i]]
            if missing:
                raise ValueError(f"ray_table: the surface prior of view {i} lacks {missing}")
            pr = surface_priors(rays, SceneFrame(*_frame(center, range, cs), cs="utm"), priors[i]["dsm"], priors[i]["grid"],
                                weight=priors[i].get("weight", 1.0), stdscale=stdscale, margin=margin, std_span=std_span)
            if want_normals:                   # a raster's normals are not served: the view's rows carry no normal target
                pr["normals"] = torch.tensor([0.0, 0.0, 1.0], device=rays.device).repeat(H * W, 1)
                pr["valid_normal"] = torch.zeros((H * W,), device=rays.device)
        else:
            missing = [k for k in ("pts2d", "pts3d", "correl") if k not in priors[i]]
            if missing:
                raise ValueError(f"ray_table: the priors of view {i} lack {missing}")
            down = float(v.get("downscale", 1.0))
            if down != 1.0 and not ("full_H" in v and "full_W" in v):
                raise ValueError(f"ray_table: view {i} is downscaled by {down}: its priors need full_H and full_W")
            pr = depth_priors(rpc, int(v.get("full_H", H)), int(v.get("full_W", W)), priors[i]["pts2d"], priors[i]["pts3d"],
                              priors[i]["correl"], min_alt, max_alt, center, range, cs=cs, zone=zone, south=south, downscale=down,
                              corrscale=corrscale, stdscale=stdscale, margin=margin, std_span=std_span, precision=precision,
                              want_normals=bool(want_normals), device=rays.device)
            if pr["shape"] != (H, W):
                raise ValueError(f"ray_table: the priors of view {i} come out {pr['shape'][0]} x {pr['shape'][1]}, its rays are {H} x {W}")
        for k in cols:
            cols[k].append(pr[k].float())
    rays = torch.cat(tables, 0)
    rgbs = torch.cat([torch.as_tensor(img).to(rays.device).float() for img in images], 0)
    if priors is None:
        return RayTable(rays, rgbs, device=rays.device, seed=seed)
    return RayTable(rays, rgbs, **{k: torch.cat(v, 0) for k, v in cols.items()}, device=rays.device, seed=seed)


__all__ = ["Rpc", "utm_zone", "sun_direction", "project", "localize", "geo_world", "ecef_geodetic", "utm_geodetic", "view_direction",
           "view_rays", "scene_bounds",
           "ray_table", "nearest_lines", "tie_priors", "depth_priors"]
