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
  view_rays          get_rays + normalize_rays + get_sun_dirs of one view in one launch per chunk (bn_rpc_rays)
  scene_bounds       init_scaling_params (:238-261): the scene.loc dictionary, the centre and the range
  ray_table          the views of a scene concatenated into a RayTable (load_data, :311-394, without its file readers)
  utm_zone           the zone of a point, with the Norway and Svalbard exceptions (utm.latlon_to_zone_number)
  sun_direction      get_sun_dirs (:561-576)

precision="reference" reproduces upstream's rounding: the WORLD origin is cast to float32 (:76-77) before the centre is
subtracted (:550-559), which at a UTM northing of 3.3e6 m puts the origins on a 0.25 m lattice.  precision="exact" subtracts
and divides in float64 and rounds once.  The coordinate system is this module's own parameter (`cs`, 'utm' or 'ecef');
dsm.SceneFrame keeps refusing 'ecef'.  The UTM zone is a parameter of the scene, not taken from the first pixel of each call as
upstream does (sat_utils.py:156-159); south=False adds no false northing, which is what upstream's "+proj=utm +zone=17R" does in
both hemispheres.

Not here: the file readers (JSON, GeoTIFF), image scaling, the tie-point depth priors of load_depth_data, an inverse UTM.  The
RPC rule is the public RPC00B definition and the UTM series Karney's; neither was checked against rpcm or pyproj.
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


def _frame(center, range, cs):
    """(center (3 floats), range) from the two values or from a dsm.SceneFrame in place of `center`."""
    from .dsm import SceneFrame
    if isinstance(center, SceneFrame):
        if cs != "utm":
            raise ValueError("camera: a SceneFrame states a 'utm' scene; pass center and range with cs='ecef'")
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


@torch.no_grad()
def ray_table(views, images, center, range=None, cs="utm", zone=None, south=False, precision="reference", device=None, seed=0,
              chunk=None):
    """The views of a scene as one RayTable without depth columns (load_data, :311-394): views as scene_bounds takes them, each
    with "sun": (elevation_deg, azimuth_deg); images: per view the (H W, 3) colours, row-major.  cs='utm' without a zone: the
    zone of the first view's lat / lon offset."""
    from .raytable import RayTable
    if len(views) != len(images) or not views:
        raise ValueError(f"ray_table: {len(views)} views and {len(images)} images")
    tables = []
    for v, img in zip(views, images):
        rpc, H, W, min_alt, max_alt = _view_args(v)
        if cs == "utm" and zone is None:
            zone = utm_zone(rpc.lat_offset, rpc.lon_offset)
        if tuple(img.shape) != (H * W, 3):
            raise ValueError(f"ray_table: an image of shape {tuple(img.shape)} for a view of {H} x {W} pixels ({H * W}, 3)")
        rays, _ = view_rays(rpc, H, W, min_alt, max_alt, center, range, cs=cs, zone=zone, south=south, sun=v["sun"], chunk=chunk,
                            precision=precision, device=device)
        tables.append(rays)
    rays = torch.cat(tables, 0)
    rgbs = torch.cat([torch.as_tensor(img).to(rays.device).float() for img in images], 0)
    return RayTable(rays, rgbs, device=rays.device, seed=seed)


__all__ = ["Rpc", "utm_zone", "sun_direction", "project", "localize", "geo_world", "view_rays", "scene_bounds", "ray_table"]
