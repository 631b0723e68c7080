"""The digital surface model (DSM) of a rendered view and its altitude MAE, on the device and bitwise reproducible.

The reference's evaluation reports PSNR, SSIM and the altitude MAE of the DSM per view (eval.py:467-479); the DSM comes from a
host path: get_latlonalt_from_nerf_prediction builds the point cloud in numpy (datasets/satellite_rgb_dep.py:601-634),
plyflatten(cloud, xoff, yoff, resolution, xsize, ysize, radius=1, sigma=inf) rasterises it (:636-699), and GeoTIFF round trips
through rasterio / gdal compute the MAE (sat_utils.py:185-350).  Here:

  SceneFrame       the dataset's normalisation (center, range; :622-625) and its coordinate system: 'utm', or 'ecef' with the
                   scene's UTM zone (SceneFrame.ecef takes it from the centre)
  Grid             the raster: from_cloud (the bounds rule of :665-671) or from_roi (the ground truth's grid, :658-663)
  point_cloud      (east, north, altitude) of every ray in float64 (:613-633); altitude_image its third column (eval.py:170-172)
  DsmAccumulator   bn_dsm_splat (an 'ecef' frame: bn_dsm_splat_world) into an int64 (sum, count) grid - chunk by chunk, view by
                   view, rank by rank - and bn_dsm_resolve; add_points for world points that already are (east, north, altitude)
  tie_point_dsm    the DSM of a view's tie points (datasets/cal_rmse_depth.py:15-64, 115-121): how the depth priors are judged
  dsm_image        render_image's walk (viewwalk.py) with each chunk's depth splatted as it is produced (fill=True: and the holes
                   filled, fill.fill_holes)
  altitude_mae     the z-registered mean absolute altitude error (sat_utils.py:235, 246, 340-349)

The sums are integer (altitudes in units of 2^-20 m, added atomically), so a DSM's bits do not depend on the order of the rays, on
the chunking, or on how many GPUs shared the view: DsmAccumulator.merge is one SUM all-reduce.

An 'ecef' scene goes through include/brdfnerf_hip.h's "World points of an ECEF scene" on the device (sat_utils.
ecef_to_latlon_custom as written, then the UTM series of camera.geo_world in the frame's zone), converted ONCE: upstream's own
get_dsm_from_nerf_prediction converts an ECEF cloud twice (:649-651 on top of :629-631) and rasterises garbage; the reading
here is the one its altitude image takes (eval.py:170).  Refused by name: cs='ecef' without the scene's zone.  Only sigma = inf,
the unweighted mean upstream always asks for, is served.  The footprint (a disc of `radius` cells, or the square) is the rule
bn_dsm_splat states in include/brdfnerf_hip.h; it was not checked against the plyflatten package, which this project does not depend on.
"""
import math

import torch

from . import _lib as L
from . import functions as Fn

_FOOTPRINTS = {"disc": L.BN_DSM_DISC, "square": L.BN_DSM_SQUARE}


class SceneFrame:
    """The normalisation of a scene (datasets/satellite_rgb_dep.py:622-625): world = normalised * range + center, float64.
    cs: the coordinate system of `center`.  'utm': a world point is (east, north, altitude), :632-633; a zone or south given is
    kept and plays no part.  'ecef': a world point goes through the rule of include/brdfnerf_hip.h ("World points of an ECEF
    scene") into the UTM `zone` (1 to 60) of the SCENE - upstream takes the zone from the first point of each call
    (sat_utils.py:156-159) - with south=False adding no false northing, as upstream's "+proj=utm +zone=17R" does in both
    hemispheres.  SceneFrame.ecef takes the zone of the centre."""

    def __init__(self, center, range, cs="utm", zone=None, south=False):
        if cs not in ("utm", "ecef"):
            raise ValueError(f"SceneFrame: unknown coordinate system {cs!r} ('utm' or 'ecef')")
        if zone is not None and not 1 <= int(zone) <= 60:
            raise ValueError(f"SceneFrame: zone {zone} outside 1-60")
        if cs == "ecef" and zone is None:
            raise NotImplementedError("SceneFrame: cs='ecef' without the scene's UTM zone is not served: name it (zone=, 1 to 60), or "
                                      "let SceneFrame.ecef(center, range) take the zone of the centre")
        self.center = tuple(float(c) for c in (center.tolist() if hasattr(center, "tolist") else center))
        self.range = float(range)
        self.cs = cs
        self.zone, self.south = (None if zone is None else int(zone)), bool(south)
        if len(self.center) != 3 or not all(math.isfinite(v) for v in self.center + (self.range,)):
            raise ValueError(f"SceneFrame: center {self.center} and range {self.range} must be 3 + 1 finite numbers")

    @classmethod
    def ecef(cls, center, range, zone=None, south=False):
        """The frame of an ECEF scene.  zone=None: the zone of the centre - the rule on the host in Python float64, then
        camera.utm_zone."""
        if zone is None:
            from .camera import utm_zone
            lon, lat, _ = ecef_geodetic_host(*(float(c) for c in (center.tolist() if hasattr(center, "tolist") else center)))
            zone = utm_zone(lat, lon)
        return cls(center, range, cs="ecef", zone=zone, south=south)

    def world_args(self):
        """(cs code, zone, south) as the C ABI takes them; a 'utm' frame without a zone passes 1, which nothing reads."""
        return (L.BN_CS_ECEF if self.cs == "ecef" else L.BN_CS_UTM), (1 if self.zone is None else self.zone), int(self.south)

    def __repr__(self):
        tail = "" if self.zone is None else f", zone={self.zone}, south={self.south}"
        return f"SceneFrame(center={self.center}, range={self.range}, cs={self.cs!r}{tail})"


def ecef_geodetic_host(x, y, z):
    """sat_utils.ecef_to_latlon_custom (sat_utils.py:127-146) for ONE point in Python float64, the operations of the header's rule
    in its order: -> (lon_deg, lat_deg, alt).  A point on the axis or a non-finite one is a ValueError."""
    a, e = 6378137.0, 8.1819190842622e-2
    asq, esq = a * a, e * e
    b = math.sqrt(asq * (1 - esq))
    bsq = b * b
    ep = math.sqrt((asq - bsq) / bsq)
    k1, k2 = (ep * ep) * b, esq * a
    p = math.sqrt(x * x + y * y)
    if not (p > 0 and math.isfinite(p) and math.isfinite(z)):
        raise ValueError(f"ecef_geodetic_host: ({x}, {y}, {z}) is on the axis or not finite")
    th = math.atan2(a * z, b * p)
    s, c = math.sin(th), math.cos(th)
    lon = math.atan2(y, x)
    lat = math.atan2(z + k1 * ((s * s) * s), p - k2 * ((c * c) * c))
    sl = math.sin(lat)
    alt = p / math.cos(lat) - a / math.sqrt(1 - esq * (sl * sl))
    return lon * 180 / math.pi, lat * 180 / math.pi, alt


class Grid:
    """A north-up raster: (xoff, yoff) is the corner of its north-west cell, `resolution` the cell size in metres, width x height
    its cells.  Cell (row j, column i) covers east [xoff + i res, xoff + (i + 1) res) and north (yoff - (j + 1) res, yoff - j res]:
    the affine transform (res, 0, xoff, 0, -res, yoff) of datasets/satellite_rgb_dep.py:695."""

    def __init__(self, xoff, yoff, resolution, width, height):
        self.xoff, self.yoff, self.resolution = float(xoff), float(yoff), float(resolution)
        self.width, self.height = int(width), int(height)
        if not (self.resolution > 0 and math.isfinite(self.resolution) and math.isfinite(self.xoff) and math.isfinite(self.yoff)):
            raise ValueError(f"Grid: origin ({self.xoff}, {self.yoff}) must be finite and resolution {self.resolution} positive")
        if self.width < 1 or self.height < 1 or self.width * self.height > 1 << 31:
            raise ValueError(f"Grid: {self.width} x {self.height} cells (1 to 2^31)")

    @classmethod
    def from_cloud(cls, xy_min, xy_max, resolution=0.5):
        """The grid that holds a cloud with bounds xy_min = (xmin, ymin), xy_max = (xmax, ymax): datasets/satellite_rgb_dep.py:665-671."""
        res = float(resolution)
        (xmin, ymin), (xmax, ymax) = (float(v) for v in xy_min), (float(v) for v in xy_max)
        xoff = math.floor(xmin / res) * res
        xsize = int(1 + math.floor((xmax - xoff) / res))
        yoff = math.ceil(ymax / res) * res
        ysize = int(1 - math.floor((ymin - yoff) / res))
        return cls(xoff, yoff, res, xsize, ysize)

    @classmethod
    def from_roi(cls, roi):
        """The ground truth's grid from its (x, y, size, resolution) metadata (the *_DSM.txt of a scene; :658-663): square, y is the
        SOUTHERN edge there, so yoff = y + size * resolution."""
        x, y, size, res = (float(v) for v in roi)
        size = int(size)
        return cls(x, y + size * res, res, size, size)

    def __eq__(self, other):
        return isinstance(other, Grid) and (self.xoff, self.yoff, self.resolution, self.width, self.height) == \
            (other.xoff, other.yoff, other.resolution, other.width, other.height)

    def __repr__(self):
        return f"Grid(xoff={self.xoff}, yoff={self.yoff}, resolution={self.resolution}, width={self.width}, height={self.height})"


def _rows_f32(rays, depth):
    """A chunk as the splat entries take it: the rays and the flattened depth, float32 unless they already are."""
    depth = depth.reshape(-1)
    return (rays if rays.dtype == torch.float32 else rays.float()), (depth if depth.dtype == torch.float32 else depth.float())


def _check_footprint(who, radius, footprint):
    if footprint not in _FOOTPRINTS:
        raise ValueError(f"{who}: footprint {footprint!r} ('disc' or 'square')")
    if not 0 <= int(radius) <= L.BN_DSM_MAX_RADIUS:
        raise ValueError(f"{who}: radius {radius} outside [0, {L.BN_DSM_MAX_RADIUS}]")


def _ecef_points(rays, depth, frame, what):
    """bn_surface_points of an 'ecef' frame: float64 (R, 3) = (east, north, altitude), NaN where a row is refused."""
    if not rays.is_cuda:
        raise ValueError(f"{what}: the world points of an 'ecef' frame are converted on the device; the rays are on {rays.device}")
    rays, depth = _rows_f32(rays, depth.to(rays.device))
    return Fn.surface_points(rays, depth, frame.center, frame.range, *frame.world_args(),
                             torch.zeros((1,), dtype=torch.int64, device=rays.device))


@torch.no_grad()
def point_cloud(rays, depth, frame):
    """(east, north, altitude) of every ray's surface point: (o + d depth) range + center in float64, each operation rounded on
    its own (datasets/satellite_rgb_dep.py:613-633, cs == 'utm'); an 'ecef' frame: that point through bn_surface_points (:629-631),
    NaN where it is refused.  rays (R, >= 6), depth (R,) -> float64 (R, 3) on their device."""
    if frame.cs == "ecef":
        return _ecef_points(rays, depth, frame, "point_cloud")
    rays = rays.double()
    xyz = (rays[:, 0:3] + rays[:, 3:6] * depth.double().reshape(-1, 1)) * frame.range
    return xyz + torch.tensor(frame.center, dtype=torch.float64, device=xyz.device)


@torch.no_grad()
def altitude_image(rays, depth, frame):
    """The altitude of every ray's surface point, float64 (R,): what the reference writes to depth/*.tif (eval.py:170-172).  An
    'ecef' frame: column 2 of point_cloud."""
    if frame.cs == "ecef":
        return _ecef_points(rays, depth, frame, "altitude_image")[:, 2].contiguous()
    return (rays[:, 2].double() + rays[:, 5].double() * depth.double().reshape(-1)) * frame.range + frame.center[2]


def _cloud_grid(rays, depth, frame, resolution):
    """Grid.from_cloud of the finite points of a view."""
    xy = point_cloud(rays, depth, frame)
    xy = xy[torch.isfinite(xy).all(-1)][:, :2]
    if xy.shape[0] == 0:
        raise ValueError("dsm: no ray of the view has a finite surface point, so the cloud has no bounds (pass grid=)")
    return Grid.from_cloud(xy.min(0).values.tolist(), xy.max(0).values.tolist(), resolution)


class DsmAccumulator:
    """The (sum, count) grid of a DSM on `device`: int64 (H, W, 2), altitudes summed in units of 2^-20 m.
      add(rays, depth, frame)   splat one chunk (bn_dsm_splat; an 'ecef' frame: bn_dsm_splat_world); chunks of a view, and
                                several views, accumulate - a fused multi-view DSM is every view added to one accumulator
      add_points(enz)           splat world points that already are (east, north, altitude): float64 (n, >= 3) (bn_dsm_splat_points)
      merge(group)              SUM all-reduce over the ranks of a group: every rank then holds the whole (call it once)
      result()                  -> dsm (H, W) float32, NaN where no point fell (the reference's nodata), count (H, W) int32
      skipped                   rows left out so far: non-finite point, or |altitude| >= 2^23 m (an 'ecef' frame: also a point on
                                the axis)
    radius: cells around a point's own that also receive it (0 to 4; upstream: 1); footprint 'disc' (k1^2 + k2^2 <= radius^2) or
    'square'.  Integer sums: the accumulator's bits depend on the set of rays alone."""

    def __init__(self, grid, device, radius=1, footprint="disc"):
        _check_footprint("DsmAccumulator", radius, footprint)
        self.grid, self.radius, self.footprint = grid, int(radius), footprint
        self.acc = torch.zeros((grid.height, grid.width, 2), dtype=torch.int64, device=device)
        self._skipped = torch.zeros((1,), dtype=torch.int64, device=device)

    @torch.no_grad()
    def add(self, rays, depth, frame):
        g = self.grid
        rays, depth = _rows_f32(rays, depth)
        if frame.cs == "ecef":
            Fn.dsm_splat_world(rays, depth, frame.center, frame.range, g.xoff, g.yoff, g.resolution, self.radius,
                               _FOOTPRINTS[self.footprint], *frame.world_args(), self.acc, self._skipped)
        else:
            Fn.dsm_splat(rays, depth, frame.center, frame.range, g.xoff, g.yoff, g.resolution, self.radius, _FOOTPRINTS[self.footprint],
                         self.acc, self._skipped)
        return self

    @torch.no_grad()
    def add_points(self, enz):
        g = self.grid
        enz = torch.as_tensor(enz, dtype=torch.float64).to(self.acc.device)
        if enz.dim() != 2 or enz.shape[1] < 3:
            raise ValueError(f"DsmAccumulator.add_points: points must be (n, >= 3) = (east, north, altitude), got {tuple(enz.shape)}")
        if enz.shape[0]:
            Fn.dsm_splat_points(enz, g.xoff, g.yoff, g.resolution, self.radius, _FOOTPRINTS[self.footprint], self.acc, self._skipped)
        return self

    def merge(self, group=None):
        from .distributed import allreduce_
        for t in (self.acc, self._skipped):
            allreduce_(t, group=group)
        return self

    @property
    def skipped(self):
        return int(self._skipped.item())

    @torch.no_grad()
    def result(self):
        return Fn.dsm_resolve(self.acc)


@torch.no_grad()
def dsm_image(models, args, rays, frame, grid=None, chunk=None, group=None, radius=1, footprint="disc", resolution=0.5, fill=False,
              **render_kw):
    """evaluate.render_image with the surface model as its output: the same shard bounds, the same chunks and, after the same
    torch.manual_seed, the same draws - `depth` is render_image's depth bit for bit - and each chunk's depth_coarse is splatted
    into the DSM as it is produced; nothing larger than a chunk's outputs is held.  Under data parallelism every rank splats its
    own share and the accumulators are summed (DsmAccumulator.merge): the result is bitwise the single-process one.
    grid=None: the grid comes from the bounds of the cloud (Grid.from_cloud at `resolution`), which needs every depth first - the
    depths are kept (4 bytes per ray) and splatted after the last chunk.  render_kw: apply_brdf, cos_irra_on, ... as render_image.
    fill=True: also the surface model the reference publishes (the *_Grid.tif of save_dsm_grid, eval.py:135-149): every NaN cell
    replaced by its nearest known cell (fill.fill_holes; with a group each rank fills a band of rows).
    -> {"dsm" (H, W) float32, "count" (H, W) int32, "depth" (R,), "altitude" (R,) float64, "grid", "skipped"}
    (+ "dsm_grid" (H, W) float32 without NaN, "holes", "max_dist" with fill)"""
    from .rendering import render_rays
    from .viewwalk import ViewWalk
    walk = ViewWalk(rays.shape[0], chunk or args.chunk, group)
    acc = None if grid is None else DsmAccumulator(grid, rays.device, radius, footprint)
    parts = []
    for i, j in walk.chunks():
        out, _ = render_rays(models, args, rays[i:j], None, mode="test", **render_kw)
        parts.append(out["depth_coarse"])
        if acc is not None:
            acc.add(rays[i:j], parts[-1], frame)
    depth = walk.join(parts, (), rays.dtype, rays.device)
    if acc is None:
        grid = _cloud_grid(rays, depth, frame, resolution)
        acc = DsmAccumulator(grid, rays.device, radius, footprint).add(rays[walk.lo:walk.hi], depth[walk.lo:walk.hi], frame)
    acc.merge(group)
    dsm, count = acc.result()
    res = {"dsm": dsm, "count": count, "depth": depth, "altitude": altitude_image(rays, depth, frame), "grid": grid,
           "skipped": acc.skipped}
    if fill:
        from .fill import fill_holes
        filled = fill_holes(dsm, group=group)
        res.update(dsm_grid=filled["filled"], holes=filled["holes"], max_dist=filled["max_dist"])
    return res


@torch.no_grad()
def tie_point_dsm(pts3d, cs="utm", zone=None, south=False, grid=None, resolution=0.5, radius=1, footprint="disc", fill=True, device=None):
    """The DSM of a view's tie points - get_dsm_from_dense_depth and the grid fill of datasets/cal_rmse_depth.py:15-64, 115-121 -
    from the content of its *_3DPts.txt (cs='utm': rows of east, north, altitude) or *_3DPts_ecef.txt (cs='ecef': rows of x, y, z,
    taken through camera.ecef_geodetic and camera.geo_world into the scene's `zone`, which cs='ecef' needs).  pts3d (T, 3).
    grid=None: Grid.from_cloud of the finite points at `resolution`, as upstream.  The result goes straight into altitude_mae,
    register.altitude_mae_xy and metrics.normal_angle_mae.
    -> {"dsm" (H, W) float32, "count" (H, W) int32, "grid", "skipped", "points" float64 (T, 3) = (east, north, altitude)}
    (+ "dsm_grid" without NaN, "holes", "max_dist" with fill, as dsm_image)."""
    from . import camera
    frame = SceneFrame((0.0, 0.0, 0.0), 1.0, cs=cs, zone=zone, south=south)               # the refusals of the coordinate system
    pts = torch.as_tensor(pts3d, dtype=torch.float64)
    pts = pts.to(camera._device(device, pts)).reshape(-1, 3)
    if frame.cs == "ecef":
        lonlat, alt = camera.ecef_geodetic(pts)
        pts = camera.geo_world(lonlat, alt, cs="utm", zone=frame.zone, south=frame.south)
    if grid is None:
        xy = pts[torch.isfinite(pts).all(-1)][:, :2]
        if xy.shape[0] == 0:
            raise ValueError("tie_point_dsm: no tie point is finite, so the cloud has no bounds (pass grid=)")
        grid = Grid.from_cloud(xy.min(0).values.tolist(), xy.max(0).values.tolist(), resolution)
    acc = DsmAccumulator(grid, pts.device, radius, footprint).add_points(pts)
    dsm, count = acc.result()
    res = {"dsm": dsm, "count": count, "grid": grid, "skipped": acc.skipped, "points": pts}
    if fill:
        from .fill import fill_holes
        filled = fill_holes(dsm)
        res.update(dsm_grid=filled["filled"], holes=filled["holes"], max_dist=filled["max_dist"])
    return res


def altitude_mae(dsm, gt, mask=None):
    """Mean absolute altitude error of a DSM against the ground truth on the SAME grid, after the z-only registration the reference
    falls back to without dsmr (sat_utils.py:235, 246, 340-349), in float64; NaN cells of either image are left out (nanmean):
      pred_r = pred + nanmean(gt - pred) ;  diff = pred_r - gt ;  mae = nanmean(|diff|)
    mask (bool, True inside; MaskDoD, sat_utils.py:278-297): also mae_in over the cells inside and mae_out over the others.
    Plain torch on the tensors' device (host tensors too).  -> {"mae", "shift", "diff"} (+ "mae_in", "mae_out").
    The xy registration of dsmr - the path the reference takes when dsmr imports - is register.altitude_mae_xy.  Not covered:
    GeoTIFF I/O.  The normal-angle MAE (mae_nr) is metrics.normal_angle_mae."""
    pred, gt = torch.as_tensor(dsm).double(), torch.as_tensor(gt).double()
    if pred.shape != gt.shape:
        raise ValueError(f"altitude_mae: dsm {tuple(pred.shape)} and ground truth {tuple(gt.shape)} are not on one grid")
    gt = gt.to(pred.device)
    shift = torch.nanmean(gt - pred)
    diff = (pred + shift) - gt
    res = {"mae": float(torch.nanmean(diff.abs())), "shift": float(shift), "diff": diff}
    if mask is not None:
        mask = torch.as_tensor(mask).to(diff.device) != 0
        nan = torch.full_like(diff, float("nan"))
        res["mae_in"] = float(torch.nanmean(torch.where(mask, diff, nan).abs()))
        res["mae_out"] = float(torch.nanmean(torch.where(mask, nan, diff).abs()))
    return res


__all__ = ["SceneFrame", "Grid", "point_cloud", "altitude_image", "DsmAccumulator", "dsm_image", "tie_point_dsm", "altitude_mae"]
