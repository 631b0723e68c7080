"""The digital surface model (DSM) of a rendered view and its altitude MAE, on the device and bitwise reproducible.

The reference's evaluation reports PSNR, SSIM and the altitude MAE of the DSM per view (eval.py:467-479); the DSM comes from a
host path: get_latlonalt_from_nerf_prediction builds the point cloud in numpy (datasets/satellite_rgb_dep.py:601-634),
plyflatten(cloud, xoff, yoff, resolution, xsize, ysize, radius=1, sigma=inf) rasterises it (:636-699), and GeoTIFF round trips
through rasterio / gdal compute the MAE (sat_utils.py:185-350).  Here:

  SceneFrame       the dataset's normalisation (center, range; :622-625), `utm` coordinates
  Grid             the raster: from_cloud (the bounds rule of :665-671) or from_roi (the ground truth's grid, :658-663)
  point_cloud      (east, north, altitude) of every ray in float64 (:613-633); altitude_image its third column (eval.py:170-172)
  DsmAccumulator   bn_dsm_splat into an int64 (sum, count) grid - chunk by chunk, view by view, rank by rank - and bn_dsm_resolve
  dsm_image        render_image's walk (viewwalk.py) with each chunk's depth splatted as it is produced (fill=True: and the holes
                   filled, fill.fill_holes)
  altitude_mae     the z-registered mean absolute altitude error (sat_utils.py:235, 246, 340-349)

The sums are integer (altitudes in units of 2^-20 m, added atomically), so a DSM's bits do not depend on the order of the rays, on
the chunking, or on how many GPUs shared the view: DsmAccumulator.merge is one SUM all-reduce.

Refused by name: cs='ecef' (geodetic conversion and the utm package).  Only sigma = inf, the unweighted mean upstream always
asks for, is served.  The footprint (a disc of `radius` cells, or the square) is the rule bn_dsm_splat states in
include/brdfnerf_hip.h; it was not checked against the plyflatten package, which this project does not depend on.
"""
import math

import torch

from . import _lib as L
from . import functions as Fn

_FOOTPRINTS = {"disc": L.BN_DSM_DISC, "square": L.BN_DSM_SQUARE}


class SceneFrame:
    """The normalisation of a scene (datasets/satellite_rgb_dep.py:622-625): world = normalised * range + center, float64.
    cs: the coordinate system of `center`; only 'utm' - a world point is (east, north, altitude), :632-633 - is served."""

    def __init__(self, center, range, cs="utm"):
        if cs == "ecef":
            raise NotImplementedError("SceneFrame: cs='ecef' is not served: it needs the ECEF -> geodetic -> UTM conversion of "
                                      "sat_utils.ecef_to_latlon_custom / utm_from_latlon; only cs='utm' is")
        if cs != "utm":
            raise ValueError(f"SceneFrame: unknown coordinate system {cs!r} ('utm')")
        self.center = tuple(float(c) for c in (center.tolist() if hasattr(center, "tolist") else center))
        self.range = float(range)
        self.cs = cs
        if len(self.center) != 3 or not all(math.isfinite(v) for v in self.center + (self.range,)):
            raise ValueError(f"SceneFrame: center {self.center} and range {self.range} must be 3 + 1 finite numbers")

    def __repr__(self):
        return f"SceneFrame(center={self.center}, range={self.range}, cs={self.cs!r})"


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


@torch.no_grad()
def point_cloud(rays, depth, frame):
    """(east, north, altitude) of every ray's surface point: (o + d depth) range + center in float64, each operation rounded on
    its own (datasets/satellite_rgb_dep.py:613-633, cs == 'utm').  rays (R, >= 6), depth (R,) -> float64 (R, 3) on their device."""
    rays = rays.double()
    xyz = (rays[:, 0:3] + rays[:, 3:6] * depth.double().reshape(-1, 1)) * frame.range
    return xyz + torch.tensor(frame.center, dtype=torch.float64, device=xyz.device)


@torch.no_grad()
def altitude_image(rays, depth, frame):
    """The altitude of every ray's surface point, float64 (R,): what the reference writes to depth/*.tif (eval.py:170-172)."""
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
      add(rays, depth, frame)   splat one chunk (bn_dsm_splat); chunks of a view, and several views, accumulate - a fused
                                multi-view DSM is every view added to one accumulator
      merge(group)              SUM all-reduce over the ranks of a group: every rank then holds the whole (call it once)
      result()                  -> dsm (H, W) float32, NaN where no point fell (the reference's nodata), count (H, W) int32
      skipped                   rows left out so far: non-finite point, or |altitude| >= 2^23 m
    radius: cells around a point's own that also receive it (0 to 4; upstream: 1); footprint 'disc' (k1^2 + k2^2 <= radius^2) or
    'square'.  Integer sums: the accumulator's bits depend on the set of rays alone."""

    def __init__(self, grid, device, radius=1, footprint="disc"):
        if footprint not in _FOOTPRINTS:
            raise ValueError(f"DsmAccumulator: footprint {footprint!r} ('disc' or 'square')")
        if not 0 <= int(radius) <= L.BN_DSM_MAX_RADIUS:
            raise ValueError(f"DsmAccumulator: radius {radius} outside [0, {L.BN_DSM_MAX_RADIUS}]")
        self.grid, self.radius, self.footprint = grid, int(radius), footprint
        self.acc = torch.zeros((grid.height, grid.width, 2), dtype=torch.int64, device=device)
        self._skipped = torch.zeros((1,), dtype=torch.int64, device=device)

    @torch.no_grad()
    def add(self, rays, depth, frame):
        g = self.grid
        depth = depth.reshape(-1)
        Fn.dsm_splat(rays if rays.dtype == torch.float32 else rays.float(), depth if depth.dtype == torch.float32 else depth.float(),
                     frame.center, frame.range, g.xoff, g.yoff, g.resolution, self.radius, _FOOTPRINTS[self.footprint], self.acc,
                     self._skipped)
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


__all__ = ["SceneFrame", "Grid", "point_cloud", "altitude_image", "DsmAccumulator", "dsm_image", "altitude_mae"]
