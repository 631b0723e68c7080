"""Horizon and sky-view factor of a surface model on the device: how much of the sky does a cell, or a pixel, see?

The reference's irradiance is sun_v + (1 - sun_v) * sky.  visibility.py computes what the geometry implies for the first term: a
shadow march per sun.  This module computes the geometric counterpart of the second: per start and azimuth the tangent of the
horizon's elevation (the HORIZON TABLE, which also answers "is this start shadowed for a sun at elevation e" for every e at once:
slope > tan e), and its average cos^2 over the azimuths, the SKY-VIEW FACTOR of an isotropic sky for a level surface.

  azimuths          n evenly spaced azimuths as (east, north) rows on the host
  grid_horizon      every cell of a DSM as a start (bn_grid_horizon): the horizon table (D, H, W)
  sky_view_factor   the table walked dir_tile azimuths at a time into one float64 accumulator (bn_sky_view): svf (H, W)
  point_sky_view    world points (east, north, altitude) as starts (bn_points_horizon)
  view_sky_view     point_cloud of a view's depth, then point_sky_view: the ambient map of a VIEW under the geometry of a DSM

The rule (include/brdfnerf_hip.h, "Horizon and sky view over a surface model", states it as the ABI's contract).  An azimuth
(dx, dy) is a horizontal (east, north) vector and need not be normalised; the host computes it and the device evaluates no sin or
cos.  With a = max(|dx|, |dy|) a step moves (dx / a, -(dy / a)) cells - exactly one cell along the dominant axis - over
L = sqrt(su^2 + sv^2) res metres of ground.  At step t = 1, 2, ... the march is at u0 + t su, v0 + t sv (the product with t, never
a running sum), reads the cell it is over and keeps s = (h - z0) / (t L) if it is STRICTLY greater than the best so far, which
starts at 0: the first cell wins a tie, a NaN cell never raises the horizon, and 0 stands for an open, level horizon beyond the
grid's edge.  slope = (float)best.  The sky view adds 1 / (1 + s^2) of the STORED float32 slopes in ascending azimuth order into a
float64 accumulator, one at a time, and divides by D at the end; a NaN slope (a start without data) makes svf NaN.  Everything is
float64 with each operation rounded on its own, so every bit of `slope`, `hit`, `svf` and `sums` depends on the grid, the starts
and the azimuths alone: not on row bands (rows=), on how the azimuths are tiled (dir_tile=), or on how many GPUs shared the grid
(gridwalk.py: bands gathered, sums merged by one SUM all-reduce).

max_dist (metres) becomes max_steps = max(1, floor(max_dist / resolution)): it bounds the march in CELLS ALONG THE DOMINANT AXIS, so
the starts looked at lie in a square window of that half-side around the start, not in a disc: along a diagonal the march reaches
sqrt(2) max_dist.

lift (metres, point and view modes) is added to the points' altitude before the march.  A DSM made of the very points that are
tested holds, per cell, the MEAN altitude of several points: a point slightly below its neighbour cell's mean sees a horizon that
the surface does not have - the situation `eps` answers in visibility.py.  A small lift forgives it.

Refused by name: host tensors, a grid that is not float32, 2-D and contiguous, points that are not float64 (R, 3), azimuths that are
not finite or are (0, 0), more than 4096 azimuths, a max_dist or resolution that is not positive, rows outside [0, H], a dir_tile
below 1, a lift that is not finite, an 'ecef' frame.

Not covered: interpolated heights; tilted receiving surfaces (the SVF is for a level one); an anisotropic sky; terrain beyond the
grid (the horizon there is level); ECEF frames; using the SVF inside relight or score_view; GeoTIFF I/O.
"""
import math

import torch

from . import functions as Fn
from .gridwalk import GridWalk
from .visibility import _on_grid, _zmax

SVF_FIX = 1 << 30


def azimuths(n, start_deg=0.0):
    """n azimuths az_k = start_deg + 360 k / n degrees, clockwise from north (relight.directions' convention), as (n, 2) float64
    rows (sin az_k, cos az_k) = (east, north) on the host."""
    n = int(n)
    if n < 1:
        raise ValueError(f"azimuths: n {n} must be at least 1")
    az = [math.radians(float(start_deg) + 360.0 * k / n) for k in range(n)]
    return torch.tensor([[math.sin(a), math.cos(a)] for a in az], dtype=torch.float64).reshape(n, 2)


def _max_steps(name, max_dist, resolution):
    """max_dist metres -> the march's bound in cells along the dominant axis (None: the whole grid)."""
    if max_dist is None:
        return None
    max_dist, resolution = float(max_dist), float(resolution)
    if not (max_dist > 0) or math.isnan(max_dist):
        raise ValueError(f"{name}: max_dist {max_dist} must be positive")
    if not (resolution > 0 and math.isfinite(resolution)):
        raise ValueError(f"{name}: resolution {resolution} must be positive and finite")
    return max(1, int(min(math.floor(max_dist / resolution), (1 << 31) - 1)))


def _tile(name, dir_tile, D):
    step = D if dir_tile is None else int(dir_tile)
    if step < 1:
        raise ValueError(f"{name}: dir_tile {dir_tile} must be at least 1")
    return step


@torch.no_grad()
def grid_horizon(dsm, resolution, az, max_dist=None, rows=None, group=None, want_hit=False):
    """The horizon table of a DSM.  dsm: (H, W) float32 on the device, contiguous, NaN = no data; resolution: the cell size in
    metres; az: (D, 2) or (2,), any float dtype, (east, north) - azimuths() makes them.  max_dist (metres) bounds the march in
    cells along the dominant axis: a square window, not a disc.  rows, group: as in grid_visibility - with a group of more than one
    rank each rank marches its band, the bands are gathered and every rank returns the single-process bits; a lone band leaves
    NaN (and hit -1) outside it.
    -> {"slope" (D, H, W) float32: the tangent of the horizon's elevation, floored at 0, NaN for a cell without data, "hit" (D, H, W)
    int32 with want_hit, else None: the flat index of the cell that made the horizon, or -1}."""
    name = "grid_horizon"
    Fn._need(name, dsm, **Fn.VIS_DSM)
    az = Fn._horizon_az(name, az)
    steps = _max_steps(name, max_dist, resolution)
    H, W = dsm.shape
    D = az.shape[0]
    walk = GridWalk(name, H, rows, group)
    Fn._horizon_scalars(name, resolution, steps, 0.0)
    Fn._on_device(name, dsm)
    slope = walk.buffer((D, H, W), torch.float32, float("nan"), dsm.device)
    hit = walk.buffer((D, H, W), torch.int32, -1, dsm.device) if want_hit else None
    Fn.grid_horizon(dsm, resolution, az, steps, _zmax(dsm), rows=walk.rows, slope=slope, hit=hit)
    return {"slope": walk.join(slope, 1), "hit": walk.join(hit, 1) if want_hit else None}


def _svf_result(svf, sums, D):
    sums = sums.cpu()
    return {"svf": svf, "mean": Fn.fixed_mean(int(sums[0]), int(sums[1]), SVF_FIX), "sums": sums, "n_az": D}


@torch.no_grad()
def sky_view_factor(dsm, resolution, n_az=32, start_deg=0.0, az=None, max_dist=None, rows=None, group=None, dir_tile=8,
                    want_slope=False):
    """The sky-view factor of every cell of a DSM: the mean over the azimuths of cos^2 of the horizon's elevation.  The azimuths
    are azimuths(n_az, start_deg) unless `az` (D, 2) names them.  The table is walked dir_tile azimuths at a time - one
    (dir_tile, H, W) slope tile, then bn_sky_view into ONE float64 accumulator - so it is never held unless want_slope; dir_tile
    changes no bit.  max_dist, rows, group: as in grid_horizon; a lone band leaves NaN outside it and sums only its rows.
    -> {"svf" (H, W) float32 in [0, 1], NaN for a cell without data, "mean" = sums[0] / (sums[1] 2^30), "sums" (3,) int64 on the
    host = (sum of llrint(svf 2^30) over the non-NaN cells, their count, the NaN count), "n_az" = D} (+ "slope" (D, H, W))."""
    name = "sky_view_factor"
    Fn._need(name, dsm, **Fn.VIS_DSM)
    az = Fn._horizon_az(name, azimuths(n_az, start_deg) if az is None else az)
    steps = _max_steps(name, max_dist, resolution)
    H, W = dsm.shape
    D = az.shape[0]
    step = _tile(name, dir_tile, D)
    walk = GridWalk(name, H, rows, group)
    Fn._horizon_scalars(name, resolution, steps, 0.0)
    Fn._on_device(name, dsm)
    zmax = _zmax(dsm)
    dev = dsm.device
    cells = (walk.rows[0] * W, walk.rows[1] * W)
    table = walk.buffer((D, H, W), torch.float32, float("nan"), dev) if want_slope else None
    tile = None if want_slope else torch.empty((min(step, D), H, W), dtype=torch.float32, device=dev)
    acc = torch.zeros((H, W), dtype=torch.float64, device=dev)
    svf = walk.buffer((H, W), torch.float32, float("nan"), dev)
    sums = torch.zeros((3,), dtype=torch.int64, device=dev)
    for k0 in range(0, D, step):
        k1 = min(D, k0 + step)
        part = table[k0:k1] if want_slope else tile[:k1 - k0]
        Fn.grid_horizon(dsm, resolution, az[k0:k1], steps, zmax, rows=walk.rows, slope=part)
        last = k1 == D
        Fn.sky_view(part, acc, D, cells=cells, svf=svf if last else None, sums=sums if last else None, last=last)
    res = _svf_result(walk.join(svf, 0), walk.merge(sums), D)
    if want_slope:
        res["slope"] = walk.join(table, 1)
    return res


@torch.no_grad()
def point_sky_view(points, dsm, grid, n_az=32, start_deg=0.0, az=None, max_dist=None, dir_tile=8, want_slope=False, lift=0.0):
    """The sky-view factor of world points over a DSM.  points: float64 (R, 3) = (east, north, altitude) on the device, what
    point_cloud returns; dsm: (grid.height, grid.width) float32 on `grid`; lift (metres) is added to the altitudes first.  A point
    that is not finite, or not over the grid, has no data: svf NaN.
    -> sky_view_factor's result with "svf" (R,) (+ "slope" (D, R))."""
    name = "point_sky_view"
    points = Fn._need(name, points, **Fn.VIS_POINTS)
    _on_grid(name, dsm, grid)
    az = Fn._horizon_az(name, azimuths(n_az, start_deg) if az is None else az)
    steps = _max_steps(name, max_dist, grid.resolution)
    D = az.shape[0]
    step = _tile(name, dir_tile, D)
    lift = float(lift)
    if not math.isfinite(lift):
        raise ValueError(f"{name}: lift {lift} must be finite")
    Fn._on_device(name, points, dsm)
    if lift != 0.0:
        points = points.clone()
        points[:, 2] += lift
    R = points.shape[0]
    dev = dsm.device
    zmax = _zmax(dsm)
    acc = torch.zeros((R,), dtype=torch.float64, device=dev)
    svf = torch.empty((R,), dtype=torch.float32, device=dev)
    sums = torch.zeros((3,), dtype=torch.int64, device=dev)
    parts = []
    for k0 in range(0, D, step):
        k1 = min(D, k0 + step)
        part, _ = Fn.points_horizon(points, dsm, grid.xoff, grid.yoff, grid.resolution, az[k0:k1], steps, zmax)
        if R:
            last = k1 == D
            Fn.sky_view(part, acc, D, svf=svf if last else None, sums=sums if last else None, last=last)
        if want_slope:
            parts.append(part)
    res = _svf_result(svf, sums, D)
    if want_slope:
        res["slope"] = torch.cat(parts, 0)
    return res


@torch.no_grad()
def view_sky_view(rays, depth, frame, dsm, grid, n_az=32, start_deg=0.0, az=None, max_dist=None, dir_tile=8, want_slope=False,
                  lift=0.0):
    """The ambient map of a view under the geometry of a DSM: point_cloud(rays, depth, frame), then point_sky_view.  rays (R, >= 6),
    depth (R,) as render_image returns it, frame the scene's (a 'utm' one).  -> point_sky_view's result, "svf" (R,)."""
    from .dsm import point_cloud
    if frame.cs == "ecef":
        raise ValueError("view_sky_view: an 'ecef' frame is not served: its world axes are not (east, north, up), and the azimuths "
                         "are east and north of the scene's UTM frame")
    _on_grid("view_sky_view", dsm, grid)
    return point_sky_view(point_cloud(rays, depth.to(rays.device), frame), dsm, grid, n_az, start_deg, az, max_dist, dir_tile,
                          want_slope, lift)


__all__ = ["azimuths", "grid_horizon", "sky_view_factor", "point_sky_view", "view_sky_view"]
