"""Sun shadows and view occlusion of a surface model on the device: which cells, or pixels, does a direction reach?

shadows.sun_visibility is the LEARNED visibility of a `--sun_v analystic` model and costs a sigma-only field pass per sun.  What
the geometry itself implies - of the lidar ground truth, of a model's own DSM - needs no field evaluation: march a ray over the
height grid from a start along a direction and report whether some cell rises above it.

  grid_visibility    every cell of a DSM as a start (bn_grid_visibility): the shadow mask of the raster under K directions
  point_visibility   world points (east, north, altitude) as starts (bn_points_visibility)
  view_visibility    point_cloud of a view's depth, then point_visibility: the shadow map of a VIEW under the geometry of a DSM

The rule (include/brdfnerf_hip.h, "Visibility over a surface model", states it as the ABI's contract).  A direction (dx, dy, dz) is
(east, north, up), pointing from the surface towards the sun or the sensor - relight.directions' convention on a UTM scene -
and need not be normalised.  With a = max(|dx|, |dy|) a step moves (dx / a, -(dy / a)) cells - exactly one cell along the dominant
axis - and rises (dz / a) res metres; at step t = 1, 2, ... the ray is at u0 + t su, v0 + t sv, z0 + t sz (the product with t,
never a running sum), reads the cell it is over and is BLOCKED (0) if that cell's altitude is strictly above zt + eps.  Leaving the
grid makes the start VISIBLE (1); a start without data - a NaN or infinite cell, a point that is not finite or not over the grid -
is NODATA (2).  A NaN cell never blocks.  Everything is float64 with each operation rounded on its own, so every bit of `visible`,
`hit` and `counts` depends on the grid, the starts and the directions alone: not on row bands (rows=), on how the directions are
split over launches (dir_tile=), or on how many GPUs shared the grid (gridwalk.py: bands gathered, counts merged by one SUM all-reduce).

The sun's shadow mask: pass the sun direction.  The view-occlusion mask - "this view saw this cell" - is the same march towards
the sensor: pass -rays[:, 3:6] of the view (one direction per call: the mean of the view's rays, or any ray's; over a scene of a
few hundred metres a satellite's rays are parallel) as `dirs`.

eps (metres, default 0) is the height by which a cell must exceed the ray to block it.  A DSM made of the very points that are
tested - view_visibility of a view over its own DSM - holds, per cell, the MEAN altitude of several points: a point slightly below
its neighbour cell's mean is shadowed by it at eps = 0.  A small eps (a fraction of the resolution) forgives that self-shadowing
at the price of missing obstacles lower than eps; profiles/visibility_throughput.txt counts the pixels it changes.  eps never
turns a visible start into a blocked one.

Refused by name: host tensors, a grid that is not float32, 2-D and contiguous, points that are not float64 (R, 3), directions that
are not finite or have dz <= 0 (a sun below the horizon is the caller's case), more than 4096 directions, a negative or
non-finite eps, rows outside [0, H], an 'ecef' frame (its world axes are not east, north, up: rotating the directions is the
caller's business).

Not covered: soft shadows, interpolated heights, converging rays, directions in an ECEF frame, GeoTIFF I/O.
"""
import torch

from . import _lib as L
from . import functions as Fn
from .gridwalk import GridWalk

BLOCKED, VISIBLE, NODATA = L.BN_VIS_BLOCKED, L.BN_VIS_VISIBLE, L.BN_VIS_NODATA


def _zmax(dsm):
    """The maximum of the non-NaN cells (+inf if one is +inf, -inf on an all-NaN grid): with it the early exit changes no bit."""
    return float(torch.where(torch.isnan(dsm), torch.full_like(dsm, float("-inf")), dsm).max())


def _result(vis, hit, counts, want_hit):
    res = {"visible": vis, "counts": counts.cpu()}
    if want_hit:
        res["hit"] = hit
    return res


@torch.no_grad()
def grid_visibility(dsm, resolution, dirs, eps=0.0, rows=None, group=None, want_hit=False, dir_tile=None):
    """The visibility of every cell of a DSM under K directions.  dsm: (H, W) float32 on the device, contiguous, NaN = no data;
    resolution: the cell size in metres; dirs: (K, 3) or (3,), any float dtype, (east, north, up) towards the sun or the sensor.
    rows = (row0, row1): this process marches only the starts of those rows (the whole grid is still what they march over).  With
    a `group` of more than one rank each rank marches its band (shard_bounds, or `rows`: the bands must partition [0, H) in rank
    order), the bands are gathered and the counts merged: every rank returns the single-process result, bit for bit.  Without a
    group and with `rows`, the rows outside the band are NODATA, `hit` is -1 there and they are not counted.
    dir_tile: directions per call of the entry (None: all K in one).
    -> {"visible" (K, H, W) uint8 in {0 blocked, 1 visible, 2 nodata}, "counts" (K, 3) int64 on the host = (blocked, visible,
    nodata)} (+ "hit" (K, H, W) int32: the flat index of the first blocking cell, or -1)."""
    name = "grid_visibility"
    Fn._need(name, dsm, **Fn.VIS_DSM)
    dirs = Fn._vis_dirs(name, dirs)
    H, W = dsm.shape
    K = dirs.shape[0]
    walk = GridWalk(name, H, rows, group)
    step = K if dir_tile is None else int(dir_tile)
    if step < 1:
        raise ValueError(f"{name}: dir_tile {dir_tile} must be at least 1")
    Fn._vis_scalars(name, resolution, eps, 0.0)
    Fn._on_device(name, dsm)
    zmax = _zmax(dsm)
    vis = walk.buffer((K, H, W), torch.uint8, NODATA, dsm.device)         # outside a lone band: NODATA and -1
    hit = walk.buffer((K, H, W), torch.int32, -1, dsm.device) if want_hit else None
    counts = torch.zeros((K, 3), dtype=torch.int64, device=dsm.device)
    for k0 in range(0, K, step):
        k1 = min(K, k0 + step)
        Fn.grid_visibility(dsm, resolution, dirs[k0:k1], eps, zmax, rows=walk.rows, vis=vis[k0:k1],
                           hit=None if hit is None else hit[k0:k1], counts=counts[k0:k1])
    vis = walk.join(vis, 1)
    if want_hit:
        hit = walk.join(hit, 1)
    return _result(vis, hit, walk.merge(counts), want_hit)


def _on_grid(name, dsm, grid):
    Fn._need(name, dsm, **Fn.VIS_DSM)
    if tuple(dsm.shape) != (grid.height, grid.width):
        raise ValueError(f"{name}: dsm {tuple(dsm.shape)} is not on the grid of {grid.height} x {grid.width} cells")


@torch.no_grad()
def point_visibility(points, dsm, grid, dirs, eps=0.0, want_hit=False):
    """The visibility of world points over a DSM.  points: float64 (R, 3) = (east, north, altitude) on the device, what
    point_cloud returns; dsm: (grid.height, grid.width) float32 on `grid`; dirs (K, 3) or (3,).  A point that is not finite, or
    not over the grid, is NODATA.
    -> {"visible" (K, R) uint8, "counts" (K, 3) int64 on the host} (+ "hit" (K, R) int32)."""
    name = "point_visibility"
    Fn._need(name, points, **Fn.VIS_POINTS)
    _on_grid(name, dsm, grid)
    Fn._vis_dirs(name, dirs)
    Fn._on_device(name, points, dsm)
    vis, hit, counts = Fn.points_visibility(points, dsm, grid.xoff, grid.yoff, grid.resolution, dirs, eps, _zmax(dsm), want_hit=want_hit)
    return _result(vis, hit, counts, want_hit)


@torch.no_grad()
def view_visibility(rays, depth, frame, dsm, grid, dirs, eps=0.0):
    """The shadow map of a view under the geometry of a DSM: point_cloud(rays, depth, frame), then point_visibility.  rays (R, >= 6),
    depth (R,) as render_image returns it, frame the scene's (a 'utm' one).  -> point_visibility's result, "visible" (K, R)."""
    from .dsm import point_cloud
    if frame.cs == "ecef":
        raise ValueError("view_visibility: an 'ecef' frame is not served: its world axes are not (east, north, up), and rotating the "
                         "directions into the scene's UTM frame is the caller's business")
    _on_grid("view_visibility", dsm, grid)
    return point_visibility(point_cloud(rays, depth.to(rays.device), frame), dsm, grid, dirs, eps)


__all__ = ["grid_visibility", "point_visibility", "view_visibility", "BLOCKED", "VISIBLE", "NODATA"]
