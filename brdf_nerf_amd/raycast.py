"""The depth of a surface model along a view's rays, on the device: at what depth does each ray meet a DSM?

dsm_image, ortho_image, orthophoto and orthomosaic take a view to the ground, and visibility.py marches over a raster between
ground points; this module takes the ground to a view.

  cast_rays        each ray's segment [near, far] walked over the cells of a DSM (bn_cast_rays): depth, state, the cell that was
                   hit and the NaN cells that were passed
  grid_to_view     any raster of the grid seen from the view: one gather through the hit cells (as apply_fill does for the fill's
                   source map) - a class mask, grid_visibility's shadow mask, the orthomosaic's mean or std
  surface_priors   the depth columns FusedTrainer reads (depths, valid_depth, depth_std) from a surface model instead of tie points:
                   a lidar DSM, a coarse public one, dsm_image(..., fill=True) of an earlier run, tie_point_dsm's raster;
                   camera.ray_table(priors=[{"dsm": ..., "grid": ...}, ...]) builds a table's columns from it

The rule (include/brdfnerf_hip.h, "Depth of a surface model along a ray", states it as the ABI's contract).  A cell is a flat-topped
column.  The ray's ends p(near), p(far) - point_cloud's own expression, so a cast depth fed back to point_cloud lands on the
surface - are taken to cell coordinates, and the segment is walked cell by cell in its parameter lam in [0, 1], the crossings always
formed from the integer line index.  A cell whose height is at or above the ray where the ray ENTERS it is hit on its WALL (1) -
or, in the start cell, the ray starts BELOW (4) the surface; otherwise a cell at or above the ray where it LEAVES is hit on its TOP
(0), at the depth solved for its height.  Both comparisons are <=.  On a tie of the two crossings both indices move: a ray through
a corner does not test the two cells that touch it only there.  A ray that reaches `far`, or leaves the grid for good, is a MISS
(2); one with a non-finite end, or longer than 65536 cells, is NODATA (3).  A NaN cell is never hit and is counted per ray
(`nan_cells`): the surface under such a ray is unknown up to its hit.  Everything is float64 with each operation rounded on its
own, so every bit of `depth`, `state`, `cell`, `nan_cells` and `counts` depends on the ray, the frame and the raster alone: not on
the chunks (chunk=) or on how many GPUs shared the view (viewwalk.py: rows gathered, counts merged by one SUM all-reduce).

Refused by name: host tensors, rays that are not float32 (R, >= 8), a dsm that is not float32, 2-D, contiguous and on `grid`, an
'ecef' frame (its world axes are not east, north, up).

Not covered: interpolated heights (a cell is a column, not a facet), converging-ray footprints (a pixel is one ray), ECEF frames,
normals from the raster, GeoTIFF I/O.
"""
import torch

from . import _lib as L
from . import functions as Fn
from .distributed import allreduce_
from .viewwalk import ViewWalk
from .visibility import _on_grid, _zmax

TOP, WALL, MISS, NODATA, BELOW = L.BN_CAST_TOP, L.BN_CAST_WALL, L.BN_CAST_MISS, L.BN_CAST_NODATA, L.BN_CAST_BELOW


def _check(name, rays, frame, dsm, grid):
    if frame.cs == "ecef":
        raise ValueError(f"{name}: an 'ecef' frame is not served: its world axes are not (east, north, up)")
    rays = Fn._need(name, rays, "rays", torch.float32, ("R", ">=8"), "rows")
    _on_grid(name, dsm, grid)
    return rays


@torch.no_grad()
def cast_rays(rays, frame, dsm, grid, chunk=None, group=None, want_cell=True):
    """The depth at which each ray of a view meets a DSM.  rays: (R, >= 8) float32 on the device (o, d, near, far, ...); frame: the
    scene's, a 'utm' one; dsm: (grid.height, grid.width) float32 on `grid`, NaN = no data.  chunk: rays per launch (None: all of
    this rank's).  With a `group` of more than one rank each rank casts its ViewWalk share, the rows are gathered and the counts
    merged: every rank returns the single-process result, bit for bit.
    -> {"depth" (R,) float32 in the rays' units, NaN without a hit, "state" (R,) uint8 in {0 top, 1 wall, 2 miss, 3 nodata, 4
    below}, "nan_cells" (R,) int32, "counts": five Python integers, the rays per state in the order of the codes} (+ "cell" (R,)
    int32: the flat index of the hit cell, or -1)."""
    name = "cast_rays"
    rays = _check(name, rays, frame, dsm, grid)
    R = rays.shape[0]
    if chunk is not None and int(chunk) < 1:
        raise ValueError(f"{name}: chunk {chunk} must be at least 1")
    Fn._on_device(name, rays, dsm)
    walk = ViewWalk(R, max(1, R) if chunk is None else int(chunk), group)
    n, dev = walk.hi - walk.lo, dsm.device
    zmax = _zmax(dsm)
    depth = torch.empty((n,), dtype=torch.float32, device=dev)
    state = torch.empty((n,), dtype=torch.uint8, device=dev)
    cell = torch.empty((n,), dtype=torch.int32, device=dev) if want_cell else None
    nan_cells = torch.empty((n,), dtype=torch.int32, device=dev)
    counts = torch.zeros((5,), dtype=torch.int64, device=dev)
    for i, j in walk.chunks():
        a, b = i - walk.lo, j - walk.lo
        Fn.cast_rays(rays[i:j], frame.center, frame.range, dsm, grid.xoff, grid.yoff, grid.resolution, zmax, depth=depth[a:b],
                     state=state[a:b], cell=None if cell is None else cell[a:b], nan_cells=nan_cells[a:b], counts=counts,
                     want_cell=want_cell)
    res = {"depth": walk.join([depth], ()), "state": walk.join([state], ()), "nan_cells": walk.join([nan_cells], ()),
           "counts": [int(v) for v in allreduce_(counts, group=group).tolist()]}
    if want_cell:
        res["cell"] = walk.join([cell], ())
    return res


def grid_to_view(layer, cell, fill=float("nan")):
    """A raster of the grid seen from the view: out[r] = layer.flat[cell[r]] (one torch.take: the bits are copied), `fill` where
    cell[r] < 0.  layer: (H, W) of any dtype on the grid that was cast; cell: cast_rays' "cell".  An integer or bool layer needs a
    `fill` of its own (NaN is not one of its values)."""
    layer, cell = torch.as_tensor(layer), torch.as_tensor(cell)
    if layer.dim() != 2:
        raise ValueError(f"grid_to_view: layer {tuple(layer.shape)} is not an (H, W) raster")
    if cell.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"grid_to_view: cell is {cell.dtype}, not the int32 map of cast_rays")
    if not (layer.is_floating_point() or fill == fill):
        raise ValueError(f"grid_to_view: a {layer.dtype} layer needs a fill of its own (NaN is not one of its values)")
    cell = cell.to(layer.device)
    if cell.numel() and int(cell.max()) >= layer.numel():
        raise ValueError(f"grid_to_view: cell index {int(cell.max())} outside the layer's {layer.numel()} cells")
    hit = cell >= 0
    out = torch.take(layer.contiguous(), torch.where(hit, cell, torch.zeros_like(cell)).long())
    return torch.where(hit, out, torch.full((), fill, dtype=layer.dtype, device=layer.device))


@torch.no_grad()
def surface_priors(rays, frame, dsm, grid, weight=1.0, stdscale=1.0, margin=1e-4, std_span=0.0):
    """The depth priors of a view from a surface model, in depth_priors' columns.  A ray is valid where it met the surface from
    outside (TOP or WALL) without passing a NaN cell.  weight: the weight of every valid ray (the tie points' is their normalised
    correlation).  depth_std = (stdscale (1 - weight) + margin) std_span in float32, left to right, as the tie-point priors form
    it; std_span is upstream's depth_max - depth_min, which is 0.  Where valid_depth == 0 the depth is the float32 of the float64
    mean of the kept depths (padding, no loss reads it), weight and std are 0.
    -> {"depths" (R, 2) = (depth, weight), "valid_depth" (R,), "depth_std" (R,), float32, "counts": cast_rays' five integers}."""
    cast = cast_rays(rays, frame, dsm, grid, want_cell=False)
    depth, state = cast["depth"], cast["state"]
    valid = ((state == TOP) | (state == WALL)) & (cast["nan_cells"] == 0)
    f32 = lambda v: torch.tensor(float(v), dtype=torch.float32, device=depth.device)
    zero, w = f32(0.0), f32(weight)
    kept = torch.where(valid, depth, zero)
    mean = (kept.double().sum() / valid.sum(dtype=torch.float64).clamp(min=1.0)).float()
    std = (f32(stdscale) * (f32(1.0) - w) + f32(margin)) * f32(std_span)
    depths = torch.stack([torch.where(valid, depth, mean), torch.where(valid, w, zero)], -1).contiguous()
    return {"depths": depths, "valid_depth": valid.float(), "depth_std": torch.where(valid, std, zero), "counts": cast["counts"]}


__all__ = ["cast_rays", "grid_to_view", "surface_priors", "TOP", "WALL", "MISS", "NODATA", "BELOW"]
