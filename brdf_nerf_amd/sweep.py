"""The altitude sweep of a DSM under several observed images, in one launch: the photo-consistent altitude of every cell.

orthomosaic's consistency says THAT a surface model is wrong: a wrong altitude sends a cell to different ground in every image, so
the spread of the observed values rises.  It does not say by how much, nor in which direction.  This module evaluates the same
spread with the cell's altitude moved through a list of offsets and keeps the offset at which it is smallest - a plane sweep
around the surface model.  None of what it gives needs ground truth:

  a per-cell altitude residual of any DSM              result["offset"]
  a refined DSM, dsm + the best offset                 result["altitude"]; surface_priors and ray_table(priors=[{"dsm": ...}]) take it
                                                       as --ds_lambda supervision as they are
  a surface model from the images alone                a constant DSM, offsets that span the scene, occlusion=False

  altitude_sweep   grid_visibility towards every sensor (one launch, on the BASE model), then bn_grid_sweep: one launch takes a cell
                   to its geodetic point once, walks the Z levels and under each the K views, and keeps three small maps

Composed from Z orthomosaic calls on dsm + offset the same answer costs Z inverse UTMs per cell, Z marches, Z sets of (C, H, W)
maps and a torch argmin over the stacked std, which is float32 per channel - the cost below is formed in float64 before any cast.

The rule (include/brdfnerf_hip.h, "Altitude sweep of a surface model under several observed images").  Per cell, levels in ascending
order: a_l = dsm + offsets[l] in float64; the views in ascending order exactly as the orthomosaic walks them - pixel, state, values,
finiteness, Welford's update; the mask of a view is the base model's at every level.  A level is valid where at least min_views
views were used; its cost is the sum over the channels of the population variance M2 / n.  The best level is the valid one of the
smallest cost, the FIRST of them on a tie (a strict <).  Everything depends on the inputs alone: not on row bands (rows=) or on
how many GPUs shared the grid (gridwalk.py: the bands are gathered, every counter merges by one SUM all-reduce).

Refused by name (ValueError, before any launch): everything orthomosaic refuses of the views, the DSM, the zone, the mode, the
layout, the rows, view_dirs and alt_bounds; empty offsets or more than 256; an offset that is not finite; a min_views that is not
an integer from 1 to 32; a colrow that is not (Z, K, H, W, 2) float64.

Aggregation (aggregate=dict(p1=, p2=, paths=8, quantum=None)): the per-cell minimum above is a weak cue where the images are noisy.
With `aggregate` the cost volume goes through aggregate.aggregate_costs - semi-global matching over the levels, 4 or 8 paths - and
"level", "offset", "altitude" and "wins" are the aggregated pick's; the per-cell pick stays as "level_wta".  Level adjacency is index
adjacency, so the offsets must then be strictly increasing, and the paths cross row bands, so rows= is refused.

Not covered: occlusion per level (the masks are the base model's), NCC or census costs (the cost volume is returned for that:
want_cost), radiometric normalisation between views, sub-level (parabolic) refinement - on the box scene a 4 m
step with a parabola left ground cells up to 1.6 m off, so it is left out on purpose -, ECEF frames, GeoTIFF I/O.
"""
import torch

from . import functions as Fn
from .aggregate import aggregate_costs, path_mask, penalties
from .mosaic import Q20, sensor_masks, views_on_dsm
from .orthophoto import _sensor_dirs


@torch.no_grad()
def altitude_sweep(views, dsm, grid, zone, offsets, south=False, occlusion=True, eps=0.0, view_dirs=None, alt_bounds=None, min_views=2,
                   mode="bilinear", rows=None, group=None, layout="image", colrow=None, want_cost=False, aggregate=None):
    """The altitude, among dsm + offsets, at which the views of every cell agree best.  views, dsm, grid, zone, south, occlusion, eps,
    view_dirs, alt_bounds, mode, rows, group, layout: as orthomosaic takes them; the occlusion masks are those of `dsm` at every level.
    offsets: Z finite floats in metres, a sequence or a tensor, 1 to 256, in any order.  min_views: a level counts where at least that
    many views were used (1 to 32).  colrow (Z, K, H, W, 2) float64: the pixels per level and view, used in place of the projection.
    -> {"level" (H, W) int32, -1 where no level is valid, "offset" (H, W) float64 = offsets[level], NaN there, "altitude" (H, W)
    float32 = (float)(dsm + offsets[level]), "cost_min" (H, W) float32, the best level's sum over the channels of the population
    variance, "count" (H, W) uint8, its used views, "cost" (Z, H, W) float32 with want_cost, else None, "visible" (K, H, W) uint8 as
    grid_visibility's (None without occlusion), "view_dirs" float64 (K, 3) on the host or None, "offsets" (Z,) float64 on the host,
    "valid", "wins": Z integers each - the cells valid at a level, the cells it is the best of -, "mean_cost": q / (cells 2^20), NaN
    without a cell, "cells", "skipped"}.
    aggregate: None, or {"p1", "p2", and optionally "paths" (8), "quantum" (None)} as aggregate_costs takes them: the cost volume is
    formed as with want_cost (and returned only with it) and aggregated; the offsets must be strictly increasing and rows= is refused.
    "level", "offset", "altitude" = (float)((double)dsm + offsets[level]) and "wins" are then the aggregated pick's, and the result gains
    "level_wta" (H, W) int32, the per-cell pick that "level" is otherwise, and "sum_min" (H, W) int32, the smallest sum of the paths.
    "cost_min", "count", "valid", "mean_cost", "cells" and "skipped" stay the per-cell sweep's."""
    name = "altitude_sweep"
    taken, K, C, zone, south, walk, res, eps = views_on_dsm(name, views, dsm, grid, zone, south, eps, mode, rows, group, layout)
    H, W = dsm.shape
    off = Fn._sweep_offsets(name, offsets)
    Z = off.numel()
    min_views = Fn._sweep_min_views(name, min_views)
    Fn._maybe(name, colrow, "colrow", Fn.F64, (Z, K, H, W, 2))
    if aggregate is not None:
        if not isinstance(aggregate, dict) or not {"p1", "p2"} <= set(aggregate) <= {"p1", "p2", "paths", "quantum"}:
            raise ValueError(f"{name}: aggregate {aggregate!r} is not a dict of p1, p2 and optionally paths and quantum")
        penalties(name, aggregate["p1"], aggregate["p2"], aggregate.get("quantum"))
        path_mask(name, aggregate.get("paths", 8))
        if rows is not None:
            raise ValueError(f"{name}: rows= cannot be combined with aggregate (the paths cross row bands)")
        if not bool((off[1:] > off[:-1]).all()):
            raise ValueError(f"{name}: with aggregate the offsets must be strictly increasing (level adjacency is index adjacency)")
    view_dirs = _sensor_dirs(name, "view_dirs", view_dirs, [t[4] for t in taken], dsm, zone, south, alt_bounds, occlusion,
                             (dsm, colrow, *[t[0] for t in taken]))
    dev, nan = dsm.device, float("nan")                     # outside a lone band: no level is valid
    totals = torch.zeros((2 * Z + 3 + 3 * K,), dtype=torch.int64, device=dev)  # valid (Z), wins (Z), sums (3), grid_visibility's (K, 3)
    valid, wins, sums = totals[:Z], totals[Z:2 * Z], totals[2 * Z:2 * Z + 3]
    visible = sensor_masks(walk, dsm, res, view_dirs, eps, totals[2 * Z + 3:].view(K, 3)) if occlusion else None
    table = [(t[0], t[1], t[2], t[3], None if visible is None else visible[k], 0, t[4]) for k, t in enumerate(taken)]
    out = Fn.grid_sweep(table, C, dsm, grid.xoff, grid.yoff, res, zone, south, off, min_views=min_views, rows=walk.rows, mode=mode,
                        colrow=colrow, level=walk.buffer((H, W), Fn.I32, -1, dev), cost_min=walk.buffer((H, W), Fn.F32, nan, dev),
                        count=walk.buffer((H, W), Fn.U8, 0, dev), altitude=walk.buffer((H, W), Fn.F32, nan, dev),
                        cost=walk.buffer((Z, H, W), Fn.F32, nan, dev) if want_cost or aggregate else None, valid=valid, wins=wins,
                        sums=sums)
    level, cost_min, count, altitude = (walk.join(out[k]) for k in ("level", "cost_min", "count", "altitude"))
    cost = walk.join(out["cost"], 1) if want_cost or aggregate else None
    if occlusion:
        visible = walk.join(visible, 1)
    walk.merge(totals)
    extra, wins = {}, wins.tolist()
    if aggregate:
        picked = aggregate_costs(cost, aggregate["p1"], aggregate["p2"], aggregate.get("quantum"), aggregate.get("paths", 8), group)
        extra = {"level_wta": level, "sum_min": picked["sum_min"]}
        level, wins = picked["level"], picked["wins"]
    offset = torch.where(level >= 0, off.to(dev)[level.clamp(min=0).long()], torch.full((), nan, dtype=torch.float64, device=dev))
    if aggregate:
        altitude = (dsm.double() + offset).float()              # NaN where no level is valid
    cells, q, skipped = sums.tolist()
    return {"level": level, "offset": offset, "altitude": altitude, "cost_min": cost_min, "count": count, "cost": cost if want_cost else None,
            "visible": visible, "view_dirs": view_dirs, "offsets": off, "valid": valid.tolist(), "wins": wins,
            "mean_cost": q / (cells * Q20) if cells else float("nan"), "cells": cells, "skipped": skipped, **extra}


__all__ = ["altitude_sweep"]
