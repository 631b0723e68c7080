"""The orthomosaic of several observed images on the grid of a DSM, in one launch, and the multi-view photo-consistency of the DSM.

orthophoto puts ONE observed image on the grid; behind every building it leaves the cells that image did not see as NaN.  A site
has 10 to 30 views and each sees another side, so this module fuses them: per cell the value of the best view that saw it, the
mean over all views that saw it - a mosaic without holes - and the spread of the observed values over those views.  A wrong
altitude sends a cell to different ground in every image, so the spread rises: it is the one quality score of a surface model
that needs no ground truth, and it belongs beside altitude_mae and ortho_psnr (ortho_psnr(pred_rgb, mosaic["mean"]) works as it is).

  orthomosaic      grid_visibility towards every sensor (one launch), then bn_grid_mosaic: one launch takes a cell to its geodetic
                   point once, walks the K views and keeps only the results

Composed from K orthophoto calls the same result costs K inverse UTMs per cell, a (K, H, W, 2) float64 pixel map and a (K, C, H,
W) stack; here nothing per view is stored but the occlusion mask.

The rule (include/brdfnerf_hip.h, "Orthomosaic of several observed images").  Per cell, views in ascending order: the pixel under
the view's RPC (bn_grid_pixels' bits), the state as in orthophoto - NODATA 0, OUTSIDE 1, OCCLUDED 2 - and for a kept cell the
values (bn_image_gather's bits).  A view with a NaN or infinite value is NONFINITE (4) and contributes nothing; the others are
USED (3) and enter Welford's update of the mean and the sum of squares in float64.  `best` is the used view of the smallest rank,
ties to the lower index; by default the ranks order the views by elevation, most nadir first.  std is the population's: 0 where
one view saw the cell.  The consistency of the grid is the mean of std over the cells seen by at least two views and the channels,
summed in integers of 2^-20.  Everything depends on the inputs alone: not on row bands (rows=) or on how many GPUs shared the grid
(gridwalk.py: the bands are gathered, every counter merges by one SUM all-reduce).

Refused by name (ValueError, before any launch): an empty list of views or more than 32, views of different channel counts or more
than 4 channels, a rank that is not K integers, view_dirs that are not (K, 3), finite and pointing upwards, a colrow that is not
(K, H, W, 2) float64, and everything orthophoto refuses of an image, the DSM, the zone, the mode, the layout and the rows.

Not covered: a median, radiometric normalisation between views, more than 4 channels per call, per-cell view directions, GeoTIFF I/O.
"""
import numbers

import torch

from . import _lib as L
from . import functions as Fn
from .gridwalk import GridWalk
from .orthophoto import _image, _sensor_dirs
from .visibility import NODATA as VIS_NODATA, _on_grid, _zmax

NODATA, OUTSIDE, OCCLUDED, USED, NONFINITE = (L.BN_GATHER_NODATA, L.BN_GATHER_OUTSIDE, L.BN_GATHER_OCCLUDED, L.BN_MOSAIC_USED,
                                              L.BN_MOSAIC_NONFINITE)
STATES = ("nodata", "outside", "occluded", "used", "nonfinite")
Q20 = 1 << 20


def nadir_ranks(view_dirs):
    """The default ranks: the views sorted by descending dz / |d| of their direction, most nadir first, ties by index -> K ints,
    rank[k] = the place of view k in that order."""
    d = torch.as_tensor(view_dirs, dtype=torch.float64)
    up = (d[:, 2] / d.norm(dim=1)).tolist()
    order = sorted(range(len(up)), key=lambda k: (-up[k], k))
    rank = [0] * len(up)
    for place, k in enumerate(order):
        rank[k] = place
    return rank


def views_on_dsm(name, views, dsm, grid, zone, south, eps, mode, rows, group, layout):
    """What orthomosaic and sweep.altitude_sweep check of their views, the DSM, the zone, the mode, the layout and the rows, in one
    place -> the views as (image, H_img, W_img, strides, rpc, C) each, K, C, zone, south, the GridWalk of the rows, res, eps."""
    views = list(views)
    K = len(views)
    if not 1 <= K <= L.BN_MOSAIC_MAX_VIEWS:
        raise ValueError(f"{name}: {K} views (1 to {L.BN_MOSAIC_MAX_VIEWS})")
    taken = []
    for k, view in enumerate(views):
        if len(view) != 4:
            raise ValueError(f"{name}: view {k} is not (image, H_img, W_img, rpc)")
        image, H_img, W_img, rpc = view
        image, C, strides = _image(f"{name}: view {k}", image, H_img, W_img, layout)
        taken.append((image, int(H_img), int(W_img), strides, rpc, C))
    C = taken[0][5]
    if any(t[5] != C for t in taken) or C > L.BN_MOSAIC_MAX_CHANNELS:
        raise ValueError(f"{name}: the views have {[t[5] for t in taken]} channels (all the same, 1 to {L.BN_MOSAIC_MAX_CHANNELS})")
    _on_grid(name, dsm, grid)
    if mode not in Fn.GATHER_MODES:
        raise ValueError(f"{name}: mode {mode!r} ('bilinear' or 'nearest')")
    zone, south = Fn._zone(name, zone, south)
    walk = GridWalk(name, dsm.shape[0], rows, group)
    res, eps, _ = Fn._vis_scalars(name, grid.resolution, eps, 0.0)
    return taken, K, C, zone, south, walk, res, eps


def sensor_masks(walk, dsm, res, view_dirs, eps, counts):
    """The ONE grid_visibility launch towards the K sensors over the walk's rows -> visible (K, H, W) uint8, NODATA in the unseen
    rows of a lone band; counts (K, 3) int64 are accumulated into."""
    K, (H, W) = len(view_dirs), dsm.shape
    return Fn.grid_visibility(dsm, res, view_dirs, eps, _zmax(dsm), rows=walk.rows, counts=counts,
                              vis=walk.buffer((K, H, W), Fn.U8, VIS_NODATA, dsm.device))[0]


@torch.no_grad()
def orthomosaic(views, dsm, grid, zone, south=False, occlusion=True, eps=0.0, view_dirs=None, alt_bounds=None, rank=None,
                mode="bilinear", rows=None, group=None, layout="image", colrow=None):
    """Several observed images fused on the grid of a DSM.  views: a list of K (image, H_img, W_img, rpc), each as orthophoto takes
    one, all of the same 1 to 4 channels, K from 1 to 32; dsm, grid, zone, south, eps, mode, layout, rows, group: as orthophoto.
    occlusion=True: ONE grid_visibility(dsm, grid.resolution, view_dirs (K, 3), eps) decides which cells each sensor saw; view_dirs
    are given or camera.view_direction of every view between alt_bounds (orthophoto's default).  rank: K integers, the smaller
    wins `best`; by default nadir_ranks(view_dirs), and the views' order without occlusion and without view_dirs.  colrow (K, H, W,
    2) float64: the views' pixels as grid_pixels gives them, used in place of the projection.
    -> {"best_rgb", "mean", "std" (C, H, W) float32, NaN where no view saw the cell, "count" (H, W) uint8, "best" (H, W) int32 (-1
    there), "visible" (K, H, W) uint8 as grid_visibility's (None without occlusion), "view_dirs" float64 (K, 3) on the host or None,
    "rank" [K ints], "counts" {"nodata", "outside", "occluded", "used", "nonfinite": [K ints]}, "consistency": q / (cells C 2^20),
    NaN without a cell seen twice, "cells", "skipped"}."""
    name = "orthomosaic"
    taken, K, C, zone, south, walk, res, eps = views_on_dsm(name, views, dsm, grid, zone, south, eps, mode, rows, group, layout)
    H, W = dsm.shape
    if rank is not None:
        rank = list(rank)
        if len(rank) != K or any(isinstance(r, bool) or not isinstance(r, numbers.Integral) or not -(1 << 31) <= r < 1 << 31 for r in rank):
            raise ValueError(f"{name}: rank {rank} is not {K} integers, one per view")
        rank = [int(r) for r in rank]
    Fn._maybe(name, colrow, "colrow", Fn.F64, (K, H, W, 2))
    view_dirs = _sensor_dirs(name, "view_dirs", view_dirs, [t[4] for t in taken], dsm, zone, south, alt_bounds, occlusion,
                             (dsm, colrow, *[t[0] for t in taken]))
    if rank is None:
        rank = list(range(K)) if view_dirs is None else nadir_ranks(view_dirs)
    dev, nan = dsm.device, float("nan")                     # outside a lone band: no view saw the cell
    totals = torch.zeros((8 * K + 3,), dtype=torch.int64, device=dev)          # counts (K, 5), sums (3), grid_visibility's (K, 3)
    counts, sums = totals[:5 * K].view(K, 5), totals[5 * K:5 * K + 3]
    visible = None
    if occlusion:
        visible = sensor_masks(walk, dsm, res, view_dirs, eps, totals[5 * K + 3:].view(K, 3))
    table = [(t[0], t[1], t[2], t[3], None if visible is None else visible[k], rank[k], t[4]) for k, t in enumerate(taken)]
    out = Fn.grid_mosaic(table, C, dsm, grid.xoff, grid.yoff, res, zone, south, rows=walk.rows, mode=mode, colrow=colrow,
                         count=walk.buffer((H, W), Fn.U8, 0, dev), best=walk.buffer((H, W), Fn.I32, -1, dev),
                         best_val=walk.buffer((C, H, W), Fn.F32, nan, dev), mean=walk.buffer((C, H, W), Fn.F32, nan, dev),
                         std=walk.buffer((C, H, W), Fn.F32, nan, dev), counts=counts, sums=sums)
    maps = [walk.join(out[k], 1) for k in ("best_val", "mean", "std")]
    count, best = walk.join(out["count"]), walk.join(out["best"])
    if occlusion:
        visible = walk.join(visible, 1)
    walk.merge(totals)
    per_view = counts.tolist()
    cells, q, skipped = sums.tolist()
    return {"best_rgb": maps[0], "mean": maps[1], "std": maps[2], "count": count, "best": best, "visible": visible,
            "view_dirs": view_dirs, "rank": rank, "counts": {s: [row[i] for row in per_view] for i, s in enumerate(STATES)},
            "consistency": q / (cells * C * Q20) if cells else float("nan"), "cells": cells, "skipped": skipped}


__all__ = ["orthomosaic", "nadir_ranks", "NODATA", "OUTSIDE", "OCCLUDED", "USED", "NONFINITE", "STATES"]
