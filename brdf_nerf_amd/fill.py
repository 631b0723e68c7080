"""The hole filling of a DSM on the device: every NaN cell takes its nearest known cell, exactly and bitwise reproducibly.

The surface model the reference publishes for a view is the *_Grid.tif of save_dsm_grid (eval.py:135-149, called at :176): the
splatted DSM with every NaN cell replaced by quickly_interpolate_nans_from_singlechannel_img (:107-133), that is by scipy's
griddata(method='nearest') - a k-d tree over every known cell, built on the host once per view.  dsm.dsm_image returns a grid
with NaN wherever no ray fell; here that grid is filled where it lies:

  fill_holes   the column pass (bn_grid_nearest_col) and the row pass (bn_grid_fill) -> filled, holes, max_dist (+ source)
  apply_fill   another raster of the same grid gathered through the same source map

The rule (include/brdfnerf_hip.h states it as the ABI's contract).  A cell is a hole if and only if it is NaN: +-inf is a known
value, as for np.isnan upstream.  The source of a hole (j, i) is the known cell (j', i') that minimises the integer triple
(d2, j', i'), d2 = (j - j')^2 + (i - i')^2: the nearest by exact squared Euclidean distance, the lowest row-major index among
equidistant ones.  The output is the source cell's 32 bits, copied: no arithmetic touches a value.  Where the nearest known cell
is unique this IS upstream's answer; on a tie upstream returns the value of some cell at the minimal d2, picked by the k-d
tree's traversal order, and the rule picks the first in row-major order.

Everything is integer, so the result does not depend on how the rows are split (rows=) or on how many GPUs shared the grid:
each rank fills a band of rows, the bands are gathered, and (holes, max d2) merge by one SUM and one MAX all-reduce (gridwalk.py).

Refused by name: host tensors, a dtype other than float32, a grid that is not 2-D and contiguous, more than 8192 cells a side,
rows outside [0, H], a grid without a known cell (upstream's griddata raises there too).

Not covered: GeoTIFF I/O; method='linear' / 'cubic' (upstream always fills with 'nearest').
"""
import math

import torch

from . import functions as Fn
from .gridwalk import GridWalk


@torch.no_grad()
def fill_holes(dsm, rows=None, group=None, want_source=False):
    """quickly_interpolate_nans_from_singlechannel_img(dsm) on the device.  dsm: (H, W) float32, contiguous, NaN = hole.
    rows = (row0, row1): this process fills only those rows.  With a `group` of more than one rank the column pass runs on the whole
    grid on every rank, each rank fills its band (shard_bounds, or `rows`: the bands must partition [0, H) in rank order), the
    bands are gathered and the counts merged: every rank returns the single-process result, bit for bit.  Without a group and
    with `rows`, the rows outside the band are returned as they came (holes included) and `source` is -1 there.
    -> {"filled" (H, W) float32, "holes" int, "max_dist" float = sqrt(largest d2)} (+ "source" (H, W) int32 flat indices)."""
    import torch.distributed as dist
    Fn._need("fill_holes", dsm, "dsm", torch.float32, **Fn.FILL_GRID)
    H, W = dsm.shape
    walk = GridWalk("fill_holes", H, rows, group)
    near_row = Fn.grid_nearest_col(dsm)                    # refuses a host tensor before any launch
    if int(near_row.max()) < 0:
        raise ValueError(f"fill_holes: the {H} x {W} grid has no known cell (every cell is NaN)")
    dst, source, _, counts = Fn.grid_fill(dsm, near_row, rows=walk.rows, want_source=want_source)
    if walk.world > 1:
        dst = walk.join(dst)
        if want_source:
            source = walk.join(source)
        holes, far = counts[0:1].clone(), counts[1:2].clone()
        counts = torch.cat([walk.merge(holes), walk.merge(far, dist.ReduceOp.MAX)])
    elif walk.alone:                                       # the rows outside a lone band: as they came, which no constant states
        band = torch.zeros((H, 1), dtype=torch.bool, device=dsm.device)
        band[walk.rows[0]:walk.rows[1]] = True
        dst = torch.where(band, dst, dsm)
        if want_source:
            source = torch.where(band, source, torch.full_like(source, -1))
    n, far = (int(x) for x in counts.cpu())
    res = {"filled": dst, "holes": n, "max_dist": math.sqrt(far)}
    if want_source:
        res["source"] = source
    return res


@torch.no_grad()
def apply_fill(layer, source):
    """Another co-registered (H, W) raster filled consistently with a DSM: out[j][i] = layer.flat[source[j][i]], `source` the map
    fill_holes(want_source=True) returned (one torch.take).  Any dtype; known cells come back unchanged."""
    layer, source = torch.as_tensor(layer), torch.as_tensor(source)
    if layer.dim() != 2 or layer.shape != source.shape:
        raise ValueError(f"apply_fill: layer {tuple(layer.shape)} and source {tuple(source.shape)} are not on one (H, W) grid")
    if source.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"apply_fill: source is {source.dtype}, not the int32 map of fill_holes")
    return torch.take(layer.contiguous(), source.to(layer.device).long())


__all__ = ["fill_holes", "apply_fill"]
