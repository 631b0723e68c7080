"""The orthophoto of an observed image on the grid of a DSM, on the device: which pixel of a satellite image saw each cell?

ortho_image puts the MODEL's rgb, albedo, normals and BRDF parameters on the grid of the DSM by splatting a view's rays into cells.
This module is the opposite direction: an observed image - or any per-pixel raster in image geometry - is put on that same grid,
so that the model's orthorectified rgb has something observed beside it, a lidar DSM an image over it, and two views can be
compared cell by cell.

  world_pixels     (east, north, altitude) points -> pixels: bn_utm_geodetic, then bn_rpc_project (no kernel of its own)
  grid_pixels      every cell of a DSM -> its pixel (bn_grid_pixels): the two steps in one launch, the same bits
  sample_image     an image gathered at pixel coordinates, bilinear or nearest (bn_image_gather)
  orthophoto       grid_pixels, grid_visibility towards the sensor, sample_image: the image on the grid, occluded cells masked
  ortho_psnr       image_psnr of the model's orthorectified rgb against the orthophoto, on the cells where both are finite

The rule (include/brdfnerf_hip.h, "Orthophoto of an observed image", states it as the ABI's contract).  Cell (j, i) of the grid has
its centre at e = xoff + (i + 0.5) res, n = yoff - (j + 0.5) res - row 0 is the northern edge, Grid's and grid_visibility's
convention - and the altitude of the DSM there.  (e, n) goes through the inverse UTM series (Karney 2011, eq. 36, then Newton for
the latitude, four iterations for every lane) to degrees, and (lon, lat, altitude) through the RPC polynomials to (col, row).  A
pixel index is its coordinate: (col, row) = (k, l) is the centre of pixel (l, k), as view_rays localises arange(W).  A cell is, in
this order, NODATA (0: its pixel is NaN - a NaN or infinite cell of the DSM, a point the geodesy refuses), OUTSIDE (1: not 0 <= col
<= W - 1 and 0 <= row <= H - 1), OCCLUDED (2: grid_visibility towards the sensor says another cell is in the way) or KEPT (3);
only kept cells carry values, the others are NaN.  Bilinear values are formed in float64 from the four taps, every operation
rounded on its own, and cast to float32; a NaN tap propagates.  Nearest copies the pixel's 32 bits.  Everything depends on the
inputs alone: not on row bands (rows=) or on how many GPUs shared the grid (gridwalk.py: the bands are gathered, the counts merge
by one SUM all-reduce).

ONE direction serves the whole scene in the occlusion test (view_direction at the image's centre pixel): over a scene of a few
hundred metres a satellite's rays are parallel to well within a cell.  A NaN cell never blocks, so a DSM with holes lets the
sensor see through them: pass a filled DSM (fill_holes) when the holes are not real.

Refused by name (ValueError, before any launch): host tensors, a DSM that is not float32, 2-D, contiguous and on `grid`, an image
that is not float32 and contiguous or does not hold H_img W_img pixels of 1 to 32 channels, points that are not float64 (n, 3), a
zone outside 1-60, a view_dir that is not finite or does not point upwards, an unknown mode or layout, rows outside [0, H].

Not covered: radiometric normalisation, per-cell view directions, GeoTIFF I/O, pyproj parity of the inverse UTM (it is held to the
project's own forward series).  Several views fused into one mosaic: mosaic.py.
"""
import math

import torch

from . import _lib as L
from . import camera
from . import functions as Fn
from .gridwalk import GridWalk
from .visibility import NODATA as VIS_NODATA, _on_grid, _zmax

NODATA, OUTSIDE, OCCLUDED, KEPT = L.BN_GATHER_NODATA, L.BN_GATHER_OUTSIDE, L.BN_GATHER_OCCLUDED, L.BN_GATHER_KEPT
STATES = ("nodata", "outside", "occluded", "kept")
_LAYOUTS = ("image", "planes")


def _image(name, image, H_img, W_img, layout):
    """The image as the gather reads it -> (buffer, C, element strides (row, col, channel)).  'image': an (H W, C) or (H, W, C)
    buffer, channel c of pixel (r, k) at flat[(r W + k) C + c]; 'planes': (C, H, W).  A 2-D (H, W) raster is either."""
    if layout not in _LAYOUTS:
        raise ValueError(f"{name}: layout {layout!r} ('image' or 'planes')")
    H_img, W_img = int(H_img), int(W_img)
    Fn._need(name, image, "image", Fn.F32)
    if H_img < 1 or W_img < 1 or image.numel() == 0 or image.numel() % (H_img * W_img) != 0:
        raise ValueError(f"{name}: image {tuple(image.shape)} does not hold {H_img} x {W_img} pixels")
    C = image.numel() // (H_img * W_img)
    if not 1 <= C <= L.BN_GATHER_MAX_CHANNELS:
        raise ValueError(f"{name}: image {tuple(image.shape)} has {C} channels at {H_img} x {W_img} pixels (1 to {L.BN_GATHER_MAX_CHANNELS})")
    return image, C, ((W_img * C, C, 1) if layout == "image" else (W_img, 1, H_img * W_img))


def _counts(states, skipped=None):
    res = {} if skipped is None else {"skipped": int(skipped)}
    res.update({k: int(v) for k, v in zip(STATES, states)})
    return res


@torch.no_grad()
def world_pixels(rpc, points, zone, south=False):
    """The pixels of world points: points float64 (n, 3) = (east, north, altitude) on the device in the UTM `zone`, what
    point_cloud returns -> colrow float64 (n, 2) = (col, row), NaN in both where the point, its geodetic point or its pixel is not
    finite, and the number of those rows.  bn_utm_geodetic followed by bn_rpc_project: the same device functions as grid_pixels."""
    name = "world_pixels"
    points = Fn._need(name, points, **Fn.VIS_POINTS)
    Fn._zone(name, zone, south)
    Fn._on_device(name, points)
    skipped = torch.zeros((1,), dtype=torch.int64, device=points.device)
    lonlat = Fn.utm_geodetic(points[:, :2].contiguous(), zone, south, skipped)
    col, row = camera.project(rpc, lonlat[:, 0].contiguous(), lonlat[:, 1].contiguous(), points[:, 2].contiguous())
    colrow = torch.stack([col, row], -1)
    bad = ~(torch.isfinite(colrow).all(-1) & torch.isfinite(points[:, 2]))
    colrow[bad] = float("nan")
    return colrow, int(bad.sum())


@torch.no_grad()
def grid_pixels(dsm, grid, rpc, zone, south=False, rows=None, want_skipped=False):
    """The pixel of the image of `rpc` that every cell of a DSM projects to.  dsm: (grid.height, grid.width) float32 on the device,
    NaN = no data; zone, south: the UTM zone the grid's coordinates are in.  rows = (row0, row1): only those rows are computed, the
    others are NaN.  -> colrow (H, W, 2) float64 = (col, row), NaN where the cell has no finite altitude or pixel (want_skipped:
    also their number within the rows)."""
    name = "grid_pixels"
    _on_grid(name, dsm, grid)
    H = dsm.shape[0]
    rows = (0, H) if rows is None else (int(rows[0]), int(rows[1]))
    Fn._zone(name, zone, south)
    Fn._on_device(name, dsm)
    colrow = torch.full((H, dsm.shape[1], 2), float("nan"), dtype=torch.float64, device=dsm.device) if rows != (0, H) else None
    colrow, counts = Fn.grid_pixels(rpc, dsm, grid.xoff, grid.yoff, grid.resolution, zone, south, rows=rows, colrow=colrow)
    return (colrow, int(counts.item())) if want_skipped else colrow


@torch.no_grad()
def sample_image(image, H_img, W_img, colrow, visible=None, mode="bilinear", layout="image"):
    """An image gathered at pixel coordinates.  image: float32 on the device, H_img x W_img pixels of C channels - layout 'image':
    (H W, C) or (H, W, C), the buffers of this project; 'planes': (C, H, W); colrow (..., 2) float64 = (col, row), what grid_pixels
    and world_pixels return; visible: uint8 of colrow's leading shape (grid_visibility's `visible` of one direction) or None -
    only cells equal to VISIBLE are kept; mode 'bilinear' or 'nearest'.
    -> {"ortho" (C, ...) float32, NaN where the state is not KEPT, "state" (...) uint8 in {NODATA 0, OUTSIDE 1, OCCLUDED 2, KEPT 3},
    "counts" {"nodata", "outside", "occluded", "kept"}}."""
    name = "sample_image"
    image, C, strides = _image(name, image, H_img, W_img, layout)
    Fn._need(name, colrow, "colrow", Fn.F64)
    if colrow.dim() < 1 or colrow.shape[-1] != 2:
        raise ValueError(f"{name}: colrow {tuple(colrow.shape)} is not (..., 2)")
    cells = tuple(colrow.shape[:-1])
    if visible is not None:
        Fn._need(name, visible, "visible", Fn.U8, cells)
    out, state, counts = Fn.image_gather(image, H_img, W_img, C, strides, colrow, visible, mode=mode)
    return {"ortho": out.reshape((C,) + cells), "state": state.reshape(cells), "counts": _counts(counts.tolist())}


def _sensor_dirs(name, noun, given, rpcs, dsm, zone, south, alt_bounds, occlusion, on_device):
    """The directions from the surface towards the sensors of the K `rpcs`, one for the whole scene each -> float64 (K, 3) on the
    host, or None without occlusion and without `given`.  given: the caller's `noun` - "view_dir": any 3 floats, "view_dirs": (K, 3)
    floats - else camera.view_direction of every rpc between alt_bounds = (alt_lo, alt_hi), by default the minimum and maximum of
    the finite cells (at least a metre apart).  Every direction must be finite and point upwards.  The arguments are refused first,
    then - the caller's last host-side check - a host tensor among `on_device`, then what reads the device: a DSM without a finite
    cell, a derived direction."""
    K, one = len(rpcs), noun == "view_dir"

    def checked(d):
        d = torch.as_tensor(d)
        if not d.is_floating_point() or (d.numel() != 3 if one else tuple(d.shape) != (K, 3)):
            shape = "3 floats (east, north, up)" if one else f"({K}, 3) floats (east, north, up), one direction per view"
            raise ValueError(f"{name}: {noun} must be {shape}")
        d = d.detach().to(device="cpu", dtype=torch.float64).reshape(K, 3)
        if not bool(torch.isfinite(d).all()) or not bool((d[:, 2] > 0).all()):
            raise ValueError(f"{name}: {f'view_dir {d[0].tolist()}' if one else 'every view_dir'} must be finite and point upwards, from "
                             "the surface towards the sensor")
        return d
    if given is not None:
        given = checked(given)
    if alt_bounds is not None:
        alt_bounds = (float(alt_bounds[0]), float(alt_bounds[1]))
        if not (math.isfinite(alt_bounds[0]) and math.isfinite(alt_bounds[1]) and alt_bounds[1] > alt_bounds[0]):
            raise ValueError(f"{name}: alt_bounds {alt_bounds} must be finite and ascending")
    Fn._on_device(name, *on_device)
    if given is not None or not occlusion:
        return given
    if alt_bounds is None:
        known = dsm[torch.isfinite(dsm)]
        if known.numel() == 0:
            raise ValueError(f"{name}: the {dsm.shape[0]} x {dsm.shape[1]} DSM has no finite cell to take alt_bounds from")
        lo, hi = float(known.min()), float(known.max())
        alt_bounds = (lo, max(hi, lo + 1.0))
    return checked(torch.stack([torch.as_tensor(camera.view_direction(r, zone, south, *alt_bounds, device=dsm.device)) for r in rpcs]))


@torch.no_grad()
def orthophoto(image, H_img, W_img, rpc, dsm, grid, zone, south=False, occlusion=True, eps=0.0, view_dir=None, alt_bounds=None,
               mode="bilinear", rows=None, group=None, layout="image"):
    """An observed image on the grid of a DSM.  image, H_img, W_img, layout, mode: as sample_image; rpc: the image's camera.Rpc;
    dsm: (grid.height, grid.width) float32 on the device, NaN = no data - a NaN cell never blocks, so pass a FILLED DSM (fill_holes)
    unless its holes are real; zone, south: the UTM zone of the grid.
    occlusion=True: grid_visibility(dsm, grid.resolution, view_dir[None], eps) decides which cells the sensor saw.  ONE direction
    serves the whole scene: view_dir (east, north, up), from the surface towards the sensor, or by default camera.view_direction at
    the image's centre pixel between alt_bounds = (alt_lo, alt_hi) - by default the minimum and maximum of the finite cells (at
    least a metre apart).  eps: grid_visibility's, in metres.
    rows = (row0, row1): this process works only on those rows.  With a `group` of more than one rank each rank does its band
    (shard_bounds, or `rows`: the bands must partition [0, H) in rank order), the bands are gathered and the counts merged by one
    SUM all-reduce: every rank returns the single-process result, bit for bit.  Without a group and with `rows`, the rows outside
    the band are NODATA and NaN and are not counted.
    -> {"ortho" (C, H, W) float32, NaN where the state is not KEPT, "state" (H, W) uint8 in {NODATA 0, OUTSIDE 1, OCCLUDED 2,
    KEPT 3}, "colrow" (H, W, 2) float64, "visible" (H, W) uint8 as grid_visibility's (None without occlusion), "counts"
    {"skipped", "nodata", "outside", "occluded", "kept"}, "view_dir" float64 (3,) on the host (None without occlusion)}."""
    name = "orthophoto"
    image, C, strides = _image(name, image, H_img, W_img, layout)
    _on_grid(name, dsm, grid)
    if mode not in Fn.GATHER_MODES:
        raise ValueError(f"{name}: mode {mode!r} ('bilinear' or 'nearest')")
    zone, south = Fn._zone(name, zone, south)
    H, W = dsm.shape
    walk = GridWalk(name, H, rows, group)
    rows = walk.rows
    res, eps, _ = Fn._vis_scalars(name, grid.resolution, eps, 0.0)
    dirs = _sensor_dirs(name, "view_dir", view_dir, [rpc], dsm, zone, south, alt_bounds, occlusion, (image, dsm))
    dev, nan = dsm.device, float("nan")                     # outside a lone band: NODATA and NaN
    counts = torch.zeros((8,), dtype=torch.int64, device=dev)          # skipped, the four states, grid_visibility's three
    colrow, _ = Fn.grid_pixels(rpc, dsm, grid.xoff, grid.yoff, res, zone, south, rows=rows, colrow=walk.buffer((H, W, 2), Fn.F64, nan, dev),
                               counts=counts[0:1])
    visible = None
    if occlusion:
        visible, _, _ = Fn.grid_visibility(dsm, res, dirs, eps, _zmax(dsm), rows=rows, vis=walk.buffer((1, H, W), Fn.U8, VIS_NODATA, dev),
                                           counts=counts[5:8].reshape(1, 3))
        visible = visible[0]
    ortho, state, _ = Fn.image_gather(image, H_img, W_img, C, strides, colrow, visible, cells=(rows[0] * W, rows[1] * W), mode=mode,
                                      out=walk.buffer((C, H, W), Fn.F32, nan, dev), state=walk.buffer((H, W), Fn.U8, NODATA, dev),
                                      counts=counts[1:5])
    ortho, state, colrow = walk.join(ortho, 1), walk.join(state), walk.join(colrow)
    if occlusion:
        visible = walk.join(visible)
    walk.merge(counts)
    c = counts.tolist()
    return {"ortho": ortho, "state": state, "colrow": colrow, "visible": visible, "counts": _counts(c[1:5], c[0]),
            "view_dir": None if dirs is None else dirs[0]}


@torch.no_grad()
def ortho_psnr(pred_rgb, ortho, mask=None):
    """image_psnr of a model's orthorectified rgb against the orthophoto of the observed image, on the cells where both are finite
    in every channel (and `mask`, one value per cell, is nonzero): pred_rgb, ortho (C, H, W) on one grid - ortho_image(...)["maps"]
    ["rgb"] beside orthophoto(...)["ortho"].  No kernel of its own.  -> (psnr, cells compared); upstream's normaliser, the maximum
    of the whole target, is taken over the compared cells' target values (a NaN would poison it)."""
    from .metrics import image_psnr
    if pred_rgb.shape != ortho.shape or pred_rgb.dim() != 3:
        raise ValueError(f"ortho_psnr: maps {tuple(pred_rgb.shape)} and {tuple(ortho.shape)} are not both (C, H, W) on one grid")
    ortho = ortho.to(pred_rgb.device)
    keep = torch.isfinite(pred_rgb).all(0) & torch.isfinite(ortho).all(0)
    if mask is not None:
        m = torch.as_tensor(mask).to(pred_rgb.device)
        if m.numel() != keep.numel():
            raise ValueError(f"ortho_psnr: mask of {m.numel()} elements for a grid of {tuple(keep.shape)}")
        keep = keep & (m.reshape(keep.shape) != 0)
    n = int(keep.sum())
    if n == 0:
        return torch.tensor(float("nan"), device=pred_rgb.device), 0
    a, b = pred_rgb[:, keep].t().contiguous(), ortho[:, keep].t().contiguous()        # (n, C) rows, as image_psnr takes them
    return image_psnr(a, b)[0], n


__all__ = ["world_pixels", "grid_pixels", "sample_image", "orthophoto", "ortho_psnr", "NODATA", "OUTSIDE", "OCCLUDED", "KEPT", "STATES"]
