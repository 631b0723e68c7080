"""Orthorectified maps of a view: the ray-level maps of view_maps splatted into the grid of the DSM, on the device and bitwise
reproducible.

view_maps gives the maps of a view in IMAGE geometry; dsm_image gives one quantity, the altitude, in GROUND geometry.  What a
satellite BRDF model is asked for is the albedo and the BRDF parameters as geo-referenced rasters on the grid of the DSM and of
its lidar ground truth, fused over several views.  **The reference has no counterpart**: it rasterises the altitude alone
(plyflatten, datasets/satellite_rgb_dep.py:636-699).  The rule for the feature channels (include/brdfnerf_hip.h, "Orthorectified
maps of a view") is this project's own; its altitude part is bn_dsm_splat's (bn_dsm_splat_world's) rule bit for bit.

  OrthoAccumulator   bn_ortho_top (pass 1) and bn_ortho_splat (pass 2) into integer grids - chunk by chunk, view by view, rank
                     by rank - and bn_ortho_resolve
  ortho_image        one view_maps walk, the chosen maps as one (R, E) feature tensor, both passes over the rank's share, the merge

An oblique view reaches the cells along a building's edge at several heights: roof, facade and ground.  The mean over all of
them is right for plyflatten's altitude and mixes their colours.  mode='top' keeps, per cell, the points within `band` metres of
the highest point that reaches that cell (through its own footprint or a neighbour's); mode='mean' is the plain mean.  Features
are summed as integers in units of 2^-24 (|x| < 2^16), altitudes in units of 2^-20 m: every output bit depends on the set of rays
alone, provided pass 1 has seen every ray before pass 2 starts.  The mean of unit normals is NOT a unit vector and is not
renormalised: its length says how much the normals of a cell agree.

Refused by name (ValueError): an unknown mode, a negative or non-finite band, channels outside [0, 32], features that are not
(R, channels) float32 on the device, add_top in mean mode, add_top after the first add; in ortho_image an unknown key, a key the
model does not have, and more than 32 channels in total.  Not covered: GeoTIFF I/O, sigma < inf, a weighted mean.
"""
import math

import torch

from . import _lib as L
from . import functions as Fn
from .dsm import _FOOTPRINTS, _check_footprint, _cloud_grid, _rows_f32

_MODES = ("top", "mean")
BAND_FIX = 2.0 ** 20
# the ray-level maps of view_maps that a grid can carry: float32 (R, D) or (R,)
_NOT_FEATURES = ("surf_idx",)


def band_quanta(band):
    """band in metres -> band_q = llrint(band 2^20), at most 2^62 (the ABI treats everything above alike)."""
    band = float(band)
    if not (math.isfinite(band) and band >= 0):
        raise ValueError(f"ortho: band {band} must be a finite number of metres, at least 0")
    return 1 << 62 if band >= 2.0 ** 42 else int(round(band * BAND_FIX))


class OrthoAccumulator:
    """The integer grids of the orthorectified maps on `device`: acc int64 (H, W, 2 + channels) = (sum_z, count, sum_0 ...) and, in
    top mode, top int64 (H, W).
      add_top(rays, depth, frame)        pass 1 on one chunk (bn_ortho_top); top mode only, and only before the first add
      merge_top(group)                   MAX all-reduce of top over the ranks of a group (call it once, after the last add_top)
      add(rays, depth, frame, features)  pass 2 on one chunk (bn_ortho_splat): features (R, channels) float32 on the device, a
                                         column slice of a wider tensor is read in place
      merge(group)                       SUM all-reduce of acc and the counters
      result()                           -> maps (channels, H, W) float32, dsm (H, W) float32 - NaN where nothing fell - and
                                         count (H, W) int32
      skipped, bad_features, culled      rays with a bad point, rays with a non-finite or |x| >= 2^16 feature, deposits left out
                                         by the top-surface test
    mode 'top': per cell the points with altitude >= (highest altitude reaching that cell) - band; 'mean': all of them.  band in
    metres, band_q = llrint(band 2^20).  radius, footprint as DsmAccumulator.  With channels=0 and mode='mean' acc is
    DsmAccumulator's, bit for bit."""

    def __init__(self, grid, device, channels, radius=1, footprint="disc", mode="top", band=0.5):
        _check_footprint("OrthoAccumulator", radius, footprint)
        if mode not in _MODES:
            raise ValueError(f"OrthoAccumulator: unknown mode {mode!r} ('top' or 'mean')")
        if not 0 <= int(channels) <= L.BN_ORTHO_MAX_CHANNELS:
            raise ValueError(f"OrthoAccumulator: {channels} channels outside [0, {L.BN_ORTHO_MAX_CHANNELS}]")
        self.band_q = band_quanta(band)
        self.grid, self.radius, self.footprint, self.mode, self.band = grid, int(radius), footprint, mode, float(band)
        self.channels = int(channels)
        self.acc = torch.zeros((grid.height, grid.width, 2 + self.channels), dtype=torch.int64, device=device)
        self.top = torch.full((grid.height, grid.width), L.BN_ORTHO_EMPTY, dtype=torch.int64, device=device) if mode == "top" else None
        self._counters = torch.zeros((3,), dtype=torch.int64, device=device)
        self._top_skipped = torch.zeros((1,), dtype=torch.int64, device=device)
        self._added = False

    def _args(self, frame):
        g = self.grid
        return (frame.center, frame.range, g.xoff, g.yoff, g.resolution, self.radius, _FOOTPRINTS[self.footprint]) + frame.world_args()

    @torch.no_grad()
    def add_top(self, rays, depth, frame):
        if self.mode != "top":
            raise ValueError("OrthoAccumulator.add_top: mode='mean' has no top-surface pass")
        if self._added:
            raise ValueError("OrthoAccumulator.add_top: pass 1 must have seen every ray before pass 2 starts, and add() has been called")
        rays, depth = _rows_f32(rays, depth)
        Fn.ortho_top(rays, depth, *self._args(frame), self.top, self._top_skipped)
        return self

    def merge_top(self, group=None):
        import torch.distributed as dist
        from .distributed import allreduce_
        if self.mode != "top":
            raise ValueError("OrthoAccumulator.merge_top: mode='mean' has no top-surface pass")
        allreduce_(self.top, dist.ReduceOp.MAX, group)
        return self

    @torch.no_grad()
    def add(self, rays, depth, frame, features=None):
        R, E = rays.shape[0], self.channels
        given = torch.is_tensor(features) and features.is_cuda and features.dtype == torch.float32 and tuple(features.shape) == (R, E)
        if not given and not (E == 0 and features is None):
            what = f"{tuple(features.shape)} {features.dtype} on {features.device}" if torch.is_tensor(features) else repr(type(features))
            raise ValueError(f"OrthoAccumulator.add: features must be ({R}, {E}) float32 on the device, got {what}")
        rays, depth = _rows_f32(rays, depth)
        self._added = True
        Fn.ortho_splat(rays, depth, *self._args(frame), features if E else None, self.top, self.band_q, self.acc, self._counters)
        return self

    def merge(self, group=None):
        from .distributed import allreduce_
        for t in (self.acc, self._counters):
            allreduce_(t, group=group)
        return self

    @property
    def skipped(self):
        return int(self._counters[0].item())

    @property
    def bad_features(self):
        return int(self._counters[1].item())

    @property
    def culled(self):
        return int(self._counters[2].item())

    @torch.no_grad()
    def result(self):
        return Fn.ortho_resolve(self.acc)


@torch.no_grad()
def ortho_image(models, args, rays, H, W, frame, grid=None, keys=("rgb", "albedo"), mode="top", band=0.5, radius=1, footprint="disc",
                resolution=0.5, fill=False, group=None, **view_maps_kw):
    """The maps of one view on the grid of its DSM.  view_maps runs ONCE (after the same torch.manual_seed its `rgb` and `depth`
    are bitwise view_maps' and render_image's); the view's ray-level maps are small and are kept.  The maps named by `keys` are
    concatenated into one (R, E) feature tensor - `channels` is the key -> (first channel, width) table - and splatted with the
    depth: pass 1 (top mode) and pass 2 over this rank's share of the rays, merged over the `group`.  grid=None: Grid.from_cloud
    of the view's points at `resolution`, as dsm_image.  In mean mode `dsm` is dsm_image's bit for bit.
    -> {"maps": {key: (D, H, W) float32}, "dsm" (H, W), "count" (H, W) int32, "grid", "depth" (R,), "rgb" (R, 3), "skipped",
        "bad_features", "culled", "channels"} - NaN where no point fell.
    fill=True: + "dsm_grid" and "maps_grid" {key: (D, H, W)}: every layer filled through ONE fill_holes(dsm, want_source=True)
    source map with apply_fill, so a hole takes all its channels from the same cell (+ "holes", "max_dist", "source").
    Refused (ValueError naming the key): a key view_maps does not produce for this model, a map that is not float32 per ray,
    more than 32 channels in total.  What view_maps refuses (gsam_only, --sun_v analystic) stays refused by its own message.
    Normals are averaged, not renormalised."""
    from .maps import view_maps
    from .viewwalk import ViewWalk
    keys = tuple(keys)
    if mode not in _MODES:
        raise ValueError(f"ortho_image: unknown mode {mode!r} ('top' or 'mean')")
    band_quanta(band)
    vm = view_maps(models, args, rays, H, W, frame=None, group=group, **view_maps_kw)["maps"]
    channels, cols, E = {}, [], 0
    for key in keys:
        if key not in vm or key in _NOT_FEATURES or vm[key].dtype != torch.float32:
            raise ValueError(f"ortho_image: no ray-level map {key!r} for this model (it has {sorted(k for k in vm if k not in _NOT_FEATURES)})")
        t = vm[key].reshape(rays.shape[0], -1)
        channels[key] = (E, t.shape[1])
        E += t.shape[1]
        if E > L.BN_ORTHO_MAX_CHANNELS:
            raise ValueError(f"ortho_image: {E} channels up to key {key!r}, more than {L.BN_ORTHO_MAX_CHANNELS} in one call")
        cols.append(t)
    features = torch.cat(cols, 1) if cols else None
    depth = vm["depth"]
    if grid is None:
        grid = _cloud_grid(rays, depth, frame, resolution)
    walk = ViewWalk(rays.shape[0], rays.shape[0], group)
    lo, hi = walk.lo, walk.hi
    acc = OrthoAccumulator(grid, rays.device, E, radius, footprint, mode, band)
    if mode == "top":
        acc.add_top(rays[lo:hi], depth[lo:hi], frame).merge_top(group)
    acc.add(rays[lo:hi], depth[lo:hi], frame, None if features is None else features[lo:hi]).merge(group)
    maps, dsm, count = acc.result()
    res = {"maps": {key: maps[c0:c0 + d] for key, (c0, d) in channels.items()}, "dsm": dsm, "count": count, "grid": grid, "depth": depth,
           "rgb": vm["rgb"], "skipped": acc.skipped, "bad_features": acc.bad_features, "culled": acc.culled, "channels": channels}
    if fill:
        from .fill import apply_fill, fill_holes
        filled = fill_holes(dsm, group=group, want_source=True)
        src = filled["source"]
        layers = torch.stack([apply_fill(maps[e], src) for e in range(E)]) if E else maps
        res.update(dsm_grid=filled["filled"], maps_grid={key: layers[c0:c0 + d] for key, (c0, d) in channels.items()},
                   holes=filled["holes"], max_dist=filled["max_dist"], source=src)
    return res


__all__ = ["OrthoAccumulator", "ortho_image"]
