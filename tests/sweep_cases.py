"""The numpy statement of the altitude sweep (include/brdfnerf_hip.h, "Altitude sweep of a surface model under several observed
images") and its cases.

pick is the rule's steps 2 to 5 from the per-level, per-view values and states on: a loop over the levels, then the views, of array
expressions in float64, one ufunc per operation, with its own Welford loop and argmin and nothing of tiles, lanes or blocks in it.
sweep composes the per-view statements the project already has - orthophoto_cases.cell_centres, world_pixels and gather,
visibility_cases.grid_statement - with pick.  Nothing here is shared with brdf_nerf_amd/sweep.py or the kernel.
"""
import numpy as np

import mosaic_cases as M
import orthophoto_cases as O
import visibility_cases as V

MAX_LEVELS = 256
Q20 = 2.0 ** 20
SCENE_OFFSETS = np.arange(-8, 9) * 1.0                                      # -8 .. 8 m in steps of 1 m: level 2 is -6 m, level 8 is 0
# (K, C, Z, min_views) of the bit-equality cases: every K, C, Z and min_views the rule names, no full product
STATEMENT_CASES = ((1, 1, 1, 1), (2, 3, 2, 2), (3, 4, 17, 3), (5, 3, 17, 2), (32, 1, 2, 2), (32, 4, 17, 3), (2, 1, 256, 1), (3, 3, 256, 2))


def pick(levels, base, offsets, min_views=2, strict=True, want_cost=True):
    """levels: an iterable of Z pairs (values float32 (K, C, n), states (K, n) in {0, 1, 2, KEPT 3}), what the gather gave per view at
    each level; base float32 (n): the DSM; offsets Z floats.  strict=False: the `<=` comparison the rule does NOT use.
    -> {"level" int32 (n), "cost_min", "altitude" float32 (n), "count" uint8 (n), "cost" float32 (Z, n) or None, "valid", "wins" Z
    ints, "sums" [cells, q, skipped], "cost64" (n): best_v before the cast}."""
    base = np.asarray(base, np.float32).reshape(-1)
    n_cells = base.size
    offsets = np.asarray(offsets, np.float64)
    best = np.full(n_cells, -1, dtype=np.int32)
    best_v, best_n = np.zeros(n_cells), np.zeros(n_cells, dtype=np.int64)
    valid, volume = [], []
    for l, (values, states) in enumerate(levels):
        values = np.asarray(values, np.float32)
        K, C, _ = values.shape
        n = np.zeros(n_cells, dtype=np.int64)
        m, M2 = np.zeros((C, n_cells)), np.zeros((C, n_cells))
        for k in range(K):
            used = (np.asarray(states[k]) == O.KEPT) & np.isfinite(values[k]).all(0)
            n = n + used
            with np.errstate(all="ignore"):
                x = values[k].astype(np.float64)
                delta = x - m
                m_next = m + delta / np.maximum(n, 1).astype(np.float64)
                M2_next = M2 + delta * (x - m_next)
            m, M2 = np.where(used, m_next, m), np.where(used, M2_next, M2)
        ok = n >= min_views
        v = np.zeros(n_cells)
        for ch in range(C):
            v = v + M2[ch] / np.maximum(n, 1).astype(np.float64)
        if want_cost:
            volume.append(np.where(ok, v.astype(np.float32), np.float32(np.nan)).astype(np.float32))
        better = (v < best_v) if strict else (v <= best_v)
        take = ok & ((best < 0) | better)
        best, best_v, best_n = np.where(take, np.int32(l), best), np.where(take, v, best_v), np.where(take, n, best_n)
        valid.append(int(ok.sum()))
    Z = len(valid)
    assert Z == len(offsets)
    has = best >= 0
    with np.errstate(all="ignore"):
        alt = (base.astype(np.float64) + offsets[np.maximum(best, 0)]).astype(np.float32)
    small = best_v[has] < Q20
    sums = [int(has.sum()), int(np.rint(best_v[has][small] * Q20).astype(np.int64).sum()), int((~small).sum())]
    return {"level": best.astype(np.int32), "cost_min": np.where(has, best_v.astype(np.float32), np.float32(np.nan)).astype(np.float32),
            "altitude": np.where(has, alt, np.float32(np.nan)).astype(np.float32), "count": np.where(has, best_n, 0).astype(np.uint8),
            "cost": np.stack(volume) if want_cost else None, "valid": valid, "wins": np.bincount(best[has], minlength=Z).tolist(),
            "sums": sums, "cost64": np.where(has, best_v, np.nan)}


def level_pixels(ds, dsm, xoff, yoff, res, zone, offsets, south=False):
    """colrow float64 (Z, K, H, W, 2): the pixel of every cell at a_l = (double)dsm + offsets[l] under every view."""
    dsm = np.asarray(dsm, np.float32)
    e, n = O.cell_centres(*dsm.shape, xoff, yoff, res)
    with np.errstate(all="ignore"):
        return np.stack([np.stack([O.world_pixels(d, e, n, dsm.astype(np.float64) + float(o), zone, south)[0] for d in ds])
                         for o in offsets])


def gathered(planes, colrow, vis, mode):
    """The levels of pick from the pixels: planes K arrays (C, Hi_k, Wi_k), colrow (Z, K, ..., 2), vis K masks or Nones."""
    for per_level in colrow:
        per_view = [O.gather(p, cr, v, mode) for p, cr, v in zip(planes, per_level, vis)]
        yield np.stack([p[0] for p in per_view]), np.stack([p[1] for p in per_view])


def sweep(ds, planes, dsm, xoff, yoff, res, zone, offsets, south=False, occlusion=True, eps=0.0, view_dirs=None, min_views=2,
          mode="bilinear", strict=True):
    """The whole chain: ds K descriptors, planes K arrays (C, Hi_k, Wi_k).  The masks are those of `dsm` itself, at every level.
    -> pick's dictionary with (H, W) / (Z, H, W) shapes, and "colrow" (Z, K, H, W, 2), "vis" (K, H, W) or None, "view_dirs"."""
    dsm = np.asarray(dsm, np.float32)
    H, W = dsm.shape
    K = len(ds)
    vis = None
    if occlusion:
        if view_dirs is None:
            known = dsm[np.isfinite(dsm)]
            lo, hi = float(known.min()), float(known.max())
            view_dirs = np.stack([O.view_direction(d, zone, south, lo, max(hi, lo + 1.0)) for d in ds])
        vis = V.grid_statement(dsm, res, list(view_dirs), eps, V.grid_zmax(dsm))[0]
    colrow = level_pixels(ds, dsm, xoff, yoff, res, zone, offsets, south)
    got = pick(gathered(planes, colrow, [None] * K if vis is None else vis, mode), dsm, offsets, min_views, strict)
    for key in ("level", "cost_min", "altitude", "count", "cost64"):
        got[key] = got[key].reshape(H, W)
    got["cost"] = got["cost"].reshape(-1, H, W)
    got.update(colrow=colrow, vis=vis, view_dirs=view_dirs)
    return got


def roof_mask(dsm):
    roof = np.zeros(np.asarray(dsm).shape, dtype=bool)
    roof[M.BOX] = True
    return roof


def scene():
    """mosaic_cases.fine_views with the one texture painted on it: -> ds, planes, dsm, xoff, yoff, res, zone."""
    ds, dsm, xoff, yoff, res, zone = M.fine_views()
    return ds, M.textured_images(ds, dsm, xoff, yoff, res, zone), dsm, xoff, yoff, res, zone


def scene_counts(got, dsm, roof_level, ground_level=8):
    """(roof cells at roof_level, ground cells with a result, ground cells among them NOT at ground_level, cells without a result)."""
    roof = roof_mask(dsm)
    level = np.asarray(got["level"]).reshape(roof.shape)
    has = level >= 0
    return (int((level[roof] == roof_level).sum()), int((has & ~roof).sum()), int((has & ~roof & (level != ground_level)).sum()),
            int((~has).sum()))


# the exact counts of the scene under SCENE_OFFSETS, min_views = 2, bilinear, with occlusion: recorded from the statement
SCENE_RECORD = {"raised": {"roof": 82, "ground": 1599, "none": 221, "valid": [1699] * 17,
                           "wins": [0, 8, 82, 4, 1, 2, 2, 1, 1599, 0, 0, 0, 0, 0, 0, 0, 0]},
                "true": {"roof": 82, "ground": 1599, "none": 221, "valid": [1699] * 17,
                         "wins": [0, 0, 0, 0, 0, 0, 0, 8, 1681, 4, 1, 2, 2, 1, 0, 0, 0]},
                # offsets + 0.1 m, non-dyadic: level 2 is -5.9 m
                "raised_tenth": {"roof": 85, "ground": 1599, "none": 221, "valid": [1699] * 17,
                                 "wins": [0, 12, 85, 0, 0, 0, 2, 1, 1599, 0, 0, 0, 0, 0, 0, 0, 0]},
                # occlusion=False: the cells behind the facades get a result too, and 36 of them not at 0
                "raised_unoccluded": {"roof": 82, "ground": 1820, "none": 0, "valid": [1920] * 17,
                                      "wins": [0, 8, 82, 4, 7, 8, 13, 14, 1784, 0, 0, 0, 0, 0, 0, 0, 0]}}
