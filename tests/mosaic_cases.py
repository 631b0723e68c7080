"""The numpy statement of the orthomosaic rule (include/brdfnerf_hip.h, "Orthomosaic of several observed images") and its cases.

fuse is the rule's step 3 from the per-view values and states on: a loop over the views of array expressions in float64, one ufunc
per operation, with nothing of tiles, lanes or blocks in it.  mosaic composes the per-view statements the project already has -
orthophoto_cases.grid_pixels and gather, visibility_cases.grid_statement - with fuse.  Nothing here is shared with
brdf_nerf_amd/mosaic.py or the kernel.
"""
import numpy as np

import orthophoto_cases as O
import visibility_cases as V
from camera_cases import SITES, make_rpc

NODATA, OUTSIDE, OCCLUDED, USED, NONFINITE = 0, 1, 2, 3, 4
STATES = ("nodata", "outside", "occluded", "used", "nonfinite")
MAX_VIEWS, MAX_CHANNELS = 32, 4
Q20 = 2.0 ** 20
GRIDS = ((1, 1), (3, 5), (1, 255), (1, 256), (1, 257), (33, 65))          # (H, W): one lane, lane and block edges, two rows of blocks
VIEW_COUNTS = (1, 2, 3, 5, 32)
CHANNELS = (1, 3, 4)
IMAGE_SIZES = ((1, 1), (2, 2), (5, 7), (33, 65))                            # (Hi, Wi), different ones in one call
ROW_SPLITS = (0, 1, 32)                                                     # and H
SCENE_SEEDS = (3, 5, 7)                                                     # the three views of the box scene
PLANTED = (0.001, 0.002, 0.0005, 0.0017, 0.0011)                            # around 4096: where sum-of-squares loses the spread


def fuse(values, states, rank):
    """values float32 (K, C, n): what the gather gave per view; states (K, n) in {0, 1, 2, KEPT 3}; rank K integers.
    -> {"count" uint8 (n), "best" int32 (n), "best_val", "mean", "std" float32 (C, n), "states" uint8 (K, n) with 3 = USED and
    4 = NONFINITE, "counts" int64 (K, 5), "sums" [cells, q, skipped], and "mean64", "std64" (C, n): m and sqrt(M2 / n) before the cast}."""
    values = np.asarray(values, np.float32)
    K, C, n = values.shape
    states = np.array(states, dtype=np.uint8).reshape(K, n)
    count = np.zeros(n, dtype=np.int64)
    m, M2 = np.zeros((C, n)), np.zeros((C, n))
    best, best_rank = np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=np.int64)
    best_val = np.full((C, n), np.nan, dtype=np.float32)
    for k in range(K):
        kept = states[k] == O.KEPT
        finite = np.isfinite(values[k]).all(0)
        states[k][kept & ~finite] = NONFINITE
        used = kept & finite
        count = count + used
        with np.errstate(all="ignore"):
            x = values[k].astype(np.float64)
            delta = x - m
            m_next = m + delta / np.maximum(count, 1).astype(np.float64)
            M2_next = M2 + delta * (x - m_next)
        m, M2 = np.where(used, m_next, m), np.where(used, M2_next, M2)
        wins = used & ((count == 1) | (int(rank[k]) < best_rank))
        best[wins], best_rank[wins] = k, int(rank[k])
        best_val.view(np.uint32)[:, wins] = values[k].view(np.uint32)[:, wins]          # 32 bits each
    seen = count > 0
    with np.errstate(all="ignore"):
        s = np.sqrt(M2 / count.astype(np.float64))
    mean = np.where(seen, m.astype(np.float32), np.float32(np.nan)).astype(np.float32)
    std = np.where(seen, s.astype(np.float32), np.float32(np.nan)).astype(np.float32)
    twice = s[:, count >= 2]
    small = twice < Q20
    sums = [int((count >= 2).sum()), int(np.rint(twice[small] * Q20).astype(np.int64).sum()), int((~small).sum())]
    counts = np.array([[(states[k] == st).sum() for st in range(5)] for k in range(K)], dtype=np.int64)
    return {"count": count.astype(np.uint8), "best": best, "best_val": best_val, "mean": mean, "std": std, "states": states,
            "counts": counts, "sums": sums, "mean64": np.where(seen, m, np.nan), "std64": np.where(seen, s, np.nan)}


def two_pass(values, used):
    """The float64 mean and population std of the used views of every cell by np.mean / np.std: values (K, C, n), used bool (K, n)
    -> mean, std (C, n), NaN where no view is used."""
    values = np.asarray(values, np.float32).astype(np.float64)
    K, C, n = values.shape
    mean, std = np.full((C, n), np.nan), np.full((C, n), np.nan)
    for i in range(n):
        if used[:, i].any():
            mean[:, i], std[:, i] = values[used[:, i], :, i].mean(0), values[used[:, i], :, i].std(0)
    return mean, std


def sum_of_squares_std(values):
    """The std of ONE cell's used values (K,) float32 by q / n - m m in float64: the form the rule does not use."""
    x = np.asarray(values, np.float32).astype(np.float64)
    s, q = 0.0, 0.0
    for v in x:
        s, q = s + v, q + v * v
    m = s / len(x)
    return np.sqrt(max(q / len(x) - m * m, 0.0))


def planted_values(C=1):
    """float32 (5, C, 1): five views of one cell, 4096 + PLANTED (+ the channel)."""
    return np.stack([np.full((C, 1), 4096.0 + p, dtype=np.float64) + np.arange(C)[:, None] for p in PLANTED]).astype(np.float32)


def planted_image(C, Hi, Wi, k):
    """A constant image of view k of the planted stack: every gather of it, in either mode, is the planted value."""
    return np.broadcast_to(planted_values(C)[k % len(PLANTED)][:, :, None], (C, Hi, Wi)).astype(np.float32).copy()


def random_stack(K, C, n, seed=0, specials=True):
    """values (K, C, n) float32 in [-2, 3) and states (K, n) over all four gather states; specials: some NaN and inf values."""
    rng = np.random.default_rng(seed + 100 * K + 10 * C + n)
    values = rng.uniform(-2.0, 3.0, (K, C, n)).astype(np.float32)
    states = rng.choice(np.array([0, 1, 2, 3, 3, 3, 3], dtype=np.uint8), (K, n))
    if specials:
        values[rng.random((K, C, n)) < 0.03] = np.nan
        values[rng.random((K, C, n)) < 0.02] = np.inf
    return values, states


def nadir_ranks(view_dirs):
    """rank[k] = the place of view k among the views sorted by descending dz / |d|, ties by index."""
    d = np.asarray(view_dirs, np.float64)
    up = d[:, 2] / np.sqrt((d * d).sum(1))
    order = sorted(range(len(up)), key=lambda k: (-up[k], k))
    return [order.index(k) for k in range(len(up))]


def mosaic(ds, planes, dsm, xoff, yoff, res, zone, south=False, occlusion=True, eps=0.0, view_dirs=None, rank=None, mode="bilinear"):
    """The whole chain: ds K descriptors, planes K arrays (C, Hi_k, Wi_k).  -> fuse's dictionary with (C, H, W) / (H, W) shapes, and
    "colrow" (K, H, W, 2), "vis" (K, H, W) or None, "view_dirs", "rank"."""
    dsm = np.asarray(dsm, np.float32)
    H, W = dsm.shape
    K = len(ds)
    colrow = np.stack([O.grid_pixels(d, dsm, xoff, yoff, res, zone, south)[0] for d in ds])
    vis = None
    if occlusion:
        if view_dirs is None:
            known = dsm[np.isfinite(dsm)]
            lo, hi = float(known.min()), float(known.max())
            view_dirs = np.stack([O.view_direction(d, zone, south, lo, max(hi, lo + 1.0)) for d in ds])
        vis = V.grid_statement(dsm, res, list(view_dirs), eps, V.grid_zmax(dsm))[0]
    if rank is None:
        rank = list(range(K)) if view_dirs is None else nadir_ranks(view_dirs)
    per_view = [O.gather(planes[k], colrow[k], None if vis is None else vis[k], mode) for k in range(K)]
    res_ = fuse(np.stack([p[0] for p in per_view]), np.stack([p[1] for p in per_view]), rank)
    for key in ("best_val", "mean", "std"):
        res_[key] = res_[key].reshape(-1, H, W)
    for key in ("count", "best"):
        res_[key] = res_[key].reshape(H, W)
    res_.update(colrow=colrow, vis=vis, view_dirs=view_dirs, rank=list(rank))
    return res_


def box_views():
    """The box scene of orthophoto_cases under three cameras: -> ds (3 descriptors), dsm, xoff, yoff, res, zone."""
    _, dsm, xoff, yoff, res = O.box_scene()
    return [make_rpc(O.SCENE_SITE, s) for s in SCENE_SEEDS], dsm, xoff, yoff, res, SITES[O.SCENE_SITE][2]


def consistency(sums, C):
    cells, q, _ = sums
    return q / (cells * C * (1 << 20)) if cells else float("nan")


# ------------------------------------------------------------------------------------------------ one texture under three cameras
TEXTURE_IMAGE = (192, 192)
TEXTURE_GRADIENT = (1.0, 0.75)               # per metre east and north: 6 m of altitude error move a roof's texture by several units
BOX = (slice(18, 28), slice(14, 24))         # the box of orthophoto_cases.box_scene: rows, columns


def fine_views():
    """box_views with every camera eight times finer (0.54 m per pixel) and centred in a TEXTURE_IMAGE, so that the 24 x 20 m scene
    spans some forty pixels: the four image scales and offsets are the camera's affine part, any values are a camera."""
    ds, dsm, xoff, yoff, res, zone = box_views()
    Hi, Wi = TEXTURE_IMAGE
    fine = [dict(d, col_scale=d["col_scale"] * 8.0, row_scale=d["row_scale"] * 8.0, col_offset=Wi / 2.0, row_offset=Hi / 2.0) for d in ds]
    return fine, dsm, xoff, yoff, res, zone


def textured_images(ds, dsm, xoff, yoff, res, zone):
    """What each camera sees of ONE texture T(e, n) = gx (e - e0) + gy (n - n0) painted on the box scene `dsm` (flat ground with
    one box): a pixel whose ray meets the roof's altitude inside the box's footprint shows the roof point, every other pixel the
    ground point (a facade shows the ground behind it: those cells are occluded for that camera).  -> K arrays (1, Hi, Wi)."""
    from camera_cases import localize, utm
    Hi, Wi = TEXTURE_IMAGE
    ground, roof = float(dsm[0, 0]), float(dsm[BOX][0, 0])
    e0, n0 = xoff + 0.5 * dsm.shape[1] * res, yoff - 0.5 * dsm.shape[0] * res
    west, east = xoff + BOX[1].start * res, xoff + BOX[1].stop * res
    north, south = yoff - BOX[0].start * res, yoff - BOX[0].stop * res
    rr, cc = np.meshgrid(np.arange(Hi, dtype=np.float64), np.arange(Wi, dtype=np.float64), indexing="ij")
    images = []
    for d in ds:
        pts = []
        for alt in (roof, ground):
            lon, lat, bad = localize(d, cc.ravel(), rr.ravel(), alt)
            assert not bad.any()
            pts.append(utm(lon, lat, zone, False))
        on_roof = (pts[0][0] >= west) & (pts[0][0] < east) & (pts[0][1] > south) & (pts[0][1] <= north)
        e, n = np.where(on_roof, pts[0][0], pts[1][0]), np.where(on_roof, pts[0][1], pts[1][1])
        images.append((TEXTURE_GRADIENT[0] * (e - e0) + TEXTURE_GRADIENT[1] * (n - n0)).astype(np.float32).reshape(1, Hi, Wi))
    return images


def raised(dsm, by=6.0):
    """The box scene with the box `by` metres too high: a wrong surface model of the same site."""
    out = np.array(dsm, dtype=np.float32)
    out[BOX] += np.float32(by)
    return out
