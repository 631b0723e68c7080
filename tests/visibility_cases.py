"""The visibility rule of include/brdfnerf_hip.h ("Visibility over a surface model") as a numpy float64 statement, and the cases
of tests/test_visibility_cpu.py and tests/test_gpu_visibility.py.

The statement is a loop over the step t with array expressions over ALL starts at once: it knows nothing of tiles, blocks, row
bands or direction chunks.  Every operation is one numpy float64 operation, so each is rounded on its own, as in the kernel.
"""
import math

import numpy as np

BLOCKED, VISIBLE, NODATA = 0, 1, 2
INF = float("inf")


def direction(elevation_deg, azimuth_deg):
    """(east, north, up) of relight.directions' convention in float64: (sin az cos el, cos az cos el, sin el)."""
    el, az = math.radians(elevation_deg), math.radians(azimuth_deg)
    return np.array([math.sin(az) * math.cos(el), math.cos(az) * math.cos(el), math.sin(el)], dtype=np.float64)


def _march(dsm, u0, v0, z0, nodata, d, res, eps, zmax):
    H, W = dsm.shape
    n = u0.size
    vis = np.where(nodata, NODATA, VISIBLE).astype(np.uint8)
    hit = np.full(n, -1, dtype=np.int32)
    dx, dy, dz = (np.float64(v) for v in d)
    a = np.fmax(np.fabs(dx), np.fabs(dy))
    if a == 0:
        return vis, hit
    with np.errstate(all="ignore"):
        su, sv, sz = dx / a, -(dy / a), (dz / a) * np.float64(res)
        cells = dsm.astype(np.float64)
        live = ~nodata
        for t in range(1, max(W, H) + 1):
            if not live.any():
                break
            tt = np.float64(t)
            ut, vt, zt = u0 + tt * su, v0 + tt * sv, z0 + tt * sz
            live &= (ut >= 0) & (ut < W) & (vt >= 0) & (vt < H)      # outside: visible, stop
            live &= ~(zt > zmax)                                       # the early exit (zmax = inf: never)
            at = np.flatnonzero(live)
            j, i = np.floor(vt[at]).astype(np.int64), np.floor(ut[at]).astype(np.int64)
            blocked = cells[j, i] > zt[at] + np.float64(eps)
            vis[at[blocked]] = BLOCKED
            hit[at[blocked]] = (j[blocked] * W + i[blocked]).astype(np.int32)
            live[at[blocked]] = False
    return vis, hit


def _counts(vis):
    return np.stack([(vis == c).sum(-1) for c in (BLOCKED, VISIBLE, NODATA)], -1).astype(np.int64)


def grid_zmax(dsm):
    """What the wrappers pass as zmax: the maximum of the non-NaN cells (-inf on an all-NaN grid)."""
    known = dsm[~np.isnan(dsm)]
    return float(known.max()) if known.size else -INF


def grid_statement(dsm, res, dirs, eps=0.0, zmax=INF):
    """-> vis (K, H, W) uint8, hit (K, H, W) int32, counts (K, 3) int64: every cell of the grid as a start."""
    dsm = np.asarray(dsm, dtype=np.float32)
    H, W = dsm.shape
    dirs = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    u0, v0 = (ii.reshape(-1) + 0.5).astype(np.float64), (jj.reshape(-1) + 0.5).astype(np.float64)
    z0 = dsm.reshape(-1).astype(np.float64)
    nodata = ~np.isfinite(z0)
    out = [_march(dsm, u0, v0, z0, nodata, d, res, eps, zmax) for d in dirs]
    vis = np.stack([o[0] for o in out]).reshape(-1, H, W)
    return vis, np.stack([o[1] for o in out]).reshape(-1, H, W), _counts(vis.reshape(len(dirs), -1))


def points_statement(enz, dsm, xoff, yoff, res, dirs, eps=0.0, zmax=INF):
    """-> vis (K, R) uint8, hit (K, R) int32, counts (K, 3) int64: the points (east, north, altitude) as starts."""
    dsm = np.asarray(dsm, dtype=np.float32)
    H, W = dsm.shape
    enz = np.asarray(enz, dtype=np.float64).reshape(-1, 3)
    dirs = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        u0 = (enz[:, 0] - np.float64(xoff)) / np.float64(res)
        v0 = (np.float64(yoff) - enz[:, 1]) / np.float64(res)
        z0 = enz[:, 2].copy()
        nodata = ~(np.isfinite(u0) & np.isfinite(v0) & np.isfinite(z0)) | ~((u0 >= 0) & (u0 < W) & (v0 >= 0) & (v0 < H))
    out = [_march(dsm, u0, v0, z0, nodata, d, res, eps, zmax) for d in dirs]
    vis = np.stack([o[0] for o in out]).reshape(len(dirs), -1)
    return vis, np.stack([o[1] for o in out]).reshape(len(dirs), -1), _counts(vis)


def cell_centres(dsm, xoff, yoff, res):
    """(H W, 3) float64: the centre and the altitude of every cell, row-major - grid mode's starts as points (exact on a dyadic
    origin and resolution)."""
    dsm = np.asarray(dsm, dtype=np.float32)
    H, W = dsm.shape
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    e = xoff + (ii.reshape(-1) + 0.5) * res
    n = yoff - (jj.reshape(-1) + 0.5) * res
    return np.stack([e, n, dsm.reshape(-1).astype(np.float64)], -1)


# ------------------------------------------------------------------------------------------------------------------- cases
RES = 0.5
BLOCK_DIRS = [(30.0, 135.0), (45.0, 90.0), (89.9, 203.0), (5.0, 17.0), (60.0, 315.0)]
BLOCK_BLOCKED = [744, 384, 0, 531, 496]          # the prototype's counts of blocked cells, per direction of BLOCK_DIRS

ZENITH = np.array([0.0, 0.0, 1.0])
CARDINALS = np.array([[0.0, 1.0, 1.0], [1.0, 0.0, 1.0], [0.0, -1.0, 1.0], [-1.0, 0.0, 1.0]]) * np.array([1.0, 1.0, 0.5])
DIAGONAL = np.array([1.0, 1.0, 0.4])             # dx == dy: both axes step by exactly 1
TIE_DIR = np.array([2.0 ** -0.5, 0.0, 2.0 ** -0.5])     # su == 1.0 and, at 0.5 m cells, sz == 0.5 exactly


def oblique_dirs():
    """Azimuths 17 and 203 degrees at elevations 5 (marches that cross the whole grid), 30 and 89.9."""
    return np.stack([direction(el, az) for el in (5.0, 30.0, 89.9) for az in (17.0, 203.0)])


# Non-dyadic slopes whose PRODUCTS land on cell edges: with sv = -0.1 and v0 = j + 0.5, v0 + 5 sv == j exactly, while five additions
# of 0.1 do not add up to 0.5 beside j: a running sum ut += su leaves the rule's cell on these long, flat marches.
EDGE_DIRS = np.array([[1.0, 0.1, 0.02], [-1.0, -0.3, 0.015], [0.7, -1.0, 0.03]])


def all_dirs():
    """Every direction family of the GPU tests in one (18, 3) table, unnormalised twins of two oblique ones included."""
    ob = oblique_dirs()
    return np.concatenate([ZENITH[None], CARDINALS, DIAGONAL[None], ob, (ob[1] * 37.25)[None], (ob[2] * 1e-3)[None], TIE_DIR[None],
                           EDGE_DIRS])


def block_scene():
    """64 x 64 cells of 0.5 m: ground at 10 m, a roof at 30 m on [24:40, 24:40]."""
    dsm = np.full((64, 64), 10.0, dtype=np.float32)
    dsm[24:40, 24:40] = 30.0
    vis, _, _ = grid_statement(dsm, RES, [direction(30.0, 135.0), direction(45.0, 90.0)])
    assert (vis[0] == BLOCKED).sum() >= 300 and (vis[0] == VISIBLE).sum() >= 3000      # conditions on the inputs
    assert (vis[1] == BLOCKED).sum() == 384
    return dsm


def relief(H, W, seed=0, nan=0.05, specials=True, low=-20.0):
    """A rough relief with towers, negative altitudes, a -0.0 cell, `nan` of its cells NaN and one +inf and one -inf cell."""
    rng = np.random.default_rng(seed)
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    dsm = (low + 6.0 * np.sin(0.37 * ii) * np.cos(0.23 * jj) + rng.uniform(0.0, 2.0, (H, W))).astype(np.float32)
    for _ in range(max(1, H * W // 200)):
        j, i = int(rng.integers(H)), int(rng.integers(W))
        dsm[j:j + 3, i:i + 3] += np.float32(rng.uniform(5.0, 40.0))
    flat = dsm.reshape(-1)
    if nan > 0:
        flat[rng.random(flat.size) < nan] = np.nan
    if specials and flat.size >= 8:
        where = rng.choice(flat.size, 3, replace=False)
        flat[where[0]], flat[where[1]], flat[where[2]] = np.inf, -np.inf, -0.0
    return dsm


def tie_row(eps=0.0, above=False):
    """1 x 9 cells of 10.0 with cell 4 at 12 + eps: from cell 0 along TIE_DIR, h == zt + eps at t = 4, which does not block;
    above=True: the next float32 above it, which does.  (12 + eps must be a float32 for the tie to be exact.)"""
    row = np.full((1, 9), 10.0, dtype=np.float32)
    top = np.float32(12.0 + eps)
    assert float(top) == 12.0 + eps
    row[0, 4] = np.nextafter(top, np.float32(np.inf)) if above else top
    return row


GRID_SHAPES = [(1, 1), (1, 7), (7, 1), (7, 9), (33, 65), (64, 64), (40, 257)]


def grid_case(shape):
    """The grid of one of GRID_SHAPES: the block scene at 64 x 64, a relief with every special cell elsewhere."""
    if shape == (64, 64):
        return block_scene()
    if shape[0] * shape[1] < 8:
        return relief(*shape, seed=shape[0] * 1000 + shape[1], nan=0.0, specials=False, low=3.0)
    return relief(*shape, seed=shape[0] * 1000 + shape[1])


def point_case(R, dsm, xoff, yoff, res, seed=0):
    """R points over and around a grid: inside at random altitudes, outside the grid, NaN and inf points, points exactly on cell
    edges and corners, a point on the grid's own western, northern, eastern and southern edge."""
    rng = np.random.default_rng(seed + R)
    H, W = dsm.shape
    lo = float(np.nanmin(np.where(np.isfinite(dsm), dsm, np.nan)))
    e = xoff + rng.uniform(-0.1 * W, 1.1 * W, R) * res
    n = yoff - rng.uniform(-0.1 * H, 1.1 * H, R) * res
    a = lo + rng.uniform(-2.0, 30.0, R)
    pts = np.stack([e, n, a], -1)
    edge = [(xoff + 3 * res, yoff - 2 * res), (xoff, yoff), (xoff + W * res, yoff - res), (xoff + res, yoff - H * res),
            (xoff + (W - 1) * res, yoff - (H - 1) * res)]
    for k, (pe, pn) in enumerate(edge):
        if 5 + k < R:
            pts[5 + k, 0], pts[5 + k, 1] = pe, pn
    if R > 12:
        pts[10, 0], pts[11, 1], pts[12, 2] = np.nan, np.inf, np.nan
    return pts
