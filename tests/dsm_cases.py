"""Cases and the float64 statement of the DSM rasteriser (bn_dsm_splat / bn_dsm_resolve), shared by tests/test_dsm_cpu.py and
tests/test_gpu_dsm.py.

The statement is written from the rule the C header gives and from the reference lines it cites (datasets/satellite_rgb_dep.py:
613-633 for the point, :665-671 and :695 for the grid), not from the product's code: numpy float64 with one rounding per
operation, Python integers for the sums, a loop over points and footprint cells.

  point      p = (o + d depth) range + center, fp32 inputs widened to float64
  skipped    p not finite, or |p.z| >= 2^23: no deposit, skipped += 1
  cell       i = floor((p.x - xoff) / res), j = floor((yoff - p.y) / res); row 0 is the northern edge
  footprint  (j + k2, i + k1) for k1, k2 in [-radius, radius], inside the grid; disc: k1^2 + k2^2 <= radius^2
  deposit    sum += rint(p.z 2^20) as an integer, count += 1
  resolve    dsm = float32(float64(sum) / float64(count) 2^-20), NaN where count == 0; count saturates at 2^31 - 1
"""
import functools

import numpy as np

CENTER = (368412.25, 3359871.75, 12.5)         # a UTM easting / northing: fp32 holds the northing to 0.25 m only
RANGE = 6.0
FIX = 2.0 ** 20
ZMAX = 2.0 ** 23


def points(rays, depth, center=CENTER, rng=RANGE, fp32_positions=False):
    """(R, 3) float64 world points of fp32 rays (R, >= 6) and depths (R,).  fp32_positions: the positions a float32
    implementation would hold (rounded once at the end, its best case)."""
    rays = np.asarray(rays, dtype=np.float32)
    o, d = rays[:, 0:3].astype(np.float64), rays[:, 3:6].astype(np.float64)
    t = np.asarray(depth, dtype=np.float32).astype(np.float64).reshape(-1, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        p = d * t
        p = o + p
        p = p * np.float64(rng)
        p = p + np.asarray(center, dtype=np.float64)
        if fp32_positions:
            p = p.astype(np.float32).astype(np.float64)
    return p


def splat(rays, depth, grid, radius, footprint, center=CENTER, rng=RANGE, fp32_positions=False, acc=None):
    """-> (sums (H, W) of Python ints as an object array, counts likewise, skipped).  grid = (xoff, yoff, res, W, H).
    acc = (sums, counts, skipped) of an earlier call is added to (chunks, several views)."""
    xoff, yoff, res, W, H = grid
    xoff, yoff, res = np.float64(xoff), np.float64(yoff), np.float64(res)
    if acc is None:
        sums, counts, skipped = np.zeros((H, W), dtype=object), np.zeros((H, W), dtype=object), 0
    else:
        sums, counts, skipped = acc[0].copy(), acc[1].copy(), acc[2]
    for px, py, pz in points(rays, depth, center, rng, fp32_positions):
        if not (np.isfinite(px) and np.isfinite(py) and np.isfinite(pz)) or not abs(pz) < ZMAX:
            skipped += 1
            continue
        fi, fj = np.floor((px - xoff) / res), np.floor((yoff - py) / res)
        if not (-radius <= fi <= W - 1 + radius and -radius <= fj <= H - 1 + radius):     # (in float64: a far point's index may be huge)
            continue
        i, j = int(fi), int(fj)
        q = int(np.rint(pz * FIX))
        for k2 in range(-radius, radius + 1):
            for k1 in range(-radius, radius + 1):
                row, col = j + k2, i + k1
                if not (0 <= row < H and 0 <= col < W):
                    continue
                if footprint == "disc" and k1 * k1 + k2 * k2 > radius * radius:
                    continue
                sums[row, col] += q
                counts[row, col] += 1
    return sums, counts, skipped


def resolve(sums, counts):
    """-> dsm (H, W) float32 with NaN where nothing fell, count (H, W) int32."""
    H, W = sums.shape
    dsm = np.full((H, W), np.nan, dtype=np.float32)
    cnt = np.zeros((H, W), dtype=np.int32)
    for r in range(H):
        for c in range(W):
            n = int(counts[r, c])
            cnt[r, c] = min(n, 2 ** 31 - 1)
            if n:
                dsm[r, c] = np.float32(np.float64(int(sums[r, c])) / np.float64(n) * (1.0 / FIX))
    return dsm, cnt


def as_int64(a):
    return np.array(a.tolist(), dtype=np.int64).reshape(a.shape)


# ------------------------------------------------------------------------------------------------------------------ cases
# Grids: 7 x 5 cells of 0.5 m whose corner is 3 m west / 1 m north of the centre (non-square: a transposition shows), and
# 40 x 30 cells of 0.3 m (a resolution that is no power of two: the division rounds).
SMALL = (CENTER[0] - 3.0, CENTER[1] + 1.0, 0.5, 7, 5)
LARGE = (CENTER[0] - 6.0, CENTER[1] + 4.5, 0.3, 40, 30)


def _nadir(x_m, y_m, z_m, depth):
    """Rays looking straight down whose point is EXACTLY (center.x + x_m, center.y + y_m, center.z + z_m) for offsets that are
    multiples of 1.5 m / 2^k (o = offset / 6 is then a dyadic fp32 number and o * 6 is exact): d = (0, 0, -1), o.z = z / 6 + depth."""
    x_m, y_m, z_m = np.broadcast_arrays(np.asarray(x_m, np.float64), np.asarray(y_m, np.float64), np.asarray(z_m, np.float64))
    n = x_m.size
    rays = np.zeros((n, 8), dtype=np.float32)
    rays[:, 0], rays[:, 1] = (x_m / RANGE).ravel(), (y_m / RANGE).ravel()
    rays[:, 2] = (z_m / RANGE).ravel() + depth
    rays[:, 5] = -1.0
    rays[:, 6], rays[:, 7] = 0.0, 2.0
    return rays, np.full((n,), depth, dtype=np.float32)


def _edge_points():
    """Points on cell edges of SMALL and on its outer edges, and points just outside it whose neighbours are inside.
    SMALL spans x in [-3, 0.5) and y in (-1.5, 1] metres around the centre; offsets are multiples of 0.75 m (dyadic / 6).
      x  -3 the west outer edge (column 0), -1.5 and 0 interior edges (columns 3, 6), -2.25 / -0.75 cell centres, 0.75 one column
         east of the grid, -3.75 two columns west of it
      y  1.5 exactly on the upper edge of the row ABOVE the grid (row -1), 0 an interior edge (row 2), -1.5 exactly the south outer
         edge (row 5, outside), 0.75 / -0.75 cell centres (rows 0, 3), 2.25 three rows north: out of reach of radius 2"""
    xs = np.array([-3.0, -2.25, -1.5, -0.75, 0.0, 0.75, -3.75])
    ys = np.array([1.5, 0.75, 0.0, -0.75, -1.5, 2.25])
    X, Y = np.meshgrid(xs, ys)
    Z = -3.0 + 1.5 * ((np.arange(X.size) % 5) - 1).reshape(X.shape)      # altitudes 8, 9.5, ..., 14: offsets -4.5 .. 1.5
    r, t = _nadir(X.ravel(), Y.ravel(), Z.ravel(), 0.5)
    # negative altitudes: 12.5 - 18 = -5.5 m and 12.5 - 13.5 = -1 m, inside the grid
    r2, t2 = _nadir(np.array([-1.5, -0.375]), np.array([0.375, 0.75]), np.array([-18.0, -13.5]), 0.25)
    return np.concatenate([r, r2]), np.concatenate([t, t2])


def _bad_rows():
    """Rows that must be skipped: NaN depth, +-inf depth, |p.z| == 2^23 exactly and far beyond; and one just inside the bound."""
    r, t = _nadir(np.zeros(6) - 1.5, np.zeros(6), np.zeros(6), 0.0)
    r[:, 2] = 0.25
    t[:] = [np.nan, np.inf, -np.inf, 0.0, 0.0, 0.0]
    r[3, 5], t[3] = 1.0, 1398099.0          # (0.25 + 1398099) 6 + 12.5 == 8388608 == 2^23: skipped
    r[4, 5], t[4] = -1.0, 2.0e6             # about -1.2e7 m: skipped
    r[5, 5], t[5] = 1.0, 1398098.0          # 8388602 m: the largest altitudes are deposited
    return r, t, 5


def _random(n, seed, half_x, half_y):
    """Oblique rays (|d.xy| up to ~0.1) with depths 0-4: points spread over +-half metres around the centre and beyond, altitudes
    from about -6 m to 19 m."""
    g = np.random.RandomState(seed)
    rays = np.zeros((n, 8), dtype=np.float32)
    rays[:, 0] = g.uniform(-half_x, half_x, n) / RANGE
    rays[:, 1] = g.uniform(-half_y, half_y, n) / RANGE
    rays[:, 2] = 1.0 + g.uniform(-0.1, 0.1, n)
    d = np.stack([g.uniform(-0.1, 0.1, n), g.uniform(-0.1, 0.1, n), -np.ones(n)], -1)
    rays[:, 3:6] = d / np.linalg.norm(d, axis=-1, keepdims=True)
    rays[:, 7] = 4.0
    return rays, g.uniform(0.0, 4.0, n).astype(np.float32)


def _mixed(R, seed, grid):
    """R rows: the edge points and the rows to skip first (as many as fit), random rows for the rest."""
    half_x, half_y = 0.6 * grid[2] * grid[3], 0.6 * grid[2] * grid[4]
    er, et = _edge_points()
    br, bt, _ = _bad_rows()
    rr, rt = _random(R, seed, half_x, half_y)
    # shift the random rows over the grid's middle (SMALL and LARGE are not centred on the frame's centre)
    rr[:, 0] += np.float32((grid[0] + 0.5 * grid[2] * grid[3] - CENTER[0]) / RANGE)
    rr[:, 1] += np.float32((grid[1] - 0.5 * grid[2] * grid[4] - CENTER[1]) / RANGE)
    rays, depth = np.concatenate([br, er, rr])[:R], np.concatenate([bt, et, rt])[:R]
    perm = np.random.RandomState(seed + 1).permutation(R)             # the rows to skip are not all in one wavefront
    return np.ascontiguousarray(rays[perm]), np.ascontiguousarray(depth[perm])


def _one_point():
    return _nadir(np.array([-1.5]), np.array([0.0]), np.array([1.5]), 0.5)          # on the corner of four interior cells


def _contention():
    """4096 points inside ONE cell of SMALL (cell row 1, column 3: x in [-1.5, -1), y in (0, 0.5]), altitudes of both signs."""
    g = np.random.RandomState(7)
    n = 4096
    r, t = _nadir(np.zeros(n), np.zeros(n), np.zeros(n), 0.5)
    r[:, 0] = g.uniform(-1.45, -1.05, n) / RANGE
    r[:, 1] = g.uniform(0.05, 0.45, n) / RANGE
    r[:, 2] += g.uniform(-4.0, 1.0, n).astype(np.float32)
    return r, t


# name -> (grid, radius, footprint, builder): R in {1, 63, 65, 300, 4096}, radius in {0, 1, 2}, both footprints
CASES = {
    "one_point_r1_disc": (SMALL, 1, "disc", _one_point),
    "small_R63_r0_square": (SMALL, 0, "square", lambda: _mixed(63, 1, SMALL)),
    "small_R65_r1_disc": (SMALL, 1, "disc", lambda: _mixed(65, 2, SMALL)),
    "small_R65_r1_square": (SMALL, 1, "square", lambda: _mixed(65, 2, SMALL)),
    "small_R63_r2_disc": (SMALL, 2, "disc", lambda: _mixed(63, 3, SMALL)),
    "large_R300_r0_disc": (LARGE, 0, "disc", lambda: _mixed(300, 4, LARGE)),
    "large_R300_r1_disc": (LARGE, 1, "disc", lambda: _mixed(300, 5, LARGE)),
    "large_R300_r2_square": (LARGE, 2, "square", lambda: _mixed(300, 6, LARGE)),
    "large_R300_r2_disc": (LARGE, 2, "disc", lambda: _mixed(300, 6, LARGE)),
    "contention_R4096_r1_disc": (SMALL, 1, "disc", _contention),
}
# the case of the fp32-position guard: rounding the positions to fp32 (0.25 m at this northing) must change its result
FP32_GUARD_CASE = "large_R300_r1_disc"


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (grid, radius, footprint, rays (R, 8) float32, depth (R,) float32), built once."""
    grid, radius, footprint, make = CASES[name]
    rays, depth = make()
    rays.setflags(write=False)
    depth.setflags(write=False)
    return grid, radius, footprint, rays, depth


@functools.lru_cache(maxsize=None)
def expected(name, fp32_positions=False):
    """The statement's result for a case, computed once and shared: dict sums / counts (int64 (H, W)), skipped, dsm, count."""
    grid, radius, footprint, rays, depth = case(name)
    sums, counts, skipped = splat(rays, depth, grid, radius, footprint, fp32_positions=fp32_positions)
    dsm, cnt = resolve(sums, counts)
    res = {"sums": as_int64(sums), "counts": as_int64(counts), "skipped": skipped, "dsm": dsm, "count": cnt}
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res
