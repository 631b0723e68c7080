"""Cases and the float64 / Python-integer statement of the orthorectified maps (bn_ortho_top / bn_ortho_splat / bn_ortho_resolve),
shared by tests/test_ortho_cpu.py and tests/test_gpu_ortho.py.

There is no upstream counterpart for the feature channels: the statement is written from the rule the C header gives
("Orthorectified maps of a view"), not from the product's code - numpy float64 with one rounding per operation for the point
(dsm_cases.points), Python integers for every sum and maximum, a plain loop over rays, footprint cells and channels.

  point      p = (o + d depth) range + center ; bad: p not finite or |p.z| >= 2^23
  cell       i = floor((p.x - xoff) / res), j = floor((yoff - p.y) / res) ; q = rint(p.z 2^20)
  footprint  (j + k2, i + k1), k1, k2 in [-radius, radius], inside the grid; disc: k1^2 + k2^2 <= radius^2
  top        top[cell] = max(top[cell], q) over the footprint ; EMPTY = -2^63 ; a bad point: skipped += 1
  splat      a bad point: counters[0] += 1 and nothing else.  Otherwise f_e = rint(float64(x_e) 2^24); any x_e not finite or
             |x_e| >= 2^16: counters[1] += 1 and nothing else.  Per footprint cell: q + band_q < top[cell] -> counters[2] += 1,
             else sum_z += q, count += 1, sum_e += f_e
  resolve    maps[e] = float32(float64(sum_e) / float64(count) 2^-24), dsm = float32(float64(sum_z) / float64(count) 2^-20), NaN
             where count == 0; count saturates at 2^31 - 1
"""
import functools

import numpy as np

import dsm_cases as D

EMPTY = -(1 << 63)
FIX_X = 2.0 ** 24
XMAX = 2.0 ** 16
CENTER, RANGE = D.CENTER, D.RANGE


def band_q(band):
    return int(np.rint(np.float64(band) * D.FIX))


def _footprint(i, j, W, H, radius, footprint):
    for k2 in range(-radius, radius + 1):
        for k1 in range(-radius, radius + 1):
            row, col = j + k2, i + k1
            if not (0 <= row < H and 0 <= col < W):
                continue
            if footprint == "disc" and k1 * k1 + k2 * k2 > radius * radius:
                continue
            yield row, col


def _cells(rays, depth, grid, radius, center, rng):
    """Per ray: None (bad point), () (a footprint that cannot touch the grid) or (i, j, q)."""
    xoff, yoff, res, W, H = grid
    xoff, yoff, res = np.float64(xoff), np.float64(yoff), np.float64(res)
    out = []
    for px, py, pz in D.points(rays, depth, center, rng):
        if not (np.isfinite(px) and np.isfinite(py) and np.isfinite(pz)) or not abs(pz) < D.ZMAX:
            out.append(None)
            continue
        fi, fj = np.floor((px - xoff) / res), np.floor((yoff - py) / res)
        if not (-radius <= fi <= W - 1 + radius and -radius <= fj <= H - 1 + radius):
            out.append(())
            continue
        out.append((int(fi), int(fj), int(np.rint(pz * D.FIX))))
    return out


def top_pass(rays, depth, grid, radius, footprint, center=CENTER, rng=RANGE, top=None):
    """-> (top (H, W) object array of Python ints, skipped).  top = (array, skipped) of an earlier call is continued."""
    _, _, _, W, H = grid
    if top is None:
        t, skipped = np.full((H, W), EMPTY, dtype=object), 0
    else:
        t, skipped = top[0].copy(), top[1]
    for cell in _cells(rays, depth, grid, radius, center, rng):
        if cell is None:
            skipped += 1
            continue
        if not cell:
            continue
        i, j, q = cell
        for row, col in _footprint(i, j, W, H, radius, footprint):
            t[row, col] = max(t[row, col], q)
    return t, skipped


def splat(rays, depth, features, grid, radius, footprint, top=None, band=0, center=CENTER, rng=RANGE, acc=None):
    """features (R, E) float32, top an (H, W) array of ints or None, band = band_q in quanta.
    -> (acc (H, W, 2 + E) object array of Python ints, [bad points, bad features, culled]); acc = an earlier result, continued."""
    _, _, _, W, H = grid
    features = np.asarray(features, dtype=np.float32).reshape(len(rays), -1)
    E = features.shape[1]
    if acc is None:
        a, counters = np.zeros((H, W, 2 + E), dtype=object), [0, 0, 0]
    else:
        a, counters = acc[0].copy(), list(acc[1])
    for cell, x in zip(_cells(rays, depth, grid, radius, center, rng), features):
        if cell is None:
            counters[0] += 1
            continue
        x = x.astype(np.float64)
        if not all(np.isfinite(v) and abs(v) < XMAX for v in x):
            counters[1] += 1
            continue
        if not cell:
            continue
        f = [int(np.rint(v * FIX_X)) for v in x]
        i, j, q = cell
        for row, col in _footprint(i, j, W, H, radius, footprint):
            if top is not None and q + band < int(top[row, col]):
                counters[2] += 1
                continue
            a[row, col, 0] += q
            a[row, col, 1] += 1
            for e in range(E):
                a[row, col, 2 + e] += f[e]
    return a, counters


def resolve(acc):
    """-> maps (E, H, W) float32, dsm (H, W) float32, count (H, W) int32."""
    H, W, S = acc.shape
    maps = np.full((S - 2, H, W), np.nan, dtype=np.float32)
    dsm = np.full((H, W), np.nan, dtype=np.float32)
    cnt = np.zeros((H, W), dtype=np.int32)
    for r in range(H):
        for c in range(W):
            n = int(acc[r, c, 1])
            cnt[r, c] = min(n, 2 ** 31 - 1)
            if n:
                dsm[r, c] = np.float32(np.float64(int(acc[r, c, 0])) / np.float64(n) * (1.0 / D.FIX))
                for e in range(S - 2):
                    maps[e, r, c] = np.float32(np.float64(int(acc[r, c, 2 + e])) / np.float64(n) * (1.0 / FIX_X))
    return maps, dsm, cnt


def as_int64(a):
    return np.array(a.tolist(), dtype=np.int64).reshape(a.shape)


def statement(rays, depth, features, grid, radius, footprint, mode="mean", band=0.0, center=CENTER, rng=RANGE):
    """Both passes and the resolve on one set of rays -> dict top (int64 or None), acc (int64), counters, top_skipped, maps, dsm, count."""
    top, top_skipped = (None, 0)
    if mode == "top":
        top, top_skipped = top_pass(rays, depth, grid, radius, footprint, center, rng)
    acc, counters = splat(rays, depth, features, grid, radius, footprint, top, band_q(band), center, rng)
    maps, dsm, count = resolve(acc)
    return {"top": None if top is None else as_int64(top), "acc": as_int64(acc), "counters": counters, "top_skipped": top_skipped,
            "maps": maps, "dsm": dsm, "count": count}


# ------------------------------------------------------------------------------------------------------------------ features
def features_for(R, E, seed):
    """(R, E) float32: values of both signs up to +-300, with -0.0, denormals, the largest accepted magnitude and exact dyadics
    sprinkled in."""
    g = np.random.RandomState(seed)
    x = (g.standard_normal((R, E)) * g.choice([1e-3, 1.0, 300.0], size=(R, E))).astype(np.float32)
    special = np.array([-0.0, 1e-42, -1e-42, np.nextafter(np.float32(XMAX), np.float32(0)), -np.nextafter(np.float32(XMAX), np.float32(0)),
                        0.5, -0.375, 2.0 ** -25, 3 * 2.0 ** -25], dtype=np.float32)
    flat = x.reshape(-1)
    if flat.size:
        at = g.permutation(flat.size)[:min(flat.size, len(special))]
        flat[at] = special[:len(at)]
    return x


# ---------------------------------------------------------------------------------------------------------------- the sweep
# grids: one cell; 9 x 7 cells of 0.5 m; 65 x 33 cells of 0.3 m (a resolution that is no power of two).  (xoff, yoff, res, W, H)
GRIDS = {"1x1": (CENTER[0] - 1.0, CENTER[1] + 1.0, 2.0, 1, 1), "7x9": (CENTER[0] - 2.5, CENTER[1] + 2.0, 0.5, 9, 7),
         "33x65": (CENTER[0] - 9.0, CENTER[1] + 5.0, 0.3, 65, 33)}
# Every R in {1, 63, 64, 65, 257}, E in {0, 1, 3, 16, 17, 32}, grid, radius in {0, 1, 2, 4} and footprint of the sweep appears, and
# each value of one axis meets at least two values of every other: (R, E, grid, radius, footprint, mode).  The full product (720
# cases) would cost minutes of Python statement for no further path of the kernel.
SWEEP = [(1, 0, "1x1", 0, "disc", "mean"), (1, 32, "7x9", 4, "square", "top"), (63, 1, "7x9", 1, "disc", "top"),
         (63, 17, "33x65", 2, "square", "mean"), (64, 3, "33x65", 0, "square", "top"), (64, 16, "1x1", 4, "disc", "mean"),
         (65, 32, "33x65", 1, "disc", "mean"), (65, 0, "7x9", 2, "disc", "top"), (257, 3, "7x9", 2, "disc", "mean"),
         (257, 17, "33x65", 4, "disc", "top"), (257, 1, "1x1", 1, "square", "top"), (65, 16, "7x9", 0, "disc", "top"),
         (63, 32, "1x1", 2, "square", "top"), (64, 17, "7x9", 1, "square", "mean"), (257, 16, "33x65", 1, "square", "top"),
         (1, 3, "33x65", 4, "disc", "mean"), (65, 1, "33x65", 0, "disc", "mean"), (64, 0, "33x65", 2, "square", "top")]
SWEEP_BAND = 1.5


def sweep_id(c):
    return "R%d_E%d_%s_r%d_%s_%s" % c


@functools.lru_cache(maxsize=None)
def sweep_case(c):
    """-> (grid, rays (R, 8), depth (R,), features (R, E)): dsm_cases' mixed rows (edge points, rows to skip, random oblique rays)."""
    R, E, gname, radius, footprint, mode = c
    grid = GRIDS[gname]
    rays, depth = D._mixed(max(R, 40), 11 + R + E, grid)
    if R < 40:                                                            # a single ray is one that deposits
        keep = np.nonzero(np.isfinite(depth) & (np.abs(depth) < 10))[0][:R]
        rays, depth = np.ascontiguousarray(rays[keep]), np.ascontiguousarray(depth[keep])
    feats = features_for(R, E, 5 + R + E)
    for a in (rays, depth, feats):
        a.setflags(write=False)
    return grid, rays, depth, feats


@functools.lru_cache(maxsize=None)
def sweep_expected(c):
    R, E, gname, radius, footprint, mode = c
    grid, rays, depth, feats = sweep_case(c)
    return statement(rays, depth, feats, grid, radius, footprint, mode, SWEEP_BAND)


# ------------------------------------------------------------------------------------------------------------- crafted cases
def contention_case():
    """300 rays on a 3 x 3 grid of 0.5 m cells, radius 1: every cell takes deposits from most rays."""
    grid = (CENTER[0] - 0.75, CENTER[1] + 0.75, 0.5, 3, 3)
    g = np.random.RandomState(21)
    n = 300
    rays, depth = D._nadir(np.zeros(n), np.zeros(n), np.zeros(n), 0.5)
    rays[:, 0] = g.uniform(-0.7, 0.7, n) / RANGE
    rays[:, 1] = g.uniform(-0.7, 0.7, n) / RANGE
    rays[:, 2] += g.uniform(-4.0, 1.0, n).astype(np.float32)          # altitudes of both signs around 12.5 - 24 .. 12.5 + 6
    return grid, rays, depth, features_for(n, 5, 22)


def outside_case():
    """Centre cells one column west / one row north of SMALL (dsm_cases' _edge_points has them) - the footprint reaches in."""
    rays, depth = D._edge_points()
    return D.SMALL, rays, depth, features_for(len(rays), 4, 23)


def boundary_case():
    """Exact nadir points in ONE cell of SMALL (row 1, column 3: x in [-1.5, -1), y in (0, 0.5]) at 14 m (twice), 13.625 m and
    13.25 m, and the band 0.375 m: q + band_q == top exactly for the 13.625 m point, which is kept; the 13.25 m point is culled.
    Offsets are multiples of 1.5 / 2^k metres, so every point and every q is exact."""
    x = np.array([-1.125, -1.3125, -1.125, -1.21875])
    y = np.array([0.375, 0.1875, 0.28125, 0.375])
    z = np.array([1.5, 1.5, 1.125, 0.75])
    rays, depth = D._nadir(x, y, z, 0.5)
    feats = np.array([[0.5, 1.0], [0.25, 2.0], [-0.75, 4.0], [100.0, 8.0]], dtype=np.float32)
    return D.SMALL, rays, depth, feats, 0.375


# ------------------------------------------------------------------------------------------------------------ the block scene
# A block of 4 x 4 m with a flat roof at 30 m on ground at 10 m, seen 30 degrees off nadir from the west, on 0.5 m cells: the
# camera sees the ground (but for the block's shadow east of it), the roof and the west facade.  One ray per visible surface
# sample: the ground and the roof at cell centres, the facade 0.875 m apart in height in the middle of the column west of the
# roof.  o = P - d t with t = 2 (normalised), rounded to fp32: the point the chain recovers is P within 4e-6 m, far from any cell
# edge and from the band's edge.  Colours are dyadic per surface, so every sum and every single-surface mean is exact.
BLOCK_GRID = (CENTER[0] - 6.0, CENTER[1] + 4.5, 0.5, 32, 18)          # x in [-6, 10), y in (-4.5, 4.5] metres around the centre
BLOCK_COLOURS = {"ground": (0.125, 0.375, 0.625), "roof": (0.5, 0.25, 0.125), "facade": (0.75, 0.5, 0.25)}
BLOCK_BAND = 1.0
ROOF_COLS, ROOF_ROWS, FACADE_COL = range(14, 22), range(5, 13), 13    # the roof's cells; the facade's column


@functools.lru_cache(maxsize=None)
def block_scene():
    """-> dict rays (R, 8), depth (R,), features (R, 3), surface (R,) of names, grid, and the statement in mean and top mode."""
    xoff, yoff, res, W, H = BLOCK_GRID
    off = 30.0 * np.pi / 180.0
    d = np.array([np.sin(off), 0.0, -np.cos(off)])
    shadow = 20.0 * np.tan(off)                                           # the ground the block hides, east of it
    P, surf = [], []
    for j in range(H):
        for i in range(W):
            x, y = xoff + (i + 0.5) * res, yoff - (j + 0.5) * res
            on_roof = i in ROOF_COLS and j in ROOF_ROWS
            hidden = j in ROOF_ROWS and ROOF_COLS[-1] < i and x < xoff + (ROOF_COLS[-1] + 1) * res + shadow
            if on_roof:
                P.append((x, y, 30.0)); surf.append("roof")
            elif not hidden:
                P.append((x, y, 10.0)); surf.append("ground")
    for j in ROOF_ROWS:
        for k in range(22):                                               # 10.5 .. 28.875 m: below the band under the roof
            P.append((xoff + (FACADE_COL + 0.5) * res, yoff - (j + 0.5) * res, 10.5 + 0.875 * k)); surf.append("facade")
    P = np.array(P)
    t = 2.0
    d32 = d.astype(np.float32)
    rays = np.zeros((len(P), 8), dtype=np.float32)
    rays[:, 3:6] = d32
    rays[:, 0:3] = ((P - np.array(CENTER)) / RANGE - d32.astype(np.float64) * t).astype(np.float32)
    rays[:, 7] = 4.0
    depth = np.full((len(P),), t, dtype=np.float32)
    feats = np.array([BLOCK_COLOURS[s] for s in surf], dtype=np.float32)
    perm = np.random.RandomState(31).permutation(len(P))                  # the surfaces are not sorted along the rays
    rays, depth, feats, surf, P = rays[perm], depth[perm], feats[perm], np.array(surf)[perm], P[perm]
    assert np.abs(D.points(rays, depth) - P).max() < 4e-6
    mean = statement(rays, depth, feats, BLOCK_GRID, 1, "disc", "mean")
    top = statement(rays, depth, feats, BLOCK_GRID, 1, "disc", "top", BLOCK_BAND)
    for a in (rays, depth, feats):
        a.setflags(write=False)
    return {"rays": rays, "depth": depth, "features": feats, "surface": surf, "grid": BLOCK_GRID, "mean": mean, "top": top}


def block_conditions():
    """The conditions on the scene that the tests rest on, as numbers: cells where mean and top mode differ, roof cells that are
    not exactly the roof colour in top mode, cells whose highest point comes in through a neighbour's footprint only."""
    s = block_scene()
    mean, top = s["mean"], s["top"]
    differ = int(((mean["maps"].view(np.int32) != top["maps"].view(np.int32)).any(0)).sum())
    roof = np.array(BLOCK_COLOURS["roof"], dtype=np.float32)
    off_colour = sum(1 for j in ROOF_ROWS for i in ROOF_COLS if not np.array_equal(top["maps"][:, j, i], roof))
    # the highest q among the points whose CENTRE cell this is, against the top the footprints brought
    xoff, yoff, res, W, H = BLOCK_GRID
    own = np.full((H, W), EMPTY, dtype=object)
    for cell in _cells(s["rays"], s["depth"], BLOCK_GRID, 1, CENTER, RANGE):
        i, j, q = cell
        if 0 <= i < W and 0 <= j < H:
            own[j, i] = max(own[j, i], q)
    neighbour_only = int(sum(1 for j in range(H) for i in range(W) if own[j, i] != EMPTY and int(top["top"][j, i]) > own[j, i] + band_q(BLOCK_BAND)))
    return {"differ": differ, "roof_off_colour": off_colour, "neighbour_only": neighbour_only, "culled": top["counters"][2]}


BLOCK_CONDITIONS = block_conditions()
assert BLOCK_CONDITIONS["differ"] >= 20 and BLOCK_CONDITIONS["roof_off_colour"] == 0 and BLOCK_CONDITIONS["neighbour_only"] >= 5, BLOCK_CONDITIONS
