"""The statement the hole filling (brdf_nerf_amd/fill.py, bn_grid_nearest_col / bn_grid_fill) is held to, and its cases.

statement(u)     the rule of include/brdfnerf_hip.h as a brute force in numpy int64: for every hole the argmin of
                 d2 (H W) + flat index over ALL known cells.  It shares no structure with the two-pass kernels.
two_pass(u)      a numpy restatement of the decomposition: the column pass (nearest known row per column, ties to the smaller
                 row), then the row pass over every column WITHOUT the early stop.  test_fill_cpu.py proves it equal to the
                 brute force on every case; the GPU test holds near_row to its first half.
against_reference  what can be compared with scipy's griddata on a golden: bit-equality where the nearest known cell is
                 unique, membership among the known cells at the minimal d2 on a tie.
"""
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDENS = ("holes5", "holes30", "sparse90")
ROW_BLOCK = 256                                  # the row pass's block size: cells of a row are taken in strides of it


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def statement(u, chunk=512):
    """-> filled float32 (H, W), source int32 flat indices, dist2 int32.  A grid without a known cell: filled = u, -1, -1."""
    u = np.ascontiguousarray(u, dtype=np.float32)
    H, W = u.shape
    hole = np.isnan(u)
    flat = np.arange(H * W, dtype=np.int64).reshape(H, W)
    source, dist2 = flat.copy(), np.zeros((H, W), dtype=np.int64)
    kj, ki = np.nonzero(~hole)
    if kj.size == 0:
        return u.copy(), np.full((H, W), -1, np.int32), np.full((H, W), -1, np.int32)
    kflat = kj.astype(np.int64) * W + ki
    hj, hi = np.nonzero(hole)
    for s in range(0, hj.size, chunk):
        j, i = hj[s:s + chunk, None].astype(np.int64), hi[s:s + chunk, None].astype(np.int64)
        d2 = (j - kj[None]) ** 2 + (i - ki[None]) ** 2
        at = np.argmin(d2 * (H * W) + kflat[None], axis=1)
        source[hj[s:s + chunk], hi[s:s + chunk]] = kflat[at]
        dist2[hj[s:s + chunk], hi[s:s + chunk]] = d2[np.arange(at.size), at]
    filled = u.reshape(-1).view(np.int32)[source].view(np.float32)          # the bits, not the values
    return filled, source.astype(np.int32), dist2.astype(np.int32)


def near_rows(u):
    """The column pass: near_row[j][i] = the row j' of the known cell of column i minimising (|j - j'|, j'), -1 without one."""
    u = np.asarray(u, dtype=np.float32)
    H, W = u.shape
    out = np.full((H, W), -1, dtype=np.int32)
    for i in range(W):
        known = np.nonzero(~np.isnan(u[:, i]))[0]
        if known.size:
            j = np.arange(H)[:, None]
            out[:, i] = known[np.argmin(np.abs(j - known[None]) * H + known[None], axis=1)]
    return out


def two_pass(u):
    """The row pass over near_rows(u), every column scanned: the minimum of (dx^2 + dy^2, near_row[j][i'], i')."""
    u = np.ascontiguousarray(u, dtype=np.float32)
    H, W = u.shape
    nr = near_rows(u).astype(np.int64)
    source, dist2 = np.full((H, W), -1, np.int64), np.full((H, W), -1, np.int64)
    cols = np.arange(W, dtype=np.int64)
    for j in range(H):
        ok = nr[j] >= 0
        if not ok.any():
            continue
        d2 = (cols[:, None] - cols[None, ok]) ** 2 + ((j - nr[j, ok]) ** 2)[None]
        key = (d2 * H + nr[j, ok][None]) * W + cols[None, ok]
        at = np.argmin(key, axis=1)
        source[j] = nr[j, ok][at] * W + cols[ok][at]
        dist2[j] = d2[np.arange(W), at]
    if (source < 0).any():
        return u.copy(), source.astype(np.int32), dist2.astype(np.int32)
    filled = u.reshape(-1).view(np.int32)[source].view(np.float32)
    return filled, source.astype(np.int32), dist2.astype(np.int32)


def counts(u):
    """(holes, largest d2) of the statement."""
    return int(np.isnan(u).sum()), int(statement(u)[2].max())


# ------------------------------------------------------------------------------------------------------------ cases
def _values(H, W, seed):
    return np.random.default_rng(seed).uniform(-50.0, 150.0, (H, W)).astype(np.float32)


def _random(H, W, frac, seed):
    u = _values(H, W, seed)
    u[np.random.default_rng(seed + 1000).random((H, W)) < frac] = np.nan
    if np.isnan(u).all():
        u[H // 2, W // 2] = 1.0
    return u


def _special():
    """-0.0, denormals, +-inf as known cells and two different NaN payloads among the holes."""
    u = _random(7, 9, 0.4, 77)
    u[0, 0], u[0, 8], u[6, 0], u[3, 4], u[6, 8] = -0.0, np.float32(1e-42), np.inf, -np.inf, np.float32(-1e-45)
    raw = u.view(np.uint32)
    raw[1, 1], raw[5, 7], raw[2, 6] = 0x7FC00001, 0xFFC12345, 0x7F800001     # quiet, negative quiet and signalling payloads
    return u


def _build():
    nan = np.nan
    c = {}
    c["1x1"] = np.array([[3.5]], np.float32)
    c["1x7_ends"] = np.array([[nan, nan, 1.0, 2.0, nan, 3.0, nan]], np.float32)
    c["7x1_ends"] = c["1x7_ends"].T.copy()
    c["5x6_all_known"] = _values(5, 6, 1)
    for name, (j, i) in {"nw": (0, 0), "ne": (0, 10), "sw": (8, 0), "se": (8, 10)}.items():
        u = np.full((9, 11), nan, np.float32)
        u[j, i] = 7.25
        c[f"9x11_corner_{name}"] = u
    u = _random(12, 14, 0.3, 2)
    u[:, [0, 5, 6, 13]] = nan
    c["12x14_empty_columns"] = u
    u = _random(12, 14, 0.3, 3)
    u[[0, 4, 5, 11], :] = nan
    c["12x14_empty_rows"] = u
    c["33x65"] = _random(33, 65, 0.5, 4)
    c["31x257"] = _random(31, 257, 0.7, 5)
    c["3x300"] = _random(3, 300, 0.9, 6)
    for W in (ROW_BLOCK - 1, ROW_BLOCK, ROW_BLOCK + 1, 2 * ROW_BLOCK - 1, 2 * ROW_BLOCK, 2 * ROW_BLOCK + 1):
        c[f"2x{W}"] = _random(2, W, 0.8, 100 + W)
    u = np.full((40, 600), nan, np.float32)
    u[:, 598:] = _values(40, 2, 7)
    u[np.random.default_rng(8).random((40, 600)) < 0.5] = nan
    u[3, 599] = 1.0
    c["40x600_last_two_columns"] = u
    for parity in (0, 1):
        u = _values(10, 13, 9 + parity)
        jj, ii = np.meshgrid(np.arange(10), np.arange(13), indexing="ij")
        u[(jj + ii) % 2 == parity] = nan
        c[f"10x13_checkerboard_{parity}"] = u
    c["7x9_special_values"] = _special()
    return c


CASES = _build()
ALL_NAN = np.full((4, 6), np.nan, np.float32)


def patterns_3x3():
    """Every one of the 511 non-empty known / hole patterns of a 3 x 3 grid, nine distinct values: all tie orientations."""
    base = np.arange(1.0, 10.0, dtype=np.float32).reshape(3, 3)
    out = []
    for m in range(1, 512):
        u = base.copy()
        u.reshape(-1)[[(m >> b) & 1 == 0 for b in range(9)]] = np.nan
        out.append(u)
    return out


def patterns_4x5(n=200, seed=21):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        u = np.arange(1.0, 21.0, dtype=np.float32).reshape(4, 5)
        u[rng.random((4, 5)) < rng.uniform(0.2, 0.9)] = np.nan
        if np.isnan(u).all():
            u[rng.integers(4), rng.integers(5)] = 1.0
        out.append(u)
    return out


def tie_pair():
    """Known at (2, 1) and (1, 2), hole at (1, 1): both at d2 = 1, the answer is (1, 2), the lower row-major index."""
    u = np.full((3, 3), np.nan, np.float32)
    u[2, 1], u[1, 2] = 21.0, 12.0
    return u


# ------------------------------------------------------------------------------------------------------------ goldens
def golden(name):
    with np.load(os.path.join(GOLDEN_DIR, f"fill_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def unique_and_ties(u, chunk=512):
    """Per hole: how many known cells lie at the minimal d2.  -> (hole rows, hole columns, multiplicity)."""
    u = np.asarray(u, np.float32)
    kj, ki = np.nonzero(~np.isnan(u))
    hj, hi = np.nonzero(np.isnan(u))
    mult = np.zeros(hj.size, dtype=np.int64)
    for s in range(0, hj.size, chunk):
        d2 = (hj[s:s + chunk, None].astype(np.int64) - kj[None]) ** 2 + (hi[s:s + chunk, None].astype(np.int64) - ki[None]) ** 2
        mult[s:s + chunk] = (d2 == d2.min(axis=1, keepdims=True)).sum(axis=1)
    return hj, hi, mult


def against_reference(u, filled, dist2, ref):
    """The comparison with upstream's output `ref` on the grid u: known cells unchanged on both sides; every hole with a unique
    nearest known cell bit-equal; on every other hole the reference's value is the value of a known cell at the rule's d2.
    -> (unique-nearest holes, tie holes); AssertionError otherwise."""
    u, ref = np.asarray(u, np.float32), np.asarray(ref, np.float32)
    known = ~np.isnan(u)
    assert ref.dtype == np.float32 and ref.shape == u.shape and not np.isnan(ref).any() and not np.isnan(filled).any()
    assert np.array_equal(bits(ref)[known], bits(u)[known]) and np.array_equal(bits(filled)[known], bits(u)[known])
    hj, hi, mult = unique_and_ties(u)
    one = mult == 1
    assert np.array_equal(bits(filled)[hj[one], hi[one]], bits(ref)[hj[one], hi[one]])
    kj, ki = np.nonzero(known)
    for j, i in zip(hj[~one], hi[~one]):
        at = (j - kj) ** 2 + (i - ki) ** 2 == dist2[j, i]
        assert bits(ref)[j, i] in bits(u)[kj[at], ki[at]], (j, i)
    return int(one.sum()), int((~one).sum())
