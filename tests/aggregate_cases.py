"""The numpy statement of the semi-global aggregation of a cost volume (include/brdfnerf_hip.h, "Semi-global aggregation of a cost
volume") and its cases.

quanta, paths and pick are the rule's three steps: plain Python loops over direction, row and column with one array expression over
the levels per step, in int64, and nothing of waves, lanes, tiles or blocks in them.  Nothing here is shared with
brdf_nerf_amd/aggregate.py or the kernels.  The scene fixture is the sweep's box scene with noise on its three images.
"""
import numpy as np

import mosaic_cases as M
import sweep_cases as S

QINV = 1 << 20
CAP = QINV - 1
MAX_LEVELS = 256
# (row step, column step) of bit 0 .. 7 of a direction mask
DIRECTIONS = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (-1, -1), (1, -1), (-1, 1))
PENALTIES = ((0, 0), (1, 1), (256, 2048), (0, QINV), (QINV, QINV))
MASKS = tuple(1 << b for b in range(8)) + (0x0F, 0xFF)
# (H, W, Z) of the bit-equality cases: every grid and every Z the rule names, no full product.  1 x 1, 1 x 7, 7 x 1: lines of one
# cell; 3 x 5, 2 x 130: diagonals shorter than both sides; 33 x 65: 388 lines of 8 directions, more than one block of 4 waves holds.
# Z: the lane edges of 1, 2, 3 and 4 levels per lane
SHAPES = ((1, 1, 1), (1, 1, 256), (1, 7, 2), (1, 7, 65), (7, 1, 3), (7, 1, 129), (3, 5, 1), (3, 5, 63), (3, 5, 64), (3, 5, 128),
          (3, 5, 255), (2, 130, 3), (2, 130, 65), (2, 130, 256), (33, 65, 2), (33, 65, 63), (33, 65, 64), (33, 65, 65), (33, 65, 128),
          (33, 65, 129), (33, 65, 255), (33, 65, 256))
SCENE_P1, SCENE_P2, SCENE_QUANTUM, SCENE_NOISE = 1.0, 8.0, 1.0 / 256.0, 0.005


def quanta(cost, quantum):
    """Step 1.  cost float32 (Z, H, W), NaN where a level is not valid -> int32 (H, W, Z), counters [cells, pairs, capped]."""
    cost = np.asarray(cost, np.float32)
    assert cost.ndim == 3 and quantum > 0
    c = np.moveaxis(cost, 0, -1)
    known = ~np.isnan(c)
    with np.errstate(all="ignore"):
        t = c.astype(np.float64) / np.float64(quantum)                       # one float64 division
    t = np.where(known, t, 0.0)
    q = np.where(t >= CAP, float(CAP), np.where(t <= 0.0, 0.0, np.rint(np.clip(t, 0.0, float(CAP))))).astype(np.int64)
    q = np.where(known, q, QINV)
    q = np.where(known.any(-1, keepdims=True), q, -1)
    return np.ascontiguousarray(q, np.int32), [int(known.any(-1).sum()), int(known.sum()), int((known & (t >= CAP)).sum())]


def line_costs(q, P1, P2, direction):
    """L_r of one direction over the grid: int64 (H, W, Z)."""
    H, W, Z = q.shape
    dj, di = direction
    c = np.maximum(np.asarray(q, np.int64), 0)
    L = np.zeros((H, W, Z), dtype=np.int64)
    for j in (range(H) if dj >= 0 else range(H - 1, -1, -1)):
        for i in (range(W) if di >= 0 else range(W - 1, -1, -1)):
            pj, pi = j - dj, i - di
            if not (0 <= pj < H and 0 <= pi < W):
                L[j, i] = c[j, i]
                continue
            prev = L[pj, pi]
            m = prev.min()
            best = np.minimum(prev, m + P2)
            best[1:] = np.minimum(best[1:], prev[:-1] + P1)
            best[:-1] = np.minimum(best[:-1], prev[1:] + P1)
            L[j, i] = c[j, i] + best - m
    return L


def paths(q, P1, P2, mask=0xFF):
    """Step 2 from a zeroed sum: int32 (H, W, Z), the sum of L_r over the directions of the mask."""
    assert 0 <= P1 <= P2 <= QINV and 1 <= mask <= 0xFF
    total = np.zeros(q.shape, dtype=np.int64)
    for b, direction in enumerate(DIRECTIONS):
        if mask >> b & 1:
            total += line_costs(q, P1, P2, direction)
    assert total.max() <= 8 * 2 * QINV
    return total.astype(np.int32)


def pick(q, total, strict=True):
    """Step 3.  strict=False: the `<=` comparison the rule does NOT use (the last level keeps a tie).
    -> {"level", "sum_min" int32 (H, W), "wins" Z ints, "sums" [cells, sum of sum_min]}."""
    H, W, Z = q.shape
    level = np.full((H, W), -1, dtype=np.int32)
    best = np.zeros((H, W), dtype=np.int64)
    for d in range(Z):
        ok = (q[..., d] >= 0) & (q[..., d] < QINV)
        s = total[..., d].astype(np.int64)
        take = ok & ((level < 0) | ((s < best) if strict else (s <= best)))
        level, best = np.where(take, np.int32(d), level), np.where(take, s, best)
    has = level >= 0
    return {"level": level.astype(np.int32), "sum_min": np.where(has, best, -1).astype(np.int32),
            "wins": np.bincount(level[has], minlength=Z).tolist(), "sums": [int(has.sum()), int(best[has].sum())]}


def aggregate(cost, quantum, P1, P2, mask=0xFF, strict=True):
    """The three steps -> pick's dictionary with "quanta", "sum" (H, W, Z) and "counters"."""
    q, counters = quanta(cost, quantum)
    total = paths(q, P1, P2, mask)
    return dict(pick(q, total, strict), quanta=q, sum=total, counters=counters)


def random_volume(Z, H, W, seed=0, quantum=0.25):
    """A volume with every special the rule names: NaN levels, all-NaN cells, +-inf, negatives, -0.0, denormals, costs at and above
    the cap, and exact half-quantum values (ties of the rounding)."""
    rng = np.random.default_rng(seed + 1000 * Z + 10 * H + W)
    cost = (rng.integers(0, 4000, (Z, H, W)) * (quantum / 8)).astype(np.float32)          # eighths of a quantum: halves among them
    n = cost.size
    flat = cost.reshape(-1)
    specials = np.array([np.nan, np.inf, -np.inf, -3.5, -0.0, 1e-42, CAP * quantum, (CAP + 0.5) * quantum, (CAP - 0.5) * quantum,
                         QINV * quantum, 3e38, 0.5 * quantum, 1.5 * quantum, 2.5 * quantum], dtype=np.float32)
    at = rng.permutation(n)[:max(1, n // 6)]
    flat[at] = specials[rng.integers(0, len(specials), len(at))]
    flat[rng.permutation(n)[:n // 8]] = np.nan
    cells = rng.random((H, W)) < 0.08
    cost[:, cells] = np.nan
    return cost


def noisy_scene():
    """The sweep's scene with noise of SCENE_NOISE of the value range on every image, the box 6 m too high: -> the cost volume
    float32 (17, 48, 40) of the sweep's statement, the true DSM (for scene_counts)."""
    ds, planes, dsm, xoff, yoff, res, zone = S.scene()
    rng = np.random.default_rng(7)
    noisy = [(p + rng.normal(0, SCENE_NOISE * float(p.max() - p.min()), p.shape)).astype(np.float32) for p in planes]
    return S.sweep(ds, noisy, M.raised(dsm), xoff, yoff, res, zone, S.SCENE_OFFSETS)["cost"], dsm


def wta_level(cost):
    """The per-cell pick of the sweep from its volume: the first level of the smallest cost, -1 where every level is NaN."""
    cost = np.asarray(cost)
    known = ~np.isnan(cost)
    return np.where(known.any(0), np.argmin(np.where(known, cost, np.inf), 0), -1).astype(np.int32)


# the noisy scene under SCENE_P1, SCENE_P2, SCENE_QUANTUM (P1 = 256, P2 = 2048): roof cells at -6 m of 100, ground cells not at 0 m of
# 1599, recorded from the statement.  1699 cells have a result, 221 none; 28883 valid pairs, the largest quantum 57895, none capped
SCENE_RECORD = {"wta": {"roof": 57, "astray": 885}, "cells": 1699, "none": 221, "valid_pairs": 28883, "capped": 0, "max_quantum": 57895,
                8: {"roof": 73, "astray": 118, "wins": [0, 4, 73, 8, 3, 5, 7, 104, 1481, 14, 0, 0, 0, 0, 0, 0, 0], "sum_total": 1915547,
                    "max_sum": 479544},
                4: {"roof": 75, "astray": 131, "wins": [0, 4, 75, 8, 3, 3, 5, 102, 1468, 31, 0, 0, 0, 0, 0, 0, 0], "sum_total": 864752,
                    "max_sum": 239772}}
