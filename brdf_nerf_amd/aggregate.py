"""Semi-global aggregation of the altitude sweep's cost volume on the device: a surface from the volume, not from cell-wise minima.

altitude_sweep picks every cell's level on its own - the level whose photo-consistency cost is smallest - and the variance of a
few samples is a weak cue: with noise of 0.5 % of the value range on the three images of the test scene, 885 of 1599 ground cells
leave 0 m.  Semi-global matching over the levels adds, per cell and level, the minimum-cost paths that reach the cell from 4 or 8
directions, with a small penalty p1 for a change of one level between neighbouring cells and a larger p2 for a jump, and picks the
level of the smallest sum: 118 cells leave 0 m.

  aggregate_costs   bn_cost_quanta ((Z, H, W) float32 -> integer quanta [H][W][Z]), bn_cost_paths (one wave per line and direction,
                    all lines of all directions in one launch, added into `sum` by integer atomics), bn_cost_pick (the first valid
                    level of the smallest sum)

The rule (include/brdfnerf_hip.h, "Semi-global aggregation of a cost volume").  A non-NaN cost c becomes q = rint((double)c / quantum),
clamped to [0, 2^20 - 1]; a NaN level of a cell with a result 2^20, which never wins; a cell without a result is neutral (cost 0 at
every level) and gets level -1.  Along direction r, L_r(p, d) = c(p, d) + min(L_r(p - r, d), L_r(p - r, d +- 1) + P1, min_k L_r(p - r,
k) + P2) - min_k L_r(p - r, k), and L_r = c on the border the path starts from.  Everything after the quanta is int32, so every bit
depends on the inputs alone: not on blocks, not on how the directions are split over launches or ranks (under a group rank i runs the
directions whose bit index is i modulo the world; one SUM all-reduce of `sum` merges them; every rank picks).

Refused by name (ValueError, before any launch): a cost volume that is not a 3-D float32 tensor on the device, with 1 to 256 levels
and fewer than 2^31 elements; p1 < 0, p2 < p1, or penalties that are not finite; a quantum that is not finite and positive, or
missing while p1 is 0; penalties of more than 2^20 quanta; paths other than 4 or 8.

Not covered: an adaptive p2 from image gradients, more than 8 paths, sub-level refinement, a left-right style consistency check,
uint16 quanta.
"""
import math
import numbers

import torch

from . import functions as Fn
from .distributed import allreduce_, world_info

PATH_MASKS = {4: 0x0F, 8: 0xFF}


def penalties(name, p1, p2, quantum):
    """p1, p2 in cost units and the quantum (None: p1 / 256) -> quantum, P1, P2 with P = llrint(p / quantum), or ValueError by name."""
    for what, v in (("p1", p1), ("p2", p2)) + ((("quantum", quantum),) if quantum is not None else ()):
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v):
            raise ValueError(f"{name}: {what} {v!r} is not a finite number")
    p1, p2 = float(p1), float(p2)
    if not 0.0 <= p1 <= p2:
        raise ValueError(f"{name}: penalties p1={p1}, p2={p2} (0 <= p1 <= p2)")
    if quantum is None:
        if p1 == 0.0:
            raise ValueError(f"{name}: with p1 = 0 a quantum must be given")
        quantum = p1 / 256.0
    quantum = float(quantum)
    if not quantum > 0.0:
        raise ValueError(f"{name}: quantum {quantum!r} must be finite and positive")
    scaled = (p1 / quantum, p2 / quantum)
    if not all(s <= Fn.L.BN_AGG_QINV for s in scaled):
        raise ValueError(f"{name}: penalties p1={p1}, p2={p2} are more than 2^20 quanta of {quantum}")
    P1, P2 = (int(round(s)) for s in scaled)                 # round(): ties to even, as llrint
    return quantum, P1, P2


def path_mask(name, paths):
    if isinstance(paths, bool) or paths not in PATH_MASKS:
        raise ValueError(f"{name}: paths {paths!r} (4 or 8)")
    return PATH_MASKS[paths]


@torch.no_grad()
def aggregate_costs(cost, p1, p2, quantum=None, paths=8, group=None, want_sum=False):
    """cost (Z, H, W) float32 on the device, NaN where a level is not valid at a cell - altitude_sweep(want_cost=True)["cost"]; p1 <= p2:
    the penalties of a change of one level and of a jump, in cost units; quantum: the cost of one integer quantum (None: p1 / 256);
    paths: 4 (along rows and columns) or 8 (and diagonals); group: the ranks that share the directions.
    -> {"level" (H, W) int32, -1 where no level is valid, "sum_min" (H, W) int32, the smallest sum, -1 there, "sum" (Z, H, W) int32 with
    want_sum, else None, "wins": Z integers, the cells per level, "cells": the cells with a result - those with a level -, "sum_total": the sum of sum_min,
    "valid_pairs", "capped": the non-NaN (cell, level) pairs and those at or above the cap of 2^20 - 1 quanta, "quantum", "P1", "P2"}."""
    name = "aggregate_costs"
    if not isinstance(cost, torch.Tensor) or cost.dim() != 3:
        raise ValueError(f"{name}: cost must be a 3-D tensor (Z, H, W) on the device")
    quantum, P1, P2 = penalties(name, p1, p2, quantum)
    mask = path_mask(name, paths)
    Fn._need(name, cost, "cost", Fn.F32, ("Z", "H", "W"))
    rank, world = world_info(group)
    quanta, counters = Fn.cost_quanta(cost, quantum)
    mine = sum(1 << b for b in range(8) if mask >> b & 1 and b % world == rank)
    total = torch.zeros_like(quanta)
    if mine:
        Fn.cost_paths(quanta, P1, P2, mine, total)
    if world > 1:
        allreduce_(total, None, group)
    out = Fn.cost_pick(quanta, total)
    cells, valid_pairs, capped = counters.tolist()
    return {"level": out["level"], "sum_min": out["sum_min"], "sum": total.permute(2, 0, 1).contiguous() if want_sum else None,
            "wins": out["wins"].tolist(), "cells": cells, "sum_total": out["sums"].tolist()[1], "valid_pairs": valid_pairs,
            "capped": capped, "quantum": quantum, "P1": P1, "P2": P2}


__all__ = ["aggregate_costs"]
