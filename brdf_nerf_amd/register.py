"""The xy registration of a DSM on its ground truth, on the device and bitwise reproducible: the reference's real altitude line.

dsm.altitude_mae is the branch the reference takes only when `import dsmr` fails (sat_utils.py:228-237).  dsmr.py ships with the
reference, so what it reports comes from sat_utils.py:239-246: dsmr.compute_shift(gt, pred, scaling=False) finds the integer
cell shift (dx, dy) that maximises the normalised cross-correlation, coarse to fine over a 2x pyramid, and the z offset b;
dsmr.apply_shift writes the registered DSM; mae and mae_nr are computed from THAT.  Here (u the ground truth, v the prediction):

  register_xy          the pyramid (bn_grid_halve), per level the integer moments of the (2 irange + 1)^2 shifts around the
                       start (bn_ncc_moments), and the argmax on the host in Python integers -> dx, dy, b
  apply_registration   rdsm = pred shifted by (dx, dy) cells and b metres, diff = rdsm - gt in float32, the MAEs (bn_dsm_shift_diff)
  altitude_mae_xy      the reference's line: mask the prediction, register, apply

The rule.  Upstream's correlation is a float64 sum over every cell in row-major order, which no parallel sum reproduces, so the
moments are integers.  pivot = floor(min finite cell of u and v), top = ceil(max), span = max(top - pivot, 1); k is the largest
integer in [0, 16] with span 2^k <= 2^20 (a span above 2^20 m is refused); a finite cell's quantum is q = rint((z - pivot) 2^k),
0 <= q <= 2^20, and ONE (pivot, k), taken at level 0, serves every level (box means stay inside [min, max]).  Per shift
(N, Su, Sv, Suu, Svv, Suv) are the sums of 1, qu, qv, qu^2, qv^2, qu qv over the valid pairs, int64 (grids of more than 2^22 cells
are refused).  On the host, in Python integers: A = N Suv - Su Sv, B = N Suu - Su^2, C = N Svv - Sv^2, corr = A / sqrt(B C) if
N > 0, B > 0 and C > 0, else the shift cannot win; dy outer and dx inner, strict >, as upstream; a level where no shift can win
returns its start.  b = (Su - Sv) / (N 2^k) at the final shift of level 0, within 2^-k of upstream's float64 b.

The sums are integers, so (dx, dy, b) do not depend on the block order, on how the rows of u are split (rows=) or on how many
GPUs shared the grid: ranks merge by one SUM all-reduce of the moments per level.

Not covered: GeoTIFF I/O, scaling=True (the reference passes False), sub-cell shifts (upstream has none), LPIPS.
"""
import math

import torch

from . import _lib as L
from . import functions as Fn

MAE_FIX = 2.0 ** 20
MAX_SPAN = 1 << 20


def quantisation(lo, hi):
    """(pivot, k) for finite cells in [lo, hi]: pivot = floor(lo), span = max(ceil(hi) - pivot, 1), k the largest integer in
    [0, 16] with span 2^k <= 2^20.  ValueError when the span is above 2^20 m or a bound is not finite."""
    if not (math.isfinite(lo) and math.isfinite(hi)) or lo > hi:
        raise ValueError(f"register_xy: the altitudes' bounds [{lo}, {hi}] are not finite")
    pivot = math.floor(lo)
    span = max(math.ceil(hi) - pivot, 1)
    if span > MAX_SPAN:
        raise ValueError(f"register_xy: the altitudes span {span} m, more than 2^20")
    k = L.BN_NCC_MAX_SCALE
    while span << k > MAX_SPAN:
        k -= 1
    return pivot, k


def correlation(m):
    """The correlation of one shift from its six integer moments, or None when the shift cannot win (no pair, or a constant side)."""
    N, Su, Sv, Suu, Svv, Suv = (int(x) for x in m)
    A, B, C = N * Suv - Su * Sv, N * Suu - Su * Su, N * Svv - Sv * Sv
    if N > 0 and B > 0 and C > 0:
        return A / math.sqrt(B * C)
    return None


def best_shift(moments, dx0, dy0, r):
    """dsmr.compute_ncc's scan over the (2r + 1)^2 x 6 integers of one level: dy outer, dx inner, strict > (the first maximum
    wins), the start when no shift can win.  -> (dx, dy, index of the winner or None)."""
    best, at, side = -math.inf, None, 2 * r + 1
    for s, m in enumerate(moments):
        c = correlation(m)
        if c is not None and c > best:
            best, at = c, s
    if at is None:
        return dx0, dy0, None
    return dx0 - r + at % side, dy0 - r + at // side, at


def _grid_pair(name, dsm, gt):
    dsm, gt = torch.as_tensor(dsm), torch.as_tensor(gt)
    if dsm.dim() != 2 or dsm.shape != gt.shape:
        raise ValueError(f"{name}: dsm {tuple(dsm.shape)} and ground truth {tuple(gt.shape)} are not on one (H, W) grid")
    if dsm.numel() < 1 or dsm.numel() > L.BN_NCC_MAX_CELLS:
        raise ValueError(f"{name}: a grid of {dsm.shape[0]} x {dsm.shape[1]} cells (1 to 2^22)")
    return dsm, gt.to(dsm.device)


def _band(rows, level):
    """The rows of level `level` that come from the level-0 rows [rows[0], rows[1]): ceil(row / 2^level), so bands that
    partition level 0 partition every level."""
    s = 1 << level
    return (rows[0] + s - 1) // s, (rows[1] + s - 1) // s


@torch.no_grad()
def register_xy(dsm, gt, irange=5, min_size=100, rows=None, group=None):
    """dsmr.compute_shift(gt, dsm, scaling=False) (dsmr.py:120-135, 163-190) on the device: the integer shift (dx, dy) that
    maximises the correlation of gt[j][i] with dsm[j + dy][i + dx], +-irange cells around twice the coarser level's answer, the
    grids halved while min(H, W) > min_size; and b = mean(gt) - mean(dsm shifted) over the valid pairs.  dsm, gt: (H, W), any
    float dtype (widened to float64 exactly, as numba's typing does upstream), NaN or infinite cells missing.
    rows = (row0, row1): only those rows of gt (level 0; ceil(row / 2^l) at level l) enter the moments.  With a `group` of more
    than one rank each rank takes its band (shard_bounds, or `rows`: the bands must partition [0, H)) and one SUM all-reduce
    of the moments per level merges them: every rank returns the single-process result, bit for bit.
    -> {"dx", "dy", "b", "k", "pivot", "levels": [(H, W, dx, dy), ...] coarsest first, "moments": [(2 irange + 1)^2 x 6 int64
    host tensor per level], "skipped"}."""
    from .distributed import allreduce_, row_band
    v, u = _grid_pair("register_xy", dsm, gt)
    if not isinstance(irange, int) or not 0 <= irange <= L.BN_NCC_MAX_RANGE:
        raise ValueError(f"register_xy: irange {irange!r} outside [0, {L.BN_NCC_MAX_RANGE}]")
    if not v.is_cuda:
        raise ValueError("register_xy: the grids must be on the device (there is no host path)")
    H, W = u.shape
    rows = row_band("register_xy", H, rows, group)
    u, v = u.double().contiguous(), v.double().contiguous()
    inf = torch.full((), math.inf, dtype=torch.float64, device=u.device)
    both = torch.stack([u, v])
    ok = torch.isfinite(both)
    lo, hi = (float(x) for x in torch.stack([torch.where(ok, both, inf).min(), torch.where(ok, both, -inf).max()]).cpu())
    if lo > hi:
        raise ValueError("register_xy: neither grid has a finite cell")
    pivot, k = quantisation(lo, hi)
    pyramid = [(u, v)]
    while min(pyramid[-1][0].shape) > min_size:
        pyramid.append((Fn.grid_halve(pyramid[-1][0]), Fn.grid_halve(pyramid[-1][1])))
    dx = dy = 0
    levels, moments = [], []
    skipped = torch.zeros((1,), dtype=torch.int64, device=u.device)
    for level in range(len(pyramid) - 1, -1, -1):
        lu, lv = pyramid[level]
        dx0, dy0 = 2 * dx, 2 * dy                           # (0, 0) at the coarsest level: upstream's 0 // 2 all the way down
        sums, _ = Fn.ncc_moments(lu, lv, pivot, k, dx0, dy0, irange, skipped=skipped, rows=_band(rows, level))
        host = allreduce_(sums, group=group).cpu()
        dx, dy, at = best_shift(host.tolist(), dx0, dy0, irange)
        levels.append((lu.shape[0], lu.shape[1], dx, dy))
        moments.append(host)
    allreduce_(skipped, group=group)
    if at is None:                                          # no shift of level 0 can win: the offset of the start, if it has a pair
        at = ((2 * irange + 1) ** 2) // 2
    N, Su, Sv = (int(x) for x in moments[-1][at][:3])
    b = (Su - Sv) / (N << k) if N > 0 else float("nan")
    return {"dx": dx, "dy": dy, "b": b, "k": k, "pivot": pivot, "levels": levels, "moments": moments, "skipped": int(skipped.item())}


@torch.no_grad()
def apply_registration(dsm, gt, dx, dy, b, mask=None):
    """dsmr.apply_shift and the difference of sat_utils.py:246: rdsm[j][i] = (float)(dsm[j + dy][i + dx] + b), NaN where that cell
    is out of range, diff = rdsm - gt in float32, mae = nanmean(|diff|) (:340) from an integer sum.  mask (nonzero inside;
    MaskDoD, :344-345): also mae_in over the cells inside and mae_out over the others.
    -> {"rdsm", "diff" (H, W) float32, "mae", "sums" (6,) int64} (+ "mae_in", "mae_out")."""
    from .metrics import _mask_hw
    pred, gt = _grid_pair("apply_registration", dsm, gt)
    if not pred.is_cuda:
        raise ValueError("apply_registration: the grids must be on the device (there is no host path)")
    if not math.isfinite(b):
        raise ValueError(f"apply_registration: b = {b} is not finite")
    if max(abs(int(dx)), abs(int(dy))) > L.BN_NCC_MAX_SHIFT:
        raise ValueError(f"apply_registration: shift ({dx}, {dy}) beyond 2^20 cells")
    H, W = pred.shape
    if mask is not None and torch.as_tensor(mask).numel() != H * W:
        raise ValueError(f"apply_registration: mask of {torch.as_tensor(mask).numel()} cells for a grid of {H} x {W}")
    rdsm, diff, sums = Fn.dsm_shift_diff(Fn._f32(pred), Fn._f32(gt), dx, dy, b, _mask_hw(mask, H, W, pred.device))
    s = sums.cpu()
    mean = [Fn.fixed_mean(t, n, MAE_FIX) for t, n in s.reshape(3, 2).tolist()]              # all, inside, outside
    res = {"rdsm": rdsm, "diff": diff, "mae": mean[0], "sums": s}
    if mask is not None:
        res.update(mae_in=mean[1], mae_out=mean[2])
    return res


@torch.no_grad()
def altitude_mae_xy(dsm, gt, mask=None, irange=5, min_size=100, group=None):
    """The reference's altitude line with dsmr (sat_utils.py:211-218, 239-246, 340-349): the prediction set to NaN outside
    `mask`, registered on the ground truth in xy and z (register_xy), shifted (apply_registration).
    -> altitude_mae's keys {"mae", "shift" (= b), "diff"} (+ "mae_in", "mae_out") and "dx", "dy", "rdsm", "registration"."""
    pred, gt = _grid_pair("altitude_mae_xy", dsm, gt)
    if mask is not None:
        m = torch.as_tensor(mask).to(pred.device)
        if m.numel() != pred.numel():
            raise ValueError(f"altitude_mae_xy: mask of {m.numel()} cells for a grid of {pred.shape[0]} x {pred.shape[1]}")
        pred = torch.where(m.reshape(pred.shape) != 0, pred, torch.full_like(pred, float("nan")))
    reg = register_xy(pred, gt, irange=irange, min_size=min_size, group=group)
    if not math.isfinite(reg["b"]):
        raise ValueError("altitude_mae_xy: no cell of the prediction meets a cell of the ground truth at the shift found")
    out = apply_registration(pred, gt, reg["dx"], reg["dy"], reg["b"], mask=mask)
    res = {"mae": out["mae"], "shift": reg["b"], "diff": out["diff"], "dx": reg["dx"], "dy": reg["dy"], "rdsm": out["rdsm"],
           "registration": reg}
    if mask is not None:
        res.update(mae_in=out["mae_in"], mae_out=out["mae_out"])
    return res


__all__ = ["register_xy", "apply_registration", "altitude_mae_xy"]
