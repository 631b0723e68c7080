"""Cases and the float64 statements of the metric kernels (bn_ssim_map, bn_grid_normals, bn_normal_angle), shared by
tests/test_metrics_cpu.py and tests/test_gpu_metrics.py.

The statements are written from the rules the C header gives and from the reference lines it cites, not from the product's
code: numpy float64 with one rounding per operation (numpy ufuncs do not fuse), Python integers for the sums, Python loops over
the taps (k2 outer, k1 inner) vectorised over the pixels.

  SSIM      x = (float64(pred) float64(mask)) / div, y likewise; 'reflect' padding without repeating the edge; w = g[k2] g[k1];
            mu_x, mu_y, E[xx], E[yy], E[xy] start at 0.0 and take s = s + w v tap by tap in row-major order; C1 = (0.01 max_val)^2,
            C2 = (0.03 max_val)^2; sxx = E[xx] - mu_x mu_x ...; v = ((2 mu_x mu_y + C1)(2 sxy + C2)) /
            ((mu_x mu_x + mu_y mu_y + C1)(sxx + syy + C2) + 1e-12); sum += rint(v 2^30) over the finite v with |v| < 4, the others
            counted as skipped.  g = exp(-x^2 / (2 1.5^2)) / sum, float64 on the host.
  normals   P(r, c) = (c res, r res, z); S, N, E, W = N(P(neighbour) - P); N(v) = v / sqrt(max((v.x^2 + v.y^2) + v.z^2, 2^-23));
            n = N((((N(E x N) + N(W x S)) + N(N x W)) + N(S x E)) / 4); border cells zero; float32 at the end.
  angle     a = arccos(clip((a.x b.x + a.y b.y) + a.z b.z, -1, 1)) 180 / pi from the float32 normals; sum += rint(a 2^20), NaN left out.

The SSIM rule follows kornia 0.5.3 (ssim with a Gaussian window, as metrics.py:327-341 calls it) as read from its documented
definition.  It was NOT checked against the package, which is not installed here and which this project does not depend on.
"""
import functools
import math

import numpy as np

SSIM_FIX = 2.0 ** 30
ANGLE_FIX = 2.0 ** 20
EPS32 = np.float64(2.0 ** -23)


# ------------------------------------------------------------------------------------------------------------------ SSIM
def gaussian(window):
    e = [math.exp(-float((k - window // 2) ** 2) / (2.0 * 1.5 ** 2)) for k in range(window)]
    s = sum(e)
    return np.array([v / s for v in e], dtype=np.float64)


def strides(layout, C, H, W):
    """(plane, row, col) element strides in an (H W, C) ray-major buffer: 'reference' is eval.py:471's .view(1, C, H, W), a
    reinterpretation (plane c = flat[c H W : (c + 1) H W]); 'image' is the true image (channel c of pixel p at flat[p C + c])."""
    return {"reference": (H * W, W, 1), "image": (1, C * W, C)}[layout]


def planes(flat, layout, C, H, W):
    """The (C, H, W) planes a layout addresses in a flat buffer, gathered element by element through the strides."""
    sp, sr, sc = strides(layout, C, H, W)
    c, r, col = np.meshgrid(np.arange(C), np.arange(H), np.arange(W), indexing="ij")
    return np.asarray(flat).reshape(-1)[c * sp + r * sr + col * sc]


def reflect_index(n, pad):
    i = np.arange(-pad, n + pad)
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def ssim_map(pred, gt, mask, div, max_val, window, g=None, pad_index=reflect_index, column_major=False):
    """pred, gt (C, H, W) float32 planes, mask (H, W) uint8 or None -> v (C, H, W) float64.
    pad_index / column_major: the two perturbations the tests must be able to see (another padding rule, another tap order)."""
    g = gaussian(window) if g is None else np.asarray(g, dtype=np.float64)
    C, H, W = pred.shape
    pad = window // 2
    assert H > pad and W > pad
    m = np.ones((H, W), dtype=np.float64) if mask is None else np.asarray(mask).astype(np.float64)
    div = np.float64(div)
    with np.errstate(all="ignore"):
        x = (pred.astype(np.float64) * m) / div
        y = (gt.astype(np.float64) * m) / div
        ri, ci = pad_index(H, pad), pad_index(W, pad)
        xp, yp = x[:, ri][:, :, ci], y[:, ri][:, :, ci]
        mx, my, exx, eyy, exy = (np.zeros((C, H, W), dtype=np.float64) for _ in range(5))
        taps = [(k2, k1) for k2 in range(window) for k1 in range(window)]
        if column_major:
            taps = [(k2, k1) for k1 in range(window) for k2 in range(window)]
        for k2, k1 in taps:
            w = g[k2] * g[k1]
            xs, ys = xp[:, k2:k2 + H, k1:k1 + W], yp[:, k2:k2 + H, k1:k1 + W]
            xx, yy, xy = xs * xs, ys * ys, xs * ys
            mx = mx + w * xs
            my = my + w * ys
            exx = exx + w * xx
            eyy = eyy + w * yy
            exy = exy + w * xy
        a1, a2 = np.float64(0.01) * np.float64(max_val), np.float64(0.03) * np.float64(max_val)
        C1, C2 = a1 * a1, a2 * a2
        sxx, syy, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
        num = (2.0 * mx * my + C1) * (2.0 * sxy + C2)
        den = (mx * mx + my * my + C1) * (sxx + syy + C2) + 1e-12
        return num / den


def ssim_sums(v, rows=None):
    """-> (sum of rint(v 2^30), cells summed, cells skipped) as Python integers, over the output rows [row0, row1)."""
    v = v if rows is None else v[:, rows[0]:rows[1]]
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(v) & (np.abs(v) < 4.0)
    q = np.rint(v[ok] * SSIM_FIX)
    return sum(int(t) for t in q), int(ok.sum()), int(v.size - ok.sum())


def _images(C, H, W, seed, scale=1.0):
    g = np.random.RandomState(seed)
    gt = (g.rand(H * W * C) * scale).astype(np.float32)
    pred = np.clip(gt + 0.1 * scale * g.randn(H * W * C), 0.0, None).astype(np.float32)
    return pred, gt


def _blob_mask(H, W, seed):
    g = np.random.RandomState(seed)
    m = (g.rand(H, W) < 0.7).astype(np.uint8)
    m[: H // 4, : W // 3] = 0                      # a solid masked corner as well as scattered pixels
    return m


def _identical(C, H, W, seed):
    pred, gt = _images(C, H, W, seed)
    return gt.copy(), gt


def _constant(C, H, W):
    return np.full(H * W * C, 0.3, dtype=np.float32), np.full(H * W * C, 0.5, dtype=np.float32)


def _gt_zero(C, H, W, seed):
    pred, gt = _images(C, H, W, seed)
    return pred, np.zeros_like(gt)


def _illcond(C, H, W, seed):
    """Two nearly constant images, 64 + 1e-3 noise: E[xx] - mu_x mu_x cancels 4096 down to 1e-6, so a rounding of the tap sums
    (1 ulp of float64) is a relative 1e-7 of the variance - visible in the float32 map once C1 and C2 are small."""
    g = np.random.RandomState(seed)
    return (64.0 + 1.0e-3 * g.randn(H * W * C)).astype(np.float32), (64.0 + 1.0e-3 * g.randn(H * W * C)).astype(np.float32)


NAN_AT = (1, 6, 7)                                # plane, row, column of the NaN pixel (interior: its window cuts no edge)


def _nan_pixel(C, H, W, seed):
    pred, gt = _images(C, H, W, seed)
    pred[NAN_AT[0] * H * W + NAN_AT[1] * W + NAN_AT[2]] = np.nan
    return pred, gt


# name -> (C, H, W, window, layout, masked, rescaled, builder of (pred, gt) flat float32 buffers of H W C elements)
SSIM_CASES = {
    "2x2_w3": (3, 2, 2, 3, "reference", False, False, lambda: _images(3, 2, 2, 1)),                # every cell reflects
    "3x5_w3": (3, 3, 5, 3, "reference", False, False, lambda: _images(3, 3, 5, 2)),
    "3x5_w3_illcond": (3, 3, 5, 3, "reference", False, False, lambda: _illcond(3, 3, 5, 13)),      # see MAX_VAL
    "6x7_w11": (3, 6, 7, 11, "reference", False, False, lambda: _images(3, 6, 7, 3)),              # the smallest legal image
    "32x32_w3": (3, 32, 32, 3, "reference", False, False, lambda: _images(3, 32, 32, 4)),          # exactly one tile
    "33x31_w11": (3, 33, 31, 11, "reference", False, False, lambda: _images(3, 33, 31, 5)),        # ragged both ways
    "17x65_w7": (3, 17, 65, 7, "reference", False, False, lambda: _images(3, 17, 65, 6)),
    "33x31_w3_image": (3, 33, 31, 3, "image", False, False, lambda: _images(3, 33, 31, 5)),
    "64x96_mask_reference": (3, 64, 96, 3, "reference", True, False, lambda: _images(3, 64, 96, 7)),
    "64x96_mask_reference_scl": (3, 64, 96, 3, "reference", True, True, lambda: _images(3, 64, 96, 7)),
    "64x96_mask_image": (3, 64, 96, 3, "image", True, False, lambda: _images(3, 64, 96, 7)),
    "64x96_mask_image_scl": (3, 64, 96, 5, "image", True, True, lambda: _images(3, 64, 96, 7)),
    "c1_20x24_w5": (1, 20, 24, 5, "reference", False, False, lambda: _images(1, 20, 24, 8)),       # a single plane
    "identical_16x18": (3, 16, 18, 3, "reference", False, False, lambda: _identical(3, 16, 18, 9)),
    "constant_16x18": (3, 16, 18, 3, "reference", False, False, lambda: _constant(3, 16, 18)),     # zero variance
    "gt_zero_16x18": (3, 16, 18, 3, "reference", False, False, lambda: _gt_zero(3, 16, 18, 10)),   # max_val = 0: C1 = C2 = 0
    "gt_zero_16x18_scl": (3, 16, 18, 3, "reference", False, True, lambda: _gt_zero(3, 16, 18, 10)),  # div = 0: every cell skipped
    "nan_pixel_16x18_w3": (3, 16, 18, 3, "reference", False, False, lambda: _nan_pixel(3, 16, 18, 11)),
    "nan_pixel_16x18_w5": (3, 16, 18, 5, "reference", False, False, lambda: _nan_pixel(3, 16, 18, 11)),
    "large_1e4_16x18": (3, 16, 18, 3, "reference", False, False, lambda: _images(3, 16, 18, 12, scale=1.0e4)),
}
# cases handed another max_val than max(target * mask) (the entry takes any finite one): 2^-10 makes C1 and C2 negligible
MAX_VAL = {"3x5_w3_illcond": 2.0 ** -10}
# the cases the two perturbations must break: edge-repeat padding changes both, a column-major tap order (w is symmetric, so
# only the roundings of the sums move) the ill-conditioned one
PERTURBATION_CASES = ("3x5_w3", "3x5_w3_illcond")


def edge_index(n, pad):
    return np.clip(np.arange(-pad, n + pad), 0, n - 1)


@functools.lru_cache(maxsize=None)
def ssim_case(name):
    """-> dict: C, H, W, window, layout, strides, pred, gt (flat float32), mask ((H, W) uint8 or None), div, max_val, g."""
    C, H, W, window, layout, masked, scl, make = SSIM_CASES[name]
    pred, gt = make()
    mask = _blob_mask(H, W, 21) if masked else None
    gp = planes(gt, layout, C, H, W)
    top = float(np.max(gp if mask is None else gp * mask.astype(np.float32)))          # max_val = max(target * mask)
    top = MAX_VAL.get(name, top)
    for a in (pred, gt) + (() if mask is None else (mask,)):
        a.setflags(write=False)
    return dict(C=C, H=H, W=W, window=window, layout=layout, strides=strides(layout, C, H, W), pred=pred, gt=gt, mask=mask,
                div=top if scl else 1.0, max_val=1.0 if scl else top, g=gaussian(window), top=top, scl=scl)


@functools.lru_cache(maxsize=None)
def ssim_expected(name):
    """The statement's result for a case, computed once and shared: v (C, H, W) float64, map float32, sums (3 Python ints)."""
    c = ssim_case(name)
    v = ssim_map(planes(c["pred"], c["layout"], c["C"], c["H"], c["W"]), planes(c["gt"], c["layout"], c["C"], c["H"], c["W"]),
                 c["mask"], c["div"], c["max_val"], c["window"], c["g"])
    with np.errstate(all="ignore"):
        m32 = v.astype(np.float32)
    v.setflags(write=False)
    m32.setflags(write=False)
    return {"v": v, "map": m32, "sums": ssim_sums(v)}


# ------------------------------------------------------------------------------------------------------------------ normals
def _unit(v):
    n = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]
    return v / np.sqrt(np.maximum(n, EPS32))[..., None]             # np.maximum keeps a NaN, as torch.maximum does


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def normals(z, res, as_float32=True):
    """z (H, W) float32 -> (H, W, 3): the reference's four-cross-product normals (sat_utils.py:16-50, 175-183) in float64."""
    z = np.asarray(z, dtype=np.float32).astype(np.float64)
    H, W = z.shape
    res = np.float64(res)
    rows, cols = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    P = np.stack([cols * res, rows * res, z], -1)
    out = np.zeros((H, W, 3), dtype=np.float64)
    if H >= 3 and W >= 3:
        with np.errstate(all="ignore"):
            c = P[1:-1, 1:-1]
            S, N = _unit(P[2:, 1:-1] - c), _unit(P[:-2, 1:-1] - c)
            E, Wv = _unit(P[1:-1, 2:] - c), _unit(P[1:-1, :-2] - c)
            n1, n2, n3, n4 = _unit(_cross(E, N)), _unit(_cross(Wv, S)), _unit(_cross(N, Wv)), _unit(_cross(S, E))
            out[1:-1, 1:-1] = _unit((((n1 + n2) + n3) + n4) / 4.0)
    return out.astype(np.float32) if as_float32 else out


def plane_normal(a, b):
    """The exact normal of z = a x + b y + d under the reference's axes: (a, b, -1) / sqrt(1 + a^2 + b^2)."""
    return np.array([a, b, -1.0]) / math.sqrt(1.0 + a * a + b * b)


def angle_map(n1, n2, border):
    """n1, n2 (H, W, 3) float32 -> a (H, W) float64 degrees; border 1: NaN on the border cells."""
    a, b = np.asarray(n1, dtype=np.float32).astype(np.float64), np.asarray(n2, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        d = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
        ang = np.arccos(np.clip(d, -1.0, 1.0)) * 180.0 / np.pi
    if border:
        ang[0, :] = ang[-1, :] = np.nan
        ang[:, 0] = ang[:, -1] = np.nan
    return ang


def angle_sums(ang, mask):
    """-> [sum, count] over all, inside and outside cells (6 Python ints); no mask: every cell is inside."""
    inside = np.ones(ang.shape, dtype=bool) if mask is None else np.asarray(mask) != 0
    out = []
    for sel in (np.ones(ang.shape, dtype=bool), inside, ~inside):
        a = ang[sel & ~np.isnan(ang)]
        out += [sum(int(t) for t in np.rint(a * ANGLE_FIX)), int(a.size)]
    return out


def _terrain(H, W, seed, amp=2.0):
    g = np.random.RandomState(seed)
    return (30.0 + amp * g.randn(H, W)).astype(np.float32)


def _plane(H, W, a, b, res):
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return (20.0 + a * c * res + b * r * res).astype(np.float32)


def _step(H, W):
    z = np.full((H, W), 10.0, dtype=np.float32)
    z[:, W // 2:] = 14.0
    return z


def _with_nan(z, at):
    z = z.copy()
    z[at] = np.nan
    return z


PLANE = (0.25, -0.5, 0.5)                       # a, b, resolution: dyadic, so the float32 altitudes of the plane are exact
# name -> (resolution, builder of z (H, W) float32)
NORMAL_CASES = {
    "3x3": (0.5, lambda: _terrain(3, 3, 1)),                               # one interior cell
    "4x9": (0.3, lambda: _terrain(4, 9, 2)),
    "33x31": (0.3, lambda: _terrain(33, 31, 3)),                           # more than one block
    "33x31_other": (0.3, lambda: _terrain(33, 31, 4)),
    "plane_6x7": (PLANE[2], lambda: _plane(6, 7, PLANE[0], PLANE[1], PLANE[2])),
    "flat_5x5": (0.5, lambda: np.full((5, 5), 12.0, dtype=np.float32)),
    "step_8x10": (0.5, lambda: _step(8, 10)),
    "nan_9x8": (0.5, lambda: _with_nan(_terrain(9, 8, 5), (4, 3))),
    "9x8": (0.5, lambda: _terrain(9, 8, 6)),
    "2x5": (0.5, lambda: _terrain(2, 5, 7)),                               # no interior cell at all
}
# name -> (first grid, second grid, masked, border)
ANGLE_CASES = {
    "3x3_equal": ("3x3", "3x3", False, 0),                                 # angle 0 inside, 90 on the reference's border
    "33x31_equal_b1": ("33x31", "33x31", False, 1),
    "33x31": ("33x31", "33x31_other", False, 0),
    "33x31_mask": ("33x31", "33x31_other", True, 0),
    "33x31_mask_b1": ("33x31", "33x31_other", True, 1),
    "nan_9x8_mask": ("nan_9x8", "9x8", True, 0),
    "nan_9x8_b1": ("nan_9x8", "9x8", False, 1),
    "step_equal": ("step_8x10", "step_8x10", False, 0),
}


@functools.lru_cache(maxsize=None)
def normal_case(name):
    res, make = NORMAL_CASES[name]
    z = make()
    z.setflags(write=False)
    return res, z


@functools.lru_cache(maxsize=None)
def normals_expected(name):
    res, z = normal_case(name)
    n = normals(z, res)
    n.setflags(write=False)
    return n


@functools.lru_cache(maxsize=None)
def angle_mask(name):
    first = ANGLE_CASES[name][0]
    H, W = normal_case(first)[1].shape
    m = _blob_mask(H, W, 31) if ANGLE_CASES[name][2] else None
    if m is not None:
        m.setflags(write=False)
    return m
