#!/usr/bin/env python
"""Generate the registration goldens (tests/golden/dsmr_*.npz) by running the REFERENCE's dsmr.py on synthetic grids.

Run only where the reference tree is present (BRDFNERF_REFERENCE, default /root/reference, read-only):

    python tests/golden/make_dsmr_goldens.py

dsmr.py is imported with empty stub modules for numba (jit = identity) and rasterio, as make_goldens.py stubs its I/O imports;
its downsample2x, recursive_ncc (-> compute_ncc -> ncc -> mean_std), mean_std and apply_shift_ then run as plain Python (about
a minute in all).  The inputs are stored as float32 and WIDENED to float64 before every call: numba types a float32 image's
sums as float64, while NumPy 2 without numba would keep them in float32.  The altitudes of the two larger fixtures are multiples
of 2^-6 m so that the files compress (their quanta are then exact); the small one keeps every float32 bit, so its quanta round.

Recorded per fixture: u (ground truth) and v (prediction) float32; the pyramid levels u1, v1, u2, v2, ... float64 as
recursive_ncc formed them; `levels` int64 rows (H, W, dx, dy), coarsest first, as compute_ncc returned them; `corr` the
(2r + 1)^2 correlations of every level in scan order; `gaps` the difference between the best and the second-best correlation
of every level; muu, muv, b of compute_shift(scaling=False) at the final shift; rdsm float32, apply_shift_'s output.

CONDITION ON THE INPUTS (not a tolerance on any code): the top-two gap is at least 1e-3 at every level of every fixture, so an
integer restatement of the correlation, which differs from the float64 one by about 1e-7, must find the same shift.  A true
shift that is odd puts the coarser level on a near-tie between its two neighbours; the fixtures with a pyramid use shifts
that stay integral at every level.
"""
import os
import sys
import types

import numpy as np

REF = os.environ.get("BRDFNERF_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
MIN_GAP = 1e-3

# name: (H, W, true (dx, dy), z offset of the prediction, seed)
FIXTURES = {
    "no_pyramid": (60, 72, (3, -2), 1.5, 11),
    "one_level": (104, 112, (8, -4), -3.25, 12),
    "two_levels": (204, 208, (12, -8), 2.75, 13),
}


def load_dsmr():
    numba = types.ModuleType("numba")
    numba.jit = lambda f=None, *a, **k: f if callable(f) else (lambda g: g)
    sys.modules["numba"] = numba
    sys.modules["rasterio"] = types.ModuleType("rasterio")
    sys.path.insert(0, REF)
    import dsmr
    return dsmr


def surface(H, W, shift, offset, seed):
    """A smooth surface plus steps (buildings) plus 0.05 m noise on a canvas with a margin; the ground truth is a crop, the
    prediction the crop moved by `shift` and lowered / raised by `offset`, with noise of its own; 5 % NaN cells in the
    prediction and a NaN patch in the ground truth.  gt[j][i] pairs with pred[j + dy][i + dx]."""
    rng = np.random.default_rng(seed)
    m = 20
    jj, ii = np.meshgrid(np.arange(H + 2 * m), np.arange(W + 2 * m), indexing="ij")
    f = 40.0 + 4.0 * np.sin(jj / 17.0) * np.cos(ii / 23.0) + 0.02 * ii
    for _ in range(12):
        r0, c0 = rng.integers(0, H + 2 * m - 8), rng.integers(0, W + 2 * m - 8)
        f[r0:r0 + rng.integers(6, 24), c0:c0 + rng.integers(6, 24)] += rng.uniform(3.0, 15.0)
    dx, dy = shift
    gt = f[m:m + H, m:m + W] + 0.05 * rng.standard_normal((H, W))
    pred = f[m - dy:m - dy + H, m - dx:m - dx + W] - offset + 0.05 * rng.standard_normal((H, W))
    pred[rng.random((H, W)) < 0.05] = np.nan
    gt[H // 3:H // 3 + 7, W // 2:W // 2 + 9] = np.nan
    q = lambda a: (np.round(a * 64.0) / 64.0 if H > 100 else a).astype(np.float32)
    return q(gt), q(pred)


def run(dsmr, name):
    H, W, shift, offset, seed = FIXTURES[name]
    u32, v32 = surface(H, W, shift, offset, seed)
    u, v = u32.astype(np.float64)[None], v32.astype(np.float64)[None]
    pyramid, levels, corrs = [], [], []
    real_down, real_ncc, real_compute = dsmr.downsample2x, dsmr.ncc, dsmr.compute_ncc

    def down(a):
        out = real_down(a)
        pyramid.append(out[0].copy())
        return out

    def ncc(a, b, dx=0, dy=0):
        with np.errstate(all="ignore"):
            c = real_ncc(a, b, dx, dy)
        corrs[-1].append(float(c))
        return c

    def compute(a, b, irange, initdx, initdy):
        corrs.append([])
        dx, dy = real_compute(a, b, irange, initdx, initdy)
        levels.append((a.shape[-2], a.shape[-1], dx, dy))
        return dx, dy

    dsmr.downsample2x, dsmr.ncc, dsmr.compute_ncc = down, ncc, compute
    try:
        dx, dy = dsmr.recursive_ncc(u, v)
    finally:
        dsmr.downsample2x, dsmr.ncc, dsmr.compute_ncc = real_down, real_ncc, real_compute
    muu, muv, _, _, _ = dsmr.mean_std(u, v, dx, dy)
    b = muu - muv * 1                                     # compute_shift(scaling=False): a = 1
    out = np.zeros((1, H, W), dtype=np.float32)           # np.zeros_like(v) of the float32 raster upstream reads
    dsmr.apply_shift_(v, out, dx, dy, 1, np.float64(b), 0, 0)
    gaps = []
    for c in corrs:
        top = np.sort(np.asarray(c)[np.isfinite(c)])[::-1]
        gaps.append(float(top[0] - top[1]))
    assert (dx, dy) == shift, (name, dx, dy)
    assert min(gaps) >= MIN_GAP, f"{name}: top-two correlation gaps {gaps}: choose inputs without a near-tie"
    data = {"u": u32, "v": v32, "levels": np.asarray(levels, dtype=np.int64), "gaps": np.asarray(gaps),
            "corr": np.asarray(corrs, dtype=np.float64), "muu": np.float64(muu), "muv": np.float64(muv), "b": np.float64(b),
            "rdsm": out[0]}
    for l in range(len(pyramid) // 2):                    # recursive_ncc halves u, then v, level by level
        data[f"u{l + 1}"], data[f"v{l + 1}"] = pyramid[2 * l], pyramid[2 * l + 1]
    path = os.path.join(OUT, f"dsmr_{name}.npz")
    np.savez_compressed(path, **data)
    print(f"{name}: {H} x {W}, levels {levels}, gaps {['%.3g' % g for g in gaps]}, b {b!r}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    mod = load_dsmr()
    for fixture in (sys.argv[1:] or FIXTURES):
        run(mod, fixture)
