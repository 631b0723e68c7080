"""Statements and cases of the validation maps (brdf_nerf_amd/maps.py, bn_ray_maps / bn_point_normals).

The statements are numpy restatements of the rules include/brdfnerf_hip.h gives, sharing no structure with the kernels: the
nearest sample is np.argmin, the variance and the accumulated sum are plain loops over s on float64 arrays, the counters are
Python integers, the normals are sliced array expressions.  tests/test_maps_cpu.py holds them to the goldens recorded from the
reference (tests/golden/make_maps_goldens.py); tests/test_gpu_maps.py holds the kernels to them bit for bit.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STD_FIX = 2.0 ** 20
EPS32 = 2.0 ** -23
COUNTERS = ("std_sum", "std_count", "std_skipped", "bad_nr", "nr0", "nr_total")
RAY_GOLDENS = ("maps_rays_s128", "maps_rays_s24")
NORMAL_GOLDENS = ("maps_normals_utm", "maps_normals_local")


def golden(name):
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------------------ bn_ray_maps
def surf_idx(z, depth):
    """np.argmin of |z - depth| in float32 (eval.py:411-412): the first NaN, else the first minimum."""
    dev = np.abs(z.astype(np.float32) - depth.astype(np.float32)[:, None])
    assert dev.dtype == np.float32
    return np.argmin(dev, axis=1).astype(np.int32)


def surf(X, idx):
    return X[np.arange(X.shape[0]), idx.astype(np.int64)]


def variance(z, w, depth):
    """-> var, std float32: v = v + (t t) w in float64, s ascending, one numpy operation per rounding."""
    v = np.zeros(z.shape[0], dtype=np.float64)
    d = depth.astype(np.float64)
    with np.errstate(all="ignore"):
        for s in range(z.shape[1]):
            t = z[:, s].astype(np.float64) - d
            tt = t * t
            v = v + tt * w[:, s].astype(np.float64)
        return v.astype(np.float32), np.sqrt(v).astype(np.float32)


def accum(w, X):
    a = np.zeros((X.shape[0], X.shape[2]), dtype=np.float64)
    with np.errstate(all="ignore"):
        for s in range(X.shape[1]):
            a = a + w[:, s, None].astype(np.float64) * X[:, s, :].astype(np.float64)
        return a.astype(np.float32)


def counters(std, S, normals=None, view=None):
    """The six integers of a launch as Python ints; normals (R, S, 3) float32 with view (R, 3) float32, or None."""
    out = dict.fromkeys(COUNTERS, 0)
    for sd in std.astype(np.float64):
        if np.isfinite(sd) and sd < 2.0 ** 40:
            out["std_sum"] += int(np.rint(sd * STD_FIX))
            out["std_count"] += 1
        else:
            out["std_skipped"] += 1
    if normals is not None:
        n, v = normals.astype(np.float64), view.astype(np.float64)[:, None, :]
        with np.errstate(all="ignore"):
            px, py, pz = n[..., 0] * v[..., 0], n[..., 1] * v[..., 1], n[..., 2] * v[..., 2]
            dot = (px + py) + pz
            norm = np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2])
            out["bad_nr"] = int((dot < 0).sum())
            out["nr0"] = int((~(norm > 0.99999)).sum())
        out["nr_total"] = int(normals.shape[0]) * int(S)
    return out


def ray_statement(z, w, depth, X=None, normal_col=None, view=None, accumulate=False):
    idx = surf_idx(z, depth)
    var, std = variance(z, w, depth)
    nr = None if normal_col is None else X[:, :, normal_col:normal_col + 3]
    return {"surf_idx": idx, "surf": None if X is None or X.shape[2] == 0 else surf(X, idx), "var": var, "std": std,
            "accum": accum(w, X) if accumulate else None, "counters": counters(std, z.shape[1], nr, view)}


def ray_inputs(R, S, E, seed, normal_col=None):
    """Depth-sorted samples around a surface, weights that sum to about one, a per-sample tensor and unit view vectors; with a
    normal column those three channels are unit normals scattered over the sphere, a few shortened (check_vec0 counts them)."""
    rng = np.random.default_rng(seed)
    z = np.sort(rng.uniform(0.2, 1.8, (R, S)), axis=1).astype(np.float32)
    w = rng.random((R, S)) ** 4
    w = (w / w.sum(1, keepdims=True) * rng.uniform(0.6, 1.0, (R, 1))).astype(np.float32)
    depth = (z.astype(np.float64) * w).sum(1).astype(np.float32)
    X = rng.standard_normal((R, S, E)).astype(np.float32)
    view = rng.standard_normal((R, 3))
    view = (view / np.linalg.norm(view, axis=1, keepdims=True)).astype(np.float32)
    if normal_col is not None:
        n = rng.standard_normal((R, S, 3))
        n /= np.linalg.norm(n, axis=2, keepdims=True)
        # length 1.0001, not 1: a float32 unit vector is 1e-5 -+ 1e-7 above check_vec0's 0.99999, inside the generator's margin
        n *= np.where(rng.random((R, S, 1)) < 0.1, rng.uniform(0.0, 0.9, (R, S, 1)), 1.0001)
        X[:, :, normal_col:normal_col + 3] = n.astype(np.float32)
    return z, w, depth, X, view


RAY_R = (1, 63, 64, 65, 257)
RAY_S = (1, 2, 63, 64, 65, 128, 192)
RAY_E = (0, 1, 3, 16, 28)


def tie_case(R=70, S=65):
    """z symmetric about depth in exactly representable steps: every ray has an exact tie between two samples (the first wins);
    a third of the rays have the depth below z_0, a third above z_{S-1}."""
    k = np.arange(S, dtype=np.float64) - (S - 1) / 2.0           # ..., -1, 0, 1, ... (odd S) or ..., -0.5, 0.5, ... (even S)
    z = np.tile((1.0 + k / 64.0)[None], (R, 1))
    depth = np.full(R, 1.0)
    z[1::3] += 0.25 + S / 64.0                                   # the depth lies below the first sample
    z[2::3] -= 0.25 + S / 64.0                                   # ... above the last one
    z[0::3, (S - 1) // 2] = 1.0 - 3.0 / 64.0                     # break the centre sample so that the tie is between two samples
    z[0::3] = np.sort(z[0::3], axis=1)
    rng = np.random.default_rng(5)
    w = rng.random((R, S)).astype(np.float32)
    return z.astype(np.float32), w, depth.astype(np.float32)


# -------------------------------------------------------------------------------------------------------- bn_point_normals
def l2n(v):
    n = ((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])[..., None]
    with np.errstate(all="ignore"):
        return v / np.sqrt(np.where(n < EPS32, EPS32, n))        # a NaN norm stays NaN: NaN < eps is False


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def point_normals(points, round_f32=True):
    """calc_normal_from_pts3d (sat_utils.py:16-50) in float64, on the float32-rounded points with round_f32 -> (H, W, 3) float32."""
    p = points.astype(np.float64)
    if round_f32:
        p = p.astype(np.float32).astype(np.float64)
    out = np.zeros(p.shape, dtype=np.float32)
    if p.shape[0] < 3 or p.shape[1] < 3:
        return out
    with np.errstate(all="ignore"):
        c = p[1:-1, 1:-1]
        south, north = l2n(p[2:, 1:-1] - c), l2n(p[:-2, 1:-1] - c)
        east, west = l2n(p[1:-1, 2:] - c), l2n(p[1:-1, :-2] - c)
        n1, n2, n3, n4 = l2n(cross(east, north)), l2n(cross(west, south)), l2n(cross(north, west)), l2n(cross(south, east))
        out[1:-1, 1:-1] = l2n((((n1 + n2) + n3) + n4) / 4.0).astype(np.float32)
    return out


def valid_normal(valid):
    v = valid.astype(np.float32)
    out = np.where(v < np.float32(1e-5), v, np.float32(1.0)).astype(np.float32)
    if v.shape[0] >= 3 and v.shape[1] >= 3:
        out[1:-1, 1:-1] = ((v[2:, 1:-1] * v[:-2, 1:-1]) * v[1:-1, 2:]) * v[1:-1, :-2]
    return out


def utm_points(H=9, W=11, seed=3, east=3.7e5, north=3.3e6, spacing=0.4):
    """An H x W image of surface points about `spacing` metres apart at UTM-sized coordinates, with relief of a few metres."""
    rng = np.random.default_rng(seed)
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x = east + spacing * ii + 0.03 * rng.standard_normal((H, W))
    y = north - spacing * jj + 0.03 * rng.standard_normal((H, W))
    zz = 30.0 + 1.5 * np.sin(ii / 2.0) * np.cos(jj / 3.0) + 0.05 * rng.standard_normal((H, W))
    return np.stack([x, y, zz], axis=-1)


def grid_points(z, res):
    """get_pts3d_from_dsm's points (c res, r res, z) in float64: bn_point_normals on them is bn_grid_normals."""
    H, W = z.shape
    jj, ii = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return np.stack([ii * res, jj * res, z.astype(np.float64)], axis=-1)


POINT_SHAPES = ((1, 1), (2, 7), (3, 3), (3, 300), (33, 65), (64, 64))


def angle_deg(a, b):
    d = np.clip((a.astype(np.float64) * b.astype(np.float64)).sum(-1), -1.0, 1.0)
    return np.degrees(np.arccos(d))
