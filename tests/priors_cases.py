"""The numpy statement of the tie-point depth priors (include/brdfnerf_hip.h, "The depth priors of a view") and its inputs.

The statement is OUTPUT-PIXEL-MAJOR: for every output pixel it takes the source pixel of the nearest resize, then the tie point
that owns that pixel by a plain Python maximum over the tie points that name it, then that tie point's values.  The kernel is
tie-major and places through inverse index vectors from the host; the two share no structure.  The arithmetic of a tie point
(chain) is written with numpy float32 / float64 arrays, one ufunc per operation, so every operation is rounded on its own.

The ray of a tie point is an INPUT of the statement (tie_rays): the CPU tests pass the camera statement's rays
(camera_cases.rays), the GPU tests the device's own tie_rays, which holds the new arithmetic bit for bit without inheriting the
transcendental tolerance of the ray chain (test_gpu_camera.py holds that).
"""
import numpy as np

import camera_cases as M

F = np.float32
TIE_T = (1, 63, 64, 65, 257)
DOWNSCALES = (1.0, 1.5, 2.0, 3.0)
# name: (camera fixture whose SECOND view - 33 x 65 - carries the tie points, seed)
GOLDENS = {"priors_z17_utm": ("camera_z17_utm_d1", 1), "priors_z38_ecef": ("camera_z38_ecef_d2", 2),
           "priors_z21_utm_south": ("camera_z21_utm_south_d1", 3)}
# (H, W, downscale) of the stored scale_depth cases
RESIZE_CASES = ((1, 1, 1.0), (2, 1000, 1.5), (33, 65, 1.0), (33, 65, 1.5), (33, 65, 2.0), (33, 65, 3.0), (9, 11, 2.5), (9, 11, 4.0),
                (69, 7, 7.0), (257, 3, 1.5), (5, 513, 3.0), (3, 1000, 1.5), (3, 2047, 2.5))


def nearest_src(n, downscale):
    """-> n_out, [source line of output line j]: torch's nearest rule with its float32 scale n / n_out."""
    n_out = int(n / downscale)
    scale = F(n) / F(n_out)
    return n_out, [min(int(np.floor(F(j) * scale)), n - 1) for j in range(n_out)]


def chain(tie_rays, pts3d, correl, center, rng, cmin, cmax, corrscale=1.0, stdscale=1.0, margin=0.0, std_span=0.0,
          precision="reference"):
    """Steps 2-6 for every tie point: -> p (T, 3), depth, w, std (T) float32, ok (T) bool."""
    ray = np.asarray(tie_rays, F)
    P, c64 = np.asarray(pts3d, np.float64).reshape(-1, 3), np.asarray(center, np.float64)
    with np.errstate(all="ignore"):
        if precision == "reference":
            p = (P.astype(F) - c64.astype(F)) / F(rng)
        else:
            p = ((P - c64) / float(rng)).astype(F)
        t = p - ray[:, :3]
        depth = np.sqrt((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2])
        cn = ((np.asarray(correl, np.float64).reshape(-1) - float(cmin)) / (float(cmax) - float(cmin))) * float(corrscale)
        w = cn.astype(F) * (-ray[:, 5])
        s = F(stdscale) * (F(1.0) - w) + F(margin)
        std = s * F(std_span)
    assert p.dtype == depth.dtype == w.dtype == s.dtype == std.dtype == F
    ok = np.isfinite(ray[:, :8]).all(1) & np.isfinite(p).all(1) & np.isfinite(depth) & np.isfinite(w) & np.isfinite(s)
    return p, depth, w, std, ok


def priors(px, pts3d, correl, tie_rays, H, W, downscale, center, rng, cmin, cmax, **kw):
    """-> {"owner" int32 (H, W), "points" (H, W, 3), "valid_full" (H, W), "valid", "depths", "depth_std", "rays" at (Hout Wout),
    "shape", "outside", "duplicates", "skipped", "unsampled", "kept"}.  px: (T, 2) integers (col, row) at full resolution."""
    px = np.asarray(px, np.int64).reshape(-1, 2)
    T = len(px)
    p, depth, w, std, ok = chain(tie_rays, pts3d, correl, center, rng, cmin, cmax, **kw)

    def owner_of(c, r):
        return max(np.flatnonzero((px[:, 0] == c) & (px[:, 1] == r)).tolist(), default=-1)

    owner = np.full((H, W), -1, np.int32)
    points, valid_full = np.zeros((H, W, 3), F), np.zeros((H, W), F)
    for r in range(H):
        for c in range(W):
            t = owner_of(c, r)
            owner[r, c] = t
            if t >= 0 and ok[t]:
                points[r, c], valid_full[r, c] = p[t], 1.0
    Hout, src_r = nearest_src(H, downscale)
    Wout, src_c = nearest_src(W, downscale)
    valid, depths = np.zeros((Hout, Wout), F), np.zeros((Hout, Wout, 2), F)
    depth_std, rays = np.zeros((Hout, Wout), F), np.zeros((Hout, Wout, 8), F)
    sampled = set()
    for i in range(Hout):
        for j in range(Wout):
            r, c = src_r[i], src_c[j]
            sampled.add((r, c))
            t = owner_of(c, r)
            if t >= 0 and ok[t]:
                valid[i, j], depths[i, j], depth_std[i, j], rays[i, j] = 1.0, (depth[t], w[t]), std[t], np.asarray(tie_rays, F)[t, :8]
    inside = (px[:, 0] >= 0) & (px[:, 0] < W) & (px[:, 1] >= 0) & (px[:, 1] < H)
    owners = [int(t) for t in owner.ravel() if t >= 0]
    good = [t for t in owners if ok[t]]
    return {"owner": owner, "points": points, "valid_full": valid_full, "valid": valid.ravel(), "depths": depths.reshape(-1, 2),
            "depth_std": depth_std.ravel(), "rays": rays.reshape(-1, 8), "shape": (Hout, Wout), "outside": int(T - inside.sum()),
            "duplicates": int(inside.sum()) - len(owners), "skipped": len(owners) - len(good),
            "unsampled": sum((int(px[t, 1]), int(px[t, 0])) not in sampled for t in good), "kept": int(valid.sum())}


def padded(res):
    """depth_priors' padding: the float32 of the float64 mean of the kept depths where valid == 0."""
    d = res["depths"].copy()
    keep = res["valid"] > 0
    mean = F(d[keep, 0].astype(np.float64).mean()) if keep.any() else F(0.0)
    d[~keep, 0] = mean
    return d


def normals(res, H, W, downscale, precision="reference"):
    """-> normals (Hout Wout, 3), valid_normal (Hout Wout): the maps statement on the full-resolution points, (0, 0, 1) where
    valid_normal == 0, then the sampled lines."""
    import maps_cases as MP
    n = MP.point_normals(res["points"], round_f32=precision == "reference")
    vn = MP.valid_normal(res["valid_full"])
    n = np.where(vn[..., None] > 0, n, np.array([0.0, 0.0, 1.0], F)).astype(F)
    _, src_r = nearest_src(H, downscale)
    _, src_c = nearest_src(W, downscale)
    return n[src_r][:, src_c].reshape(-1, 3), vn[src_r][:, src_c].reshape(-1)


# ------------------------------------------------------------------------------------------------------------- the inputs
def world_points(d, cols, rows, min_alt, max_alt, cs, zone, south, seed):
    """World points on the rays of the pixels, on a smooth relief between 30 % and 70 % of the way from max_alt to min_alt with
    2 per mille of noise, and correlation scores in [0.3, 1): what a tie-point file holds.  Rounded to the 3 and 6 decimals the
    text files carry."""
    rng = np.random.default_rng(seed)
    r = M.rays(d, cols, rows, min_alt, max_alt, cs, zone, south, (0.0, 0.0, 0.0), 1.0, precision="exact")
    u = 0.5 + 0.2 * np.sin(np.asarray(cols) / 5.0) * np.cos(np.asarray(rows) / 4.0) + 0.002 * rng.standard_normal(len(cols))
    far = r["world_near"] + (r["rays"][:, 3:6].astype(np.float64) * r["len"][:, None])
    pts = r["world_near"] + u[:, None] * (far - r["world_near"])
    return np.round(pts, 3), np.round(rng.uniform(0.3, 1.0, len(cols)), 6)


def random_ties(H, W, T, seed):
    """T distinct pixels of the view in a shuffled order: (T, 2) int64 (col, row)."""
    rng = np.random.default_rng(seed)
    flat = rng.choice(H * W, size=min(T, H * W), replace=False)
    if T > H * W:
        flat = np.concatenate([flat, rng.integers(0, H * W, T - H * W)])
    return np.stack([flat % W, flat // W], -1).astype(np.int64)


def hard_ties(H, W, T, seed):
    """T tie points with the four corners, points outside on every side (negatives included) and up to five on one pixel."""
    px = random_ties(H, W, T, seed)
    special = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (-1, 0), (0, -1), (W, 0), (0, H), (-7, -3), (W + 5, H + 2), (2 ** 31 - 1, 1),
               (-2 ** 31, 0)] + [(W // 2, H // 2)] * 5 + [(1 % W, 1 % H)] * 2
    k = min(len(special), T)
    where = np.random.default_rng(seed + 1).permutation(T)[:k]
    px[where] = np.asarray(special[:k], np.int64)
    return px


def golden_ties(name):
    """The inputs of a priors fixture: the second view (33 x 65) of its camera fixture at downscale 1, with about four pixels in
    five a tie point - a checkerboard inside every fifth 4 x 4 block and one pixel in eleven left out - sorted row-major and
    unique.  -> view, px (T, 2), the camera fixture's (cs, zone, south)."""
    cam, _ = GOLDENS[name]
    site, cs, south, _ = M.GOLDENS[cam]
    v = M.golden_views(cam)[1]
    H, W = v["H"], v["W"]
    rows, cols = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    keep = ((rows // 4 + cols // 4) % 5 != 0) | ((rows + cols) % 2 == 0)
    keep &= (rows * 7 + cols * 3) % 11 != 0
    px = np.stack([cols[keep], rows[keep]], -1).astype(np.int64)
    return v, px, (cs, M.SITES[site][2], south)
