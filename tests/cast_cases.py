"""The ray-casting rule of include/brdfnerf_hip.h ("Depth of a surface model along a ray") as a numpy float64 statement, and the
cases of tests/test_cast_cpu.py and tests/test_gpu_cast.py.

The statement is a loop over the walk's steps with array expressions over ALL rays at once: it knows nothing of blocks, chunks or
lanes, skips nothing (a ray far outside the grid is walked cell by cell) and forms both crossing parameters in every cell.  Every
operation is one numpy float64 operation, so each is rounded on its own, as in the kernel.  Its three keyword switches (le, tie,
top) state PERTURBED rules for test_cast_cpu.py; the defaults are the rule.
"""
import math

import numpy as np

import visibility_cases as V

TOP, WALL, MISS, NODATA, BELOW = 0, 1, 2, 3, 4
MAX_SPAN = 65536.0
INF = float("inf")


def cast_statement(rays, center, rng, dsm, xoff, yoff, res, zmax=INF, le=np.less_equal, tie="both", top="solve"):
    """rays (R, >= 8) float32 = (o, d, near, far, ...); center (3,), rng: the frame; dsm (H, W) float32 on (xoff, yoff, res).
    -> depth (R,) float32, state (R,) uint8, cell (R,) int32, nan_cells (R,) int32, counts (5,) int64.
    zmax: cells wholly above it are not tested (NaN cells are counted all the same).  Perturbations: le=np.less (a strict
    comparison), tie='u' (on lam_u == lam_v only i moves), top='out' (a top hit reported at lam_out instead of solved for h)."""
    rays = np.asarray(rays, dtype=np.float32)
    dsm = np.asarray(dsm, dtype=np.float32)
    H, W = dsm.shape
    cells = dsm.astype(np.float64)
    R = rays.shape[0]
    f8 = np.float64
    o, d = rays[:, 0:3].astype(f8), rays[:, 3:6].astype(f8)
    near, far = rays[:, 6].astype(f8), rays[:, 7].astype(f8)
    c, rng, xoff, yoff, res = np.asarray(center, dtype=f8), f8(rng), f8(xoff), f8(yoff), f8(res)
    depth = np.full(R, np.nan, dtype=np.float32)
    cell = np.full(R, -1, dtype=np.int32)
    nan_cells = np.zeros(R, dtype=np.int32)
    with np.errstate(all="ignore"):
        P0 = (o + d * near[:, None]) * rng + c
        P1 = (o + d * far[:, None]) * rng + c
        u0, v0, z0 = (P0[:, 0] - xoff) / res, (yoff - P0[:, 1]) / res, P0[:, 2]
        u1, v1, z1 = (P1[:, 0] - xoff) / res, (yoff - P1[:, 1]) / res, P1[:, 2]
        du, dv, dz = u1 - u0, v1 - v0, z1 - z0
        finite = np.isfinite(u0) & np.isfinite(v0) & np.isfinite(z0) & np.isfinite(u1) & np.isfinite(v1) & np.isfinite(z1)
        nodata = ~finite | (np.fabs(du) + np.fabs(dv) > MAX_SPAN)
        state = np.where(nodata, NODATA, MISS).astype(np.uint8)
        live = ~nodata
        assert (np.fabs(u0[live]) < 2.0 ** 52).all() and (np.fabs(v0[live]) < 2.0 ** 52).all()      # the line indices are integers
        i = np.where(live, np.floor(u0), 0.0).astype(np.int64)
        j = np.where(live, np.floor(v0), 0.0).astype(np.int64)
        si, sj = np.where(du > 0, 1, -1), np.where(dv > 0, 1, -1)
        lam_in = np.zeros(R, dtype=f8)
        step = 0
        while live.any():
            at = np.flatnonzero(live)
            ii, jj, du_, dv_, dz_ = i[at], j[at], du[at], dv[at], dz[at]
            lam_u = np.where(du_ == 0, INF, (np.where(du_ > 0, ii + 1, ii).astype(f8) - u0[at]) / du_)
            lam_v = np.where(dv_ == 0, INF, (np.where(dv_ > 0, jj + 1, jj).astype(f8) - v0[at]) / dv_)
            m = np.fmin(lam_u, lam_v)
            lam_out = np.fmax(lam_in[at], np.fmin(m, f8(1.0)))
            inside = (ii >= 0) & (ii < W) & (jj >= 0) & (jj < H)
            h = np.full(at.size, np.nan)
            h[inside] = cells[jj[inside], ii[inside]]
            hole = inside & np.isnan(h)
            nan_cells[at[hole]] += 1
            z_in, z_out = z0[at] + lam_in[at] * dz_, z0[at] + lam_out * dz_
            tested = inside & ~hole & ~(np.fmin(z_in, z_out) > zmax)
            below = tested & le(z_in, h)
            on_top = tested & ~below & le(z_out, h)
            lam_top = np.fmax(lam_in[at], np.fmin((h - z0[at]) / dz_, lam_out)) if top == "solve" else lam_out
            lam = np.where(below, lam_in[at], lam_top)
            hit = below | on_top
            state[at[hit]] = np.where(below, BELOW if step == 0 else WALL, TOP)[hit]
            depth[at[hit]] = (near[at] + lam * (far[at] - near[at])).astype(np.float32)[hit]
            cell[at[hit]] = (jj * W + ii).astype(np.int32)[hit]
            go = ~hit & ~(m >= 1)                                        # the others are done: a hit, or a MISS at the far end
            move_u, move_v = go & (lam_u == m), go & (lam_v == m)
            if tie == "u":
                move_v &= ~move_u
            i[at[move_u]] += si[at[move_u]]
            j[at[move_v]] += sj[at[move_v]]
            ii, jj = i[at], j[at]
            away = ((ii < 0) & (du_ < 0)) | ((ii >= W) & (du_ > 0)) | ((jj < 0) & (dv_ < 0)) | ((jj >= H) & (dv_ > 0))
            go &= ~away
            lam_in[at[go]] = lam_out[go]
            live[at] = go
            step += 1
            assert step <= 2 * int(MAX_SPAN) + 8
    counts = np.array([(state == k).sum() for k in range(5)], dtype=np.int64)
    return depth, state, cell, nan_cells, counts


def surface_prior_statement(cast, weight=1.0, stdscale=1.0, margin=1e-4, std_span=0.0):
    """surface_priors' columns from the statement's outputs -> depths (R, 2) float32, valid_depth (R,), depth_std (R,) float32."""
    depth, state, _, nan_cells, _ = cast
    valid = ((state == TOP) | (state == WALL)) & (nan_cells == 0)
    kept = depth[valid].astype(np.float64)
    mean = np.float32(kept.sum() / max(1.0, float(valid.sum())))
    w = np.float32(weight)
    std = np.float32((np.float32(stdscale) * (np.float32(1.0) - w) + np.float32(margin)) * np.float32(std_span))
    depths = np.stack([np.where(valid, depth, mean), np.where(valid, w, np.float32(0.0))], -1).astype(np.float32)
    return depths, valid.astype(np.float32), np.where(valid, std, np.float32(0.0)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------- cases
RES = V.RES
ORIGINS = {"dyadic": (1024.0, 2048.0), "utm": (368000.25, 3357000.75)}            # (xoff, yoff): the grid's north-west corner


def frame_of(dsm, xoff, yoff, res=RES, rng=40.0):
    """The frame of a scene over a grid: the centre over the grid's middle at 20 m, range `rng`."""
    H, W = dsm.shape
    return (xoff + 0.5 * W * res, yoff - 0.5 * H * res, 20.0), float(rng)


def view(targets, elevation, azimuth, center, rng, z_ref, z_near, z_far, z_origin=None, cols=8):
    """Parallel rays of a view at (elevation, azimuth) of the SENSOR (V.direction's convention) through the world points `targets`
    (n, 2) = (east, north) on the plane z_ref: origins on the plane z_origin (default 20 m above z_near), near on the plane z_near,
    far 5 % beyond the plane z_far -> (n, cols) float32 rows (o, d, near, far, zeros), formed in float64 and rounded once."""
    targets = np.asarray(targets, dtype=np.float64).reshape(-1, 2)
    up = V.direction(elevation, azimuth)                  # from the ground towards the sensor
    z_origin = z_near + 20.0 if z_origin is None else z_origin
    t = (z_origin - z_ref) / up[2]                        # metres along the ray between the two planes
    world = np.concatenate([targets, np.full((len(targets), 1), float(z_ref))], -1) + up * t
    rays = np.zeros((len(targets), cols), dtype=np.float64)
    rays[:, 0:3] = (world - np.asarray(center)) / rng
    rays[:, 3:6] = -up
    rays[:, 6] = (z_origin - z_near) / up[2] / rng
    rays[:, 7] = (z_origin - z_far) / up[2] / rng * 1.05
    return rays.astype(np.float32)


def lattice(n, e0, n0, step):
    """n x n world points, row-major from the north-west: east e0 + step c, north n0 - step r."""
    rr, cc = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return np.stack([e0 + step * cc.reshape(-1), n0 - step * rr.reshape(-1)], -1)


BLOCK_COUNTS = {"top": 1898, "wall": 406, "roof": 225}     # the statement's counts on block_view, at both origins


def block_view(origin="dyadic"):
    """The block scene under a 48 x 48 view at elevation 60, azimuth 135: the rays aim at a lattice of 0.55 m on the 10 m plane
    inside the grid; near on the 40 m plane - 17 m to the south-east, so the south-eastern rays start outside the grid - far 5 %
    beyond the 5 m plane.  -> dsm, rays, center, rng, xoff, yoff."""
    dsm = V.block_scene()
    xoff, yoff = ORIGINS[origin]
    center, rng = frame_of(dsm, xoff, yoff)
    rays = view(lattice(48, xoff + 3.0, yoff - 3.0, 0.55), 60.0, 135.0, center, rng, z_ref=10.0, z_near=40.0, z_far=5.0)
    depth, state, cell, nan_cells, counts = cast_statement(rays, center, rng, dsm, xoff, yoff, RES)
    roof = int(((state == TOP) & (dsm.reshape(-1)[np.maximum(cell, 0)] == 30.0)).sum())
    assert counts[TOP] >= 1500 and counts[WALL] >= 400 and roof >= 100 and counts[TOP] + counts[WALL] == 48 * 48     # on the inputs
    u_start = ((rays[:, 0].astype(np.float64) + rays[:, 3].astype(np.float64) * rays[:, 6]) * rng + center[0] - xoff) / RES
    assert (u_start >= 64).sum() >= 100                    # rays that start east of the grid
    return dsm, rays, center, rng, xoff, yoff


def scatter_view(R, dsm, xoff, yoff, elevation, azimuth, seed=0, res=RES, cols=8):
    """R rays through random points over and around a grid (a tenth of its extent beyond every edge), descending from 25 m above
    its highest finite cell to 5 m below its lowest; from R = 63 on, rows 10 to 12 are a NaN origin, an infinite direction and a
    ray longer than the span cap.  -> rays, center, rng."""
    rng_ = np.random.default_rng(seed * 7919 + R)
    H, W = dsm.shape
    known = dsm[np.isfinite(dsm)]
    lo, hi = (float(known.min()), float(known.max())) if known.size else (0.0, 1.0)
    center, rng = frame_of(dsm, xoff, yoff, res)
    t = np.stack([xoff + rng_.uniform(-0.1 * W, 1.1 * W, R) * res, yoff - rng_.uniform(-0.1 * H, 1.1 * H, R) * res], -1)
    rays = view(t, elevation, azimuth, center, rng, z_ref=0.5 * (lo + hi), z_near=hi + 25.0, z_far=lo - 5.0, cols=cols)
    if R >= 63:
        rays[10, 1], rays[11, 4], rays[12, 7] = np.nan, np.inf, np.float32(3.0e6)
    return rays, center, rng


def unit_frame():
    return (0.0, 0.0, 0.0), 1.0


def ray(o, d, near, far):
    return np.array([list(o) + list(d) + [near, far]], dtype=np.float32)


def graze_case():
    """1 x 9 cells of 10.0 with cell 4 at 12.25; the ray leaves cell 4 at lam = 0.5625 with z_out == 12.25 == h exactly: TOP at depth
    4.5 under <=, a MISS under <.  -> dsm, rays, center, rng, xoff, yoff."""
    row = np.full((1, 9), 10.0, dtype=np.float32)
    row[0, 4] = 12.25
    return (row, ray((0.25, 0.25, 14.5), (0.5, 0.0, -0.5), 0.0, 8.0)) + unit_frame() + (0.0, 0.5)


def corner_case():
    """3 x 3 cells of 1.0 with +inf at (0, 1) and (1, 0); the ray runs down the diagonal through the corners (1, 1) and (2, 2) and
    ends above the ground: a MISS.  Moving along u alone on the tie enters (0, 1): WALL at cell 1."""
    dsm = np.full((3, 3), 1.0, dtype=np.float32)
    dsm[0, 1] = dsm[1, 0] = np.inf
    return (dsm, ray((0.25, 1.25, 5.0), (0.25, -0.25, -0.5), 0.0, 4.0)) + unit_frame() + (0.0, 1.5)


def closed_form_cases():
    """Three rays over the block scene in the unit frame, xoff = 0, yoff = 32, every number dyadic so the hand-worked depth is exact.
    Each runs west along the row north = 16.25 (j = 31).  -> dsm, rays (3, 8), center, rng, xoff, yoff, [(state, depth, cell)]."""
    rays = np.concatenate([
        ray((26.25, 16.25, 40.0), (-0.5, 0.0, -0.5), 0.0, 64.0),       # z = 30 at s = 20 over east 16.25: the roof, cell i = 32
        ray((30.25, 16.25, 36.0), (-0.5, 0.0, -0.5), 0.0, 64.0),       # the roof's east wall (east 20) at s = 20.5, z = 25.75: cell i = 39
        ray((21.25, 16.25, 70.0), (-0.125, 0.0, -0.5), 0.0, 128.0),    # clears the roof (z = 33 over east 12), ground at s = 120, east 6.25
    ])
    want = [(TOP, 20.0, 31 * 64 + 32), (WALL, 20.5, 31 * 64 + 39), (TOP, 120.0, 31 * 64 + 12)]
    return (V.block_scene(), rays) + unit_frame() + (0.0, 32.0, want)


def single_cases():
    """Engineered rays over a 4 x 5 grid of 0.5 m cells at 2.0 (xoff = 0, yoff = 2, unit frame) with a NaN cell at (1, 2) and (1, 3):
    name -> (ray, (state, depth or None, cell, nan_cells))."""
    dsm = np.full((4, 5), 2.0, dtype=np.float32)
    dsm[1, 2] = dsm[1, 3] = np.nan
    nan = float("nan")
    cases = {
        "nadir": (ray((0.75, 1.75, 6.0), (0.0, 0.0, -1.0), 0.0, 8.0), (TOP, 4.0, 1, 0)),                    # du == dv == 0
        "nadir_short": (ray((0.75, 1.75, 6.0), (0.0, 0.0, -1.0), 0.0, 3.0), (MISS, None, -1, 0)),
        "below": (ray((0.75, 1.75, 1.5), (0.5, 0.0, 0.25), 0.0, 2.0), (BELOW, 0.0, 1, 0)),                  # starts under the surface
        "below_at_near": (ray((0.75, 1.75, 3.0), (0.0, 0.0, -1.0), 1.0, 4.0), (BELOW, 1.0, 1, 0)),          # z_in == h at the start: <=
        "miss_west": (ray((0.75, 1.25, 3.0), (-0.5, 0.0, 0.0), 0.0, 8.0), (MISS, None, -1, 0)),
        "miss_east": (ray((0.75, 1.75, 3.0), (0.5, 0.0, 0.0), 0.0, 8.0), (MISS, None, -1, 0)),
        "miss_north": (ray((0.75, 1.75, 3.0), (0.0, 0.5, 0.0), 0.0, 8.0), (MISS, None, -1, 0)),
        "miss_south": (ray((0.75, 1.75, 3.0), (0.0, -0.5, 0.0), 0.0, 8.0), (MISS, None, -1, 0)),
        "far_away": (ray((1.0e9, 1.75, 3.0), (0.5, 0.0, -0.5), 0.0, 1.0), (MISS, None, -1, 0)),             # both ends east of the grid
        "from_outside": (ray((-1.25, 1.75, 4.0), (0.5, 0.0, -0.5), 0.0, 16.0), (TOP, 4.0, 1, 0)),           # enters from the west at z = 2.75
        "nan_ray": (ray((nan, 1.75, 3.0), (0.5, 0.0, 0.0), 0.0, 8.0), (NODATA, None, -1, 0)),
        "nan_far": (ray((0.75, 1.75, 3.0), (0.5, 0.0, 0.0), 0.0, nan), (NODATA, None, -1, 0)),
        "span_cap": (ray((0.75, 1.75, 3.0), (0.5, 0.0, 0.0), 0.0, 65537.0), (NODATA, None, -1, 0)),         # du = 65537 cells
        "span_at_cap": (ray((0.75, 1.75, 3.0), (0.5, 0.0, 0.0), 0.0, 65536.0), (MISS, None, -1, 0)),        # du = 65536: walked
        # along row 1 eastwards, descending from 4 m: over the NaN cells (1, 2) and (1, 3) it is below 3.25 m, and it reaches 2.0 in
        # the middle of cell (1, 4): the NaN cells are passed, counted and not hit
        "nan_cells": (ray((0.25, 1.25, 4.0), (0.5, 0.0, -0.5), 0.0, 8.0), (TOP, 4.0, 1 * 5 + 4, 2)),
        "nan_then_out": (ray((0.25, 1.25, 3.0), (0.5, 0.0, 0.0), 0.0, 8.0), (MISS, None, -1, 2)),
    }
    return dsm, cases, (0.0, 0.0, 0.0), 1.0, 0.0, 2.0


GRID_SHAPES = [(1, 1), (1, 9), (3, 3), (7, 9), (33, 65), (64, 64), (40, 257)]
ELEVATIONS = [90.0, 80.0, 45.0, 12.0]
AZIMUTHS = [0.0, 17.0, 135.0, 263.0]
SIZES = [1, 63, 64, 65, 257, 2304]


def grid_case(shape):
    """The grid of one of GRID_SHAPES: the block scene at 64 x 64, V.relief with its NaN, +-inf and -0.0 cells elsewhere."""
    if shape == (64, 64):
        return V.block_scene()
    if shape[0] * shape[1] < 8:
        return V.relief(*shape, seed=shape[0] * 1000 + shape[1], nan=0.0, specials=False, low=3.0)
    return V.relief(*shape, seed=shape[0] * 1000 + shape[1])
