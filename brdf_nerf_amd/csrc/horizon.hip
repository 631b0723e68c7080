// Horizon and sky-view factor of a surface model: from a start on or above a height grid, march along a horizontal azimuth and keep
// the steepest slope (h - z0) / run met on the way - the tangent of the horizon's elevation, floored at 0 - then average
// 1 / (1 + slope^2) = cos^2 of that elevation over the azimuths: the view factor of an isotropic sky for a level surface.
// include/brdfnerf_hip.h ("Horizon and sky view over a surface model") states the rule operation by operation.  It has NO upstream
// counterpart, so the rule is this project's own and there is nothing to check it against but its statement - and visibility.hip's
// march, which answers "is this start shadowed at elevation e" one elevation at a time where the horizon answers it for all.
//
//   grid_horizon_kernel    the starts are the cells of rows [row0, row1): (i + 0.5, j + 0.5, dsm[j][i])
//   points_horizon_kernel  the starts are points (east, north, altitude): surface_cell::point_cell's two quotients, unfloored
//   sky_view_kernel        acc[c] += 1 / (1 + slope[k][c]^2), k ascending, one addition at a time; on the last tile svf and its sums
//
// Both horizon kernels call ONE march (march): float64, every operation rounded on its own, the step coordinate always
// u0 + (double)t su and never a running sum, the update s > best strict (the first cell in ascending t wins a tie, a NaN cell never
// raises the horizon).  The start cell is never tested.  Unlike the shadow march it does not end at the first obstacle: it ends when
// it leaves the grid, after max_steps, or when (zmax - z0) / run <= best, which no later cell can beat (the header has the proof;
// the test is valid at any step and is made once per batch of steps).
//
// The mapping is visibility.hip's, measured there.  A block of 256 lanes owns a tile of 64 x 4 starts and ONE azimuth (point mode: 256
// consecutive points).  A wave is a strip of 64 cells of one row; all its lanes share (su, sv), one of which is +-1, so at step t the
// strip reads 64 consecutive cells of one row.  The azimuths of a launch travel as kernel arguments (HOR_DIRS of them, 16 bytes
// each); the entries check every azimuth on the host before the first launch and a call of D azimuths is ceil(D / HOR_DIRS) launches.
//
// slope and hit are plain stores of the lane's own start; acc is a plain read-modify-write of the lane's own cell.  sums: the lanes'
// (llrint(v 2^30), 1, 0) or (0, 0, 1) are added over the block (block_sums.h) and ONE integer atomic per counter and block goes out.
// There is no float atomic: every bit depends on the grid, the starts and the azimuths alone.
//
// As the compiler reports them for gfx950: grid_horizon_kernel 72 VGPRs, points_horizon_kernel 72 VGPRs, no LDS, 7 waves per SIMD;
// sky_view_kernel 26 VGPRs, 32 B of LDS, 8 waves per SIMD; no scratch in any.
// The march takes HOR_BATCH = 8 steps at a time (see march).  Its first form took one step per iteration and tested the early exit at
// each (38 VGPRs): there the exit made the march 6 to 40 % SLOWER than the same loop without it, and testing it at every 8th step
// changed nothing - not the division but the chain load -> best -> exit -> next load was the cost, the loop without the exit being
// free to run its loads ahead.  With the loads of a batch issued together and the exit tested once per batch, 2048 x 2048 cells under
// D = 64 take 248.0 ms against 320.1 ms, and the exit now buys 21 % there (315.0 ms without it), nothing at 512 x 512 and costs 3 to 5 %
// under max_dist = 100 m.  profiles/horizon_throughput.txt holds every timing of both forms.
// BN_HORIZON_NO_ZMAX (diag.h: a -D of profiles/horizon_throughput.py's variant library, never of the build) drops the early exit, to
// price it.
#include <cmath>
#include "common.h"
#include "block_sums.h"
#include "brdfnerf_hip.h"
// every float64 operation below is rounded on its own (see above); the build also passes -ffp-contract=off for this file
#pragma clang fp contract(off)

namespace {

constexpr int HOR_TILE_W = 64;                 // a wave: 64 cells of one row
constexpr int HOR_TILE_H = 4;                  // a block: four rows
constexpr int HOR_BLOCK = HOR_TILE_W * HOR_TILE_H;
constexpr int HOR_DIRS = 64;                   // azimuths per launch (1024 bytes of kernel arguments)
constexpr int64_t HOR_MAX_CELLS = (int64_t)1 << 30;
constexpr double SVF_FIX = 1073741824.0;       // 2^30: svf lies in [0, 1]
constexpr int HOR_BATCH = 8;                   // steps whose loads go out together; the early exit is tested once per batch

struct Azimuths {
  double d[HOR_DIRS][2];
};

struct GridView {
  const float *dsm;
  int32_t H, W, steps;                         // steps = min(max(W, H), max_steps)
  double res, zmax;
};

struct Step {
  double su, sv, L;
};

__device__ __forceinline__ Step step_of(const double *d, double res) {
  Step s;
  const double a = fmax(fabs(d[0]), fabs(d[1]));       // > 0: the entries refuse (0, 0)
  s.su = d[0] / a;
  s.sv = -(d[1] / a);
  s.L = sqrt(s.su * s.su + s.sv * s.sv) * res;
  return s;
}

__device__ __forceinline__ bool inside(const GridView &G, double u, double v) {
  return u >= 0.0 && u < (double)G.W && v >= 0.0 && v < (double)G.H;
}

// the march of one start that has data -> best, the steepest slope met (0 if none rises above the start); hit = its cell, or -1.
// HOR_BATCH steps at a time: their cells are found first (none of that depends on a loaded value), their HOR_BATCH loads go out
// together, and only then are the slopes compared in ascending t - the rule's order.  A step outside the grid, or beyond max_steps,
// loads cell 0 instead and ends the march when its turn comes.
__device__ __forceinline__ double march(const GridView &G, const Step &s, double u0, double v0, double z0, int32_t &hit) {
  double best = 0.0;
  hit = -1;
#ifndef BN_HORIZON_NO_ZMAX
  const double top = G.zmax - z0;
#endif
  for (int t0 = 1; t0 <= G.steps; t0 += HOR_BATCH) {
#ifndef BN_HORIZON_NO_ZMAX
    // no cell is above zmax: from step t0 on nothing can be strictly steeper.  Valid at any step, so tested once per batch
    if (top / ((double)t0 * s.L) <= best) break;
#endif
    int32_t c[HOR_BATCH];
    float h[HOR_BATCH];
#pragma unroll
    for (int q = 0; q < HOR_BATCH; ++q) {
      const double tt = (double)(t0 + q);
      const double ut = u0 + tt * s.su, vt = v0 + tt * s.sv;
      const bool in = t0 + q <= G.steps && inside(G, ut, vt);
      c[q] = in ? (int32_t)floor(vt) * G.W + (int32_t)floor(ut) : -1;      // inside: 0 <= c < H W <= 2^30
    }
#pragma unroll
    for (int q = 0; q < HOR_BATCH; ++q) h[q] = G.dsm[c[q] < 0 ? 0 : c[q]];
    bool left = false;
#pragma unroll
    for (int q = 0; q < HOR_BATCH; ++q) {
      left = left || c[q] < 0;
      if (!left) {
        const double sl = ((double)h[q] - z0) / ((double)(t0 + q) * s.L);
        if (sl > best) {                         // strict; false for a NaN cell
          best = sl;
          hit = c[q];
        }
      }
    }
    if (left) break;
  }
  return best;
}

__global__ __launch_bounds__(HOR_BLOCK)
void grid_horizon_kernel(const GridView G, const Azimuths A, int row0, int row1, int tiles_x, float *__restrict__ slope,
                         int32_t *__restrict__ hit) {
  const int tid = (int)threadIdx.x, k = (int)blockIdx.y;
  const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)tiles_x);
  const int i = tx * HOR_TILE_W + (tid & (HOR_TILE_W - 1));
  const int64_t j = (int64_t)row0 + (int64_t)ty * HOR_TILE_H + (tid >> 6);
  if (i >= G.W || j >= row1) return;
  const int64_t c = j * G.W + i;
  const double z0 = (double)G.dsm[c];
  int32_t h = -1;
  float out = __builtin_nanf("");
  if (isfinite(z0)) out = (float)march(G, step_of(A.d[k], G.res), (double)i + 0.5, (double)j + 0.5, z0, h);
  const int64_t at = (int64_t)k * ((int64_t)G.H * G.W) + c;
  slope[at] = out;
  if (hit) hit[at] = h;
}

__global__ __launch_bounds__(HOR_BLOCK)
void points_horizon_kernel(const GridView G, const Azimuths A, const double *__restrict__ enz, int64_t R, double xoff, double yoff,
                           float *__restrict__ slope, int32_t *__restrict__ hit) {
  const int k = (int)blockIdx.y;
  const int64_t r = (int64_t)blockIdx.x * HOR_BLOCK + threadIdx.x;
  if (r >= R) return;
  const double u0 = (enz[3 * r] - xoff) / G.res, v0 = (yoff - enz[3 * r + 1]) / G.res, z0 = enz[3 * r + 2];
  int32_t h = -1;
  float out = __builtin_nanf("");
  if (isfinite(u0) && isfinite(v0) && isfinite(z0) && inside(G, u0, v0)) out = (float)march(G, step_of(A.d[k], G.res), u0, v0, z0, h);
  const int64_t at = (int64_t)k * R + r;
  slope[at] = out;
  if (hit) hit[at] = h;
}

// cells [c0, c1): acc += the n planes' terms in ascending k; with svf (the last tile) also svf = (float)(acc / D) and the sums
__global__ __launch_bounds__(HOR_BLOCK)
void sky_view_kernel(const float *__restrict__ slope, int n, int64_t cells, int64_t c0, int64_t c1, double *__restrict__ acc, double D,
                     float *__restrict__ svf, unsigned long long *__restrict__ sums) {
  __shared__ long long red[4];
  const int64_t c = c0 + (int64_t)blockIdx.x * HOR_BLOCK + threadIdx.x;
  long long q = 0, cnt = 0, nans = 0;
  if (c < c1) {
    double a = acc[c];
    for (int k = 0; k < n; ++k) {
      const double s = (double)slope[(int64_t)k * cells + c];
      a = a + 1.0 / (1.0 + s * s);
    }
    acc[c] = a;
    if (svf) {
      const double v = a / D;
      svf[c] = (float)v;
      if (isnan(v)) {
        nans = 1;
      } else {
        q = llrint(v * SVF_FIX);
        cnt = 1;
      }
    }
  }
  if (!svf) return;                              // uniform over the block
  const long long s0 = block_sums::block_sum(q, red), s1 = block_sums::block_sum(cnt, red), s2 = block_sums::block_sum(nans, red);
  if (threadIdx.x == 0) {
    if (s0) atomicAdd(sums + 0, (unsigned long long)s0);
    if (s1) atomicAdd(sums + 1, (unsigned long long)s1);
    if (s2) atomicAdd(sums + 2, (unsigned long long)s2);
  }
}

// what both horizon entries refuse of the grid, the azimuths and the bounds; 0 or BN_EINVAL with the error set
int require_horizon(const char *who, const float *dsm, int32_t H, int32_t W, double res, const double *az, int32_t D, int32_t max_steps,
                    double zmax, const void *slope) {
  BN_REQUIRE(dsm && az && slope, "%s: null argument", who);
  BN_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= HOR_MAX_CELLS, "%s: grid %d x %d (H W from 1 to 2^30 cells)", who, H, W);
  BN_REQUIRE(D >= 1 && D <= BN_HORIZON_MAX_DIRS, "%s: D=%d azimuths outside [1, %d]", who, D, BN_HORIZON_MAX_DIRS);
  BN_REQUIRE(res > 0.0 && std::isfinite(res), "%s: resolution %g must be positive and finite", who, res);
  BN_REQUIRE(max_steps >= 1, "%s: max_steps %d must be at least 1", who, max_steps);
  BN_REQUIRE(!std::isnan(zmax), "%s: zmax is NaN", who);
  for (int32_t k = 0; k < D; ++k) {
    const double *d = az + 2 * (int64_t)k;
    BN_REQUIRE(std::isfinite(d[0]) && std::isfinite(d[1]) && (d[0] != 0.0 || d[1] != 0.0),
               "%s: azimuth %d = (%g, %g) must be finite and not (0, 0)", who, k, d[0], d[1]);
  }
  return 0;
}

Azimuths az_chunk(const double *az, int32_t k0, int32_t n) {
  Azimuths A;
  for (int k = 0; k < HOR_DIRS; ++k)
    for (int c = 0; c < 2; ++c) A.d[k][c] = k < n ? az[2 * (int64_t)(k0 + k) + c] : 1.0;
  return A;
}

GridView grid_view(const float *dsm, int32_t H, int32_t W, double res, int32_t max_steps, double zmax) {
  const int32_t side = W > H ? W : H;
  return GridView{dsm, H, W, max_steps < side ? max_steps : side, res, zmax};
}

}  // namespace

extern "C" int bn_grid_horizon(const float *dsm, int32_t H, int32_t W, double res, int32_t row0, int32_t row1, const double *az,
                               int32_t D, int32_t max_steps, double zmax, float *slope, int32_t *hit, void *stream) {
  if (int bad = require_horizon("grid_horizon", dsm, H, W, res, az, D, max_steps, zmax, slope)) return bad;
  BN_REQUIRE(0 <= row0 && row0 <= row1 && row1 <= H, "grid_horizon: rows [%d, %d) outside [0, %d)", row0, row1, H);
  if (row0 == row1) return 0;
  const GridView G = grid_view(dsm, H, W, res, max_steps, zmax);
  const int tiles_x = (W + HOR_TILE_W - 1) / HOR_TILE_W;
  const int64_t tiles = (int64_t)tiles_x * ((row1 - row0 + HOR_TILE_H - 1) / HOR_TILE_H);      // at most 2^28 + 2^24
  const int64_t plane = (int64_t)H * W;
  for (int32_t k0 = 0; k0 < D; k0 += HOR_DIRS) {
    const int32_t n = D - k0 < HOR_DIRS ? D - k0 : HOR_DIRS;
    grid_horizon_kernel<<<dim3((unsigned)tiles, (unsigned)n), HOR_BLOCK, 0, (hipStream_t)stream>>>(
        G, az_chunk(az, k0, n), row0, row1, tiles_x, slope + k0 * plane, hit ? hit + k0 * plane : nullptr);
    BN_LAUNCH_CHECK("grid_horizon");
  }
  return 0;
}

extern "C" int bn_points_horizon(const double *enz, int64_t R, const float *dsm, int32_t H, int32_t W, double xoff, double yoff,
                                 double res, const double *az, int32_t D, int32_t max_steps, double zmax, float *slope, int32_t *hit,
                                 void *stream) {
  if (int bad = require_horizon("points_horizon", dsm, H, W, res, az, D, max_steps, zmax, slope)) return bad;
  BN_REQUIRE(enz, "points_horizon: null argument");
  BN_REQUIRE(R >= 0 && R <= HOR_MAX_CELLS, "points_horizon: R=%lld points outside [0, 2^30]", (long long)R);
  BN_REQUIRE(std::isfinite(xoff) && std::isfinite(yoff), "points_horizon: grid origin (%g, %g) is not finite", xoff, yoff);
  if (R == 0) return 0;
  const GridView G = grid_view(dsm, H, W, res, max_steps, zmax);
  for (int32_t k0 = 0; k0 < D; k0 += HOR_DIRS) {
    const int32_t n = D - k0 < HOR_DIRS ? D - k0 : HOR_DIRS;
    points_horizon_kernel<<<dim3((unsigned)ceil_div64(R, HOR_BLOCK), (unsigned)n), HOR_BLOCK, 0, (hipStream_t)stream>>>(
        G, az_chunk(az, k0, n), enz, R, xoff, yoff, slope + k0 * R, hit ? hit + k0 * R : nullptr);
    BN_LAUNCH_CHECK("points_horizon");
  }
  return 0;
}

extern "C" int bn_sky_view(const float *slope, int32_t n, int64_t cells, int64_t c0, int64_t c1, double *acc, int32_t D, float *svf,
                           long long *sums, void *stream) {
  BN_REQUIRE(slope && acc, "sky_view: null argument");
  BN_REQUIRE(!svf || sums, "sky_view: svf without sums");
  BN_REQUIRE(n >= 1 && n <= BN_HORIZON_MAX_DIRS, "sky_view: n=%d planes outside [1, %d]", n, BN_HORIZON_MAX_DIRS);
  BN_REQUIRE(D >= 1 && D <= BN_HORIZON_MAX_DIRS, "sky_view: D=%d azimuths outside [1, %d]", D, BN_HORIZON_MAX_DIRS);
  BN_REQUIRE(cells >= 1 && cells <= HOR_MAX_CELLS, "sky_view: %lld cells outside [1, 2^30]", (long long)cells);
  BN_REQUIRE(0 <= c0 && c0 <= c1 && c1 <= cells, "sky_view: cells [%lld, %lld) outside [0, %lld)", (long long)c0, (long long)c1,
             (long long)cells);
  if (c0 == c1) return 0;
  sky_view_kernel<<<dim3((unsigned)ceil_div64(c1 - c0, HOR_BLOCK)), HOR_BLOCK, 0, (hipStream_t)stream>>>(
      slope, n, cells, c0, c1, acc, (double)D, svf, reinterpret_cast<unsigned long long *>(sums));
  BN_LAUNCH_CHECK("sky_view");
  return 0;
}
