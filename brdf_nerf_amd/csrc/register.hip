// The xy registration of a DSM on its ground truth (dsmr.compute_shift(scaling=False) / apply_shift as sat_utils.py:239-246 call
// them) on the device: the step of the evaluation's line (eval.py:467-479) between the rasteriser of world.hip and the MAEs.
//
// bn_grid_halve      one level of dsmr.downsample2x: the mean of the finite cells of a 2 x 2 box, float64, a lane per output cell.
// bn_ncc_moments     the six INTEGER moments (N, Su, Sv, Suu, Svv, Suv) of the valid pairs u[j][i], v[j + dy][i + dx] for every
//                    shift of a (2r + 1)^2 window, altitudes quantised to q = rint((z - pivot) 2^k) in [0, 2^20].  The host forms the
//                    correlation from them in Python integers (dsmr.mean_std / ncc / compute_ncc).
// bn_dsm_shift_diff  dsmr.apply_shift_ and the float32 difference of sat_utils.py:246 per cell, and integer (sum, count) pairs of
//                    |diff| over all / inside / outside cells (the nanmean of :340 and MaskDoD, :344-345).
//
// As in world.hip and metrics.hip every float64 operation is rounded on its own (the build passes -ffp-contract=off for this file
// and it carries the pragma) and every sum is an integer: the results' bits do not depend on the block order, on how the rows
// are split over launches or on how many devices shared the grid.  There is no float atomic in this file.
//
// bn_ncc_moments, the mapping.  One block of 256 lanes owns a 32 x 32 tile of u.  It quantises the tile and the v tile with its
// r-cell halo ONCE into LDS as int32, -1 for a missing cell.  Then lanes own SHIFTS, not cells: lane (g, s) walks 32 / G rows
// of the tile for shift s, G the largest power of two with G (2r + 1)^2 <= 256 (r = 5: 121 shifts, G = 2, 242 lanes busy; r = 8:
// 289 shifts, G = 1 and the lanes take a second shift).  Per cell a lane reads u once (every lane of a row group reads the same
// word: a broadcast) and v once, and issues three 32-bit adds (N, Su, Sv: at most 1024 2^20 = 2^30 per tile) and three 64-bit
// multiply-adds from 32-bit operands (v_mad_u64_u32).  No cross-lane reduction per shift; the G row groups are combined through
// LDS and ONE integer atomic goes out per (shift, moment) per block (zero sums send none).
// LDS banks: the v tile's row pitch is 33 + 2r words, which is 2r + 1 modulo 32.  Lanes of one row group read word
// (lr + sy) pitch + lc + sx, that is (sy (2r + 1) + sx) + const = s + const modulo 32: the 32 lanes of a ds_read_b32 group touch
// 32 distinct banks at every r.  (A wave that straddles two row groups reads two such runs 32 / G rows apart and can meet
// 2-way; at r = 5 that is one wave of four.)
#include <cmath>
#include "common.h"
#include "brdfnerf_hip.h"
#include "block_sums.h"
// every float64 operation below is rounded on its own (see above); the build also passes -ffp-contract=off for this file
#pragma clang fp contract(off)

namespace {

constexpr int TILE = 32;
constexpr int MAXR = BN_NCC_MAX_RANGE;
constexpr int VROWS = TILE + 2 * MAXR;                  // 48
constexpr int VPITCH = TILE + 2 * MAXR + 1;             // 49: the largest pitch, 33 + 2r
constexpr int MAXSHIFTS = (2 * MAXR + 1) * (2 * MAXR + 1);
constexpr double QMAX = 1048576.0;                      // 2^20: the largest quantum
constexpr double MAE_FIX = 1048576.0;                   // 2^20
constexpr double MAE_LIMIT = 2097152.0;                 // 2^21 m: |diff| 2^20 < 2^41, 2^22 cells of it stay below 2^63

__global__ __launch_bounds__(256)
void grid_halve_kernel(const double *__restrict__ src, int H, int W, int Ho, int Wo, double *__restrict__ dst) {
  const int cell = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (cell >= Ho * Wo) return;
  const int J = cell / Wo, I = cell - J * Wo;
  // upstream writes out[j / 2][i / 2] for EVERY input cell and the last write wins: the box whose corner is the last (j, i) of
  // the output cell, (2J + 1, 2I + 1), or (2J, .) / (., 2I) when that is past the edge
  const int j = 2 * J + 1 < H ? 2 * J + 1 : 2 * J, i = 2 * I + 1 < W ? 2 * I + 1 : 2 * I;
  double s = 0.0;
  int n = 0;
  for (int k = 0; k < 2; ++k)                  // column offset outer, row offset inner: (j, i), (j + 1, i), (j, i + 1), (j + 1, i + 1)
    for (int l = 0; l < 2; ++l) {
      if (j + l >= H || i + k >= W) continue;
      const double t = src[(int64_t)(j + l) * W + (i + k)];
      if (isfinite(t)) {
        s = s + t;
        n += 1;
      }
    }
  dst[cell] = n ? s / (double)n : __builtin_nan("");
}

// the quantum of an altitude, -1 for a missing cell; a finite one outside [0, 2^20] is missing too and counted
__device__ __forceinline__ int quantum(double z, double pivot, double scale, int &skipped) {
  if (!isfinite(z)) return -1;
  const double t = rint((z - pivot) * scale);
  if (!(t >= 0.0 && t <= QMAX)) {
    skipped += 1;
    return -1;
  }
  return (int)t;
}

__global__ __launch_bounds__(256)
void ncc_moments_kernel(const double *__restrict__ u, const double *__restrict__ v, int H, int W, double pivot, double scale, int dx0,
                        int dy0, int r, int row0, int row1, unsigned long long *__restrict__ sums,
                        unsigned long long *__restrict__ skipped) {
  __shared__ int su[TILE * TILE];
  __shared__ int sv[VROWS * VPITCH];
  __shared__ long long red[MAXSHIFTS * 6];
  __shared__ long long wred[4];
  const int tid = (int)threadIdx.x;
  const int side = 2 * r + 1, nsh = side * side, ext = TILE + 2 * r, pitch = ext + 1;
  const int tr0 = row0 + (int)blockIdx.y * TILE, tc0 = (int)blockIdx.x * TILE;
  int skip = 0;
  for (int i = tid; i < TILE * TILE; i += 256) {
    const int j = tr0 + (i >> 5), c = tc0 + (i & 31);
    int q = -1;
    if (j < row1 && c < W) {
      q = quantum(u[(int64_t)j * W + c], pivot, scale, skip);
      // `skipped` counts every cell of u AND of v in the rows of the launch once: v's at the tile's own coordinates, not in the
      // halo that several blocks stage
      (void)quantum(v[(int64_t)j * W + c], pivot, scale, skip);
    }
    su[i] = q;
  }
  for (int i = tid; i < ext * ext; i += 256) {
    const int lr = i / ext, lc = i - lr * ext;
    const int j = tr0 + lr + dy0 - r, c = tc0 + lc + dx0 - r;
    int q = -1, unused = 0;
    if (j >= 0 && j < H && c >= 0 && c < W) q = quantum(v[(int64_t)j * W + c], pivot, scale, unused);
    sv[lr * pitch + lc] = q;
  }
  __syncthreads();
  int G = 1;
  while (G < TILE && 2 * G * nsh <= 256) G *= 2;
  const int rows_per = TILE / G;
  for (int w = tid; w < G * nsh; w += 256) {
    const int g = w / nsh, s = w - g * nsh;
    const int sy = s / side, sx = s - sy * side;           // scan order: dy outer, dx inner
    uint32_t n = 0, a = 0, b = 0;
    unsigned long long aa = 0, bb = 0, ab = 0;
    for (int lr = g * rows_per; lr < (g + 1) * rows_per; ++lr) {
      const int *pu = su + lr * TILE, *pv = sv + (lr + sy) * pitch + sx;
#pragma unroll 8
      for (int lc = 0; lc < TILE; ++lc) {
        const int qu = pu[lc], qv = pv[lc];
        const bool ok = (qu | qv) >= 0;                    // both present
        const uint32_t x = ok ? (uint32_t)qu : 0u, y = ok ? (uint32_t)qv : 0u;
        n += ok ? 1u : 0u;
        a += x;
        b += y;
        aa += (unsigned long long)x * x;
        bb += (unsigned long long)y * y;
        ab += (unsigned long long)x * y;
      }
    }
    long long *o = red + (int64_t)w * 6;
    o[0] = n; o[1] = a; o[2] = b; o[3] = (long long)aa; o[4] = (long long)bb; o[5] = (long long)ab;
  }
  __syncthreads();
  for (int idx = tid; idx < nsh * 6; idx += 256) {
    long long t = 0;
    for (int g = 0; g < G; ++g) t += red[g * nsh * 6 + idx];
    if (t != 0) atomicAdd(sums + idx, (unsigned long long)t);
  }
  const long long sk = block_sums::block_sum(skip, wred);
  if (tid == 0 && sk != 0) atomicAdd(skipped, (unsigned long long)sk);
}

__global__ __launch_bounds__(256)
void dsm_shift_diff_kernel(const float *__restrict__ pred, const float *__restrict__ gt, int H, int W, int dx, int dy, double b,
                           const uint8_t *__restrict__ mask, float *__restrict__ rdsm, float *__restrict__ diff,
                           unsigned long long *__restrict__ sums) {
  __shared__ long long red[4];
  const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
  long long q = 0, n = 0;
  bool inside = true;
  if (cell < (int64_t)H * W) {
    const int j = (int)(cell / W), i = (int)(cell - (int64_t)j * W);
    const int sj = j + dy, si = i + dx;
    float rz = __builtin_nanf("");
    if (sj >= 0 && sj < H && si >= 0 && si < W) rz = (float)((double)pred[(int64_t)sj * W + si] + b);
    const float d = (float)((double)rz - (double)gt[cell]);
    if (rdsm) rdsm[cell] = rz;
    if (diff) diff[cell] = d;
    const double ad = fabs((double)d);
    if (ad < MAE_LIMIT) {                                  // NaN cells are left out (nanmean); so is what would overflow the sum
      q = llrint(ad * MAE_FIX);
      n = 1;
    }
    inside = !mask || mask[cell] != 0;
  }
  block_sums::masked_sums6(q, n, inside, red, sums);
}

}  // namespace

extern "C" int bn_grid_halve(const double *src, int32_t H, int32_t W, double *dst, void *stream) {
  BN_REQUIRE(src && dst, "grid_halve: null argument");
  BN_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= BN_NCC_MAX_CELLS, "grid_halve: grid %d x %d (1 to 2^22 cells)", H, W);
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  grid_halve_kernel<<<(unsigned)ceil_div64((int64_t)Ho * Wo, 256), 256, 0, (hipStream_t)stream>>>(src, H, W, Ho, Wo, dst);
  BN_LAUNCH_CHECK("grid_halve");
  return 0;
}

extern "C" int bn_ncc_moments(const double *u, const double *v, int32_t H, int32_t W, double pivot, int32_t k, int32_t dx0, int32_t dy0,
                              int32_t r, int32_t row0, int32_t row1, long long *sums, long long *skipped, void *stream) {
  BN_REQUIRE(u && v && sums && skipped, "ncc_moments: null argument");
  BN_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= BN_NCC_MAX_CELLS, "ncc_moments: grid %d x %d (1 to 2^22 cells)", H, W);
  BN_REQUIRE(r >= 0 && r <= BN_NCC_MAX_RANGE, "ncc_moments: r=%d outside [0, %d]", r, BN_NCC_MAX_RANGE);
  BN_REQUIRE(k >= 0 && k <= BN_NCC_MAX_SCALE, "ncc_moments: k=%d outside [0, %d]", k, BN_NCC_MAX_SCALE);
  BN_REQUIRE(0 <= row0 && row0 <= row1 && row1 <= H, "ncc_moments: rows [%d, %d) outside [0, %d)", row0, row1, H);
  BN_REQUIRE(std::isfinite(pivot), "ncc_moments: pivot=%g is not finite", pivot);
  BN_REQUIRE(dx0 >= -BN_NCC_MAX_SHIFT && dx0 <= BN_NCC_MAX_SHIFT && dy0 >= -BN_NCC_MAX_SHIFT && dy0 <= BN_NCC_MAX_SHIFT,
             "ncc_moments: start (%d, %d) beyond 2^20 cells", dx0, dy0);
  if (row0 == row1) return 0;
  const dim3 grid((unsigned)((W + TILE - 1) / TILE), (unsigned)((row1 - row0 + TILE - 1) / TILE));
  BN_REQUIRE(grid.y <= 65535u, "ncc_moments: %u row tiles exceed the launch grid", grid.y);
  ncc_moments_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(u, v, H, W, pivot, (double)(1 << k), dx0, dy0, r, row0, row1,
                                                            reinterpret_cast<unsigned long long *>(sums),
                                                            reinterpret_cast<unsigned long long *>(skipped));
  BN_LAUNCH_CHECK("ncc_moments");
  return 0;
}

extern "C" int bn_dsm_shift_diff(const float *pred, const float *gt, int32_t H, int32_t W, int32_t dx, int32_t dy, double b,
                                 const uint8_t *mask, float *rdsm, float *diff, long long *sums6, void *stream) {
  BN_REQUIRE(pred && gt && sums6, "dsm_shift_diff: null argument");
  BN_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= BN_NCC_MAX_CELLS, "dsm_shift_diff: grid %d x %d (1 to 2^22 cells)", H, W);
  BN_REQUIRE(std::isfinite(b), "dsm_shift_diff: b=%g is not finite", b);
  BN_REQUIRE(dx >= -BN_NCC_MAX_SHIFT && dx <= BN_NCC_MAX_SHIFT && dy >= -BN_NCC_MAX_SHIFT && dy <= BN_NCC_MAX_SHIFT,
             "dsm_shift_diff: shift (%d, %d) beyond 2^20 cells", dx, dy);
  dsm_shift_diff_kernel<<<(unsigned)ceil_div64((int64_t)H * W, 256), 256, 0, (hipStream_t)stream>>>(
      pred, gt, H, W, dx, dy, b, mask, rdsm, diff, reinterpret_cast<unsigned long long *>(sums6));
  BN_LAUNCH_CHECK("dsm_shift_diff");
  return 0;
}
