// Step 4 of "Orthophoto of an observed image" (include/brdfnerf_hip.h), shared by orthophoto.hip (image_gather_kernel: one image)
// and mosaic.hip (grid_mosaic_kernel: several images fused per cell): the state of a cell under one image, the taps of an axis and
// the bilinear expression.  One statement, so that a view's value is the same bits wherever it is formed.  Only + x and
// comparisons occur; both files are built with fp contraction off and the pragma below covers the functions here wherever they
// are included.
#pragma once
#include <cmath>
#include "common.h"
#include "brdfnerf_hip.h"
#pragma clang fp contract(off)

namespace gather_rule {

// NODATA, OUTSIDE, OCCLUDED or KEPT, tested in this order; vis: the view's mask over the cells (nullable), c: the cell
__device__ __forceinline__ int cell_state(double col, double row, int32_t Hi, int32_t Wi, const uint8_t *vis, int64_t c) {
  if (isnan(col) || isnan(row)) return BN_GATHER_NODATA;
  if (!(col >= 0.0 && col <= (double)(Wi - 1) && row >= 0.0 && row <= (double)(Hi - 1))) return BN_GATHER_OUTSIDE;
  if (vis && vis[c] != BN_VIS_VISIBLE) return BN_GATHER_OCCLUDED;
  return BN_GATHER_KEPT;
}

// the two taps of one axis (bilinear): x in [0, n - 1] -> t0, t1 in [0, n - 1] and the weight of t1
__device__ __forceinline__ void taps(double x, int32_t n, int32_t &t0, int32_t &t1, double &f) {
  const int32_t fl = (int32_t)floor(x);
  t0 = fl < n - 2 ? fl : n - 2;
  t0 = t0 > 0 ? t0 : 0;                         // n == 1: both taps are pixel 0
  t1 = t0 + 1 < n ? t0 + 1 : n - 1;
  f = x - (double)t0;
}

__device__ __forceinline__ int32_t nearest_tap(double x, int32_t n) {
  const int32_t r = (int32_t)floor(x + 0.5);
  return r < n - 1 ? r : n - 1;
}

// the four taps of a kept cell as element offsets into one channel's pixels
struct Taps4 {
  int64_t a00, a01, a10, a11;
  double fx, fy;
};

__device__ __forceinline__ Taps4 bilinear_taps(double col, double row, int32_t Hi, int32_t Wi, int64_t s_row, int64_t s_col) {
  int32_t c0, c1, r0, r1;
  Taps4 t;
  taps(col, Wi, c0, c1, t.fx);
  taps(row, Hi, r0, r1, t.fy);
  t.a00 = r0 * s_row + c0 * s_col; t.a01 = r0 * s_row + c1 * s_col;
  t.a10 = r1 * s_row + c0 * s_col; t.a11 = r1 * s_row + c1 * s_col;
  return t;
}

// p: channel ch of pixel (0, 0); a NaN tap propagates even at weight 0
__device__ __forceinline__ float bilinear(const float *p, const Taps4 &t) {
  const double p00 = (double)p[t.a00], p01 = (double)p[t.a01], p10 = (double)p[t.a10], p11 = (double)p[t.a11];
  const double v = (1.0 - t.fy) * ((1.0 - t.fx) * p00 + t.fx * p01) + t.fy * ((1.0 - t.fx) * p10 + t.fx * p11);
  return (float)v;
}

__device__ __forceinline__ int64_t nearest_at(double col, double row, int32_t Hi, int32_t Wi, int64_t s_row, int64_t s_col) {
  return (int64_t)nearest_tap(row, Hi) * s_row + (int64_t)nearest_tap(col, Wi) * s_col;
}

}  // namespace gather_rule
