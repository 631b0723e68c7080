// The rest of the evaluation's line (eval.py:467-479) on the device: SSIM of a rendered view and the normal-angle MAE of its DSM.
//
// bn_ssim_map      kornia 0.5.3 `ssim` as metrics.py:327-341 calls it (Gaussian window, sigma 1.5, reflect padding, max_val passed):
//                  per output cell the five windowed moments of the two images in float64 and the index v; (float)v into the map,
//                  llrint(v 2^30) into an INTEGER sum.  One block owns a 32 x 32 output tile of one plane: it stages the tile and
//                  its window/2 halo of both images into LDS once - already masked, divided and widened to float64 - computes every
//                  tap from LDS, reduces its integers over the block and issues ONE atomic triple (sum, count, skipped).
// bn_grid_normals  the four-cross-product normals of an altitude grid (sat_utils.py:16-50 on get_pts3d_from_dsm, :175-183), a lane
//                  per cell, float64.
// bn_normal_angle  the angle between two normal grids in degrees (calc_nr_diff, :164-173), a lane per cell, and integer
//                  (sum, count) pairs over all / inside / outside cells: the nanmean of :341 and MaskDoD (:278-297, :346).
//
// As in world.hip every float64 operation is rounded on its own (the file is built with fp contraction off and carries the pragma):
// the tests hold the maps to a numpy float64 statement bit for bit, and a fused multiply-add in a tap sum would round differently.
// The sums are integer, so their bits do not depend on the block order or on how the rows are split over launches or devices;
// there is no float atomic in this file.
// LDS: a row of the staged tile is 32 + window - 1 float64 values; a 64-lane wave reads two output rows, each half-wave 32
// consecutive float64 values of one row - 64 consecutive banks, one ds_read_b64 cycle per half, no conflict at any row pitch.
#include <cmath>
#include "common.h"
#include "brdfnerf_hip.h"
#include "block_sums.h"
#include "normal_chain.h"
// every float64 operation below is rounded on its own (see above); the build also passes -ffp-contract=off for this file
#pragma clang fp contract(off)

namespace {

constexpr int TILE = 32;                       // output tile edge; 256 lanes, four output rows per lane (r, r + 8, r + 16, r + 24)
constexpr int MAXWIN = BN_SSIM_MAX_WINDOW;
constexpr int PITCH = TILE + MAXWIN - 1;       // 42
constexpr double SSIM_FIX = 1073741824.0;      // 2^30
constexpr double ANGLE_FIX = 1048576.0;        // 2^20

struct SsimArgs {
  const float *pred, *gt;
  const uint8_t *mask;
  int64_t sp, sr, sc;
  double div, C1, C2;
  double g[MAXWIN];
  int32_t C, H, W, window, row0, row1;
};

__device__ __forceinline__ int reflect(int i, int n) {
  // 'reflect' without repeating the edge: -1 -> 1, n -> n - 2.  pad < n, so one fold suffices for every index a VALID output
  // reads; halo cells that only outputs beyond the image would read are clamped into the image (they are never used).
  if (i < 0) i = -i;
  if (i >= n) i = 2 * (n - 1) - i;
  return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

__global__ __launch_bounds__(256)
void ssim_map_kernel(const SsimArgs A, float *__restrict__ map, unsigned long long *__restrict__ sums) {
  __shared__ double sx[PITCH * PITCH], sy[PITCH * PITCH];
  __shared__ long long red[4];
  const int win = A.window, pad = win >> 1, ext = TILE + win - 1;
  const int plane = blockIdx.z;
  const int tr0 = A.row0 + (int)blockIdx.y * TILE, tc0 = (int)blockIdx.x * TILE;
  const float *p = A.pred + plane * A.sp, *q = A.gt + plane * A.sp;
  for (int i = threadIdx.x; i < ext * ext; i += 256) {
    const int lr = i / ext, lc = i - lr * ext;
    const int r = reflect(tr0 + lr - pad, A.H), c = reflect(tc0 + lc - pad, A.W);
    const int64_t at = r * A.sr + c * A.sc;
    const double m = A.mask ? (double)A.mask[(int64_t)r * A.W + c] : 1.0;
    sx[lr * PITCH + lc] = ((double)p[at] * m) / A.div;
    sy[lr * PITCH + lc] = ((double)q[at] * m) / A.div;
  }
  __syncthreads();
  const int lc = threadIdx.x & 31, lr0 = threadIdx.x >> 5;
  long long qsum = 0, cnt = 0, skip = 0;
  for (int j = 0; j < 4; ++j) {
    const int lr = lr0 + 8 * j, r = tr0 + lr, c = tc0 + lc;
    if (r >= A.row1 || c >= A.W) continue;
    double mx = 0.0, my = 0.0, exx = 0.0, eyy = 0.0, exy = 0.0;
    for (int k2 = 0; k2 < win; ++k2) {
      const double g2 = A.g[k2];
      const double *rx = sx + (lr + k2) * PITCH + lc, *ry = sy + (lr + k2) * PITCH + lc;
      for (int k1 = 0; k1 < win; ++k1) {
        const double w = g2 * A.g[k1];
        const double x = rx[k1], y = ry[k1];
        const double xx = x * x, yy = y * y, xy = x * y;
        mx = mx + w * x;
        my = my + w * y;
        exx = exx + w * xx;
        eyy = eyy + w * yy;
        exy = exy + w * xy;
      }
    }
    const double mxx = mx * mx, myy = my * my, mxy = mx * my;
    const double sxx = exx - mxx, syy = eyy - myy, sxy = exy - mxy;
    const double num = (2.0 * mx * my + A.C1) * (2.0 * sxy + A.C2);
    const double den = ((mxx + myy) + A.C1) * ((sxx + syy) + A.C2) + 1e-12;
    const double v = num / den;
    if (map) map[((int64_t)plane * A.H + r) * A.W + c] = (float)v;
    if (isfinite(v) && fabs(v) < 4.0) {
      qsum += llrint(v * SSIM_FIX);
      cnt += 1;
    } else {
      skip += 1;
    }
  }
  const long long s0 = block_sums::block_sum(qsum, red), s1 = block_sums::block_sum(cnt, red), s2 = block_sums::block_sum(skip, red);
  if (threadIdx.x == 0) {
    atomicAdd(sums + 0, (unsigned long long)s0);           // two's complement: a negative sum wraps
    atomicAdd(sums + 1, (unsigned long long)s1);
    atomicAdd(sums + 2, (unsigned long long)s2);
  }
}

using normal_chain::V3;       // the per-cell chain lives in normal_chain.h, shared with bn_point_normals (view_maps.hip)

__global__ __launch_bounds__(256)
void grid_normals_kernel(const float *__restrict__ z, int H, int W, double res, float *__restrict__ out) {
  const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (cell >= (int64_t)H * W) return;
  const int r = (int)(cell / W), c = (int)(cell - (int64_t)r * W);
  float *o = out + cell * 3;
  if (r == 0 || r == H - 1 || c == 0 || c == W - 1) {
    o[0] = o[1] = o[2] = 0.0f;
    return;
  }
  // P(r, c) = (c res, r res, z): x grows with the column, y with the ROW (sat_utils.py:178-182)
  const double x0 = (double)c * res, y0 = (double)r * res, z0 = (double)z[cell];
  const V3 n = normal_chain::cell_normal({0.0, (double)(r + 1) * res - y0, (double)z[cell + W] - z0},
                                         {0.0, (double)(r - 1) * res - y0, (double)z[cell - W] - z0},
                                         {(double)(c + 1) * res - x0, 0.0, (double)z[cell + 1] - z0},
                                         {(double)(c - 1) * res - x0, 0.0, (double)z[cell - 1] - z0});
  o[0] = (float)n.x;
  o[1] = (float)n.y;
  o[2] = (float)n.z;
}

__global__ __launch_bounds__(256)
void normal_angle_kernel(const float *__restrict__ n1, const float *__restrict__ n2, int H, int W, const uint8_t *__restrict__ mask,
                         int border, float *__restrict__ angle, unsigned long long *__restrict__ sums) {
  __shared__ long long red[4];
  const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
  long long q = 0, n = 0;
  bool inside = true;
  if (cell < (int64_t)H * W) {
    const int r = (int)(cell / W), c = (int)(cell - (int64_t)r * W);
    const float *a = n1 + cell * 3, *b = n2 + cell * 3;
    double ang;
    if (border && (r == 0 || r == H - 1 || c == 0 || c == W - 1)) {
      ang = __builtin_nan("");
    } else {
      double d = ((double)a[0] * (double)b[0] + (double)a[1] * (double)b[1]) + (double)a[2] * (double)b[2];
      d = d < -1.0 ? -1.0 : (d > 1.0 ? 1.0 : d);           // a NaN passes through, as torch.clamp lets it
      ang = acos(d) * 180.0 / 3.141592653589793;
    }
    if (angle) angle[cell] = (float)ang;
    if (ang == ang) {                                      // nanmean: NaN cells are left out
      q = llrint(ang * ANGLE_FIX);
      n = 1;
    }
    inside = !mask || mask[cell] != 0;
  }
  block_sums::masked_sums6(q, n, inside, red, sums);
}

}  // namespace

extern "C" int bn_ssim_map(const float *pred, const float *gt, int32_t C, int32_t H, int32_t W, int64_t plane_stride,
                           int64_t row_stride, int64_t col_stride, const uint8_t *mask, double div, double max_val, int32_t window,
                           const double *g, int32_t row0, int32_t row1, float *map, long long *sums, void *stream) {
  BN_REQUIRE(pred && gt && g && sums, "ssim_map: null argument");
  BN_REQUIRE(window >= 3 && window <= BN_SSIM_MAX_WINDOW && (window & 1), "ssim_map: window=%d must be odd, 3 to %d", window, BN_SSIM_MAX_WINDOW);
  BN_REQUIRE(C > 0 && H > 0 && W > 0 && (int64_t)C * H * W <= ((int64_t)1 << 30), "ssim_map: image %d x %d x %d (C H W at most 2^30 elements)", C, H, W);
  BN_REQUIRE(H > window / 2 && W > window / 2, "ssim_map: image %d x %d too small for the reflect padding of window %d (needs more than %d)",
             H, W, window, window / 2);
  BN_REQUIRE(plane_stride >= 0 && row_stride >= 0 && col_stride >= 0, "ssim_map: negative stride");
  BN_REQUIRE(std::isfinite(max_val), "ssim_map: max_val=%g is not finite", max_val);
  BN_REQUIRE(std::isfinite(div), "ssim_map: div=%g is not finite", div);
  BN_REQUIRE(0 <= row0 && row0 <= row1 && row1 <= H, "ssim_map: rows [%d, %d) outside [0, %d)", row0, row1, H);
  for (int k = 0; k < window; ++k) BN_REQUIRE(std::isfinite(g[k]), "ssim_map: weight %d is not finite", k);
  if (row0 == row1) return 0;
  SsimArgs a;
  a.pred = pred; a.gt = gt; a.mask = mask; a.sp = plane_stride; a.sr = row_stride; a.sc = col_stride;
  a.div = div;
  const double c1 = 0.01 * max_val, c2 = 0.03 * max_val;
  a.C1 = c1 * c1; a.C2 = c2 * c2;
  for (int k = 0; k < MAXWIN; ++k) a.g[k] = k < window ? g[k] : 0.0;
  a.C = C; a.H = H; a.W = W; a.window = window; a.row0 = row0; a.row1 = row1;
  const dim3 grid((unsigned)((W + TILE - 1) / TILE), (unsigned)((row1 - row0 + TILE - 1) / TILE), (unsigned)C);
  BN_REQUIRE(grid.y <= 65535u && grid.z <= 65535u, "ssim_map: %u row tiles x %u planes exceed the launch grid", grid.y, grid.z);
  ssim_map_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(a, map, reinterpret_cast<unsigned long long *>(sums));
  BN_LAUNCH_CHECK("ssim_map");
  return 0;
}

extern "C" int bn_grid_normals(const float *z, int32_t H, int32_t W, double resolution, float *normals, void *stream) {
  BN_REQUIRE(z && normals, "grid_normals: null argument");
  BN_REQUIRE(W > 0 && H > 0 && (int64_t)W * H <= ((int64_t)1 << 30), "grid_normals: grid %d x %d (W H at most 2^30 cells)", W, H);
  BN_REQUIRE(resolution > 0 && std::isfinite(resolution), "grid_normals: resolution=%g must be positive", resolution);
  grid_normals_kernel<<<(unsigned)ceil_div64((int64_t)W * H, 256), 256, 0, (hipStream_t)stream>>>(z, H, W, resolution, normals);
  BN_LAUNCH_CHECK("grid_normals");
  return 0;
}

extern "C" int bn_normal_angle(const float *n1, const float *n2, int32_t H, int32_t W, const uint8_t *mask, int32_t border, float *angle,
                               long long *sums, void *stream) {
  BN_REQUIRE(n1 && n2 && sums, "normal_angle: null argument");
  BN_REQUIRE(W > 0 && H > 0 && (int64_t)W * H <= ((int64_t)1 << 30), "normal_angle: grid %d x %d (W H at most 2^30 cells)", W, H);
  BN_REQUIRE(border == 0 || border == 1, "normal_angle: border=%d (0: the reference's 90 degrees, 1: left out)", border);
  normal_angle_kernel<<<(unsigned)ceil_div64((int64_t)W * H, 256), 256, 0, (hipStream_t)stream>>>(
      n1, n2, H, W, mask, border, angle, reinterpret_cast<unsigned long long *>(sums));
  BN_LAUNCH_CHECK("normal_angle");
  return 0;
}
