// Sun shadows and view occlusion of a surface model: from a start on or above a height grid, march along a direction and report
// whether some cell rises above the ray.  include/brdfnerf_hip.h ("Visibility over a surface model") states the rule operation by
// operation.  It has NO upstream counterpart - the reference never computes a geometric shadow - so the rule is this project's own
// and there is nothing to check it against but its statement.
//
//   grid_visibility_kernel    the starts are the cells of rows [row0, row1): (i + 0.5, j + 0.5, dsm[j][i])
//   points_visibility_kernel  the starts are points (east, north, altitude): surface_cell::point_cell's two quotients, unfloored
//
// Both call ONE march (march): float64, every operation rounded on its own, the step coordinate always u0 + (double)t su and
// never a running sum, the comparison h > zt + eps strict.  The start cell is never tested; a NaN cell never blocks.
//
// The mapping.  A block of 256 lanes owns a tile of 64 x 4 starts and ONE direction (grid mode; point mode: 256 consecutive points).
// A wave is a strip of 64 cells of one row.  All lanes of a tile share (su, sv), one of which is +-1, so at step t the strip reads
// 64 consecutive cells of the row floor(v0 + t sv): one or two 256-byte requests, and the four waves of the tile read four
// neighbouring rows.  A 512 x 512 grid is 1 MiB and stays in an XCD's 4 MiB L2; the lanes of a strip leave the march one by one
// (blocked, out of the grid, above zmax) and the wave ends with its last lane.  The directions of a launch travel as kernel
// arguments (VIS_DIRS of them, 24 bytes each): the entries check every direction on the host before the first launch and a call of
// K directions is ceil(K / VIS_DIRS) launches.
//
// counts: a wave counts its lanes' three classes by ballot, the block adds its four waves in LDS and sends ONE integer atomic per
// counter.  There is no float atomic.  vis and hit are plain stores of the lane's own start: every bit depends on the grid, the
// starts and the directions alone.
//
// As the compiler reports them for gfx950: grid_visibility_kernel 31 VGPRs, points_visibility_kernel 29 VGPRs, 48 B of LDS each, no
// scratch, 8 waves per SIMD.
// A tile-max table (the maximum non-NaN altitude per 8 x 8 cells, built by a small kernel, letting a lane skip the dsm load of
// every step with zt + eps at or above its tile's maximum) was priced against this form, alternately in one process, and retired:
// it was 1 to 11 % SLOWER on every case (512 x 512, K = 64, elevation 30: 3.151 against 2.825 ms; 2048 x 2048, K = 64, elevation
// 15: 130.3 against 126.3 ms) - the dsm load it saves hits L2 or the CU's L1 in a coalesced strip, and the table's own load, the
// tile index and the extra branch cost more.  profiles/visibility_throughput.txt holds both timings for every case.
#include <cmath>
#include "common.h"
#include "brdfnerf_hip.h"
// every float64 operation below is rounded on its own (see above); the build also passes -ffp-contract=off for this file
#pragma clang fp contract(off)

namespace {

constexpr int VIS_TILE_W = 64;                 // a wave: 64 cells of one row
constexpr int VIS_TILE_H = 4;                  // a block: four rows
constexpr int VIS_BLOCK = VIS_TILE_W * VIS_TILE_H;
constexpr int VIS_DIRS = 64;                   // directions per launch (1536 bytes of kernel arguments)
constexpr int64_t VIS_MAX_CELLS = (int64_t)1 << 30;

struct Dirs {
  double d[VIS_DIRS][3];
};

struct GridView {
  const float *dsm;
  int32_t H, W;
  double res, eps, zmax;
};

struct Slope {
  double su, sv, sz;
  bool zenith;
};

__device__ __forceinline__ Slope slope_of(const double *d, double res) {
  Slope s;
  const double a = fmax(fabs(d[0]), fabs(d[1]));
  s.zenith = a == 0.0;
  s.su = d[0] / a;
  s.sv = -(d[1] / a);
  s.sz = (d[2] / a) * res;
  return s;
}

__device__ __forceinline__ bool inside(const GridView &G, double u, double v) {
  return u >= 0.0 && u < (double)G.W && v >= 0.0 && v < (double)G.H;
}

// the march of one start that has data: BN_VIS_BLOCKED with hit = the first blocking cell in ascending t, else BN_VIS_VISIBLE
__device__ __forceinline__ int march(const GridView &G, const Slope &s, double u0, double v0, double z0, int32_t &hit) {
  hit = -1;
  if (s.zenith) return BN_VIS_VISIBLE;
  const int steps = G.W > G.H ? G.W : G.H;
  for (int t = 1; t <= steps; ++t) {
    const double tt = (double)t;
    const double ut = u0 + tt * s.su, vt = v0 + tt * s.sv, zt = z0 + tt * s.sz;
    if (!inside(G, ut, vt)) return BN_VIS_VISIBLE;
    if (zt > G.zmax) return BN_VIS_VISIBLE;      // no cell is above zmax: nothing further can block
    const int32_t c = (int32_t)floor(vt) * G.W + (int32_t)floor(ut);      // inside: 0 <= c < H W <= 2^30
    const double h = (double)G.dsm[c];
    if (h > zt + G.eps) {                          // strict; false for a NaN cell
      hit = c;
      return BN_VIS_BLOCKED;
    }
  }
  return BN_VIS_VISIBLE;
}

// (blocked, visible, nodata) of the block's lanes into counts[0..3): one integer atomic per counter and block
__device__ __forceinline__ void count_classes(int cls, unsigned long long *counts) {
  __shared__ unsigned int red[VIS_BLOCK / 64][3];
  const int tid = (int)threadIdx.x;
  for (int c = 0; c < 3; ++c) {
    const unsigned long long b = __ballot(cls == c);
    if ((tid & 63) == 0) red[tid >> 6][c] = (unsigned int)__popcll(b);
  }
  __syncthreads();
  if (tid < 3) {
    unsigned int n = 0;
    for (int w = 0; w < VIS_BLOCK / 64; ++w) n += red[w][tid];
    if (n) atomicAdd(counts + tid, (unsigned long long)n);
  }
}

__global__ __launch_bounds__(VIS_BLOCK)
void grid_visibility_kernel(const GridView G, const Dirs D, int row0, int row1, int tiles_x, uint8_t *__restrict__ vis,
                            int32_t *__restrict__ hit, unsigned long long *__restrict__ counts) {
  const int tid = (int)threadIdx.x, k = (int)blockIdx.y;
  const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)tiles_x);
  const int i = tx * VIS_TILE_W + (tid & (VIS_TILE_W - 1));
  const int64_t j = (int64_t)row0 + (int64_t)ty * VIS_TILE_H + (tid >> 6);
  int cls = -1;                                  // a lane outside the band counts nowhere
  if (i < G.W && j < row1) {
    const int64_t c = j * G.W + i;
    const double z0 = (double)G.dsm[c];
    int32_t h = -1;
    cls = BN_VIS_NODATA;
    if (isfinite(z0)) cls = march(G, slope_of(D.d[k], G.res), (double)i + 0.5, (double)j + 0.5, z0, h);
    const int64_t at = (int64_t)k * ((int64_t)G.H * G.W) + c;
    vis[at] = (uint8_t)cls;
    if (hit) hit[at] = h;
  }
  count_classes(cls, counts + 3 * k);
}

__global__ __launch_bounds__(VIS_BLOCK)
void points_visibility_kernel(const GridView G, const Dirs D, const double *__restrict__ enz, int64_t R, double xoff, double yoff,
                              uint8_t *__restrict__ vis, int32_t *__restrict__ hit, unsigned long long *__restrict__ counts) {
  const int k = (int)blockIdx.y;
  const int64_t r = (int64_t)blockIdx.x * VIS_BLOCK + threadIdx.x;
  int cls = -1;
  if (r < R) {
    const double u0 = (enz[3 * r] - xoff) / G.res, v0 = (yoff - enz[3 * r + 1]) / G.res, z0 = enz[3 * r + 2];
    int32_t h = -1;
    cls = BN_VIS_NODATA;
    if (isfinite(u0) && isfinite(v0) && isfinite(z0) && inside(G, u0, v0)) cls = march(G, slope_of(D.d[k], G.res), u0, v0, z0, h);
    const int64_t at = (int64_t)k * R + r;
    vis[at] = (uint8_t)cls;
    if (hit) hit[at] = h;
  }
  count_classes(cls, counts + 3 * k);
}


// what both entries refuse of the grid, the directions and the tolerances; 0 or BN_EINVAL with the error set
int require_march(const char *who, const float *dsm, int32_t H, int32_t W, double res, const double *dirs, int32_t K, double eps,
                  double zmax, const void *vis, const void *counts) {
  BN_REQUIRE(dsm && dirs && vis && counts, "%s: null argument", who);
  BN_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= VIS_MAX_CELLS, "%s: grid %d x %d (H W from 1 to 2^30 cells)", who, H, W);
  BN_REQUIRE(K >= 1 && K <= BN_VIS_MAX_DIRS, "%s: K=%d directions outside [1, %d]", who, K, BN_VIS_MAX_DIRS);
  BN_REQUIRE(res > 0.0 && std::isfinite(res), "%s: resolution %g must be positive and finite", who, res);
  BN_REQUIRE(eps >= 0.0 && std::isfinite(eps), "%s: eps %g must be finite and not negative", who, eps);
  BN_REQUIRE(!std::isnan(zmax), "%s: zmax is NaN", who);
  for (int32_t k = 0; k < K; ++k) {
    const double *d = dirs + 3 * (int64_t)k;
    BN_REQUIRE(std::isfinite(d[0]) && std::isfinite(d[1]) && std::isfinite(d[2]) && d[2] > 0.0,
               "%s: direction %d = (%g, %g, %g) must be finite and point above the horizon (dz > 0)", who, k, d[0], d[1], d[2]);
  }
  return 0;
}

Dirs dirs_chunk(const double *dirs, int32_t k0, int32_t n) {
  Dirs D;
  for (int k = 0; k < VIS_DIRS; ++k)
    for (int c = 0; c < 3; ++c) D.d[k][c] = k < n ? dirs[3 * (int64_t)(k0 + k) + c] : 0.0;
  return D;
}

}  // namespace

extern "C" int bn_grid_visibility(const float *dsm, int32_t H, int32_t W, double res, int32_t row0, int32_t row1, const double *dirs,
                                  int32_t K, double eps, double zmax, uint8_t *vis, int32_t *hit, long long *counts, void *stream) {
  if (int bad = require_march("grid_visibility", dsm, H, W, res, dirs, K, eps, zmax, vis, counts)) return bad;
  BN_REQUIRE(0 <= row0 && row0 <= row1 && row1 <= H, "grid_visibility: rows [%d, %d) outside [0, %d)", row0, row1, H);
  if (row0 == row1) return 0;
  const GridView G{dsm, H, W, res, eps, zmax};
  const int tiles_x = (W + VIS_TILE_W - 1) / VIS_TILE_W;
  const int64_t tiles = (int64_t)tiles_x * ((row1 - row0 + VIS_TILE_H - 1) / VIS_TILE_H);      // at most 2^28 + 2^24
  const int64_t plane = (int64_t)H * W;
  for (int32_t k0 = 0; k0 < K; k0 += VIS_DIRS) {
    const int32_t n = K - k0 < VIS_DIRS ? K - k0 : VIS_DIRS;
    grid_visibility_kernel<<<dim3((unsigned)tiles, (unsigned)n), VIS_BLOCK, 0, (hipStream_t)stream>>>(
        G, dirs_chunk(dirs, k0, n), row0, row1, tiles_x, vis + k0 * plane, hit ? hit + k0 * plane : nullptr,
        reinterpret_cast<unsigned long long *>(counts) + 3 * (int64_t)k0);
    BN_LAUNCH_CHECK("grid_visibility");
  }
  return 0;
}

extern "C" int bn_points_visibility(const double *enz, int64_t R, const float *dsm, int32_t H, int32_t W, double xoff, double yoff,
                                    double res, const double *dirs, int32_t K, double eps, double zmax, uint8_t *vis, int32_t *hit,
                                    long long *counts, void *stream) {
  if (int bad = require_march("points_visibility", dsm, H, W, res, dirs, K, eps, zmax, vis, counts)) return bad;
  BN_REQUIRE(enz, "points_visibility: null argument");
  BN_REQUIRE(R >= 0 && R <= VIS_MAX_CELLS, "points_visibility: R=%lld points outside [0, 2^30]", (long long)R);
  BN_REQUIRE(std::isfinite(xoff) && std::isfinite(yoff), "points_visibility: grid origin (%g, %g) is not finite", xoff, yoff);
  if (R == 0) return 0;
  const GridView G{dsm, H, W, res, eps, zmax};
  for (int32_t k0 = 0; k0 < K; k0 += VIS_DIRS) {
    const int32_t n = K - k0 < VIS_DIRS ? K - k0 : VIS_DIRS;
    points_visibility_kernel<<<dim3((unsigned)ceil_div64(R, VIS_BLOCK), (unsigned)n), VIS_BLOCK, 0, (hipStream_t)stream>>>(
        G, dirs_chunk(dirs, k0, n), enz, R, xoff, yoff, vis + k0 * R, hit ? hit + k0 * R : nullptr,
        reinterpret_cast<unsigned long long *>(counts) + 3 * (int64_t)k0);
    BN_LAUNCH_CHECK("points_visibility");
  }
  return 0;
}
