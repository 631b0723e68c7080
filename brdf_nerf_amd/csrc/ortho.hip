// Orthorectified maps of a view: the per-ray maps of view_maps (rgb, albedo, normals, BRDF parameters) splatted into the grid of
// the DSM, channel by channel, with an optional top-surface pass.  include/brdfnerf_hip.h ("Orthorectified maps of a view") states
// the rule operation by operation.  The feature channels have NO upstream counterpart: the reference rasterises the altitude alone
// (plyflatten, datasets/satellite_rgb_dep.py:636-699); the rule for the channels is this project's own.  The altitude part is
// bn_dsm_splat's (bn_dsm_splat_world's) bit for bit: the point, the cell, the footprint and q come from surface_cell.h, the very
// device functions world.hip is made of.
//
//   ortho_top_kernel      pass 1, one lane per ray: top[cell] = max(top[cell], q) over the footprint, a signed 64-bit integer atomic
//   ortho_splat_kernel    pass 2.  Phase 1: the first ORTHO_RAYS lanes of a block form their ray's point (the ECEF chain has some
//                         30 float64 transcendentals: once per ray, not once per channel) and leave (i, j, q, state) in LDS; all
//                         lanes then look through the block's features for a bad one.  Phase 2: lanes own (ray, slot) pairs,
//                         slot = (sum_z, count, sum_0 .. sum_{E-1}); consecutive lanes add into consecutive int64 of ONE cell and
//                         walk the footprint together, so a wave's atomic instruction covers whole cells of 8 (2 + E) contiguous
//                         bytes instead of one 8-byte word per cell.  The lanes of a ray read top[cell] at one address, which the
//                         wave's load merges into one request.
//                         The plain form (a lane per ray issues the 2 + E atomics of a cell one after the other) gave the same
//                         integers in another order and was retired; profiles/ortho_throughput.txt records the comparison.
//   ortho_resolve_kernel  one lane per cell: the means
//
// Integer atomics only (add and signed max): every output bit depends on the set of rays alone.  Each counter is summed per block
// in LDS and goes out as ONE integer atomic per block.
// As the compiler reports them for gfx950: ortho_top_kernel 62 VGPRs and 4 B of LDS, ortho_splat_kernel 63 VGPRs and 1296 B of LDS,
// ortho_resolve_kernel 22 VGPRs and no LDS; none uses scratch, all run 8 waves per SIMD.  Timed alternately in one process
// (profiles/ortho_throughput.txt; 512 x 512 view, 1.3 M deposits), the pair form takes 0.089 ms at E = 3 and 0.287 ms at E = 28
// against 0.288 and 1.760 ms of the retired lane-per-ray form.
#include <cmath>
#include "common.h"
#include "brdfnerf_hip.h"
#include "block_sums.h"
#include "geodesy.h"
#include "surface_cell.h"
// every float64 operation below is rounded on its own (see above); the build also passes -ffp-contract=off for this file
#pragma clang fp contract(off)

namespace {

using namespace surface_cell;

constexpr int ORTHO_BLOCK = 256;
constexpr int ORTHO_RAYS = 64;                 // rays per block of the splat: one wave forms the points
constexpr double ORTHO_FIX = 16777216.0;       // 2^24: features are summed in units of 2^-24
constexpr float ORTHO_XMAX = 65536.0f;         // 2^16
constexpr long long ORTHO_BAND_MAX = 1ll << 62;

enum { RAY_DEPOSIT = 0, RAY_BAD_POINT = 1, RAY_FAR = 2, RAY_BAD_FEATURE = 3, RAY_NONE = 4 };

struct FeatureArgs {
  const float *x;
  int64_t stride;
  int32_t E;
  const long long *top;
  long long band_q;
};

__device__ __forceinline__ bool bad_feature(float x) { return !(fabsf(x) < ORTHO_XMAX); }          // NaN and inf included
__device__ __forceinline__ long long feature_q(float x) { return llrint((double)x * ORTHO_FIX); }

__device__ __forceinline__ bool culled(const FeatureArgs &F, long long q, int64_t c) {
  return F.top != nullptr && q + F.band_q < F.top[c];
}

__global__ __launch_bounds__(ORTHO_BLOCK)
void ortho_top_kernel(const PointArgs A, const ToEnz T, const GridArgs G, long long *__restrict__ top,
                      unsigned long long *__restrict__ skipped) {
  const int64_t ray = (int64_t)blockIdx.x * ORTHO_BLOCK + threadIdx.x;
  bool bad = false;
  if (ray < A.R) {
    double e, n, a;
    surface_point(A, T, ray, e, n, a);             // a refused point is NaN, which point_cell skips
    int i, j;
    long long q;
    const int what = point_cell(G, e, n, a, i, j, q);
    bad = what == POINT_SKIPPED;
    if (what == POINT_DEPOSIT)
      for_footprint(G, i, j, [&](int64_t c) { __hip_atomic_fetch_max(top + c, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); });
  }
  block_sums::block_count(bad, skipped);
}

__global__ __launch_bounds__(ORTHO_BLOCK)
void ortho_splat_kernel(const PointArgs A, const ToEnz T, const GridArgs G, const FeatureArgs F, unsigned long long *__restrict__ acc,
                        unsigned long long *__restrict__ counters) {
  __shared__ int s_i[ORTHO_RAYS], s_j[ORTHO_RAYS], s_state[ORTHO_RAYS];
  __shared__ long long s_q[ORTHO_RAYS];
  __shared__ unsigned int s_count[3];
  const int tid = threadIdx.x;
  const int64_t ray0 = (int64_t)blockIdx.x * ORTHO_RAYS;
  const int64_t left = A.R - ray0;
  const int rays = left < ORTHO_RAYS ? (int)left : ORTHO_RAYS;
  if (tid < 3) s_count[tid] = 0;
  // phase 1: a ray's point, once
  if (tid < ORTHO_RAYS) {
    int state = RAY_NONE, i = 0, j = 0;
    long long q = 0;
    if (tid < rays) {
      double e, n, a;
      surface_point(A, T, ray0 + tid, e, n, a);
      const int what = point_cell(G, e, n, a, i, j, q);
      state = what == POINT_SKIPPED ? RAY_BAD_POINT : (what == POINT_FAR ? RAY_FAR : RAY_DEPOSIT);
    }
    s_i[tid] = i; s_j[tid] = j; s_q[tid] = q; s_state[tid] = state;
  }
  __syncthreads();
  // a bad feature anywhere in a ray's row takes the whole ray out; a bad point comes first and is counted as that
  for (int p = tid; p < rays * F.E; p += ORTHO_BLOCK) {
    const int r = p / F.E, e = p - r * F.E;
    if (s_state[r] != RAY_BAD_POINT && bad_feature(F.x[(ray0 + r) * F.stride + e])) s_state[r] = RAY_BAD_FEATURE;   // every writer writes this value
  }
  __syncthreads();
  if (tid < rays) {
    if (s_state[tid] == RAY_BAD_POINT) atomicAdd(&s_count[0], 1u);
    if (s_state[tid] == RAY_BAD_FEATURE) atomicAdd(&s_count[1], 1u);
  }
  // phase 2: (ray, slot) pairs; the lanes of a ray walk its footprint together
  const int S = 2 + F.E;
  unsigned int n_culled = 0;
  for (int p = tid; p < rays * S; p += ORTHO_BLOCK) {
    const int r = p / S, slot = p - r * S;
    if (s_state[r] != RAY_DEPOSIT) continue;
    const long long q = s_q[r];
    const long long v = slot == 0 ? q : (slot == 1 ? 1ll : feature_q(F.x[(ray0 + r) * F.stride + (slot - 2)]));
    for_footprint(G, s_i[r], s_j[r], [&](int64_t c) {
      if (culled(F, q, c)) {
        n_culled += slot == 0;                       // once per (ray, cell)
        return;
      }
      atomicAdd(acc + c * S + slot, (unsigned long long)v);      // two's complement: a negative value wraps
    });
  }
  if (n_culled) atomicAdd(&s_count[2], n_culled);
  __syncthreads();
  if (tid < 3 && s_count[tid]) atomicAdd(counters + tid, (unsigned long long)s_count[tid]);
}

__global__ __launch_bounds__(ORTHO_BLOCK)
void ortho_resolve_kernel(const long long *__restrict__ acc, int64_t n, int32_t E, float *__restrict__ maps, float *__restrict__ dsm,
                          int32_t *__restrict__ count) {
  const int64_t c = (int64_t)blockIdx.x * ORTHO_BLOCK + threadIdx.x;
  if (c >= n) return;
  const long long *cell = acc + c * (2 + E);
  const long long cnt = cell[1];
  dsm[c] = cell_mean(cell[0], cnt, DSM_FIX);
  if (count) count[c] = cell_count(cnt);
  for (int e = 0; e < E; ++e) maps[(int64_t)e * n + c] = cell_mean(cell[2 + e], cnt, ORTHO_FIX);
}

}  // namespace

extern "C" int bn_ortho_top(const float *rays, int64_t ray_stride, const float *depth, int64_t R, const double *center, double range,
                            double xoff, double yoff, double resolution, int32_t W, int32_t H, int32_t radius, int32_t footprint,
                            int32_t cs, int32_t zone, int32_t south, long long *top, unsigned long long *skipped, void *stream) {
  BN_REQUIRE(rays && depth && center && top && skipped, "ortho_top: null argument");
  if (int bad = require_rays("ortho_top", R, ray_stride, center, range, cs, zone, south)) return bad;
  if (int bad = require_cells("ortho_top", xoff, yoff, resolution, W, H, radius, footprint)) return bad;      // (top: 8-byte words)
  if (R == 0) return 0;
  ortho_top_kernel<<<(unsigned)ceil_div64(R, ORTHO_BLOCK), ORTHO_BLOCK, 0, (hipStream_t)stream>>>(
      make_point_args(rays, ray_stride, depth, R, center, range), make_to_enz(cs, zone, south),
      make_grid_args(xoff, yoff, resolution, W, H, radius, footprint), top, skipped);
  BN_LAUNCH_CHECK("ortho_top");
  return 0;
}

extern "C" int bn_ortho_splat(const float *rays, int64_t ray_stride, const float *depth, int64_t R, const double *center, double range,
                              double xoff, double yoff, double resolution, int32_t W, int32_t H, int32_t radius, int32_t footprint,
                              int32_t cs, int32_t zone, int32_t south, const float *features, int64_t feature_stride, int32_t E,
                              const long long *top, long long band_q, long long *acc, unsigned long long *counters, void *stream) {
  BN_REQUIRE(rays && depth && center && acc && counters, "ortho_splat: null argument");
  BN_REQUIRE(E >= 0 && E <= BN_ORTHO_MAX_CHANNELS, "ortho_splat: E=%d outside [0, %d]", E, BN_ORTHO_MAX_CHANNELS);
  BN_REQUIRE(E == 0 || features, "ortho_splat: E=%d channels without features", E);
  BN_REQUIRE(feature_stride >= E, "ortho_splat: feature rows of %lld floats hold no %d channels", (long long)feature_stride, E);
  BN_REQUIRE(band_q >= 0, "ortho_splat: band_q=%lld is negative", band_q);
  if (int bad = require_rays("ortho_splat", R, ray_stride, center, range, cs, zone, south)) return bad;
  if (int bad = require_grid("ortho_splat", acc, xoff, yoff, resolution, W, H, radius, footprint)) return bad;
  BN_REQUIRE(R <= (int64_t)ORTHO_RAYS * 0x7fffffff, "ortho_splat: R=%lld too large", (long long)R);
  if (R == 0) return 0;
  // |q| <= 2^43: a band of 2^44 or more already keeps everything, and q + band_q must not overflow
  const FeatureArgs f{features, feature_stride, E, top, band_q > ORTHO_BAND_MAX ? ORTHO_BAND_MAX : band_q};
  ortho_splat_kernel<<<(unsigned)ceil_div64(R, ORTHO_RAYS), ORTHO_BLOCK, 0, (hipStream_t)stream>>>(
      make_point_args(rays, ray_stride, depth, R, center, range), make_to_enz(cs, zone, south),
      make_grid_args(xoff, yoff, resolution, W, H, radius, footprint), f, reinterpret_cast<unsigned long long *>(acc), counters);
  BN_LAUNCH_CHECK("ortho_splat");
  return 0;
}

extern "C" int bn_ortho_resolve(const long long *acc, int32_t W, int32_t H, int32_t E, float *maps, float *dsm, int32_t *count,
                                void *stream) {
  BN_REQUIRE(acc && dsm, "ortho_resolve: null argument");
  BN_REQUIRE(E >= 0 && E <= BN_ORTHO_MAX_CHANNELS, "ortho_resolve: E=%d outside [0, %d]", E, BN_ORTHO_MAX_CHANNELS);
  BN_REQUIRE(E == 0 || maps, "ortho_resolve: E=%d channels without maps", E);
  BN_REQUIRE(((uintptr_t)acc & 15) == 0, "ortho_resolve: acc must be 16-byte aligned");
  BN_REQUIRE(W > 0 && H > 0 && (int64_t)W * H <= ((int64_t)1 << 31), "ortho_resolve: grid %d x %d (W H at most 2^31 cells)", W, H);
  const int64_t n = (int64_t)W * H;
  ortho_resolve_kernel<<<(unsigned)ceil_div64(n, ORTHO_BLOCK), ORTHO_BLOCK, 0, (hipStream_t)stream>>>(acc, n, E, maps, dsm, count);
  BN_LAUNCH_CHECK("ortho_resolve");
  return 0;
}
