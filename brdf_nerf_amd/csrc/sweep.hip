// The altitude sweep of a surface model under several observed images, in one launch: mosaic.hip says how far the views of a cell
// disagree at the model's altitude; grid_sweep_kernel asks the same at the altitude moved through a list of Z offsets and keeps the
// offset at which they disagree least - a plane sweep around the surface model.  include/brdfnerf_hip.h ("Altitude sweep of a
// surface model under several observed images") states the rule operation by operation; there is no upstream counterpart.
//
//   grid_sweep_kernel<C>   one lane per cell of rows [row0, row1), 256-lane blocks.  Centre and altitude as grid_mosaic_kernel forms
//                          them, geodesy.h's utm_geodetic ONCE, then for l = 0 .. Z - 1: a_l = a0 + off[l] in float64 and, for k = 0
//                          .. K - 1, view_step.h's add_view - grid_mosaic_kernel's per-view step, the same device function - on (lon,
//                          lat, a_l); the level's cost is the sum of the channels' population variances, and the first level of
//                          the smallest cost is kept (strict <).
//
// Levels are the outer loop and views the inner one, so that only the 2 C doubles of one level's Welford state and the running best
// are live.  View records and offsets are read with the loops' own indices, which every lane shares: the compiler fetches them
// through the scalar cache.  Both loops are uniform: `valid` is a table of Z LDS words fed by one ballot and popcount per wave and
// level, `wins` one LDS integer add per lane after the loop; one barrier, then at most 2 Z integer atomics per block and three
// more for the sums (block_sums.h).  There is no float atomic in this file, and every output is a plain store of the lane's own
// cell: every bit depends on the inputs alone, not on blocks, row bands or ranks.
#include <cmath>
#include "common.h"
#include "brdfnerf_hip.h"
#include "block_sums.h"
#include "gather_rule.h"
#include "geodesy.h"
#include "rpc_poly.h"
#include "view_step.h"
// every float64 operation below is rounded on its own (see above); the build also passes -ffp-contract=off for this file
#pragma clang fp contract(off)

namespace {

using namespace geodesy;

constexpr int SWEEP_BLOCK = 256;
constexpr uint32_t F32_NAN_BITS = 0x7FC00000u;
constexpr double Q20 = 1048576.0;

struct SweepArgs {
  const bn_mosaic_view *views;   // device, K records
  const double *offsets;         // device, Z
  const float *dsm;
  const double *colrow_in;       // [Z][K][H][W][2] or NULL
  int32_t K, Z, mode, W, row0, min_views;
  int64_t n, HW;                 // cells of the band: (row1 - row0) W; cells of the grid
  double xoff, yoff, res;
  UtmInvK U;
  int32_t *best_level;
  float *best_cost, *altitude, *cost;
  uint8_t *best_count;
  unsigned long long *valid, *wins, *sums;
};

template <int C>
__global__ __launch_bounds__(SWEEP_BLOCK)
void grid_sweep_kernel(const SweepArgs A) {
  __shared__ unsigned int valid_t[BN_SWEEP_MAX_LEVELS], wins_t[BN_SWEEP_MAX_LEVELS];
  __shared__ long long red[4];
  for (int t = threadIdx.x; t < A.Z; t += SWEEP_BLOCK) { valid_t[t] = 0; wins_t[t] = 0; }
  __syncthreads();

  const int64_t at = (int64_t)blockIdx.x * SWEEP_BLOCK + threadIdx.x;
  const bool live = at < A.n;
  const int64_t c = (int64_t)A.row0 * A.W + (live ? at : 0);        // below H W <= 2^30
  double lon = 0.0, lat = 0.0;
  const double a0 = (double)A.dsm[c];
  bool bad0 = false;
  if (live && !A.colrow_in) {
    const int64_t j = c / A.W, i = c - j * A.W;
    const double e = A.xoff + ((double)i + 0.5) * A.res, nn = A.yoff - ((double)j + 0.5) * A.res;
    bad0 = utm_geodetic(A.U, e, nn, lon, lat);
  }

  int32_t best = -1, best_n = 0;
  double best_v = 0.0;
  for (int l = 0; l < A.Z; ++l) {
    const double a = a0 + A.offsets[l];                              // l is the same in every lane: a scalar load; ONE float64 addition
    int32_t n = 0;
    double m[C], M2[C];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) { m[ch] = 0.0; M2[ch] = 0.0; }
    if (live) {
      for (int k = 0; k < A.K; ++k) {
        uint32_t v[C];
        view_step::add_view<C>(A.views[k], A.colrow_in ? A.colrow_in + 2 * (((int64_t)l * A.K + k) * A.HW + c) : nullptr, c, bad0, lon,
                               lat, a, A.mode, n, m, M2, v);
      }
    }
    const bool ok = live && n >= A.min_views;                        // min_views >= 1: n > 0 below
    double v_l = 0.0;
    if (ok) {
#pragma unroll
      for (int ch = 0; ch < C; ++ch) v_l = v_l + M2[ch] / (double)n;
      if (best < 0 || v_l < best_v) { best = l; best_v = v_l; best_n = n; }          // strict: the first level keeps a tie
    }
    if (live && A.cost) A.cost[(int64_t)l * A.HW + c] = ok ? (float)v_l : __uint_as_float(F32_NAN_BITS);
    const unsigned long long ballot = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && ballot) atomicAdd(&valid_t[l], (unsigned int)__popcll(ballot));       // LDS, integer
  }

  long long cells = 0, q = 0, skipped = 0;
  if (live) {
    A.best_level[c] = best;
    if (A.best_cost) A.best_cost[c] = best >= 0 ? (float)best_v : __uint_as_float(F32_NAN_BITS);
    if (A.best_count) A.best_count[c] = (uint8_t)best_n;           // best_n is set with best alone: 0 when no level is valid
    if (A.altitude) A.altitude[c] = best >= 0 ? (float)(a0 + A.offsets[best]) : __uint_as_float(F32_NAN_BITS);
    if (best >= 0) {
      atomicAdd(&wins_t[best], 1u);                                  // LDS, integer
      cells = 1;
      if (best_v < Q20) q = llrint(best_v * Q20);
      else skipped = 1;
    }
  }

  __syncthreads();
  for (int t = threadIdx.x; t < A.Z; t += SWEEP_BLOCK) {
    if (valid_t[t]) atomicAdd(A.valid + t, (unsigned long long)valid_t[t]);
    if (wins_t[t]) atomicAdd(A.wins + t, (unsigned long long)wins_t[t]);
  }
  const long long v3[3] = {cells, q, skipped};
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const long long s = block_sums::block_sum(v3[t], red);
    if (threadIdx.x == 0 && s != 0) atomicAdd(A.sums + t, (unsigned long long)s);
  }
}

}  // namespace

extern "C" int bn_grid_sweep(const bn_mosaic_view *views_host, const bn_mosaic_view *views_dev, int32_t K, int32_t C,
                             const float *dsm, int32_t H, int32_t W, double xoff, double yoff, double res, int32_t row0,
                             int32_t row1, int32_t zone, int32_t south, int32_t mode, const double *offsets_host,
                             const double *offsets_dev, int32_t Z, int32_t min_views, const double *colrow_in, int32_t *best_level,
                             float *best_cost, uint8_t *best_count, float *altitude, float *cost, unsigned long long *valid,
                             unsigned long long *wins, unsigned long long *sums, void *stream) {
  BN_REQUIRE(views_host && views_dev && dsm && offsets_host && offsets_dev && best_level && valid && wins && sums,
             "grid_sweep: null argument");
  if (view_step::check_views_on_grid("grid_sweep", views_host, K, C, H, W, xoff, yoff, res, row0, row1, zone, south, mode)) return BN_EINVAL;
  BN_REQUIRE(Z >= 1 && Z <= BN_SWEEP_MAX_LEVELS, "grid_sweep: Z=%d levels outside [1, %d]", Z, BN_SWEEP_MAX_LEVELS);
  for (int32_t l = 0; l < Z; ++l) BN_REQUIRE(std::isfinite(offsets_host[l]), "grid_sweep: offset %d is not finite", l);
  BN_REQUIRE(min_views >= 1 && min_views <= BN_MOSAIC_MAX_VIEWS, "grid_sweep: min_views=%d outside [1, %d]", min_views,
             BN_MOSAIC_MAX_VIEWS);
  if (row0 == row1) return 0;
  SweepArgs a;
  a.views = views_dev; a.offsets = offsets_dev; a.dsm = dsm; a.colrow_in = colrow_in;
  a.K = K; a.Z = Z; a.mode = mode; a.W = W; a.row0 = row0; a.min_views = min_views;
  a.n = (int64_t)(row1 - row0) * W; a.HW = (int64_t)H * W;
  a.xoff = xoff; a.yoff = yoff; a.res = res;
  a.U = make_utm_inv(zone, south);
  a.best_level = best_level; a.best_cost = best_cost; a.altitude = altitude; a.cost = cost; a.best_count = best_count;
  a.valid = valid; a.wins = wins; a.sums = sums;
  const unsigned blocks = (unsigned)ceil_div64(a.n, SWEEP_BLOCK);
  hipStream_t s = (hipStream_t)stream;
  switch (C) {
    case 1: grid_sweep_kernel<1><<<blocks, SWEEP_BLOCK, 0, s>>>(a); break;
    case 2: grid_sweep_kernel<2><<<blocks, SWEEP_BLOCK, 0, s>>>(a); break;
    case 3: grid_sweep_kernel<3><<<blocks, SWEEP_BLOCK, 0, s>>>(a); break;
    default: grid_sweep_kernel<4><<<blocks, SWEEP_BLOCK, 0, s>>>(a); break;
  }
  BN_LAUNCH_CHECK("grid_sweep");
  return 0;
}
