// The orthomosaic of several observed images on the grid of a surface model, in one launch: orthophoto.hip takes a cell to the
// pixel of ONE image; a site has 10 to 30, and each sees another side of every building.  grid_mosaic_kernel takes a cell to its
// geodetic point once, walks the K views and keeps only the results: how many views saw the cell, the best of them, the mean and
// the spread of what they saw.  include/brdfnerf_hip.h ("Orthomosaic of several observed images") states the rule operation by
// operation; there is no upstream counterpart.
//
//   grid_mosaic_kernel<C>   one lane per cell of rows [row0, row1), 256-lane blocks.  Centre and altitude as grid_pixels_kernel forms
//                           them, geodesy.h's utm_geodetic ONCE, then for k = 0 .. K - 1: rpc_poly.h's project under view k's
//                           descriptor (or the pixel read from colrow_in), gather_rule.h's state and value - bn_grid_pixels' and
//                           bn_image_gather's device functions on the same operands, so a view's value is the K-launch chain's
//                           bits - and Welford's update of the C means and sums of squares in float64.  That per-view step is
//                           view_step.h's add_view, which sweep.hip walks per altitude level.
//
// The K view records (776 bytes each) live in device memory and are read with the loop's own index, which every lane shares: the
// compiler fetches them through the scalar cache, as kernel arguments are fetched.  C is a template parameter and every per-channel
// array is indexed by a fully unrolled loop, so the running values stay in registers.  The loop over the views is uniform: the
// per-view counters are a K x 5 table of LDS words fed by one ballot and popcount per wave, view and state; one barrier, then at
// most 5 K integer atomics per block, and three more for the sums (block_sums.h).  There is no float atomic in this file, and every
// output is a plain store of the lane's own cell: every bit depends on the inputs alone, not on blocks, row bands or ranks.
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

constexpr int MOS_BLOCK = 256;
constexpr uint32_t F32_NAN_BITS = 0x7FC00000u;
constexpr double Q20 = 1048576.0;

struct MosaicArgs {
  const bn_mosaic_view *views;   // device, K records
  const float *dsm;
  const double *colrow_in;       // [K][H][W][2] or NULL
  int32_t K, mode, W, row0;
  int64_t n, HW;                 // cells of the band: (row1 - row0) W; cells of the grid
  double xoff, yoff, res;
  UtmInvK U;
  uint8_t *count;
  int32_t *best;
  uint32_t *best_val;            // the best view's 32 bits
  float *mean, *std;
  unsigned long long *counts, *sums;
};

template <int C>
__global__ __launch_bounds__(MOS_BLOCK)
void grid_mosaic_kernel(const MosaicArgs A) {
  __shared__ unsigned int table[BN_MOSAIC_MAX_VIEWS * 5];
  __shared__ long long red[4];
  for (int t = threadIdx.x; t < A.K * 5; t += MOS_BLOCK) table[t] = 0;
  __syncthreads();

  const int64_t at = (int64_t)blockIdx.x * MOS_BLOCK + threadIdx.x;
  const bool live = at < A.n;
  const int64_t c = (int64_t)A.row0 * A.W + (live ? at : 0);        // below H W <= 2^30
  double lon = 0.0, lat = 0.0, a = 0.0;
  bool bad0 = false;
  if (live && !A.colrow_in) {
    const int64_t j = c / A.W, i = c - j * A.W;
    const double e = A.xoff + ((double)i + 0.5) * A.res, nn = A.yoff - ((double)j + 0.5) * A.res;
    a = (double)A.dsm[c];
    bad0 = utm_geodetic(A.U, e, nn, lon, lat);
  }

  int32_t n = 0, best = -1, best_rank = 0;
  double m[C], M2[C];
  uint32_t bv[C];
#pragma unroll
  for (int ch = 0; ch < C; ++ch) { m[ch] = 0.0; M2[ch] = 0.0; bv[ch] = F32_NAN_BITS; }

  for (int k = 0; k < A.K; ++k) {
    const bn_mosaic_view &V = A.views[k];                            // k is the same in every lane: scalar loads
    int st = -1;                                                     // a lane outside the band counts nowhere
    if (live) {
      uint32_t v[C];
      st = view_step::add_view<C>(V, A.colrow_in ? A.colrow_in + 2 * ((int64_t)k * A.HW + c) : nullptr, c, bad0, lon, lat, a, A.mode, n,
                                  m, M2, v);
      if (st == BN_MOSAIC_USED && (n == 1 || V.rank < best_rank)) {
        best = k;
        best_rank = V.rank;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) bv[ch] = v[ch];
      }
    }
#pragma unroll
    for (int s = 0; s < 5; ++s) {
      const unsigned long long ballot = __ballot(st == s);
      if ((threadIdx.x & 63) == 0 && ballot) atomicAdd(&table[k * 5 + s], (unsigned int)__popcll(ballot));       // LDS, integer
    }
  }

  long long cells = 0, q = 0, skipped = 0;
  if (live) {
    A.count[c] = (uint8_t)n;
    if (A.best) A.best[c] = best;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
      const double s = n ? sqrt(M2[ch] / (double)n) : 0.0;
      if (A.best_val) A.best_val[ch * A.HW + c] = bv[ch];
      if (A.mean) A.mean[ch * A.HW + c] = n ? (float)m[ch] : __uint_as_float(F32_NAN_BITS);
      if (A.std) A.std[ch * A.HW + c] = n ? (float)s : __uint_as_float(F32_NAN_BITS);
      if (n >= 2) {
        if (s < Q20) q += llrint(s * Q20);
        else skipped += 1;
      }
    }
    cells = n >= 2 ? 1 : 0;
  }

  __syncthreads();
  for (int t = threadIdx.x; t < A.K * 5; t += MOS_BLOCK)
    if (table[t]) atomicAdd(A.counts + t, (unsigned long long)table[t]);
  if (A.sums) {
    const long long v3[3] = {cells, q, skipped};
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const long long s = block_sums::block_sum(v3[t], red);
      if (threadIdx.x == 0 && s != 0) atomicAdd(A.sums + t, (unsigned long long)s);
    }
  }
}

}  // namespace

extern "C" int bn_grid_mosaic(const bn_mosaic_view *views_host, const bn_mosaic_view *views_dev, int32_t K, int32_t C,
                              const float *dsm, int32_t H, int32_t W, double xoff, double yoff, double res, int32_t row0,
                              int32_t row1, int32_t zone, int32_t south, int32_t mode, const double *colrow_in, uint8_t *count,
                              int32_t *best, float *best_val, float *mean, float *std, unsigned long long *counts,
                              unsigned long long *sums, void *stream) {
  BN_REQUIRE(views_host && views_dev && dsm && count && counts, "grid_mosaic: null argument");
  if (view_step::check_views_on_grid("grid_mosaic", views_host, K, C, H, W, xoff, yoff, res, row0, row1, zone, south, mode)) return BN_EINVAL;
  if (row0 == row1) return 0;
  MosaicArgs a;
  a.views = views_dev; a.dsm = dsm; a.colrow_in = colrow_in;
  a.K = K; a.mode = mode; a.W = W; a.row0 = row0;
  a.n = (int64_t)(row1 - row0) * W; a.HW = (int64_t)H * W;
  a.xoff = xoff; a.yoff = yoff; a.res = res;
  a.U = make_utm_inv(zone, south);
  a.count = count; a.best = best; a.best_val = reinterpret_cast<uint32_t *>(best_val); a.mean = mean; a.std = std;
  a.counts = counts; a.sums = sums;
  const unsigned blocks = (unsigned)ceil_div64(a.n, MOS_BLOCK);
  hipStream_t s = (hipStream_t)stream;
  switch (C) {
    case 1: grid_mosaic_kernel<1><<<blocks, MOS_BLOCK, 0, s>>>(a); break;
    case 2: grid_mosaic_kernel<2><<<blocks, MOS_BLOCK, 0, s>>>(a); break;
    case 3: grid_mosaic_kernel<3><<<blocks, MOS_BLOCK, 0, s>>>(a); break;
    default: grid_mosaic_kernel<4><<<blocks, MOS_BLOCK, 0, s>>>(a); break;
  }
  BN_LAUNCH_CHECK("grid_mosaic");
  return 0;
}
