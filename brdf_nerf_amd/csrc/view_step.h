// Step 3 a - e of "Orthomosaic of several observed images" (include/brdfnerf_hip.h): what ONE view adds to a cell's running values -
// the pixel under the view's RPC (or the pixel given), gather_rule.h's state, the C values in `mode`, their finiteness and Welford's
// update of the C means and sums of squares in float64.  Shared by mosaic.hip (grid_mosaic_kernel: the views of one altitude) and
// sweep.hip (grid_sweep_kernel: the views of every altitude of a list): one statement, so that a view's contribution is the same
// bits wherever it is formed.  Both files are built with fp contraction off and the pragma below covers the function wherever it
// is included.
#pragma once
#include <cmath>
#include "common.h"
#include "brdfnerf_hip.h"
#include "gather_rule.h"
#include "rpc_poly.h"
#pragma clang fp contract(off)

namespace view_step {

// View V on cell c.  pixel: (col, row) of this view and cell if the caller holds it, else NULL and the pixel is V.rpc's of (lon,
// lat, a), NaN in both if bad0 or a, col or row is not finite.  -> the view's state, 0 to 4; on BN_MOSAIC_USED n, m and M2 carry
// the view and v its C values (32 bits each), in every other state they are as they came.
template <int C>
__device__ __forceinline__ int add_view(const bn_mosaic_view &V, const double *pixel, int64_t c, bool bad0, double lon, double lat,
                                        double a, int32_t mode, int32_t &n, double (&m)[C], double (&M2)[C], uint32_t (&v)[C]) {
  double col, row;
  if (pixel) {
    col = pixel[0];
    row = pixel[1];
  } else {
    rpc_poly::project(V.rpc, lon, lat, a, col, row);
    if (bad0 || !(isfinite(a) && isfinite(col) && isfinite(row))) col = row = __builtin_nan("");
  }
  const int st = gather_rule::cell_state(col, row, V.Hi, V.Wi, V.vis, c);
  if (st != BN_GATHER_KEPT) return st;
  if (mode == BN_GATHER_NEAREST) {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(V.img) + gather_rule::nearest_at(col, row, V.Hi, V.Wi, V.s_row, V.s_col);
#pragma unroll
    for (int ch = 0; ch < C; ++ch) v[ch] = src[ch * V.s_chan];                       // the pixel's 32 bits
  } else {
    const gather_rule::Taps4 t = gather_rule::bilinear_taps(col, row, V.Hi, V.Wi, V.s_row, V.s_col);
#pragma unroll
    for (int ch = 0; ch < C; ++ch) v[ch] = __float_as_uint(gather_rule::bilinear(V.img + ch * V.s_chan, t));
  }
  bool finite = true;
#pragma unroll
  for (int ch = 0; ch < C; ++ch) finite = finite && isfinite(__uint_as_float(v[ch]));
  if (!finite) return BN_MOSAIC_NONFINITE;
  n = n + 1;
#pragma unroll
  for (int ch = 0; ch < C; ++ch) {
    const double x = (double)__uint_as_float(v[ch]);
    const double delta = x - m[ch];
    m[ch] = m[ch] + delta / (double)n;
    M2[ch] = M2[ch] + delta * (x - m[ch]);
  }
  return BN_MOSAIC_USED;
}

// What both entries refuse of the view table, the grid, the rows, the zone and the mode (host; `who` names the entry in the message)
static inline int check_views_on_grid(const char *who, const bn_mosaic_view *views_host, int32_t K, int32_t C, int32_t H, int32_t W,
                                      double xoff, double yoff, double res, int32_t row0, int32_t row1, int32_t zone, int32_t south,
                                      int32_t mode) {
  BN_REQUIRE(K >= 1 && K <= BN_MOSAIC_MAX_VIEWS, "%s: K=%d views outside [1, %d]", who, K, BN_MOSAIC_MAX_VIEWS);
  BN_REQUIRE(C >= 1 && C <= BN_MOSAIC_MAX_CHANNELS, "%s: C=%d channels outside [1, %d]", who, C, BN_MOSAIC_MAX_CHANNELS);
  BN_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= ((int64_t)1 << 30), "%s: grid %d x %d (H W from 1 to 2^30 cells)", who, H, W);
  BN_REQUIRE(0 <= row0 && row0 <= row1 && row1 <= H, "%s: rows [%d, %d) outside [0, %d)", who, row0, row1, H);
  BN_REQUIRE(res > 0.0 && std::isfinite(res), "%s: resolution %g must be positive and finite", who, res);
  BN_REQUIRE(std::isfinite(xoff) && std::isfinite(yoff), "%s: grid origin (%g, %g) is not finite", who, xoff, yoff);
  BN_REQUIRE(zone >= 1 && zone <= 60, "%s: zone=%d outside [1, 60]", who, zone);
  BN_REQUIRE(south == 0 || south == 1, "%s: south=%d (0 or 1)", who, south);
  BN_REQUIRE(mode == BN_GATHER_BILINEAR || mode == BN_GATHER_NEAREST, "%s: mode=%d (BN_GATHER_BILINEAR or BN_GATHER_NEAREST)", who, mode);
  for (int32_t k = 0; k < K; ++k) {
    const bn_mosaic_view &v = views_host[k];
    BN_REQUIRE(v.img, "%s: view %d has no image", who, k);
    BN_REQUIRE(v.Hi >= 1 && v.Wi >= 1, "%s: view %d has an image of %d x %d pixels", who, k, v.Hi, v.Wi);
    BN_REQUIRE(v.s_row >= 0 && v.s_col >= 0 && v.s_chan >= 0, "%s: view %d has a negative stride (%lld, %lld, %lld)", who, k,
               (long long)v.s_row, (long long)v.s_col, (long long)v.s_chan);
    BN_REQUIRE(rpc_poly::rpc_ok(&v.rpc), "%s: the descriptor of view %d has a zero scale or a non-finite entry", who, k);
  }
  return 0;
}

}  // namespace view_step
