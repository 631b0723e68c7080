// The orthophoto of an observed image on the grid of a surface model: every cell of a DSM is taken to the pixel of a satellite
// image that saw it, and the image is gathered there.  ortho.hip splats a VIEW's rays into cells (the forward direction); this
// file is the opposite one.  include/brdfnerf_hip.h ("Orthophoto of an observed image") states the rule operation by operation.
// It has NO upstream counterpart - the reference never orthorectifies an image and reaches UTM only forwards, through pyproj - so
// the rule is this project's own and there is nothing to check it against but its statement and the project's forward series.
//
//   utm_geodetic_kernel   (east, north) -> (lon, lat) in degrees: geodesy.h's utm_geodetic, one lane per point
//   grid_pixels_kernel    cell centre and DSM altitude -> utm_geodetic -> rpc_poly.h's project, one lane per cell of rows
//                         [row0, row1): float64, every operation rounded on its own.  utm_geodetic followed by project are the
//                         SAME device functions as bn_utm_geodetic followed by bn_rpc_project, and after the geodetic point only
//                         + x / occur, so the fused launch gives the two-launch chain's bits
//   image_gather_kernel   one lane per cell of [n0, n1): the state of the cell (no data, outside, occluded, kept), then the
//                         bilinear taps in float64 or the nearest pixel's 32 bits, channel after channel through element strides
//                         (gather_rule.h: the state, the taps and the expression, shared with mosaic.hip)
//
// The descriptor's 80 coefficients travel in the kernel arguments (as in rpc_project_kernel): a wave reads them through the scalar
// cache once.  Counted cells and the four states are summed per block and added with ONE integer atomic per counter
// (block_sums.h); there is no float atomic in this file, and every output is a plain store of the lane's own cell: every bit
// depends on the inputs alone, not on blocks, row bands, cell ranges or the number of ranks.
#include <cmath>
#include "common.h"
#include "brdfnerf_hip.h"
#include "block_sums.h"
#include "gather_rule.h"
#include "geodesy.h"
#include "rpc_poly.h"
// every float64 operation below is rounded on its own (see above); the build also passes -ffp-contract=off for this file
#pragma clang fp contract(off)

namespace {

using namespace geodesy;

constexpr int OPH_BLOCK = 256;
constexpr int64_t OPH_MAX_CELLS = (int64_t)1 << 30;

__global__ __launch_bounds__(OPH_BLOCK)
void utm_geodetic_kernel(const UtmInvK K, const double *__restrict__ en, int64_t n, double *__restrict__ lonlat,
                         unsigned long long *__restrict__ skipped) {
  const int64_t i = (int64_t)blockIdx.x * OPH_BLOCK + threadIdx.x;
  bool bad = false;
  if (i < n) {
    double lon, lat;
    bad = utm_geodetic(K, en[2 * i], en[2 * i + 1], lon, lat);
    lonlat[2 * i] = lon;
    lonlat[2 * i + 1] = lat;
  }
  block_sums::block_count(bad, skipped);
}

struct CellGrid {
  const float *dsm;
  int32_t W, row0;
  int64_t n;                     // cells of the band: (row1 - row0) W
  double xoff, yoff, res;
};

__global__ __launch_bounds__(OPH_BLOCK)
void grid_pixels_kernel(const bn_rpc R, const UtmInvK K, const CellGrid G, double *__restrict__ colrow,
                        unsigned long long *__restrict__ counts) {
  const int64_t k = (int64_t)blockIdx.x * OPH_BLOCK + threadIdx.x;
  bool bad = false;
  if (k < G.n) {
    const int64_t c = (int64_t)G.row0 * G.W + k;                    // below H W <= 2^30
    const int64_t j = c / G.W, i = c - j * G.W;
    const double e = G.xoff + ((double)i + 0.5) * G.res, nn = G.yoff - ((double)j + 0.5) * G.res;
    const double a = (double)G.dsm[c];
    double lon, lat, col, row;
    bad = utm_geodetic(K, e, nn, lon, lat);
    rpc_poly::project(R, lon, lat, a, col, row);
    bad = bad || !(isfinite(a) && isfinite(col) && isfinite(row));
    colrow[2 * c] = bad ? __builtin_nan("") : col;
    colrow[2 * c + 1] = bad ? __builtin_nan("") : row;
  }
  block_sums::block_count(bad, counts);
}

struct GatherArgs {
  const float *img;
  int32_t Hi, Wi, C, mode;
  int64_t s_row, s_col, s_chan, n0, n1, out_chan_stride;
  const double *colrow;
  const uint8_t *vis;
  float *out;
  uint8_t *state;
  unsigned long long *counts;
};

__global__ __launch_bounds__(OPH_BLOCK)
void image_gather_kernel(const GatherArgs A) {
  const int64_t c = A.n0 + (int64_t)blockIdx.x * OPH_BLOCK + threadIdx.x;
  int st = -1;                                   // a lane outside the range counts nowhere
  if (c < A.n1) {
    const double col = A.colrow[2 * c], row = A.colrow[2 * c + 1];
    st = gather_rule::cell_state(col, row, A.Hi, A.Wi, A.vis, c);
    A.state[c] = (uint8_t)st;
    float *out = A.out + c;
    if (st != BN_GATHER_KEPT) {
      for (int ch = 0; ch < A.C; ++ch) out[ch * A.out_chan_stride] = __builtin_nanf("");
    } else if (A.mode == BN_GATHER_NEAREST) {
      const int64_t at = gather_rule::nearest_at(col, row, A.Hi, A.Wi, A.s_row, A.s_col);
      const uint32_t *src = reinterpret_cast<const uint32_t *>(A.img);
      uint32_t *dst = reinterpret_cast<uint32_t *>(out);
      for (int ch = 0; ch < A.C; ++ch) dst[ch * A.out_chan_stride] = src[at + ch * A.s_chan];      // the pixel's 32 bits
    } else {
      const gather_rule::Taps4 t = gather_rule::bilinear_taps(col, row, A.Hi, A.Wi, A.s_row, A.s_col);
      for (int ch = 0; ch < A.C; ++ch) out[ch * A.out_chan_stride] = gather_rule::bilinear(A.img + ch * A.s_chan, t);
    }
  }
  for (int s = 0; s < 4; ++s) block_sums::block_count(st == s, A.counts + s);
}

int require_zone(const char *who, int32_t zone, int32_t south) {
  BN_REQUIRE(zone >= 1 && zone <= 60, "%s: zone=%d outside [1, 60]", who, zone);
  BN_REQUIRE(south == 0 || south == 1, "%s: south=%d (0 or 1)", who, south);
  return 0;
}

}  // namespace

extern "C" int bn_utm_geodetic(const double *en, int64_t n, int32_t zone, int32_t south, double *lonlat, unsigned long long *skipped,
                               void *stream) {
  BN_REQUIRE(en && lonlat && skipped, "utm_geodetic: null argument");
  BN_REQUIRE(n >= 0 && n <= OPH_MAX_CELLS, "utm_geodetic: n=%lld (0 to 2^30)", (long long)n);
  if (int bad = require_zone("utm_geodetic", zone, south)) return bad;
  if (n == 0) return 0;
  utm_geodetic_kernel<<<(unsigned)ceil_div64(n, OPH_BLOCK), OPH_BLOCK, 0, (hipStream_t)stream>>>(make_utm_inv(zone, south), en, n, lonlat,
                                                                                             skipped);
  BN_LAUNCH_CHECK("utm_geodetic");
  return 0;
}

extern "C" int bn_grid_pixels(const bn_rpc *rpc, const float *dsm, int32_t H, int32_t W, double xoff, double yoff, double res,
                              int32_t row0, int32_t row1, int32_t zone, int32_t south, double *colrow, unsigned long long *counts,
                              void *stream) {
  BN_REQUIRE(rpc && dsm && colrow && counts, "grid_pixels: null argument");
  BN_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= OPH_MAX_CELLS, "grid_pixels: grid %d x %d (H W from 1 to 2^30 cells)", H, W);
  BN_REQUIRE(0 <= row0 && row0 <= row1 && row1 <= H, "grid_pixels: rows [%d, %d) outside [0, %d)", row0, row1, H);
  BN_REQUIRE(res > 0.0 && std::isfinite(res), "grid_pixels: resolution %g must be positive and finite", res);
  BN_REQUIRE(std::isfinite(xoff) && std::isfinite(yoff), "grid_pixels: grid origin (%g, %g) is not finite", xoff, yoff);
  if (int bad = require_zone("grid_pixels", zone, south)) return bad;
  BN_REQUIRE(rpc_poly::rpc_ok(rpc), "grid_pixels: the descriptor has a zero scale or a non-finite entry");
  if (row0 == row1) return 0;
  const CellGrid G{dsm, W, row0, (int64_t)(row1 - row0) * W, xoff, yoff, res};
  grid_pixels_kernel<<<(unsigned)ceil_div64(G.n, OPH_BLOCK), OPH_BLOCK, 0, (hipStream_t)stream>>>(*rpc, make_utm_inv(zone, south), G, colrow,
                                                                                              counts);
  BN_LAUNCH_CHECK("grid_pixels");
  return 0;
}

extern "C" int bn_image_gather(const float *img, int32_t Hi, int32_t Wi, int32_t C, int64_t s_row, int64_t s_col, int64_t s_chan,
                               const double *colrow, const uint8_t *vis, int64_t n0, int64_t n1, int32_t mode, float *out,
                               int64_t out_chan_stride, uint8_t *state, unsigned long long *counts, void *stream) {
  BN_REQUIRE(img && colrow && out && state && counts, "image_gather: null argument");
  BN_REQUIRE(C >= 1 && C <= BN_GATHER_MAX_CHANNELS, "image_gather: C=%d channels outside [1, %d]", C, BN_GATHER_MAX_CHANNELS);
  BN_REQUIRE(Hi >= 1 && Wi >= 1, "image_gather: an image of %d x %d pixels", Hi, Wi);
  BN_REQUIRE(s_row >= 0 && s_col >= 0 && s_chan >= 0 && out_chan_stride >= 0, "image_gather: a negative stride (%lld, %lld, %lld; %lld)",
             (long long)s_row, (long long)s_col, (long long)s_chan, (long long)out_chan_stride);
  BN_REQUIRE(n0 >= 0 && n0 <= n1 && n1 <= OPH_MAX_CELLS, "image_gather: cells [%lld, %lld) (0 <= n0 <= n1 <= 2^30)", (long long)n0,
             (long long)n1);
  BN_REQUIRE(mode == BN_GATHER_BILINEAR || mode == BN_GATHER_NEAREST, "image_gather: mode=%d (BN_GATHER_BILINEAR or BN_GATHER_NEAREST)",
             mode);
  if (n0 == n1) return 0;
  GatherArgs a;
  a.img = img; a.Hi = Hi; a.Wi = Wi; a.C = C; a.mode = mode;
  a.s_row = s_row; a.s_col = s_col; a.s_chan = s_chan; a.n0 = n0; a.n1 = n1; a.out_chan_stride = out_chan_stride;
  a.colrow = colrow; a.vis = vis; a.out = out; a.state = state; a.counts = counts;
  image_gather_kernel<<<(unsigned)ceil_div64(n1 - n0, OPH_BLOCK), OPH_BLOCK, 0, (hipStream_t)stream>>>(a);
  BN_LAUNCH_CHECK("image_gather");
  return 0;
}
