// Digital surface model (DSM) of a rendered view: the rays' depths splatted into a geo-referenced altitude grid, deterministically,
// for a scene whose world coordinates are UTM or ECEF.
//
// The reference builds the point cloud in numpy on the host (datasets/satellite_rgb_dep.py:601-634, cs == 'utm': a denormalised
// point IS (east, north, altitude), :632-633) and rasterises it with plyflatten(cloud, xoff, yoff, resolution, xsize, ysize,
// radius=1, sigma=inf) (:636-699): the unweighted mean altitude of the points whose footprint covers a cell, NaN where none does
// (:693), row 0 at the northern edge (the affine transform of :695).  Here a lane owns a ray:
//
//   point      p = (o + d depth) range + center in float64, the fp32 inputs widened exactly and EVERY operation rounded on its
//              own (this file is compiled with fp contraction off: fp32 cannot hold a UTM northing of ~3.4e6 m at a 0.5 m cell,
//              and a fused multiply-add would round differently from numpy at cell boundaries)
//   cell       column i from (p.x - xoff) / resolution and row j from (yoff - p.y) / resolution, each rounded down, both in float64
//              (point_cell of surface_cell.h spells the expression, once)
//   footprint  cells (j + k2, i + k1), k1, k2 in [-radius, radius] (BN_DSM_DISC: k1^2 + k2^2 <= radius^2), each tested against
//              the grid on its own - a point whose centre cell lies outside still reaches its neighbours inside
//   deposit    q = llrint(p.z 2^20) added to the cell's 64-bit sum with an INTEGER atomic, 1 to its count
//
// Integer addition is associative, so the accumulator's bits do not depend on the lane order, on how a view is chunked, or on
// which GPU splatted which ray; there is no float atomic in this file.  A row with a non-finite p or |p.z| >= 2^23 m deposits
// nothing and is counted in skipped[0]: |q| <= 2^43, so a cell's sum cannot overflow before it holds 2^20 points.
// The footprint rule is the statement above (the issue's specification), not the plyflatten package, which this project neither
// depends on nor was checked against.
// The sum and the count go in as two 8-byte atomics: gfx950 has no 16-byte atomic add, and a compare-and-swap loop on the pair
// would retry under exactly the contention the pair was meant to help with.  A near-nadir view at its own ground sampling
// distance puts about one ray centre per cell (neighbouring lanes -> neighbouring cells of a row); every point on ONE cell
// serialises in the L2 and is merely correct.
//
// An ECEF scene: the reference converts on the host (datasets/satellite_rgb_dep.py:629-631: sat_utils.ecef_to_latlon_custom, then
// utm_from_latlon through pyproj); datasets/cal_rmse_depth.py:15-64 rasterises a view's tie points the same way.  Here, one lane
// per ray or per point, every kernel below is made of the device functions of surface_cell.h (shared with ortho.hip): surface_point,
// the point above, for cs = ecef taken to (east, north, altitude) in the SCENE's zone, NaN and counted when refused; and deposit.
// bn_dsm_splat_world runs surface_point and deposit in one lane with no cloud in between; bn_surface_points followed by
// bn_dsm_splat_points runs the same two functions in two launches, so both give the same accumulator bits.  bn_dsm_splat IS
// bn_dsm_splat_world with cs = utm: one kernel, instantiated with and without the ECEF conversion, and the host picks by cs.
// Integer atomics only.  The rows a kernel leaves out are summed per block and added with ONE integer atomic.
// The ECEF chain has some 30 float64 transcendentals per point (4 atan2, 13 sin / cos, 2 atanh, 3 sinh / cosh).
// As the compiler reports them for gfx950: ecef_geodetic_kernel 64, surface_points_kernel 64, dsm_splat_points_kernel 18,
// dsm_splat_world_kernel 62 with the conversion and 18 without, dsm_resolve_kernel 16 VGPRs; 4 B of LDS (the block's counter) in
// each but dsm_resolve_kernel, which has none; none uses scratch, all run 8 waves per SIMD.
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

__global__ __launch_bounds__(WORLD_BLOCK)
void ecef_geodetic_kernel(const EcefK K, const double *__restrict__ xyz, int64_t n, double *__restrict__ lonlat,
                          double *__restrict__ alt, unsigned long long *__restrict__ skipped) {
  const int64_t i = (int64_t)blockIdx.x * WORLD_BLOCK + threadIdx.x;
  bool bad = false;
  if (i < n) {
    double lon, lat, a;
    bad = ecef_geodetic(K, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], lon, lat, a);
    lonlat[2 * i] = bad ? __builtin_nan("") : lon;
    lonlat[2 * i + 1] = bad ? __builtin_nan("") : lat;
    alt[i] = bad ? __builtin_nan("") : a;
  }
  block_sums::block_count(bad, skipped);
}

__global__ __launch_bounds__(WORLD_BLOCK)
void surface_points_kernel(const PointArgs A, const ToEnz T, double *__restrict__ enz, unsigned long long *__restrict__ skipped) {
  const int64_t ray = (int64_t)blockIdx.x * WORLD_BLOCK + threadIdx.x;
  bool bad = false;
  if (ray < A.R) {
    double e, n, a;
    bad = surface_point(A, T, ray, e, n, a);
    enz[3 * ray] = e;
    enz[3 * ray + 1] = n;
    enz[3 * ray + 2] = a;
  }
  block_sums::block_count(bad, skipped);
}

__global__ __launch_bounds__(WORLD_BLOCK)
void dsm_splat_points_kernel(const double *__restrict__ enz, int64_t stride, int64_t n, const GridArgs G,
                             unsigned long long *__restrict__ acc, unsigned long long *__restrict__ skipped) {
  const int64_t i = (int64_t)blockIdx.x * WORLD_BLOCK + threadIdx.x;
  bool bad = false;
  if (i < n) {
    const double *p = enz + i * stride;
    bad = deposit(G, p[0], p[1], p[2], acc);
  }
  block_sums::block_count(bad, skipped);
}

// ECEF: the conversion is compiled in (and taken when T.ecef says so) or out.  No lane returns before block_count
template <bool ECEF> __global__ __launch_bounds__(WORLD_BLOCK)
void dsm_splat_world_kernel(const PointArgs A, const ToEnz T, const GridArgs G, unsigned long long *__restrict__ acc,
                            unsigned long long *__restrict__ skipped) {
  const int64_t ray = (int64_t)blockIdx.x * WORLD_BLOCK + threadIdx.x;
  bool bad = false;
  if (ray < A.R) {
    double e, n, a;
    surface_point<ECEF>(A, T, ray, e, n, a);       // a refused point is NaN, which deposit skips
    bad = deposit(G, e, n, a, acc);
  }
  block_sums::block_count(bad, skipped);
}

__global__ __launch_bounds__(WORLD_BLOCK)
void dsm_resolve_kernel(const long long *__restrict__ acc, int64_t n, float *__restrict__ dsm, int32_t *__restrict__ count) {
  const int64_t c = (int64_t)blockIdx.x * WORLD_BLOCK + threadIdx.x;
  if (c >= n) return;
  const longlong2 sc = reinterpret_cast<const longlong2 *>(acc)[c];          // (sum, count): one 16-byte load
  dsm[c] = cell_mean(sc.x, sc.y, DSM_FIX);
  if (count) count[c] = cell_count(sc.y);
}

// bn_dsm_splat (cs = utm) and bn_dsm_splat_world under the name `what`
int splat_rays(const char *what, const float *rays, int64_t ray_stride, const float *depth, int64_t R, const double *center, double range,
               double xoff, double yoff, double resolution, int32_t W, int32_t H, int32_t radius, int32_t footprint, int32_t cs,
               int32_t zone, int32_t south, long long *acc, unsigned long long *skipped, void *stream) {
  BN_REQUIRE(rays && depth && center && acc && skipped, "%s: null argument", what);
  if (int bad = require_rays(what, R, ray_stride, center, range, cs, zone, south)) return bad;
  if (int bad = require_grid(what, acc, xoff, yoff, resolution, W, H, radius, footprint)) return bad;
  if (R == 0) return 0;
  const auto kernel = cs == BN_CS_ECEF ? dsm_splat_world_kernel<true> : dsm_splat_world_kernel<false>;
  kernel<<<(unsigned)ceil_div64(R, WORLD_BLOCK), WORLD_BLOCK, 0, (hipStream_t)stream>>>(
      make_point_args(rays, ray_stride, depth, R, center, range), make_to_enz(cs, zone, south),
      make_grid_args(xoff, yoff, resolution, W, H, radius, footprint), reinterpret_cast<unsigned long long *>(acc), skipped);
  BN_LAUNCH_CHECK(what);
  return 0;
}

}  // namespace

extern "C" int bn_ecef_geodetic(const double *xyz, int64_t n, double *lonlat, double *alt, unsigned long long *skipped, void *stream) {
  BN_REQUIRE(xyz && lonlat && alt && skipped, "ecef_geodetic: null argument");
  BN_REQUIRE(n >= 0 && n <= WORLD_MAX_ROWS, "ecef_geodetic: n=%lld", (long long)n);
  if (n == 0) return 0;
  ecef_geodetic_kernel<<<(unsigned)ceil_div64(n, WORLD_BLOCK), WORLD_BLOCK, 0, (hipStream_t)stream>>>(make_ecef_k(), xyz, n, lonlat, alt,
                                                                                                    skipped);
  BN_LAUNCH_CHECK("ecef_geodetic");
  return 0;
}

extern "C" int bn_surface_points(const float *rays, int64_t ray_stride, const float *depth, int64_t R, const double *center, double range,
                                 int32_t cs, int32_t zone, int32_t south, double *enz, unsigned long long *skipped, void *stream) {
  BN_REQUIRE(rays && depth && center && enz && skipped, "surface_points: null argument");
  if (int bad = require_rays("surface_points", R, ray_stride, center, range, cs, zone, south)) return bad;
  if (R == 0) return 0;
  surface_points_kernel<<<(unsigned)ceil_div64(R, WORLD_BLOCK), WORLD_BLOCK, 0, (hipStream_t)stream>>>(
      make_point_args(rays, ray_stride, depth, R, center, range), make_to_enz(cs, zone, south), enz, skipped);
  BN_LAUNCH_CHECK("surface_points");
  return 0;
}

extern "C" int bn_dsm_splat_points(const double *enz, int64_t stride, int64_t n, double xoff, double yoff, double resolution, int32_t W,
                                   int32_t H, int32_t radius, int32_t footprint, long long *acc, unsigned long long *skipped,
                                   void *stream) {
  BN_REQUIRE(enz && acc && skipped, "dsm_splat_points: null argument");
  BN_REQUIRE(n >= 0 && n <= WORLD_MAX_ROWS && stride >= 3, "dsm_splat_points: n=%lld rows of %lld doubles (a point takes 3)", (long long)n,
             (long long)stride);
  if (int bad = require_grid("dsm_splat_points", acc, xoff, yoff, resolution, W, H, radius, footprint)) return bad;
  if (n == 0) return 0;
  dsm_splat_points_kernel<<<(unsigned)ceil_div64(n, WORLD_BLOCK), WORLD_BLOCK, 0, (hipStream_t)stream>>>(
      enz, stride, n, make_grid_args(xoff, yoff, resolution, W, H, radius, footprint), reinterpret_cast<unsigned long long *>(acc), skipped);
  BN_LAUNCH_CHECK("dsm_splat_points");
  return 0;
}

extern "C" int bn_dsm_splat(const float *rays, int64_t ray_stride, const float *depth, int64_t R, const double *center, double range,
                            double xoff, double yoff, double resolution, int32_t W, int32_t H, int32_t radius, int32_t footprint,
                            long long *acc, unsigned long long *skipped, void *stream) {
  return splat_rays("dsm_splat", rays, ray_stride, depth, R, center, range, xoff, yoff, resolution, W, H, radius, footprint, BN_CS_UTM, 1, 0,
                    acc, skipped, stream);
}

extern "C" int bn_dsm_splat_world(const float *rays, int64_t ray_stride, const float *depth, int64_t R, const double *center, double range,
                                  double xoff, double yoff, double resolution, int32_t W, int32_t H, int32_t radius, int32_t footprint,
                                  int32_t cs, int32_t zone, int32_t south, long long *acc, unsigned long long *skipped, void *stream) {
  return splat_rays("dsm_splat_world", rays, ray_stride, depth, R, center, range, xoff, yoff, resolution, W, H, radius, footprint, cs, zone,
                    south, acc, skipped, stream);
}

extern "C" int bn_dsm_resolve(const long long *acc, int32_t W, int32_t H, float *dsm, int32_t *count, void *stream) {
  BN_REQUIRE(acc && dsm, "dsm_resolve: null argument");
  BN_REQUIRE(((uintptr_t)acc & 15) == 0, "dsm_resolve: acc must be 16-byte aligned");
  BN_REQUIRE(W > 0 && H > 0 && (int64_t)W * H <= ((int64_t)1 << 31), "dsm_resolve: grid %d x %d (W H at most 2^31 cells)", W, H);
  const int64_t n = (int64_t)W * H;
  dsm_resolve_kernel<<<(unsigned)ceil_div64(n, WORLD_BLOCK), WORLD_BLOCK, 0, (hipStream_t)stream>>>(acc, n, dsm, count);
  BN_LAUNCH_CHECK("dsm_resolve");
  return 0;
}
