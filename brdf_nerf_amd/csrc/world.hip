// The surface model of an ECEF scene: a ray's surface point taken from the scene's world coordinates to (east, north, altitude),
// and world points splatted into the DSM accumulator of dsm.hip.
//
// The reference converts on the host (datasets/satellite_rgb_dep.py:629-631: sat_utils.ecef_to_latlon_custom, then
// utm_from_latlon through pyproj); datasets/cal_rmse_depth.py:15-64 rasterises a view's tie points the same way.  Here, one lane
// per ray or per point, three device functions (surface_cell.h, shared with ortho.hip) that every kernel below is made of:
//
//   surface_point  P = (o + d depth) range + center as dsm.hip forms it; cs = ecef: P through geodesy.h's ecef_geodetic (Bowring's
//                  one-step formula with upstream's truncated eccentricity) and the UTM series of geo_world in the SCENE's zone
//   refused        a point on the axis, or with a non-finite coordinate at any stage: NaN, counted
//   deposit        the cell, footprint and integer deposit of bn_dsm_splat, on a given (east, north, altitude)
//
// bn_dsm_splat_world runs surface_point and deposit in one lane with no cloud in between; bn_surface_points followed by
// bn_dsm_splat_points runs the same two functions in two launches, so both give the same accumulator bits.  For cs = utm a
// world point already is (east, north, altitude) and the accumulator is bn_dsm_splat's bit for bit.
// Integer atomics only.  The rows a kernel leaves out are summed per block and added with ONE integer atomic.
// The ECEF chain has some 30 float64 transcendentals per point (4 atan2, 13 sin / cos, 2 atanh, 3 sinh / cosh).
// As the compiler reports them for gfx950: ecef_geodetic_kernel 64, surface_points_kernel 64, dsm_splat_points_kernel 18 and
// dsm_splat_world_kernel 62 VGPRs; none uses scratch, all run 8 waves per SIMD.
#include <cmath>
#include "common.h"
#include "brdfnerf_hip.h"
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
  count_block(bad, skipped);
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
  count_block(bad, skipped);
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
  count_block(bad, skipped);
}

__global__ __launch_bounds__(WORLD_BLOCK)
void dsm_splat_world_kernel(const PointArgs A, const ToEnz T, const GridArgs G, unsigned long long *__restrict__ acc,
                            unsigned long long *__restrict__ skipped) {
  const int64_t ray = (int64_t)blockIdx.x * WORLD_BLOCK + threadIdx.x;
  bool bad = false;
  if (ray < A.R) {
    double e, n, a;
    surface_point(A, T, ray, e, n, a);             // a refused point is NaN, which deposit skips
    bad = deposit(G, e, n, a, acc);
  }
  count_block(bad, skipped);
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
  WORLD_REQUIRE_FRAME("surface_points");
  WORLD_REQUIRE_CS("surface_points");
  if (R == 0) return 0;
  const PointArgs a{rays, depth, ray_stride, R, center[0], center[1], center[2], range};
  surface_points_kernel<<<(unsigned)ceil_div64(R, WORLD_BLOCK), WORLD_BLOCK, 0, (hipStream_t)stream>>>(a, make_to_enz(cs, zone, south), enz,
                                                                                                     skipped);
  BN_LAUNCH_CHECK("surface_points");
  return 0;
}

extern "C" int bn_dsm_splat_points(const double *enz, int64_t stride, int64_t n, double xoff, double yoff, double resolution, int32_t W,
                                   int32_t H, int32_t radius, int32_t footprint, long long *acc, unsigned long long *skipped,
                                   void *stream) {
  BN_REQUIRE(enz && acc && skipped, "dsm_splat_points: null argument");
  BN_REQUIRE(n >= 0 && n <= WORLD_MAX_ROWS && stride >= 3, "dsm_splat_points: n=%lld rows of %lld doubles (a point takes 3)", (long long)n,
             (long long)stride);
  WORLD_REQUIRE_GRID("dsm_splat_points");
  if (n == 0) return 0;
  const GridArgs g{xoff, yoff, resolution, W, H, radius, footprint == BN_DSM_DISC};
  dsm_splat_points_kernel<<<(unsigned)ceil_div64(n, WORLD_BLOCK), WORLD_BLOCK, 0, (hipStream_t)stream>>>(
      enz, stride, n, g, reinterpret_cast<unsigned long long *>(acc), skipped);
  BN_LAUNCH_CHECK("dsm_splat_points");
  return 0;
}

extern "C" int bn_dsm_splat_world(const float *rays, int64_t ray_stride, const float *depth, int64_t R, const double *center, double range,
                                  double xoff, double yoff, double resolution, int32_t W, int32_t H, int32_t radius, int32_t footprint,
                                  int32_t cs, int32_t zone, int32_t south, long long *acc, unsigned long long *skipped, void *stream) {
  BN_REQUIRE(rays && depth && center && acc && skipped, "dsm_splat_world: null argument");
  WORLD_REQUIRE_FRAME("dsm_splat_world");
  WORLD_REQUIRE_GRID("dsm_splat_world");
  WORLD_REQUIRE_CS("dsm_splat_world");
  if (R == 0) return 0;
  const PointArgs a{rays, depth, ray_stride, R, center[0], center[1], center[2], range};
  const GridArgs g{xoff, yoff, resolution, W, H, radius, footprint == BN_DSM_DISC};
  dsm_splat_world_kernel<<<(unsigned)ceil_div64(R, WORLD_BLOCK), WORLD_BLOCK, 0, (hipStream_t)stream>>>(
      a, make_to_enz(cs, zone, south), g, reinterpret_cast<unsigned long long *>(acc), skipped);
  BN_LAUNCH_CHECK("dsm_splat_world");
  return 0;
}
