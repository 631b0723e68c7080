// The surface model of an ECEF scene: a ray's surface point taken from the scene's world coordinates to (east, north, altitude),
// and world points splatted into the DSM accumulator of dsm.hip.
//
// The reference converts on the host (datasets/satellite_rgb_dep.py:629-631: sat_utils.ecef_to_latlon_custom, then
// utm_from_latlon through pyproj); datasets/cal_rmse_depth.py:15-64 rasterises a view's tie points the same way.  Here, one lane
// per ray or per point, three device functions that every kernel below is made of:
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
// every float64 operation below is rounded on its own (see above); the build also passes -ffp-contract=off for this file
#pragma clang fp contract(off)

namespace {

using namespace geodesy;

constexpr int WORLD_BLOCK = 256;
constexpr double DSM_FIX = 1048576.0;          // 2^20: altitudes are summed in units of 2^-20 m (dsm.hip)
constexpr double DSM_ZMAX = 8388608.0;         // 2^23 m
constexpr int64_t WORLD_MAX_ROWS = (int64_t)WORLD_BLOCK * 0x7fffffff;

struct PointArgs {
  const float *rays, *depth;
  int64_t ray_stride, R;
  double cx, cy, cz, range;
};

struct GridArgs {
  double xoff, yoff, resolution;
  int32_t W, H, radius, disc;
};

// what takes a world point of the scene to (east, north, altitude): nothing for a utm scene
struct ToEnz {
  int32_t ecef;
  EcefK K;
  World utm;
};

// (east, north, altitude) of a world point.  -> true when the point is refused (NaN then)
__device__ __forceinline__ bool world_enz(const ToEnz &T, double x, double y, double z, double &e, double &n, double &a) {
  bool bad;
  if (T.ecef) {
    double lon, lat;
    bad = ecef_geodetic(T.K, x, y, z, lon, lat, a);
    double up;
    geo_world(T.utm, lon, lat, a, e, n, up);
    bad = bad || !(isfinite(e) && isfinite(n));
  } else {
    e = x; n = y; a = z;
    bad = !(isfinite(x) && isfinite(y) && isfinite(z));
  }
  if (bad) e = n = a = __builtin_nan("");
  return bad;
}

__device__ __forceinline__ bool surface_point(const PointArgs &A, const ToEnz &T, int64_t ray, double &e, double &n, double &a) {
  const float *r = A.rays + ray * A.ray_stride;
  const double t = (double)A.depth[ray];
  const double px = ((double)r[0] + (double)r[3] * t) * A.range + A.cx;
  const double py = ((double)r[1] + (double)r[4] * t) * A.range + A.cy;
  const double pz = ((double)r[2] + (double)r[5] * t) * A.range + A.cz;
  return world_enz(T, px, py, pz, e, n, a);
}

// the deposit of bn_dsm_splat for one point.  -> true when the point is skipped
__device__ __forceinline__ bool deposit(const GridArgs &G, double px, double py, double pz, unsigned long long *__restrict__ acc) {
  if (!(isfinite(px) && isfinite(py) && isfinite(pz)) || !(fabs(pz) < DSM_ZMAX)) return true;
  const double fi = floor((px - G.xoff) / G.resolution);
  const double fj = floor((G.yoff - py) / G.resolution);
  const int rad = G.radius;
  // a footprint that cannot touch the grid (compared in float64: the cell index of a far point need not fit an integer)
  if (!(fi >= (double)(-rad) && fi <= (double)(G.W - 1 + rad) && fj >= (double)(-rad) && fj <= (double)(G.H - 1 + rad))) return false;
  const int i = (int)fi, j = (int)fj;
  const unsigned long long q = (unsigned long long)llrint(pz * DSM_FIX);      // two's complement: a negative altitude wraps
  for (int k2 = -rad; k2 <= rad; ++k2) {
    const int row = j + k2;
    if (row < 0 || row >= G.H) continue;
    for (int k1 = -rad; k1 <= rad; ++k1) {
      const int col = i + k1;
      if (col < 0 || col >= G.W) continue;
      if (G.disc && k1 * k1 + k2 * k2 > rad * rad) continue;
      unsigned long long *cell = acc + ((int64_t)row * G.W + col) * 2;
      atomicAdd(cell, q);
      atomicAdd(cell + 1, 1ull);
    }
  }
  return false;
}

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

ToEnz make_to_enz(int32_t cs, int32_t zone, int32_t south) {
  ToEnz t;
  t.ecef = cs == BN_CS_ECEF;
  t.K = make_ecef_k();
  t.utm = make_world(BN_CS_UTM, zone, south);
  return t;
}

}  // namespace

#define WORLD_REQUIRE_CS(what)                                                                                         \
  BN_REQUIRE(cs == BN_CS_ECEF || cs == BN_CS_UTM, what ": cs=%d (BN_CS_ECEF or BN_CS_UTM)", cs);                       \
  BN_REQUIRE(zone >= 1 && zone <= 60, what ": zone=%d outside [1, 60]", zone);                                         \
  BN_REQUIRE(south == 0 || south == 1, what ": south=%d (0 or 1)", south)

#define WORLD_REQUIRE_FRAME(what)                                                                                      \
  BN_REQUIRE(R >= 0 && R <= WORLD_MAX_ROWS && ray_stride >= 6, what ": R=%lld rows of %lld floats (origin and direction take 6)", \
             (long long)R, (long long)ray_stride);                                                                     \
  BN_REQUIRE(std::isfinite(range) && std::isfinite(center[0]) && std::isfinite(center[1]) && std::isfinite(center[2]), \
             what ": the frame must be finite")

#define WORLD_REQUIRE_GRID(what)                                                                                       \
  BN_REQUIRE(((uintptr_t)acc & 15) == 0, what ": acc must be 16-byte aligned");                                        \
  BN_REQUIRE(radius >= 0 && radius <= BN_DSM_MAX_RADIUS, what ": radius=%d outside [0, %d]", radius, BN_DSM_MAX_RADIUS); \
  BN_REQUIRE(footprint == BN_DSM_DISC || footprint == BN_DSM_SQUARE, what ": footprint=%d", footprint);                \
  BN_REQUIRE(resolution > 0 && std::isfinite(resolution), what ": resolution=%g must be positive", resolution);        \
  BN_REQUIRE(std::isfinite(xoff) && std::isfinite(yoff), what ": the grid origin must be finite");                     \
  BN_REQUIRE(W > 0 && H > 0 && (int64_t)W * H <= ((int64_t)1 << 31), what ": grid %d x %d (W H at most 2^31 cells)", W, H)

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
