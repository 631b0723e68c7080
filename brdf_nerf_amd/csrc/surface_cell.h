// The float64 point, cell and footprint chain of world.hip (the DSM of a view, of a scene in world coordinates) and ortho.hip (the
// orthorectified maps of a view), stated once: a ray's surface point taken to (east, north, altitude), the cell it falls in, the
// quantised altitude, the walk over its footprint and the deposit, as include/brdfnerf_hip.h states them for bn_dsm_splat /
// bn_dsm_splat_world and world.hip's head explains them; the mean of a cell; and what the host entries of both files refuse.
//
//   surface_point  P = (o + d depth) range + center; cs = ecef: P through geodesy.h's ecef_geodetic (Bowring's one-step formula
//                  with upstream's truncated eccentricity) and the UTM series of geo_world in the SCENE's zone
//   refused        a point on the axis, or with a non-finite coordinate at any stage: NaN
//   point_cell     the skip rule, the centre cell (j, i) and q = llrint(p.z 2^20) of bn_dsm_splat, on a given (east, north, altitude)
//   for_footprint  the cells (j + k2, i + k1) of the footprint that lie inside the grid, each tested on its own, in row-major order
//   deposit        point_cell, then q and 1 added to every footprint cell's (sum, count) with two integer atomics
//   cell_mean      sum / count in units of 1 / fix as float32, NaN at count 0; cell_count the saturated count
//
// Every operation is rounded on its own: both files are built with fp contraction off and the pragma below covers the functions
// here wherever they are included.
#pragma once
#include <cmath>
#include "common.h"
#include "brdfnerf_hip.h"
#include "geodesy.h"
#pragma clang fp contract(off)

namespace surface_cell {

using namespace geodesy;

constexpr int WORLD_BLOCK = 256;
constexpr double DSM_FIX = 1048576.0;          // 2^20: altitudes are summed in units of 2^-20 m
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

// (east, north, altitude) of a world point.  -> true when the point is refused (NaN then).  ECEF = false compiles the conversion
// out: what a kernel of utm scenes alone is made of (bn_dsm_splat is bn_dsm_splat_world's kernel instantiated so)
template <bool ECEF = true>
__device__ __forceinline__ bool world_enz(const ToEnz &T, double x, double y, double z, double &e, double &n, double &a) {
  bool bad;
  if (ECEF && T.ecef) {
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

template <bool ECEF = true>
__device__ __forceinline__ bool surface_point(const PointArgs &A, const ToEnz &T, int64_t ray, double &e, double &n, double &a) {
  const float *r = A.rays + ray * A.ray_stride;
  const double t = (double)A.depth[ray];
  const double px = ((double)r[0] + (double)r[3] * t) * A.range + A.cx;
  const double py = ((double)r[1] + (double)r[4] * t) * A.range + A.cy;
  const double pz = ((double)r[2] + (double)r[5] * t) * A.range + A.cz;
  return world_enz<ECEF>(T, px, py, pz, e, n, a);
}

// what point_cell makes of a point: skipped (counted), a footprint that cannot touch the grid (not counted), or a deposit
enum { POINT_DEPOSIT = 0, POINT_SKIPPED = 1, POINT_FAR = 2 };

// the skip rule, the centre cell and the quantised altitude of bn_dsm_splat for one point; i, j, q only with POINT_DEPOSIT
__device__ __forceinline__ int point_cell(const GridArgs &G, double px, double py, double pz, int &i, int &j, long long &q) {
  if (!(isfinite(px) && isfinite(py) && isfinite(pz)) || !(fabs(pz) < DSM_ZMAX)) return POINT_SKIPPED;
  const double fi = floor((px - G.xoff) / G.resolution);
  const double fj = floor((G.yoff - py) / G.resolution);
  const int rad = G.radius;
  // a footprint that cannot touch the grid (compared in float64: the cell index of a far point need not fit an integer)
  if (!(fi >= (double)(-rad) && fi <= (double)(G.W - 1 + rad) && fj >= (double)(-rad) && fj <= (double)(G.H - 1 + rad))) return POINT_FAR;
  i = (int)fi;
  j = (int)fj;
  q = llrint(pz * DSM_FIX);
  return POINT_DEPOSIT;
}

// f(row * W + col) for every footprint cell of the centre cell (j, i) inside the grid
template <typename F> __device__ __forceinline__ void for_footprint(const GridArgs &G, int i, int j, F f) {
  const int rad = G.radius;
  for (int k2 = -rad; k2 <= rad; ++k2) {
    const int row = j + k2;
    if (row < 0 || row >= G.H) continue;
    for (int k1 = -rad; k1 <= rad; ++k1) {
      const int col = i + k1;
      if (col < 0 || col >= G.W) continue;
      if (G.disc && k1 * k1 + k2 * k2 > rad * rad) continue;
      f((int64_t)row * G.W + col);
    }
  }
}

// the deposit of bn_dsm_splat for one point.  -> true when the point is skipped
__device__ __forceinline__ bool deposit(const GridArgs &G, double px, double py, double pz, unsigned long long *__restrict__ acc) {
  int i, j;
  long long qs;
  const int what = point_cell(G, px, py, pz, i, j, qs);
  if (what != POINT_DEPOSIT) return what == POINT_SKIPPED;
  const unsigned long long q = (unsigned long long)qs;      // two's complement: a negative altitude wraps
  for_footprint(G, i, j, [&](int64_t c) {
    unsigned long long *cell = acc + c * 2;
    atomicAdd(cell, q);
    atomicAdd(cell + 1, 1ull);
  });
  return false;
}

// the mean of a cell from its integer sum in units of 1 / fix: NaN where nothing fell
__device__ __forceinline__ float cell_mean(long long sum, long long count, double fix) {
  return count == 0 ? __builtin_nanf("") : (float)((double)sum / (double)count * (1.0 / fix));
}

// a cell's count as the int32 maps hold it: it saturates
__device__ __forceinline__ int32_t cell_count(long long count) { return count > 0x7fffffffLL ? 0x7fffffff : (int32_t)count; }

inline ToEnz make_to_enz(int32_t cs, int32_t zone, int32_t south) {
  ToEnz t;
  t.ecef = cs == BN_CS_ECEF;
  t.K = make_ecef_k();
  t.utm = make_world(BN_CS_UTM, zone, south);
  return t;
}

inline PointArgs make_point_args(const float *rays, int64_t ray_stride, const float *depth, int64_t R, const double *center, double range) {
  return PointArgs{rays, depth, ray_stride, R, center[0], center[1], center[2], range};
}

inline GridArgs make_grid_args(double xoff, double yoff, double resolution, int32_t W, int32_t H, int32_t radius, int32_t footprint) {
  return GridArgs{xoff, yoff, resolution, W, H, radius, footprint == BN_DSM_DISC};
}

// ------------------------------------------------------------------------------------------------------- what every entry refuses
// `what` is the entry's name, the first word of the refusal's text.  -> 0, or BN_EINVAL with bn_last_error() set
// the rows (a launch of WORLD_BLOCK rows per block holds WORLD_MAX_ROWS = 256 * 0x7fffffff of them), the frame and its coordinate system
inline int require_rays(const char *what, int64_t R, int64_t ray_stride, const double *center, double range, int32_t cs, int32_t zone,
                        int32_t south) {
  BN_REQUIRE(R >= 0 && R <= WORLD_MAX_ROWS && ray_stride >= 6, "%s: R=%lld rows of %lld floats (origin and direction take 6)", what,
             (long long)R, (long long)ray_stride);
  BN_REQUIRE(std::isfinite(range) && std::isfinite(center[0]) && std::isfinite(center[1]) && std::isfinite(center[2]),
             "%s: the frame must be finite", what);
  BN_REQUIRE(cs == BN_CS_ECEF || cs == BN_CS_UTM, "%s: cs=%d (BN_CS_ECEF or BN_CS_UTM)", what, cs);
  BN_REQUIRE(zone >= 1 && zone <= 60, "%s: zone=%d outside [1, 60]", what, zone);
  BN_REQUIRE(south == 0 || south == 1, "%s: south=%d (0 or 1)", what, south);
  return 0;
}

// the grid, radius and footprint refusals of bn_dsm_splat, without the alignment of an accumulator
inline int require_cells(const char *what, double xoff, double yoff, double resolution, int32_t W, int32_t H, int32_t radius,
                         int32_t footprint) {
  BN_REQUIRE(radius >= 0 && radius <= BN_DSM_MAX_RADIUS, "%s: radius=%d outside [0, %d]", what, radius, BN_DSM_MAX_RADIUS);
  BN_REQUIRE(footprint == BN_DSM_DISC || footprint == BN_DSM_SQUARE, "%s: footprint=%d", what, footprint);
  BN_REQUIRE(resolution > 0 && std::isfinite(resolution), "%s: resolution=%g must be positive", what, resolution);
  BN_REQUIRE(std::isfinite(xoff) && std::isfinite(yoff), "%s: the grid origin must be finite", what);
  BN_REQUIRE(W > 0 && H > 0 && (int64_t)W * H <= ((int64_t)1 << 31), "%s: grid %d x %d (W H at most 2^31 cells)", what, W, H);
  return 0;
}

// require_cells and the 16-byte alignment of an accumulator of (sum, count) cells
inline int require_grid(const char *what, const void *acc, double xoff, double yoff, double resolution, int32_t W, int32_t H,
                        int32_t radius, int32_t footprint) {
  BN_REQUIRE(((uintptr_t)acc & 15) == 0, "%s: acc must be 16-byte aligned", what);
  return require_cells(what, xoff, yoff, resolution, W, H, radius, footprint);
}

}  // namespace surface_cell
