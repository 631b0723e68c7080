// Digital surface model (DSM) of a rendered view: the rays' depths splatted into a geo-referenced altitude grid, deterministically.
//
// The reference builds the point cloud in numpy on the host (datasets/satellite_rgb_dep.py:601-634, cs == 'utm': a denormalised
// point IS (east, north, altitude), :632-633) and rasterises it with plyflatten(cloud, xoff, yoff, resolution, xsize, ysize,
// radius=1, sigma=inf) (:636-699): the unweighted mean altitude of the points whose footprint covers a cell, NaN where none does
// (:693), row 0 at the northern edge (the affine transform of :695).  Here a lane owns a ray:
//
//   point      p = (o + d depth) range + center in float64, the fp32 inputs widened exactly and EVERY operation rounded on its
//              own (this file is compiled with fp contraction off: fp32 cannot hold a UTM northing of ~3.4e6 m at a 0.5 m cell,
//              and a fused multiply-add would round differently from numpy at cell boundaries)
//   cell       i = floor((p.x - xoff) / resolution), j = floor((yoff - p.y) / resolution), both in float64
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
#include <cmath>
#include "common.h"
#include "brdfnerf_hip.h"
// every float64 operation below is rounded on its own (see above); the build also passes -ffp-contract=off for this file
#pragma clang fp contract(off)

namespace {

struct DsmArgs {
  const float *rays, *depth;
  int64_t ray_stride, R;
  double cx, cy, cz, range, xoff, yoff, resolution;
  int32_t W, H, radius, disc;
};

constexpr double DSM_FIX = 1048576.0;          // 2^20: altitudes are summed in units of 2^-20 m
constexpr double DSM_ZMAX = 8388608.0;         // 2^23 m

__global__ __launch_bounds__(256)
void dsm_splat_kernel(const DsmArgs A, unsigned long long *__restrict__ acc, unsigned long long *__restrict__ skipped) {
  const int64_t ray = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (ray >= A.R) return;
  const float *r = A.rays + ray * A.ray_stride;
  const double t = (double)A.depth[ray];
  const double px = ((double)r[0] + (double)r[3] * t) * A.range + A.cx;
  const double py = ((double)r[1] + (double)r[4] * t) * A.range + A.cy;
  const double pz = ((double)r[2] + (double)r[5] * t) * A.range + A.cz;
  if (!(isfinite(px) && isfinite(py) && isfinite(pz)) || !(fabs(pz) < DSM_ZMAX)) {
    atomicAdd(skipped, 1ull);
    return;
  }
  const double fi = floor((px - A.xoff) / A.resolution);
  const double fj = floor((A.yoff - py) / A.resolution);
  const int rad = A.radius;
  // a footprint that cannot touch the grid (compared in float64: the cell index of a far point need not fit an integer)
  if (!(fi >= (double)(-rad) && fi <= (double)(A.W - 1 + rad) && fj >= (double)(-rad) && fj <= (double)(A.H - 1 + rad))) return;
  const int i = (int)fi, j = (int)fj;
  const unsigned long long q = (unsigned long long)llrint(pz * DSM_FIX);      // two's complement: a negative altitude wraps
  for (int k2 = -rad; k2 <= rad; ++k2) {
    const int row = j + k2;
    if (row < 0 || row >= A.H) continue;
    for (int k1 = -rad; k1 <= rad; ++k1) {
      const int col = i + k1;
      if (col < 0 || col >= A.W) continue;
      if (A.disc && k1 * k1 + k2 * k2 > rad * rad) continue;
      unsigned long long *cell = acc + ((int64_t)row * A.W + col) * 2;
      atomicAdd(cell, q);
      atomicAdd(cell + 1, 1ull);
    }
  }
}

__global__ __launch_bounds__(256)
void dsm_resolve_kernel(const long long *__restrict__ acc, int64_t n, float *__restrict__ dsm, int32_t *__restrict__ count) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  const longlong2 sc = reinterpret_cast<const longlong2 *>(acc)[c];          // (sum, count): one 16-byte load
  dsm[c] = sc.y == 0 ? __builtin_nanf("") : (float)((double)sc.x / (double)sc.y * (1.0 / DSM_FIX));
  if (count) count[c] = sc.y > 0x7fffffffLL ? 0x7fffffff : (int32_t)sc.y;
}

}  // namespace

extern "C" int bn_dsm_splat(const float *rays, int64_t ray_stride, const float *depth, int64_t R, const double *center, double range,
                            double xoff, double yoff, double resolution, int32_t W, int32_t H, int32_t radius, int32_t footprint,
                            long long *acc, unsigned long long *skipped, void *stream) {
  BN_REQUIRE(rays && depth && center && acc && skipped, "dsm_splat: null argument");
  BN_REQUIRE(((uintptr_t)acc & 15) == 0, "dsm_splat: acc must be 16-byte aligned");
  BN_REQUIRE(R >= 0 && ray_stride >= 6, "dsm_splat: R=%lld rows of %lld floats (origin and direction take 6)", (long long)R, (long long)ray_stride);
  BN_REQUIRE(radius >= 0 && radius <= BN_DSM_MAX_RADIUS, "dsm_splat: radius=%d outside [0, %d]", radius, BN_DSM_MAX_RADIUS);
  BN_REQUIRE(footprint == BN_DSM_DISC || footprint == BN_DSM_SQUARE, "dsm_splat: footprint=%d", footprint);
  BN_REQUIRE(resolution > 0 && std::isfinite(resolution), "dsm_splat: resolution=%g must be positive", resolution);
  BN_REQUIRE(std::isfinite(xoff) && std::isfinite(yoff) && std::isfinite(range) && std::isfinite(center[0]) && std::isfinite(center[1]) && std::isfinite(center[2]),
             "dsm_splat: the frame and the grid origin must be finite");
  BN_REQUIRE(W > 0 && H > 0 && (int64_t)W * H <= ((int64_t)1 << 31), "dsm_splat: grid %d x %d (W H at most 2^31 cells)", W, H);
  BN_REQUIRE(R <= (int64_t)256 * 0x7fffffff, "dsm_splat: R=%lld too large", (long long)R);
  if (R == 0) return 0;
  DsmArgs a;
  a.rays = rays; a.depth = depth; a.ray_stride = ray_stride; a.R = R;
  a.cx = center[0]; a.cy = center[1]; a.cz = center[2]; a.range = range; a.xoff = xoff; a.yoff = yoff; a.resolution = resolution;
  a.W = W; a.H = H; a.radius = radius; a.disc = footprint == BN_DSM_DISC;
  dsm_splat_kernel<<<(unsigned)ceil_div64(R, 256), 256, 0, (hipStream_t)stream>>>(a, reinterpret_cast<unsigned long long *>(acc), skipped);
  BN_LAUNCH_CHECK("dsm_splat");
  return 0;
}

extern "C" int bn_dsm_resolve(const long long *acc, int32_t W, int32_t H, float *dsm, int32_t *count, void *stream) {
  BN_REQUIRE(acc && dsm, "dsm_resolve: null argument");
  BN_REQUIRE(((uintptr_t)acc & 15) == 0, "dsm_resolve: acc must be 16-byte aligned");
  BN_REQUIRE(W > 0 && H > 0 && (int64_t)W * H <= ((int64_t)1 << 31), "dsm_resolve: grid %d x %d (W H at most 2^31 cells)", W, H);
  const int64_t n = (int64_t)W * H;
  dsm_resolve_kernel<<<(unsigned)ceil_div64(n, 256), 256, 0, (hipStream_t)stream>>>(acc, n, dsm, count);
  BN_LAUNCH_CHECK("dsm_resolve");
  return 0;
}
