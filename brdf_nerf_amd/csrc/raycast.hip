// Depth of a surface model along a view's rays: walk each ray's segment [near, far] over the cells of a height grid and report where
// it first meets a cell's column - on its top, on its wall, or already below it at the start.  include/brdfnerf_hip.h ("Depth of a
// surface model along a ray") states the rule operation by operation.  It has NO upstream counterpart - the reference never
// intersects a ray with a raster - so the rule is this project's own and is checked against its statement (tests/cast_cases.py)
// and against the project's other rules (point_cloud, the DSM splat).
//
// ONE walk (cast_one): float64, every operation rounded on its own; the crossing parameters lam_u, lam_v are always formed from the
// integer line index and the ray's own u0, du - never from a running sum - and are formed again only for the axis that moved, which
// gives the same bits as forming both per cell.  Both height comparisons are <=; a NaN cell is never hit and is counted.
//
// The mapping.  One lane per ray, blocks of 256.  Neighbouring pixels of a view are neighbouring lanes and walk neighbouring cells,
// so a wave's loads of one step fall into a few rows of the raster, which is read through L2 (a 2048 x 2048 grid is 16 MiB and does
// not stay in one XCD's 4 MiB: the walk then runs at the fabric's latency, hidden only by the other waves of the CU).  No LDS
// beyond block_count's word.  The lanes of a wave leave the walk one by one and the wave ends with its last lane.
// Rays whose ends both lie on one side of the grid are a MISS without a walk (the walk visits only cells between the ends); the
// cells outside the grid are walked without a load.  With nan_cells == NULL a cell wholly above zmax is not loaded either.
//
// counts: one integer atomic per class and block (block_sums::block_count).  There is no float atomic.  depth, state, cell and
// nan_cells are plain stores of the lane's own ray: every bit depends on the ray, the frame and the raster alone.
//
// As the compiler reports them for gfx950: cast_rays_kernel<true> (with nan_cells) 56 VGPRs, cast_rays_kernel<false> 54 VGPRs, 4 B of
// LDS each, no scratch, no spill, 8 waves per SIMD.
#include <cmath>
#include "common.h"
#include "block_sums.h"
#include "brdfnerf_hip.h"
// every float64 operation below is rounded on its own (see above); the build also passes -ffp-contract=off for this file
#pragma clang fp contract(off)

namespace {

constexpr int CAST_BLOCK = 256;
constexpr int64_t CAST_MAX_RAYS = (int64_t)1 << 30;
constexpr int64_t CAST_MAX_CELLS = (int64_t)1 << 30;
// the rule's bound is fabs(du) + fabs(dv) + 3 cells; the loop's own bound only keeps a lane from walking on if that reasoning failed
constexpr int CAST_MAX_STEPS = 2 * BN_CAST_MAX_SPAN + 8;

struct Scene {
  const float *dsm;
  int32_t H, W;
  double center[3], range, xoff, yoff, res, zmax;
};

struct Hit {
  int state;
  float depth;
  int32_t cell, nan_cells;
};

template <bool COUNT_NAN>
__device__ __forceinline__ Hit cast_one(const Scene &S, const float *__restrict__ row) {
  Hit out{BN_CAST_NODATA, __builtin_nanf(""), -1, 0};
  const double near = (double)row[6], far = (double)row[7];
  double P0[3], P1[3];
  for (int c = 0; c < 3; ++c) {
    const double o = (double)row[c], d = (double)row[3 + c];
    P0[c] = (o + d * near) * S.range + S.center[c];
    P1[c] = (o + d * far) * S.range + S.center[c];
  }
  const double u0 = (P0[0] - S.xoff) / S.res, v0 = (S.yoff - P0[1]) / S.res, z0 = P0[2];
  const double u1 = (P1[0] - S.xoff) / S.res, v1 = (S.yoff - P1[1]) / S.res, z1 = P1[2];
  const double du = u1 - u0, dv = v1 - v0, dz = z1 - z0;
  if (!(isfinite(u0) && isfinite(v0) && isfinite(z0) && isfinite(u1) && isfinite(v1) && isfinite(z1))) return out;
  if (fabs(du) + fabs(dv) > (double)BN_CAST_MAX_SPAN) return out;
  out.state = BN_CAST_MISS;
  // both ends on one side of the grid: no cell of the walk is inside it
  if (fmax(u0, u1) < 0.0 || fmin(u0, u1) >= (double)S.W || fmax(v0, v1) < 0.0 || fmin(v0, v1) >= (double)S.H) return out;
  // here |u0| <= 2^30 + BN_CAST_MAX_SPAN and likewise v0: the indices fit 32 bits with room for the walk
  int32_t i = (int32_t)floor(u0), j = (int32_t)floor(v0);
  const int32_t si = du > 0.0 ? 1 : -1, sj = dv > 0.0 ? 1 : -1;
  const double inf = __builtin_inf();
  double lam_u = du == 0.0 ? inf : ((double)(du > 0.0 ? i + 1 : i) - u0) / du;
  double lam_v = dv == 0.0 ? inf : ((double)(dv > 0.0 ? j + 1 : j) - v0) / dv;
  double lam_in = 0.0;
  bool first = true;
  for (int step = 0; step < CAST_MAX_STEPS; ++step) {
    const double m = fmin(lam_u, lam_v);
    const double lam_out = fmax(lam_in, fmin(m, 1.0));
    if (i >= 0 && i < S.W && j >= 0 && j < S.H) {
      const double z_in = z0 + lam_in * dz, z_out = z0 + lam_out * dz;
      if (COUNT_NAN || !(fmin(z_in, z_out) > S.zmax)) {
        const int32_t c = j * S.W + i;                  // inside: 0 <= c < H W <= 2^30
        const double h = (double)S.dsm[c];
        double lam = -1.0;
        if (isnan(h)) {
          ++out.nan_cells;
        } else if (z_in <= h) {
          lam = lam_in;
          out.state = first ? BN_CAST_BELOW : BN_CAST_WALL;
        } else if (z_out <= h) {
          lam = fmax(lam_in, fmin((h - z0) / dz, lam_out));
          out.state = BN_CAST_TOP;
        }
        if (lam >= 0.0) {
          out.depth = (float)(near + lam * (far - near));
          out.cell = c;
          return out;
        }
      }
    }
    if (m >= 1.0) return out;
    const bool move_u = lam_u == m, move_v = lam_v == m;
    if (move_u) {
      i += si;
      lam_u = ((double)(du > 0.0 ? i + 1 : i) - u0) / du;      // a move on this axis means du != 0
    }
    if (move_v) {
      j += sj;
      lam_v = ((double)(dv > 0.0 ? j + 1 : j) - v0) / dv;
    }
    if ((i < 0 && du < 0.0) || (i >= S.W && du > 0.0) || (j < 0 && dv < 0.0) || (j >= S.H && dv > 0.0)) return out;
    lam_in = lam_out;
    first = false;
  }
  return out;
}

template <bool COUNT_NAN>
__global__ __launch_bounds__(CAST_BLOCK)
void cast_rays_kernel(const Scene S, const float *__restrict__ rays, int64_t ray_stride, int64_t R, float *__restrict__ depth,
                      uint8_t *__restrict__ state, int32_t *__restrict__ cell, int32_t *__restrict__ nan_cells,
                      unsigned long long *__restrict__ counts) {
  const int64_t r = (int64_t)blockIdx.x * CAST_BLOCK + threadIdx.x;
  int cls = -1;                                  // a lane past the last ray counts nowhere
  if (r < R) {
    const Hit hit = cast_one<COUNT_NAN>(S, rays + r * ray_stride);
    cls = hit.state;
    depth[r] = hit.depth;
    state[r] = (uint8_t)hit.state;
    if (cell) cell[r] = hit.cell;
    if (COUNT_NAN) nan_cells[r] = hit.nan_cells;
  }
  for (int c = 0; c < 5; ++c) block_sums::block_count(cls == c, counts + c);
}

}  // namespace

extern "C" int bn_cast_rays(const float *rays, int64_t ray_stride, int64_t R, const double *center, double range, const float *dsm,
                            int32_t H, int32_t W, double xoff, double yoff, double res, double zmax, float *depth, uint8_t *state,
                            int32_t *cell, int32_t *nan_cells, long long *counts, void *stream) {
  BN_REQUIRE(rays && center && dsm && depth && state && counts, "cast_rays: null argument");
  BN_REQUIRE(R >= 0 && R <= CAST_MAX_RAYS, "cast_rays: R=%lld rays outside [0, 2^30]", (long long)R);
  BN_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= CAST_MAX_CELLS, "cast_rays: grid %d x %d (H W from 1 to 2^30 cells)", H, W);
  BN_REQUIRE(ray_stride >= 8, "cast_rays: ray_stride %lld below 8 (o, d, near, far)", (long long)ray_stride);
  BN_REQUIRE(res > 0.0 && std::isfinite(res), "cast_rays: resolution %g must be positive and finite", res);
  BN_REQUIRE(range > 0.0 && std::isfinite(range), "cast_rays: range %g must be positive and finite", range);
  BN_REQUIRE(std::isfinite(center[0]) && std::isfinite(center[1]) && std::isfinite(center[2]),
             "cast_rays: centre (%g, %g, %g) is not finite", center[0], center[1], center[2]);
  BN_REQUIRE(std::isfinite(xoff) && std::isfinite(yoff), "cast_rays: grid origin (%g, %g) is not finite", xoff, yoff);
  BN_REQUIRE(!std::isnan(zmax), "cast_rays: zmax is NaN");
  if (R == 0) return 0;
  const Scene S{dsm, H, W, {center[0], center[1], center[2]}, range, xoff, yoff, res, zmax};
  const dim3 grid((unsigned)ceil_div64(R, CAST_BLOCK));
  unsigned long long *n = reinterpret_cast<unsigned long long *>(counts);
  if (nan_cells)
    cast_rays_kernel<true><<<grid, CAST_BLOCK, 0, (hipStream_t)stream>>>(S, rays, ray_stride, R, depth, state, cell, nan_cells, n);
  else
    cast_rays_kernel<false><<<grid, CAST_BLOCK, 0, (hipStream_t)stream>>>(S, rays, ray_stride, R, depth, state, cell, nan_cells, n);
  BN_LAUNCH_CHECK("cast_rays");
  return 0;
}
