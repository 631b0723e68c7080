// The rays of a satellite view from its RPC camera model: localisation of every pixel at two altitudes, geodetic -> world, and the
// normalised ray row, one lane per ray.
//
// The reference does this on the host per image (datasets/satellite_rgb_dep.py:23-78 get_rays, :550-559 normalize_rays) through
// rpcm's localisation and pyproj's UTM projection; this project depends on neither.  include/brdfnerf_hip.h states every step
// operation by operation ("The rays of a satellite view"); the order of the operations below IS that statement, and the file is
// compiled with fp contraction off so that each one rounds on its own:
//
//   monomials    20 products of (L, P, H), each formed left to right, shared by the four polynomials of a Newton step
//   localise     Newton on (L, P) from (0, 0), analytic Jacobian, Cramer's rule, BN_RPC_NEWTON_ITERS iterations for every lane:
//                no data-dependent exit, so lanes do not diverge and the bits are a pure function of the pixel.  Only + - x /
//                occur: float64 division on the device is correctly rounded, the result is numpy's bit for bit.
//   world        ECEF as sat_utils.latlon_to_ecef_custom writes it, or the Krueger series to n^6 (Karney 2011) for UTM.  The
//                device's float64 sin / cos / atanh / sinh / cosh / atan2 are not bit-specified: held to 1e-6 m, not to bits.
//   ray          near (max_alt) and far (min_alt) in ONE lane, one after the other: the two Newton chains share nothing but the
//                pixel, and a lane that owns both needs no exchange to form far - near.  The other form - a lane pair per ray,
//                the far point handed over by a lane swap - gave the same bits at 95 VGPRs and 5 waves per SIMD, and took 1.22
//                against 1.19 ms (UTM) and 1.02 against 0.98 ms (ECEF) on a 2048 x 2048 view: not kept.
//
// The 80 coefficients are uniform across lanes: the descriptor travels in the kernel arguments, which a wave reads through the
// scalar cache once (s_load), not per lane.  The four polynomials of a step are evaluated one after another over the shared
// monomials (value and both derivatives of one coefficient set in one pass) in a loop that is NOT unrolled: 80 doubles are 160
// scalar registers, more than a wave has, and with all four sets in flight the compiler parked them in lanes of vector
// registers (142 VGPRs, 3 waves per SIMD); one set at a time the ray kernel takes 101 VGPRs, no scratch, 4 waves per SIMD.
// A counted row (zero determinant, non-finite result) is summed per block and added with ONE integer atomic; there
// is no float atomic in this file.
//
// The tie-point depth priors ("The depth priors of a view" in the header; load_depth_data, datasets/satellite_rgb_dep.py:401-548)
// run the same ray chain (ray_chain below: ONE statement, called by both kernels) for the tie points of a view, one lane per tie
// point: a view has far fewer tie points than pixels, so a lane per output pixel would leave most lanes idle.  Ownership of a
// pixel is an integer atomicMax of the tie index in a launch of its own; the second launch works for the owners only and
// scatters through inverse index vectors of the resize made on the host.  tie_priors_kernel: 109 VGPRs, no scratch, 4 waves per
// SIMD (the eight ray values stay live across the point arithmetic); rpc_rays_kernel keeps its 101.
#include <cmath>
#include "common.h"
#include "brdfnerf_hip.h"
#include "block_sums.h"
#include "geodesy.h"
#include "rpc_poly.h"
// every float64 operation below is rounded on its own (see above); the build also passes -ffp-contract=off for this file
#pragma clang fp contract(off)

namespace {

// UtmK, World, geo_world and make_world: geodesy.h, shared with world.hip
using namespace geodesy;
// Mono, monomials, poly, project and rpc_ok: rpc_poly.h, shared with orthophoto.hip
using namespace rpc_poly;

constexpr int CAM_BLOCK = 256;

// value and d / dL, d / dP of one polynomial (the derivative table of the header)
__device__ __forceinline__ void poly_d(const double *c, const Mono &m, double &v, double &dL, double &dP) {
  v = poly(c, m);
  double s = c[1];
  s = s + c[4] * m.P; s = s + c[5] * m.H; s = s + c[7] * (2.0 * m.L); s = s + c[10] * m.m6; s = s + c[11] * (3.0 * m.m7);
  s = s + c[12] * m.m8; s = s + c[13] * m.m9; s = s + c[14] * (2.0 * m.m4); s = s + c[17] * (2.0 * m.m5);
  dL = s;
  s = c[2];
  s = s + c[4] * m.L; s = s + c[6] * m.H; s = s + c[8] * (2.0 * m.P); s = s + c[10] * m.m5; s = s + c[12] * (2.0 * m.m4);
  s = s + c[14] * m.m7; s = s + c[15] * (3.0 * m.m8); s = s + c[16] * m.m9; s = s + c[18] * (2.0 * m.m6);
  dP = s;
}

// step 3 of the header: -> true when the pixel is counted (lon = lat = NaN then)
__device__ __forceinline__ bool localize(const bn_rpc &R, double col, double row, double alt, double &lon, double &lat) {
  const double cn = (col - R.col_offset) / R.col_scale, rn = (row - R.row_offset) / R.row_scale;
  const double H = (alt - R.alt_offset) / R.alt_scale;
  double L = 0.0, P = 0.0;
  bool bad = false;
#pragma unroll 1
  for (int it = 0; it < BN_RPC_NEWTON_ITERS; ++it) {
    const Mono m = monomials(L, P, H);
    // row_num, row_den, col_num, col_den lie one after another: polynomial p reads its 20 coefficients at a scalar offset, so
    // a wave holds one set at a time (all 80 at once do not fit the scalar registers)
    double N = 0.0, NL = 0.0, NP = 0.0, fc = 0.0, a = 0.0, b = 0.0, fr = 0.0, c = 0.0, d = 0.0;
#pragma unroll 1
    for (int p = 0; p < 4; ++p) {
      double v, vL, vP;
      poly_d(R.row_num + 20 * p, m, v, vL, vP);
      if ((p & 1) == 0) {
        N = v; NL = vL; NP = vP;
      } else {                                       // v is the denominator D of the numerator held
        const double f = N / v - (p == 1 ? rn : cn);
        const double jL = (NL * v - N * vL) / (v * v), jP = (NP * v - N * vP) / (v * v);
        if (p == 1) {
          fr = f; c = jL; d = jP;
        } else {
          fc = f; a = jL; b = jP;
        }
      }
    }
    const double det = a * d - b * c;
    bad = bad || det == 0.0;
    L = L - (fc * d - b * fr) / det;
    P = P - (a * fr - fc * c) / det;
  }
  lon = L * R.lon_scale + R.lon_offset;
  lat = P * R.lat_scale + R.lat_offset;
  bad = bad || !isfinite(lon) || !isfinite(lat);
  if (bad) lon = lat = __builtin_nan("");
  return bad;
}

// the pixel of ray r: grid mode (cols == NULL) or the arrays
__device__ __forceinline__ void pixel_of(const double *cols, const double *rows, int32_t W, int64_t r, double &col, double &row) {
  if (cols) {
    col = cols[r];
    row = rows[r];
  } else {
    col = (double)(r % W);
    row = (double)(r / W);
  }
}

__global__ __launch_bounds__(CAM_BLOCK)
void rpc_project_kernel(const bn_rpc R, const double *__restrict__ lon, const double *__restrict__ lat,
                        const double *__restrict__ alt, int64_t n, double *__restrict__ col, double *__restrict__ row) {
  const int64_t i = (int64_t)blockIdx.x * CAM_BLOCK + threadIdx.x;
  if (i >= n) return;
  double c, r;
  project(R, lon[i], lat[i], alt[i], c, r);
  col[i] = c;
  row[i] = r;
}

__global__ __launch_bounds__(CAM_BLOCK)
void rpc_localize_kernel(const bn_rpc R, const double *__restrict__ cols, const double *__restrict__ rows, int32_t W, int64_t r0,
                         int64_t r1, double alt, double *__restrict__ lonlat, unsigned long long *__restrict__ counts) {
  const int64_t k = (int64_t)blockIdx.x * CAM_BLOCK + threadIdx.x, r = r0 + k;
  bool bad = false;
  if (r < r1) {
    double col, row, lon, lat;
    pixel_of(cols, rows, W, r, col, row);
    bad = localize(R, col, row, alt, lon, lat);
    lonlat[2 * k] = lon;
    lonlat[2 * k + 1] = lat;
  }
  block_sums::block_count(bad, counts);
}

__global__ __launch_bounds__(CAM_BLOCK)
void geo_world_kernel(const World Wd, const double *__restrict__ lonlat, const double *__restrict__ alt, int64_t n,
                      double *__restrict__ xyz) {
  const int64_t i = (int64_t)blockIdx.x * CAM_BLOCK + threadIdx.x;
  if (i >= n) return;
  double x, y, z;
  geo_world(Wd, lonlat[2 * i], lonlat[2 * i + 1], alt[i], x, y, z);
  xyz[3 * i] = x;
  xyz[3 * i + 1] = y;
  xyz[3 * i + 2] = z;
}

// the scene's normalisation and the altitude bounds of a view: what the ray chain reads besides the pixel
struct Frame {
  int32_t round_f32;
  double min_alt, max_alt, cx, cy, cz, range;
};

// step 5 of the header for one pixel: the eight values of the ray row into v (as computed, NOT yet NaN where counted) and the
// geodetic near / far points.  -> true when the ray is counted.  The one statement of the chain: rpc_rays_kernel and
// tie_priors_kernel both call it.
__device__ __forceinline__ bool ray_chain(const bn_rpc &R, const World &Wd, const Frame &F, double col, double row, float (&v)[8],
                                          double &lon_n, double &lat_n, double &lon_f, double &lat_f) {
  bool bad = localize(R, col, row, F.max_alt, lon_n, lat_n);
  bad = localize(R, col, row, F.min_alt, lon_f, lat_f) || bad;
  double nx, ny, nz, fx, fy, fz;
  geo_world(Wd, lon_n, lat_n, F.max_alt, nx, ny, nz);
  geo_world(Wd, lon_f, lat_f, F.min_alt, fx, fy, fz);
  const double dx = fx - nx, dy = fy - ny, dz = fz - nz;
  const double len = sqrt((dx * dx + dy * dy) + dz * dz);
  v[3] = (float)(dx / len);
  v[4] = (float)(dy / len);
  v[5] = (float)(dz / len);
  v[6] = 0.f;
  if (F.round_f32) {
    const float rg = (float)F.range;
    v[0] = ((float)nx - (float)F.cx) / rg;
    v[1] = ((float)ny - (float)F.cy) / rg;
    v[2] = ((float)nz - (float)F.cz) / rg;
    v[7] = (float)len / rg;
  } else {
    v[0] = (float)((nx - F.cx) / F.range);
    v[1] = (float)((ny - F.cy) / F.range);
    v[2] = (float)((nz - F.cz) / F.range);
    v[7] = (float)(len / F.range);
  }
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 8; ++i) finite = finite && isfinite(v[i]);
  return bad || !finite;
}

struct RayArgs {
  const double *cols, *rows;
  int32_t W, has_sun;
  int64_t r0, r1, ray_stride;
  Frame F;
  float sun[3];
  float *rays;
  double *lonlat_near, *lonlat_far;
  unsigned long long *counts;
};

__global__ __launch_bounds__(CAM_BLOCK)
void rpc_rays_kernel(const bn_rpc R, const World Wd, const RayArgs A) {
  const int64_t k = (int64_t)blockIdx.x * CAM_BLOCK + threadIdx.x, r = A.r0 + k;
  bool bad = false;
  if (r < A.r1) {
    double col, row, lon_n, lat_n, lon_f, lat_f;
    pixel_of(A.cols, A.rows, A.W, r, col, row);
    float v[8];
    bad = ray_chain(R, Wd, A.F, col, row, v, lon_n, lat_n, lon_f, lat_f);
    if (A.lonlat_near) {
      A.lonlat_near[2 * k] = lon_n;
      A.lonlat_near[2 * k + 1] = lat_n;
    }
    if (A.lonlat_far) {
      A.lonlat_far[2 * k] = lon_f;
      A.lonlat_far[2 * k + 1] = lat_f;
    }
    float *out = A.rays + k * A.ray_stride;
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = bad ? __builtin_nanf("") : v[i];
    if (A.has_sun) {
      out[8] = A.sun[0];
      out[9] = A.sun[1];
      out[10] = A.sun[2];
    }
  }
  block_sums::block_count(bad, A.counts);
}

// The tie-point depth priors of a view ("The depth priors of a view" in the header).  Two launches, one lane per tie point:
// tie_owner_kernel settles which tie owns a pixel with an integer atomicMax, tie_priors_kernel runs the ray chain and the
// prior arithmetic for the owners only and scatters them; distinct pixels have distinct destinations, so no write races.
__global__ __launch_bounds__(CAM_BLOCK)
void tie_owner_kernel(const int32_t *__restrict__ px, int32_t T, int32_t H, int32_t W, int32_t *__restrict__ owner,
                      unsigned long long *__restrict__ counts) {
  const int64_t t = (int64_t)blockIdx.x * CAM_BLOCK + threadIdx.x;
  bool outside = false, dup = false;
  if (t < T) {
    const int32_t col = px[2 * t], row = px[2 * t + 1];
    outside = col < 0 || col >= W || row < 0 || row >= H;
    if (!outside) dup = atomicMax(&owner[(int64_t)row * W + col], (int32_t)t) != -1;
  }
  block_sums::block_count(outside, counts);
  block_sums::block_count(dup, counts + 1);
}

struct TieArgs {
  const int32_t *px, *owner, *dst_row, *dst_col;
  const double *pts3d, *correl;
  int32_t T, H, W, Hout, Wout;
  double downscale, cmin, cmax, corrscale;
  float stdscale, margin, std_span;
  Frame F;
  float *valid, *depths, *depth_std, *rays, *points, *valid_full, *tie_rays;
  unsigned long long *counts;
};

__global__ __launch_bounds__(CAM_BLOCK)
void tie_priors_kernel(const bn_rpc R, const World Wd, const TieArgs A) {
  const int64_t t = (int64_t)blockIdx.x * CAM_BLOCK + threadIdx.x;
  bool skipped = false, unsampled = false;
  if (t < A.T) {
    const int32_t col = A.px[2 * t], row = A.px[2 * t + 1];
    const bool inside = col >= 0 && col < A.W && row >= 0 && row < A.H;
    const int64_t pix = (int64_t)row * A.W + col;
    if (inside && A.owner[pix] == (int32_t)t) {
      float v[8];
      double lon_n, lat_n, lon_f, lat_f;
      skipped = ray_chain(R, Wd, A.F, (double)col / A.downscale, (double)row / A.downscale, v, lon_n, lat_n, lon_f, lat_f);
      if (A.tie_rays) {
#pragma unroll
        for (int i = 0; i < 8; ++i) A.tie_rays[8 * t + i] = skipped ? __builtin_nanf("") : v[i];
      }
      const double X = A.pts3d[3 * t], Y = A.pts3d[3 * t + 1], Z = A.pts3d[3 * t + 2];
      float p[3];
      if (A.F.round_f32) {
        const float rg = (float)A.F.range;
        p[0] = ((float)X - (float)A.F.cx) / rg;
        p[1] = ((float)Y - (float)A.F.cy) / rg;
        p[2] = ((float)Z - (float)A.F.cz) / rg;
      } else {
        p[0] = (float)((X - A.F.cx) / A.F.range);
        p[1] = (float)((Y - A.F.cy) / A.F.range);
        p[2] = (float)((Z - A.F.cz) / A.F.range);
      }
      const float tx = p[0] - v[0], ty = p[1] - v[1], tz = p[2] - v[2];
      const float depth = sqrtf((tx * tx + ty * ty) + tz * tz);
      const double cn = ((A.correl[t] - A.cmin) / (A.cmax - A.cmin)) * A.corrscale;
      const float w = (float)cn * (-v[5]);
      const float s = A.stdscale * (1.0f - w) + A.margin;
      skipped = skipped || !(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) && isfinite(depth) && isfinite(w) && isfinite(s));
      if (!skipped) {
        if (A.points) {
          A.points[3 * pix] = p[0];
          A.points[3 * pix + 1] = p[1];
          A.points[3 * pix + 2] = p[2];
        }
        if (A.valid_full) A.valid_full[pix] = 1.f;
        const int32_t dr = A.dst_row ? A.dst_row[row] : row, dc = A.dst_col ? A.dst_col[col] : col;
        unsampled = dr < 0 || dr >= A.Hout || dc < 0 || dc >= A.Wout;
        if (!unsampled) {
          const int64_t q = (int64_t)dr * A.Wout + dc;
          A.valid[q] = 1.f;
          if (A.depths) {
            A.depths[2 * q] = depth;
            A.depths[2 * q + 1] = w;
          }
          if (A.depth_std) A.depth_std[q] = s * A.std_span;
          if (A.rays) {
#pragma unroll
            for (int i = 0; i < 8; ++i) A.rays[8 * q + i] = v[i];
          }
        }
      }
    }
  }
  block_sums::block_count(skipped, A.counts + 2);
  block_sums::block_count(unsampled, A.counts + 3);
}

// ---------------------------------------------------------------------------------------------------------------- host side
constexpr int64_t CAM_MAX_RAYS = (int64_t)1 << 30;

}  // namespace

#define CAM_REQUIRE_WORLD(what)                                                                                        \
  BN_REQUIRE(cs == BN_CS_ECEF || cs == BN_CS_UTM, what ": cs=%d (BN_CS_ECEF or BN_CS_UTM)", cs);                       \
  BN_REQUIRE(zone >= 1 && zone <= 60, what ": zone=%d outside [1, 60]", zone);                                         \
  BN_REQUIRE(south == 0 || south == 1, what ": south=%d (0 or 1)", south)

#define CAM_REQUIRE_PIXELS(what)                                                                                       \
  BN_REQUIRE((cols == nullptr) == (rows == nullptr), what ": cols and rows come together");                            \
  BN_REQUIRE(r0 >= 0 && r0 <= r1 && r1 - r0 <= CAM_MAX_RAYS, what ": rays [%lld, %lld) (r0 <= r1, at most 2^30)",      \
             (long long)r0, (long long)r1);                                                                            \
  BN_REQUIRE(cols != nullptr || W >= 1, what ": W=%d in grid mode", W)

extern "C" int bn_rpc_project(const bn_rpc *rpc, const double *lon, const double *lat, const double *alt, int64_t n, double *col,
                              double *row, void *stream) {
  BN_REQUIRE(rpc && lon && lat && alt && col && row, "rpc_project: null argument");
  BN_REQUIRE(n >= 0 && n <= CAM_MAX_RAYS, "rpc_project: n=%lld (0 to 2^30)", (long long)n);
  BN_REQUIRE(rpc_ok(rpc), "rpc_project: the descriptor has a zero scale or a non-finite entry");
  if (n == 0) return 0;
  rpc_project_kernel<<<(unsigned)ceil_div64(n, CAM_BLOCK), CAM_BLOCK, 0, (hipStream_t)stream>>>(*rpc, lon, lat, alt, n, col, row);
  BN_LAUNCH_CHECK("rpc_project");
  return 0;
}

extern "C" int bn_rpc_localize(const bn_rpc *rpc, const double *cols, const double *rows, int32_t W, int64_t r0, int64_t r1,
                               double alt, double *lonlat, unsigned long long *counts, void *stream) {
  BN_REQUIRE(rpc && lonlat && counts, "rpc_localize: null argument");
  CAM_REQUIRE_PIXELS("rpc_localize");
  BN_REQUIRE(std::isfinite(alt), "rpc_localize: alt=%g must be finite", alt);
  BN_REQUIRE(rpc_ok(rpc), "rpc_localize: the descriptor has a zero scale or a non-finite entry");
  if (r1 == r0) return 0;
  rpc_localize_kernel<<<(unsigned)ceil_div64(r1 - r0, CAM_BLOCK), CAM_BLOCK, 0, (hipStream_t)stream>>>(*rpc, cols, rows, W, r0, r1, alt,
                                                                                                   lonlat, counts);
  BN_LAUNCH_CHECK("rpc_localize");
  return 0;
}

extern "C" int bn_geo_world(const double *lonlat, const double *alt, int64_t n, int32_t cs, int32_t zone, int32_t south, double *xyz,
                            void *stream) {
  BN_REQUIRE(lonlat && alt && xyz, "geo_world: null argument");
  BN_REQUIRE(n >= 0 && n <= CAM_MAX_RAYS, "geo_world: n=%lld (0 to 2^30)", (long long)n);
  CAM_REQUIRE_WORLD("geo_world");
  if (n == 0) return 0;
  geo_world_kernel<<<(unsigned)ceil_div64(n, CAM_BLOCK), CAM_BLOCK, 0, (hipStream_t)stream>>>(make_world(cs, zone, south), lonlat, alt, n,
                                                                                          xyz);
  BN_LAUNCH_CHECK("geo_world");
  return 0;
}

extern "C" int bn_rpc_rays(const bn_rpc *rpc, const double *cols, const double *rows, int32_t W, int64_t r0, int64_t r1,
                           double min_alt, double max_alt, int32_t cs, int32_t zone, int32_t south, const double *center,
                           double range, const float *sun, int32_t round_f32, float *rays, int64_t ray_stride, double *lonlat_near,
                           double *lonlat_far, unsigned long long *counts, void *stream) {
  BN_REQUIRE(rpc && center && rays && counts, "rpc_rays: null argument");
  CAM_REQUIRE_PIXELS("rpc_rays");
  CAM_REQUIRE_WORLD("rpc_rays");
  BN_REQUIRE(round_f32 == 0 || round_f32 == 1, "rpc_rays: round_f32=%d (0 or 1)", round_f32);
  BN_REQUIRE(std::isfinite(min_alt) && std::isfinite(max_alt), "rpc_rays: altitudes [%g, %g] must be finite", min_alt, max_alt);
  BN_REQUIRE(range > 0 && std::isfinite(range), "rpc_rays: range=%g must be positive and finite", range);
  BN_REQUIRE(std::isfinite(center[0]) && std::isfinite(center[1]) && std::isfinite(center[2]), "rpc_rays: the centre must be finite");
  BN_REQUIRE(ray_stride >= (sun ? 11 : 8), "rpc_rays: ray_stride=%lld below the %d columns written", (long long)ray_stride, sun ? 11 : 8);
  BN_REQUIRE(rpc_ok(rpc), "rpc_rays: the descriptor has a zero scale or a non-finite entry");
  if (r1 == r0) return 0;
  RayArgs a;
  a.cols = cols; a.rows = rows; a.W = W; a.has_sun = sun != nullptr;
  a.r0 = r0; a.r1 = r1; a.ray_stride = ray_stride;
  a.F = Frame{round_f32, min_alt, max_alt, center[0], center[1], center[2], range};
  for (int i = 0; i < 3; ++i) a.sun[i] = sun ? sun[i] : 0.f;
  a.rays = rays; a.lonlat_near = lonlat_near; a.lonlat_far = lonlat_far; a.counts = counts;
  rpc_rays_kernel<<<(unsigned)ceil_div64(r1 - r0, CAM_BLOCK), CAM_BLOCK, 0, (hipStream_t)stream>>>(*rpc, make_world(cs, zone, south), a);
  BN_LAUNCH_CHECK("rpc_rays");
  return 0;
}

extern "C" int bn_tie_owner(const int32_t *px, int32_t T, int32_t H, int32_t W, int32_t *owner, unsigned long long *counts,
                            void *stream) {
  BN_REQUIRE(px && owner && counts, "tie_owner: null argument");
  BN_REQUIRE(T >= 0 && T <= CAM_MAX_RAYS, "tie_owner: T=%d tie points (0 to 2^30)", T);
  BN_REQUIRE(H >= 1 && W >= 1, "tie_owner: a view of %d x %d pixels", H, W);
  BN_REQUIRE((int64_t)H * W <= (int64_t)1 << 31, "tie_owner: %d x %d pixels (H W at most 2^31)", H, W);
  if (T == 0) return 0;
  tie_owner_kernel<<<(unsigned)ceil_div64(T, CAM_BLOCK), CAM_BLOCK, 0, (hipStream_t)stream>>>(px, T, H, W, owner, counts);
  BN_LAUNCH_CHECK("tie_owner");
  return 0;
}

extern "C" int bn_tie_priors(const bn_rpc *rpc, const int32_t *px, const int32_t *owner, const double *pts3d, const double *correl,
                             int32_t T, int32_t H, int32_t W, int32_t Hout, int32_t Wout, const int32_t *dst_row,
                             const int32_t *dst_col, double downscale, double min_alt, double max_alt, int32_t cs, int32_t zone,
                             int32_t south, const double *center, double range, int32_t round_f32, double cmin, double cmax,
                             double corrscale, double stdscale, double margin, double std_span, float *valid, float *depths,
                             float *depth_std, float *rays, float *points, float *valid_full, float *tie_rays,
                             unsigned long long *counts, void *stream) {
  BN_REQUIRE(rpc && px && owner && pts3d && correl && center && valid && counts, "tie_priors: null argument");
  BN_REQUIRE(T >= 0 && T <= CAM_MAX_RAYS, "tie_priors: T=%d tie points (0 to 2^30)", T);
  BN_REQUIRE(H >= 1 && W >= 1 && Hout >= 1 && Wout >= 1, "tie_priors: a view of %d x %d pixels, an output of %d x %d", H, W, Hout, Wout);
  BN_REQUIRE((int64_t)H * W <= (int64_t)1 << 31, "tie_priors: %d x %d pixels (H W at most 2^31)", H, W);
  BN_REQUIRE((dst_row || Hout == H) && (dst_col || Wout == W),
             "tie_priors: without dst_row / dst_col the output is the view (%d x %d, not %d x %d)", H, W, Hout, Wout);
  CAM_REQUIRE_WORLD("tie_priors");
  BN_REQUIRE(round_f32 == 0 || round_f32 == 1, "tie_priors: round_f32=%d (0 or 1)", round_f32);
  BN_REQUIRE(std::isfinite(downscale) && downscale >= 1.0, "tie_priors: downscale=%g must be finite and at least 1", downscale);
  BN_REQUIRE(std::isfinite(min_alt) && std::isfinite(max_alt), "tie_priors: altitudes [%g, %g] must be finite", min_alt, max_alt);
  BN_REQUIRE(range > 0 && std::isfinite(range), "tie_priors: range=%g must be positive and finite", range);
  BN_REQUIRE(std::isfinite(center[0]) && std::isfinite(center[1]) && std::isfinite(center[2]), "tie_priors: the centre must be finite");
  BN_REQUIRE(std::isfinite(cmin) && std::isfinite(cmax) && cmax > cmin, "tie_priors: correlations [%g, %g] (finite, cmax > cmin)", cmin,
             cmax);
  BN_REQUIRE(std::isfinite(corrscale) && std::isfinite(stdscale) && std::isfinite(margin) && std::isfinite(std_span),
             "tie_priors: corrscale=%g, stdscale=%g, margin=%g, std_span=%g must be finite", corrscale, stdscale, margin, std_span);
  BN_REQUIRE(rpc_ok(rpc), "tie_priors: the descriptor has a zero scale or a non-finite entry");
  if (T == 0) return 0;
  TieArgs a;
  a.px = px; a.owner = owner; a.dst_row = dst_row; a.dst_col = dst_col; a.pts3d = pts3d; a.correl = correl;
  a.T = T; a.H = H; a.W = W; a.Hout = Hout; a.Wout = Wout;
  a.downscale = downscale; a.cmin = cmin; a.cmax = cmax; a.corrscale = corrscale;
  a.stdscale = (float)stdscale; a.margin = (float)margin; a.std_span = (float)std_span;
  a.F = Frame{round_f32, min_alt, max_alt, center[0], center[1], center[2], range};
  a.valid = valid; a.depths = depths; a.depth_std = depth_std; a.rays = rays; a.points = points; a.valid_full = valid_full;
  a.tie_rays = tie_rays; a.counts = counts;
  tie_priors_kernel<<<(unsigned)ceil_div64(T, CAM_BLOCK), CAM_BLOCK, 0, (hipStream_t)stream>>>(*rpc, make_world(cs, zone, south), a);
  BN_LAUNCH_CHECK("tie_priors");
  return 0;
}
