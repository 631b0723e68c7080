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
#include <cmath>
#include "common.h"
#include "brdfnerf_hip.h"
// every float64 operation below is rounded on its own (see above); the build also passes -ffp-contract=off for this file
#pragma clang fp contract(off)

namespace {

constexpr int CAM_BLOCK = 256;
constexpr double CAM_D2R = 3.14159265358979323846 / 180.0;        // np.pi / 180.0
constexpr double WGS84_A = 6378137.0, WGS84_FINV = 298.257223563;

struct Mono {
  double L, P, H, m4, m5, m6, m7, m8, m9, m10, m11, m12, m13, m14, m15, m16, m17, m18, m19;
};

__device__ __forceinline__ Mono monomials(double L, double P, double H) {
  Mono m;
  m.L = L; m.P = P; m.H = H;
  m.m4 = L * P; m.m5 = L * H; m.m6 = P * H; m.m7 = L * L; m.m8 = P * P; m.m9 = H * H;
  m.m10 = (P * L) * H; m.m11 = m.m7 * L; m.m12 = m.m4 * P; m.m13 = m.m5 * H; m.m14 = m.m7 * P; m.m15 = m.m8 * P;
  m.m16 = m.m6 * H; m.m17 = m.m7 * H; m.m18 = m.m8 * H; m.m19 = m.m9 * H;
  return m;
}

__device__ __forceinline__ double poly(const double *c, const Mono &m) {
  double s = c[0];
  s = s + c[1] * m.L; s = s + c[2] * m.P; s = s + c[3] * m.H; s = s + c[4] * m.m4; s = s + c[5] * m.m5; s = s + c[6] * m.m6;
  s = s + c[7] * m.m7; s = s + c[8] * m.m8; s = s + c[9] * m.m9; s = s + c[10] * m.m10; s = s + c[11] * m.m11;
  s = s + c[12] * m.m12; s = s + c[13] * m.m13; s = s + c[14] * m.m14; s = s + c[15] * m.m15; s = s + c[16] * m.m16;
  s = s + c[17] * m.m17; s = s + c[18] * m.m18; s = s + c[19] * m.m19;
  return s;
}

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

// the constants of the UTM series, formed once on the host
struct UtmK {
  double e, k0A, alpha[6], lon0, false_north;
};

struct World {
  int32_t cs;
  double e2;               // ECEF: 1 - (1 - f)(1 - f)
  UtmK utm;
};

__device__ __forceinline__ void geo_world(const World &Wd, double lon, double lat, double alt, double &x, double &y, double &z) {
  const double rlat = lat * CAM_D2R;
  const double sp = sin(rlat), cp = cos(rlat);
  if (Wd.cs == BN_CS_ECEF) {
    const double rlon = lon * CAM_D2R;
    const double v = WGS84_A / sqrt(1.0 - Wd.e2 * sp * sp);
    x = (v + alt) * cp * cos(rlon);
    y = (v + alt) * cp * sin(rlon);
    z = (v * (1.0 - Wd.e2) + alt) * sp;
    return;
  }
  const UtmK &K = Wd.utm;
  const double dl = (lon - K.lon0) * CAM_D2R;
  const double tau = sp / cp;
  const double t = sinh(K.e * atanh(K.e * sp));
  const double taup = tau * sqrt(1.0 + t * t) - t * sqrt(1.0 + tau * tau);
  const double xip = atan2(taup, cos(dl));
  const double etap = atanh(sin(dl) / sqrt(1.0 + taup * taup));
  // sin(2 j (xi' + i eta')), j = 1 .. 6, by the angle-addition recurrence on complex numbers (re, im)
  const double s2 = sin(2.0 * xip), c2 = cos(2.0 * xip), sh2 = sinh(2.0 * etap), ch2 = cosh(2.0 * etap);
  const double zr = s2 * ch2, zi = c2 * sh2;        // sin(2 zeta)
  const double wr = c2 * ch2, wi = -(s2 * sh2);     // cos(2 zeta)
  double Sr = zr, Si = zi, Cr = wr, Ci = wi;
  double xi = xip, eta = etap;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    xi = xi + K.alpha[j] * Sr;
    eta = eta + K.alpha[j] * Si;
    const double nSr = (Sr * wr - Si * wi) + (Cr * zr - Ci * zi), nSi = (Sr * wi + Si * wr) + (Cr * zi + Ci * zr);
    const double nCr = (Cr * wr - Ci * wi) - (Sr * zr - Si * zi), nCi = (Cr * wi + Ci * wr) - (Sr * zi + Si * zr);
    Sr = nSr; Si = nSi; Cr = nCr; Ci = nCi;
  }
  x = 500000.0 + K.k0A * eta;
  y = K.false_north + K.k0A * xi;
  z = alt;
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

// the block's counted rows, one integer atomic (every thread of the block calls this)
__device__ __forceinline__ void count_block(bool bad, unsigned long long *counts) {
  __shared__ unsigned int block_bad;
  if (threadIdx.x == 0) block_bad = 0;
  __syncthreads();
  const unsigned long long ballot = __ballot(bad);
  if ((threadIdx.x & 63) == 0 && ballot) atomicAdd(&block_bad, (unsigned int)__popcll(ballot));       // LDS, integer
  __syncthreads();
  if (threadIdx.x == 0 && block_bad) atomicAdd(counts, (unsigned long long)block_bad);
}

__global__ __launch_bounds__(CAM_BLOCK)
void rpc_project_kernel(const bn_rpc R, const double *__restrict__ lon, const double *__restrict__ lat,
                        const double *__restrict__ alt, int64_t n, double *__restrict__ col, double *__restrict__ row) {
  const int64_t i = (int64_t)blockIdx.x * CAM_BLOCK + threadIdx.x;
  if (i >= n) return;
  const double L = (lon[i] - R.lon_offset) / R.lon_scale, P = (lat[i] - R.lat_offset) / R.lat_scale;
  const double H = (alt[i] - R.alt_offset) / R.alt_scale;
  const Mono m = monomials(L, P, H);
  col[i] = (poly(R.col_num, m) / poly(R.col_den, m)) * R.col_scale + R.col_offset;
  row[i] = (poly(R.row_num, m) / poly(R.row_den, m)) * R.row_scale + R.row_offset;
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
  count_block(bad, counts);
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

struct RayArgs {
  const double *cols, *rows;
  int32_t W, round_f32, has_sun;
  int64_t r0, r1, ray_stride;
  double min_alt, max_alt, cx, cy, cz, range;
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
    bad = localize(R, col, row, A.max_alt, lon_n, lat_n);
    bad = localize(R, col, row, A.min_alt, lon_f, lat_f) || bad;
    if (A.lonlat_near) {
      A.lonlat_near[2 * k] = lon_n;
      A.lonlat_near[2 * k + 1] = lat_n;
    }
    if (A.lonlat_far) {
      A.lonlat_far[2 * k] = lon_f;
      A.lonlat_far[2 * k + 1] = lat_f;
    }
    double nx, ny, nz, fx, fy, fz;
    geo_world(Wd, lon_n, lat_n, A.max_alt, nx, ny, nz);
    geo_world(Wd, lon_f, lat_f, A.min_alt, fx, fy, fz);
    const double dx = fx - nx, dy = fy - ny, dz = fz - nz;
    const double len = sqrt((dx * dx + dy * dy) + dz * dz);
    float v[8];
    v[3] = (float)(dx / len);
    v[4] = (float)(dy / len);
    v[5] = (float)(dz / len);
    v[6] = 0.f;
    if (A.round_f32) {
      const float rg = (float)A.range;
      v[0] = ((float)nx - (float)A.cx) / rg;
      v[1] = ((float)ny - (float)A.cy) / rg;
      v[2] = ((float)nz - (float)A.cz) / rg;
      v[7] = (float)len / rg;
    } else {
      v[0] = (float)((nx - A.cx) / A.range);
      v[1] = (float)((ny - A.cy) / A.range);
      v[2] = (float)((nz - A.cz) / A.range);
      v[7] = (float)(len / A.range);
    }
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 8; ++i) finite = finite && isfinite(v[i]);
    bad = bad || !finite;
    float *out = A.rays + k * A.ray_stride;
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = bad ? __builtin_nanf("") : v[i];
    if (A.has_sun) {
      out[8] = A.sun[0];
      out[9] = A.sun[1];
      out[10] = A.sun[2];
    }
  }
  count_block(bad, A.counts);
}

// ---------------------------------------------------------------------------------------------------------------- host side
bool rpc_ok(const bn_rpc *rpc) {
  const double *v = &rpc->row_offset;
  for (int i = 0; i < 90; ++i)
    if (!std::isfinite(v[i])) return false;
  for (int i = 5; i < 10; ++i)
    if (v[i] == 0.0) return false;
  return true;
}

// World of (cs, zone, south): the WGS84 constants of both coordinate systems
World make_world(int32_t cs, int32_t zone, int32_t south) {
  World w;
  const double f = 1.0 / WGS84_FINV;
  w.cs = cs;
  w.e2 = 1.0 - (1.0 - f) * (1.0 - f);
  const double n = f / (2.0 - f), n2 = n * n;
  UtmK &K = w.utm;
  K.e = std::sqrt(f * (2.0 - f));
  K.k0A = 0.9996 * (WGS84_A / (1.0 + n) * (1.0 + n2 / 4.0 + n2 * n2 / 64.0 + n2 * n2 * n2 / 256.0));
  // Karney 2011, eq. 35: alpha_j / n^j as polynomials in n (highest power first), over a common denominator
  K.alpha[0] = n * (((((31564.0 * n - 66675.0) * n + 34440.0) * n + 47250.0) * n - 100800.0) * n + 75600.0) / 151200.0;
  K.alpha[1] = n2 * ((((-1983433.0 * n + 863232.0) * n + 748608.0) * n - 1161216.0) * n + 524160.0) / 1935360.0;
  K.alpha[2] = n2 * n * (((670412.0 * n + 406647.0) * n - 533952.0) * n + 184464.0) / 725760.0;
  K.alpha[3] = n2 * n2 * ((6601661.0 * n - 7732800.0) * n + 2230245.0) / 7257600.0;
  K.alpha[4] = n2 * n2 * n * (-13675556.0 * n + 3438171.0) / 7983360.0;
  K.alpha[5] = n2 * n2 * n2 * 212378941.0 / 319334400.0;
  K.lon0 = 6.0 * zone - 183.0;
  K.false_north = south ? 10000000.0 : 0.0;
  return w;
}

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
  a.cols = cols; a.rows = rows; a.W = W; a.round_f32 = round_f32; a.has_sun = sun != nullptr;
  a.r0 = r0; a.r1 = r1; a.ray_stride = ray_stride;
  a.min_alt = min_alt; a.max_alt = max_alt; a.cx = center[0]; a.cy = center[1]; a.cz = center[2]; a.range = range;
  for (int i = 0; i < 3; ++i) a.sun[i] = sun ? sun[i] : 0.f;
  a.rays = rays; a.lonlat_near = lonlat_near; a.lonlat_far = lonlat_far; a.counts = counts;
  rpc_rays_kernel<<<(unsigned)ceil_div64(r1 - r0, CAM_BLOCK), CAM_BLOCK, 0, (hipStream_t)stream>>>(*rpc, make_world(cs, zone, south), a);
  BN_LAUNCH_CHECK("rpc_rays");
  return 0;
}
