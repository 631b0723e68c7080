// The float64 geodesy shared by camera.hip (geodetic -> world: the rays and the depth priors of a view), world.hip (world ->
// east, north, altitude: the surface model of an ECEF scene) and orthophoto.hip (east, north -> geodetic: the cells of a surface
// model on their way to the pixels of an image): the WGS84 constants as the host forms them, the forward rule of
// include/brdfnerf_hip.h ("The rays of a satellite view", step 4), the ECEF inverse ("World points of an ECEF scene") and the
// UTM inverse ("Orthophoto of an observed image", step 2).  Every
// operation is rounded on its own: both files are built with fp contraction off and the pragma below covers the functions here
// wherever they are included.  The device's float64 sin / cos / atan2 / atanh / sinh / cosh are not bit-specified: what comes out
// of them is held to a bound, not to bits.
#pragma once
#include <cmath>
#include "common.h"
#pragma clang fp contract(off)

namespace geodesy {

constexpr double CAM_D2R = 3.14159265358979323846 / 180.0;        // np.pi / 180.0
constexpr double CAM_PI = 3.14159265358979323846;                 // np.pi
constexpr double WGS84_A = 6378137.0, WGS84_FINV = 298.257223563;

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

// the constants of the inverse UTM series, formed once on the host (make_utm_inv); a struct of its own, so that UtmK and World -
// kernel arguments of camera.hip, world.hip and ortho.hip - keep their layout
struct UtmInvK {
  double e, e2m, k0A, beta[6], lon0, false_north;        // e2m = 1 - e e
};

// "Orthophoto of an observed image" in the header, step 2: (east, north) in the zone of K -> geodetic degrees.  Karney 2011,
// eq. 36 (the series back to the conformal sphere, the six sin(2 j (xi + i eta)) by geo_world's angle-addition recurrence) and
// eqs. 19-21 (Newton for tau = tan(lat) from tau', BN_UTM_NEWTON_ITERS iterations for every lane, no data-dependent exit).
// -> true when the point is refused (lon or lat not finite; both are NaN then).
__device__ __forceinline__ bool utm_geodetic(const UtmInvK &K, double east, double north, double &lon, double &lat) {
  const double xi = (north - K.false_north) / K.k0A, eta = (east - 500000.0) / K.k0A;
  const double s2 = sin(2.0 * xi), c2 = cos(2.0 * xi), sh2 = sinh(2.0 * eta), ch2 = cosh(2.0 * eta);
  const double zr = s2 * ch2, zi = c2 * sh2;        // sin(2 zeta)
  const double wr = c2 * ch2, wi = -(s2 * sh2);     // cos(2 zeta)
  double Sr = zr, Si = zi, Cr = wr, Ci = wi;
  double xip = xi, etap = eta;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    xip = xip - K.beta[j] * Sr;
    etap = etap - K.beta[j] * Si;
    const double nSr = (Sr * wr - Si * wi) + (Cr * zr - Ci * zi), nSi = (Sr * wi + Si * wr) + (Cr * zi + Ci * zr);
    const double nCr = (Cr * wr - Ci * wi) - (Sr * zr - Si * zi), nCi = (Cr * wi + Ci * wr) - (Sr * zi + Si * zr);
    Sr = nSr; Si = nSi; Cr = nCr; Ci = nCi;
  }
  const double sh = sinh(etap), cx = cos(xip);
  const double taup = sin(xip) / sqrt(sh * sh + cx * cx);
  double tau = taup;
#pragma unroll 1
  for (int it = 0; it < BN_UTM_NEWTON_ITERS; ++it) {
    const double r = sqrt(1.0 + tau * tau);
    const double sigma = sinh(K.e * atanh(K.e * tau / r));
    const double t = tau * sqrt(1.0 + sigma * sigma) - sigma * r;
    tau = tau + (taup - t) / sqrt(1.0 + t * t) * (1.0 + K.e2m * (tau * tau)) / (K.e2m * r);
  }
  lon = K.lon0 + atan2(sh, cx) * 180.0 / CAM_PI;
  lat = atan(tau) * 180.0 / CAM_PI;
  const bool bad = !(isfinite(lon) && isfinite(lat));
  if (bad) lon = lat = __builtin_nan("");
  return bad;
}

// the constants of sat_utils.ecef_to_latlon_custom (:131-137), formed once on the host
struct EcefK {
  double a, b, esq, k1, k2;        // k1 = (ep ep) b, k2 = esq a
};

// "World points of an ECEF scene" in the header: Bowring's one-step formula as upstream writes it, the cubes as (s s) s.
// -> true when the point is refused: on the axis (p == 0), or x, y, z, lat or alt not finite.  lon, lat in degrees.
__device__ __forceinline__ bool ecef_geodetic(const EcefK &K, double x, double y, double z, double &lon, double &lat, double &alt) {
  const double p = sqrt(x * x + y * y);
  const double th = atan2(K.a * z, K.b * p);
  const double s = sin(th), c = cos(th);
  const double rlon = atan2(y, x);
  const double rlat = atan2(z + K.k1 * ((s * s) * s), p - K.k2 * ((c * c) * c));
  const double sl = sin(rlat);
  const double N = K.a / sqrt(1.0 - K.esq * (sl * sl));
  alt = p / cos(rlat) - N;
  lon = rlon * 180.0 / CAM_PI;
  lat = rlat * 180.0 / CAM_PI;
  return p == 0.0 || !(isfinite(x) && isfinite(y) && isfinite(z) && isfinite(rlat) && isfinite(alt));
}

// ---------------------------------------------------------------------------------------------------------------- host side
// World of (cs, zone, south): the WGS84 constants of both coordinate systems
inline World make_world(int32_t cs, int32_t zone, int32_t south) {
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

// UtmInvK of (zone, south): n, e and k0 A exactly as make_world forms them; Karney 2011, eq. 36: beta_j as polynomials in n, in
// Horner form, every fraction one division
inline UtmInvK make_utm_inv(int32_t zone, int32_t south) {
  UtmInvK K;
  const double f = 1.0 / WGS84_FINV;
  const double n = f / (2.0 - f), n2 = n * n;
  K.e = std::sqrt(f * (2.0 - f));
  K.e2m = 1.0 - K.e * K.e;
  K.k0A = 0.9996 * (WGS84_A / (1.0 + n) * (1.0 + n2 / 4.0 + n2 * n2 / 64.0 + n2 * n2 * n2 / 256.0));
  K.beta[0] = n * (1.0 / 2.0 + n * (-2.0 / 3.0 + n * (37.0 / 96.0 + n * (-1.0 / 360.0 + n * (-81.0 / 512.0 + n * (96199.0 / 604800.0))))));
  K.beta[1] = n2 * (1.0 / 48.0 + n * (1.0 / 15.0 + n * (-437.0 / 1440.0 + n * (46.0 / 105.0 + n * (-1118711.0 / 3870720.0)))));
  K.beta[2] = n2 * n * (17.0 / 480.0 + n * (-37.0 / 840.0 + n * (-209.0 / 4480.0 + n * (5569.0 / 90720.0))));
  K.beta[3] = n2 * n2 * (4397.0 / 161280.0 + n * (-11.0 / 504.0 + n * (-830251.0 / 7257600.0)));
  K.beta[4] = n2 * n2 * n * (4583.0 / 161280.0 + n * (-108847.0 / 3991680.0));
  K.beta[5] = n2 * n2 * n2 * (20648693.0 / 638668800.0);
  K.lon0 = 6.0 * zone - 183.0;
  K.false_north = south ? 10000000.0 : 0.0;
  return K;
}

// upstream's truncated eccentricity, NOT the one of 1 / 298.257223563 that make_world uses (6e-15 apart, relative)
inline EcefK make_ecef_k() {
  EcefK k;
  const double e = 8.1819190842622e-2;
  k.a = WGS84_A;
  const double asq = k.a * k.a;
  k.esq = e * e;
  k.b = std::sqrt(asq * (1.0 - k.esq));
  const double bsq = k.b * k.b;
  const double ep = std::sqrt((asq - bsq) / bsq);
  k.k1 = (ep * ep) * k.b;
  k.k2 = k.esq * k.a;
  return k;
}

}  // namespace geodesy
