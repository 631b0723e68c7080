// The RPC polynomials shared by camera.hip (the rays and the depth priors of a view) and orthophoto.hip (the cells of a surface
// model taken to the pixels of an observed image): the 20 monomials of (L, P, H), a polynomial over them and the projection of a
// geodetic point, steps 1 and 2 of include/brdfnerf_hip.h ("The rays of a satellite view").  One statement, so that the pixel of
// a point is the same bits wherever it is formed.  Only + x / occur; both files are built with fp contraction off and the pragma
// below covers the functions here wherever they are included.
#pragma once
#include <cmath>
#include "common.h"
#include "brdfnerf_hip.h"
#pragma clang fp contract(off)

namespace rpc_poly {

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

// steps 1 and 2 of the header: the pixel (col, row) of the geodetic point (lon, lat, alt)
__device__ __forceinline__ void project(const bn_rpc &R, double lon, double lat, double alt, double &col, double &row) {
  const double L = (lon - R.lon_offset) / R.lon_scale, P = (lat - R.lat_offset) / R.lat_scale;
  const double H = (alt - R.alt_offset) / R.alt_scale;
  const Mono m = monomials(L, P, H);
  col = (poly(R.col_num, m) / poly(R.col_den, m)) * R.col_scale + R.col_offset;
  row = (poly(R.row_num, m) / poly(R.row_den, m)) * R.row_scale + R.row_offset;
}

// ---------------------------------------------------------------------------------------------------------------- host side
// what every entry that takes a descriptor refuses of it: a non-finite entry, a scale of zero
inline bool rpc_ok(const bn_rpc *rpc) {
  const double *v = &rpc->row_offset;
  for (int i = 0; i < 90; ++i)
    if (!std::isfinite(v[i])) return false;
  for (int i = 5; i < 10; ++i)
    if (v[i] == 0.0) return false;
  return true;
}

}  // namespace rpc_poly
