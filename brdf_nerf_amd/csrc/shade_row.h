// What the kernels that shade a row of field outputs with a bn_shade_desc share: the descriptor's argument checks, the
// KIND x MASK dispatch and the direction tile on the host; on the device the unpacking of a row and the call of its BRDF body, as
// floats with a compile-time MASK (relight.hip, sun_shadow.hip) and in forward-mode duals (ray_tail.hip, sample_brdf.hip).
// Training and relighting must round alike, so each of these is stated once.
// Include it behind the file's `#pragma clang fp contract(off)` and behind brdf_eval.h: it inherits the contraction setting.
#pragma once
#include <type_traits>
#include "brdf_eval.h"
#include "brdfnerf_hip.h"

// ------------------------------------------------------------------ host side
// The clauses every shading entry point puts to its descriptor (`what`: the entry's name, the head of the message).  have_dirs:
// the directions a BRDF kind is evaluated at were given.  Clauses of one entry alone stay with that entry.
static inline int shade_desc_check(const bn_shade_desc &q, bool have_dirs, const char *what) {
  BN_REQUIRE(q.C >= 4 && q.C <= BN_MAX_CH, "%s: C=%d unsupported", what, q.C);
  BN_REQUIRE(q.kind >= BN_SHADE_LAMBERT && q.kind <= BN_SHADE_MICROFACET, "%s: kind=%d", what, q.kind);
  auto in_range = [&](int ch, int n) { return ch < 0 || (ch >= 4 && ch + n <= q.C); };
  BN_REQUIRE(in_range(q.ch_normal, 3), "%s: normal channel %d outside [4, %d)", what, q.ch_normal, q.C);
  if (q.kind != BN_SHADE_LAMBERT) {
    BN_REQUIRE(q.ch_normal >= 4 && have_dirs, "%s: BRDF shading needs a normal field and the ray directions", what);
    const int n2 = q.kind == BN_SHADE_HAPKE ? 1 : 3;           // Hapke's theta is one channel wide
    const int n0 = q.kind == BN_SHADE_MICROFACET ? 1 : 3;
    BN_REQUIRE(in_range(q.ch_p0, n0) && in_range(q.ch_p1, 3) && in_range(q.ch_p2, n2), "%s: parameter channels (%d, %d, %d) outside [4, %d)",
               what, q.ch_p0, q.ch_p1, q.ch_p2, q.C);
    BN_REQUIRE(q.kind != BN_SHADE_MICROFACET || q.ch_p0 >= 4, "%s: microfacet needs the roughness channel", what);
    BN_REQUIRE(q.kind != BN_SHADE_HAPKE || q.ch_p0 >= 4 || (q.shell >= 1 && q.shell <= 3), "%s: Hapke without b needs shell_hapke in {1,2,3}", what);
  }
  return 0;
}

// MASK of the float kernels: which of the BRDF's parameter heads exist (bit 0 p0, bit 1 p1, bit 2 p2 - or, for RPV, rhoc = albedo)
static inline int shade_mask(const bn_shade_desc &q) {
  return (q.ch_p0 >= 0 ? 1 : 0) | (q.ch_p1 >= 0 ? 2 : 0) | ((q.ch_p2 >= 0 || (q.kind == BN_SHADE_RPV && q.rhoc_is_albedo)) ? 4 : 0);
}

// f(integral_constant KIND, integral_constant MASK) for a checked descriptor.  The pairs it can name are the kernels that exist:
// Lambert (0, 0), RPV and Hapke masks 0..7, microfacet (3, 1).  A kernel without a MASK (the dual form) ignores the second.
template <int KIND, typename F> void shade_dispatch_mask(int mask, F &&f) {
  using K = std::integral_constant<int, KIND>;
  switch (mask) {
    case 0: f(K{}, std::integral_constant<int, 0>{}); break;
    case 1: f(K{}, std::integral_constant<int, 1>{}); break;
    case 2: f(K{}, std::integral_constant<int, 2>{}); break;
    case 3: f(K{}, std::integral_constant<int, 3>{}); break;
    case 4: f(K{}, std::integral_constant<int, 4>{}); break;
    case 5: f(K{}, std::integral_constant<int, 5>{}); break;
    case 6: f(K{}, std::integral_constant<int, 6>{}); break;
    default: f(K{}, std::integral_constant<int, 7>{}); break;
  }
}
template <typename F> void shade_dispatch(const bn_shade_desc &q, F &&f) {
  switch (q.kind) {
    case BN_SHADE_LAMBERT: f(std::integral_constant<int, BN_SHADE_LAMBERT>{}, std::integral_constant<int, 0>{}); break;
    case BN_SHADE_RPV: shade_dispatch_mask<BN_SHADE_RPV>(shade_mask(q), f); break;
    case BN_SHADE_HAPKE: shade_dispatch_mask<BN_SHADE_HAPKE>(shade_mask(q), f); break;
    default: f(std::integral_constant<int, BN_SHADE_MICROFACET>{}, std::integral_constant<int, 1>{}); break;
  }
}

// Directions one block takes (grid = ray blocks x direction tiles): as many as possible, up to `cap` - a ray's row is loaded and
// prepared once per tile - while ray blocks x tiles still give every CU several waves; at least what keeps gridDim.y <= 65535;
// a multiple of `trip`, the directions the kernel walks together.  Every (direction, ray) is computed on its own: the tiling
// changes no bit.
static inline int64_t dir_tile(int64_t K, int64_t blocks, int64_t cap, int64_t trip) {
  int64_t kt = K * blocks / 2048;
  kt = kt < 1 ? 1 : (kt > cap ? cap : kt);
  const int64_t need = ceil_div64(K, 65535);               // gridDim.y <= 65535
  if (kt < need) kt = need;
  return ceil_div64(kt, trip) * trip;
}

// ------------------------------------------------------------------ device side, both forms
// l2_normalize (train_utils.py:28-33)
template <typename S> __device__ __forceinline__ V3<S> unit_normal(const V3<S> &n) {
  const S nrm = sqrt_(clamp_min_(dot3(n, n), 1.1920928955078125e-07f));
  return {n.x / nrm, n.y / nrm, n.z / nrm};
}

// one channel of the composited albedo sum_s w (albedo (1 + 2 pad) - pad)   (models/spsbrdfnerf.py:270, :275)
__device__ __forceinline__ float padded_albedo(float acc, float pad, float wsum) { return acc * (1.f + 2.f * pad) - pad * wsum; }

// ------------------------------------------------------------------ device side, float form
// KIND: BN_SHADE_*.  MASK: shade_mask() as a compile-time constant, so that the nullable-pointer arguments of the BRDF bodies fold
// away and the parameters stay in registers (a run-time select between a local array and nullptr forces the array into scratch).

// The parameter channels of row x into p0 / p1 / p2 (the caller zeroes them; w: the row's albedo, seeded as the body takes it).
template <int KIND, int MASK>
__device__ __forceinline__ void row_params(const bn_shade_desc &q, const float *x, const float (&w)[3], float (&p0)[3], float (&p1)[3],
                                           float (&p2)[3]) {
  if (KIND == BN_SHADE_MICROFACET) {
    p0[0] = x[q.ch_p0];
  } else {
    const int n2 = KIND == BN_SHADE_HAPKE ? 1 : 3;          // Hapke's theta is one channel wide
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (MASK & 1) p0[c] = x[q.ch_p0 + c];
      if (MASK & 2) p1[c] = x[q.ch_p1 + c];
      if ((MASK & 4) && c < n2) p2[c] = (KIND == BN_SHADE_RPV && q.rhoc_is_albedo) ? w[c] : x[q.ch_p2 + c];   // funcH == 2 (:288-291)
    }
  }
}

// The row's BRDF under sun l and view v; Lambert: the albedo itself.
template <int KIND, int MASK>
__device__ __forceinline__ void brdf_value(const bn_shade_desc &q, const V3<float> &l, const V3<float> &v, const V3<float> &ns,
                                           const float (&w)[3], const float (&p0)[3], const float (&p1)[3], const float (&p2)[3],
                                           float (&out)[3]) {
  if (KIND == BN_SHADE_LAMBERT) {
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = w[c];
  } else if (KIND == BN_SHADE_RPV) {
    rpv_eval<float>(l, v, ns, w, (MASK & 1) ? p0 : nullptr, (MASK & 2) ? p1 : nullptr, (MASK & 4) ? p2 : nullptr, out, nullptr);
  } else if (KIND == BN_SHADE_HAPKE) {
    hapke_eval<float>(l, v, ns, w, (MASK & 1) ? p0 : nullptr, (MASK & 2) ? p1 : nullptr, (MASK & 4) ? p2 : nullptr, q.hpk_scl,
                      q.shell, out, nullptr);
  } else {
    microfacet_eval<float>(l, v, ns, w, p0[0], q.f0, out, nullptr);
  }
}

// ------------------------------------------------------------------ device side, dual form
// Which heads exist is read from the descriptor at run time here; the kernels are instantiated per KIND only.
// Dual slots: normal 0-2, albedo 3-5, then the BRDF parameters (RPV: k 6-8, theta 9-11, rhoc 12-14; Hapke: b 6-8, c 9-11,
// theta 12; microfacet: roughness 6).
template <int KIND> struct Slots { static constexpr int N = KIND == BN_SHADE_RPV ? 15 : KIND == BN_SHADE_HAPKE ? 13 : 7; };

// The BRDF of a row over the scalar type S (float: values; Dual<N>: values + Jacobian).  n, w: the normal and the albedo as the
// body takes them, seeded by the caller (the raw row, or the normalised composited normal and the padded composited albedo);
// the parameter slots are seeded here from the channels of x.
template <int KIND, typename S, typename Seed>
__device__ __forceinline__ void row_brdf(const bn_shade_desc &q, const float *x, const float (&sun)[3], const float (&view)[3], const V3<S> &n,
                                         const S (&w_)[3], Seed seed_, S (&out)[3]) {
  // (a copy of this function's own: the bodies take w as a pointer, and beside the run-time selects below an array of the caller's
  // stays in scratch - 12 bytes more in the float RPV kernel of sample_brdf.hip)
  const S w[3] = {w_[0], w_[1], w_[2]};
  const V3<S> l = {cst(w[0], sun[0]), cst(w[0], sun[1]), cst(w[0], sun[2])}, v = {cst(w[0], view[0]), cst(w[0], view[1]), cst(w[0], view[2])};
  if (KIND == BN_SHADE_RPV) {
    S k[3], th[3], rc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      k[c] = seed_(q.ch_p0 >= 0 ? x[q.ch_p0 + c] : 0.f, 6 + c);
      th[c] = seed_(q.ch_p1 >= 0 ? x[q.ch_p1 + c] : 0.f, 9 + c);
      rc[c] = q.rhoc_is_albedo ? w[c] : seed_(q.ch_p2 >= 0 ? x[q.ch_p2 + c] : 0.f, 12 + c);      // funcH == 2 (spsbrdfnerf.py:288-291)
    }
    rpv_eval<S>(l, v, n, w, q.ch_p0 >= 0 ? k : nullptr, q.ch_p1 >= 0 ? th : nullptr, (q.ch_p2 >= 0 || q.rhoc_is_albedo) ? rc : nullptr,
                out, nullptr);
  } else if (KIND == BN_SHADE_HAPKE) {
    S b[3], cc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      b[c] = seed_(q.ch_p0 >= 0 ? x[q.ch_p0 + c] : 0.f, 6 + c);
      cc[c] = seed_(q.ch_p1 >= 0 ? x[q.ch_p1 + c] : 0.f, 9 + c);
    }
    const S th = seed_(q.ch_p2 >= 0 ? x[q.ch_p2] : 0.f, 12);
    hapke_eval<S>(l, v, n, w, q.ch_p0 >= 0 ? b : nullptr, q.ch_p1 >= 0 ? cc : nullptr, q.ch_p2 >= 0 ? &th : nullptr, q.hpk_scl, q.shell, out,
                  nullptr);
  } else {
    const S rg = seed_(x[q.ch_p0], 6);
    microfacet_eval<S>(l, v, n, w, rg, q.f0, out, nullptr);
  }
}

// J^T of row_brdf, slots -> the normal and parameter channels of dst.  ACCUM: added to what dst holds (a row's pass-through
// terms), else stored - a store is not an add onto a zeroed row: 0 + (-0) is +0.  The albedo channels stay with the caller
// (gain and padding differ).
template <int KIND, bool ACCUM, int N>
__device__ __forceinline__ void scatter_jt(const bn_shade_desc &q, const Dual<N> (&out)[3], const float (&db)[3], float *dst) {
  auto put = [&](int ch, int slot) {
    const float g = jt(out, db, slot);
    if (ACCUM) dst[ch] += g;
    else dst[ch] = g;
  };
#pragma unroll
  for (int c = 0; c < 3; ++c) put(q.ch_normal + c, c);
  if (KIND == BN_SHADE_RPV || KIND == BN_SHADE_HAPKE) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (q.ch_p0 >= 0) put(q.ch_p0 + c, 6 + c);
      if (q.ch_p1 >= 0) put(q.ch_p1 + c, 9 + c);
      if (KIND == BN_SHADE_RPV && q.ch_p2 >= 0 && !q.rhoc_is_albedo) put(q.ch_p2 + c, 12 + c);
    }
    if (KIND == BN_SHADE_HAPKE && q.ch_p2 >= 0) put(q.ch_p2, 12);
  } else {
    put(q.ch_p0, 6);
  }
}
