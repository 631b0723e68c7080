// Per-SAMPLE shading on the field-output rows as they are stored, forward and backward, one thread per row (round 5):
// --MultiBRDF (models/spsbrdfnerf.py:289-307, 350-352: every sample is shaded by its own BRDF and the shaded colours are
// composited), and the per-sample irradiance of the sun-visibility pass (:265-273, :350-354: with --sun_v analystic each sample's
// colour - its BRDF value, or its padded albedo when no BRDF shades - is weighted by the sun pass's transparency at its position).  The BRDF is a pointwise function of a row - its normal, albedo and BRDF-parameter channels - and of
// its ray's sun / view directions, so the training step evaluates it on the [pass-1 block | guided block] rows without
// materialising the merged set and composites the result through the sort index (bn_lambert_tail / bn_merged_composite_*).
// Rounds 3-4 did this through torch.autograd.Function wrappers of the per-point BRDF kernels (brdf.hip): ~20 glue launches
// (gathers of the per-ray directions, channel slices, the padding / irradiance arithmetic and their backward).  Here: ONE launch
// forward (the padded, irradiance-weighted colour as channels 0-2 of a 4-wide [bp, sigma] or full-width copy of the rows) and
// ONE backward (J^T of the same evaluation in forward-mode duals, like ray_tail.hip, added to the pass-through channels).
#include "common.h"
#include "brdfnerf_hip.h"
#include "prof.h"
// (no FMA contraction, like brdf.hip: the degenerate-geometry branches must round like the reference's separate ATen ops)
#pragma clang fp contract(off)
#include "brdf_eval.h"
#include "shade_row.h"

namespace {

struct SampleArgs {
  bn_shade_desc d;       // kind, C, ch_normal, ch_p0..2, rhoc_is_albedo, shell, cos_irradiance, hpk_scl, f0, rgb_padding
  const float *X;        // [N][C] field-output rows
  const float *rays;     // [R][ray_stride]: view = -rays[3:6], sun = rays[sun_col : +3] (sun_col < 0: (1, 1, 1))
  int64_t ray_stride;
  int sun_col;
  int64_t N, n1;         // rows [0, n1) belong to ray row / S1, rows [n1, N) to ray (row - n1) / S2
  int S1, S2;
  float *B;              // forward: [N][b_stride]; b_stride == 4: [bp, sigma]; b_stride == C: the row with channels 0-2 replaced by bp
  int b_stride;
  const float *dB;       // backward: [N][b_stride]
  float *dX;             // backward: [N][C]
};

// the row's BRDF (shade_row.h row_brdf) at the row's own normal and albedo, as they are stored
template <int KIND, typename S, typename Seed>
__device__ __forceinline__ void raw_row_brdf(const bn_shade_desc &q, const float *x, const float (&sun)[3], const float (&view)[3], Seed seed_,
                                             S (&out)[3]) {
  const V3<S> n = {seed_(x[q.ch_normal], 0), seed_(x[q.ch_normal + 1], 1), seed_(x[q.ch_normal + 2], 2)};
  S w[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) w[c] = seed_(x[c], 3 + c);
  row_brdf<KIND, S>(q, x, sun, view, n, w, seed_, out);
}

template <int KIND, bool BWD> __global__ __launch_bounds__(128) void sample_brdf_kernel(const SampleArgs A) {
  const int64_t row = (int64_t)blockIdx.x * 128 + threadIdx.x;
  if (row >= A.N) return;
  const bn_shade_desc &q = A.d;
  const int C = q.C;
  const int64_t ray = row < A.n1 ? row / A.S1 : (row - A.n1) / A.S2;
  const float *rr = A.rays + ray * A.ray_stride;
  const float view[3] = {-rr[3], -rr[4], -rr[5]};
  const float sun[3] = {A.sun_col >= 0 ? rr[A.sun_col] : 1.f, A.sun_col >= 0 ? rr[A.sun_col + 1] : 1.f, A.sun_col >= 0 ? rr[A.sun_col + 2] : 1.f};
  const float pad = q.rgb_padding;
  // bp = brdf (1 + 2 pad) - pad, times |sun_z| with the cosine irradiance of an upward normal (spsbrdfnerf.py:260-264, 270-275:
  // only a model with a normal field has it), else times the row's sun visibility (:265-273), else as it is
  const float gain = (1.f + 2.f * pad);
  const float irr = (q.cos_irradiance && q.ch_normal >= 0) ? fabsf(sun[2]) : (q.irr ? q.irr[row * q.irr_stride] : 1.f);
  const float *x = A.X + row * C;
  if constexpr (KIND == BN_SHADE_LAMBERT) {
    // no BRDF: the padded albedo itself (the Lambertian rgb under a per-sample irradiance)
    if constexpr (!BWD) {
      float *b = A.B + row * A.b_stride;
      if (A.b_stride == C)
        for (int c = 4; c < C; ++c) b[c] = x[c];
#pragma unroll
      for (int c = 0; c < 3; ++c) b[c] = (x[c] * gain - pad) * irr;
      b[3] = x[3];
    } else {
      const float *db_ = A.dB + row * A.b_stride;
      float *dx = A.dX + row * C;
#pragma unroll
      for (int c = 0; c < 3; ++c) dx[c] = db_[c] * gain * irr;
      dx[3] = db_[3];
      for (int c = 4; c < C; ++c) dx[c] = A.b_stride == C ? db_[c] : 0.f;
    }
    return;
  }
  if constexpr (!BWD) {
    float out[3];
    raw_row_brdf<KIND, float>(q, x, sun, view, [](float v_, int) { return v_; }, out);
    float *b = A.B + row * A.b_stride;
    if (A.b_stride == C)
      for (int c = 4; c < C; ++c) b[c] = x[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) b[c] = (out[c] * gain - pad) * irr;
    b[3] = x[3];
  } else {
    constexpr int NS = Slots<KIND>::N;
    typedef Dual<NS> D;
    D out[3];
    raw_row_brdf<KIND, D>(q, x, sun, view, [](float v_, int slot) { return seed<NS>(v_, slot); }, out);
    const float *db_ = A.dB + row * A.b_stride;
    const float db[3] = {db_[0] * gain * irr, db_[1] * gain * irr, db_[2] * gain * irr};
    float *dx = A.dX + row * C;
    // pass-through channels: sigma always; everything behind it when the copy is full width (the regularisers' terms on the
    // per-sample normals arrive there); the colour channels of the copy are the BRDF's output, so the row's own albedo gets the
    // BRDF path only
    dx[3] = db_[3];
    for (int c = 4; c < C; ++c) dx[c] = A.b_stride == C ? db_[c] : 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) dx[c] = jt(out, db, 3 + c);
    scatter_jt<KIND, true>(q, out, db, dx);
  }
}

int check_args(const bn_shade_desc *desc, const float *X, const float *rays, int64_t R, int64_t ray_stride, int32_t sun_col, int64_t N,
               int64_t n1, int32_t S1, int32_t S2, int32_t stride, const char *what) {
  BN_REQUIRE(desc && X && rays && N > 0, "%s: null argument", what);
  const bn_shade_desc &q = *desc;
  if (int e = shade_desc_check(q, true, what)) return e;
  BN_REQUIRE(stride == 4 || stride == q.C, "%s: C=%d, row stride %d (4 or C)", what, q.C, stride);
  BN_REQUIRE(!q.irr || q.irr_stride >= 0, "%s: irradiance stride %lld", what, (long long)q.irr_stride);
  BN_REQUIRE(ray_stride >= 6 && (sun_col < 0 || sun_col + 3 <= ray_stride), "%s: ray stride %lld, sun column %d", what, (long long)ray_stride, sun_col);
  // every row's ray exists: the blocks are R rays of S1 (and, behind row n1, R rays of S2) samples each
  BN_REQUIRE(R > 0 && S1 > 0 && n1 == R * (int64_t)S1 && (n1 == N || (S2 > 0 && N - n1 == R * (int64_t)S2)),
             "%s: %lld rows do not split into %lld rays of %d (+ %d) samples at row %lld", what, (long long)N, (long long)R, S1, S2, (long long)n1);
  return 0;
}

template <bool BWD> int launch(const SampleArgs &a, hipStream_t st) {
  const dim3 grid((unsigned)ceil_div64(a.N, 128));
  BnProfScope prof_(BN_K_BRDF, st);
  shade_dispatch(a.d, [&](auto kind, auto) { sample_brdf_kernel<decltype(kind)::value, BWD><<<grid, 128, 0, st>>>(a); });
  BN_LAUNCH_CHECK(BWD ? "sample_brdf_backward" : "sample_brdf_forward");
  return 0;
}

}  // namespace

extern "C" int bn_sample_brdf_forward(const bn_shade_desc *desc, const float *X, const float *rays, int64_t R, int64_t ray_stride,
                                      int32_t sun_col, int64_t N, int64_t n1, int32_t S1, int32_t S2, float *B, int32_t b_stride,
                                      void *stream) {
  if (int e = check_args(desc, X, rays, R, ray_stride, sun_col, N, n1, S1, S2, b_stride, "sample_brdf_forward")) return e;
  BN_REQUIRE(B, "sample_brdf_forward: null output");
  SampleArgs a;
  a.d = *desc; a.X = X; a.rays = rays; a.ray_stride = ray_stride; a.sun_col = sun_col; a.N = N; a.n1 = n1; a.S1 = S1; a.S2 = S2 > 0 ? S2 : 1;
  a.B = B; a.b_stride = b_stride; a.dB = nullptr; a.dX = nullptr;
  return launch<false>(a, (hipStream_t)stream);
}

extern "C" int bn_sample_brdf_backward(const bn_shade_desc *desc, const float *X, const float *rays, int64_t R, int64_t ray_stride,
                                       int32_t sun_col, int64_t N, int64_t n1, int32_t S1, int32_t S2, const float *dB, int32_t b_stride,
                                       float *dX, void *stream) {
  if (int e = check_args(desc, X, rays, R, ray_stride, sun_col, N, n1, S1, S2, b_stride, "sample_brdf_backward")) return e;
  BN_REQUIRE(dB && dX, "sample_brdf_backward: null argument");
  SampleArgs a;
  a.d = *desc; a.X = X; a.rays = rays; a.ray_stride = ray_stride; a.sun_col = sun_col; a.N = N; a.n1 = n1; a.S1 = S1; a.S2 = S2 > 0 ? S2 : 1;
  a.B = nullptr; a.b_stride = b_stride; a.dB = dB; a.dX = dX;
  return launch<true>(a, (hipStream_t)stream);
}
