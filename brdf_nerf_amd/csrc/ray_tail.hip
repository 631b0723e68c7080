// Ray-level shading + losses of the fused training step, forward and backward in one launch, one thread per ray.
//
// The step composites the merged sample set into per-ray sums acc[c] = sum_s w_s out[s][c] (bn_merged_composite_forward);
// everything the loss reads after that is a function of those sums when every ray has ONE BRDF (MultiBRDF == 0) and no
// per-sample irradiance: the composited albedo, the normalised composited normal, the composited BRDF parameters, the BRDF
// itself, the clamp, SNerfLoss, DepthLoss and HardSurfaceLoss.  This kernel evaluates that chain with forward-mode duals
// seeded at the sums and returns d loss / d acc, d loss / d (sum w) and d loss / d depth for bn_merged_composite_backward.
// Replaces, for the training step: models/spsbrdfnerf.py:259-357 (ray-level shading), BRDF/*.py, metrics.py:39-61
// (SNerfLoss, lambda_sc = 0), metrics.py:82-161 (DepthLoss), metrics.py:263-290 (HardSurfaceLoss) and their autograd graphs.
#include "common.h"
#include "brdfnerf_hip.h"
#include "prof.h"
// (no FMA contraction, like brdf.hip: the degenerate-geometry branches must round like the reference's separate ATen ops)
#pragma clang fp contract(off)
#include "brdf_eval.h"
#include "shade_row.h"
#include "composite_ray.h"

namespace {

struct ShadeArgs {
  bn_shade_desc d;
  const float *acc, *wsum, *depth, *var;
  const float *rays_d, *sun_d;           // sun_d nullptr: (1, 1, 1) (the non-satellite data sets, rendering.py:190)
  int64_t rd_stride, sd_stride;
  const float *rgbs;
  DepthPrior prior;
  int64_t R;
  float *rgb, *ray_loss, *loss_acc;
  int loss_slots;                       // report_ray_loss (composite_ray.h)
  float *d_acc, *d_wsum, *d_depth;
  const float *extra_loss;              // nullable: per-ray loss terms computed elsewhere (NormalRegLoss of the compositing kernel)
  unsigned long long *nonfinite;        // nullable: report_ray_loss
};

// KIND: BN_SHADE_LAMBERT / RPV / HAPKE / MICROFACET.  Dual slots (shade_row.h): the normal and albedo slots are seeded at the
// COMPOSITED normal and albedo.
template <int KIND> __global__ __launch_bounds__(64) void ray_shade_loss_kernel(const ShadeArgs A) {
  constexpr int N = Slots<KIND>::N;
  typedef Dual<N> D;
  const int64_t ray = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (ray >= A.R) return;
  const bn_shade_desc &q = A.d;
  const int C = q.C;
  const float *acc = A.acc + ray * C;
  const float ws = A.wsum[ray], depth = A.depth[ray];
  const float pad = q.rgb_padding;
  const bool has_n = q.ch_normal >= 0;
  const float sun[3] = {A.sun_d ? A.sun_d[ray * A.sd_stride] : 1.f, A.sun_d ? A.sun_d[ray * A.sd_stride + 1] : 1.f,
                        A.sun_d ? A.sun_d[ray * A.sd_stride + 2] : 1.f};
  // upward normal: |sun_z| (spsbrdfnerf.py:260-264); else the sun pass's visibility of the ray's last sample (:354), else 1
  const float irr = (q.cos_irradiance && has_n) ? fabsf(sun[2]) : (q.irr ? q.irr[ray * q.irr_stride] : 1.f);
  D w[3], out[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) w[c] = seed<N>(padded_albedo(acc[c], pad, ws), 3 + c);
  if (KIND == BN_SHADE_LAMBERT) {
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = w[c];
  } else {
    const float *rd = A.rays_d + ray * A.rd_stride;
    const float view[3] = {-rd[0], -rd[1], -rd[2]};
    // the normalisation of the composited normal is differentiated with the rest
    const float *an = acc + q.ch_normal;
    const V3<D> ns = unit_normal<D>({seed<N>(an[0], 0), seed<N>(an[1], 1), seed<N>(an[2], 2)});
    row_brdf<KIND, D>(q, acc, sun, view, ns, w, [](float v_, int slot) { return seed<N>(v_, slot); }, out);
  }
  // rgb = clamp(irradiance * brdf, 0, 1); SNerfLoss = lambda_rgb * mean over (rays, 3) of (rgb - target)^2
  const float invn = 1.f / (3.f * (float)A.R);
  float loss = 0.f, db[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float x = irr * out[c].v;          // (irr == 1 without the cosine term: exact)
    const float y = clamp_(x, 0.f, 1.f);
    const float e = y - A.rgbs[ray * 3 + c];
    loss += q.lambda_rgb * e * e * invn;
    const float dy = (x >= 0.f && x <= 1.f) ? q.lambda_rgb * 2.f * e * invn : 0.f;
    db[c] = dy * irr;
    if (A.rgb) A.rgb[ray * 3 + c] = y;
  }
  float dd, dws = 0.f;
  const float var = A.var ? A.var[ray] : 0.f;
  depth_loss(A.prior, ray, depth, var, q.lambda_ds, q.usealldepth, A.R, loss, dd);
  if (q.lambda_hs > 0.f) {
    // HardSurfaceLoss: lambda/R * sum_s w_s (z_s - depth)^2; the per-sample part of its gradient, lambda/R (z_s - depth)^2,
    // is added by the composite backward (hs_scale); d/d depth = -2 lambda/R (sum_s w_s z_s - depth sum_s w_s)
    const float k = q.lambda_hs / (float)A.R;
    loss += k * var;
    dd += -2.f * k * (depth - depth * ws);
  }
  if (A.extra_loss) loss += A.extra_loss[ray];
  const bool drop = report_ray_loss(true, ray, loss, A.nonfinite, A.ray_loss, A.loss_acc, A.loss_slots);
  // J^T: slots -> composited sums
  float *da = A.d_acc + ray * C;
  for (int c = 0; c < C; ++c) da[c] = 0.f;
  if (drop) { A.d_wsum[ray] = 0.f; A.d_depth[ray] = 0.f; return; }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float dw = jt(out, db, 3 + c);
    da[c] = dw * (1.f + 2.f * pad);
    dws -= dw * pad;
  }
  if (KIND != BN_SHADE_LAMBERT) scatter_jt<KIND, false>(q, out, db, da);
  A.d_wsum[ray] = dws;
  A.d_depth[ray] = dd;
}

}  // namespace

extern "C" int bn_ray_shade_loss(const bn_shade_desc *desc, const float *acc, const float *wsum, const float *depth, const float *var,
                                 const float *rays_d, int64_t rd_stride, const float *sun_d, int64_t sd_stride, const float *rgbs,
                                 const float *valid_depth, int64_t v_stride, const float *target_depth, int64_t td_stride,
                                 const float *target_weight, int64_t tw_stride, const float *target_std, int64_t ts_stride, int64_t R,
                                 float *rgb, float *ray_loss, float *loss_acc, int32_t loss_slots, float *d_acc, float *d_wsum,
                                 float *d_depth, unsigned long long *nonfinite, const float *extra_loss, void *stream) {
  BN_REQUIRE(desc && acc && wsum && depth && rgbs && d_acc && d_wsum && d_depth && R > 0, "ray_shade_loss: null argument");
  const bn_shade_desc &q = *desc;
  if (int e = shade_desc_check(q, rays_d != nullptr, "ray_shade_loss")) return e;
  ShadeArgs a;
  a.prior = DepthPrior{valid_depth, target_depth, target_weight, target_std, v_stride, td_stride, tw_stride, ts_stride};
  if (int e = depth_prior_check(a.prior, var != nullptr, "ray_shade_loss")) return e;
  BN_REQUIRE(!(q.lambda_hs > 0.f) || var, "ray_shade_loss: lambda_hs needs the per-ray variance");
  a.d = q; a.acc = acc; a.wsum = wsum; a.depth = depth; a.var = var; a.rays_d = rays_d; a.sun_d = sun_d; a.rd_stride = rd_stride;
  a.sd_stride = sd_stride; a.rgbs = rgbs; a.R = R; a.rgb = rgb;
  a.ray_loss = ray_loss; a.loss_acc = loss_acc; a.loss_slots = loss_slots > 0 ? loss_slots : 1; a.d_acc = d_acc; a.d_wsum = d_wsum;
  a.d_depth = d_depth; a.nonfinite = nonfinite; a.extra_loss = extra_loss;
  const dim3 grid((unsigned)ceil_div64(R, 64));
  hipStream_t st = (hipStream_t)stream;
  BnProfScope prof_(BN_K_BRDF, st);
  shade_dispatch(q, [&](auto kind, auto) { ray_shade_loss_kernel<decltype(kind)::value><<<grid, 64, 0, st>>>(a); });
  BN_LAUNCH_CHECK("ray_shade_loss");
  return 0;
}
