// Ray-level shading of ONE set of composited sums under MANY sun / view directions, forward only: relighting a rendered view and
// the BRDF lobe of a pixel without another field pass.
//
// With one BRDF per ray (MultiBRDF == 0) and no sun-visibility pass the colour of a ray is a function of the composited sums
// acc [R][C], wsum [R], the view direction and the sun direction (ray_tail.hip; models/spsbrdfnerf.py:259-357), and none of the
// sums depends on the sun.  K directions therefore cost one geometry pass and this kernel: a lane owns one ray, prepares its row
// once (composited albedo, normalised composited normal, BRDF parameters) and walks a tile of directions.  The directions are
// the same for every lane of a wave: inside the loop they are read with s_load_dwordx2 + s_load_dword into SGPRs (the direction and
// output pointers are __restrict__ kernel parameters, see the kernel) and cost no vector registers or vector-memory waits.  The stores
// to rgb[k][ray][0:3] are contiguous across the lanes of a wave (768 B per direction).  Grid = ray blocks x direction tiles.
// Replaces eval.py's eval_pixel_variedvw / get_view_dirs loop and create_dsm.py:44-77 (rays[:, 8:11] = sun, render again).
//
// With one BRDF per SAMPLE (MultiBRDF == 1; models/spsbrdfnerf.py:289-307, 350-352) the same holds one level down: the colour is
// sum_s w_s (brdf(row_s, sun, view) (1 + 2 pad) - pad) irr, and neither the depth-sorted rows nor their weights depend on the sun.
// sample_shade_dirs_kernel (second half of this file) walks a ray's samples once per direction tile and keeps the tile's sums in
// registers: one geometry pass + R S K pointwise BRDF evaluations instead of K field passes.
#include "common.h"
#include "brdfnerf_hip.h"
#include "prof.h"
// (no FMA contraction, like brdf.hip and ray_tail.hip: one direction must round like bn_ray_shade_loss)
#pragma clang fp contract(off)
#include "brdf_eval.h"
#include "shade_row.h"

namespace {

struct RelightArgs {
  bn_shade_desc d;
  const float *acc, *wsum, *rays_d;
  int64_t rd_stride;
  int64_t R;
  int32_t K, ktile;
};

// KIND / MASK: shade_row.h.
// sun / view [K][3] (view nullptr: -rays_d of the ray, sun mode; else the lobe's view directions) and rgb / brdf [K][R][3] (brdf
// nullable) are kernel parameters of their own, __restrict__: only then can the compiler know that the stores of the direction loop
// do not touch the directions, and read sun[k] / view[k] through the scalar cache.
template <int KIND, int MASK> __global__ __launch_bounds__(64)
void ray_shade_dirs_kernel(const RelightArgs A, const float *__restrict__ sun, const float *__restrict__ view, float *__restrict__ rgb_out,
                           float *__restrict__ brdf_out) {
  const int64_t ray = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (ray >= A.R) return;
  const bn_shade_desc &q = A.d;
  const float *acc = A.acc + ray * q.C;
  const float ws = A.wsum[ray];
  const float pad = q.rgb_padding;
  const bool has_n = q.ch_normal >= 0;
  // ---- the ray's row, once
  float w[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) w[c] = padded_albedo(acc[c], pad, ws);
  V3<float> ns = {0.f, 0.f, 1.f}, vray = {0.f, 0.f, 1.f};
  float p0[3] = {0.f, 0.f, 0.f}, p1[3] = {0.f, 0.f, 0.f}, p2[3] = {0.f, 0.f, 0.f};
  if (KIND != BN_SHADE_LAMBERT) {
    const float *an = acc + q.ch_normal;
    ns = unit_normal<float>({an[0], an[1], an[2]});
    if (!view) {
      const float *rd = A.rays_d + ray * A.rd_stride;
      vray = {-rd[0], -rd[1], -rd[2]};
    }
    row_params<KIND, MASK>(q, acc, w, p0, p1, p2);
  }
  // ---- the tile of directions: k is the same in every lane, sun[k] / view[k] come through the scalar cache
  const int k0 = (int)blockIdx.y * A.ktile;
  const int k1 = min(A.K, k0 + A.ktile);
  const int64_t plane = A.R * 3;
  for (int k = k0; k < k1; ++k) {
    const float *sk = sun + (int64_t)k * 3;
    const V3<float> l = {sk[0], sk[1], sk[2]};
    V3<float> v = vray;
    if (view) {
      const float *vk = view + (int64_t)k * 3;
      v = {vk[0], vk[1], vk[2]};
    }
    // upward normal: |sun_z| (spsbrdfnerf.py:260-264), else 1
    const float irr = (q.cos_irradiance && has_n) ? fabsf(l.z) : 1.f;
    float out[3];
    brdf_value<KIND, MASK>(q, l, v, ns, w, p0, p1, p2, out);
    float *rgb = rgb_out + (int64_t)k * plane + ray * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[c] = clamp_(irr * out[c], 0.f, 1.f);            // (irr == 1 without the cosine term: exact)
    if (brdf_out) {
      float *b = brdf_out + (int64_t)k * plane + ray * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) b[c] = out[c];
    }
  }
}

// ------------------------------------------------------------------ one BRDF per sample (MultiBRDF): X [R][S][C], w [R][S]
struct SampleDirsArgs {
  bn_shade_desc d;
  const float *X, *w, *rays_d;
  int64_t rd_stride;
  int64_t R, rgb_plane, brdf_plane;
  int32_t S, K, ktile;
};

// directions of a tile at most: 6 accumulators each (rgb and brdf sums) stay in registers next to the BRDF body's own
constexpr int SAMPLE_KT = 8;

// A lane owns a ray.  Outer loop: the ray's samples in ascending s, each row loaded and unpacked ONCE - the raw normal, the raw
// albedo and the parameter channels, what sample_brdf.hip hands to the same *_eval bodies.  Inner loop: the tile's
// directions (wave-uniform, through the scalar cache as above).  Every (ray, direction, channel) has one fp32 accumulator that
// takes its terms in ascending s - no atomics, no cross-lane step - so a result's bits depend on nothing but its own ray and
// direction: not on the tile, the ray block, K or the caller's chunking.  No sample is skipped: 0 * inf stays the NaN of the
// reference's sum.
// The accumulators are indexed by constants only: the direction loop stays ROLLED (one BRDF body per kernel) and rotates the
// accumulator file by one place per trip - the current direction's sums are always in place 0, and after SAMPLE_KT trips every
// sum is back where it started.  Trips beyond the tile's n directions (a wave-uniform test) only rotate.
template <int KIND, int MASK> __global__ __launch_bounds__(64)
void sample_shade_dirs_kernel(const SampleDirsArgs A, const float *__restrict__ sun, const float *__restrict__ view,
                              float *__restrict__ rgb_out, float *__restrict__ brdf_out) {
  const int64_t ray = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (ray >= A.R) return;
  const bn_shade_desc &q = A.d;
  const int C = q.C;
  const float pad = q.rgb_padding, gain = 1.f + 2.f * pad;
  const bool cosi = q.cos_irradiance && q.ch_normal >= 0;
  V3<float> vray = {0.f, 0.f, 1.f};
  if (!view) {
    const float *rd = A.rays_d + ray * A.rd_stride;
    vray = {-rd[0], -rd[1], -rd[2]};
  }
  const int k0 = (int)blockIdx.y * A.ktile;
  const int n = min(A.K - k0, A.ktile);                    // 1 <= n <= SAMPLE_KT, the same in every lane
  float ar[SAMPLE_KT][3], ab[SAMPLE_KT][3];                // sum_s w bp irr ; sum_s w brdf
#pragma unroll
  for (int j = 0; j < SAMPLE_KT; ++j)
#pragma unroll
    for (int c = 0; c < 3; ++c) ar[j][c] = ab[j][c] = 0.f;
  const float *x = A.X + ray * A.S * C;
  const float *wr = A.w + ray * A.S;
  for (int s = 0; s < A.S; ++s, x += C) {
    const float ws = wr[s];
    const V3<float> ns = {x[q.ch_normal], x[q.ch_normal + 1], x[q.ch_normal + 2]};
    float w[3] = {x[0], x[1], x[2]};
    float p0[3] = {0.f, 0.f, 0.f}, p1[3] = {0.f, 0.f, 0.f}, p2[3] = {0.f, 0.f, 0.f};
    row_params<KIND, MASK>(q, x, w, p0, p1, p2);
#pragma nounroll
    for (int j = 0; j < SAMPLE_KT; ++j) {
      float r0 = ar[0][0], r1 = ar[0][1], r2 = ar[0][2], b0 = ab[0][0], b1 = ab[0][1], b2 = ab[0][2];
      if (j < n) {
        const float *sk = sun + (int64_t)(k0 + j) * 3;
        const V3<float> l = {sk[0], sk[1], sk[2]};
        V3<float> v = vray;
        if (view) {
          const float *vk = view + (int64_t)(k0 + j) * 3;
          v = {vk[0], vk[1], vk[2]};
        }
        const float irr = cosi ? fabsf(l.z) : 1.f;           // upward normal: |sun_z| (spsbrdfnerf.py:260-264), else 1
        float out[3];
        brdf_value<KIND, MASK>(q, l, v, ns, w, p0, p1, p2, out);
        // (w bp) irr, the reference's order (:350-352); irr == 1 without the cosine term: exact
        r0 = r0 + ws * (out[0] * gain - pad) * irr;
        r1 = r1 + ws * (out[1] * gain - pad) * irr;
        r2 = r2 + ws * (out[2] * gain - pad) * irr;
        b0 = b0 + ws * out[0];
        b1 = b1 + ws * out[1];
        b2 = b2 + ws * out[2];
      }
#pragma unroll
      for (int i = 0; i + 1 < SAMPLE_KT; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          ar[i][c] = ar[i + 1][c];
          ab[i][c] = ab[i + 1][c];
        }
      ar[SAMPLE_KT - 1][0] = r0; ar[SAMPLE_KT - 1][1] = r1; ar[SAMPLE_KT - 1][2] = r2;
      ab[SAMPLE_KT - 1][0] = b0; ab[SAMPLE_KT - 1][1] = b1; ab[SAMPLE_KT - 1][2] = b2;
    }
  }
#pragma unroll
  for (int j = 0; j < SAMPLE_KT; ++j) {
    if (j < n) {
      float *rgb = rgb_out + (int64_t)(k0 + j) * A.rgb_plane + ray * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) rgb[c] = clamp_(ar[j][c], 0.f, 1.f);
      if (brdf_out) {
        float *b = brdf_out + (int64_t)(k0 + j) * A.brdf_plane + ray * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) b[c] = ab[j][c];
      }
    }
  }
}

}  // namespace

extern "C" int bn_ray_shade_dirs(const bn_shade_desc *desc, const float *acc, const float *wsum, const float *rays_d,
                                 int64_t rd_stride, const float *sun, const float *view, int64_t R, int32_t K, float *rgb,
                                 float *brdf, void *stream) {
  BN_REQUIRE(desc && acc && wsum && sun && rgb && R > 0 && K > 0, "ray_shade_dirs: null argument");
  const bn_shade_desc &q = *desc;
  if (int e = shade_desc_check(q, rays_d || view, "ray_shade_dirs")) return e;
  BN_REQUIRE(!q.irr, "ray_shade_dirs: a per-ray irradiance of the sun pass depends on the sun direction (not relightable)");
  BN_REQUIRE(R <= (int64_t)64 * 0x7fffffff, "ray_shade_dirs: R=%lld too large", (long long)R);
  RelightArgs a;
  a.d = q; a.acc = acc; a.wsum = wsum; a.rays_d = rays_d; a.rd_stride = rd_stride; a.R = R; a.K = K;
  // an image has thousands of ray blocks and takes all its directions in one tile (up to 32), a lobe has one ray block and tens of
  // thousands of directions
  const int64_t blocks = ceil_div64(R, 64);
  const int64_t kt = dir_tile(K, blocks, 32, 1);
  a.ktile = (int32_t)kt;
  const dim3 grid((unsigned)blocks, (unsigned)ceil_div64(K, kt));
  hipStream_t st = (hipStream_t)stream;
  BnProfScope prof_(BN_K_BRDF, st);
  shade_dispatch(q, [&](auto kind, auto mask) {
    ray_shade_dirs_kernel<decltype(kind)::value, decltype(mask)::value><<<grid, 64, 0, st>>>(a, sun, view, rgb, brdf);
  });
  BN_LAUNCH_CHECK("ray_shade_dirs");
  return 0;
}

extern "C" int bn_sample_shade_dirs(const bn_shade_desc *desc, const float *X, const float *w, const float *rays_d, int64_t rd_stride,
                                    const float *sun, const float *view, int64_t R, int32_t S, int32_t K, float *rgb, int64_t rgb_plane,
                                    float *brdf, int64_t brdf_plane, void *stream) {
  BN_REQUIRE(desc && X && w && sun && rgb && R > 0 && S > 0 && K > 0, "sample_shade_dirs: null argument");
  const bn_shade_desc &q = *desc;
  BN_REQUIRE(q.kind > BN_SHADE_LAMBERT && q.kind <= BN_SHADE_MICROFACET,
             "sample_shade_dirs: kind=%d (a Lambertian colour is a function of the composited sums: bn_ray_shade_dirs)", q.kind);
  if (int e = shade_desc_check(q, rays_d || view, "sample_shade_dirs")) return e;
  BN_REQUIRE(!q.irr, "sample_shade_dirs: an irradiance of the sun pass depends on the sun direction (not relightable)");
  BN_REQUIRE(R <= (int64_t)64 * 0x7fffffff, "sample_shade_dirs: R=%lld too large", (long long)R);
  BN_REQUIRE(rgb_plane >= R * 3 && (!brdf || brdf_plane >= R * 3), "sample_shade_dirs: planes (%lld, %lld) shorter than R * 3 = %lld",
             (long long)rgb_plane, (long long)brdf_plane, (long long)(R * 3));
  SampleDirsArgs a;
  a.d = q; a.X = X; a.w = w; a.rays_d = rays_d; a.rd_stride = rd_stride; a.R = R; a.rgb_plane = rgb_plane; a.brdf_plane = brdf_plane;
  a.S = S;
  // The tile is capped by the accumulators, so gridDim.y <= 65535 cannot be met by a longer tile: more directions than a grid of
  // full tiles holds take more launches (and the tile is that of such a grid)
  const int64_t blocks = ceil_div64(R, 64);
  const int64_t grid_k = (int64_t)65535 * SAMPLE_KT;
  const int64_t kt = dir_tile(K < grid_k ? K : grid_k, blocks, SAMPLE_KT, 1);
  a.ktile = (int32_t)kt;
  hipStream_t st = (hipStream_t)stream;
  BnProfScope prof_(BN_K_BRDF, st);
  const int64_t per_launch = 65535 * kt;
  for (int64_t kb = 0; kb < K; kb += per_launch) {
    a.K = (int32_t)(K - kb < per_launch ? K - kb : per_launch);
    const dim3 grid((unsigned)blocks, (unsigned)ceil_div64(a.K, kt));
    const float *sun_b = sun + kb * 3, *view_b = view ? view + kb * 3 : nullptr;
    float *rgb_b = rgb + kb * rgb_plane, *brdf_b = brdf ? brdf + kb * brdf_plane : nullptr;
    shade_dispatch(q, [&](auto kind, auto mask) {
      if constexpr (decltype(kind)::value != BN_SHADE_LAMBERT)         // (refused above)
        sample_shade_dirs_kernel<decltype(kind)::value, decltype(mask)::value><<<grid, 64, 0, st>>>(a, sun_b, view_b, rgb_b, brdf_b);
    });
  }
  BN_LAUNCH_CHECK("sample_shade_dirs");
  return 0;
}
