// Relighting WITH cast shadows, forward only: the sun-visibility pass of a --sun_v analystic model (rendering.py:244-259,
// models/spsbrdfnerf.py:259-273, 354) under K sun directions from ONE geometry pass.
//
// Per ray only one thing depends on the sun: a sigma-only field pass over G points along the sun ray from the ray's pass-1
// surface point, the transmittance scan of those G densities, and the shading.  bn_field_sigma serves the points; this file
// holds what stands before and behind it:
//
//   bn_sun_ray_table    rays [K R][8] and stratified depths [K R][G] of the sun pass for K directions in one launch - bitwise
//                       rendering.sun_far + bn_stratified_z + the torch.cat of rendering._sample_passes, per direction
//   bn_sun_shade_dirs   transmittance T_s = prod_{j<s} (1 - alpha_j + 1e-10) of every (direction, ray) and the shading that reads
//                       it, fused: alphas, weights and transparencies are never materialised.  Replaces, per direction,
//                       bn_composite_forward on the sun pass + the ray-level statement of shade() (models/spsbrdfnerf.py:265-273,
//                       350-354) in torch.
//
// bn_sun_shade_dirs reads 8 bytes per (direction, ray, sample) - sigma and z - and is bound by them.  A lane owns a ray, and a
// lane that read its own [G] row would stride the wave across G * 4 bytes per load.  So the 64 rays of a block take their rows
// through LDS: the block's rows of one direction are ONE contiguous piece of sigma_sun / z_sun, the wave loads it with consecutive
// lanes on consecutive words, SC samples of every ray at a time (+ 1 depth, for the last delta of the piece), into rows padded to
// SC + 1 words (lane l then reads word l * (SC + 1) + t: no bank conflict).  Every (direction, ray) is a serial computation of
// its own lane, in ascending s: no value depends on the direction tile, the grid or the other rays of the launch.
#include "common.h"
#include "brdfnerf_hip.h"
#include "prof.h"
// (no FMA contraction: the table must round like the separate ATen operations it replaces, the shading like relight.hip)
#pragma clang fp contract(off)
#include "brdf_eval.h"
#include "shade_row.h"
#include "composite_ray.h"

namespace {

// torch.linspace(start, end, steps)[i] in fp32, as in render_kernels.hip
__device__ __forceinline__ float sun_linspace_at(float start, float end, int steps, int i) {
  const float step = (end - start) / (float)(steps - 1);
  return i < steps / 2 ? start + step * (float)i : end - step * (float)(steps - i - 1);
}

// One thread per depth: i = (k R + r) G + s.  The 8 columns of row (k, r) are written by its first threads (column c by thread
// s = c mod G, so G < 8 is served too).
__global__ __launch_bounds__(256)
void sun_ray_table_kernel(const float *__restrict__ rays, int64_t ray_stride, const float *__restrict__ d1, const float *__restrict__ sun,
                          const float *__restrict__ u, int64_t R, int K, int G, float *__restrict__ table, float *__restrict__ z) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)K * R * G) return;
  const int64_t kr = i / G;
  const int s = (int)(i - kr * G);
  const int64_t k = kr / R, r = kr - k * R;
  const float *sk = sun + k * 3;
  // far = |d_z / sun_z| of ROW 0 times the pass-1 depth (rendering.sun_far; the reference's quirk), near = 0.01 far
  const float s0 = sk[2], r0 = rays[5];
  const float ratio = fabsf(s0) > 0.00001f ? fabsf(r0 / s0) : 1.f;
  const float dep = d1[r];
  const float f = ratio * dep;
  const float n = f * 0.01f;
  auto zc = [&](int j) {
    const float t = sun_linspace_at(0.f, 1.f, G, j);
    return n * (1.f - t) + f * t;
  };
  const float zi = zc(s);
  const float lower = s == 0 ? zi : 0.5f * (zc(s - 1) + zi);
  const float upper = s == G - 1 ? zi : 0.5f * (zi + zc(s + 1));
  z[i] = lower + (upper - lower) * u[r * G + s];
  const float *ray = rays + r * ray_stride;
  for (int c = s; c < 8; c += G) {
    float v;
    if (c < 3) v = ray[c] + ray[3 + c] * dep;        // the pass-1 surface point o + d * depth
    else if (c < 6) v = sk[c - 3];
    else v = c == 6 ? n : f;
    table[kr * 8 + c] = v;
  }
}

struct SunShadeArgs {
  bn_shade_desc d;
  const float *sigma, *z, *noise, *acc, *wsum, *X, *w, *rays_d;
  float noise_std;
  int64_t rd_stride, R, rgb_plane, vis_plane;
  int32_t G, K, ktile;
};

// directions a block of the per-sample mode walks together: a sample's row is read and unpacked once for all of them
constexpr int SUN_KT = 4;

// 1 - alpha + 1e-10 of one sample: the alpha step of the compositing kernels (composite_ray.h)
__device__ __forceinline__ float sun_step(const float *zr, const float *sr, int t, bool last) {
  return alpha_step(last ? 1e10f : zr[t + 1] - zr[t], sr[t]).u;
}

// KIND / MASK: shade_row.h.  SAMPLES false: one BRDF per ray from the composited sums, rgb = clamp(T_{G-1} BRDF); true: the
// view ray's own rows X [R][G][C] and weights w [R][G], rgb = clamp(sum_s w_s (c_s (1 + 2 pad) - pad) T_s) with c_s the row's
// albedo (LAMBERT) or its BRDF, one fp32 accumulator per channel fed in ascending s.
template <int KIND, int MASK, bool SAMPLES> __global__ __launch_bounds__(64)
void sun_shade_dirs_kernel(const SunShadeArgs A, const float *__restrict__ sun, float *__restrict__ rgb_out, float *__restrict__ vis_out) {
  constexpr int KT = SAMPLES ? SUN_KT : 1;
  constexpr int SC = SAMPLES ? 16 : 32;
  constexpr int LD = SC + 1;
  __shared__ float s_sg[KT][64 * LD];
  __shared__ float s_z[KT][64 * LD];
  const int lane = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  const int nr = (int)(A.R - r0 < 64 ? A.R - r0 : 64);     // rays of this block
  const bool live = lane < nr;
  const int64_t ray = live ? r0 + lane : r0;               // (a lane without a ray walks the block's first: it stores nothing)
  const bn_shade_desc &q = A.d;
  const int G = A.G, C = q.C;
  const float pad = q.rgb_padding, gain = 1.f + 2.f * pad;
  V3<float> vray = {0.f, 0.f, 1.f};
  if (KIND != BN_SHADE_LAMBERT) {
    const float *rd = A.rays_d + ray * A.rd_stride;
    vray = {-rd[0], -rd[1], -rd[2]};
  }
  // ---- per ray: the row of the composited sums, once (relight.hip ray_shade_dirs_kernel)
  float wa[3] = {0.f, 0.f, 0.f};
  V3<float> nsa = {0.f, 0.f, 1.f};
  float q0[3] = {0.f, 0.f, 0.f}, q1[3] = {0.f, 0.f, 0.f}, q2[3] = {0.f, 0.f, 0.f};
  if (!SAMPLES) {
    const float *acc = A.acc + ray * C;
    const float ws = A.wsum[ray];
#pragma unroll
    for (int c = 0; c < 3; ++c) wa[c] = padded_albedo(acc[c], pad, ws);
    const float *an = acc + q.ch_normal;
    nsa = unit_normal<float>({an[0], an[1], an[2]});
    row_params<KIND, MASK>(q, acc, wa, q0, q1, q2);
  }
  const float *zr = nullptr, *sr = nullptr;
  const int kbeg = (int)blockIdx.y * A.ktile;
  const int kend = min(A.K, kbeg + A.ktile);
  for (int kb = kbeg; kb < kend; kb += KT) {
    const int nk = min(KT, kend - kb);                       // directions of this trip, the same in every lane
    // per direction: T_s so far, T_{G-1}, the three sums.  Indexed by constants only: the direction loop below stays rolled and
    // rotates the file by one place per trip, as relight.hip's sample_shade_dirs_kernel does.
    float st[KT][5];
#pragma unroll
    for (int j = 0; j < KT; ++j) {
      st[j][0] = st[j][1] = 1.f;
      st[j][2] = st[j][3] = st[j][4] = 0.f;
    }
    for (int s0 = 0; s0 < G; s0 += SC) {
      const int n = min(SC, G - s0);
      __syncthreads();                                       // the piece before this one has been consumed
      for (int j = 0; j < nk; ++j) {
        const int64_t base = ((int64_t)(kb + j) * A.R + r0) * G;
        for (int idx = lane; idx < 64 * LD; idx += 64) {
          const int rj = idx / LD, t = idx - rj * LD, s = s0 + t;
          float zv = 0.f, sg = 0.f;
          if (rj < nr && t <= n && s < G) {                  // t == n: the depth behind the piece, for its last delta
            const int64_t o = base + (int64_t)rj * G + s;
            zv = A.z[o];
            if (t < n) {
              sg = A.sigma[o];
              if (A.noise) sg = sg + A.noise[(r0 + rj) * G + s] * A.noise_std;
            }
          }
          s_z[j][idx] = zv;
          s_sg[j][idx] = sg;
        }
      }
      __syncthreads();
      if (!SAMPLES) {
        zr = s_z[0] + lane * LD;
        sr = s_sg[0] + lane * LD;
        for (int t = 0; t < n; ++t) {
          const bool last = s0 + t == G - 1;
          const float u = sun_step(zr, sr, t, last);
          if (last) st[0][1] = st[0][0];
          st[0][0] = st[0][0] * u;
        }
      } else {
        for (int t = 0; t < n; ++t) {
          const int s = s0 + t;
          const bool last = s == G - 1;
          const float *x = A.X + (ray * G + s) * C;
          const float ws = A.w[ray * G + s];
          float w[3] = {x[0], x[1], x[2]};
          V3<float> ns = {0.f, 0.f, 1.f};
          float p0[3] = {0.f, 0.f, 0.f}, p1[3] = {0.f, 0.f, 0.f}, p2[3] = {0.f, 0.f, 0.f};
          if (KIND != BN_SHADE_LAMBERT) {
            ns = {x[q.ch_normal], x[q.ch_normal + 1], x[q.ch_normal + 2]};
            row_params<KIND, MASK>(q, x, w, p0, p1, p2);
          }
#pragma nounroll
          for (int j = 0; j < KT; ++j) {
            float T = st[0][0], Tl = st[0][1], a0 = st[0][2], a1 = st[0][3], a2 = st[0][4];
            if (j < nk) {
              const float u = sun_step(s_z[j] + lane * LD, s_sg[j] + lane * LD, t, last);
              float out[3];
              V3<float> l = {0.f, 0.f, 1.f};
              if (KIND != BN_SHADE_LAMBERT) {
                const float *sk = sun + (int64_t)(kb + j) * 3;
                l = {sk[0], sk[1], sk[2]};
              }
              brdf_value<KIND, MASK>(q, l, vray, ns, w, p0, p1, p2, out);
              // (w (c (1 + 2 pad) - pad)) T, the reference's order (:270-273, :350-352)
              a0 = a0 + ws * (out[0] * gain - pad) * T;
              a1 = a1 + ws * (out[1] * gain - pad) * T;
              a2 = a2 + ws * (out[2] * gain - pad) * T;
              if (last) Tl = T;
              T = T * u;
            }
#pragma unroll
            for (int i = 0; i + 1 < KT; ++i)
#pragma unroll
              for (int c = 0; c < 5; ++c) st[i][c] = st[i + 1][c];
            st[KT - 1][0] = T; st[KT - 1][1] = Tl; st[KT - 1][2] = a0; st[KT - 1][3] = a1; st[KT - 1][4] = a2;
          }
        }
      }
    }
    if (!SAMPLES) {
      // irradiance of the LAST sample times the ray's BRDF (models/spsbrdfnerf.py:354)
      const float *sk = sun + (int64_t)kb * 3;
      const V3<float> l = {sk[0], sk[1], sk[2]};
      float out[3];
      brdf_value<KIND, MASK>(q, l, vray, nsa, wa, q0, q1, q2, out);
#pragma unroll
      for (int c = 0; c < 3; ++c) st[0][2 + c] = st[0][1] * out[c];
    }
    if (live) {
#pragma unroll
      for (int j = 0; j < KT; ++j) {
        if (j < nk) {
          float *rgb = rgb_out + (int64_t)(kb + j) * A.rgb_plane + ray * 3;
#pragma unroll
          for (int c = 0; c < 3; ++c) rgb[c] = clamp_(st[j][2 + c], 0.f, 1.f);
          if (vis_out) vis_out[(int64_t)(kb + j) * A.vis_plane + ray] = st[j][1];
        }
      }
    }
  }
}

}  // namespace

extern "C" int bn_sun_ray_table(const float *rays, int64_t ray_stride, const float *d1, const float *sun, const float *u, int64_t R,
                                int32_t K, int32_t G, float *table, float *z_sun, void *stream) {
  BN_REQUIRE(rays && d1 && sun && u && table && z_sun && R > 0 && K > 0, "sun_ray_table: null argument");
  BN_REQUIRE(ray_stride >= 6, "sun_ray_table: ray_stride=%lld < 6 (origin and direction)", (long long)ray_stride);
  BN_REQUIRE(G >= 2 && G <= BN_MAX_G, "sun_ray_table: G=%d unsupported", G);
  const int64_t n = (int64_t)K * R * G;
  BN_REQUIRE(ceil_div64(n, 256) <= 0x7fffffff, "sun_ray_table: K R G = %lld too large", (long long)n);
  hipStream_t st = (hipStream_t)stream;
  BnProfScope prof_(BN_K_STRATIFIED, st);
  sun_ray_table_kernel<<<dim3((unsigned)ceil_div64(n, 256)), 256, 0, st>>>(rays, ray_stride, d1, sun, u, R, K, G, table, z_sun);
  BN_LAUNCH_CHECK("sun_ray_table");
  return 0;
}

extern "C" int bn_sun_shade_dirs(const bn_shade_desc *desc, const float *sigma_sun, const float *z_sun, const float *noise, float noise_std,
                                 const float *acc, const float *wsum, const float *X, const float *w, const float *rays_d,
                                 int64_t rd_stride, const float *sun, int64_t R, int32_t G, int32_t K, float *rgb, int64_t rgb_plane,
                                 float *vis, int64_t vis_plane, void *stream) {
  BN_REQUIRE(desc && sigma_sun && z_sun && sun && rgb && R > 0 && K > 0, "sun_shade_dirs: null argument");
  const bn_shade_desc &q = *desc;
  if (int e = shade_desc_check(q, rays_d != nullptr, "sun_shade_dirs")) return e;
  BN_REQUIRE(!q.irr, "sun_shade_dirs: the descriptor carries a sun-pass irradiance (this call computes it per direction)");
  BN_REQUIRE(G >= 3 && G <= BN_MAX_G, "sun_shade_dirs: G=%d outside [3, %d]", G, BN_MAX_G);
  BN_REQUIRE(!(q.cos_irradiance && q.ch_normal >= 0), "sun_shade_dirs: cos_irradiance with a normal channel - the cosine branch wins and "
             "the sun pass is unused (models/spsbrdfnerf.py:260-266): bn_ray_shade_dirs / bn_sample_shade_dirs");
  BN_REQUIRE((acc != nullptr) != (X != nullptr), "sun_shade_dirs: give either the composited sums (acc, wsum) or the rows (X, w), not %s",
             acc ? "both" : "neither");
  const bool samples = X != nullptr;
  BN_REQUIRE(samples ? w != nullptr : wsum != nullptr, "sun_shade_dirs: %s", samples ? "rows without their weights w" : "acc without wsum");
  BN_REQUIRE(samples || q.kind != BN_SHADE_LAMBERT, "sun_shade_dirs: a Lambertian colour under per-sample irradiance is a sum over the "
             "samples (models/spsbrdfnerf.py:265-273): give the rows X, w");
  BN_REQUIRE(R <= (int64_t)64 * 0x7fffffff, "sun_shade_dirs: R=%lld too large", (long long)R);
  BN_REQUIRE(rgb_plane >= R * 3 && (!vis || vis_plane >= R), "sun_shade_dirs: planes (%lld, %lld) shorter than R * 3 = %lld, R = %lld",
             (long long)rgb_plane, (long long)vis_plane, (long long)(R * 3), (long long)R);
  SunShadeArgs a;
  a.d = q; a.sigma = sigma_sun; a.z = z_sun; a.noise = (noise && noise_std != 0.f) ? noise : nullptr; a.noise_std = noise_std;
  a.acc = acc; a.wsum = wsum; a.X = X; a.w = w; a.rays_d = rays_d; a.rd_stride = rd_stride; a.R = R; a.rgb_plane = rgb_plane;
  a.vis_plane = vis_plane; a.G = G; a.K = K;
  // a block walks its tile one trip after the other (the per-ray mode prepares its row once for all of them)
  const int64_t blocks = ceil_div64(R, 64);
  const int64_t kt = dir_tile(K, blocks, 8, samples ? SUN_KT : 1);
  a.ktile = (int32_t)kt;
  const dim3 grid((unsigned)blocks, (unsigned)ceil_div64(K, kt));
  hipStream_t st = (hipStream_t)stream;
  BnProfScope prof_(BN_K_BRDF, st);
  shade_dispatch(q, [&](auto kind, auto mask) {
    constexpr int KIND = decltype(kind)::value, MASK = decltype(mask)::value;
    if (samples) sun_shade_dirs_kernel<KIND, MASK, true><<<grid, 64, 0, st>>>(a, sun, rgb, vis);
    else if constexpr (KIND != BN_SHADE_LAMBERT) sun_shade_dirs_kernel<KIND, MASK, false><<<grid, 64, 0, st>>>(a, sun, rgb, vis);   // (refused above)
  });
  BN_LAUNCH_CHECK("sun_shade_dirs");
  return 0;
}
