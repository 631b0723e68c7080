// Volume compositing of one ray (cal_weight, models/spsbrdfnerf.py:50-69), and the ray-level loss terms behind it, each stated once:
//   delta = last ? 1e10 : z[s+1] - z[s];  alpha = 1 - exp(-delta relu(sigma));  u = 1 - alpha + 1e-10;
//   T = exclusive product of u;  w = alpha T
// for composite_kernel, composite_guided_kernel, merged_composite_kernel (render_kernels.hip; one wave per ray) and sun_step
// (sun_shadow.hip; one thread per ray, serial product).  DepthLoss and the non-finite-ray rule serve lambert_loss_kernel, MODE 1
// of the merged kernel and ray_shade_loss_kernel (ray_tail.hip).
// Include it behind the file's `#pragma clang fp contract(off)`: it inherits the contraction setting, and all three files that
// include it have contraction off.  alpha_step holds no multiply-add pair (every product feeds expf, a subtraction's right side
// or a select), so its rounding does not depend on the setting: keep it that way.  depth_loss does hold one.
#pragma once
#include "common.h"

// ------------------------------------------------------------------ wave helpers (64 lanes)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ void lds_wave_sync() {   // LDS hand-over inside one wave: its DS operations execute in order
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ float wave_excl_prod(float v, int lane) {
  // inclusive Hillis-Steele scan, then shift by one lane
  float p = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float t = __shfl_up(p, o);
    if (lane >= o) p *= t;
  }
  const float e = __shfl_up(p, 1);
  return lane == 0 ? 1.f : e;
}
__device__ __forceinline__ float wave_excl_sum_rev(float v, int lane) {
  // exclusive suffix sum: sum of v over lanes > lane
  float p = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float t = __shfl_down(p, o);
    if (lane + o < 64) p += t;
  }
  const float e = __shfl_down(p, 1);
  return lane == 63 ? 0.f : e;
}

// ------------------------------------------------------------------ the alpha step
struct AlphaStep {
  float al, u, dad;   // alpha, 1 - alpha + 1e-10, d alpha / d sigma
};
__device__ __forceinline__ AlphaStep alpha_step(float delta, float sg) {
  const float rs = sg > 0.f ? sg : 0.f;
  const float e = expf(-delta * rs);
  AlphaStep a;
  a.al = 1.f - e;
  a.u = 1.f - a.al + 1e-10f;
  a.dad = sg > 0.f ? delta * e : 0.f;
  return a;
}

// ------------------------------------------------------------------ the lane-owned front of a ray
// One wave per ray.  Lane l owns samples [l cpl, (l+1) cpl), cpl = ceil(S/64) <= BN_MAX_CPL: the exclusive prefix product of u is a
// per-lane serial product + a 6-step wavefront shuffle scan.  Everything is inlined and the arrays live in registers, so a kernel
// that never reads one of them (composite_guided_kernel: dad, tr) does not carry it.
#define BN_MAX_CPL 8   // samples per lane -> S <= 512
// BN_RAY_EACH(F, j, s) { ... }: the lane's samples of RayFront F, ascending: j the slot, s = lane cpl + j the position on the ray
#define BN_RAY_EACH(F, j, s) \
  _Pragma("unroll") for (int j = 0; j < BN_MAX_CPL; ++j) \
    if (const int s = (F).lane * (F).cpl + j; j < (F).cpl && s < (F).S)

struct RayFront {
  int S, cpl, lane;
  float zv[BN_MAX_CPL], al[BN_MAX_CPL], u[BN_MAX_CPL], dad[BN_MAX_CPL], tr[BN_MAX_CPL], w[BN_MAX_CPL];

  __device__ __forceinline__ RayFront(int S_, int lane_) : S(S_), cpl((S_ + 63) / 64), lane(lane_) {}
  // z: the ray's S depths.  sigma_at(j, s): the density of sample s (noise added) - each kernel keeps its own source.
  template <typename F> __device__ __forceinline__ void load(const float *z, F &&sigma_at) {
    float lp = 1.f;
#pragma unroll
    for (int j = 0; j < BN_MAX_CPL; ++j) {
      zv[j] = 0.f; al[j] = 0.f; u[j] = 1.f; dad[j] = 0.f;
      const int s = lane * cpl + j;
      if (j < cpl && s < S) {
        zv[j] = z[s];
        const float delta = s == S - 1 ? 1e10f : z[s + 1] - zv[j];
        const AlphaStep a = alpha_step(delta, sigma_at(j, s));
        al[j] = a.al; u[j] = a.u; dad[j] = a.dad;
        lp *= u[j];
      }
    }
    float T = wave_excl_prod(lp, lane);  // transparency before this lane's first sample
#pragma unroll
    for (int j = 0; j < BN_MAX_CPL; ++j) {
      tr[j] = T;
      w[j] = al[j] * T;
      T *= u[j];
    }
  }
  // the optional per-sample stores (row o = ray S of [R][S] arrays); depth = sum w z and wsum = sum w, in every lane
  __device__ __forceinline__ void store(int64_t o, float *alphas, float *trans, float *weights, float &depth, float &wsum) const {
    float dsum = 0.f, ws = 0.f;
    BN_RAY_EACH(*this, j, s) {
      if (alphas) alphas[o + s] = al[j];
      if (trans) trans[o + s] = tr[j];
      if (weights) weights[o + s] = w[j];
      dsum += w[j] * zv[j];
      ws += w[j];
    }
    depth = wave_sum(dsum);
    wsum = wave_sum(ws);
  }
  // the ray's weights into the wave's LDS slice
  __device__ __forceinline__ void weights_to(float *wl) const {
    BN_RAY_EACH(*this, j, s) wl[s] = w[j];
  }
  // backward: g[j] = dL/dw_s of the lane's samples, gw = sum_j g[j] w[j].  dL/dalpha_s = g_s T_s - (1/u_s) sum_{k>s} g_k w_k
  // (SURVEY.md appendix B), swept in descending s; g[j] becomes dL/dsigma_s.  (In place, not a callable per sample: the row store of
  // the largest merged kernel, handed over as a by-reference lambda, left that kernel's locals in scratch.)
  __device__ __forceinline__ void backward(float (&g)[BN_MAX_CPL], float gw) const {
    float suffix = wave_excl_sum_rev(gw, lane);  // sum of g*w over later lanes
#pragma unroll
    for (int j = BN_MAX_CPL - 1; j >= 0; --j) {
      const int s = lane * cpl + j;
      if (j < cpl && s < S) {
        const float gj = g[j];
        g[j] = (gj * tr[j] - suffix / u[j]) * dad[j];
        suffix += gj * w[j];
      }
    }
  }
};

// ------------------------------------------------------------------ ray-level loss terms
// The SNerfLoss lines in front of these terms are NOT shared, because their clamps differ on a NaN colour x and nobody has decided
// which is right:
//   lambert_loss_kernel     y = fminf(fmaxf(x, 0), 1)                  NaN -> y = 0,   dy = 0
//   merged kernel, MODE 1   y = isnan(x) ? x : fminf(fmaxf(x, 0), 1)   NaN -> y = NaN, dy = NaN
//   ray_shade_loss_kernel   y = clamp_(x, 0, 1) (brdf_eval.h)          NaN -> y = NaN, dy = 0
// Making them agree changes behaviour: a decision for a change of its own.

// The depth prior of a batch: per-ray arrays with element strides (depths[:, 0] of an [R][2] table).  tdepth == nullptr: no prior.
struct DepthPrior {
  const float *valid, *tdepth, *tweight, *tstd;
  int64_t v_stride, td_stride, tw_stride, ts_stride;
};
// complete: what else the entry point needs once a prior is given (ray_shade_loss: the per-ray variance)
static inline int depth_prior_check(const DepthPrior &p, bool complete, const char *what) {
  BN_REQUIRE(!p.tdepth || (p.valid && p.tweight && p.tstd && complete), "%s: incomplete depth prior", what);
  return 0;
}
// DepthLoss (metrics.py:82-161, the subset rule as a mask) of a ray with depth d and depth variance var: adds the ray's term to
// loss and returns d term / d d in dd
__device__ __forceinline__ void depth_loss(const DepthPrior &P, int64_t ray, float d, float var, float lambda_ds, int usealldepth, int64_t R,
                                           float &loss, float &dd) {
  dd = 0.f;
  if (!(P.tdepth && P.valid[ray * P.v_stride] > 0.f)) return;
  const float td = P.tdepth[ray * P.td_stride], tw = P.tweight[ray * P.tw_stride], ts = P.tstd[ray * P.ts_stride];
  const bool apply = usealldepth || (fabsf(d - td) - ts > 0.f) || (ts < sqrtf(var));
  if (apply) {
    const float k = lambda_ds / 3.f / (float)R;
    loss += k * tw * (d - td) * (d - td);
    dd = k * 2.f * tw * (d - td);
  }
}
// A ray whose loss term is not finite (a NaN colour, a BRDF at a singular geometry that the reference's check_nan replacements do
// not cover) makes the reference's loss NaN and its whole gradient with it.  With `nonfinite` (FusedTrainer.sanitize_grads) such
// a ray is left out of the step and counted ([0] NaN, [1] Inf): its loss term becomes 0 and the function returns true - the
// caller zeroes the ray's gradients.  Then the term goes to ray_loss[ray] and / or loss_acc[ray % loss_slots] (spread: same-address
// atomics serialise).  `one`: the lane or thread that reports for the ray.
__device__ __forceinline__ bool report_ray_loss(bool one, int64_t ray, float &loss, unsigned long long *nonfinite, float *ray_loss,
                                                float *loss_acc, int loss_slots) {
  const bool drop = nonfinite && !(fabsf(loss) <= 3.0e38f);
  if (drop) {
    if (one) atomicAdd(nonfinite + (isnan(loss) ? 0 : 1), 1ull);
    loss = 0.f;
  }
  if (one) {
    if (ray_loss) ray_loss[ray] = loss;
    if (loss_acc) atomicAdd(loss_acc + (int)(ray % loss_slots), loss);
  }
  return drop;
}
