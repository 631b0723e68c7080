// NormalLoss against per-ray TARGET normals (metrics.py:218-261, keywords 'an' / 'lr' = --nr_spv_type 3 / 2, main.py:310-322) of the
// fused training step: the composited normal acc[r][ch : ch + 3] of the rays with a depth prior is pulled towards the tie-point
// normal of the ray, an L1 mean over the selected rays weighted by valid_normal.  One ABI entry, two launches: a one-workgroup
// integer count of the selected rays, then one lane per ray for the term and its gradient, which is ADDED to the d_acc that
// bn_ray_shade_loss wrote.  The rule is stated in include/brdfnerf_hip.h.
// Replaces, for the training step: NormalLoss.calc_subset_normal_loss (metrics.py:232-243: three np.where(valid.cpu() > 0), a
// device -> host copy each), torch's L1Loss and their autograd graph.
#include "common.h"
#include "brdfnerf_hip.h"
// (no FMA contraction, like ray_tail.hip: every operation of the stated rule rounds on its own)
#pragma clang fp contract(off)

namespace {

struct TargetArgs {
  const float *acc, *normals, *valid_normal, *valid_depth;
  int64_t n_stride, vn_stride, vd_stride, R;
  int C, ch;
  float lambda;
  float *d_acc, *ray_loss, *loss_acc;
  int loss_slots;
  unsigned long long *nonfinite;
  long long *count;
};

// n_sel = #{r : valid_depth[r] > 0} (NaN does not count).  One workgroup: thread t takes rays t, t + 1024, ..., then a binary tree
// over the threads; an integer, so no order changes a bit.  count[0] is WRITTEN: nothing to zero before a graph replay.
__global__ __launch_bounds__(1024) void normal_target_count_kernel(const float *valid_depth, int64_t vd_stride, int64_t R, long long *count) {
  __shared__ int sn[1024];
  int n = 0;                                               // R <= 2^30: fits
  for (int64_t r = threadIdx.x; r < R; r += 1024) n += valid_depth[r * vd_stride] > 0.f ? 1 : 0;
  sn[threadIdx.x] = n;
  __syncthreads();
  for (int o = 512; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) sn[threadIdx.x] += sn[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) count[0] = (long long)sn[0];
}

__global__ __launch_bounds__(256) void normal_target_ray_kernel(const TargetArgs A) {
  const int64_t ray = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (ray >= A.R) return;
  const long long n_sel = A.count[0];
  if (n_sel <= 0) return;                                  // an empty selection adds nothing anywhere
  if (!(A.valid_depth[ray * A.vd_stride] > 0.f)) return;   // (NaN: not selected)
  const float k = A.lambda / (3.f * (float)n_sel);
  const float vn = A.valid_normal[ray * A.vn_stride];
  const float *gt = A.normals + ray * A.n_stride;
  float *da = A.d_acc + ray * A.C + A.ch;
  const float *an = A.acc + ray * A.C + A.ch;
  float e[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float a = vn * gt[c], b = vn * an[c];
    e[c] = a - b;
  }
  const float term = k * ((fabsf(e[0]) + fabsf(e[1])) + fabsf(e[2]));
  // a ray whose term is not finite: with `nonfinite` it is left out and counted ([0] NaN, [1] Inf); without, the NaN / Inf reaches the
  // loss as it does upstream and the gradient follows the comparisons below
  if (A.nonfinite && !(fabsf(term) <= 3.0e38f)) {
    atomicAdd(A.nonfinite + (isnan(term) ? 0 : 1), 1ull);
    return;
  }
  const float kv = k * vn;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    // d |e| / d acc = -vn sign(e); sign by comparison: 0 at e == 0 and at a NaN e, as torch's L1 backward
    const float s = e[c] > 0.f ? -1.f : (e[c] < 0.f ? 1.f : 0.f);
    da[c] += kv * s;
  }
  if (A.ray_loss) A.ray_loss[ray] += term;
  if (A.loss_acc) atomicAdd(A.loss_acc + (int)(ray % A.loss_slots), term);
}

}  // namespace

extern "C" int bn_normal_target_loss(const float *acc, int32_t C, int32_t ch, const float *normals, int64_t n_stride,
                                     const float *valid_normal, int64_t vn_stride, const float *valid_depth, int64_t vd_stride,
                                     float lambda, int64_t R, float *d_acc, float *ray_loss, float *loss_acc, int32_t loss_slots,
                                     unsigned long long *nonfinite, long long *count, void *stream) {
  BN_REQUIRE(acc && normals && valid_normal && valid_depth && d_acc && count, "normal_target_loss: null argument");
  BN_REQUIRE(R >= 1 && R <= ((int64_t)1 << 30), "normal_target_loss: R=%lld outside [1, 2^30]", (long long)R);
  BN_REQUIRE(C >= 4 && C <= BN_MAX_CH, "normal_target_loss: C=%d unsupported", C);
  BN_REQUIRE(ch >= 0 && ch <= C - 3, "normal_target_loss: channel %d outside [0, %d]", ch, C - 3);
  BN_REQUIRE(fabsf(lambda) <= 3.0e38f, "normal_target_loss: lambda is not finite");
  BN_REQUIRE(n_stride >= 0 && vn_stride >= 0 && vd_stride >= 0, "normal_target_loss: negative stride");
  TargetArgs a;
  a.acc = acc; a.normals = normals; a.valid_normal = valid_normal; a.valid_depth = valid_depth;
  a.n_stride = n_stride; a.vn_stride = vn_stride; a.vd_stride = vd_stride; a.R = R; a.C = C; a.ch = ch; a.lambda = lambda;
  a.d_acc = d_acc; a.ray_loss = ray_loss; a.loss_acc = loss_acc; a.loss_slots = loss_slots > 0 ? loss_slots : 1;
  a.nonfinite = nonfinite; a.count = count;
  hipStream_t st = (hipStream_t)stream;
  BnProfScope prof_(BN_K_BRDF, st);
  normal_target_count_kernel<<<1, 1024, 0, st>>>(valid_depth, vd_stride, R, count);
  normal_target_ray_kernel<<<dim3((unsigned)ceil_div64(R, 256)), 256, 0, st>>>(a);
  BN_LAUNCH_CHECK("normal_target_loss");
  return 0;
}
