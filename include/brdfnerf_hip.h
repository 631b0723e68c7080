/*
 * brdfnerf_hip.h - C ABI of the MI355X (gfx950) implementation of BRDF-NeRF's ray-batched
 * volume-rendering hot path (spsbrdf-nerf).
 *
 * The reference (LulinZhang/BRDF-NeRF) has no FFI layer: its boundary is the Python signatures
 * of `SpSBRDFNeRF.forward`, `inference`, `cal_weight`, `render_rays`, the BRDF classes and the
 * guided-sampling helpers.  Each entry point below replaces the ATen op
 * sequence of one of those functions; the file:line it replaces is cited per function
 * (paths relative to the reference repo root).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (PyTorch's caching allocator in
 *    the shipped host code); nothing is allocated, freed or synchronised inside a call;
 *  - `stream` is a hipStream_t passed as void*; all calls are asynchronous on that stream,
 *    re-entrant, and keep no global state (graph-capturable);
 *  - return value: 0 on success, a negative bn_status otherwise; bn_last_error() returns a
 *    thread-local description of the last failure.  Nothing throws across the boundary;
 *  - NaN handling follows the reference's check_nan(val_rep=...) replacement values
 *    (train_utils.py:61-78) in-kernel, without its prints and host syncs.
 *  - `dtype`: BN_F32 computes the MLP with exact-fp32 MFMA (v_mfma_f32_32x32x2_f32; parity
 *    mode, 1e-4 relative vs the reference), BN_BF16 with bf16 MFMA (v_mfma_f32_32x32x16_bf16,
 *    fp32 accumulate; throughput mode), BN_F16 with fp16 MFMA (v_mfma_f32_32x32x16_f16, fp32
 *    accumulate; same rate as bf16, 3 more mantissa bits; the backward chains run on gradients
 *    scaled by a power of two chosen on the device from max|d_out|, removed again before the
 *    fp32 gradient accumulation - BASELINE config 5).  Everything outside the dense layers is fp32.
 */
#ifndef BRDFNERF_HIP_H
#define BRDFNERF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BN_ABI_VERSION 7
#define BN_MAX_LAYERS 12
#define BN_MAX_HEADS 6 /* rgb (+ beta) + up to 3 BRDF heads evaluated together, two per pass */

typedef enum { BN_OK = 0, BN_EINVAL = -1, BN_EUNSUPPORTED = -2, BN_ELAUNCH = -3 } bn_status;
typedef enum { BN_F32 = 0, BN_BF16 = 1, BN_F16 = 2 } bn_dtype;
typedef enum { BN_ACT_SIN = 0, BN_ACT_RELU = 1 } bn_act;
/* post-sigmoid rescale of a head (spsbrdfnerf.py:730,735,754) */
typedef enum {
  BN_HEAD_PLAIN = 0,       /* sigmoid, width = head_out (rgb, roughness)                        */
  BN_HEAD_RPV_K = 1,       /* (v-.5)*2+1, 1-wide tiled x3                                       */
  BN_HEAD_RPV_THETA = 2,   /* (v-.5)*2,   1-wide tiled x3                                       */
  BN_HEAD_HAPKE_THETA = 3, /* v*pi/6, width 1                                                   */
  BN_HEAD_TILE3 = 4,       /* sigmoid, 1-wide tiled x3 (rhoc, b, c)                             */
  BN_HEAD_BETA = 5         /* --beta (spsbrdfnerf.py:571-575,708-711): SOFTPLUS instead of sigmoid, width 1, written to
                              channel 4 (right after sigma, before the normals); only as head 1; its first layer also
                              reads the per-image embedding (desc.t_dim columns)                  */
} bn_head_kind;

int bn_abi_version(void);
const char *bn_last_error(void);
/* Diagnostic / A-B preprocessor switches this build of the library was compiled with, space-separated ("" for the release
 * build).  Timing builds under profiles/ change instruction streams or drop work; the test-suite asserts that the library
 * it validates reports none. */
const char *bn_build_flags(void);
/* First 16 hex digits of the sha256 over the sources the library was compiled from (csrc/, this header, the build recipe). */
const char *bn_source_hash(void);
/* The reference trains with Lightning's deterministic=True (main.py:726).  Since ABI 5 bn_field_backward's parameter gradients
 * are bitwise identical for identical inputs in EVERY mode: the weight-gradient kernels write the partial tile of every point
 * split to a slab of the stash and a reduce kernel adds the slabs in split order (no fp32 atomics, no turn counters).  The
 * switch remains for callers that keyed on it (the Python trainer reports a fixed-order loss sum with it); the library's kernels
 * no longer read it.  Process-wide; returns the old value. */
int bn_set_deterministic(int on);
/* The current setting (read-only: callers that only want to know must not toggle a process-wide switch to find out). */
int bn_get_deterministic(void);

/* ---------------------------------------------------------------------------------------------
 * Field MLP (SpSBRDFNeRF.forward, models/spsbrdfnerf.py:662-757; calc_features :636-646;
 * Mapping.forward models/nerf.py:53-70).
 *
 * Geometry: F = feat (multiple of 64, <= 512), `layers` trunk layers, skip-concat [PE, h] at
 * layer `skip` (-1: none), PE with `pe_freqs` octaves (0: raw xyz).  Heads: sigma (F->1,
 * softplus), feats (F->F, linear), then n_heads two-layer heads F -> F/2 (act) -> head_out[i]
 * (sigmoid), head 0 = rgb.  Optional learned normal (grad_from_xyz, F->3, -l2_normalize).
 *
 * Weights are consumed in a packed, MFMA-fragment-ordered copy produced by bn_pack_field();
 * biases and the small second-layer head matrices are read as fp32 from the caller's tensors.
 * ------------------------------------------------------------------------------------------- */
typedef struct bn_field_desc {
  int32_t feat, layers, skip, pe_freqs, act, dtype;
  int32_t n_heads;                     /* heads evaluated in this call (>=1, head 0 = rgb)    */
  int32_t head_out[BN_MAX_HEADS];      /* 1 or 3                                              */
  int32_t head_kind[BN_MAX_HEADS];     /* bn_head_kind                                        */
  int32_t normal_lr;                   /* 1: evaluate grad_from_xyz                            */
  int32_t normal_an;                   /* 1: analytic normal = -normalize(d sigma/d xyz)       */
  int32_t out_channels;                /* row length of `out`                                  */
  int32_t fold_feats;                  /* 1: the linear feats layer is folded into every head's first layer by the caller:
                                          params.head_w1[h] = <head>.0.weight * feats_from_xyz.weight  ([F/2][F]),
                                          params.head_b1[h] = <head>.0.weight * feats_from_xyz.bias + <head>.0.bias,
                                          feats_w / feats_b are ignored; bn_field_backward then returns dL/d(folded w1),
                                          dL/d(folded b1) in grads.head_w1/head_b1 and leaves grads.feats_* untouched
                                          (chain rule back to the three factors: brdf_nerf_amd/functions.py, unfold_grads).
                                          Same function, one F x F product less per point in forward, backward and
                                          weight gradient.                                           */
  int32_t dir_dim;                     /* --input_viewdir 1 (spsbrdfnerf.py:458,689-692): width of the (encoded) view direction the
                                          rgb head's first layer reads beside the features: 0 (off), 3 (raw, no --mapping) or
                                          6 * dir_freqs.  Needs fold_feats = 1: params.head_w1[0] is the folded [F/2][F] matrix and
                                          params.head0_wdir the direction columns of <rgb head>.0.weight                        */
  int32_t dir_freqs;                   /* octaves of the direction encoding (mapping_sizes[1] = 4), 0 = raw direction              */
  int32_t t_dim;                       /* --beta: width of the per-image embedding (--t_embbeding_tau, default 4) that head 1
                                          (kind BN_HEAD_BETA) reads beside the features; 0 without that head.  Needs fold_feats;
                                          params.head1_wt = beta_from_xyz.0.weight[:, F:].  Together with dir_dim:
                                          round_up(dir_dim, 8) + t_dim <= 32                                                      */
} bn_field_desc;

/* fp32 parameter tensors in PyTorch nn.Linear layout (weight [out][in], row-major). */
typedef struct bn_field_params {
  const float *trunk_w[BN_MAX_LAYERS]; /* fc_net.{2i}.weight                                   */
  const float *trunk_b[BN_MAX_LAYERS];
  const float *sigma_w, *sigma_b;      /* sigma_from_xyz.0                                     */
  const float *feats_w, *feats_b;      /* feats_from_xyz                                       */
  const float *head_w1[BN_MAX_HEADS], *head_b1[BN_MAX_HEADS]; /* <head>.0                      */
  const float *head_w2[BN_MAX_HEADS], *head_b2[BN_MAX_HEADS]; /* <head>.2                      */
  const float *normal_w, *normal_b;    /* grad_from_xyz (may be NULL)                          */
  const float *head0_wdir;             /* rgb_from_xyzdir.0.weight[:, F:]  ([F/2][dir_dim], row stride head0_wdir_ld); NULL when dir_dim == 0 */
  int64_t head0_wdir_ld;
  const float *head1_wt;               /* beta_from_xyz.0.weight[:, F:]  ([F/2][t_dim], row stride head1_wt_ld); NULL when t_dim == 0 */
  int64_t head1_wt_ld;
} bn_field_params;

/* Same shape as bn_field_params but writable: gradient accumulators (fp32, += semantics). */
typedef struct bn_field_grads {
  float *trunk_w[BN_MAX_LAYERS], *trunk_b[BN_MAX_LAYERS];
  float *sigma_w, *sigma_b, *feats_w, *feats_b;
  float *head_w1[BN_MAX_HEADS], *head_b1[BN_MAX_HEADS], *head_w2[BN_MAX_HEADS], *head_b2[BN_MAX_HEADS];
  float *normal_w, *normal_b;
  float *head0_wdir;                   /* += d/d rgb_from_xyzdir.0.weight[:, F:]  (row stride head0_wdir_ld) */
  int64_t head0_wdir_ld;
  float *head1_wt;                     /* += d/d beta_from_xyz.0.weight[:, F:]  (row stride head1_wt_ld) */
  int64_t head1_wt_ld;
  float *d_t_embed;                    /* nullable; = (overwritten) d/d t_embed per POINT, [n_points][t_dim], in both point forms
                                          (the rays form's per-ray gradient is its sum over the ray's samples)            */
} bn_field_grads;

/* Bytes of the packed weight buffer (forward + transposed copies) for `desc`. */
size_t bn_field_packed_bytes(const bn_field_desc *desc);
/* Re-pack after every optimizer step (a few MB; one launch per matrix). */
int bn_pack_field(const bn_field_desc *desc, const bn_field_params *params, void *packed, void *stream);

/* Bytes of the activation stash a training forward writes for `n_points` points. */
size_t bn_field_stash_bytes(const bn_field_desc *desc, int64_t n_points);

/* Points: either `xyz` [n_points][3], or rays (`rays` [n_rays][ray_stride] = o3,d3,near,far[,sun3];
 * `z` [n_rays][n_samples]; xyz = o + d*z, rendering.py:184) when xyz == NULL. */
typedef struct bn_points {
  const float *xyz;
  const float *rays;
  const float *z;
  int32_t ray_stride, n_samples;
  int64_t n_points;
  const float *dirs;                   /* xyz form with desc.dir_dim > 0: view direction per point [n_points][3] (the rays form reads
                                          rays[ray][3:6], as inference() repeats rays_d per sample, spsbrdfnerf.py:96,121)       */
  const float *t_embed;                /* desc.t_dim > 0: the per-image embedding models['t'](ts) (rendering.py:226-229) - xyz form:
                                          per point [n_points][t_dim]; rays form: per ray [n_rays][t_dim] (repeated per sample,
                                          spsbrdfnerf.py:98)                                                                       */
  /* One output array and ONE stash for several forward calls (round 3: pass 1 and pass 2 of the fused step are evaluated by
   * two launches - the second needs the first's result to place its samples - and back-propagated by ONE set of launches).
   * Forward / normals: this call's points are points [point_offset, point_offset + n_points) of a set of total_points points
   * (point_offset a multiple of the tile: 128 points in the 16-bit modes, 64 in fp32; `out` and `stash` are the SET's);
   * total_points == 0: a set of its own.  Backward over the whole set (rays form): points [0, seg1_points) are samples
   * z[r][0 .. n_samples) of ray r, points [seg1_points, n_points) are samples z2[r][0 .. n_samples2); seg1_points == 0: one block. */
  int64_t point_offset, total_points;
  const float *z2;
  int32_t n_samples2;
  int64_t seg1_points;
} bn_points;

/* sigma-only forward (forward(sigma_only=True), spsbrdfnerf.py:684): sigma[n_points]. */
int bn_field_sigma(const bn_field_desc *desc, const bn_field_params *params, const void *packed,
                   const bn_points *pts, float *sigma, void *stream);
/* full forward: out[n_points][desc->out_channels], channel order of spsbrdfnerf.py:694-755:
 * [rgb3, sigma, (beta1), (normal_an3), (normal_lr3), head outputs (1-wide RPV/Hapke b,c heads tiled x3)].
 * `stash` != NULL keeps what bn_field_backward needs. */
int bn_field_forward(const bn_field_desc *desc, const bn_field_params *params, const void *packed,
                     const bn_points *pts, float *out, void *stash, void *stream);
/* Analytic normals (calc_normals, models/spsbrdfnerf.py:648-660 and :713-716): fills channels [4,7) of `out` with
 * -l2_normalize(d sigma / d xyz) by the explicit adjoint chain over the stash of a preceding bn_field_forward() call on
 * the same points (desc->normal_an must be 1 in both).  grad_x (nullable) receives the raw gradient [n_points][3].
 * keep_for_backward = 1 also stashes what bn_field_backward needs to differentiate THROUGH the normals (the reference's
 * create_graph=True double backward). */
int bn_field_normals(const bn_field_desc *desc, const bn_field_params *params, const void *packed,
                     const bn_points *pts, const void *stash, float *out, float *grad_x, int32_t keep_for_backward,
                     void *stream);
/* Parameter gradients from d_out[n_points][out_channels] (autograd of forward, K9 in SURVEY.md).
 * `out` is the forward's output.  grads are accumulated (+=). */
int bn_field_backward(const bn_field_desc *desc, const bn_field_params *params, const void *packed,
                      const bn_points *pts, const float *out, const float *d_out, void *stash,
                      const bn_field_grads *grads, void *stream);

/* bn_field_backward in parts (a bit mask), for callers that overlap the gradient all-reduce with the rest of the backward
 * (the reference: Lightning DDP's bucketed all-reduce, main.py:720-731): BN_BWD_CHAIN = the dX chain(s) that fill the
 * stash with the pre-activation gradients; BN_BWD_WGRAD_TRUNK = the weight gradients of the trunk layers (the leading,
 * contiguous share of a flat parameter buffer in state_dict order); BN_BWD_WGRAD_HEADS = those of the (folded) head first
 * layers, the feats layer and the extra-input columns; BN_BWD_SKINNY = the one- to four-row matrices (sigma head, learned
 * normal, second head layers) and d_t_embed.  The parts of one backward are called in this order on one stream.
 * Every mask is served whatever bn_set_deterministic says (the switch changes nothing: the slab sums run in a fixed order);
 * a gradient is written by the jobs of ONE part, so it is final once the call that carries that part has run. */
enum { BN_BWD_CHAIN = 1, BN_BWD_WGRAD_TRUNK = 2, BN_BWD_WGRAD_HEADS = 4, BN_BWD_SKINNY = 8, BN_BWD_ALL = 15 };
int bn_field_backward_parts(const bn_field_desc *desc, const bn_field_params *params, const void *packed,
                            const bn_points *pts, const float *out, const float *d_out, void *stash,
                            const bn_field_grads *grads, int32_t parts, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Alpha compositing (cal_weight, models/spsbrdfnerf.py:50-69) fused with the per-ray weighted
 * sums of inference() (:198,:242,:271,:275,:292,:314-317,:326-338).
 * z, sigma: [R][S]; noise (nullable): [R][S] standard normals, used as sigma + noise*noise_std.
 * chan (nullable): [R][S][C] per-sample channels; acc: [R][C] = sum_s w*chan.
 * Outputs alphas, trans, weights [R][S] (nullable individually), depth [R].
 * ------------------------------------------------------------------------------------------- */
int bn_composite_forward(const float *z, const float *sigma, int64_t sigma_stride, const float *noise,
                         float noise_std, const float *chan, int64_t chan_stride, int32_t C, int64_t R, int32_t S,
                         float *alphas, float *trans, float *weights, float *depth, float *acc, void *stream);
/* Backward: given d_weights [R][S] (nullable), d_depth [R] (nullable), d_acc [R][C] (nullable),
 * writes d_sigma (strided like sigma) and d_chan (strided like chan, nullable). */
int bn_composite_backward(const float *z, const float *sigma, int64_t sigma_stride, const float *noise,
                          float noise_std, const float *chan, int64_t chan_stride, int32_t C, int64_t R, int32_t S,
                          const float *d_weights, const float *d_depth, const float *d_acc, float *d_sigma,
                          int64_t d_sigma_stride, float *d_chan, int64_t d_chan_stride, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Ray-level tail of a Lambertian training step in one launch: shading of the composited sums
 * (models/spsbrdfnerf.py:270-282, rgb = clamp(sum_s w (albedo (1+2p) - p), 0, 1)), SNerfLoss
 * (metrics.py:39-61, lambda_sc = 0) and DepthLoss (metrics.py:82-161, subset=True, GNLL=False; the
 * np.where row selection as a mask), with the gradients autograd would return for acc [R][C], depth [R] and
 * weights [R][S].  target_depth == NULL: no depth term.  ray_loss [R] sums to the step's loss.
 * ------------------------------------------------------------------------------------------- */
int bn_lambert_loss(const float *acc, int32_t C, const float *weights, const float *z, int32_t S, const float *depth,
                    const float *rgbs, const float *valid_depth, const float *target_depth, const float *target_weight,
                    const float *target_std, float rgb_padding, float lambda_rgb, float lambda_ds, int32_t usealldepth,
                    int64_t R, float *ray_loss, float *rgb, float *d_acc, float *d_depth, float *d_weights, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Stratified depths (get_z_vals, rendering.py:149-166, perturb=1): z[R][S] from near/far taken
 * from rays[:,6], rays[:,7] (or explicit near/far arrays) and uniforms u[R][S].
 * ------------------------------------------------------------------------------------------- */
int bn_stratified_z(const float *near, const float *far, int64_t nf_stride, const float *u, int64_t R, int32_t S,
                    float *z, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Depth-guided resampling + merge (GenerateGuidedSamples .. sample_pdf, rendering.py:13-91,
 * :116-147; merge :263-272).  Per ray: std = sqrt(sum w (z-depth)^2); 3-sigma window clamped to
 * [near0, far0] and symmetrised; G Gaussian-weighted bins; inverse-CDF with u[R][G]; sort;
 * then z_all[R][S+G] = sort(cat[z, z2]) with sort_idx int64 (bit-exact index semantics).
 * Rows with use_target[r] != 0 (train mode & valid depth) sample around target_depth/target_std
 * with u_target[target_row[r]][G] instead (rendering.py:135-145: the reference draws one row per VALID ray,
 * target_row[r] = rank of ray r among them; target_row == NULL: u_target has one row per ray, [R][G]).
 * ------------------------------------------------------------------------------------------- */
int bn_guided_samples(const float *z, const float *weights, const float *depth, const float *u, int64_t R,
                      int32_t S, int32_t G, float near0, float far0, float d_range, const float *use_target,
                      const float *target_depth, const float *target_std, const float *u_target,
                      const int32_t *target_row, float *z2_sorted, float *z_all, int64_t *sort_idx, void *stream);

/* The same with the clamp window read on the device: near_far -> two floats (near0, far0), e.g. &rays[0][6] for
 * the reference's `near[0,0]`, `far[0,0]` (rendering.py:133,144) - no device->host read in the caller. */
int bn_guided_samples_nf(const float *z, const float *weights, const float *depth, const float *u, int64_t R,
                         int32_t S, int32_t G, const float *near_far, float d_range, const float *use_target,
                         const float *target_depth, const float *target_std, const float *u_target,
                         const int32_t *target_row, float *z2_sorted, float *z_all, int64_t *sort_idx, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Per-ray BRDF shading (eval_RPV / eval_Hapke / eval_microfacet_brdf, models/spsbrdfnerf.py:9-30;
 * BRDF/RPV.py:40-63, BRDF/Hapke.py:139-200, BRDF/microfacet.py:20-72, BRDF/basic_func.py:5-44).
 * All inputs [N][3] unless noted; nullable inputs select the reference's "None" branches.
 * Forward writes brdf [N][3] and aux [N][BN_BRDF_AUX] (model specific, see csrc/brdf.hip);
 * backward writes gradients w.r.t. the non-null differentiable inputs.
 * ------------------------------------------------------------------------------------------- */
#define BN_BRDF_AUX 16
int bn_brdf_rpv_forward(const float *l, const float *v, const float *n, const float *w, const float *k,
                        const float *theta, const float *rhoc, int64_t N, float *brdf, float *aux, void *stream);
int bn_brdf_rpv_backward(const float *l, const float *v, const float *n, const float *w, const float *k,
                         const float *theta, const float *rhoc, const float *d_brdf, int64_t N, float *d_n,
                         float *d_w, float *d_k, float *d_theta, float *d_rhoc, void *stream);
int bn_brdf_hapke_forward(const float *l, const float *v, const float *n, const float *w, const float *b,
                          const float *c, const float *theta /*[N]*/, float hpk_scl, int32_t shell, int64_t N,
                          float *brdf, float *aux, void *stream);
int bn_brdf_hapke_backward(const float *l, const float *v, const float *n, const float *w, const float *b,
                           const float *c, const float *theta, float hpk_scl, int32_t shell, const float *d_brdf,
                           int64_t N, float *d_n, float *d_w, float *d_b, float *d_c, float *d_theta, void *stream);
int bn_brdf_microfacet_forward(const float *l, const float *v, const float *n, const float *albedo,
                               const float *rough /*[N]*/, float f0, int64_t N, float *brdf, float *aux,
                               void *stream);
int bn_brdf_microfacet_backward(const float *l, const float *v, const float *n, const float *albedo,
                                const float *rough, float f0, const float *d_brdf, int64_t N, float *d_n,
                                float *d_albedo, float *d_rough, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Training-step tail (main.py:147-168 Adam; metrics.py:39-61 MSE): fused Adam over one flat fp32
 * parameter buffer (the nn.Parameters are views into it).
 * ------------------------------------------------------------------------------------------- */
/* The betas of bn_adam_step / bn_adam_multi are the float32 values the arguments hold, promoted to double wherever a power
 * is taken: beta^step is ((double)beta)^step (bn_adam_step: pow; bn_adam_multi: a running product in the step state), and
 * 1.f - beta is exact in float32.  A caller that writes the state's powers itself (resume) takes powers of the same
 * float32 values: for beta2 = 0.999 (0.99900001287 in float32) the double's power is 1.3e-5 away after 1000 steps. */
int bn_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, float lr,
                 float beta1, float beta2, float eps, float weight_decay, int32_t step, float grad_scale,
                 void *stream);

/* ---------------------------------------------------------------------------------------------
 * Launch-lean fused training step (round 3).  The reference's step is ~150 ATen launches of glue around the field
 * evaluations (rendering.py:168-291, models/spsbrdfnerf.py:198-416, metrics.py:39-161, main.py:147-168); these entry points
 * fold that glue into a handful of per-ray kernels so that a Lambertian step is <= 20 launches and can be captured in a
 * HIP graph (no argument changes from step to step: draws, step counters and the learning rate live in device memory).
 * ------------------------------------------------------------------------------------------- */

/* Device-resident state of the fused step (bn_step_state, 512 bytes, 16-byte aligned; the caller allocates and zero-fills
 * it, sets rng_seed / lr, and may rewrite lr between steps):
 *   [0]  u64 rng_seed      Philox key of the in-kernel draws
 *   [8]  u64 rng_step      Philox counter word, advanced by bn_adam_multi (one per training step)
 *   [16] f32 lr            learning rate read by bn_adam_multi
 *   [20] u32 done          internal (completion ticket of bn_adam_multi)
 *   [24] i32 adam_step[4]  optimiser step count per parameter group (torch.optim.Adam keeps one per parameter)
 *   [40] f32 noise_std     --noise_std of the running step, read by the compositing kernels when bn_noise.noise_std < 0 (ABI 7)
 *   [64] f32 loss_ring[64] loss of step t at slot t % 64 (written by bn_adam_multi from the partial sums)
 *   [320] f64 beta1_pow[4], [352] f64 beta2_pow[4]   beta^adam_step per group (1.0 at step 0): the bias corrections
 *   [512] f32 loss_part[64] partial sums of the running step's loss (bn_lambert_tail adds ray r's term to slot r % 64;
 *                           bn_adam_multi folds them into the ring and clears them) */
#define BN_STATE_BYTES 1024
#define BN_STATE_NOISE_OFF 40
#define BN_STATE_LOSS_OFF 64
#define BN_STATE_LOSS_SLOTS 64
#define BN_STATE_POW_OFF 320
#define BN_STATE_PART_OFF 512
#define BN_ADAM_MAX_GROUPS 4
/* in-kernel draw streams of one step */
enum { BN_RNG_COARSE = 1, BN_RNG_GUIDED = 2, BN_RNG_GUIDED_TARGET = 3, BN_RNG_NOISE_COARSE = 4, BN_RNG_NOISE_MERGED = 5, BN_RNG_SUN = 6 };

/* --noise_std (models/spsbrdfnerf.py:57-59: alphas = 1 - exp(-deltas * relu(sigmas + randn * noise_std)), main.py:246) with
 * in-kernel draws (ABI 6): a standard normal per (ray, sample position) from stream `rng_stream` of the state at `rng`
 * (Box-Muller on a Philox pair), element (ray_offset + r) * S + s of the stream, S = the sample count of the compositing it
 * perturbs (pass 1: the S coarse samples; the final compositing: the depth-sorted S + G set, position = sorted position).
 * NULL, or noise_std == 0: no noise.  noise_std < 0 (ABI 7): the kernels read the value from the step state at `rng` (f32 at byte
 * BN_STATE_NOISE_OFF): the reference multiplies noise_std by 0.9 after EVERY step (main.py:246), and a value baked into the launch
 * arguments would give every step a new signature - no graph replay while the noise decays.  The forward and the backward of a
 * step name the same stream and see the same draws. */
typedef struct {
  const unsigned long long *rng;
  float noise_std;
  uint32_t rng_stream;
  int64_t ray_offset;
} bn_noise;
/* The standard normals an in-kernel noise stream hands to elements 0..n-1, as an array (tests, replay). */
int bn_rng_normal(const unsigned long long *rng, uint32_t rng_stream, int64_t n, float *x, void *stream);

/* bn_stratified_z with in-kernel uniforms (stream `rng_stream` of the state at `rng` = &state[0]).  The draw of sample s of
 * ray r is element (ray_offset + r) * S + s of the stream: a rank that holds rays [ray_offset, ray_offset + R) of a global
 * batch draws exactly what a single process would draw for them. */
int bn_stratified_z_rng(const float *near, const float *far, int64_t nf_stride, const unsigned long long *rng,
                        uint32_t rng_stream, int64_t ray_offset, int64_t R, int32_t S, float *z, void *stream);
/* The uniforms an in-kernel stream hands to elements 0..n-1, as an array (tests, and callers that want to replay a step). */
int bn_rng_uniform(const unsigned long long *rng, uint32_t rng_stream, int64_t n, float *u, void *stream);

/* Pass-1 compositing (cal_weight on sigma [R][S], element stride sigma_stride; `noise` nullable, see bn_noise) +
 * bn_guided_samples_nf in one launch.  Per-ray prior arrays carry an element stride (depths[:, 0] of the [R][2] table, satellite_rgb_dep.py:339).
 * Draws: arrays u [R][G] / u_target [R][G] (one row per ray), or - when u == NULL - the in-kernel streams rng_u / rng_ut
 * of `rng`.  weights [R][S] / depth [R] (nullable) receive the pass-1 weights and depth. */
int bn_composite_guided(const float *z, const float *sigma, int64_t sigma_stride, int64_t R, int32_t S, int32_t G,
                        const float *near_far, float d_range, const float *use_target, int64_t ut_stride,
                        const float *target_depth, int64_t td_stride, const float *target_std, int64_t ts_stride,
                        const float *u, const float *u_target, const unsigned long long *rng, uint32_t rng_u,
                        uint32_t rng_ut, int64_t ray_offset, float *z2_sorted, float *z_all, int64_t *sort_idx, float *weights,
                        float *depth, const bn_noise *noise, void *stream);

/* Compositing of the depth-sorted union of two field outputs without materialising it: sample s of ray r is row
 * sort_idx[r][s] of cat[out1[r] ([S1][C]), out2[r] ([S2-S1][C])] (rendering.py:263-272; sigma = channel 3).  sort_idx ==
 * NULL: out1 alone (S1 == S2).  Forward: cal_weight + the weighted sums acc [R][C] (acc[:, 3] is not defined), wsum [R] =
 * sum_s w.  Backward: from d_weights [R][S2], d_depth [R], d_acc [R][C] (d_acc[:, 3] ignored), d_wsum [R] (all nullable)
 * to the gradient rows d_out1 / d_out2 in the SOURCE layouts (channel 3 = d sigma).  nonfinite (nullable): NaN / Inf
 * gradient elements are written as 0 and counted ([0] NaN, [1] Inf) - FusedTrainer.sanitize_grads without extra passes. */
/* NormalRegLoss (metrics.py:179-216) inside the merged-set compositing: lambda_an sum_s w_s min(0, n_an,s . view)^2 + the same
 * for the learned normals, view = -rays_d [R] rows with element stride rd_stride; channel < 0 or lambda <= 0: that field is off.
 * The forward writes the ray's term to reg_out [R] (an extra loss term for bn_ray_shade_loss), the backward adds its gradient
 * w.r.t. the weights and the per-sample normal channels.  NULL (or rays_d == NULL): off. */
typedef struct {
  const float *rays_d;
  int64_t rd_stride;
  int32_t ch_an, ch_lr;
  float lambda_an, lambda_lr;
  /* NormalLoss between the two per-sample normal fields (metrics.py:218-261, keyword 'an_lr' = --nr_spv_type 1, main.py:297-303):
   * lambda_spv * mean(weights) * mean|n_an - n_lr| over the whole batch - two batch-wide means, so the step makes three stops:
   * the forward writes each ray's (sum_s w_s, sum_s sum_c |n_an - n_lr|) to spv_ray [R][2]; bn_normal_spv_reduce adds them up in a
   * fixed order into spv_tot [4] = (d loss / d w_s, d loss / d n_an per component and unit sign, the loss term, 0) and adds the
   * term to the step's loss; the backward reads spv_tot.  lambda_spv == 0: off.  (ABI 6) */
  float lambda_spv;
  int32_t spv_ch_an, spv_ch_lr;
  float *spv_ray;
  float *spv_tot;
} bn_normal_reg;
int bn_normal_spv_reduce(const float *spv_ray, int64_t R, int32_t S, float lambda_spv, float *spv_tot, float *ray_loss,
                         float *loss_acc, void *stream);
int bn_merged_composite_forward(const float *z, const int64_t *sort_idx, const float *out1, const float *out2, int32_t S1,
                                int32_t S2, int32_t C, int64_t R, float *alphas, float *trans, float *weights, float *depth,
                                float *acc, float *wsum, float *var, const bn_normal_reg *nreg, float *reg_out,
                                const bn_noise *noise, void *stream);
/* hs_scale != 0 (with depth [R], the forward's result): adds hs_scale (z_s - depth)^2 to d loss / d w_s - the per-sample part
 * of HardSurfaceLoss's gradient (metrics.py:263-290), see bn_ray_shade_loss. */
int bn_merged_composite_backward(const float *z, const int64_t *sort_idx, const float *out1, const float *out2, int32_t S1,
                                 int32_t S2, int32_t C, int64_t R, const float *d_weights, const float *d_depth,
                                 const float *d_acc, const float *d_wsum, float hs_scale, const float *depth,
                                 const bn_normal_reg *nreg, float *d_out1, float *d_out2, unsigned long long *nonfinite,
                                 const bn_noise *noise, void *stream);

/* Ray-level shading + losses of a training step whose rays have ONE BRDF each (MultiBRDF == 0) and no per-sample
 * irradiance, forward AND backward in one launch (one thread per ray), between bn_merged_composite_forward and
 * bn_merged_composite_backward.  From the composited sums acc [R][C], wsum [R], depth [R] and var [R] = sum_s w (z - depth)^2:
 *   albedo_s = acc[0:3] (1 + 2 pad) - pad wsum ;  n = l2_normalize(acc[ch_normal : +3]) ;  parameters = acc[ch_p* : ...]
 *   rgb = clamp(irradiance * BRDF(sun_d, -rays_d, n, albedo_s, parameters), 0, 1)        (models/spsbrdfnerf.py:259-357)
 *   loss = SNerfLoss(rgb, rgbs) + DepthLoss + HardSurfaceLoss                           (metrics.py:39-61, 82-161, 263-290)
 * and d loss / d acc [R][C], d loss / d wsum [R], d loss / d depth [R] (the HardSurfaceLoss term's per-sample part is
 * bn_merged_composite_backward's hs_scale = lambda_hs / R).  kind: BN_SHADE_*; channels < 0: head absent (RPV: p0 k, p1
 * theta, p2 rhoc, or rhoc = albedo_s with rhoc_is_albedo (funcH == 2); Hapke: p0 b, p1 c, p2 theta (1 wide); microfacet: p0
 * roughness (1 wide)).  sun_d NULL: (1,1,1).  The prior arrays carry element strides and are nullable together.  nonfinite
 * (nullable, [0] NaN [1] Inf counters): a ray whose loss term is not finite is left out (loss 0, gradients 0) and counted -
 * without it the NaN reaches the loss and the gradients as it does upstream.  extra_loss [R] (nullable): per-ray terms computed
 * elsewhere that belong to the step's loss (bn_merged_composite_forward's reg_out), added to the ray's term. */
enum { BN_SHADE_LAMBERT = 0, BN_SHADE_RPV = 1, BN_SHADE_HAPKE = 2, BN_SHADE_MICROFACET = 3 };
typedef struct {
  int32_t kind, C, ch_normal, ch_p0, ch_p1, ch_p2;
  int32_t rhoc_is_albedo, shell, cos_irradiance, usealldepth;
  float hpk_scl, f0, rgb_padding, lambda_rgb, lambda_ds, lambda_hs;
  /* ABI 6: per-ray irradiance (nullable; element stride irr_stride) - the sun visibility of the ray's LAST sample from the
   * sun pass (--sun_v analystic, rendering.py:244-259, models/spsbrdfnerf.py:354), a constant of the step; the cosine term
   * (cos_irradiance) wins when both are given, as upstream (:260-266). */
  const float *irr;
  int64_t irr_stride;
} bn_shade_desc;
int bn_ray_shade_loss(const bn_shade_desc *desc, const float *acc, const float *wsum, const float *depth, const float *var,
                      const float *rays_d, int64_t rd_stride, const float *sun_d, int64_t sd_stride, const float *rgbs,
                      const float *valid_depth, int64_t v_stride, const float *target_depth, int64_t td_stride,
                      const float *target_weight, int64_t tw_stride, const float *target_std, int64_t ts_stride, int64_t R,
                      float *rgb, float *ray_loss, float *loss_acc, int32_t loss_slots, float *d_acc, float *d_wsum,
                      float *d_depth, unsigned long long *nonfinite, const float *extra_loss, void *stream);
/* NormalLoss against per-ray target normals (additive to ABI 7): metrics.py:218-261 with keyword 'an' (--nr_spv_type 3, main.py:316-320)
 * or 'lr' (type 2, main.py:310-313), between bn_ray_shade_loss and bn_merged_composite_backward.  It ADDS into the three columns
 * d_acc[:, ch : ch + 3] that bn_ray_shade_loss wrote and into the step's loss; every other column and every unselected row of d_acc
 * is left as it is.  acc, d_acc [R][C]; ch the first channel of the composited normal; normals [R] rows of 3 floats, row stride
 * n_stride elements; valid_normal, valid_depth [R] with element strides (a column of wider storage).
 * In float32, every operation rounded on its own (no fused multiply-add):
 *   n_sel = #{r : valid_depth[r] > 0}                 (a NaN does not count; valid_normal plays no part in the count: upstream selects
 *                                                      by valid_depth and weights by valid_normal, main.py:319, metrics.py:238-242, so
 *                                                      a selected ray with valid_normal == 0 contributes 0 and still counts)
 *   n_sel == 0: nothing is added anywhere             (upstream's L1Loss over an empty selection is NaN)
 *   k = lambda / (3.f * (float)n_sel)
 *   for a ray r with valid_depth[r] > 0, vn = valid_normal[r]:
 *     e_c  = vn * normals[r][c] - vn * acc[r][ch + c]                  c = 0, 1, 2: two products, one subtraction
 *     term = k * ((|e_0| + |e_1|) + |e_2|)
 *     d_acc[r][ch + c] += (k * vn) * s_c,   s_c = -1 if e_c > 0, +1 if e_c < 0, else 0   (by comparison: 0 at e_c == 0 and at a NaN
 *                                                                                          e_c, as torch's L1 backward)
 *     ray_loss[r] += term   and / or   atomicAdd(loss_acc + r % loss_slots, term)          (both nullable)
 * nonfinite (nullable, [0] NaN [1] Inf counters): a selected ray whose term is not finite adds nothing - no loss, no gradient - and is
 * counted; without it the term reaches the loss and the gradient follows the comparisons.  A ray that bn_ray_shade_loss itself
 * dropped (its shading term was not finite: loss 0, gradients 0) KEEPS its normal term: the two decisions are independent.
 * Two launches: a one-workgroup count that WRITES count[0] (int64, device; nothing to zero before a graph replay), then one lane
 * per ray.  n_sel is an integer and the gradient path holds no float atomic: d_acc and ray_loss repeat bit for bit.
 * Refused (BN_EINVAL, nothing launched): NULL acc / normals / valid_normal / valid_depth / d_acc / count, R < 1 or over 2^30, C outside
 * [4, BN_MAX_CH = 32], ch outside [0, C - 3], a lambda that is not finite, a negative stride. */
int bn_normal_target_loss(const float *acc, int32_t C, int32_t ch, const float *normals, int64_t n_stride, const float *valid_normal,
                          int64_t vn_stride, const float *valid_depth, int64_t vd_stride, float lambda, int64_t R, float *d_acc,
                          float *ray_loss, float *loss_acc, int32_t loss_slots, unsigned long long *nonfinite, long long *count,
                          void *stream);
/* The shading of bn_ray_shade_loss under K directions at once, forward only: relighting a rendered view and the BRDF lobe of a
 * pixel from ONE geometry pass (acc, wsum do not depend on the sun; replaces create_dsm.py:44-77 and eval.py's
 * eval_pixel_variedvw, which render again per direction).  desc as above (its loss fields unused; irr must be NULL: a sun-pass
 * irradiance depends on the sun).  acc [R][C], wsum [R]; rays_d [R] rows with element stride rd_stride; sun [K][3];
 * view [K][3] nullable: when given it replaces -rays_d for every ray (lobe mode; rays_d may then be NULL).
 *   brdf[k][r] = BRDF(sun[k], view ? view[k] : -rays_d[r], l2_normalize(acc[r][ch_normal : +3]), albedo_s[r], parameters[r])
 *   rgb[k][r]  = clamp(irradiance[k] * brdf[k][r], 0, 1),  irradiance = |sun[k].z| with cos_irradiance and a normal channel, else 1
 * rgb [K][R][3]; brdf [K][R][3] nullable.  kind LAMBERT: the "BRDF" is albedo_s.  With K == 1 and sun = the rays' own sun, rgb is
 * what bn_ray_shade_loss writes.  Every (direction, ray) is computed on its own: results do not depend on K or on how the
 * directions are split over calls. */
int bn_ray_shade_dirs(const bn_shade_desc *desc, const float *acc, const float *wsum, const float *rays_d, int64_t rd_stride,
                      const float *sun, const float *view, int64_t R, int32_t K, float *rgb, float *brdf, void *stream);
/* bn_ray_shade_dirs one level down, for a model with one BRDF per SAMPLE (--MultiBRDF 1, models/spsbrdfnerf.py:289-307, 350-352),
 * forward only: K directions from the depth-sorted field-output rows X [R][S][C] and compositing weights w [R][S] of ONE geometry
 * pass (neither depends on the sun; replaces K calls of render_rays with rays[:, 8:11] = sun, create_dsm.py:44-77, and eval.py's
 * eval_pixel_variedvw for such a model).  desc, rays_d, sun, view as in bn_ray_shade_dirs; a sample's BRDF reads the row's raw
 * normal, raw albedo (channels 0-2) and parameter channels, exactly as bn_sample_brdf_forward does.
 *   brdf[k][r] = sum_s w[r][s] BRDF(sun[k], view ? view[k] : -rays_d[r], X[r][s])
 *   rgb[k][r]  = clamp(sum_s w[r][s] (BRDF(...) (1 + 2 pad) - pad) irradiance[k], 0, 1)
 * written at rgb[k * rgb_plane + r * 3 + c] (rgb_plane >= 3 R: a caller that shades a view chunk by chunk passes the plane of the
 * whole view) and brdf[k * brdf_plane + r * 3 + c] (nullable).  The sums run over ascending s in fp32, one accumulator per (ray,
 * direction, channel), and no sample is skipped (0 * inf stays NaN): results do not depend on K, on how directions or rays are
 * split over calls, or on the kernel's tiling.  kind LAMBERT is refused: that colour is bn_ray_shade_dirs of the composited sums. */
int bn_sample_shade_dirs(const bn_shade_desc *desc, const float *X, const float *w, const float *rays_d, int64_t rd_stride,
                         const float *sun, const float *view, int64_t R, int32_t S, int32_t K, float *rgb, int64_t rgb_plane,
                         float *brdf, int64_t brdf_plane, void *stream);
/* Relighting WITH cast shadows (--sun_v analystic; additive to ABI 7): the two ends of the sun-visibility pass (rendering.py:
 * 244-259) for K sun directions at once; between them bn_field_sigma evaluates the K R G points (rays = table, z = z_sun).
 *
 * bn_sun_ray_table: rays and depths of the pass.  rays [R] rows of ray_stride >= 6 floats (origin, direction), d1 [R] the pass-1
 * depth, sun [K][3], u [R][G] uniforms shared by all K (what K reseeded render_rays calls draw).  Row k R + r of table [K R][8]
 * is (o_r + d_r d1_r, sun_k, 0.01 far, far) with far = ratio_k d1_r, ratio_k = |rays[0].d_z / sun_k.z| where |sun_k.z| > 1e-5, else 1
 * - ROW 0 of this call's rays, as upstream (:246-248); z_sun [K R][G] is stratified from (0.01 far, far, u) exactly as
 * bn_stratified_z does.  Bitwise what rendering.sun_far + bn_stratified_z + the torch.cat of the sun rays give for direction k. */
#define BN_MAX_G 256             /* guided / sun-pass samples per ray at most */
int bn_sun_ray_table(const float *rays, int64_t ray_stride, const float *d1, const float *sun, const float *u, int64_t R, int32_t K,
                     int32_t G, float *table, float *z_sun, void *stream);
/* bn_sun_shade_dirs: transmittance and shading fused.  sigma_sun, z_sun [K][R][G] (bn_field_sigma's result on the table, and the
 * table's depths); noise [R][G] nullable, shared by all K, applied as bn_composite_forward applies it (sigma + noise noise_std).
 *   alpha_s = 1 - exp(-delta_s relu(sigma_s + noise_s noise_std)), delta_s = z_{s+1} - z_s, delta_{G-1} = 1e10
 *   T_s = prod_{j<s} (1 - alpha_j + 1e-10), multiplied in ascending j                    (models/spsbrdfnerf.py:50-69)
 * desc as in bn_ray_shade_dirs, with irr NULL.  Exactly one of (acc [R][C], wsum [R]) and (X [R][G][C], w [R][G]) is given:
 *   per ray    (acc; kind not LAMBERT)  rgb = clamp(T_{G-1} BRDF(sun_k, -rays_d, l2_normalize(acc normal), albedo_s, parameters)):
 *              the irradiance of the LAST sample (:354) times the BRDF body of bn_ray_shade_dirs
 *   per sample (X, w)                   rgb = clamp(sum_s w_s (c_s (1 + 2 pad) - pad) T_s), ascending s, one fp32 accumulator per
 *              channel; c_s the row's albedo for kind LAMBERT (:265-273), else BRDF(row_s, sun_k, -rays_d) as in
 *              bn_sample_shade_dirs (--MultiBRDF 1, :350-352).  The sun ray's sample index is the view ray's, as upstream.
 * rgb[k * rgb_plane + r * 3 + c]; vis[k * vis_plane + r] = T_{G-1} (nullable): the shadow map.  Replaces, per direction,
 * bn_composite_forward on the sun pass (alphas, transparency, weights [R][G] each) and the torch statement of the shading.
 * Refused: NULL inputs, irr set, cos_irradiance with a normal channel (the cosine branch wins upstream and the sun pass is unused:
 * bn_ray_shade_dirs / bn_sample_shade_dirs), both or neither of acc / X, per-ray mode with kind LAMBERT, G < 3 or G > BN_MAX_G.
 * Every (direction, ray) is computed on its own: results do not depend on K, on how directions or rays are split over calls, or on
 * the kernel's tiling. */
int bn_sun_shade_dirs(const bn_shade_desc *desc, const float *sigma_sun, const float *z_sun, const float *noise, float noise_std,
                      const float *acc, const float *wsum, const float *X, const float *w, const float *rays_d, int64_t rd_stride,
                      const float *sun, int64_t R, int32_t G, int32_t K, float *rgb, int64_t rgb_plane, float *vis, int64_t vis_plane,
                      void *stream);
/* Digital surface model of a rendered view (additive to ABI 7): the reference's host path - the point cloud of
 * get_latlonalt_from_nerf_prediction (datasets/satellite_rgb_dep.py:601-634, cs == 'utm': a denormalised point is (east, north,
 * altitude), :632-633) rasterised by plyflatten(cloud, xoff, yoff, resolution, xsize, ysize, radius=1, sigma=inf) (:636-699) -
 * as two launches on the device, bitwise reproducible.
 *
 * bn_dsm_splat: rays [R] rows of ray_stride >= 6 floats (origin, direction), depth [R]; center (HOST pointer, 3 doubles) and
 * range are the dataset's normalisation (:622-625); xoff / yoff the grid's western / NORTHERN edge (the affine transform of :695:
 * row 0 is the northern edge), resolution > 0 the cell size, W x H the grid.  Per ray, in float64 with the fp32 inputs widened
 * exactly and every operation rounded on its own (no fused multiply-add):
 *   p = (o + d depth) range + center ;  i = floor((p.x - xoff) / resolution) ;  j = floor((yoff - p.y) / resolution)
 *   for k1, k2 in [-radius, radius] (footprint BN_DSM_DISC: only k1^2 + k2^2 <= radius^2; BN_DSM_SQUARE: all (2 radius + 1)^2):
 *     cell (row j + k2, column i + k1), if inside the grid - each cell tested on its own, so a point whose centre cell is outside
 *     still reaches its neighbours inside - receives  sum += llrint(p.z 2^20), count += 1
 * acc: int64 [H][W][2] = (sum, count) per cell, 16-byte aligned device memory that the CALLER zeroes; several calls (chunks of a
 * view, several views) accumulate into it.  Both are integer atomic adds (the sum in two's complement) and there is no float
 * atomic: acc's bits do not depend on the order of the rays, on how they are split over calls, or on which device splatted
 * which ray - accumulators of several devices add up (SUM all-reduce) to the single-device one.
 * A row with a non-finite p or |p.z| >= 2^23 m deposits nothing and adds 1 to skipped[0] (a 64-bit device counter the caller
 * zeroes).  With that bound |llrint(p.z 2^20)| <= 2^43: a cell holds at least 2^20 points before its sum can overflow.
 * sigma = inf (the unweighted mean) is the only mode upstream uses and the only one served.  The footprint is the rule stated
 * HERE; it was not, and could not be, checked against the plyflatten package, which this project does not depend on.
 * Refused (BN_EINVAL): NULL pointers, radius < 0 or > BN_DSM_MAX_RADIUS, another footprint, resolution <= 0, a non-finite frame
 * or origin, W H over 2^31 cells, ray_stride < 6.
 *
 * bn_dsm_resolve: dsm [H][W] = (float)((double)sum / (double)count 2^-20), NaN where count == 0 - the reference's nodata
 * (:693); count [H][W] int32 (nullable), saturating at 2^31 - 1. */
enum { BN_DSM_DISC = 0, BN_DSM_SQUARE = 1 };
#define BN_DSM_MAX_RADIUS 4
int bn_dsm_splat(const float *rays, int64_t ray_stride, const float *depth, int64_t R, const double *center, double range, double xoff,
                 double yoff, double resolution, int32_t W, int32_t H, int32_t radius, int32_t footprint, long long *acc,
                 unsigned long long *skipped, void *stream);
int bn_dsm_resolve(const long long *acc, int32_t W, int32_t H, float *dsm, int32_t *count, void *stream);
/* Image and normal metrics of a rendered view (additive to ABI 7): the numbers of the reference's evaluation line (eval.py:467-479)
 * that neither render_image's PSNR nor the altitude MAE covers, as three launches.  Every float64 operation is rounded on its own
 * (no fused multiply-add) and every sum is an INTEGER atomic add: the results' bits do not depend on the block order or on how
 * an image's rows are split over calls or devices (SUM all-reduce of the integers merges ranks).
 *
 * bn_ssim_map: replaces metrics.py:327-341 (ssim_ -> kornia 0.5.3 ssim(pred, gt, window, max_val): Gaussian window of sigma 1.5,
 * reflect padding) and the `* mask.view(1, 1, H, W)` of eval.py:471.  pred, gt: C planes of H x W float32; element (c, r, col) is
 * at [c plane_stride + r row_stride + col col_stride] of BOTH (eval.py:471's .view(1, 3, H, W) of an (H W, 3) buffer is strides
 * (H W, W, 1); the true image of that buffer is (1, 3 W, 3)).  mask: uint8 [H][W] or NULL (all ones), multiplied in as a number.
 * g: `window` normalised 1-D Gaussian weights (HOST pointer; the device computes no exp).  Per output cell, in float64:
 *   x = ((double)pred (double)mask) / div, y likewise from gt; rows and columns outside the image by 'reflect' without repeating
 *   the edge (-1 -> 1, H -> H - 2); w[k2][k1] = g[k2] g[k1]; the five moments mu_x, mu_y, E[xx], E[yy], E[xy] start at 0.0 and take
 *   the taps in row-major order (k2 outer, k1 inner) as s = s + w v, v = x, y, x x, y y, x y rounded before the multiply;
 *   C1 = (0.01 max_val)^2, C2 = (0.03 max_val)^2; sxx = E[xx] - mu_x mu_x, syy, sxy likewise;
 *   v = ((2 mu_x mu_y + C1) (2 sxy + C2)) / ((mu_x mu_x + mu_y mu_y + C1) (sxx + syy + C2) + 1e-12)
 * for the output rows [row0, row1) only (the taps still read the whole image).  map: float32 [C][H][W] (nullable) receives (float)v,
 * rows outside the range untouched.  sums: int64 [3] the CALLER zeroes, += {sum of llrint(v 2^30), cells in that sum, cells
 * skipped}; a cell whose v is not finite or |v| >= 4 is skipped.  The SSIM is sums[0] / (sums[1] 2^30).  The rule follows kornia
 * 0.5.3 as documented; it was not checked against the package, which this project does not depend on.
 * Refused (BN_EINVAL): NULL pred / gt / g / sums, a window that is even or outside [3, BN_SSIM_MAX_WINDOW], H or W <= window / 2
 * (too small for the reflect padding), C H W over 2^30 (below it the sum cannot overflow), a negative stride, max_val, div or a
 * weight that is not finite, rows outside [0, H].
 *
 * bn_grid_normals: replaces calc_normal_from_pts3d (sat_utils.py:16-50) on get_pts3d_from_dsm (:175-183), as :251-255 call them.
 * z: float32 [H][W] altitudes.  Interior cell (r, c): P(r, c) = (c resolution, r resolution, z[r][c]) in float64; the vectors to the
 * south (r + 1), north (r - 1), east (c + 1) and west (c - 1) neighbours, each N(v) = v / sqrt(max((v.x^2 + v.y^2) + v.z^2, 2^-23))
 * (l2_normalize); n1 = N(E x N), n2 = N(W x S), n3 = N(N x W), n4 = N(S x E), n = N((((n1 + n2) + n3) + n4) / 4).  normals: float32
 * [H][W][3], rounded from float64; border cells (0, 0, 0); a NaN altitude makes the (up to five) normals that read it NaN.
 * AXES: as upstream y grows with the ROW, so the frame is left-handed and flat ground gives n = (0, 0, -1); the angle between
 * two grids does not depend on that.
 *
 * bn_normal_angle: replaces calc_nr_diff (sat_utils.py:164-173, normalize=False), the nanmean of :341 and MaskDoD (:278-297, :346).
 * n1, n2: float32 [H][W][3].  a = acos(clamp((n1.x n2.x + n1.y n2.y) + n1.z n2.z, -1, 1)) 180 / pi in float64; angle: float32 [H][W]
 * (nullable).  border = 0 is the reference (border normals are zero, so border cells count as 90 degrees); border = 1 writes NaN
 * there and leaves them out.  mask: uint8 [H][W], nonzero = inside; NULL: every cell is inside.  sums: int64 [6] the CALLER zeroes,
 * += {sum, count} over all cells, the inside cells and the outside cells, sum of llrint(a 2^20); NaN cells are left out. */
#define BN_SSIM_MAX_WINDOW 11
int bn_ssim_map(const float *pred, const float *gt, int32_t C, int32_t H, int32_t W, int64_t plane_stride, int64_t row_stride,
                int64_t col_stride, const uint8_t *mask, double div, double max_val, int32_t window, const double *g, int32_t row0,
                int32_t row1, float *map, long long *sums, void *stream);
int bn_grid_normals(const float *z, int32_t H, int32_t W, double resolution, float *normals, void *stream);
int bn_normal_angle(const float *n1, const float *n2, int32_t H, int32_t W, const uint8_t *mask, int32_t border, float *angle,
                    long long *sums, void *stream);
/* The xy registration of a DSM on its ground truth (additive to ABI 7): dsmr.compute_shift(gt, pred, scaling=False) and
 * dsmr.apply_shift as sat_utils.py:239-246 call them - the path the reference takes whenever dsmr imports - as three launches.
 * u is the ground truth, v the prediction, both [H][W] on one grid; a shift (dx, dy) pairs u[j][i] with v[j + dy][i + dx].
 * Every float64 operation is rounded on its own and every sum is an INTEGER atomic add, as above.
 *
 * bn_grid_halve: replaces dsmr.downsample2x (dsmr.py:16-46).  src: float64 [H][W]; dst: float64 [ceil(H / 2)][ceil(W / 2)].
 * Upstream writes out[j / 2][i / 2] for every input cell and the last write wins, so output cell (J, I) is the mean of the FINITE
 * cells of the 2 x 2 box whose corner is (j, i) = (2J + 1, 2I + 1) - (2J, .) when 2J + 1 == H, (., 2I) when 2I + 1 == W - cells
 * outside the image ignored: s = 0.0, then s = s + t in the order (j, i), (j + 1, i), (j, i + 1), (j + 1, i + 1), s / count; NaN
 * when no cell of the box is finite (an infinite cell counts as missing).
 *
 * bn_ncc_moments: replaces the two image passes of dsmr.mean_std (dsmr.py:49-88) for every shift that dsmr.compute_ncc
 * (:102-117) scans around (dx0, dy0): shift s = (dy - dy0 + r) (2r + 1) + (dx - dx0 + r), dy outer and dx inner as upstream.
 * A finite cell z has the quantum q = rint((z - pivot) 2^k), a float64 subtraction, an exact scaling and a round to nearest
 * even; with pivot = floor(min) and span 2^k <= 2^20 (the caller's choice) 0 <= q <= 2^20.  A finite cell whose q falls outside
 * [0, 2^20] is treated as missing, and skipped[0] += the number of such cells of u and of v in rows [row0, row1) (each cell
 * once; only a wrong pivot / k makes any).  sums: int64 [(2r + 1)^2][6] the CALLER zeroes, += (N, Su, Sv, Suu, Svv, Suv) = the
 * sums of 1, qu, qv, qu^2, qv^2, qu qv over the cells (j, i) of u with row0 <= j < row1 where qu and qv = q(v[j + dy][i + dx]) both
 * exist (v in range and finite).  With at most 2^22 cells a sum of q^2 <= 2^40 stays below 2^63.  The correlation
 * (N Suv - Su Sv) / sqrt((N Suu - Su^2) (N Svv - Sv^2)) and the z offset (Su - Sv) / (N 2^k) are the host's, in exact integers.
 * Row ranges that partition [0, H) add up, over launches or devices, to the single launch's integers.
 *
 * bn_dsm_shift_diff: replaces dsmr.apply_shift_ (:138-149; a = 1, and its loop variable shadows the coefficient c, so the c i + d j
 * terms are zero) and `diff = pred_rdsm - gt_dsm` (sat_utils.py:246), the nanmean of :340 and MaskDoD (:278-297, :344-345).
 * pred, gt: float32 [H][W].  rdsm[j][i] = (float)((double)pred[j + dy][i + dx] + b), NaN where that cell is out of range;
 * diff = (float)((double)rdsm - (double)gt), the float32 subtraction bit for bit; both float32 [H][W], nullable.  mask: uint8
 * [H][W], nonzero = inside; NULL: every cell is inside.  sums6: int64 [6] the CALLER zeroes, += {sum, count} over all cells, the
 * inside cells and the outside cells, sum of llrint(|diff| 2^20); cells whose diff is NaN are left out, and so is a |diff| of
 * 2^21 m or more (an infinity included), which the sum could not hold.
 *
 * Refused (BN_EINVAL): NULL pointers (rdsm, diff and mask may be NULL), H or W < 1, more than 2^22 cells, r outside
 * [0, BN_NCC_MAX_RANGE], k outside [0, BN_NCC_MAX_SCALE], rows outside [0, H], a pivot or b that is not finite, |dx| or |dy|
 * above 2^20. */
#define BN_NCC_MAX_RANGE 8
#define BN_NCC_MAX_SCALE 16
#define BN_NCC_MAX_SHIFT (1 << 20)
#define BN_NCC_MAX_CELLS ((int64_t)1 << 22)
int bn_grid_halve(const double *src, int32_t H, int32_t W, double *dst, void *stream);
int bn_ncc_moments(const double *u, const double *v, int32_t H, int32_t W, double pivot, int32_t k, int32_t dx0, int32_t dy0, int32_t r,
                   int32_t row0, int32_t row1, long long *sums, long long *skipped, void *stream);
int bn_dsm_shift_diff(const float *pred, const float *gt, int32_t H, int32_t W, int32_t dx, int32_t dy, double b, const uint8_t *mask,
                      float *rdsm, float *diff, long long *sums6, void *stream);
/* The hole filling of a DSM (additive to ABI 7): quickly_interpolate_nans_from_singlechannel_img (eval.py:107-133; scipy's
 * griddata(method='nearest') over a k-d tree of every known cell) as save_dsm_grid (:135-149) applies it to write the *_Grid.tif,
 * as two launches in integers: an exact Euclidean distance transform with its feature map.
 *
 * THE RULE.  u: float32 [H][W].  A cell is a HOLE if and only if it is NaN (any payload; np.isnan is upstream's test, so +-inf is
 * a known value and is copied like any other).  The source of a hole (j, i) is the known cell (j', i') that minimises the integer
 * triple (d2, j', i') lexicographically, d2 = (j - j')^2 + (i - i')^2: the nearest known cell by exact squared Euclidean distance,
 * and among equidistant ones the one with the lowest row-major index.  A known cell is its own source, d2 = 0.  The output cell
 * is the source cell's 32 bits, copied without any arithmetic: -0.0, denormals, +-inf and the known cells keep their bits.
 * The tie rule is this project's: scipy's k-d tree breaks ties by its traversal order, which nobody can state (on a tie upstream
 * returns the value of SOME known cell at the minimal d2).
 *
 * bn_grid_nearest_col: near_row int32 [H][W]; near_row[j][i] = the row j' of the known cell of COLUMN i that minimises
 * (|j - j'|, j'), or -1 if the column has no known cell.  One lane per column, one sweep down and one sweep up.
 *
 * bn_grid_fill: for the cells of rows [row0, row1) the minimum of (dx^2 + dy^2, near_row[j][i'], i') over the columns i' with
 * near_row[j][i'] >= 0, dx = i - i', dy = j - near_row[j][i'].  That is the rule's minimiser: within one column d2 is minimal
 * exactly where |dy| is, and the column pass has resolved that column's ties towards the smaller row.  near_row must be
 * bn_grid_nearest_col's output for the same src.  It writes, in rows [row0, row1) only (other rows are not touched):
 *   dst     float32 [H][W]             the source cell's bits
 *   source  int32 [H][W] (nullable)    the flat index j' W + i'
 *   dist2   int32 [H][W] (nullable)    d2; with H, W <= BN_FILL_MAX_SIDE, d2 < 2^27
 *   counts  int64 [2] (nullable)       the CALLER zeroes; [0] += the holes of the rows (an integer add), [1] = max([1], largest
 *                                      d2 of the rows) (an integer max): row ranges that partition [0, H) add and max, over
 *                                      launches or devices, to the single launch's
 * On a grid WITHOUT a known cell every cell keeps its bits, source and dist2 are -1 and counts[1] is left alone (the Python
 * layer refuses such a grid, as upstream's griddata raises on it).
 * COST: the row pass scans outwards from a cell's own column and stops a side once dx^2 > best d2, so it is bounded by the
 * distance to the nearest known cell: a dense DSM with holes of a few cells costs a few LDS reads per cell, a grid with a single
 * known cell W reads per cell.  That is accepted, not defended: the splat leaves holes of a few cells.
 * Refused (BN_EINVAL): NULL src, near_row or dst, H or W < 1 or > BN_FILL_MAX_SIDE, rows outside [0, H] or row0 > row1. */
#define BN_FILL_MAX_SIDE 8192
int bn_grid_nearest_col(const float *src, int32_t H, int32_t W, int32_t *near_row, void *stream);
int bn_grid_fill(const float *src, const int32_t *near_row, int32_t H, int32_t W, int32_t row0, int32_t row1, float *dst, int32_t *source,
                 int32_t *dist2, long long *counts, void *stream);
/* The validation maps of a rendered view (additive to ABI 7): what eval.py:403-456 and main.py:451-595 build from the per-sample
 * dict of a whole view - the host np.argmin, the Python double loop of train_utils.get_surface_feature, calc_depth_std,
 * visualize_accumulated_feature's sum, check_vec0, NormalRegLoss's percentage, calc_normal_from_pts3d - as reductions of one
 * chunk of rays while it is on the device.
 *
 * bn_ray_maps.  z, w: float32 [R][S], the depth-sorted sample depths and their weights; depth: float32 [R].  X (nullable with
 * E == 0): a per-sample float32 tensor of E channels, element (r, s, e) at X[r x_ray + s x_sample + e x_chan] (a column slice of
 * the field rows is read in place).  normal_col: the first of three channels of X that hold a normal, or -1; view: float32, the
 * view vector of ray r (-rays_d) at view[r view_stride + 0..2].  A NULL output is not computed.  Per ray r:
 *   surf_idx int32 [R]   dev_s = fabsf(z_s - depth) in float32 (one rounding, then the sign cleared: torch.abs(z - depth)); the
 *                        first s whose dev_s is NaN; without one the first s that attains the minimum.  That is np.argmin
 *                        (eval.py:411-412) on every input, ties included.
 *   surf float32 [R][E]  the 32 bits of X[r][surf_idx][e], copied without arithmetic (-0.0, denormals and NaN payloads keep
 *                        their bits): get_surface_feature.
 *   var, std float32 [R] v = 0.0 in float64; for s ascending t = (double)z_s - (double)depth, v = v + (t t) (double)w_s, every
 *                        operation rounded on its own; var = (float)v, std = (float)sqrt(v): calc_depth_std_2, calc_depth_std.
 *                        The order is serial per ray: the bits depend on no split.
 *   accum float32 [R][E] a = 0.0 in float64; for s ascending a = a + (double)w_s (double)X[r][s][e] (the product of two float32
 *                        values is exact in float64); accum = (float)a: the Accum=True rule of visualize_accumulated_feature.
 * counters: int64 [6] the CALLER zeroes; integer adds only, one atomic per counter and block, so their values do not depend on
 * the block order, on how the rays are chunked or on the number of devices that share a view:
 *   [0] std_sum     += llrint((double)std 2^20) over the rays whose std is finite and below 2^40
 *   [1] std_count   += those rays           [2] std_skipped += the other rays (NaN or inf: a NaN weight, a negative variance)
 *   with a normal column n = X[r][s][normal_col + 0..2], per sample, in float64:
 *   [3] bad_nr      += 1 where ((n.x v.x + n.y v.y) + n.z v.z) < 0, the products formed first (NormalRegLoss's perc_ng_nr; a NaN
 *                      dot product is not counted, as `n_dot_v < 0` is false on it)
 *   [4] nr0         += 1 where sqrt((n.x n.x + n.y n.y) + n.z n.z) > 0.99999 is FALSE (check_vec0; a NaN norm is counted, as
 *                      torch.where(norm > 0.99999, 1, 0) gives 0 on it)
 *   [5] nr_total    += S per ray
 * The mean std of a view is counters[0] / (counters[1] 2^20), the percentages 100 counters[3 or 4] / counters[5].
 * Refused (BN_EINVAL): NULL z, w, depth or counters; R < 0 or over 2^30; S < 1 or > BN_MAPS_MAX_SAMPLES; E outside [0, BN_MAPS_MAX_CHANNELS];
 * E > 0 without X; surf or accum with E == 0; a normal column outside [0, E - 3] (other than -1) or without view; a negative
 * stride.  R == 0 launches nothing.
 *
 * bn_point_normals: calc_normal_from_pts3d (sat_utils.py:16-50) for an image of points; bn_grid_normals is its special case
 * P = (c resolution, r resolution, z) and shares the float64 chain per cell (its comment above states it).  points: float64
 * [H][W][3].  round_f32 = 1: every coordinate is first rounded to float32 - the `.type(torch.FloatTensor)` of
 * calc_normal_from_depth_v2 (datasets/satellite_rgb_dep.py:581), which at a UTM northing of 3.3e6 m quantises to 0.25 m - and
 * the chain then runs in float64 on the rounded points; round_f32 = 0 is the exact reading.  The four neighbour vectors
 * P(r + 1, c) - P, P(r - 1, c) - P, P(r, c + 1) - P, P(r, c - 1) - P are formed in float64, then as bn_grid_normals.  normals: float32
 * [H][W][3], (0, 0, 0) on the border, NaN where a NaN coordinate is read.  The cross product is over the coordinate axis always:
 * upstream's torch.cross without dim takes the FIRST axis of size 3 and so goes wrong when H - 2 == 3 or W - 2 == 3; that quirk
 * is not reproduced.  valid_in float32 [H][W] with valid_out float32 [H][W] (both or neither), the rule of :19-24 in float32:
 * valid_out = valid_in where valid_in < 1e-5f, else 1; an interior cell instead ((v(r + 1, c) v(r - 1, c)) v(r, c + 1)) v(r, c - 1).
 * Refused (BN_EINVAL): NULL points or normals, H or W < 1, H W over 2^30, round_f32 other than 0 or 1, one of valid_in /
 * valid_out without the other. */
#define BN_MAPS_MAX_SAMPLES 4096
#define BN_MAPS_MAX_CHANNELS 64
int bn_ray_maps(const float *z, const float *w, const float *depth, const float *X, int64_t x_ray, int64_t x_sample, int64_t x_chan,
                int32_t normal_col, const float *view, int64_t view_stride, int64_t R, int32_t S, int32_t E, int32_t *surf_idx,
                float *surf, float *var, float *std, float *accum, long long *counters, void *stream);
int bn_point_normals(const double *points, int32_t H, int32_t W, int32_t round_f32, const float *valid_in, float *normals,
                     float *valid_out, void *stream);
/* The rays of a satellite view from its RPC camera model (additive to ABI 7): get_rays, normalize_rays and the localisation they
 * call (datasets/satellite_rgb_dep.py:23-78, 550-559), per pixel, in float64 with EVERY operation rounded on its own (camera.hip
 * is compiled with fp contraction off).  Only + - x / and sqrt occur up to the geodetic point; both are correctly rounded on the
 * device, so that part is a pure function of its inputs and is held to a numpy statement bit for bit.
 *
 * The descriptor: 90 doubles, the keys of the `rpc` dictionary of a scene's JSON.  The 20 coefficients of a polynomial follow
 * the RPC00B order; with L, P, H the normalised longitude, latitude and altitude the monomials are, each product formed left
 * to right as written:
 *   m0 = 1      m1 = L        m2 = P        m3 = H        m4 = L P      m5 = L H      m6 = P H      m7 = L L      m8 = P P
 *   m9 = H H    m10 = (P L) H m11 = m7 L    m12 = m4 P    m13 = m5 H    m14 = m7 P    m15 = m8 P    m16 = m6 H    m17 = m7 H
 *   m18 = m8 H  m19 = m9 H
 * A polynomial is s = c0; s = s + c_k m_k for k = 1 .. 19 ascending.  This is the public RPC00B definition; it was not checked
 * against the rpcm package.
 * 1. normalise    L = (lon - lon_offset) / lon_scale, P = (lat - lat_offset) / lat_scale, H = (alt - alt_offset) / alt_scale
 * 2. project      col = (col_num.m / col_den.m) col_scale + col_offset ; row likewise
 * 3. localise     pixel (col, row) at altitude alt: cn = (col - col_offset) / col_scale, rn = (row - row_offset) / row_scale,
 *                 (L, P) = (0, 0), then BN_RPC_NEWTON_ITERS times, without a data-dependent exit:
 *                   N, D the numerator and denominator of col, N_L, N_P, D_L, D_P their derivatives, formed from
 *                     d m / d L: m1: 1, m4: P, m5: H, m7: 2 L, m10: m6, m11: 3 m7, m12: m8, m13: m9, m14: 2 m4, m17: 2 m5
 *                     d m / d P: m2: 1, m4: L, m6: H, m8: 2 P, m10: m5, m12: 2 m4, m14: m7, m15: 3 m8, m16: m9, m18: 2 m6
 *                   as s = c_k of the term whose derivative is 1, then s = s + c_k (d m_k) for the other terms, k ascending;
 *                   fc = N / D - cn ; a = (N_L D - N D_L) / (D D) ; b = (N_P D - N D_P) / (D D) ; fr, c, d the same for the row;
 *                   det = a d - b c ; L = L - (fc d - b fr) / det ; P = P - (a fr - fc c) / det
 *                 lon = L lon_scale + lon_offset, lat = P lat_scale + lat_offset.  A pixel for which det == 0 in one of the
 *                 iterations, or whose lon or lat is not finite, gives (NaN, NaN) and is counted.
 * 4. world        cs BN_CS_ECEF: sat_utils.latlon_to_ecef_custom (:110-125) as written there: rlat = lat (pi / 180), rlon
 *                 likewise, v = a / sqrt(1 - (e2 sin rlat) sin rlat), x = ((v + alt) cos rlat) cos rlon, y = ((v + alt) cos rlat)
 *                 sin rlon, z = (v (1 - e2) + alt) sin rlat.
 *                 cs BN_CS_UTM: the Krueger series to n^6 (Karney 2011, eq. 35) on WGS84, k0 = 0.9996, false easting 500000,
 *                 central meridian 6 zone - 183; with t = sinh(e atanh(e sin rlat)), tau = sin rlat / cos rlat, tau' = tau sqrt(1 + t t) -
 *                 t sqrt(1 + tau tau): xi' = atan2(tau', cos dlon), eta' = atanh(sin dlon / sqrt(1 + tau' tau')), and the six
 *                 terms alpha_j sin(2 j (xi' + i eta')) summed by the angle-addition recurrence from sin / cos of 2 xi' and sinh /
 *                 cosh of 2 eta'.  x = 500000 + k0 A eta, y = k0 A xi (+ 10,000,000 with south = 1), z = alt.  The zone is a
 *                 parameter of the scene (upstream takes it from the first pixel of each call, sat_utils.py:156-159).  The
 *                 device's float64 sin, cos, atanh, sinh, cosh and atan2 are not bit-specified: this step is held to the
 *                 numpy statement within 1e-6 m, not bit for bit.  Not checked against pyproj.
 * 5. ray          near = world point at max_alt, far = world point at min_alt ; d = far - near ; len = sqrt((d.x d.x + d.y d.y) +
 *                 d.z d.z) ; dir = d / len.  round_f32 = 1 (upstream, :76-77 then :550-559): o32 = (float)near, the row is
 *                 ((o32 - (float)center) / (float)range, (float)dir, 0, (float)len / (float)range), the subtraction and the
 *                 divisions in float32 - at a UTM northing of 3.3e6 m the origin is on a 0.25 m lattice.  round_f32 = 0: the
 *                 row is ((float)((near - center) / range), (float)dir, 0, (float)(len / range)), formed in float64.
 *                 sun (HOST pointer, 3 floats, nullable): columns 8-10 of every row.  A ray whose near or far pixel is
 *                 counted by step 3, or one of whose eight values is not finite, has NaN in its columns 0-7 and is counted once.
 *
 * rpc is a HOST pointer.  Grid mode (cols == NULL): ray r of [r0, r1) is pixel (col r % W, row r / W).  Array mode: (cols[r],
 * rows[r]), float64 device arrays.  Outputs are indexed from r0: ray r writes row r - r0.  counts (device, the CALLER zeroes):
 * counts[0] += the counted rows, one integer atomic per block; no float atomic anywhere.
 *   bn_rpc_project   lon, lat, alt float64 [n] -> col, row float64 [n]  (step 2)
 *   bn_rpc_localize  alt: one altitude for all -> lonlat float64 [r1 - r0][2]  (step 3)
 *   bn_geo_world     lonlat float64 [n][2], alt -> xyz float64 [n][3]  (step 4)
 *   bn_rpc_rays      steps 1-5 in one launch: rays float32 [r1 - r0] rows of ray_stride >= 8 (11 with sun) floats; lonlat_near /
 *                    lonlat_far (nullable) float64 [r1 - r0][2], the geodetic points the rays were formed from.
 * Refused (BN_EINVAL): NULL rpc or outputs (counts included), one of cols / rows without the other, r0 < 0, r0 > r1, n < 0, more
 * than 2^30 rays, W < 1 in grid mode, another cs, zone outside [1, 60], south or round_f32 other than 0 or 1, a range that is
 * not positive and finite, a centre or altitude that is not finite, a scale of zero (or a non-finite scale or offset) in the
 * descriptor, a ray_stride below the columns written. */
#define BN_RPC_NEWTON_ITERS 8
enum { BN_CS_ECEF = 0, BN_CS_UTM = 1 };
typedef struct {
  double row_offset, col_offset, lat_offset, lon_offset, alt_offset, row_scale, col_scale, lat_scale, lon_scale, alt_scale;
  double row_num[20], row_den[20], col_num[20], col_den[20];
} bn_rpc;
int bn_rpc_project(const bn_rpc *rpc, const double *lon, const double *lat, const double *alt, int64_t n, double *col, double *row,
                   void *stream);
int bn_rpc_localize(const bn_rpc *rpc, const double *cols, const double *rows, int32_t W, int64_t r0, int64_t r1, double alt,
                    double *lonlat, unsigned long long *counts, void *stream);
int bn_geo_world(const double *lonlat, const double *alt, int64_t n, int32_t cs, int32_t zone, int32_t south, double *xyz,
                 void *stream);
int bn_rpc_rays(const bn_rpc *rpc, const double *cols, const double *rows, int32_t W, int64_t r0, int64_t r1, double min_alt,
                double max_alt, int32_t cs, int32_t zone, int32_t south, const double *center, double range, const float *sun,
                int32_t round_f32, float *rays, int64_t ray_stride, double *lonlat_near, double *lonlat_far,
                unsigned long long *counts, void *stream);
/* The depth priors of a view from its tie points (additive to ABI 7): load_depth_data (datasets/satellite_rgb_dep.py:401-548)
 * for one view, paired BY PIXEL.  Upstream pairs the k-th tie point with the k-th valid pixel in raster order (:474), which is the
 * pixel pairing only for a file sorted row-major without repeats; here a tie point belongs to the pixel it names.  One lane per
 * tie point in both launches; camera.hip is compiled with fp contraction off, every operation below is rounded on its own.
 *
 * bn_tie_owner: px int32 [T][2] as (col, row) at FULL resolution; owner int32 [H][W], the CALLER fills it with -1.
 *   A tie point outside [0, W) x [0, H) is left out and counts[0] (outside) += 1.  Otherwise atomicMax(owner[row W + col], t):
 *   the HIGHEST index owns the pixel, whatever the order of arrival; a tie point that meets a value other than -1 adds 1 to
 *   counts[1] (duplicates), so the total is (ties inside) - (distinct pixels).  Integer atomics only, one per counter and block.
 * bn_tie_priors: for tie point t with owner[row W + col] == t only (every other lane does nothing):
 *   1. ray      step 5 above (the very device function bn_rpc_rays runs) at pixel (col / downscale, row / downscale), the
 *               division in float64; rpc is the view's descriptor ALREADY rescaled by the caller.  v[0..7] is the ray row.
 *   2. point    P = pts3d[t] float64 [3] in world units.  round_f32 = 1 (:456-463): p = ((float)P - (float)center) / (float)range
 *               per axis, in float32; round_f32 = 0: p = (float)((P - center) / range), formed in float64.
 *   3. depth    t = p - (v0, v1, v2) in float32 ; depth = sqrtf((t.x t.x + t.y t.y) + t.z t.z)
 *   4. weight   cn = ((correl[t] - cmin) / (cmax - cmin)) corrscale in float64 (:433-436) ; w = (float)cn * (-v5), the
 *               product with the nadir (0, 0, -1) of :479-492
 *   5. std      s = (float)stdscale * (1.0f - w) + (float)margin, left to right in float32 (:498) ; depth_std = s *
 *               (float)std_span.  std_span is upstream's depth_max - depth_min, the literal 0 of :407-408, 539.
 *   6. skipped  a tie point whose ray is counted by step 5, or whose p, depth, w or s is not finite, writes nothing but
 *               tie_rays (NaN) and counts[2] (skipped) += 1: its pixel stays invalid.
 *   7. placing  points float32 [H][W][3] = p and valid_full float32 [H][W] = 1 at the tie point's own pixel (both nullable; the
 *               input of the normals).  The output pixel is (dst_row[row], dst_col[col]): int32 vectors of H and W entries
 *               from the host, -1 where the resize samples no such line; NULL is the identity (then Hout == H, Wout == W).
 *               A tie point whose line is not sampled (or whose entry is outside the output) adds 1 to counts[3] (unsampled);
 *               otherwise valid float32 [Hout][Wout] = 1, depths float32 [Hout][Wout][2] = (depth, w), depth_std [Hout][Wout],
 *               rays float32 [Hout][Wout][8] = v (upstream's all_deprays).  No float index arithmetic runs on the device.
 *   All outputs but valid are nullable, and the CALLER zero-fills them.  tie_rays float32 [T][8] (nullable): v of every owner
 *   tie point (NaN where its ray is counted); rows of the other tie points are not written.
 *   counts: int64 [4] = (outside, duplicates, skipped, unsampled), the CALLER zeroes; bn_tie_owner adds to [0] and [1],
 *   bn_tie_priors to [2] and [3].
 * Refused (BN_EINVAL): NULL rpc, px, owner, pts3d, correl, center, valid or counts; T < 0 or over 2^30; H, W, Hout or Wout < 1;
 * H W over 2^31; Hout != H without dst_row, Wout != W without dst_col; a downscale that is not finite or below 1; a cmin, cmax,
 * corrscale, stdscale, margin or std_span that is not finite; cmax <= cmin; another cs, zone outside [1, 60], south or
 * round_f32 other than 0 or 1; a range that is not positive and finite; a centre or altitude that is not finite; a scale of
 * zero (or a non-finite entry) in the descriptor.  T == 0 launches nothing. */
int bn_tie_owner(const int32_t *px, int32_t T, int32_t H, int32_t W, int32_t *owner, unsigned long long *counts, void *stream);
int bn_tie_priors(const bn_rpc *rpc, const int32_t *px, const int32_t *owner, const double *pts3d, const double *correl, int32_t T,
                  int32_t H, int32_t W, int32_t Hout, int32_t Wout, const int32_t *dst_row, const int32_t *dst_col,
                  double downscale, double min_alt, double max_alt, int32_t cs, int32_t zone, int32_t south, const double *center,
                  double range, int32_t round_f32, double cmin, double cmax, double corrscale, double stdscale, double margin,
                  double std_span, float *valid, float *depths, float *depth_std, float *rays, float *points, float *valid_full,
                  float *tie_rays, unsigned long long *counts, void *stream);
/* World points of an ECEF scene (additive to ABI 7): what takes a point of a scene whose world coordinates are ECEF to (east,
 * north, altitude), so that the surface model - bn_dsm_splat's accumulator, the altitude image, the altitude MAE - is served for
 * such a scene as it is for a UTM one.  The reference does it on the host: sat_utils.ecef_to_latlon_custom (sat_utils.py:127-146),
 * Bowring's one-step formula, then utm_from_latlon through pyproj (datasets/satellite_rgb_dep.py:629-631).  world.hip and the
 * geodesy.h it shares with camera.hip are compiled with fp contraction off: all of it is float64 and every operation is rounded
 * on its own.  The constants are formed on the host exactly as upstream forms them, with its TRUNCATED eccentricity - not the one
 * of step 4 above (f = 1 / 298.257223563; the two differ by 6e-15 relative, which moves no output by more than 4e-9 m).  Geodetic
 * -> ECEF -> geodetic does not close: the single step leaves 7.2e-7 m in latitude, 4.6e-9 m in longitude and 8.6e-7 m in altitude
 * over |lat| <= 80 degrees and altitudes of -500 to 9000 m.  Upstream's rule is reproduced as written; no exact variant is served.
 *   a = 6378137.0 ; e = 8.1819190842622e-2 ; asq = a a ; esq = e e
 *   b = sqrt(asq (1 - esq)) ; bsq = b b ; ep = sqrt((asq - bsq) / bsq)
 *   k1 = (ep ep) b ; k2 = esq a
 *   p   = sqrt(x x + y y)
 *   th  = atan2(a z, b p) ; s = sin(th) ; c = cos(th)
 *   lon = atan2(y, x)
 *   lat = atan2(z + k1 ((s s) s), p - k2 ((c c) c))
 *   sl  = sin(lat) ; N = a / sqrt(1 - esq (sl sl))
 *   alt = p / cos(lat) - N
 *   lon_deg = lon 180 / pi ; lat_deg = lat 180 / pi          (left to right)
 *   (east, north) = the UTM series of step 4 above at (lon_deg, lat_deg), zone, south ; z = alt
 * Upstream writes the cubes as np.sin(th) ** 3, a pow; (s s) s differs from it by roundings only (at most 3.2e-9 m in latitude and
 * 7.5e-9 m in altitude over |lat| <= 80 degrees, the longitude is equal).  The zone is a parameter of the scene, as in step 4;
 * south = 0 adds no false northing.  The device's float64 atan2, sin and cos are not bit-specified: as for bn_geo_world the
 * results are held to the numpy statement within 1e-6 m, not to bits.
 * A point is REFUSED - it gives NaN, deposits nothing and is counted in skipped[0] - when p == 0 (on the axis), or when x, y, z,
 * lat, alt, east or north is not finite; where it is deposited into a DSM also when |alt| >= 2^23 m, bn_dsm_splat's rule.
 * upstream's get_dsm_from_nerf_prediction converts an ECEF cloud TWICE (:649-651 runs utm_from_latlon on what :629-631 already
 * returned as easts and norths); this project converts once, the reading eval.py:170 takes for the altitude image.
 *
 *   bn_ecef_geodetic     xyz float64 [n][3] -> lonlat float64 [n][2] in degrees, alt float64 [n]: the inverse alone, the
 *                        counterpart of bn_geo_world with cs = BN_CS_ECEF.
 *   bn_surface_points    P = (o + d depth) range + center, formed as bn_dsm_splat forms it; cs = BN_CS_ECEF: P through the rule;
 *                        cs = BN_CS_UTM: P as it is.  enz float64 [R][3] = (east, north, altitude), a refused row is NaN.
 *   bn_dsm_splat_points  the cell, footprint and deposit of bn_dsm_splat for n given points: enz float64 rows of stride >= 3
 *                        doubles = (east, north, altitude).  Covers the tie points of a view (datasets/cal_rmse_depth.py:15-64).
 *   bn_dsm_splat_world   bn_dsm_splat's arguments and (cs, zone, south): ray -> world point -> deposit in ONE launch, no cloud
 *                        in between.  It runs the very device functions of the two entries above, so its accumulator is
 *                        theirs bit for bit; for cs = BN_CS_UTM it is bn_dsm_splat's bit for bit.
 * One lane per ray or point.  acc and skipped as in bn_dsm_splat (the CALLER zeroes them; calls accumulate); skipped[0] is summed
 * per block and added with ONE integer atomic.  Integer atomics only: no float atomic.
 * Refused (BN_EINVAL): NULL pointers, a negative count, ray_stride < 6 or stride < 3, another cs, zone outside [1, 60] (read for
 * cs = BN_CS_UTM too), south other than 0 or 1, a non-finite frame or grid origin, and the grid, radius and footprint refusals of
 * bn_dsm_splat. */
int bn_ecef_geodetic(const double *xyz, int64_t n, double *lonlat, double *alt, unsigned long long *skipped, void *stream);
int bn_surface_points(const float *rays, int64_t ray_stride, const float *depth, int64_t R, const double *center, double range,
                      int32_t cs, int32_t zone, int32_t south, double *enz, unsigned long long *skipped, void *stream);
int bn_dsm_splat_points(const double *enz, int64_t stride, int64_t n, double xoff, double yoff, double resolution, int32_t W, int32_t H,
                        int32_t radius, int32_t footprint, long long *acc, unsigned long long *skipped, void *stream);
int bn_dsm_splat_world(const float *rays, int64_t ray_stride, const float *depth, int64_t R, const double *center, double range,
                       double xoff, double yoff, double resolution, int32_t W, int32_t H, int32_t radius, int32_t footprint, int32_t cs,
                       int32_t zone, int32_t south, long long *acc, unsigned long long *skipped, void *stream);
/* Orthorectified maps of a view (additive to ABI 7): the ray-level maps of a view (rgb, albedo, normals, BRDF parameters) splatted
 * into the grid of the DSM, channel by channel, so that they lie on the DSM's cells and fuse over views as it does.  The feature
 * channels have NO upstream counterpart - the reference rasterises the altitude alone (plyflatten, datasets/satellite_rgb_dep.py:
 * 636-699) - so the rule below is this project's own and there is nothing to check it against but its statement.  Its altitude
 * part IS bn_dsm_splat's rule: the point p, the cell (j, i), the footprint, the skip rule of a bad point (p not finite or
 * |p.z| >= 2^23 m; cs = BN_CS_ECEF: also what bn_dsm_splat_world refuses) and q = llrint(p.z 2^20) are exactly those of
 * bn_dsm_splat, for cs = BN_CS_ECEF those of bn_dsm_splat_world - the same device functions, float64, every operation rounded on
 * its own, no fused multiply-add.  An oblique view reaches a cell along a building's edge at several heights (roof, facade,
 * ground); the mean that is right for the altitude mixes their colours, hence the optional top-surface pass.
 *
 * bn_ortho_top (pass 1, top mode only): top int64 [H][W], which the CALLER fills with BN_ORTHO_EMPTY = INT64_MIN.  Every
 *   footprint cell of a ray inside the grid takes top = max(top, q), a signed 64-bit integer atomic max.  A bad point adds 1 to
 *   skipped[0].  Arguments as bn_dsm_splat_world.
 * bn_ortho_splat (pass 2): the arguments of bn_dsm_splat_world and
 *     features  float32 [R] rows of E channels, row stride feature_stride >= E floats, unit channel stride (NULL with E == 0)
 *     E         channels, in [0, BN_ORTHO_MAX_CHANNELS]
 *     top       the finished grid of pass 1, or NULL (mean mode)
 *     band_q    int64 >= 0, in units of 2^-20 m (a value above 2^62 acts as 2^62: |q| <= 2^43, so every band from 2^44 keeps all)
 *     acc       int64 [H][W][2 + E] = (sum_z, count, sum_0 .. sum_{E-1}) per cell, 16-byte aligned, which the CALLER zeroes; calls
 *               accumulate into it
 *     counters  uint64 [3] = (bad points, bad features, culled deposits), which the caller zeroes
 *   Per ray: a bad point deposits nothing and adds 1 to counters[0].  Otherwise f_e = llrint((double)x_e 2^24) for each channel; a
 *   ray with any x_e that is not finite or has |x_e| >= 2^16 deposits nothing and adds 1 to counters[1] (a ray with a bad point AND
 *   a bad feature counts as a bad point only).  Then |f_e| <= 2^40: a cell's sum cannot overflow below 2^22 points.
 *   For each footprint cell inside the grid, tested cell by cell on its own:
 *     if top is given and q + band_q < top[cell]: the cell gets nothing from this ray and counters[2] gains 1 (the comparison is
 *       written this way so that an EMPTY cell passes everything and nothing overflows);
 *     otherwise sum_z += q, count += 1, sum_e += f_e, all integer atomic adds (two's complement).
 *   There is no float atomic in this path; each counter goes out as one integer atomic per block.
 * bn_ortho_resolve: maps [E][H][W], maps[e] = (float)((double)sum_e / (double)count 2^-24); dsm [H][W] as bn_dsm_resolve gives it;
 *   a cell with count == 0 is NaN in all of them; count [H][W] int32 (nullable), saturating at 2^31 - 1.
 *
 * Consequences.  With E == 0 and top == NULL acc is bn_dsm_splat's accumulator bit for bit (bn_dsm_splat_world's for
 * cs = BN_CS_ECEF).  Every output bit depends on the SET of rays alone - not on their order, on how they are split over calls,
 * views or devices (top merges by a MAX, acc and the counters by a SUM all-reduce) - provided pass 1 has seen every ray before
 * pass 2 starts.  top == NULL is the mean over all points of a cell; top mode with a band of b metres (band_q = llrint(b 2^20))
 * keeps, per cell, the points within b of the highest point that reaches that cell.  The mean of unit normals is not a unit
 * vector and is not renormalised.
 * Refused (BN_EINVAL, nothing launched, buffers untouched): NULL required pointers, E outside [0, BN_ORTHO_MAX_CHANNELS],
 * feature_stride < E, band_q < 0, E > 0 without features (maps in bn_ortho_resolve), acc not 16-byte aligned, and everything
 * bn_dsm_splat_world refuses. */
#define BN_ORTHO_MAX_CHANNELS 32
#define BN_ORTHO_EMPTY INT64_MIN
int bn_ortho_top(const float *rays, int64_t ray_stride, const float *depth, int64_t R, const double *center, double range, double xoff,
                 double yoff, double resolution, int32_t W, int32_t H, int32_t radius, int32_t footprint, int32_t cs, int32_t zone,
                 int32_t south, long long *top, unsigned long long *skipped, void *stream);
int bn_ortho_splat(const float *rays, int64_t ray_stride, const float *depth, int64_t R, const double *center, double range,
                   double xoff, double yoff, double resolution, int32_t W, int32_t H, int32_t radius, int32_t footprint, int32_t cs,
                   int32_t zone, int32_t south, const float *features, int64_t feature_stride, int32_t E, const long long *top,
                   long long band_q, long long *acc, unsigned long long *counters, void *stream);
int bn_ortho_resolve(const long long *acc, int32_t W, int32_t H, int32_t E, float *maps, float *dsm, int32_t *count, void *stream);
/* Visibility over a surface model (additive to ABI 7): from a start on or above a height grid, march along a direction and report
 * whether some cell rises above the ray.  With a sun direction that is the shadow mask of the grid (or of a view's surface
 * points), with the direction towards the sensor the view's occlusion mask.  There is NO upstream counterpart - the reference
 * never computes a geometric shadow - so the rule is this project's own and there is nothing to check it against but its statement.
 *
 * Grid.  dsm is float32 [H][W], north-up (the Grid of the DSM entries): cell (j, i) covers east [xoff + i res, xoff + (i + 1) res),
 *   row 0 is the northern edge.
 * Direction.  d = (dx, dy, dz), float64 (east, north, up), pointing FROM the surface TOWARDS the sun or the sensor; it need not be
 *   normalised.  dirs is [K][3] in HOST memory: the entries read and check every direction before the first launch.
 * Everything below is float64 and every operation is rounded on its own (no fused multiply-add).
 * Start.  Grid mode: cell (j, i) starts at u0 = i + 0.5, v0 = j + 0.5, z0 = (double)dsm[j][i].  Point mode: a point (e, n, a)
 *   starts at u0 = (e - xoff) / res, v0 = (yoff - n) / res, z0 = a (bn_dsm_splat's two quotients without the floor).  A start
 *   that is NaN in z0 or not finite in any coordinate is BN_VIS_NODATA; so is a point-mode start with
 *   !(u0 >= 0 && u0 < W && v0 >= 0 && v0 < H).
 * Slope.  a = fmax(fabs(dx), fabs(dy)).  a == 0 (the zenith): every start with data is BN_VIS_VISIBLE.  Otherwise su = dx / a,
 *   sv = -(dy / a), sz = (dz / a) * res: one of su, sv is exactly +-1, so a step crosses exactly one cell along the dominant axis.
 *   The start cell itself is never tested.
 * March.  For t = 1, 2, ...:
 *     ut = u0 + (double)t * su ;  vt = v0 + (double)t * sv ;  zt = z0 + (double)t * sz      (the product with t, never a running sum)
 *     if !(ut >= 0 && ut < W && vt >= 0 && vt < H): the start is BN_VIS_VISIBLE, stop
 *     h = (double)dsm[(int)floor(vt)][(int)floor(ut)]
 *     if h > zt + eps: the start is BN_VIS_BLOCKED and hit = that cell's flat index floor(vt) W + floor(ut), stop
 *   The comparison is strict (h == zt + eps does not block) and false for a NaN cell, which therefore never blocks; +inf blocks,
 *   -inf never does.  The march ends after at most max(W, H) steps (by then the dominant axis has left the grid): visible.
 * zmax is an optimisation argument: a kernel may declare a start visible as soon as zt > zmax.  With eps >= 0 and zmax >= every
 *   non-NaN cell this cannot change a bit (h <= zmax < zt <= zt + eps); zmax = +inf is the plain rule.  A smaller zmax is the
 *   caller's error and is not detected.
 * Outputs.  vis uint8 [K][N] in {BN_VIS_BLOCKED, BN_VIS_VISIBLE, BN_VIS_NODATA}; hit int32 [K][N] (nullable): the flat index of the
 *   first blocking cell in ascending t, or -1; counts int64 [K][3] = (blocked, visible, nodata) over the starts of the call, which
 *   the CALLER zeroes and calls accumulate into, one integer atomic per counter and block.  There is no float atomic.  Every bit
 *   depends on the grid, the starts and the directions alone - not on blocks, on row bands, on how K is split over calls, or on
 *   the number of ranks (the counts of bands or ranks add up).
 * bn_grid_visibility: N = H W, the starts are the cells of rows [row0, row1); vis and hit are [K][H][W] and only the band's rows
 *   are written.  An empty band is accepted and launches nothing.
 * bn_points_visibility: N = R, enz float64 [R][3] = (east, north, altitude) on the device.  R == 0 launches nothing.
 * Refused (BN_EINVAL, nothing launched, buffers untouched): NULL dsm, dirs, vis, counts or enz; H or W < 1, or H W > 2^30; K outside
 * [1, BN_VIS_MAX_DIRS]; R < 0 or over 2^30; rows outside [0, H] or row0 > row1; res not positive and finite; a non-finite grid
 * origin; eps negative or not finite; a NaN zmax; a direction with a non-finite component or dz <= 0 (a sun below the horizon is
 * the caller's case, not a march). */
#define BN_VIS_BLOCKED 0
#define BN_VIS_VISIBLE 1
#define BN_VIS_NODATA 2
#define BN_VIS_MAX_DIRS 4096
int bn_grid_visibility(const float *dsm, int32_t H, int32_t W, double res, int32_t row0, int32_t row1, const double *dirs, int32_t K,
                       double eps, double zmax, uint8_t *vis, int32_t *hit, long long *counts, void *stream);
int bn_points_visibility(const double *enz, int64_t R, const float *dsm, int32_t H, int32_t W, double xoff, double yoff, double res,
                         const double *dirs, int32_t K, double eps, double zmax, uint8_t *vis, int32_t *hit, long long *counts,
                         void *stream);
/* Depth of a surface model along a ray (additive to ABI 7): at what depth does a view's ray meet a height grid?  The splats above
 * take a view to the ground and the march above runs between ground points; this takes the ground to a view: depth priors from a
 * lidar or an earlier DSM, a per-pixel ground truth of a rendered depth, any raster of the grid seen from the view (gather it
 * through `cell`).  There is NO upstream counterpart - the reference never intersects a ray with a raster - so the rule is this
 * project's own and there is nothing to check it against but its statement and the project's other rules.
 *
 * Grid.  dsm float32 [H][W], north-up, with xoff, yoff, res as in "Visibility over a surface model"; a cell is a flat-topped column.
 * Rays.  rays float32 [R] rows of ray_stride >= 8 floats: o[3], d[3], near, far.  Frame: center[3], range of a UTM scene (world axes
 *   east, north, up).
 * Everything below is float64 and every operation is rounded on its own (no fused multiply-add).
 * Point.  p(s) = ((double)o + (double)d * s) * range + center, per component: the expression of the DSM splats, so a cast depth fed
 *   back to them lands on the surface.
 * Segment.  P0 = p((double)near), P1 = p((double)far);  u = (P.x - xoff) / res, v = (yoff - P.y) / res, z = P.z for both ends;
 *   du = u1 - u0, dv = v1 - v0, dz = z1 - z0.  A ray with a non-finite one of u0, v0, z0, u1, v1, z1, or with
 *   fabs(du) + fabs(dv) > BN_CAST_MAX_SPAN, is BN_CAST_NODATA: depth = NaN, cell = -1, nan_cells = 0.
 * Walk.  An exact cell walk in the segment parameter lam in [0, 1]: (i, j) = (floor(u0), floor(v0)), lam_in = 0.  Per cell:
 *     lam_u = ((double)(du > 0 ? i + 1 : i) - u0) / du, or +inf when du == 0 ;  lam_v likewise from j, v0, dv
 *       (always from the INTEGER line index, never from a running sum)
 *     m = fmin(lam_u, lam_v) ;  lam_out = fmax(lam_in, fmin(m, 1.0))
 *   Test.  If 0 <= i < W and 0 <= j < H, h = (double)dsm[j][i].  A NaN h is never hit and is counted (nan_cells += 1).  Otherwise
 *     z_in = z0 + lam_in * dz ;  z_out = z0 + lam_out * dz
 *     if z_in <= h:        the ray meets the cell at lam = lam_in: BN_CAST_BELOW if this is the start cell, else BN_CAST_WALL
 *     else if z_out <= h:  BN_CAST_TOP at lam = fmax(lam_in, fmin((h - z0) / dz, lam_out))
 *     Both comparisons are <= (a ray that only touches a top at the cell's far edge meets it).  +inf always stops a ray, -inf never.
 *   Hit.  depth = (float)((double)near + lam * ((double)far - (double)near)), cell = j W + i, stop.
 *   No hit in this cell.  If m >= 1 the ray is BN_CAST_MISS (depth = NaN, cell = -1), stop.  Otherwise i moves by the sign of du if
 *     lam_u == m and j by the sign of dv if lam_v == m - BOTH on a tie, so a ray through a corner moves diagonally and the two
 *     cells that touch it only at the corner are not tested.  If then (i < 0 and du < 0) or (i >= W and du > 0), or likewise j, H
 *     and dv - outside the grid and moving away from it on that axis - the ray is BN_CAST_MISS, stop.  Then lam_in = lam_out.
 *   The walk crosses no line beyond the far end, so it ends after at most fabs(du) + fabs(dv) + 3 cells.
 * zmax is an optimisation argument, as in the visibility entries: with nan_cells == NULL a cell whose fmin(z_in, z_out) > zmax need
 *   not be loaded.  With zmax >= every non-NaN cell this cannot change a bit; zmax = +inf is the plain rule.  With nan_cells every
 *   cell of the walk inside the grid is loaded: a NaN cell counts wherever the ray passes it.  A smaller zmax is the caller's error.
 * Skipping.  The walk only visits cells between the two ends on either axis, so a ray whose ends are both west, east, north or
 *   south of the grid is BN_CAST_MISS with nan_cells = 0 without a walk; the cells outside the grid are walked without a load.
 * Outputs, plain stores of the lane's own ray: depth float32 [R]; state uint8 [R]; cell int32 [R] (nullable); nan_cells int32 [R]
 *   (nullable); counts int64 [5] += the rays of the call per state, in the order of the codes: the CALLER zeroes them, one integer
 *   atomic per class and block, no float atomic.  Every bit depends on the ray, the frame and the raster alone - not on blocks, on
 *   how the rays are cut into calls, or on the number of ranks (the counts of calls or ranks add up).  R == 0 launches nothing.
 * Refused (BN_EINVAL, nothing launched, buffers untouched): NULL rays, center, dsm, depth, state or counts; R < 0 or over 2^30; H or
 * W < 1, or H W > 2^30; ray_stride < 8; res or range not positive and finite; a non-finite centre or grid origin; a NaN zmax. */
#define BN_CAST_TOP 0
#define BN_CAST_WALL 1
#define BN_CAST_MISS 2
#define BN_CAST_NODATA 3
#define BN_CAST_BELOW 4
#define BN_CAST_MAX_SPAN 65536
int bn_cast_rays(const float *rays, int64_t ray_stride, int64_t R, const double *center, double range, const float *dsm, int32_t H,
                 int32_t W, double xoff, double yoff, double res, double zmax, float *depth, uint8_t *state, int32_t *cell,
                 int32_t *nan_cells, long long *counts, void *stream);
/* Horizon and sky view over a surface model (additive to ABI 7): from a start on or above a height grid, march along a horizontal
 * azimuth and keep the steepest slope met - the tangent of the horizon's elevation - then average cos^2 of that elevation over the
 * azimuths: the sky-view factor, the geometric counterpart of the `sky` term of the reference's irradiance
 * sun_v + (1 - sun_v) * sky (models/spsbrdfnerf.py:265-268) as the march of "Visibility over a surface model" is that of sun_v.  The
 * horizon table answers "is this start shadowed by a sun at elevation e" for every e at once: slope > tan e.  There is NO upstream
 * counterpart, so the rule is this project's own and there is nothing to check it against but its statement and the shadow march.
 *
 * Grid.  dsm float32 [H][W], north-up, NaN = no data, with xoff, yoff, res as in "Visibility over a surface model".
 * Azimuth.  (dx, dy), float64 (east, north): a horizontal vector, finite, not (0, 0), not necessarily normalised.  az is [D][2] in
 *   HOST memory: the entries read and check every azimuth before the first launch; the device evaluates no sin or cos.
 * Everything below is float64 and every operation is rounded on its own (no fused multiply-add).
 * Start.  Grid mode: cell (j, i) starts at u0 = i + 0.5, v0 = j + 0.5, z0 = (double)dsm[j][i].  Point mode: a point (e, n, a)
 *   starts at u0 = (e - xoff) / res, v0 = (yoff - n) / res, z0 = a.  A start that is not finite in any coordinate, or a point-mode
 *   start with !(u0 >= 0 && u0 < W && v0 >= 0 && v0 < H), has no data: slope = NaN, hit = -1.
 * Step.  a = fmax(fabs(dx), fabs(dy)) ;  su = dx / a ;  sv = -(dy / a) ;  L = sqrt(su * su + sv * sv) * res, the metres of ground
 *   per step.  One of su, sv is exactly +-1, as in the visibility march.
 * March.  best = 0.0, hit = -1.  For t = 1 .. min(max(W, H), max_steps):
 *     tt = (double)t ;  ut = u0 + tt * su ;  vt = v0 + tt * sv                      (the product with t, never a running sum)
 *     if !(ut >= 0 && ut < W && vt >= 0 && vt < H): stop
 *     run = tt * L
 *     if (zmax - z0) / run <= best: stop                                            (the early exit, see below)
 *     h = (double)dsm[(int)floor(vt)][(int)floor(ut)]
 *     s = (h - z0) / run
 *     if s > best: best = s and hit = that cell's flat index floor(vt) W + floor(ut)
 *   The comparison is strict and false for NaN: the first cell in ascending t wins a tie and a NaN cell never raises the horizon;
 *   +inf gives best = +inf, -inf never wins.  The start cell itself is never tested.
 *   slope = (float)best: the tangent of the horizon's elevation, floored at 0 - an open and level horizon beyond the grid's edge.
 * zmax is an optimisation argument.  If zmax >= every non-NaN cell the early exit cannot change a bit: rounded subtraction is
 *   monotone, so every later step has fl(h - z0) <= fl(zmax - z0); if fl(zmax - z0) <= 0 every later s <= 0 <= best; otherwise
 *   rounded division by a growing positive run is monotone too, so every later s is at most the bound just tested, hence at most
 *   best - and the update needs s strictly greater.  The argument holds at whatever step the test is made, so a kernel may make it
 *   at some steps only (csrc/horizon.hip tests once per batch of 8 steps, before the batch's loads go out).  zmax = +inf is the
 *   plain rule (inf / run <= best only once best is +inf, which nothing beats).  A smaller zmax is the caller's error and is not
 *   detected.
 * max_steps bounds the march in cells along the dominant axis: a square window around the start, not a disc.
 * Sky view.  D is the TOTAL number of azimuths; acc float64 [cells] is zeroed by the caller.  Per cell, for k ascending over the n
 *   planes of the call, one at a time:   s = (double)slope[k][c]   (the STORED float32, not best) ;  acc = acc + 1.0 / (1.0 + s * s)
 *   and with svf != NULL (the call of the last planes):   v = acc / (double)D ;  svf = (float)v.
 *   1 / (1 + tan^2) is cos^2 of the horizon's elevation and no transcendental is evaluated; a NaN slope makes svf NaN, an infinite
 *   one contributes exactly 0.  acc is observable: its bits fix the summation order whatever tiling of the azimuths a caller chooses.
 *   sums int64 [3] += (the sum of llrint(v 2^30) over the non-NaN v, their count, the NaN count) over [c0, c1): the CALLER zeroes
 *   them, block-reduced, one integer atomic per counter and block.  There is no float atomic.
 * Outputs.  slope float32 [D][N], hit int32 [D][N] (nullable), plain stores of the lane's own start: every bit depends on the grid,
 *   the starts and the azimuths alone - not on blocks, row bands, how D is split over calls, or the number of ranks.
 * bn_grid_horizon: N = H W, the starts are the cells of rows [row0, row1); only the band's rows are written.  An empty band is
 *   accepted and launches nothing.
 * bn_points_horizon: N = R, enz float64 [R][3] = (east, north, altitude) on the device.  R == 0 launches nothing.
 * bn_sky_view: slope holds n planes of `cells` floats; only cells [c0, c1) of acc and svf are read and written.  An empty range is
 *   accepted and launches nothing.
 * Refused (BN_EINVAL, nothing launched, buffers untouched): NULL dsm, az, slope, enz or acc; H or W < 1, or H W > 2^30; D or n outside
 * [1, BN_HORIZON_MAX_DIRS]; R < 0 or over 2^30; cells outside [1, 2^30]; rows outside [0, H] or row0 > row1; c0, c1 outside [0, cells] or
 * c0 > c1; res not positive and finite; a non-finite grid origin; max_steps < 1; a NaN zmax; an azimuth with a non-finite component
 * or both components zero; svf without sums. */
#define BN_HORIZON_MAX_DIRS 4096
int bn_grid_horizon(const float *dsm, int32_t H, int32_t W, double res, int32_t row0, int32_t row1, const double *az, int32_t D,
                    int32_t max_steps, double zmax, float *slope, int32_t *hit, void *stream);
int bn_points_horizon(const double *enz, int64_t R, const float *dsm, int32_t H, int32_t W, double xoff, double yoff, double res,
                      const double *az, int32_t D, int32_t max_steps, double zmax, float *slope, int32_t *hit, void *stream);
int bn_sky_view(const float *slope, int32_t n, int64_t cells, int64_t c0, int64_t c1, double *acc, int32_t D, float *svf,
                long long *sums, void *stream);
/* Orthophoto of an observed image (additive to ABI 7): every cell of a surface model is taken to the pixel of a satellite image
 * that saw it, and the image - or any per-pixel raster in image geometry - is gathered there.  The ortho entries above splat a
 * VIEW's rays into cells; this is the opposite direction.  There is NO upstream counterpart - the reference never orthorectifies
 * an image and reaches UTM only forwards, through pyproj - so the rule is this project's own.  Everything up to the gather's cast
 * is float64 and every operation is rounded on its own (csrc/orthophoto.hip is compiled with fp contraction off).
 *
 * 1. cell         cell (j, i) of the north-up grid (row 0 is the northern edge, as in the visibility entries):
 *                 e = xoff + ((double)i + 0.5) res ; nn = yoff - ((double)j + 0.5) res ; a = (double)dsm[j][i]
 * 2. inverse UTM  (e, nn) in `zone` (south = 1: the false northing of 10,000,000 m is taken off) -> (lon, lat) in degrees:
 *                 Karney 2011, eq. 36 and eqs. 19-21, with n, e and k0 A as step 4 of "The rays of a satellite view" forms them.
 *                 The coefficients, on the host, in Horner form in n with every fraction one division:
 *                   beta1 = n/2 - 2n^2/3 + 37n^3/96 - n^4/360 - 81n^5/512 + 96199n^6/604800
 *                   beta2 = n^2/48 + n^3/15 - 437n^4/1440 + 46n^5/105 - 1118711n^6/3870720
 *                   beta3 = 17n^3/480 - 37n^4/840 - 209n^5/4480 + 5569n^6/90720
 *                   beta4 = 4397n^4/161280 - 11n^5/504 - 830251n^6/7257600
 *                   beta5 = 4583n^5/161280 - 108847n^6/3991680          beta6 = 20648693n^6/638668800
 *                 xi = (nn - false_north) / k0A ; eta = (e - 500000) / k0A
 *                 xi' = xi - sum_j beta_j sin(2 j xi) cosh(2 j eta) ; eta' = eta - sum_j beta_j cos(2 j xi) sinh(2 j eta), j ascending,
 *                   the six complex sines sin(2 j (xi + i eta)) by the angle-addition recurrence of the forward series from ONE
 *                   sin, cos, sinh and cosh of the double angle
 *                 lon = lon0 + atan2(sinh eta', cos xi') 180 / pi          (lon0 = 6 zone - 183; times 180, then divided by pi)
 *                 tau' = sin xi' / sqrt(sinh eta' sinh eta' + cos xi' cos xi')
 *                 tau = tau', then BN_UTM_NEWTON_ITERS times, without a data-dependent exit, with e2m = 1 - e e:
 *                   r = sqrt(1 + tau tau) ; sigma = sinh(e atanh(e tau / r)) ; t = tau sqrt(1 + sigma sigma) - sigma r
 *                   tau = tau + (tau' - t) / sqrt(1 + t t) * (1 + e2m (tau tau)) / (e2m r)
 *                 lat = atan(tau) 180 / pi
 *                 A point whose lon or lat is not finite gives (NaN, NaN) and is counted.  The device's float64 sin, cos, sinh,
 *                 cosh, atan2, atanh and atan are not bit-specified: this step is held to a numpy statement within 1e-6 m carried
 *                 to degrees, and the statement to the project's own FORWARD series by the round trip (7.5e-9 m measured).  Not
 *                 checked against pyproj.
 * 3. pixel        steps 1 and 2 of "The rays of a satellite view" on (lon, lat, a) -> (col, row).
 *                 A cell whose a, lon, lat, col or row is NaN or not finite has NaN in both outputs and is counted once.
 * 4. gather       A pixel index is its coordinate: (col, row) = (k, l) is the centre of pixel (l, k).  Per cell, in this order:
 *                   col or row is NaN                                              state BN_GATHER_NODATA
 *                   !(0 <= col && col <= Wi - 1 && 0 <= row && row <= Hi - 1)      state BN_GATHER_OUTSIDE
 *                   vis != NULL && vis[cell] != BN_VIS_VISIBLE                     state BN_GATHER_OCCLUDED
 *                   otherwise                                                      state BN_GATHER_KEPT
 *                 In the first three states every channel is NaN.  Pixel (r, c) of channel ch is img[r s_row + c s_col + ch
 *                 s_chan] (element strides: s_chan = 1, s_col = C, s_row = Wi C for an [Hi Wi][C] buffer; s_chan = Hi Wi, s_row =
 *                 Wi, s_col = 1 for [C][Hi][Wi] planes).
 *                 BN_GATHER_BILINEAR: c0 = max(min((int)floor(col), Wi - 2), 0), c1 = min(c0 + 1, Wi - 1), fx = col - (double)c0
 *                 (at col = Wi - 1 the taps are the last two and fx = 1; with Wi == 1, c0 = c1 = 0 and fx = 0); rows likewise;
 *                 v = (1 - fy) ((1 - fx) p00 + fx p01) + fy ((1 - fx) p10 + fx p11) with the four taps widened to float64, p_rc the
 *                 tap of row r_r and column c_c; out = (float)v.  Plain arithmetic: a NaN tap propagates even at weight 0.
 *                 BN_GATHER_NEAREST: c = min((int)floor(col + 0.5), Wi - 1), rows likewise; the pixel's 32 bits are copied.
 *
 * bn_utm_geodetic  en float64 [n][2] = (east, north) -> lonlat float64 [n][2]; skipped[0] += the counted points  (step 2)
 * bn_grid_pixels   rpc is a HOST pointer; dsm float32 [H][W]; the cells of rows [row0, row1) -> colrow float64 [H][W][2] = (col,
 *                  row), only the band's rows written; counts[0] += the counted cells.  An empty band launches nothing.  Equal bit
 *                  for bit to bn_utm_geodetic followed by bn_rpc_project on the same cell centres.  (steps 1-3)
 * bn_image_gather  cells [n0, n1) of colrow float64 [.][2], vis uint8 [.] (nullable), state uint8 [.] and out float32, channel ch of
 *                  cell c at out[ch out_chan_stride + c]: every per-cell array is indexed by the cell itself, so a band of
 *                  cells writes its part of whole buffers.  counts uint64 [4] += the cells of the call in each state.  (step 4)
 * skipped and counts are device memory, the CALLER zeroes them, one integer atomic per counter and block; there is no float atomic.
 * Every bit depends on the inputs alone - not on blocks, row bands, cell ranges or the number of ranks.
 * Refused (BN_EINVAL, nothing launched, buffers untouched): NULL en, lonlat, skipped, rpc, dsm, colrow, counts, img, out or state;
 * n < 0 or over 2^30; a zone outside [1, 60]; south other than 0 or 1; H or W < 1, or H W > 2^30; rows outside [0, H] or row0 >
 * row1; res not positive and finite; a non-finite grid origin; a scale of zero or a non-finite entry in the descriptor; C outside
 * [1, BN_GATHER_MAX_CHANNELS]; Hi or Wi < 1; a negative stride; n0 < 0, n0 > n1 or n1 over 2^30; another mode.  The image buffer's
 * extent is the caller's to check: the taps lie in [0, Hi - 1] x [0, Wi - 1] and nowhere else. */
#define BN_UTM_NEWTON_ITERS 4
#define BN_GATHER_MAX_CHANNELS 32
enum { BN_GATHER_BILINEAR = 0, BN_GATHER_NEAREST = 1 };
enum { BN_GATHER_NODATA = 0, BN_GATHER_OUTSIDE = 1, BN_GATHER_OCCLUDED = 2, BN_GATHER_KEPT = 3 };
int bn_utm_geodetic(const double *en, int64_t n, int32_t zone, int32_t south, double *lonlat, unsigned long long *skipped,
                    void *stream);
int bn_grid_pixels(const bn_rpc *rpc, const float *dsm, int32_t H, int32_t W, double xoff, double yoff, double res, int32_t row0,
                   int32_t row1, int32_t zone, int32_t south, double *colrow, unsigned long long *counts, void *stream);
int bn_image_gather(const float *img, int32_t Hi, int32_t Wi, int32_t C, int64_t s_row, int64_t s_col, int64_t s_chan,
                    const double *colrow, const uint8_t *vis, int64_t n0, int64_t n1, int32_t mode, float *out,
                    int64_t out_chan_stride, uint8_t *state, unsigned long long *counts, void *stream);
/* Orthomosaic of several observed images (additive to ABI 7): the cells of a surface model under K images at once.  A site has 10
 * to 30 views and each sees another side of every building; one launch takes a cell to its geodetic point ONCE, walks the views
 * and keeps only the results - how many views saw the cell, the best of them, the mean and the spread of what they saw (the
 * multi-view photo-consistency of the surface model: a wrong altitude sends a cell to different ground in every image).  There is
 * NO upstream counterpart.  Float64, every operation rounded on its own (csrc/mosaic.hip is compiled with fp contraction off).
 *
 * views_host / views_dev: the same K records in host memory - read and checked before the launch - and in device memory, which
 *   the kernel reads (the CALLER makes the copy; 90 doubles per view do not fit into kernel arguments).  K in [1,
 *   BN_MOSAIC_MAX_VIEWS].  img, Hi, Wi, s_row, s_col, s_chan: as bn_image_gather takes them, C channels in every view, C in [1,
 *   BN_MOSAIC_MAX_CHANNELS]; vis: uint8 [H][W] of bn_grid_visibility towards that view's sensor, or NULL (never occluded); rank:
 *   the smaller rank wins `best`, ties go to the lower view index; rpc: the view's descriptor.
 * dsm, H, W, xoff, yoff, res, row0, row1, zone, south: as bn_grid_pixels takes them.  mode: BN_GATHER_BILINEAR or BN_GATHER_NEAREST.
 * colrow_in (nullable): float64 [K][H][W][2] = (col, row) per view and cell, on the device.  When given, steps 2 and 3a are skipped
 *   and these pixels are used (what bn_grid_pixels wrote for every view).
 *
 * Per cell (j, i) of rows [row0, row1):
 * 1. centre     e, nn, a as step 1 of "Orthophoto of an observed image".
 * 2. point      bad0 = (step 2 of that section refuses (e, nn)) ; (lon, lat) from it - once per cell, not per view.
 * 3. views      n = 0 ; m_c = 0.0, M2_c = 0.0 for c < C ; then for k = 0 .. K - 1, ascending:
 *    a. pixel   (col, row) = step 3 of that section under rpc_k on (lon, lat, a); both NaN if bad0 || !(isfinite(a) && isfinite(col)
 *               && isfinite(row)).  These are bn_grid_pixels' bits for view k: the same device functions on the same operands.
 *    b. state   step 4's state with Hi_k, Wi_k, vis_k: BN_GATHER_NODATA 0, BN_GATHER_OUTSIDE 1, BN_GATHER_OCCLUDED 2, else kept.
 *    c. value   if kept: v_c (float32) for c < C in `mode`, step 4's taps and expression: bn_image_gather's bits.
 *    d. if any v_c is NaN or infinite the view's state is BN_MOSAIC_NONFINITE 4 and it contributes nothing.
 *    e. otherwise the state is BN_MOSAIC_USED 3 and
 *               n = n + 1
 *               per channel: x = (double)v_c ; delta = x - m_c ; m_c = m_c + delta / (double)n ; M2_c = M2_c + delta * (x - m_c)
 *               (Welford's update: with float32 values near 4096 that spread by 1e-3 the sum-of-squares form q / n - m m loses
 *               the spread's third digit)
 *               if n == 1 || rank_k < best_rank: view k is the best, best_rank = rank_k, its v_c (32 bits each) are kept.
 * Outputs, each a plain store of the lane's own cell, only the band's rows written; best, best_val, mean, std and sums are
 * nullable one by one, count and counts are required:
 *   count     uint8 [H][W]      n
 *   best      int32 [H][W]      the best view's index, -1 when n == 0
 *   best_val  float32 [C][H][W] the best view's values, bits copied; NaN when n == 0
 *   mean      float32 [C][H][W] (float)m_c ; NaN when n == 0
 *   std       float32 [C][H][W] (float)sqrt(M2_c / (double)n): the population's, 0 at n == 1 ; NaN when n == 0
 *   counts    uint64 [K][5]     += the cells of the band per view and state 0 to 4
 *   sums      uint64 [3]        += (cells, q, skipped) over the cells with n >= 2: cells += 1 per cell; per channel, s = sqrt(M2_c /
 *                               (double)n): q += llrint(s 2^20) if s < 2^20, otherwise skipped += 1.  The photo-consistency of
 *                               the grid is q / (cells C 2^20).
 * counts and sums are device memory, the CALLER zeroes them, one integer atomic per counter and block; there is no float atomic.
 * Every bit depends on the inputs alone - not on blocks, row bands or the number of ranks (the bands are gathered, counts and sums
 * add up).  An empty band is accepted and launches nothing.
 * Refused (BN_EINVAL, nothing launched, buffers untouched): NULL views_host, views_dev, dsm, count or counts; K or C out of range;
 * everything bn_grid_pixels refuses of the grid, the rows and the zone; per view a NULL img, Hi or Wi < 1, a negative stride, a
 * scale of zero or a non-finite entry in the descriptor (with colrow_in too); another mode.  The image buffers' extents are the
 * caller's to check, as in bn_image_gather. */
#define BN_MOSAIC_MAX_VIEWS 32
#define BN_MOSAIC_MAX_CHANNELS 4
enum { BN_MOSAIC_USED = 3, BN_MOSAIC_NONFINITE = 4 };
typedef struct {
  const float *img;          /* device, read through the strides, as bn_image_gather */
  const uint8_t *vis;        /* device [H][W] of grid_visibility for this view, or NULL: never occluded */
  int32_t Hi, Wi;
  int64_t s_row, s_col, s_chan;
  int32_t rank;              /* smaller wins `best`; ties go to the lower view index */
  bn_rpc rpc;
} bn_mosaic_view;
int bn_grid_mosaic(const bn_mosaic_view *views_host, const bn_mosaic_view *views_dev, int32_t K, int32_t C, const float *dsm,
                   int32_t H, int32_t W, double xoff, double yoff, double res, int32_t row0, int32_t row1, int32_t zone,
                   int32_t south, int32_t mode, const double *colrow_in, uint8_t *count, int32_t *best, float *best_val, float *mean,
                   float *std, unsigned long long *counts, unsigned long long *sums, void *stream);
/* Altitude sweep of a surface model under several observed images (additive to ABI 7): the orthomosaic's spread says THAT a surface
 * model is wrong - a wrong altitude sends a cell to different ground in every image - but not by how much nor in which direction.
 * One launch evaluates the spread with the cell's altitude moved through a list of Z offsets and keeps the offset at which it is
 * smallest: a plane sweep around the surface model.  It gives a per-cell altitude residual, a refined model (dsm + best offset) and,
 * from a constant dsm with offsets that span the scene, a surface model from the images alone; none needs ground truth.  There is NO
 * upstream counterpart.  Float64, every operation rounded on its own (csrc/sweep.hip is compiled with fp contraction off).
 *
 * views_host / views_dev, K, C, dsm, H, W, xoff, yoff, res, row0, row1, zone, south, mode: as bn_grid_mosaic takes them (rank is not
 *   read).  offsets_host / offsets_dev: the same Z float64 offsets in metres in host memory - checked before the launch - and in
 *   device memory, which the kernel reads; Z in [1, BN_SWEEP_MAX_LEVELS]; they need not be sorted or distinct.  min_views in [1,
 *   BN_MOSAIC_MAX_VIEWS].  colrow_in (nullable): float64 [Z][K][H][W][2] = (col, row) per level, view and cell, on the device; when
 *   given, the inverse UTM and the projections are skipped and these pixels are used.
 *
 * Per cell c = (j, i) of rows [row0, row1):
 * 1. centre     e, nn and a0 = (double)dsm[c] as step 1 of "Orthophoto of an observed image"; bad0 and (lon, lat) as step 2 of
 *               "Orthomosaic of several observed images" - the inverse UTM runs ONCE per cell, not per level or view.
 * 2. levels     best_level = -1 ; then for l = 0 .. Z - 1, ascending:
 *               a_l = a0 + off[l]                                      (one float64 addition; never formed in float32)
 *               n = 0 ; m_c = 0.0, M2_c = 0.0 for c < C ; then for k = 0 .. K - 1, ascending, steps 3 a - e of the orthomosaic on (lon,
 *               lat, a_l): the pixel under rpc_k, NaN in both if bad0 || !(isfinite(a_l) && isfinite(col) && isfinite(row)) (with
 *               colrow_in: colrow_in[l][k][c]); the state with Hi_k, Wi_k and vis_k - the mask is the base model's and the same at
 *               every level; for a kept cell its C values in `mode`; a view with a NaN or infinite value contributes nothing;
 *               otherwise n = n + 1 and per channel x = (double)v_c ; delta = x - m_c ; m_c = m_c + delta / (double)n ; M2_c = M2_c +
 *               delta * (x - m_c).  (One device function, csrc/view_step.h, under both kernels.)
 * 3. cost       level l is valid iff n >= min_views.  v_l = 0.0 ; for c ascending: v_l = v_l + M2_c / (double)n - the sum of the
 *               channels' population variances, NOT the square of a rounded square root.
 * 4. volume     if cost != NULL: cost[l][c] = (float)v_l when the level is valid, else NaN.
 * 5. argmin     if the level is valid and (best_level < 0 || v_l < best_v): best_level = l, best_v = v_l, best_n = n.  The
 *               comparison is strict: the FIRST level in ascending l keeps a tie.
 * Outputs, each a plain store of the lane's own cell, only the band's rows written; best_cost, best_count, altitude and cost are
 * nullable one by one:
 *   best_level  int32 [H][W]      -1 when no level is valid
 *   best_cost   float32 [H][W]    (float)best_v ; NaN when none
 *   best_count  uint8 [H][W]      best_n ; 0 when none
 *   altitude    float32 [H][W]    (float)(a0 + off[best_level]) ; NaN when none
 *   cost        float32 [Z][H][W] step 4
 *   valid       uint64 [Z]        += the cells of the band that are valid at level l
 *   wins        uint64 [Z]        += the cells of the band whose best is level l
 *   sums        uint64 [3]        += (cells, q, skipped) over the cells with a best: cells += 1; q += llrint(best_v 2^20) if best_v <
 *                                 2^20, otherwise skipped += 1.  The mean cost of the grid is q / (cells 2^20).
 * valid, wins and sums are device memory, the CALLER zeroes them; at most 2 Z + 3 integer atomics per block; there is no float
 * atomic.  Every bit depends on the inputs alone - not on blocks, row bands or the number of ranks (the bands are gathered, the
 * counters add up).  An empty band is accepted and launches nothing.
 * Refused (BN_EINVAL, nothing launched, buffers untouched): everything bn_grid_mosaic refuses of the views, K, C, the grid, the rows,
 * the zone and the mode; NULL views_host, views_dev, dsm, offsets_host, offsets_dev, best_level, valid, wins or sums; Z outside [1,
 * BN_SWEEP_MAX_LEVELS]; an offset that is not finite; min_views outside [1, BN_MOSAIC_MAX_VIEWS]. */
#define BN_SWEEP_MAX_LEVELS 256
int bn_grid_sweep(const bn_mosaic_view *views_host, const bn_mosaic_view *views_dev, int32_t K, int32_t C, const float *dsm,
                  int32_t H, int32_t W, double xoff, double yoff, double res, int32_t row0, int32_t row1, int32_t zone,
                  int32_t south, int32_t mode, const double *offsets_host, const double *offsets_dev, int32_t Z, int32_t min_views,
                  const double *colrow_in, int32_t *best_level, float *best_cost, uint8_t *best_count, float *altitude, float *cost,
                  unsigned long long *valid, unsigned long long *wins, unsigned long long *sums, void *stream);
/* Semi-global aggregation of a cost volume (additive to ABI 7): bn_grid_sweep picks every cell's level on its own, and the variance of
 * a few samples is a weak cue.  The three entries below turn the volume it returns into integer quanta, add over the grid the
 * minimum-cost paths of up to 8 directions - a small penalty P1 for a change of one level between neighbouring cells, a larger P2 for
 * a jump - and pick the level of the smallest sum: semi-global matching over the levels.  There is NO upstream counterpart.  Level
 * adjacency is index adjacency: the levels are meant in ascending order of what they stand for.
 *
 * 1. quanta     bn_cost_quanta: cost float32 [Z][H][W], NaN where a level is not valid at a cell (bn_grid_sweep's `cost`), quantum > 0
 *               in float64 -> quanta int32 [H][W][Z], the level fastest:
 *               a cell with no non-NaN level: -1 at every level;  otherwise a NaN level: BN_AGG_QINV = 2^20;
 *               a non-NaN level: t = (double)c / quantum (ONE float64 division) ; q = 2^20 - 1 if t >= 2^20 - 1, 0 if t <= 0, else
 *               (int)rint(t), ties to even.  So +inf is the cap, and negatives, -0.0 and -inf are 0.
 *               That division and rounding is the only floating-point arithmetic of the three entries.
 *               counters uint64 [3] += (cells with a result, non-NaN (cell, level) pairs, pairs with t >= 2^20 - 1).
 * 2. paths      bn_cost_paths: the directions r = (row step, column step) in bit order 0 to 7 of `mask`:
 *               (0,+1) (0,-1) (+1,0) (-1,0) (+1,+1) (-1,-1) (+1,-1) (-1,+1).
 *               c(p, d) = max(quanta[p][d], 0): a cell without a result is neutral - it passes messages on and restarts no path.
 *               If p - r lies outside the grid: L_r(p, d) = c(p, d).  Otherwise, with m = min_k L_r(p - r, k):
 *                 L_r(p, d) = c(p, d) + min(L_r(p - r, d), L_r(p - r, d - 1) + P1, L_r(p - r, d + 1) + P1, m + P2) - m
 *               where the d - 1 term is absent at d = 0 and the d + 1 term at d = Z - 1.  All int32; 0 <= L_r - c <= P2.
 *               sum int32 [H][W][Z]: sum[p][d] += L_r(p, d) for every direction of the mask - at most 8 x 2^21 over the 8 directions.
 *               The entry ADDS: the CALLER zeroes sum, which is what lets launches and ranks split the directions.
 * 3. pick       bn_cost_pick: level d of cell p is valid iff 0 <= quanta[p][d] < 2^20.
 *               level int32 [H][W]: the valid level of the smallest sum[p][d], the FIRST of them on a tie (a strict <); -1 where no
 *               level is valid.  sum_min int32 [H][W]: that sum; -1 where none.  (sum is taken as what step 2 leaves: >= 0.)
 *               wins uint64 [Z] += the cells whose level is d ;  sums uint64 [2] += (cells with a level, the sum of their sum_min).
 * counters, wins and sums are device memory, the CALLER zeroes them.  Everything after step 1 is integer: the sums are int32 atomics,
 * every other output a plain store of its own cell.  No bit depends on the block order, on how the directions are split over
 * launches, or on the number of ranks.
 * Refused (BN_EINVAL, nothing launched, buffers untouched): a NULL pointer; Z outside [1, BN_SWEEP_MAX_LEVELS]; H or W < 1; H W Z >=
 * 2^31; a quantum that is not finite or <= 0; P1 < 0, P2 < P1 or P2 > 2^20; a mask that is 0 or has bits above 0xFF. */
#define BN_AGG_QINV 1048576
int bn_cost_quanta(const float *cost, int32_t Z, int32_t H, int32_t W, double quantum, int32_t *quanta, unsigned long long *counters,
                   void *stream);
int bn_cost_paths(const int32_t *quanta, int32_t Z, int32_t H, int32_t W, int32_t P1, int32_t P2, int32_t mask, int32_t *sum,
                  void *stream);
int bn_cost_pick(const int32_t *quanta, const int32_t *sum, int32_t Z, int32_t H, int32_t W, int32_t *level, int32_t *sum_min,
                 unsigned long long *wins, unsigned long long *sums, void *stream);
/* Ray-level tail of a Lambertian step in ONE launch: bn_merged_composite_forward + bn_lambert_loss (shading, SNerfLoss,
 * DepthLoss; metrics.py:39-61,82-161) + bn_merged_composite_backward.  The prior arrays carry element strides.  ray_loss [R]
 * (nullable) and/or loss_acc (nullable): ray r's term is atomically added to loss_acc[r % loss_slots] - partial sums the
 * caller adds up (4096 atomics on ONE word serialise to ~50 us; the step state's 64 partials are folded into its loss ring
 * by bn_adam_multi).  nonfinite (nullable, [0] NaN [1] Inf counters), as in bn_ray_shade_loss / bn_merged_composite_backward:
 * a ray whose loss term is not finite is left out (loss 0, gradients 0) and counted, non-finite gradient elements are zeroed
 * and counted; without it a NaN colour stays a NaN in rgb, in the loss and in the gradients, as it does upstream. */
int bn_lambert_tail(const float *z, const int64_t *sort_idx, const float *out1, const float *out2, int32_t S1, int32_t S2,
                    int32_t C, int64_t R, const float *rgbs, const float *valid_depth, int64_t v_stride,
                    const float *target_depth, int64_t td_stride, const float *target_weight, int64_t tw_stride,
                    const float *target_std, int64_t ts_stride, float rgb_padding, float lambda_rgb, float lambda_ds,
                    int32_t usealldepth, float *ray_loss, float *loss_acc, int32_t loss_slots, float *rgb,
                    float *weights, float *depth, float *d_out1, float *d_out2, unsigned long long *nonfinite,
                    const bn_noise *noise, void *stream);

/* Per-SAMPLE shading on the field-output rows as they are stored, one launch forward and one backward: --MultiBRDF
 * (models/spsbrdfnerf.py:289-307, 350-352: every sample is shaded by its own BRDF, the shaded colours are composited) and the
 * per-sample irradiance of the sun pass (:265-273).  X [N][C]: rows [0, n1) belong to ray row / S1, rows [n1, N) to ray
 * (row - n1) / S2 (the [pass-1 | guided] blocks of a training step, n1 == R S1 and N - n1 == R S2 for the R rays; n1 == N: one block).  view = -rays[ray][3:6], sun =
 * rays[ray][sun_col : +3] (sun_col < 0: (1, 1, 1)); the normal, albedo (channels 0-2) and parameter channels are read per row as
 * bn_shade_desc names them (its loss fields unused).  kind LAMBERT: the "BRDF" is the albedo itself.  irradiance: |sun_z| with
 * cos_irradiance and a normal channel, else desc->irr[row * irr_stride] - here per ROW, not per ray - when given, else 1.
 *   forward:  B[row][0:3] = (BRDF (1 + 2 pad) - pad) * irradiance ;  B[row][3] = sigma ;
 *             b_stride == C: B[row][4:] = X[row][4:]   (b_stride is 4 or C)
 *   backward: dX[row] = J^T dB[row][0:3] on the normal / albedo / parameter channels + dB[row][3] on sigma
 *             (+ dB[row][4:] on the channels behind it when b_stride == C); every channel of dX is written.
 * The derivative conventions are those of the per-point BRDF backward entry points above: torch autograd's. */
int bn_sample_brdf_forward(const bn_shade_desc *desc, const float *X, const float *rays, int64_t R, int64_t ray_stride,
                           int32_t sun_col, int64_t N, int64_t n1, int32_t S1, int32_t S2, float *B, int32_t b_stride, void *stream);
int bn_sample_brdf_backward(const bn_shade_desc *desc, const float *X, const float *rays, int64_t R, int64_t ray_stride,
                            int32_t sun_col, int64_t N, int64_t n1, int32_t S1, int32_t S2, const float *dB, int32_t b_stride,
                            float *dX, void *stream);

/* Folding of the linear feats layer into the heads' first layers (bn_field_desc.fold_feats) and the chain rule back, as
 * two launches of exact-fp32 MFMA tiles:
 *   bn_fold_heads:    w_fold[h] = w1[h][:, :F] wf ;  b_fold[h] = w1[h][:, :F] bf + b1[h] ;  m[h] = 0, s[h] = 0
 *   bn_unfold_heads:  d_w1[h][:, :F] += m[h] wf^T + s[h] bf^T ;  d_b1[h] += s[h] ;  d_wf += sum_h w1[h]^T m[h] ;  d_bf += sum_h w1[h]^T s[h]
 * m[h] [rows][F] / s[h] [rows] are the gradients of the folded first layers that bn_field_backward accumulates. */
typedef struct {
  int32_t n_heads, F, rows;              /* rows = hidden width of the heads (F / 2) */
  const float *wf, *bf;                  /* feats_from_xyz [F][F], [F] */
  const float *w1[BN_MAX_HEADS];         /* first-layer weights [rows][w1_ld], columns [0, F) used */
  int64_t w1_ld[BN_MAX_HEADS];
  const float *b1[BN_MAX_HEADS];
  float *w_fold[BN_MAX_HEADS], *b_fold[BN_MAX_HEADS];   /* [rows][F], [rows] */
  float *m[BN_MAX_HEADS], *s[BN_MAX_HEADS];             /* folded-gradient accumulators (nullable: inference) */
  float *d_w1[BN_MAX_HEADS];
  int64_t d_w1_ld[BN_MAX_HEADS];
  float *d_b1[BN_MAX_HEADS];
  float *d_wf, *d_bf;
} bn_fold_desc;
int bn_fold_heads(const bn_fold_desc *d, void *stream);
int bn_unfold_heads(const bn_fold_desc *d, void *stream);

/* Adam over the parameter groups of one flat buffer in ONE launch (torch.optim.Adam semantics per group, main.py:147-168):
 * group g = elements [lo[g], hi[g]) (multiples of 4), stepped only when active[g] (a group that is not in this step's graph
 * has grad None upstream and is skipped).  Step counts, the learning rate and the draw counter live in `state`
 * (bn_step_state): the kernel uses adam_step[g] + 1 and, when its last workgroup finishes, increments the active groups'
 * counts and rng_step and folds the loss partials into the loss ring.  zero_grad != 0: the gradient elements it read are set to 0.
 * beta1, beta2: see bn_adam_step - the state's beta1_pow / beta2_pow are powers of the float32 values. */
int bn_adam_multi(float *param, float *grad, float *exp_avg, float *exp_avg_sq, int32_t n_groups, const int64_t *lo,
                  const int64_t *hi, const int32_t *active, float beta1, float beta2, float eps, float weight_decay,
                  float grad_scale, int32_t zero_grad, void *state, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Debug hook replacing the reference's check_nan / checknan / check_nan_parms (train_utils.py:14-78,
 * models/spsbrdfnerf.py:32-48,419-424), which copy a flag to the host and print after every call:
 * counts[0] += number of NaN elements of x[0..n), counts[1] += number of +-Inf elements, on the
 * stream, without a device->host synchronisation; the caller reads the two counters when it wants.
 * ------------------------------------------------------------------------------------------- */
int bn_count_nonfinite(const float *x, int64_t n, unsigned long long *counts, void *stream);

/* Device-side fault word of the fused kernels (bit 0: a wave of the barrier-free forward trunk gave up waiting for an LDS
 * hand-over - never in a correct run; the affected launch's results are invalid; bit 1: the same for the barrier-free trunk of
 * the backward chain (round 4; ABI 3-4 reported their turn-taking deterministic mode there).  The library mirrors both bits to
 * the host asynchronously (every 64th forward launch outside a stream capture) and fails the NEXT bn_field_forward /
 * bn_field_backward call with BN_ELAUNCH once one is set; bn_adam_multi reads both words on the device and leaves parameters and
 * moments untouched while one is set (ABI 7: a replayed graph cannot train on an invalid gradient); this call synchronises
 * `stream` and reads them directly. */
int bn_device_faults(unsigned int *faults, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Measurement hooks (no reference counterpart; the reference only has Lightning's wall-clock
 * "simple" profiler, main.py:731).  When enabled, every kernel launch of this library is
 * bracketed by HIP events on the caller's stream; bn_prof_collect() synchronises them, adds the
 * durations per kernel id (order below) and clears the log.
 * ids: 0 pack, 1 field_fwd(sigma only), 2 field_fwd(full), 3 field_bwd chain, 4 wgrad, 5 skinny
 * wgrad, 6 composite fwd, 7 composite bwd, 8 guided samples, 9 stratified z, 10 adam, 11 brdf, 12 normals adjoint,
 * 13 normals adjoint backward.
 * ------------------------------------------------------------------------------------------- */
#define BN_PROF_IDS 14
int bn_prof_enable(int on);
int bn_prof_collect(double *ms_sum, int *count, int n_ids);

#ifdef __cplusplus
}
#endif
#endif /* BRDFNERF_HIP_H */
