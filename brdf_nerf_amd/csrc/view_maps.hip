// The validation maps of a rendered view (eval.py:403-456, main.py:451-595), reduced chunk by chunk on the device.
//
// bn_ray_maps       per ray, over its depth-sorted samples: the index of the sample nearest the composited depth (np.argmin of
//                   |z - depth|, eval.py:411-412), that sample's row of a per-sample tensor X copied as bits
//                   (get_surface_feature), the sampling variance / standard deviation of the depth (calc_depth_std_2 /
//                   calc_depth_std), optionally sum_s w X (visualize_accumulated_feature's Accum=True) and, for a normal column of
//                   X, the integer counts behind val/bad_nr_*% (NormalRegLoss) and val/nr_an0% (check_vec0).
// bn_point_normals  calc_normal_from_pts3d (sat_utils.py:16-50) of an H x W image of float64 points, a lane per cell; the chain
//                   per cell is normal_chain.h's, the one bn_grid_normals runs.
//
// THE MAPPING of bn_ray_maps, and why.  The per-ray sums are serial in ascending s (a float64 sum is not associative and the
// bits must not depend on a split), so the natural worker is a lane per ray - but a lane per ray that walks z[r][s] in global
// memory reads 64 rows S floats apart per instruction.  So a wave owns a set of rays and every global read goes through LDS,
// in two launches on the caller's stream:
//   ray_maps_kernel   ONE WAVE (a block of 64 lanes) OWNS 64 RAYS.  z and w come in tiles of 64 rays x 32 samples: each load
//            instruction reads two rays' 32 consecutive floats (2 x 128 B, whole lines).  The tile rows have a pitch of 33 words:
//            lane r then walks row r, word r 33 + s, and the 32 lanes of a half-wave sit on 32 different banks (33 is odd;
//            ds_read_b32 conflicts only within a half-wave).  The gather of the surface row, R E words read once with E
//            consecutive words per ray, follows in the same launch.
//   ray_accum_kernel  (only with accum or a normal column) ONE WAVE OWNS G = 64 / E' RAYS and takes X in tiles of G rays x 32
//            samples x E' channels: with accum E' = E, without it only the three normal channels are staged (E' = 3).
//            Staging reads each sample's E' channels as one run; lane (g, e) then sums its channel in ascending s reading
//            consecutive words (no conflict), and the normal tests take a lane per (ray, sample), reading words E' apart
//            (gcd(E', 32)-way conflicts on three reads per sample: accepted, the tile is read once).  The rays per wave shrink
//            as the channels grow, so a chunk of 16 k rays is 780 (E' = 3) to 8192 (E' = 28) waves, not the 256 of one wave
//            per 64 rays, which left one wave per CU waiting on its own loads (measured: 0.41 ms against 0.16 ms for the
//            normal counts of a 16 k x 128 x 28 chunk).
// LDS: 17 KB per block and one wave per block in both, so nine blocks per CU.
// Integer counters: reduced over the wave by shuffles, then ONE atomic per counter and block; there is no float atomic, so the
// counters do not depend on block order, chunking or the number of ranks.
#include <cmath>
#include "common.h"
#include "brdfnerf_hip.h"
#include "block_sums.h"
#include "normal_chain.h"
// every float64 operation below is rounded on its own; the build also passes -ffp-contract=off for this file
#pragma clang fp contract(off)

namespace {

constexpr int RAYS = 64;                       // rays per block = lanes per wave
constexpr int TS = 32;                         // samples per tile
constexpr int PITCH = TS + 1;                  // odd: the rows of a z / w tile start on different banks
constexpr double STD_FIX = 1048576.0;          // 2^20
constexpr double STD_MAX = 1099511627776.0;    // 2^40: llrint(std 2^20) stays below 2^60

struct RayArgs {
  const float *z, *w, *depth, *X, *view;
  int64_t xr, xs, xc, vs, R;
  int32_t S, E, normal_col;
  int32_t *surf_idx;
  float *surf, *var, *std, *accum;
  unsigned long long *counters;
};

using block_sums::wave_sum;

__global__ __launch_bounds__(RAYS)
void ray_maps_kernel(const RayArgs A) {
  __shared__ float tile[2 * RAYS * PITCH];     // z tile | w tile
  __shared__ int sidx[RAYS];
  const int lane = threadIdx.x, S = A.S;
  const int64_t r0 = (int64_t)blockIdx.x * RAYS;
  const int nrays = (int)(A.R - r0 < RAYS ? A.R - r0 : RAYS);
  const bool mine = lane < nrays;
  float *zt = tile, *wt = tile + RAYS * PITCH;

  // ---- nearest sample and variance, a lane per ray
  const float dep = mine ? A.depth[r0 + lane] : 0.0f;
  const double dep64 = (double)dep;
  int best = 0;
  float best_dev = 0.0f;
  bool first = true, stuck = false;            // stuck: a NaN deviation was met, np.argmin returns the first one
  double v = 0.0;
  for (int s0 = 0; s0 < S; s0 += TS) {
    const int ns = S - s0 < TS ? S - s0 : TS;
    __syncthreads();
    for (int i = lane; i < RAYS * TS; i += RAYS) {
      const int row = i >> 5, col = i & (TS - 1);
      if (row < nrays && col < ns) {
        const int64_t at = (r0 + row) * S + s0 + col;
        zt[row * PITCH + col] = A.z[at];
        wt[row * PITCH + col] = A.w[at];
      }
    }
    __syncthreads();
    if (mine) {
      for (int s = 0; s < ns; ++s) {
        const float zs = zt[lane * PITCH + s], ws = wt[lane * PITCH + s];
        const float dev = fabsf(zs - dep);
        if (!stuck) {
          if (dev != dev) {
            best = s0 + s;
            stuck = true;
          } else if (first || dev < best_dev) {
            best = s0 + s;
            best_dev = dev;
          }
          first = false;
        }
        const double t = (double)zs - dep64;
        v = v + (t * t) * (double)ws;
      }
    }
  }
  long long q = 0, cnt = 0, skip = 0;
  if (mine) {
    const float sd = (float)sqrt(v);
    if (A.surf_idx) A.surf_idx[r0 + lane] = best;
    if (A.var) A.var[r0 + lane] = (float)v;
    if (A.std) A.std[r0 + lane] = sd;
    if (isfinite(sd) && (double)sd < STD_MAX) {
      q = llrint((double)sd * STD_FIX);
      cnt = 1;
    } else {
      skip = 1;
    }
  }
  sidx[lane] = best;
  q = wave_sum(q);
  cnt = wave_sum(cnt);
  skip = wave_sum(skip);
  if (lane == 0) {
    atomicAdd(A.counters + 0, (unsigned long long)q);
    atomicAdd(A.counters + 1, (unsigned long long)cnt);
    atomicAdd(A.counters + 2, (unsigned long long)skip);
  }
  __syncthreads();

  // ---- the surface row: the 32 bits of X[r][surf_idx][e]
  if (A.surf) {
    const int E = A.E;
    for (int i = lane; i < nrays * E; i += RAYS) {
      const int row = i / E, e = i - row * E;
      const uint32_t *src = reinterpret_cast<const uint32_t *>(A.X + (r0 + row) * A.xr + (int64_t)sidx[row] * A.xs + (int64_t)e * A.xc);
      reinterpret_cast<uint32_t *>(A.surf)[(r0 + row) * E + e] = *src;
    }
  }
}

// sum_s w X and the tests of the normal column: one wave owns G = 64 / Ee rays
__global__ __launch_bounds__(RAYS)
void ray_accum_kernel(const RayArgs A, int Ee, int c0, int nc, int G) {
  __shared__ float xt[RAYS * TS];              // [G][TS][Ee], G Ee <= 64
  __shared__ float wt[RAYS * TS];              // [G][TS]
  __shared__ float views[RAYS * 3];
  const int lane = threadIdx.x, S = A.S;
  const int64_t r0 = (int64_t)blockIdx.x * G;
  const int ng = (int)(A.R - r0 < G ? A.R - r0 : G);
  const bool normals = nc >= 0;
  if (normals)
    for (int i = lane; i < ng * 3; i += RAYS) {
      const int row = i / 3;
      views[i] = A.view[(r0 + row) * A.vs + (i - row * 3)];
    }
  const int sub = lane / Ee, e = lane - sub * Ee;
  const bool active = A.accum && sub < ng;
  long long bad = 0, nr0 = 0;
  double a = 0.0;
  for (int s0 = 0; s0 < S; s0 += TS) {
    const int ns = S - s0 < TS ? S - s0 : TS;
    const int per_ray = ns * Ee;
    __syncthreads();
    for (int i = lane; i < ng * per_ray; i += RAYS) {
      const int g = i / per_ray, rem = i - g * per_ray;
      const int s = rem / Ee, ch = rem - s * Ee;
      xt[g * (TS * Ee) + rem] = A.X[(r0 + g) * A.xr + (int64_t)(s0 + s) * A.xs + (int64_t)(c0 + ch) * A.xc];
    }
    for (int i = lane; i < ng * TS; i += RAYS) {
      const int g = i >> 5, s = i & (TS - 1);
      if (s < ns) wt[i] = A.w[(r0 + g) * S + s0 + s];
    }
    __syncthreads();
    if (active) {
      const float *xp = xt + sub * (TS * Ee) + e, *wp = wt + sub * TS;
      for (int s = 0; s < ns; ++s) a = a + (double)wp[s] * (double)xp[s * Ee];
    }
    if (normals) {
      for (int i = lane; i < ng * TS; i += RAYS) {
        const int g = i >> 5, s = i & (TS - 1);
        if (s >= ns) continue;
        const float *n = xt + g * (TS * Ee) + s * Ee + nc, *vw = views + g * 3;
        const double x = (double)n[0], y = (double)n[1], zc = (double)n[2];
        const double px = x * (double)vw[0], py = y * (double)vw[1], pz = zc * (double)vw[2];
        const double dot = (px + py) + pz;
        if (dot < 0.0) bad += 1;
        const double norm = sqrt((x * x + y * y) + zc * zc);
        if (!(norm > 0.99999)) nr0 += 1;
      }
    }
  }
  if (active) A.accum[(r0 + sub) * A.E + e] = (float)a;
  if (normals) {
    bad = wave_sum(bad);
    nr0 = wave_sum(nr0);
    if (lane == 0) {
      atomicAdd(A.counters + 3, (unsigned long long)bad);
      atomicAdd(A.counters + 4, (unsigned long long)nr0);
      atomicAdd(A.counters + 5, (unsigned long long)((long long)ng * S));
    }
  }
}

using normal_chain::V3;

__global__ __launch_bounds__(256)
void point_normals_kernel(const double *__restrict__ P, int H, int W, int round_f32, const float *__restrict__ valid_in,
                          float *__restrict__ out, float *__restrict__ valid_out) {
  const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (cell >= (int64_t)H * W) return;
  const int r = (int)(cell / W), c = (int)(cell - (int64_t)r * W);
  const bool border = r == 0 || r == H - 1 || c == 0 || c == W - 1;
  if (valid_out) {
    // sat_utils.py:19-24: where(valid < 1e-5, valid, 1) everywhere, the interior overwritten by the neighbours' product
    const float vc = valid_in[cell];
    float vo = vc < 1e-5f ? vc : 1.0f;
    if (!border) vo = ((valid_in[cell + W] * valid_in[cell - W]) * valid_in[cell + 1]) * valid_in[cell - 1];
    valid_out[cell] = vo;
  }
  float *o = out + cell * 3;
  if (border) {
    o[0] = o[1] = o[2] = 0.0f;
    return;
  }
  auto at = [&](int64_t k) -> V3 {
    const double *p = P + k * 3;
    if (round_f32) return {(double)(float)p[0], (double)(float)p[1], (double)(float)p[2]};     // the reference's FloatTensor cast
    return {p[0], p[1], p[2]};
  };
  auto sub = [](V3 a, V3 b) -> V3 { return {a.x - b.x, a.y - b.y, a.z - b.z}; };
  const V3 p0 = at(cell);
  const V3 n = normal_chain::cell_normal(sub(at(cell + W), p0), sub(at(cell - W), p0), sub(at(cell + 1), p0), sub(at(cell - 1), p0));
  o[0] = (float)n.x;
  o[1] = (float)n.y;
  o[2] = (float)n.z;
}

}  // namespace

extern "C" int bn_ray_maps(const float *z, const float *w, const float *depth, const float *X, int64_t x_ray, int64_t x_sample,
                           int64_t x_chan, int32_t normal_col, const float *view, int64_t view_stride, int64_t R, int32_t S, int32_t E,
                           int32_t *surf_idx, float *surf, float *var, float *std, float *accum, long long *counters, void *stream) {
  BN_REQUIRE(z && w && depth && counters, "ray_maps: null z, w, depth or counters");
  BN_REQUIRE(R >= 0 && R <= ((int64_t)1 << 30), "ray_maps: R=%lld (0 to 2^30 rays a launch)", (long long)R);
  BN_REQUIRE(S >= 1 && S <= BN_MAPS_MAX_SAMPLES, "ray_maps: S=%d (1 to %d samples)", S, BN_MAPS_MAX_SAMPLES);
  BN_REQUIRE(E >= 0 && E <= BN_MAPS_MAX_CHANNELS, "ray_maps: E=%d (0 to %d channels)", E, BN_MAPS_MAX_CHANNELS);
  BN_REQUIRE(E == 0 || X, "ray_maps: E=%d channels without X", E);
  BN_REQUIRE(E > 0 || (!surf && !accum), "ray_maps: surf and accum need a per-sample tensor X (E > 0)");
  BN_REQUIRE(x_ray >= 0 && x_sample >= 0 && x_chan >= 0 && view_stride >= 0, "ray_maps: negative stride");
  BN_REQUIRE(normal_col == -1 || (normal_col >= 0 && normal_col <= E - 3), "ray_maps: normal column %d outside [0, E - 3] (E=%d; -1: none)",
             normal_col, E);
  BN_REQUIRE(normal_col < 0 || view, "ray_maps: a normal column needs the view vectors");
  if (R == 0) return 0;
  RayArgs a;
  a.z = z; a.w = w; a.depth = depth; a.X = X; a.view = view;
  a.xr = x_ray; a.xs = x_sample; a.xc = x_chan; a.vs = view_stride; a.R = R;
  a.S = S; a.E = E; a.normal_col = normal_col;
  a.surf_idx = surf_idx; a.surf = surf; a.var = var; a.std = std; a.accum = accum;
  a.counters = reinterpret_cast<unsigned long long *>(counters);
  ray_maps_kernel<<<(unsigned)ceil_div64(R, RAYS), RAYS, 0, (hipStream_t)stream>>>(a);
  BN_LAUNCH_CHECK("ray_maps");
  if (accum || normal_col >= 0) {
    const int Ee = accum ? E : 3;                            // channels staged per sample
    const int c0 = accum ? 0 : normal_col;                   // the first of them in X
    const int nc = normal_col >= 0 ? normal_col - c0 : -1;   // the normal column inside the staged channels
    const int G = RAYS / Ee;                                 // rays per wave (E <= 64, so G >= 1)
    ray_accum_kernel<<<(unsigned)ceil_div64(R, G), RAYS, 0, (hipStream_t)stream>>>(a, Ee, c0, nc, G);
    BN_LAUNCH_CHECK("ray_maps (accum)");
  }
  return 0;
}

extern "C" int bn_point_normals(const double *points, int32_t H, int32_t W, int32_t round_f32, const float *valid_in, float *normals,
                                float *valid_out, void *stream) {
  BN_REQUIRE(points && normals, "point_normals: null argument");
  BN_REQUIRE(W > 0 && H > 0 && (int64_t)W * H <= ((int64_t)1 << 30), "point_normals: image %d x %d (W H at most 2^30 cells)", W, H);
  BN_REQUIRE(round_f32 == 0 || round_f32 == 1, "point_normals: round_f32=%d (1: the reference's float32 points, 0: exact)", round_f32);
  BN_REQUIRE((valid_in == nullptr) == (valid_out == nullptr), "point_normals: valid_in and valid_out go together");
  point_normals_kernel<<<(unsigned)ceil_div64((int64_t)W * H, 256), 256, 0, (hipStream_t)stream>>>(points, H, W, round_f32, valid_in,
                                                                                                  normals, valid_out);
  BN_LAUNCH_CHECK("point_normals");
  return 0;
}
