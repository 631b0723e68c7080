// Semi-global aggregation of a cost volume over its levels: sweep.hip keeps, per cell, the level of the smallest cost; the three
// entries below turn the volume it returns into integer quanta, add the minimum-cost paths of up to 8 directions over the grid and
// pick the level of the smallest sum.  include/brdfnerf_hip.h ("Semi-global aggregation of a cost volume") states the rule operation
// by operation; there is no upstream counterpart.
//
//   cost_quanta_kernel     (Z, H, W) float32 -> [H][W][Z] int32 through an LDS tile: the block's cells are read level by level, one
//                          coalesced row segment per level, and written as ONE contiguous span of cells x Z words.  The one float64
//                          division and rounding of the feature is here.
//   cost_paths_kernel<N>   the hot path.  One wave owns one (direction, line) and walks it from its border cell; a lane holds N =
//                          ceil(Z / 64) CONSECUTIVE levels, so a cell's quanta are one 4 N-byte load per lane, the d +- 1 neighbours
//                          are in-lane but for the two edge levels (lane +- 1, one DPP move each) and the minimum over the levels
//                          is an in-lane minimum and a 6-step DPP reduction.  The loads do not depend on the recurrence: they run
//                          RING cells ahead through a register ring, so that the dependent chain of a step is VALU and cross-lane
//                          moves only.  L_r is added into `sum` by int32 atomics without return.  No LDS.
//   cost_pick_kernel       the first valid level of the smallest sum per cell, through the same tile; `wins` by one LDS table per
//                          block, as sweep.hip's.
//
// Everything after the quanta is int32: the sums are integer atomics and every other output a plain store of its own cell, so no bit
// depends on the block order, on how the directions are split over launches, or on ranks.
#include <cmath>
#include "common.h"
#include "brdfnerf_hip.h"
#include "block_sums.h"
// the one float64 division below is a single operation; nothing here can contract
#pragma clang fp contract(off)

namespace {

constexpr int AGG_BLOCK = 256;
constexpr int QCAP = BN_AGG_QINV - 1;                // the largest quantum of a valid level
constexpr int PAD = 1 << 29;                         // a level beyond Z: L stays in [PAD, PAD + P2] and never wins a minimum
constexpr int TILE_WORDS = 8448;                     // 256 x 33 >= 128 x 65, 64 x 129, 32 x 257: cells x (Z | 1) words
constexpr int RING = 4;                              // cells a line's loads run ahead of its recurrence

// the cells of one tile: the most of 256, 128, 64, 32 whose rows of Z | 1 words fit TILE_WORDS
inline int tile_cells_log2(int Z) { return Z <= 32 ? 8 : Z <= 64 ? 7 : Z <= 128 ? 6 : 5; }

// ------------------------------------------------------------------------------------------------------------------ quanta
__global__ __launch_bounds__(AGG_BLOCK)
void cost_quanta_kernel(const float *__restrict__ cost, int Z, int64_t HW, double quantum, int tc_log2, int32_t *__restrict__ quanta,
                        unsigned long long *counters) {
  __shared__ int32_t tile[TILE_WORDS];
  __shared__ unsigned int any[AGG_BLOCK];
  __shared__ long long red[4];
  const int TC = 1 << tc_log2, zp = Z | 1;
  const int tx = threadIdx.x & (TC - 1), ty = threadIdx.x >> tc_log2, rows = AGG_BLOCK >> tc_log2;
  const int64_t c0 = (int64_t)blockIdx.x * TC;
  const int cells = (int)(HW - c0 < TC ? HW - c0 : TC);
  any[threadIdx.x] = 0;
  __syncthreads();
  long long pairs = 0, capped = 0;
  if (tx < cells) {
    unsigned int seen = 0;
    for (int l = ty; l < Z; l += rows) {
      const float c = cost[(int64_t)l * HW + c0 + tx];
      int32_t q = BN_AGG_QINV;
      if (c == c) {
        const double t = (double)c / quantum;                          // ONE float64 division
        q = t >= (double)QCAP ? QCAP : (t <= 0.0 ? 0 : (int32_t)rint(t));
        seen = 1;
        ++pairs;
        capped += t >= (double)QCAP;
      }
      tile[tx * zp + l] = q;
    }
    if (seen) atomicOr(&any[tx], 1u);                                  // LDS
  }
  __syncthreads();
  int32_t *out = quanta + c0 * Z;
  for (int e = threadIdx.x; e < cells * Z; e += AGG_BLOCK) {
    const int cell = e / Z;
    out[e] = any[cell] ? tile[cell * zp + (e - cell * Z)] : -1;
  }
  const long long v3[3] = {(threadIdx.x < cells && any[threadIdx.x]) ? 1 : 0, pairs, capped};
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const long long s = block_sums::block_sum(v3[t], red);
    if (threadIdx.x == 0 && s != 0) atomicAdd(counters + t, (unsigned long long)s);
  }
}

// ------------------------------------------------------------------------------------------------------------------- paths
struct PathArgs {
  const int32_t *quanta;
  int32_t *sum;
  int32_t Z, H, W, P1, P2;
  int64_t first[9];              // first[b] .. first[b + 1]: the lines of direction b (none when the mask leaves it out)
};

__constant__ const int8_t DIR_ROW[8] = {0, 0, 1, -1, 1, -1, 1, -1};
__constant__ const int8_t DIR_COL[8] = {1, -1, 0, 0, 1, -1, -1, 1};

// lane i's value from lane i - 1 (shr) or lane i + 1 (shl) of the wave; the lane without a source gets `old`
__device__ __forceinline__ int wave_shr1(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, 0x138, 0xF, 0xF, false); }
__device__ __forceinline__ int wave_shl1(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, 0x130, 0xF, 0xF, false); }

// the minimum over the 64 lanes, the same in every lane: a prefix minimum over each row of 16 lanes (row_shr 1, 2, 4, 8), the
// rows' last lanes into the next row (row_bcast 15 into rows 1 and 3, row_bcast 31 into rows 2 and 3), then lane 63
__device__ __forceinline__ int wave_min(int v) {
  constexpr int TOP = 0x7FFFFFFF;
  v = min(v, __builtin_amdgcn_update_dpp(TOP, v, 0x111, 0xF, 0xF, false));
  v = min(v, __builtin_amdgcn_update_dpp(TOP, v, 0x112, 0xF, 0xF, false));
  v = min(v, __builtin_amdgcn_update_dpp(TOP, v, 0x114, 0xF, 0xF, false));
  v = min(v, __builtin_amdgcn_update_dpp(TOP, v, 0x118, 0xF, 0xF, false));
  v = min(v, __builtin_amdgcn_update_dpp(TOP, v, 0x142, 0xA, 0xF, false));
  v = min(v, __builtin_amdgcn_update_dpp(TOP, v, 0x143, 0xC, 0xF, false));
  return __builtin_amdgcn_readlane(v, 63);
}

template <int N> struct Levels { int32_t v[N]; };

// a cell's quanta of this lane's levels as c(p, d) = max(q, 0); PAD beyond Z.  have = the lane's levels below Z, 0 .. N
template <int N>
__device__ __forceinline__ Levels<N> load_cell(const int32_t *p, int have) {
  Levels<N> q;
  if (have == N) {
    __builtin_memcpy(q.v, p, sizeof(q.v));                             // 4 N contiguous bytes, dword-aligned
#pragma unroll
    for (int k = 0; k < N; ++k) q.v[k] = max(q.v[k], 0);
  } else {
#pragma unroll
    for (int k = 0; k < N; ++k) q.v[k] = k < have ? max(p[k], 0) : PAD;
  }
  return q;
}

template <int N>
__global__ __launch_bounds__(AGG_BLOCK)
void cost_paths_kernel(const PathArgs A) {
  const int lane = threadIdx.x & 63;
  const int d0 = lane * N;
  const int have = min(max(A.Z - d0, 0), N);
  const int64_t waves = (int64_t)gridDim.x * (AGG_BLOCK / 64);
  for (int64_t g = (int64_t)blockIdx.x * (AGG_BLOCK / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); g < A.first[8]; g += waves) {
    int b = 0;
    while (g >= A.first[b + 1]) ++b;
    const int64_t t = g - A.first[b];
    const int dj = DIR_ROW[b], di = DIR_COL[b];
    // the line's border cell: a row's or a column's end; a diagonal starts on the row it enters by (W lines), then on the column
    int j0, i0;
    if (dj == 0) { j0 = (int)t; i0 = di > 0 ? 0 : A.W - 1; }
    else if (di == 0 || t < A.W) { j0 = dj > 0 ? 0 : A.H - 1; i0 = (int)t; }
    else { j0 = (int)(t - A.W) + (dj > 0 ? 1 : 0); i0 = di > 0 ? 0 : A.W - 1; }
    const int room_j = dj > 0 ? A.H - j0 : (dj < 0 ? j0 + 1 : 0x7FFFFFFF);
    const int room_i = di > 0 ? A.W - i0 : (di < 0 ? i0 + 1 : 0x7FFFFFFF);
    const int len = min(room_j, room_i);                               // >= 1; every cell of the line is inside the grid
    const int64_t step = ((int64_t)dj * A.W + di) * A.Z;               // |step| and every offset below H W Z < 2^31
    const int64_t at0 = ((int64_t)j0 * A.W + i0) * A.Z + d0;
    const int32_t *q = A.quanta + at0;
    int32_t *s = A.sum + at0;

    Levels<N> ring[RING];
#pragma unroll
    for (int u = 0; u < RING; ++u)
      if (u < len) ring[u] = load_cell<N>(q + u * step, have);
    Levels<N> L;
    for (int i = 0; i < len; i += RING) {
#pragma unroll
      for (int u = 0; u < RING; ++u) {
        if (i + u < len) {                                             // the same in every lane
          const Levels<N> c = ring[u];
          if (i + u + RING < len) ring[u] = load_cell<N>(q + (int64_t)(i + u + RING) * step, have);
          if (i + u == 0) {
            L = c;                                                     // p - r outside the grid
          } else {
            int low = L.v[0];
#pragma unroll
            for (int k = 1; k < N; ++k) low = min(low, L.v[k]);
            const int m = wave_min(low);
            const int below = wave_shr1(PAD, L.v[N - 1]), above = wave_shl1(PAD, L.v[0]);      // levels d0 - 1 and d0 + N
            const int jump = m + A.P2;
            Levels<N> next;
#pragma unroll
            for (int k = 0; k < N; ++k) {
              const int dn = k > 0 ? L.v[k - 1] : below, up = k < N - 1 ? L.v[k + 1] : above;
              next.v[k] = c.v[k] + min(min(L.v[k], min(dn, up) + A.P1), jump) - m;
            }
            L = next;
          }
#pragma unroll
          for (int k = 0; k < N; ++k)
            if (k < have) (void)__hip_atomic_fetch_add(s + (int64_t)(i + u) * step + k, L.v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
  }
}

// -------------------------------------------------------------------------------------------------------------------- pick
__global__ __launch_bounds__(AGG_BLOCK)
void cost_pick_kernel(const int32_t *__restrict__ quanta, const int32_t *__restrict__ sum, int Z, int64_t HW, int tc_log2,
                      int32_t *__restrict__ level, int32_t *__restrict__ sum_min, unsigned long long *wins, unsigned long long *sums) {
  __shared__ uint32_t tile[TILE_WORDS];              // the key of a level: its sum when it is valid, else NONE
  __shared__ uint32_t part_key[AGG_BLOCK];
  __shared__ int32_t part_level[AGG_BLOCK];
  __shared__ unsigned int wins_t[BN_SWEEP_MAX_LEVELS];
  __shared__ long long red[4];
  constexpr uint32_t NONE = 0xFFFFFFFFu;
  const int TC = 1 << tc_log2, zp = Z | 1;
  const int tx = threadIdx.x & (TC - 1), ty = threadIdx.x >> tc_log2, rows = AGG_BLOCK >> tc_log2;
  const int64_t c0 = (int64_t)blockIdx.x * TC;
  const int cells = (int)(HW - c0 < TC ? HW - c0 : TC);
  for (int t = threadIdx.x; t < Z; t += AGG_BLOCK) wins_t[t] = 0;
  const int32_t *qin = quanta + c0 * Z, *sin = sum + c0 * Z;
  for (int e = threadIdx.x; e < cells * Z; e += AGG_BLOCK) {
    const int cell = e / Z;
    const int32_t qv = qin[e];
    tile[cell * zp + (e - cell * Z)] = (qv >= 0 && qv < BN_AGG_QINV) ? (uint32_t)sin[e] : NONE;
  }
  __syncthreads();
  // `rows` threads share a cell: each the first smallest key of its span of levels, then thread 0 of the cell over the spans in order
  const int span = (Z + rows - 1) / rows;
  uint32_t key = NONE;
  int32_t lv = -1;
  if (tx < cells) {
    const int l1 = min(Z, (ty + 1) * span);
    for (int l = ty * span; l < l1; ++l) {
      const uint32_t k = tile[tx * zp + l];
      if (k < key) { key = k; lv = l; }                                // strict: the first level keeps a tie; NONE never enters
    }
  }
  part_key[threadIdx.x] = key;
  part_level[threadIdx.x] = lv;
  __syncthreads();
  long long has = 0, total = 0;
  if (ty == 0 && tx < cells) {
    for (int r = 1; r < rows; ++r) {
      const uint32_t k = part_key[r * TC + tx];
      if (k < key) { key = k; lv = part_level[r * TC + tx]; }
    }
    level[c0 + tx] = lv;
    sum_min[c0 + tx] = lv >= 0 ? (int32_t)key : -1;
    if (lv >= 0) {
      atomicAdd(&wins_t[lv], 1u);                                      // LDS, integer
      has = 1;
      total = (long long)key;
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < Z; t += AGG_BLOCK)
    if (wins_t[t]) atomicAdd(wins + t, (unsigned long long)wins_t[t]);
  const long long v2[2] = {has, total};
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const long long s = block_sums::block_sum(v2[t], red);
    if (threadIdx.x == 0 && s != 0) atomicAdd(sums + t, (unsigned long long)s);
  }
}

int check_volume(const char *name, int32_t Z, int32_t H, int32_t W) {
  BN_REQUIRE(Z >= 1 && Z <= BN_SWEEP_MAX_LEVELS, "%s: Z=%d levels outside [1, %d]", name, Z, BN_SWEEP_MAX_LEVELS);
  BN_REQUIRE(H >= 1 && W >= 1, "%s: a grid of %d x %d cells", name, H, W);
  BN_REQUIRE((int64_t)H * W * Z < ((int64_t)1 << 31), "%s: %d x %d cells x %d levels are 2^31 elements or more", name, H, W, Z);
  return 0;
}

}  // namespace

extern "C" int bn_cost_quanta(const float *cost, int32_t Z, int32_t H, int32_t W, double quantum, int32_t *quanta,
                              unsigned long long *counters, void *stream) {
  BN_REQUIRE(cost && quanta && counters, "cost_quanta: null argument");
  if (check_volume("cost_quanta", Z, H, W)) return BN_EINVAL;
  BN_REQUIRE(std::isfinite(quantum) && quantum > 0.0, "cost_quanta: quantum=%g must be finite and positive", quantum);
  const int64_t HW = (int64_t)H * W;
  const int tc = tile_cells_log2(Z);
  cost_quanta_kernel<<<(unsigned)ceil_div64(HW, (int64_t)1 << tc), AGG_BLOCK, 0, (hipStream_t)stream>>>(cost, Z, HW, quantum, tc, quanta, counters);
  BN_LAUNCH_CHECK("cost_quanta");
  return 0;
}

extern "C" int bn_cost_paths(const int32_t *quanta, int32_t Z, int32_t H, int32_t W, int32_t P1, int32_t P2, int32_t mask, int32_t *sum,
                             void *stream) {
  BN_REQUIRE(quanta && sum, "cost_paths: null argument");
  if (check_volume("cost_paths", Z, H, W)) return BN_EINVAL;
  BN_REQUIRE(P1 >= 0 && P2 >= P1 && P2 <= BN_AGG_QINV, "cost_paths: penalties P1=%d, P2=%d (0 <= P1 <= P2 <= %d)", P1, P2, BN_AGG_QINV);
  BN_REQUIRE(mask >= 1 && mask <= 0xFF, "cost_paths: direction mask 0x%X (bits 0 to 7, at least one)", (unsigned)mask);
  PathArgs a;
  a.quanta = quanta; a.sum = sum; a.Z = Z; a.H = H; a.W = W; a.P1 = P1; a.P2 = P2;
  const int64_t lines[8] = {H, H, W, W, (int64_t)H + W - 1, (int64_t)H + W - 1, (int64_t)H + W - 1, (int64_t)H + W - 1};
  a.first[0] = 0;
  for (int b = 0; b < 8; ++b) a.first[b + 1] = a.first[b] + ((mask >> b) & 1 ? lines[b] : 0);
  // one wave per line; beyond 2^20 blocks the waves stride over the lines
  const int64_t blocks64 = ceil_div64(a.first[8], AGG_BLOCK / 64);
  const unsigned blocks = (unsigned)(blocks64 < ((int64_t)1 << 20) ? blocks64 : ((int64_t)1 << 20));
  hipStream_t s = (hipStream_t)stream;
  switch ((Z + 63) / 64) {
    case 1: cost_paths_kernel<1><<<blocks, AGG_BLOCK, 0, s>>>(a); break;
    case 2: cost_paths_kernel<2><<<blocks, AGG_BLOCK, 0, s>>>(a); break;
    case 3: cost_paths_kernel<3><<<blocks, AGG_BLOCK, 0, s>>>(a); break;
    default: cost_paths_kernel<4><<<blocks, AGG_BLOCK, 0, s>>>(a); break;
  }
  BN_LAUNCH_CHECK("cost_paths");
  return 0;
}

extern "C" int bn_cost_pick(const int32_t *quanta, const int32_t *sum, int32_t Z, int32_t H, int32_t W, int32_t *level, int32_t *sum_min,
                            unsigned long long *wins, unsigned long long *sums, void *stream) {
  BN_REQUIRE(quanta && sum && level && sum_min && wins && sums, "cost_pick: null argument");
  if (check_volume("cost_pick", Z, H, W)) return BN_EINVAL;
  const int64_t HW = (int64_t)H * W;
  const int tc = tile_cells_log2(Z);
  cost_pick_kernel<<<(unsigned)ceil_div64(HW, (int64_t)1 << tc), AGG_BLOCK, 0, (hipStream_t)stream>>>(quanta, sum, Z, HW, tc, level, sum_min,
                                                                                                      wins, sums);
  BN_LAUNCH_CHECK("cost_pick");
  return 0;
}
