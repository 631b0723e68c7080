// Instrumentation of the chain kernels: phase-cycle counters (BN_PH*), clock stamps (BN_CLK*) and the per-wave event timeline
// (BN_TL*).  Each family is compiled only into the diagnostic library its tool builds (diag.h, kind T); in the product build
// every macro below expands to nothing and BnPhaseClock is empty.
#pragma once
#include <hip/hip_runtime.h>

// Phase-cycle instrumentation, compiled only into the diagnostic library built by profiles/phase_timing.py
// (-DBN_PHASE_TIMING): per-wave shader-clock cycles spent between BN_PH() marks, summed over the grid.
#ifdef BN_PHASE_TIMING
#define BN_PH_N 16
static __device__ unsigned long long bn_phase_clk[BN_PH_N + 1];
#define BN_PH_DEFINE_READER(NAME)                                                                              \
  extern "C" int NAME(unsigned long long *out, int reset) {                                                    \
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(bn_phase_clk), sizeof(unsigned long long) * (BN_PH_N + 1)) != hipSuccess) return -1; \
    if (reset) {                                                                                               \
      unsigned long long z[BN_PH_N + 1] = {0};                                                                 \
      if (hipMemcpyToSymbol(HIP_SYMBOL(bn_phase_clk), z, sizeof(z)) != hipSuccess) return -1;                  \
    }                                                                                                          \
    return 0;                                                                                                  \
  }
// The wave's clock lives in the kernel (BN_PH_DECL); `phc_` refers to it, and a device function that sets marks of its own
// takes that handle as a `const BnPhaseClock &phc_` parameter (an empty struct in the product build: one signature for both).
struct BnPhaseClock { unsigned long long (&ph)[BN_PH_N], &pt; };
#define BN_PH_DECL unsigned long long ph_[BN_PH_N] = {0}, pt_ = __builtin_readcyclecounter(); const BnPhaseClock phc_{ph_, pt_};
#define BN_PH(i) { const unsigned long long n_ = __builtin_readcyclecounter(); phc_.ph[i] += n_ - phc_.pt; phc_.pt = n_; }
#define BN_PH_FLUSH if ((threadIdx.x & 63) == 0) { for (int i_ = 0; i_ < BN_PH_N; ++i_) atomicAdd(&bn_phase_clk[i_], phc_.ph[i_]); atomicAdd(&bn_phase_clk[BN_PH_N], 1ull); }
#else
struct BnPhaseClock {};
#define BN_PH_DEFINE_READER(NAME)
#define BN_PH_DECL const BnPhaseClock phc_{};
#define BN_PH(i)
#define BN_PH_FLUSH
#endif

// In-kernel clock stamps, compiled only into the diagnostic library built by profiles/clock_probe.py (-DBN_CLOCK_STAMP):
// wave 0 of every workgroup stamps s_memtime (shader clock) and s_memrealtime (100 MHz) at entry and exit; the quotient of
// the two differences is the clock the chip holds under this kernel (MI355X_MICROARCH.md, DVFS give-back item 6).  The stamps
// go to a buffer nothing else reads; no output depends on them.
#ifdef BN_CLOCK_STAMP
#define BN_CLK_N 8192
#define BN_CLK_DEFINE(NAME)                                                                                    \
  static __device__ unsigned long long bn_clk_buf[BN_CLK_N][2];                                               \
  extern "C" int NAME(unsigned long long *out, int n) {                                                        \
    if (n > BN_CLK_N) n = BN_CLK_N;                                                                            \
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(bn_clk_buf), sizeof(unsigned long long) * 2 * n) == hipSuccess ? 0 : -1; \
  }
#define BN_CLK_BEGIN const unsigned long long clk0_ = __builtin_amdgcn_s_memtime(), clk1_ = __builtin_amdgcn_s_memrealtime();
#define BN_CLK_END                                                                                             \
  if (threadIdx.x == 0 && blockIdx.x < BN_CLK_N) {                                                             \
    bn_clk_buf[blockIdx.x][0] = __builtin_amdgcn_s_memtime() - clk0_;                                          \
    bn_clk_buf[blockIdx.x][1] = __builtin_amdgcn_s_memrealtime() - clk1_;                                      \
  }
#else
#define BN_CLK_DEFINE(NAME)
#define BN_CLK_BEGIN
#define BN_CLK_END
#endif

// Per-wave event timeline, compiled only into the diagnostic library built by profiles/simd_timeline.py (-DBN_TIMELINE):
// every wave of the first BN_TL_BLOCKS workgroups stamps s_memtime at the phase boundaries of the trunk into an LDS log
// (a region the trunk does not use) and dumps it to a buffer nothing else reads; word 0 of a wave's log is its HW_ID
// (which SIMD it sits on).  No output depends on the stamps; the product build executes none of this.
#ifdef BN_TIMELINE
#define BN_TL_BLOCKS 8
#define BN_TL_EVENTS 112
static __device__ unsigned long long bn_tl_buf[BN_TL_BLOCKS][8][BN_TL_EVENTS];
#define BN_TL_DEFINE_READER(NAME)                                                                              \
  extern "C" int NAME(unsigned long long *out) {                                                               \
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(bn_tl_buf), sizeof(unsigned long long) * BN_TL_BLOCKS * 8 * BN_TL_EVENTS) == hipSuccess ? 0 : -1; \
  }
// log = LDS pointer to this wave's BN_TL_EVENTS slots; event code in the top byte
#define BN_TL_DECL(LDSBASE) unsigned long long *tl_log_ = (unsigned long long *)(LDSBASE) + (threadIdx.x >> 6) * BN_TL_EVENTS; int tl_n_ = 1; \
  if ((threadIdx.x & 63) == 0) tl_log_[0] = (unsigned long long)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));
#define BN_TL(ev) { if ((threadIdx.x & 63) == 0 && tl_n_ < BN_TL_EVENTS) tl_log_[tl_n_] = ((unsigned long long)(ev) << 56) | (__builtin_amdgcn_s_memtime() & 0x00ffffffffffffffull); ++tl_n_; }
#define BN_TL_DUMP { if (blockIdx.x < BN_TL_BLOCKS && (threadIdx.x & 63) == 0) { const int w_ = threadIdx.x >> 6; const int n_ = tl_n_ < BN_TL_EVENTS ? tl_n_ : BN_TL_EVENTS; \
    for (int i_ = 0; i_ < BN_TL_EVENTS; ++i_) bn_tl_buf[blockIdx.x][w_][i_] = i_ < n_ ? tl_log_[i_] : 0ull; } }
#else
#define BN_TL_DEFINE_READER(NAME)
#define BN_TL_DECL(LDSBASE)
#define BN_TL(ev)
#define BN_TL_DUMP
#endif
