// Every -D switch the library's sources react to, in ONE place: one BN_SWITCH(NAME) line each, with what it is and its default.
// The product library is built with none of them (tests/test_host_cpu.py asserts an empty bn_build_flags(), and that every
// name a preprocessor conditional of csrc/ tests is listed here); variant libraries come from
// `python -m brdf_nerf_amd.build -DSWITCH[=value] --tag=...` and are loaded with BRDFNERF_HIP_LIB=... by profiles/ab_kernels.py
// (variants alternating in one process) and the timing tools.
//
// Two parts.  Included with BN_SWITCH defined (error.cpp, inside bn_build_flags()), this file is the list alone: the defaults
// below must not be visible there, or a valued switch would always look set.  Included plainly (first, by common.h) it only
// applies the defaults of the valued switches.
//   kind T: timing / diagnostic code compiled in, results unchanged, slower      kind A: A/B switch or tunable, results unchanged
//   kind D: numerical diagnostic, results CHANGED on purpose                     kind P: timing probe, RESULTS WRONG - never ship
#ifdef BN_SWITCH
BN_SWITCH(BN_PHASE_TIMING)        // T  per-phase cycle counters of the chain kernels (profiles/phase_timing.py)
BN_SWITCH(BN_PHASE_TIMING_WGRAD)  // T  ... of wgrad256 instead (with BN_PHASE_TIMING)
BN_SWITCH(BN_CLOCK_STAMP)         // T  s_memtime / s_memrealtime stamps: the clock the chip holds (profiles/clock_probe.py)
BN_SWITCH(BN_CLOCK_STAMP_WGRAD)   // T  ... of wgrad256 instead (with BN_CLOCK_STAMP)
BN_SWITCH(BN_TIMELINE)            // T  per-wave event log of the forward trunk (profiles/simd_timeline.py)
BN_SWITCH(BN_GEMM_PRIO)           // A  =<n>: s_setprio of a wave while it multiplies in the barrier-free forward trunk (default 1)
BN_SWITCH(BN_NO_NT_STASH)         // A  plain instead of non-temporal stash stores / loads
BN_SWITCH(BN_NO_PINGPONG)         // A  the forward trunk under workgroup barriers instead of LDS hand-overs
BN_SWITCH(BN_BWD_NO_PINGPONG)     // A  the backward trunk under workgroup barriers instead of LDS hand-overs
BN_SWITCH(BN_FWD_DEPTH_TRAIN)     // A  =<n>: weight-fragment prefetch depth of the training forward (default 6)
BN_SWITCH(BN_BWD_DEPTH)           // A  =<n>: ... of the backward / adjoint chains under barriers (default 2)
BN_SWITCH(BN_BWD_PP_DEPTH)        // A  =<n>: ... of the barrier-free backward trunk (default 6)
BN_SWITCH(BN_BWD_D_AT)            // A  =<0|1|2>: where the barrier-free backward trunk issues a layer's derivative loads (default 0)
BN_SWITCH(BN_NO_FLAT_COMPOSITE)   // A  the per-(sample, channel) scalar compositing path everywhere
BN_SWITCH(SKINNY_SPLITS)          // A  =<n>: point splits of skinny_wgrad_kernel (default 256)
BN_SWITCH(BN_W2_BLOCKS)           // A  =<n>: wgrad256, tiles x point splits per round of the 256 CUs (default 256)
BN_SWITCH(BN_FILL_NO_LDS)         // A  the row pass of the hole filling reads near_row through L2 instead of staging it (profiles/fill_throughput.py)
BN_SWITCH(BN_HORIZON_NO_ZMAX)     // A  the horizon march without its (zmax - z0) / run <= best exit (profiles/horizon_throughput.py)
BN_SWITCH(BN_DIAG_D8_IN_F32)     // D  the fp32 mode sends its activation derivatives through the 16-bit modes' 8-bit codec (Siren
                                  //    layers): what the 8-bit D stash alone does to the analytic normals (profiles/diag_c5_rows.py)
BN_SWITCH(BN_PROBE_NO_A)          // P  chain GEMM without its weight fragment traffic (profiles/probe_gemm_rate.py)
BN_SWITCH(BN_PROBE_NO_B)          // P  chain GEMM without its LDS fragment traffic
BN_SWITCH(BN_PROBE_NO_D)          // P  backward chain without its derivative loads
BN_SWITCH(BN_PROBE_NO_RIDE)       // P  row-major stash copy without its global stores
BN_SWITCH(BN_ABLATION_BUILD)      // P  marker set by profiles/ scripts that patch sources for an ablation
#else
#ifndef BN_GEMM_PRIO
#define BN_GEMM_PRIO 1
#endif
#ifndef BN_FWD_DEPTH_TRAIN
#define BN_FWD_DEPTH_TRAIN 6
#endif
#ifndef BN_BWD_DEPTH
#define BN_BWD_DEPTH 2
#endif
#ifndef BN_BWD_PP_DEPTH
#define BN_BWD_PP_DEPTH 6
#endif
#ifndef BN_BWD_D_AT
#define BN_BWD_D_AT 0
#endif
#ifndef SKINNY_SPLITS
#define SKINNY_SPLITS 256   // 512: 0.129 ms, 256: 0.102 ms, 128: 0.169 ms per launch (round 2)
#endif
#ifndef BN_W2_BLOCKS
#define BN_W2_BLOCKS 256
#endif
#endif
