// The order-free integer reductions of the evaluation kernels: the lanes' int64 values (or flags) are added over the wave or the
// block and ONE integer atomic per sum goes out, so no bit depends on the block order or on how the work is split.
// Elsewhere, each with its one user: visibility.hip's count_classes (three classes under one barrier), fill.hip's fused (sum, max),
// ortho_splat_kernel's LDS counters (under the kernel's own barriers), optim.hip and normal_target.hip (the training step).
#pragma once
#include "common.h"

namespace block_sums {

__device__ __forceinline__ long long wave_sum(long long v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;                                    // valid in lane 0
}

// sum of one int64 per lane over the 256 lanes of the block; valid in lane 0 of wave 0.  red: four int64 of LDS.  The loop is
// written out as it was: called through wave_sum, ssim_map_kernel and ncc_moments_kernel are scheduled differently
__device__ __forceinline__ long long block_sum(long long v, long long *red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  const int wave = threadIdx.x >> 6;
  __syncthreads();                             // red may still be read from the previous call
  if ((threadIdx.x & 63) == 0) red[wave] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// the block's counted rows, one integer atomic (every thread of the block calls this)
__device__ __forceinline__ void block_count(bool bad, unsigned long long *counts) {
  __shared__ unsigned int block_bad;
  if (threadIdx.x == 0) block_bad = 0;
  __syncthreads();
  const unsigned long long ballot = __ballot(bad);
  if ((threadIdx.x & 63) == 0 && ballot) atomicAdd(&block_bad, (unsigned int)__popcll(ballot));       // LDS, integer
  __syncthreads();
  if (threadIdx.x == 0 && block_bad) atomicAdd(counts, (unsigned long long)block_bad);
}

// a cell's (q, n) into sums[6] = (sum, count) over all / inside / outside cells, by block_sum; zero sums send no atomic
__device__ __forceinline__ void masked_sums6(long long q, long long n, bool inside, long long *red, unsigned long long *sums) {
  const long long v[6] = {q, n, inside ? q : 0, inside ? n : 0, inside ? 0 : q, inside ? 0 : n};
  for (int k = 0; k < 6; ++k) {
    const long long s = block_sum(v[k], red);
    if (threadIdx.x == 0 && s != 0) atomicAdd(sums + k, (unsigned long long)s);
  }
}

}  // namespace block_sums
