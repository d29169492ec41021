// The two halves of an ordered compaction that more than one unit uses (kmap.hip, mix.hip):
//   scan_counts_kernel  the exclusive scan of per-block kept counts, one workgroup of 1024 threads
//   block_rank          the exclusive rank of a thread's kept element inside its block, by wave ballots
// Everything is order-preserving; nothing here is atomic.
#pragma once
#include "common.h"

namespace lidal {
namespace {

// Exclusive scan of `counts[n]` (int) -> offsets[n] (int64), total -> offsets[n].
__device__ __forceinline__ void scan_counts_body(const int* __restrict__ counts, int64_t n,
                                                 int64_t* __restrict__ offsets) {
  __shared__ int64_t wave_sum[16];
  __shared__ int64_t carry_s;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t base = 0; base < n; base += 1024) {
    int64_t i = base + threadIdx.x;
    int64_t v = (i < n) ? counts[i] : 0;
    int64_t incl = v;                         // inclusive scan inside the wave
    for (int d = 1; d < 64; d <<= 1) {
      int64_t t = __shfl_up(incl, d, 64);
      if (lane >= d) incl += t;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int64_t wave_off = 0;
    for (int w = 0; w < wave; ++w) wave_off += wave_sum[w];
    int64_t carry = carry_s;
    if (i < n) offsets[i] = carry + wave_off + incl - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry_s = carry + wave_off + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) offsets[n] = carry_s;
}
__global__ void __launch_bounds__(1024) scan_counts_kernel(const int* __restrict__ counts, int64_t n,
                                                           int64_t* __restrict__ offsets) {
  scan_counts_body(counts, n, offsets);
}

// block-level ordered rank: returns the exclusive rank of this thread's kept element among the
// kept elements of the whole block iteration, and the iteration total through *total.
template <int kThreads = 256>
__device__ __forceinline__ int block_rank(bool keep, int* wave_cnt /*[kThreads / 64] LDS*/, int* total) {
  unsigned long long m = __ballot(keep);
  int r = ballot_rank(m);
  int wave = threadIdx.x >> 6;
  if (lane_id() == 0) wave_cnt[wave] = __popcll(m);
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kThreads / 64; ++w) {
    int c = wave_cnt[w];
    if (w < wave) off += c;
    tot += c;
  }
  __syncthreads();
  *total = tot;
  return off + r;
}

}  // namespace
}  // namespace lidal
