// The ordered scans and compactions that more than one unit uses.  Everything is order-preserving; nothing is atomic.
//   scan_counts_kernel  the exclusive scan of per-block counts, one workgroup of 1024 threads
//                       (kmap.hip, mix.hip: kept counts; tiled_scan below: its tile sums)
//   block_rank          the exclusive rank of a thread's kept element inside its block, by wave ballots
//                       (kmap.hip, mix.hip)
//   tiled_scan          the scan of an int array of any length in three launches: tile sums, their scan, the tiles again
//                       (vccs.hip: head and seed flags; cluster.hip: kept-root flags; neighbours.hip: row lengths)
#pragma once
#include "common.h"

namespace lidal {
namespace {

// Exclusive scan of `counts[n]` (int or int64) -> offsets[n] (int64), total -> offsets[n].
template <typename In>
__device__ __forceinline__ void scan_counts_body(const In* __restrict__ counts, int64_t n,
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
template <typename In>
__global__ void __launch_bounds__(1024) scan_counts_kernel(const In* __restrict__ counts, int64_t n,
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

// ---------------------------------------------------------------- tiled_scan: 256 threads x 8 items per tile
constexpr int kScanBlock = 256;
constexpr int kScanItems = 8;
constexpr int kScanTile = kScanBlock * kScanItems;
inline int64_t scan_tiles(int64_t n) { return cdiv(n, kScanTile); }

// the sum of v over the threads below this one in its block of kScanBlock, and the block's sum through *total
template <typename T>
__device__ __forceinline__ T block_exclusive(T v, T* wave_sum /*[kScanBlock / 64] LDS*/, T* total) {
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  T incl = v;
  for (int d = 1; d < kWave; d <<= 1) {
    const T t = __shfl_up(incl, d, kWave);
    if (lane >= d) incl += t;
  }
  if (lane == kWave - 1) wave_sum[wave] = incl;
  __syncthreads();
  T off = 0, tot = 0;
  for (int w = 0; w < kScanBlock / kWave; ++w) {
    const T c = wave_sum[w];
    if (w < wave) off += c;
    tot += c;
  }
  __syncthreads();
  if (total != nullptr) *total = tot;
  return off + incl - v;
}

template <typename T>
__global__ void __launch_bounds__(kScanBlock) scan_tile_sums_kernel(const int* __restrict__ in, int64_t n,
                                                                    T* __restrict__ sums) {
  __shared__ T sh[kScanBlock / kWave];
  const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  T mine = 0;
  for (int j = 0; j < kScanItems; ++j)
    if (base + j < n) mine += in[base + j];
  T total;
  block_exclusive(mine, sh, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// offs: the exclusive scan of the tile sums and, at [tiles], their total
template <typename T, bool INCLUSIVE, bool TOTAL>
__global__ void __launch_bounds__(kScanBlock) scan_tile_apply_kernel(const int* __restrict__ in, int64_t n,
                                                                     const int64_t* __restrict__ offs,
                                                                     T* __restrict__ out) {
  __shared__ T sh[kScanBlock / kWave];
  const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  int v[kScanItems];
  T mine = 0;
  for (int j = 0; j < kScanItems; ++j) {
    v[j] = base + j < n ? in[base + j] : 0;
    mine += v[j];
  }
  T run = (T)offs[blockIdx.x] + block_exclusive(mine, sh, (T*)nullptr);
  for (int j = 0; j < kScanItems; ++j) {
    if (INCLUSIVE) run += v[j];
    if (base + j < n) out[base + j] = run;
    if (!INCLUSIVE) run += v[j];
  }
  if (TOTAL && blockIdx.x == 0 && threadIdx.x == 0) out[n] = (T)offs[gridDim.x];
}

// out[i] = in[0] + .. + in[i] (INCLUSIVE) or in[0] + .. + in[i - 1], as T, for i < n; TOTAL: out[n] = the sum of all.
// n >= 1.  Scratch: sums T [scan_tiles(n)], offs int64 [scan_tiles(n) + 1]; a tile's sum is not narrowed on the way.
template <typename T, bool INCLUSIVE, bool TOTAL>
int tiled_scan(const int* in, int64_t n, T* sums, int64_t* offs, T* out, hipStream_t s) {
  const int64_t nb = scan_tiles(n);
  scan_tile_sums_kernel<T><<<(unsigned)nb, kScanBlock, 0, s>>>(in, n, sums);
  LIDAL_CHECK_LAUNCH("scan_tile_sums");
  scan_counts_kernel<T><<<1, 1024, 0, s>>>(sums, nb, offs);
  LIDAL_CHECK_LAUNCH("scan_tile_offsets");
  scan_tile_apply_kernel<T, INCLUSIVE, TOTAL><<<(unsigned)nb, kScanBlock, 0, s>>>(in, n, offs, out);
  LIDAL_CHECK_LAUNCH("scan_tile_apply");
  return 0;
}

}  // namespace
}  // namespace lidal
