// One launch over every tensor of a model: what the optimizer step (optim.hip) and the teacher's EMA (semi.hip) share.
//
// Work layout.  A device table has one record per tensor (include/lidal_amd.h: lidal_adam_step, lidal_ema_step).  The
// tensors are laid side by side on a VIRTUAL axis of 32-bit elements, record r at [vstart, vstart + n), gaps allowed;
// the axis is cut into chunks of kChunk elements, and a workgroup takes a run of consecutive chunks: one binary search
// of the records for its first chunk, then it walks the records forward (walk_chunks).  The host lays the axis out so
// that vstart = (address of the tensor) / 4 mod 32 (flat.place_on_axis): a chunk boundary is then a 128-byte boundary
// of every large tensor, and the piece of a tensor inside a chunk is moved as whole-wave 16-byte accesses (four per
// thread and array, all loads issued before the first use: 64 KiB in flight per workgroup with four arrays).  Nothing
// here DEPENDS on that layout: a piece whose arrays do not share one 16-byte phase is moved with 4-byte accesses, and
// the up to three elements before / after the whole vectors of a piece likewise (move_piece).  No atomics, no
// packed-f32 instructions (build.py), no synchronisation, no read-back.
//
// What is done to an element is a RULE, a type with
//     Elem                 float, or unsigned where some rule of the kernel moves words that no arithmetic may touch
//     kArrays              the arrays it touches; array 0 is the one whose address places the tensor on the axis
//     kLoads, kStores      bit k: array k is read / written.  An array a rule has no use for is not among its arrays:
//                          neither loaded, nor stored, nor part of the phase test
//     update(x)            one element: x[k] is the element of array k (0 where it was not loaded)
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace lidal {
namespace multi_tensor {

constexpr int kThreads = 256;
constexpr int kVecs = 4;                                // 16-byte vectors per thread, array and chunk
constexpr int kChunk = kThreads * kVecs * 4;            // 32-bit elements
constexpr int kBlocksPerCU = 4;

// (a pointer built from a table word is a generic one to the compiler: it would move the tensors with flat_ instructions)
#if defined(__HIP_DEVICE_COMPILE__)
#define LIDAL_GLOBAL __attribute__((address_space(1)))
#else
#define LIDAL_GLOBAL
#endif
template <typename T> using Vec4 = T __attribute__((ext_vector_type(4)));

// The chunks [c0, c1) of this workgroup, out of n_chunks from v_begin on, over the records [r0, r1) (ascending vstart,
// no overlap): piece(R, a, e) for every record R that reaches into a chunk, [a, e) being its elements inside the chunk.
// Everything here is uniform over the workgroup.  The callable takes R by value (by reference ema_step_kernel came out
// with two more VGPRs).
template <typename Rec, typename Piece>
__device__ __forceinline__ void walk_chunks(const Rec* __restrict__ recs, int r0, int r1, int64_t v_begin, int64_t n_chunks,
                                            const Piece& piece) {
  const int64_t c0 = n_chunks * (int64_t)blockIdx.x / gridDim.x, c1 = n_chunks * ((int64_t)blockIdx.x + 1) / gridDim.x;
  if (c0 >= c1) return;
  // first record that ends behind the start of chunk c0
  const int64_t first = v_begin + c0 * kChunk;
  int lo = r0, hi = r1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (recs[mid].vstart + recs[mid].n <= first) lo = mid + 1; else hi = mid;
  }
  int r = lo;
  for (int64_t c = c0; c < c1; ++c) {
    const int64_t cs = v_begin + c * kChunk, ce = cs + kChunk;
    while (r < r1 && recs[r].vstart + recs[r].n <= cs) ++r;
    for (int s = r; s < r1; ++s) {
      const Rec R = recs[s];
      if (R.vstart >= ce) break;
      const int64_t a = (cs > R.vstart ? cs : R.vstart) - R.vstart;
      const int64_t e = (ce < R.vstart + R.n ? ce : R.vstart + R.n) - R.vstart;
      piece(R, a, e);
    }
  }
}

template <typename Rule> struct Arrays {
  typedef typename Rule::Elem Elem;
  static constexpr int N = Rule::kArrays;
  static constexpr bool loads(int k) { return (Rule::kLoads >> k) & 1; }
  static constexpr bool stores(int k) { return (Rule::kStores >> k) & 1; }
  LIDAL_GLOBAL Elem* p[N];                              // the tensor's first element in every array
};

template <typename Rule>
__device__ __forceinline__ void move_scalar(const Rule& rule, const Arrays<Rule>& A, int64_t i) {
  typedef Arrays<Rule> AR;
  typename AR::Elem x[AR::N];
#pragma unroll
  for (int k = 0; k < AR::N; ++k) x[k] = AR::loads(k) ? A.p[k][i] : 0;
  rule.update(x);
#pragma unroll
  for (int k = 0; k < AR::N; ++k)
    if (AR::stores(k)) A.p[k][i] = x[k];
}

template <typename Rule>
__device__ __forceinline__ void update_vec(const Rule& rule, Vec4<typename Rule::Elem> (&v)[Rule::kArrays]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    typename Rule::Elem x[Rule::kArrays];
#pragma unroll
    for (int k = 0; k < Rule::kArrays; ++k) x[k] = v[k][e];
    rule.update(x);
#pragma unroll
    for (int k = 0; k < Rule::kArrays; ++k) v[k][e] = x[k];
  }
}

// elements [a, b) of one tensor (b - a <= kChunk), by the whole workgroup
template <typename Rule>
__device__ __forceinline__ void move_piece(const Rule& rule, const Arrays<Rule>& A, int64_t a, int64_t b) {
  typedef Arrays<Rule> AR;
  typedef Vec4<typename AR::Elem> V4;
  constexpr int N = AR::N;
  const int tid = threadIdx.x;
  const uintptr_t pa = (uintptr_t)(A.p[0] + a);
  uintptr_t diff = 0;
#pragma unroll
  for (int k = 1; k < N; ++k) diff |= pa ^ (uintptr_t)(A.p[k] + a);
  if ((diff & 15) != 0) {
    for (int64_t i = a + tid; i < b; i += kThreads) move_scalar(rule, A, i);
    return;
  }
  int64_t head = (int64_t)(((16 - (pa & 15)) & 15) >> 2);         // elements before the first 16-byte boundary
  if (head > b - a) head = b - a;
  const int64_t v0 = a + head;
  const int64_t nvec = (b - v0) >> 2;
  const int64_t tail = v0 + nvec * 4;
  LIDAL_GLOBAL V4* p4[N];
#pragma unroll
  for (int k = 0; k < N; ++k) p4[k] = (LIDAL_GLOBAL V4*)(A.p[k] + v0);
  const V4 zero = {0, 0, 0, 0};
  if (nvec == kThreads * kVecs) {                                 // a whole chunk: every load before the first use
    V4 x[kVecs][N];
#pragma unroll
    for (int j = 0; j < kVecs; ++j)
#pragma unroll
      for (int k = 0; k < N; ++k) x[j][k] = AR::loads(k) ? p4[k][tid + j * kThreads] : zero;
    asm volatile("" ::: "memory");                                // (the compiler would sink most of the loads behind the
    __builtin_amdgcn_sched_barrier(0);                            //  arithmetic of the first vectors)
#pragma unroll
    for (int j = 0; j < kVecs; ++j) {
      update_vec(rule, x[j]);
#pragma unroll
      for (int k = 0; k < N; ++k)
        if (AR::stores(k)) p4[k][tid + j * kThreads] = x[j][k];
    }
  } else {
    for (int64_t i = tid; i < nvec; i += kThreads) {
      V4 x[N];
#pragma unroll
      for (int k = 0; k < N; ++k) x[k] = AR::loads(k) ? p4[k][i] : zero;
      update_vec(rule, x);
#pragma unroll
      for (int k = 0; k < N; ++k)
        if (AR::stores(k)) p4[k][i] = x[k];
    }
  }
  if (tid < head) move_scalar(rule, A, a + tid);
  if (tid < b - tail) move_scalar(rule, A, tail + tid);
}

// compute units of the current device
inline int device_cus() {
  static int cus[MAX_DEVICES] = {0};
  const int dev = current_device();
  if (cus[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cus[dev] = n;
  }
  return cus[dev];
}

// the grid of a launch over n_chunks chunks
inline int grid_for(int64_t n_chunks) {
  const int64_t cap = (int64_t)device_cus() * kBlocksPerCU;
  return (int)(n_chunks < cap ? n_chunks : cap);
}

}  // namespace multi_tensor
}  // namespace lidal
