// numpy's summation orders restated on the device: the one home of the pairwise sums, for the units whose results a
// numpy restatement pins (score.hip, redal.hip, kmeans.hip, frame_level.hip).  Build those units with
// -ffp-contract=off (lidal_amd/build.py) so that a*b+c stays two roundings.
#pragma once

#include "common.h"

namespace lidal {
namespace npsum {

// classes of a probability row (19 SemanticKITTI, 16 nuScenes): the per-thread rows of the scoring kernels hold this many
constexpr int kMaxClasses = 32;

// numpy's pairwise float32 add-reduce of n <= 128 values, element t read by get(off + t); I: int (np_sum_f32) or int64_t
template <class Get, class I>
__device__ __forceinline__ float np_leaf_f32(Get get, I off, I n) {
  if (n < 8) {
    float r = 0.f;
    for (I i = 0; i < n; ++i) r = __fadd_rn(r, get(off + i));
    return r;
  }
  float r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = get(off + j);
  I i = 8;
  for (; i < n - (n % 8); i += 8)
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = __fadd_rn(r[j], get(off + i + j));
  float res = __fadd_rn(__fadd_rn(__fadd_rn(r[0], r[1]), __fadd_rn(r[2], r[3])),
                        __fadd_rn(__fadd_rn(r[4], r[5]), __fadd_rn(r[6], r[7])));
  for (; i < n; ++i) res = __fadd_rn(res, get(off + i));
  return res;
}

// ... of a[0 .. n), n = the number of classes
__device__ __forceinline__ float np_sum_f32(const float* a, int n) {
  return np_leaf_f32([&](int t) { return a[t]; }, 0, n);
}

// np.add.reduce over a contiguous f32 array does not run one pairwise tree over the whole array: its iterator hands the
// inner loop blocks of at most 8192 values (the ufunc buffer size), each summed with the pairwise tree, and the block
// sums are added in order to 0.
constexpr int64_t NP_BUFSIZE = 8192;

// The pairwise tree of one block, m <= NP_BUFSIZE values from offset b0, walked post-order by one lane with an explicit
// stack (st_*: 64 entries each, in LDS; a block of 8192 needs 7 levels): a node of at most 128 values is a leaf, a
// larger one splits at m/2 - (m/2) % 8.  on_leaf(off, len) is called for every leaf, left to right, and on_add() where
// numpy adds the sums of the two subtrees finished last (left + right).
template <class Leaf, class Add>
__device__ __forceinline__ void np_block_walk(int64_t b0, int64_t m, int64_t* st_off, int64_t* st_n, int* st_phase,
                                              Leaf on_leaf, Add on_add) {
  int sp = 1;
  st_off[0] = b0; st_n[0] = m; st_phase[0] = 0;
  while (sp > 0) {
    const int top = sp - 1;
    const int64_t o = st_off[top], len = st_n[top];
    if (len <= 128) {
      on_leaf(o, len);
      --sp;
      continue;
    }
    int64_t h = len / 2;
    h -= h % 8;
    if (st_phase[top] == 0) {
      st_phase[top] = 1;
      st_off[sp] = o; st_n[sp] = h; st_phase[sp] = 0; ++sp;
    } else if (st_phase[top] == 1) {
      st_phase[top] = 2;
      st_off[sp] = o + h; st_n[sp] = len - h; st_phase[sp] = 0; ++sp;
    } else {
      on_add();
      --sp;
    }
  }
}

// numpy's f32 mean of n values get(0 .. n) of a contiguous array, by one lane (st_val: the walk's value stack, 64 entries)
template <class Get>
__device__ float np_mean_f32(Get get, int64_t n, int64_t* st_off, int64_t* st_n, int* st_phase, float* st_val) {
  float total = 0.f;
  for (int64_t b0 = 0; b0 < n; b0 += NP_BUFSIZE) {
    int vp = 0;
    np_block_walk(b0, n - b0 < NP_BUFSIZE ? n - b0 : NP_BUFSIZE, st_off, st_n, st_phase,
                  [&](int64_t o, int64_t m) { st_val[vp++] = np_leaf_f32(get, o, m); },
                  [&] {
                    const float rgt = st_val[--vp], lft = st_val[--vp];
                    st_val[vp++] = __fadd_rn(lft, rgt);
                  });
    total = __fadd_rn(total, st_val[0]);
  }
  return __fdiv_rn(total, (float)n);       // n == 0: 0 / 0 = NaN, as numpy's mean of an empty selection
}

constexpr int NP_DMAX = 128;

// numpy's pairwise f64 sum of the squared differences of one row (f32, widened) and one centre (f64), d <= 128:
// r[j] = sq[j]; r[j] += sq[i + j] for whole blocks of 8; ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)); the rest in order.
template <class C>
__device__ __forceinline__ double np_d2_f64(const float (&x)[NP_DMAX], C cget, int d) {
  const int d8 = d - d % 8;
  if (d < 8) {
    double r = 0.0;
#pragma unroll
    for (int f = 0; f < 8; ++f)
      if (f < d) { const double e = (double)x[f] - cget(f); r = __dadd_rn(r, __dmul_rn(e, e)); }
    return r;
  }
  double r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { const double e = (double)x[j] - cget(j); r[j] = __dmul_rn(e, e); }
#pragma unroll
  for (int i = 8; i < NP_DMAX; i += 8)
    if (i < d8)
#pragma unroll
      for (int j = 0; j < 8; ++j) { const double e = (double)x[i + j] - cget(i + j); r[j] = __dadd_rn(r[j], __dmul_rn(e, e)); }
  double res = __dadd_rn(__dadd_rn(__dadd_rn(r[0], r[1]), __dadd_rn(r[2], r[3])),
                         __dadd_rn(__dadd_rn(r[4], r[5]), __dadd_rn(r[6], r[7])));
#pragma unroll
  for (int f = 0; f < NP_DMAX; ++f)
    if (f >= d8 && f < d) { const double e = (double)x[f] - cget(f); res = __dadd_rn(res, __dmul_rn(e, e)); }
  return res;
}

__device__ __forceinline__ void load_row_f32(const float* __restrict__ x, int64_t i, int d, float (&r)[NP_DMAX]) {
#pragma unroll
  for (int f = 0; f < NP_DMAX; ++f) r[f] = f < d ? x[i * d + f] : 0.f;
}

}  // namespace npsum
}  // namespace lidal
