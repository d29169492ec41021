// The one home of what the kernels over [n, c] class rows (c <= kMaxClasses) share: loss.hip, semi.hip, score.hip and
// the cross-entropy of elementwise.hip.  A thread takes one row into registers, runs a softmax or a log-sum-exp on it,
// and the workgroup of 256 reduces a few values in a fixed order.  Nothing here is exported.
//
// RULE: no a * b + c in this header -- no product that feeds an add or a subtract.  elementwise.hip is built with fma
// contraction allowed, the other three without (NO_CONTRACT in lidal_amd/build.py); without such an expression the
// functions below mean the same statements, and give the same bits, in both kinds of unit.
#pragma once

#include "npsum.h"

namespace lidal {
namespace rows {

using npsum::kMaxClasses;

constexpr int kRows = 256;                                  // rows, and threads, per workgroup
constexpr int kTileFloats = kRows * (kMaxClasses + 1);      // LDS extent of a Tile

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;

template <typename T> struct Vec16;
template <> struct Vec16<float> {
  static constexpr int N = 4;
  typedef float4 vec;
  __device__ static void unpack(const vec& v, float (&f)[4]) { f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w; }
  __device__ static vec pack(const float (&f)[4]) { return make_float4(f[0], f[1], f[2], f[3]); }
};
template <> struct Vec16<__bf16> {
  static constexpr int N = 8;
  typedef bf16x8_t vec;
  __device__ static void unpack(const vec& v, float (&f)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = (float)v[i];
  }
  __device__ static vec pack(const float (&f)[8]) {
    vec v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (__bf16)f[i];
    return v;
  }
};

__device__ __forceinline__ bool label_ok(int64_t y, int c, int64_t ignore_index) {
  return y != ignore_index && y >= 0 && y < c;
}

// ---- rows through LDS.  A workgroup's 256 rows are ONE contiguous piece of a [n, c] matrix, moved with whole-wave
// contiguous accesses whatever c is; in the LDS image (kTileFloats floats, declared by the kernel) the rows are c | 1
// words apart, so that lanes reading their own row do not meet in one bank.  `vec`: 16-byte vectors per lane -- the
// piece starts at a multiple of 256 * c elements, 16-byte aligned when the matrix is, which the host decides.  Without
// it: element accesses, (row, column) of element q + 256 stepped from those of q, no division per element.
struct Tile {
  float* lds;
  int c, cs, nrows;               // classes, LDS row stride, rows of this workgroup that exist
  int64_t row0;

  __device__ __forceinline__ Tile(float* lds_, int64_t n, int c_) : lds(lds_), c(c_), cs(c_ | 1) {
    row0 = (int64_t)blockIdx.x * kRows;
    const int64_t left = n - row0;
    nrows = left < kRows ? (left > 0 ? (int)left : 0) : kRows;
  }

  __device__ __forceinline__ int at(int e) const { return (e / c) * cs + (e % c); }

  // mv(p + q, lds + at) for every element q of the piece: vec == false
  template <typename P, typename Move>
  __device__ __forceinline__ void walk(P* p, Move mv) const {
    const int total = nrows * c;
    const int dr = kRows / c, dc = kRows % c;
    int r = threadIdx.x / c, k = threadIdx.x % c;
    for (int q = threadIdx.x; q < total; q += kRows) {
      mv(p[q], lds[r * cs + k]);
      r += dr; k += dc;
      if (k >= c) { k -= c; ++r; }
    }
  }

  template <typename T>
  __device__ __forceinline__ void load(const T* __restrict__ src, bool vec) const {
    constexpr int V = Vec16<T>::N;
    const T* p = src + row0 * c;
    const int total = nrows * c;
    if (!vec) return walk(p, [](const T& g, float& l) { l = (float)g; });
    for (int q = threadIdx.x * V; q < total; q += kRows * V) {
      if (q + V <= total) {
        float f[V];
        Vec16<T>::unpack(*reinterpret_cast<const typename Vec16<T>::vec*>(p + q), f);
#pragma unroll
        for (int u = 0; u < V; ++u) lds[at(q + u)] = f[u];
      } else {
        for (int u = 0; q + u < total; ++u) lds[at(q + u)] = (float)p[q + u];
      }
    }
  }

  template <typename T>
  __device__ __forceinline__ void store(T* __restrict__ dst, bool vec) const {
    constexpr int V = Vec16<T>::N;
    T* p = dst + row0 * c;
    const int total = nrows * c;
    if (!vec) return walk(p, [](T& g, const float& l) { g = (T)l; });
    for (int q = threadIdx.x * V; q < total; q += kRows * V) {
      if (q + V <= total) {
        float f[V];
#pragma unroll
        for (int u = 0; u < V; ++u) f[u] = lds[at(q + u)];
        *reinterpret_cast<typename Vec16<T>::vec*>(p + q) = Vec16<T>::pack(f);
      } else {
        for (int u = 0; q + u < total; ++u) p[q + u] = (T)lds[at(q + u)];
      }
    }
  }

  // the thread's own row of the image; own: into registers (0 past c and past the last row), put: the reverse
  __device__ __forceinline__ float* mine() const { return lds + threadIdx.x * cs; }
  __device__ __forceinline__ void own(float (&x)[kMaxClasses]) const {
#pragma unroll
    for (int j = 0; j < kMaxClasses; ++j) x[j] = (j < c && (int)threadIdx.x < nrows) ? lds[threadIdx.x * cs + j] : 0.f;
  }
  __device__ __forceinline__ void put(const float (&x)[kMaxClasses]) const {
#pragma unroll
    for (int j = 0; j < kMaxClasses; ++j)
      if (j < c) lds[threadIdx.x * cs + j] = x[j];
  }
};

// ---- the row exponential: x[j] = expf(src[j] - mx) with mx the row's maximum, s = their sum in class order in Acc
// (float: the "view" form of DESIGN.md section 17; double, rounded once by the caller: the losses).  Returns the class
// of the FIRST maximum.  src may be x itself.  The probability of class j is x[j] / s.
template <typename Acc, typename Src>
__device__ __forceinline__ int row_exp(const Src& src, int c, float (&x)[kMaxClasses], float& mx, Acc& s) {
  mx = -INFINITY;
  int arg = 0;
#pragma unroll
  for (int j = 0; j < kMaxClasses; ++j)
    if (j < c) {
      x[j] = (float)src[j];
      if (x[j] > mx) arg = j;
      mx = fmaxf(mx, x[j]);
    }
  s = (Acc)0;
#pragma unroll
  for (int j = 0; j < kMaxClasses; ++j)
    if (j < c) { x[j] = expf(x[j] - mx); s += (Acc)x[j]; }
  return arg;
}

// ... and the softmax for callers that do not need s: x[j] = expf(src[j] - mx) / (float)s
template <typename Acc, typename Src>
__device__ __forceinline__ int row_softmax(const Src& src, int c, float (&x)[kMaxClasses]) {
  float mx;
  Acc sa;
  const int arg = row_exp<Acc>(src, c, x, mx, sa);
  const float s = (float)sa;
#pragma unroll
  for (int j = 0; j < kMaxClasses; ++j)
    if (j < c) x[j] = x[j] / s;
  return arg;
}

// the value of x[arg] for a run-time arg, without indexing the register array
__device__ __forceinline__ float pick(const float (&x)[kMaxClasses], int c, int arg) {
  float v = 0.f;
#pragma unroll
  for (int j = 0; j < kMaxClasses; ++j)
    if (j < c && j == arg) v = x[j];
  return v;
}

// ---- fixed-order sums of a workgroup of 256: red[k][0] = the sum of every thread's v[k], by halving from 128
template <int N, typename V>
__device__ __forceinline__ void block_sum(const V (&v)[N], V (*red)[kRows]) {
#pragma unroll
  for (int k = 0; k < N; ++k) red[k][threadIdx.x] = v[k];
  __syncthreads();
  for (int w = kRows / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
#pragma unroll
      for (int k = 0; k < N; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + w];
    }
    __syncthreads();
  }
}

// ... of the block partials part[nblocks][N], by ONE workgroup: stride 256 over the blocks, then the tree
template <int N, typename P, typename V>
__device__ __forceinline__ void sum_partials(const P* __restrict__ part, int64_t nblocks, V (*red)[kRows]) {
  V a[N];
#pragma unroll
  for (int k = 0; k < N; ++k) a[k] = (V)0;
  for (int64_t i = threadIdx.x; i < nblocks; i += kRows) {
#pragma unroll
    for (int k = 0; k < N; ++k) a[k] += part[i * N + k];
  }
  block_sum<N>(a, red);
}

}  // namespace rows
}  // namespace lidal
