// Adam for any number of f32 parameter tensors in ONE launch (train.py:56,140: torch.optim.Adam(...).step()).
//
// The arithmetic is torch's single-tensor Adam (torch/optim/adam.py _single_tensor_adam), every operation rounded
// separately in f32 -- this unit is compiled with -ffp-contract=off (build.py NO_CONTRACT), `/` and sqrtf are the
// compiler's correctly rounded forms, subnormals are kept (tests/adam_ref.py restates it in numpy, bit for bit):
//
//     g   = grad                                   (weight_decay != 0:  g = grad + wd * p)
//     m   = m + (g - m) * (1 - beta1)
//     v   = v * beta2 + ((1 - beta2) * g) * g
//     den = sqrtf(v) / sqrt(1 - beta2^t) + eps
//     p   = p + (-(lr / (1 - beta1^t))) * (m / den)
//
// Work layout.  A device table has one record per tensor (include/lidal_amd.h: lidal_adam_step).  The tensors are laid
// side by side on a VIRTUAL element axis, record r at [vstart, vstart + n), gaps allowed; the axis is cut into chunks of
// kAdamChunk elements, and a workgroup takes a run of consecutive chunks: one binary search of the records for its
// first chunk, then it walks the records forward.  The host lays the axis out so that vstart = (address of p) / 4 mod
// 32: a chunk boundary is then a 128-byte boundary of every large tensor, and the piece of a tensor inside a chunk is
// moved as whole-wave 16-byte accesses (four per thread and array, all loads issued before the first use: 64 KiB in
// flight per workgroup).  Nothing here DEPENDS on that layout: a piece whose parameter, gradient and state addresses do
// not share one 16-byte phase is moved with 4-byte accesses, and the up to three elements before / after the whole
// vectors of a piece likewise.  No atomics, no packed-f32 instructions (build.py), no synchronisation, no read-back.
//
// Further down, on the same table and piece mover: AdamW and SGD with momentum (optim_step_kernel), and the global
// gradient norm with its clip coefficient formed on the device (grad_norm_partials_kernel, grad_norm_finish_kernel).
#include "common.h"

#pragma clang fp contract(off)

namespace lidal {

constexpr int kAdamThreads = 256;
constexpr int kAdamVecs = 4;                                    // 16-byte vectors per thread, array and chunk
constexpr int kAdamChunk = kAdamThreads * kAdamVecs * 4;        // elements
constexpr int kAdamBlocksPerCU = 4;

struct AdamRec {            // five 64-bit words: the table's record
  uint64_t p;               // address of the parameter
  int64_t g;                // gradient: byte offset from the `grad_base` of the launch (absolute address: base 0)
  int64_t state;            // first element of its m / v in the two flat state buffers
  int64_t vstart;           // first element on the virtual axis (ascending with the record index, no overlap)
  int64_t n;                // elements
};

// (a pointer built from a table word is a generic one to the compiler: it would move the parameters with flat_ instructions)
typedef float f32x4 __attribute__((ext_vector_type(4)));
#if defined(__HIP_DEVICE_COMPILE__)
#define LIDAL_GLOBAL __attribute__((address_space(1)))
#else
#define LIDAL_GLOBAL
#endif
typedef LIDAL_GLOBAL float gfloat;
typedef LIDAL_GLOBAL const float cgfloat;
typedef LIDAL_GLOBAL f32x4 gfloat4;
typedef LIDAL_GLOBAL const f32x4 cgfloat4;

struct AdamScalars { float omb1, b2, omb2, bc2_sqrt, eps, neg_step, wd; };

__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, const AdamScalars& k, bool decay) {
  if (decay) g = g + k.wd * p;
  m = m + (g - m) * k.omb1;
  v = v * k.b2 + (k.omb2 * g) * g;
  const float den = sqrtf(v) / k.bc2_sqrt + k.eps;
  p = p + k.neg_step * (m / den);
}

__device__ __forceinline__ void adam_scalar(gfloat* p, cgfloat* g, gfloat* m, gfloat* v, int64_t i, const AdamScalars& k,
                                            bool decay) {
  float pi = p[i], mi = m[i], vi = v[i];
  adam_update(pi, g[i], mi, vi, k, decay);
  p[i] = pi; m[i] = mi; v[i] = vi;
}

__device__ __forceinline__ void adam_vec(f32x4& p, const f32x4& g, f32x4& m, f32x4& v, const AdamScalars& k, bool decay) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float pe = p[e], me = m[e], ve = v[e];
    adam_update(pe, g[e], me, ve, k, decay);
    p[e] = pe; m[e] = me; v[e] = ve;
  }
}

// elements [a, b) of one tensor (b - a <= kAdamChunk), by the whole workgroup
__device__ __forceinline__ void adam_piece(gfloat* p, cgfloat* g, gfloat* m, gfloat* v, int64_t a, int64_t b,
                                           const AdamScalars& k, bool decay) {
  const int tid = threadIdx.x;
  const uintptr_t pa = (uintptr_t)(p + a);
  const bool one_phase = (((pa ^ (uintptr_t)(g + a)) | (pa ^ (uintptr_t)(m + a)) | (pa ^ (uintptr_t)(v + a))) & 15) == 0;
  if (!one_phase) {
    for (int64_t i = a + tid; i < b; i += kAdamThreads) adam_scalar(p, g, m, v, i, k, decay);
    return;
  }
  int64_t head = (int64_t)(((16 - (pa & 15)) & 15) >> 2);         // elements before the first 16-byte boundary
  if (head > b - a) head = b - a;
  const int64_t v0 = a + head;
  const int64_t nvec = (b - v0) >> 2;
  const int64_t tail = v0 + nvec * 4;
  gfloat4* p4 = (gfloat4*)(p + v0);
  cgfloat4* g4 = (cgfloat4*)(g + v0);
  gfloat4* m4 = (gfloat4*)(m + v0);
  gfloat4* v4 = (gfloat4*)(v + v0);
  if (nvec == kAdamThreads * kAdamVecs) {                         // a whole chunk: every load before the first use
    f32x4 pp[kAdamVecs], gg[kAdamVecs], mm[kAdamVecs], vv[kAdamVecs];
#pragma unroll
    for (int j = 0; j < kAdamVecs; ++j) {
      const int i = tid + j * kAdamThreads;
      pp[j] = p4[i]; gg[j] = g4[i]; mm[j] = m4[i]; vv[j] = v4[i];
    }
    asm volatile("" ::: "memory");                                // (the compiler would sink most of the loads behind the
    __builtin_amdgcn_sched_barrier(0);                            //  arithmetic of the first vectors)
#pragma unroll
    for (int j = 0; j < kAdamVecs; ++j) {
      const int i = tid + j * kAdamThreads;
      adam_vec(pp[j], gg[j], mm[j], vv[j], k, decay);
      p4[i] = pp[j]; m4[i] = mm[j]; v4[i] = vv[j];
    }
  } else {
    for (int64_t i = tid; i < nvec; i += kAdamThreads) {
      f32x4 pp = p4[i], mm = m4[i], vv = v4[i];
      adam_vec(pp, g4[i], mm, vv, k, decay);
      p4[i] = pp; m4[i] = mm; v4[i] = vv;
    }
  }
  if (tid < head) adam_scalar(p, g, m, v, a + tid, k, decay);
  if (tid < b - tail) adam_scalar(p, g, m, v, tail + tid, k, decay);
}

__global__ __launch_bounds__(kAdamThreads) void adam_step_kernel(const AdamRec* __restrict__ recs, int r0, int r1,
                                                                 int64_t v_begin, int64_t n_chunks, const char* grad_base,
                                                                 float* m, float* v, int64_t state_numel, AdamScalars k,
                                                                 int decay) {
  const int64_t c0 = n_chunks * (int64_t)blockIdx.x / gridDim.x, c1 = n_chunks * ((int64_t)blockIdx.x + 1) / gridDim.x;
  if (c0 >= c1) return;
  // first record that ends behind the start of chunk c0 (all of this is uniform over the workgroup)
  const int64_t first = v_begin + c0 * kAdamChunk;
  int lo = r0, hi = r1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (recs[mid].vstart + recs[mid].n <= first) lo = mid + 1; else hi = mid;
  }
  int r = lo;
  for (int64_t c = c0; c < c1; ++c) {
    const int64_t cs = v_begin + c * kAdamChunk, ce = cs + kAdamChunk;
    while (r < r1 && recs[r].vstart + recs[r].n <= cs) ++r;
    for (int s = r; s < r1; ++s) {
      const AdamRec R = recs[s];
      if (R.vstart >= ce) break;
      if (R.n <= 0 || R.state < 0 || R.state + R.n > state_numel) continue;      // never outside the state buffers
      const int64_t a = (cs > R.vstart ? cs : R.vstart) - R.vstart;
      const int64_t e = (ce < R.vstart + R.n ? ce : R.vstart + R.n) - R.vstart;
      adam_piece((gfloat*)R.p, (cgfloat*)((uintptr_t)grad_base + (uintptr_t)R.g), (gfloat*)(uintptr_t)(m + R.state),
                 (gfloat*)(uintptr_t)(v + R.state), a, e, k, decay != 0);
    }
  }
}

// ---- AdamW, SGD with momentum, and either of the three behind a clipped gradient ----------------------------------------
// Beside adam_step_kernel (which `Adam` without clipping goes on launching): the same table, virtual axis, chunk walk
// and piece mover, with the update RULE as a template argument and the arrays a rule has no use for left alone --
//
//   kAdamCoupled / kAdamW   p, g, m, v   torch's _single_tensor_adam; kAdamW runs p = p * (1 - lr * wd) first and then the
//                                        five lines above with g = grad (decoupled_weight_decay=True)
//   kSgdPlain               p, g         torch's _single_tensor_sgd, momentum == 0: no state, no state traffic
//   kSgdFirst               p, g, buf    the first step of a parameter: buf = g (buf is written, never read)
//   kSgdMom                 p, g, buf    buf = buf * mom + (1 - dampening) * g
//                                        then g = g + mom * buf (nesterov) or g = buf;  p = p + (-lr) * g
//
// CLIP: g = grad * coef before anything else, coef read from the device (grad_norm_finish_kernel below wrote it), also
// when coef == 1; `.grad` itself is not written.  Weight decay and Nesterov are uniform scalar branches, as `decay` above.
enum { kAdamCoupled = 0, kAdamW = 1, kSgdPlain = 2, kSgdFirst = 3, kSgdMom = 4 };

struct StepScalars {
  AdamScalars a;                      // kAdamCoupled / kAdamW
  float decay_mul;                    // kAdamW: 1 - lr * wd
  float mom, omd, neg_lr, wd;         // SGD: momentum, 1 - dampening, -lr, weight decay
  int decay, nesterov;
};

template <int RULE> struct RuleArrays {
  static constexpr int kStates = RULE <= kAdamW ? 2 : (RULE == kSgdPlain ? 0 : 1);
  static constexpr bool kLoadsState = RULE != kSgdFirst;
};

template <int RULE, bool CLIP>
__device__ __forceinline__ void rule_update(float& p, float g, float& s0, float& s1, const StepScalars& k, float coef) {
  if constexpr (CLIP) g = g * coef;
  if constexpr (RULE == kAdamCoupled) {
    adam_update(p, g, s0, s1, k.a, k.decay != 0);
  } else if constexpr (RULE == kAdamW) {
    p = p * k.decay_mul;
    adam_update(p, g, s0, s1, k.a, false);
  } else {
    if (k.decay) g = g + k.wd * p;
    if constexpr (RULE == kSgdFirst) s0 = g;
    if constexpr (RULE == kSgdMom) s0 = s0 * k.mom + k.omd * g;
    if constexpr (RULE != kSgdPlain) g = k.nesterov ? g + k.mom * s0 : s0;
    p = p + k.neg_lr * g;
  }
}

template <int RULE, bool CLIP>
__device__ __forceinline__ void rule_scalar(gfloat* p, cgfloat* g, gfloat* s0, gfloat* s1, int64_t i, const StepScalars& k,
                                            float coef) {
  constexpr int NS = RuleArrays<RULE>::kStates;
  float pi = p[i], a = 0.f, b = 0.f;
  if constexpr (NS >= 1 && RuleArrays<RULE>::kLoadsState) a = s0[i];
  if constexpr (NS >= 2) b = s1[i];
  rule_update<RULE, CLIP>(pi, g[i], a, b, k, coef);
  p[i] = pi;
  if constexpr (NS >= 1) s0[i] = a;
  if constexpr (NS >= 2) s1[i] = b;
}

template <int RULE, bool CLIP>
__device__ __forceinline__ void rule_vec(f32x4& p, const f32x4& g, f32x4& s0, f32x4& s1, const StepScalars& k, float coef) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float pe = p[e], a = s0[e], b = s1[e];
    rule_update<RULE, CLIP>(pe, g[e], a, b, k, coef);
    p[e] = pe; s0[e] = a; s1[e] = b;
  }
}

// elements [a, b) of one tensor (b - a <= kAdamChunk), by the whole workgroup: adam_piece over the arrays of the rule
template <int RULE, bool CLIP>
__device__ __forceinline__ void rule_piece(gfloat* p, cgfloat* g, gfloat* s0, gfloat* s1, int64_t a, int64_t b,
                                           const StepScalars& k, float coef) {
  constexpr int NS = RuleArrays<RULE>::kStates;
  constexpr bool LD = RuleArrays<RULE>::kLoadsState;
  const int tid = threadIdx.x;
  const uintptr_t pa = (uintptr_t)(p + a);
  uintptr_t diff = pa ^ (uintptr_t)(g + a);
  if constexpr (NS >= 1) diff |= pa ^ (uintptr_t)(s0 + a);
  if constexpr (NS >= 2) diff |= pa ^ (uintptr_t)(s1 + a);
  if ((diff & 15) != 0) {
    for (int64_t i = a + tid; i < b; i += kAdamThreads) rule_scalar<RULE, CLIP>(p, g, s0, s1, i, k, coef);
    return;
  }
  int64_t head = (int64_t)(((16 - (pa & 15)) & 15) >> 2);         // elements before the first 16-byte boundary
  if (head > b - a) head = b - a;
  const int64_t v0 = a + head;
  const int64_t nvec = (b - v0) >> 2;
  const int64_t tail = v0 + nvec * 4;
  gfloat4* p4 = (gfloat4*)(p + v0);
  cgfloat4* g4 = (cgfloat4*)(g + v0);
  gfloat4* a4 = (gfloat4*)(s0 + v0);
  gfloat4* b4 = (gfloat4*)(s1 + v0);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  if (nvec == kAdamThreads * kAdamVecs) {                         // a whole chunk: every load before the first use
    f32x4 pp[kAdamVecs], gg[kAdamVecs], aa[kAdamVecs], bb[kAdamVecs];
#pragma unroll
    for (int j = 0; j < kAdamVecs; ++j) {
      const int i = tid + j * kAdamThreads;
      pp[j] = p4[i]; gg[j] = g4[i];
      if constexpr (NS >= 1 && LD) aa[j] = a4[i]; else aa[j] = zero;
      if constexpr (NS >= 2) bb[j] = b4[i]; else bb[j] = zero;
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < kAdamVecs; ++j) {
      const int i = tid + j * kAdamThreads;
      rule_vec<RULE, CLIP>(pp[j], gg[j], aa[j], bb[j], k, coef);
      p4[i] = pp[j];
      if constexpr (NS >= 1) a4[i] = aa[j];
      if constexpr (NS >= 2) b4[i] = bb[j];
    }
  } else {
    for (int64_t i = tid; i < nvec; i += kAdamThreads) {
      f32x4 pp = p4[i], aa = zero, bb = zero;
      if constexpr (NS >= 1 && LD) aa = a4[i];
      if constexpr (NS >= 2) bb = b4[i];
      rule_vec<RULE, CLIP>(pp, g4[i], aa, bb, k, coef);
      p4[i] = pp;
      if constexpr (NS >= 1) a4[i] = aa;
      if constexpr (NS >= 2) b4[i] = bb;
    }
  }
  if (tid < head) rule_scalar<RULE, CLIP>(p, g, s0, s1, a + tid, k, coef);
  if (tid < b - tail) rule_scalar<RULE, CLIP>(p, g, s0, s1, tail + tid, k, coef);
}

template <int RULE, bool CLIP>
__global__ __launch_bounds__(kAdamThreads) void optim_step_kernel(const AdamRec* __restrict__ recs, int r0, int r1,
                                                                  int64_t v_begin, int64_t n_chunks, const char* grad_base,
                                                                  float* s0, float* s1, int64_t state_numel, StepScalars k,
                                                                  const float* __restrict__ coef_ptr) {
  constexpr int NS = RuleArrays<RULE>::kStates;
  const int64_t c0 = n_chunks * (int64_t)blockIdx.x / gridDim.x, c1 = n_chunks * ((int64_t)blockIdx.x + 1) / gridDim.x;
  if (c0 >= c1) return;
  float coef = 1.0f;
  if constexpr (CLIP) coef = *coef_ptr;
  const int64_t first = v_begin + c0 * kAdamChunk;
  int lo = r0, hi = r1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (recs[mid].vstart + recs[mid].n <= first) lo = mid + 1; else hi = mid;
  }
  int r = lo;
  for (int64_t c = c0; c < c1; ++c) {
    const int64_t cs = v_begin + c * kAdamChunk, ce = cs + kAdamChunk;
    while (r < r1 && recs[r].vstart + recs[r].n <= cs) ++r;
    for (int s = r; s < r1; ++s) {
      const AdamRec R = recs[s];
      if (R.vstart >= ce) break;
      if (R.n <= 0) continue;
      if (NS > 0 && (R.state < 0 || R.state + R.n > state_numel)) continue;     // never outside the state buffers
      const int64_t a = (cs > R.vstart ? cs : R.vstart) - R.vstart;
      const int64_t e = (ce < R.vstart + R.n ? ce : R.vstart + R.n) - R.vstart;
      const int64_t so = NS > 0 ? R.state : 0;
      rule_piece<RULE, CLIP>((gfloat*)R.p, (cgfloat*)((uintptr_t)grad_base + (uintptr_t)R.g),
                             (gfloat*)(uintptr_t)(s0 + so), (gfloat*)(uintptr_t)(s1 + so), a, e, k, coef);
    }
  }
}

// ---- the global gradient norm, without a read-back -----------------------------------------------------------------------
// sum of g * g over every record, in f64 (the square of an f32 is exact there), in an order that is a function of
// (record, element index inside the tensor) ONLY: tensor r is cut into blocks of kNormBlock of its own elements, block
// j of record r owns partial slot slot_start[r] + j.  Inside a block element e belongs to thread (e / 4) % 256, which
// adds its squares in ascending e; the 256 sums meet in a fixed tree (s = 128 .. 1: sum[t] += sum[t + s]); elements behind
// the tensor's end add +0.  grad_norm_finish_kernel adds the slots in ascending order.  Neither the grid, nor the
// address phase (a gradient off the 16-byte grid is read with 4-byte loads: same elements, same thread, same order),
// nor the virtual axis, nor the gradient form enters.  No atomics.
constexpr int kNormThreads = 256;
constexpr int kNormRounds = 16;                                 // 16-byte vectors per thread and block
constexpr int kNormBatch = 8;                                   // of which in flight at once
constexpr int kNormBlock = kNormThreads * kNormRounds * 4;      // elements

__global__ __launch_bounds__(kNormThreads) void grad_norm_partials_kernel(const AdamRec* __restrict__ recs,
                                                                          const int64_t* __restrict__ slot_start, int r0,
                                                                          int r1, const char* grad_base,
                                                                          double* __restrict__ partials, int64_t n_slots,
                                                                          int zero) {
  __shared__ double sums[kNormThreads];
  const int tid = threadIdx.x;
  const int64_t s_begin = slot_start[r0], s_end = slot_start[r1] < n_slots ? slot_start[r1] : n_slots;
  for (int64_t s = s_begin + blockIdx.x; s < s_end; s += gridDim.x) {
    if (zero) {
      if (tid == 0) partials[s] = 0.0;
      continue;
    }
    int lo = r0, hi = r1 - 1;                                   // the record whose slots hold s (uniform)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (slot_start[mid + 1] <= s) lo = mid + 1; else hi = mid;
    }
    const AdamRec R = recs[lo];
    const int64_t e0 = (s - slot_start[lo]) * kNormBlock;
    const int64_t cnt = R.n - e0 < kNormBlock ? R.n - e0 : kNormBlock;      // elements of this block (<= 0: none)
    cgfloat* g = (cgfloat*)((uintptr_t)grad_base + (uintptr_t)R.g) + e0;
    const bool aligned = ((uintptr_t)g & 15) == 0;
    double acc = 0.0;
    if (aligned && cnt == kNormBlock) {
      cgfloat4* g4 = (cgfloat4*)g;
#pragma unroll
      for (int k0 = 0; k0 < kNormRounds; k0 += kNormBatch) {
        f32x4 x[kNormBatch];
#pragma unroll
        for (int k = 0; k < kNormBatch; ++k) x[k] = g4[(k0 + k) * kNormThreads + tid];
#pragma unroll
        for (int k = 0; k < kNormBatch; ++k)
#pragma unroll
          for (int e = 0; e < 4; ++e) { const double d = (double)x[k][e]; acc = acc + d * d; }
      }
    } else {
      for (int k = 0; k < kNormRounds; ++k) {
        const int64_t e = ((int64_t)k * kNormThreads + tid) * 4;
        if (e >= cnt) break;
        float x[4] = {0.f, 0.f, 0.f, 0.f};
        if (aligned && e + 4 <= cnt) {
          const f32x4 q = *(cgfloat4*)(g + e);
          x[0] = q[0]; x[1] = q[1]; x[2] = q[2]; x[3] = q[3];
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) if (e + j < cnt) x[j] = g[e + j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) { const double d = (double)x[j]; acc = acc + d * d; }
      }
    }
    sums[tid] = acc;
    __syncthreads();
#pragma unroll
    for (int w = kNormThreads / 2; w >= 1; w >>= 1) {
      if (tid < w) sums[tid] = sums[tid] + sums[tid + w];
      __syncthreads();
    }
    if (tid == 0) partials[s] = sums[0];        // (thread 0 alone touches sums[0] before the next block's first barrier)
  }
}

// total = f32(sqrt_f64(sum of the slots, ascending));  coef = min(max_norm / (total + 1e-6f), 1) with a NaN kept (torch's
// clip_grad_norm_).  One workgroup: the slots come in through LDS a tile at a time, thread 0 adds them.  out[0] = total,
// out[1] = coef.
constexpr int kNormTile = 2048;

__global__ __launch_bounds__(kNormThreads) void grad_norm_finish_kernel(const double* __restrict__ partials, int64_t n_slots,
                                                                        float max_norm, float* __restrict__ out) {
  __shared__ double tile[kNormTile];
  double sum = 0.0;
  for (int64_t t0 = 0; t0 < n_slots; t0 += kNormTile) {
    const int cnt = (int)(n_slots - t0 < kNormTile ? n_slots - t0 : kNormTile);
    for (int i = threadIdx.x; i < cnt; i += kNormThreads) tile[i] = partials[t0 + i];
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < cnt; ++i) sum = sum + tile[i];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float total = (float)sqrt(sum);
    const float q = max_norm / (total + 1e-6f);
    out[0] = total;
    out[1] = q > 1.0f ? 1.0f : q;                               // (a NaN compares false and stays)
  }
}

static int optim_cus() {
  static int cus[MAX_DEVICES] = {0};
  const int dev = current_device();
  if (cus[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cus[dev] = n;
  }
  return cus[dev];
}

template <int RULE>
static void launch_rule(bool clip, int grid, hipStream_t stream, const void* table, int rec_begin, int rec_end,
                        int64_t v_begin, int64_t n_chunks, const void* grad_base, float* s0, float* s1, int64_t state_numel,
                        const StepScalars& k, const float* coef) {
  if (clip)
    hipLaunchKernelGGL((optim_step_kernel<RULE, true>), dim3(grid), dim3(kAdamThreads), 0, stream, (const AdamRec*)table,
                       rec_begin, rec_end, v_begin, n_chunks, (const char*)grad_base, s0, s1, state_numel, k, coef);
  else
    hipLaunchKernelGGL((optim_step_kernel<RULE, false>), dim3(grid), dim3(kAdamThreads), 0, stream, (const AdamRec*)table,
                       rec_begin, rec_end, v_begin, n_chunks, (const char*)grad_base, s0, s1, state_numel, k, coef);
}

}  // namespace lidal

extern "C" int lidal_adam_chunk_elems(void) { return lidal::kAdamChunk; }
extern "C" int lidal_grad_norm_block_elems(void) { return lidal::kNormBlock; }

extern "C" int lidal_adam_step(const void* table, int rec_begin, int rec_end, int64_t v_begin, int64_t v_end,
                               const void* grad_base, float* m, float* v, int64_t state_numel, double one_minus_beta1,
                               double beta2, double one_minus_beta2, double bias_correction2_sqrt, double eps,
                               double neg_step_size, double weight_decay, void* stream) {
  using namespace lidal;
  LIDAL_REQUIRE(table != nullptr && m != nullptr && v != nullptr, "lidal_adam_step: null table or state buffer");
  LIDAL_REQUIRE(0 <= rec_begin && rec_begin <= rec_end, "lidal_adam_step: records [%d, %d)", rec_begin, rec_end);
  LIDAL_REQUIRE(v_begin >= 0 && v_begin <= v_end && state_numel >= 0, "lidal_adam_step: virtual range [%lld, %lld)",
                (long long)v_begin, (long long)v_end);
  if (rec_begin == rec_end || v_begin == v_end) return 0;
  const int64_t n_chunks = cdiv(v_end - v_begin, kAdamChunk);
  static int cus[MAX_DEVICES] = {0};
  const int dev = current_device();
  if (cus[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cus[dev] = n;
  }
  const int64_t cap = (int64_t)cus[dev] * kAdamBlocksPerCU;
  const int grid = (int)(n_chunks < cap ? n_chunks : cap);
  AdamScalars k;
  k.omb1 = (float)one_minus_beta1; k.b2 = (float)beta2; k.omb2 = (float)one_minus_beta2;
  k.bc2_sqrt = (float)bias_correction2_sqrt; k.eps = (float)eps; k.neg_step = (float)neg_step_size;
  k.wd = (float)weight_decay;
  hipLaunchKernelGGL(adam_step_kernel, dim3(grid), dim3(kAdamThreads), 0, (hipStream_t)stream, (const AdamRec*)table,
                     rec_begin, rec_end, v_begin, n_chunks, (const char*)grad_base, m, v, state_numel, k,
                     weight_decay != 0.0 ? 1 : 0);
  LIDAL_CHECK_LAUNCH("lidal_adam_step");
  return 0;
}

// [v_begin, v_end) in chunks and the grid of a step launch; 0 chunks: nothing to do
static int step_grid(int64_t v_begin, int64_t v_end, int64_t* n_chunks) {
  using namespace lidal;
  *n_chunks = cdiv(v_end - v_begin, kAdamChunk);
  const int64_t cap = (int64_t)optim_cus() * kAdamBlocksPerCU;
  return (int)(*n_chunks < cap ? *n_chunks : cap);
}

extern "C" int lidal_adam_step_ex(const void* table, int rec_begin, int rec_end, int64_t v_begin, int64_t v_end,
                                  const void* grad_base, float* m, float* v, int64_t state_numel, double one_minus_beta1,
                                  double beta2, double one_minus_beta2, double bias_correction2_sqrt, double eps,
                                  double neg_step_size, double weight_decay, int decoupled, double decay_factor,
                                  const float* clip_coef, void* stream) {
  using namespace lidal;
  LIDAL_REQUIRE(table != nullptr && m != nullptr && v != nullptr, "lidal_adam_step_ex: null table or state buffer");
  LIDAL_REQUIRE(0 <= rec_begin && rec_begin <= rec_end, "lidal_adam_step_ex: records [%d, %d)", rec_begin, rec_end);
  LIDAL_REQUIRE(v_begin >= 0 && v_begin <= v_end && state_numel >= 0, "lidal_adam_step_ex: virtual range [%lld, %lld)",
                (long long)v_begin, (long long)v_end);
  LIDAL_REQUIRE(decoupled != 0 || clip_coef != nullptr,
                "lidal_adam_step_ex: coupled weight decay without clipping is lidal_adam_step");
  if (rec_begin == rec_end || v_begin == v_end) return 0;
  int64_t n_chunks = 0;
  const int grid = step_grid(v_begin, v_end, &n_chunks);
  StepScalars k = {};
  k.a.omb1 = (float)one_minus_beta1; k.a.b2 = (float)beta2; k.a.omb2 = (float)one_minus_beta2;
  k.a.bc2_sqrt = (float)bias_correction2_sqrt; k.a.eps = (float)eps; k.a.neg_step = (float)neg_step_size;
  k.a.wd = (float)weight_decay;
  k.decay_mul = (float)decay_factor;
  k.decay = weight_decay != 0.0 ? 1 : 0;
  if (decoupled)
    launch_rule<kAdamW>(clip_coef != nullptr, grid, (hipStream_t)stream, table, rec_begin, rec_end, v_begin, n_chunks,
                        grad_base, m, v, state_numel, k, clip_coef);
  else
    launch_rule<kAdamCoupled>(true, grid, (hipStream_t)stream, table, rec_begin, rec_end, v_begin, n_chunks, grad_base, m,
                              v, state_numel, k, clip_coef);
  LIDAL_CHECK_LAUNCH("lidal_adam_step_ex");
  return 0;
}

extern "C" int lidal_sgd_step(const void* table, int rec_begin, int rec_end, int64_t v_begin, int64_t v_end,
                              const void* grad_base, float* momentum_buffer, int64_t state_numel, double momentum,
                              double one_minus_dampening, double neg_lr, double weight_decay, int nesterov, int first_step,
                              const float* clip_coef, void* stream) {
  using namespace lidal;
  LIDAL_REQUIRE(table != nullptr, "lidal_sgd_step: null table");
  LIDAL_REQUIRE(momentum == 0.0 || momentum_buffer != nullptr, "lidal_sgd_step: momentum %g without a momentum buffer",
                momentum);
  LIDAL_REQUIRE(0 <= rec_begin && rec_begin <= rec_end, "lidal_sgd_step: records [%d, %d)", rec_begin, rec_end);
  LIDAL_REQUIRE(v_begin >= 0 && v_begin <= v_end && state_numel >= 0, "lidal_sgd_step: virtual range [%lld, %lld)",
                (long long)v_begin, (long long)v_end);
  if (rec_begin == rec_end || v_begin == v_end) return 0;
  int64_t n_chunks = 0;
  const int grid = step_grid(v_begin, v_end, &n_chunks);
  StepScalars k = {};
  k.mom = (float)momentum; k.omd = (float)one_minus_dampening; k.neg_lr = (float)neg_lr; k.wd = (float)weight_decay;
  k.decay = weight_decay != 0.0 ? 1 : 0;
  k.nesterov = nesterov != 0 ? 1 : 0;
  const bool clip = clip_coef != nullptr;
  hipStream_t st = (hipStream_t)stream;
  if (momentum == 0.0)
    launch_rule<kSgdPlain>(clip, grid, st, table, rec_begin, rec_end, v_begin, n_chunks, grad_base, nullptr, nullptr, 0, k,
                           clip_coef);
  else if (first_step)
    launch_rule<kSgdFirst>(clip, grid, st, table, rec_begin, rec_end, v_begin, n_chunks, grad_base, momentum_buffer,
                           nullptr, state_numel, k, clip_coef);
  else
    launch_rule<kSgdMom>(clip, grid, st, table, rec_begin, rec_end, v_begin, n_chunks, grad_base, momentum_buffer, nullptr,
                         state_numel, k, clip_coef);
  LIDAL_CHECK_LAUNCH("lidal_sgd_step");
  return 0;
}

extern "C" int lidal_grad_norm_partials(const void* table, const int64_t* slot_start, int rec_begin, int rec_end,
                                        const void* grad_base, double* partials, int64_t n_slots, int zero, void* stream) {
  using namespace lidal;
  LIDAL_REQUIRE(table != nullptr && slot_start != nullptr && partials != nullptr,
                "lidal_grad_norm_partials: null table, slot starts or partials");
  LIDAL_REQUIRE(0 <= rec_begin && rec_begin <= rec_end && n_slots >= 0, "lidal_grad_norm_partials: records [%d, %d)",
                rec_begin, rec_end);
  if (rec_begin == rec_end || n_slots == 0) return 0;
  const int64_t cap = (int64_t)optim_cus() * 8;
  const int grid = (int)(n_slots < cap ? n_slots : cap);
  hipLaunchKernelGGL(grad_norm_partials_kernel, dim3(grid), dim3(kNormThreads), 0, (hipStream_t)stream,
                     (const AdamRec*)table, slot_start, rec_begin, rec_end, (const char*)grad_base, partials, n_slots, zero);
  LIDAL_CHECK_LAUNCH("lidal_grad_norm_partials");
  return 0;
}

extern "C" int lidal_grad_norm_finish(const double* partials, int64_t n_slots, double max_norm, float* out, void* stream) {
  using namespace lidal;
  LIDAL_REQUIRE(out != nullptr && n_slots >= 0 && (n_slots == 0 || partials != nullptr),
                "lidal_grad_norm_finish: null output or partials (%lld slots)", (long long)n_slots);
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(kNormThreads), 0, (hipStream_t)stream, partials, n_slots,
                     (float)max_norm, out);
  LIDAL_CHECK_LAUNCH("lidal_grad_norm_finish");
  return 0;
}
