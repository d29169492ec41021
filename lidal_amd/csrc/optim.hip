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

}  // namespace lidal

extern "C" int lidal_adam_chunk_elems(void) { return lidal::kAdamChunk; }

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
