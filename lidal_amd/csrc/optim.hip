// The optimizer step for any number of f32 parameter tensors in ONE launch (train.py:56,140: optimizer.step()): one
// kernel, optim_step_kernel<RULE, CLIP>, over the record table, virtual axis, chunk walk and piece mover of
// multi_tensor.h, with the update RULE as a template argument and the arrays a rule has no use for left alone --
//
//   kAdamCoupled / kAdamW   p, g, m, v   torch's _single_tensor_adam (adam_update below); kAdamW runs p = p * (1 - lr * wd)
//                                        first and then the five lines with g = grad (decoupled_weight_decay=True)
//   kSgdPlain               p, g         torch's _single_tensor_sgd, momentum == 0: no state, no state traffic
//   kSgdFirst               p, g, buf    the first step of a parameter: buf = g (buf is written, never read)
//   kSgdMom                 p, g, buf    buf = buf * mom + (1 - dampening) * g
//                                        then g = g + mom * buf (nesterov) or g = buf;  p = p + (-lr) * g
//
// CLIP: g = grad * coef before anything else, coef read from the device (grad_norm_finish_kernel below wrote it), also
// when coef == 1; `.grad` itself is not written.  Weight decay and Nesterov are uniform scalar branches.
//
// Every operation is rounded separately in f32 -- this unit is compiled with -ffp-contract=off (build.py NO_CONTRACT),
// `/` and sqrtf are the compiler's correctly rounded forms, subnormals are kept (tests/adam_ref.py and
// tests/optim_ref.py restate the rules in numpy, bit for bit).
//
// Further down: the global gradient norm with its clip coefficient formed on the device (grad_norm_partials_kernel,
// grad_norm_finish_kernel).
#include "multi_tensor.h"

#pragma clang fp contract(off)

namespace lidal {

using multi_tensor::kChunk;
using multi_tensor::kThreads;

struct AdamRec {            // five 64-bit words: the table's record
  uint64_t p;               // address of the parameter
  int64_t g;                // gradient: byte offset from the `grad_base` of the launch (absolute address: base 0)
  int64_t state;            // first element of its m / v in the two flat state buffers
  int64_t vstart;           // first element on the virtual axis (ascending with the record index, no overlap)
  int64_t n;                // elements
};

typedef multi_tensor::Vec4<float> f32x4;
typedef LIDAL_GLOBAL float gfloat;
typedef LIDAL_GLOBAL const float cgfloat;
typedef LIDAL_GLOBAL const f32x4 cgfloat4;

struct AdamScalars { float omb1, b2, omb2, bc2_sqrt, eps, neg_step, wd; };

//     g   = grad                                   (weight_decay != 0:  g = grad + wd * p)
//     m   = m + (g - m) * (1 - beta1)
//     v   = v * beta2 + ((1 - beta2) * g) * g
//     den = sqrtf(v) / sqrt(1 - beta2^t) + eps
//     p   = p + (-(lr / (1 - beta1^t))) * (m / den)
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, const AdamScalars& k, bool decay) {
  if (decay) g = g + k.wd * p;
  m = m + (g - m) * k.omb1;
  v = v * k.b2 + (k.omb2 * g) * g;
  const float den = sqrtf(v) / k.bc2_sqrt + k.eps;
  p = p + k.neg_step * (m / den);
}

enum { kAdamCoupled = 0, kAdamW = 1, kSgdPlain = 2, kSgdFirst = 3, kSgdMom = 4 };

struct StepScalars {
  AdamScalars a;                      // kAdamCoupled / kAdamW
  float decay_mul;                    // kAdamW: 1 - lr * wd
  float mom, omd, neg_lr, wd;         // SGD: momentum, 1 - dampening, -lr, weight decay
  int decay, nesterov;
};

// A rule for multi_tensor::move_piece.  Its arrays: 0 the parameter, 1 the gradient (never written), then its state.
template <int RULE, bool CLIP> struct StepRule {
  typedef float Elem;
  static constexpr int kStates = RULE <= kAdamW ? 2 : (RULE == kSgdPlain ? 0 : 1);
  static constexpr int kArrays = 2 + kStates;
  static constexpr unsigned kLoads = RULE == kSgdFirst ? 3u : (1u << kArrays) - 1;
  static constexpr unsigned kStores = ((1u << kArrays) - 1) & ~2u;
  const StepScalars& k;
  float coef;

  __device__ __forceinline__ void update(float (&x)[kArrays]) const {
    float g = x[1];
    if constexpr (CLIP) g = g * coef;
    if constexpr (RULE == kAdamCoupled) {
      adam_update(x[0], g, x[2], x[3], k.a, k.decay != 0);
    } else if constexpr (RULE == kAdamW) {
      x[0] = x[0] * k.decay_mul;
      adam_update(x[0], g, x[2], x[3], k.a, false);
    } else {
      if (k.decay) g = g + k.wd * x[0];
      if constexpr (RULE == kSgdFirst) x[2] = g;
      if constexpr (RULE == kSgdMom) x[2] = x[2] * k.mom + k.omd * g;
      if constexpr (RULE != kSgdPlain) g = k.nesterov ? g + k.mom * x[2] : x[2];
      x[0] = x[0] + k.neg_lr * g;
    }
  }
};

template <int RULE, bool CLIP>
__global__ __launch_bounds__(kThreads) void optim_step_kernel(const AdamRec* __restrict__ recs, int r0, int r1,
                                                              int64_t v_begin, int64_t n_chunks, const char* grad_base,
                                                              float* s0, float* s1, int64_t state_numel, StepScalars k,
                                                              const float* __restrict__ coef_ptr) {
  typedef StepRule<RULE, CLIP> Rule;
  float coef = 1.0f;
  if constexpr (CLIP) coef = *coef_ptr;
  const Rule rule = {k, coef};
  multi_tensor::walk_chunks(recs, r0, r1, v_begin, n_chunks, [&](const AdamRec R, int64_t a, int64_t e) {
    if (R.n <= 0) return;
    if (Rule::kStates > 0 && (R.state < 0 || R.state + R.n > state_numel)) return;     // never outside the state buffers
    multi_tensor::Arrays<Rule> A;
    A.p[0] = (gfloat*)R.p;
    A.p[1] = (gfloat*)((uintptr_t)grad_base + (uintptr_t)R.g);
    if constexpr (Rule::kStates >= 1) A.p[2] = (gfloat*)(uintptr_t)(s0 + R.state);
    if constexpr (Rule::kStates >= 2) A.p[3] = (gfloat*)(uintptr_t)(s1 + R.state);
    multi_tensor::move_piece(rule, A, a, e);
  });
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

// one step launch of RULE over the non-empty virtual range [v_begin, v_end)
template <int RULE>
static void launch_rule(const float* coef, hipStream_t stream, const void* table, int rec_begin, int rec_end, int64_t v_begin,
                        int64_t v_end, const void* grad_base, float* s0, float* s1, int64_t state_numel,
                        const StepScalars& k) {
  const int64_t n_chunks = cdiv(v_end - v_begin, kChunk);
  const int grid = multi_tensor::grid_for(n_chunks);
  if (coef != nullptr)
    hipLaunchKernelGGL((optim_step_kernel<RULE, true>), dim3(grid), dim3(kThreads), 0, stream, (const AdamRec*)table,
                       rec_begin, rec_end, v_begin, n_chunks, (const char*)grad_base, s0, s1, state_numel, k, coef);
  else
    hipLaunchKernelGGL((optim_step_kernel<RULE, false>), dim3(grid), dim3(kThreads), 0, stream, (const AdamRec*)table,
                       rec_begin, rec_end, v_begin, n_chunks, (const char*)grad_base, s0, s1, state_numel, k, coef);
}

static StepScalars adam_scalars(double one_minus_beta1, double beta2, double one_minus_beta2, double bias_correction2_sqrt,
                                double eps, double neg_step_size, double weight_decay) {
  StepScalars k = {};
  k.a.omb1 = (float)one_minus_beta1; k.a.b2 = (float)beta2; k.a.omb2 = (float)one_minus_beta2;
  k.a.bc2_sqrt = (float)bias_correction2_sqrt; k.a.eps = (float)eps; k.a.neg_step = (float)neg_step_size;
  k.a.wd = (float)weight_decay;
  k.decay = weight_decay != 0.0 ? 1 : 0;
  return k;
}

}  // namespace lidal

extern "C" int lidal_adam_chunk_elems(void) { return lidal::kChunk; }
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
  const StepScalars k = adam_scalars(one_minus_beta1, beta2, one_minus_beta2, bias_correction2_sqrt, eps, neg_step_size,
                                     weight_decay);
  launch_rule<kAdamCoupled>(nullptr, (hipStream_t)stream, table, rec_begin, rec_end, v_begin, v_end, grad_base, m, v,
                            state_numel, k);
  LIDAL_CHECK_LAUNCH("lidal_adam_step");
  return 0;
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
  StepScalars k = adam_scalars(one_minus_beta1, beta2, one_minus_beta2, bias_correction2_sqrt, eps, neg_step_size,
                               weight_decay);
  k.decay_mul = (float)decay_factor;
  if (decoupled)
    launch_rule<kAdamW>(clip_coef, (hipStream_t)stream, table, rec_begin, rec_end, v_begin, v_end, grad_base, m, v,
                        state_numel, k);
  else
    launch_rule<kAdamCoupled>(clip_coef, (hipStream_t)stream, table, rec_begin, rec_end, v_begin, v_end, grad_base, m, v,
                              state_numel, k);
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
  StepScalars k = {};
  k.mom = (float)momentum; k.omd = (float)one_minus_dampening; k.neg_lr = (float)neg_lr; k.wd = (float)weight_decay;
  k.decay = weight_decay != 0.0 ? 1 : 0;
  k.nesterov = nesterov != 0 ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  if (momentum == 0.0)
    launch_rule<kSgdPlain>(clip_coef, st, table, rec_begin, rec_end, v_begin, v_end, grad_base, nullptr, nullptr, 0, k);
  else if (first_step)
    launch_rule<kSgdFirst>(clip_coef, st, table, rec_begin, rec_end, v_begin, v_end, grad_base, momentum_buffer, nullptr,
                           state_numel, k);
  else
    launch_rule<kSgdMom>(clip_coef, st, table, rec_begin, rec_end, v_begin, v_end, grad_base, momentum_buffer, nullptr,
                         state_numel, k);
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
  const int64_t cap = (int64_t)multi_tensor::device_cus() * 8;
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
