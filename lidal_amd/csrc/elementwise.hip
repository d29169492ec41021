// Small fused row-wise ops of the training step for gfx950:
//   * add + ReLU of the residual blocks (network/utils.py:171), forward and backward;
//   * cross-entropy with ignore_index and mean reduction (train.py:136): forward (per-block loss
//     partials, fixed-order final sum) and backward (softmax - onehot) / n_valid in one pass each.
// All HBM-bound; 16-byte lane accesses where rows allow, f32 arithmetic.
#include "rows.h"

using namespace lidal;
using namespace lidal::rows;

namespace {

// y = max(a + b, 0)                 (n = number of VEC-wide chunks)
template <typename T>
__global__ void __launch_bounds__(256) add_relu_fwd_kernel(const T* __restrict__ a,
                                                           const T* __restrict__ b,
                                                           T* __restrict__ y, int64_t n) {
  constexpr int VEC = Vec16<T>::N;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (; i < n; i += stride) {
    float fa[VEC], fb[VEC];
    Vec16<T>::unpack(reinterpret_cast<const typename Vec16<T>::vec*>(a)[i], fa);
    Vec16<T>::unpack(reinterpret_cast<const typename Vec16<T>::vec*>(b)[i], fb);
#pragma unroll
    for (int e = 0; e < VEC; ++e) fa[e] = fmaxf(fa[e] + fb[e], 0.f);
    reinterpret_cast<typename Vec16<T>::vec*>(y)[i] = Vec16<T>::pack(fa);
  }
}

// g_in = g * (y > 0)  (the same tensor is the gradient of both summands)
template <typename T>
__global__ void __launch_bounds__(256) add_relu_bwd_kernel(const T* __restrict__ y,
                                                           const T* __restrict__ g,
                                                           T* __restrict__ gin, int64_t n) {
  constexpr int VEC = Vec16<T>::N;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (; i < n; i += stride) {
    float fy[VEC], fg[VEC];
    Vec16<T>::unpack(reinterpret_cast<const typename Vec16<T>::vec*>(y)[i], fy);
    Vec16<T>::unpack(reinterpret_cast<const typename Vec16<T>::vec*>(g)[i], fg);
#pragma unroll
    for (int e = 0; e < VEC; ++e) fg[e] = fy[e] > 0.f ? fg[e] : 0.f;
    reinterpret_cast<typename Vec16<T>::vec*>(gin)[i] = Vec16<T>::pack(fg);
  }
}

// per-row -log softmax(logits)[label]; block partial sums of loss and of the valid-row count
template <typename T>
__global__ void __launch_bounds__(256) ce_fwd_kernel(const T* __restrict__ logits,
                                                     const int64_t* __restrict__ labels, int64_t n,
                                                     int c, int64_t ignore_index,
                                                     float* __restrict__ part /*[blocks][2]*/) {
  __shared__ float red[2][256];
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float v[2] = {0.f, 0.f};              // {loss, 1} of a valid row
  if (i < n) {
    const int64_t y = labels[i];
    if (label_ok(y, c, ignore_index)) {
      const T* row = logits + i * c;
      const float xy = (float)row[y];
      float x[kMaxClasses], mx, s;
      row_exp<float>(row, c, x, mx, s);
      v[0] = logf(s) + mx - xy;
      v[1] = 1.f;
    }
  }
  block_sum<2>(v, red);
  if (threadIdx.x == 0) { part[blockIdx.x * 2] = red[0][0]; part[blockIdx.x * 2 + 1] = red[1][0]; }
}

// out[0] = sum(loss) / n_valid, out[1] = n_valid        (single block, fixed order)
__global__ void __launch_bounds__(256) ce_final_kernel(const float* __restrict__ part,
                                                       int64_t nblocks, float* __restrict__ out) {
  __shared__ double red[2][256];
  sum_partials<2>(part, nblocks, red);
  if (threadIdx.x == 0) {
    out[0] = red[1][0] > 0.0 ? (float)(red[0][0] / red[1][0]) : NAN;   // torch: nan if all ignored
    out[1] = (float)red[1][0];
  }
}

// dlogits = (softmax - onehot) * gscale / n_valid   (0 for ignored rows)
template <typename T>
__global__ void __launch_bounds__(256) ce_bwd_kernel(const T* __restrict__ logits,
                                                     const int64_t* __restrict__ labels, int64_t n,
                                                     int c, int64_t ignore_index,
                                                     const float* __restrict__ fwd_out,
                                                     const float* __restrict__ gscale,
                                                     T* __restrict__ dlogits) {
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t y = labels[i];
  T* drow = dlogits + i * c;
  if (!label_ok(y, c, ignore_index)) {
#pragma unroll
    for (int j = 0; j < kMaxClasses; ++j)
      if (j < c) drow[j] = (T)0.f;
    return;
  }
  const float k = gscale[0] / fwd_out[1];
  float x[kMaxClasses], mx, s;
  row_exp<float>(logits + i * c, c, x, mx, s);
#pragma unroll
  for (int j = 0; j < kMaxClasses; ++j)
    if (j < c) drow[j] = (T)((x[j] / s - (j == (int)y ? 1.f : 0.f)) * k);
}

static inline unsigned ew_grid(int64_t n) {
  int64_t g = cdiv(n, 256);
  return (unsigned)(g < 1 ? 1 : (g > 256 * 16 ? 256 * 16 : g));
}

}  // namespace

extern "C" int lidal_add_relu_fwd(const void* a, const void* b, void* y, int64_t numel, int dtype,
                                  void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (numel == 0) return 0;
  if (dtype == LIDAL_F32) {
    LIDAL_REQUIRE(numel % 4 == 0, "add_relu: element count must be a multiple of 4");
    add_relu_fwd_kernel<float><<<ew_grid(numel / 4), 256, 0, s>>>((const float*)a, (const float*)b,
                                                                  (float*)y, numel / 4);
  } else if (dtype == LIDAL_BF16) {
    LIDAL_REQUIRE(numel % 8 == 0, "add_relu: element count must be a multiple of 8");
    add_relu_fwd_kernel<__bf16><<<ew_grid(numel / 8), 256, 0, s>>>((const __bf16*)a, (const __bf16*)b,
                                                                   (__bf16*)y, numel / 8);
  } else {
    set_error("add_relu: bad dtype %d", dtype);
    return 2;
  }
  LIDAL_CHECK_LAUNCH("lidal_add_relu_fwd");
  return 0;
}

extern "C" int lidal_add_relu_bwd(const void* y, const void* g, void* gin, int64_t numel, int dtype,
                                  void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (numel == 0) return 0;
  if (dtype == LIDAL_F32) {
    LIDAL_REQUIRE(numel % 4 == 0, "add_relu: element count must be a multiple of 4");
    launch_tail(add_relu_bwd_kernel<float>, dim3(ew_grid(numel / 4)), dim3(256), 0, s, (const float*)y, (const float*)g,
                (float*)gin, numel / 4);
  } else if (dtype == LIDAL_BF16) {
    LIDAL_REQUIRE(numel % 8 == 0, "add_relu: element count must be a multiple of 8");
    launch_tail(add_relu_bwd_kernel<__bf16>, dim3(ew_grid(numel / 8)), dim3(256), 0, s, (const __bf16*)y, (const __bf16*)g,
                (__bf16*)gin, numel / 8);
  } else {
    set_error("add_relu: bad dtype %d", dtype);
    return 2;
  }
  LIDAL_CHECK_LAUNCH("lidal_add_relu_bwd");
  return 0;
}

extern "C" int64_t lidal_ce_workspace_bytes(int64_t n) { return cdiv(n > 0 ? n : 1, 256) * 8 + 256; }

extern "C" int lidal_ce_fwd(const void* logits, int dtype, const int64_t* labels, int64_t n, int c,
                            int64_t ignore_index, float* out2, void* ws, int64_t ws_bytes,
                            void* stream) {
  hipStream_t s = (hipStream_t)stream;
  LIDAL_REQUIRE(c > 0 && c <= kMaxClasses, "cross_entropy: classes must be in 1..%d", kMaxClasses);
  LIDAL_REQUIRE(ws_bytes >= lidal_ce_workspace_bytes(n), "cross_entropy workspace too small");
  int64_t blocks = cdiv(n > 0 ? n : 1, 256);
  if (int rc = with_dtype(dtype, "cross_entropy", [&](auto t) {
        using T = decltype(t);
        ce_fwd_kernel<T><<<(unsigned)blocks, 256, 0, s>>>((const T*)logits, labels, n, c, ignore_index, (float*)ws);
        LIDAL_CHECK_LAUNCH("ce_fwd");
        return 0;
      }))
    return rc;
  ce_final_kernel<<<1, 256, 0, s>>>((const float*)ws, blocks, out2);
  LIDAL_CHECK_LAUNCH("ce_final");
  return 0;
}

extern "C" int lidal_ce_bwd(const void* logits, int dtype, const int64_t* labels, int64_t n, int c,
                            int64_t ignore_index, const float* fwd_out2, const float* grad_scale,
                            void* dlogits, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  LIDAL_REQUIRE(c > 0 && c <= kMaxClasses, "cross_entropy: classes must be in 1..%d", kMaxClasses);
  if (n == 0) return 0;
  return with_dtype(dtype, "cross_entropy", [&](auto t) {
    using T = decltype(t);
    ce_bwd_kernel<T><<<(unsigned)cdiv(n, 256), 256, 0, s>>>((const T*)logits, labels, n, c, ignore_index, fwd_out2,
                                                            grad_scale, (T*)dlogits);
    LIDAL_CHECK_LAUNCH("ce_bwd");
    return 0;
  });
}
