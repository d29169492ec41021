// Counter-based dropout: the mask is a pure function of (seed, call, element index), so nothing
// is kept for the backward pass -- it is the same call on the gradient -- and a numpy restatement gives the same bits
// (tests/dropout_ref.py).  Replaces, for models that opt in, torch's nn.Dropout(p, inplace=True) at SPVCNN's two sites
// (network/spvcnn.py:139,147: bernoulli_ + div_ + mul_ and a tensor-sized noise buffer held until backward).
//
// Element e = first + i of the tensor takes word e & 3 of Philox4x32-10 under key (seed lo, seed hi) and counter
// (g lo, g hi, call lo, call hi), g = e >> 2; it is kept iff that word is below thr.  One 32-bit word per element, ten
// rounds (two 32 x 32 -> 64 multiplies each): a 16-byte vector of f32 is one generator call, one of bf16 two.
#include "common.h"
#include "rows.h"

using namespace lidal;
using lidal::rows::Vec16;

namespace {

struct Philox4 { uint32_t w[4]; };

__host__ __device__ __forceinline__ uint32_t mulhi32(uint32_t a, uint32_t b) {
  return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
}

// Philox4x32-10 (Salmon et al., SC'11; Random123's constants)
__host__ __device__ __forceinline__ Philox4 philox4x32_10(uint64_t g, uint64_t call, uint64_t seed) {
  uint32_t c0 = (uint32_t)g, c1 = (uint32_t)(g >> 32), c2 = (uint32_t)call, c3 = (uint32_t)(call >> 32);
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = mulhi32(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = mulhi32(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

constexpr int kBlock = 256;
constexpr int kMaxBlocks = 2048;        // 256 CUs x 8 workgroups; the vectors beyond one grid take further trips

// x[i] = (T)((float)x[i] * (kept ? scale : 0.0f)) over n elements at 16-byte aligned x; g0 = first >> 2 (first % 8 == 0,
// so a vector never straddles a generator call).  The n % N elements behind the last whole vector go to the first
// threads of workgroup 0, one element each.
template <typename T>
__global__ void __launch_bounds__(kBlock) dropout_apply_kernel(T* __restrict__ x, int64_t n, uint64_t g0, uint64_t seed,
                                                               uint64_t call, uint32_t thr, float scale) {
  constexpr int N = Vec16<T>::N;
  typedef typename Vec16<T>::vec vec;
  const int64_t nv = n / N;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < nv; j += stride) {
    float f[N];
    Vec16<T>::unpack(reinterpret_cast<const vec*>(x)[j], f);
#pragma unroll
    for (int h = 0; h < N / 4; ++h) {
      const Philox4 u = philox4x32_10(g0 + (uint64_t)j * (N / 4) + h, call, seed);
#pragma unroll
      for (int k = 0; k < 4; ++k) f[4 * h + k] = f[4 * h + k] * (u.w[k] < thr ? scale : 0.0f);
    }
    reinterpret_cast<vec*>(x)[j] = Vec16<T>::pack(f);
  }
  const int64_t t = nv * N + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < N && t < n) {
    const uint64_t e = (g0 << 2) + (uint64_t)t;
    const Philox4 u = philox4x32_10(e >> 2, call, seed);
    const int k = (int)(e & 3);
    const uint32_t word = k == 0 ? u.w[0] : k == 1 ? u.w[1] : k == 2 ? u.w[2] : u.w[3];
    x[t] = (T)((float)x[t] * (word < thr ? scale : 0.0f));
  }
}

}  // namespace

extern "C" int lidal_dropout_apply(void* x, int64_t n_elems, int dtype, int64_t first, int64_t seed, int64_t call,
                                   int64_t thr, double scale, void* stream) {
  LIDAL_REQUIRE(n_elems >= 0, "dropout_apply: negative element count %lld", (long long)n_elems);
  LIDAL_REQUIRE(first >= 0 && first % 8 == 0, "dropout_apply: first (%lld) must be a non-negative multiple of 8",
                (long long)first);
  LIDAL_REQUIRE(thr >= 0 && thr < (1ll << 32), "dropout_apply: thr (%lld) must be in [0, 2^32)", (long long)thr);
  LIDAL_REQUIRE(((uintptr_t)x & 15) == 0, "dropout_apply: the tensor must be 16-byte aligned");
  return with_dtype(dtype, "dropout_apply", [&](auto tag) {
    typedef decltype(tag) T;
    if (n_elems == 0) return 0;
    LIDAL_REQUIRE(x != nullptr, "dropout_apply: null tensor");
    const int64_t nv = n_elems / Vec16<T>::N;
    const int64_t blocks = cdiv(nv, kBlock);
    const unsigned grid = (unsigned)(blocks < 1 ? 1 : (blocks > kMaxBlocks ? kMaxBlocks : blocks));
    launch_tail(dropout_apply_kernel<T>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, (T*)x, n_elems,
                (uint64_t)first >> 2, (uint64_t)seed, (uint64_t)call, (uint32_t)thr, (float)scale);
    LIDAL_CHECK_LAUNCH("lidal_dropout_apply");
    return 0;
  });
}
