// BatchNorm over the rows of a [N, C] feature matrix (spnn.BatchNorm = nn.BatchNorm1d on .feats,
// network/utils.py:115, 49 instances per model) for gfx950.
//
// HBM-bound: training forward reads x twice (statistics, normalise) and writes y once; backward
// reads x and dy twice and writes dx once.  All accesses are 16-byte lane loads covering whole
// rows; per-channel reductions are hierarchical (thread -> LDS tree -> per-workgroup partial ->
// one combining workgroup) with Chan's parallel-variance merge on SHIFTED sums, so the variance does
// not cancel when |mean| >> std, and the order is fixed (bitwise reproducible, no atomics).
//
// The file is built from a few pieces that the kernels share: a thread's place in its slab (Slab), the row walk
// (walk_rows; the note there lists the kernels that keep a loop of their own or are written out in full, and why), the
// element forms (apply_piece, dx_piece, xhat_and_mask + add_sum_terms), the reducing epilogue store_partials_f64 and the
// three merges (merge_tile_stats, merge_tile_sums, merge_partial_sums), which the stand-alone merge kernels and the
// first workgroups of their consumers both call.
#include "common.h"
#include <type_traits>

using namespace lidal;

namespace {

constexpr int NT = 256;
// row loads in flight per thread (per operand), in every kernel family: statistics pass, normalising pass, backward
// sums, dx (8 in any of them measured in round 5, profiles/README.md "BatchNorm backward": families 3.77 ->
// 3.77-3.82 ms, not kept)
constexpr int UNR = 4;
constexpr int MIN_ROWS_PER_WG = 32;    // rows per workgroup (one statistics partial each), at least

template <typename T> struct IO;
template <> struct IO<float> {
  static constexpr int VEC = 4;
  typedef float4 vec;
  __device__ static void unpack(const vec& v, float (&f)[4]) { f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w; }
  __device__ static vec pack(const float (&f)[4]) { return make_float4(f[0], f[1], f[2], f[3]); }
};
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
template <> struct IO<__bf16> {
  static constexpr int VEC = 8;
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

// VEC consecutive per-channel values (a thread's channel group), or `dflt` for a NULL array.  One uniform branch per array
// and 16-byte loads where the array allows: rounds 1-4 loaded them one element at a time behind a NULL test each -- and
// tested the ReLU / residual flags per element inside the row loops (36 scalar branches per 16-byte piece in the ISA of
// the apply kernel).  The flags are template parameters of the element-wise kernels since round 5.
template <int VEC>
__device__ __forceinline__ void load_channels(const float* __restrict__ p, int off, float dflt, float (&o)[VEC]) {
  if (p == nullptr) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) o[i] = dflt;
  } else if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
#pragma unroll
    for (int i = 0; i < VEC; i += 4) {
      const float4 v = *reinterpret_cast<const float4*>(p + off + i);
      o[i] = v.x; o[i + 1] = v.y; o[i + 2] = v.z; o[i + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < VEC; ++i) o[i] = p[off + i];
  }
}

// merge (nb, mb, M2b) into (na, ma, M2a)  -- Chan et al.
__device__ __forceinline__ void chan_merge(double& na, double& ma, double& m2a, double nb, double mb,
                                           double m2b) {
  if (nb == 0.) return;
  double n = na + nb;
  double d = mb - ma;
  ma = ma + d * (nb / n);
  m2a = m2a + m2b + d * d * (na * nb / n);
  na = n;
}

// ---- a thread's place in its slab ----
// Thread layout shared by every row kernel below: thread t of a 256-thread workgroup owns channel
// group t % cg_n (VEC consecutive channels from `col` = one 16-byte access) and row lane rl = t / cg_n; the
// workgroup owns rows [blockIdx.x * rpw, ...) and row lane rl walks rows rl, rl+rpi, ...
// (rpi = 256 / cg_n rows per sweep; lanes rl >= rpi are idle).  Consecutive threads touch consecutive 16-byte pieces
// of a row, then the next row: fully coalesced, and no per-element div/mod.
struct Slab {
  int cg_n, rpi, col, rl;
  int64_t r_beg, r_end;
};
template <int VEC>
__device__ inline Slab slab_of(int c, int64_t n, int rpw) {
  Slab g;
  g.cg_n = c / VEC; g.rpi = NT / g.cg_n;
  g.col = ((int)threadIdx.x % g.cg_n) * VEC; g.rl = (int)threadIdx.x / g.cg_n;
  g.r_beg = (int64_t)blockIdx.x * rpw;
  g.r_end = (g.r_beg + rpw < n) ? g.r_beg + rpw : n;
  return g;
}

// ---- the row walk ----
// Up to four row operands with their own row strides (elements).  A row lane takes U rows at a time -- U independent
// 16-byte loads in flight per operand -- as long as U sweeps fit its slab, then one row at a time; body(r, v) gets the
// K pieces of row r.  Idle lanes return at once.
//   TWO_BATCHES: the loads of batch i + 1 are requested before batch i is handed to the body (same rows, same order
//     per thread: the sums are those of the plain loop).
// Used by bn_stats_partial_kernel, bn_apply_kernel, bn_bwd_partial_kernel and bn_bwd_dx_kernel.  Six kernels keep a loop
// of their own.  bn_apply_tiles_kernel and bn_bwd_dx_merge_kernel request their first batch before the merged values
// are waited for and share everything but the loop.  bn_bwd_slab_sums_kernel, bn_bwd_partial_masked_kernel,
// tail_tile_sums_kernel and colsum_partial_kernel are written out in full, geometry and epilogue included: behind this
// function (or behind slab_of alone, in the column sums) the same rows and the same arithmetic came out of the
// compiler in another schedule -- the bf16 instances requested part of a batch, waited, and requested the rest one
// load at a time (5 + 3 of 8 in the slab sums, 9 + 7 of 16 in the column sums) -- and measured 1 to 3 us slower per
// launch (profiles/README.md, "BatchNorm").  The helpers here are `inline`, not forced: inlined before the optimiser
// ran, bn_apply_kernel<bf16> took 125 VGPRs for the parent's 92.
template <typename T> struct RowOps { const T* p[4]; int64_t ld[4]; };
template <typename T>
__device__ inline typename IO<T>::vec load_piece(const T* p, int64_t ld, const Slab& g, int64_t r) {
  return *reinterpret_cast<const typename IO<T>::vec*>(p + r * ld + g.col);
}

template <int U, int K, bool TWO_BATCHES = false, typename T, typename Body>
__device__ inline void walk_rows(const Slab& g, const RowOps<T>& o, Body&& body) {
  typedef typename IO<T>::vec V;
  const int rpi = g.rpi;
  auto load = [&](V (&v)[K], int64_t r) {
#pragma unroll
    // (not load_piece: through it bn_bwd_partial_kernel<float> took 132 VGPRs for 116 and lost a wave per SIMD)
    for (int k = 0; k < K; ++k) v[k] = *reinterpret_cast<const V*>(o.p[k] + r * o.ld[k] + g.col);
  };
  auto load_batch = [&](V (&v)[U][K], int64_t r) {
#pragma unroll
    for (int u = 0; u < U; ++u) load(v[u], r + u * rpi);
  };
  auto run_batch = [&](const V (&v)[U][K], int64_t r) {
#pragma unroll
    for (int u = 0; u < U; ++u) body(r + u * rpi, v[u]);
  };
  const int64_t fit_end = g.r_end - (U - 1) * rpi;           // a batch from row r fits the slab iff r < fit_end
  auto fits = [&](int64_t r) { return r < fit_end; };
  int64_t r = g.r_beg + g.rl;
  V v[U][K];
  if (g.rl >= rpi) return;
  if (TWO_BATCHES) {
    if (fits(r)) {
      V w[U][K];
      load_batch(v, r);
      int64_t rv = r;
      r += U * rpi;
      while (fits(r)) {
        load_batch(w, r);
        run_batch(v, rv);
        rv = r;
        r += U * rpi;
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
          for (int k = 0; k < K; ++k) v[u][k] = w[u][k];
        }
      }
      run_batch(v, rv);
    }
  } else {
    for (; fits(r); r += U * rpi) {
      load_batch(v, r);
      run_batch(v, r);
    }
  }
  for (; r < g.r_end; r += rpi) {
    load(v[0], r);
    body(r, v[0]);
  }
}

template <typename T>
__device__ inline void store_piece(T* __restrict__ p, int64_t ld, const Slab& g, int64_t r,
                                            const typename IO<T>::vec& v) {
  *reinterpret_cast<typename IO<T>::vec*>(p + r * ld + g.col) = v;
}

// ---- element forms ----
// The ReLU / residual flags of the normalising pass select one of six specialised copies of the row loops: F bit 0 =
// ReLU on the normalised value, bit 1 = a residual is added, bit 2 = ReLU after the sum.
__host__ __device__ __forceinline__ int apply_flags(int relu, bool has_res) {
  return (relu & 1) | (has_res ? 2 : 0) | ((has_res && (relu & 2)) ? 4 : 0);
}
template <typename Fn>
__host__ __device__ __forceinline__ void with_apply_flags(int flags, Fn&& fn) {
  switch (flags) {
    case 0: fn(std::integral_constant<int, 0>{}); break;
    case 1: fn(std::integral_constant<int, 1>{}); break;
    case 2: fn(std::integral_constant<int, 2>{}); break;
    case 3: fn(std::integral_constant<int, 3>{}); break;
    case 6: fn(std::integral_constant<int, 6>{}); break;
    default: fn(std::integral_constant<int, 7>{}); break;
  }
}

// y = (x - mean) * invstd * gamma + beta  ==  (x - mu) * sc + sh   (per-channel mu, sc, sh held in registers)
// With a residual: y = act(...) rounded to T, + res -- the sum of the point branch
// (network/spvcnn.py:104 `z1.F = z1.F + point_transforms(z.F)`) without a pass of its own, and
// relu(bn(x) + shortcut), the end of a residual block (network/utils.py:171 `relu(net(x) + downsample(x))`).
template <typename T, int F, int VEC>
__device__ inline typename IO<T>::vec apply_piece(const typename IO<T>::vec& v, const typename IO<T>::vec& vr,
                                                           const float (&mu)[VEC], const float (&sc)[VEC],
                                                           const float (&sh)[VEC]) {
  constexpr bool RELU1 = (F & 1) != 0, HAS_RES = (F & 2) != 0, RELU2 = (F & 4) != 0;
  float f[VEC], fr[VEC];
  IO<T>::unpack(v, f);
  if (HAS_RES) IO<T>::unpack(vr, fr);
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    f[i] = (f[i] - mu[i]) * sc[i] + sh[i];
    if (RELU1) f[i] = fmaxf(f[i], 0.f);
    if (HAS_RES) {
      f[i] = (float)(T)f[i] + fr[i];       // as the stand-alone sum of two T rows
      if (RELU2) f[i] = fmaxf(f[i], 0.f);
    }
  }
  return IO<T>::pack(f);
}

// what the backward kernels hold per channel: mean, invstd, gamma, beta
template <int VEC> struct Channels {
  float mu[VEC], is[VEC], ga[VEC], be[VEC];
  __device__ __forceinline__ void load(const float* mean, const float* invstd, const float* gamma, const float* beta,
                                       int col) {
    load_channels<VEC>(mean, col, 0.f, mu);
    load_channels<VEC>(invstd, col, 0.f, is);
    load_channels<VEC>(gamma, col, 1.f, ga);
    load_channels<VEC>(beta, col, 0.f, be);
  }
};

// xhat of channel i of the piece and, behind a fused ReLU, dy where y > 0
template <int VEC>
__device__ inline float xhat_and_mask(bool relu, const Channels<VEC>& k, int i, float fx, float& fd) {
  const float xhat = (fx - k.mu[i]) * k.is[i];
  if (relu && !(xhat * k.ga[i] + k.be[i] > 0.f)) fd = 0.f;
  return xhat;
}

// dx = gamma * invstd * (dy - sum_dy/n - xhat * sum_dy_xhat/n)      (k1 = sum_dy / n, k2 = sum_dy_xhat / n)
template <typename T, bool RELU, int VEC>
__device__ inline typename IO<T>::vec dx_piece(const typename IO<T>::vec& vx, const typename IO<T>::vec& vd,
                                                        const Channels<VEC>& k, const float (&k1)[VEC],
                                                        const float (&k2)[VEC]) {
  float fx[VEC], fd[VEC];
  IO<T>::unpack(vx, fx);
  IO<T>::unpack(vd, fd);
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    const float xhat = xhat_and_mask(RELU, k, i, fx[i], fd[i]);
    fd[i] = k.ga[i] * k.is[i] * (fd[i] - k1[i] - xhat * k2[i]);
  }
  return IO<T>::pack(fd);
}

// the backward-sum terms of an element in the accumulator's width: a += dy, b += dy * xhat
template <typename Acc>
__device__ inline void add_sum_terms(float fd, float xhat, Acc& a, Acc& b) {
  a += (Acc)fd;
  b += (Acc)fd * (Acc)xhat;
}

// ---- reducing epilogue ----
// LDS tree sum over the row lanes of each channel group: v[tid*VEC+i] += ... ; result in rl == 0
template <int VEC, typename A>
__device__ __forceinline__ void tree_sum_rows(A* v, int tid, int cg_n, int rpi, int rl) {
  int span = 1;
  while (span < rpi) span <<= 1;
  for (int s = span >> 1; s >= 1; s >>= 1) {
    __syncthreads();
    if (rl < s && rl + s < rpi) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) v[tid * VEC + i] += v[(tid + s * cg_n) * VEC + i];
    }
  }
  __syncthreads();
}

// per-thread f64 sums -> one (a, b) pair per (workgroup, channel), [part][c][2].  sh: [2][NT][VEC] doubles
template <int VEC>
__device__ inline void store_partials_f64(double* sh, const Slab& g, const double (&a)[VEC],
                                                   const double (&b)[VEC], int c, double* __restrict__ part) {
  const int tid = threadIdx.x;
  double* sa = sh; double* sb = sh + NT * VEC;
#pragma unroll
  for (int i = 0; i < VEC; ++i) { sa[tid * VEC + i] = a[i]; sb[tid * VEC + i] = b[i]; }
  tree_sum_rows<VEC, double>(sa, tid, g.cg_n, g.rpi, g.rl);
  tree_sum_rows<VEC, double>(sb, tid, g.cg_n, g.rpi, g.rl);
  if (g.rl == 0) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      double* dst = part + ((int64_t)blockIdx.x * c + g.col + i) * 2;
      dst[0] = sa[tid * VEC + i]; dst[1] = sb[tid * VEC + i];
    }
  }
}

// ---- statistics: per-workgroup partial (count, mean, M2) per channel ----
// All threads of the workgroup shift by the SAME value (the slab's first row), so inside the slab
// plain sums of (x-K) and (x-K)^2 can be added; only slabs are merged with Chan's formula.
// Every sum of this file is ACCUMULATED IN F64 (per thread, in the LDS tree, across slabs): the
// kernels are HBM-bound, the f64 adds are free, and the reductions then carry no summation error
// at all -- what is left is the f32 rounding of each term.  (With f32 accumulation the gradient of
// one BatchNorm gamma of the 49-layer golden model was off by 1.2e-3 against the f64 reference,
// 4x the error of the f32 CPU oracle: an ill-conditioned sum(dy * xhat), see tests/test_ops_gpu.py.)
template <typename T>
__global__ void __launch_bounds__(NT) bn_stats_partial_kernel(const T* __restrict__ x, int64_t n,
                                                              int c, double* __restrict__ part, int rpw) {
  constexpr int VEC = IO<T>::VEC;
  typedef typename IO<T>::vec V;
  extern __shared__ double sh[];                // [2][NT][VEC]
  const Slab g = slab_of<VEC>(c, n, rpw);
  const int tid = threadIdx.x;
  // f32 rows: x - K between two f32 values ROUNDS (2^-24 |x - K| a term), which a column whose mean is small beside its
  // spread shows in save_mean (46 ulp on 31 rows, 512 on two: tests/test_batchnorm_edges_gpu.py).  The mean is therefore
  // taken from a third sum of the differences in f64, where they are exact.  M2 stays the sum over the f32 differences
  // about THEIR OWN mean (s2 - s1^2 / count): the exact M2 of values 2^-24 away from the data, inside invstd's bound,
  // and the bits it always had.  Between two bf16 values the f32 difference is exact (unless the exponents lie 16
  // binades apart) and nothing changes.
  constexpr bool EXACT1 = sizeof(T) == 4;
  float shift[VEC];
  double s1[VEC], s2[VEC], sx[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) { shift[i] = 0.f; s1[i] = 0.; s2[i] = 0.; sx[i] = 0.; }
  if (g.rl < g.rpi) IO<T>::unpack(*reinterpret_cast<const V*>(x + g.r_beg * c + g.col), shift);
  walk_rows<UNR, 1>(g, RowOps<T>{{x}, {c}}, [&](int64_t, const V (&v)[1]) {
    float f[VEC];
    IO<T>::unpack(v[0], f);
#pragma unroll
    for (int i = 0; i < VEC; ++i) { float d = f[i] - shift[i]; s1[i] += (double)d; s2[i] += (double)d * (double)d; if (EXACT1) sx[i] += (double)f[i] - (double)shift[i]; }
  });
  double* a1 = sh; double* a2 = sh + NT * VEC;
#pragma unroll
  for (int i = 0; i < VEC; ++i) { a1[tid * VEC + i] = s1[i]; a2[tid * VEC + i] = s2[i]; }
  tree_sum_rows<VEC, double>(a1, tid, g.cg_n, g.rpi, g.rl);
  tree_sum_rows<VEC, double>(a2, tid, g.cg_n, g.rpi, g.rl);
  double t1[VEC], t2[VEC], tx[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) { t1[i] = a1[tid * VEC + i]; t2[i] = a2[tid * VEC + i]; tx[i] = t1[i]; }
  if (EXACT1) {           // (a thread rewrites its own slot only, and every read of the first tree lies behind a barrier)
#pragma unroll
    for (int i = 0; i < VEC; ++i) a1[tid * VEC + i] = sx[i];
    tree_sum_rows<VEC, double>(a1, tid, g.cg_n, g.rpi, g.rl);
#pragma unroll
    for (int i = 0; i < VEC; ++i) tx[i] = a1[tid * VEC + i];
  }
  if (g.rl == 0) {
    const double cnt = (double)(g.r_end - g.r_beg);
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      double d = t1[i] / cnt, m2 = t2[i] - t1[i] * d;
      double* dst = part + ((int64_t)blockIdx.x * c + g.col + i) * 3;
      dst[0] = cnt; dst[1] = (double)shift[i] + (EXACT1 ? tx[i] / cnt : d); dst[2] = m2 < 0. ? 0. : m2;
    }
  }
}

// mean / invstd of a channel from its merged (count, mean, M2), and the running statistics exactly as
// torch.nn.BatchNorm1d (biased var to normalise, unbiased for running_var)
__device__ inline void write_stats(int ch, double n, double m, double m2, float eps, float momentum,
                                            float* __restrict__ mean, float* __restrict__ invstd,
                                            float* __restrict__ running_mean, float* __restrict__ running_var,
                                            float& fm, float& fi) {
  const double var = n > 0. ? m2 / n : 0.;
  fm = (float)m; fi = (float)(1. / sqrt(var + (double)eps));
  mean[ch] = fm;
  invstd[ch] = fi;
  if (running_mean != nullptr) {
    const float unbiased = (float)(n > 1. ? m2 / (n - 1.) : var);
    running_mean[ch] = (1.f - momentum) * running_mean[ch] + momentum * fm;
    running_var[ch] = (1.f - momentum) * running_var[ch] + momentum * unbiased;
  }
}

// One workgroup folds the slab partials of 8 channels: 32 lanes per channel each merge a strided
// subset in order, then a fixed LDS tree merges the 32 lanes.
template <typename P>
__global__ void __launch_bounds__(NT) bn_stats_final_kernel(const P* __restrict__ part,
                                                            int nparts, int c, float eps,
                                                            float momentum,
                                                            float* __restrict__ mean,
                                                            float* __restrict__ invstd,
                                                            float* __restrict__ running_mean,
                                                            float* __restrict__ running_var,
                                                            long long* __restrict__ num_batches) {
  __shared__ double sn[NT], sm[NT], sq[NT];
  if (num_batches != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *num_batches += 1;
  const int tid = threadIdx.x, cl = tid & 7, pl = tid >> 3;      // 8 channels x 32 lanes
  const int ch = blockIdx.x * 8 + cl;
  double na = 0., ma = 0., qa = 0.;
  if (ch < c)
    for (int p = pl; p < nparts; p += 32) {
      const P* s = part + ((int64_t)p * c + ch) * 3;
      if (na == 0.) { na = (double)s[0]; ma = (double)s[1]; qa = (double)s[2]; }
      else chan_merge(na, ma, qa, (double)s[0], (double)s[1], (double)s[2]);
    }
  sn[tid] = na; sm[tid] = ma; sq[tid] = qa;
  for (int s = 16; s >= 1; s >>= 1) {
    __syncthreads();
    if (pl < s) {
      double nb = sn[tid + s * 8], mb = sm[tid + s * 8], qb = sq[tid + s * 8];
      double n0 = sn[tid], m0 = sm[tid], q0 = sq[tid];
      if (n0 == 0.) { n0 = nb; m0 = mb; q0 = qb; }
      else chan_merge(n0, m0, q0, nb, mb, qb);
      sn[tid] = n0; sm[tid] = m0; sq[tid] = q0;
    }
  }
  __syncthreads();
  if (pl == 0 && ch < c) {
    float fm, fi;
    write_stats(ch, sn[tid], sm[tid], sq[tid], eps, momentum, mean, invstd, running_mean, running_var, fm, fi);
  }
}

template <typename T, bool VAR_IN>
__global__ void __launch_bounds__(NT) bn_apply_kernel(const T* __restrict__ x, int64_t n, int c,
                                                      const float* __restrict__ mean,
                                                      const float* __restrict__ istd_or_var,
                                                      const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float eps,
                                                      int relu, const T* __restrict__ res,
                                                      T* __restrict__ y, int rpw) {
  constexpr int VEC = IO<T>::VEC;
  typedef typename IO<T>::vec V;
  const Slab g = slab_of<VEC>(c, n, rpw);
  if (g.rl >= g.rpi) return;
  float mu[VEC], sc[VEC], sh[VEC], iv[VEC];
  load_channels<VEC>(mean, g.col, 0.f, mu);
  load_channels<VEC>(istd_or_var, g.col, 0.f, iv);
  load_channels<VEC>(gamma, g.col, 1.f, sc);
  load_channels<VEC>(beta, g.col, 0.f, sh);
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    const float is = VAR_IN ? 1.f / sqrtf(iv[i] + eps) : iv[i];
    sc[i] = is * sc[i];
  }
  with_apply_flags(apply_flags(relu, res != nullptr), [&](auto fc) {
    constexpr int F = decltype(fc)::value;
    constexpr int K = (F & 2) ? 2 : 1;
    // (without a residual K = 1: the walk never reads the second operand, a null `res`)
    walk_rows<UNR, K>(g, RowOps<T>{{x, res}, {c, c}}, [&](int64_t r, const V (&v)[K]) {
      store_piece<T>(y, c, g, r, apply_piece<T, F>(v[0], v[K - 1], mu, sc, sh));
    });
  });
}

// backward partials: per workgroup and channel  sum(dy), sum(dy * xhat), f64
template <typename T>
__global__ void __launch_bounds__(NT) bn_bwd_partial_kernel(const T* __restrict__ x,
                                                            const T* __restrict__ dy, int64_t n,
                                                            int c, const float* __restrict__ mean,
                                                            const float* __restrict__ invstd,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta,
                                                            int relu, double* __restrict__ part, int rpw,
                                                            int64_t ldy) {
  constexpr int VEC = IO<T>::VEC;
  typedef typename IO<T>::vec V;
  extern __shared__ double sh[];                // [2][NT][VEC]
  const Slab g = slab_of<VEC>(c, n, rpw);
  double a[VEC], b[VEC];
  Channels<VEC> k;
#pragma unroll
  for (int i = 0; i < VEC; ++i) { a[i] = 0.; b[i] = 0.; k.mu[i] = 0.f; k.is[i] = 0.f; k.ga[i] = 1.f; k.be[i] = 0.f; }
  if (g.rl < g.rpi) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      k.mu[i] = mean[g.col + i]; k.is[i] = invstd[g.col + i];
      if (gamma) k.ga[i] = gamma[g.col + i];
      if (beta) k.be[i] = beta[g.col + i];
    }
  }
  // two batches in flight: with ONE wave per SIMD (256 workgroups of 4 waves) nothing else hides the arithmetic of a
  // batch (~90 VALU instructions per 16-byte pair, f64 sums) behind the memory round trip
  walk_rows<UNR, 2, true>(g, RowOps<T>{{x, dy}, {c, ldy}}, [&](int64_t, const V (&v)[2]) {
    float fx[VEC], fd[VEC];
    IO<T>::unpack(v[0], fx);
    IO<T>::unpack(v[1], fd);
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const float xhat = xhat_and_mask(relu != 0, k, i, fx[i], fd[i]);
      add_sum_terms<double>(fd[i], xhat, a[i], b[i]);
    }
  });
  store_partials_f64<VEC>(sh, g, a, b, c, part);
}

// bf16 (round 5): the same sums as an ELEMENT-WISE-shaped launch -- ew_grid slabs (512 workgroups on the large
// levels: two waves per SIMD), f32 sums per thread (~40 rows) and through the LDS tree, one f32 pair per (channel, slab)
// in the layout of the convolutions' tile sums ([channel][part][2]); bn_bwd_dx_merge_kernel<T, true> merges the slabs
// in f64.  The f64 kernel above runs one wave per SIMD and streams (x, dy) at ~3.7 TB/s; this one at the ~5 TB/s of the
// dx pass (tail_tile_sums_kernel below is the same idea with the ReLU mask of a block's tail in front).  The f32 parity
// mode keeps the f64 sums.
template <typename T, bool RELU>
__global__ void __launch_bounds__(NT) bn_bwd_slab_sums_kernel(const T* __restrict__ x, const T* __restrict__ dy, int64_t n,
                                                              int c, const float* __restrict__ mean,
                                                              const float* __restrict__ invstd,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta,
                                                              float* __restrict__ sums, int rpw, int64_t ldy) {
  constexpr int VEC = IO<T>::VEC;
  __shared__ float sh[NT * VEC];
  const int cg_n = c / VEC, rpi = NT / cg_n;
  const int tid = threadIdx.x, cg = tid % cg_n, rl = tid / cg_n;
  const int64_t r_beg = (int64_t)blockIdx.x * rpw;
  const int64_t r_end = (r_beg + rpw < n) ? r_beg + rpw : n;
  float a[VEC], b[VEC];
  float mu[VEC], is[VEC], ga[VEC], be[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) { a[i] = 0.f; b[i] = 0.f; mu[i] = 0.f; is[i] = 0.f; ga[i] = 1.f; be[i] = 0.f; }
  if (rl < rpi) {
    load_channels<VEC>(mean, cg * VEC, 0.f, mu);
    load_channels<VEC>(invstd, cg * VEC, 0.f, is);
    load_channels<VEC>(gamma, cg * VEC, 1.f, ga);
    load_channels<VEC>(beta, cg * VEC, 0.f, be);
    auto one = [&](const typename IO<T>::vec& vx, const typename IO<T>::vec& vd) {
      float fx[VEC], fd[VEC];
      IO<T>::unpack(vx, fx);
      IO<T>::unpack(vd, fd);
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const float xhat = (fx[i] - mu[i]) * is[i];
        if (RELU && !(xhat * ga[i] + be[i] > 0.f)) fd[i] = 0.f;
        a[i] += fd[i]; b[i] += fd[i] * xhat;
      }
    };
    int64_t r = r_beg + rl;
    for (; r + (UNR - 1) * rpi < r_end; r += UNR * rpi) {
      typename IO<T>::vec vx[UNR], vd[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        vx[u] = *reinterpret_cast<const typename IO<T>::vec*>(x + (r + u * rpi) * c + cg * VEC);
        vd[u] = *reinterpret_cast<const typename IO<T>::vec*>(dy + (r + u * rpi) * ldy + cg * VEC);
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) one(vx[u], vd[u]);
    }
    for (; r < r_end; r += rpi)
      one(*reinterpret_cast<const typename IO<T>::vec*>(x + r * c + cg * VEC),
          *reinterpret_cast<const typename IO<T>::vec*>(dy + r * ldy + cg * VEC));
  }
  const int nparts = (int)gridDim.x, part = (int)blockIdx.x;
#pragma unroll
  for (int i = 0; i < VEC; ++i) sh[tid * VEC + i] = a[i];
  tree_sum_rows<VEC, float>(sh, tid, cg_n, rpi, rl);
  if (rl == 0) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) sums[((int64_t)(cg * VEC + i) * nparts + part) * 2] = sh[tid * VEC + i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < VEC; ++i) sh[tid * VEC + i] = b[i];
  tree_sum_rows<VEC, float>(sh, tid, cg_n, rpi, rl);
  if (rl == 0) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) sums[((int64_t)(cg * VEC + i) * nparts + part) * 2 + 1] = sh[tid * VEC + i];
  }
}

// The tail of a residual block backwards (network/blocks.py _Residual.backward): gm = g * (out > 0) is the gradient of
// BOTH summands of relu(bn2(x_a) + shortcut).  Written once here and, in the same pass, summed against xhat of bn2 (and,
// DUAL, of the shortcut's BatchNorm over x_b): the terms of bn_bwd_partial_kernel over (x, gm) with relu = 0, one by one
// and in the same order -- the sums are bit for bit those of the separate pass, which no longer reads gm and x back.
template <typename T, bool DUAL>
__global__ void __launch_bounds__(NT) bn_bwd_partial_masked_kernel(
    const T* __restrict__ out, const T* __restrict__ g, T* __restrict__ gm, int64_t n, int c,
    const T* __restrict__ xa, const float* __restrict__ mean_a, const float* __restrict__ invstd_a, double* __restrict__ part_a,
    const T* __restrict__ xb, const float* __restrict__ mean_b, const float* __restrict__ invstd_b, double* __restrict__ part_b,
    int rpw) {
  constexpr int VEC = IO<T>::VEC;
  extern __shared__ double sh[];                // [2][NT][VEC]
  const int cg_n = c / VEC, rpi = NT / cg_n;
  const int tid = threadIdx.x, cg = tid % cg_n, rl = tid / cg_n;
  const int64_t r_beg = (int64_t)blockIdx.x * rpw;
  const int64_t r_end = (r_beg + rpw < n) ? r_beg + rpw : n;
  double a[VEC], b[VEC], a2[VEC], b2[VEC];
  float mu[VEC], is[VEC], mu2[VEC], is2[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) { a[i] = 0.; b[i] = 0.; a2[i] = 0.; b2[i] = 0.; mu[i] = 0.f; is[i] = 0.f; mu2[i] = 0.f; is2[i] = 0.f; }
  if (rl < rpi) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      mu[i] = mean_a[cg * VEC + i]; is[i] = invstd_a[cg * VEC + i];
      if (DUAL) { mu2[i] = mean_b[cg * VEC + i]; is2[i] = invstd_b[cg * VEC + i]; }
    }
    typedef typename IO<T>::vec V;
    auto one = [&](int64_t r, const V& vo, const V& vg, const V& vx, const V& vx2) {
      float fo[VEC], fd[VEC], fx[VEC], fx2[VEC];
      IO<T>::unpack(vo, fo);
      IO<T>::unpack(vg, fd);
      IO<T>::unpack(vx, fx);
      if (DUAL) IO<T>::unpack(vx2, fx2);
#pragma unroll
      for (int i = 0; i < VEC; ++i) fd[i] = fo[i] > 0.f ? fd[i] : 0.f;
      *reinterpret_cast<V*>(gm + r * c + cg * VEC) = IO<T>::pack(fd);
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const float xhat = (fx[i] - mu[i]) * is[i];
        a[i] += (double)fd[i]; b[i] += (double)fd[i] * (double)xhat;
        if (DUAL) {
          const float xhat2 = (fx2[i] - mu2[i]) * is2[i];
          a2[i] += (double)fd[i]; b2[i] += (double)fd[i] * (double)xhat2;
        }
      }
    };
    int64_t r = r_beg + rl;
    for (; r + (UNR - 1) * rpi < r_end; r += UNR * rpi) {
      V vo[UNR], vg[UNR], vx[UNR], vx2[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int64_t off = (r + u * rpi) * c + cg * VEC;
        vo[u] = *reinterpret_cast<const V*>(out + off);
        vg[u] = *reinterpret_cast<const V*>(g + off);
        vx[u] = *reinterpret_cast<const V*>(xa + off);
        if (DUAL) vx2[u] = *reinterpret_cast<const V*>(xb + off);
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) one(r + u * rpi, vo[u], vg[u], vx[u], vx2[u]);
    }
    for (; r < r_end; r += rpi) {
      const int64_t off = r * c + cg * VEC;
      V vx2 = *reinterpret_cast<const V*>(xa + off);
      if (DUAL) vx2 = *reinterpret_cast<const V*>(xb + off);
      one(r, *reinterpret_cast<const V*>(out + off), *reinterpret_cast<const V*>(g + off), *reinterpret_cast<const V*>(xa + off), vx2);
    }
  }
  double* sa = sh; double* sb = sh + NT * VEC;
#pragma unroll
  for (int i = 0; i < VEC; ++i) { sa[tid * VEC + i] = a[i]; sb[tid * VEC + i] = b[i]; }
  tree_sum_rows<VEC, double>(sa, tid, cg_n, rpi, rl);
  tree_sum_rows<VEC, double>(sb, tid, cg_n, rpi, rl);
  if (rl == 0) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      double* dst = part_a + ((int64_t)blockIdx.x * c + cg * VEC + i) * 2;
      dst[0] = sa[tid * VEC + i]; dst[1] = sb[tid * VEC + i];
    }
  }
  if (DUAL) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < VEC; ++i) { sa[tid * VEC + i] = a2[i]; sb[tid * VEC + i] = b2[i]; }
    tree_sum_rows<VEC, double>(sa, tid, cg_n, rpi, rl);
    tree_sum_rows<VEC, double>(sb, tid, cg_n, rpi, rl);
    if (rl == 0) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        double* dst = part_b + ((int64_t)blockIdx.x * c + cg * VEC + i) * 2;
        dst[0] = sa[tid * VEC + i]; dst[1] = sb[tid * VEC + i];
      }
    }
  }
}

// The same tail on the levels with many rows (round 5): the mask as an ELEMENT-WISE launch -- 512 workgroups, two waves
// per SIMD -- that also leaves, per workgroup and channel, the f32 sums of its slab of rows in the layout of the
// convolutions' tile sums ([channel][part][2]); lidal_bn_bwd_tiles merges them (f64 across the parts) in front of its dx
// pass.  bn_bwd_partial_masked_kernel above keeps f64 sums per thread on 256 workgroups and streams at ~2.5 TB/s on
// the 397 k-row level (115 / 156 us against 44 + 41 (+ 41) for the separate passes: profiles/README.md, round 5), which
// is why rounds 3-4 kept the separate passes there.  A thread sums ~40 rows in f32, a slab is ~775 rows: the error of a
// part is that of a convolution's 128-row tile sum.
template <typename T, bool DUAL>
__global__ void __launch_bounds__(NT) tail_tile_sums_kernel(
    const T* __restrict__ out, const T* __restrict__ g, T* __restrict__ gm, int64_t n, int c,
    const T* __restrict__ xa, const float* __restrict__ mean_a, const float* __restrict__ invstd_a, float* __restrict__ sums_a,
    const T* __restrict__ xb, const float* __restrict__ mean_b, const float* __restrict__ invstd_b, float* __restrict__ sums_b,
    int rpw) {
  constexpr int VEC = IO<T>::VEC;
  __shared__ float sh[NT * VEC];
  const int cg_n = c / VEC, rpi = NT / cg_n;
  const int tid = threadIdx.x, cg = tid % cg_n, rl = tid / cg_n;
  const int64_t r_beg = (int64_t)blockIdx.x * rpw;
  const int64_t r_end = (r_beg + rpw < n) ? r_beg + rpw : n;
  float a[VEC], b[VEC], b2[VEC];
  float mu[VEC], is[VEC], mu2[VEC], is2[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) { a[i] = 0.f; b[i] = 0.f; b2[i] = 0.f; mu[i] = 0.f; is[i] = 0.f; mu2[i] = 0.f; is2[i] = 0.f; }
  if (rl < rpi) {
    load_channels<VEC>(mean_a, cg * VEC, 0.f, mu);
    load_channels<VEC>(invstd_a, cg * VEC, 0.f, is);
    if (DUAL) {
      load_channels<VEC>(mean_b, cg * VEC, 0.f, mu2);
      load_channels<VEC>(invstd_b, cg * VEC, 0.f, is2);
    }
    typedef typename IO<T>::vec V;
    auto one = [&](int64_t r, const V& vo, const V& vg, const V& vx, const V& vx2) {
      float fo[VEC], fd[VEC], fx[VEC], fx2[VEC];
      IO<T>::unpack(vo, fo);
      IO<T>::unpack(vg, fd);
      IO<T>::unpack(vx, fx);
      if (DUAL) IO<T>::unpack(vx2, fx2);
#pragma unroll
      for (int i = 0; i < VEC; ++i) fd[i] = fo[i] > 0.f ? fd[i] : 0.f;
      *reinterpret_cast<V*>(gm + r * c + cg * VEC) = IO<T>::pack(fd);
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        a[i] += fd[i];
        b[i] += fd[i] * ((fx[i] - mu[i]) * is[i]);
        if (DUAL) b2[i] += fd[i] * ((fx2[i] - mu2[i]) * is2[i]);
      }
    };
    int64_t r = r_beg + rl;
    for (; r + (UNR - 1) * rpi < r_end; r += UNR * rpi) {
      V vo[UNR], vg[UNR], vx[UNR], vx2[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int64_t off = (r + u * rpi) * c + cg * VEC;
        vo[u] = *reinterpret_cast<const V*>(out + off);
        vg[u] = *reinterpret_cast<const V*>(g + off);
        vx[u] = *reinterpret_cast<const V*>(xa + off);
        vx2[u] = DUAL ? *reinterpret_cast<const V*>(xb + off) : vx[u];
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) one(r + u * rpi, vo[u], vg[u], vx[u], vx2[u]);
    }
    for (; r < r_end; r += rpi) {
      const int64_t off = r * c + cg * VEC;
      const V vx = *reinterpret_cast<const V*>(xa + off);
      one(r, *reinterpret_cast<const V*>(out + off), *reinterpret_cast<const V*>(g + off), vx,
          DUAL ? *reinterpret_cast<const V*>(xb + off) : vx);
    }
  }
  const int nparts = (int)gridDim.x, part = (int)blockIdx.x;
  // three LDS trees over the row lanes (sum gm, sum gm xhat_a, sum gm xhat_b), each left with rl == 0
#pragma unroll
  for (int i = 0; i < VEC; ++i) sh[tid * VEC + i] = a[i];
  tree_sum_rows<VEC, float>(sh, tid, cg_n, rpi, rl);
  if (rl == 0) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const int64_t o = ((int64_t)(cg * VEC + i) * nparts + part) * 2;
      sums_a[o] = sh[tid * VEC + i];
      if (DUAL) sums_b[o] = sh[tid * VEC + i];
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < VEC; ++i) sh[tid * VEC + i] = b[i];
  tree_sum_rows<VEC, float>(sh, tid, cg_n, rpi, rl);
  if (rl == 0) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) sums_a[((int64_t)(cg * VEC + i) * nparts + part) * 2 + 1] = sh[tid * VEC + i];
  }
  if (DUAL) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < VEC; ++i) sh[tid * VEC + i] = b2[i];
    tree_sum_rows<VEC, float>(sh, tid, cg_n, rpi, rl);
    if (rl == 0) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) sums_b[((int64_t)(cg * VEC + i) * nparts + part) * 2 + 1] = sh[tid * VEC + i];
    }
  }
}

// ---- merges: each is called by its stand-alone kernel and by the first workgroups of its consumer ----
// A BatchNorm layer was three launches forwards (tile merge, apply) and backwards (partial / tile merge, dx); the merges
// are 5-7 us launches that compute for 2 us (104 per step: on one scan every eighth microsecond of the step).  So
// the consumer kernel's first workgroups do the merge -- workgroup b the channels b, b + grid, ... -- and PUBLISH
// the two f32 values of a channel as two 64-bit words
// (value | launch token << 32; agent-scope atomics, no fence needed: the token travels with the value); every
// workgroup then fetches the words of all channels (spinning until the token matches) and streams its rows.  Forward
// progress: the merging workgroups have the lowest ids of the launch and are dispatched first (the assumption the
// radix sort's look-back makes, sort.hip).  The slots of a launch are one of TWO buffers that belong to the launch's
// STREAM (a fixed pool of 64 buffers per device, 2 MiB, allocated by this library at the first fused launch: 32
// streams per device; a 33rd stream, or a pool that cannot be allocated, takes the separate merge launches): launches
// of one stream execute in order, so a buffer is never rewritten while an earlier launch still reads it, whatever
// other streams or host threads do; the token is a process-wide counter, so a stale word never matches.  A fetch
// gives up after ~30 s (a broken dispatch-order assumption must fail a test, not hang a GPU): it poisons its channel
// with NaN AND raises the pool's error word (pinned host memory), which the next BatchNorm entry point or
// lidal_plan_run on that device turns into an error return -- never a silent NaN.
struct Slots { unsigned long long* v; unsigned token; unsigned* error; };
constexpr int SLOT_RING = 64, SLOT_CH = 2048, SLOTS_PER_STREAM = 2;
constexpr unsigned SPIN_LIMIT = 1u << 25;     // ~1 us per probe: half a minute (a time-sliced device may stall a launch for seconds)

__device__ __forceinline__ void publish(const Slots& s, int ch, float a, float b) {
  const unsigned long long t = (unsigned long long)s.token << 32;
  __hip_atomic_store(s.v + 2 * ch, t | (unsigned long long)__float_as_uint(a), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(s.v + 2 * ch + 1, t | (unsigned long long)__float_as_uint(b), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float fetch_one(const Slots& s, int idx) {
  unsigned long long v = __hip_atomic_load(s.v + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  unsigned spins = 0;
  while ((unsigned)(v >> 32) != s.token) {
    if (++spins > SPIN_LIMIT) {
      __hip_atomic_store(s.error, s.token, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      return __uint_as_float(0x7fc00000u);
    }
    __builtin_amdgcn_s_sleep(2);
    v = __hip_atomic_load(s.v + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return __uint_as_float((unsigned)v);
}
// every channel's published pair, from whichever workgroup merged it, into two LDS arrays (and a barrier)
__device__ inline void fetch_all(const Slots& s, int c, float* s0, float* s1) {
  for (int ch = threadIdx.x; ch < c; ch += NT) {
    s0[ch] = fetch_one(s, 2 * ch);
    s1[ch] = fetch_one(s, 2 * ch + 1);
  }
  __syncthreads();
}

// plain sum of NT doubles per array, left in [0]; thread 0 may read its own result without a further barrier
template <int N>
__device__ inline void tree_sum_wg(double* (&s)[N], int tid) {
  for (int st = NT / 2; st >= 1; st >>= 1) {
    __syncthreads();
    if (tid < st) {
#pragma unroll
      for (int k = 0; k < N; ++k) s[k][tid] += s[k][tid + st];
    }
  }
}

// Merge of the per-tile (count, mean, M2) f32 triples a convolution left (thousands of tiles) for channel `ch` by one
// workgroup: plain f64 sums N, S1 = sum n m, S2 = sum (M2 + n m^2) -- in f64 the cancellation of S2/N - mean^2 is
// harmless, and no per-element division (Chan's formula) is needed.  Eight tiles' triples are requested at once and
// summed in tile order: the sums of a one-at-a-time loop, with the loads of a batch in flight together -- in a
// consumer the merge is on the layer's critical path.  Writes the statistics and, given slots, publishes them.
__device__ inline void merge_tile_stats(const float* __restrict__ part, int nparts, int ch, float eps,
                                                 float momentum, float* __restrict__ mean, float* __restrict__ invstd,
                                                 float* __restrict__ running_mean, float* __restrict__ running_var,
                                                 double* sn, double* s1, double* s2, const Slots* slots) {
  const int tid = threadIdx.x;
  double nn = 0., a = 0., b = 0.;
  for (int p0 = tid; p0 < nparts; p0 += 8 * NT) {
    float t0[8], t1[8], t2[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int p = p0 + u * NT;
      const float* sp = part + ((int64_t)ch * nparts + (p < nparts ? p : p0)) * 3;   // [c][tiles][3]: a channel's triples are one run
      t0[u] = sp[0]; t1[u] = sp[1]; t2[u] = sp[2];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (p0 + u * NT < nparts) {
        const double pn = (double)t0[u], pm = (double)t1[u];
        nn += pn; a += pn * pm; b += (double)t2[u] + pn * pm * pm;
      }
  }
  sn[tid] = nn; s1[tid] = a; s2[tid] = b;
  double* s[3] = {sn, s1, s2};
  tree_sum_wg(s, tid);
  if (tid == 0) {
    nn = sn[0];
    const double m = nn > 0. ? s1[0] / nn : 0.;
    double m2 = s2[0] - nn * m * m;
    if (m2 < 0.) m2 = 0.;
    float fm, fi;
    write_stats(ch, nn, m, m2, eps, momentum, mean, invstd, running_mean, running_var, fm, fi);
    if (slots != nullptr) publish(*slots, ch, fm, fi);
  }
}

// Merge of the f32 (sum dy, sum dy xhat) pairs per tile or slab of rows, [c][parts][2], for channel `ch` by one
// workgroup: f64 sums, batched loads as above.  sum_dy = grad_beta, sum_dy_xhat = grad_gamma.
__device__ inline void merge_tile_sums(const float* __restrict__ part, int nparts, int ch,
                                                float* __restrict__ sum_dy, float* __restrict__ sum_dy_xhat,
                                                double* sa, double* sb, const Slots* slots) {
  const int tid = threadIdx.x;
  double a = 0., b = 0.;
  for (int p0 = tid; p0 < nparts; p0 += 8 * NT) {
    float t0[8], t1[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int p = p0 + u * NT;
      const float* sp = part + ((int64_t)ch * nparts + (p < nparts ? p : p0)) * 2;
      t0[u] = sp[0]; t1[u] = sp[1];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (p0 + u * NT < nparts) { a += (double)t0[u]; b += (double)t1[u]; }
  }
  sa[tid] = a; sb[tid] = b;
  double* s[2] = {sa, sb};
  tree_sum_wg(s, tid);
  if (tid == 0) {
    const float fa = (float)sa[0], fb = (float)sb[0];
    sum_dy[ch] = fa; sum_dy_xhat[ch] = fb;
    if (slots != nullptr) publish(*slots, ch, fa, fb);
  }
}

// Merge of the f64 pairs of the partial kernels, [part][c][2], for the 8 channels of unit `u` by one workgroup: 32
// lanes per channel each sum a strided subset in order, a fixed LDS tree sums the lanes.
__device__ inline void merge_partial_sums(const double* __restrict__ part, int nparts, int c, int u,
                                                   float* __restrict__ sum_dy, float* __restrict__ sum_dy_xhat,
                                                   double* sa, double* sb, const Slots* slots) {
  const int tid = threadIdx.x, cl = tid & 7, pl = tid >> 3;
  const int ch = u * 8 + cl;
  double a = 0., b = 0.;
  if (ch < c)
    for (int p = pl; p < nparts; p += 32) {
      a += part[((int64_t)p * c + ch) * 2];
      b += part[((int64_t)p * c + ch) * 2 + 1];
    }
  sa[tid] = a; sb[tid] = b;
  for (int st = 16; st >= 1; st >>= 1) {
    __syncthreads();
    if (pl < st) { sa[tid] += sa[tid + st * 8]; sb[tid] += sb[tid + st * 8]; }
  }
  __syncthreads();
  if (pl == 0 && ch < c) {
    const float fa = (float)sa[tid], fb = (float)sb[tid];
    sum_dy[ch] = fa; sum_dy_xhat[ch] = fb;
    if (slots != nullptr) publish(*slots, ch, fa, fb);
  }
}

__global__ void __launch_bounds__(NT) bn_tiles_final_kernel(const float* __restrict__ part, int nparts,
                                                            int c, float eps, float momentum,
                                                            float* __restrict__ mean,
                                                            float* __restrict__ invstd,
                                                            float* __restrict__ running_mean,
                                                            float* __restrict__ running_var,
                                                            long long* __restrict__ num_batches) {
  __shared__ double sn[NT], s1[NT], s2[NT];
  if (num_batches != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *num_batches += 1;
  merge_tile_stats(part, nparts, blockIdx.x, eps, momentum, mean, invstd, running_mean, running_var, sn, s1, s2, nullptr);
}

__global__ void __launch_bounds__(NT) bn_bwd_tiles_final_kernel(const float* __restrict__ part, int nparts, int c,
                                                                float* __restrict__ sum_dy,
                                                                float* __restrict__ sum_dy_xhat) {
  __shared__ double sa[NT], sb[NT];
  merge_tile_sums(part, nparts, blockIdx.x, sum_dy, sum_dy_xhat, sa, sb, nullptr);
}

__global__ void __launch_bounds__(NT) bn_bwd_final_kernel(const double* __restrict__ part,
                                                          int nparts, int c,
                                                          float* __restrict__ sum_dy,
                                                          float* __restrict__ sum_dy_xhat) {
  __shared__ double sa[NT], sb[NT];
  merge_partial_sums(part, nparts, c, blockIdx.x, sum_dy, sum_dy_xhat, sa, sb, nullptr);
}

// bn_tiles_final_kernel + bn_apply_kernel<T, false> in one launch.  The streaming part wants waves in flight, not
// workgroups: every workgroup pays the wait for the merged values once.
template <typename T, int F>
__global__ void __launch_bounds__(NT) bn_apply_tiles_kernel(const T* __restrict__ x, int64_t n, int c,
                                                           const float* __restrict__ part, int nparts, float eps,
                                                           float momentum, float* __restrict__ mean,
                                                           float* __restrict__ invstd, float* __restrict__ running_mean,
                                                           float* __restrict__ running_var,
                                                           long long* __restrict__ num_batches,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           const T* __restrict__ res, T* __restrict__ y, int rpw,
                                                           Slots slots) {
  constexpr int VEC = IO<T>::VEC;
  constexpr bool HAS_RES = (F & 2) != 0;
  typedef typename IO<T>::vec V;
  __shared__ double sn[NT], s1[NT], s2[NT];
  __shared__ float smu[SLOT_CH], sis[SLOT_CH];
  if (num_batches != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *num_batches += 1;
  for (int ch = blockIdx.x; ch < c; ch += gridDim.x) {
    merge_tile_stats(part, nparts, ch, eps, momentum, mean, invstd, running_mean, running_var, sn, s1, s2, &slots);
    __syncthreads();
  }
  // ---- the first rows of this workgroup's slab are requested BEFORE the statistics are waited for: the merge's
  //      latency (a strided read of the tiles, an 8-step LDS tree) hides behind them.  (Its own loop, not walk_rows:
  //      see the note there.)
  const Slab g = slab_of<VEC>(c, n, rpw);
  const int rpi = g.rpi;
  const T* rsrc = HAS_RES ? res : x;
  int64_t r = g.r_beg + g.rl;
  const bool first = g.rl < rpi && r + (UNR - 1) * rpi < g.r_end;
  V v0[UNR], vr0[UNR];
  if (first) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) v0[u] = load_piece(x, c, g, r + u * rpi);
    if (HAS_RES) {
#pragma unroll
      for (int u = 0; u < UNR; ++u) vr0[u] = load_piece(rsrc, c, g, r + u * rpi);
    }
  }
  fetch_all(slots, c, smu, sis);
  if (g.rl >= rpi) return;
  float mu[VEC], sc[VEC], sh[VEC];
  load_channels<VEC>(gamma, g.col, 1.f, sc);
  load_channels<VEC>(beta, g.col, 0.f, sh);
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    mu[i] = smu[g.col + i];
    sc[i] = sis[g.col + i] * sc[i];
  }
  auto one = [&](const V& v, const V& vr, int64_t r) { store_piece<T>(y, c, g, r, apply_piece<T, F>(v, vr, mu, sc, sh)); };
  if (first) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) one(v0[u], HAS_RES ? vr0[u] : v0[u], r + u * rpi);
    r += UNR * rpi;
  }
  for (; r + (UNR - 1) * rpi < g.r_end; r += UNR * rpi) {
    V v[UNR], vr[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) v[u] = load_piece(x, c, g, r + u * rpi);
    if (HAS_RES) {
#pragma unroll
      for (int u = 0; u < UNR; ++u) vr[u] = load_piece(rsrc, c, g, r + u * rpi);
    } else {
#pragma unroll
      for (int u = 0; u < UNR; ++u) vr[u] = v[u];
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) one(v[u], vr[u], r + u * rpi);
  }
  for (; r < g.r_end; r += rpi) {
    const V v = load_piece(x, c, g, r);
    one(v, HAS_RES ? load_piece(res, c, g, r) : v, r);
  }
}

template <typename T>
__global__ void __launch_bounds__(NT) bn_bwd_dx_kernel(const T* __restrict__ x,
                                                       const T* __restrict__ dy, int64_t n, int c,
                                                       const float* __restrict__ mean,
                                                       const float* __restrict__ invstd,
                                                       const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, int relu,
                                                       const float* __restrict__ sum_dy,
                                                       const float* __restrict__ sum_dy_xhat,
                                                       T* __restrict__ dx, int rpw, int64_t ldy) {
  constexpr int VEC = IO<T>::VEC;
  typedef typename IO<T>::vec V;
  const Slab g = slab_of<VEC>(c, n, rpw);
  if (g.rl >= g.rpi) return;
  const float inv_n = 1.f / (float)n;
  Channels<VEC> k;
  float k1[VEC], k2[VEC];
  k.load(mean, invstd, gamma, beta, g.col);
  load_channels<VEC>(sum_dy, g.col, 0.f, k1);
  load_channels<VEC>(sum_dy_xhat, g.col, 0.f, k2);
#pragma unroll
  for (int i = 0; i < VEC; ++i) { k1[i] = k1[i] * inv_n; k2[i] = k2[i] * inv_n; }
  auto run = [&](auto rc) {
    constexpr bool RELU = decltype(rc)::value;
    walk_rows<UNR, 2>(g, RowOps<T>{{x, dy}, {c, ldy}}, [&](int64_t r, const V (&v)[2]) {
      store_piece<T>(dx, c, g, r, dx_piece<T, RELU>(v[0], v[1], k, k1, k2));
    });
  };
  if (relu) run(std::true_type{}); else run(std::false_type{});
}

// bn_bwd_final_kernel (TILES = false: f64 partial pairs of bn_bwd_partial_kernel, 8 channels x 32 lanes per unit) or
// bn_bwd_tiles_final_kernel (TILES = true: f32 pairs per 128-row tile or slab, one channel per unit) + bn_bwd_dx_kernel
template <typename T, bool TILES, bool RELU>
__global__ void __launch_bounds__(NT) bn_bwd_dx_merge_kernel(const T* __restrict__ x, const T* __restrict__ dy, int64_t n,
                                                             int c, const float* __restrict__ mean,
                                                             const float* __restrict__ invstd,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             const void* __restrict__ part, int nparts,
                                                             float* __restrict__ sum_dy, float* __restrict__ sum_dy_xhat,
                                                             T* __restrict__ dx, int rpw, int64_t ldy, Slots slots) {
  constexpr int VEC = IO<T>::VEC;
  typedef typename IO<T>::vec V;
  __shared__ double sa[NT], sb[NT];
  __shared__ float sk1[SLOT_CH], sk2[SLOT_CH];
  if (TILES) {
    for (int ch = blockIdx.x; ch < c; ch += gridDim.x) {
      merge_tile_sums((const float*)part, nparts, ch, sum_dy, sum_dy_xhat, sa, sb, &slots);
      __syncthreads();
    }
  } else {
    for (int u = blockIdx.x; u * 8 < c; u += gridDim.x) {
      merge_partial_sums((const double*)part, nparts, c, u, sum_dy, sum_dy_xhat, sa, sb, &slots);
      __syncthreads();
    }
  }
  if (dx == nullptr) return;            // (only the parameter gradients were wanted)
  // ---- the first rows are requested before the sums are waited for (as in bn_apply_tiles_kernel; its own loop too)
  const Slab g = slab_of<VEC>(c, n, rpw);
  const int rpi = g.rpi;
  int64_t r = g.r_beg + g.rl;
  const bool first = g.rl < rpi && r + (UNR - 1) * rpi < g.r_end;
  V vx0[UNR], vd0[UNR];
  if (first) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      vx0[u] = load_piece(x, c, g, r + u * rpi);
      vd0[u] = load_piece(dy, ldy, g, r + u * rpi);
    }
  }
  fetch_all(slots, c, sk1, sk2);
  if (g.rl >= rpi) return;
  const float inv_n = 1.f / (float)n;
  Channels<VEC> k;
  float k1[VEC], k2[VEC];
  k.load(mean, invstd, gamma, beta, g.col);
#pragma unroll
  for (int i = 0; i < VEC; ++i) { k1[i] = sk1[g.col + i] * inv_n; k2[i] = sk2[g.col + i] * inv_n; }
  auto one = [&](const V& vx, const V& vd, int64_t r) { store_piece<T>(dx, c, g, r, dx_piece<T, RELU>(vx, vd, k, k1, k2)); };
  if (first) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) one(vx0[u], vd0[u], r + u * rpi);
    r += UNR * rpi;
  }
  for (; r + (UNR - 1) * rpi < g.r_end; r += UNR * rpi) {
    V vx[UNR], vd[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      vx[u] = load_piece(x, c, g, r + u * rpi);
      vd[u] = load_piece(dy, ldy, g, r + u * rpi);
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) one(vx[u], vd[u], r + u * rpi);
  }
  for (; r < g.r_end; r += rpi) one(load_piece(x, c, g, r), load_piece(dy, ldy, g, r), r);
}

// eval-mode BatchNorm as a per-channel affine map: y = x * scale + shift
__global__ void __launch_bounds__(256) bn_fold_kernel(const float* __restrict__ gamma,
                                                      const float* __restrict__ beta,
                                                      const float* __restrict__ mean,
                                                      const float* __restrict__ var, float eps,
                                                      int c, float* __restrict__ scale,
                                                      float* __restrict__ shift) {
  int ch = blockIdx.x * 256 + threadIdx.x;
  if (ch >= c) return;
  float sc = (1.f / sqrtf(var[ch] + eps)) * (gamma ? gamma[ch] : 1.f);
  scale[ch] = sc;
  shift[ch] = (beta ? beta[ch] : 0.f) - mean[ch] * sc;
}

// Column sums of a [n, c] matrix (bias gradients of the dense layers): one pass, f64 sums per thread in row order, the
// LDS tree of the statistics kernels, pairs (sum, 0) per (workgroup, channel) for bn_bwd_final_kernel.  (Rounds 1-4 ran
// bn_bwd_partial_kernel with x = dy = the matrix, mean 0: two reads of every row and the BatchNorm arithmetic around a
// plain sum -- 72 us for the 396 662 x 256 gradient of the point branch.)  Sixteen loads in flight per thread: at one
// workgroup per CU a reducing kernel is short of bytes in flight (profiles/README.md, round 5).
constexpr int UNR_C = 16;
// (written out -- geometry, loop and epilogue -- not through slab_of / walk_rows / store_partials_f64: see the note at
// walk_rows)
template <typename T>
__global__ void __launch_bounds__(NT) colsum_partial_kernel(const T* __restrict__ x, int64_t n, int c,
                                                            double* __restrict__ part, int rpw) {
  constexpr int VEC = IO<T>::VEC;
  extern __shared__ double sh[];                // [NT][VEC]
  const int cg_n = c / VEC, rpi = NT / cg_n;
  const int tid = threadIdx.x, cg = tid % cg_n, rl = tid / cg_n;
  const int64_t r_beg = (int64_t)blockIdx.x * rpw;
  const int64_t r_end = (r_beg + rpw < n) ? r_beg + rpw : n;
  double s1[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) s1[i] = 0.;
  if (rl < rpi) {
    int64_t r = r_beg + rl;
    for (; r + (UNR_C - 1) * rpi < r_end; r += UNR_C * rpi) {
      typename IO<T>::vec v[UNR_C];
#pragma unroll
      for (int u = 0; u < UNR_C; ++u)
        v[u] = *reinterpret_cast<const typename IO<T>::vec*>(x + (r + u * rpi) * c + cg * VEC);
#pragma unroll
      for (int u = 0; u < UNR_C; ++u) {
        float f[VEC];
        IO<T>::unpack(v[u], f);
#pragma unroll
        for (int i = 0; i < VEC; ++i) s1[i] += (double)f[i];
      }
    }
    for (; r < r_end; r += rpi) {
      float f[VEC];
      IO<T>::unpack(*reinterpret_cast<const typename IO<T>::vec*>(x + r * c + cg * VEC), f);
#pragma unroll
      for (int i = 0; i < VEC; ++i) s1[i] += (double)f[i];
    }
  }
#pragma unroll
  for (int i = 0; i < VEC; ++i) sh[tid * VEC + i] = s1[i];
  tree_sum_rows<VEC, double>(sh, tid, cg_n, rpi, rl);
  if (rl == 0) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      double* dst = part + ((int64_t)blockIdx.x * c + cg * VEC + i) * 2;
      dst[0] = sh[tid * VEC + i]; dst[1] = 0.;
    }
  }
}

// ---- host side: launch geometry ----
// Slab size = rows / 256: one workgroup per CU on every level.  Each workgroup pays a fixed set-up
// (per-channel parameters, and an LDS tree in the reducing kernels), so fewer and larger slabs win
// as long as every CU has one; and an equal share per CU matters: with 512-row slabs the 396k-row
// level ran as 775 workgroups, 3.03 per CU (measured sweep: profiles/README.md).
constexpr int BN_WGS = 256;
struct Grid { int wgs, rpw; };          // workgroups of a row kernel, rows of each
static inline Grid grid_of(int64_t n, int wgs) {
  int64_t rpw = (n + wgs - 1) / wgs;
  if (rpw < MIN_ROWS_PER_WG) rpw = MIN_ROWS_PER_WG;
  return Grid{(int)cdiv(n > 0 ? n : 1, rpw), (int)rpw};
}
static inline Grid slab_grid(int64_t n) { return grid_of(n, BN_WGS); }
// The element-wise kernels (apply, dx) have no tree and a light set-up, and at one workgroup per CU the
// large levels are short of bytes in flight: 512 workgroups took dx at 396662 x 96 bf16 from 61.7 to
// 44.3 us (3.7 -> 5.2 TB/s), while the small levels lost (43000 x 128: 14.4 -> 18.3 us) and 1024 lost
// everywhere.  The reducing kernels are best at 256 on every level (sweep: profiles/README.md).
constexpr int64_t EW_WIDE_BYTES = 12ll << 20;
static inline Grid ew_grid(int64_t n, int64_t row_bytes) {
  return grid_of(n, n * row_bytes >= EW_WIDE_BYTES ? 2 * BN_WGS : BN_WGS);
}
template <typename T> static inline Grid ew_grid(int64_t n, int c) { return ew_grid(n, (int64_t)c * sizeof(T)); }

// LIDAL_BN_SLAB_SUMS=0 / lidal_bn_set_slab_sums(0): the f64 partial sums for bf16 too (A/B, and the bitwise tests against
// the fused tail of the f32 mode)
static int g_slab_sums = -1;            // -1: not read yet
static inline bool slab_sums_enabled() {
  if (g_slab_sums < 0) { const char* e = getenv("LIDAL_BN_SLAB_SUMS"); g_slab_sums = (e && e[0] == '0') ? 0 : 1; }
  return g_slab_sums != 0;
}

}  // namespace

// ---- host side of the slots: a pool of buffers per device, two per stream, one token per launch
#include <atomic>
#include <mutex>
#include <unordered_map>
namespace {
std::atomic<unsigned> g_token{1};
std::atomic<int> g_fused{-1};           // -1: not read yet (LIDAL_BN_FUSED, default on)
struct SlotPool {
  unsigned long long* base = nullptr;   // SLOT_RING buffers of 2 * SLOT_CH words
  unsigned* error_host = nullptr;       // pinned, read by the host without a synchronisation
  unsigned* error_dev = nullptr;        // the same word as the device addresses it
  bool failed = false;                  // the pool could not be allocated: separate launches from now on
  std::unordered_map<hipStream_t, unsigned> streams;   // stream -> (index of its first buffer) << 1 | next buffer
};
SlotPool g_pool[MAX_DEVICES];
std::mutex g_pool_mutex;

bool bn_fused() {
  int f = g_fused.load();
  if (f < 0) {
    const char* e = getenv("LIDAL_BN_FUSED");
    f = (e == nullptr || e[0] != '0') ? 1 : 0;
    g_fused.store(f);
  }
  return f != 0;
}

// the slots of the next launch on stream `s` of the current device (false: no pool, or more than SLOT_RING /
// SLOTS_PER_STREAM streams on this device -- the caller launches merge and consumer apart)
bool next_slots(Slots* out, hipStream_t s) {
  const int d = current_device();
  std::lock_guard<std::mutex> lock(g_pool_mutex);
  SlotPool& pool = g_pool[d];
  if (pool.failed) return false;
  if (pool.base == nullptr) {
    void *p = nullptr, *h = nullptr, *hd = nullptr;
    const size_t bytes = (size_t)SLOT_RING * 2 * SLOT_CH * sizeof(unsigned long long);
    if (hipMalloc(&p, bytes) != hipSuccess || hipMemset(p, 0, bytes) != hipSuccess ||
        hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess ||
        hipHostGetDevicePointer(&hd, h, 0) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
      (void)hipGetLastError();
      pool.failed = true;
      return false;
    }
    *(volatile unsigned*)h = 0;
    pool.base = (unsigned long long*)p;
    pool.error_host = (unsigned*)h;
    pool.error_dev = (unsigned*)hd;
  }
  auto it = pool.streams.find(s);
  if (it == pool.streams.end()) {
    if (pool.streams.size() >= (size_t)(SLOT_RING / SLOTS_PER_STREAM)) return false;
    it = pool.streams.emplace(s, (unsigned)(pool.streams.size() * SLOTS_PER_STREAM) << 1).first;
  }
  const unsigned first = it->second >> 1, turn = it->second & 1;
  it->second ^= 1;
  unsigned t = g_token.fetch_add(1);
  if (t == 0) t = g_token.fetch_add(1);          // (0 is what the pool was cleared to)
  out->token = t;
  out->v = pool.base + (size_t)(first + turn) * 2 * SLOT_CH;
  out->error = pool.error_dev;
  return true;
}
// the slots of a launch that merges inside its consumer, if that form is on and can be taken for c channels
bool fused_slots(Slots* out, int c, hipStream_t s) { return bn_fused() && c <= SLOT_CH && next_slots(out, s); }

// ---- host side: the launches the entry points share ----
// what every backward entry point passes on
struct BwdArgs {
  const void *x, *dy;
  int64_t ldy, n;
  int c;
  const float *gamma, *beta;
  int relu;
  const float *mean, *invstd;
  void* dx;
  float *ggamma, *gbeta;
};

template <typename T>
int launch_dx(const BwdArgs& a, hipStream_t s) {
  const Grid e = ew_grid<T>(a.n, a.c);
  launch_tail(bn_bwd_dx_kernel<T>, dim3(e.wgs), dim3(NT), 0, s, (const T*)a.x, (const T*)a.dy, a.n, a.c, a.mean, a.invstd,
              a.gamma, a.beta, a.relu, a.gbeta, a.ggamma, (T*)a.dx, e.rpw, a.ldy);
  LIDAL_CHECK_LAUNCH("bn_bwd_dx");
  return 0;
}

// The end of every backward: the merge of the sums (TILES: f32 pairs [c][nparts][2], else the f64 pairs of the partial
// kernels) inside the dx launch -- the last launch of the operation: it carries a pending fork event, launch_tail --
// or, where that form cannot be taken (no dx wanted, LIDAL_BN_FUSED=0, no slots), the merge kernel and the dx pass.
template <typename T, bool TILES>
int finish_bwd(const BwdArgs& a, const void* part, int nparts, const char* merged_name, const char* final_name,
               hipStream_t s) {
  Slots slots;
  if (a.dx != nullptr && fused_slots(&slots, a.c, s)) {
    const Grid e = ew_grid<T>(a.n, a.c);
    auto go = [&](auto rc) {
      launch_tail(bn_bwd_dx_merge_kernel<T, TILES, decltype(rc)::value>, dim3(e.wgs), dim3(NT), 0, s, (const T*)a.x,
                  (const T*)a.dy, a.n, a.c, a.mean, a.invstd, a.gamma, a.beta, part, nparts, a.gbeta, a.ggamma, (T*)a.dx,
                  e.rpw, a.ldy, slots);
    };
    if (a.relu) go(std::true_type{}); else go(std::false_type{});
    LIDAL_CHECK_LAUNCH(merged_name);
    return 0;
  }
  if (TILES) {
    bn_bwd_tiles_final_kernel<<<(unsigned)a.c, NT, 0, s>>>((const float*)part, nparts, a.c, a.gbeta, a.ggamma);
  } else {
    bn_bwd_final_kernel<<<(unsigned)cdiv(a.c, 8), NT, 0, s>>>((const double*)part, nparts, a.c, a.gbeta, a.ggamma);
  }
  LIDAL_CHECK_LAUNCH(final_name);
  return a.dx != nullptr ? launch_dx<T>(a, s) : 0;
}

template <typename T>
int bn_bwd(const BwdArgs& a, double* part, hipStream_t s) {
  constexpr int VEC = IO<T>::VEC;
  if (sizeof(T) == 2 && slab_sums_enabled()) {
    // bf16: f32 slab sums on the element-wise grid, merged like the convolutions' tile sums (bn_bwd_slab_sums_kernel)
    const Grid e = ew_grid<T>(a.n, a.c);
    float* sums = (float*)part;               // c * parts * 8 bytes <= lidal_bn_workspace_bytes (parts <= 2 * slab_grid)
    auto go = [&](auto rc) {
      bn_bwd_slab_sums_kernel<T, decltype(rc)::value><<<e.wgs, NT, 0, s>>>((const T*)a.x, (const T*)a.dy, a.n, a.c, a.mean,
                                                                          a.invstd, a.gamma, a.beta, sums, e.rpw, a.ldy);
    };
    if (a.relu) go(std::true_type{}); else go(std::false_type{});
    LIDAL_CHECK_LAUNCH("bn_bwd_slab_sums");
    return finish_bwd<T, true>(a, sums, e.wgs, "bn_bwd_dx(slab sums merged in the launch)", "bn_bwd_final(slabs)", s);
  }
  const Grid g = slab_grid(a.n);
  bn_bwd_partial_kernel<T><<<g.wgs, NT, 2 * NT * VEC * sizeof(double), s>>>(
      (const T*)a.x, (const T*)a.dy, a.n, a.c, a.mean, a.invstd, a.gamma, a.beta, a.relu, part, g.rpw, a.ldy);
  LIDAL_CHECK_LAUNCH("bn_bwd_partial");
  return finish_bwd<T, false>(a, part, g.wgs, "bn_bwd_dx(sums merged in the launch)", "bn_bwd_final", s);
}
}  // namespace

// 0, or 1 with lidal_last_error() set: a fused BatchNorm launch on the current device gave up waiting for its merged
// values (see `Slots`).  Sticky until lidal_bn_set_fused() is called; checked by every BatchNorm entry point that can
// take the fused form and by lidal_plan_run.
extern "C" int lidal_bn_check_device(void) {
  const int d = current_device();
  const unsigned* e = g_pool[d].error_host;
  if (e == nullptr) return 0;
  const unsigned t = *(const volatile unsigned*)e;
  if (t == 0) return 0;
  set_error("BatchNorm: the launch with token %u timed out waiting for the values its first workgroups merge (in-order "
            "workgroup dispatch did not hold, or the device was stalled for ~30 s); its outputs hold NaN.  "
            "lidal_bn_set_fused(0) / LIDAL_BN_FUSED=0 selects the separate merge launches", t);
  return 1;
}

// test / A-B aid: 1 = bf16 lidal_bn_bwd takes its sums as f32 slab sums (default), 0 = the f64 partial sums of the f32 mode.
// Returns the previous setting.
extern "C" int lidal_bn_set_slab_sums(int on) {
  const int was = slab_sums_enabled() ? 1 : 0;
  g_slab_sums = on ? 1 : 0;
  return was;
}

// test / A-B aid: 1 = merge kernels inside their consumers (default), 0 = separate launches
extern "C" int lidal_bn_set_fused(int on) {
  g_fused.store(on ? 1 : 0);
  for (int d = 0; d < MAX_DEVICES; ++d)          // (also acknowledges a reported time-out)
    if (g_pool[d].error_host != nullptr) *(volatile unsigned*)g_pool[d].error_host = 0;
  return 0;
}

static int bn_check(int64_t n, int c, int dtype) {
  if (int rc = lidal_bn_check_device()) return rc;       // a fused launch of this device timed out earlier: not a silent NaN
  int vec = dtype == LIDAL_BF16 ? 8 : 4;
  LIDAL_REQUIRE(dtype == LIDAL_F32 || dtype == LIDAL_BF16, "bn: bad dtype %d", dtype);
  LIDAL_REQUIRE(c > 0 && c % vec == 0 && c / vec <= NT, "bn: channels %d must be a multiple of %d and <= %d",
                c, vec, NT * vec);
  LIDAL_REQUIRE(n >= 0, "bn: bad row count");
  return 0;
}
// the dy row stride every backward entry point takes
static int dy_stride_check(const char* name, int c, int dtype, int64_t dy_stride) {
  const int vec = dtype == LIDAL_F32 ? 4 : 8;
  LIDAL_REQUIRE(dy_stride >= c && dy_stride % vec == 0, "%s: dy row stride %lld (rows of %d, 16-byte steps)", name,
                (long long)dy_stride, c);
  return 0;
}

extern "C" int64_t lidal_bn_workspace_bytes(int64_t n, int c) {
  return (int64_t)slab_grid(n).wgs * c * 3 * sizeof(double) + 256;
}

extern "C" int lidal_bn_train_fwd(const void* x, int dtype, int64_t n, int c, const float* gamma,
                                  const float* beta, float eps, float momentum,
                                  float* running_mean, float* running_var,
                                  int64_t* num_batches_tracked, int relu, const void* residual,
                                  void* y, float* save_mean, float* save_invstd, void* ws,
                                  int64_t ws_bytes, void* stream) {
  if (int rc = bn_check(n, c, dtype)) return rc;
  LIDAL_REQUIRE(n > 0, "bn_train_fwd: needs at least one row");
  LIDAL_REQUIRE(ws_bytes >= lidal_bn_workspace_bytes(n, c), "bn workspace too small");
  hipStream_t s = (hipStream_t)stream;
  return with_dtype(dtype, "bn_train_fwd", [&](auto t) {
    using T = decltype(t);
    const Grid g = slab_grid(n), e = ew_grid<T>(n, c);
    bn_stats_partial_kernel<T><<<g.wgs, NT, 2 * NT * IO<T>::VEC * sizeof(double), s>>>((const T*)x, n, c, (double*)ws, g.rpw);
    LIDAL_CHECK_LAUNCH("bn_stats_partial");
    bn_stats_final_kernel<double><<<(unsigned)cdiv(c, 8), NT, 0, s>>>((const double*)ws, g.wgs, c, eps, momentum, save_mean,
                                                                      save_invstd, running_mean, running_var,
                                                                      (long long*)num_batches_tracked);
    LIDAL_CHECK_LAUNCH("bn_stats_final");
    bn_apply_kernel<T, false><<<e.wgs, NT, 0, s>>>((const T*)x, n, c, save_mean, save_invstd, gamma, beta, eps, relu,
                                                   (const T*)residual, (T*)y, e.rpw);
    LIDAL_CHECK_LAUNCH("bn_apply");
    return 0;
  });
}

// statistics already reduced per 128-row tile by the producing convolution (conv_img.hip,
// store_tile): merge the tiles, then normalise -- no statistics pass over x
extern "C" int lidal_bn_train_fwd_tiles(const void* x, int dtype, int64_t n, int c, const float* gamma,
                                        const float* beta, float eps, float momentum,
                                        float* running_mean, float* running_var,
                                        int64_t* num_batches_tracked, int relu,
                                        const void* residual, void* y, float* save_mean,
                                        float* save_invstd, const float* tile_stats, int64_t n_tiles,
                                        void* stream) {
  if (int rc = bn_check(n, c, dtype)) return rc;
  LIDAL_REQUIRE(n > 0 && n_tiles > 0 && tile_stats != nullptr, "bn_train_fwd_tiles: needs rows and tile statistics");
  hipStream_t s = (hipStream_t)stream;
  return with_dtype(dtype, "bn_train_fwd_tiles", [&](auto t) {
    using T = decltype(t);
    const Grid e = ew_grid<T>(n, c);
    Slots slots;
    if (fused_slots(&slots, c, s)) {
      with_apply_flags(apply_flags(relu, residual != nullptr), [&](auto fc) {
        launch_tail(bn_apply_tiles_kernel<T, decltype(fc)::value>, dim3(e.wgs), dim3(NT), 0, s, (const T*)x, n, c,
                    tile_stats, (int)n_tiles, eps, momentum, save_mean, save_invstd, running_mean, running_var,
                    (long long*)num_batches_tracked, gamma, beta, (const T*)residual, (T*)y, e.rpw, slots);
      });
      LIDAL_CHECK_LAUNCH("bn_apply(tiles merged in the launch)");
      return 0;
    }
    bn_tiles_final_kernel<<<(unsigned)c, NT, 0, s>>>(tile_stats, (int)n_tiles, c, eps, momentum, save_mean,
                                                     save_invstd, running_mean, running_var,
                                                     (long long*)num_batches_tracked);
    LIDAL_CHECK_LAUNCH("bn_stats_final(tiles)");
    launch_tail(bn_apply_kernel<T, false>, dim3(e.wgs), dim3(NT), 0, s, (const T*)x, n, c, save_mean, save_invstd, gamma,
                beta, eps, relu, (const T*)residual, (T*)y, e.rpw);
    LIDAL_CHECK_LAUNCH("bn_apply");
    return 0;
  });
}

extern "C" int lidal_bn_eval_fwd(const void* x, int dtype, int64_t n, int c, const float* gamma,
                                 const float* beta, const float* running_mean,
                                 const float* running_var, float eps, int relu, void* y,
                                 void* stream) {
  if (int rc = bn_check(n, c, dtype)) return rc;
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  return with_dtype(dtype, "bn_eval_fwd", [&](auto t) {
    using T = decltype(t);
    const Grid e = ew_grid<T>(n, c);
    bn_apply_kernel<T, true><<<e.wgs, NT, 0, s>>>((const T*)x, n, c, running_mean, running_var, gamma, beta, eps, relu,
                                                  (const T*)nullptr, (T*)y, e.rpw);
    LIDAL_CHECK_LAUNCH("lidal_bn_eval_fwd");
    return 0;
  });
}

extern "C" int lidal_bn_bwd(const void* x, const void* dy, int64_t dy_stride, int dtype, int64_t n, int c,
                            const float* gamma, const float* beta, int relu,
                            const float* save_mean, const float* save_invstd, void* dx,
                            float* grad_gamma, float* grad_beta, void* ws, int64_t ws_bytes,
                            void* stream) {
  if (int rc = bn_check(n, c, dtype)) return rc;
  LIDAL_REQUIRE(n > 0, "bn_bwd: needs at least one row");
  LIDAL_REQUIRE(ws_bytes >= lidal_bn_workspace_bytes(n, c), "bn workspace too small");
  if (int rc = dy_stride_check("bn_bwd", c, dtype, dy_stride)) return rc;
  const BwdArgs a{x, dy, dy_stride, n, c, gamma, beta, relu, save_mean, save_invstd, dx, grad_gamma, grad_beta};
  return with_dtype(dtype, "bn_bwd", [&](auto t) { return bn_bwd<decltype(t)>(a, (double*)ws, (hipStream_t)stream); });
}

extern "C" int lidal_add_relu_bwd_bn_sums(const void* out, const void* g, void* gm, int dtype, int64_t n, int c,
                                          const void* x_a, const float* mean_a, const float* invstd_a, void* part_a,
                                          const void* x_b, const float* mean_b, const float* invstd_b, void* part_b,
                                          int64_t part_bytes, void* stream) {
  if (int rc = bn_check(n, c, dtype)) return rc;
  LIDAL_REQUIRE(n > 0, "add_relu_bwd_bn_sums: needs at least one row");
  LIDAL_REQUIRE(part_bytes >= lidal_bn_workspace_bytes(n, c), "add_relu_bwd_bn_sums: partial buffers too small");
  LIDAL_REQUIRE(x_a != nullptr && part_a != nullptr && (x_b == nullptr || part_b != nullptr),
                "add_relu_bwd_bn_sums: a BatchNorm input without a buffer for its partial sums");
  hipStream_t s = (hipStream_t)stream;
  return with_dtype(dtype, "add_relu_bwd_bn_sums", [&](auto t) {
    using T = decltype(t);
    const Grid sg = slab_grid(n);
    auto go = [&](auto dual) {
      launch_tail(bn_bwd_partial_masked_kernel<T, decltype(dual)::value>, dim3(sg.wgs), dim3(NT),
                  (unsigned)(2 * NT * IO<T>::VEC * sizeof(double)), s, (const T*)out, (const T*)g, (T*)gm, n, c,
                  (const T*)x_a, mean_a, invstd_a, (double*)part_a, (const T*)x_b, mean_b, invstd_b, (double*)part_b, sg.rpw);
    };
    if (x_b != nullptr) go(std::true_type{}); else go(std::false_type{});
    LIDAL_CHECK_LAUNCH("bn_bwd_partial_masked");
    return 0;
  });
}

// lidal_bn_bwd without its first pass: the f64 partials are in `part` already
extern "C" int lidal_bn_bwd_from_sums(const void* x, const void* dy, int64_t dy_stride, int dtype, int64_t n, int c,
                                      const float* gamma, const float* beta, int relu, const float* save_mean,
                                      const float* save_invstd, void* dx, float* grad_gamma, float* grad_beta,
                                      const void* part, int64_t part_bytes, void* stream) {
  if (int rc = bn_check(n, c, dtype)) return rc;
  LIDAL_REQUIRE(n > 0, "bn_bwd_from_sums: needs at least one row");
  LIDAL_REQUIRE(part_bytes >= lidal_bn_workspace_bytes(n, c), "bn_bwd_from_sums: partial buffer too small");
  if (int rc = dy_stride_check("bn_bwd_from_sums", c, dtype, dy_stride)) return rc;
  const BwdArgs a{x, dy, dy_stride, n, c, gamma, beta, relu, save_mean, save_invstd, dx, grad_gamma, grad_beta};
  return with_dtype(dtype, "bn_bwd_from_sums", [&](auto t) {
    return finish_bwd<decltype(t), false>(a, part, slab_grid(n).wgs, "bn_bwd_dx(sums merged in the launch)", "bn_bwd_final",
                                          (hipStream_t)stream);
  });
}

// The tail of a residual block backwards on the levels with many rows: gm = g * (out > 0) and, per part (a slab of
// rows: lidal_bn_tail_parts of them) and channel, the f32 pairs (sum gm, sum gm xhat) of the BatchNorm over x_a -- and
// over x_b, if given -- as [channel][part][2]: what lidal_bn_bwd_tiles takes as tile sums (n_tiles = the parts).
extern "C" int64_t lidal_bn_tail_parts(int64_t n, int c, int dtype) {
  return ew_grid(n, (int64_t)c * (dtype == LIDAL_F32 ? 4 : 2)).wgs;
}
extern "C" int lidal_add_relu_bwd_bn_tile_sums(const void* out, const void* g, void* gm, int dtype, int64_t n, int c,
                                               const void* x_a, const float* mean_a, const float* invstd_a, float* sums_a,
                                               const void* x_b, const float* mean_b, const float* invstd_b, float* sums_b,
                                               int64_t n_parts, void* stream) {
  if (int rc = bn_check(n, c, dtype)) return rc;
  LIDAL_REQUIRE(n > 0, "add_relu_bwd_bn_tile_sums: needs at least one row");
  LIDAL_REQUIRE(n_parts == lidal_bn_tail_parts(n, c, dtype), "add_relu_bwd_bn_tile_sums: %lld parts, lidal_bn_tail_parts says %lld",
                (long long)n_parts, (long long)lidal_bn_tail_parts(n, c, dtype));
  LIDAL_REQUIRE(x_a != nullptr && sums_a != nullptr && (x_b == nullptr || sums_b != nullptr),
                "add_relu_bwd_bn_tile_sums: a BatchNorm input without a buffer for its sums");
  hipStream_t s = (hipStream_t)stream;
  return with_dtype(dtype, "add_relu_bwd_bn_tile_sums", [&](auto t) {
    using T = decltype(t);
    const Grid e = ew_grid<T>(n, c);
    auto go = [&](auto dual) {
      launch_tail(tail_tile_sums_kernel<T, decltype(dual)::value>, dim3(e.wgs), dim3(NT), 0, s, (const T*)out, (const T*)g,
                  (T*)gm, n, c, (const T*)x_a, mean_a, invstd_a, sums_a, (const T*)x_b, mean_b, invstd_b, sums_b, e.rpw);
    };
    if (x_b != nullptr) go(std::true_type{}); else go(std::false_type{});
    LIDAL_CHECK_LAUNCH("add_relu_bwd_bn_tile_sums");
    return 0;
  });
}

// The backward sums came with dy as f32 (sum dy', sum dy' xhat) pairs per tile or slab of rows and column,
// [c][n_tiles][2] (lidal_add_relu_bwd_bn_tile_sums, or a producer's epilogue): merge them in f64, then the dx pass
extern "C" int lidal_bn_bwd_tiles(const void* x, const void* dy, int64_t dy_stride, int dtype, int64_t n, int c,
                                  const float* gamma, const float* beta, int relu, const float* save_mean,
                                  const float* save_invstd, void* dx, float* grad_gamma, float* grad_beta,
                                  const float* tile_sums, int64_t n_tiles, void* stream) {
  if (int rc = bn_check(n, c, dtype)) return rc;
  LIDAL_REQUIRE(n > 0 && n_tiles > 0 && tile_sums != nullptr, "bn_bwd_tiles: needs rows and tile sums");
  if (int rc = dy_stride_check("bn_bwd_tiles", c, dtype, dy_stride)) return rc;
  const BwdArgs a{x, dy, dy_stride, n, c, gamma, beta, relu, save_mean, save_invstd, dx, grad_gamma, grad_beta};
  return with_dtype(dtype, "bn_bwd_tiles", [&](auto t) {
    return finish_bwd<decltype(t), true>(a, tile_sums, (int)n_tiles, "bn_bwd_dx(tile sums merged in the launch)",
                                         "bn_bwd_final(tiles)", (hipStream_t)stream);
  });
}

extern "C" int lidal_bn_fold(const float* gamma, const float* beta, const float* running_mean,
                             const float* running_var, float eps, int c, float* scale,
                             float* shift, void* stream) {
  if (c <= 0) return 0;
  bn_fold_kernel<<<(unsigned)cdiv(c, 256), 256, 0, (hipStream_t)stream>>>(
      gamma, beta, running_mean, running_var, eps, c, scale, shift);
  LIDAL_CHECK_LAUNCH("lidal_bn_fold");
  return 0;
}

extern "C" int lidal_colsum(const void* x, int dtype, int64_t n, int c, float* out, void* ws,
                            int64_t ws_bytes, void* stream) {
  if (int rc = bn_check(n, c, dtype)) return rc;
  LIDAL_REQUIRE(n > 0, "colsum: needs at least one row");
  LIDAL_REQUIRE(ws_bytes >= lidal_bn_workspace_bytes(n, c) + 3 * (int64_t)c * 4, "colsum ws too small");
  hipStream_t s = (hipStream_t)stream;
  // ws: the partials, then (behind two unused rows of c floats that the required size has always counted) a row that
  // takes the merge kernel's second output
  double* part = (double*)ws;
  float* scratch = (float*)((char*)ws + (lidal_bn_workspace_bytes(n, c) / 8) * 8) + 2 * c;
  const Grid g = slab_grid(n);
  if (int rc = with_dtype(dtype, "colsum", [&](auto t) {
        using T = decltype(t);
        colsum_partial_kernel<T><<<g.wgs, NT, NT * IO<T>::VEC * sizeof(double), s>>>((const T*)x, n, c, part, g.rpw);
        LIDAL_CHECK_LAUNCH("colsum_partial");
        return 0;
      }))
    return rc;
  launch_tail(bn_bwd_final_kernel, dim3((unsigned)cdiv(c, 8)), dim3(NT), 0, s, (const double*)part, g.wgs, c, out, scratch);
  LIDAL_CHECK_LAUNCH("colsum_final");
  return 0;
}
