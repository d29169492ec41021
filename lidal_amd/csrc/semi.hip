// The mean-teacher step of semi-supervised training (Tarvainen & Valpola 2017; what LaserMix / PolarMix train with):
//   * lidal_ema_step          teacher = EMA of the student over EVERY parameter and buffer, in ONE launch;
//   * lidal_pseudo_labels     the teacher's confident predictions as labels of the points nobody annotated, one launch;
//   * lidal_consistency_fwd   the consistency term between student and teacher, 'mse' of the two softmaxes (mean teacher,
//     lidal_consistency_bwd   LaserMix) or 'kl' (distillation), and its gradient with respect to the student.
// The definitions are this project's own; tests/semi_ref.py restates them in numpy.  Built without fma contraction and
// without packed-f32 instructions (lidal_amd/build.py); vector stores only, no float atomics: every float sum has one
// fixed order, so two runs give the same bits.
//
// The row softmax everywhere is the view form of rows.h, score.hip's: first maximum, expf(x - mx), running f32 sum in
// class order, f32 divide.
#include "multi_tensor.h"
#include "rows.h"

#pragma clang fp contract(off)

namespace lidal {
namespace {

using npsum::np_sum_f32;
using namespace rows;

// ---------------------------------------------------------------------------------------------------------- EMA
// t = t + (s - t) * oma per f32 element (kind 0), or a copy of 32-bit words with no arithmetic on them (kind 1), over the
// record table, virtual axis (vstart from the teacher's address), chunk walk and piece mover of multi_tensor.h.
struct EmaRec {             // five 64-bit words: the table's record
  uint64_t t;               // address of the teacher's tensor
  uint64_t s;               // address of the student's
  int64_t vstart;           // first word on the virtual axis (ascending with the record index, no overlap)
  int64_t n;                // 32-bit words (an int64 element is two)
  int64_t kind;             // 0: lerp (f32), 1: copy
};

__device__ __forceinline__ unsigned ema_word(unsigned t, unsigned s, float oma) {
  const float tf = __uint_as_float(t), sf = __uint_as_float(s);
  return __float_as_uint(tf + (sf - tf) * oma);
}

// The two rules for multi_tensor::move_piece, on words: array 0 the teacher, 1 the student (never written).
struct EmaLerp {
  typedef unsigned Elem;
  static constexpr int kArrays = 2;
  static constexpr unsigned kLoads = 3, kStores = 1;
  float oma;
  __device__ __forceinline__ void update(unsigned (&x)[2]) const { x[0] = ema_word(x[0], x[1], oma); }
};

struct EmaCopy {            // the teacher is written, never read
  typedef unsigned Elem;
  static constexpr int kArrays = 2;
  static constexpr unsigned kLoads = 2, kStores = 1;
  __device__ __forceinline__ void update(unsigned (&x)[2]) const { x[0] = x[1]; }
};

template <typename Rule>
__device__ __forceinline__ void ema_piece(const Rule& rule, const EmaRec& R, int64_t a, int64_t e) {
  multi_tensor::Arrays<Rule> A;
  A.p[0] = (LIDAL_GLOBAL unsigned*)R.t;
  A.p[1] = (LIDAL_GLOBAL unsigned*)R.s;
  multi_tensor::move_piece(rule, A, a, e);
}

__global__ __launch_bounds__(multi_tensor::kThreads) void ema_step_kernel(const EmaRec* __restrict__ recs, int n_recs,
                                                                          int64_t n_chunks, float oma, int all_copy) {
  multi_tensor::walk_chunks(recs, 0, n_recs, 0, n_chunks, [&](const EmaRec R, int64_t a, int64_t e) {
    if (R.n <= 0) return;
    if (all_copy || R.kind != 0)
      ema_piece(EmaCopy{}, R, a, e);
    else
      ema_piece(EmaLerp{oma}, R, a, e);
  });
}

// ---------------------------------------------------------------------------------------------------------- pseudo labels
constexpr int PL_THREADS = 256;

template <typename T>
__global__ void __launch_bounds__(PL_THREADS) pseudo_labels_kernel(const T* __restrict__ logits, int64_t nv, int c,
                                                                   const float* __restrict__ thresholds, float threshold,
                                                                   const int64_t* __restrict__ inverse,
                                                                   const int64_t* __restrict__ labels,
                                                                   int64_t ignore_index, int64_t p,
                                                                   int64_t* __restrict__ out,
                                                                   unsigned long long* __restrict__ stats,
                                                                   float* __restrict__ conf_out) {
  __shared__ int cnt[kMaxClasses + 2];
  if (threadIdx.x < kMaxClasses + 2) cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x;
  if (i < p) {
    const int64_t row = inverse != nullptr ? inverse[i] : i;
    const bool in = row >= 0 && row < nv;                 // a bad index is never read through
    const int64_t human = labels != nullptr ? labels[i] : ignore_index;
    int arg = 0;
    float conf = 0.f;
    if (in) {
      float x[kMaxClasses], mx, s;
      arg = row_exp<float>(logits + row * c, c, x, mx, s);
      conf = pick(x, c, arg) / s;
    }
    int64_t y = ignore_index;
    int slot = -1;
    if (human != ignore_index) {
      y = human;                                          // (in none of the counts)
    } else if (!in) {
      slot = c + 1;
    } else {
      const float thr = thresholds != nullptr ? thresholds[arg] : threshold;
      if (conf >= thr) { y = arg; slot = arg; } else slot = c;        // (a NaN compares false: rejected)
    }
    out[i] = y;
    if (conf_out != nullptr) conf_out[i] = conf;
    if (slot >= 0) atomicAdd(&cnt[slot], 1);
  }
  __syncthreads();
  if ((int)threadIdx.x < c + 2 && cnt[threadIdx.x] != 0)
    atomicAdd(&stats[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------------------- consistency
enum { KIND_MSE = 0, KIND_KL = 1 };

// What both passes know of one row.  Logits: ps / pt the two softmaxes, ls / lt the log-softmaxes (kind 'kl').
// Probabilities: ps / pt as given.  conf = the teacher's first maximum.
struct RowPair {
  float ps[kMaxClasses], pt[kMaxClasses], dl[kMaxClasses];      // dl = lt - ls ('kl' on logits)
  float conf;
};

template <bool PROBS>
__device__ __forceinline__ void row_pair(const float (&zs)[kMaxClasses], const float (&zt)[kMaxClasses], int c, int kind,
                                         RowPair& R) {
  if (PROBS) {
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < kMaxClasses; ++j)
      if (j < c) { R.ps[j] = zs[j]; R.pt[j] = zt[j]; mx = fmaxf(mx, R.pt[j]); }
    R.conf = mx;
    return;
  }
  float mxs, ss, mxt, st;
  row_exp<float>(zs, c, R.ps, mxs, ss);
  const int arg = row_exp<float>(zt, c, R.pt, mxt, st);
  R.conf = pick(R.pt, c, arg) / st;
  const float lss = logf(ss), lst = logf(st);
#pragma unroll
  for (int j = 0; j < kMaxClasses; ++j)
    if (j < c) {
      R.ps[j] = R.ps[j] / ss;
      R.pt[j] = R.pt[j] / st;
      if (kind == KIND_KL) R.dl[j] = ((zt[j] - mxt) - lst) - ((zs[j] - mxs) - lss);
    }
}

// the workgroup's rows of both operands, each thread's own pair into its registers, through ONE LDS image
template <typename TS, typename TT>
__device__ __forceinline__ void load_pair(const Tile& tile, const TS* __restrict__ zs_g, const TT* __restrict__ zt_g,
                                          float (&zs)[kMaxClasses], float (&zt)[kMaxClasses]) {
  tile.load<TS>(zs_g, false);           // false here, and at the store of dz: the switch to 16-byte vectors
  __syncthreads();
  tile.own(zs);
  __syncthreads();
  tile.load<TT>(zt_g, false);
  __syncthreads();
  tile.own(zt);
}

// r_i (masked) of every row, per_row (optional), and the workgroup's f64 partial in a fixed order
template <typename TS, typename TT, bool PROBS>
__global__ void __launch_bounds__(kRows) consistency_fwd_kernel(const TS* __restrict__ zs, const TT* __restrict__ zt,
                                                                int64_t n, int c, int kind, float min_conf,
                                                                float* __restrict__ per_row,
                                                                double* __restrict__ part) {
  __shared__ float lds[kTileFloats];
  __shared__ double red[1][kRows];
  const Tile tile(lds, n, c);
  float xs[kMaxClasses], xt[kMaxClasses];
  load_pair<TS, TT>(tile, zs, zt, xs, xt);
  float r = 0.f;
  if ((int)threadIdx.x < tile.nrows) {
    float* mine = tile.mine();
    RowPair R;
    row_pair<PROBS>(xs, xt, c, kind, R);
    if (R.conf >= min_conf) {                               // (a NaN confidence masks the row)
#pragma unroll
      for (int j = 0; j < kMaxClasses; ++j)
        if (j < c) {
          if (kind == KIND_MSE) {
            const float d = R.ps[j] - R.pt[j];
            mine[j] = d * d;
          } else {
            mine[j] = R.pt[j] == 0.f ? 0.f : R.pt[j] * R.dl[j];
          }
        }
      r = np_sum_f32(mine, c);                              // (the thread's own LDS row: no one else reads it any more)
    }
    if (per_row != nullptr) per_row[tile.row0 + threadIdx.x] = r;
  }
  const double v[1] = {(double)r};
  block_sum<1>(v, red);
  if (threadIdx.x == 0) part[blockIdx.x] = red[0][0];
}

// out2 = {sum / denom, sum}: one workgroup, fixed order
__global__ void __launch_bounds__(kRows) consistency_final_kernel(const double* __restrict__ part, int64_t nblocks,
                                                                  double denom, double* __restrict__ out2) {
  __shared__ double red[1][kRows];
  sum_partials<1>(part, nblocks, red);
  if (threadIdx.x == 0) {
    out2[0] = red[0][0] / denom;
    out2[1] = red[0][0];
  }
}

// dz of every row; k1 = the scale of the objective as f32: 1 / (n c) ('mse' on logits), 2 / (n c) ('mse' on
// probabilities), 1 / n ('kl'); coef = g * k1 is ONE f32 product, and so is every product below.
template <typename TS, typename TT, bool PROBS>
__global__ void __launch_bounds__(kRows) consistency_bwd_kernel(const TS* __restrict__ zs, const TT* __restrict__ zt,
                                                                int64_t n, int c, int kind, float min_conf, float k1,
                                                                const float* __restrict__ grad_scale,
                                                                TS* __restrict__ dz) {
  __shared__ float lds[kTileFloats];
  const Tile tile(lds, n, c);
  float xs[kMaxClasses], xt[kMaxClasses];
  load_pair<TS, TT>(tile, zs, zt, xs, xt);
  if ((int)threadIdx.x < tile.nrows) {
    float* mine = tile.mine();
    const float coef = grad_scale[0] * k1;
    RowPair R;
    row_pair<PROBS>(xs, xt, c, kind, R);
    const bool on = R.conf >= min_conf;
    float dot = 0.f;
    if (!PROBS && kind == KIND_MSE) {
#pragma unroll
      for (int j = 0; j < kMaxClasses; ++j)
        if (j < c) dot = dot + R.ps[j] * (2.f * (R.ps[j] - R.pt[j]));
    }
#pragma unroll
    for (int j = 0; j < kMaxClasses; ++j)
      if (j < c) {
        const float d = R.ps[j] - R.pt[j];
        float g;
        if (PROBS || kind == KIND_KL) g = coef * d;
        else g = coef * (R.ps[j] * (2.f * d - dot));
        mine[j] = on ? g : 0.f;
      }
  }
  __syncthreads();
  tile.store<TS>(dz, false);
}

int consistency_check(const char* what, int64_t n, int c, int s_dtype, int t_dtype, int kind, int is_probs) {
  LIDAL_REQUIRE(c >= 1 && c <= kMaxClasses, "%s: classes must be in 1..%d (got %d)", what, kMaxClasses, c);
  LIDAL_REQUIRE(n >= 0 && n * (int64_t)c < (1ll << 30), "%s: %lld rows x %d classes reach 2^30 entries", what,
                (long long)n, c);
  LIDAL_REQUIRE(kind == KIND_MSE || kind == KIND_KL, "%s: kind must be 0 (mse) or 1 (kl), got %d", what, kind);
  LIDAL_REQUIRE(s_dtype == LIDAL_F32 || s_dtype == LIDAL_BF16, "%s: bad student dtype %d", what, s_dtype);
  LIDAL_REQUIRE(t_dtype == LIDAL_F32 || t_dtype == LIDAL_BF16, "%s: bad teacher dtype %d", what, t_dtype);
  LIDAL_REQUIRE(!is_probs || (kind == KIND_MSE && s_dtype == LIDAL_F32 && t_dtype == LIDAL_F32),
                "%s: probabilities are f32 and take 'mse' only", what);
  return 0;
}

struct ConsistencyWs {
  double* part;
  int64_t nb, total;
};

ConsistencyWs consistency_layout(void* base, int64_t n) {
  ConsistencyWs w;
  w.nb = cdiv(n > 0 ? n : 1, kRows);
  Carver cv(base);
  w.part = cv.take<double>(w.nb);
  w.total = cv.total();
  return w;
}

}  // namespace
}  // namespace lidal

using namespace lidal;

extern "C" int lidal_ema_chunk_elems(void) { return multi_tensor::kChunk; }

extern "C" int lidal_ema_step(const void* table, int n_recs, int64_t v_end, double one_minus_alpha, int all_copy,
                              void* stream) {
  LIDAL_REQUIRE(n_recs >= 0 && v_end >= 0, "lidal_ema_step: %d records, virtual end %lld", n_recs, (long long)v_end);
  LIDAL_REQUIRE(table != nullptr || n_recs == 0, "lidal_ema_step: null table");
  LIDAL_REQUIRE(one_minus_alpha >= 0.0 && one_minus_alpha <= 1.0, "lidal_ema_step: 1 - alpha = %g is outside [0, 1]",
                one_minus_alpha);
  if (n_recs == 0 || v_end == 0) return 0;
  const int64_t n_chunks = cdiv(v_end, multi_tensor::kChunk);
  hipLaunchKernelGGL(ema_step_kernel, dim3(multi_tensor::grid_for(n_chunks)), dim3(multi_tensor::kThreads), 0,
                     (hipStream_t)stream, (const EmaRec*)table, n_recs, n_chunks, (float)one_minus_alpha, all_copy);
  LIDAL_CHECK_LAUNCH("lidal_ema_step");
  return 0;
}

extern "C" int lidal_pseudo_labels(const void* logits, int dtype, int64_t nv, int c, const float* thresholds,
                                   double threshold, const int64_t* inverse, const int64_t* labels, int64_t ignore_index,
                                   int64_t p, int64_t* out, int64_t* stats, float* conf, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  LIDAL_REQUIRE(c >= 1 && c <= kMaxClasses, "pseudo_labels: classes must be in 1..%d (got %d)", kMaxClasses, c);
  LIDAL_REQUIRE(nv >= 0 && p >= 0 && nv * (int64_t)c < (1ll << 40), "pseudo_labels: %lld rows, %lld points",
                (long long)nv, (long long)p);
  LIDAL_REQUIRE(inverse != nullptr || p == nv, "pseudo_labels: without an inverse map there is one point per row");
  LIDAL_REQUIRE(dtype == LIDAL_F32 || dtype == LIDAL_BF16, "pseudo_labels: bad dtype %d", dtype);
  LIDAL_REQUIRE(stats != nullptr && (out != nullptr || p == 0) && (logits != nullptr || nv == 0),
                "pseudo_labels: null output or logits");
  LIDAL_HIP(hipMemsetAsync(stats, 0, (size_t)(c + 2) * 8, s));
  if (p == 0) return 0;
  const unsigned nb = (unsigned)cdiv(p, PL_THREADS);
  return with_dtype(dtype, "pseudo_labels", [&](auto t) {
    using T = decltype(t);
    pseudo_labels_kernel<T><<<nb, PL_THREADS, 0, s>>>((const T*)logits, nv, c, thresholds, (float)threshold, inverse,
                                                      labels, ignore_index, p, out, (unsigned long long*)stats, conf);
    LIDAL_CHECK_LAUNCH("pseudo_labels");
    return 0;
  });
}

extern "C" int64_t lidal_consistency_workspace_bytes(int64_t n) {
  if (n < 0) return 0;
  return consistency_layout(nullptr, n).total;
}

extern "C" int lidal_consistency_fwd(const void* student, int s_dtype, const void* teacher, int t_dtype, int64_t n, int c,
                                     int kind, int is_probs, double min_conf, double* out2, float* per_row, void* ws,
                                     int64_t ws_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (int rc = consistency_check("consistency_fwd", n, c, s_dtype, t_dtype, kind, is_probs)) return rc;
  LIDAL_REQUIRE(n > 0 && student != nullptr && teacher != nullptr && out2 != nullptr && ws != nullptr,
                "consistency_fwd: no rows or a null operand");
  const ConsistencyWs w = consistency_layout(ws, n);
  LIDAL_REQUIRE(ws_bytes >= w.total, "consistency workspace too small: %lld < %lld", (long long)ws_bytes,
                (long long)w.total);
  const unsigned nb = (unsigned)w.nb;
  const float mc = (float)min_conf;
#define LIDAL_CS_FWD(TS, TT, P) \
  consistency_fwd_kernel<TS, TT, P><<<nb, kRows, 0, s>>>((const TS*)student, (const TT*)teacher, n, c, kind, mc, per_row, w.part)
  if (is_probs) LIDAL_CS_FWD(float, float, true);
  else if (s_dtype == LIDAL_F32 && t_dtype == LIDAL_F32) LIDAL_CS_FWD(float, float, false);
  else if (s_dtype == LIDAL_F32) LIDAL_CS_FWD(float, __bf16, false);
  else if (t_dtype == LIDAL_F32) LIDAL_CS_FWD(__bf16, float, false);
  else LIDAL_CS_FWD(__bf16, __bf16, false);
#undef LIDAL_CS_FWD
  LIDAL_CHECK_LAUNCH("consistency_fwd");
  const double denom = kind == KIND_MSE ? (double)n * (double)c : (double)n;
  consistency_final_kernel<<<1, 256, 0, s>>>(w.part, w.nb, denom, out2);
  LIDAL_CHECK_LAUNCH("consistency_final");
  return 0;
}

extern "C" int lidal_consistency_bwd(const void* student, int s_dtype, const void* teacher, int t_dtype, int64_t n, int c,
                                     int kind, int is_probs, double min_conf, const float* grad_scale, void* dz,
                                     void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (int rc = consistency_check("consistency_bwd", n, c, s_dtype, t_dtype, kind, is_probs)) return rc;
  LIDAL_REQUIRE(n > 0 && student != nullptr && teacher != nullptr && grad_scale != nullptr && dz != nullptr,
                "consistency_bwd: no rows or a null operand");
  const unsigned nb = (unsigned)cdiv(n, kRows);
  const float mc = (float)min_conf;
  const double nd = (double)n;
  const float k1 = kind == KIND_KL ? (float)(1.0 / nd) : (float)((is_probs ? 2.0 : 1.0) / (nd * (double)c));
#define LIDAL_CS_BWD(TS, TT, P) \
  consistency_bwd_kernel<TS, TT, P><<<nb, kRows, 0, s>>>((const TS*)student, (const TT*)teacher, n, c, kind, mc, k1, grad_scale, (TS*)dz)
  if (is_probs) LIDAL_CS_BWD(float, float, true);
  else if (s_dtype == LIDAL_F32 && t_dtype == LIDAL_F32) LIDAL_CS_BWD(float, float, false);
  else if (s_dtype == LIDAL_F32) LIDAL_CS_BWD(float, __bf16, false);
  else if (t_dtype == LIDAL_F32) LIDAL_CS_BWD(__bf16, float, false);
  else LIDAL_CS_BWD(__bf16, __bf16, false);
#undef LIDAL_CS_BWD
  LIDAL_CHECK_LAUNCH("consistency_bwd");
  return 0;
}
