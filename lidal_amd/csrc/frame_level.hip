// Frame-level selection baselines (score/frame_level/ of the reference) for gfx950: the per-frame softmax entropy,
// margin and confidence (softmax_entropy.py, margin_sampling.py, least_confidence_sampling.py), the segment entropy
// (segment_entropy.py), the frame feature outfeat.mean(0) and the greedy k-center core-set (core_set.py).
//
// Every reduction runs in a fixed order that restates numpy; this unit is built with
// -ffp-contract=off (lidal_amd/build.py).  No float atomics: the only atomics are integer ones (an LDS class histogram,
// a min over the bits of non-negative floats, a max over packed (value, ~index) keys), exact in any order.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "npsum.h"

using namespace lidal;
using namespace lidal::npsum;

namespace {

// scipy.special.entr on an f32 value: -x * log(x) evaluated in double and rounded once; entr(0) = 0, entr(x < 0) = -inf
__device__ __forceinline__ float entr_f32(float x) {
  if (isnan(x)) return x;
  if (x > 0.f) {
    const double v = (double)x;
    return (float)(-v * log(v));
  }
  if (x == 0.f) return 0.f;
  return -INFINITY;
}

// per point of prob f32 [p, c]: ent = sum(entr(p / sum(p))) (both sums numpy's pairwise order of one row), and the
// two largest values as np.sort orders them: mar = top1 - top2, conf = top1.  Series k of `out` starts at out + k * p.
__global__ void __launch_bounds__(256) point_uncertainty_kernel(const float* __restrict__ prob, int64_t p, int c,
                                                                float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p) return;
  const float* row = prob + i * c;
  const float s = np_sum_f32(row, c);
  float term[kMaxClasses];
  float t1 = -INFINITY, t2 = -INFINITY;
#pragma unroll
  for (int j = 0; j < kMaxClasses; ++j)
    if (j < c) {
      const float v = row[j];
      term[j] = entr_f32(__fdiv_rn(v, s));
      if (v > t1) {
        t2 = t1;
        t1 = v;
      } else if (v > t2) {
        t2 = v;
      }
    }
  out[i] = np_sum_f32(term, c);
  out[p + i] = __fsub_rn(t1, t2);
  out[2 * p + i] = t1;
}

// numpy's f32 add-reduce of one block of at most 8192 contiguous values (npsum.h's np_block_walk), in parallel: lane 0
// walks the pairwise tree once and writes its leaves (at most 128: every leaf below a split holds more than 64 values)
// and the post-order of the additions to LDS, one lane sums each leaf, lane 0 combines the leaf sums in the walk's
// order.  Block b of series k (blockIdx = (b, k)) reads src[k * stride + b * 8192 ..) and writes sums[k * nb + b].
constexpr int MEAN_LANES = 128;
__global__ void __launch_bounds__(MEAN_LANES) block_sum_kernel(const float* __restrict__ src, int64_t n, int64_t stride,
                                                               int64_t nb, float* __restrict__ sums) {
  __shared__ int64_t st_off[64], st_n[64];
  __shared__ int st_phase[64];
  __shared__ int64_t leaf_off[MEAN_LANES];
  __shared__ int leaf_n[MEAN_LANES];
  __shared__ float leaf_val[MEAN_LANES];
  __shared__ short prog[2 * MEAN_LANES];        // post-order: a leaf index, or -1 = add the two values on top
  __shared__ float vals[64];
  __shared__ int n_leaves, n_prog;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x, k = blockIdx.y;
  const float* a = src + k * stride;
  const int64_t b0 = b * NP_BUFSIZE;
  const int64_t m = std::min<int64_t>(NP_BUFSIZE, n - b0);
  if (tid == 0) {
    int nl = 0, np_ = 0;
    np_block_walk(b0, m, st_off, st_n, st_phase,
                  [&](int64_t o, int64_t len) {
                    leaf_off[nl] = o; leaf_n[nl] = (int)len;
                    prog[np_++] = (short)nl++;
                  },
                  [&] { prog[np_++] = -1; });
    n_leaves = nl;
    n_prog = np_;
  }
  __syncthreads();
  if (tid < n_leaves) leaf_val[tid] = np_leaf_f32([&](int64_t t) { return a[t]; }, leaf_off[tid], (int64_t)leaf_n[tid]);
  __syncthreads();
  if (tid != 0) return;
  int vp = 0;
  for (int q = 0; q < n_prog; ++q) {
    const int op = prog[q];
    if (op >= 0) {
      vals[vp++] = leaf_val[op];
    } else {
      const float rgt = vals[--vp], lft = vals[--vp];
      vals[vp++] = __fadd_rn(lft, rgt);
    }
  }
  sums[k * nb + b] = vals[0];
}

// out[k] = (the block sums of series k added in order to 0) / n: numpy's f32 mean; n == 0 gives 0 / 0 = NaN
__global__ void mean_finish_kernel(const float* __restrict__ sums, int64_t nb, int series, int64_t n,
                                   float* __restrict__ out) {
  const int k = threadIdx.x;
  if (k >= series) return;
  float total = 0.f;
  for (int64_t b = 0; b < nb; ++b) total = __fadd_rn(total, sums[k * nb + b]);
  out[k] = __fdiv_rn(total, (float)n);
}

int np_means(const float* src, int64_t n, int series, float* sums, float* out, hipStream_t s) {
  const int64_t nb = cdiv(n, NP_BUFSIZE);
  if (nb > 0) {
    block_sum_kernel<<<dim3((unsigned)nb, (unsigned)series), MEAN_LANES, 0, s>>>(src, n, n, nb, sums);
    LIDAL_CHECK_LAUNCH("frame_block_sum");
  }
  mean_finish_kernel<<<1, 64, 0, s>>>(sums, nb, series, n, out);
  LIDAL_CHECK_LAUNCH("frame_mean_finish");
  return 0;
}

// segment_entropy.py:41-49 for supervoxel s (one workgroup): an LDS histogram of the predicted classes (predictions
// outside [0, class_num) count in n only), then in f64 and class order sv += -q_c * log2(q_c + 1e-12), q_c = cnt / n
constexpr int SE_BLOCK = 256;
constexpr int SE_MAXC = 256;
__global__ void __launch_bounds__(SE_BLOCK) sv_entropy_kernel(const int64_t* __restrict__ pred, int64_t p,
                                                              const int64_t* __restrict__ sv_ptr,
                                                              const int64_t* __restrict__ sv_idx, int class_num,
                                                              double* __restrict__ sv_ent) {
  __shared__ int hist[SE_MAXC];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int64_t beg = sv_ptr[s], end = sv_ptr[s + 1];
  for (int c = tid; c < class_num; c += SE_BLOCK) hist[c] = 0;
  __syncthreads();
  for (int64_t t = beg + tid; t < end; t += SE_BLOCK) {
    const int64_t q = sv_idx[t];
    if (q < 0 || q >= p) continue;               // refused on the host (lidal_amd.score.frame_level)
    const int64_t v = pred[q];
    if (v >= 0 && v < class_num) atomicAdd(&hist[v], 1);
  }
  __syncthreads();
  if (tid != 0) return;
  const double dn = (double)(end - beg);
  double sv = 0.0;
  for (int c = 0; c < class_num; ++c) {
    const double qc = (double)hist[c] / dn;     // an empty supervoxel: 0 / 0 = NaN, as the reference
    sv = __dadd_rn(sv, __dmul_rn(-qc, log2(__dadd_rn(qc, 1e-12))));
  }
  sv_ent[s] = sv;
}

// frame_sege += sv_sege * n / P over the supervoxels in order, left to right
__global__ void sv_entropy_sum_kernel(const double* __restrict__ sv_ent, const int64_t* __restrict__ sv_ptr, int s,
                                      int64_t p, double* __restrict__ out) {
  if (threadIdx.x != 0) return;
  const double dp = (double)p;
  double f = 0.0;
  for (int k = 0; k < s; ++k) f = __dadd_rn(f, __dmul_rn(sv_ent[k], (double)(sv_ptr[k + 1] - sv_ptr[k])) / dp);
  *out = f;
}

// outfeat.mean(0) of f32 [p, d >= 2]: numpy adds the rows one after the other, so each column is a sequential f32
// chain and stays one.  One workgroup per FF_COLS columns: all its lanes stream tiles of FF_ROWS rows into LDS (double
// buffered, the next tile's loads issued before the current tile is added), FF_COLS lanes of wave 0 walk the rows.
constexpr int FF_COLS = 16, FF_ROWS = 512, FF_THREADS = 512;
constexpr int FF_PER = FF_ROWS * FF_COLS / FF_THREADS;
__global__ void __launch_bounds__(FF_THREADS) frame_feature_kernel(const float* __restrict__ feat, int64_t p, int d,
                                                                   float* __restrict__ out) {
  __shared__ float tile[2][FF_ROWS][FF_COLS];
  const int tid = threadIdx.x;
  const int c0 = blockIdx.x * FF_COLS;
  const int lc = tid % FF_COLS, lr = tid / FF_COLS;
  const bool col_ok = c0 + lc < d;
  const int64_t ntiles = cdiv(p, FF_ROWS);
  float reg[FF_PER];
  auto load = [&](int64_t r0) {
#pragma unroll
    for (int k = 0; k < FF_PER; ++k) {
      const int64_t r = r0 + lr + k * (FF_THREADS / FF_COLS);
      reg[k] = (col_ok && r < p) ? feat[r * d + c0 + lc] : 0.f;
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int k = 0; k < FF_PER; ++k) tile[buf][lr + k * (FF_THREADS / FF_COLS)][lc] = reg[k];
  };
  if (ntiles > 0) {
    load(0);
    store(0);
  }
  __syncthreads();
  float acc = 0.f;
  for (int64_t t = 0; t < ntiles; ++t) {
    const int buf = (int)(t & 1);
    if (t + 1 < ntiles) load((t + 1) * FF_ROWS);
    if (tid < FF_COLS) {
      const int rows = (int)std::min<int64_t>(FF_ROWS, p - t * FF_ROWS);
      if (rows == FF_ROWS) {
#pragma unroll 16
        for (int r = 0; r < FF_ROWS; ++r) acc = __fadd_rn(acc, tile[buf][r][tid]);
      } else {
        for (int r = 0; r < rows; ++r) acc = __fadd_rn(acc, tile[buf][r][tid]);
      }
    }
    if (t + 1 < ntiles) store(buf ^ 1);
    __syncthreads();
  }
  if (tid < FF_COLS && c0 + tid < d) out[c0 + tid] = __fdiv_rn(acc, (float)p);
}

// ---- greedy core-set (core_set.py:74-92).  The distance of two rows: f32(numpy's pairwise f64 sum of the squared
// differences), then the f32 square root.  sqrtf, not __fsqrt_rn: without
// OCML_BASIC_ROUNDED_OPERATIONS the latter is the native (not correctly rounded) square root.
__device__ __forceinline__ float cs_dist(const float (&r)[NP_DMAX], const float* __restrict__ c, int d) {
  return sqrtf((float)np_d2_f64(r, [&](int f) { return (double)c[f]; }, d));
}

__global__ void __launch_bounds__(256) cs_reset_kernel(int64_t n, unsigned* __restrict__ md_bits,
                                                       int* __restrict__ selected) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  md_bits[i] = 0x7F800000u;          // +inf
  selected[i] = 0;
}

__global__ void __launch_bounds__(256) cs_mark_kernel(const int64_t* __restrict__ labeled, int64_t nl, int64_t n,
                                                      int* __restrict__ selected, int* __restrict__ status) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nl) return;
  const int64_t c = labeled[j];
  if (c < 0 || c >= n) {
    atomicAdd(&status[1], 1);
    return;
  }
  selected[c] = 1;
}

// min_dist[i] = min over the labeled rows of dist(x_i, x_l): CS_LCHUNK labeled rows per workgroup column, combined
// with an integer min over the bits of the (non-negative) f32 distances
constexpr int CS_LCHUNK = 32;
__global__ void __launch_bounds__(256) cs_init_kernel(const float* __restrict__ x, int64_t n, int d,
                                                      const int64_t* __restrict__ labeled, int64_t nl,
                                                      unsigned* __restrict__ md_bits) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float r[NP_DMAX];
  load_row_f32(x, i, d, r);
  const int64_t j0 = (int64_t)blockIdx.y * CS_LCHUNK, j1 = std::min<int64_t>(nl, j0 + CS_LCHUNK);
  float best = INFINITY;
  for (int64_t j = j0; j < j1; ++j) {
    const int64_t c = labeled[j];
    if (c < 0 || c >= n) continue;
    const float v = cs_dist(r, x + c * d, d);
    best = v < best ? v : best;
  }
  atomicMin(&md_bits[i], __float_as_uint(best));
}

// step t: take pick t-1 (the row of the largest key of step t-1; flag it if it was selected already), min_dist =
// minimum(min_dist, dist(., pick)); then (t < num_add) keys[t] = max over the rows of (bits(min_dist) << 32 | ~row):
// the largest distance, the lowest row on ties (np.argmax)
__global__ void __launch_bounds__(256) cs_step_kernel(const float* __restrict__ x, int64_t n, int d, int t, int num_add,
                                                      unsigned long long* __restrict__ keys, int64_t* __restrict__ picks,
                                                      int* __restrict__ selected, int* __restrict__ status,
                                                      float* __restrict__ md) {
  __shared__ unsigned long long red[256 / kWave];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + tid;
  int64_t c = -1;
  if (t > 0) {
    c = (int64_t)(~(unsigned)(keys[t - 1] & 0xFFFFFFFFull));
    if (c >= n) {                         // cannot happen (row 0 always offers a key); never read out of bounds
      if (blockIdx.x == 0 && tid == 0) status[0] = -t;
      c = 0;
    }
    if (blockIdx.x == 0 && tid == 0) {
      picks[t - 1] = c;
      if (selected[c] && status[0] == 0) status[0] = t;        // core_set.py:86 asserts here
      selected[c] = 1;
    }
  }
  unsigned long long key = 0;
  if (i < n) {
    float m = md[i];
    if (t > 0) {
      float r[NP_DMAX];
      load_row_f32(x, i, d, r);
      const float v = cs_dist(r, x + c * d, d);
      m = v < m ? v : m;
      md[i] = m;
    }
    key = ((unsigned long long)__float_as_uint(m) << 32) | (unsigned long long)(~(unsigned)i);
  }
  if (t >= num_add) return;
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(key, o);
    key = other > key ? other : key;
  }
  if ((tid % kWave) == 0) red[tid / kWave] = key;
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < 256 / kWave; ++w) key = red[w] > key ? red[w] : key;
  atomicMax(&keys[t], key);
}

// Workspace layouts: one function per builder sizes its scratch (NULL address) and carves it (common.h Carver; the
// members are the regions in order).
struct CoresetWs { unsigned long long* keys; int* selected; int64_t total; };
CoresetWs cs_layout(int64_t n, int num_add, void* ws) {
  Carver c(ws);
  return {c.take<unsigned long long>(std::max(num_add, 1)), c.take<int>(std::max<int64_t>(n, 1)), c.total()};
}

struct UncertaintyWs { float *per_point, *sums; int64_t total; };      // [p, 3] | np_means' partial sums of the columns
UncertaintyWs uncertainty_layout(int64_t p, void* ws) {
  Carver c(ws);
  return {c.take<float>(3 * std::max<int64_t>(p, 1)), c.take<float>(3 * std::max<int64_t>(cdiv(p, NP_BUFSIZE), 1)), c.total()};
}

}  // namespace

// ---------------------------------------------------------------- ENT / MAR / CONF
extern "C" int64_t lidal_frame_uncertainty_workspace_bytes(int64_t p) { return uncertainty_layout(p, nullptr).total; }

extern "C" int lidal_frame_uncertainty(const float* prob, int64_t p, int c, float* out, void* ws, int64_t ws_bytes,
                                       void* stream) {
  LIDAL_REQUIRE(c >= 2 && c <= kMaxClasses, "frame_uncertainty: classes must be in 2..%d (the margin needs two)",
                kMaxClasses);
  LIDAL_REQUIRE(p >= 0, "frame_uncertainty: negative point count");
  const UncertaintyWs w = uncertainty_layout(p, ws);
  LIDAL_REQUIRE(ws_bytes >= w.total, "frame_uncertainty workspace too small");
  hipStream_t s = (hipStream_t)stream;
  if (p > 0) {
    point_uncertainty_kernel<<<(unsigned)cdiv(p, 256), 256, 0, s>>>(prob, p, c, w.per_point);
    LIDAL_CHECK_LAUNCH("frame_point_uncertainty");
  }
  return np_means(w.per_point, p, 3, w.sums, out, s);
}

// ---------------------------------------------------------------- SEGENT
extern "C" int64_t lidal_segment_entropy_workspace_bytes(int s) { return align_up(8 * (int64_t)std::max(s, 1), 256); }

extern "C" int lidal_segment_entropy(const int64_t* pred, int64_t p, const int64_t* sv_ptr, const int64_t* sv_idx, int s,
                                     int class_num, double* out, void* ws, int64_t ws_bytes, void* stream) {
  LIDAL_REQUIRE(class_num >= 1 && class_num <= SE_MAXC, "segment_entropy: class_num must be in 1..%d", SE_MAXC);
  LIDAL_REQUIRE(s >= 0 && p >= 0, "segment_entropy: negative supervoxel or point count");
  LIDAL_REQUIRE(ws_bytes >= lidal_segment_entropy_workspace_bytes(s), "segment_entropy workspace too small");
  hipStream_t st = (hipStream_t)stream;
  double* sv_ent = (double*)ws;
  if (s > 0) {
    sv_entropy_kernel<<<(unsigned)s, SE_BLOCK, 0, st>>>(pred, p, sv_ptr, sv_idx, class_num, sv_ent);
    LIDAL_CHECK_LAUNCH("segment_entropy_sv");
  }
  sv_entropy_sum_kernel<<<1, 64, 0, st>>>(sv_ent, sv_ptr, s, p, out);
  LIDAL_CHECK_LAUNCH("segment_entropy_sum");
  return 0;
}

// ---------------------------------------------------------------- CSET frame feature
extern "C" int64_t lidal_frame_feature_workspace_bytes(int64_t p) {
  return align_up(4 * std::max<int64_t>(cdiv(p, NP_BUFSIZE), 1), 256);
}

extern "C" int lidal_frame_feature(const float* feat, int64_t p, int d, float* out, void* ws, int64_t ws_bytes,
                                   void* stream) {
  LIDAL_REQUIRE(d >= 1, "frame_feature: the feature width must be positive");
  LIDAL_REQUIRE(p >= 0, "frame_feature: negative point count");
  LIDAL_REQUIRE(ws_bytes >= lidal_frame_feature_workspace_bytes(p), "frame_feature workspace too small");
  hipStream_t s = (hipStream_t)stream;
  if (d == 1) return np_means(feat, p, 1, (float*)ws, out, s);     // an [n, 1] array is reduced as a contiguous one
  frame_feature_kernel<<<(unsigned)cdiv(d, FF_COLS), FF_THREADS, 0, s>>>(feat, p, d, out);
  LIDAL_CHECK_LAUNCH("frame_feature");
  return 0;
}

// ---------------------------------------------------------------- CSET greedy k-center
extern "C" int64_t lidal_coreset_workspace_bytes(int64_t n, int num_add) {
  return cs_layout(n, num_add, nullptr).total;
}

extern "C" int lidal_coreset(const float* feats, int64_t n, int d, const int64_t* labeled, int64_t n_labeled, int num_add,
                             int64_t* picks, float* min_dist, int32_t* status_dev, void* ws, int64_t ws_bytes,
                             void* stream) {
  LIDAL_REQUIRE(d >= 1 && d <= NP_DMAX, "coreset: the feature width must be in 1..%d", NP_DMAX);
  LIDAL_REQUIRE(n >= 1 && n < 0x7FFFFFFF, "coreset: the frame count must be in 1..2^31 - 2");
  LIDAL_REQUIRE(n_labeled >= 1, "coreset: no labeled frame (the reference's np.min over an empty axis fails)");
  LIDAL_REQUIRE(n_labeled <= (int64_t)CS_LCHUNK * 65535, "coreset: at most %d labeled frames", CS_LCHUNK * 65535);
  LIDAL_REQUIRE(num_add >= 0 && (int64_t)num_add <= n - n_labeled,
                "coreset: num_add (%d) must be in 0..the unlabeled count (%lld)", num_add, (long long)(n - n_labeled));
  const CoresetWs w = cs_layout(n, num_add, ws);
  LIDAL_REQUIRE(ws_bytes >= w.total, "coreset workspace too small");
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* keys = w.keys;
  int* selected = w.selected;
  const unsigned gn = (unsigned)cdiv(n, 256);
  LIDAL_HIP(hipMemsetAsync(status_dev, 0, 8, s));
  LIDAL_HIP(hipMemsetAsync(keys, 0, 8 * (size_t)std::max(num_add, 1), s));
  cs_reset_kernel<<<gn, 256, 0, s>>>(n, (unsigned*)min_dist, selected);
  LIDAL_CHECK_LAUNCH("coreset_reset");
  cs_mark_kernel<<<(unsigned)cdiv(n_labeled, 256), 256, 0, s>>>(labeled, n_labeled, n, selected, status_dev);
  LIDAL_CHECK_LAUNCH("coreset_mark");
  cs_init_kernel<<<dim3(gn, (unsigned)cdiv(n_labeled, CS_LCHUNK)), 256, 0, s>>>(feats, n, d, labeled, n_labeled,
                                                                                 (unsigned*)min_dist);
  LIDAL_CHECK_LAUNCH("coreset_init");
  // one launch per pick: each step needs the previous step's whole-array argmax (dependent, latency-bound seams)
  for (int t = 0; t <= num_add; ++t) {
    cs_step_kernel<<<gn, 256, 0, s>>>(feats, n, d, t, num_add, keys, picks, selected, status_dev, min_dist);
    LIDAL_CHECK_LAUNCH("coreset_step");
  }
  return 0;
}
