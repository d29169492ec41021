// Probability-inference post-processing and LiDAL inter-frame divergence / entropy scoring
// for gfx950.  Replaces score/prob_inference.py:100-113 and score/sv_level/LiDAL.py:59-98.
//
// All kernels are HBM/L2-bound gathers over [points, classes] f32 rows (76-byte rows for 19
// classes); the arithmetic follows numpy/scipy's float widths and summation orders
// (f32 pairwise-8 row sums, f64 KL terms rounded to f32, f64 divergence accumulator).
#include <cstring>


#include "common.h"
#include "grid.h"
#include "rows.h"

// The reference computes these quantities with numpy (separately rounded products and sums); hipcc
// contracts a*b+c into fma even through __dmul_rn/__dadd_rn, so this unit is built with
// -ffp-contract=off (lidal_amd/build.py).

using namespace lidal;
using namespace lidal::grid;
using namespace lidal::npsum;
using lidal::rows::row_exp;

namespace {

// ---------------- view-mean softmax ----------------
__global__ void __launch_bounds__(256) view_mean_softmax_kernel(const float* __restrict__ logits,
                                                                const int64_t* __restrict__ inverse,
                                                                int reps, int64_t p, int c,
                                                                float* __restrict__ prob,
                                                                int64_t* __restrict__ pred) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p) return;
  float acc[kMaxClasses];
#pragma unroll
  for (int j = 0; j < kMaxClasses; ++j) acc[j] = 0.f;
  for (int v = 0; v < reps; ++v) {
    float x[kMaxClasses], mx, s;
    row_exp<float>(logits + inverse[(int64_t)v * p + i] * c, c, x, mx, s);
#pragma unroll
    for (int j = 0; j < kMaxClasses; ++j)
      if (j < c) acc[j] = (v == 0) ? (x[j] / s) : __fadd_rn(acc[j], x[j] / s);
  }
  float best = -INFINITY;
  int arg = 0;
  const float inv = (float)reps;
#pragma unroll
  for (int j = 0; j < kMaxClasses; ++j)
    if (j < c) {
      float m = acc[j] / inv;
      prob[i * c + j] = m;
      if (m > best) { best = m; arg = j; }
    }
  pred[i] = arg;
}

// ---------------- disagreement of the views ----------------
// The soft-max of a gathered logits row is rows.h's row_exp<float> and a divide by s, view_mean_softmax_kernel's: view_scores_kernel
// reads every row twice through it and gets the same bits both times.
//
// LiDAL.py:59-81 with the point's own view mean m where the query frame stands and its views p_v where the matched
// neighbours stand: viewd = (1 / reps) sum_v np_sum_f32_k (float)kl_div(m_k + eps, p_vk + eps) in an f64 accumulator,
// viewe = scipy's entropy(m), agree = the views whose logits row has its first maximum at pred.  prob and pred are
// view_mean_softmax_kernel's, restated (tests/test_view_scores_gpu.py holds the two to the same bytes).  m needs every
// view before the first term can be formed, and reps rows of probabilities do not fit registers at a run-time reps: the
// thread gathers its rows a second time (they are in the caches from the first) and recomputes p_v.
__global__ void __launch_bounds__(256) view_scores_kernel(const float* __restrict__ logits,
                                                          const int64_t* __restrict__ inverse, int reps, int64_t p,
                                                          int c, float* __restrict__ prob, int64_t* __restrict__ pred,
                                                          double* __restrict__ viewd, float* __restrict__ viewe,
                                                          int* __restrict__ agree) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p) return;
  float m[kMaxClasses];
#pragma unroll
  for (int j = 0; j < kMaxClasses; ++j) m[j] = 0.f;
  for (int v = 0; v < reps; ++v) {
    float x[kMaxClasses], mx, s;
    row_exp<float>(logits + inverse[(int64_t)v * p + i] * c, c, x, mx, s);
#pragma unroll
    for (int j = 0; j < kMaxClasses; ++j)
      if (j < c) m[j] = (v == 0) ? (x[j] / s) : __fadd_rn(m[j], x[j] / s);
  }
  float best = -INFINITY;
  int arg = 0;
  const float inv = (float)reps;
#pragma unroll
  for (int j = 0; j < kMaxClasses; ++j)
    if (j < c) {
      m[j] = m[j] / inv;
      prob[i * c + j] = m[j];
      if (m[j] > best) { best = m[j]; arg = j; }
    }
  pred[i] = arg;
  const float eps = 0.00001f;
  double div = 0.0;
  int votes = 0;
  for (int v = 0; v < reps; ++v) {
    float x[kMaxClasses], mx, s;
    votes += (row_exp<float>(logits + inverse[(int64_t)v * p + i] * c, c, x, mx, s) == arg) ? 1 : 0;
    float term[kMaxClasses];
#pragma unroll
    for (int k = 0; k < kMaxClasses; ++k)
      if (k < c) {
        double a = (double)__fadd_rn(m[k], eps), b = (double)__fadd_rn(x[k] / s, eps);
        // scipy.special.kl_div(a, b) = a log(a/b) - a + b  (a, b > 0 here), f32 result
        term[k] = (float)(a * log(a / b) - a + b);
      }
    div += (double)np_sum_f32(term, c);
  }
  // scipy.stats.entropy(m), as interframe_kernel takes it of its mean row
  float tot = np_sum_f32(m, c);
  float ent[kMaxClasses];
#pragma unroll
  for (int k = 0; k < kMaxClasses; ++k)
    if (k < c) {
      float q = m[k] / tot;
      ent[k] = (q > 0.f) ? (float)(-(double)q * log((double)q)) : 0.f;
    }
  viewe[i] = np_sum_f32(ent, c);
  viewd[i] = div / (double)reps;
  agree[i] = votes;
}

// ---------------- MC-dropout: mutual information of the passes ----------------
// H(q) = sum_k (q_k > 0 ? -q_k log q_k : 0): an f64 expression of the f32 q_k, summed in f64 in class order
__device__ __forceinline__ double entropy_f64(const float (&q)[kMaxClasses], int c) {
  double h = 0.0;
#pragma unroll
  for (int k = 0; k < kMaxClasses; ++k)
    if (k < c && q[k] > 0.f) h += -(double)q[k] * log((double)q[k]);
  return h;
}

// view_scores_kernel's shape (the view mean first, then the rows a second time), with the `reps` rows of a point being
// the passes of one view under different masks: bald = H(m) - (1 / reps) sum_v H(p_v), ment = that mean entropy.
// prob, pred and agree as in view_scores_kernel.
//
// Two sums are taken more exactly than a chain of rounded adds, so that passes that agree score exactly 0 whatever their
// number (five or more equal addends do not sum exactly in a chain):
//  * the m of H(m) is the f32 nearest to the mean of the rows -- their f64 sum in pass order (exact for equal rows, and
//    within 2^-53 of exact otherwise) over reps, rounded once.  prob stays view_mean_softmax_kernel's f32 chain, byte
//    for byte; the two differ by at most a unit in the last place of an f32.
//  * S = sum_v H(p_v) in pass order keeps the rounding error of every add (Knuth's two-sum) and adds their sum at the end.
__global__ void __launch_bounds__(256) mc_scores_kernel(const float* __restrict__ logits,
                                                        const int64_t* __restrict__ inverse, int reps, int64_t p, int c,
                                                        float* __restrict__ prob, int64_t* __restrict__ pred,
                                                        double* __restrict__ bald, float* __restrict__ ment,
                                                        int* __restrict__ agree) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p) return;
  float m[kMaxClasses];
  double md[kMaxClasses];
#pragma unroll
  for (int j = 0; j < kMaxClasses; ++j) { m[j] = 0.f; md[j] = 0.0; }
  for (int v = 0; v < reps; ++v) {
    float x[kMaxClasses], mx, s;
    row_exp<float>(logits + inverse[(int64_t)v * p + i] * c, c, x, mx, s);
#pragma unroll
    for (int j = 0; j < kMaxClasses; ++j)
      if (j < c) {
        const float q = x[j] / s;
        m[j] = (v == 0) ? q : __fadd_rn(m[j], q);
        md[j] = md[j] + (double)q;
      }
  }
  float best = -INFINITY;
  int arg = 0;
  const float inv = (float)reps;
#pragma unroll
  for (int j = 0; j < kMaxClasses; ++j)
    if (j < c) {
      const float mean = m[j] / inv;
      prob[i * c + j] = mean;
      if (mean > best) { best = mean; arg = j; }
      m[j] = (float)(md[j] / (double)reps);
    }
  pred[i] = arg;
  double S = 0.0, S_err = 0.0;
  int votes = 0;
  for (int v = 0; v < reps; ++v) {
    float x[kMaxClasses], mx, s;
    votes += (row_exp<float>(logits + inverse[(int64_t)v * p + i] * c, c, x, mx, s) == arg) ? 1 : 0;
#pragma unroll
    for (int k = 0; k < kMaxClasses; ++k)
      if (k < c) x[k] = x[k] / s;
    const double h = entropy_f64(x, c);
    const double t = S + h, hh = t - S;
    S_err += (S - (t - hh)) + (h - hh);
    S = t;
  }
  const double mean = (S + S_err) / (double)reps;
  bald[i] = entropy_f64(m, c) - mean;
  ment[i] = (float)mean;
  agree[i] = votes;
}

// ---------------- confusion matrix of evaluate.py:100-109 + utils/iou_sk.py:14-19 ----------------
// per point: voxel row through the inverse index, argmax over the c logits (first maximum, as
// torch.max / np.argmax), and conf[pred * c + gt] += 1 for labelled points (gt < 100).  Integer
// counts: per-workgroup LDS histogram, then global integer atomics (order independent, exact).
__global__ void __launch_bounds__(256) confusion_kernel(const float* __restrict__ logits,
                                                        const int64_t* __restrict__ inverse,
                                                        const int64_t* __restrict__ labels,
                                                        int64_t p, int c, int* __restrict__ conf) {
  __shared__ int hist[kMaxClasses * kMaxClasses];
  for (int i = threadIdx.x; i < c * c; i += 256) hist[i] = 0;
  __syncthreads();
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < p) {
    const int64_t gt = labels[i];
    if (gt >= 0 && gt < 100 && gt < c) {
      const float* row = logits + inverse[i] * c;
      float best = row[0];
      int arg = 0;
      for (int j = 1; j < c; ++j) {
        float v = row[j];
        if (v > best) { best = v; arg = j; }
      }
      atomicAdd(&hist[arg * c + (int)gt], 1);
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < c * c; j += 256)
    if (hist[j]) atomicAdd(&conf[j], hist[j]);
}

// ---------------- world-frame registration (dataset/prepare_kdtree_sk.py:76-80) ----------------
// world[p][j] = ((h0*P[j][0] + h1*P[j][1]) + h2*P[j][2]) + 1*P[j][3] with h = (f64)point: the
// reference's np.sum(expand_dims(hcoords, 2) * pose.T, axis=1), products rounded individually.
__global__ void __launch_bounds__(256) register_kernel(const float* __restrict__ pts, int64_t p,
                                                       const double* __restrict__ pose,
                                                       double* __restrict__ world) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p) return;
  const double h0 = (double)pts[i * 3 + 0], h1 = (double)pts[i * 3 + 1], h2 = (double)pts[i * 3 + 2];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    double v = __dadd_rn(__dmul_rn(h0, pose[j * 4 + 0]), __dmul_rn(h1, pose[j * 4 + 1]));
    v = __dadd_rn(v, __dmul_rn(h2, pose[j * 4 + 2]));
    world[i * 3 + j] = __dadd_rn(v, pose[j * 4 + 3]);
  }
}

// ---------------- uniform grid for radius-limited nearest neighbour ----------------
static inline int64_t grid_cap(int64_t p) { return table_capacity(p); }

__global__ void __launch_bounds__(256) grid_keys_kernel(const double* __restrict__ pts, int64_t p,
                                                        double cell, uint64_t* __restrict__ keys,
                                                        int* __restrict__ idx, GridHeader* __restrict__ hdr) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p) return;
  if (i == 0) { hdr->p = p; hdr->cap = 0; hdr->cell = cell; hdr->inv_cell_unused = 0.; }     // the queries read the cell size
  // (a coordinate that is NaN, +-Inf or beyond 2^20 cells goes to the parking cell of its axis: grid.h)
  keys[i] = cell_key(cell_index(pts[i * 3 + 0], cell), cell_index(pts[i * 3 + 1], cell), cell_index(pts[i * 3 + 2], cell));
  idx[i] = (int)i;
}

__global__ void __launch_bounds__(256) grid_heads_kernel(const uint64_t* __restrict__ skeys,
                                                         int64_t p, TableView t, const double* __restrict__ pts,
                                                         const int* __restrict__ sidx, GridRec* __restrict__ rec) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p) return;
  {                     // the point itself, into cell order
    const int64_t j = sidx[i];
    GridRec r;
    r.key = skeys[i]; r.x = pts[j * 3 + 0]; r.y = pts[j * 3 + 1]; r.z = pts[j * 3 + 2]; r.idx = (int)j; r.pad = 0;
    rec[i] = r;
  }
  uint64_t key = skeys[i];
  if (i > 0 && skeys[i - 1] == key) return;
  const uint64_t mixed = mix_key(key);
  uint64_t s = mixed & t.mask;
  if (t.bits != nullptr) {
    const uint64_t b = bit_of(mixed, t.mask);
    atomicOr(&t.bits[b >> 5], 1u << (b & 31));
  }
  while (true) {       // cell keys are unique among heads
    unsigned long long prev = atomicCAS(&t.keys[s], (unsigned long long)kEmptyKey,
                                        (unsigned long long)key);
    if (prev == kEmptyKey) { t.vals[s] = (int)i; break; }
    s = (s + 1) & t.mask;
  }
}

// (the radius-limited nearest neighbour over a grid, grid_nearest, is grid.h's: icp.hip asks the same question)
constexpr int MAXNEI = 32;
struct NeiArgs {
  const void* grid[MAXNEI];
  const double* pts[MAXNEI];
  const float* prob[MAXNEI];
  int64_t p[MAXNEI];
  int64_t cap[MAXNEI];
  int n;
};

__device__ __forceinline__ GridView nei_grid(const NeiArgs& nei, int n, double cell) {
  return grid_view(nei.grid[n], nei.p[n], nei.cap[n], cell);
}

// Stage 1: one thread per (neighbour frame, query point): the nearest point of that frame within
// the match radius, or -1.  The 24 (or 10) look-ups of a query point are independent, so they run
// as p * n_nei threads instead of one serial chain of 27 * n_nei hash probes per point.
// q_order (round 6): the query frame's point ids in CELL order (the sorted ids of its own grid), or NULL.  Thread t then
// takes point q_order[t]: the 64 queries of a wave sit in a handful of neighbouring cells, so their bitmap words, slots and
// candidate records are the SAME few cache lines (2-3 points share a cell, neighbouring cells share half of the eight cells
// they probe) instead of ~20 random 64-byte sectors per query in scan order.  match[] is kept in thread order; stage 2
// walks the same order.  Same per-point arithmetic: same results bit for bit.
__global__ void __launch_bounds__(256)
interframe_match_kernel(const double* __restrict__ q_pts, int64_t p, NeiArgs nei, double dis_thresh,
                        int* __restrict__ match /*[n_nei][p]*/, const int* __restrict__ q_order) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int n = blockIdx.y;
  if (t >= p) return;
  if (nei.p[n] <= 0) { match[(int64_t)n * p + t] = -1; return; }
  const int64_t i = q_order != nullptr ? (int64_t)q_order[t] : t;
  const double qx = q_pts[i * 3 + 0], qy = q_pts[i * 3 + 1], qz = q_pts[i * 3 + 2];
  const GridView g = nei_grid(nei, n, reinterpret_cast<const GridHeader*>(nei.grid[n])->cell);
  double d2;
  int j = grid_nearest(g, nei.pts[n], qx, qy, qz, dis_thresh, &d2);
  if (j >= 0 && !(sqrt(d2) <= dis_thresh)) j = -1;
  match[(int64_t)n * p + t] = j;
}

// Stage 2: one thread per query point walks its matches in the reference's neighbour order and
// accumulates with numpy's widths and summation orders.
__global__ void __launch_bounds__(256)
interframe_kernel(const float* __restrict__ q_prob, int64_t p, int c, NeiArgs nei,
                  const int* __restrict__ match, double* __restrict__ interd,
                  float* __restrict__ intere, int* __restrict__ map_count, const int* __restrict__ q_order) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= p) return;
  const int64_t i = q_order != nullptr ? (int64_t)q_order[t] : t;       // (match[] is in thread order)
  float q[kMaxClasses], sum[kMaxClasses];
#pragma unroll
  for (int j = 0; j < kMaxClasses; ++j) {
    q[j] = (j < c) ? q_prob[i * c + j] : 0.f;
    sum[j] = q[j];
  }
  const float eps = 0.00001f;
  double div = 0.0;
  int cnt = 0;
  for (int n = 0; n < nei.n; ++n) {
    const int j = match[(int64_t)n * p + t];
    if (j < 0) continue;
    const float* np = nei.prob[n] + (int64_t)j * c;
    float term[kMaxClasses];
#pragma unroll
    for (int k = 0; k < kMaxClasses; ++k)
      if (k < c) {
        float nv = np[k];
        sum[k] = __fadd_rn(sum[k], nv);
        double x = (double)__fadd_rn(q[k], eps), y = (double)__fadd_rn(nv, eps);
        // scipy.special.kl_div(x, y) = x log(x/y) - x + y  (x, y > 0 here), f32 result
        term[k] = (float)(x * log(x / y) - x + y);
      }
    div += (double)np_sum_f32(term, c);
    cnt += 1;
  }
  // sum_prob /= map_count (f64 divide, f32 store); entropy = scipy.stats.entropy(sum_prob)
  float pk[kMaxClasses];
  const double mc = (double)(cnt + 1);
#pragma unroll
  for (int k = 0; k < kMaxClasses; ++k)
    if (k < c) pk[k] = (float)((double)sum[k] / mc);
  float tot = np_sum_f32(pk, c);
  float ent[kMaxClasses];
#pragma unroll
  for (int k = 0; k < kMaxClasses; ++k)
    if (k < c) {
      float v = pk[k] / tot;
      ent[k] = (v > 0.f) ? (float)(-(double)v * log((double)v)) : 0.f;
    }
  intere[i] = np_sum_f32(ent, c);
  interd[i] = (cnt > 0) ? div / (double)cnt : div;
  map_count[i] = cnt;
}

// ---------------- per-supervoxel means ----------------
__global__ void __launch_bounds__(256)
supervoxel_reduce_kernel(const double* __restrict__ interd, const float* __restrict__ intere,
                         const double* __restrict__ pts, const int64_t* __restrict__ sv_ptr,
                         const int64_t* __restrict__ sv_idx, float* __restrict__ sv_interd,
                         float* __restrict__ sv_intere, float* __restrict__ sv_center) {
  __shared__ double red[5][256];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int64_t beg = sv_ptr[s], end = sv_ptr[s + 1];
  double a[5] = {0, 0, 0, 0, 0};
  for (int64_t t = beg + tid; t < end; t += 256) {
    int64_t i = sv_idx[t];
    a[0] += interd[i];
    a[1] += (double)intere[i];
    a[2] += pts[i * 3 + 0];
    a[3] += pts[i * 3 + 1];
    a[4] += pts[i * 3 + 2];
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) red[k][tid] = a[k];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w)
#pragma unroll
      for (int k = 0; k < 5; ++k) red[k][tid] += red[k][tid + w];
    __syncthreads();
  }
  if (tid == 0) {
    double n = (double)(end - beg);
    sv_interd[s] = (float)(red[0][0] / n);
    sv_intere[s] = (float)(red[1][0] / n);
    sv_center[s * 3 + 0] = (float)(red[2][0] / n);
    sv_center[s * 3 + 1] = (float)(red[3][0] / n);
    sv_center[s * 3 + 2] = (float)(red[4][0] / n);
  }
}

// The one layout of lidal_nn_grid_build's scratch: it sizes with a NULL address and carves with a real one (common.h
// Carver; the members are the regions in order).
struct GridBuildWs { uint64_t* keys; int* idx; char* sort_tmp; int64_t sort_tmp_bytes, total; };
GridBuildWs grid_build_layout(int64_t p, void* ws) {
  const int64_t q = p > 0 ? p : 1, tmp = radix_sort_ws_bytes(q, 8, true);
  Carver c(ws);
  return {c.take<uint64_t>(q), c.take<int>(q), c.take(tmp), tmp, c.total()};
}

}  // namespace

extern "C" int lidal_view_mean_softmax(const float* logits, const int64_t* inverse, int reps,
                                       int64_t p, int c, float* prob, int64_t* pred,
                                       void* stream) {
  LIDAL_REQUIRE(c > 0 && c <= kMaxClasses, "view_mean_softmax: classes must be in 1..%d", kMaxClasses);
  LIDAL_REQUIRE(reps > 0, "view_mean_softmax: reps must be positive");
  if (p == 0) return 0;
  view_mean_softmax_kernel<<<(unsigned)cdiv(p, 256), 256, 0, (hipStream_t)stream>>>(
      logits, inverse, reps, p, c, prob, pred);
  LIDAL_CHECK_LAUNCH("lidal_view_mean_softmax");
  return 0;
}

extern "C" int lidal_view_scores(const float* logits, const int64_t* inverse, int reps, int64_t p, int c,
                                 float* prob, int64_t* pred, double* viewd, float* viewe, int32_t* agree,
                                 void* stream) {
  LIDAL_REQUIRE(c > 0 && c <= kMaxClasses, "view_scores: classes must be in 1..%d", kMaxClasses);
  LIDAL_REQUIRE(reps > 0, "view_scores: reps must be positive");
  if (p == 0) return 0;
  view_scores_kernel<<<(unsigned)cdiv(p, 256), 256, 0, (hipStream_t)stream>>>(
      logits, inverse, reps, p, c, prob, pred, viewd, viewe, agree);
  LIDAL_CHECK_LAUNCH("lidal_view_scores");
  return 0;
}

extern "C" int lidal_mc_scores(const float* logits, const int64_t* inverse, int reps, int64_t p, int c, float* prob,
                               int64_t* pred, double* bald, float* ment, int32_t* agree, void* stream) {
  LIDAL_REQUIRE(c > 0 && c <= kMaxClasses, "mc_scores: classes must be in 1..%d", kMaxClasses);
  LIDAL_REQUIRE(reps > 0, "mc_scores: reps must be positive");
  if (p == 0) return 0;
  mc_scores_kernel<<<(unsigned)cdiv(p, 256), 256, 0, (hipStream_t)stream>>>(
      logits, inverse, reps, p, c, prob, pred, bald, ment, agree);
  LIDAL_CHECK_LAUNCH("lidal_mc_scores");
  return 0;
}

extern "C" int64_t lidal_nn_grid_bytes(int64_t p) {
  int64_t q = p > 0 ? p : 1;
  return 64 + grid_off_bits(grid_cap(q), q) + grid_cap(q);
}

extern "C" int64_t lidal_nn_grid_workspace_bytes(int64_t p) { return grid_build_layout(p, nullptr).total; }

extern "C" int lidal_nn_grid_build(const double* pts, int64_t p, double cell, void* grid,
                                   int64_t grid_bytes, void* ws, int64_t ws_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  LIDAL_REQUIRE(cell > 0, "nn_grid_build: cell must be positive");
  LIDAL_REQUIRE(grid_bytes >= lidal_nn_grid_bytes(p), "nn grid buffer too small");
  const GridBuildWs w = grid_build_layout(p, ws);
  LIDAL_REQUIRE(ws_bytes >= w.total, "nn grid workspace too small");
  int64_t q = p > 0 ? p : 1;
  int64_t cap = grid_cap(q);
  char* base = (char*)grid + 64;
  LIDAL_HIP(hipMemsetAsync(base, 0xFF, cap * 8, s));
  LIDAL_HIP(hipMemsetAsync(base + cap * 8, 0xFF, cap * 4, s));
  if (p == 0) return 0;
  uint64_t* skeys = (uint64_t*)(base + grid_off_skeys(cap));
  int* sidx = (int*)(base + grid_off_sidx(cap, q));
  LIDAL_HIP(hipMemsetAsync(base + grid_off_bits(cap, q), 0, cap, s));
  grid_keys_kernel<<<(unsigned)cdiv(p, 256), 256, 0, s>>>(pts, p, cell, w.keys, w.idx, (GridHeader*)grid);
  LIDAL_CHECK_LAUNCH("grid_keys");
  if (int rc = radix_sort(w.keys, w.idx, skeys, sidx, p, 8, 63, w.sort_tmp, w.sort_tmp_bytes, s)) return rc;
  TableView t;
  t.keys = (unsigned long long*)base;
  t.vals = (int*)(base + cap * 8);
  t.mask = (uint64_t)cap - 1;
  t.bits = (unsigned*)(base + grid_off_bits(cap, q));
  t.sbits = nullptr; t.hdr = nullptr;
  grid_heads_kernel<<<(unsigned)cdiv(p, 256), 256, 0, s>>>(skeys, p, t, pts, sidx, (GridRec*)(base + grid_off_spts(cap, q)));
  LIDAL_CHECK_LAUNCH("grid_heads");
  return 0;
}

extern "C" int64_t lidal_interframe_workspace_bytes(int64_t p, int n_nei) {
  return (int64_t)(n_nei > 0 ? n_nei : 1) * (p > 0 ? p : 1) * 4 + 256;
}

// the neighbour frames of a query frame as the kernels take them (nei_prob_host NULL: the match stage reads none)
static NeiArgs nei_args(const void* const* nei_grids_host, const double* const* nei_pts_host,
                        const float* const* nei_prob_host, const int64_t* nei_p_host, int n_nei) {
  NeiArgs a;
  memset(&a, 0, sizeof(a));
  a.n = n_nei;
  for (int n = 0; n < n_nei; ++n) {
    a.grid[n] = nei_grids_host[n];
    a.pts[n] = nei_pts_host[n];
    a.prob[n] = nei_prob_host != nullptr ? nei_prob_host[n] : nullptr;
    a.p[n] = nei_p_host[n];
    a.cap[n] = grid_cap(nei_p_host[n] > 0 ? nei_p_host[n] : 1);
  }
  return a;
}

static int interframe_score(const double* q_pts, const float* q_prob, int64_t p, int c,
                            const void* const* nei_grids_host, const double* const* nei_pts_host,
                            const float* const* nei_prob_host, const int64_t* nei_p_host,
                            int n_nei, double dis_thresh, double* interd, float* intere,
                            int32_t* map_count, void* ws, int64_t ws_bytes, const void* q_grid,
                            void* stream) {
  LIDAL_REQUIRE(c > 0 && c <= kMaxClasses, "interframe_score: classes must be in 1..%d", kMaxClasses);
  LIDAL_REQUIRE(n_nei >= 0 && n_nei <= MAXNEI, "interframe_score: at most %d neighbours", MAXNEI);
  if (p == 0) return 0;
  LIDAL_REQUIRE(ws_bytes >= lidal_interframe_workspace_bytes(p, n_nei), "interframe workspace too small");
  int* match = (int*)ws;
  const NeiArgs a = nei_args(nei_grids_host, nei_pts_host, nei_prob_host, nei_p_host, n_nei);
  hipStream_t s = (hipStream_t)stream;
  // the query frame's points in cell order: the sorted ids inside its own grid buffer (lidal_nn_grid_build of q_pts)
  const int* q_order = nullptr;
  if (q_grid != nullptr) {
    const int64_t cap = grid_cap(p);
    q_order = (const int*)((const char*)q_grid + 64 + grid_off_sidx(cap, p));
  }
  if (n_nei > 0) {
    interframe_match_kernel<<<dim3((unsigned)cdiv(p, 256), (unsigned)n_nei), 256, 0, s>>>(
        q_pts, p, a, dis_thresh, match, q_order);
    LIDAL_CHECK_LAUNCH("interframe_match");
  }
  interframe_kernel<<<(unsigned)cdiv(p, 256), 256, 0, s>>>(q_prob, p, c, a, match, interd, intere,
                                                           map_count, q_order);
  LIDAL_CHECK_LAUNCH("lidal_interframe_score");
  return 0;
}

// Stage 1 alone: the match table of lidal_interframe_score, kept by the caller.
extern "C" int lidal_interframe_match(const double* q_pts, int64_t p, const void* const* nei_grids_host,
                                      const double* const* nei_pts_host, const int64_t* nei_p_host, int n_nei,
                                      double dis_thresh, int32_t* match, void* stream) {
  LIDAL_REQUIRE(n_nei >= 0 && n_nei <= MAXNEI, "interframe_match: at most %d neighbours", MAXNEI);
  LIDAL_REQUIRE(p >= 0, "interframe_match: p must not be negative");
  if (p == 0 || n_nei == 0) return 0;
  LIDAL_REQUIRE(q_pts != nullptr && match != nullptr && nei_grids_host != nullptr && nei_pts_host != nullptr &&
                    nei_p_host != nullptr, "interframe_match: a NULL argument");
  for (int n = 0; n < n_nei; ++n)
    LIDAL_REQUIRE(nei_p_host[n] <= 0 || (nei_grids_host[n] != nullptr && nei_pts_host[n] != nullptr),
                  "interframe_match: neighbour %d has points but no grid", n);
  const NeiArgs a = nei_args(nei_grids_host, nei_pts_host, nullptr, nei_p_host, n_nei);
  interframe_match_kernel<<<dim3((unsigned)cdiv(p, 256), (unsigned)n_nei), 256, 0, (hipStream_t)stream>>>(
      q_pts, p, a, dis_thresh, match, nullptr);
  LIDAL_CHECK_LAUNCH("lidal_interframe_match");
  return 0;
}

extern "C" int lidal_interframe_score(const double* q_pts, const float* q_prob, int64_t p, int c,
                                      const void* const* nei_grids_host,
                                      const double* const* nei_pts_host,
                                      const float* const* nei_prob_host, const int64_t* nei_p_host,
                                      int n_nei, double dis_thresh, double* interd, float* intere,
                                      int32_t* map_count, void* ws, int64_t ws_bytes,
                                      void* stream) {
  return interframe_score(q_pts, q_prob, p, c, nei_grids_host, nei_pts_host, nei_prob_host, nei_p_host, n_nei, dis_thresh,
                          interd, intere, map_count, ws, ws_bytes, nullptr, stream);
}

extern "C" int lidal_interframe_score_ordered(const double* q_pts, const float* q_prob, int64_t p, int c,
                                              const void* const* nei_grids_host,
                                              const double* const* nei_pts_host,
                                              const float* const* nei_prob_host, const int64_t* nei_p_host,
                                              int n_nei, double dis_thresh, double* interd, float* intere,
                                              int32_t* map_count, void* ws, int64_t ws_bytes,
                                              const void* q_grid, void* stream) {
  return interframe_score(q_pts, q_prob, p, c, nei_grids_host, nei_pts_host, nei_prob_host, nei_p_host, n_nei, dis_thresh,
                          interd, intere, map_count, ws, ws_bytes, q_grid, stream);
}

extern "C" int lidal_supervoxel_reduce(const double* interd, const float* intere,
                                       const double* pts, const int64_t* sv_ptr,
                                       const int64_t* sv_idx, int s, float* sv_interd,
                                       float* sv_intere, float* sv_center, void* stream) {
  if (s == 0) return 0;
  supervoxel_reduce_kernel<<<(unsigned)s, 256, 0, (hipStream_t)stream>>>(
      interd, intere, pts, sv_ptr, sv_idx, sv_interd, sv_intere, sv_center);
  LIDAL_CHECK_LAUNCH("lidal_supervoxel_reduce");
  return 0;
}

extern "C" int lidal_register_points(const float* points, int64_t p, const double* pose_dev,
                                     double* world, void* stream) {
  if (p == 0) return 0;
  register_kernel<<<(unsigned)cdiv(p, 256), 256, 0, (hipStream_t)stream>>>(points, p, pose_dev, world);
  LIDAL_CHECK_LAUNCH("lidal_register_points");
  return 0;
}

extern "C" int lidal_confusion_accumulate(const float* logits, const int64_t* inverse,
                                          const int64_t* labels, int64_t p, int c, int32_t* conf,
                                          void* stream) {
  LIDAL_REQUIRE(c > 0 && c <= kMaxClasses, "confusion: classes must be in 1..%d", kMaxClasses);
  if (p == 0) return 0;
  confusion_kernel<<<(unsigned)cdiv(p, 256), 256, 0, (hipStream_t)stream>>>(logits, inverse, labels,
                                                                            p, c, conf);
  LIDAL_CHECK_LAUNCH("lidal_confusion_accumulate");
  return 0;
}
