// ReDAL region selection (score/sv_level/ReDAL.py and dataset/ReDAL/gen_surface_variation_sk.py of the reference) for
// gfx950: the k-nearest-neighbour surface variation of a raw scan and the per-supervoxel information scores and mean
// features.  (The k-means that replaces sklearn.cluster.KMeans in the diversity-aware selection is kmeans.hip.)
//
// Every reduction runs in a fixed order and restates numpy where the result is pinned by a numpy restatement
// (DESIGN.md section 8); this unit is built with -ffp-contract=off (lidal_amd/build.py) so that a*b+c stays two
// roundings.  No float atomics anywhere.
#include <cmath>

#include "common.h"
#include "grid.h"
#include "npsum.h"
#include "sym3.h"

using namespace lidal;
using namespace lidal::grid;
using namespace lidal::npsum;
using namespace lidal::sym3;

extern "C" int64_t lidal_nn_grid_bytes(int64_t p);
extern "C" int64_t lidal_nn_grid_workspace_bytes(int64_t p);
extern "C" int lidal_nn_grid_build(const double* pts, int64_t p, double cell, void* grid, int64_t grid_bytes, void* ws,
                                   int64_t ws_bytes, void* stream);

namespace {

// ================================ k nearest neighbours / surface variation ================================
constexpr int KNN_BLOCK = 64;     // one wave per workgroup: the top-k lists of its 64 queries live in LDS
constexpr int KNN_KMAX = 64;

__global__ void __launch_bounds__(256) knn_prep_kernel(const float* __restrict__ xyz, int64_t p, double cell,
                                                       double* __restrict__ pts, int* __restrict__ bounds) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p) return;
  int c[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double v = (double)xyz[i * 3 + a];
    pts[i * 3 + a] = v;
    c[a] = (int)floor(v / cell);
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    atomicMin(&bounds[a], c[a]);          // integer atomics: the cell box of the scan, exact in any order
    atomicMax(&bounds[3 + a], c[a]);
  }
}

__global__ void knn_bounds_init_kernel(int* __restrict__ bounds) {
  const int t = threadIdx.x;
  if (t < 6) bounds[t] = t < 3 ? 0x7FFFFFFF : (int)0x80000000;
}

struct KnnGrid {
  TableView t;
  const GridRec* rec;
  int64_t p;
  double cell;
};

// (d, j) precedes (e, l): nearer, or as near with the lower index
__device__ __forceinline__ bool knn_before(double d, int j, double e, int l) { return d < e || (d == e && j < l); }

// Squared distance from q to the cell box [c * cell, (c + 1) * cell) along one axis, shrunk by a margin that covers the
// rounding of floor(x / cell): a cell is skipped only if none of its points can be nearer.
__device__ __forceinline__ double axis_gap(double q, int64_t c, double cell) {
  const double lo = (double)c * cell, hi = (double)(c + 1) * cell;
  const double margin = 1e-9 * (fabs(q) + cell);
  double g = 0.0;
  if (q < lo) g = lo - q - margin;
  else if (q > hi) g = q - hi - margin;
  return g > 0.0 ? g : 0.0;
}

// One query: the k nearest other points, sorted by (distance, index).  The list is kept in LDS, [slot][lane]
// (dynamic shared memory: k * 64 * 12 bytes), so that no runtime-indexed per-thread array goes to scratch.
// The cells are visited ring by ring (Chebyshev distance R from the query's cell); the search stops once the k-th
// best distance is smaller than the distance from the query to the faces of the visited cube (no unvisited point can
// be nearer) or when the cube covers the scan's cell box.  Inside a ring a cell whose box is farther than the k-th
// best is skipped.
template <bool SIGMA>
__global__ void __launch_bounds__(KNN_BLOCK)
knn_kernel(KnnGrid g, const double* __restrict__ pts, int k, const int* __restrict__ bounds, int* __restrict__ knn_out,
           float* __restrict__ sigma_out, float threshold) {
  extern __shared__ unsigned char knn_smem[];
  double* ld = reinterpret_cast<double*>(knn_smem);                            // [k][64]
  int* li = reinterpret_cast<int*>(knn_smem + (size_t)k * KNN_BLOCK * 8);      // [k][64]
  const int lane = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * KNN_BLOCK + lane;
  if (i >= g.p) return;                // (no barrier below: every lane works in its own LDS column)
  const double qx = pts[i * 3 + 0], qy = pts[i * 3 + 1], qz = pts[i * 3 + 2];
  const double cell = g.cell;
  const int64_t cx = (int64_t)floor(qx / cell), cy = (int64_t)floor(qy / cell), cz = (int64_t)floor(qz / cell);
  const int64_t bx0 = bounds[0], by0 = bounds[1], bz0 = bounds[2], bx1 = bounds[3], by1 = bounds[4], bz1 = bounds[5];
  int cnt = 0;
  double worst = INFINITY;
  int worst_j = 0x7FFFFFFF;
  for (int64_t R = 0;; ++R) {
    for (int64_t ix = cx - R; ix <= cx + R; ++ix) {
      if (ix < bx0 || ix > bx1) continue;
      const double gx = axis_gap(qx, ix, cell);
      for (int64_t iy = cy - R; iy <= cy + R; ++iy) {
        if (iy < by0 || iy > by1) continue;
        const double gy = axis_gap(qy, iy, cell);
        const bool shell = (ix == cx - R || ix == cx + R || iy == cy - R || iy == cy + R);
        const int64_t step = shell ? 1 : (R > 0 ? 2 * R : 1);     // inside the ring's x/y shell: only z = cz +- R
        for (int64_t iz = cz - R; iz <= cz + R; iz += step) {
          if (iz < bz0 || iz > bz1) continue;
          if (cnt == k) {
            const double gz = axis_gap(qz, iz, cell);
            const double box = __dadd_rn(__dadd_rn(__dmul_rn(gx, gx), __dmul_rn(gy, gy)), __dmul_rn(gz, gz));
            if (box > worst) continue;
          }
          const uint64_t key = cell_key(ix, iy, iz);
          if (g.t.bits != nullptr) {
            const uint64_t b = bit_of(mix_key(key), g.t.mask);
            if (!((g.t.bits[b >> 5] >> (b & 31)) & 1u)) continue;
          }
          const int start = table_lookup(g.t, key);
          if (start < 0) continue;
          for (int64_t s = start; s < g.p; ++s) {
            const GridRec r = g.rec[s];
            if (r.key != key) break;
            const int j = r.idx;
            if (j == (int)i) continue;
            const double ex = r.x - qx, ey = r.y - qy, ez = r.z - qz;
            const double d2 = __dadd_rn(__dadd_rn(__dmul_rn(ex, ex), __dmul_rn(ey, ey)), __dmul_rn(ez, ez));
            if (cnt == k && !knn_before(d2, j, worst, worst_j)) continue;
            int pos = cnt < k ? cnt++ : k - 1;
            while (pos > 0) {
              const double pd = ld[(pos - 1) * KNN_BLOCK + lane];
              const int pj = li[(pos - 1) * KNN_BLOCK + lane];
              if (!knn_before(d2, j, pd, pj)) break;
              ld[pos * KNN_BLOCK + lane] = pd;
              li[pos * KNN_BLOCK + lane] = pj;
              --pos;
            }
            ld[pos * KNN_BLOCK + lane] = d2;
            li[pos * KNN_BLOCK + lane] = j;
            if (cnt == k) {
              worst = ld[(k - 1) * KNN_BLOCK + lane];
              worst_j = li[(k - 1) * KNN_BLOCK + lane];
            }
          }
        }
      }
    }
    if (cx - R <= bx0 && cx + R >= bx1 && cy - R <= by0 && cy + R >= by1 && cz - R <= bz0 && cz + R >= bz1) break;
    if (cnt == k) {
      // distance from q to the nearest face of the visited cube [c - R, c + R + 1) * cell, less the rounding margin
      double m = INFINITY;
      const double q3[3] = {qx, qy, qz};
      const int64_t c3[3] = {cx, cy, cz};
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const double lo = (double)(c3[a] - R) * cell, hi = (double)(c3[a] + R + 1) * cell;
        m = fmin(m, fmin(q3[a] - lo, hi - q3[a]));
      }
      m -= 1e-9 * (fabs(qx) + fabs(qy) + fabs(qz) + cell);
      if (m > 0.0 && worst < __dmul_rn(m, m)) break;
    }
  }
  if (knn_out != nullptr)
    for (int s = 0; s < k; ++s) knn_out[i * k + s] = li[s * KNN_BLOCK + lane];
  if (!SIGMA) return;
  // population covariance of the k neighbours (f64, neighbour order), eigenvalues by cyclic Jacobi (sym3.h)
  double a[3][3], none[3][3];
  covariance3([&](auto visit) {
    for (int s = 0; s < k; ++s) {
      const int64_t j = li[s * KNN_BLOCK + lane];
      visit(pts[j * 3 + 0], pts[j * 3 + 1], pts[j * 3 + 2]);
    }
  }, k, a);
  jacobi3<false>(a, none);
  const double l0 = a[0][0], l1 = a[1][1], l2 = a[2][2];
  const double lmin = fmin(l0, fmin(l1, l2));
  float sigma = (float)(lmin / (l0 + l1 + l2));
  if (sigma > threshold) sigma = threshold;     // NaN (k identical points) passes, as in the reference
  sigma_out[i] = sigma;
}

// ================================ region scores (ReDAL.py worker_func) ================================
// per point: uncertain = mean_c(-p * log2(p + 1e-12)) (f32 terms, pairwise class sum, divided by C), then
// point_score = alpha * uncertain + gamma * curvature (ReDAL.py:59-63).  log2 is taken in f64 and rounded (numpy's f32
// log2 may dispatch to a SIMD routine that differs in the last bit: the one step not restated).
__global__ void __launch_bounds__(256) point_score_kernel(const float* __restrict__ prob, int64_t p, int c,
                                                          const float* __restrict__ curv, float alpha, float gamma,
                                                          float* __restrict__ score) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p) return;
  float term[kMaxClasses];
#pragma unroll
  for (int j = 0; j < kMaxClasses; ++j)
    if (j < c) {
      const float pj = prob[i * c + j];
      const float l = (float)log2((double)__fadd_rn(pj, 1e-12f));
      term[j] = __fmul_rn(-pj, l);
    }
  const float u = __fdiv_rn(np_sum_f32(term, c), (float)c);
  score[i] = __fadd_rn(__fmul_rn(alpha, u), __fmul_rn(gamma, curv[i]));
}

// one workgroup per supervoxel: score = point_score[p_ids].mean() (np_mean_f32, lane 0), feats = outfeat[p_ids].mean(0),
// pnum = len(p_ids).  numpy reduces the rows of an [n, d >= 2] array one after the other, so the feature mean is a
// sequential f32 sum over the rows, one lane per feature; an [n, 1] array is reduced as a contiguous one (np_mean_f32).
constexpr int REG_BLOCK = 128;
__global__ void __launch_bounds__(REG_BLOCK)
region_reduce_kernel(const float* __restrict__ score, const float* __restrict__ feat, int d,
                     const int64_t* __restrict__ sv_ptr, const int64_t* __restrict__ sv_idx,
                     float* __restrict__ sv_scores, float* __restrict__ sv_feats, int64_t* __restrict__ sv_pnums) {
  __shared__ int64_t st_off[64], st_n[64];
  __shared__ int st_phase[64];
  __shared__ float st_val[64];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int64_t beg = sv_ptr[s], end = sv_ptr[s + 1], n = end - beg;
  const float fn = (float)n;
  if (d > 1)
    for (int f = tid; f < d; f += REG_BLOCK) {
      float acc = 0.f;
      for (int64_t t = beg; t < end; ++t) acc = __fadd_rn(acc, feat[sv_idx[t] * d + f]);
      sv_feats[(int64_t)s * d + f] = __fdiv_rn(acc, fn);
    }
  if (tid != 0) return;
  sv_pnums[s] = n;
  if (d == 1)
    sv_feats[s] = np_mean_f32([&](int64_t t) { return feat[sv_idx[beg + t]]; }, n, st_off, st_n, st_phase, st_val);
  sv_scores[s] = np_mean_f32([&](int64_t t) { return score[sv_idx[beg + t]]; }, n, st_off, st_n, st_phase, st_val);
}

// Workspace layouts: one function per builder sizes its scratch (NULL address) and carves it (common.h Carver; the
// members are the regions in order).

// k-NN: the points as f64, the cell bounds of the scan, the search grid and the scratch of its build
struct KnnWs { double* pts; int* bounds; char *grid, *grid_ws; int64_t grid_bytes, grid_ws_bytes, total; };
KnnWs knn_layout(int64_t p, void* ws) {
  const int64_t q = p > 0 ? p : 1, gb = lidal_nn_grid_bytes(q), gwb = lidal_nn_grid_workspace_bytes(q);
  Carver c(ws);
  return {c.take<double>(3 * q), c.take<int>(6), c.take(gb), c.take(gwb), gb, gwb, c.total()};
}

}  // namespace

// ---------------------------------------------------------------- k-NN / surface variation
extern "C" int64_t lidal_knn_workspace_bytes(int64_t p) { return knn_layout(p, nullptr).total; }

static int knn_run(const float* xyz, int64_t p, int k, double cell, int32_t* knn, float* sigma, float threshold, void* ws,
                   int64_t ws_bytes, void* stream) {
  LIDAL_REQUIRE(k >= 1 && k <= KNN_KMAX, "knn: k must be in 1..%d", KNN_KMAX);
  LIDAL_REQUIRE(p >= (int64_t)k + 1, "knn: %lld points cannot have %d nearest other points (need at least k + 1)",
                (long long)p, k);
  LIDAL_REQUIRE(p < 0x7FFFFFFF, "knn: at most 2^31 - 1 points");
  LIDAL_REQUIRE(cell > 0, "knn: cell must be positive");
  const KnnWs w = knn_layout(p, ws);
  LIDAL_REQUIRE(ws_bytes >= w.total, "knn workspace too small");
  hipStream_t s = (hipStream_t)stream;
  double* pts = w.pts;
  int* bounds = w.bounds;
  char* grid = w.grid;
  knn_bounds_init_kernel<<<1, 64, 0, s>>>(bounds);
  LIDAL_CHECK_LAUNCH("knn_bounds_init");
  knn_prep_kernel<<<(unsigned)cdiv(p, 256), 256, 0, s>>>(xyz, p, cell, pts, bounds);
  LIDAL_CHECK_LAUNCH("knn_prep");
  if (int rc = lidal_nn_grid_build(pts, p, cell, grid, w.grid_bytes, w.grid_ws, w.grid_ws_bytes, stream)) return rc;
  KnnGrid g;
  const int64_t cap = table_capacity(p);
  char* gb = grid + 64;
  g.t.keys = (unsigned long long*)gb;
  g.t.vals = (int*)(gb + cap * 8);
  g.t.mask = (uint64_t)cap - 1;
  g.t.bits = (unsigned*)(gb + grid_off_bits(cap, p));
  g.t.sbits = nullptr;
  g.t.hdr = nullptr;
  g.rec = (const GridRec*)(gb + grid_off_spts(cap, p));
  g.p = p;
  g.cell = cell;
  const size_t lds = (size_t)k * KNN_BLOCK * 12;
  if (sigma != nullptr)
    knn_kernel<true><<<(unsigned)cdiv(p, KNN_BLOCK), KNN_BLOCK, lds, s>>>(g, pts, k, bounds, knn, sigma, threshold);
  else
    knn_kernel<false><<<(unsigned)cdiv(p, KNN_BLOCK), KNN_BLOCK, lds, s>>>(g, pts, k, bounds, knn, nullptr, threshold);
  LIDAL_CHECK_LAUNCH("knn");
  return 0;
}

extern "C" int lidal_knn(const float* xyz, int64_t p, int k, double cell, int32_t* knn, void* ws, int64_t ws_bytes,
                         void* stream) {
  return knn_run(xyz, p, k, cell, knn, nullptr, 0.f, ws, ws_bytes, stream);
}

extern "C" int lidal_surface_variation(const float* xyz, int64_t p, int k, double cell, float threshold, float* sigma,
                                       void* ws, int64_t ws_bytes, void* stream) {
  return knn_run(xyz, p, k, cell, nullptr, sigma, threshold, ws, ws_bytes, stream);
}

// ---------------------------------------------------------------- region scores
extern "C" int64_t lidal_region_scores_workspace_bytes(int64_t p) { return align_up(4 * (p > 0 ? p : 1), 256); }

extern "C" int lidal_region_scores(const float* prob, int64_t p, int c, const float* feat, int d, const float* curvature,
                                   const int64_t* sv_ptr, const int64_t* sv_idx, int s, float alpha, float gamma,
                                   float* sv_scores, float* sv_feats, int64_t* sv_pnums, void* ws, int64_t ws_bytes,
                                   void* stream) {
  LIDAL_REQUIRE(c > 0 && c <= kMaxClasses, "region_scores: classes must be in 1..%d", kMaxClasses);
  LIDAL_REQUIRE(d > 0, "region_scores: the feature width must be positive");
  LIDAL_REQUIRE(ws_bytes >= lidal_region_scores_workspace_bytes(p), "region_scores workspace too small");
  if (s == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  float* score = (float*)ws;
  if (p > 0) {
    point_score_kernel<<<(unsigned)cdiv(p, 256), 256, 0, st>>>(prob, p, c, curvature, alpha, gamma, score);
    LIDAL_CHECK_LAUNCH("region_point_score");
  }
  region_reduce_kernel<<<(unsigned)s, REG_BLOCK, 0, st>>>(score, feat, d, sv_ptr, sv_idx, sv_scores, sv_feats, sv_pnums);
  LIDAL_CHECK_LAUNCH("region_reduce");
  return 0;
}
