// ReDAL region selection (score/sv_level/ReDAL.py and dataset/ReDAL/gen_surface_variation_sk.py of the reference) for
// gfx950: the k-nearest-neighbour surface variation of a raw scan, the per-supervoxel information scores and mean
// features, and the k-means that replaces sklearn.cluster.KMeans in the diversity-aware selection.
//
// Every reduction runs in a fixed order and restates numpy where the result is pinned by a numpy restatement
// (DESIGN.md section 8); this unit is built with -ffp-contract=off (lidal_amd/build.py) so that a*b+c stays two
// roundings.  No float atomics anywhere: the k-means is deterministic run to run.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "grid.h"
#include "kmeans.h"
#include "npsum.h"

using namespace lidal;
using namespace lidal::grid;
using namespace lidal::npsum;

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
  // population covariance of the k neighbours (f64, neighbour order), eigenvalues by cyclic Jacobi
  double mx = 0.0, my = 0.0, mz = 0.0;
  for (int s = 0; s < k; ++s) {
    const int64_t j = li[s * KNN_BLOCK + lane];
    mx += pts[j * 3 + 0]; my += pts[j * 3 + 1]; mz += pts[j * 3 + 2];
  }
  const double inv = 1.0 / (double)k;
  mx *= inv; my *= inv; mz *= inv;
  double a00 = 0, a01 = 0, a02 = 0, a11 = 0, a12 = 0, a22 = 0;
  for (int s = 0; s < k; ++s) {
    const int64_t j = li[s * KNN_BLOCK + lane];
    const double dx = pts[j * 3 + 0] - mx, dy = pts[j * 3 + 1] - my, dz = pts[j * 3 + 2] - mz;
    a00 += dx * dx; a01 += dx * dy; a02 += dx * dz;
    a11 += dy * dy; a12 += dy * dz; a22 += dz * dz;
  }
  double a[3][3] = {{a00 * inv, a01 * inv, a02 * inv}, {a01 * inv, a11 * inv, a12 * inv}, {a02 * inv, a12 * inv, a22 * inv}};
  // Jacobi keeps the small eigenvalue of a nearly planar neighbourhood to ~1 ulp of the large ones (the closed
  // trigonometric form loses it to cancellation)
  auto rot = [&](int P, int Q) {
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    const int r = 3 - P - Q;
    const double arp = a[r][P], arq = a[r][Q];
    a[r][P] = a[P][r] = c * arp - s * arq;
    a[r][Q] = a[Q][r] = s * arp + c * arq;
    a[P][P] -= t * apq;
    a[Q][Q] += t * apq;
    a[P][Q] = a[Q][P] = 0.0;
  };
  for (int sweep = 0; sweep < 32; ++sweep) {
    const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]);
    const double dia = fabs(a[0][0]) + fabs(a[1][1]) + fabs(a[2][2]);
    if (!(off > 1e-300) || off <= 1e-18 * dia) break;
    rot(0, 1);
    rot(0, 2);
    rot(1, 2);
  }
  const double l0 = a[0][0], l1 = a[1][1], l2 = a[2][2];
  const double lmin = fmin(l0, fmin(l1, l2));
  float sigma = (float)(lmin / (l0 + l1 + l2));
  if (sigma > threshold) sigma = threshold;     // NaN (k identical points) passes, as in the reference
  sigma_out[i] = sigma;
}

// ================================ region scores (ReDAL.py worker_func) ================================
constexpr int MAXC = 32;

// per point: uncertain = mean_c(-p * log2(p + 1e-12)) (f32 terms, pairwise class sum, divided by C), then
// point_score = alpha * uncertain + gamma * curvature (ReDAL.py:59-63).  log2 is taken in f64 and rounded (numpy's f32
// log2 may dispatch to a SIMD routine that differs in the last bit: the one step not restated).
__global__ void __launch_bounds__(256) point_score_kernel(const float* __restrict__ prob, int64_t p, int c,
                                                          const float* __restrict__ curv, float alpha, float gamma,
                                                          float* __restrict__ score) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p) return;
  float term[MAXC];
#pragma unroll
  for (int j = 0; j < MAXC; ++j)
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

// ================================ k-means ================================
constexpr int KM_CHUNK = 256;     // the scan of D^2: sequential inside chunks of 256, then sequential over the chunks
constexpr int KM_DMAX = NP_DMAX;


__global__ void km_first_seed_kernel(int* __restrict__ seeds, int first) {
  if (threadIdx.x == 0) seeds[0] = first;
}

// closest[i] = d2(x_i, x_first)
__global__ void __launch_bounds__(256) km_first_kernel(const float* __restrict__ x, int64_t n, int d, int64_t first,
                                                       double* __restrict__ closest) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float r[KM_DMAX];
  load_row_f32(x, i, d, r);
  closest[i] = np_d2_f64(r, [&](int f) { return (double)x[first * d + f]; }, d);
}

// tot[r][c] = sequential sum of src[r][c * 256 .. ) (the last value of the chunk's inclusive scan)
__global__ void __launch_bounds__(256) km_chunk_sums_kernel(const double* __restrict__ src, int64_t n, int rows,
                                                            double* __restrict__ tot) {
  const int64_t nc = cdiv(n, KM_CHUNK);
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nc * rows) return;
  const int64_t r = t / nc, c = t % nc;
  const double* a = src + r * n;
  const int64_t e = std::min<int64_t>(n, (c + 1) * KM_CHUNK);
  double s = 0.0;
  for (int64_t i = c * KM_CHUNK; i < e; ++i) s = __dadd_rn(s, a[i]);
  tot[t] = s;
}

// off[r][c] = sequential exclusive scan of tot[r][.], pot[r] = the total
__global__ void km_offsets_kernel(const double* __restrict__ tot, int64_t nc, int rows, double* __restrict__ off,
                                  double* __restrict__ pot) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  double s = 0.0;
  for (int64_t c = 0; c < nc; ++c) {
    off[r * nc + c] = s;
    s = __dadd_rn(s, tot[r * nc + c]);
  }
  pot[r] = s;
}

// cs[i] = off[c] + (inclusive sequential scan of src inside chunk c); row `*row` of off (row == NULL: row 0)
__global__ void __launch_bounds__(256) km_scan_apply_kernel(const double* __restrict__ src, int64_t n,
                                                            const double* __restrict__ off, const int* __restrict__ row,
                                                            double* __restrict__ cs) {
  const int64_t nc = cdiv(n, KM_CHUNK);
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const double o = off[(row != nullptr ? (int64_t)*row : 0) * nc + c];
  const int64_t e = std::min<int64_t>(n, (c + 1) * KM_CHUNK);
  double s = 0.0;
  for (int64_t i = c * KM_CHUNK; i < e; ++i) {
    s = __dadd_rn(s, src[i]);
    cs[i] = __dadd_rn(o, s);
  }
}

// candidates of centre c: searchsorted(cs, u[t] * pot, side='left'), clipped to n - 1
__global__ void km_search_kernel(const double* __restrict__ cs, int64_t n, const double* __restrict__ pot,
                                 const double* __restrict__ u, int trials, int* __restrict__ cand) {
  const int t = threadIdx.x;
  if (t >= trials) return;
  const double v = __dmul_rn(u[t], *pot);
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) / 2;
    if (cs[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  cand[t] = (int)(lo < n - 1 ? lo : n - 1);
}

// D[t][i] = min(closest[i], d2(x_i, x_cand[t]))
__global__ void __launch_bounds__(256) km_trial_kernel(const float* __restrict__ x, int64_t n, int d,
                                                       const int* __restrict__ cand, int trials,
                                                       const double* __restrict__ closest, double* __restrict__ D) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float r[KM_DMAX];
  load_row_f32(x, i, d, r);
  const double ci = closest[i];
  for (int t = 0; t < trials; ++t) {
    const int64_t cj = cand[t];
    const double v = np_d2_f64(r, [&](int f) { return (double)x[cj * d + f]; }, d);
    D[(int64_t)t * n + i] = v < ci ? v : ci;
  }
}

// the trial of least potential (the first on ties) becomes centre c
__global__ void km_pick_kernel(const double* __restrict__ pot_t, int trials, const int* __restrict__ cand, int c,
                               int* __restrict__ best, int* __restrict__ seeds, double* __restrict__ pot) {
  if (threadIdx.x != 0) return;
  int b = 0;
  for (int t = 1; t < trials; ++t)
    if (pot_t[t] < pot_t[b]) b = t;
  *best = b;
  seeds[c] = cand[b];
  *pot = pot_t[b];
}

__global__ void __launch_bounds__(256) km_take_kernel(const double* __restrict__ D, int64_t n, const int* __restrict__ best,
                                                      double* __restrict__ closest) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  closest[i] = D[(int64_t)*best * n + i];
}

__global__ void __launch_bounds__(256) km_gather_kernel(const float* __restrict__ x, int d, const int* __restrict__ seeds,
                                                        int k, double* __restrict__ centers) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)k * d) return;
  centers[t] = (double)x[(int64_t)seeds[t / d] * d + t % d];
}

// labels[i] = argmin_j d2(x_i, c_j) (the lower index on ties), mind2[i] = that distance; counts[j] += 1 (integer
// atomics); changed += (labels[i] != old[i]) when old != NULL
__global__ void __launch_bounds__(256) km_assign_kernel(const float* __restrict__ x, int64_t n, int d,
                                                        const double* __restrict__ centers, int k,
                                                        int* __restrict__ labels, double* __restrict__ mind2,
                                                        int* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float r[KM_DMAX];
  load_row_f32(x, i, d, r);
  double best = INFINITY;
  int arg = 0;
  for (int j = 0; j < k; ++j) {
    const double* c = centers + (int64_t)j * d;
    const double v = np_d2_f64(r, [&](int f) { return c[f]; }, d);
    if (v < best) { best = v; arg = j; }
  }
  labels[i] = arg;
  mind2[i] = best;
  atomicAdd(&counts[arg], 1);
}

__global__ void __launch_bounds__(256) km_iota_kernel(int* __restrict__ v, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = (int)i;
}

// changed += (labels != old); old = labels
__global__ void __launch_bounds__(256) km_changed_kernel(const int* __restrict__ labels, int* __restrict__ old, int64_t n,
                                                         int* __restrict__ changed) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int l = labels[i];
  if (l != old[i]) atomicAdd(changed, 1);
  old[i] = l;
}

// new centre j, feature f: the sequential f64 sum of x over the rows of cluster j in row order (the rows sorted by
// (label, row): `order` from the stable radix sort), divided by the count; an empty cluster keeps its centre
__global__ void __launch_bounds__(256) km_update_kernel(const float* __restrict__ x, int d, int k,
                                                        const int* __restrict__ order, const int* __restrict__ starts,
                                                        const int* __restrict__ counts,
                                                        const double* __restrict__ centers, double* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)k * d) return;
  const int j = (int)(t / d), f = (int)(t % d);
  const int b = starts[j], m = counts[j];
  if (m == 0) { out[t] = centers[t]; return; }
  double s = 0.0;
  for (int q = b; q < b + m; ++q) s = __dadd_rn(s, (double)x[(int64_t)order[q] * d + f]);
  out[t] = s / (double)m;
}

// shift = sum (new - old)^2 over the k x d values: per-lane strided sums, then a fixed tree (one workgroup)
__global__ void __launch_bounds__(256) km_shift_kernel(const double* __restrict__ a, const double* __restrict__ b,
                                                       int64_t m, double* __restrict__ shift) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int64_t t = tid; t < m; t += 256) { const double e = a[t] - b[t]; s = __dadd_rn(s, __dmul_rn(e, e)); }
  red[tid] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] = __dadd_rn(red[tid], red[tid + w]);
    __syncthreads();
  }
  if (tid == 0) *shift = red[0];
}

__global__ void km_starts_kernel(const int* __restrict__ counts, int k, int* __restrict__ starts) {
  if (threadIdx.x != 0) return;
  int s = 0;
  for (int j = 0; j < k; ++j) { starts[j] = s; s += counts[j]; }
}

// Workspace layouts: one function per builder sizes its scratch (NULL address) and carves it (common.h Carver; the
// members are the regions in order).  The k-means one is kmeans.h's km_layout, below.

// k-NN: the points as f64, the cell bounds of the scan, the search grid and the scratch of its build
struct KnnWs { double* pts; int* bounds; char *grid, *grid_ws; int64_t grid_bytes, grid_ws_bytes, total; };
KnnWs knn_layout(int64_t p, void* ws) {
  const int64_t q = p > 0 ? p : 1, gb = lidal_nn_grid_bytes(q), gwb = lidal_nn_grid_workspace_bytes(q);
  Carver c(ws);
  return {c.take<double>(3 * q), c.take<int>(6), c.take(gb), c.take(gwb), gb, gwb, c.total()};
}

// one assignment + its counts; rows of empty clusters relocated (host side: rare)
int km_assign(const float* x, int64_t n, int d, const double* centers, int k, int* labels, const KmWs& w, hipStream_t s,
              bool relocate, int* n_empty_out) {
  LIDAL_HIP(hipMemsetAsync(w.counts, 0, 4 * (size_t)k, s));
  km_assign_kernel<<<(unsigned)cdiv(n, 256), 256, 0, s>>>(x, n, d, centers, k, labels, w.mind2, w.counts);
  LIDAL_CHECK_LAUNCH("km_assign");
  *n_empty_out = 0;
  if (!relocate) return 0;
  std::vector<int> cnt(k);
  LIDAL_HIP(hipMemcpyAsync(cnt.data(), w.counts, 4 * (size_t)k, hipMemcpyDeviceToHost, s));
  LIDAL_HIP(hipStreamSynchronize(s));
  std::vector<int> empty;
  for (int j = 0; j < k; ++j)
    if (cnt[j] == 0) empty.push_back(j);
  *n_empty_out = (int)empty.size();
  if (empty.empty()) return 0;
  // the e-th empty cluster (ascending) takes the e-th farthest row from its centre (the lower index on ties)
  std::vector<double> md(n);
  std::vector<int> lab(n);
  LIDAL_HIP(hipMemcpyAsync(md.data(), w.mind2, 8 * (size_t)n, hipMemcpyDeviceToHost, s));
  LIDAL_HIP(hipMemcpyAsync(lab.data(), labels, 4 * (size_t)n, hipMemcpyDeviceToHost, s));
  LIDAL_HIP(hipStreamSynchronize(s));
  std::vector<int> idx(n);
  for (int64_t i = 0; i < n; ++i) idx[i] = (int)i;
  const size_t m = std::min(empty.size(), (size_t)n);
  std::partial_sort(idx.begin(), idx.begin() + m, idx.end(),
                    [&](int a, int b) { return md[a] > md[b] || (md[a] == md[b] && a < b); });
  for (size_t e = 0; e < m; ++e) {
    --cnt[lab[idx[e]]];
    lab[idx[e]] = empty[e];
    cnt[empty[e]] = 1;
    md[idx[e]] = 0.0;
  }
  LIDAL_HIP(hipMemcpyAsync(labels, lab.data(), 4 * (size_t)n, hipMemcpyHostToDevice, s));
  LIDAL_HIP(hipMemcpyAsync(w.counts, cnt.data(), 4 * (size_t)k, hipMemcpyHostToDevice, s));
  LIDAL_HIP(hipMemcpyAsync(w.mind2, md.data(), 8 * (size_t)n, hipMemcpyHostToDevice, s));
  LIDAL_HIP(hipStreamSynchronize(s));       // (the host vectors go out of scope)
  return 0;
}

int km_total(const double* v, int64_t n, const KmWs& w, hipStream_t s, double* out_dev) {
  const int64_t nc = cdiv(n, KM_CHUNK);
  km_chunk_sums_kernel<<<(unsigned)cdiv(nc, 256), 256, 0, s>>>(v, n, 1, w.tot);
  LIDAL_CHECK_LAUNCH("km_chunk_sums");
  km_offsets_kernel<<<1, 64, 0, s>>>(w.tot, nc, 1, w.off, out_dev);
  LIDAL_CHECK_LAUNCH("km_offsets");
  return 0;
}

}  // namespace


// ---------------------------------------------------------------- k-means steps shared with supervoxel.hip (kmeans.h)
namespace lidal {

KmWs km_layout(int64_t n_rows, int d, int k, int trials, void* ws) {
  const int64_t n = n_rows > 0 ? n_rows : 1, nc = cdiv(n, KM_CHUNK), tr = trials > 0 ? trials : 1;
  const int64_t tmp = radix_sort_ws_bytes(n, 4, true);
  Carver c(ws);
  return {c.take<double>(n), c.take<double>(n * tr), c.take<double>(n), c.take<double>(nc * tr), c.take<double>(nc * tr),
          c.take<double>(tr), c.take<double>(1), c.take<double>(n), c.take<double>((int64_t)k * d), c.take<double>(1),
          c.take<int>(tr), c.take<int>(1), c.take<int>(n), c.take<int>(n), c.take<int>(n), c.take<int>(n), c.take<int>(n),
          c.take<int>(k), c.take<int>(k), c.take<int>(1), c.take(tmp), tmp, c.total()};
}

int km_seed(const float* x, int64_t n, int d, int k, int64_t first, const double* u, int trials, int32_t* seeds,
            double* centers, const KmWs& w, hipStream_t s) {
  const int64_t nc = cdiv(n, KM_CHUNK);
  const unsigned gn = (unsigned)cdiv(n, 256);
  km_first_seed_kernel<<<1, 64, 0, s>>>(seeds, (int)first);
  LIDAL_CHECK_LAUNCH("km_first_seed");
  km_first_kernel<<<gn, 256, 0, s>>>(x, n, d, first, w.closest);
  LIDAL_CHECK_LAUNCH("km_first");
  if (int rc = km_total(w.closest, n, w, s, w.pot)) return rc;
  for (int c = 1; c < k; ++c) {
    km_scan_apply_kernel<<<(unsigned)cdiv(nc, 256), 256, 0, s>>>(w.closest, n, w.off, c == 1 ? nullptr : w.best, w.cs);
    LIDAL_CHECK_LAUNCH("km_scan_apply");
    km_search_kernel<<<1, 64, 0, s>>>(w.cs, n, w.pot, u + (int64_t)(c - 1) * trials, trials, w.cand);
    LIDAL_CHECK_LAUNCH("km_search");
    km_trial_kernel<<<gn, 256, 0, s>>>(x, n, d, w.cand, trials, w.closest, w.D);
    LIDAL_CHECK_LAUNCH("km_trial");
    km_chunk_sums_kernel<<<(unsigned)cdiv(nc * trials, 256), 256, 0, s>>>(w.D, n, trials, w.tot);
    LIDAL_CHECK_LAUNCH("km_chunk_sums");
    km_offsets_kernel<<<1, 64, 0, s>>>(w.tot, nc, trials, w.off, w.pot_t);
    LIDAL_CHECK_LAUNCH("km_offsets");
    km_pick_kernel<<<1, 64, 0, s>>>(w.pot_t, trials, w.cand, c, w.best, seeds, w.pot);
    LIDAL_CHECK_LAUNCH("km_pick");
    km_take_kernel<<<gn, 256, 0, s>>>(w.D, n, w.best, w.closest);
    LIDAL_CHECK_LAUNCH("km_take");
  }
  km_gather_kernel<<<(unsigned)cdiv((int64_t)k * d, 256), 256, 0, s>>>(x, d, seeds, k, centers);
  LIDAL_CHECK_LAUNCH("km_gather");
  return 0;
}

int km_iota(int64_t n, const KmWs& w, hipStream_t s) {
  km_iota_kernel<<<(unsigned)cdiv(n, 256), 256, 0, s>>>(w.iota, n);
  LIDAL_CHECK_LAUNCH("km_iota");
  return 0;
}

int km_update(const float* x, int64_t n, int d, int k, const int32_t* labels, const int* counts, const double* centers,
              double* out, const KmWs& w, hipStream_t s) {
  int end_bit = 1;
  while ((1 << end_bit) < k) ++end_bit;
  if (int rc = radix_sort(labels, w.iota, w.skeys, w.order, n, 4, end_bit, w.sort_tmp, w.sort_bytes, s)) return rc;
  km_starts_kernel<<<1, 64, 0, s>>>(counts, k, w.starts);
  LIDAL_CHECK_LAUNCH("km_starts");
  km_update_kernel<<<(unsigned)cdiv((int64_t)k * d, 256), 256, 0, s>>>(x, d, k, w.order, w.starts, counts, centers, out);
  LIDAL_CHECK_LAUNCH("km_update");
  return 0;
}

}  // namespace lidal

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
  LIDAL_REQUIRE(c > 0 && c <= MAXC, "region_scores: classes must be in 1..%d", MAXC);
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

// ---------------------------------------------------------------- k-means
extern "C" int64_t lidal_kmeans_workspace_bytes(int64_t n, int d, int k, int trials) {
  return km_layout(n, d, k, trials, nullptr).total;
}

extern "C" int lidal_kmeans(const float* x, int64_t n, int d, int k, int64_t first, const double* u, int trials,
                            int max_iter, double tol, int32_t* seeds, int32_t* labels, double* centers,
                            double* inertia_host, int32_t* n_iter_host, void* ws, int64_t ws_bytes, void* stream) {
  LIDAL_REQUIRE(d >= 1 && d <= KM_DMAX, "kmeans: the feature width must be in 1..%d", KM_DMAX);
  LIDAL_REQUIRE(k >= 1 && (int64_t)k <= n, "kmeans: n_clusters (%d) must be in 1..n_samples (%lld)", k, (long long)n);
  LIDAL_REQUIRE(n < 0x7FFFFFFF, "kmeans: at most 2^31 - 1 rows");
  LIDAL_REQUIRE(trials >= 1 && trials <= 64, "kmeans: local trials must be in 1..64");
  LIDAL_REQUIRE(first >= 0 && first < n, "kmeans: first centre out of range");
  LIDAL_REQUIRE(max_iter >= 0, "kmeans: max_iter must not be negative");
  const KmWs w = km_layout(n, d, k, trials, ws);
  LIDAL_REQUIRE(ws_bytes >= w.total, "kmeans workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const unsigned gn = (unsigned)cdiv(n, 256);
  if (int rc = km_seed(x, n, d, k, first, u, trials, seeds, centers, w, s)) return rc;
  // ---- Lloyd
  if (int rc = km_iota(n, w, s)) return rc;
  LIDAL_HIP(hipMemsetAsync(w.old, 0xFF, 4 * (size_t)n, s));         // labels_old = -1
  bool strict = false;
  int it = 0;
  for (; it < max_iter; ++it) {
    int n_empty = 0;
    if (int rc = km_assign(x, n, d, centers, k, labels, w, s, true, &n_empty)) return rc;
    LIDAL_HIP(hipMemsetAsync(w.changed, 0, 4, s));
    km_changed_kernel<<<gn, 256, 0, s>>>(labels, w.old, n, w.changed);
    LIDAL_CHECK_LAUNCH("km_changed");
    if (int rc = km_update(x, n, d, k, labels, w.counts, centers, w.cnew, w, s)) return rc;
    km_shift_kernel<<<1, 256, 0, s>>>(w.cnew, centers, (int64_t)k * d, w.shift);
    LIDAL_CHECK_LAUNCH("km_shift");
    LIDAL_HIP(hipMemcpyAsync(centers, w.cnew, 8 * (size_t)k * d, hipMemcpyDeviceToDevice, s));
    int changed = 0;
    double shift = 0.0;
    LIDAL_HIP(hipMemcpyAsync(&changed, w.changed, 4, hipMemcpyDeviceToHost, s));
    LIDAL_HIP(hipMemcpyAsync(&shift, w.shift, 8, hipMemcpyDeviceToHost, s));
    LIDAL_HIP(hipStreamSynchronize(s));
    if (changed == 0) { strict = true; ++it; break; }
    if (shift <= tol) { ++it; break; }
  }
  if (!strict) {        // the labels of the returned centres
    int n_empty = 0;
    if (int rc = km_assign(x, n, d, centers, k, labels, w, s, false, &n_empty)) return rc;
  }
  if (int rc = km_total(w.mind2, n, w, s, w.pot)) return rc;
  double inertia = 0.0;
  LIDAL_HIP(hipMemcpyAsync(&inertia, w.pot, 8, hipMemcpyDeviceToHost, s));
  LIDAL_HIP(hipStreamSynchronize(s));
  *inertia_host = inertia;
  *n_iter_host = it;
  return 0;
}
