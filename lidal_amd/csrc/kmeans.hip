// The k-means that replaces sklearn.cluster.KMeans in ReDAL's diversity-aware selection (lidal_kmeans), and the steps
// of it that supervoxel.hip shares (kmeans.h), for gfx950.  Every reduction runs in a fixed order and restates numpy
// (DESIGN.md section 8); built with -ffp-contract=off (lidal_amd/build.py) so that a*b+c stays two roundings.  No
// float atomics anywhere: the k-means is deterministic run to run.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"
#include "kmeans.h"
#include "npsum.h"

using namespace lidal;
using namespace lidal::npsum;

namespace {

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