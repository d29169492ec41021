// Scan-to-scan registration by point-to-plane ICP: the normals of a target scan and the
// iterations that move a source scan onto it, all enqueued without a read-back.
//   * lidal_point_normals: the k nearest other points of every point (lidal_knn, redal.hip), their population covariance
//     and its cyclic Jacobi with eigenvectors (sym3.h); the normal is the eigenvector of the smallest eigenvalue, turned
//     to face the sensor origin.
//   * lidal_icp_run: per iteration an ACCUMULATE launch (one correspondence per source point through grid_nearest,
//     grid.h, and the 29 sums of the normal equations in a fixed order) and a FINISH launch of one workgroup (the sums
//     of the partial rows, a 6x6 Cholesky solve, the pose update by a normalised quaternion, the stopping rules).
// The definitions are this project's own; tests/icp_ref.py restates them in numpy.  Built without fma contraction and
// without packed-f32 instructions (lidal_amd/build.py).  + - * / and sqrt only, no float atomics: every output is a
// function of the inputs alone.
#include <cmath>

#include "common.h"
#include "grid.h"
#include "sym3.h"

using namespace lidal;
using namespace lidal::grid;
using namespace lidal::sym3;

extern "C" int64_t lidal_knn_workspace_bytes(int64_t p);
extern "C" int lidal_knn(const float* xyz, int64_t p, int k, double cell, int32_t* knn, void* ws, int64_t ws_bytes,
                         void* stream);

namespace {

constexpr int kThreads = 256;
constexpr int kTerms = 29;          // 21 products J_u J_v (u <= v), 6 terms -(J_u r), r r, 1
constexpr int kRow = 32;            // doubles per partial row
constexpr int kTrace = 64;          // doubles per trace row (include/lidal_amd.h: LIDAL_ICP_TRACE_*)
constexpr int kMaxBlocks = 1024;
constexpr int kMaxIters = 256;
// trace row offsets
enum { TR_SUMS = 0, TR_XI = 29, TR_STATUS = 35, TR_MAX_DIST = 36, TR_POSE = 37, TR_END = 53 };
enum { ST_OK = 0, ST_CONVERGED, ST_SKIPPED, ST_FEW_PAIRS, ST_DEGENERATE, ST_AFTER_FAILURE };
// state words: the status of the iteration that failed (0: none), 1 + the level that converged (0: none)
enum { SW_FAILED = 0, SW_CONVERGED = 1, SW_WORDS = 64 };

// ================================ normals ================================
__global__ void __launch_bounds__(kThreads)
normals_kernel(const float* __restrict__ xyz, int64_t p, int k, const int* __restrict__ knn, double max_variation,
               double* __restrict__ normals) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= p) return;
  bool bad = false;
  for (int s = 0; s < k; ++s) {
    const int j = knn[i * k + s];
    bad |= (j < 0 || (int64_t)j >= p);          // (a list that a non-finite query never filled)
  }
  double nx = 0.0, ny = 0.0, nz = 0.0;
  if (!bad) {
    double a[3][3], e[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    covariance3([&](auto visit) {
      for (int s = 0; s < k; ++s) {
        const int64_t j = knn[i * k + s];
        visit((double)xyz[j * 3 + 0], (double)xyz[j * 3 + 1], (double)xyz[j * 3 + 2]);
      }
    }, k, a);
    jacobi3<true>(a, e);
    const double l0 = a[0][0], l1 = a[1][1], l2 = a[2][2];
    double lmin = l0;
    nx = e[0][0]; ny = e[1][0]; nz = e[2][0];
    if (l1 < lmin) { lmin = l1; nx = e[0][1]; ny = e[1][1]; nz = e[2][1]; }       // ties: the lowest column
    if (l2 < lmin) { lmin = l2; nx = e[0][2]; ny = e[1][2]; nz = e[2][2]; }
    const double sum = l0 + l1 + l2;
    const double var = lmin / sum;
    const double x = (double)xyz[i * 3 + 0], y = (double)xyz[i * 3 + 1], z = (double)xyz[i * 3 + 2];
    const double facing = __dadd_rn(__dadd_rn(__dmul_rn(nx, x), __dmul_rn(ny, y)), __dmul_rn(nz, z));
    if (facing > 0.0) { nx = -nx; ny = -ny; nz = -nz; }
    const bool finite = fabs(nx) < INFINITY && fabs(ny) < INFINITY && fabs(nz) < INFINITY && fabs(var) < INFINITY &&
                        fabs(facing) < INFINITY;
    if (sum == 0.0 || !finite || var > max_variation) { nx = 0.0; ny = 0.0; nz = 0.0; }
  }
  normals[i * 3 + 0] = nx;
  normals[i * 3 + 1] = ny;
  normals[i * 3 + 2] = nz;
}

struct NormalsWs { int* knn; char* knn_ws; int64_t knn_ws_bytes, total; };
NormalsWs normals_layout(int64_t p, int k, void* ws) {
  const int64_t q = p > 0 ? p : 1, kk = k > 0 ? k : 1, kb = lidal_knn_workspace_bytes(q);
  Carver c(ws);
  return {c.take<int>(q * kk), c.take(kb), kb, c.total()};
}

// ================================ ICP ================================
// One source point per thread and trip (thread t takes the source points (t + n * threads) * stride): its correspondence
// and the 29 terms of the normal equations, summed per thread in trip order, then over the workgroup by a fixed tree.
__global__ void __launch_bounds__(kThreads)
icp_accumulate_kernel(const float* __restrict__ src, int64_t n_used, int64_t stride, const void* __restrict__ grid,
                      int64_t p_tgt, int64_t cap, const double* __restrict__ tgt_pts,
                      const double* __restrict__ tgt_normals, const double* __restrict__ pose, double max_dist, int level,
                      const int* __restrict__ state, double* __restrict__ partial) {
  __shared__ double red[kTerms][kThreads];
  if (state[SW_FAILED] != 0 || state[SW_CONVERGED] == level + 1) return;      // (the same answer in every thread)
  const int tid = threadIdx.x;
  double acc[kTerms];
#pragma unroll
  for (int q = 0; q < kTerms; ++q) acc[q] = 0.0;
  if (p_tgt > 0) {
    double P[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) P[q] = pose[q];
    const GridView g = grid_view(grid, p_tgt, cap, reinterpret_cast<const GridHeader*>(grid)->cell);
    for (int64_t t = (int64_t)blockIdx.x * kThreads + tid; t < n_used; t += (int64_t)gridDim.x * kThreads) {
      const int64_t i = t * stride;
      const double h0 = (double)src[i * 3 + 0], h1 = (double)src[i * 3 + 1], h2 = (double)src[i * 3 + 2];
      double s[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {        // register_kernel's order (score.hip)
        double v = __dadd_rn(__dmul_rn(h0, P[j * 4 + 0]), __dmul_rn(h1, P[j * 4 + 1]));
        v = __dadd_rn(v, __dmul_rn(h2, P[j * 4 + 2]));
        s[j] = __dadd_rn(v, P[j * 4 + 3]);
      }
      double d2;
      int j = grid_nearest(g, tgt_pts, s[0], s[1], s[2], max_dist, &d2);      // (a non-finite s matches nothing)
      if (j >= 0 && !(sqrt(d2) <= max_dist)) j = -1;
      if (j < 0 || (int64_t)j >= p_tgt) continue;
      const double nx = tgt_normals[(int64_t)j * 3 + 0], ny = tgt_normals[(int64_t)j * 3 + 1],
                   nz = tgt_normals[(int64_t)j * 3 + 2];
      if (nx == 0.0 && ny == 0.0 && nz == 0.0) continue;
      const double tx = tgt_pts[(int64_t)j * 3 + 0], ty = tgt_pts[(int64_t)j * 3 + 1], tz = tgt_pts[(int64_t)j * 3 + 2];
      const double r = __dadd_rn(__dadd_rn(__dmul_rn(s[0] - tx, nx), __dmul_rn(s[1] - ty, ny)), __dmul_rn(s[2] - tz, nz));
      double J[6];
      J[0] = __dsub_rn(__dmul_rn(s[1], nz), __dmul_rn(s[2], ny));             // a = s x n
      J[1] = __dsub_rn(__dmul_rn(s[2], nx), __dmul_rn(s[0], nz));
      J[2] = __dsub_rn(__dmul_rn(s[0], ny), __dmul_rn(s[1], nx));
      J[3] = nx; J[4] = ny; J[5] = nz;
      int q = 0;
#pragma unroll
      for (int u = 0; u < 6; ++u)
#pragma unroll
        for (int v = u; v < 6; ++v) { acc[q] = __dadd_rn(acc[q], __dmul_rn(J[u], J[v])); ++q; }
#pragma unroll
      for (int u = 0; u < 6; ++u) acc[21 + u] = __dadd_rn(acc[21 + u], -__dmul_rn(J[u], r));
      acc[27] = __dadd_rn(acc[27], __dmul_rn(r, r));
      acc[28] = __dadd_rn(acc[28], 1.0);
    }
  }
#pragma unroll
  for (int q = 0; q < kTerms; ++q) red[q][tid] = acc[q];
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if (tid < w)
#pragma unroll
      for (int q = 0; q < kTerms; ++q) red[q][tid] = __dadd_rn(red[q][tid], red[q][tid + w]);
    __syncthreads();
  }
  if (tid < kRow) partial[(int64_t)blockIdx.x * kRow + tid] = tid < kTerms ? red[tid][0] : 0.0;
}

// One workgroup: the partial rows summed in index order, then thread 0 solves A xi = b (Cholesky, fixed order), updates
// the pose and applies the stopping rules.
__global__ void __launch_bounds__(64)
icp_finish_kernel(const double* __restrict__ partial, int n_blocks, double* __restrict__ pose, double max_dist, int level,
                  int min_pairs, double eps_rot, double eps_trans, int* __restrict__ state, double* __restrict__ row) {
  __shared__ double sums[kRow];
  const int tid = threadIdx.x;
  const int failed = state[SW_FAILED];
  const bool skip = state[SW_CONVERGED] == level + 1;
  if (failed != 0 || skip) {
    double v = 0.0;
    if (tid == TR_STATUS) v = failed != 0 ? (double)ST_AFTER_FAILURE : (double)ST_SKIPPED;
    else if (tid == TR_MAX_DIST) v = max_dist;
    else if (tid >= TR_POSE && tid < TR_END) v = pose[tid - TR_POSE];
    row[tid] = v;
    return;
  }
  if (tid < kTerms) {
    double s = 0.0;
    for (int b = 0; b < n_blocks; ++b) s = __dadd_rn(s, partial[(int64_t)b * kRow + tid]);
    sums[tid] = s;
  }
  __syncthreads();
  if (tid != 0) return;
  double P[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) P[q] = pose[q];
  double A[6][6], b[6], xi[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  {
    int q = 0;
#pragma unroll
    for (int u = 0; u < 6; ++u)
#pragma unroll
      for (int v = u; v < 6; ++v) { A[u][v] = A[v][u] = sums[q]; ++q; }
#pragma unroll
    for (int u = 0; u < 6; ++u) b[u] = sums[21 + u];
  }
  int status = ST_OK;
  if (!(sums[28] >= (double)min_pairs)) status = ST_FEW_PAIRS;
  double L[6][6];
  if (status == ST_OK) {
    double dmax = A[0][0];
#pragma unroll
    for (int u = 1; u < 6; ++u) dmax = A[u][u] > dmax ? A[u][u] : dmax;
    const double floor_ = __dmul_rn(1e-12, dmax);
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double d = A[j][j];
#pragma unroll
      for (int k = 0; k < j; ++k) d = __dsub_rn(d, __dmul_rn(L[j][k], L[j][k]));
      if (!(d > floor_) || !(d < INFINITY)) status = ST_DEGENERATE;       // (NaN fails the first test)
      L[j][j] = sqrt(d);
#pragma unroll
      for (int i = j + 1; i < 6; ++i) {
        double s = A[i][j];
#pragma unroll
        for (int k = 0; k < j; ++k) s = __dsub_rn(s, __dmul_rn(L[i][k], L[j][k]));
        L[i][j] = s / L[j][j];
      }
    }
  }
  if (status == ST_OK) {
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double s = b[i];
#pragma unroll
      for (int k = 0; k < i; ++k) s = __dsub_rn(s, __dmul_rn(L[i][k], y[k]));
      y[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
      double s = y[i];
#pragma unroll
      for (int k = i + 1; k < 6; ++k) s = __dsub_rn(s, __dmul_rn(L[k][i], xi[k]));
      xi[i] = s / L[i][i];
    }
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 6; ++i) finite = finite && fabs(xi[i]) < INFINITY;
    if (!finite) status = ST_DEGENERATE;
  }
  if (status == ST_OK) {
    // q = (1, omega / 2) / |.|, R its rotation, pose <- [R | v; 0 0 0 1] pose
    double qx = __dmul_rn(0.5, xi[0]), qy = __dmul_rn(0.5, xi[1]), qz = __dmul_rn(0.5, xi[2]);
    const double nrm = sqrt(__dadd_rn(__dadd_rn(__dadd_rn(1.0, __dmul_rn(qx, qx)), __dmul_rn(qy, qy)), __dmul_rn(qz, qz)));
    const double qw = 1.0 / nrm;
    qx = qx / nrm; qy = qy / nrm; qz = qz / nrm;
    const double xx = __dmul_rn(qx, qx), yy = __dmul_rn(qy, qy), zz = __dmul_rn(qz, qz);
    const double xy = __dmul_rn(qx, qy), xz = __dmul_rn(qx, qz), yz = __dmul_rn(qy, qz);
    const double wx = __dmul_rn(qw, qx), wy = __dmul_rn(qw, qy), wz = __dmul_rn(qw, qz);
    double R[3][3];
    R[0][0] = __dsub_rn(1.0, __dmul_rn(2.0, __dadd_rn(yy, zz)));
    R[0][1] = __dmul_rn(2.0, __dsub_rn(xy, wz));
    R[0][2] = __dmul_rn(2.0, __dadd_rn(xz, wy));
    R[1][0] = __dmul_rn(2.0, __dadd_rn(xy, wz));
    R[1][1] = __dsub_rn(1.0, __dmul_rn(2.0, __dadd_rn(xx, zz)));
    R[1][2] = __dmul_rn(2.0, __dsub_rn(yz, wx));
    R[2][0] = __dmul_rn(2.0, __dsub_rn(xz, wy));
    R[2][1] = __dmul_rn(2.0, __dadd_rn(yz, wx));
    R[2][2] = __dsub_rn(1.0, __dmul_rn(2.0, __dadd_rn(xx, yy)));
    double N[12];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        double v = __dadd_rn(__dmul_rn(R[i][0], P[0 * 4 + j]), __dmul_rn(R[i][1], P[1 * 4 + j]));
        v = __dadd_rn(v, __dmul_rn(R[i][2], P[2 * 4 + j]));
        N[i * 4 + j] = __dadd_rn(v, __dmul_rn(xi[3 + i], P[3 * 4 + j]));
      }
#pragma unroll
    for (int q = 0; q < 12; ++q) pose[q] = N[q];
    const double rot = fmax(fabs(xi[0]), fmax(fabs(xi[1]), fabs(xi[2])));
    const double tra = fmax(fabs(xi[3]), fmax(fabs(xi[4]), fabs(xi[5])));
    if (rot < eps_rot && tra < eps_trans) {
      status = ST_CONVERGED;
      state[SW_CONVERGED] = level + 1;
    }
  } else {
    state[SW_FAILED] = status;
#pragma unroll
    for (int i = 0; i < 6; ++i) xi[i] = 0.0;
  }
#pragma unroll
  for (int q = 0; q < kTerms; ++q) row[TR_SUMS + q] = sums[q];
#pragma unroll
  for (int i = 0; i < 6; ++i) row[TR_XI + i] = xi[i];
  row[TR_STATUS] = (double)status;
  row[TR_MAX_DIST] = max_dist;
#pragma unroll
  for (int q = 0; q < 16; ++q) row[TR_POSE + q] = P[q];
  for (int q = TR_END; q < kTrace; ++q) row[q] = 0.0;
}

int64_t icp_blocks(int64_t p_src, int64_t stride) {
  const int64_t n_used = (p_src > 0 && stride > 0) ? cdiv(p_src, stride) : 0;
  const int64_t b = cdiv(n_used, kThreads);
  return b < kMaxBlocks ? b : kMaxBlocks;
}

struct IcpWs { int* state; double* partial; int64_t total; };
IcpWs icp_layout(int64_t p_src, int64_t stride, void* ws) {
  const int64_t nb = icp_blocks(p_src, stride);
  Carver c(ws);
  return {c.take<int>(SW_WORDS), c.take<double>((nb > 0 ? nb : 1) * kRow), c.total()};
}

}  // namespace

// ---------------------------------------------------------------- normals
extern "C" int64_t lidal_point_normals_workspace_bytes(int64_t p, int k) { return normals_layout(p, k, nullptr).total; }

extern "C" int lidal_point_normals(const float* xyz, int64_t p, int k, double cell, double max_variation, double* normals,
                                   void* ws, int64_t ws_bytes, void* stream) {
  LIDAL_REQUIRE(k >= 1 && k <= 64, "point_normals: k must be in 1..64");
  LIDAL_REQUIRE(p >= (int64_t)k + 1, "point_normals: %lld points cannot have %d nearest other points (need at least k + 1)",
                (long long)p, k);
  LIDAL_REQUIRE(p < 0x7FFFFFFF, "point_normals: at most 2^31 - 1 points");
  LIDAL_REQUIRE(cell > 0, "point_normals: cell must be positive");
  LIDAL_REQUIRE(max_variation == max_variation, "point_normals: max_variation is NaN");
  LIDAL_REQUIRE(xyz != nullptr && normals != nullptr && ws != nullptr, "point_normals: a NULL argument");
  const NormalsWs w = normals_layout(p, k, ws);
  LIDAL_REQUIRE(ws_bytes >= w.total, "point_normals workspace too small");
  if (int rc = lidal_knn(xyz, p, k, cell, w.knn, w.knn_ws, w.knn_ws_bytes, stream)) return rc;
  normals_kernel<<<(unsigned)cdiv(p, kThreads), kThreads, 0, (hipStream_t)stream>>>(xyz, p, k, w.knn, max_variation, normals);
  LIDAL_CHECK_LAUNCH("lidal_point_normals");
  return 0;
}

// ---------------------------------------------------------------- ICP
extern "C" int64_t lidal_icp_workspace_bytes(int64_t p_src, int64_t stride) { return icp_layout(p_src, stride, nullptr).total; }

extern "C" int lidal_icp_run(const float* src, int64_t p_src, int64_t stride, const void* tgt_grid, const double* tgt_pts,
                             const double* tgt_normals, int64_t p_tgt, double* pose, const double* max_dist_host,
                             int n_iters, int min_pairs, double eps_rot, double eps_trans, double* trace, void* ws,
                             int64_t ws_bytes, void* stream) {
  LIDAL_REQUIRE(stride >= 1, "icp_run: stride must be at least 1");
  LIDAL_REQUIRE(n_iters >= 1 && n_iters <= kMaxIters, "icp_run: n_iters must be in 1..%d", kMaxIters);
  LIDAL_REQUIRE(min_pairs >= 6, "icp_run: min_pairs must be at least 6");
  LIDAL_REQUIRE(p_src >= 0 && p_tgt >= 0, "icp_run: a negative point count");
  LIDAL_REQUIRE(p_tgt < 0x7FFFFFFF, "icp_run: at most 2^31 - 1 target points");
  LIDAL_REQUIRE(max_dist_host != nullptr, "icp_run: max_dist_host is NULL");
  for (int i = 0; i < n_iters; ++i)
    LIDAL_REQUIRE(max_dist_host[i] > 0.0 && max_dist_host[i] < INFINITY, "icp_run: max_dist[%d] must be finite and positive", i);
  LIDAL_REQUIRE(eps_rot == eps_rot && eps_trans == eps_trans, "icp_run: eps_rot / eps_trans is NaN");
  LIDAL_REQUIRE((src != nullptr || p_src == 0) && tgt_grid != nullptr && ((tgt_pts != nullptr && tgt_normals != nullptr) || p_tgt == 0) &&
                    pose != nullptr && trace != nullptr && ws != nullptr, "icp_run: a NULL argument");
  const IcpWs w = icp_layout(p_src, stride, ws);
  LIDAL_REQUIRE(ws_bytes >= w.total, "icp workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int64_t n_used = p_src > 0 ? cdiv(p_src, stride) : 0;
  const int n_blocks = (int)icp_blocks(p_src, stride);
  const int64_t cap = table_capacity(p_tgt > 0 ? p_tgt : 1);
  LIDAL_HIP(hipMemsetAsync(w.state, 0, SW_WORDS * sizeof(int), s));
  int level = 0;
  for (int i = 0; i < n_iters; ++i) {
    if (i > 0 && max_dist_host[i] != max_dist_host[i - 1]) level = i;
    if (n_blocks > 0) {
      icp_accumulate_kernel<<<(unsigned)n_blocks, kThreads, 0, s>>>(src, n_used, stride, tgt_grid, p_tgt, cap, tgt_pts,
                                                                   tgt_normals, pose, max_dist_host[i], level, w.state,
                                                                   w.partial);
      LIDAL_CHECK_LAUNCH("icp_accumulate");
    }
    icp_finish_kernel<<<1, 64, 0, s>>>(w.partial, n_blocks, pose, max_dist_host[i], level, min_pairs, eps_rot, eps_trans,
                                       w.state, trace + (int64_t)i * kTrace);
    LIDAL_CHECK_LAUNCH("icp_finish");
  }
  return 0;
}
