// Fixed-radius neighbour lists of a centre array for gfx950: which supervoxel centres lie within `radius` of each other,
// as a CSR table (row_ptr i64 [n + 1], col i32).  It replaces the distance work of the greedy selection
// (score/sv_level/LiDAL.py:225-325 of the reference, lidal_amd/score/selection.py: select_indexed); which hit the
// reference's loop meets FIRST stays on the host, what a hit IS is this table.
//
// THE TABLE.  Row i lists every j != i for which the reference's own expression is true,
//     np.sqrt(np.square(c[i] - c[j]).sum()) < radius
// on f32 rows, every operation separately rounded and the rounded root kept: within() of cellsort.h, whose header says
// why each step is written as it is.  The predicate is symmetric, so the table is.
//
// THE GRID.  Centres are sorted by the 63-bit cell key of grid.h with a cell edge of the smallest power of two >= radius
// (8 m for 5 m), and a query probes the 27 cells around its own.  That cannot miss a pair:
//   1. computed distance < radius  =>  |fl(a - b)| < radius on every axis.  Rounding is monotone, so the sum is at least
//      fl(dx^2), and in binary floating point fl(sqrt(fl(x * x))) == |x| unless x * x underflows; that takes
//      |x| < 2^-63, which is below every radius the entry points accept (>= 2^-60).
//   2. |fl(a - b)| < radius <= cell  =>  |a - b| < cell exactly: were |a - b| >= cell, a representable number, monotone
//      rounding would give |fl(a - b)| >= cell.
//   3. dividing by a power of two is exact, so floor(a / cell) and floor(b / cell) are the true cell indices, and two
//      reals less than one cell apart lie in the same or in adjacent cells.
// A cell edge of 5.0 does not give step 3: fl(x / 5) can round up across an integer boundary.
// The cells (x, y, z - 1 .. z + 1) are contiguous in key order, so 9 range look-ups (18 binary searches, one lane each:
// run_bound of cellsort.h) cover a query's 27 cells.
//
// One wave per query centre; its lanes stride over the candidates of a cell run, a wave ballot counts the hits
// (count pass) or ranks them into the row (fill pass): no atomics, the order of a row is a function of the centres
// alone.  The fill leaves a row in cell order; one wave then sorts it ascending in j with a bitonic network, in LDS
// when it fits and in place otherwise (rows of any length).
//
// What has no pairs: a centre with a NaN or infinite coordinate is filed in the parking cell (key 0, grid.h), which no
// probe reaches: its row is empty and it is in nobody's row, as in numpy, where such a distance is never < radius.
// What is refused: a finite coordinate whose cell index does not fit the key's 21-bit field raises *status_dev (the
// centre is parked, so the launches stay in bounds; the table is then not the reference's and the caller raises).
#include "cellsort.h"
#include "common.h"
#include "grid.h"
#include "scan.h"

using namespace lidal;
using namespace lidal::grid;
using namespace lidal::cellsort;

namespace {

constexpr int RP_BLOCK = 256;
constexpr int RP_WAVES = RP_BLOCK / kWave;         // query centres per workgroup, one wave each
constexpr int RP_SORT_LDS = 1024;                  // the longest row a wave sorts in LDS

__global__ void __launch_bounds__(RP_BLOCK) rp_keys_kernel(const float* __restrict__ centers, int64_t n, double cell,
                                                           u64* __restrict__ keys, int* __restrict__ idx,
                                                           int* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = centers[i * 3 + 0], y = centers[i * 3 + 1], z = centers[i * 3 + 2];
  u64 key = 0;                                 // the parking cell: every field 0
  if (finite_f32(x) && finite_f32(y) && finite_f32(z)) {
    const int64_t ix = cell_index((double)x, cell), iy = cell_index((double)y, cell), iz = cell_index((double)z, cell);
    if (ix == -kBias || iy == -kBias || iz == -kBias) {
      if (status != nullptr) atomicMax(status, (int)LIDAL_PAIRS_CELL_RANGE);
    } else {
      key = cell_key(ix, iy, iz);
    }
  }
  keys[i] = key;
  idx[i] = (int)i;
}

// FILL = false: counts[i] = length of row i.  FILL = true: col[row_ptr[i] ..) = row i in cell order.
template <bool FILL>
__global__ void __launch_bounds__(RP_BLOCK)
rp_pairs_kernel(const u64* __restrict__ skeys, const Rec* __restrict__ rec, int64_t n, float radius,
                int* __restrict__ counts, const int64_t* __restrict__ row_ptr, int* __restrict__ col) {
  const int lane = lane_id();
  for (int64_t q = (int64_t)blockIdx.x * RP_WAVES + (threadIdx.x >> 6); q < n; q += (int64_t)gridDim.x * RP_WAVES) {
    const u64 key = skeys[q];                  // (q, and everything derived from it alone, is uniform in the wave)
    const Rec me = rec[q];
    if (key == 0) {                                 // parked: no pairs
      if (!FILL && lane == 0) counts[me.idx] = 0;
      continue;
    }
    const int bound = run_bound(skeys, 0, (int)n, key, lane);        // lanes 0..8: a run begins; 9..17: it ends
    int64_t out = 0, out_end = 0;
    if (FILL) { out = row_ptr[me.idx]; out_end = row_ptr[(int64_t)me.idx + 1]; }
    int total = 0;
    for (int r = 0; r < 9; ++r) {
      const int lo = __shfl(bound, r), hi = __shfl(bound, r + 9);
      for (int64_t base = lo; base < hi; base += kWave) {
        const int64_t t = base + lane;
        bool hit = false;
        int j = 0;
        if (t < hi) {
          const Rec o = rec[t];
          j = o.idx;
          hit = j != me.idx && within(me, o, radius);
        }
        const unsigned long long mask = __ballot(hit);
        if (FILL && hit) {
          const int64_t pos = out + total + ballot_rank(mask);
          if (pos < out_end) col[pos] = j;          // (a row_ptr that is not this table's cannot push a write past its row)
        }
        total += __popcll(mask);
      }
    }
    if (!FILL && lane == 0) counts[me.idx] = total;
  }
}

// Rows ascending in j: one wave per row, a bitonic network whose merges all run upwards (the first step of a merge
// mirrors its halves), so that the positions past the row's end stand for +infinity and are simply never touched.
__global__ void __launch_bounds__(kWave) rp_sort_rows_kernel(const int64_t* __restrict__ row_ptr, int64_t n,
                                                             int* __restrict__ col) {
  __shared__ int sh[RP_SORT_LDS];
  const int lane = threadIdx.x;
  for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
    const int64_t beg = row_ptr[i], len = row_ptr[i + 1] - beg;
    if (len < 2) continue;                          // (uniform in the workgroup, as is every bound below)
    const bool in_lds = len <= RP_SORT_LDS;
    int* a = in_lds ? sh : col + beg;
    if (in_lds)
      for (int64_t t = lane; t < len; t += kWave) sh[t] = col[beg + t];
    __syncthreads();
    for (int kl = 1; (1ll << (kl - 1)) < len; ++kl) {         // merges of 2^kl positions
      for (int jl = kl - 1; jl >= 0; --jl) {                  // steps of a merge: partners 2^jl apart
        const bool mirror = jl == kl - 1;
        const int64_t j = 1ll << jl;
        // pair t of this step: block t >> jl of 2 j positions, lo = its (t mod j)-th position
        for (int64_t t = lane;; t += kWave) {
          const int64_t first = (t >> jl) << (jl + 1), off = t & (j - 1), lo = first + off;
          if (lo >= len) break;                     // lo grows with t
          const int64_t hi = mirror ? first + (2 * j - 1 - off) : lo + j;
          if (hi < len) {
            const int u = a[lo], v = a[hi];
            if (u > v) { a[lo] = v; a[hi] = u; }
          }
        }
        __syncthreads();
      }
    }
    if (in_lds)
      for (int64_t t = lane; t < len; t += kWave) col[beg + t] = sh[t];
    __syncthreads();
  }
}

// The one layout of the scratch (common.h Carver; the members are the regions in order): cell keys and ids before and
// after the sort, the centres in cell order, the row lengths, the scan's tile sums and their offsets (scan.h), the
// sort's own scratch.
struct PairsWs {
  u64* keys; int* idx; u64* skeys; int* sidx; Rec* rec; int* counts; int64_t *sums, *offs; char* sort_tmp;
  int64_t sort_tmp_bytes, total;
};
PairsWs pairs_layout(int64_t n, void* ws) {
  const int64_t q = n > 0 ? n : 1, tmp = radix_sort_ws_bytes(q, 8, true);
  Carver c(ws);
  return {c.take<u64>(q), c.take<int>(q), c.take<u64>(q), c.take<int>(q), c.take<Rec>(q),
          c.take<int>(q), c.take<int64_t>(scan_tiles(q)), c.take<int64_t>(scan_tiles(q) + 1), c.take(tmp), tmp, c.total()};
}

int pairs_check(const char* what, int64_t n, float radius, int64_t ws_bytes) {
  LIDAL_REQUIRE(n >= 0 && n <= 0x7FFFFFFF, "%s: n must be in 0..2^31 - 1", what);
  LIDAL_REQUIRE(radius > 0.f && radius <= 3.402823466e38f, "%s: the radius must be finite and positive", what);
  LIDAL_REQUIRE(radius >= 0x1p-60f, "%s: a radius below 2^-60 is not served (squares of such differences underflow)",
                what);
  LIDAL_REQUIRE(ws_bytes >= pairs_layout(n, nullptr).total, "%s: workspace too small", what);
  return 0;
}

// cell keys, the sort, the centres in cell order: what both passes read.  Each pass makes its own, so the fill does not
// depend on what the workspace held between the two calls.
int pairs_prepare(const float* centers, int64_t n, float radius, const PairsWs& w, int* status, hipStream_t s) {
  rp_keys_kernel<<<(unsigned)cdiv(n, RP_BLOCK), RP_BLOCK, 0, s>>>(centers, n, cell_edge(radius), w.keys, w.idx, status);
  LIDAL_CHECK_LAUNCH("radius_pairs_keys");
  if (int rc = radix_sort(w.keys, w.idx, w.skeys, w.sidx, n, 8, 63, w.sort_tmp, w.sort_tmp_bytes, s)) return rc;
  records_kernel<false><<<(unsigned)cdiv(n, RP_BLOCK), RP_BLOCK, 0, s>>>(centers, n, w.sidx, nullptr, w.rec,
                                                                          nullptr);
  LIDAL_CHECK_LAUNCH("radius_pairs_records");
  return 0;
}

}  // namespace

extern "C" int64_t lidal_radius_pairs_workspace_bytes(int64_t n) { return pairs_layout(n, nullptr).total; }

extern "C" int lidal_radius_pairs_count(const float* centers, int64_t n, float radius, int64_t* row_ptr,
                                        int32_t* status_dev, void* ws, int64_t ws_bytes, void* stream) {
  if (int rc = pairs_check("radius_pairs_count", n, radius, ws_bytes)) return rc;
  hipStream_t s = (hipStream_t)stream;
  LIDAL_HIP(hipMemsetAsync(status_dev, 0, sizeof(int32_t), s));
  if (n == 0) {
    LIDAL_HIP(hipMemsetAsync(row_ptr, 0, sizeof(int64_t), s));
    return 0;
  }
  const PairsWs w = pairs_layout(n, ws);
  if (int rc = pairs_prepare(centers, n, radius, w, status_dev, s)) return rc;
  rp_pairs_kernel<false><<<capped(cdiv(n, RP_WAVES)), RP_BLOCK, 0, s>>>(w.skeys, w.rec, n, radius, w.counts, nullptr,
                                                                        nullptr);
  LIDAL_CHECK_LAUNCH("radius_pairs_count");
  // counts i32 [n] -> row_ptr i64 [n + 1]: exclusive, i64 sums (the pairs of a board can exceed an int), the total last
  return tiled_scan<int64_t, false, true>(w.counts, n, w.sums, w.offs, row_ptr, s);
}

extern "C" int lidal_radius_pairs_fill(const float* centers, int64_t n, float radius, const int64_t* row_ptr,
                                       int32_t* col, void* ws, int64_t ws_bytes, void* stream) {
  if (int rc = pairs_check("radius_pairs_fill", n, radius, ws_bytes)) return rc;
  if (n < 2) return 0;                              // no pairs
  hipStream_t s = (hipStream_t)stream;
  const PairsWs w = pairs_layout(n, ws);
  if (int rc = pairs_prepare(centers, n, radius, w, nullptr, s)) return rc;
  rp_pairs_kernel<true><<<capped(cdiv(n, RP_WAVES)), RP_BLOCK, 0, s>>>(w.skeys, w.rec, n, radius, nullptr, row_ptr, col);
  LIDAL_CHECK_LAUNCH("radius_pairs_fill");
  rp_sort_rows_kernel<<<capped(n), kWave, 0, s>>>(row_ptr, n, col);
  LIDAL_CHECK_LAUNCH("radius_pairs_sort_rows");
  return 0;
}
