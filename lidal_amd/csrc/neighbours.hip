// Fixed-radius neighbour lists of a centre array for gfx950: which supervoxel centres lie within `radius` of each other,
// as a CSR table (row_ptr i64 [n + 1], col i32).  It replaces the distance work of the greedy selection
// (score/sv_level/LiDAL.py:225-325 of the reference, lidal_amd/score/selection.py: select_indexed); which hit the
// reference's loop meets FIRST stays on the host, what a hit IS is this table.
//
// THE TABLE.  Row i lists every j != i for which the reference's own expression is true,
//     np.sqrt(np.square(c[i] - c[j]).sum()) < radius
// on f32 rows: f32 differences, f32 squares, the f32 sum ((dx^2 + dy^2) + dz^2) (numpy adds three values in order), the
// correctly rounded f32 square root, then a strict compare.  The root is kept: for (0,0,0) and (3, nextafter(4,0), 0) the
// squared distance 24.999998 is below 25 while its rounded root is exactly 5.0, and the reference says "not within 5 m".
// Differences, products and sums are written with __fsub_rn / __fmul_rn / __fadd_rn, so nothing is contracted whatever
// the flags (the unit is built with -ffp-contract=off as well, lidal_amd/build.py); the root is sqrtf, which hipcc
// expands to the correctly rounded sequence -- not __fsqrt_rn, which without OCML_BASIC_ROUNDED_OPERATIONS is the
// native, not correctly rounded, instruction.  fl(a - b) = -fl(b - a) and only squares follow, so the table is symmetric.
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
// The cells (x, y, z - 1 .. z + 1) are contiguous in key order, so 9 range look-ups (18 binary searches, one lane each)
// cover a query's 27 cells.
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
#include <cmath>

#include "common.h"
#include "grid.h"

using namespace lidal;
using namespace lidal::grid;

namespace {

constexpr int RP_BLOCK = 256;
constexpr int RP_WAVES = RP_BLOCK / kWave;         // query centres per workgroup, one wave each
constexpr int RP_MAX_BLOCKS = 1 << 20;             // launches are grid-stride loops: n may reach 2^31 - 1
constexpr int RP_SORT_LDS = 1024;                  // the longest row a wave sorts in LDS
constexpr int RP_SCAN_ITEMS = 8;
constexpr int RP_SCAN_TILE = RP_BLOCK * RP_SCAN_ITEMS;
constexpr int64_t kFieldMax = (1ll << kCellBits) - 1;

struct __attribute__((aligned(16))) CentreRec { float x, y, z; int idx; };

// the reference's expression (header comment)
__device__ __forceinline__ bool within(const CentreRec& a, const CentreRec& b, float radius) {
  const float dx = __fsub_rn(a.x, b.x), dy = __fsub_rn(a.y, b.y), dz = __fsub_rn(a.z, b.z);
  const float s = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
  return sqrtf(s) < radius;
}

__device__ __forceinline__ bool finite_f32(float v) { return fabsf(v) <= 3.402823466e38f; }      // false for NaN

__global__ void __launch_bounds__(RP_BLOCK) rp_keys_kernel(const float* __restrict__ centers, int64_t n, double cell,
                                                           uint64_t* __restrict__ keys, int* __restrict__ idx,
                                                           int* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = centers[i * 3 + 0], y = centers[i * 3 + 1], z = centers[i * 3 + 2];
  uint64_t key = 0;                                 // the parking cell: every field 0
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

__global__ void __launch_bounds__(RP_BLOCK) rp_records_kernel(const float* __restrict__ centers, int64_t n,
                                                              const int* __restrict__ sidx,
                                                              CentreRec* __restrict__ rec) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  const int64_t j = sidx[q];
  CentreRec r;
  r.x = centers[j * 3 + 0]; r.y = centers[j * 3 + 1]; r.z = centers[j * 3 + 2]; r.idx = (int)j;
  rec[q] = r;
}

// first position in the ascending keys[0, n) whose key is >= target: at most 32 halvings
__device__ __forceinline__ int lower_bound(const uint64_t* __restrict__ keys, int64_t n, uint64_t target) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < target) lo = mid + 1; else hi = mid;
  }
  return (int)lo;                                   // n <= 2^31 - 1
}

// FILL = false: counts[i] = length of row i.  FILL = true: col[row_ptr[i] ..) = row i in cell order.
template <bool FILL>
__global__ void __launch_bounds__(RP_BLOCK)
rp_pairs_kernel(const uint64_t* __restrict__ skeys, const CentreRec* __restrict__ rec, int64_t n, float radius,
                int* __restrict__ counts, const int64_t* __restrict__ row_ptr, int* __restrict__ col) {
  const int lane = lane_id();
  for (int64_t q = (int64_t)blockIdx.x * RP_WAVES + (threadIdx.x >> 6); q < n; q += (int64_t)gridDim.x * RP_WAVES) {
    const uint64_t key = skeys[q];                  // (q, and everything derived from it alone, is uniform in the wave)
    const CentreRec me = rec[q];
    if (key == 0) {                                 // parked: no pairs
      if (!FILL && lane == 0) counts[me.idx] = 0;
      continue;
    }
    int64_t cx, cy, cz;
    cell_unpack(key, &cx, &cy, &cz);
    // lanes 0..8: where run (dx, dy) begins; lanes 9..17: where it ends.  A probe keeps to the field values
    // 1 .. 2^21 - 1 of in-range cells: it never forms a key with a zero field (the parking cell) nor carries into the
    // next field.
    int bound = 0;
    if (lane < 18) {
      const int r = lane < 9 ? lane : lane - 9;
      const int64_t fx = cx + kBias + (r / 3 - 1), fy = cy + kBias + (r % 3 - 1), fz = cz + kBias;
      if (fx >= 1 && fx <= kFieldMax && fy >= 1 && fy <= kFieldMax) {
        const int64_t z0 = fz - 1 >= 1 ? fz - 1 : 1, z1 = fz + 1 <= kFieldMax ? fz + 1 : kFieldMax;
        const uint64_t xy = ((uint64_t)fx << (2 * kCellBits)) | ((uint64_t)fy << kCellBits);
        bound = lower_bound(skeys, n, lane < 9 ? (xy | (uint64_t)z0) : (xy | (uint64_t)z1) + 1);
      }
    }
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
          const CentreRec o = rec[t];
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

// ---------------------------------------------------------------- counts i32 [n] -> row_ptr i64 [n + 1], three launches
// (the form of vccs.hip's scan of head flags, exclusive and with i64 sums: the pairs of a board can exceed an int)
__device__ __forceinline__ int64_t block_exclusive(int64_t v, int64_t* sh, int64_t* total) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int o = 1; o < RP_BLOCK; o <<= 1) {
    const int64_t t = tid >= o ? sh[tid - o] : 0;
    __syncthreads();
    sh[tid] += t;
    __syncthreads();
  }
  const int64_t incl = sh[tid];
  if (total != nullptr) *total = sh[RP_BLOCK - 1];
  __syncthreads();
  return incl - v;
}

__global__ void __launch_bounds__(RP_BLOCK) rp_scan_sums_kernel(const int* __restrict__ counts, int64_t n,
                                                                int64_t* __restrict__ sums) {
  __shared__ int64_t sh[RP_BLOCK];
  const int64_t base = (int64_t)blockIdx.x * RP_SCAN_TILE + (int64_t)threadIdx.x * RP_SCAN_ITEMS;
  int64_t mine = 0;
  for (int j = 0; j < RP_SCAN_ITEMS; ++j)
    if (base + j < n) mine += counts[base + j];
  int64_t total;
  block_exclusive(mine, sh, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// sums[nb] -> their exclusive scan in place and the grand total in sums[nb], by one block
__global__ void __launch_bounds__(RP_BLOCK) rp_scan_top_kernel(int64_t* __restrict__ sums, int nb) {
  __shared__ int64_t sh[RP_BLOCK];
  int64_t carry = 0;
  for (int base = 0; base < nb; base += RP_BLOCK) {
    const int i = base + (int)threadIdx.x;
    const int64_t v = i < nb ? sums[i] : 0;
    int64_t total;
    const int64_t ex = block_exclusive(v, sh, &total);
    if (i < nb) sums[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) sums[nb] = carry;
}

__global__ void __launch_bounds__(RP_BLOCK) rp_scan_apply_kernel(const int* __restrict__ counts, int64_t n,
                                                                 const int64_t* __restrict__ sums, int nb,
                                                                 int64_t* __restrict__ row_ptr) {
  __shared__ int64_t sh[RP_BLOCK];
  const int64_t base = (int64_t)blockIdx.x * RP_SCAN_TILE + (int64_t)threadIdx.x * RP_SCAN_ITEMS;
  int c[RP_SCAN_ITEMS];
  int64_t mine = 0;
  for (int j = 0; j < RP_SCAN_ITEMS; ++j) {
    c[j] = base + j < n ? counts[base + j] : 0;
    mine += c[j];
  }
  int64_t run = sums[blockIdx.x] + block_exclusive(mine, sh, nullptr);
  for (int j = 0; j < RP_SCAN_ITEMS; ++j) {
    if (base + j < n) row_ptr[base + j] = run;
    run += c[j];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) row_ptr[n] = sums[nb];
}

// The one layout of the scratch (common.h Carver; the members are the regions in order): cell keys and ids before and
// after the sort, the centres in cell order, the row lengths, the scan's block sums, the sort's own scratch.
struct PairsWs {
  uint64_t* keys; int* idx; uint64_t* skeys; int* sidx; CentreRec* rec; int* counts; int64_t* sums; char* sort_tmp;
  int64_t sort_tmp_bytes, total;
};
PairsWs pairs_layout(int64_t n, void* ws) {
  const int64_t q = n > 0 ? n : 1, tmp = radix_sort_ws_bytes(q, 8, true);
  Carver c(ws);
  return {c.take<uint64_t>(q), c.take<int>(q), c.take<uint64_t>(q), c.take<int>(q), c.take<CentreRec>(q),
          c.take<int>(q), c.take<int64_t>(cdiv(q, RP_SCAN_TILE) + 1), c.take(tmp), tmp, c.total()};
}

unsigned capped(int64_t blocks) { return (unsigned)(blocks < RP_MAX_BLOCKS ? blocks : RP_MAX_BLOCKS); }

int pairs_check(const char* what, int64_t n, float radius, int64_t ws_bytes) {
  LIDAL_REQUIRE(n >= 0 && n <= 0x7FFFFFFF, "%s: n must be in 0..2^31 - 1", what);
  LIDAL_REQUIRE(radius > 0.f && radius <= 3.402823466e38f, "%s: the radius must be finite and positive", what);
  LIDAL_REQUIRE(radius >= 0x1p-60f, "%s: a radius below 2^-60 is not served (squares of such differences underflow)",
                what);
  LIDAL_REQUIRE(ws_bytes >= pairs_layout(n, nullptr).total, "%s: workspace too small", what);
  return 0;
}

// the smallest power of two >= radius, exactly
double cell_edge(float radius) {
  int e;
  const double m = frexp((double)radius, &e);       // radius = m 2^e, m in [0.5, 1)
  return m == 0.5 ? (double)radius : ldexp(1.0, e);
}

// cell keys, the sort, the centres in cell order: what both passes read.  Each pass makes its own, so the fill does not
// depend on what the workspace held between the two calls.
int pairs_prepare(const float* centers, int64_t n, float radius, const PairsWs& w, int* status, hipStream_t s) {
  rp_keys_kernel<<<(unsigned)cdiv(n, RP_BLOCK), RP_BLOCK, 0, s>>>(centers, n, cell_edge(radius), w.keys, w.idx, status);
  LIDAL_CHECK_LAUNCH("radius_pairs_keys");
  if (int rc = radix_sort(w.keys, w.idx, w.skeys, w.sidx, n, 8, 63, w.sort_tmp, w.sort_tmp_bytes, s)) return rc;
  rp_records_kernel<<<(unsigned)cdiv(n, RP_BLOCK), RP_BLOCK, 0, s>>>(centers, n, w.sidx, w.rec);
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
  const int nb = (int)cdiv(n, RP_SCAN_TILE);
  rp_scan_sums_kernel<<<(unsigned)nb, RP_BLOCK, 0, s>>>(w.counts, n, w.sums);
  LIDAL_CHECK_LAUNCH("radius_pairs_scan_sums");
  rp_scan_top_kernel<<<1, RP_BLOCK, 0, s>>>(w.sums, nb);
  LIDAL_CHECK_LAUNCH("radius_pairs_scan_top");
  rp_scan_apply_kernel<<<(unsigned)nb, RP_BLOCK, 0, s>>>(w.counts, n, w.sums, nb, row_ptr);
  LIDAL_CHECK_LAUNCH("radius_pairs_scan_apply");
  return 0;
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
