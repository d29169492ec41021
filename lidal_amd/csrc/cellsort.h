// The fixed-radius walk over records sorted by cell key (grid.h: the 63-bit key), shared by the units that probe the 27
// cells around a query (neighbours.hip: the pairs of a centre array; cluster.hip: the edges of Euclidean clustering), and
// the small look-ups vccs.hip shares with them (lower_bound, segment_of, raise).  What a unit does with a hit -- count
// it, rank it into a row, unite two rows -- stays written out in the unit.
//
// THE PREDICATE.  within(a, b, radius) is the reference's own expression on f32 rows,
//     np.sqrt(np.square(c[i] - c[j]).sum()) < radius
// f32 differences, f32 squares, the f32 sum ((dx^2 + dy^2) + dz^2) (numpy adds three values in order), the correctly
// rounded f32 square root, then a strict compare.  The root is kept: for (0,0,0) and (3, nextafter(4,0), 0) the squared
// distance 24.999998 is below 25 while its rounded root is exactly 5.0, and the reference says "not within 5 m".
// Differences, products and sums are written with __fsub_rn / __fmul_rn / __fadd_rn, so nothing is contracted whatever
// the flags (the units are built with -ffp-contract=off as well, lidal_amd/build.py); the root is sqrtf, which hipcc
// expands to the correctly rounded sequence -- not __fsqrt_rn, which without OCML_BASIC_ROUNDED_OPERATIONS is the
// native, not correctly rounded, instruction.  fl(a - b) = -fl(b - a) and only squares follow, so it is symmetric.
//
// THE PROBE.  With a cell edge that is a power of two >= radius (cell_edge), the 27 cells around a query's own hold
// every record the predicate accepts: the proof is in the header of neighbours.hip ("THE GRID").  The cells
// (x, y, z - 1 .. z + 1) are contiguous in key order, so 9 runs cover them; run_bound finds their 18 ends, one lane each.
#pragma once
#include <cmath>

#include "common.h"
#include "grid.h"

namespace lidal {
namespace cellsort {
namespace {

using namespace lidal::grid;

typedef unsigned long long u64;

constexpr int kMaxBlocks = 1 << 20;                // the wave-per-query launches are grid-stride loops
constexpr int64_t kFieldMax = (1ll << kCellBits) - 1;

struct __attribute__((aligned(16))) Rec { float x, y, z; int idx; };

__device__ __forceinline__ bool within(const Rec& a, const Rec& b, float radius) {
  const float dx = __fsub_rn(a.x, b.x), dy = __fsub_rn(a.y, b.y), dz = __fsub_rn(a.z, b.z);
  const float s = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
  return sqrtf(s) < radius;
}

__device__ __forceinline__ bool finite_f32(float v) { return fabsf(v) <= 3.402823466e38f; }      // false for NaN

// the error word of a status array (word 0) only ever grows
__device__ __forceinline__ void raise(long long* status, int word) { atomicMax((u64*)&status[0], (u64)word); }

// first position in the ascending keys[lo, hi) whose key is >= target, hi if there is none: at most 32 halvings
__device__ __forceinline__ int lower_bound(const u64* __restrict__ keys, int lo, int hi, u64 target) {
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < target) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the last s in [0, n_seg) with ptr[s] <= i, for an ascending ptr with ptr[0] <= i: at most 32 halvings
__device__ __forceinline__ int segment_of(const int64_t* __restrict__ ptr, int n_seg, int64_t i) {
  int lo = 0, hi = n_seg;
  for (int it = 0; it < 32 && hi - lo > 1; ++it) {
    const int mid = lo + ((hi - lo) >> 1);
    if (ptr[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// The nine cell runs around the cell `key` of a query, inside the segment skeys[seg_lo, seg_hi) of ascending keys: lane
// r < 9 returns where run (dx, dy) = (r / 3 - 1, r % 3 - 1) begins, lane 9 + r where it ends; every other lane, and both
// lanes of a run outside the key range, return seg_lo.  A probe keeps to the field values 1 .. 2^21 - 1 of in-range
// cells: it never forms a key with a zero field (the parking cell) nor carries into the next field.
__device__ __forceinline__ int run_bound(const u64* __restrict__ skeys, int seg_lo, int seg_hi, u64 key, int lane) {
  int64_t cx, cy, cz;
  cell_unpack(key, &cx, &cy, &cz);
  int bound = seg_lo;
  if (lane < 18) {
    const int r = lane < 9 ? lane : lane - 9;
    const int64_t fx = cx + kBias + (r / 3 - 1), fy = cy + kBias + (r % 3 - 1), fz = cz + kBias;
    if (fx >= 1 && fx <= kFieldMax && fy >= 1 && fy <= kFieldMax) {
      const int64_t z0 = fz - 1 >= 1 ? fz - 1 : 1, z1 = fz + 1 <= kFieldMax ? fz + 1 : kFieldMax;
      const u64 xy = ((u64)fx << (2 * kCellBits)) | ((u64)fy << kCellBits);
      bound = lower_bound(skeys, seg_lo, seg_hi, lane < 9 ? (xy | (u64)z0) : (xy | (u64)z1) + 1);
    }
  }
  return bound;
}

// the rows in sorted order: one 16-byte record each and, with KEYS, the row's key (a unit that launches neither form
// gets neither kernel)
template <bool KEYS>
__global__ void __launch_bounds__(256) records_kernel(const float* __restrict__ xyz, int64_t n,
                                                      const int* __restrict__ sidx, const u64* __restrict__ key,
                                                      Rec* __restrict__ rec, u64* __restrict__ skey) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  const int64_t j = sidx[q];
  Rec r;
  r.x = xyz[j * 3 + 0]; r.y = xyz[j * 3 + 1]; r.z = xyz[j * 3 + 2]; r.idx = (int)j;
  rec[q] = r;
  if (KEYS) skey[q] = key[j];
}

// the smallest power of two >= radius, exactly
inline double cell_edge(float radius) {
  int e;
  const double m = frexp((double)radius, &e);       // radius = m 2^e, m in [0.5, 1)
  return m == 0.5 ? (double)radius : ldexp(1.0, e);
}

inline unsigned capped(int64_t blocks) { return (unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks); }

}  // namespace
}  // namespace cellsort
}  // namespace lidal
