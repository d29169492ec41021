// The uniform-grid buffer that lidal_nn_grid_build (score.hip) writes: its layout, shared by the units that read it
// (score.hip: the inter-frame matches; redal.hip: the k-nearest-neighbour search).
#pragma once

#include "common.h"

namespace lidal {
namespace grid {

// grid buffer: [header 64 B][table 12*cap][sorted_keys 8*p][sorted_idx 4*p]
struct GridHeader {
  int64_t p;
  int64_t cap;
  double cell;
  double inv_cell_unused;
};

struct __attribute__((aligned(16))) GridRec { unsigned long long key; double x, y, z; int idx; int pad; };

struct GridView {
  TableView t;
  const uint64_t* keys;
  const int* idx;
  const struct GridRec* rec;     // the points in cell order, one 48-byte record each (round 5: a candidate -- its cell key, its
                                 // coordinates, its id -- is ONE access instead of three arrays and a gathered point)
  int64_t p;
  double cell;
};
// byte offsets inside a grid buffer (after the 64-byte header) for p points and capacity cap:
//   keys u64 [cap] | vals i32 [cap] | sorted cell keys u64 [p] | sorted point ids i32 [p] | records GridRec [p] |
//   occupancy bitmap u32 [cap / 4] (8 bits per slot, csrc/common.h: most probed cells are empty)
__host__ __device__ inline int64_t grid_off_skeys(int64_t cap) { return cap * 12; }
__host__ __device__ inline int64_t grid_off_sidx(int64_t cap, int64_t q) { return cap * 12 + ((8 * q + 255) / 256) * 256; }
__host__ __device__ inline int64_t grid_off_spts(int64_t cap, int64_t q) { return grid_off_sidx(cap, q) + ((4 * q + 255) / 256) * 256; }
__host__ __device__ inline int64_t grid_off_bits(int64_t cap, int64_t q) { return grid_off_spts(cap, q) + ((48 * q + 255) / 256) * 256; }

constexpr int64_t kBias = 1 << 20;

// The key range.  A cell index is IN RANGE iff floor(v / cell), as a double, lies in [-(2^20 - 1), 2^20 - 1]: it then
// fits its 21-bit field of cell_key with field value >= 1.  Written so that NaN fails (and +-Inf, and anything a cast
// to int64_t could not hold): the test is made on the double, BEFORE any cast.
constexpr int64_t kCellMax = kBias - 1;
__host__ __device__ inline bool cell_in_range(double f) { return f >= -(double)kCellMax && f <= (double)kCellMax; }
// The cell index of coordinate v, or -2^20 (field value 0: the PARKING cell of that axis) when v is out of range.
// The build files an out-of-range point there; a query whose probed cube is in range never forms a key with a zero
// field, so a parked point is a candidate of nobody.
__host__ __device__ inline int64_t cell_index(double v, double cell) {
  const double f = floor(v / cell);
  return cell_in_range(f) ? (int64_t)f : -kBias;
}

__device__ __forceinline__ uint64_t cell_key(int64_t ix, int64_t iy, int64_t iz) {
  return ((uint64_t)(ix + kBias) << 42) | ((uint64_t)(iy + kBias) << 21) | (uint64_t)(iz + kBias);
}

}  // namespace grid
}  // namespace lidal
