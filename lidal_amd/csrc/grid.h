// The uniform-grid buffer that lidal_nn_grid_build (score.hip) writes: its layout, shared by the units that read it
// (score.hip: the inter-frame matches; redal.hip: the k-nearest-neighbour search), and the 63-bit cell key, which
// vccs.hip packs its voxel and seed cells into as well.
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

constexpr int kCellBits = 21;       // a cell key: x << 42 | y << 21 | z, each field the cell index + 2^20
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

__device__ __forceinline__ void cell_unpack(uint64_t key, int64_t* ix, int64_t* iy, int64_t* iz) {
  const uint64_t m = (1ull << kCellBits) - 1;
  *ix = (int64_t)(key >> (2 * kCellBits)) - kBias;
  *iy = (int64_t)((key >> kCellBits) & m) - kBias;
  *iz = (int64_t)(key & m) - kBias;
}

// cell_key with a range check: false, and *key untouched, unless every field value lies in [0, 2^21).  That is the
// whole field: unlike cell_in_range above, value 0 is a cell here (vccs.hip parks nothing: out of range is an error).
__device__ __forceinline__ bool cell_pack(int64_t ix, int64_t iy, int64_t iz, uint64_t* key) {
  const int64_t bx = ix + kBias, by = iy + kBias, bz = iz + kBias, lim = 1ll << kCellBits;
  if (bx < 0 || bx >= lim || by < 0 || by >= lim || bz < 0 || bz >= lim) return false;
  *key = ((uint64_t)bx << (2 * kCellBits)) | ((uint64_t)by << kCellBits) | (uint64_t)bz;
  return true;
}

}  // namespace grid
}  // namespace lidal
