// The uniform-grid buffer that lidal_nn_grid_build (score.hip) writes: its layout, shared by the units that read it
// (score.hip: the inter-frame matches; redal.hip: the k-nearest-neighbour search; icp.hip: the correspondences of a
// registration), the radius-limited nearest-neighbour query over it, and the 63-bit cell key, which vccs.hip packs its
// voxel and seed cells into as well.
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

// The view of a grid buffer of p points and capacity cap (table_capacity(max(p, 1))), as the kernels that query it take it.
__host__ __device__ inline GridView grid_view(const void* grid, int64_t p, int64_t cap, double cell) {
  GridView g;
  char* base = (char*)grid + 64;
  g.t.keys = (unsigned long long*)base;
  g.t.vals = (int*)(base + cap * 8);
  g.t.mask = (uint64_t)cap - 1;
  const int64_t q = p > 0 ? p : 1;
  g.t.bits = (unsigned*)(base + grid_off_bits(cap, q));
  g.t.sbits = nullptr; g.t.hdr = nullptr;
  g.keys = (const uint64_t*)(base + grid_off_skeys(cap));
  g.idx = (const int*)(base + grid_off_sidx(cap, q));
  g.rec = (const GridRec*)(base + grid_off_spts(cap, q));
  g.p = p;
  g.cell = cell;
  return g;
}

// nearest point of the grid's frame among the cells that meet the cube [q - r, q + r]^3 (27 cells when the cell is the
// radius r, at most 8 when it is 2 r: round 4 -- a look-up is a random probe of a hash table, and LiDAR cells are mostly
// empty); returns index or -1, *d2out.  The candidates are a superset of the ball's points either way and ties go to the
// lowest index, so the answer does not depend on the cell size.  One copy for the units that match across frames
// (score.hip: the inter-frame matches; icp.hip: the correspondences of a registration).
__device__ __forceinline__ void grid_scan_cell(const GridView& g, uint64_t key, int start, double qx, double qy, double qz,
                                               double& best, int& arg) {
  for (int64_t s = start; s < g.p; ++s) {
    const GridRec r = g.rec[s];
    if (r.key != key) break;
    const int j = r.idx;
    double ex = r.x - qx, ey = r.y - qy, ez = r.z - qz;
    double d2 = __dadd_rn(__dadd_rn(__dmul_rn(ex, ex), __dmul_rn(ey, ey)), __dmul_rn(ez, ez));
    if (d2 < best || (d2 == best && j < arg)) { best = d2; arg = j; }
  }
}

__device__ __forceinline__ int grid_nearest(const GridView& g, const double* __restrict__ npts,
                                            double qx, double qy, double qz, double r, double* d2out) {
  const double rr = r * (1.0 + 1e-9) + 1e-12;            // (a point at exactly r must not fall off the cube through rounding)
  const double fx0 = floor((qx - rr) / g.cell), fx1 = floor((qx + rr) / g.cell);
  const double fy0 = floor((qy - rr) / g.cell), fy1 = floor((qy + rr) / g.cell);
  const double fz0 = floor((qz - rr) / g.cell), fz1 = floor((qz + rr) / g.cell);
  double best = INFINITY;
  int arg = -1;
  // a query that is NaN, +-Inf or whose cube leaves the key range matches nothing: told on the doubles, before any cast
  // (a saturated bound would make the loops below endless)
  if (!(cell_in_range(fx0) && cell_in_range(fx1) && cell_in_range(fy0) && cell_in_range(fy1) && cell_in_range(fz0) &&
        cell_in_range(fz1))) {
    *d2out = best;
    return arg;
  }
  const int64_t x0 = (int64_t)fx0, x1 = (int64_t)fx1, y0 = (int64_t)fy0, y1 = (int64_t)fy1, z0 = (int64_t)fz0, z1 = (int64_t)fz1;
  // (round 5, measured: probing the eight cells of a query in stages -- eight bitmap words, then the slots, then the values,
  // each stage's loads in flight together -- 287.8 us against this loop's 289.1: the kernel is bound by the ~20 random
  // 64-byte sectors a query touches beyond the L2s, 1.5 GB per launch, not by a thread's dependent chain)
  for (int64_t ix = x0; ix <= x1; ++ix)
    for (int64_t iy = y0; iy <= y1; ++iy)
      for (int64_t iz = z0; iz <= z1; ++iz) {
        uint64_t key = cell_key(ix, iy, iz);
        if (g.t.bits != nullptr) {      // an empty cell is the common answer: told by the bitmap, from the L2s
          const uint64_t b = bit_of(mix_key(key), g.t.mask);
          if (!((g.t.bits[b >> 5] >> (b & 31)) & 1u)) continue;
        }
        int start = table_lookup(g.t, key);
        if (start < 0) continue;
        grid_scan_cell(g, key, start, qx, qy, qz, best, arg);
      }
  *d2out = best;
  return arg;
}

}  // namespace grid
}  // namespace lidal
