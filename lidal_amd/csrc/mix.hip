// Mixed training samples for gfx950: the rows of two scans selected by inclination band and azimuth sector (LaserMix /
// PolarMix style) plus rotated copies of the rows of chosen classes, written as one concatenated point list (DESIGN.md
// section 18).  The definition is the project's own and is restated in numpy by tests/mix_ref.py; include/lidal_amd.h
// states it next to lidal_mix_scans.
//
// THE PREDICATE.  r = sqrtf(fl(fl(x*x) + fl(y*y))), band = #{ j : z >= fl(tans[j] * r) }, the sector by the signs of two
// cross products: products, sums and differences are __fmul_rn / __fadd_rn / __fsub_rn (and the unit is built with
// -ffp-contract=off, lidal_amd/build.py), the root is sqrtf for the reason csrc/neighbours.hip gives.  No atan, no atan2:
// every operation is correctly rounded, so numpy computes the same bits.  NaN compares false, as there.
//
// THE SLOT SPACE.  Mix m owns na + nb * (1 + n_rot) slots: one per row of A, one per row of B, and one per row of B and
// rotation.  Blocks of 256 slots are laid out per (mix, part), so a block reads one descriptor and one part's predicate:
//   1. mix_count_kernel    per-block kept count (wave ballots, summed through LDS)
//   2. scan_counts_kernel  the exclusive scan of the counts (scan.h)
//   3. mix_write_kernel    the predicate again; row -> offset[block] + rank inside the block; block 0 also writes
//                          point_ptr and parts from the scanned offsets of the parts' first blocks
// No atomics and no memset: every word that is read was written by the same call.
#include <cmath>
#include <cstring>

#include "common.h"
#include "scan.h"

using namespace lidal;

namespace {

constexpr int kMixBlock = 256;
constexpr int kMixParts = LIDAL_MIX_MAX * LIDAL_MIX_PARTS;

// first block of every (mix, part), the total at the end; a part without rows has no blocks.  By value in the kernel
// arguments (780 bytes); the descriptors themselves (8 KiB at 32 mixes) are uploaded.
struct MixBlocks {
  int block0[kMixParts + 1];
  int n_mixes;
};

// the (mix, part) that owns block `blk`: the last entry with block0 <= blk (empty parts share their successor's block0)
__device__ __forceinline__ int part_of(const MixBlocks& L, int blk) {
  int lo = 0, hi = L.n_mixes * LIDAL_MIX_PARTS;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (L.block0[mid] <= blk) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int cell_of(const lidal_mix_desc& d, float x, float y, float z) {
  const float r = sqrtf(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)));
  int band = 0;
  for (int j = 0; j < d.n_tans; ++j) band += (z >= __fmul_rn(d.tans[j], r)) ? 1 : 0;
  const bool inw = d.has_wedge != 0 &&
                   __fsub_rn(__fmul_rn(d.wedge[0], y), __fmul_rn(d.wedge[1], x)) >= 0.0f &&
                   __fsub_rn(__fmul_rn(d.wedge[2], y), __fmul_rn(d.wedge[3], x)) < 0.0f;
  return band + (inw ? d.n_tans + 1 : 0);
}

// One slot: part `part` of the mix `d`, local row `r`.  Returns whether the row is kept and its input row in *src.
__device__ __forceinline__ bool slot_kept(const lidal_mix_desc& d, int part, long long r, const float* __restrict__ xyz,
                                          const int64_t* __restrict__ labels, long long* src) {
  const long long n = part == 0 ? d.na : d.nb;
  if (r >= n) return false;
  const long long row = (part == 0 ? d.a0 : d.b0) + r;
  *src = row;
  if (part >= 2) {                                   // a paste: by class, whatever the cell
    const int64_t l = labels[row];
    return l >= 0 && l < 64 && ((d.paste_classes >> l) & 1ull);
  }
  const int cell = cell_of(d, xyz[row * 3 + 0], xyz[row * 3 + 1], xyz[row * 3 + 2]);
  return ((part == 0 ? d.take_a : d.take_b) >> cell) & 1ull;
}

__global__ void __launch_bounds__(kMixBlock) mix_count_kernel(MixBlocks L, const lidal_mix_desc* __restrict__ desc,
                                                              const float* __restrict__ xyz,
                                                              const int64_t* __restrict__ labels,
                                                              int* __restrict__ counts) {
  __shared__ int wave_cnt[kMixBlock / 64];
  const int t = part_of(L, blockIdx.x), part = t % LIDAL_MIX_PARTS;
  const lidal_mix_desc& d = desc[t / LIDAL_MIX_PARTS];
  const long long r = (long long)(blockIdx.x - L.block0[t]) * kMixBlock + threadIdx.x;
  long long src;
  const bool keep = slot_kept(d, part, r, xyz, labels, &src);
  const unsigned long long m = __ballot(keep);
  if (lane_id() == 0) wave_cnt[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < kMixBlock / 64; ++w) c += wave_cnt[w];
    counts[blockIdx.x] = c;
  }
}

// grid = max(blocks, 1): block 0 writes point_ptr and parts even when no mix has a row
__global__ void __launch_bounds__(kMixBlock) mix_write_kernel(MixBlocks L, int n_blocks,
                                                              const lidal_mix_desc* __restrict__ desc,
                                                              const float* __restrict__ xyz,
                                                              const float* __restrict__ intensity,
                                                              const int64_t* __restrict__ labels,
                                                              const int64_t* __restrict__ offsets,
                                                              float* __restrict__ out_xyz, float* __restrict__ out_intensity,
                                                              int64_t* __restrict__ out_labels, int64_t* __restrict__ out_src,
                                                              int64_t* __restrict__ point_ptr /*[M + 1]*/,
                                                              int64_t* __restrict__ parts /*[M, 6]*/) {
  __shared__ int wave_cnt[kMixBlock / 64];
  if (blockIdx.x == 0) {
    const int np = L.n_mixes * LIDAL_MIX_PARTS;
    for (int i = threadIdx.x; i < np; i += kMixBlock) parts[i] = offsets[L.block0[i + 1]] - offsets[L.block0[i]];
    for (int i = threadIdx.x; i <= L.n_mixes; i += kMixBlock) point_ptr[i] = offsets[L.block0[i * LIDAL_MIX_PARTS]];
  }
  if ((int)blockIdx.x >= n_blocks) return;
  const int t = part_of(L, blockIdx.x), part = t % LIDAL_MIX_PARTS;
  const lidal_mix_desc& d = desc[t / LIDAL_MIX_PARTS];
  const long long r = (long long)(blockIdx.x - L.block0[t]) * kMixBlock + threadIdx.x;
  long long src = 0;
  const bool keep = slot_kept(d, part, r, xyz, labels, &src);
  int total;
  const int rank = block_rank<kMixBlock>(keep, wave_cnt, &total);
  if (!keep) return;
  const int64_t o = offsets[blockIdx.x] + rank;
  float x = xyz[src * 3 + 0], y = xyz[src * 3 + 1];
  if (part >= 2) {
    const float c = d.rot[2 * (part - 2)], s = d.rot[2 * (part - 2) + 1];
    const float xr = __fsub_rn(__fmul_rn(c, x), __fmul_rn(s, y));
    y = __fadd_rn(__fmul_rn(s, x), __fmul_rn(c, y));
    x = xr;
  }
  out_xyz[o * 3 + 0] = x;
  out_xyz[o * 3 + 1] = y;
  out_xyz[o * 3 + 2] = xyz[src * 3 + 2];
  out_intensity[o] = intensity[src];
  if (out_labels != nullptr) out_labels[o] = labels[src];
  out_src[o] = src;
}

// per-block counts | their scan | the uploaded descriptors
struct MixWs {
  int* counts; int64_t* offsets; lidal_mix_desc* desc;
  int64_t total;
};
MixWs mix_layout(int64_t n_slots, int n_mixes, void* ws) {
  const int64_t q = n_slots > 0 ? n_slots : 0, nm = n_mixes > 0 ? n_mixes : 1;
  const int64_t blocks = cdiv(q, kMixBlock) + nm * LIDAL_MIX_PARTS;      // sum of ceil(rows / 256) over the parts <= this
  Carver c(ws);
  return {c.take<int>(blocks), c.take<int64_t>(blocks + 1), c.take<lidal_mix_desc>(nm), c.total()};
}

}  // namespace

extern "C" int64_t lidal_mix_scans_workspace_bytes(int64_t n_slots, int n_mixes) {
  return mix_layout(n_slots, n_mixes, nullptr).total;
}

extern "C" int lidal_mix_scans(const float* xyz, const float* intensity, const int64_t* labels, int64_t p_total,
                               const lidal_mix_desc* mixes_host, int n_mixes, float* out_xyz, float* out_intensity,
                               int64_t* out_labels, int64_t* out_src, int64_t* counts_dev, void* ws, int64_t ws_bytes,
                               void* stream) {
  hipStream_t s = (hipStream_t)stream;
  static_assert(sizeof(lidal_mix_desc) == 256, "lidal_mix_desc is 256 bytes");
  LIDAL_REQUIRE(n_mixes >= 1 && n_mixes <= LIDAL_MIX_MAX, "mix_scans: 1..%d mixes, not %d", LIDAL_MIX_MAX, n_mixes);
  // (an input without rows has no address: nothing is read or kept then, and the label pointers are not compared)
  LIDAL_REQUIRE(p_total >= 0 && (p_total == 0 || (labels == nullptr) == (out_labels == nullptr)),
                "mix_scans: labels and out_labels come together");
  MixBlocks L;
  memset(&L, 0, sizeof(L));
  L.n_mixes = n_mixes;
  long long slots = 0, blocks = 0;
  for (int m = 0; m < n_mixes; ++m) {
    const lidal_mix_desc& d = mixes_host[m];
    LIDAL_REQUIRE(d.na >= 0 && d.a0 >= 0 && d.a0 <= p_total && d.na <= p_total - d.a0 && d.nb >= 0 && d.b0 >= 0 &&
                  d.b0 <= p_total && d.nb <= p_total - d.b0, "mix_scans: mix %d: rows outside the %lld of the input", m,
                  (long long)p_total);
    LIDAL_REQUIRE(d.n_tans >= 0 && d.n_tans <= LIDAL_MIX_MAX_TANS, "mix_scans: mix %d: %d boundaries (at most %d)", m,
                  d.n_tans, LIDAL_MIX_MAX_TANS);
    for (int j = 0; j < d.n_tans; ++j)
      LIDAL_REQUIRE(std::isfinite(d.tans[j]) && (j == 0 || d.tans[j] >= d.tans[j - 1]),
                    "mix_scans: mix %d: the boundaries must be finite and ascending", m);
    LIDAL_REQUIRE(d.n_rot >= 0 && d.n_rot <= LIDAL_MIX_MAX_ROT, "mix_scans: mix %d: %d rotations (at most %d)", m, d.n_rot,
                  LIDAL_MIX_MAX_ROT);
    LIDAL_REQUIRE(d.n_rot == 0 || labels != nullptr || p_total == 0, "mix_scans: mix %d: a paste needs labels", m);
    const int cells = (d.n_tans + 1) * (d.has_wedge ? 2 : 1);
    LIDAL_REQUIRE(cells == 64 || ((d.take_a | d.take_b) >> cells) == 0,
                  "mix_scans: mix %d: a mask bit at or above the %d cells", m, cells);
    for (int k = 0; k < LIDAL_MIX_PARTS; ++k) {
      const long long rows = k == 0 ? d.na : (k - 1 <= d.n_rot ? d.nb : 0);
      L.block0[m * LIDAL_MIX_PARTS + k] = (int)blocks;
      slots += rows;
      blocks += cdiv(rows, kMixBlock);
      LIDAL_REQUIRE(slots < (1ll << 30), "mix_scans: %lld slots in one call (fewer than 2^30)", slots);
    }
  }
  for (int t = n_mixes * LIDAL_MIX_PARTS; t <= kMixParts; ++t) L.block0[t] = (int)blocks;
  const MixWs w = mix_layout(slots, n_mixes, ws);
  LIDAL_REQUIRE(ws_bytes >= w.total, "mix_scans ws too small");
  LIDAL_HIP(hipMemcpyAsync(w.desc, mixes_host, sizeof(lidal_mix_desc) * (size_t)n_mixes, hipMemcpyHostToDevice, s));
  if (blocks > 0) {
    mix_count_kernel<<<(unsigned)blocks, kMixBlock, 0, s>>>(L, w.desc, xyz, labels, w.counts);
    LIDAL_CHECK_LAUNCH("mix_count");
  }
  scan_counts_kernel<<<1, 1024, 0, s>>>(w.counts, blocks, w.offsets);
  LIDAL_CHECK_LAUNCH("scan_counts");
  mix_write_kernel<<<(unsigned)(blocks > 0 ? blocks : 1), kMixBlock, 0, s>>>(
      L, (int)blocks, w.desc, xyz, intensity, labels, w.offsets, out_xyz, out_intensity, out_labels, out_src, counts_dev,
      counts_dev + n_mixes + 1);
  LIDAL_CHECK_LAUNCH("mix_write");
  return 0;
}
