// Training labels from the round's selection flags (dataset/sk_dataset.py:106-141,170-171 and dataset/nu_dataset.py:
// 128-160,189-190 of the reference) for gfx950: raw annotation words -> mapped classes, masked by the supervoxels the
// round labeled (flag 1), overridden by last round's predictions inside the pseudo-labeled ones (flag 2), gathered to
// the voxels of the scan.  Everything is an integer, so the result is bit-exact.
//
// Three small launches on one stream, no host read:
//   mark    one workgroup per supervoxel with flag 1 or 2: an atomic OR of a two-bit state per listed point (bit 0:
//           listed by a flag-1 supervoxel, bit 1: by a flag-2 one) into a word array of 16 points per u32.  OR does not
//           depend on the order, so overlapping lists form the union the reference's loop forms and two runs agree.
//   points  16 bytes of the raw stream per lane (4 u32 words or 16 u8), the label table in LDS, the state word of those
//           points, labels_p written.
//   voxels  labels_v[j] = labels_p[unique_idx[j]].
#include <algorithm>

#include "common.h"

using namespace lidal;

namespace {

constexpr int LB_BLOCK = 256;
constexpr int LB_MAXMAP = 1024;          // entries of the label table kept in LDS (260 and 100 in the reference)
constexpr int64_t LB_IGNORE = 255;       // the ignore_index of the loss (train.py:136)

// sk_dataset.py:129-141: supervoxel blockIdx.x with flag 1 (flag 2 where pseudo labels are in use) ORs its bit into the
// state of each point it lists.  A list outside [0, nnz) or a point outside [0, p) is counted and skipped.
__global__ void __launch_bounds__(LB_BLOCK) mark_kernel(const int64_t* __restrict__ sv_ptr,
                                                         const int64_t* __restrict__ sv_idx, int64_t nnz,
                                                         const int64_t* __restrict__ sv_flag, int with_pseudo, int64_t p,
                                                         unsigned* __restrict__ state, int* __restrict__ n_invalid) {
  const int s = blockIdx.x;
  const int64_t f = sv_flag[s];
  const unsigned bit = f == 1 ? 1u : (f == 2 && with_pseudo) ? 2u : 0u;
  if (bit == 0u) return;
  const int64_t beg = sv_ptr[s], end = sv_ptr[s + 1];
  if (beg < 0 || end < beg || end > nnz) {
    if (threadIdx.x == 0) atomicAdd(n_invalid, 1);
    return;
  }
  int bad = 0;
  for (int64_t t = beg + threadIdx.x; t < end; t += LB_BLOCK) {
    const int64_t q = sv_idx[t];
    if (q < 0 || q >= p) {
      ++bad;
      continue;
    }
    atomicOr(&state[q >> 4], bit << (2 * (unsigned)(q & 15)));
  }
  if (bad) atomicAdd(n_invalid, bad);
}

// the label of one point: sk_dataset.py:111-113 (the table; an id beyond it is counted and reads as 255), :133 (255
// unless a flag-1 supervoxel lists the point), :141 (the pseudo label where a flag-2 supervoxel lists it)
__device__ __forceinline__ int64_t point_label(unsigned raw, const int64_t* map, int map_len, bool masked, unsigned st,
                                               const int64_t* __restrict__ pseudo, int64_t i, int& bad) {
  int64_t lab = LB_IGNORE;
  if (raw < (unsigned)map_len) lab = map[raw];
  else ++bad;
  if (masked && !(st & 1u)) lab = LB_IGNORE;
  if (pseudo != nullptr && (st & 2u)) lab = pseudo[i];
  return lab;
}

// VEC points per lane = 16 bytes of raw labels: T = uint32_t (SemanticKITTI: the low half is the class, :111), VEC = 4;
// T = uint8_t (nuScenes), VEC = 16.  `vec` says that raw is 16-byte aligned; the last, partial group of a scan and an
// unaligned stream are read point by point.
template <typename T, int VEC>
__global__ void __launch_bounds__(LB_BLOCK) points_kernel(const T* __restrict__ raw, int64_t p, int vec,
                                                           const int64_t* __restrict__ label_map, int map_len,
                                                           const unsigned* __restrict__ state, int masked,
                                                           const int64_t* __restrict__ pseudo,
                                                           int64_t* __restrict__ labels_p, int* __restrict__ n_invalid) {
  static_assert(sizeof(T) * VEC == 16 && 16 % VEC == 0, "one 16-byte vector of raw labels per lane");
  __shared__ int64_t map[LB_MAXMAP];
  for (int c = threadIdx.x; c < map_len; c += LB_BLOCK) map[c] = label_map[c];
  __syncthreads();
  const int64_t base = ((int64_t)blockIdx.x * LB_BLOCK + threadIdx.x) * VEC;
  if (base >= p) return;
  const int m = p - base < VEC ? (int)(p - base) : VEC;
  T r[VEC];
  if (vec && m == VEC) {
    const uint4 v = *reinterpret_cast<const uint4*>(raw + base);
    __builtin_memcpy(r, &v, 16);
  } else {
#pragma unroll
    for (int j = 0; j < VEC; ++j) r[j] = j < m ? raw[base + j] : (T)0;
  }
  // the two-bit states of points base .. base + VEC - 1: 2 VEC bits of one word (VEC divides 16)
  unsigned st = 0u;
  if (state != nullptr) st = state[base >> 4] >> (2 * (unsigned)(base & 15));
  int bad = 0;
  int64_t out[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    const unsigned id = sizeof(T) == 4 ? ((unsigned)r[j] & 0xFFFFu) : (unsigned)r[j];
    out[j] = j < m ? point_label(id, map, map_len, masked != 0, st >> (2 * j), pseudo, base + j, bad) : 0;
  }
  if (m == VEC) {                       // labels_p + base is 16-byte aligned: base is a multiple of 4
#pragma unroll
    for (int j = 0; j < VEC; j += 2)
      *reinterpret_cast<longlong2*>(labels_p + base + j) = make_longlong2(out[j], out[j + 1]);
  } else {
#pragma unroll
    for (int j = 0; j < VEC; ++j)
      if (j < m) labels_p[base + j] = out[j];
  }
  if (bad) atomicAdd(n_invalid, bad);
}

// sk_dataset.py:171: labels_v = labels_p[unique_idxs] (an index outside [0, p) is counted and reads as 255)
__global__ void __launch_bounds__(LB_BLOCK) voxels_kernel(const int64_t* __restrict__ labels_p, int64_t p,
                                                           const int64_t* __restrict__ unique_idx, int64_t n,
                                                           int64_t* __restrict__ labels_v, int* __restrict__ n_invalid) {
  const int64_t j = (int64_t)blockIdx.x * LB_BLOCK + threadIdx.x;
  if (j >= n) return;
  const int64_t q = unique_idx[j];
  const bool ok = q >= 0 && q < p;
  labels_v[j] = ok ? labels_p[q] : LB_IGNORE;
  if (!ok) atomicAdd(n_invalid, 1);
}

}  // namespace

extern "C" int64_t lidal_train_labels_workspace_bytes(int64_t p) {
  return align_up(4 * cdiv(std::max<int64_t>(p, 1), 16), 256);          /* two bits per point */
}

extern "C" int lidal_train_labels(const void* raw, int raw_bytes, int64_t p, const int64_t* label_map, int map_len,
                                  const int64_t* sv_ptr, const int64_t* sv_idx, int64_t nnz, int s,
                                  const int64_t* sv_flag, const int64_t* pseudo, const int64_t* unique_idx, int64_t n,
                                  int64_t* labels_p, int64_t* labels_v, int32_t* n_invalid_dev, void* ws,
                                  int64_t ws_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  LIDAL_REQUIRE(raw_bytes == 4 || raw_bytes == 1, "train_labels: raw labels are 4 bytes (SemanticKITTI) or 1 (nuScenes)");
  LIDAL_REQUIRE(p >= 0 && n >= 0 && s >= 0 && nnz >= 0, "train_labels: negative point, voxel, supervoxel or entry count");
  LIDAL_REQUIRE(p < (1ll << 38) && n < (1ll << 38), "train_labels: too many points or voxels");
  LIDAL_REQUIRE(label_map != nullptr && map_len >= 1 && map_len <= LB_MAXMAP,
                "train_labels: the label table must have 1..%d entries", LB_MAXMAP);
  const bool masked = sv_flag != nullptr;
  LIDAL_REQUIRE(masked ? (sv_ptr != nullptr && (sv_idx != nullptr || nnz == 0))
                       : (sv_ptr == nullptr && sv_idx == nullptr && s == 0 && nnz == 0),
                "train_labels: sv_ptr, sv_idx and sv_flag come together (all NULL: every point keeps its label)");
  LIDAL_REQUIRE(n_invalid_dev != nullptr, "train_labels: no counter of invalid ids");
  LIDAL_REQUIRE(p == 0 || (raw != nullptr && labels_p != nullptr), "train_labels: no raw labels or no labels_p");
  LIDAL_REQUIRE(((uintptr_t)labels_p & 15) == 0, "train_labels: labels_p must be 16-byte aligned");
  LIDAL_REQUIRE(n == 0 || (unique_idx != nullptr && labels_v != nullptr), "train_labels: no unique_idx or no labels_v");
  LIDAL_HIP(hipMemsetAsync(n_invalid_dev, 0, 4, st));
  unsigned* state = nullptr;
  if (masked && p > 0) {
    LIDAL_REQUIRE(ws != nullptr && ws_bytes >= lidal_train_labels_workspace_bytes(p), "train_labels workspace too small");
    state = (unsigned*)ws;
    LIDAL_HIP(hipMemsetAsync(state, 0, (size_t)(4 * cdiv(p, 16)), st));
    if (s > 0) {
      mark_kernel<<<(unsigned)s, LB_BLOCK, 0, st>>>(sv_ptr, sv_idx, nnz, sv_flag, pseudo != nullptr, p, state,
                                                    n_invalid_dev);
      LIDAL_CHECK_LAUNCH("train_labels_mark");
    }
  }
  if (p > 0) {
    const int vec = ((uintptr_t)raw & 15) == 0;
    if (raw_bytes == 4) {
      points_kernel<uint32_t, 4><<<(unsigned)cdiv(p, (int64_t)LB_BLOCK * 4), LB_BLOCK, 0, st>>>(
          (const uint32_t*)raw, p, vec, label_map, map_len, state, masked, pseudo, labels_p, n_invalid_dev);
    } else {
      points_kernel<uint8_t, 16><<<(unsigned)cdiv(p, (int64_t)LB_BLOCK * 16), LB_BLOCK, 0, st>>>(
          (const uint8_t*)raw, p, vec, label_map, map_len, state, masked, pseudo, labels_p, n_invalid_dev);
    }
    LIDAL_CHECK_LAUNCH("train_labels_points");
  }
  if (n > 0) {
    voxels_kernel<<<(unsigned)cdiv(n, LB_BLOCK), LB_BLOCK, 0, st>>>(labels_p, p, unique_idx, n, labels_v, n_invalid_dev);
    LIDAL_CHECK_LAUNCH("train_labels_voxels");
  }
  return 0;
}
