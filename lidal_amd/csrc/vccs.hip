// VCCS supervoxels of raw scans (dataset/prepare_supervoxel_VCCS_{sk,nu}.py of the reference, which pipe every scan
// through a PCL program) for gfx950, as this project defines them: occupied cells of edge Rv with
// exact fixed-point centroids, 26-adjacency, normals by Jacobi over the two-ring, one seed candidate per occupied cell
// of edge Rs, and a fixed number of synchronous rounds in which every voxel takes the least (D, label) among its
// neighbours' owners.  The library's labels are NOT reproduced and nothing here claims them.
//
// Built with -ffp-contract=off (lidal_amd/build.py): every product and sum is rounded on its own, as the numpy
// restatement (tests/vccs_ref.py) rounds them.  Whatever more than one thread adds up is an integer (point and voxel
// sums in 2^-16 m, normals in 2^-30), and every choice has an explicit tie rule, so two runs are bit-identical.
//
// All frames of a batch advance in the same launches: voxels, seed cells and supervoxels are numbered across the
// batch, frame after frame, and the grids run over their bound (the batch's points).  Their counts stay on the device
// (status[1..3]); a thread beyond the live count leaves.  Every loop has a bound known at launch; a state that should
// be impossible writes an error word (status[0]) that the wrapper raises from.  The scans of the flags are scan.h's
// tiled_scan; the look-ups by key and by frame and the error word are cellsort.h's (lower_bound, segment_of, raise).
#include <math.h>

#include "cellsort.h"
#include "common.h"
#include "grid.h"
#include "scan.h"
#include "sym3.h"

using namespace lidal;
using namespace lidal::grid;
using namespace lidal::cellsort;
using namespace lidal::sym3;

namespace {

constexpr int VC_BLOCK = 256;
constexpr int LABEL_BITS = 24;                         // a label is at most the frame's voxels, below 2^24
// status words (include/lidal_amd.h)
constexpr int ST_ERR = 0, ST_V = 1, ST_G = 2, ST_S = 3, ST_PTR = 4;

// position of `key` among the ascending keys[lo, hi), or -1
__device__ __forceinline__ int find_key(const u64* __restrict__ keys, int lo, int hi, u64 key) {
  const int at = lower_bound(keys, lo, hi, key);
  return (at < hi && keys[at] == key) ? at : -1;
}

// ---------------------------------------------------------------- points -> voxels
// per point: its frame, the key of its cell floor(x / Rv), its own index as the sort's payload
__global__ void __launch_bounds__(VC_BLOCK) point_key_kernel(const float* __restrict__ xyz, int64_t p,
                                                             const int64_t* __restrict__ frame_ptr, int n_frames,
                                                             double rv, u64* __restrict__ key, int* __restrict__ pframe,
                                                             int* __restrict__ iota, long long* status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p) return;
  pframe[i] = segment_of(frame_ptr, n_frames, i);
  iota[i] = (int)i;
  const double x = (double)xyz[i * 3 + 0], y = (double)xyz[i * 3 + 1], z = (double)xyz[i * 3 + 2];
  uint64_t k = 0;
  if (!cell_pack((int64_t)floor(x / rv), (int64_t)floor(y / rv), (int64_t)floor(z / rv), &k)) raise(status, LIDAL_VCCS_CELL_RANGE);
  key[i] = k;
}

// the frames of the items in sorted position, as the key of the second, stable sort
__global__ void __launch_bounds__(VC_BLOCK) frame_key_kernel(const int* __restrict__ item, const int* __restrict__ frame_of,
                                                             int64_t cap, const long long* __restrict__ n_live,
                                                             unsigned* __restrict__ key32) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= cap) return;
  key32[j] = (n_live == nullptr || j < *n_live) ? (unsigned)frame_of[item[j]] : 0u;
}

// flag[j] = the item in sorted position j opens a new (frame, key) group; 0 beyond the live items
__global__ void __launch_bounds__(VC_BLOCK) head_kernel(const int* __restrict__ item, const int* __restrict__ frame_of,
                                                        const u64* __restrict__ key, int64_t cap,
                                                        const long long* __restrict__ n_live, int* __restrict__ flag) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= cap) return;
  int h = 0;
  if (n_live == nullptr || j < *n_live) {
    h = 1;
    if (j > 0) {
      const int a = item[j], b = item[j - 1];
      h = (frame_of[a] != frame_of[b] || key[a] != key[b]) ? 1 : 0;
    }
  }
  flag[j] = h;
}

// per sorted point: its voxel (the group's number), the voxel's key and frame, the exact sums of the voxel
__global__ void __launch_bounds__(VC_BLOCK) voxel_fill_kernel(const float* __restrict__ xyz, int64_t p, int n_frames,
                                                              const int* __restrict__ item, const int* __restrict__ pframe,
                                                              const u64* __restrict__ key, const int* __restrict__ flag,
                                                              const int* __restrict__ incl, int* __restrict__ pvox,
                                                              u64* __restrict__ vkey, int* __restrict__ vframe,
                                                              long long* __restrict__ qs, int* __restrict__ nv,
                                                              long long* status) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= p) return;
  const int i = item[j], v = incl[j] - 1, f = pframe[i];
  pvox[i] = v;
  if (flag[j]) {
    vkey[v] = key[i];
    vframe[v] = f;
    if (j == 0 || pframe[item[j - 1]] != f) status[ST_PTR + f] = v;
  }
  if (j == p - 1) {
    status[ST_V] = incl[j];
    status[ST_PTR + n_frames] = incl[j];
  }
  for (int a = 0; a < 3; ++a)
    atomicAdd((u64*)&qs[(int64_t)v * 3 + a], (u64)(long long)rint((double)xyz[(int64_t)i * 3 + a] * 65536.0));
  atomicAdd(&nv[v], 1);
}

// per voxel: the cell, the centroid (double) qs / (double) n / 65536, and qv = rint(c * 65536)
__global__ void __launch_bounds__(VC_BLOCK) centroid_kernel(int64_t cap, const long long* __restrict__ status,
                                                            const u64* __restrict__ vkey, const long long* __restrict__ qs,
                                                            const int* __restrict__ nv, int* __restrict__ cells,
                                                            double* __restrict__ cen, long long* __restrict__ qv) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= cap || v >= status[ST_V]) return;
  int64_t c[3];
  cell_unpack(vkey[v], &c[0], &c[1], &c[2]);
  const double n = (double)nv[v];
  for (int a = 0; a < 3; ++a) {
    cells[v * 3 + a] = (int)c[a];
    const double m = (double)qs[v * 3 + a] / n / 65536.0;
    cen[v * 3 + a] = m;
    qv[v * 3 + a] = (long long)rint(m * 65536.0);
  }
}

// nbr[o][v]: the voxel of cell(v) + offset o, o = (dx + 1) * 9 + (dy + 1) * 3 + (dz + 1), or -1; o = 13 is v itself
__global__ void __launch_bounds__(VC_BLOCK) adjacency_kernel(int64_t cap, long long* status, const u64* __restrict__ vkey,
                                                             const int* __restrict__ vframe, int* __restrict__ nbr) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t v = t % cap;
  const int o = (int)(t / cap);
  if (o >= 27 || v >= status[ST_V]) return;
  int64_t x, y, z;
  cell_unpack(vkey[v], &x, &y, &z);
  const int f = vframe[v];
  uint64_t k;
  int u = -1;
  if (cell_pack(x + o / 9 - 1, y + (o / 3) % 3 - 1, z + o % 3 - 1, &k))
    u = find_key(vkey, (int)status[ST_PTR + f], (int)status[ST_PTR + f + 1], k);
  if (o == 13 && u != (int)v) raise(status, LIDAL_VCCS_NO_SLOT);
  nbr[(int64_t)o * cap + v] = u;
}

// ---------------------------------------------------------------- normals
// One thread per voxel.  S(v): the voxels within two adjacency steps, as a 125-bit mask over the cell offsets
// (dx + 2) * 25 + (dy + 2) * 5 + (dz + 2), walked in ascending order; mean, population covariance and cyclic Jacobi are
// sym3.h's, the ones of the surface variation (redal.hip), the rotations applied to an eigenvector matrix as well.
__global__ void __launch_bounds__(VC_BLOCK) normal_kernel(int64_t cap, long long* status, const u64* __restrict__ vkey,
                                                          const int* __restrict__ vframe, const int* __restrict__ nbr,
                                                          const double* __restrict__ cen, double* __restrict__ nrm,
                                                          long long* __restrict__ qn) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= cap || v >= status[ST_V]) return;
  u64 m0 = 0, m1 = 0;
  for (int o1 = 0; o1 < 27; ++o1) {
    const int u = nbr[(int64_t)o1 * cap + v];
    if (u < 0) continue;
    for (int o2 = 0; o2 < 27; ++o2) {
      if (nbr[(int64_t)o2 * cap + u] < 0) continue;
      const int dx = o1 / 9 + o2 / 9, dy = (o1 / 3) % 3 + (o2 / 3) % 3, dz = o1 % 3 + o2 % 3;   // each offset + 2
      const int idx = dx * 25 + dy * 5 + dz;
      if (idx < 64) m0 |= 1ull << idx; else m1 |= 1ull << (idx - 64);
    }
  }
  const int count = __popcll(m0) + __popcll(m1);
  double n3[3] = {0.0, 0.0, 0.0};
  if (count >= 3) {
    int64_t x, y, z;
    cell_unpack(vkey[v], &x, &y, &z);
    const int f = vframe[v];
    const int lo = (int)status[ST_PTR + f], hi = (int)status[ST_PTR + f + 1];
    auto member = [&](int idx) {
      uint64_t k = 0;
      int w = -1;
      if (cell_pack(x + idx / 25 - 2, y + (idx / 5) % 5 - 2, z + idx % 5 - 2, &k)) w = find_key(vkey, lo, hi, k);
      if (w < 0) { raise(status, LIDAL_VCCS_NO_SLOT); w = (int)v; }
      return (int64_t)w;
    };
    double a[3][3], e[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    covariance3([&](auto visit) {
      for (int idx = 0; idx < 125; ++idx) {
        if (!(((idx < 64 ? m0 >> idx : m1 >> (idx - 64))) & 1ull)) continue;
        const int64_t w = member(idx);
        visit(cen[w * 3 + 0], cen[w * 3 + 1], cen[w * 3 + 2]);
      }
    }, count, a);
    jacobi3<true>(a, e);
    // the column of the smallest diagonal entry, the lowest index among equals
    double best = a[0][0];
    n3[0] = e[0][0]; n3[1] = e[1][0]; n3[2] = e[2][0];
    if (a[1][1] < best) { best = a[1][1]; n3[0] = e[0][1]; n3[1] = e[1][1]; n3[2] = e[2][1]; }
    if (a[2][2] < best) { best = a[2][2]; n3[0] = e[0][2]; n3[1] = e[1][2]; n3[2] = e[2][2]; }
    // toward the sensor at the origin
    if ((n3[0] * cen[v * 3 + 0] + n3[1] * cen[v * 3 + 1]) + n3[2] * cen[v * 3 + 2] > 0.0) {
      n3[0] = -n3[0]; n3[1] = -n3[1]; n3[2] = -n3[2];
    }
  }
  for (int a = 0; a < 3; ++a) {
    nrm[v * 3 + a] = n3[a];
    qn[v * 3 + a] = (long long)rint(n3[a] * 1073741824.0);
  }
}

// ---------------------------------------------------------------- seeds
// per voxel: the key of its seed cell floor(c / Rs) and the squared distance of its centroid to that cell's centre
__global__ void __launch_bounds__(VC_BLOCK) seed_key_kernel(int64_t cap, long long* status, const double* __restrict__ cen,
                                                            double rs, u64* __restrict__ key, double* __restrict__ sd2,
                                                            int* __restrict__ iota) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= cap) return;
  iota[v] = (int)v;
  if (v >= status[ST_V]) { key[v] = 0; return; }
  int64_t c[3];
  double d[3];
  for (int a = 0; a < 3; ++a) {
    const double x = cen[v * 3 + a];
    c[a] = (int64_t)floor(x / rs);
    d[a] = x - ((double)c[a] + 0.5) * rs;
  }
  uint64_t k = 0;
  if (!cell_pack(c[0], c[1], c[2], &k)) raise(status, LIDAL_VCCS_CELL_RANGE);
  key[v] = k;
  sd2[v] = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
}

// per sorted voxel: its seed cell (the group's number), the cell's frame, the frames' first cells
__global__ void __launch_bounds__(VC_BLOCK) seed_cell_kernel(int64_t cap, int n_frames, long long* status,
                                                             const int* __restrict__ item, const int* __restrict__ vframe,
                                                             const int* __restrict__ flag, const int* __restrict__ incl,
                                                             int* __restrict__ vseg, long long* __restrict__ gptr) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t V = status[ST_V];
  if (j >= cap || j >= V) return;
  const int v = item[j], g = incl[j] - 1, f = vframe[v];
  vseg[v] = g;
  if (flag[j] && (j == 0 || vframe[item[j - 1]] != f)) gptr[f] = g;
  if (j == V - 1) {
    status[ST_G] = incl[j];
    gptr[n_frames] = incl[j];
  }
}

// the least squared distance of a seed cell's voxels (a non-negative double orders as its bits) ...
__global__ void __launch_bounds__(VC_BLOCK) seed_min_kernel(int64_t cap, const long long* __restrict__ status,
                                                            const int* __restrict__ vseg, const double* __restrict__ sd2,
                                                            u64* __restrict__ gmin) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= cap || v >= status[ST_V]) return;
  atomicMin(&gmin[vseg[v]], (u64)__double_as_longlong(sd2[v]));
}
// ... and the lowest voxel that has it: voxels are numbered in (x, y, z) order of their cells
__global__ void __launch_bounds__(VC_BLOCK) seed_cand_kernel(int64_t cap, const long long* __restrict__ status,
                                                             const int* __restrict__ vseg, const double* __restrict__ sd2,
                                                             const u64* __restrict__ gmin, int* __restrict__ gcand) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= cap || v >= status[ST_V]) return;
  const int g = vseg[v];
  if ((u64)__double_as_longlong(sd2[v]) == gmin[g]) atomicMin(&gcand[g], (int)v);
}

// every voxel counts itself into the candidates of its frame whose centroid is within the search radius
__global__ void __launch_bounds__(VC_BLOCK) seed_count_kernel(int64_t cap, long long* status, const int* __restrict__ vframe,
                                                              const double* __restrict__ cen, const long long* __restrict__ gptr,
                                                              const int* __restrict__ gcand, double r2,
                                                              int* __restrict__ gcount) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t V = status[ST_V];
  if (v >= cap || v >= V) return;
  const int f = vframe[v];
  const double x = cen[v * 3 + 0], y = cen[v * 3 + 1], z = cen[v * 3 + 2];
  const int64_t g0 = gptr[f], g1 = gptr[f + 1];
  for (int64_t g = g0; g < g1 && g < cap; ++g) {
    const int64_t u = gcand[g];
    if (u < 0 || u >= V) { raise(status, LIDAL_VCCS_NO_CANDIDATE); continue; }
    const double dx = x - cen[u * 3 + 0], dy = y - cen[u * 3 + 1], dz = z - cen[u * 3 + 2];
    if ((dx * dx + dy * dy) + dz * dz <= r2) atomicAdd(&gcount[g], 1);
  }
}

__global__ void __launch_bounds__(VC_BLOCK) seed_flag_kernel(int64_t cap, const long long* __restrict__ status,
                                                             const int* __restrict__ gcount, double min_seed,
                                                             int* __restrict__ flag) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= cap) return;
  flag[g] = (g < status[ST_G] && (double)gcount[g] > min_seed) ? 1 : 0;
}

// survivors in ascending order of their seed cells are the supervoxels; the frames' first supervoxels
__global__ void __launch_bounds__(VC_BLOCK) seed_fill_kernel(int64_t cap, int n_frames, long long* status,
                                                             const long long* __restrict__ gptr, const int* __restrict__ vframe,
                                                             const int* __restrict__ gcand, const int* __restrict__ flag,
                                                             const int* __restrict__ incl, int* __restrict__ seed_voxel) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t G = status[ST_G];
  if (g >= cap || g >= G) return;
  const int u = gcand[g];
  if (u < 0 || u >= status[ST_V]) return;                  // (reported by seed_count_kernel)
  const int f = vframe[u];
  if (flag[g]) seed_voxel[incl[g] - 1] = u;
  if (g == gptr[f]) status[ST_PTR + n_frames + 1 + f] = incl[g] - flag[g];
  if (g == G - 1) {
    status[ST_S] = incl[g];
    status[ST_PTR + 2 * n_frames + 1] = incl[g];
  }
}

// ---------------------------------------------------------------- the rounds
__global__ void __launch_bounds__(VC_BLOCK) state_init_kernel(int64_t cap, const long long* __restrict__ status,
                                                              int* __restrict__ owner, double* __restrict__ dist) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= cap || v >= status[ST_V]) return;
  owner[v] = 0;
  dist[v] = INFINITY;
}

// a seed voxel starts with its label (1.. inside its frame) and distance 0; the supervoxel's sums are the voxel's
__global__ void __launch_bounds__(VC_BLOCK) seed_init_kernel(int64_t cap, int n_frames, const long long* __restrict__ status,
                                                             const int* __restrict__ seed_voxel, const int* __restrict__ vframe,
                                                             const long long* __restrict__ qv, const long long* __restrict__ qn,
                                                             int* __restrict__ owner, double* __restrict__ dist,
                                                             long long* __restrict__ acc) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= cap || s >= status[ST_S]) return;
  const int64_t v = seed_voxel[s];
  owner[v] = (int)(s - status[ST_PTR + n_frames + 1 + vframe[v]]) + 1;
  dist[v] = 0.0;
  for (int a = 0; a < 3; ++a) {
    acc[s * 7 + a] = qv[v * 3 + a];
    acc[s * 7 + 3 + a] = qn[v * 3 + a];
  }
  acc[s * 7 + 6] = 1;
}

// centre and unit normal of every live supervoxel from its integer sums; a dead one keeps what it had
__global__ void __launch_bounds__(VC_BLOCK) finalise_kernel(int64_t cap, const long long* __restrict__ status,
                                                            const long long* __restrict__ acc, double* __restrict__ svc,
                                                            double* __restrict__ svn) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= cap || s >= status[ST_S]) return;
  const long long k = acc[s * 7 + 6];
  if (k <= 0) return;
  for (int a = 0; a < 3; ++a) svc[s * 3 + a] = (double)acc[s * 7 + a] / (double)k / 65536.0;
  const double sx = (double)acc[s * 7 + 3], sy = (double)acc[s * 7 + 4], sz = (double)acc[s * 7 + 5];
  const double len = sqrt((sx * sx + sy * sy) + sz * sz);
  svn[s * 3 + 0] = len > 0.0 ? sx / len : 0.0;
  svn[s * 3 + 1] = len > 0.0 ? sy / len : 0.0;
  svn[s * 3 + 2] = len > 0.0 ? sz / len : 0.0;
}

// One round, one thread per voxel, pulling: from the owners, distances and centres of the round's start the voxel
// takes the least (D, label) among its neighbours' owners if that D is strictly below its own.  The sums of the
// supervoxels are integers, so a voxel that changes hands moves its terms from the old sums to the new ones and the
// sums equal those taken afresh over the members, whatever the order.
__global__ void __launch_bounds__(VC_BLOCK) round_kernel(int64_t cap, int n_frames, const long long* __restrict__ status,
                                                         const int* __restrict__ vframe, const int* __restrict__ nbr,
                                                         const double* __restrict__ cen, const double* __restrict__ nrm,
                                                         const long long* __restrict__ qv, const long long* __restrict__ qn,
                                                         const double* __restrict__ svc, const double* __restrict__ svn,
                                                         double w_s, double w_n, double rs,
                                                         const int* __restrict__ owner_in, const double* __restrict__ dist_in,
                                                         int* __restrict__ owner_out, double* __restrict__ dist_out,
                                                         long long* __restrict__ acc) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= cap || v >= status[ST_V]) return;
  const int mine = owner_in[v];
  const int64_t s0 = status[ST_PTR + n_frames + 1 + vframe[v]];
  const double cx = cen[v * 3 + 0], cy = cen[v * 3 + 1], cz = cen[v * 3 + 2];
  const double nx = nrm[v * 3 + 0], ny = nrm[v * 3 + 1], nz = nrm[v * 3 + 2];
  double best = INFINITY;
  int best_l = 0;
  for (int o = 0; o < 27; ++o) {
    if (o == 13) continue;
    const int u = nbr[(int64_t)o * cap + v];
    if (u < 0) continue;
    const int l = owner_in[u];
    if (l == 0 || l == mine || l == best_l) continue;
    const int64_t s = s0 + l - 1;
    const double dx = svc[s * 3 + 0] - cx, dy = svc[s * 3 + 1] - cy, dz = svc[s * 3 + 2] - cz;
    const double dot = (svn[s * 3 + 0] * nx + svn[s * 3 + 1] * ny) + svn[s * 3 + 2] * nz;
    const double d = w_n * (1.0 - fabs(dot)) + w_s * (sqrt((dx * dx + dy * dy) + dz * dz) / rs);
    if (best_l == 0 || d < best || (d == best && l < best_l)) { best = d; best_l = l; }
  }
  int now = mine;
  double dnow = dist_in[v];
  if (best_l != 0 && best < dnow) { now = best_l; dnow = best; }
  owner_out[v] = now;
  dist_out[v] = dnow;
  if (now != mine) {
    for (int a = 0; a < 6; ++a) {
      const long long q = a < 3 ? qv[v * 3 + a] : qn[v * 3 + a - 3];
      atomicAdd((u64*)&acc[(s0 + now - 1) * 7 + a], (u64)q);
      if (mine != 0) atomicAdd((u64*)&acc[(s0 + mine - 1) * 7 + a], (u64)(-q));
    }
    atomicAdd((u64*)&acc[(s0 + now - 1) * 7 + 6], 1ull);
    if (mine != 0) atomicAdd((u64*)&acc[(s0 + mine - 1) * 7 + 6], (u64)(-1ll));
  }
}

// ---------------------------------------------------------------- labels and the CSR's order
__global__ void __launch_bounds__(VC_BLOCK) label_kernel(int64_t p, const int* __restrict__ pvox,
                                                         const int* __restrict__ pframe, const int* __restrict__ owner,
                                                         long long* __restrict__ labels, u64* __restrict__ key,
                                                         int* __restrict__ iota) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p) return;
  const int l = owner[pvox[i]];
  labels[i] = l;
  key[i] = ((u64)pframe[i] << LABEL_BITS) | (u64)l;
  iota[i] = (int)i;
}

// points per supervoxel, a voxel at a time (a thread per point would pile 10^5 atomics on each counter)
__global__ void __launch_bounds__(VC_BLOCK) count_kernel(int64_t cap, int n_frames, const long long* __restrict__ status,
                                                         const int* __restrict__ vframe, const int* __restrict__ owner,
                                                         const int* __restrict__ nv, int* __restrict__ counts) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= cap || v >= status[ST_V]) return;
  const int l = owner[v];
  if (l != 0) atomicAdd(&counts[status[ST_PTR + n_frames + 1 + vframe[v]] + l - 1], nv[v]);
}

// ---------------------------------------------------------------- workspace: one routine for sizing and carving
struct VccsWs {
  int64_t* frame_ptr;
  long long* gptr;
  u64 *key, *skey, *vkey, *gmin;
  unsigned *key32, *skey32;
  int *idx_a, *idx_b, *idx_c, *pframe, *vframe, *flag, *incl, *sums, *nbr, *vseg, *gcand, *gcount, *owner;
  int64_t* offs;
  long long *qv, *qn, *acc;
  double *sd2, *dist, *svc, *svn;
  char* sort;
  int64_t sort_bytes, total;
};
VccsWs vccs_layout(int64_t p_total, int n_frames, void* ws) {
  const int64_t p = p_total > 0 ? p_total : 1, nf = n_frames > 0 ? n_frames : 1;
  const int64_t sb = radix_sort_ws_bytes(p, 8, true);
  Carver c(ws);
  VccsWs w;
  w.frame_ptr = c.take<int64_t>(nf + 1);
  w.gptr = c.take<long long>(nf + 1);
  w.key = c.take<u64>(p); w.skey = c.take<u64>(p); w.vkey = c.take<u64>(p); w.gmin = c.take<u64>(p);
  w.key32 = c.take<unsigned>(p); w.skey32 = c.take<unsigned>(p);
  w.idx_a = c.take<int>(p); w.idx_b = c.take<int>(p); w.idx_c = c.take<int>(p);
  w.pframe = c.take<int>(p); w.vframe = c.take<int>(p);
  w.flag = c.take<int>(p); w.incl = c.take<int>(p);
  w.sums = c.take<int>(scan_tiles(p)); w.offs = c.take<int64_t>(scan_tiles(p) + 1);
  w.nbr = c.take<int>(27 * p);
  w.vseg = c.take<int>(p); w.gcand = c.take<int>(p); w.gcount = c.take<int>(p);
  w.owner = c.take<int>(2 * p);
  w.qv = c.take<long long>(3 * p); w.qn = c.take<long long>(3 * p); w.acc = c.take<long long>(7 * p);
  w.sd2 = c.take<double>(p); w.dist = c.take<double>(2 * p);
  w.svc = c.take<double>(3 * p); w.svn = c.take<double>(3 * p);
  w.sort = c.take(sb);
  w.sort_bytes = sb;
  w.total = c.total();
  return w;
}

// items [0, cap) (the live ones: n_live on the device, or all) sorted by (frame, key), stable: by the key, then, in a
// batch, by the frame.  Returns the array that holds the sorted items.
int sort_by_frame_key(const VccsWs& w, const int* frame_of, int64_t cap, int n_frames, int fbits, const long long* n_live,
                      const int** sorted, hipStream_t s) {
  if (int rc = radix_sort(w.key, w.idx_a, w.skey, w.idx_b, cap, 8, 3 * kCellBits, w.sort, w.sort_bytes, s,
                          (const int64_t*)n_live))
    return rc;
  *sorted = w.idx_b;
  if (n_frames == 1) return 0;
  frame_key_kernel<<<(unsigned)cdiv(cap, VC_BLOCK), VC_BLOCK, 0, s>>>(w.idx_b, frame_of, cap, n_live, w.key32);
  LIDAL_CHECK_LAUNCH("vccs_frame_key");
  if (int rc = radix_sort(w.key32, w.idx_b, w.skey32, w.idx_c, cap, 4, fbits, w.sort, w.sort_bytes, s,
                          (const int64_t*)n_live))
    return rc;
  *sorted = w.idx_c;
  return 0;
}

}  // namespace

extern "C" int64_t lidal_vccs_workspace_bytes(int64_t p_total, int n_frames) {
  return vccs_layout(p_total, n_frames, nullptr).total;
}

extern "C" int lidal_vccs(const float* xyz, const int64_t* frame_ptr_host, int n_frames, double rv, double rs, double w_s,
                          double w_n, double min_seed, int rounds, int64_t* labels, int32_t* point_voxel, int32_t* cells,
                          int64_t* qs, int32_t* nv, double* centroids, double* normals, int32_t* seed_voxels,
                          int32_t* owners, int32_t* order, int32_t* counts, int64_t* status, void* ws, int64_t ws_bytes,
                          void* stream) {
  LIDAL_REQUIRE(n_frames >= 1 && n_frames <= (1 << 16), "vccs: 1..65536 frames");
  LIDAL_REQUIRE(frame_ptr_host[0] == 0, "vccs: frame_ptr must start at 0");
  for (int f = 0; f < n_frames; ++f) {
    const int64_t p = frame_ptr_host[f + 1] - frame_ptr_host[f];
    LIDAL_REQUIRE(p >= 1 && p < (1 << LABEL_BITS), "vccs: frame %d has %lld points (1..2^24 - 1)", f, (long long)p);
  }
  const int64_t P = frame_ptr_host[n_frames];
  LIDAL_REQUIRE(P < 0x7FFFFFFF / 27, "vccs: at most %d points in a batch", 0x7FFFFFFF / 27 - 1);
  LIDAL_REQUIRE(rv > 0.0 && rs >= 2.0 * rv && w_s >= 0.0 && w_n >= 0.0 && rounds >= 0 && rounds <= 100000,
                "vccs: resolutions, importances or rounds out of range");
  const VccsWs w = vccs_layout(P, n_frames, ws);
  LIDAL_REQUIRE(ws_bytes >= w.total, "vccs workspace too small");
  hipStream_t s = (hipStream_t)stream;
  long long* st = (long long*)status;
  const unsigned grid = (unsigned)cdiv(P, VC_BLOCK);
  int fbits = 0;
  while ((1 << fbits) < n_frames) ++fbits;
  const double r2 = (0.5 * rs) * (0.5 * rs);

  LIDAL_HIP(hipMemcpyAsync(w.frame_ptr, frame_ptr_host, 8 * (size_t)(n_frames + 1), hipMemcpyHostToDevice, s));
  LIDAL_HIP(hipMemsetAsync(status, 0, 8 * (size_t)(ST_PTR + 2 * (n_frames + 1)), s));
  LIDAL_HIP(hipMemsetAsync(qs, 0, 24 * (size_t)P, s));
  LIDAL_HIP(hipMemsetAsync(nv, 0, 4 * (size_t)P, s));
  LIDAL_HIP(hipMemsetAsync(counts, 0, 4 * (size_t)P, s));
  LIDAL_HIP(hipMemsetAsync(w.gptr, 0, 8 * (size_t)(n_frames + 1), s));
  LIDAL_HIP(hipMemsetAsync(w.gmin, 0xFF, 8 * (size_t)P, s));
  LIDAL_HIP(hipMemsetAsync(w.gcand, 0x7F, 4 * (size_t)P, s));
  LIDAL_HIP(hipMemsetAsync(w.gcount, 0, 4 * (size_t)P, s));
  LIDAL_HIP(hipMemsetAsync(w.acc, 0, 56 * (size_t)P, s));

  // ---- voxels: the points sorted by (frame, cell), the groups numbered, the exact sums, the centroids
  point_key_kernel<<<grid, VC_BLOCK, 0, s>>>(xyz, P, w.frame_ptr, n_frames, rv, w.key, w.pframe, w.idx_a, st);
  LIDAL_CHECK_LAUNCH("vccs_point_key");
  const int* sorted = nullptr;
  if (int rc = sort_by_frame_key(w, w.pframe, P, n_frames, fbits, nullptr, &sorted, s)) return rc;
  head_kernel<<<grid, VC_BLOCK, 0, s>>>(sorted, w.pframe, w.key, P, nullptr, w.flag);
  LIDAL_CHECK_LAUNCH("vccs_head");
  if (int rc = tiled_scan<int, true, false>(w.flag, P, w.sums, w.offs, w.incl, s)) return rc;
  voxel_fill_kernel<<<grid, VC_BLOCK, 0, s>>>(xyz, P, n_frames, sorted, w.pframe, w.key, w.flag, w.incl, point_voxel,
                                              w.vkey, w.vframe, (long long*)qs, nv, st);
  LIDAL_CHECK_LAUNCH("vccs_voxel_fill");
  centroid_kernel<<<grid, VC_BLOCK, 0, s>>>(P, st, w.vkey, (const long long*)qs, nv, cells, centroids, w.qv);
  LIDAL_CHECK_LAUNCH("vccs_centroid");
  // ---- adjacency and normals
  adjacency_kernel<<<(unsigned)cdiv(27 * P, VC_BLOCK), VC_BLOCK, 0, s>>>(P, st, w.vkey, w.vframe, w.nbr);
  LIDAL_CHECK_LAUNCH("vccs_adjacency");
  normal_kernel<<<grid, VC_BLOCK, 0, s>>>(P, st, w.vkey, w.vframe, w.nbr, centroids, normals, w.qn);
  LIDAL_CHECK_LAUNCH("vccs_normal");
  // ---- seeds: the voxels sorted by (frame, seed cell), one candidate per cell, the survivors numbered
  seed_key_kernel<<<grid, VC_BLOCK, 0, s>>>(P, st, centroids, rs, w.key, w.sd2, w.idx_a);
  LIDAL_CHECK_LAUNCH("vccs_seed_key");
  if (int rc = sort_by_frame_key(w, w.vframe, P, n_frames, fbits, st + ST_V, &sorted, s)) return rc;
  head_kernel<<<grid, VC_BLOCK, 0, s>>>(sorted, w.vframe, w.key, P, st + ST_V, w.flag);
  LIDAL_CHECK_LAUNCH("vccs_seed_head");
  if (int rc = tiled_scan<int, true, false>(w.flag, P, w.sums, w.offs, w.incl, s)) return rc;
  seed_cell_kernel<<<grid, VC_BLOCK, 0, s>>>(P, n_frames, st, sorted, w.vframe, w.flag, w.incl, w.vseg, w.gptr);
  LIDAL_CHECK_LAUNCH("vccs_seed_cell");
  seed_min_kernel<<<grid, VC_BLOCK, 0, s>>>(P, st, w.vseg, w.sd2, w.gmin);
  LIDAL_CHECK_LAUNCH("vccs_seed_min");
  seed_cand_kernel<<<grid, VC_BLOCK, 0, s>>>(P, st, w.vseg, w.sd2, w.gmin, w.gcand);
  LIDAL_CHECK_LAUNCH("vccs_seed_cand");
  seed_count_kernel<<<grid, VC_BLOCK, 0, s>>>(P, st, w.vframe, centroids, w.gptr, w.gcand, r2, w.gcount);
  LIDAL_CHECK_LAUNCH("vccs_seed_count");
  seed_flag_kernel<<<grid, VC_BLOCK, 0, s>>>(P, st, w.gcount, min_seed, w.flag);
  LIDAL_CHECK_LAUNCH("vccs_seed_flag");
  if (int rc = tiled_scan<int, true, false>(w.flag, P, w.sums, w.offs, w.incl, s)) return rc;
  seed_fill_kernel<<<grid, VC_BLOCK, 0, s>>>(P, n_frames, st, w.gptr, w.vframe, w.gcand, w.flag, w.incl, seed_voxels);
  LIDAL_CHECK_LAUNCH("vccs_seed_fill");
  // ---- state and rounds
  int* owner[2] = {w.owner, w.owner + P};
  double* dist[2] = {w.dist, w.dist + P};
  state_init_kernel<<<grid, VC_BLOCK, 0, s>>>(P, st, owner[0], dist[0]);
  LIDAL_CHECK_LAUNCH("vccs_state_init");
  seed_init_kernel<<<grid, VC_BLOCK, 0, s>>>(P, n_frames, st, seed_voxels, w.vframe, w.qv, w.qn, owner[0], dist[0], w.acc);
  LIDAL_CHECK_LAUNCH("vccs_seed_init");
  finalise_kernel<<<grid, VC_BLOCK, 0, s>>>(P, st, w.acc, w.svc, w.svn);
  LIDAL_CHECK_LAUNCH("vccs_finalise");
  for (int r = 0; r < rounds; ++r) {
    const int a = r & 1, b = a ^ 1;
    round_kernel<<<grid, VC_BLOCK, 0, s>>>(P, n_frames, st, w.vframe, w.nbr, centroids, normals, w.qv, w.qn, w.svc, w.svn,
                                           w_s, w_n, rs, owner[a], dist[a], owner[b], dist[b], w.acc);
    LIDAL_CHECK_LAUNCH("vccs_round");
    finalise_kernel<<<grid, VC_BLOCK, 0, s>>>(P, st, w.acc, w.svc, w.svn);
    LIDAL_CHECK_LAUNCH("vccs_finalise");
  }
  const int* final_owner = owner[rounds & 1];
  // ---- labels, the points of every frame sorted by (label, point), the supervoxels' point counts
  label_kernel<<<grid, VC_BLOCK, 0, s>>>(P, point_voxel, w.pframe, final_owner, (long long*)labels, w.key, w.idx_a);
  LIDAL_CHECK_LAUNCH("vccs_label");
  count_kernel<<<grid, VC_BLOCK, 0, s>>>(P, n_frames, st, w.vframe, final_owner, nv, counts);
  LIDAL_CHECK_LAUNCH("vccs_count");
  if (int rc = radix_sort(w.key, w.idx_a, w.skey, order, P, 8, LABEL_BITS + fbits, w.sort, w.sort_bytes, s)) return rc;
  LIDAL_HIP(hipMemcpyAsync(owners, final_owner, 4 * (size_t)P, hipMemcpyDeviceToDevice, s));
  return 0;
}
