// Euclidean clustering for gfx950: the connected components of the fixed-radius graph over the points of one class of
// one scan (what PCL calls EuclideanClusterExtraction), as instance ids, membership lists and boxes (DESIGN.md
// section 24; tests/cluster_ref.py restates the definition in numpy).
//
// THE GRAPH.  A point is LIVE iff its coordinates are finite, 0 <= label < 64 and tol[label] > 0.  Two live points of
// the same scan and the same class c are joined iff the expression of neighbours.hip holds with radius = tol[c]: f32
// differences, f32 squares, (dx^2 + dy^2) + dz^2, the correctly rounded sqrtf, a strict <.  The edges are never stored.
//
// THE GRID.  Cell edge = the smallest power of two >= the largest positive tolerance, so the 27-cell probe of
// neighbours.hip (its header carries the proof; tolerances here are >= 2^-10, far above its 2^-60) cannot miss an edge
// of any class.  Points are sorted by cell key, then stably by group = scan * 64 + class (not live: group 2048, last),
// so a group is one cell-ordered segment and the nine range look-ups of a probe (run_bound of cellsort.h) stay inside it.
//
// THE UNION.  One wave per live point: its lanes stride over the candidates of a cell run (coalesced 16-byte records),
// and every lane whose candidate has a SMALLER original row and passes the predicate unites the two rows in a
// lock-free union-find over parent[], indexed by original row.  parent[i] <= i always: a root is hooked under a
// smaller root by atomicCAS(&parent[hi], hi, lo) and by nothing else, so a walk only descends, nobody waits for
// anybody, and a failed CAS means that another CAS on that word succeeded.  The root of a finished component is its
// smallest row whatever the schedule, which is the numbering the definition asks for.  Walks shorten the paths they
// pass (atomicMin of a grandparent: still an ancestor, still smaller).  A unite spends at most 2 p + 2 steps -- its two
// walks descend strictly across retries -- and a thread that runs out, or reads a parent outside [0, x], raises the
// status word and leaves.
//
// THE TABLES.  Flatten (root per row, sizes by integer atomicAdd at the root), flag the kept roots, one flag scan
// (tiled_scan of scan.h) = ids in ascending root order, inst, one stable sort of (id, row) = members, heads of the
// sorted ids = member_ptr, one wave per instance = class and box (min / max: exact, order-free).  Integer atomics only,
// vector stores only.
#include "cellsort.h"
#include "common.h"
#include "grid.h"
#include "scan.h"

using namespace lidal;
using namespace lidal::grid;
using namespace lidal::cellsort;

namespace {

constexpr int EC_BLOCK = 256;
constexpr int EC_WAVES = EC_BLOCK / kWave;
constexpr int EC_CLASSES = 64;
constexpr int EC_MAX_SCANS = 32;
constexpr unsigned EC_DEAD = EC_MAX_SCANS * EC_CLASSES;         // the group of a point that is not live: sorts last
constexpr int EC_GROUP_BITS = 12;
constexpr int EC_GPTR = EC_DEAD + 2;               // gptr[g] = where group g begins, g = 0 .. EC_DEAD + 1
constexpr int ST_ERR = 0, ST_PTR = 1;              // status words (include/lidal_amd.h)

// ---------------------------------------------------------------- keys, groups, records
// per point: its group, the key of its cell (the parking cell unless live and in range), itself as the sort's
// payload and as its own parent
__global__ void __launch_bounds__(EC_BLOCK) ec_keys_kernel(const float* __restrict__ xyz, const int64_t* __restrict__ labels,
                                                           int64_t p, const int64_t* __restrict__ point_ptr, int n_scans,
                                                           const float* __restrict__ tol, double cell,
                                                           u64* __restrict__ key, unsigned* __restrict__ gkey,
                                                           int* __restrict__ iota, int* __restrict__ parent,
                                                           long long* status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p) return;
  const float x = xyz[i * 3 + 0], y = xyz[i * 3 + 1], z = xyz[i * 3 + 2];
  const int64_t lab = labels != nullptr ? labels[i] : 0;
  u64 k = 0;                                        // the parking cell: every field 0
  unsigned g = EC_DEAD;
  if (finite_f32(x) && finite_f32(y) && finite_f32(z) && lab >= 0 && lab < EC_CLASSES && tol[lab] > 0.f) {
    const int64_t ix = cell_index((double)x, cell), iy = cell_index((double)y, cell), iz = cell_index((double)z, cell);
    if (ix == -kBias || iy == -kBias || iz == -kBias) {
      raise(status, LIDAL_CLUSTERS_CELL_RANGE);     // parked with the points that are not live: the launches stay in bounds
    } else {
      k = cell_key(ix, iy, iz);
      g = (unsigned)segment_of(point_ptr, n_scans, i) * EC_CLASSES + (unsigned)lab;
    }
  }
  key[i] = k;
  gkey[i] = g;
  iota[i] = (int)i;
  parent[i] = (int)i;
}

// the groups of the points in cell order, as the key of the second, stable sort
__global__ void __launch_bounds__(EC_BLOCK) ec_group_key_kernel(const int* __restrict__ sidx, const unsigned* __restrict__ gkey,
                                                                int64_t p, unsigned* __restrict__ key32) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < p) key32[q] = gkey[sidx[q]];
}

// gptr[g] = the first sorted position whose group is >= g, g = 0 .. EC_DEAD + 1: at most 32 halvings each
__global__ void __launch_bounds__(EC_BLOCK) ec_group_ptr_kernel(const unsigned* __restrict__ sgroup, int64_t p,
                                                                int* __restrict__ gptr) {
  const int g = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (g >= EC_GPTR) return;
  int64_t lo = 0, hi = p;
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (sgroup[mid] < (unsigned)g) lo = mid + 1; else hi = mid;
  }
  gptr[g] = (int)lo;
}

// ---------------------------------------------------------------- the union
__device__ __forceinline__ int load_parent(const int* parent, int x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root above row x, or -1 when the budget ran out or a parent lies outside [0, x] (the caller raises).  Every step
// descends strictly and costs one unit of *budget; a grandparent found on the way replaces the parent (atomicMin: the
// word of a row that is no root only ever moves to a smaller ancestor).
__device__ __forceinline__ int find_root(int* parent, int x, int64_t* budget) {
  while (true) {
    const int q = load_parent(parent, x);
    if (q == x) return x;
    if ((unsigned)q > (unsigned)x || --*budget < 0) return -1;
    const int g = load_parent(parent, q);
    if ((unsigned)g > (unsigned)q) return -1;
    if (g < q) atomicMin(parent + x, g);
    x = g;
  }
}

// rows a and b are of one component from here on; false = give up (the caller raises)
__device__ __forceinline__ bool unite(int* parent, int a, int b, int64_t p) {
  int64_t budget = 2 * p + 2;
  while (true) {
    a = find_root(parent, a, &budget);
    if (a < 0) return false;
    b = find_root(parent, b, &budget);
    if (b < 0) return false;
    if (a == b) return true;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int seen = atomicCAS(parent + hi, hi, lo);
    if (seen == hi) return true;
    // another CAS hooked hi first: go on from where it points, below hi
    if ((unsigned)seen > (unsigned)hi || --budget < 0) return false;
    a = seen;
    b = lo;
  }
}

__global__ void __launch_bounds__(EC_BLOCK)
ec_union_kernel(const u64* __restrict__ skey, const unsigned* __restrict__ sgroup, const Rec* __restrict__ rec,
                const int* __restrict__ gptr, const float* __restrict__ tol, int64_t p, int* parent, long long* status) {
  const int lane = lane_id();
  const int64_t n_live = gptr[EC_DEAD];             // the live points come first
  for (int64_t q = (int64_t)blockIdx.x * EC_WAVES + (threadIdx.x >> 6); q < n_live; q += (int64_t)gridDim.x * EC_WAVES) {
    const u64 key = skey[q];                        // (q, and everything derived from it alone, is uniform in the wave)
    const unsigned g = sgroup[q];
    const Rec me = rec[q];
    if (g >= EC_DEAD || key == 0) continue;         // (cannot be: a live point has a group and a cell)
    const float radius = tol[g & (EC_CLASSES - 1)];
    const int seg_lo = gptr[g], seg_hi = gptr[g + 1];
    const int bound = run_bound(skey, seg_lo, seg_hi, key, lane);    // lanes 0..8: a run begins; 9..17: it ends
    bool ok = true;
    for (int r = 0; r < 9; ++r) {
      const int lo = __shfl(bound, r), hi = __shfl(bound, r + 9);
      for (int64_t t = (int64_t)lo + lane; t < hi; t += kWave) {
        const Rec o = rec[t];
        if (o.idx < me.idx && within(me, o, radius)) ok = unite(parent, me.idx, o.idx, p) && ok;
      }
    }
    if (!ok) raise(status, LIDAL_CLUSTERS_WALK);
  }
}

// ---------------------------------------------------------------- the tables
// root[i] = the smallest row of i's component (-1: not live), size[root] += 1.  The union has finished: plain loads.
__global__ void __launch_bounds__(EC_BLOCK) ec_flatten_kernel(const int* __restrict__ parent, const unsigned* __restrict__ gkey,
                                                              int64_t p, int* __restrict__ root, int* __restrict__ size,
                                                              long long* status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p) return;
  int x = -1;
  if (gkey[i] < EC_DEAD) {
    x = (int)i;
    for (int64_t budget = p; ; --budget) {
      const int q = parent[x];
      if (q == x) break;
      if ((unsigned)q > (unsigned)x || budget <= 0) { x = -1; break; }
      x = q;
    }
    if (x < 0) raise(status, LIDAL_CLUSTERS_WALK); else atomicAdd(size + x, 1);
  }
  root[i] = x;
}

__global__ void __launch_bounds__(EC_BLOCK) ec_flag_kernel(const int* __restrict__ root, const int* __restrict__ size,
                                                           int64_t p, int64_t min_points, int64_t max_points,
                                                           int* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p) return;
  flag[i] = (root[i] == (int)i && size[i] >= min_points && size[i] <= max_points) ? 1 : 0;
}

// inst[i], the key of the members' sort (a point of no instance: p, behind every id), and, by the first n_scans + 1
// threads, inst_ptr[s] = the kept roots below the scan's first row
__global__ void __launch_bounds__(EC_BLOCK) ec_inst_kernel(const int* __restrict__ root, const int* __restrict__ flag,
                                                           const int* __restrict__ incl, int64_t p,
                                                           const int64_t* __restrict__ point_ptr, int n_scans,
                                                           int* __restrict__ inst, unsigned* __restrict__ mkey,
                                                           int* __restrict__ iota, long long* status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= n_scans) {
    const int64_t first = point_ptr[i];
    status[ST_PTR + i] = first > 0 ? incl[first - 1] : 0;
  }
  if (i >= p) return;
  const int r = root[i];
  const int id = (r >= 0 && flag[r]) ? incl[r] - 1 : -1;
  inst[i] = id;
  mkey[i] = id >= 0 ? (unsigned)id : (unsigned)p;
  iota[i] = (int)i;
}

// member_ptr[k] = where id k begins among the rows sorted by (id, row); member_ptr[K] = where the ids end
__global__ void __launch_bounds__(EC_BLOCK) ec_member_ptr_kernel(const unsigned* __restrict__ smkey, int64_t p,
                                                                 const int* __restrict__ incl,
                                                                 int64_t* __restrict__ member_ptr) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t > p) return;
  const unsigned none = (unsigned)p;
  const int64_t n_inst = incl[p - 1];
  if (t == p) {
    if (smkey[p - 1] != none) member_ptr[n_inst] = p;
    return;
  }
  const unsigned k = smkey[t];
  if (t > 0 && smkey[t - 1] == k) return;
  const int64_t slot = k == none ? n_inst : (int64_t)k;
  if (slot <= n_inst) member_ptr[slot] = t;         // (an id is below K: nothing can be written past the table)
}

// one wave per instance: its class (the group of its first member) and its box; beside it, by the first n_scans + 1
// threads, member_start[s] = where the members of scan s's instances begin
__global__ void __launch_bounds__(EC_BLOCK) ec_box_kernel(const float* __restrict__ xyz, const int* __restrict__ members,
                                                          const int64_t* __restrict__ member_ptr,
                                                          const unsigned* __restrict__ gkey, const int* __restrict__ incl,
                                                          int64_t p, const int64_t* __restrict__ point_ptr, int n_scans,
                                                          int* __restrict__ cls, float* __restrict__ bbox,
                                                          long long* status) {
  const int lane = lane_id();
  const int64_t n_inst = incl[p - 1];
  if (blockIdx.x == 0 && (int)threadIdx.x <= n_scans) {
    const int64_t first = point_ptr[threadIdx.x];
    status[ST_PTR + n_scans + 1 + threadIdx.x] = member_ptr[first > 0 ? incl[first - 1] : 0];
  }
  for (int64_t k = (int64_t)blockIdx.x * EC_WAVES + (threadIdx.x >> 6); k < n_inst; k += (int64_t)gridDim.x * EC_WAVES) {
    int64_t beg = member_ptr[k], end = member_ptr[k + 1];
    if (beg < 0) beg = 0;
    if (end > p) end = p;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t t = beg + lane; t < end; t += kWave) {
      const int64_t j = members[t];
      for (int a = 0; a < 3; ++a) {
        const float v = xyz[j * 3 + a];
        lo[a] = fminf(lo[a], v);
        hi[a] = fmaxf(hi[a], v);
      }
    }
    for (int d = kWave / 2; d >= 1; d >>= 1)
      for (int a = 0; a < 3; ++a) {
        lo[a] = fminf(lo[a], __shfl_xor(lo[a], d, kWave));
        hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], d, kWave));
      }
    if (lane == 0 && beg < end) cls[k] = (int)(gkey[members[beg]] & (EC_CLASSES - 1));
    const float out = lane == 0 ? lo[0] : lane == 1 ? lo[1] : lane == 2 ? lo[2] : lane == 3 ? hi[0] : lane == 4 ? hi[1] : hi[2];
    if (lane < 6) bbox[k * 6 + lane] = out;
  }
}

// ---------------------------------------------------------------- workspace: one routine for sizing and carving
struct ClusterWs {
  int64_t* point_ptr;
  float* tol;
  int* gptr;
  u64 *key, *skey, *gskey;
  unsigned *gkey, *key32, *sgroup, *mkey, *smkey;
  int *idx_a, *idx_b, *idx_c, *parent, *root, *size, *flag, *incl, *sums;
  int64_t* offs;
  Rec* rec;
  char* sort;
  int64_t sort_bytes, total;
};
ClusterWs cluster_layout(int64_t p_total, int n_scans, void* ws) {
  const int64_t p = p_total > 0 ? p_total : 1, ns = n_scans > 0 ? n_scans : 1, nb = scan_tiles(p);
  const int64_t sb = radix_sort_ws_bytes(p, 8, true);
  Carver c(ws);
  ClusterWs w;
  w.point_ptr = c.take<int64_t>(ns + 1);
  w.tol = c.take<float>(EC_CLASSES);
  w.gptr = c.take<int>(EC_GPTR);
  w.key = c.take<u64>(p); w.skey = c.take<u64>(p); w.gskey = c.take<u64>(p);
  w.gkey = c.take<unsigned>(p); w.key32 = c.take<unsigned>(p); w.sgroup = c.take<unsigned>(p);
  w.mkey = c.take<unsigned>(p); w.smkey = c.take<unsigned>(p);
  w.idx_a = c.take<int>(p); w.idx_b = c.take<int>(p); w.idx_c = c.take<int>(p);
  w.parent = c.take<int>(p); w.root = c.take<int>(p); w.size = c.take<int>(p);
  w.flag = c.take<int>(p); w.incl = c.take<int>(p); w.sums = c.take<int>(nb);
  w.offs = c.take<int64_t>(nb + 1);
  w.rec = c.take<Rec>(p);
  w.sort = c.take(sb);
  w.sort_bytes = sb;
  w.total = c.total();
  return w;
}

}  // namespace

extern "C" int64_t lidal_euclidean_clusters_workspace_bytes(int64_t p, int n_scans) {
  return cluster_layout(p, n_scans, nullptr).total;
}

extern "C" int lidal_euclidean_clusters(const float* xyz, const int64_t* labels, int64_t p,
                                        const int64_t* point_ptr_host, int n_scans, const float* tol_host, int64_t min_points, int64_t max_points, int32_t* inst,
                                        int32_t* cls, int64_t* member_ptr, int32_t* members, float* bbox, int64_t* status,
                                        void* ws, int64_t ws_bytes, void* stream) {
  LIDAL_REQUIRE(n_scans >= 1 && n_scans <= EC_MAX_SCANS, "euclidean_clusters: 1..%d scans, not %d", EC_MAX_SCANS, n_scans);
  LIDAL_REQUIRE(point_ptr_host != nullptr && tol_host != nullptr, "euclidean_clusters: point_ptr and tol are host arrays");
  LIDAL_REQUIRE(point_ptr_host[0] == 0, "euclidean_clusters: point_ptr must start at 0");
  for (int s = 0; s < n_scans; ++s)
    LIDAL_REQUIRE(point_ptr_host[s + 1] >= point_ptr_host[s], "euclidean_clusters: point_ptr must ascend (scan %d)", s);
  const int64_t P = p;
  LIDAL_REQUIRE(point_ptr_host[n_scans] == P, "euclidean_clusters: point_ptr must end at p = %lld", (long long)P);
  // (the radix sort serves fewer than 2^30 items)
  LIDAL_REQUIRE(P >= 0 && P < (1ll << 30), "euclidean_clusters: %lld points in a batch (fewer than 2^30)", (long long)P);
  float top = 0.f;
  for (int c = 0; c < EC_CLASSES; ++c) {
    const float t = tol_host[c];
    LIDAL_REQUIRE(t >= 0.f, "euclidean_clusters: the tolerance of class %d is negative or NaN", c);
    LIDAL_REQUIRE(t == 0.f || (t >= 0x1p-10f && t <= 0x1p10f),
                  "euclidean_clusters: the tolerance of class %d is outside [2^-10, 2^10] m", c);
    if (t > top) top = t;
  }
  LIDAL_REQUIRE(min_points >= 1 && max_points >= min_points, "euclidean_clusters: 1 <= min_points <= max_points");
  const ClusterWs w = cluster_layout(P, n_scans, ws);
  LIDAL_REQUIRE(ws_bytes >= w.total, "euclidean_clusters: workspace too small");
  if (P == 0 || top == 0.f) return 0;               // no instance: nothing is launched, nothing is written
  const double cell = cell_edge(top);

  hipStream_t s = (hipStream_t)stream;
  long long* st = (long long*)status;
  const unsigned grid = (unsigned)cdiv(P, EC_BLOCK);
  LIDAL_HIP(hipMemcpyAsync(w.point_ptr, point_ptr_host, 8 * (size_t)(n_scans + 1), hipMemcpyHostToDevice, s));
  LIDAL_HIP(hipMemcpyAsync(w.tol, tol_host, 4 * (size_t)EC_CLASSES, hipMemcpyHostToDevice, s));
  LIDAL_HIP(hipMemsetAsync(status, 0, 8 * (size_t)(ST_PTR + 2 * (n_scans + 1)), s));
  LIDAL_HIP(hipMemsetAsync(w.size, 0, 4 * (size_t)P, s));
  // ---- the points sorted by (group, cell)
  ec_keys_kernel<<<grid, EC_BLOCK, 0, s>>>(xyz, labels, P, w.point_ptr, n_scans, w.tol, cell, w.key, w.gkey, w.idx_a,
                                           w.parent, st);
  LIDAL_CHECK_LAUNCH("clusters_keys");
  if (int rc = radix_sort(w.key, w.idx_a, w.skey, w.idx_b, P, 8, 3 * kCellBits, w.sort, w.sort_bytes, s)) return rc;
  ec_group_key_kernel<<<grid, EC_BLOCK, 0, s>>>(w.idx_b, w.gkey, P, w.key32);
  LIDAL_CHECK_LAUNCH("clusters_group_key");
  if (int rc = radix_sort(w.key32, w.idx_b, w.sgroup, w.idx_c, P, 4, EC_GROUP_BITS, w.sort, w.sort_bytes, s)) return rc;
  records_kernel<true><<<grid, EC_BLOCK, 0, s>>>(xyz, P, w.idx_c, w.key, w.rec, w.gskey);
  LIDAL_CHECK_LAUNCH("clusters_records");
  ec_group_ptr_kernel<<<(unsigned)cdiv(EC_GPTR, EC_BLOCK), EC_BLOCK, 0, s>>>(w.sgroup, P, w.gptr);
  LIDAL_CHECK_LAUNCH("clusters_group_ptr");
  // ---- the union
  ec_union_kernel<<<capped(cdiv(P, EC_WAVES)), EC_BLOCK, 0, s>>>(w.gskey, w.sgroup, w.rec, w.gptr, w.tol, P, w.parent, st);
  LIDAL_CHECK_LAUNCH("clusters_union");
  // ---- the tables
  ec_flatten_kernel<<<grid, EC_BLOCK, 0, s>>>(w.parent, w.gkey, P, w.root, w.size, st);
  LIDAL_CHECK_LAUNCH("clusters_flatten");
  ec_flag_kernel<<<grid, EC_BLOCK, 0, s>>>(w.root, w.size, P, min_points, max_points, w.flag);
  LIDAL_CHECK_LAUNCH("clusters_flag");
  if (int rc = tiled_scan<int, true, false>(w.flag, P, w.sums, w.offs, w.incl, s)) return rc;
  ec_inst_kernel<<<(unsigned)cdiv(P > n_scans ? P : n_scans + 1, EC_BLOCK), EC_BLOCK, 0, s>>>(
      w.root, w.flag, w.incl, P, w.point_ptr, n_scans, inst, w.mkey, w.idx_a, st);
  LIDAL_CHECK_LAUNCH("clusters_inst");
  int mbits = 1;
  while ((1ll << mbits) <= P) ++mbits;              // the keys are 0 .. P
  if (int rc = radix_sort(w.mkey, w.idx_a, w.smkey, members, P, 4, mbits, w.sort, w.sort_bytes, s)) return rc;
  ec_member_ptr_kernel<<<(unsigned)cdiv(P + 1, EC_BLOCK), EC_BLOCK, 0, s>>>(w.smkey, P, w.incl, member_ptr);
  LIDAL_CHECK_LAUNCH("clusters_member_ptr");
  ec_box_kernel<<<capped(cdiv(P, EC_WAVES)), EC_BLOCK, 0, s>>>(xyz, members, member_ptr, w.gkey, w.incl, P, w.point_ptr,
                                                               n_scans, cls, bbox, st);
  LIDAL_CHECK_LAUNCH("clusters_box");
  return 0;
}
