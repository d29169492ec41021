// Size-constrained k-means supervoxels (dataset/prepare_supervoxel_kmeans_{sk,nu}.py of the reference, which calls
// KMeansConstrained(n_clusters=20, size_min, size_max, n_init=1, max_iter=1)) for gfx950, as this project defines them
// (DESIGN.md section 11): greedy k-means++ seeds and the centre update shared with lidal_kmeans (kmeans.h), integer arc
// costs rint(1000 * distance), and an exact balanced assignment by successive shortest paths on the K + 1 node cluster
// graph, one workgroup per frame.
//
// Built with -ffp-contract=off (lidal_amd/build.py): the costs restate numpy's separately rounded products and sums.
// Everything after the costs is integer arithmetic whose reductions are mins over (delta, point) words and integer
// sums, so the result does not depend on the order the lanes arrive in: two runs are bit-identical.
#include <climits>

#include "common.h"
#include "kmeans.h"

using namespace lidal;

namespace {

constexpr int SV_KMAX = 64;            // clusters per frame: one bit each in the 64-bit row and column masks
constexpr int FLOW_BLOCK = 1024;
constexpr int FLOW_NODES = SV_KMAX + 1;
constexpr unsigned long long NO_ARC = ~0ull;
constexpr long long FAR = LLONG_MAX;
constexpr unsigned NO_LABEL = 0xFFu;   // the padding bytes of the last 16-label group
constexpr int SV_BLOCK = 128;          // points per block of the two-level arc words: two per lane of a wave

// error words (include/lidal_amd.h LIDAL_FLOW_*)
constexpr int FLOW_INFEASIBLE = 1, FLOW_NO_TARGET = 2, FLOW_WALK = 3, FLOW_NOT_SETTLED = 4, FLOW_NO_POINT = 5;

// An arc's word: (delta + 2^32) in the high 33 bits, the point in the low 31.  The least word is the least delta and,
// among equal deltas, the lowest point; all ones (delta 2^32 - 1 of point 2^31 - 1, which no frame has) is "no arc".
__device__ __forceinline__ unsigned long long arc_word(long long delta, int point) {
  return ((unsigned long long)(delta + (1ll << 32)) << 31) | (unsigned long long)(unsigned)point;
}
__device__ __forceinline__ long long arc_delta(unsigned long long w) { return (long long)(w >> 31) - (1ll << 32); }
__device__ __forceinline__ int arc_point(unsigned long long w) { return (int)(w & 0x7FFFFFFFull); }

// first byte of frame f's one-byte labels in the workspace: 16-byte aligned, so that a lane reads 16 labels at once
__host__ __device__ __forceinline__ int64_t lab8_offset(int64_t frame_start, int f) {
  return ((frame_start + 15) & ~(int64_t)15) + 16 * (int64_t)f;
}

// first block of frame f's block words in the workspace (frame f has ceil(P / 128) blocks of k * k words)
__host__ __device__ __forceinline__ int64_t bm_first_block(int64_t frame_start, int f) {
  return frame_start / SV_BLOCK + f;
}

// cost[i][c] = (int32) rint(1000 * sqrt((dx*dx + dy*dy) + dz*dz)), f64, the f32 point widened against the f64 centre
__global__ void __launch_bounds__(256) sv_cost_kernel(const float* __restrict__ xyz, int64_t p,
                                                      const double* __restrict__ centers, int k,
                                                      int* __restrict__ cost) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p) return;
  const double x = (double)xyz[i * 3 + 0], y = (double)xyz[i * 3 + 1], z = (double)xyz[i * 3 + 2];
  for (int c = 0; c < k; ++c) {
    const double dx = x - centers[c * 3 + 0], dy = y - centers[c * 3 + 1], dz = z - centers[c * 3 + 2];
    const double d2 = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
    cost[i * k + c] = (int)rint(__dmul_rn(1000.0, __dsqrt_rn(d2)));
  }
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long t = __shfl_xor(v, o);
    v = t < v ? t : v;
  }
  return v;
}

// Bellman-Ford's candidate word: (distance + 2^40) above the 7 bits of the node it comes from; the least word is the
// least distance and, among equal distances, the lowest node.  |distance| <= 65 * 2^32 < 2^40.
__device__ __forceinline__ unsigned long long bf_word(long long d, int u) {
  return ((unsigned long long)(d + (1ll << 40)) << 7) | (unsigned long long)u;
}
__device__ __forceinline__ long long bf_dist(unsigned long long w) { return (long long)(w >> 7) - (1ll << 40); }
__device__ __forceinline__ int bf_node(unsigned long long w) { return (int)(w & 127ull); }

// The least arc word a -> b among the (at most two) points of this lane, p and p + 64, with labels l0 and l1; by the
// whole wave: the least over a block of SV_BLOCK = 128 consecutive points.
__device__ __forceinline__ unsigned long long block_min(const int* __restrict__ cost, int k, int P, int p, unsigned l0,
                                                        unsigned l1, int a, int b) {
  unsigned long long w = NO_ARC;
  if (p < P && l0 == (unsigned)a) {
    const int* row = cost + (int64_t)p * k;
    w = arc_word((long long)row[b] - (long long)row[a], p);
  }
  if (p + 64 < P && l1 == (unsigned)a) {
    const int* row = cost + (int64_t)(p + 64) * k;
    const unsigned long long w1 = arc_word((long long)row[b] - (long long)row[a], p + 64);
    w = w1 < w ? w1 : w;
  }
  return wave_min_u64(w);
}

// One workgroup per frame.  The arc words are kept on two levels: bm[a][b][block] in the workspace is the least
// (delta, point) word from cluster a to cluster b among the points of one block of 128 consecutive points, and M[a][b]
// in LDS is the least over the blocks.  A point that joins a cluster lowers the words of its block and of M; a point
// that leaves dirties only the words it held: its block is rescanned by one wave (128 labels), and M's word is taken
// again over the blocks by one wave.  No pass over the frame per augmentation.
// Also in LDS: the cluster sizes `count`, their targets `take`, the nodes' excess, Bellman-Ford's distances and
// parents.  The frame's labels are bytes in the workspace (lab8), written as i32 at the end.
//
// Every loop has a bound known before it starts: sum(max(exc, 0)) augmentations, K + 1 Bellman-Ford rounds, K + 1 steps
// of the path walk.  A state that should be impossible writes an error word and leaves.  No workgroup waits on another.
__global__ void __launch_bounds__(FLOW_BLOCK)
sv_flow_kernel(const int* __restrict__ cost_all, const int64_t* __restrict__ frame_ptr, int k,
               const int* __restrict__ size_min, const int* __restrict__ size_max, int* __restrict__ labels_all,
               int* __restrict__ counts_out, long long* __restrict__ objective, int* __restrict__ status,
               unsigned char* lab8_all, unsigned long long* bm_all) {
  __shared__ unsigned long long M[SV_KMAX * SV_KMAX];
  __shared__ unsigned long long obj;
  __shared__ long long dist[2][FLOW_NODES];
  __shared__ int parent[FLOW_NODES], exc[FLOW_NODES], chg[FLOW_NODES + 1];
  __shared__ int count[SV_KMAX], take[SV_KMAX];
  __shared__ int arc_u[FLOW_NODES], arc_v[FLOW_NODES], arc_q[FLOW_NODES];
  __shared__ unsigned char task[SV_KMAX * SV_KMAX];     // per (arc, column): 1 rescan the block's word, 2 retake M's
  __shared__ int n_arcs, n_aug, err;

  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int WAVES = FLOW_BLOCK / 64;
  const int64_t p0 = frame_ptr[f];
  const int P = (int)(frame_ptr[f + 1] - p0);
  const int* __restrict__ cost = cost_all + p0 * k;
  int* __restrict__ labels = labels_all + p0;
  unsigned char* lab8 = lab8_all + lab8_offset(p0, f);
  const int NB = (P + SV_BLOCK - 1) / SV_BLOCK;
  unsigned long long* bm = bm_all + bm_first_block(p0, f) * k * k;       // word (a, b, block) at (a k + b) NB + block
  const int lo = size_min[f], hi = size_max[f];
  const int n = k + 1, T = k;
  const int groups = (P + 15) / 16;

  for (int t = tid; t < SV_KMAX * SV_KMAX; t += FLOW_BLOCK) { M[t] = NO_ARC; task[t] = 0; }
  if (tid < SV_KMAX) count[tid] = 0;
  if (tid == 0) { obj = 0; err = 0; n_aug = 0; n_arcs = 0; }
  __syncthreads();

  // ---- the unconstrained optimum: every point at its cheapest cluster, the lowest cluster on ties
  for (int g = tid; g < groups; g += FLOW_BLOCK) {
    unsigned word[4] = {0, 0, 0, 0};
    for (int j = 0; j < 16; ++j) {
      const int p = g * 16 + j;
      unsigned a = NO_LABEL;
      if (p < P) {
        const int* row = cost + (int64_t)p * k;
        int best = row[0];
        a = 0;
        for (int c = 1; c < k; ++c) {
          const int v = row[c];
          if (v < best) { best = v; a = c; }
        }
        atomicAdd(&count[a], 1);
      }
      word[j >> 2] |= a << (8 * (j & 3));
    }
    reinterpret_cast<uint4*>(lab8)[g] = make_uint4(word[0], word[1], word[2], word[3]);
  }
  __syncthreads();
  if (tid == 0) {
    const bool feasible = lo >= 0 && lo <= hi && (int64_t)k * lo <= P && (int64_t)k * hi >= P;
    if (!feasible) err = FLOW_INFEASIBLE;
    int64_t sum_take = 0, aug = 0;
    for (int c = 0; c < k; ++c) {
      const int tk = count[c] < lo ? lo : (count[c] > hi ? hi : count[c]);
      take[c] = tk;
      exc[c] = count[c] - tk;
      sum_take += tk;
      aug += exc[c] > 0 ? exc[c] : 0;
    }
    exc[T] = (int)(sum_take - P);
    aug += exc[T] > 0 ? exc[T] : 0;
    n_aug = feasible ? (int)aug : 0;
  }
  // ---- every block's words (a wave per block), then M's words over the blocks (a wave per word)
  for (int blk = wave; blk < NB; blk += WAVES) {
    const int p = blk * SV_BLOCK + lane;
    const unsigned l0 = p < P ? lab8[p] : NO_LABEL, l1 = p + 64 < P ? lab8[p + 64] : NO_LABEL;
    for (int a = 0; a < k; ++a) {
      const bool present = __ballot(l0 == (unsigned)a || l1 == (unsigned)a) != 0;
      if (!present) {
        if (lane < k) bm[((int64_t)a * k + lane) * NB + blk] = NO_ARC;
        continue;
      }
      for (int b = 0; b < k; ++b) {
        const unsigned long long w = b == a ? NO_ARC : block_min(cost, k, P, p, l0, l1, a, b);
        if (lane == 0) bm[((int64_t)a * k + b) * NB + blk] = w;
      }
    }
  }
  __syncthreads();
  auto entry_min = [&](int a, int b) {
    const unsigned long long* e = bm + ((int64_t)a * k + b) * NB;
    unsigned long long w = NO_ARC;
    for (int blk = lane; blk < NB; blk += 64) {
      const unsigned long long t = e[blk];
      w = t < w ? t : w;
    }
    return wave_min_u64(w);
  };
  for (int e = wave; e < k * k; e += WAVES) {
    const unsigned long long w = entry_min(e / k, e % k);
    if (lane == 0) M[(e / k) * SV_KMAX + e % k] = w;
  }
  __syncthreads();

  const int augmentations = n_aug;
  int done = 0;
  for (; done < augmentations; ++done) {
    // ---- Bellman-Ford in synchronous rounds from every excess node at distance 0: a wave per node v, its lanes the
    // nodes u the distance may come from
    if (tid < n) {
      dist[0][tid] = exc[tid] > 0 ? 0 : FAR;
      parent[tid] = -1;
    }
    if (tid <= n) chg[tid] = 0;
    __syncthreads();
    int cur = 0;
    bool settled = false;
    for (int r = 0; r < n; ++r) {
      for (int v = wave; v < n; v += WAVES) {
        unsigned long long best = NO_ARC;
        for (int u = lane; u < n; u += 64) {
          const long long du = dist[cur][u];
          if (du == FAR || u == v) continue;
          long long w = 0;
          if (u < k && v < k) {
            const unsigned long long word = M[u * SV_KMAX + v];
            if (word == NO_ARC) continue;
            w = arc_delta(word);
          } else if (v == T) {
            if (!(take[u] < hi)) continue;
          } else {
            if (!(take[v] > lo)) continue;
          }
          const unsigned long long c = bf_word(du + w, u);
          best = c < best ? c : best;
        }
        best = wave_min_u64(best);
        if (lane == 0) {
          long long nd = dist[cur][v];
          if (best != NO_ARC && bf_dist(best) < nd) {
            nd = bf_dist(best);
            parent[v] = bf_node(best);
            chg[r] = 1;
          }
          dist[cur ^ 1][v] = nd;
        }
      }
      __syncthreads();
      cur ^= 1;
      if (chg[r] == 0) { settled = true; break; }
    }
    // ---- the deficit node of least distance (the lowest on ties), its path, one unit along it
    if (wave == 0) {
      unsigned long long best = NO_ARC;
      for (int v = lane; v < n; v += 64)
        if (exc[v] < 0 && dist[cur][v] != FAR) {
          const unsigned long long c = bf_word(dist[cur][v], v);
          best = c < best ? c : best;
        }
      best = wave_min_u64(best);
      if (lane == 0) {
        int e = 0, len = 0;
        if (!settled) e = FLOW_NOT_SETTLED;
        else if (best == NO_ARC) e = FLOW_NO_TARGET;
        if (e == 0) {
          // the walk back: arc i runs arc_u[i] -> arc_v[i], the target's arc first
          int node = bf_node(best);
          for (int step = 0; step < n; ++step) {
            const int u = parent[node];
            if (u < 0) break;
            if (len < FLOW_NODES) { arc_u[len] = u; arc_v[len] = node; }
            ++len;
            node = u;
          }
          if (parent[node] >= 0 || exc[node] <= 0 || len == 0 || len > k) e = FLOW_WALK;
        }
        if (e == 0) {
          for (int i = len - 1; i >= 0; --i) {
            const int u = arc_u[i], v = arc_v[i];
            arc_q[i] = -1;
            if (u == T) {
              --take[v];
            } else if (v == T) {
              ++take[u];
            } else {
              const unsigned long long word = M[u * SV_KMAX + v];
              if (word == NO_ARC) { e = FLOW_NO_POINT; break; }
              const int q = arc_point(word);
              arc_q[i] = q;
              lab8[q] = (unsigned char)v;
              --count[u];
              ++count[v];
            }
            --exc[u];            // one unit leaves u and arrives at v, whatever the arc is
            ++exc[v];
          }
        }
        n_arcs = e == 0 ? len : 0;
        if (e != 0) err = e;
      }
    }
    __syncthreads();
    if (err != 0) break;
    const int na = n_arcs, slots = na * k;
    // ---- cluster v gained point q: its word joins the mins of its block and of M
    for (int t = tid; t < slots; t += FLOW_BLOCK) {
      const int i = t / k, b = t % k, q = arc_q[i];
      if (q < 0 || b == arc_v[i]) continue;
      const int v = arc_v[i];
      const int* row = cost + (int64_t)q * k;
      const unsigned long long w = arc_word((long long)row[b] - (long long)row[v], q);
      unsigned long long* e = bm + ((int64_t)v * k + b) * NB + q / SV_BLOCK;
      if (w < *e) *e = w;                               // (this thread alone touches this word in this phase)
      atomicMin(&M[v * SV_KMAX + b], w);
    }
    __syncthreads();
    // ---- cluster u lost point q: the words q still holds are dirty.  A word the new point of the phase above has
    // already replaced is below every other member's, and exact.
    for (int t = tid; t < slots; t += FLOW_BLOCK) {
      const int i = t / k, b = t % k, q = arc_q[i];
      unsigned char todo = 0;
      if (q >= 0 && b != arc_u[i]) {
        const int u = arc_u[i];
        const unsigned long long wb = bm[((int64_t)u * k + b) * NB + q / SV_BLOCK], wm = M[u * SV_KMAX + b];
        if (wb != NO_ARC && arc_point(wb) == q) todo |= 1;
        if (wm != NO_ARC && arc_point(wm) == q) todo |= 2;
      }
      task[t] = todo;
    }
    __syncthreads();
    for (int t = wave; t < slots; t += WAVES) {
      if (!(task[t] & 1)) continue;
      const int i = t / k, b = t % k, u = arc_u[i], blk = arc_q[i] / SV_BLOCK;
      const int p = blk * SV_BLOCK + lane;
      const unsigned l0 = p < P ? lab8[p] : NO_LABEL, l1 = p + 64 < P ? lab8[p + 64] : NO_LABEL;
      const unsigned long long w = block_min(cost, k, P, p, l0, l1, u, b);
      if (lane == 0) bm[((int64_t)u * k + b) * NB + blk] = w;
    }
    __syncthreads();
    for (int t = wave; t < slots; t += WAVES) {
      if (!(task[t] & 2)) continue;
      const int u = arc_u[t / k], b = t % k;
      const unsigned long long w = entry_min(u, b);
      if (lane == 0) M[u * SV_KMAX + b] = w;
    }
    // (the barrier at the top of Bellman-Ford orders these writes before the next reads)
  }
  __syncthreads();

  // ---- labels as i32, the objective, the sizes
  long long mine = 0;
  for (int p = tid; p < P; p += FLOW_BLOCK) {
    const int a = lab8[p];
    labels[p] = a;
    mine += cost[(int64_t)p * k + a];
  }
  atomicAdd(&obj, (unsigned long long)mine);
  __syncthreads();
  if (tid < k && counts_out != nullptr) counts_out[(int64_t)f * k + tid] = count[tid];
  if (tid == 0) {
    objective[f] = (long long)obj;
    status[2 * f] = err;
    status[2 * f + 1] = done;
  }
}

// ---- workspace layouts: one routine each, for sizing (NULL) and for carving
struct FlowWs { unsigned char* lab8; unsigned long long* bm; int64_t total; };
FlowWs flow_layout(int64_t p_total, int n_frames, int k, void* ws) {
  const int64_t pt = p_total > 0 ? p_total : 0;
  Carver c(ws);
  return {c.take<unsigned char>(pt + 16 * ((int64_t)n_frames + 2)),
          c.take<unsigned long long>((pt / SV_BLOCK + n_frames + 1) * k * k), c.total()};
}

struct SvWs {
  char* km;
  int* cost;
  char* flow;
  int64_t* frame_ptr;
  int *lo, *hi;
  double* centers0;
  int64_t km_bytes, flow_bytes, total;
};
SvWs sv_layout(int64_t p_total, int64_t p_max, int n_frames, int k, int trials, void* ws) {
  const int64_t kb = km_layout(p_max, 3, k, trials, nullptr).total, fb = flow_layout(p_total, n_frames, k, nullptr).total;
  const int64_t pt = p_total > 0 ? p_total : 1, nf = n_frames > 0 ? n_frames : 1;
  Carver c(ws);
  return {c.take(kb), c.take<int>(pt * k), c.take(fb), c.take<int64_t>(nf + 1), c.take<int>(nf), c.take<int>(nf),
          c.take<double>(nf * k * 3), kb, fb, c.total()};
}

int flow_launch(const int* cost, const int64_t* frame_ptr, int n_frames, int k, const int* lo, const int* hi, int* labels,
                int* counts, int64_t* objective, int* status, const FlowWs& w, hipStream_t s) {
  sv_flow_kernel<<<(unsigned)n_frames, FLOW_BLOCK, 0, s>>>(cost, frame_ptr, k, lo, hi, labels, counts,
                                                           (long long*)objective, status, w.lab8, w.bm);
  LIDAL_CHECK_LAUNCH("balanced_assign");
  return 0;
}

}  // namespace

extern "C" int lidal_supervoxel_costs(const float* xyz, int64_t p, const double* centers, int k, int32_t* cost,
                                      void* stream) {
  LIDAL_REQUIRE(k >= 1 && k <= SV_KMAX, "supervoxel_costs: the cluster count must be in 1..%d", SV_KMAX);
  LIDAL_REQUIRE(p >= 0 && p < 0x7FFFFFFF, "supervoxel_costs: at most 2^31 - 2 points");
  if (p == 0) return 0;
  sv_cost_kernel<<<(unsigned)cdiv(p, 256), 256, 0, (hipStream_t)stream>>>(xyz, p, centers, k, cost);
  LIDAL_CHECK_LAUNCH("supervoxel_costs");
  return 0;
}

extern "C" int64_t lidal_balanced_assign_workspace_bytes(int64_t p_total, int n_frames, int k) {
  return flow_layout(p_total, n_frames, k > 0 ? k : 1, nullptr).total;
}

extern "C" int lidal_balanced_assign(const int32_t* cost, const int64_t* frame_ptr, int n_frames, int64_t p_total, int k,
                                     const int32_t* size_min, const int32_t* size_max, int32_t* labels, int32_t* counts,
                                     int64_t* objective, int32_t* status, void* ws, int64_t ws_bytes, void* stream) {
  LIDAL_REQUIRE(k >= 1 && k <= SV_KMAX, "balanced_assign: the cluster count must be in 1..%d", SV_KMAX);
  LIDAL_REQUIRE(n_frames >= 0 && p_total >= 0 && p_total < 0x7FFFFFFF, "balanced_assign: at most 2^31 - 2 points");
  const FlowWs w = flow_layout(p_total, n_frames, k, ws);
  LIDAL_REQUIRE(ws_bytes >= w.total, "balanced_assign workspace too small");
  if (n_frames == 0) return 0;
  return flow_launch(cost, frame_ptr, n_frames, k, size_min, size_max, labels, counts, objective, status, w,
                     (hipStream_t)stream);
}

extern "C" int64_t lidal_supervoxel_kmeans_workspace_bytes(int64_t p_total, int64_t p_max, int n_frames, int k,
                                                           int trials) {
  return sv_layout(p_total, p_max, n_frames, k, trials, nullptr).total;
}

extern "C" int lidal_supervoxel_kmeans(const float* xyz, const int64_t* frame_ptr_host, int n_frames, int k,
                                       const int32_t* size_min_host, const int32_t* size_max_host,
                                       const int64_t* first_host, const double* u, int trials, int32_t* seeds,
                                       int32_t* labels_first, double* centers, int32_t* labels, int32_t* order,
                                       int32_t* counts, int64_t* objective, int32_t* status, void* ws, int64_t ws_bytes,
                                       void* stream) {
  LIDAL_REQUIRE(k >= 1 && k <= SV_KMAX, "supervoxel_kmeans: the cluster count must be in 1..%d", SV_KMAX);
  LIDAL_REQUIRE(n_frames >= 1, "supervoxel_kmeans: no frames");
  LIDAL_REQUIRE(trials >= 1 && trials <= 64, "supervoxel_kmeans: local trials must be in 1..64");
  LIDAL_REQUIRE(frame_ptr_host[0] == 0, "supervoxel_kmeans: frame_ptr must start at 0");
  const int64_t p_total = frame_ptr_host[n_frames];
  int64_t p_max = 0;
  for (int f = 0; f < n_frames; ++f) {
    const int64_t p = frame_ptr_host[f + 1] - frame_ptr_host[f];
    LIDAL_REQUIRE(p >= k, "supervoxel_kmeans: frame %d has %lld points for %d clusters", f, (long long)p, k);
    LIDAL_REQUIRE(first_host[f] >= 0 && first_host[f] < p, "supervoxel_kmeans: first centre out of range");
    p_max = p > p_max ? p : p_max;
  }
  LIDAL_REQUIRE(p_total < 0x7FFFFFFF, "supervoxel_kmeans: at most 2^31 - 2 points");
  const SvWs w = sv_layout(p_total, p_max, n_frames, k, trials, ws);
  LIDAL_REQUIRE(ws_bytes >= w.total, "supervoxel_kmeans workspace too small");
  const KmWs km = km_layout(p_max, 3, k, trials, w.km);
  const FlowWs fw = flow_layout(p_total, n_frames, k, w.flow);
  hipStream_t s = (hipStream_t)stream;
  LIDAL_HIP(hipMemcpyAsync(w.frame_ptr, frame_ptr_host, 8 * (size_t)(n_frames + 1), hipMemcpyHostToDevice, s));
  LIDAL_HIP(hipMemcpyAsync(w.lo, size_min_host, 4 * (size_t)n_frames, hipMemcpyHostToDevice, s));
  LIDAL_HIP(hipMemcpyAsync(w.hi, size_max_host, 4 * (size_t)n_frames, hipMemcpyHostToDevice, s));
  const int64_t nu = (int64_t)(k - 1) * trials;
  auto costs_of = [&](int f, const double* c) {
    const int64_t p0 = frame_ptr_host[f], p = frame_ptr_host[f + 1] - p0;
    sv_cost_kernel<<<(unsigned)cdiv(p, 256), 256, 0, s>>>(xyz + p0 * 3, p, c, k, w.cost + p0 * k);
    LIDAL_CHECK_LAUNCH("supervoxel_cost");
    return 0;
  };
  // ---- seeds (the seed rows are the centres), costs, the first balanced assignment
  for (int f = 0; f < n_frames; ++f) {
    const int64_t p0 = frame_ptr_host[f], p = frame_ptr_host[f + 1] - p0;
    double* c0 = w.centers0 + (int64_t)f * k * 3;
    if (int rc = km_seed(xyz + p0 * 3, p, 3, k, first_host[f], u + f * nu, trials, seeds + (int64_t)f * k, c0, km, s))
      return rc;
    if (int rc = costs_of(f, c0)) return rc;
  }
  if (int rc = flow_launch(w.cost, w.frame_ptr, n_frames, k, w.lo, w.hi, labels_first, counts, objective, status, fw, s))
    return rc;
  // ---- the centre update, costs, the second balanced assignment: these labels are the result
  if (int rc = km_iota(p_max, km, s)) return rc;
  for (int f = 0; f < n_frames; ++f) {
    const int64_t p0 = frame_ptr_host[f], p = frame_ptr_host[f + 1] - p0;
    double* c1 = centers + (int64_t)f * k * 3;
    if (int rc = km_update(xyz + p0 * 3, p, 3, k, labels_first + p0, counts + (int64_t)f * k,
                           w.centers0 + (int64_t)f * k * 3, c1, km, s))
      return rc;
    if (int rc = costs_of(f, c1)) return rc;
  }
  if (int rc = flow_launch(w.cost, w.frame_ptr, n_frames, k, w.lo, w.hi, labels, counts, objective + n_frames,
                           status + 2 * (int64_t)n_frames, fw, s))
    return rc;
  // ---- the points of every frame sorted by (label, point): with the counts, the supervoxel CSR
  int end_bit = 1;
  while ((1 << end_bit) < k) ++end_bit;
  for (int f = 0; f < n_frames; ++f) {
    const int64_t p0 = frame_ptr_host[f], p = frame_ptr_host[f + 1] - p0;
    if (int rc = radix_sort(labels + p0, km.iota, km.skeys, order + p0, p, 4, end_bit, km.sort_tmp, km.sort_bytes, s))
      return rc;
  }
  return 0;
}
