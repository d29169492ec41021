// Labels and predictions carried across registered frames: stage 2 over the match table of
// lidal_interframe_match (score.hip).  One thread per query point walks its matches in neighbour order and
//   * votes: the labels of the matched points, a histogram in registers, the first maximum wins;
//   * fuses: the probability rows of the matched points, interframe_kernel's sum (f32 adds in neighbour order, f64
//     divide, f32 store), so the entropy of the fused row is the scorer's intere.
// The definitions are this project's own; tests/test_transfer_gpu.py restates them in numpy.  Built without fma
// contraction and without packed-f32 instructions (lidal_amd/build.py).  Integer atomics and vector stores only: every
// output is a function of the inputs alone.
#include <cstring>

#include "common.h"
#include "npsum.h"

using namespace lidal;
using lidal::npsum::kMaxClasses;

namespace {

constexpr int MAXNEI = 32;
constexpr int kThreads = 256;
// stats behind the c class counts
enum { ST_OWN = 0, ST_NONE, ST_WEAK, ST_GATED, ST_CONFIRMED, ST_CONTRADICTED, ST_INVALID, ST_EXTRA };

struct TransferArgs {
  const int64_t* labels[MAXNEI];
  const float* prob[MAXNEI];
  int64_t p[MAXNEI];
  int n;
};

// match[n][i] when it names a point of neighbour n, else -1
__device__ __forceinline__ int matched(const int* __restrict__ match, const TransferArgs& nei, int n, int64_t p, int64_t i) {
  const int j = match[(int64_t)n * p + i];
  return (j >= 0 && (int64_t)j < nei.p[n]) ? j : -1;
}

__global__ void __launch_bounds__(kThreads)
transfer_kernel(const int* __restrict__ match, int64_t p, int c, TransferArgs nei, const int64_t* __restrict__ q_labels,
                const int64_t* __restrict__ gate, int64_t ignore_index, int min_votes, double min_agree,
                int64_t* __restrict__ out, int* __restrict__ votes, int* __restrict__ agree,
                unsigned long long* __restrict__ stats, const float* __restrict__ q_prob, float* __restrict__ fused_prob,
                int64_t* __restrict__ fused_pred, float* __restrict__ fused_conf, int* __restrict__ count) {
  __shared__ int block[kMaxClasses + ST_EXTRA];
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < p;
  if (out != nullptr) {
    for (int k = threadIdx.x; k < c + ST_EXTRA; k += kThreads) block[k] = 0;
    __syncthreads();
    if (live) {
      int hist[kMaxClasses];
#pragma unroll
      for (int k = 0; k < kMaxClasses; ++k) hist[k] = 0;
      int nv = 0, invalid = 0;
      for (int n = 0; n < nei.n; ++n) {
        if (nei.labels[n] == nullptr) continue;
        const int j = matched(match, nei, n, p, i);
        if (j < 0) continue;
        const int64_t l = nei.labels[n][j];
        if (l == ignore_index) continue;
        if (l < 0 || l >= (int64_t)c) { ++invalid; continue; }
        const int li = (int)l;
#pragma unroll
        for (int k = 0; k < kMaxClasses; ++k) hist[k] += (k == li) ? 1 : 0;
        ++nv;
      }
      int winner = 0, ag = hist[0];
#pragma unroll
      for (int k = 1; k < kMaxClasses; ++k)
        if (hist[k] > ag) { ag = hist[k]; winner = k; }      // (hist[k] = 0 for k >= c)
      votes[i] = nv;
      agree[i] = ag;
      // 0: the vote goes through, else the counter of the rule that stops it
      int stop = -1;
      if (nv == 0) stop = ST_NONE;
      else if (nv < min_votes || (double)ag < min_agree * (double)nv) stop = ST_WEAK;
      else if (gate != nullptr && gate[i] != (int64_t)winner) stop = ST_GATED;
      const int64_t own = q_labels != nullptr ? q_labels[i] : ignore_index;
      int64_t o;
      if (q_labels != nullptr && own != ignore_index) {
        o = own;
        atomicAdd(&block[c + ST_OWN], 1);
        if (stop < 0) atomicAdd(&block[c + (own == (int64_t)winner ? ST_CONFIRMED : ST_CONTRADICTED)], 1);
      } else if (stop >= 0) {
        o = ignore_index;
        atomicAdd(&block[c + stop], 1);
      } else {
        o = winner;
        atomicAdd(&block[winner], 1);
      }
      out[i] = o;
      if (invalid) atomicAdd(&block[c + ST_INVALID], invalid);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < c + ST_EXTRA; k += kThreads)
      if (block[k]) atomicAdd(&stats[k], (unsigned long long)block[k]);
  }
  if (fused_prob != nullptr && live) {
    float sum[kMaxClasses];
#pragma unroll
    for (int k = 0; k < kMaxClasses; ++k) sum[k] = (k < c) ? q_prob[i * c + k] : 0.f;
    int cnt = 0;
    for (int n = 0; n < nei.n; ++n) {
      const int j = matched(match, nei, n, p, i);
      if (j < 0) continue;
      const float* np = nei.prob[n] + (int64_t)j * c;
#pragma unroll
      for (int k = 0; k < kMaxClasses; ++k)
        if (k < c) sum[k] = __fadd_rn(sum[k], np[k]);
      cnt += 1;
    }
    // interframe_kernel's sum_prob /= map_count: f64 divide, f32 store
    const double mc = (double)(cnt + 1);
    float best = 0.f;
    int arg = 0;
#pragma unroll
    for (int k = 0; k < kMaxClasses; ++k)
      if (k < c) {
        const float m = (float)((double)sum[k] / mc);
        fused_prob[i * c + k] = m;
        if (k == 0 || m > best) { best = m; arg = k; }
      }
    fused_pred[i] = arg;
    fused_conf[i] = best;
    count[i] = cnt;
  }
}

}  // namespace

extern "C" int lidal_interframe_transfer(const int32_t* match, int64_t p, int c, int n_nei, const int64_t* nei_p_host,
                                         const int64_t* const* nei_labels_host, const int64_t* q_labels,
                                         const int64_t* gate, int64_t ignore_index, int min_votes, double min_agree,
                                         int64_t* out, int32_t* votes, int32_t* agree, int64_t* stats,
                                         const float* q_prob, const float* const* nei_prob_host, float* fused_prob,
                                         int64_t* fused_pred, float* fused_conf, int32_t* count, void* stream) {
  LIDAL_REQUIRE(c > 0 && c <= kMaxClasses, "interframe_transfer: classes must be in 1..%d", kMaxClasses);
  LIDAL_REQUIRE(n_nei >= 0 && n_nei <= MAXNEI, "interframe_transfer: at most %d neighbours", MAXNEI);
  LIDAL_REQUIRE(min_votes >= 1, "interframe_transfer: min_votes must be at least 1");
  LIDAL_REQUIRE(min_agree > 0.0 && min_agree <= 1.0, "interframe_transfer: min_agree must be in (0, 1]");
  LIDAL_REQUIRE(p >= 0, "interframe_transfer: p must not be negative");
  const bool ann_any = nei_labels_host || q_labels || gate || out || votes || agree || stats;
  const bool ann_all = out && votes && agree && stats && (nei_labels_host || n_nei == 0);
  const bool pre_any = q_prob || nei_prob_host || fused_prob || fused_pred || fused_conf || count;
  const bool pre_all = q_prob && fused_prob && fused_pred && fused_conf && count && (nei_prob_host || n_nei == 0);
  LIDAL_REQUIRE(ann_any || pre_any, "interframe_transfer: both output groups are off");
  LIDAL_REQUIRE(!ann_any || ann_all, "interframe_transfer: the annotation group is only half given "
                                     "(nei_labels_host, out, votes, agree and stats come together)");
  LIDAL_REQUIRE(!pre_any || pre_all, "interframe_transfer: the prediction group is only half given "
                                     "(q_prob, nei_prob_host, fused_prob, fused_pred, fused_conf and count come together)");
  LIDAL_REQUIRE(n_nei == 0 || nei_p_host != nullptr, "interframe_transfer: nei_p_host is NULL");
  LIDAL_REQUIRE(n_nei == 0 || p == 0 || match != nullptr, "interframe_transfer: match is NULL");
  TransferArgs a;
  memset(&a, 0, sizeof(a));
  a.n = n_nei;
  for (int n = 0; n < n_nei; ++n) {
    a.p[n] = nei_p_host[n] > 0 ? nei_p_host[n] : 0;
    a.labels[n] = ann_any ? nei_labels_host[n] : nullptr;
    a.prob[n] = pre_any ? nei_prob_host[n] : nullptr;
    LIDAL_REQUIRE(!pre_any || a.p[n] == 0 || a.prob[n] != nullptr,
                  "interframe_transfer: neighbour %d has points but no probabilities", n);
  }
  hipStream_t s = (hipStream_t)stream;
  if (ann_any) LIDAL_HIP(hipMemsetAsync(stats, 0, (size_t)(c + ST_EXTRA) * sizeof(int64_t), s));
  if (p == 0) return 0;
  transfer_kernel<<<(unsigned)cdiv(p, kThreads), kThreads, 0, s>>>(
      match, p, c, a, q_labels, gate, ignore_index, min_votes, min_agree, out, votes, agree,
      (unsigned long long*)stats, q_prob, fused_prob, fused_pred, fused_conf, count);
  LIDAL_CHECK_LAUNCH("lidal_interframe_transfer");
  return 0;
}
