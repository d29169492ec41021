// Training objectives beside the plain cross-entropy, for gfx950:
//   * Lovasz-softmax (Berman et al., CVPR 2018: lovasz_softmax_flat), forward and backward, on logits (softmax inside)
//     or on given probabilities;
//   * cross-entropy with class weights (torch.nn.functional.cross_entropy(weight=...), mean reduction).
//
// Lovasz-softmax, per class k over the rows whose label is not ignore_index: e = |[label == k] - p_k|, the rows ordered
// by e descending (ties: ascending row), the Lovasz extension of the Jaccard loss along that order, L_k = <e, g>.
// ONE sort serves all classes:
//
//   count     valid rows per block of 256 rows, bad labels                         n / 256 workgroups
//   offsets   exclusive scan of the block counts -> n_valid                        1 workgroup
//   keys      e = |fg - p| in f32 (logits: softmax in f64, e rounded once; probabilities: the given f32 row, one f32
//             subtraction), key = class << 32 | ~bits(e), payload = row | fg << 30,
//             class-major: entry k * n_valid + (rank of the row among the valid rows)
//   sort      the library's stable LSD radix sort over the n_valid * c live entries (count on the device)
//   tiles     number of foreground entries per (class, tile of 2048 ranks)
//   classes   exclusive scan of the tile counts per class -> gts
//   grad      per entry: its rank r, F = foreground entries up to and including r (integers, exact), from them
//             jac[r] and jac[r - 1] in f32, g = jac[r] - jac[r - 1], dL_k/dp scattered to [row, k]; the tile's
//             sum of e * g in f64 (the product of two f32 is exact there), in rank order
//   final     L_k = the tiles' sums in tile order, loss = mean over the present (or all) classes
//
// The stable sort keeps equal keys in input order, which is ascending row: the tie rule costs nothing.  No float
// atomics anywhere: every sum has one fixed order, so two runs give the same bits.  A class's entries are the ranks
// [k * n_valid, (k + 1) * n_valid) of the sorted list, so class and rank of an entry follow from its position.
// Built without fma contraction (lidal_amd/build.py): jac and g are restated in numpy bit for bit (tests/loss_ref.py).
#include "rows.h"

using namespace lidal;
using namespace lidal::rows;

namespace {

constexpr int LV_ITEMS = 8;
constexpr int LV_TILE = 256 * LV_ITEMS;       // ranks per workgroup of the rank passes
constexpr int kFgBit = 30;                    // payload = row | fg << 30 (n * c < 2^30)

// exclusive scan of one int per thread over a workgroup of NW waves; *total = the sum.  All threads call it.
template <int NW>
__device__ __forceinline__ int block_scan_excl(int v, int* wsum /*[NW] LDS*/, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(incl, d, 64);
    if (lane >= d) incl += t;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    const int sw = wsum[w];
    if (w < wave) base += sw;
    tot += sw;
  }
  __syncthreads();
  *total = tot;
  return base + incl - v;
}

// ---------------------------------------------------------------------------------------------- Lovasz-softmax
// bcnt[b] = valid rows of block b | (a label outside [0, c) other than ignore_index) << 16
__global__ void __launch_bounds__(kRows) lv_count_kernel(const int64_t* __restrict__ labels, int64_t n, int c,
                                                         int64_t ignore_index, int* __restrict__ bcnt) {
  const int64_t i = (int64_t)blockIdx.x * kRows + threadIdx.x;
  bool ok = false, bad = false;
  if (i < n) {
    const int64_t y = labels[i];
    ok = label_ok(y, c, ignore_index);
    bad = !ok && y != ignore_index;
  }
  const int cnt = __syncthreads_count(ok);
  const int anybad = __syncthreads_or(bad);
  if (threadIdx.x == 0) bcnt[blockIdx.x] = cnt | (anybad ? 1 << 16 : 0);
}

// bcnt[nb] -> exclusive offsets in place; counts = {n_valid * c, n_valid, status}
__global__ void __launch_bounds__(1024) lv_offsets_kernel(int* __restrict__ bcnt, int64_t nb, int c,
                                                          int64_t* __restrict__ counts) {
  __shared__ int wsum[16];
  int running = 0, bad = 0;
  for (int64_t b0 = 0; b0 < nb; b0 += 1024) {
    const int64_t b = b0 + threadIdx.x;
    const int w = b < nb ? bcnt[b] : 0;
    bad |= w >> 16;
    int total;
    const int ex = block_scan_excl<16>(w & 0xFFFF, wsum, &total);
    if (b < nb) bcnt[b] = running + ex;
    running += total;
  }
  const int anybad = __syncthreads_or(bad);
  if (threadIdx.x == 0) {
    counts[0] = (int64_t)running * c;
    counts[1] = running;
    counts[2] = anybad ? 1 : 0;
  }
}

template <typename T, bool PROBS>
__global__ void __launch_bounds__(kRows) lv_keys_kernel(const T* __restrict__ x, const int64_t* __restrict__ labels,
                                                        int64_t n, int c, int64_t ignore_index, bool vec,
                                                        const int* __restrict__ boff,
                                                        const int64_t* __restrict__ counts,
                                                        unsigned long long* __restrict__ keys,
                                                        int* __restrict__ vals) {
  __shared__ float lds[kTileFloats];
  __shared__ int wcnt[kRows / 64];
  const Tile tile(lds, n, c);
  tile.load<T>(x, vec);
  const int64_t i = tile.row0 + threadIdx.x;
  int64_t y = -1;
  bool ok = false;
  if (i < n) {
    y = labels[i];
    ok = label_ok(y, c, ignore_index);
  }
  const unsigned long long m = __ballot(ok);
  if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();                                  // the rows and the waves' counts
  if (!ok) return;
  int before = ballot_rank(m);
  for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) before += wcnt[w];
  const int64_t nv = counts[1];
  const int64_t v = (int64_t)boff[blockIdx.x] + before;
  float p[kMaxClasses];
  tile.own(p);
  // On logits the errors are rounded ONCE: the softmax runs in f64 on the f32 / bf16 logits and e = |fg - p| is taken
  // there, so the key's e is the f32 nearest to the exact error -- not 1 - (a p already off by an ulp or two of expf
  // and the division), which for p near 1 leaves e only a few significant bits.  With the f32 softmax the loss of one
  // input of tests/test_loss_gpu.py (n = 63, c = 2, bf16 logits) was off by 4.8e-9 from the all-f64 value where the
  // torch formulation on the CPU happened to be off by 8.2e-10; rounded once it is off by what jac's f32 leaves.
  // Given probabilities are f32 as they come: e is the one f32 subtraction of the definition (bit for bit against
  // tests/loss_ref.py).
  double pd[kMaxClasses];
  if (!PROBS) {
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < kMaxClasses; ++j)
      if (j < c) mx = fmaxf(mx, p[j]);
    double sd = 0.0;
#pragma unroll
    for (int j = 0; j < kMaxClasses; ++j)
      if (j < c) { pd[j] = exp((double)p[j] - (double)mx); sd += pd[j]; }
#pragma unroll
    for (int j = 0; j < kMaxClasses; ++j)
      if (j < c) pd[j] = pd[j] / sd;
  }
#pragma unroll
  for (int j = 0; j < kMaxClasses; ++j)
    if (j < c) {
      const int fg = j == (int)y;
      const float e = PROBS ? fabsf((fg ? 1.f : 0.f) - p[j]) : (float)fabs((fg ? 1.0 : 0.0) - pd[j]);
      const int64_t at = (int64_t)j * nv + v;
      keys[at] = ((unsigned long long)j << 32) | (unsigned long long)(~__float_as_uint(e));
      vals[at] = (int)i | (fg << kFgBit);
    }
}

// tsum[k][t] = foreground entries among the ranks of tile t of class k
__global__ void __launch_bounds__(256) lv_tiles_kernel(const int* __restrict__ vals, const int64_t* __restrict__ counts,
                                                       int64_t nt, int* __restrict__ tsum) {
  const int64_t nv = counts[1];
  const int k = blockIdx.y;
  const int64_t r0 = (int64_t)blockIdx.x * LV_TILE;
  int f = 0;
  if (r0 < nv) {
    const int* v = vals + (int64_t)k * nv;
#pragma unroll
    for (int u = 0; u < LV_ITEMS; ++u) {
      const int64_t r = r0 + u * 256 + threadIdx.x;
      if (r < nv) f += (v[r] >> kFgBit) & 1;
    }
  }
  __shared__ int red[256];
  red[threadIdx.x] = f;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) tsum[(int64_t)k * nt + blockIdx.x] = red[0];
}

// per class: tsum[k][.] -> exclusive scan in place, gts[k] = the total
__global__ void __launch_bounds__(256) lv_classes_kernel(int* __restrict__ tsum, int64_t nt, int* __restrict__ gts) {
  __shared__ int wsum[4];
  int* row = tsum + (int64_t)blockIdx.x * nt;
  int running = 0;
  for (int64_t t0 = 0; t0 < nt; t0 += 256) {
    const int64_t t = t0 + threadIdx.x;
    const int w = t < nt ? row[t] : 0;
    int total;
    const int ex = block_scan_excl<4>(w, wsum, &total);
    if (t < nt) row[t] = running + ex;
    running += total;
  }
  if (threadIdx.x == 0) gts[blockIdx.x] = running;
}

// jac at rank r (0-based) with F foreground entries among ranks 0 .. r: 1 - (gts - F) / (gts + (r + 1 - F)), the
// counts as integers, converted once
__device__ __forceinline__ float jaccard_at(int gts, int r, int F) {
  const float inter = (float)(gts - F), uni = (float)(gts + (r + 1 - F));
  return 1.f - inter / uni;
}

__global__ void __launch_bounds__(256) lv_grad_kernel(const unsigned long long* __restrict__ keys,
                                                      const int* __restrict__ vals, const int64_t* __restrict__ counts,
                                                      int64_t nt, int c, const int* __restrict__ toff,
                                                      const int* __restrict__ gts_all, float* __restrict__ grad,
                                                      int* __restrict__ ranks, double* __restrict__ lpart) {
  __shared__ int wsum[4];
  __shared__ double red[256];
  const int64_t nv = counts[1];
  const int k = blockIdx.y;
  const int64_t r0 = (int64_t)blockIdx.x * LV_TILE + (int64_t)threadIdx.x * LV_ITEMS;     // LV_ITEMS consecutive ranks per thread
  if ((int64_t)blockIdx.x * LV_TILE >= nv) return;                      // whole workgroup
  const int gts = gts_all[k];
  const unsigned long long* kk = keys + (int64_t)k * nv;
  const int* vv = vals + (int64_t)k * nv;
  int val[LV_ITEMS];
  float e[LV_ITEMS];
  int mine = 0;
#pragma unroll
  for (int u = 0; u < LV_ITEMS; ++u) {
    const bool live = r0 + u < nv;
    val[u] = live ? vv[r0 + u] : 0;
    e[u] = live ? __uint_as_float(~(unsigned)kk[r0 + u]) : 0.f;
    mine += (val[u] >> kFgBit) & 1;
  }
  int total;
  int F = toff[(int64_t)k * nt + blockIdx.x] + block_scan_excl<4>(mine, wsum, &total);
  double acc = 0.0;
#pragma unroll
  for (int u = 0; u < LV_ITEMS; ++u) {
    if (r0 + u < nv) {
      const int r = (int)(r0 + u);
      const int fg = (val[u] >> kFgBit) & 1;
      const int row = val[u] & ((1 << kFgBit) - 1);
      const float before = r > 0 ? jaccard_at(gts, r - 1, F) : 0.f;
      F += fg;
      const float g = jaccard_at(gts, r, F) - before;
      // d|fg - p| / dp: -1 on foreground, +1 on background, 0 at e == 0 (torch's abs)
      grad[(int64_t)row * c + k] = e[u] == 0.f ? 0.f : (fg ? -g : g);
      if (ranks != nullptr) ranks[(int64_t)row * c + k] = r;
      acc += (double)e[u] * (double)g;
    }
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) lpart[(int64_t)k * nt + blockIdx.x] = red[0];
}

// out f64 [4 + 2 c] = {loss, present classes, status, n_valid, L_k [c], gts_k [c]}
__global__ void __launch_bounds__(64) lv_final_kernel(const double* __restrict__ lpart, const int64_t* __restrict__ counts,
                                                      int64_t nt, int c, int mode_all, const int* __restrict__ gts,
                                                      double* __restrict__ out) {
  __shared__ double lk[kMaxClasses];
  const int64_t nv = counts[1];
  const int64_t live = cdiv(nv, LV_TILE);
  const int k = threadIdx.x;
  if (k < c) {
    double a = 0.0;
    for (int64_t t = 0; t < live; ++t) a += lpart[(int64_t)k * nt + t];
    lk[k] = a;
    out[4 + k] = a;
    out[4 + c + k] = nv > 0 ? (double)gts[k] : 0.0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int present = 0;
    double sum = 0.0;
    for (int j = 0; j < c; ++j) {
      const bool has = nv > 0 && gts[j] > 0;
      present += has ? 1 : 0;
      if (has || (mode_all && nv > 0)) sum += lk[j];
    }
    const int denom = mode_all ? c : present;
    out[0] = (nv > 0 && denom > 0) ? sum / (double)denom : 0.0;
    out[1] = (double)present;
    out[2] = (double)counts[2];
    out[3] = (double)nv;
  }
}

// dx of one row from the saved dL_k/dp: every class k weighs in with
//     s_k = gscale * [k counts] / (classes that count) + gclass[k]
// (the first term: the gradient of the mean loss, the second: of the per-class losses L_k).
//   PROBS: dx_k = G_k s_k;     logits: a_k = G_k s_k, dx_k = p_k (a_k - sum_j a_j p_j), j ascending
template <typename T, bool PROBS>
__global__ void __launch_bounds__(kRows) lv_bwd_kernel(const T* __restrict__ x, const int64_t* __restrict__ labels,
                                                       int64_t n, int c, int64_t ignore_index, bool vec, bool gvec,
                                                       int mode_all, const double* __restrict__ out,
                                                       const float* __restrict__ grad,
                                                       const float* __restrict__ gscale,
                                                       const float* __restrict__ gclass, T* __restrict__ dx) {
  __shared__ float lds[kTileFloats];
  const Tile tile(lds, n, c);
  const int64_t i = tile.row0 + threadIdx.x;
  const bool ok = i < n && label_ok(labels[i], c, ignore_index);
  float p[kMaxClasses], a[kMaxClasses];
  if (!PROBS) {
    tile.load<T>(x, vec);
    __syncthreads();
    // The denominator is summed in f64 and rounded once: a sequential f32 sum of 32 terms is off by a few ulp, which
    // every probability of the row (and twice the gradient) would inherit -- measured on the separated inputs of
    // tests/test_loss_gpu.py: 2.7e-7 relative l2 in dz at c = 32 against 4e-8 of torch on the CPU.
    if (ok) {
      tile.own(p);
      row_softmax<double>(p, c, p);
    }
    __syncthreads();
  }
  tile.load<float>(grad, gvec);
  __syncthreads();
  tile.own(a);                        // G of the row
  const bool any = out[3] > 0.0;
  const float denom = mode_all ? (float)c : (float)out[1];
  const float gs = gscale != nullptr ? gscale[0] : 0.f;
  double dotd = 0.0;                  // (products of two f32 are exact in f64; classes ascending, one rounding at the end)
#pragma unroll
  for (int j = 0; j < kMaxClasses; ++j)
    if (j < c) {
      float sk = 0.f;
      if (ok && any) {
        const bool counts_in = mode_all || out[4 + c + j] > 0.0;
        sk = (counts_in && denom > 0.f ? gs / denom : 0.f) + (gclass != nullptr ? gclass[j] : 0.f);
      }
      a[j] = ok ? a[j] * sk : 0.f;
      if (!PROBS && ok) dotd += (double)a[j] * (double)p[j];
    }
  const float dot = (float)dotd;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kMaxClasses; ++j)
    if (j < c) a[j] = !ok ? 0.f : (PROBS ? a[j] : p[j] * (a[j] - dot));
  tile.put(a);
  __syncthreads();
  tile.store<T>(dx, vec);
}

struct LovaszWs {
  int* bcnt;
  int64_t* counts;
  unsigned long long *keys, *keys_sorted;
  int *vals, *vals_sorted;
  int *tsum, *gts;
  double* lpart;
  char* sort;
  int64_t nb, nt, sort_bytes, total;
};

LovaszWs lovasz_layout(void* base, int64_t n, int c) {
  LovaszWs w;
  const int64_t q = n > 0 ? n : 1, m = q * c;
  w.nb = cdiv(q, kRows);
  w.nt = cdiv(q, LV_TILE);
  w.sort_bytes = radix_sort_ws_bytes(m, 8, true);
  Carver cv(base);
  w.bcnt = cv.take<int>(w.nb);
  w.counts = cv.take<int64_t>(3);
  w.keys = cv.take<unsigned long long>(m);
  w.keys_sorted = cv.take<unsigned long long>(m);
  w.vals = cv.take<int>(m);
  w.vals_sorted = cv.take<int>(m);
  w.tsum = cv.take<int>(w.nt * c);
  w.gts = cv.take<int>(c);
  w.lpart = cv.take<double>(w.nt * c);
  w.sort = cv.take<char>(w.sort_bytes);
  w.total = cv.total();
  return w;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int lovasz_check(int64_t n, int c, int dtype, int is_probs) {
  LIDAL_REQUIRE(c >= 1 && c <= kMaxClasses, "lovasz: classes must be in 1..%d (got %d)", kMaxClasses, c);
  LIDAL_REQUIRE(n >= 0 && n * (int64_t)c < (1ll << 30), "lovasz: %lld rows x %d classes exceed the sort's 2^30 entries",
                (long long)n, c);
  LIDAL_REQUIRE(dtype == LIDAL_F32 || (dtype == LIDAL_BF16 && !is_probs), "lovasz: bad dtype %d%s", dtype,
                is_probs ? " (probabilities are f32)" : "");
  return 0;
}

// ---------------------------------------------------------------------------------------------- weighted cross-entropy
// block partials {sum w[y] * -log softmax(x)[y], sum w[y]} in f64
template <typename T>
__global__ void __launch_bounds__(kRows) cew_fwd_kernel(const T* __restrict__ logits, const int64_t* __restrict__ labels,
                                                        int64_t n, int c, int64_t ignore_index, bool vec,
                                                        const float* __restrict__ weight, double* __restrict__ part) {
  __shared__ float lds[kTileFloats];
  __shared__ double red[2][kRows];
  const Tile tile(lds, n, c);
  tile.load<T>(logits, vec);
  __syncthreads();
  const int64_t i = tile.row0 + threadIdx.x;
  double v[2] = {0.0, 0.0};             // {w * nll, w} of the row
  if (i < n) {
    const int64_t y = labels[i];
    if (label_ok(y, c, ignore_index)) {
      float x[kMaxClasses], mx;
      tile.own(x);
      const float xy = pick(x, c, (int)y);
      double sd;
      row_exp<double>(x, c, x, mx, sd);
      const float w = weight[y];
      v[0] = (double)(w * (logf((float)sd) + mx - xy));
      v[1] = (double)w;
    }
  }
  block_sum<2>(v, red);
  if (threadIdx.x == 0) { part[blockIdx.x * 2] = red[0][0]; part[blockIdx.x * 2 + 1] = red[1][0]; }
}

// out[0] = sum(w * nll) / sum(w) (0 / 0 = nan, as torch), out[1] = sum(w)          (single block, fixed order)
__global__ void __launch_bounds__(kRows) cew_final_kernel(const double* __restrict__ part, int64_t nblocks,
                                                          float* __restrict__ out) {
  __shared__ double red[2][kRows];
  sum_partials<2>(part, nblocks, red);
  if (threadIdx.x == 0) {
    out[0] = (float)(red[0][0] / red[1][0]);
    out[1] = (float)red[1][0];
  }
}

// dlogits = w[y] (softmax - onehot) gscale / sum(w)   (0 for ignored rows)
template <typename T>
__global__ void __launch_bounds__(kRows) cew_bwd_kernel(const T* __restrict__ logits, const int64_t* __restrict__ labels,
                                                        int64_t n, int c, int64_t ignore_index, bool vec,
                                                        const float* __restrict__ weight,
                                                        const float* __restrict__ fwd_out,
                                                        const float* __restrict__ gscale, T* __restrict__ dlogits) {
  __shared__ float lds[kTileFloats];
  const Tile tile(lds, n, c);
  tile.load<T>(logits, vec);
  __syncthreads();
  const int64_t i = tile.row0 + threadIdx.x;
  const int64_t y = i < n ? labels[i] : ignore_index;
  const bool ok = i < n && label_ok(y, c, ignore_index);
  float x[kMaxClasses];
  if (ok) {
    tile.own(x);
    row_softmax<double>(x, c, x);         // (f64 denominator: see lv_bwd_kernel)
  }
  const float k = ok ? weight[y] * (gscale[0] / fwd_out[1]) : 0.f;
#pragma unroll
  for (int j = 0; j < kMaxClasses; ++j)
    if (j < c) x[j] = ok ? (x[j] - (j == (int)y ? 1.f : 0.f)) * k : 0.f;
  tile.put(x);
  __syncthreads();
  tile.store<T>(dlogits, vec);
}

}  // namespace

extern "C" int64_t lidal_lovasz_workspace_bytes(int64_t n, int c) {
  if (c < 1 || c > kMaxClasses || n < 0 || n * (int64_t)c >= (1ll << 30)) return 0;      // refused by the entry point
  return lovasz_layout(nullptr, n, c).total;
}

extern "C" int lidal_lovasz_fwd(const void* x, int dtype, int is_probs, const int64_t* labels, int64_t n, int c,
                                int64_t ignore_index, int mode_all, double* out, float* grad, int32_t* ranks, void* ws,
                                int64_t ws_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (int rc = lovasz_check(n, c, dtype, is_probs)) return rc;
  const LovaszWs w = lovasz_layout(ws, n, c);
  LIDAL_REQUIRE(ws_bytes >= w.total, "lovasz workspace too small: %lld < %lld", (long long)ws_bytes, (long long)w.total);
  if (n > 0) {
    LIDAL_HIP(hipMemsetAsync(grad, 0, (size_t)n * c * 4, s));                        // ignored rows
    if (ranks != nullptr) LIDAL_HIP(hipMemsetAsync(ranks, 0xFF, (size_t)n * c * 4, s));      // ... have rank -1
  }
  const bool vec = aligned16(x);
  lv_count_kernel<<<(unsigned)w.nb, kRows, 0, s>>>(labels, n, c, ignore_index, w.bcnt);
  LIDAL_CHECK_LAUNCH("lovasz_count");
  lv_offsets_kernel<<<1, 1024, 0, s>>>(w.bcnt, w.nb, c, w.counts);
  LIDAL_CHECK_LAUNCH("lovasz_offsets");
  if (n > 0) {
    if (is_probs)
      lv_keys_kernel<float, true><<<(unsigned)w.nb, kRows, 0, s>>>((const float*)x, labels, n, c, ignore_index, vec,
                                                                   w.bcnt, w.counts, w.keys, w.vals);
    else if (dtype == LIDAL_F32)
      lv_keys_kernel<float, false><<<(unsigned)w.nb, kRows, 0, s>>>((const float*)x, labels, n, c, ignore_index, vec,
                                                                    w.bcnt, w.counts, w.keys, w.vals);
    else
      lv_keys_kernel<__bf16, false><<<(unsigned)w.nb, kRows, 0, s>>>((const __bf16*)x, labels, n, c, ignore_index, vec,
                                                                     w.bcnt, w.counts, w.keys, w.vals);
    LIDAL_CHECK_LAUNCH("lovasz_keys");
    int class_bits = 0;
    while ((1 << class_bits) < c) ++class_bits;
    if (int rc = radix_sort(w.keys, w.vals, w.keys_sorted, w.vals_sorted, n * c, 8, 32 + class_bits, w.sort, w.sort_bytes,
                            s, w.counts))
      return rc;
  }
  const dim3 tiles((unsigned)w.nt, (unsigned)c);
  lv_tiles_kernel<<<tiles, 256, 0, s>>>(w.vals_sorted, w.counts, w.nt, w.tsum);
  LIDAL_CHECK_LAUNCH("lovasz_tiles");
  lv_classes_kernel<<<(unsigned)c, 256, 0, s>>>(w.tsum, w.nt, w.gts);
  LIDAL_CHECK_LAUNCH("lovasz_classes");
  lv_grad_kernel<<<tiles, 256, 0, s>>>(w.keys_sorted, w.vals_sorted, w.counts, w.nt, c, w.tsum, w.gts, grad, ranks,
                                       w.lpart);
  LIDAL_CHECK_LAUNCH("lovasz_grad");
  lv_final_kernel<<<1, 64, 0, s>>>(w.lpart, w.counts, w.nt, c, mode_all, w.gts, out);
  LIDAL_CHECK_LAUNCH("lovasz_final");
  return 0;
}

extern "C" int lidal_lovasz_bwd(const void* x, int dtype, int is_probs, const int64_t* labels, int64_t n, int c,
                                int64_t ignore_index, int mode_all, const double* out, const float* grad,
                                const float* grad_scale, const float* grad_class, void* dx, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (int rc = lovasz_check(n, c, dtype, is_probs)) return rc;
  if (n == 0) return 0;
  const unsigned nb = (unsigned)cdiv(n, kRows);
  const bool vec = aligned16(x) && aligned16(dx), gvec = aligned16(grad);
  if (is_probs)
    lv_bwd_kernel<float, true><<<nb, kRows, 0, s>>>((const float*)x, labels, n, c, ignore_index, vec, gvec, mode_all, out,
                                                    grad, grad_scale, grad_class, (float*)dx);
  else if (dtype == LIDAL_F32)
    lv_bwd_kernel<float, false><<<nb, kRows, 0, s>>>((const float*)x, labels, n, c, ignore_index, vec, gvec, mode_all,
                                                     out, grad, grad_scale, grad_class, (float*)dx);
  else
    lv_bwd_kernel<__bf16, false><<<nb, kRows, 0, s>>>((const __bf16*)x, labels, n, c, ignore_index, vec, gvec, mode_all,
                                                      out, grad, grad_scale, grad_class, (__bf16*)dx);
  LIDAL_CHECK_LAUNCH("lovasz_bwd");
  return 0;
}

extern "C" int64_t lidal_ce_weighted_workspace_bytes(int64_t n) { return cdiv(n > 0 ? n : 1, kRows) * 16 + 256; }

extern "C" int lidal_ce_weighted_fwd(const void* logits, int dtype, const int64_t* labels, int64_t n, int c,
                                     int64_t ignore_index, const float* weight, float* out2, void* ws, int64_t ws_bytes,
                                     void* stream) {
  hipStream_t s = (hipStream_t)stream;
  LIDAL_REQUIRE(c >= 1 && c <= kMaxClasses, "weighted cross_entropy: classes must be in 1..%d", kMaxClasses);
  LIDAL_REQUIRE(n >= 0 && n * (int64_t)c < (1ll << 40), "weighted cross_entropy: %lld rows", (long long)n);
  LIDAL_REQUIRE(ws_bytes >= lidal_ce_weighted_workspace_bytes(n), "weighted cross_entropy workspace too small");
  const int64_t blocks = cdiv(n > 0 ? n : 1, kRows);
  const bool vec = aligned16(logits);
  if (int rc = with_dtype(dtype, "weighted cross_entropy", [&](auto t) {
        using T = decltype(t);
        cew_fwd_kernel<T><<<(unsigned)blocks, kRows, 0, s>>>((const T*)logits, labels, n, c, ignore_index, vec, weight,
                                                             (double*)ws);
        LIDAL_CHECK_LAUNCH("ce_weighted_fwd");
        return 0;
      }))
    return rc;
  cew_final_kernel<<<1, kRows, 0, s>>>((const double*)ws, blocks, out2);
  LIDAL_CHECK_LAUNCH("ce_weighted_final");
  return 0;
}

extern "C" int lidal_ce_weighted_bwd(const void* logits, int dtype, const int64_t* labels, int64_t n, int c,
                                     int64_t ignore_index, const float* weight, const float* fwd_out2,
                                     const float* grad_scale, void* dlogits, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  LIDAL_REQUIRE(c >= 1 && c <= kMaxClasses, "weighted cross_entropy: classes must be in 1..%d", kMaxClasses);
  if (n == 0) return 0;
  const unsigned nb = (unsigned)cdiv(n, kRows);
  const bool vec = aligned16(logits) && aligned16(dlogits);
  return with_dtype(dtype, "weighted cross_entropy", [&](auto t) {
    using T = decltype(t);
    cew_bwd_kernel<T><<<nb, kRows, 0, s>>>((const T*)logits, labels, n, c, ignore_index, vec, weight, fwd_out2, grad_scale,
                                           (T*)dlogits);
    LIDAL_CHECK_LAUNCH("ce_weighted_bwd");
    return 0;
  });
}
