// Panoptic quality for gfx950: the per-class sums behind PQ = SQ x RQ of predicted instances against annotated ones,
// accumulated on the device across calls (tests/panoptic_ref.py restates the definition in numpy,
// twice).  The procedure is the published one of the SemanticKITTI panoptic benchmark, in this project's own words.
//
// THE ROWS.  n_scans scans laid end to end; per row pred_sem, gt_sem (i64) and pred_inst, gt_inst (i32).  A row is VOID
// iff gt_sem is outside [0, C); void rows are absent from everything.  A non-void row has a predicted segment iff
// pred_sem is in [0, C).  A segment is (scan, class, id): id = 0 for a stuff class whatever the instance column holds,
// id = inst + 1 for a thing class (bit c of `things`), so inst = -1 ("no instance") is the class's one unassigned
// segment of that scan.  Instance values of thing rows lie in [-1, 2^30 - 2]: a gt_inst outside makes the row void, a
// pred_inst outside leaves the row without a predicted segment, and either raises LIDAL_PANOPTIC_BAD_ID.
//
// THE MATCH.  area = the non-void rows of a segment; inter = the rows in both a gt and a predicted segment of the same
// class; union = area_gt + area_pred - inter.  A pair matches iff 2 * inter > union, in integers.  For union < 2^30 this
// is the f64 test inter / union > 0.5: 2 * inter and union are integers below 2^31, so 2 * inter > union means
// 2 * inter >= union + 1 and inter / union >= 0.5 + 1 / (2 union) > 0.5 + 2^-31, eleven orders above the rounding of one
// f64 division; 2 * inter <= union gives a quotient <= 0.5 exactly, and rounding is monotone.
// A SEGMENT HAS AT MOST ONE MATCH: a match holds inter > union / 2 >= area / 2 rows of the segment, the partners of one
// segment are disjoint subsets of it, and two disjoint subsets cannot each hold more than half.  So the plain stores to
// the per-segment "matched" flags and IoU slots below have one writer each.
//
// THE SUMS, per call and class c: tp[c] += matches; fn[c] += gt segments with area >= min_points and no match;
// fp[c] += predicted segments with area >= min_points and no match; iou[c] = iou[c] + part[c], where part[c] starts at
// +0.0 and adds (double)inter / (double)union of the class's matches one by one in ascending (scan, gt id).  The
// division is the IEEE one, written as / (hipcc expands it to the correctly rounded sequence; the unit is built with
// -ffp-contract=off).  No float atomics: the order is a function of the input alone, and a permutation of the rows
// inside a scan gives the same 64 bits.
//
// THE KEYS.  class(6) | scan(5) | id(31) = 42 bits per row and side, all ones for "no segment" (class 63, scan 31 and
// id 2^31 - 1 cannot occur together: an id is below 2^30).  Class first: the sorted order is the summation order, and
// the segments of a class are one contiguous range.
//
// THE LAUNCHES.  keys (both sides) | per side: radix_sort with the row as payload, run heads, tiled_scan of the heads =
// a dense segment index per row, segment table (key, begin, end; the ends give the areas, no atomics) | pair keys
// gt segment << b | predicted segment for rows with both in one class (b = the bits of p) | radix_sort, keys only | one
// thread per run end: the run length is the intersection (its head by lower_bound), a match stores the two flags and
// the IoU at the gt segment | one wave per class: ballot counts of the class's two ranges, the IoUs summed in order by
// every lane alike, then the four accumulators.  Integer atomics only (the status word), vector stores only.
#include "cellsort.h"
#include "common.h"
#include "scan.h"

using namespace lidal;
using namespace lidal::cellsort;

namespace {

constexpr int PQ_BLOCK = 256;
constexpr int PQ_MAX_CLASSES = 64;
constexpr int PQ_MAX_SCANS = 32;
constexpr int PQ_ID_BITS = 31, PQ_SCAN_BITS = 5, PQ_CLASS_BITS = 6;
constexpr int PQ_KEY_BITS = PQ_CLASS_BITS + PQ_SCAN_BITS + PQ_ID_BITS;
constexpr int PQ_CLASS_SHIFT = PQ_SCAN_BITS + PQ_ID_BITS;
constexpr u64 PQ_NONE = ~0ull;
constexpr int64_t PQ_ID_MAX = (1ll << 30) - 2;      // the largest instance value

// ---------------------------------------------------------------- keys
// the segment key of class `sem` in scan `scan`, or PQ_NONE with *bad set when a thing's instance value is out of range
__device__ __forceinline__ u64 segment_key(int64_t sem, int inst, int scan, u64 things, bool* bad) {
  u64 id = 0;
  if ((things >> sem) & 1ull) {
    if (inst < -1 || inst > PQ_ID_MAX) { *bad = true; return PQ_NONE; }
    id = (u64)((int64_t)inst + 1);
  }
  return ((u64)sem << PQ_CLASS_SHIFT) | ((u64)scan << PQ_ID_BITS) | id;
}

__global__ void __launch_bounds__(PQ_BLOCK)
pq_keys_kernel(const int64_t* __restrict__ pred_sem, const int* __restrict__ pred_inst, const int64_t* __restrict__ gt_sem,
               const int* __restrict__ gt_inst, int64_t p, const int64_t* __restrict__ point_ptr, int n_scans, int c,
               u64 things, u64* __restrict__ gkey, u64* __restrict__ pkey, int* __restrict__ iota, long long* status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p) return;
  const int64_t gs = gt_sem[i], ps = pred_sem[i];
  u64 g = PQ_NONE, d = PQ_NONE;
  bool bad = false;
  if (gs >= 0 && gs < c) {
    const int scan = segment_of(point_ptr, n_scans, i);
    g = segment_key(gs, gt_inst[i], scan, things, &bad);
    if (g != PQ_NONE && ps >= 0 && ps < c) d = segment_key(ps, pred_inst[i], scan, things, &bad);
  }
  if (bad) raise(status, LIDAL_PANOPTIC_BAD_ID);
  gkey[i] = g;
  pkey[i] = d;
  iota[i] = (int)i;
}

// ---------------------------------------------------------------- one side: heads, dense indices, the segment table
__global__ void __launch_bounds__(PQ_BLOCK) pq_heads_kernel(const u64* __restrict__ skey, int64_t p, int* __restrict__ flag) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= p) return;
  const u64 k = skey[q];
  flag[q] = (k != PQ_NONE && (q == 0 || skey[q - 1] != k)) ? 1 : 0;
}

// incl = the inclusive scan of the heads.  seg_of[row] = the row's segment or -1; per segment its key, where its run
// begins and ends, matched = 0; n_seg = the number of segments.
__global__ void __launch_bounds__(PQ_BLOCK)
pq_segments_kernel(const u64* __restrict__ skey, const int* __restrict__ srow, const int* __restrict__ incl, int64_t p,
                   int* __restrict__ seg_of, u64* __restrict__ seg_key, int* __restrict__ seg_beg,
                   int* __restrict__ seg_end, int* __restrict__ matched, int* __restrict__ n_seg) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= p) return;
  if (q == p - 1) *n_seg = incl[q];
  const u64 k = skey[q];
  const int row = srow[q];
  if ((unsigned)row >= (unsigned)p) return;         // (cannot be: the payload is a permutation of the rows)
  const int seg = incl[q] - 1;
  if (k == PQ_NONE || seg < 0 || seg >= p) {        // (seg is in range by construction: at most one head per position)
    seg_of[row] = -1;
    return;
  }
  seg_of[row] = seg;
  if (q == 0 || skey[q - 1] != k) {
    seg_key[seg] = k;
    seg_beg[seg] = (int)q;
    matched[seg] = 0;
  }
  if (q == p - 1 || skey[q + 1] != k) seg_end[seg] = (int)q + 1;
}

// ---------------------------------------------------------------- pairs
__global__ void __launch_bounds__(PQ_BLOCK)
pq_pair_keys_kernel(const int64_t* __restrict__ pred_sem, const int64_t* __restrict__ gt_sem, const int* __restrict__ gseg,
                    const int* __restrict__ dseg, int64_t p, int bits, u64* __restrict__ key) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p) return;
  const int g = gseg[i], d = dseg[i];
  key[i] = (g >= 0 && d >= 0 && pred_sem[i] == gt_sem[i]) ? ((u64)g << bits) | (u64)d : PQ_NONE;
}

// one thread per position of the sorted pair keys; the last of a run does the work of its pair
__global__ void __launch_bounds__(PQ_BLOCK)
pq_match_kernel(const u64* __restrict__ skey, int64_t p, int bits, const int* __restrict__ gbeg, const int* __restrict__ gend,
                const int* __restrict__ dbeg, const int* __restrict__ dend, int* __restrict__ gmatched,
                int* __restrict__ dmatched, double* __restrict__ giou) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= p) return;
  const u64 k = skey[q];
  if (k == PQ_NONE || (q + 1 < p && skey[q + 1] == k)) return;
  const int64_t g = (int64_t)(k >> bits), d = (int64_t)(k & ((1ull << bits) - 1));
  if (g >= p || d >= p) return;                     // (cannot be: a segment index is below p)
  const int64_t inter = q + 1 - lower_bound(skey, 0, (int)q, k);
  const int64_t uni = (int64_t)(gend[g] - gbeg[g]) + (int64_t)(dend[d] - dbeg[d]) - inter;
  if (2 * inter > uni) {                            // at most one match per segment (the header): one writer per slot
    gmatched[g] = 1;
    dmatched[d] = 1;
    giou[g] = (double)inter / (double)uni;
  }
}

// ---------------------------------------------------------------- finalise: one wave per class
// the segments of class c among the n ascending segment keys: [*lo, *hi)
__device__ __forceinline__ void class_range(const u64* __restrict__ seg_key, int n, int c, int* lo, int* hi) {
  *lo = lower_bound(seg_key, 0, n, (u64)c << PQ_CLASS_SHIFT);
  *hi = lower_bound(seg_key, *lo, n, (u64)(c + 1) << PQ_CLASS_SHIFT);
}

// the segments of [lo, hi) without a match and with at least min_points rows; the same in every lane
__device__ __forceinline__ int64_t count_unmatched(const int* __restrict__ beg, const int* __restrict__ end,
                                                   const int* __restrict__ matched, int lo, int hi, int64_t min_points) {
  int64_t n = 0;
  for (int base = lo; base < hi; base += kWave) {
    const int t = base + lane_id();
    const bool miss = t < hi && !matched[t] && (int64_t)(end[t] - beg[t]) >= min_points;
    n += __popcll(__ballot(miss));
  }
  return n;
}

__global__ void __launch_bounds__(kWave)
pq_finalise_kernel(const u64* __restrict__ gkey, const int* __restrict__ gbeg, const int* __restrict__ gend,
                   const int* __restrict__ gmatched, const double* __restrict__ giou, const u64* __restrict__ dkey,
                   const int* __restrict__ dbeg, const int* __restrict__ dend, const int* __restrict__ dmatched,
                   const int* __restrict__ n_seg, int64_t p, int64_t min_points, int64_t* __restrict__ tp,
                   int64_t* __restrict__ fp, int64_t* __restrict__ fn, double* __restrict__ iou) {
  const int c = blockIdx.x, lane = lane_id();
  int ng = n_seg[0], nd = n_seg[1];
  if (ng < 0 || ng > p) ng = 0;                     // (cannot be: the counts are scan totals of at most p flags)
  if (nd < 0 || nd > p) nd = 0;
  int lo, hi;
  class_range(gkey, ng, c, &lo, &hi);
  const int64_t misses = count_unmatched(gbeg, gend, gmatched, lo, hi, min_points);
  int64_t hits = 0;
  double part = 0.0;
  for (int base = lo; base < hi; base += kWave) {
    const int t = base + lane;
    const bool hit = t < hi && gmatched[t];
    const double v = hit ? giou[t] : 0.0;
    u64 m = __ballot(hit);
    hits += __popcll(m);
    while (m) {                                     // ascending segments: every lane adds the same values in the same order
      const int l = __ffsll((long long)m) - 1;
      part += __shfl(v, l, kWave);
      m &= m - 1;
    }
  }
  class_range(dkey, nd, c, &lo, &hi);
  const int64_t extras = count_unmatched(dbeg, dend, dmatched, lo, hi, min_points);
  if (lane == 0) {
    tp[c] += hits;
    fn[c] += misses;
    fp[c] += extras;
    iou[c] = iou[c] + part;
  }
}

// ---------------------------------------------------------------- workspace: one routine for sizing and carving
struct Side {
  u64 *key, *seg_key;
  int *seg_of, *seg_beg, *seg_end, *matched;
};
struct PanopticWs {
  int64_t* point_ptr;
  int* n_seg;
  Side gt, pred;
  u64 *skey, *pair_key;
  int *iota, *srow, *flag, *incl, *sums;
  int64_t* offs;
  double* giou;
  char* sort;
  int64_t sort_bytes, total;
};
PanopticWs panoptic_layout(int64_t p_total, int n_scans, void* ws) {
  const int64_t p = p_total > 0 ? p_total : 1, ns = n_scans > 0 ? n_scans : 1, nb = scan_tiles(p);
  const int64_t sb = radix_sort_ws_bytes(p, 8, true);
  Carver c(ws);
  PanopticWs w;
  w.point_ptr = c.take<int64_t>(ns + 1);
  w.n_seg = c.take<int>(2);
  for (Side* s : {&w.gt, &w.pred}) {
    s->key = c.take<u64>(p); s->seg_key = c.take<u64>(p);
    s->seg_of = c.take<int>(p); s->seg_beg = c.take<int>(p); s->seg_end = c.take<int>(p); s->matched = c.take<int>(p);
  }
  w.skey = c.take<u64>(p); w.pair_key = c.take<u64>(p);
  w.iota = c.take<int>(p); w.srow = c.take<int>(p); w.flag = c.take<int>(p); w.incl = c.take<int>(p);
  w.sums = c.take<int>(nb);
  w.offs = c.take<int64_t>(nb + 1);
  w.giou = c.take<double>(p);
  w.sort = c.take(sb);
  w.sort_bytes = sb;
  w.total = c.total();
  return w;
}

// the rows of one side sorted by segment -> a dense segment index per row and the segment table
int build_side(const PanopticWs& w, const Side& side, int which, int64_t p, hipStream_t s) {
  const unsigned grid = (unsigned)cdiv(p, PQ_BLOCK);
  if (int rc = radix_sort(side.key, w.iota, w.skey, w.srow, p, 8, PQ_KEY_BITS, w.sort, w.sort_bytes, s)) return rc;
  pq_heads_kernel<<<grid, PQ_BLOCK, 0, s>>>(w.skey, p, w.flag);
  LIDAL_CHECK_LAUNCH("panoptic_heads");
  if (int rc = tiled_scan<int, true, false>(w.flag, p, w.sums, w.offs, w.incl, s)) return rc;
  pq_segments_kernel<<<grid, PQ_BLOCK, 0, s>>>(w.skey, w.srow, w.incl, p, side.seg_of, side.seg_key, side.seg_beg,
                                               side.seg_end, side.matched, w.n_seg + which);
  LIDAL_CHECK_LAUNCH("panoptic_segments");
  return 0;
}

}  // namespace

extern "C" int64_t lidal_panoptic_accumulate_workspace_bytes(int64_t p, int n_scans) {
  return panoptic_layout(p, n_scans, nullptr).total;
}

extern "C" int lidal_panoptic_accumulate(const int64_t* pred_sem, const int32_t* pred_inst, const int64_t* gt_sem,
                                         const int32_t* gt_inst, int64_t p, const int64_t* point_ptr_host, int n_scans,
                                         int c, uint64_t things, int64_t min_points, int64_t* tp, int64_t* fp, int64_t* fn,
                                         double* iou, int64_t* status, void* ws, int64_t ws_bytes, void* stream) {
  LIDAL_REQUIRE(n_scans >= 1 && n_scans <= PQ_MAX_SCANS, "panoptic_accumulate: 1..%d scans, not %d", PQ_MAX_SCANS, n_scans);
  LIDAL_REQUIRE(c >= 1 && c <= PQ_MAX_CLASSES, "panoptic_accumulate: 1..%d classes, not %d", PQ_MAX_CLASSES, c);
  LIDAL_REQUIRE(c == PQ_MAX_CLASSES || (things >> c) == 0, "panoptic_accumulate: a thing class beyond the %d classes", c);
  LIDAL_REQUIRE(min_points >= 1, "panoptic_accumulate: min_points must be at least 1");
  LIDAL_REQUIRE(point_ptr_host != nullptr, "panoptic_accumulate: point_ptr is a host array");
  LIDAL_REQUIRE(point_ptr_host[0] == 0, "panoptic_accumulate: point_ptr must start at 0");
  for (int s = 0; s < n_scans; ++s)
    LIDAL_REQUIRE(point_ptr_host[s + 1] >= point_ptr_host[s], "panoptic_accumulate: point_ptr must ascend (scan %d)", s);
  const int64_t P = p;
  LIDAL_REQUIRE(point_ptr_host[n_scans] == P, "panoptic_accumulate: point_ptr must end at p = %lld", (long long)P);
  // (the radix sort serves fewer than 2^30 items; a union is then below 2^30 as the match test needs)
  LIDAL_REQUIRE(P >= 0 && P < (1ll << 30), "panoptic_accumulate: %lld rows in a batch (fewer than 2^30)", (long long)P);
  const PanopticWs w = panoptic_layout(P, n_scans, ws);
  LIDAL_REQUIRE(ws_bytes >= w.total, "panoptic_accumulate: workspace too small");
  if (P == 0) return 0;                             // no row: nothing is launched, the sums stay as they are
  LIDAL_REQUIRE(pred_sem && pred_inst && gt_sem && gt_inst && tp && fp && fn && iou && status && ws,
                "panoptic_accumulate: a null array");

  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = (unsigned)cdiv(P, PQ_BLOCK);
  LIDAL_HIP(hipMemcpyAsync(w.point_ptr, point_ptr_host, 8 * (size_t)(n_scans + 1), hipMemcpyHostToDevice, s));
  pq_keys_kernel<<<grid, PQ_BLOCK, 0, s>>>(pred_sem, pred_inst, gt_sem, gt_inst, P, w.point_ptr, n_scans, c, things,
                                           w.gt.key, w.pred.key, w.iota, (long long*)status);
  LIDAL_CHECK_LAUNCH("panoptic_keys");
  if (int rc = build_side(w, w.gt, 0, P, s)) return rc;
  if (int rc = build_side(w, w.pred, 1, P, s)) return rc;
  int bits = 1;
  while ((1ll << bits) <= P) ++bits;                // a segment index is below P < 2^bits, the all-ones field is free
  pq_pair_keys_kernel<<<grid, PQ_BLOCK, 0, s>>>(pred_sem, gt_sem, w.gt.seg_of, w.pred.seg_of, P, bits, w.pair_key);
  LIDAL_CHECK_LAUNCH("panoptic_pair_keys");
  if (int rc = radix_sort(w.pair_key, nullptr, w.skey, nullptr, P, 8, 2 * bits, w.sort, w.sort_bytes, s)) return rc;
  pq_match_kernel<<<grid, PQ_BLOCK, 0, s>>>(w.skey, P, bits, w.gt.seg_beg, w.gt.seg_end, w.pred.seg_beg, w.pred.seg_end,
                                            w.gt.matched, w.pred.matched, w.giou);
  LIDAL_CHECK_LAUNCH("panoptic_match");
  pq_finalise_kernel<<<(unsigned)c, kWave, 0, s>>>(w.gt.seg_key, w.gt.seg_beg, w.gt.seg_end, w.gt.matched, w.giou,
                                                   w.pred.seg_key, w.pred.seg_beg, w.pred.seg_end, w.pred.matched, w.n_seg,
                                                   P, min_points, tp, fp, fn, iou);
  LIDAL_CHECK_LAUNCH("panoptic_finalise");
  return 0;
}
