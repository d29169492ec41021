// The two k-means steps that kmeans.hip (lidal_kmeans) and supervoxel.hip (lidal_supervoxel_kmeans) share: the greedy
// k-means++ seeding and the deterministic centre update, with the workspace they carve (DESIGN.md sections 8 and 11).
// Defined in kmeans.hip.
#pragma once

#include "common.h"

namespace lidal {

// one layout routine, for sizing (ws == NULL) and for carving
struct KmWs {
  double *closest, *D, *cs, *tot, *off, *pot_t, *pot, *mind2, *cnew, *shift;
  int *cand, *best, *old, *keys, *iota, *skeys, *order, *counts, *starts, *changed;
  char* sort_tmp;
  int64_t sort_bytes, total;
};
KmWs km_layout(int64_t n_rows, int d, int k, int trials, void* ws);

// Greedy k-means++ from row `first` with the host-drawn uniforms u f64 [(k-1) * trials] (device): seeds i32 [k] and
// centers f64 [k,d] = the seed rows (device).  D^2, its scan and the candidates' potentials stay on the device.
int km_seed(const float* x, int64_t n, int d, int k, int64_t first, const double* u, int trials, int32_t* seeds,
            double* centers, const KmWs& w, hipStream_t s);

// w.iota = 0..n-1 (km_update sorts it by label)
int km_iota(int64_t n, const KmWs& w, hipStream_t s);

// New centres of `labels` with the per-cluster `counts` (device, i32 [k]): the sequential f64 sum of each cluster's rows
// in row order divided by the count, an empty cluster keeps its centre.  Leaves the rows sorted by (label, row) in
// w.order and the clusters' first positions in w.starts.  out may not alias centers.
int km_update(const float* x, int64_t n, int d, int k, const int32_t* labels, const int* counts, const double* centers,
              double* out, const KmWs& w, hipStream_t s);

}  // namespace lidal
