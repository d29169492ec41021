// Thread-local error string, the thread-local tail event + version for the C-ABI.
#include <stdarg.h>
#include <stdio.h>

#include "common.h"

namespace lidal {
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// the tail event (common.h): at most one pending per host thread
static thread_local hipEvent_t g_tail_event = nullptr;
void set_tail_event(hipEvent_t ev) { g_tail_event = ev; }
hipEvent_t take_tail_event() {
  hipEvent_t ev = g_tail_event;
  g_tail_event = nullptr;
  return ev;
}
void clear_tail_event() { g_tail_event = nullptr; }
}  // namespace lidal

extern "C" const char* lidal_last_error(void) { return lidal::g_err; }
extern "C" int lidal_version(void) { return 166; }   // 1.66 (round 8): side-stream forks attached to the producing launch (lidal_plan_fork_counts); 1.65: Adam for every parameter tensor in one launch (lidal_adam_step); 1.64: fixed-radius neighbour lists of the supervoxel centres (lidal_radius_pairs_count, lidal_radius_pairs_fill); 1.63: frame-level selection (lidal_frame_uncertainty, lidal_segment_entropy, lidal_frame_feature, lidal_coreset); 1.62: ReDAL region selection (lidal_knn, lidal_surface_variation, lidal_region_scores, lidal_kmeans); 1.61 (round 6): the weight gradient on rule streams (lidal_wgrad_streams_build, lidal_conv_wgrad_streams, plan op 34), device-side item counts in sort.hip; 1.60 (round 6): data-gradient images in the split form (f32 training: lidal_conv_weight_image_job with LIDAL_F32_SPLIT and an img_bwd), the 32 x 32 x 16 MFMA forms of the split and lean kernels (measured slower, profiles/r06_mfma32_ab.txt; removed since, commit c7323ca is the last tree that has them); 1.41 (round 4): launch plans, row-wise helpers, conv offset split, NN grid cell in the header, block-tail BatchNorm sums, BatchNorm merges inside their consumers
