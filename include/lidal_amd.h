/* lidal_amd.h -- C-ABI of liblidal_amd.so, the MI355X (gfx950) backend of the LiDAL sparse-voxel
 * hot path.
 *
 * Every entry point replaces one function of the pybind module `torchsparse.backend`
 * (torchsparse==1.4.0, pinned at /root/reference/docs/requirements.txt:191; not vendored in the
 * reference) or one block of reference Python that runs on the hot path.  The "replaces" lines
 * cite the reference call site (relative to /root/reference) that reaches it.
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless the name ends in `_host`;
 *   - the caller owns every buffer (inputs, outputs, workspace).  The library allocates device memory in exactly
 *     ONE place: at the first fused BatchNorm launch on a device it takes 2 MiB of device memory (64 publication
 *     buffers, two per stream: up to 32 streams per device) and 64 pinned host bytes (an error word), with one
 *     hipDeviceSynchronize, and keeps them for the life of the process -- see lidal_bn_set_fused below;
 *     LIDAL_BN_FUSED=0 in the environment (or lidal_bn_set_fused(0) before the first BatchNorm call) avoids it;
 *   - every call only ENQUEUES work on `stream` (a hipStream_t passed as void*) and returns;
 *     counts that the host needs are written to device memory (`*_dev`) for the caller to read;
 *   - return value: 0 = OK, non-zero = error, message via lidal_last_error() (thread local);
 *   - no exceptions cross the boundary, no torch types in any signature;
 *   - dtype codes: 0 = float32, 1 = bfloat16 (features and weights; accumulation is always f32).
 */
#ifndef LIDAL_AMD_H
#define LIDAL_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LIDAL_F32 0
#define LIDAL_BF16 1
/* f32 features and f32 results with the products on the bf16 matrix cores: every operand cut into three bf16 pieces
 * (exactly: 8 + 8 + 8 significand bits), six partial products, f32 accumulation -- the error of an f32 dot product whose
 * products were rounded once more (<= 3 * 2^-24 relative per product), at 2.7x the f32 MFMA rate.  Accepted by
 * lidal_conv_weight_image[_bytes|_tiling] (the image it builds is the only one the code reads) and lidal_conv_apply_image
 * [_ws]; the reduction dimension must be a multiple of 32.  csrc/conv_img.hip: conv_split_kernel. */
#define LIDAL_F32_SPLIT 2

const char* lidal_last_error(void);
int lidal_version(void);

/* ---- hashing ------------------------------------------------------------------------------ */
/* replaces backend.hash_cuda  (F.sphash(coords): network/utils.py:17,42-47,75).
 * coords i32 [n,4] = (x,y,z,batch) -> out i64 [n]: FNV-1a-64 over the four 32-bit words folded to
 * 60 bits. */
int lidal_hash(const int32_t* coords, int64_t n, int64_t* out, void* stream);
/* network/utils.py:44-47,72-75: float rows (x, y, z, b) [n,4] -> int32 rows (floor(x/s) s, floor(y/s) s,
 * floor(z/s) s, (int)b), the voxel a point falls into at tensor stride s, in one pass. */
int lidal_floor_coords(const float* coords, int64_t n, int stride, int32_t* out, void* stream);
/* network/utils.py:14-17 (initial_voxelize): float rows (x, y, z, b) [n,4] -> out_float = ((x * init_res) / after_res,
 * ..., b) and out_floor = (int)floor(out_float), both [n,4]; IEEE f32 multiply and divide, as torch computes
 * `(C[:, :3] * init_res) / after_res` -- one pass instead of mul, div, cat, floor, int. */
int lidal_revoxelize_coords(const float* coords, int64_t n, float init_res, float after_res, float* out_float,
                            int32_t* out_floor, void* stream);
/* replaces backend.kernel_hash_cuda  (F.sphash(coords, offsets): network/utils.py:70-74).
 * offsets i32 [k,3]; out i64 [k,n], hash of (xyz + offset_k, batch). */
int lidal_kernel_hash(const int32_t* coords, int64_t n, const int32_t* offsets, int k,
                      int64_t* out, void* stream);

/* replaces backend.hash_query_cuda  (F.sphashquery: network/utils.py:19,48,76).
 * Open-addressing table of 64-bit keys in HBM; value = index of the FIRST occurrence of the key
 * (the CPU dense_hash_map::insert semantics).  Any i64 key is allowed: the all-ones key (-1), which marks an empty
 * slot, is kept in the header instead of a slot and found like any other.
 * The buffer holds cap = 2^k >= 2 n slots {key u64 | value i32} and an occupancy bitmap of 8 bits per slot that the
 * kernel-map probes test before they touch a slot (most probed neighbours do not exist), a second, SPATIAL bitmap of the
 * same size (x-contiguous, direct mapped: the three x-neighbours of a voxel in one word) and a 64-byte header. */
int64_t lidal_hash_table_bytes(int64_t n_keys);
int lidal_hash_table_build(const int64_t* keys, int64_t n, void* table, int64_t table_bytes,
                           void* stream);
/* The table of lidal_hash(coords) built from the coordinates themselves (one launch; `stride` = the tensor stride of the
 * level, a power of two): same slots and values, and the spatial bitmap is filled -- the symmetric kernel-map probes
 * (lidal_kmap_build[_batch] with symmetric = 1) then answer the 13 probed offsets of a 3x3x3 map from 5 word reads.
 * A table built by lidal_hash_table_build (bare keys) marks its spatial bitmap invalid and is probed through the
 * hashed one. */
int lidal_hash_table_build_coords(const int32_t* coords, int64_t n, int stride, void* table, int64_t table_bytes,
                                  void* stream);
/* out[i] = position of q[i] in the keys the table was built from, or -1. */
int lidal_hash_table_query(const void* table, int64_t table_bytes, const int64_t* q, int64_t nq,
                           int64_t* out, void* stream);

/* ---- sorted unique / downsample ------------------------------------------------------------- */
/* replaces torch.unique(pc_hash) in network/utils.py:18 (sorted unique of i64 keys).
 * out [n] capacity; n_out_dev i64[1].  Keys are 0 <= key < 2^63 (sphash output is 60 bit); a negative key is reported
 * as *n_out_dev = -1 (no other output is valid then). */
int64_t lidal_unique_workspace_bytes(int64_t n);
int lidal_unique_sorted_i64(const int64_t* keys, int64_t n, int64_t* out, int64_t* n_out_dev,
                            void* ws, int64_t ws_bytes, void* stream);
/* replaces F.spdownsample (torchsparse/nn/functional/downsample.py; reached from the four
 * stride-2 convs, network/spvcnn.py:28,34,40,46): xyz floored to multiples of `sample_stride`
 * (= conv stride x tensor stride), unique rows sorted by (batch,x,y,z).
 * Requires 0 <= x,y,z < 65536 and 0 <= batch < 32768; a row outside these ranges is reported as *n_out_dev = -1 (no
 * other output is valid then).  out i32 [n,4] capacity. */
int64_t lidal_downsample_workspace_bytes(int64_t n);
int lidal_downsample(const int32_t* coords, int64_t n, int sx, int sy, int sz, int32_t* out,
                     int64_t* n_out_dev, void* ws, int64_t ws_bytes, void* stream);

/* Every coarser level of a stride-2 encoder at once (the four F.spdownsample calls of network/spvcnn.py:28,34,
 * 40,46 chained): level l = 1..levels is the sorted unique of floor(c / (2^l s)) * (2^l s) over the rows of
 * `coords` (tensor stride s) -- the same rows in the same (batch, x, y, z) order as l chained lidal_downsample
 * calls, from ONE sort and with ONE set of row counts to read back.  out i32 [levels * n, 4] capacity; level l
 * occupies rows [starts[l-1], starts[l]); starts_dev i64 [levels + 1].  0 <= x, y, z < 65536, 0 <= batch < 8192,
 * levels <= 4; a row outside these ranges is reported as starts[levels] = -1 (no other output is valid then). */
int64_t lidal_downsample_pyramid_workspace_bytes(int64_t n, int levels);
int lidal_downsample_pyramid(const int32_t* coords, int64_t n, int sx, int sy, int sz, int levels, int32_t* out,
                             int64_t* starts_dev, void* ws, int64_t ws_bytes, void* stream);

/* ---- input voxelisation ("next" row 8f-1) ---------------------------------------------------- */
/* replaces dataset/sk_dataset.py:143-171 for one scan: affine augmentation p*M (f64), feats =
 * (transformed metres, intensity), x`scale`, random translation into [0, full_scale)^3 from the
 * global min/max and the host's six uniform draws rnd[6] (:156), astype(int), and
 * np.unique(axis=0, return_index=True, return_inverse=True).
 *   points f32 [p,3], intensity f32 [p], m_dev f64 [9] (row-major trans_m), rnd_dev f64 [6]
 *   feats_p f32 [p,4] (per point; caller gathers rows unique_idx), coords_v i32 [p,3] capacity
 *   (unique voxels, lexicographic x,y,z), unique_idx i64 [p] capacity (first occurrence),
 *   inverse i64 [p], n_out_dev i64 [1], n_invalid_dev i32 [1] (points outside the grid: the
 *   reference asserts there are none, :161). */
int64_t lidal_voxelize_points_workspace_bytes(int64_t p);
int lidal_voxelize_points(const float* points, const float* intensity, int64_t p,
                          const double* m_dev, const double* rnd_dev, double scale, int full_scale,
                          float* feats_p, int32_t* coords_v, int64_t* unique_idx, int64_t* inverse,
                          int64_t* n_out_dev, int32_t* n_invalid_dev, void* ws, int64_t ws_bytes,
                          void* stream);

/* The same for a WHOLE BATCH and its collate_fn (dataset/sk_dataset.py:188-242) in one call: n_samples <= 32 samples --
 * the scans of a training / validation batch, or the augmented views of ONE scan (dataset/sk_dataloader.py:199-203) --
 * from ONE sort of sample << 39 | x << 26 | y << 13 | z over all points, with ONE small buffer to read back.  Every
 * output equals, bit for bit, n_samples calls of lidal_voxelize_points collated as collate_fn does.
 *   points f32 [*,3], intensity f32 [*] (device); src_row0 / n_points i64 [n_samples] (HOST): sample j reads the
 *   source rows src_row0[j] .. src_row0[j] + n_points[j] (two samples may read the same rows) and owns the rows
 *   point_ptr[j] .. point_ptr[j+1] of the batch's concatenated point list, point_ptr = the running sum of n_points;
 *   p_total = point_ptr[n_samples] < 2^30.  m_dev f64 [n_samples,9], rnd_dev f64 [n_samples,6]: one matrix and one
 *   set of draws per sample.
 *   coords_v_b i32 [p_total,4] capacity (sample index in column 3), feats_v_b f32 [p_total,4] capacity (the feature
 *   row of each voxel's first-occurrence point, gathered inside the call), unique_idx i64 [p_total] capacity (first
 *   occurrence as a row of the concatenated point list), inverse_b i64 [p_total] (already offset by the voxels of the
 *   samples before, as collate_fn offsets it), counts_dev: voxel_ptr i64 [n_samples+1] (sample j's voxels are the
 *   rows voxel_ptr[j] .. voxel_ptr[j+1]) followed by n_invalid i32 [n_samples] (points outside the grid, per sample).
 *   A sample without points contributes no rows and no error. */
int64_t lidal_voxelize_batch_workspace_bytes(int64_t p_total, int n_samples);
int lidal_voxelize_batch(const float* points, const float* intensity, const int64_t* src_row0,
                         const int64_t* n_points, int n_samples, const double* m_dev, const double* rnd_dev,
                         double scale, int full_scale, int32_t* coords_v_b, float* feats_v_b, int64_t* unique_idx,
                         int64_t* inverse_b, int64_t* counts_dev, void* ws, int64_t ws_bytes, void* stream);

/* ---- training labels from the round's flags (csrc/labels.hip) ------------------------------------ */
/* replaces dataset/sk_dataset.py:106-141,170-171 (and dataset/nu_dataset.py:128-160,189-190) for one scan:
 *   raw         the bytes of the annotation file, u32 [p] (raw_bytes == 4, SemanticKITTI: `labels_anno_p & 0xFFFF`,
 *               :111, drops the instance id) or u8 [p] (raw_bytes == 1, nuScenes, nu_dataset.py:130)
 *   label_map   i64 [map_len <= 1024] (:113 `self.label_map[labels_anno_p].astype(np.int64)`); an id >= map_len is an
 *               IndexError there: here it is counted in *n_invalid_dev and the annotated label reads as 255
 *   sv_ptr i64 [s+1], sv_idx i64 [nnz], sv_flag i64 [s]: the supervoxel CSR of lidal_segment_entropy and the round's
 *               flags.  :129-133 `label_anno_mask[p_ids] = False` for each `sv_flag == 1`, `labels_p[label_anno_mask]
 *               = 255`: a point keeps its label only if at least one flag-1 supervoxel lists it (overlapping lists are
 *               a union; a point in no list ends at 255).  All three NULL (s = nnz = 0): every point keeps its label
 *               ('train', 'train_frame', 'val').  A list outside [0, nnz) or an index outside [0, p) is counted in
 *               *n_invalid_dev and skipped.
 *   pseudo      i64 [p] or NULL.  :137-141 `labels_p[label_pseudo_mask] = labels_pseudo_p[label_pseudo_mask]`: a point
 *               listed by at least one flag-2 supervoxel takes pseudo[point], after the mask (it wins where both
 *               apply).  NULL: flag 2 means nothing ('train_sv').
 *   unique_idx  i64 [n] or NULL / 0.  :171 `labels_v = labels_p[unique_idxs]` (an index outside [0, p): counted, 255)
 *   labels_p i64 [p] (16-byte aligned), labels_v i64 [n], n_invalid_dev i32 [1] (set by every call).
 * No host read.  Workspace: lidal_train_labels_workspace_bytes(p) (two bits per point; unused without flags). */
int64_t lidal_train_labels_workspace_bytes(int64_t p);
int lidal_train_labels(const void* raw, int raw_bytes, int64_t p, const int64_t* label_map, int map_len,
                       const int64_t* sv_ptr, const int64_t* sv_idx, int64_t nnz, int s, const int64_t* sv_flag,
                       const int64_t* pseudo, const int64_t* unique_idx, int64_t n, int64_t* labels_p,
                       int64_t* labels_v, int32_t* n_invalid_dev, void* ws, int64_t ws_bytes, void* stream);

/* ---- mixed training samples: LaserMix / PolarMix style batches (csrc/mix.hip) ------------------ */
/* The project's own definition; nothing in the reference does this.  The input is a list of
 * scans laid end to end: xyz f32 [p_total,3], intensity f32 [p_total], labels i64 [p_total] or NULL.  A mix names two
 * row ranges A and B of that list and, per point (every f32 operation rounded on its own, no fma),
 *     r    = sqrtf(x*x + y*y)
 *     band = #{ j < n_tans : z >= tans[j] * r }
 *     inw  = has_wedge and wedge[0]*y - wedge[1]*x >= 0 and wedge[2]*y - wedge[3]*x < 0
 *     cell = band + (n_tans + 1) * inw                                              (< 64)
 * Its output rows are, in this order and inside each part in source order: the rows of A whose cell bit is set in
 * take_a; the rows of B whose cell bit is set in take_b; and for each rotation k < n_rot the rows of B with a label in
 * 0..63 whose bit is set in paste_classes, with x' = c*x - s*y, y' = s*x + c*y, z' = z, (c, s) = rot[2k], rot[2k+1]. */
#define LIDAL_MIX_MAX 32          /* mixes in one call */
#define LIDAL_MIX_MAX_TANS 31
#define LIDAL_MIX_MAX_ROT 4
#define LIDAL_MIX_PARTS 6         /* A, B and four pastes */
typedef struct lidal_mix_desc {   /* 256 bytes */
  int64_t a0, na, b0, nb;         /* A = rows a0 .. a0 + na of the input list, B = rows b0 .. b0 + nb (they may overlap) */
  uint64_t take_a, take_b;        /* one bit per cell; no bit at or above (n_tans + 1) * (1 + has_wedge) */
  uint64_t paste_classes;         /* one bit per class id 0..63 */
  int32_t n_tans, has_wedge, n_rot, reserved;
  float wedge[4];                 /* (d0x, d0y, d1x, d1y) */
  float rot[2 * LIDAL_MIX_MAX_ROT];
  float tans[LIDAL_MIX_MAX_TANS]; /* ascending, finite */
  int32_t pad[3];
} lidal_mix_desc;
/*   mixes_host  n_mixes <= 32 descriptors in HOST memory; the call uploads them once (they must stay valid until the
 *               stream has passed the call).  The slot space of mix m is na + nb * (1 + n_rot); n_slots is its sum over
 *               the mixes and must be below 2^30.
 *   out_xyz f32 [n_slots,3], out_intensity f32 [n_slots], out_labels i64 [n_slots] (NULL exactly when labels is; a
 *   paste then is refused), out_src i64 [n_slots]: the input row each output row was taken from (the B row for a
 *   paste).  Rows at and above point_ptr[n_mixes] are not written.
 *   counts_dev i64 [n_mixes + 1 + 6 n_mixes]: point_ptr (mix m owns the output rows point_ptr[m] .. point_ptr[m+1])
 *   followed by parts [n_mixes,6], the row counts of A, B and the four pastes.
 * Three launches (per-block counts, their scan, the ordered write), no atomics, no memset.  Workspace:
 * lidal_mix_scans_workspace_bytes(n_slots, n_mixes). */
int64_t lidal_mix_scans_workspace_bytes(int64_t n_slots, int n_mixes);
int lidal_mix_scans(const float* xyz, const float* intensity, const int64_t* labels, int64_t p_total,
                    const lidal_mix_desc* mixes_host, int n_mixes, float* out_xyz, float* out_intensity,
                    int64_t* out_labels, int64_t* out_src, int64_t* counts_dev, void* ws, int64_t ws_bytes,
                    void* stream);

/* ---- kernel map (rule) building -------------------------------------------------------------- */
/* replaces the cache-miss branch of F.conv3d (torchsparse/nn/functional/conv.py): kernel_hash +
 * hash_query + nonzero.  `table` was built from sphash(in_coords).
 *   nbr_out  i32 [k, n_out]     input row feeding output row j through offset k, or -1
 *                               (in_coord = out_coord + offset_k)
 *   nbmaps   i32 [k*n_out, 2]   capacity; rows (in_idx, out_idx) grouped by k, ascending out_idx
 *                               -- bit-exact torchsparse order
 *   nbsizes  i32 [k],  koff i64 [k+1] exclusive prefix of nbsizes (koff[k] = total rules).
 * symmetric != 0 declares that out_coords are the coordinates the table was built from and that
 * offsets[k-1-j] == -offsets[j] (odd centred kernel at stride 1): half of the probes are then
 * replaced by mirroring (rule (i,j,k) <=> rule (j,i,k-1-j)); the result is identical.
 * mode 0 builds everything; mode 1 only nbr_out (all the forward / inference path reads; nbmaps,
 * nbsizes, koff may be NULL); mode 2 derives nbmaps / nbsizes / koff from an nbr_out built earlier
 * (the weight gradient reads them; table / out_coords / offsets are then ignored). */
int64_t lidal_kmap_workspace_bytes(int64_t n_out, int k);
int lidal_kmap_build(const void* table, int64_t table_bytes, const int32_t* out_coords,
                     int64_t n_out, const int32_t* offsets, int k, int symmetric, int32_t* nbr_out,
                     int32_t* nbmaps, int32_t* nbsizes, int64_t* koff, int mode, void* ws,
                     int64_t ws_bytes, void* stream);
/* From torchsparse-order rule lists (what backend.convolution_forward_cuda(in, out, W, nbmaps, nbsizes,
 * transposed) receives: nbmaps i32 [n_rules, 2] = (in, out) grouped by offset, nbsizes i32 [k], both on
 * the device; n_rules = capacity of nbmaps >= sum(nbsizes)) to the neighbour table lidal_kmap_order /
 * lidal_conv_apply_image consume: nbr_out i32 [k, n_out], -1 where an offset has no rule for a row.
 * n_bad_dev i32 [1] counts rules with an index out of range (0 = fine). */
int lidal_kmap_from_rules(const int32_t* nbmaps, const int32_t* nbsizes, int k, int64_t n_rules,
                          int64_t n_in, int64_t n_out, int32_t* nbr_out, int32_t* n_bad_dev, void* stream);
/* All kernel maps of a network in one chain of launches (n_jobs <= 12; HOST arrays of length n_jobs holding,
 * per map, the arguments of lidal_kmap_build; nbsizes[j] == NULL: neighbour table only): every stage (fill,
 * probe, count, scan, compact, sizes) is one launch over all maps.  Results per map are those of
 * lidal_kmap_build, an empty level (n_out[j] == 0: nbsizes and koff all zero) and every kernel volume it takes
 * (k <= 1023) included.  ws >= lidal_kmap_build_batch_workspace_bytes(n_out, k, n_jobs). */
int64_t lidal_kmap_build_batch_workspace_bytes(const int64_t* n_out, const int32_t* k, int n_jobs);
int lidal_kmap_build_batch(const void* const* tables, const int64_t* table_bytes,
                           const int32_t* const* out_coords, const int64_t* n_out,
                           const int32_t* const* offsets, const int32_t* k, const int32_t* symmetric,
                           int32_t* const* nbr_out, int32_t* const* nbmaps, int32_t* const* nbsizes,
                           int64_t* const* koff, int n_jobs, void* ws, int64_t ws_bytes, void* stream);
/* nbr_in i32 [k, n_in]: output row fed by input row i through offset k, or -1 (inverse table, used
 * by data-gradient and transposed convolution). */
int lidal_kmap_invert(const int32_t* nbr_out, int64_t n_out, int k, int32_t* nbr_in, int64_t n_in,
                      void* stream);

/* Row order for lidal_conv_apply: rows of nbr [k, n_rows] sorted by their occupancy pattern (bit j set
 * iff nbr[j][row] >= 0; stable, so ties keep row order).  perm i32 [n_rows] (sorted position ->
 * row), nbr_perm i32 [k, n_rows] = nbr[:, perm], tile_masks u32 [ceil(n_rows/128)] = OR of the row
 * patterns of each 128-row tile (may be NULL).  With them a tile only touches the offsets of its
 * own patterns. */
/* the library's own stable LSD radix sort (csrc/sort.hip: Onesweep, 8 bits per pass, 1 + ceil(bits/8)
 * launches) of (u32 or u64 key, i32 value) pairs by the low `bits` key bits -- what every sorted order
 * of this library comes from (row orders, torch.unique of hashes / packed coordinates, contributor
 * lists, the scorer's cell keys); exported for tests.  keys_in / vals_in are not written;
 * ws >= lidal_sort_pairs_workspace_bytes(n). */
int64_t lidal_sort_pairs_workspace_bytes(int64_t n);
int lidal_sort_pairs(const uint32_t* keys_in, const int32_t* vals_in, uint32_t* keys_out, int32_t* vals_out,
                     int64_t n, int bits, void* ws, int64_t ws_bytes, void* stream);
int lidal_sort_pairs_u64(const uint64_t* keys_in, const int32_t* vals_in, uint64_t* keys_out, int32_t* vals_out,
                         int64_t n, int bits, void* ws, int64_t ws_bytes, void* stream);
int64_t lidal_kmap_order_workspace_bytes(int64_t n_rows);
/* The same for n_jobs (<= 16) tables of ONE kernel volume k in one go (host arrays of device pointers /
 * row counts; ws >= lidal_kmap_order_workspace_bytes(sum of the row counts)): one key array, one sort.
 * Results are identical to n_jobs calls of lidal_kmap_order. */
int lidal_kmap_order_batch(const int32_t* const* nbr, const int64_t* n_rows, int n_jobs, int k,
                           int32_t* const* perm, int32_t* const* nbr_perm, uint32_t* const* tile_masks,
                           void* ws, int64_t ws_bytes, void* stream);
int lidal_kmap_order(const int32_t* nbr, int64_t n_rows, int k, int32_t* perm, int32_t* nbr_perm,
                     uint32_t* tile_masks, void* ws, int64_t ws_bytes, void* stream);

/* ---- point <-> voxel ------------------------------------------------------------------------- */
/* replaces backend.count_cuda (F.spcount: network/utils.py:20,49). out i32 [m] (zeroed here). */
int lidal_count(const int32_t* idx, int64_t n, int32_t* out, int64_t m, void* stream);
/* replaces backend.voxelize_forward_cuda / voxelize_backward_cuda (F.spvoxelize:
 * network/utils.py:22,25,56).  out[idx[i]] += feat[i] / counts[idx[i]]; f32 only. */
int lidal_voxelize_fwd(const float* feat, const int32_t* idx, const int32_t* counts, float* out,
                       int64_t n, int64_t m, int c, void* stream);
/* The same when every voxel holds exactly one point (idx a permutation of 0..n-1; LiDAL's scans arrive
 * voxelised, network/spvcnn.py:114): out[idx[i]] = feat[i], bit-equal to the mean form, f32 or bf16 rows. */
int lidal_voxelize_fwd_1to1(const void* feat, const int32_t* idx, void* out, int64_t n, int c, int dtype,
                            void* stream);
/* backward: gin[i] = gout[idx[i]] / counts[idx[i]] (+ residual[i], same dtype [n, c], may be NULL:
 * the gradient reaching the same point rows through a second consumer of the features). */
int lidal_voxelize_bwd(const void* gout, const int32_t* idx, const int32_t* counts,
                       const void* residual, void* gin, int64_t n, int64_t m, int c, int dtype,
                       void* stream);
/* replaces backend.devoxelize_forward_cuda / devoxelize_backward_cuda (F.spdevoxelize:
 * network/utils.py:83,95).  idx i32 [n,8], w f32 [n,8]; out[i] = sum_k w[i,k] feat[idx[i,k]]. */
int lidal_devoxelize_fwd(const void* feat, const int32_t* idx, const float* w, void* out,
                         int64_t n, int64_t m, int c, int dtype, void* stream);
int lidal_devoxelize_bwd(const float* gout, const int32_t* idx, const float* w, float* gin,
                         int64_t n, int64_t m, int c, void* stream);
/* (n_entries = length of `order`; lists averaging >= 32 contributors per voxel are split over
 * several waves / workgroups per voxel, ws from lidal_segment_workspace_bytes, may be NULL if 0) */
/* Atomic-free, bitwise reproducible forms of the two scatter sums above.  A point->voxel index
 * idx i32 [n_entries] (n_entries = n for voxelize, 8n for devoxelize: entry = point*8 + corner) is
 * transposed once into per-voxel contributor lists: order i32 [n_entries] (entries sorted by voxel,
 * ascending inside a voxel; entries with idx < 0 or weight 0 at the end), seg_ptr i64 [m+1]. */
int64_t lidal_invlist_workspace_bytes(int64_t n_entries);
int lidal_invlist_build(const int32_t* idx, const float* w, int64_t n_entries, int64_t m,
                        int32_t* order, int64_t* seg_ptr, void* ws, int64_t ws_bytes, void* stream);
int64_t lidal_segment_workspace_bytes(int64_t n_entries, int64_t m, int c);
/* Which kernel the two ordered sums below launch for these arguments (the choice follows the average list length
 * n_entries / m, the voxel count, the row width and the element type -- never the lists themselves): 0 a lane group per
 * voxel, 1 one wave per voxel, 11 / 12 / 14 a workgroup kernel with 1 / 2 / 4 workgroups per voxel (12 and 14 through f32
 * partial rows in ws and a fold); -1 what they do not take.  A query: nothing is launched. */
int64_t lidal_segment_form(int64_t n_entries, int64_t m, int c, int dtype);
int lidal_voxelize_fwd_sorted(const void* feat, const int32_t* order, const int64_t* seg_ptr,
                              const int32_t* counts, void* out, int64_t m, int c, int dtype,
                              int64_t n_entries, void* ws, int64_t ws_bytes, void* stream);
int lidal_devoxelize_bwd_sorted(const void* gout, const int32_t* order, const int64_t* seg_ptr,
                                const float* w, void* gin, int64_t m, int c, int dtype,
                                int64_t n_entries, void* ws, int64_t ws_bytes, void* stream);
/* The same gradient through the CELLS, for levels where a voxel has many contributors (stride 16): every point of a cell --
 * the voxel its own coordinates floor to, idx8[:, 0] -- interpolates from the same eight corners (network/utils.py:67-79),
 * so  cs[cell][j] = sum over the cell's points of w8[p][j] * gout[p]  (vorder / vseg: the points of every cell, the inverse
 * lists of idx8[:, 0])  and  gin[v] = sum of the cs[cell][j] whose corner j is v  (corder / cseg: the inverse lists of the
 * cells' [m, 8] corner indices, entries cell * 8 + j).  Reads every gradient row once instead of eight times.  Fixed
 * orders, no atomics; differs from lidal_devoxelize_bwd_sorted by the association of the f32 sums.  c in {32, 64, 128, 256}
 * (any power of two of 16-byte steps, 4 .. 64); ws >= lidal_devoxelize_bwd_cells_workspace_bytes(m, c) = m * 8 * c * 4. */
int64_t lidal_devoxelize_bwd_cells_workspace_bytes(int64_t m, int c);
int lidal_devoxelize_bwd_cells(const void* gout, const int32_t* vorder, const int64_t* vseg, const float* w8,
                               const int32_t* corder, const int64_t* cseg, void* gin, int64_t m, int c, int dtype,
                               void* ws, int64_t ws_bytes, void* stream);
/* replaces F.calc_ti_weights (torchsparse/nn/functional/devoxelize.py; network/utils.py:77):
 * coords f32 [n, cstride>=3], idx i64 [8,n] -> w f32 [n,8] and idx32 i32 [n,8] (both already
 * transposed as network/utils.py:78-79 does). */
int lidal_ti_weights(const float* coords, int cstride, const int64_t* idx, int64_t n, float scale,
                     float* w, int32_t* idx32, void* stream);

/* ---- sparse convolution ---------------------------------------------------------------------- */
/* replaces backend.convolution_forward_cuda and the data-gradient half of
 * convolution_backward_cuda (every spnn.Conv3d.forward/backward, 49 per model pass).
 * Output-stationary fused gather-GEMM with register accumulators:
 *     out[row(j), :] = sum_k  in[ nbr[kk][j], : ] * W[k],   kk = kflip ? K-1-k : k
 * with nbr i32 [k, n_out] (-1 = no rule) and row(j) = perm ? perm[j] : j  (pass lidal_kmap_order's perm together
 * with its permuted table and its tile_masks, which spare the kernel the offsets a tile has no rule for).
 * n_in = rows of `in` (every nbr entry is < n_in; in and the weights are addressed with 32-bit byte offsets, so
 * each must stay below 2 GiB).  No atomics: each output row is written exactly once => bitwise reproducible.
 * Optional epilogue (inference: the eval-mode spnn.BatchNorm and ReLU that follow the conv in
 * network/utils.py:110-114,147-155): ep_scale / ep_shift f32 [co] (both or neither; see
 * lidal_bn_fold) give out = act(acc * scale + shift), act = ReLU iff (ep_relu & 1); ep_residual
 * (NULL or a [n_out, co] matrix of the output's dtype) is added to that, row for row (the
 * point-branch sum network/spvcnn.py:136,143,151; the shortcut of a residual block,
 * network/utils.py:171, whose ReLU comes AFTER the sum: ep_relu & 2).  With k = 1 and nbr = NULL
 * (the identity rule list) the same kernel is the dense per-row product of the 1x1x1 convolutions
 * and nn.Linear layers.
 * (Rounds 1-3 also exported a first generation, lidal_conv_apply + lidal_conv_weight_pack, with plain [k][co][ci]
 * weights staged through registers; it left the library in round 4 and lives on as a test-only object,
 * tests/native/conv_gen1.hip, that the kernels below are compared with bit for bit.)
 * The weights are supplied as LDS IMAGES (csrc/conv_img.hip) -- every slab (offset, column block, reduction slice)
 * laid out in global memory exactly as the MFMA B-fragment reads want it in LDS, so the kernel stages a slab by
 * LDS-DMA (no vector registers, no ds_write) and reads it bank-conflict free.
 *   lidal_conv_weight_image_bytes  size of the image of a [k][n_red][n_col] weight for a
 *                                  convolution producing n_out rows (the tiling depends on it)
 *   lidal_conv_weight_image        role 0: w is [k][n_red][n_col] (forward: n_red = ci, n_col = co)
 *                                  role 1: w is [k][n_col][n_red] (data gradient of the same
 *                                  parameter: n_red = co, n_col = ci); casts to `dtype`
 *   lidal_conv_apply_image         the contraction above; wimg = the image built for the
 *                                  SAME (ci = n_red, co = n_col, k, dtype, n_out); tile_masks are
 *                                  required with a table (nbr == NULL: identity rule list, k = 1);
 *                                  ci must be a multiple of 4 (f32) / 8 (bf16).
 * tile_stats (NULL or f32 [co][ceil(n_out / 128)][3] -- column-major over the tiles, so that the merge of a channel
 * reads one contiguous run): per output column and 128-row tile of the kernel's row order, (count, mean, M2) of the values as stored -- the batch statistics of a train-mode
 * BatchNorm that follows (network/utils.py:115), taken in the epilogue instead of by a pass over the
 * stored matrix; merged by lidal_bn_train_fwd_tiles. */
/* Rows per tile of the per-tile BatchNorm statistics lidal_conv_apply_image can leave (tile_stats is
 * f32 [ceil(n_out / rows), co, 3]): size the buffer from this, not from a constant. */
int lidal_conv_stats_tile_rows(void);
int64_t lidal_conv_weight_image_bytes(int k, int ci, int co, int dtype, int64_t n_out);
/* identifies the tiling an image is built for (two n_out with the same value share images: a
 * host-side cache key for weights that do not change between calls, i.e. inference) */
int lidal_conv_weight_image_tiling(int ci, int co, int dtype, int64_t n_out);
int lidal_conv_weight_image(const void* w, int w_dtype, int role, void* img, int dtype, int k,
                            int n_red, int n_col, int64_t n_out, void* stream);
/* both images of one [k][ci][co] parameter in ONE launch: img_fwd (role 0, for a convolution
 * producing n_out_fwd rows) and img_bwd (role 1, for its data gradient producing n_out_bwd rows) */
int lidal_conv_weight_image_pair(const void* w, int w_dtype, void* img_fwd, int64_t n_out_fwd,
                                 void* img_bwd, int64_t n_out_bwd, int dtype, int k, int ci, int co,
                                 void* stream);
/* the image pairs of MANY parameters in one launch (training: every weight changes every step).
 * lidal_conv_weight_image_job fills one host record of lidal_conv_weight_image_job_bytes() bytes
 * (role 0: w is [k][ci][co], role 1: [k][co][ci] = nn.Linear's layout; `first` = segments of the
 * records before it; returns this record's segment count, < 0 on error);
 * lidal_conv_weight_image_batch takes the records as a DEVICE array. */
int lidal_conv_weight_image_job_bytes(void);
int64_t lidal_conv_weight_image_job(void* job, const void* w, int role, void* img_fwd,
                                    int64_t n_out_fwd, void* img_bwd, int64_t n_out_bwd, int dtype,
                                    int k, int ci, int co, int64_t first);
int lidal_conv_weight_image_batch(const void* jobs, int n_jobs, int64_t total_segments, int w_dtype,
                                  int dtype, void* stream);
int lidal_conv_apply_image(const void* in, const void* wimg, const int32_t* nbr, const int32_t* perm,
                           const uint32_t* tile_masks, void* out, int64_t n_in, int64_t n_out,
                           int ci, int co, int k, int kflip, int dtype, const float* ep_scale,
                           const float* ep_shift, int ep_relu, const void* ep_residual,
                           float* tile_stats, void* stream);
/* lidal_conv_apply_image with a workspace (ws >= lidal_conv_apply_workspace_bytes(n_out, co), may be NULL / 0): on the
 * coarse levels -- few 128-row tiles, each a long chain of (offset, reduction slice) phases while most of the chip
 * idles -- the launch then SPLITS every tile's active offsets over 2-4 workgroups, which leave f32 partial tiles in
 * ws; a second kernel adds them in a fixed order and runs the epilogue (permutation, affine map / ReLU / residual,
 * BatchNorm tile statistics).  bf16 only.  Which launches split is a function of (n_out, ci, co, k, dtype) alone; results differ
 * from the unsplit kernel's only by the association of the f32 sum over the offsets (~1e-7 relative before the
 * rounding to the output dtype). */
int64_t lidal_conv_apply_workspace_bytes(int64_t n_out, int co);
int lidal_conv_apply_image_ws(const void* in, const void* wimg, const int32_t* nbr, const int32_t* perm,
                              const uint32_t* tile_masks, void* out, int64_t n_in, int64_t n_out,
                              int ci, int co, int k, int kflip, int dtype, const float* ep_scale,
                              const float* ep_shift, int ep_relu, const void* ep_residual,
                              float* tile_stats, void* ws, int64_t ws_bytes, void* stream);
/* The data gradient of a convolution whose INPUT was y = act(bn(x)) (torchsparse: convolution_backward_cuda's
 * grad_input half, followed by the BatchNorm backward of network/utils.py:115): lidal_conv_apply_image on
 * (gout, data-gradient image) -> gin, and in the same launch the backward sums of that BatchNorm per 128-row
 * tile of gin's rows: bn_sums f32 [c_gin, ceil(n_gin / tile rows), 2] = (sum dy', sum dy' xhat), dy' = gin where
 * the fused ReLU (bn_relu) let the value through, xhat = (bn_x - mean) * invstd; bn_x [n_gin, c_gin] in `dtype`.
 * Feed bn_sums to lidal_bn_bwd_tiles.  c_gin must be whole 16-byte vectors. */
int lidal_conv_dgrad_bn_sums(const void* gout, const void* wimg, const int32_t* nbr, const int32_t* perm,
                             const uint32_t* tile_masks, void* gin, int64_t n_gout, int64_t n_gin, int c_gout,
                             int c_gin, int k, int kflip, int dtype, const void* bn_x, const float* bn_mean,
                             const float* bn_invstd, const float* bn_gamma, const float* bn_beta, int bn_relu,
                             float* bn_sums, void* stream);
/* (the same with the workspace of lidal_conv_apply_image_ws) */
int lidal_conv_dgrad_bn_sums_ws(const void* gout, const void* wimg, const int32_t* nbr, const int32_t* perm,
                                const uint32_t* tile_masks, void* gin, int64_t n_gout, int64_t n_gin, int c_gout,
                                int c_gin, int k, int kflip, int dtype, const void* bn_x, const float* bn_mean,
                                const float* bn_invstd, const float* bn_gamma, const float* bn_beta, int bn_relu,
                                float* bn_sums, void* ws, int64_t ws_bytes, void* stream);
/* replaces the weight-gradient half of backend.convolution_backward_cuda:
 *     gw[k] = a[ pairs[:, a_col] ]^T  *  b[ pairs[:, 1 - a_col] ]      (f32 [k][ca][cb])
 * pairs = nbmaps i32 [M,2], koff i64 [k+1] (device); n_a, n_b = rows of a and b.
 * pairs == NULL means the identity rule list (row p with row p): the weight gradient of a dense
 * [n, ca]^T x [n, cb] product (1x1x1 convolutions and the point-branch Linear layers), where a
 * library GEMM would run its whole n-long reduction in a handful of workgroups.
 * The reduction over the rules is split between workgroups; each leaves an f32 [ca][cb] slab in
 * `partial` (n_slabs slabs, at least lidal_conv_wgrad_slabs(...) of them) and a second kernel adds
 * the slabs of every offset in a fixed order => bitwise reproducible, no atomics.  bf16 with
 * ca, cb multiples of 8: W equally long runs of 64-rule stages, one per resident workgroup,
 * gathered by LDS-DMA (csrc/wgrad_dma.hip); otherwise split-K slabs per offset (csrc/conv.hip).
 * dtype LIDAL_F32_SPLIT (round 6): a and b are F32; every product runs as six bf16 MFMAs on the operands' three exact bf16
 * pieces (as LIDAL_F32_SPLIT of lidal_conv_apply_image).  The pieces (bf16 [n_a, 3 ca] and [n_b, 3 cb]) are cut by the
 * call itself into the tail of `partial`: lidal_conv_wgrad_slabs(.., LIDAL_F32_SPLIT) counts the room for them in slabs
 * (-1: the shape is not served -- ca, cb multiples of 8, split operands below 4 GiB). */
int64_t lidal_conv_wgrad_slabs(int64_t n_a, int64_t n_b, int k, int ca, int cb, int dtype);
int lidal_conv_wgrad(const void* a, const void* b, int64_t n_a, int64_t n_b, const int32_t* pairs,
                     const int64_t* koff, int a_col, float* gw, float* partial, int64_t n_slabs,
                     int k, int ca, int cb, int dtype, void* stream);

/* The weight gradient on rule lists re-ordered into ONE STREAM PER WORKGROUP (round 6; csrc/wgrad_streams.hip,
 * csrc/wgrad_dma.hip wgrad_stream_kernel).  lidal_conv_wgrad reads both rows of every rule from the fabric: the ~5 rules
 * that touch a row lie in different offsets, worked on far apart in time (96 -> 96 on 397 k rows: 851 MB per launch for
 * 152 MB of operands).  lidal_wgrad_streams_build re-orders the rules of a stride-1 map (pairs / koff of
 * lidal_kmap_build, k <= 32 offsets, n_rows rows on both sides) so that the rules of a row meet in one XCD's L2: rows are
 * cut into blocks of consecutive spatial keys -- key_tab == NULL: the row index (rows numbered in coordinate order:
 * every level lidal_downsample made), key_range = n_rows; otherwise key(row) = max over key_tab i32 [key_k, n_rows] in
 * [0, key_range): the strided map's inverse neighbour table (lidal_kmap_invert) names a row's parent on the next level,
 * for levels numbered otherwise (SPVCNN's level 0: by coordinate hash) -- block b belongs to the workgroups w with
 * w % 8 == b % 8 (one XCD under round-robin dispatch), which share the offsets in proportion to their rule counts and
 * walk the blocks in order.  Outputs: spairs i32 [spairs_rules >= lidal_wgrad_streams_rules(..), 2] (bit 31 of a
 * rule's first index: the accumulator set; out-of-range rules as padding) and sdesc i32
 * [lidal_wgrad_streams_desc_words(k, n_wg)] = {n_wg, k, stages, 0, soff[n_wg + 1], offsets of workgroup w [n_wg][2],
 * the reducer's table [k][8][3]}.  n_wg = lidal_wgrad_streams_workgroups() (512).  Nothing is read back to the host;
 * the result is a pure function of (pairs, koff, keys): integer arithmetic, stable sorts. */
int lidal_wgrad_streams_workgroups(void);
int64_t lidal_wgrad_streams_rules(int64_t n_rows, int k, int n_wg);
int64_t lidal_wgrad_streams_desc_words(int k, int n_wg);
int64_t lidal_wgrad_streams_workspace_bytes(int64_t n_rows, int k);
int lidal_wgrad_streams_build(const int32_t* pairs, const int64_t* koff, int k, int64_t n_rows, const int32_t* key_tab,
                              int key_k, int64_t key_range, int n_wg, int32_t* spairs, int64_t spairs_rules,
                              int32_t* sdesc, void* ws, int64_t ws_bytes, void* stream);
/* gw[k] = a[spairs[:, a_col]]^T b[spairs[:, 1 - a_col]] over those streams: the same rules as lidal_conv_wgrad in
 * another order -- equal to it within f32 rounding, bitwise reproducible (fixed slab order, no atomics).  bf16, ca and cb
 * multiples of 8 within ONE channel tile (<= 128); partial >= 2 n_wg slabs of [ca][cb] f32. */
int lidal_conv_wgrad_streams_serves(int64_t n_a, int64_t n_b, int k, int ca, int cb);     /* 1: the shape is served */
int lidal_conv_wgrad_streams(const void* a, const void* b, int64_t n_a, int64_t n_b, const int32_t* spairs,
                             const int32_t* sdesc, int n_wg, int a_col, float* gw, float* partial, int64_t n_slabs,
                             int k, int ca, int cb, int dtype, void* stream);

/* ---- batch normalisation over rows ------------------------------------------------------------ */
/* replaces the torch.nn.BatchNorm1d kernels behind spnn.BatchNorm (network/utils.py:115; 49 per
 * model) for x [n, c] row-major, dtype f32 or bf16 (statistics always f32).  Training forward:
 * biased batch variance for normalisation, running stats updated with `momentum` and the unbiased
 * variance (running_* may be NULL); save_mean / save_invstd f32 [c] feed the backward.
 * c must be a multiple of 4 (f32) / 8 (bf16). */
int64_t lidal_bn_workspace_bytes(int64_t n, int c);
/* `relu` != 0 fuses the ReLU that follows the normalisation in the model (forward: max(y, 0);
 * backward: dy is taken where y > 0, y recomputed from x). */
/* num_batches_tracked (nn.BatchNorm1d's i64 scalar buffer, may be NULL) is incremented by one. */
/* relu: bit 1 = ReLU on the normalised value, bit 2 (with a residual) = ReLU after the residual sum
 * (the end of a residual block, network/utils.py:171; the backward of that form takes dy already
 * masked by y > 0, e.g. from lidal_add_relu_bwd, and relu = 0).
 * residual (same dtype [n, c], may be NULL): y = act(bn(x)) + residual -- the point-branch sum of
 * network/spvcnn.py:104,111,118 (`z1.F = z1.F + point_transforms(z.F)`) inside the normalising pass;
 * its gradient is grad_y unchanged. */
int lidal_bn_train_fwd(const void* x, int dtype, int64_t n, int c, const float* gamma,
                       const float* beta, float eps, float momentum, float* running_mean,
                       float* running_var, int64_t* num_batches_tracked, int relu,
                       const void* residual, void* y, float* save_mean, float* save_invstd, void* ws,
                       int64_t ws_bytes, void* stream);
/* lidal_bn_train_fwd with the statistics pass replaced by the per-tile (count, mean, M2) triples
 * lidal_conv_apply_image wrote (tile_stats f32 [c][n_tiles][3]). */
int lidal_bn_train_fwd_tiles(const void* x, int dtype, int64_t n, int c, const float* gamma,
                             const float* beta, float eps, float momentum, float* running_mean,
                             float* running_var, int64_t* num_batches_tracked, int relu,
                             const void* residual, void* y, float* save_mean, float* save_invstd,
                             const float* tile_stats, int64_t n_tiles, void* stream);
int lidal_bn_eval_fwd(const void* x, int dtype, int64_t n, int c, const float* gamma,
                      const float* beta, const float* running_mean, const float* running_var,
                      float eps, int relu, void* y, void* stream);
/* dx may be NULL (only parameter gradients wanted).  dy_stride = elements between the rows of dy
 * (>= c, a multiple of the 16-byte vector): the gradient of a channel slice of a concatenation
 * (network/utils.py:cat in the up stages) is read in place, without a contiguous copy. */
int lidal_bn_bwd(const void* x, const void* dy, int64_t dy_stride, int dtype, int64_t n, int c, const float* gamma,
                 const float* beta, int relu, const float* save_mean, const float* save_invstd,
                 void* dx, float* grad_gamma, float* grad_beta, void* ws, int64_t ws_bytes,
                 void* stream);
/* Column sums of x [n, c] -> out f32 [c] (bias gradients of the 1x1 / Linear layers);
 * ws >= lidal_bn_workspace_bytes(n, c) + 12*c bytes. */
/* BatchNorm backward whose per-column sums came with dy: tile_sums f32 [c, n_tiles, 2] = (sum dy', sum dy' xhat)
 * per 128-row tile (lidal_conv_stats_tile_rows), left by lidal_conv_dgrad_bn_sums.  Merges the tiles in f64
 * (-> grad_beta, grad_gamma) and writes dx; no pass over (x, dy) for the sums. */
int lidal_bn_bwd_tiles(const void* x, const void* dy, int64_t dy_stride, int dtype, int64_t n, int c,
                       const float* gamma, const float* beta, int relu, const float* save_mean,
                       const float* save_invstd, void* dx, float* grad_gamma, float* grad_beta,
                       const float* tile_sums, int64_t n_tiles, void* stream);
/* The tail of a residual block backwards (network/utils.py:142-172: out = relu(bn2(x_a) + shortcut), the shortcut the
 * identity or bn_s(x_b)): gm = g where out > 0 (lidal_add_relu_bwd) and, in the same pass, the partial sums of the
 * BatchNorm backward of bn2 over (x_a, gm) -- and of the shortcut's BatchNorm over (x_b, gm) when x_b != NULL -- that
 * lidal_bn_bwd would take in its first pass over the same operands (bit for bit).  part_a / part_b: >=
 * lidal_bn_workspace_bytes(n, c) each (part_bytes), handed to lidal_bn_bwd_from_sums; relu = 0 there (the ReLU of the
 * tail follows the sum).  Rows are contiguous ([n, c], c whole 16-byte vectors). */
int lidal_add_relu_bwd_bn_sums(const void* out, const void* g, void* gm, int dtype, int64_t n, int c,
                               const void* x_a, const float* mean_a, const float* invstd_a, void* part_a,
                               const void* x_b, const float* mean_b, const float* invstd_b, void* part_b,
                               int64_t part_bytes, void* stream);
/* The same tail for the levels with many rows: gm = g where out > 0, and per part (a slab of rows; there are
 * lidal_bn_tail_parts(n, c, dtype) of them) and channel the f32 pairs (sum gm, sum gm * xhat) of the BatchNorm over x_a --
 * and over x_b, if given -- as [channel][part][2] (sums_a / sums_b: c * n_parts * 2 floats each): the tile sums
 * lidal_bn_bwd_tiles takes, with n_tiles = n_parts and relu = 0.  One element-wise pass instead of lidal_add_relu_bwd and
 * the first pass of one or two lidal_bn_bwd. */
int64_t lidal_bn_tail_parts(int64_t n, int c, int dtype);
int lidal_add_relu_bwd_bn_tile_sums(const void* out, const void* g, void* gm, int dtype, int64_t n, int c,
                                    const void* x_a, const float* mean_a, const float* invstd_a, float* sums_a,
                                    const void* x_b, const float* mean_b, const float* invstd_b, float* sums_b,
                                    int64_t n_parts, void* stream);
/* lidal_bn_bwd without its first pass: the partial sums are in `part` (lidal_add_relu_bwd_bn_sums). */
int lidal_bn_bwd_from_sums(const void* x, const void* dy, int64_t dy_stride, int dtype, int64_t n, int c,
                           const float* gamma, const float* beta, int relu, const float* save_mean,
                           const float* save_invstd, void* dx, float* grad_gamma, float* grad_beta,
                           const void* part, int64_t part_bytes, void* stream);
/* The merge steps of a BatchNorm layer (tile statistics -> mean / invstd; backward partial sums -> parameter
 * gradients) run INSIDE the launch that consumes them (the first workgroups merge and publish, all workgroups fetch;
 * csrc/bn.hip) -- same arithmetic, same results bit for bit as the separate merge launches, which on = 0 brings back
 * (also: environment LIDAL_BN_FUSED=0).
 *   Memory: the publication buffers are the library's own (the one allocation named under "Conventions"): two per
 *   STREAM, so a buffer is re-used only by a later launch of the same stream, i.e. after its last reader has finished
 *   -- any number of host threads and up to 32 streams per device may run BatchNorm launches at the same time; a 33rd
 *   stream silently takes the separate merge launches (same results).
 *   Forward progress: the waiting workgroups rely on the merging ones -- the LOWEST workgroup ids of the launch --
 *   having been dispatched before them (in-order workgroup dispatch, the assumption sort.hip's decoupled look-back
 *   makes too).  A workgroup that waits longer than ~30 s gives up: it writes NaN to its channel AND raises a
 *   per-device error word, and every later BatchNorm entry point and lidal_plan_run on that device fails with a message
 *   naming the launch (lidal_bn_check_device) until lidal_bn_set_fused() is called again: never a silent NaN.
 * lidal_bn_set_fused also acknowledges such an error. */
int lidal_bn_set_fused(int on);
/* bf16 lidal_bn_bwd takes its two sums per channel as f32 sums over slabs of rows (512 slabs on the large levels, merged in
 * f64 like the convolutions' tile sums: an element-wise-shaped first pass at ~5 TB/s) -- 1, the default -- or as the f64
 * partial sums the f32 mode uses (0; LIDAL_BN_SLAB_SUMS=0 in the environment).  Returns the previous setting. */
int lidal_bn_set_slab_sums(int on);
/* 0, or 1 with lidal_last_error() set if a fused BatchNorm launch on the current device timed out (above). */
int lidal_bn_check_device(void);
/* eval-mode BatchNorm as a per-channel affine map (scale = gamma / sqrt(var + eps),
 * shift = beta - mean * scale), the operands of lidal_conv_apply's epilogue. */
int lidal_bn_fold(const float* gamma, const float* beta, const float* running_mean,
                  const float* running_var, float eps, int c, float* scale, float* shift,
                  void* stream);
int lidal_colsum(const void* x, int dtype, int64_t n, int c, float* out, void* ws,
                 int64_t ws_bytes, void* stream);

/* ---- small fused row-wise ops of the training step --------------------------------------------- */
/* relu(a + b) of the residual blocks (network/utils.py:171), forward and backward
 * (gin = g where y > 0; both summands receive it).  numel a multiple of 4 (f32) / 8 (bf16). */
int lidal_add_relu_fwd(const void* a, const void* b, void* y, int64_t numel, int dtype,
                       void* stream);
int lidal_add_relu_bwd(const void* y, const void* g, void* gin, int64_t numel, int dtype,
                       void* stream);
/* replaces torch.nn.functional.cross_entropy(logits, labels, ignore_index, reduction='mean')
 * (train.py:136): out2 f32 [2] = {mean loss over non-ignored rows, number of such rows};
 * backward: dlogits = (softmax - onehot) * grad_scale[0] / out2[1], zero on ignored rows. */
int64_t lidal_ce_workspace_bytes(int64_t n);
int lidal_ce_fwd(const void* logits, int dtype, const int64_t* labels, int64_t n, int c,
                 int64_t ignore_index, float* out2, void* ws, int64_t ws_bytes, void* stream);
int lidal_ce_bwd(const void* logits, int dtype, const int64_t* labels, int64_t n, int c,
                 int64_t ignore_index, const float* fwd_out2, const float* grad_scale,
                 void* dlogits, void* stream);

/* ---- objectives beside the plain cross-entropy (csrc/loss.hip; not plan operations: the loss is the caller's) ---- */
/* The same cross-entropy with class weights, torch.nn.functional.cross_entropy(weight=w, reduction='mean'):
 * weight f32 [c]; out2 f32 [2] = {sum_i w[y_i] * -log p[i, y_i] / sum_i w[y_i], sum_i w[y_i]} over the non-ignored rows
 * (no such row, or only zero weights: 0 / 0 = nan, as torch); backward:
 * dlogits_i = w[y_i] * (softmax_i - onehot) * grad_scale[0] / out2[1], zero on ignored rows.  c in 1..32. */
int64_t lidal_ce_weighted_workspace_bytes(int64_t n);
int lidal_ce_weighted_fwd(const void* logits, int dtype, const int64_t* labels, int64_t n, int c, int64_t ignore_index,
                          const float* weight, float* out2, void* ws, int64_t ws_bytes, void* stream);
int lidal_ce_weighted_bwd(const void* logits, int dtype, const int64_t* labels, int64_t n, int c, int64_t ignore_index,
                          const float* weight, const float* fwd_out2, const float* grad_scale, void* dlogits,
                          void* stream);
/* Lovasz-softmax (Berman et al., CVPR 2018, lovasz_softmax_flat) over the rows whose label is not ignore_index.
 * x [n, c]: logits f32 / bf16 (is_probs = 0: the forward pass takes p = softmax in f64 and rounds
 * e once to f32, the backward pass p = softmax in f32) or probabilities f32 (is_probs = 1).  Per class k:
 * fg = (label == k), e = |fg - p_k| in f32, rows ordered by e descending, ties by ascending row (ONE stable sort for
 * all classes, key = k << 32 | ~bits(e)); gts = sum fg; at rank r: inter = gts - cumsum(fg), union = gts + cumsum(1 - fg)
 * (integers), jac = 1 - inter / union in f32, g[r] = jac[r] - jac[r - 1], g[0] = jac[0]; L_k = sum_r e[r] g[r] in f64.
 * Outputs:
 *   out   f64 [4 + 2 c] = {loss, number of present classes (gts > 0), status, valid rows, L_k [c], gts_k [c]};
 *         loss = mean of L_k over the present classes (mode_all = 0) or over all c classes (mode_all = 1), 0 without a
 *         valid row or a class that counts; status != 0: some label was outside [0, c) and not ignore_index (such rows
 *         are left out like ignored ones) -- it travels with the loss, for the caller to read where it reads the loss;
 *   grad  f32 [n, c] = dL_k / dp[i, k]: -g[rank] where fg = 1, +g[rank] where fg = 0, 0 where e == 0, 0 on ignored rows;
 *   ranks i32 [n, c] or NULL: the rank of row i in class k's order, -1 on ignored rows.
 * Backward: with s_k = grad_scale[0] * [class k counts] / (number of classes that count) + grad_class[k] (either
 * pointer may be NULL: the gradient of the loss, and of the per-class losses L_k), a_k = grad[i, k] * s_k:
 *   is_probs = 1: dx[i, k] = a_k (f32);     is_probs = 0: dx[i, k] = p_k * (a_k - sum_j a_j p_j), j ascending, in x's
 *   dtype; zero on ignored rows.
 * Limits: c in 1..32, n * c < 2^30 (refused before any launch; the workspace size of a refused shape is 0).  No float
 * atomics: two runs give the same bits. */
int64_t lidal_lovasz_workspace_bytes(int64_t n, int c);
int lidal_lovasz_fwd(const void* x, int dtype, int is_probs, const int64_t* labels, int64_t n, int c, int64_t ignore_index,
                     int mode_all, double* out, float* grad, int32_t* ranks, void* ws, int64_t ws_bytes, void* stream);
int lidal_lovasz_bwd(const void* x, int dtype, int is_probs, const int64_t* labels, int64_t n, int c, int64_t ignore_index,
                     int mode_all, const double* out, const float* grad, const float* grad_scale, const float* grad_class,
                     void* dx, void* stream);

/* ---- probability inference post-processing ------------------------------------------------- */
/* replaces score/prob_inference.py:100-113: logits f32 [nv, c] of `reps` collated views,
 * inverse i64 [reps*p] (voxel row of every point in every view) -> prob f32 [p,c] = mean over
 * views of softmax(logits[inverse]), pred i64 [p] = argmax. */
int lidal_view_mean_softmax(const float* logits, const int64_t* inverse, int reps, int64_t p,
                            int c, float* prob, int64_t* pred, void* stream);
/* The call above plus how much the views DISAGREED about every point, in one launch, no workspace:
 * LiDAL's formula (score/sv_level/LiDAL.py:59-81) with the point's view mean m = prob[i] in the query frame's place and
 * its `reps` soft-max rows p_v in the matched neighbours' place.  prob, pred: the same bytes as the call above.
 *   viewd f64 [p] = (1 / reps) sum_v sum_k kl_div(m_k + 1e-5f, p_vk + 1e-5f)   (f32 terms, numpy's f32 class sum, f64 over views)
 *   viewe f32 [p] = scipy.stats.entropy(m)
 *   agree i32 [p] = the views whose logits row has its first maximum at pred[i], 0..reps. */
int lidal_view_scores(const float* logits, const int64_t* inverse, int reps, int64_t p, int c, float* prob,
                      int64_t* pred, double* viewd, float* viewe, int32_t* agree, void* stream);

/* The same launch shape for MC-dropout: the `reps` rows of a point are the passes of ONE view under different dropout
 * masks.  prob, pred: the same bytes as lidal_view_mean_softmax; p_v the same soft-max rows.
 * With H(q) = sum_k (q_k > 0 ? -q_k log q_k : 0), an f64 expression of the f32 q_k summed in f64 in class order (no
 * epsilon, no renormalisation), S = sum_v H(p_v) in view order (the rounding error of every add kept and added at the
 * end) and m = the f32 nearest to the mean of the rows (their f64 sum in view order over reps; within one unit in the
 * last place of prob, which stays the f32 chain of lidal_view_mean_softmax) -- so that agreeing passes score exactly 0:
 *   bald f64 [p] = H(m) - S / reps      the mutual information between the prediction and the mask (BALD)
 *   ment f32 [p] = (float)(S / reps)    the mean entropy of the passes
 *   agree i32 [p] = as in lidal_view_scores. */
int lidal_mc_scores(const float* logits, const int64_t* inverse, int reps, int64_t p, int c, float* prob,
                    int64_t* pred, double* bald, float* ment, int32_t* agree, void* stream);

/* ---- counter-based dropout ------------------------------------------------------------------ */
/* In place on a contiguous tensor of n_elems F32 or BF16 elements: x[i] = rn_dtype((float)x[i] * m), m = scale where the
 * element is kept, 0.0f where it is dropped (a dropped NaN stays NaN).  The mask is a pure function of (seed, call,
 * element index): with e = first + i, Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9,
 * 0xBB67AE85) under key (seed lo, seed hi) and counter (g lo, g hi, call lo, call hi), g = e >> 2, gives four words;
 * element e is kept iff word e & 3 is below thr.  The host forms thr = min(floor((1 - p) * 2^32), 0xffffffff) and
 * scale = (float)(1 / (1 - p)).  Nothing is stored for the backward pass: it is the same call on the gradient.
 * One launch; refused before any launch when first % 8 != 0, thr is outside [0, 2^32), x is not 16-byte aligned,
 * n_elems < 0 or the dtype is neither. */
int lidal_dropout_apply(void* x, int64_t n_elems, int dtype, int64_t first, int64_t seed, int64_t call, int64_t thr,
                        double scale, void* stream);

/* replaces evaluate.py:100-109 + utils/iou_sk.py:14-19 ("next" row 8f-4): conf i32 [c*c] +=
 * bincount(argmax(logits[inverse]) * c + labels) over labelled points (label < 100); conf is
 * accumulated across calls (the caller zeroes it once and all-reduces it across ranks). */
int lidal_confusion_accumulate(const float* logits, const int64_t* inverse, const int64_t* labels,
                               int64_t p, int c, int32_t* conf, void* stream);

/* ---- inter-frame divergence / entropy scoring ---------------------------------------------- */
/* replaces dataset/prepare_kdtree_sk.py:76-80 ("next" row 8f-2): sensor-frame points f32 [p,3] ->
 * world-frame f64 [p,3] = (hcoords * pose^T)[:, :3] with pose f64 [16] row-major 4x4 (device),
 * same operation order as the reference's broadcast-multiply + sum. */
int lidal_register_points(const float* points, int64_t p, const double* pose_dev, double* world,
                          void* stream);
/* Uniform-grid nearest-neighbour structure over one frame's world-frame points (replaces the
 * pickled sklearn KDTree of dataset/prepare_kdtree_sk.py:83 as used by
 * score/sv_level/LiDAL.py:52-66).  cell: any size > 0 (kept in the grid; a query visits the cells that meet the cube of
 * its match radius: 27 for cell = radius, at most 8 for cell = 2 x radius -- the answers are the same).
 *   pts f64 [p,3];  grid bytes from lidal_nn_grid_bytes(p).
 * Key range: a cell index is packed into 21 bits per axis, so a coordinate v is IN RANGE iff floor(v / cell) lies in
 * [-(2^20 - 1), 2^20 - 1] (209 km either side of the origin at cell = 0.2 m).  A point with a coordinate that is NaN,
 * +-Inf or out of range is filed in a parking cell that no in-range query probes; a query with such a coordinate, or
 * whose cube [q - r, q + r]^3 leaves the range, matches nothing.  So such a point matches nothing and is matched by
 * nothing: map_count = 0, interd = 0, intere = the entropy of its own probability row.  Decided per point on the device
 * (no host check, no synchronisation); every other point of the frame is scored as if it were absent. */
int64_t lidal_nn_grid_bytes(int64_t p);
int64_t lidal_nn_grid_workspace_bytes(int64_t p);
int lidal_nn_grid_build(const double* pts, int64_t p, double cell, void* grid, int64_t grid_bytes,
                        void* ws, int64_t ws_bytes, void* stream);
/* replaces score/sv_level/LiDAL.py:59-81 for one query frame against `n_nei` neighbour frames
 * (host arrays of device pointers, in the reference's neighbour order):
 *   interd f64 [p] (mean KL over matched neighbours), intere f32 [p] (entropy of the mean
 *   probability), map_count i32 [p] (matches). */
int64_t lidal_interframe_workspace_bytes(int64_t p, int n_nei);
int lidal_interframe_score(const double* q_pts, const float* q_prob, int64_t p, int c,
                           const void* const* nei_grids_host, const double* const* nei_pts_host,
                           const float* const* nei_prob_host, const int64_t* nei_p_host,
                           int n_nei, double dis_thresh, double* interd, float* intere,
                           int32_t* map_count, void* ws, int64_t ws_bytes, void* stream);
/* lidal_interframe_score with the query points taken in CELL order (round 6): q_grid = the grid lidal_nn_grid_build made of
 * q_pts themselves (every frame of a sequence has one: it is the neighbour of others), or NULL = the call above.  The
 * queries of a wave then share their cells' cache lines.  Same outputs bit for bit, in the points' own order. */
int lidal_interframe_score_ordered(const double* q_pts, const float* q_prob, int64_t p, int c,
                                   const void* const* nei_grids_host, const double* const* nei_pts_host,
                                   const float* const* nei_prob_host, const int64_t* nei_p_host,
                                   int n_nei, double dis_thresh, double* interd, float* intere,
                                   int32_t* map_count, void* ws, int64_t ws_bytes, const void* q_grid,
                                   void* stream);
/* ---- labels and predictions carried across registered frames (csrc/transfer.hip) ---------- */
/* Stage 1 of lidal_interframe_score as an entry point of its own (the same kernel): match i32 [n_nei][p], caller's
 * buffer of n_nei * p entries; match[n][i] = the nearest point of neighbour n to query i with sqrt(d2) <= dis_thresh
 * (d2 = ((ex*ex + ey*ey) + ez*ez) in f64, ties to the lowest index), or -1.  A neighbour with p_n <= 0 gives a row of
 * -1; a query that is NaN, infinite or out of range matches nothing (lidal_nn_grid_build).  The host arrays are those
 * of lidal_interframe_score.  n_nei in 0..32; p == 0 or n_nei == 0 writes nothing and returns 0. */
int lidal_interframe_match(const double* q_pts, int64_t p, const void* const* nei_grids_host,
                           const double* const* nei_pts_host, const int64_t* nei_p_host, int n_nei,
                           double dis_thresh, int32_t* match, void* stream);
/* Stage 2 for labels and predictions: one thread per query point walks match[0..n_nei)[i] in order.  An entry outside
 * [0, nei_p_host[n]) is no match.  Two output groups; a group is off when ALL of its pointers are NULL, at least one
 * must be on, and a group of which only some pointers are given is refused.
 *   Annotation group: nei_labels_host (host array of device i64*, one per neighbour; a NULL entry votes nothing),
 *   q_labels i64 [p] or NULL, gate i64 [p] or NULL -> out i64 [p], votes i32 [p], agree i32 [p], stats i64 [c + 7].
 *     For neighbour n with j = match[n][i] matched and l = nei_labels[n][j]: l == ignore_index is skipped, l outside
 *     [0, c) is skipped and counted invalid, otherwise hist[l]++, nv++.  winner = the FIRST maximum of hist,
 *     ag = hist[winner]; votes[i] = nv, agree[i] = ag.  out[i] by the first rule that applies:
 *       1. q_labels[i], when given and != ignore_index                                           (own; and when rules
 *          2-4 would have let the vote through: confirmed if winner == q_labels[i], else contradicted)
 *       2. ignore_index when nv == 0                                                             (none)
 *       3. ignore_index when nv < min_votes or (double)ag < min_agree * (double)nv               (weak)
 *       4. ignore_index when gate is given and gate[i] != winner                                 (gated)
 *       5. winner                                                                                (stats[winner])
 *     stats = the c class counts, then own, none, weak, gated, confirmed, contradicted, invalid; zeroed by this call,
 *     integer atomics only, never read back here.
 *   Prediction group: q_prob f32 [p,c], nei_prob_host (as lidal_interframe_score) -> fused_prob f32 [p,c],
 *   fused_pred i64 [p], fused_conf f32 [p], count i32 [p].
 *     sum_k = q_prob[i][k]; per matched neighbour in order sum_k = fl32(sum_k + nei_prob[n][j][k]);
 *     fused_prob[i][k] = (float)((double)sum_k / (double)(count + 1)) -- the mean row whose entropy is
 *     lidal_interframe_score's intere; fused_pred = its first maximum, fused_conf that entry.
 * c in 1..32, n_nei in 0..32, min_votes >= 1, 0 < min_agree <= 1 (whichever group is on); p == 0 returns 0.  No workspace,
 * no float atomics: every output is a function of the inputs alone. */
int lidal_interframe_transfer(const int32_t* match, int64_t p, int c, int n_nei, const int64_t* nei_p_host,
                              const int64_t* const* nei_labels_host, const int64_t* q_labels, const int64_t* gate,
                              int64_t ignore_index, int min_votes, double min_agree, int64_t* out, int32_t* votes,
                              int32_t* agree, int64_t* stats, const float* q_prob,
                              const float* const* nei_prob_host, float* fused_prob, int64_t* fused_pred,
                              float* fused_conf, int32_t* count, void* stream);
/* ---- scan-to-scan registration by point-to-plane ICP (csrc/icp.hip) ------------------------- */
/* Normals of a raw scan xyz f32 [p,3]: normals f64 [p,3].  Per point: its k nearest OTHER points as lidal_knn orders
 * them (f64 distance, then index), their population covariance in f64 (mean summed in that order times 1 / k, then the
 * six second moments about it times 1 / k), cyclic Jacobi with eigenvectors (csrc/sym3.h).  The normal is the
 * eigenvector (column) of the smallest eigenvalue exactly as the Jacobi leaves it, the lowest column on a tie, negated
 * when ((nx*x + ny*y) + nz*z) > 0 so that it faces the sensor origin.  (0,0,0) is written when the unclipped surface
 * variation lambda_min / ((l1 + l2) + l3) exceeds max_variation, when the eigenvalue sum is 0, or when anything is not
 * finite.  1 <= k <= 64; p < k + 1 is refused (status 2), as by lidal_knn, whose precondition (finite coordinates) and
 * `cell` are this call's too.  Workspace: lidal_point_normals_workspace_bytes(p, k) = the k-NN table + lidal_knn's own. */
int64_t lidal_point_normals_workspace_bytes(int64_t p, int k);
int lidal_point_normals(const float* xyz, int64_t p, int k, double cell, double max_variation, double* normals,
                        void* ws, int64_t ws_bytes, void* stream);
/* n_iters iterations of point-to-plane ICP of a source scan onto a target, two launches each, nothing read back.
 *   src f32 [p_src,3] in the sensor frame; thread t takes source point t * stride (stride >= 1);
 *   tgt_grid = lidal_nn_grid_build of tgt_pts f64 [p_tgt,3] (any cell: the answers do not depend on it), tgt_normals
 *   f64 [p_tgt,3] (lidal_point_normals; a (0,0,0) row takes no part);
 *   pose f64 [16] row-major 4x4 on the device, IN PLACE: the initial estimate in, the result out;
 *   max_dist_host f64 [n_iters] (host): the match radius of every iteration; consecutive equal values are one LEVEL;
 *   trace f64 [n_iters][LIDAL_ICP_TRACE] on the device, one row per iteration (below).
 * ACCUMULATE, per source point: s = pose * src_i in f64, ((h0*P[j][0] + h1*P[j][1]) + h2*P[j][2]) + P[j][3] as
 * lidal_register_points; j = the nearest target point with sqrt(d2) <= max_dist (lidal_interframe_match's rule, ties to
 * the lowest index).  No match, a (0,0,0) normal or a non-finite s: the point is skipped.  Else with n the normal and
 * t = tgt_pts[j]:  r = ((sx-tx)*nx + (sy-ty)*ny) + (sz-tz)*nz;  a = s x n = (sy*nz - sz*ny, sz*nx - sx*nz, sx*ny - sy*nx);
 * J = (a, n).  The point adds 29 terms: J_u*J_v for u <= v (row-major upper triangle, 21), -(J_u*r) (6), r*r, 1.  Every
 * product is rounded on its own.  Sums in f64: per thread over its points (t, t + T, t + 2 T, ... with T the threads of
 * the launch), a fixed tree over the 256 threads of a workgroup, one partial row per workgroup; the number of
 * workgroups is min(ceil(ceil(p_src / stride) / 256), 1024), a function of p_src and stride alone.
 * FINISH, one workgroup: the partial rows summed in index order; A xi = b with A the symmetric 6x6 of the 21 sums and b
 * the 6, by Cholesky: for j = 0..5: d = A[j][j] - L[j][0]^2 - ... - L[j][j-1]^2 (left to right), L[j][j] = sqrt(d),
 * L[i][j] = (A[i][j] - L[i][0]*L[j][0] - ...) / L[j][j]; y[i] = (b[i] - L[i][0]*y[0] - ...) / L[i][i]; xi[i] = (y[i] -
 * L[i+1][i]*xi[i+1] - ... - L[5][i]*xi[5]) / L[i][i] for i = 5..0.  xi = (omega, v).  q = (1, omega/2) divided by
 * sqrt(((1 + qx^2) + qy^2) + qz^2); R = the quaternion's rotation matrix (R00 = 1 - 2*(yy + zz), R01 = 2*(xy - wz),
 * R02 = 2*(xz + wy), R10 = 2*(xy + wz), R11 = 1 - 2*(xx + zz), R12 = 2*(yz - wx), R20 = 2*(xz - wy), R21 = 2*(yz + wx),
 * R22 = 1 - 2*(xx + yy)); pose <- [R | v; 0 0 0 1] * pose, rows 0..2: ((R[i][0]*P[0][j] + R[i][1]*P[1][j]) +
 * R[i][2]*P[2][j]) + v[i]*P[3][j].  Only + - * / and sqrt.
 * STOPPING, on the device: when max|omega| < eps_rot and max|v| < eps_trans the iteration is CONVERGED and the remaining
 * iterations of its level return at once (SKIPPED).  Fewer than min_pairs pairs (FEW_PAIRS; p_src == 0 is that), or a
 * Cholesky pivot d that is <= 1e-12 * max_k A[k][k] or not finite (DEGENERATE): the pose stays as the iteration found
 * it and every later iteration is a no-op (AFTER_FAILURE).
 * Refused before any launch (status 2): stride < 1, n_iters outside 1..256, a max_dist that is not finite and positive,
 * min_pairs < 6, NULL pointers (src may be NULL when p_src == 0; tgt_pts and tgt_normals when p_tgt == 0).
 * Workspace: lidal_icp_workspace_bytes(p_src, stride). */
enum {
  LIDAL_ICP_TRACE = 64,            /* doubles per trace row: */
  LIDAL_ICP_TRACE_SUMS = 0,        /*   the 29 sums (zeros in a SKIPPED / AFTER_FAILURE row); [28] is the pair count */
  LIDAL_ICP_TRACE_XI = 29,         /*   xi (zeros unless the pose was updated) */
  LIDAL_ICP_TRACE_STATUS = 35,     /*   one of LIDAL_ICP_* below */
  LIDAL_ICP_TRACE_MAX_DIST = 36,   /*   the iteration's match radius */
  LIDAL_ICP_TRACE_POSE = 37        /*   the 16 entries of the pose the iteration started from; [53..63] are 0 */
};
enum {
  LIDAL_ICP_OK = 0,                /* the pose was updated */
  LIDAL_ICP_CONVERGED = 1,         /* updated, and the update was below eps_rot and eps_trans */
  LIDAL_ICP_SKIPPED = 2,           /* an earlier iteration of the level converged */
  LIDAL_ICP_FEW_PAIRS = 3,
  LIDAL_ICP_DEGENERATE = 4,
  LIDAL_ICP_AFTER_FAILURE = 5
};
int64_t lidal_icp_workspace_bytes(int64_t p_src, int64_t stride);
int lidal_icp_run(const float* src, int64_t p_src, int64_t stride, const void* tgt_grid, const double* tgt_pts,
                  const double* tgt_normals, int64_t p_tgt, double* pose, const double* max_dist_host, int n_iters,
                  int min_pairs, double eps_rot, double eps_trans, double* trace, void* ws, int64_t ws_bytes,
                  void* stream);
/* replaces score/sv_level/LiDAL.py:91-98: per-supervoxel means over point lists given as CSR
 * (sv_ptr i64 [s+1], sv_idx i64 [sv_ptr[s]]).  sv_interd f32 [s], sv_intere f32 [s],
 * sv_center f32 [s,3]. */
int lidal_supervoxel_reduce(const double* interd, const float* intere, const double* pts,
                            const int64_t* sv_ptr, const int64_t* sv_idx, int s, float* sv_interd,
                            float* sv_intere, float* sv_center, void* stream);

/* ---- fixed-radius neighbour lists of the supervoxel centres (csrc/neighbours.hip) ---------- */
/* The distance work of score/sv_level/LiDAL.py:225-325 (the greedy selection tests a candidate against every added
 * supervoxel): the CSR table of all pairs within `radius`, centers f32 [n,3].  Row i = every j != i, ascending, with
 *     sqrt(((dx*dx + dy*dy) + dz*dz)) < radius        in f32, every operation rounded, the root correctly rounded,
 * the reference's `np.sqrt(np.square(c_i - c_j).sum()) < radius` bit for bit; symmetric; a function of the centres alone.
 * Two calls make one table: lidal_radius_pairs_count writes row_ptr i64 [n + 1] (device), the caller reads row_ptr[n],
 * allocates col i32 [row_ptr[n]] and calls lidal_radius_pairs_fill with the same centres, radius and row_ptr (the fill
 * does not depend on what the workspace held in between).  A centre with a NaN or infinite coordinate has an empty row
 * and is in no row.  A finite coordinate whose cell index (cell = the smallest power of two >= radius) does not fit 21
 * bits raises *status_dev (i32 [1], written by every count call; the table is then not valid).  n <= 2^31 - 1; n = 0, 1:
 * empty tables; radius finite, >= 2^-60.  Workspace: lidal_radius_pairs_workspace_bytes(n), for both calls. */
enum {
  LIDAL_PAIRS_CELL_RANGE = 1   /* a finite centre outside the 21 bits per axis of the cell key */
};
int64_t lidal_radius_pairs_workspace_bytes(int64_t n);
int lidal_radius_pairs_count(const float* centers, int64_t n, float radius, int64_t* row_ptr, int32_t* status_dev,
                             void* ws, int64_t ws_bytes, void* stream);
int lidal_radius_pairs_fill(const float* centers, int64_t n, float radius, const int64_t* row_ptr, int32_t* col,
                            void* ws, int64_t ws_bytes, void* stream);

/* ---- Euclidean clustering: instance ids of a labelled or predicted batch (csrc/cluster.hip) ---- */
/* The connected components of the fixed-radius graph over the points of one class of one scan.  xyz f32 [p,3]: n_scans
 * (1..32) scans laid end to end, point_ptr i64 [n_scans + 1] on the HOST (ascending from 0 to p); labels i64 [p] or
 * NULL (every point has class 0); tol f32 [64] on the HOST: class c is clustered iff tol[c] > 0, and such a tolerance
 * lies in [2^-10, 2^10] m.  A point is live iff its coordinates are finite, 0 <= label < 64 and tol[label] > 0.  Two
 * live points of one scan and one class c are joined iff
 *     sqrt(((dx*dx + dy*dy) + dz*dz)) < tol[c]        in f32, every operation rounded, the root correctly rounded;
 * a component is kept iff min_points <= size <= max_points (1 <= min_points <= max_points).  Outputs, all on the device
 * and all a function of the input alone:
 *   inst i32 [p]             the instance id of a point, -1 when it is not live or its component is not kept; the K kept
 *                            components are numbered in ascending order of their smallest row
 *   cls i32 [K], bbox f32 [K,6]      class; min x, y, z, max x, y, z over the members          (allocate for K = p)
 *   member_ptr i64 [K + 1], members i32 [p]    instance k owns members[member_ptr[k] .. member_ptr[k + 1]), ascending
 *                            rows; the rows past member_ptr[K] are scratch
 *   status i64 [2 n_scans + 3]       word 0: 0 or a LIDAL_CLUSTERS_ word; then inst_ptr [n_scans + 1]: scan s owns the
 *                            ids inst_ptr[s] .. inst_ptr[s + 1], K = inst_ptr[n_scans]; then member_start [n_scans + 1] =
 *                            member_ptr[inst_ptr[s]], where the members of the scan's instances begin
 * A live point whose cell index (cell = the smallest power of two >= the largest tolerance) does not fit 21 bits raises
 * CELL_RANGE and is treated as not live; WALK says a union-find walk ran out of its step bound (a defect, never an
 * input).  p < 2^30.  With p = 0 or no positive tolerance there is no instance: the call returns 0, launches nothing and
 * writes nothing (every inst is then -1 by definition).  Refusals come before the first launch. */
enum {
  LIDAL_CLUSTERS_CELL_RANGE = 1,  /* a live point outside the 21 bits per axis of the cell key */
  LIDAL_CLUSTERS_WALK = 2         /* a walk or a retry loop of the union-find ran out of its bound */
};
int64_t lidal_euclidean_clusters_workspace_bytes(int64_t p, int n_scans);
int lidal_euclidean_clusters(const float* xyz, const int64_t* labels, int64_t p, const int64_t* point_ptr_host,
                             int n_scans, const float* tol_host, int64_t min_points, int64_t max_points, int32_t* inst,
                             int32_t* cls, int64_t* member_ptr, int32_t* members, float* bbox, int64_t* status, void* ws,
                             int64_t ws_bytes, void* stream);

/* ---- panoptic quality: predicted instances scored against annotated ones (csrc/panoptic.hip) ---- */
/* The per-class sums behind PQ = SQ x RQ, added into accumulators that live on the device across calls.  n_scans
 * (1..32) scans laid end to end, point_ptr i64 [n_scans + 1] on the HOST (ascending from 0 to p < 2^30); per row
 * pred_sem, gt_sem i64 [p] and pred_inst, gt_inst i32 [p] on the device; c in 1..64 classes; bit k of `things` set iff
 * class k has instances (no bit at or above c); min_points >= 1.
 *   A row is VOID iff gt_sem is outside [0, c); void rows take part in nothing.  A non-void row has a predicted segment
 *   iff pred_sem is in [0, c).  A segment is (scan, class, id): id = 0 for a stuff class whatever the instance column
 *   holds, id = inst + 1 for a thing class (inst = -1 is the class's one unassigned segment of the scan).  Equal ids in
 *   different scans are different segments.  An instance value of a thing row lies in [-1, 2^30 - 2]: a gt_inst outside
 *   makes the row void, a pred_inst outside leaves it without a predicted segment, either raises LIDAL_PANOPTIC_BAD_ID.
 *   area = the non-void rows of a segment; inter = the rows in both a gt and a predicted segment of one class;
 *   union = area_gt + area_pred - inter.  The pair MATCHES iff 2 * inter > union in integers -- which is
 *   inter / union > 0.5 in f64 for every union below 2^30: 2 * inter > union gives a quotient of at least
 *   0.5 + 1 / (2 union) > 0.5 + 2^-31, far above one rounding; 2 * inter <= union gives at most 0.5 exactly.  A segment
 *   has at most one match: a match holds more than half of the segment's rows, the partners of one segment are disjoint
 *   subsets of it, and two disjoint subsets cannot each hold more than half.
 * Per call and class k:  tp[k] += matches;  fn[k] += gt segments with area >= min_points and no match;
 * fp[k] += predicted segments with area >= min_points and no match;  iou[k] = iou[k] + part[k], part[k] = +0.0 plus
 * (double)inter / (double)union (the correctly rounded IEEE division) of the class's matches, added one by one in
 * ascending (scan, gt id).  No float atomics: the result is a function of the input alone, and a permutation of the
 * rows inside a scan gives the same 64 bits.
 *   tp, fp, fn i64 [c], iou f64 [c], status i64 [1] (word 0: 0 or a LIDAL_PANOPTIC_ word; it only grows): on the
 *   device, zeroed once by the caller, updated in place by every call.
 * p = 0 returns 0 and launches nothing.  Refusals (c, n_scans, min_points, point_ptr, things, the workspace) come before
 * the first launch.  Does not synchronise the stream.  Workspace: lidal_panoptic_accumulate_workspace_bytes(p, n_scans). */
enum {
  LIDAL_PANOPTIC_BAD_ID = 1  /* an instance value of a thing row outside [-1, 2^30 - 2] */
};
int64_t lidal_panoptic_accumulate_workspace_bytes(int64_t p, int n_scans);
int lidal_panoptic_accumulate(const int64_t* pred_sem, const int32_t* pred_inst, const int64_t* gt_sem,
                              const int32_t* gt_inst, int64_t p, const int64_t* point_ptr_host, int n_scans, int c,
                              uint64_t things, int64_t min_points, int64_t* tp, int64_t* fp, int64_t* fn, double* iou,
                              int64_t* status, void* ws, int64_t ws_bytes, void* stream);

/* ---- ReDAL region selection (score/sv_level/ReDAL.py, dataset/ReDAL/gen_surface_variation_sk.py; csrc/redal.hip) ---- */
/* k nearest OTHER points of every point of a raw scan xyz f32 [p,3]: knn i32 [p,k], sorted by (f64 distance, index).
 * 1 <= k <= 64; p < k + 1 is refused (status 2, lidal_last_error).  `cell`: the search grid's cell in metres (the
 * result does not depend on it).  Precondition, not checked here: every coordinate is finite (lidal_amd.score.redal
 * checks it; a NaN query never fills its list).  Workspace: lidal_knn_workspace_bytes(p). */
int64_t lidal_knn_workspace_bytes(int64_t p);
int lidal_knn(const float* xyz, int64_t p, int k, double cell, int32_t* knn, void* ws, int64_t ws_bytes, void* stream);
/* surface variation of every point: lambda_min / (lambda_1 + lambda_2 + lambda_3) of the population covariance of its
 * k nearest other points (f64, Jacobi eigenvalues), clipped at `threshold`: sigma f32 [p].  Same workspace. */
int lidal_surface_variation(const float* xyz, int64_t p, int k, double cell, float threshold, float* sigma, void* ws,
                            int64_t ws_bytes, void* stream);
/* ReDAL.py:59-74 for one frame: point_score = alpha * mean_c(-prob * log2(prob + 1e-12)) + gamma * curvature, then per
 * supervoxel s of the CSR (sv_ptr i64 [s+1], sv_idx i64): sv_scores f32 [s] (mean point_score), sv_feats f32 [s,d]
 * (mean feature row), sv_pnums i64 [s].  prob f32 [p,c] (c <= 32), feat f32 [p,d], curvature f32 [p].
 * Workspace: lidal_region_scores_workspace_bytes(p). */
int64_t lidal_region_scores_workspace_bytes(int64_t p);
int lidal_region_scores(const float* prob, int64_t p, int c, const float* feat, int d, const float* curvature,
                        const int64_t* sv_ptr, const int64_t* sv_idx, int s, float alpha, float gamma, float* sv_scores,
                        float* sv_feats, int64_t* sv_pnums, void* ws, int64_t ws_bytes, void* stream);
/* One k-means run: greedy k-means++ seeding from row `first` with the host-drawn uniforms
 * u f64 [(k-1) * trials] (device), then up to max_iter Lloyd iterations (stop: labels unchanged, or the summed squared
 * centre shift <= tol), then a final assignment.  x f32 [n,d] (d <= 128).  Out: seeds i32 [k], labels i32 [n],
 * centers f64 [k,d] (device); *inertia_host, *n_iter_host (host).  Synchronises the stream once per iteration.
 * Workspace: lidal_kmeans_workspace_bytes(n, d, k, trials). */
int64_t lidal_kmeans_workspace_bytes(int64_t n, int d, int k, int trials);
int lidal_kmeans(const float* x, int64_t n, int d, int k, int64_t first, const double* u, int trials, int max_iter,
                 double tol, int32_t* seeds, int32_t* labels, double* centers, double* inertia_host,
                 int32_t* n_iter_host, void* ws, int64_t ws_bytes, void* stream);

/* ---- size-constrained k-means supervoxels (dataset/prepare_supervoxel_kmeans_{sk,nu}.py; csrc/supervoxel.hip;
 *      DESIGN.md section 11) ------------------------------------------------------------------------------------ */
/* Error words of the balanced assignment (status[2 f]; 0: none).  Nothing retries: the caller raises. */
enum {
  LIDAL_FLOW_INFEASIBLE = 1,  /* k * size_min > p, k * size_max < p, or size_min outside 0..size_max */
  LIDAL_FLOW_NO_TARGET = 2,   /* no deficit node can be reached */
  LIDAL_FLOW_WALK = 3,        /* the walk back along the parents does not end at an excess node in k steps */
  LIDAL_FLOW_NOT_SETTLED = 4, /* the distances still change after k + 1 rounds (a negative cycle) */
  LIDAL_FLOW_NO_POINT = 5     /* an arc of the path has no point */
};
/* The integer arc costs: cost i32 [p,k] = rint(1000 * sqrt((dx*dx + dy*dy) + dz*dz)) in f64, every product and sum
 * rounded, ties to even; xyz f32 [p,3] widened against centers f64 [k,3].  1 <= k <= 64; finite coordinates of
 * magnitude below 5e5 keep the cost inside an int32 (not checked here: lidal_amd.data does). */
int lidal_supervoxel_costs(const float* xyz, int64_t p, const double* centers, int k, int32_t* cost, void* stream);
/* The exact least-cost labels with every cluster size in [size_min, size_max], for a batch of frames in one launch (one
 * workgroup per frame, successive shortest paths on the k + 1 node cluster graph).  cost i32 [p_total, k] (row p of
 * frame f at frame_ptr[f] + p), frame_ptr i64 [n_frames + 1], size_min / size_max i32 [n_frames]: all on the device;
 * 1 <= k <= 64.  Out (device): labels i32 [p_total], counts i32 [n_frames, k] (the cluster sizes; may be NULL),
 * objective i64 [n_frames] (the sum of cost[p][labels[p]]), status i32 [n_frames, 2] = (error word, augmentations).
 * A frame with an error word keeps the labels it had reached.  Workspace: lidal_balanced_assign_workspace_bytes. */
int64_t lidal_balanced_assign_workspace_bytes(int64_t p_total, int n_frames, int k);
int lidal_balanced_assign(const int32_t* cost, const int64_t* frame_ptr, int n_frames, int64_t p_total, int k,
                          const int32_t* size_min, const int32_t* size_max, int32_t* labels, int32_t* counts,
                          int64_t* objective, int32_t* status, void* ws, int64_t ws_bytes, void* stream);
/* The whole definition for a batch of frames: per frame the greedy k-means++ seeds of lidal_kmeans (from row first[f]
 * with the uniforms u f64 [n_frames, (k-1) * trials] on the device), costs rint(1000 * distance) to the seed rows, a
 * balanced assignment, the centre update of lidal_kmeans, costs again and a second balanced assignment.  xyz f32
 * [p_total, 3] (device); frame_ptr, size_min, size_max, first: HOST arrays.  Out (device): seeds i32 [n_frames, k],
 * labels_first i32 [p_total], centers f64 [n_frames, k, 3] (the updated ones), labels i32 [p_total], order i32 [p_total]
 * (per frame its point ids sorted by (label, point)), counts i32 [n_frames, k] (of `labels`), objective i64
 * [2, n_frames], status i32 [2, n_frames, 2] (first, second assignment).  Does not synchronise the stream.
 * Workspace: lidal_supervoxel_kmeans_workspace_bytes(p_total, the largest frame, n_frames, k, trials). */
int64_t lidal_supervoxel_kmeans_workspace_bytes(int64_t p_total, int64_t p_max, int n_frames, int k, int trials);
int lidal_supervoxel_kmeans(const float* xyz, const int64_t* frame_ptr_host, int n_frames, int k,
                            const int32_t* size_min_host, const int32_t* size_max_host, const int64_t* first_host,
                            const double* u, int trials, int32_t* seeds, int32_t* labels_first, double* centers,
                            int32_t* labels, int32_t* order, int32_t* counts, int64_t* objective, int32_t* status,
                            void* ws, int64_t ws_bytes, void* stream);

/* ---- VCCS supervoxels (dataset/prepare_supervoxel_VCCS_{sk,nu}.py, which pipe every scan through a PCL program;
 *      csrc/vccs.hip; DESIGN.md section 12: this project's definition, not the library's labels) ------------------- */
/* Error words (status[0]; 0: none).  Nothing retries: the caller raises. */
enum {
  LIDAL_VCCS_CELL_RANGE = 1,   /* a cell or seed cell does not fit 21 bits per axis */
  LIDAL_VCCS_NO_SLOT = 2,      /* an occupied cell is not found among the voxels' keys */
  LIDAL_VCCS_NO_CANDIDATE = 3  /* a seed cell without a voxel */
};
/* A batch of scans in one chain of launches: xyz f32 [p_total, 3] (device), frame_ptr HOST i64 [n_frames + 1].  Voxels
 * are numbered across the batch, frame after frame, in (x, y, z) order of their cells; so are the supervoxels, in
 * (x, y, z) order of their seed cells.  Out (device; every per-voxel and per-supervoxel array has p_total rows, of
 * which the first V resp. S are written): labels i64 [p_total] (1.. inside the frame, 0: none), point_voxel i32
 * [p_total], cells i32 [.,3], qs i64 [.,3] (sums of rint(x * 65536)), nv i32 [.], centroids f64 [.,3], normals f64
 * [.,3], seed_voxels i32 [.] (the voxel of supervoxel s), owners i32 [.] (the voxels' labels), order i32 [p_total] (the
 * batch's points sorted by (frame, label, point)), counts i32 [.] (points per supervoxel), status i64
 * [4 + 2 (n_frames + 1)] = {error word, V, seed cells, S, first voxel of every frame and V, first supervoxel of every
 * frame and S}.  min_seed and rounds come from the host (lidal_amd.data).  1 <= points per frame < 2^24, fewer than
 * 2^31 / 27 points in the batch (the 27-offset table is indexed by an int).  Does not synchronise the stream.
 * Workspace: lidal_vccs_workspace_bytes(p_total, n_frames). */
int64_t lidal_vccs_workspace_bytes(int64_t p_total, int n_frames);
int lidal_vccs(const float* xyz, const int64_t* frame_ptr_host, int n_frames, double voxel_resolution,
               double seed_resolution, double spatial_importance, double normal_importance, double min_seed, int rounds,
               int64_t* labels, int32_t* point_voxel, int32_t* cells, int64_t* qs, int32_t* nv, double* centroids,
               double* normals, int32_t* seed_voxels, int32_t* owners, int32_t* order, int32_t* counts, int64_t* status,
               void* ws, int64_t ws_bytes, void* stream);

/* ---- frame-level selection (score/frame_level/ of the reference; csrc/frame_level.hip) ---------------------- */
/* softmax_entropy.py, margin_sampling.py, least_confidence_sampling.py worker_func for one frame, prob f32 [p,c]
 * (2 <= c <= 32): out f32 [3] = (np.mean(entropy(prob, axis=1)), np.mean(top1 - top2), np.mean(top1)), numpy's
 * orders (pairwise row sums, blocked f32 means), entr in f64 rounded to f32.  Precondition, not checked here: prob is
 * finite (lidal_amd.score.frame_level checks it).  Workspace: lidal_frame_uncertainty_workspace_bytes(p). */
int64_t lidal_frame_uncertainty_workspace_bytes(int64_t p);
int lidal_frame_uncertainty(const float* prob, int64_t p, int c, float* out, void* ws, int64_t ws_bytes, void* stream);
/* segment_entropy.py worker_func: pred i64 [p], the supervoxel CSR (sv_ptr i64 [s+1], sv_idx i64 with values in
 * [0, p)), 1 <= class_num <= 256 -> *out f64 (device): sum over supervoxels, in order, of sv * n / p, sv the f64
 * log2 entropy of the predicted-class histogram (an empty supervoxel gives NaN).  Workspace:
 * lidal_segment_entropy_workspace_bytes(s). */
int64_t lidal_segment_entropy_workspace_bytes(int s);
int lidal_segment_entropy(const int64_t* pred, int64_t p, const int64_t* sv_ptr, const int64_t* sv_idx, int s,
                          int class_num, double* out, void* ws, int64_t ws_bytes, void* stream);
/* core_set.py:66: outfeat.mean(0) of feat f32 [p,d] -> out f32 [d]: per column the sequential f32 sum of the rows
 * (d == 1: numpy's blocked pairwise mean of the contiguous column).  Workspace: lidal_frame_feature_workspace_bytes(p). */
int64_t lidal_frame_feature_workspace_bytes(int64_t p);
int lidal_frame_feature(const float* feat, int64_t p, int d, float* out, void* ws, int64_t ws_bytes, void* stream);
/* core_set.py:74-92, the greedy k-center over feats f32 [n,d] (d <= 128) from the labeled rows labeled i64
 * [n_labeled >= 1] (device): picks i64 [num_add] in pick order and the final min_dist f32 [n].  dist = f32 sqrt of
 * f32(the pairwise-order f64 sum of squared differences); argmax takes the lowest row on ties.  status_dev i32 [2]:
 * [0] = t > 0 if pick t (1-based) was already selected (the reference asserts), [1] = labeled ids outside [0, n).
 * num_add <= n - n_labeled.  Workspace: lidal_coreset_workspace_bytes(n, num_add). */
int64_t lidal_coreset_workspace_bytes(int64_t n, int num_add);
int lidal_coreset(const float* feats, int64_t n, int d, const int64_t* labeled, int64_t n_labeled, int num_add,
                  int64_t* picks, float* min_dist, int32_t* status_dev, void* ws, int64_t ws_bytes, void* stream);

/* ---- row-wise helpers of a planned step (what torch glue did between the operators) ------------- */
/* dst[r][0 : row_bytes) = src[r][0 : row_bytes), dst[r][row_bytes : row_bytes + zero_bytes) = 0 for r < rows; rows
 * `src_pitch` / `dst_pitch` bytes apart.  One call per summand is torchsparse.cat (operators.py; network/spvcnn.py:
 * 133,137,145,149) into the channel slices of one buffer; with zero_bytes > 0 it is the channel padding of the
 * 19-class logit gradient; with src_pitch > row_bytes the contiguous copy of a channel slice. */
int lidal_copy2d(const void* src, int64_t src_pitch, void* dst, int64_t dst_pitch, int64_t rows, int64_t row_bytes,
                 int64_t zero_bytes, void* stream);
/* out[r][:c] = a[r][:c] + b[r][:c] (f32 sum rounded once to `dtype`): the sum autograd forms where a tensor has
 * two consumers (an encoder level feeds the next stage AND a decoder concatenation: network/spvcnn.py:120-128);
 * row strides in elements (a channel slice of a concatenation's gradient is read in place); c and the strides
 * whole 16-byte vectors. */
int lidal_add2d(const void* a, int64_t a_stride, const void* b, int64_t b_stride, void* out, int64_t out_stride,
                int64_t rows, int c, int dtype, void* stream);
/* dst f32 [cols][rows] = transpose of src f32 [rows][cols] (rows `src_stride` floats apart): nn.Linear keeps its
 * weight as [Cout][Cin], the weight-gradient kernel produces x^T g = [Cin][Cout]. */
int lidal_transpose_f32(const float* src, int64_t src_stride, float* dst, int rows, int cols, void* stream);
/* dst bf16 [n][c_dst] = src f32 [n][c_src] rounded to nearest even, channels c_src.. zero-filled (the 4-channel
 * input of the stem under bf16: 8-byte rows padded to one 16-byte vector, nn/functional/conv.py _pad_channels). */
int lidal_cast_rows_bf16(const float* src, int c_src, void* dst, int c_dst, int64_t n, void* stream);

/* ---- optimizer ---------------------------------------------------------------------------------------- */
/* replaces optimizer.step() of torch.optim.Adam (train.py:56,140) for any number of f32 tensors in ONE launch, no
 * synchronisation, nothing read back (csrc/optim.hip).  Per element, every operation rounded separately in f32
 * (correctly rounded sqrt and divide, subnormals kept) -- torch's single-tensor Adam:
 *     g = grad (+ weight_decay * p if weight_decay != 0);   m = m + (g - m) * one_minus_beta1;
 *     v = v * beta2 + (one_minus_beta2 * g) * g;            den = sqrtf(v) / bias_correction2_sqrt + eps;
 *     p = p + neg_step_size * (m / den)
 * with the scalars, computed by the host in double, cast to float here: bias_correction2_sqrt = sqrt(1 - beta2^t),
 * neg_step_size = -(lr / (1 - beta1^t)).
 * `table` (device): records of five 64-bit words, one per tensor --
 *     { address of p,  gradient's byte offset from grad_base,  first element of its m / v in the flat f32 state buffers
 *       `m` / `v` [state_numel],  vstart,  n elements }
 * -- of which the launch updates records [rec_begin, rec_end).  vstart places the tensor on a virtual element axis that
 * the kernel cuts into chunks of lidal_adam_chunk_elems() elements (vstart ascending with the record index, ranges
 * disjoint, gaps allowed; 16-byte accesses wherever the addresses of p, gradient and state share one 16-byte phase,
 * which vstart = address of p / 4 mod 32 = state offset mod 32 arranges for the chunks' boundaries too); [v_begin, v_end)
 * covers the virtual ranges of the launch's records.  grad_base: NULL with absolute gradient addresses in the table,
 * or the address the table's offsets are relative to (a flat gradient buffer that is a fresh allocation every step:
 * the table stays as it is).  A record whose state range leaves [0, state_numel) is skipped. */
int lidal_adam_chunk_elems(void);
int lidal_adam_step(const void* table, int rec_begin, int rec_end, int64_t v_begin, int64_t v_end, const void* grad_base,
                    float* m, float* v, int64_t state_numel, double one_minus_beta1, double beta2, double one_minus_beta2,
                    double bias_correction2_sqrt, double eps, double neg_step_size, double weight_decay, void* stream);
/* The same launch (table, records, virtual axis, grad_base, state buffers: all as lidal_adam_step) for the two forms
 * lidal_adam_step does not have:
 *   decoupled != 0: AdamW, torch's decoupled_weight_decay=True -- p = p * (float)decay_factor first (the host passes
 *     1 - lr * weight_decay), then the five lines with g = grad; `weight_decay` itself is not used;
 *   clip_coef != NULL (device, one float): g = grad * *clip_coef, rounded, before anything else -- also when it is 1.
 *     The gradient itself is not written.
 * decoupled == 0 needs clip_coef (the coupled form without clipping IS lidal_adam_step). */
int lidal_adam_step_ex(const void* table, int rec_begin, int rec_end, int64_t v_begin, int64_t v_end, const void* grad_base,
                       float* m, float* v, int64_t state_numel, double one_minus_beta1, double beta2,
                       double one_minus_beta2, double bias_correction2_sqrt, double eps, double neg_step_size,
                       double weight_decay, int decoupled, double decay_factor, const float* clip_coef, void* stream);
/* SGD over the same table in one launch -- torch's _single_tensor_sgd, every operation rounded separately in f32:
 *     g = grad (* *clip_coef if clip_coef != NULL) (+ weight_decay * p if weight_decay != 0)
 *     momentum != 0:  buf = g (first_step != 0: buf is written, not read)  or  buf = buf * momentum + one_minus_dampening * g;
 *                     g = g + momentum * buf (nesterov != 0)  or  g = buf
 *     p = p + neg_lr * g
 * `momentum_buffer` [state_numel] is the ONE flat state buffer (the table's state word indexes it); with momentum == 0
 * it may be NULL and nothing but p and the gradient is touched. */
int lidal_sgd_step(const void* table, int rec_begin, int rec_end, int64_t v_begin, int64_t v_end, const void* grad_base,
                   float* momentum_buffer, int64_t state_numel, double momentum, double one_minus_dampening, double neg_lr,
                   double weight_decay, int nesterov, int first_step, const float* clip_coef, void* stream);
/* The global gradient norm of torch's clip_grad_norm_ without a read-back.  lidal_grad_norm_partials writes, for records
 * [rec_begin, rec_end) of the table, the f64 sum of g * g of every block of lidal_grad_norm_block_elems() elements of
 * every tensor: block j of record r goes to partials[slot_start[r] + j], slot_start (device, int64 [records + 1]) being
 * the running sum of ceil(n_r / block) and n_slots its last entry (the size of `partials`).  The order of the additions
 * is a function of the record and the element's index inside its tensor only (csrc/optim.hip): not of the grid, the
 * addresses or grad_base.  zero != 0 writes 0 to those slots instead (records that have no gradient this step).
 * lidal_grad_norm_finish (one workgroup) adds the n_slots partials in ascending order and writes
 *     out[0] = total = (float)sqrt(sum),   out[1] = min((float)max_norm / (total + 1e-6f), 1)   (a NaN stays a NaN). */
int lidal_grad_norm_block_elems(void);
int lidal_grad_norm_partials(const void* table, const int64_t* slot_start, int rec_begin, int rec_end,
                             const void* grad_base, double* partials, int64_t n_slots, int zero, void* stream);
int lidal_grad_norm_finish(const double* partials, int64_t n_slots, double max_norm, float* out, void* stream);

/* ---- the mean-teacher step (csrc/semi.hip; not plan operations: all of it is the caller's loop) ------------ */
/* The teacher as an exponential moving average of the student over any number of tensors in ONE launch, no
 * synchronisation, nothing read back.  `table` (device): records of five 64-bit words, one per tensor --
 *     { address of the teacher's tensor,  address of the student's,  vstart,  n 32-bit words,  kind }
 * kind 0: t = t + (s - t) * (float)one_minus_alpha per f32 element, the two operations rounded separately (subnormals
 * kept, NaN / Inf as IEEE says);  kind 1: the words are copied, no arithmetic touches them (an int64 is two words).
 * all_copy != 0 treats every record as kind 1 (alpha == 0: t + (s - t) is not s in floating point).
 * vstart places the tensor on a virtual axis of words that the kernel cuts into chunks of lidal_ema_chunk_elems()
 * (ascending with the record index, ranges disjoint, gaps allowed, the first at or above 0, the last ending at or
 * below v_end); 16-byte accesses wherever the two addresses share one 16-byte phase, 4-byte accesses otherwise and for
 * the up to three words before / after the whole vectors.  Records with n <= 0 are skipped. */
int lidal_ema_chunk_elems(void);
int lidal_ema_step(const void* table, int n_recs, int64_t v_end, double one_minus_alpha, int all_copy, void* stream);
/* Pseudo labels from a teacher's logits [nv, c] (dtype LIDAL_F32 / LIDAL_BF16, c in 1..32), one launch behind a memset
 * of `stats`.  Per point i < p: its row is inverse[i] (inverse NULL: row i, and p == nv); arg = the first maximum of the
 * row, conf = expf(x_arg - mx) / sum_k expf(x_k - mx), the f32 sum in class order.
 *     out[i] = labels[i]                  where labels != NULL and labels[i] != ignore_index (in none of the counts)
 *            = ignore_index               where the row is outside [0, nv): counted in stats[c + 1], never read through
 *            = arg                        where conf >= thresholds[arg] (thresholds NULL: >= (float)threshold): stats[arg]
 *            = ignore_index               otherwise (a row with a NaN always: the comparison is false): stats[c]
 * out i64 [p], stats i64 [c + 2], conf f32 [p] or NULL (0 where the row is outside). */
int lidal_pseudo_labels(const void* logits, int dtype, int64_t nv, int c, const float* thresholds, double threshold,
                        const int64_t* inverse, const int64_t* labels, int64_t ignore_index, int64_t p, int64_t* out,
                        int64_t* stats, float* conf, void* stream);
/* Consistency between a student's and a teacher's rows [n, c] (each LIDAL_F32 or LIDAL_BF16 logits; is_probs = 1: f32
 * probabilities, kind 0 only), c in 1..32, 0 < n, n * c < 2^30.  Both softmaxes are the f32 row softmax above;
 * m_i = [teacher conf_i >= (float)min_conf]; r_i = np_sum_f32 over the classes of
 *     kind 0 'mse':  fl(d_k * d_k), d_k = fl(ps_k - pt_k);                              denom = n * c
 *     kind 1 'kl' :  pt_k * (lt_k - ls_k), 0 where pt_k == 0, l_k = (z_k - mx) - logf(s);   denom = n
 * out2 f64 [2] = { sum_i m_i r_i / denom, sum_i m_i r_i }: f64 partials per workgroup of 256 rows, then one workgroup, a
 * fixed order.  per_row f32 [n] or NULL: m_i r_i.  Two launches; workspace lidal_consistency_workspace_bytes(n).
 * Backward (one launch), g = grad_scale[0] read on the device, dz in the student's dtype, 0 where m_i == 0:
 *     'mse' on logits:        dz_k = (g * (float)(1 / (n c))) * (ps_k * (2 d_k - sum_j ps_j * (2 d_j))), j ascending in f32
 *     'mse' on probabilities: dz_k = (g * (float)(2 / (n c))) * d_k
 *     'kl':                   dz_k = (g * (float)(1 / n)) * (ps_k - pt_k)
 * every product and difference one f32 operation, the constants formed in double. */
int64_t lidal_consistency_workspace_bytes(int64_t n);
int lidal_consistency_fwd(const void* student, int s_dtype, const void* teacher, int t_dtype, int64_t n, int c, int kind,
                          int is_probs, double min_conf, double* out2, float* per_row, void* ws, int64_t ws_bytes,
                          void* stream);
int lidal_consistency_bwd(const void* student, int s_dtype, const void* teacher, int t_dtype, int64_t n, int c, int kind,
                          int is_probs, double min_conf, const float* grad_scale, void* dz, void* stream);

/* ---- launch plans ----------------------------------------------------------------------------------- */
/* A whole forward or backward pass as ONE call: `words` is a stream of n_ops operations,
 *     kind | flags << 16,  arg 0, arg 1, ...
 * one 64-bit word each; an operation of kind LIDAL_OP_X calls lidal_x with the words as its arguments IN THE ORDER
 * OF ITS PROTOTYPE ABOVE, stream excluded: pointers as addresses, integers as such, float arguments as the bit
 * pattern of a double (lidal_plan_op_args(kind) words).  The operations are queued on `stream` in order --
 * exactly the launches the same calls made one by one would queue (train.py:127-140 / prob_inference.py:91-113
 * issue theirs one Python call at a time); nothing is captured or cached, every call walks the words it is given.
 * The flags of an operation name the stream it is queued on: 0 = `stream`, i = side stream i (1, LIDAL_OP_FLAG_SIDE, is
 * `side_stream`, which may be NULL if unused; lidal_plan_run_streams takes streams[0] = the main stream and up to 7 side
 * streams), between a LIDAL_OP_FORK_SIDE with the same flags (side stream i waits for what the main stream holds so
 * far) and a LIDAL_OP_JOIN_SIDE (the main stream waits for side stream i).  Stops at the first failing operation;
 * lidal_last_error() names its index and kind. */
enum {
  LIDAL_OP_CONV_WEIGHT_IMAGE_BATCH = 1, LIDAL_OP_CONV_APPLY_IMAGE = 2, LIDAL_OP_CONV_DGRAD_BN_SUMS = 3,
  LIDAL_OP_CONV_WGRAD = 4, LIDAL_OP_BN_TRAIN_FWD = 5, LIDAL_OP_BN_TRAIN_FWD_TILES = 6, LIDAL_OP_BN_BWD = 7,
  LIDAL_OP_BN_BWD_TILES = 8, LIDAL_OP_BN_EVAL_FWD = 9, LIDAL_OP_BN_FOLD = 10, LIDAL_OP_COLSUM = 11,
  LIDAL_OP_ADD_RELU_FWD = 12, LIDAL_OP_ADD_RELU_BWD = 13, LIDAL_OP_VOXELIZE_FWD_1TO1 = 14,
  LIDAL_OP_VOXELIZE_FWD_SORTED = 15, LIDAL_OP_VOXELIZE_BWD = 16, LIDAL_OP_DEVOXELIZE_FWD = 17,
  LIDAL_OP_DEVOXELIZE_BWD_SORTED = 18, LIDAL_OP_CE_FWD = 19, LIDAL_OP_CE_BWD = 20, LIDAL_OP_COPY2D = 21,
  LIDAL_OP_ADD2D = 22, LIDAL_OP_TRANSPOSE_F32 = 23, LIDAL_OP_CAST_ROWS_BF16 = 24, LIDAL_OP_VIEW_MEAN_SOFTMAX = 25,
  LIDAL_OP_FORK_SIDE = 26, LIDAL_OP_JOIN_SIDE = 27, LIDAL_OP_CONV_APPLY_IMAGE_WS = 28,
  LIDAL_OP_CONV_DGRAD_BN_SUMS_WS = 29, LIDAL_OP_ADD_RELU_BWD_BN_SUMS = 30, LIDAL_OP_BN_BWD_FROM_SUMS = 31,
  LIDAL_OP_ADD_RELU_BWD_BN_TILE_SUMS = 32, LIDAL_OP_DEVOXELIZE_BWD_CELLS = 33,
  LIDAL_OP_CONV_WGRAD_STREAMS = 34, LIDAL_OP_DROPOUT_APPLY = 35
};
#define LIDAL_OP_FLAG_SIDE 1
int lidal_plan_op_args(int kind);
/* test / debug aid: synchronous copy of `nbytes` of device memory at address `dev` to `host` (a plan names its
 * buffers by address; tests that replay its operations against the oracle read the operands back with this) */
int lidal_debug_read(const void* dev, void* host, int64_t nbytes);
int lidal_plan_run(const int64_t* words, int64_t n_words, int64_t n_ops, void* stream, void* side_stream);
int lidal_plan_run_streams(const int64_t* words, int64_t n_words, int64_t n_ops, void* const* streams, int n_streams);
/* A LIDAL_OP_FORK_SIDE directly behind an operation of the main stream makes its side stream wait for that operation's
 * last LAUNCH (the event rides on the launch: no marker on the main stream); where the operation in front cannot carry
 * the event -- it ran on a side stream, its last launch does not take one, the fork opens the plan -- the fork records a
 * marker behind it.  Same ordering either way.  out[0] = forks attached to a launch, out[1] = forks that recorded a
 * marker, both since the process started or since the last call with out == NULL, which resets them. */
int lidal_plan_fork_counts(int64_t out[2]);

#ifdef __cplusplus
}
#endif
#endif /* LIDAL_AMD_H */
