/*
 * hnr.h -- C ABI of libhnr_hip.so: the MI355X-native replacement for the hot path of
 * CVMI-Lab/HybridNeuralRendering (per-ray voxel k-NN neural-point query -> point/image
 * feature gather + aggregation MLP -> front-to-back alpha composite).
 *
 * Conventions
 *   - every pointer whose name starts with d_ is a DEVICE pointer (HBM); everything else is host memory;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); no entry point synchronises
 *     the host unless its comment says so;
 *   - return value: 0 = HNR_OK, negative = error (never aborts, never throws);
 *   - all floating point is fp32, all indices int32, masks int8; the batch dimension B of the
 *     reference is always 1 and is dropped;
 *   - the caller owns every buffer; the only internal allocations are the index arrays owned by an
 *     hnr_grid handle and a small per-process scratch of counters;
 *   - ONE PROCESS PER GPU is the supported deployment (the multi-GPU path is one rank per GPU over RCCL): kernel attributes (large dynamic
 *     LDS) and the CU count are cached per device, but the training calls' side streams and the small per-process scratch belong to the
 *     device that was current when they were first used.
 *
 * Each entry point cites the reference interface it replaces (paths relative to the reference repo).
 *
 * STABILITY.  Two tiers:
 *   STABLE  -- what a reference-side binding needs and what later versions keep source- and binary-compatible: hnr_version,
 *              hnr_last_error, hnr_points_bounds, hnr_grid_* (build / destroy / stats / bytes), hnr_march_query, hnr_ray_compact*, hnr_point_records (+ _parts),
 *              hnr_image_features*, hnr_render_forward* (+ workspace sizing), hnr_render_train_forward / _backward / _backward_depth (+ sizing),
 *              hnr_shipped_loss*, hnr_composite, hnr_ray_depth, hnr_ray_march, hnr_voxel_downsample*, hnr_probe_select, hnr_blur_*,
 *              hnr_frame_metrics* (and the HNR_FM_* row layout), hnr_depth_fuse*, hnr_range_crop*, hnr_nearest_view, hnr_point_view_attrs,
 *              hnr_featnet_*, hnr_point_embed*, hnr_geo_consistency, hnr_geo_filter_select*, hnr_mvsnet_*,
 *              hnr_alpha_pack, hnr_visual_hull_select*, hnr_point_occlusion*, hnr_point_view_attrs_vis,
 *              hnr_frame_batch*, hnr_frame_item, hnr_ray_miss_rank, hnr_raft_flow*, hnr_blur_score_pair* (hnr_blur_edges and the other hnr_raft_*
 *              entries are STAGE), hnr_adam_plan, hnr_adam_step, hnr_frame_depth_rays, hnr_depth_loss, hnr_depth_metrics (and the HNR_DM_* row layout),
 *              hnr_ssim_loss, hnr_ssim_loss_scratch_bytes, hnr_pose_views, hnr_path_item, hnr_frame_store,
 *              hnr_resize_coeffs, hnr_resize_u8 (+ _scratch_bytes, _form), hnr_rgba_premultiply, hnr_rgba_unpremultiply, hnr_rgba_compose.
 *   STAGE   -- everything else (hnr_chain_*, hnr_mlp3_*, hnr_merge*, hnr_mixup_stage, hnr_proj_*, hnr_h2*, hnr_linear_*, hnr_gather_*, hnr_ksum*,
 *              hnr_segment_*, hnr_absmax, hnr_div_probe, hnr_image_features_bwd_bbox, the glue kernels of the training backward -- hnr_final_color_bwd*,
 *              hnr_ksum_bwd_rows8, hnr_extras_dgrad, hnr_point_small_grads, hnr_point_rows_bwd, hnr_dleaky_add, hnr_sum_views, hnr_unique_points*,
 *              hnr_conf0_grad, hnr_w0fd_grad, hnr_ray_drop_flags -- ...): the individual stages the two single-call entries are built from.  They are exported so
 *              that tests/ can compare every stage with the oracle and so that tools/ can time them alone; their signatures, workspace layouts and
 *              packed-image formats follow the kernels and MAY CHANGE from one version to the next (round 4 changed what hnr_chain_forward leaves
 *              in the workspace's row scalars, for example).  Do not bind to them from outside this repository.
 */
#ifndef HNR_H
#define HNR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HNR_OK            0
#define HNR_ERR_BADARG   -1   /* NULL pointer, non-positive size, unsupported K/SR ...          */
#define HNR_ERR_HIP      -2   /* a HIP runtime call failed (hnr_last_error() has the string)     */
#define HNR_ERR_TOOBIG   -3   /* grid volume or an index would overflow 32 bits                 */
#define HNR_ERR_NOMEM    -4   /* device allocation failed                                       */
#define HNR_NEED_REBUILD  1   /* hnr_grid_grow: not an error -- the update cannot be done in place, nothing was changed; call hnr_grid_build */

#define HNR_MAX_K        32   /* neighbours per shading sample (reference scripts: 8)           */

/* Library / build identification: "hnr-hip <version> gfx950".  */
const char *hnr_version(void);
/* Text of the last error on this thread ("" if none). */
const char *hnr_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * Stage 0: bounds of the point cloud.
 * Replaces the torch.min/torch.max pair of lighting_fast_querier.get_hyperparameters
 * (models/neural_points/query_point_indices_worldcoords.py:56).
 *   d_xyz [n,3] -> d_out6 = {min_x,min_y,min_z,max_x,max_y,max_z}
 */
int hnr_points_bounds(const float *d_xyz, int n, float *d_out6, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Stage 1: voxel grid over the point cloud.  Built ONCE per point-cloud version and reused by
 * every query (the reference rebuilds it for every 2304-ray chunk).
 * Replaces build_occ_vox = claim_occ + map_coor2occ + fill_occ2pnts
 * (query_point_indices_worldcoords.py:540-602, kernels :237-381).
 */
typedef struct hnr_grid hnr_grid;

typedef struct {
    float origin[3];      /* d_coord_shift  = ranges_np[:3]        (:67, :611)                  */
    float cell[3];        /* d_voxel_size   = scaled_vsize_np      (:58)                         */
    int   dims[3];        /* d_grid_size    = scaled_vdim_np       (:71)                         */
    int   query_size[3];  /* occupancy dilation, opt.query_size     (:616 passes query_size_gpu) */
    int   P;              /* max points listed per voxel            (opt.P)                      */
    int   max_o;          /* max occupied voxels                    (opt.max_o)                  */
} hnr_grid_params;

typedef struct {
    int64_t n_points;        /* points handed in                                               */
    int64_t n_inbounds;      /* points whose voxel lies inside dims                            */
    int64_t n_occ;           /* occupied voxels kept (<= max_o)                                */
    int64_t n_dropped_voxels;/* voxels beyond max_o (reference: random replacement)            */
    int64_t n_cells_over_P;  /* voxels holding more than P points (lists truncated to first P) */
    int64_t n_dilated;       /* cells set in the dilated march mask                            */
    int64_t n_words;         /* 4x4x4 bricks (64-bit words) covering dims                      */
    int64_t bytes;           /* HBM bytes owned by the handle                                  */
} hnr_grid_stats;

/* Synchronises the host once (it must size the index arrays). */
int hnr_grid_build(const float *d_xyz, int n_points, const hnr_grid_params *p, void *stream, hnr_grid **out);
int hnr_grid_free(hnr_grid *g);
int hnr_grid_get_stats(const hnr_grid *g, hnr_grid_stats *out);
int hnr_grid_get_params(const hnr_grid *g, hnr_grid_params *out);

/* After grow_points (models/neural_points/neural_points.py:376-402: new points are APPENDED to the cloud): extends the tables of a grid in place instead of
 * rebuilding them.  d_xyz [n_points,3] is the grown cloud; its first hnr_grid_get_stats().n_points rows must be the points the grid describes, unchanged,
 * and the grid parameters (origin / cell / dims, i.e. the cloud's bounding box and opt) must still apply -- the caller checks both
 * (querier.lighting_fast_querier.grow).  On HNR_OK the grid is logically what hnr_grid_build(d_xyz, n_points, same parameters) returns: same dilated
 * mask, same per-cell lists and 3x3x3 neighbourhood runs in the same order, same counters; physically the changed lists / runs were appended in the
 * slack the build leaves behind its tables (HNR_GRID_SLACK percent, default 25) and the superseded ones stay as holes.  Returns HNR_NEED_REBUILD (> 0,
 * nothing changed) when that slack is used up, when max_o would be exceeded or was, or for grids without neighbourhood lists (P > 63).  Synchronises the
 * host twice (sizes); launches already queued keep reading the old tables.  The reference has no counterpart: it rebuilds its tables for every
 * 2304-ray chunk and leaves the process after growing (run/train_ft.py:926-952). */
int hnr_grid_grow(hnr_grid *g, const float *d_xyz, int n_points, void *stream);
/* Test hook: per cell of dims, the length of its 3x3x3 neighbourhood run (-1: the cell is not in the dilated mask) and an order-dependent hash of the
 * run's records -- two grids with equal hnr_grid_export_dense and hnr_grid_export_runs outputs answer every query identically. */
int hnr_grid_export_runs(const hnr_grid *g, int32_t *d_run_len, uint64_t *d_run_hash, void *stream);

/* Test hook: expands the device tables into the reference's dense layout so they can be compared
 * with the oracle: d_coor_occ [X*Y*Z] u8 (dilated mask), d_cell_count [X*Y*Z] i32 (-1 = voxel not
 * occupied, else min(P, points listed)), d_cell_first [X*Y*Z] i32 (first listed point id or -1). */
int hnr_grid_export_dense(const hnr_grid *g, uint8_t *d_coor_occ, int32_t *d_cell_count,
                          int32_t *d_cell_first, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Stage 2: ray march + first-SR compaction + layered k-NN.
 * Replaces mask_raypos (:384-408) + the torch cumsum compaction (:645-655) + get_shadingloc
 * (:411-433) + query_neigh_along_ray_layered (:436-522), and fuses away the materialised
 * raypos tensor of near_far_linear_ray_generation (models/rendering/diff_ray_marching.py:386).
 */
typedef struct {
    int   R;              /* rays in this launch                                                */
    int   D;              /* marched samples per ray (opt.z_depth_dim = 400)                    */
    int   SR;             /* shading samples kept per ray (opt.SR)                              */
    int   K;              /* neighbours per shading sample (opt.K), <= HNR_MAX_K                */
    int   kernel_size[3]; /* k-NN neighbourhood (opt.kernel_size); layers = (kernel_size[0]+1)/2 */
    float radius2;        /* radius_limit^2, 0 = unlimited (:493, :685)                         */
    int   tmid_stride;    /* 0: d_tmid is one [D] table shared by all rays (jitter = 0);
                             D: d_tmid is [R,D], one depth table per ray (train-time jitter)    */
    int   pad_outputs;    /* 1: d_sample_pidx / d_sample_loc_w are fully written, -1 / 0 in the unused slots
                             (the reference's torch.full / torch.zeros tensors, :647-648);
                             0: only the first d_ray_nsamp[r] slots of a ray are written (fused path: consumers
                             take d_ray_nsamp; saves 1 kB of padding stores per ray)                */
    int   knn_order;      /* 0: the K slots of a sample are filled exactly as the reference kernel fills them (insertion
                             history, farthest-first replacement: query_point_indices_worldcoords.py:494-513);
                             1: the same neighbour SET in canonical order, ascending (d^2, enumeration order) -- a sorted
                             insertion instead of the replay of that rule (K = 8, 3x3x3 neighbourhood); every consumer of
                             the path sums over the K slots, so only the fp32 summation order of a sample changes.
                             Caveat: with EXACT d^2 ties at the current maximum of a full list the retained point can differ
                             (the reference evicts the first maximum in slot order, the sorted list the latest-enumerated
                             of the tied entries): use 0 for golden / PSNR comparisons on clouds with duplicate distances */
} hnr_query_params;

/* counters written by hnr_march_query (device, int64[HNR_NCOUNTS]) */
enum {
    HNR_CNT_RAYS_HIT = 0,     /* rays with >= 1 occupied marched sample (:645-646)              */
    HNR_CNT_SAMPLES,          /* shading samples kept over all rays                             */
    HNR_CNT_RAYS_VALID,       /* rays with >= 1 neighbour (:705-706), filled by hnr_ray_compact_plan */
    HNR_CNT_NEIGHBOURS,       /* sample_pidx entries >= 0                                       */
    HNR_CNT_CELLS_VISITED,    /* occupied cells whose lists were scanned by the k-NN            */
    HNR_CNT_CANDIDATES,       /* points distance-tested by the k-NN                             */
    HNR_CNT_SAMPLES_VALID,    /* shading samples with >= 1 neighbour                            */
    HNR_CNT_SAMPLES_SMALL,    /* written by hnr_chain_plan: valid samples of its second class (4 row slots: at most 4 neighbours
                                 with classes = 1, 3..4 with classes = 2), listed AFTER the first class in its d_vs_item (0 after
                                 hnr_march_query: every sample counts as a full one)                                      */
    HNR_CNT_SAMPLES_TINY,     /* written by hnr_chain_plan(classes = 2): valid samples with 1..2 neighbours (2 row slots), listed last */
    HNR_NCOUNTS = 9
};

/*
 * Outputs are in the UN-COMPACTED ray order (row r = input ray r):
 *   d_sample_pidx  [R,SR,K] i32, -1 padded         (reference: sample_pidx before :708)
 *   d_sample_loc_w [R,SR,3] f32, 0 padded          (reference: sample_loc before :709)
 *   d_ray_nsamp    [R]      i32  shading samples kept on the ray
 *   d_ray_mask     [R]      i8   1 iff the ray has >= 1 neighbour (reference: ray_mask, :707,:711)
 *   d_work         i32[hnr_query_work_elems(R,SR)]  scratch; its first counts[HNR_CNT_SAMPLES] entries are the
 *                  packed (ray*SR+slot) list of kept samples in (ray, slot) order
 *   d_counts       [HNR_NCOUNTS] i64
 * d_campos [3], d_raydir [R,3], d_tmid see tmid_stride.  No host synchronisation.
 */
int64_t hnr_query_work_elems(int R, int SR);
int hnr_march_query(const hnr_grid *g, const float *d_campos, const float *d_raydir, const float *d_tmid,
                    const hnr_query_params *q,
                    int32_t *d_sample_pidx, float *d_sample_loc_w, int32_t *d_ray_nsamp, int8_t *d_ray_mask,
                    int32_t *d_work, int64_t *d_counts, void *stream);

/*
 * Second compaction of the reference (:705-709), the ray-direction expansion of query_points
 * (:91) and the camera-perspective sample coordinates (x/z, y/z, z) of lighting_fast_querier.w2pers
 * (:96-103): rows of rays with ray_mask = 1, in ray order.
 *   hnr_ray_compact_plan : d_ray_row [R] i32 = compact row of ray r or -1; d_counts[HNR_CNT_RAYS_VALID].
 *   hnr_ray_compact      : d_out_* sized for n_valid rows (read d_counts on the host in between).
 * d_scratch: int32[(R+1023)/1024 + 1].
 */
int hnr_ray_compact_plan(const int8_t *d_ray_mask, int R, int32_t *d_ray_row, int32_t *d_scratch,
                         int64_t *d_counts, void *stream);
int hnr_ray_compact(const int32_t *d_ray_row, int R, int SR, int K,
                    const int32_t *d_sample_pidx, const float *d_sample_loc_w, const float *d_raydir,
                    const float *d_campos /*[3]*/, const float *d_camrotc2w /*[3,3] row-major*/,
                    int32_t *d_out_pidx /*[R',SR,K]*/, float *d_out_loc_w /*[R',SR,3]*/,
                    float *d_out_loc_pers /*[R',SR,3] = w2pers(loc_w), :96-103*/,
                    float *d_out_raydir /*[R',SR,3]*/, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Stage 3a: dense layers of the aggregation MLP on the matrix cores (fp32 in, fp32 accumulate).
 * Replaces the nn.Linear(+LeakyReLU) layers of PointAggregator.viewmlp
 * (models/aggregators/point_aggregators.py:948 block1, :972 block3, :1037 color_feature_branch,
 *  :1199 aux_merge_weight_block, :1292 color_mixup_block).
 *   C[M,N] = act(A[M,K] * W[N,K]^T + bias[N]),  act: 0 = none, 1 = LeakyReLU(slope)
 * W is the torch nn.Linear weight ([out,in], row-major).  It is packed ONCE per checkpoint into a
 * zero-padded [N_pad,K_pad] image (+ bias[N_pad]) by hnr_linear_pack; sizes from hnr_linear_packed_dims.
 * lda must be a multiple of 4 floats and A 16-byte aligned; ldc >= N.
 */
int hnr_linear_packed_dims(int N, int K, int *N_pad, int *K_pad);
int hnr_linear_pack(const float *d_W, const float *d_bias /*may be NULL*/, int N, int K,
                    float *d_Wp /*[N_pad*K_pad]*/, float *d_bias_p /*[N_pad]*/, void *stream);
int hnr_linear_f32(const float *d_A, int lda, const float *d_Wp, const float *d_bias_p, float *d_C, int ldc,
                   int M, int N, int K, int act, float slope, void *stream);
/* Same, with a gathered per-row addend:  C[m,:] = act(A[m,:] W^T + bias + R[ridx[m], :])  (R row stride ldr >= N).
 * Used to split block1.0 (point_aggregators.py:948): its input row is [emb | PE(emb) | PE(dists)] (:931-939) and the first
 * 224 columns depend on the POINT only, so R = [emb | PE(emb)] W[:, :224]^T is computed once per point (hnr_point_rows +
 * hnr_linear_f32) and each (sample, neighbour) row only multiplies its 60 distance-encoding columns. */
int hnr_linear_f32_gather_add(const float *d_A, int lda, const float *d_Wp, const float *d_bias_p, const float *d_R,
                              const int32_t *d_ridx, int ldr, float *d_C, int ldc, int M, int N, int K, int act, float slope,
                              void *stream);
/* General form of the side operand, applied to the output columns < r_cols only (d_ridx may be NULL = row m itself):
 *   r_mode 0: C = act(A W^T + bias + R[ridx[m], :])          (d_R == d_C gives an accumulating "+=" layer)
 *   r_mode 1: C = (A W^T + bias) * (R[m, :] > 0 ? 1 : slope)  LeakyReLU derivative of the stored activation R; act must be 0.
 * r_mode 1 is the input-gradient GEMM of the backward pass (torch autograd of nn.Linear + LeakyReLU in the reference):
 * with W^T packed as the weight, dZ_prev = (dZ W) * LeakyReLU'(Y_prev). */
int hnr_linear_f32_side(const float *d_A, int lda, const float *d_Wp, const float *d_bias_p, const float *d_R,
                        const int32_t *d_ridx, int ldr, int r_cols, int r_mode, float *d_C, int ldc, int M, int N, int K,
                        int act, float slope, void *stream);
/* ------------------------------------------------------------------------------------------------
 * Stage 3b: everything of the gather / aggregate / composite path that is not a dense layer.
 * Row order is the reference's boolean-mask order, (ray, slot, k) ascending, so packed rows line up
 * with `feat[pnt_mask_flat]` / `[ray_valid]` of point_aggregators.py:924-935, :1014-1026.
 * Every function reads its work sizes from d_counts on the device (no host sync); `cap_*` arguments
 * are the capacities of the caller's buffers (grid sizes); hnr_sample_plan raises *d_overflow when a
 * capacity is too small.
 */

/* Compact lists over the kept samples of hnr_march_query (d_work, d_counts[HNR_CNT_SAMPLES]):
 *   d_vs_item[s] = ray*SR+slot of the s-th VALID sample (>= 1 neighbour; `ray_valid`, :1441),
 *   d_vs_off[s]  = index of its first neighbour row, d_vs_cnt[s] = its neighbour count.
 * d_scratch: int32[2*ceil(max_items/1024)].  max_items = R*SR. */
int hnr_sample_plan(const int32_t *d_work, const int32_t *d_sample_pidx, const int64_t *d_counts, int K, int max_items,
                    int32_t *d_vs_item, int32_t *d_vs_off, int32_t *d_vs_cnt, int cap_samples, int cap_rows,
                    int32_t *d_scratch, int32_t *d_overflow, void *stream);

/* NeuralPoints gather (neural_points.py:709-720) + w2pers (:607-613) + dists (point_aggregators.py:1472-1480)
 * + inverse-distance weights (:825-833, :1500-1501, x clamp(conf) :1508-1512) + positional encodings
 * (:930, :938) written straight into the packed MLP inputs:
 *   d_X1[row, 0:284]     = [emb32 | PE3(emb) 192 | PE5(dists6) 60]            (block1 input)
 *   d_X3[row, 256:263]   = [color3 | dir - viewdir | dir . viewdir]            (block3 extras, :957-971)
 *   d_wagg[row]          = normalised weight * clamp(conf, 1e-4, 1)
 *   optional d_weight_out / d_conf_out [R,SR,K]: the reference's `weight` and `conf_coefficient` outputs.
 * Point buffers: xyz [N,3], emb [N,32], conf [N], dir [N,3], color [N,3].
 * d_row_pid != NULL selects the SPLIT layout: d_X1[row, 0:60] = PE5(dists6) only (ld1 >= 60) and d_row_pid[row] = point id;
 * the point-only columns [emb32 | PE3(emb)] come from hnr_point_rows through hnr_linear_f32_gather_add. */
int hnr_gather_rows(const float *d_xyz, const float *d_emb, const float *d_conf, const float *d_dir, const float *d_color,
                    int F, const int32_t *d_sample_pidx, const float *d_sample_loc_w, const float *d_raydir,
                    const float *d_campos, const float *d_camrot, const int32_t *d_vs_item, const int32_t *d_vs_off,
                    const int32_t *d_vs_cnt, const int64_t *d_counts, int SR, int K, int cap_samples,
                    float *d_X1, int ld1, float *d_X3, int ld3, float *d_wagg, float *d_weight_out, float *d_conf_out,
                    int32_t *d_row_pid, void *stream);

/* d_E[p, 0:224] = [emb32 | PE3(emb) 192] for every point (point_aggregators.py:931-938): the point-only columns of
 * block1's input row.  lde >= 224, multiple of 4.  With d_ids the rows are those of the listed points only (training:
 * the points a batch touches, hnr_unique_points). */
int hnr_point_rows(const float *d_emb, const int32_t *d_ids /*NULL or [n_points] point ids*/, int n_points, int F, float *d_E, int lde,
                   void *stream);

/* The materialised gather of NeuralPoints.forward (neural_points.py:709-720) for the drop-in 14-tuple only:
 * n_entries = R'*SR*K entries of d_sample_pidx; empty entries (-1) read point 0 (the reference clamps the index);
 * outputs [n,3] [n,3] [n] [n,F] [n,3] [n,3] and d_o_mask [n] u8 = (pidx >= 0). */
int hnr_gather_points(const int32_t *d_sample_pidx, int64_t n_entries, const float *d_xyz, const float *d_emb,
                      const float *d_conf, const float *d_dir, const float *d_color, int F, const float *d_campos,
                      const float *d_camrot, float *d_o_color, float *d_o_dir, float *d_o_conf, float *d_o_emb,
                      float *d_o_xyz_pers, float *d_o_xyz, uint8_t *d_o_mask, void *stream);

/* alpha branch + softplus(x-1) (:1005, :471-476) + K-weighted sums (:1008-1026) + view-direction encoding:
 *   d_X5[s, 0:280] = [sum_k w feat_k (256) | sin(viewdir 2^f) 12 | cos 12]   (color_feature_branch input, :1028-1036)
 *   d_sigma[s]     = sum_k w softplus(alpha_k - 1) */
int hnr_ksum(const float *d_H4, int ldh, const float *d_wagg, const float *d_alpha_w, const float *d_alpha_b,
             const int32_t *d_vs_item, const int32_t *d_vs_off, const int32_t *d_vs_cnt, const float *d_raydir,
             const int64_t *d_counts, int SR, int cap_samples, float *d_X5, int ld5, float *d_sigma, void *stream);

/* Reference-view feature pyramid, once per frame (:1047-1067, :1089): conv_w/conv_b are HOST arrays of 6 device
 * pointers (aux_block_s1.{0,2}, s2.{0,2}, s3.{0,2}); d_img [V,H,W,3]; d_featmap [V,H,W,48] channels-last
 * (45 used: RGB | up(s1) 6 | up(s2) 12 | up(s3) 24), pixel (0,0) zeroed.
 * d_scratch: float[hnr_image_features_scratch_elems(V,H,W)]. */
int64_t hnr_image_features_scratch_elems(int V, int H, int W);
int hnr_image_features(const float *d_img, int V, int H, int W, const float *const *conv_w, const float *const *conv_b,
                       float slope, float *d_scratch, float *d_featmap, void *stream);

/* Merge-weight rows: reprojection into the V reference views (neural_points_volumetric_model.py:248-255,
 * d_w2c[v] = inverse(c2w_nearest[v]) row-major), truncation to a pixel + bounds rule (:1077-1088), feature
 * gather, delta view directions (:296-310):  d_X6[v*cap+s, 0:176] = [imgfeat45 | colfeat128 | ddir3], d_vmask.
 * d_row_sample != NULL selects the SPLIT layout: rows are [imgfeat45 | ddir3] (ld6 >= 48), d_row_sample[row] = s and the
 * colour feature is not copied -- its 128 columns of aux_merge_weight_block.0 are shared by the V views of a sample, so they
 * are multiplied once per sample and added per row by hnr_linear_f32_gather_add. */
int hnr_proj_rows(const float *d_sample_loc_w, const int32_t *d_vs_item, const int64_t *d_counts, const float *d_w2c,
                  const float *d_intrinsic, const float *d_campos, const float *d_campos_nearest, const float *d_featmap,
                  int V, int H, int W, const float *d_CF, int ldcf, int cap_samples, float *d_X6, int ld6, float *d_vmask,
                  int32_t *d_row_sample, void *stream);

/* Probe (parity evidence): q_hnr[i] = the library's divide-free correctly rounded quotient (hnr_div, csrc/hnr_common.h: what chain_gather_kernel and
 * train_ksum_bwd_kernel divide with instead of the v_div_scale / v_div_fmas expansion), q_ieee[i] = num[i] / den[i] as the compiler expands it. */
int hnr_div_probe(const float *d_num, const float *d_den, int n, float *d_q_hnr, float *d_q_ieee, void *stream);
/* ... and for the other two divisions of the device code: cell_hnr[i] = the query kernels' cell index floor((p[i] - origin) / c[i]) (hnr_div_cell inside
 * cell_coord; INT32_MIN beyond +-2e9 / NaN), cell_ieee[i] = the same expression with the compiler's division; q64_* = hnr_div64 (the loss kernels' means)
 * beside the compiler's fp64 division on operands derived from p, c. */
int hnr_div_probe2(const float *d_p, const float *d_c, float origin, int n, int32_t *d_cell_hnr, int32_t *d_cell_ieee, double *d_q64_hnr, double *d_q64_ieee,
                   void *stream);

/* Probe (parity evidence, not on the render path): the integer pixel every (view v, valid sample s) row of the merge stage gathers,
 * d_pix[(v * cap_samples + s) * 2 + {0,1}] = (px, py), or (-1, -1) where the reference's bounds rule masks the row -- computed by the one
 * device function (hnr_project_pixel, csrc/hnr_common.h) that hnr_proj_rows, hnr_merge_stage and hnr_proj_rows_bwd call, so that a test or
 * bench.py can tell a sample that truncates to another pixel than the CPU oracle's projection (point_aggregators.py:1077-1078: `.to(torch.int32)`
 * of a coordinate within an ulp of a pixel border) from an arithmetic difference. */
int hnr_proj_pixels(const float *d_sample_loc_w, const int32_t *d_vs_item, const int64_t *d_counts, const float *d_w2c,
                    const float *d_intrinsic, int V, int H, int W, int cap_samples, int32_t *d_pix, void *stream);

/* Last layer + sigmoid of aux_merge_weight_block, weighted merge (:1199-1217) and the mix-up input (:1286-1292):
 *   d_X7[s, 0:90] = [colfeat[:45] | sum_v w_v f_v / (sum_v w_v + 1e-6)].  d_frame_w: optional [V].
 * d_ray_drop: optional [R] u8; samples on flagged rays get merged = 0 (train-time patch drop, :1222-1237; the caller
 * builds the flags from drop_patch_rays :14-23 over the valid-ray rows). */
int hnr_merge(const float *d_X6, int ld6, const float *d_Hm, int ldh, const float *d_w_last, const float *d_b_last,
              const float *d_vmask, const float *d_frame_w, const float *d_CF, int ldcf, const int64_t *d_counts, int V,
              int cap_samples, float *d_X7, int ld7, const uint8_t *d_ray_drop, const int32_t *d_vs_item, int SR, void *stream);

/* ------------------------------------------------------------------------------------------------
 * The per-neighbour chain of PointAggregator.viewmlp fused into one kernel (csrc/chain.hip): block1 (:948), block3 on
 * [block1_out | colour | dir - viewdir | dir.viewdir] (:957-972), alpha_branch + softplus(x - 1) (:1005, :471-476) and the
 * K-weighted sums per shading sample (:1008-1026).  Replaces hnr_gather_rows + four hnr_linear_* launches + hnr_ksum of the
 * per-layer path for K = 8: activations stay on chip, only [S_v, 256] feature sums and [S_v] densities are written.
 * fp32 in / fp32 out; dense arithmetic: every operand split into two fp16 terms (22 bits), three 16-bit MFMAs per product,
 * fp32 accumulation, exact power-of-two scaling per activation row / per layer (fp32-class error, tests/test_chain_gpu.py).
 *
 * hnr_chain_pack: the four nn.Linear weights -> the kernel's image, once per checkpoint.  d_w_b1_0_dist = block1.0.weight[:, 224:284]
 *   (row stride ldw0; the point-only columns [:, :224] go into the per-point table, hnr_point_rows + hnr_linear_f32), d_w_b1_2
 *   [256,256], d_w_b3_0 [256,263], d_w_b3_2 [256,256] contiguous, biases [256], alpha_branch.0 weight [256] / bias [1].
 * hnr_chain_gather: gather + geometry + positional encoding of the distances for the valid samples d_vs_item[0 .. n_valid)
 *   (n_valid = d_counts[HNR_CNT_SAMPLES_VALID], read on the device; cap_samples bounds it) into d_workspace
 *   (hnr_chain_workspace_bytes(cap_samples)); also d_X5[s, 256:280] = view-direction encoding (:909-913) and, optionally, the
 *   reference's `weight` / `conf_coefficient` outputs [R,SR,K] (written for valid neighbour slots only).
 * hnr_chain_plan: the list of valid samples the chain works on (the packing by `pnt_mask_flat` / `sampled_Rw2c` masks of
 *   models/aggregators/point_aggregators.py:924,935,961-970), d_vs_item[s] = ray * SR + slot, from the kept-sample work list of
 *   hnr_march_query.  classes = 0: in (ray, slot) order, exactly hnr_sample_plan's list.  classes = 1: the samples with more than four
 *   neighbours first, then those with 1..4 (each class in (ray, slot) order), and d_counts[HNR_CNT_SAMPLES_SMALL] = size of the second
 *   class: the gather and the chain kernel give a small sample 4 row slots instead of 8 (82 % of the bench frame's samples have 8
 *   neighbours, 11 % at most 4: 5.5 % fewer rows through the four dense layers; the sums are bit-identical, a slot without a neighbour
 *   contributes an exact zero).  classes = 2: three classes -- more than 4 neighbours (8 slots), 3..4 (4 slots,
 *   HNR_CNT_SAMPLES_SMALL), 1..2 (2 slots, HNR_CNT_SAMPLES_TINY; 7.5 % of the bench frame's samples): another 2 % fewer rows.
 *   Everything downstream is per sample and order-free.  hnr_chain_classes() = the largest `classes` the chain kernel selected in
 *   this process supports (0 for the older kernel variants).  d_scratch: int32[3 * ceil(max_items / 1024) + 3].
 * hnr_chain_forward: d_X5[s, 0:256] = sum_k w_k block3(...)_k, d_sigma[s] = sum_k w_k softplus(alpha_k - 1).
 *   d_point_table [N, ldt >= 256] = [emb | PE3(emb)] block1.0.weight[:, :224]^T.  d_dbg (probe, may be NULL): the post-activation
 *   output of layer dbg_layer (0..3) as [rows = 8 per valid sample, 256]. */
int64_t hnr_chain_packed_bytes(void);
int64_t hnr_chain_workspace_bytes(int cap_samples);
int hnr_chain_classes(void);
int hnr_chain_plan(const int32_t *d_work, const int32_t *d_sample_pidx, int64_t *d_counts, int K, int max_items, int classes,
                   int32_t *d_vs_item, int cap_samples, int32_t *d_scratch, void *stream);
int hnr_chain_pack(const float *d_w_b1_0_dist, int ldw0, const float *d_b_b1_0, const float *d_w_b1_2, const float *d_b_b1_2,
                   const float *d_w_b3_0, const float *d_b_b3_0, const float *d_w_b3_2, const float *d_b_b3_2,
                   const float *d_alpha_w, const float *d_alpha_b, void *d_packed, void *stream);
int hnr_chain_gather(const float *d_xyz, const float *d_conf, const float *d_dir, const float *d_color,
                     const int32_t *d_sample_pidx, const float *d_sample_loc_w, const float *d_raydir, const float *d_campos,
                     const float *d_camrot, const int32_t *d_vs_item, const int64_t *d_counts, int SR, int K, int cap_samples,
                     void *d_workspace, float *d_X5, int ld5, float *d_weight_out, float *d_conf_out, void *stream);
/* hnr_point_records: the four per-point buffers the gather reads (NeuralPoints' xyz / points_conf / points_dir / points_color, indexed by
 *   sample_pidx in models/neural_points/neural_points.py:709-720), interleaved once per cloud version into 48-byte records
 *   d_rec [N][12] f32 = {x y z conf | dir.x dir.y dir.z r | g b 0 0}; hnr_chain_gather_rec = hnr_chain_gather reading them (the same values,
 *   bit-identical outputs): one or two 64-byte sectors per neighbour instead of four scattered reads (6.0 -> 1.8 GB fetched per frame,
 *   profiles/r02_traffic.json). */
int hnr_point_records(const float *d_xyz, const float *d_conf, const float *d_dir, const float *d_color, int N, float *d_rec, void *stream);
int hnr_chain_gather_rec(const float *d_rec, const int32_t *d_sample_pidx, const float *d_sample_loc_w, const float *d_raydir,
                         const float *d_campos, const float *d_camrot, const int32_t *d_vs_item, const int64_t *d_counts, int SR, int K,
                         int cap_samples, void *d_workspace, float *d_X5, int ld5, float *d_weight_out, float *d_conf_out, void *stream);
/* Edited scenes: per-point rotations `neural_points.Rw2c` (models/neural_points/neural_points.py:720; run/editiing.py:196-209) as a PART TABLE:
 *   d_part_rot [n_parts][9] f32 row-major and one part index per point, Rw2c of point p = d_part_rot[part of p]; n_parts <= HNR_MAX_PARTS.  For a
 *   valid sample with neighbours p_0 .. p_7 on a ray of direction v (models/aggregators/point_aggregators.py:894-971):
 *     dists[k, 0:3] = R_{p_k} (xyz_{p_k} - sample_loc_w)   (columns 3..5, the weight and conf_coefficient are those of the un-rotated offset),
 *     v' = R_{p_0} v  (the point in SLOT 0, :897) feeds the view-direction encoding X5[s, 256:280] and every neighbour row's extras,
 *     dir'_k = R_{p_k} points_dir[p_k]; extras dir'_k - v', dir'_k . v'.
 *   y = R x is y_i = (R[i][0] x_0 + R[i][1] x_1) + R[i][2] x_2, every product and sum rounded on its own: the identity returns x bit for bit.
 *   Nothing else sees the rotation (colour extras, the per-point table, the image branch, ray_dist, the composite).
 * hnr_point_records_parts = hnr_point_records + the part index d_part[i] (int32, 0 .. n_parts - 1) as a float in the record's first spare slot
 *   (rec[i][10]); hnr_chain_gather_rec_parts reads it from there, hnr_chain_gather_parts from d_part [N].  n_parts = 0: no rotation, the call
 *   is hnr_chain_gather_rec / hnr_chain_gather.  A part index >= n_parts is the caller's error (not checked on the device). */
#define HNR_MAX_PARTS 65536
int hnr_point_records_parts(const float *d_xyz, const float *d_conf, const float *d_dir, const float *d_color, const int32_t *d_part, int N,
                            float *d_rec, void *stream);
int hnr_chain_gather_rec_parts(const float *d_rec, const float *d_part_rot, int n_parts, const int32_t *d_sample_pidx,
                               const float *d_sample_loc_w, const float *d_raydir, const float *d_campos, const float *d_camrot,
                               const int32_t *d_vs_item, const int64_t *d_counts, int SR, int K, int cap_samples, void *d_workspace,
                               float *d_X5, int ld5, float *d_weight_out, float *d_conf_out, void *stream);
int hnr_chain_gather_parts(const float *d_xyz, const float *d_conf, const float *d_dir, const float *d_color, const int32_t *d_part,
                           const float *d_part_rot, int n_parts, const int32_t *d_sample_pidx, const float *d_sample_loc_w,
                           const float *d_raydir, const float *d_campos, const float *d_camrot, const int32_t *d_vs_item,
                           const int64_t *d_counts, int SR, int K, int cap_samples, void *d_workspace, float *d_X5, int ld5,
                           float *d_weight_out, float *d_conf_out, void *stream);
int hnr_chain_forward(const void *d_workspace, const float *d_point_table, int ldt, const void *d_packed, const int64_t *d_counts,
                      int cap_samples, float slope, float *d_X5, int ld5, float *d_sigma, float *d_dbg, int dbg_layer, void *stream);

/* Three consecutive nn.Linear (+ LeakyReLU) layers of width <= 128 fused into one kernel (csrc/mlp.hip), fp32 in / fp32 out, the
 * same two-term fp16 split arithmetic as the chain above: the per-sample MLPs of viewmlp -- color_feature_branch (:1028-1037),
 * the first three layers of aux_merge_weight_block (:1199) and color_mixup_block (:1285-1292).
 *   hnr_mlp3_pack: d_W[l] [N[l], K[l]] (row stride ldw[l]), d_bias[l] [N[l]] or NULL; K[l] = N[l-1]; K[0] <= 288, N <= 128.
 *   hnr_mlp3_forward: d_C[m, 0:N[2]] = L2(L1(L0(d_A[m, 0:K[0]]) )), act[l] != 0 applies LeakyReLU(slope) after layer l; optional addend of
 *   layer 0 before its activation: d_R[d_ridx[m], 0:N[0]] (the colour-feature part of aux_merge_weight_block.0, shared by a sample's
 *   views).  Rows: M = min(M_cap, d_counts[count_index] * count_mult) when d_counts != NULL (device-side count), else M_cap.
 *   seg_stride > 0: the rows are count_mult SEGMENTS of d_counts[count_index] rows each, segment v starting at row v * seg_stride
 *   (the (view, sample) rows of hnr_proj_rows: row = v * cap_samples + s).
 *   n_layers = 4 adds a TAIL: a fourth layer reading layer 2's output, written to d_C2[m, 0:N[3]] (K[3] = N[2]) -- the colour-feature
 *   columns of aux_merge_weight_block.0 (128 -> 64, no activation) ride on the colour-feature launch.
 *   Built for the k-step tuples of these uses: K = (280,128,128[,128]), (48,64,64), (90,45,45). */
int64_t hnr_mlp3_packed_bytes(int n_layers, const int *K);
int hnr_mlp3_pack(int n_layers, const float *const *d_W, const int *ldw, const int *N, const int *K, const float *const *d_bias, void *d_packed,
                  void *stream);
int hnr_mlp3_forward(const float *d_A, int lda, int64_t M_cap, const int64_t *d_counts, int count_index, int count_mult, int seg_stride,
                     const void *d_packed, int n_layers, const int *N, const int *K, const int *act, float slope, const float *d_R,
                     const int32_t *d_ridx, int ldr, float *d_C, int ldc, float *d_C2, int ldc2, void *stream);

/* The merge stage of the image branch in ONE launch (V = 4): reprojection of every valid sample into the reference views + truncation +
 * feature gather + delta view directions (hnr_proj_rows: neural_points_volumetric_model.py:248-255, :296-310; point_aggregators.py:1077-1088),
 * aux_merge_weight_block on [imgfeat45 | colfeat128 | ddir3] (:1199; the colour-feature columns enter as the per-sample addend d_pre [S, 64],
 * bias included -- the tail output of the colour-feature launch), sigmoid, validity / frame weights, the weighted merge over the views
 * (:1217) and the mix-up row d_X7[s, 0:90] = [colfeat[:45] | merged45] (:1286-1292).  Replaces hnr_proj_rows + hnr_mlp3_forward + hnr_merge:
 * the [4 S, 48] rows, the [4 S, 64] activations and the per-row weights stay on chip.  d_mlp_mw: hnr_mlp3_pack image of the three layers
 * 48 -> 64 -> 64 -> 64 (first layer = the image-feature and direction columns, no bias). */
int hnr_merge_stage(const float *d_sample_loc_w, const int32_t *d_vs_item, const int64_t *d_counts, const float *d_w2c, const float *d_intrinsic,
                    const float *d_campos, const float *d_campos_nearest, const float *d_featmap, int V, int H, int W, const float *d_frame_w,
                    const float *d_pre, int ldpre, const void *d_mlp_mw, const float *d_w_last, const float *d_b_last, const float *d_CF, int ldcf,
                    int cap_samples, float slope, float *d_X7, int ld7, void *stream);

/* Mix-up stage in one launch: color_mixup_block (90 -> 45 -> 45 -> 45, :1285-1292; d_mlp_mx = its hnr_mlp_pack image), learn_residuals (:1294),
 * color_final_block + sigmoid*1.002-0.001 (:1295, :1334, :478-482), scattered with sigma into d_decoded [R*SR,4] (:1337-1338).  Equals
 * hnr_mlp3_forward + hnr_final_color bit for bit.  d_X7 [S, ld7 >= 92] (ld7 a multiple of 4, 16-B aligned), d_CF [S, ldcf >= 128];
 * d_Y (optional) receives the mix-up output rows [S, ldy >= 48]. */
int hnr_mixup_stage(const float *d_X7, int ld7, const void *d_mlp_mx, const float *d_CF, int ldcf, const float *d_w_fin, const float *d_b_fin,
                    const float *d_sigma, const int32_t *d_vs_item, const int64_t *d_counts, int cap_samples, float slope, float *d_Y, int ldy,
                    float *d_decoded, void *stream);

/* Residual + color_final_block + sigmoid*1.002-0.001 (:1294-1295, :1334, :478-482), scattered with sigma into
 * d_decoded [R*SR,4] (pre-zeroed by the caller; :1337-1338). */
int hnr_final_color(const float *d_Y, int ldy, const float *d_CF, int ldcf, const float *d_w_fin, const float *d_b_fin,
                    const float *d_sigma, const int32_t *d_vs_item, const int64_t *d_counts, int cap_samples,
                    float *d_decoded, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Stage 4: ray_dist (neural_points_volumetric_model.py:331-339) + ray_march with radiance render / alpha
 * blend (models/rendering/diff_ray_marching.py:508-557) + fill_invalid (:87-126), in input-ray order:
 *   d_raycolor [R,3] (bg colour where ray_mask = 0), d_opacity [R,SR], d_is_background [R] (T_end; 1 where
 *   ray_mask = 0), optional d_blend_weight [R,SR].
 * d_ray_nsamp: NULL when the query outputs are padded (pad_outputs = 1); else slots >= d_ray_nsamp[r] are taken as
 * the padding values (position 0, no neighbour) without being read. */
int hnr_composite(const float *d_decoded, const float *d_sample_loc_w, const int32_t *d_sample_pidx, const int8_t *d_ray_mask,
                  const int32_t *d_ray_nsamp,
                  const float *d_campos, const float *d_camrot, const float *d_bg_color, int R, int SR, int K, float vsize_z,
                  int raydist_mode_unit, float *d_raycolor, float *d_opacity, float *d_is_background, float *d_blend_weight,
                  void *stream);

/* Expected depth of every ray: the compute_depth branch of NeuralPointsRayMarching.forward (models/neural_points_volumetric_model.py:381-385),
 *   d_depth[r] = sum_s w_s z_s / (sum_s w_s + 1e-6),
 * w = d_blend_weight [R,SR] as hnr_composite / hnr_render_forward / hnr_render_train_forward write it (opacity x transmittance before the sample,
 * :382-383), z = the sample's camera-space depth (w2pers z of d_sample_loc_w [R,SR,3] with the composite's rounding: the quantity ray_dist is
 * built from, :331; the reference's `ray_ts`, which it never defines).  d_ray_nsamp: NULL for padded query outputs, else slots >= d_ray_nsamp[r]
 * are not read.  d_depth = 0 where d_ray_mask = 0.  The sums run in a fixed order: identical bits run to run.  d_campos [3], d_camrot [3,3] c2w. */
int hnr_ray_depth(const float *d_blend_weight, const float *d_sample_loc_w, const int32_t *d_ray_nsamp, const int8_t *d_ray_mask,
                  const float *d_campos, const float *d_camrot, int R, int SR, float *d_depth, void *stream);

/* Hole-probing outputs of opt.prob == 1 (models/neural_points_volumetric_model.py:392-416; consumed by the point-growing step
 * of run/train_ft.py:450-569): per ray the sample of maximum opacity -> d_max_opacity [R], its position d_max_loc_w [R,3],
 * the distance to the nearest of its K listed points d_far_dist [R] (empty slots read point 0, like the reference's clamped
 * gather), and sum_k (weight * conf_coefficient) x {color, dir, conf, embedding} of those points.  Rows = input rays. */
int hnr_probe_outputs(const float *d_opacity, const float *d_sample_loc_w, const int32_t *d_sample_pidx, const float *d_weight,
                      const float *d_conf_coefficient, const float *d_xyz, const float *d_emb, const float *d_conf, const float *d_dir,
                      const float *d_color, int F, int R, int SR, int K, float *d_max_opacity, float *d_max_loc_w, float *d_far_dist,
                      float *d_avg_color, float *d_avg_dir, float *d_avg_conf, float *d_avg_emb, void *stream);

/* ray_march alone (models/rendering/diff_ray_marching.py:508-557; radiance render + alpha blend) on existing tensors:
 * d_ray_dist [R,SR], d_ray_valid [R,SR] u8, d_features [R,SR,4] = (sigma, rgb), d_bg_color [3] or NULL ->
 * d_ray_color [R,3], d_opacity / d_acc_transmission / d_blend_weight [R,SR], d_bg_transmission [R]. */
int hnr_ray_march(const float *d_ray_dist, const uint8_t *d_ray_valid, const float *d_features, const float *d_bg_color, int R,
                  int SR, float *d_ray_color, float *d_opacity, float *d_acc_transmission, float *d_blend_weight,
                  float *d_bg_transmission, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Stage 5: backward of stages 3b and 4 (hnr_gather_aggregate_bwd / hnr_composite_bwd), one entry point per
 * forward kernel.  The reference obtains all of these from torch autograd over its eager ops; file:line below name the
 * forward code whose derivative each one is.  g_* / d_g* are gradients; weight gradients marked "atomics" are ADDED to
 * the caller's (zero-initialised or accumulating) buffers.
 */

/* ray_march + alpha blend (models/rendering/diff_ray_marching.py:508-557) and fill_invalid (:87-126):
 * d_g_raycolor [R,3] -> d_g_decoded [R,SR,4] = (d sigma, d rgb), zeros for invalid samples / rays.
 * With d_ray_nsamp given, the slots s >= nsamp[r] of d_decoded, d_sample_loc_w and d_sample_pidx are not read (hnr_composite's rule): they count as
 * decoded = 0, position 0, no neighbour, and the result is that of the padded call, bit for bit.  Holes inside nsamp (pidx < 0) ARE read:
 * their d_decoded must be finite, as the forward leaves it. */
int hnr_composite_bwd(const float *d_decoded, const float *d_sample_loc_w, const int32_t *d_sample_pidx, const int8_t *d_ray_mask,
                      const int32_t *d_ray_nsamp, const float *d_campos, const float *d_camrot, const float *d_bg_color,
                      int R, int SR, int K, float vsize_z, int raydist_mode_unit, const float *d_g_raycolor,
                      float *d_g_decoded, void *stream);
/* The same with the gradient of the expected depth (hnr_ray_depth; :381-385) added: d_g_depth [R] (may be NULL: then the result is
 * hnr_composite_bwd's, bit for bit).  dD/dw_s = (z_s - D) / (sum_s w_s + 1e-6), chained through w_s = opacity_s x transmittance_s. */
int hnr_composite_bwd_depth(const float *d_decoded, const float *d_sample_loc_w, const int32_t *d_sample_pidx, const int8_t *d_ray_mask,
                            const int32_t *d_ray_nsamp, const float *d_campos, const float *d_camrot, const float *d_bg_color,
                            int R, int SR, int K, float vsize_z, int raydist_mode_unit, const float *d_g_raycolor,
                            const float *d_g_depth, float *d_g_decoded, void *stream);

/* color_final_block + sigmoid*1.002-0.001 + residual (point_aggregators.py:1294-1295, :1334, :478-482):
 * d_g_decoded -> d_gY [S,45] (mix-up output), d_gCF [S,128] (OVERWRITTEN), d_g_sigma [S]; weights: atomics. */
int hnr_final_color_bwd(const float *d_Y, int ldy, const float *d_CF, int ldcf, const float *d_w_fin, const float *d_b_fin,
                        const int32_t *d_vs_item, const int64_t *d_counts, int cap_samples, const float *d_g_decoded,
                        float *d_gY, int ldgy, float *d_gCF, int ldgcf, float *d_g_sigma, float *d_g_w_fin, float *d_g_b_fin,
                        void *stream);

/* weighted merge + last layer of aux_merge_weight_block (:1199-1217, patch drop :1222-1237, mix-up input :1286-1292):
 * d_gX7 [S,90] -> d_gF [V*cap,48] (d image-feature columns), d_gZ3 [V*cap,64] (d pre-activation of the last hidden layer),
 * d_gCF[:, :45] += ; last-layer weights: atomics. */
int hnr_merge_bwd(const float *d_X6, int ld6, const float *d_Hm, int ldh, const float *d_w_last, const float *d_b_last,
                  const float *d_vmask, const float *d_frame_w, const int64_t *d_counts, int V, int cap_samples, float slope,
                  const uint8_t *d_ray_drop, const int32_t *d_vs_item, int SR, const float *d_gX7, int ldg7,
                  float *d_gF, int ldgf, float *d_gZ3, int ldgz, float *d_gCF, int ldgcf, float *d_g_w_last, float *d_g_b_last,
                  void *stream);

/* pixel gather (:1077-1089, :1193) + F.interpolate (:1064-1067) transposed: the rows' image-feature gradients (two sources
 * added: d_gFa from hnr_merge_bwd, optional d_gFb from the merge-weight MLP's first layer) are first added to their pixel
 * of d_g_featmap ([V,H,W,48], ZERO-INITIALISED; d_bbox int32[V,4] initialised to {W,H,-1,-1} receives the touched
 * rectangle; rows are added to their pixel with float atomics, row strides lda/ldb >= 48; d_key_scratch: 3 * V * cap_samples int32,
 * d_sort_scratch is no longer used), then gathered with the bilinear weights into the s1/s2/s3 slots of d_g_pyramid, a ZERO-INITIALISED buffer
 * laid out like the forward scratch of hnr_image_features. */
int hnr_proj_rows_bwd(const float *d_sample_loc_w, const int32_t *d_vs_item, const int64_t *d_counts, const float *d_w2c,
                      const float *d_intrinsic, int V, int H, int W, int cap_samples, const float *d_gFa, int lda,
                      const float *d_gFb, int ldb, float *d_g_featmap, int32_t *d_bbox, float *d_g_pyramid,
                      int32_t *d_key_scratch /* int32[3*V*cap_samples] */, void *d_sort_scratch,
                      int64_t sort_scratch_bytes /* hnr_sort_rows_scratch_bytes(V*cap_samples) */, void *stream);

/* Sum-by-key of gradient rows (torch autograd's index_add / scatter in the reference) without per-element atomics:
 *   hnr_sort_rows_by_key : stable radix sort of (key, row index); keys < 0 sort first and are skipped later;
 *   hnr_segment_sum_rows : d_dst[key * dst_stride + c] += sum over the rows with that key of (A[row,c] + B[row,c]),
 *                          c < n_cols (multiple of 4, <= 256; d_B may be NULL).
 * Used for d(per-point table) (rows -> touched point) and d(feature map) (rows -> pixel). */
int64_t hnr_sort_rows_scratch_bytes(int64_t M);
int hnr_sort_rows_by_key(const int32_t *d_keys, int64_t M, int32_t *d_keys_sorted, int32_t *d_perm, void *d_scratch,
                         int64_t scratch_bytes, void *stream);
int hnr_segment_sum_rows(const float *d_A, int lda, const float *d_B, int ldb, const int32_t *d_keys_sorted,
                         const int32_t *d_perm, int64_t M, int n_cols, float *d_dst, int64_t dst_stride, void *stream);

/* aux_block_s1..3 (:1047-1063): d_scratch is the forward scratch (activations), d_g_pyramid as above (used as workspace);
 * g_conv_w / g_conv_b: HOST arrays of 6 device pointers, atomics. */
int hnr_image_features_bwd(const float *d_img, int V, int H, int W, const float *const *conv_w, float slope,
                           const float *d_scratch, float *d_g_pyramid, float *const *g_conv_w, float *const *g_conv_b,
                           void *stream);
/* Test hook: the form the training step runs (csrc/render_train.hip).  d_bbox int32[V,4] = the per-view rectangle of touched pixels {min x, min y, max x,
 * max y} as hnr_proj_rows_bwd leaves it ({W, H, -1, -1}: view untouched); every convolution tile outside the rectangle's image at its level, dilated by
 * 30 / 14 / 6 cells at resolution divisor 2 / 4 / 8, is skipped.  d_g_pyramid MUST BE ZERO outside what hnr_proj_rows_bwd wrote: a skipped tile does
 * not write its share of the input gradients, and the tiles that run add to what is there.  Same results as hnr_image_features_bwd up to the order of
 * the atomic weight-gradient sums (tests/test_image_branch_gpu.py). */
int hnr_image_features_bwd_bbox(const float *d_img, int V, int H, int W, const float *const *conv_w, float slope,
                                const float *d_scratch, float *d_g_pyramid, float *const *g_conv_w, float *const *g_conv_b,
                                const int32_t *d_bbox, void *stream);

/* NeuralPoints gather (neural_points.py:709-720), block3 extras (:957-971), conf straight-through clamp (:1422-1424, :1508-1512) transposed:
 * d_gX3[:, 256:263], d_g_wagg, optional d_g_conf_out [R,SR,K] (gradient of the conf_coefficient output) -> per-row contributions
 * [d color 3 | d dir 3 | d conf | 0] in d_G8 [rows, 8]; hnr_segment_sum_rows_det over the rows sorted by touched-point index
 * (hnr_sort_rows_by_key) adds them per point in a fixed order: bit-identical gradients run to run, no float atomics. */
int hnr_gather_rows_bwd_rows(const int32_t *d_sample_pidx, const float *d_raydir, const int32_t *d_vs_item, const int32_t *d_vs_off,
                             const int32_t *d_vs_cnt, const int64_t *d_counts, int SR, int K, int cap_samples, const float *d_gX3,
                             int ldg3, const float *d_g_wagg, const float *d_weight, const float *d_g_conf_out, float *d_G8, void *stream);
/* dst[(dst_index ? dst_index[k] : k), 0:n_cols] (+)= sum of the rows A[perm[e], :] with keys_sorted[e] == k, for the DENSE keys k = 0 .. n_keys-1;
 * one wave per key, rows added in sorted (= original row) order, no atomics.  n_cols a multiple of 4, <= 256. */
int hnr_segment_sum_rows_det(const float *d_A, int lda, const int32_t *d_keys_sorted, const int32_t *d_perm, int64_t M, int n_cols,
                             int n_keys, const int32_t *d_dst_index, float *d_dst, int64_t dst_stride, int accumulate, void *stream);
/* The form the training step uses (torch autograd's index_add for the point-buffer gradients, models/neural_points/neural_points.py:709-720
 * transposed): the rows of key k are listed, in ANY order, in d_row_list[d_seg_start[k] .. + d_seg_count[k]) (a point-major list built without a
 * sort); dst[k, 0:n_cols] = their sum, added in an order that depends on the row indices only (one workgroup per key: row indices rank-sorted
 * in LDS, four partial sums over the sorted quarters added in wave order) -- bit-identical run to run, no float atomics.  Row indices of a
 * segment must be distinct.  Optional second matrix d_A2 (n_cols2 <= 256) summed into d_dst2 over the same segments; optional d_absmax:
 * max |dst| as a float bit pattern with atomicMax (exponent-exact: see csrc/hnr_common.h absmax_publish).  n_cols, n_cols2 multiples of 4. */
int hnr_segment_sum_rows_csr(const float *d_A, int lda, const int32_t *d_row_list, const int32_t *d_seg_start, const int32_t *d_seg_count,
                             int n_cols, int n_keys, float *d_dst, int64_t dst_stride, const float *d_A2, int lda2, int n_cols2,
                             float *d_dst2, int64_t dst_stride2, uint32_t *d_absmax, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Test hooks: the small kernels BETWEEN the heavy stages of hnr_render_train_backward, each alone with the grid the step gives it
 * (tests/test_backward_glue_gpu.py compares every one with float64).  "d_n / d_m / d_u" are device-side int64 counts, clamped to the
 * capacity argument (NULL where marked optional: the capacity is the count).  A capacity of 0 launches nothing.
 */
/* hnr_final_color_bwd, and *d_gY_max = max(*d_gY_max, max |d_gY[s < n_valid, 0:45]|) as a bit pattern (exponent-exact, csrc/hnr_common.h absmax_publish). */
int hnr_final_color_bwd_max(const float *d_Y, int ldy, const float *d_CF, int ldcf, const float *d_w_fin, const float *d_b_fin,
                            const int32_t *d_vs_item, const int64_t *d_counts, int cap_samples, const float *d_g_decoded,
                            float *d_gY, int ldgy, float *d_gCF, int ldgcf, float *d_g_sigma, float *d_g_w_fin, float *d_g_b_fin,
                            uint32_t *d_gY_max, void *stream);
/* hnr_merge_bwd, and *d_gZ3_max = max(*d_gZ3_max, max |d_gZ3[v * cap + s, 0:64]|, s < n_valid) as a bit pattern (exponent-exact, as above): the scale of
 * the fp16 GEMM that follows in the training step.  The other outputs are the bits of hnr_merge_bwd. */
int hnr_merge_bwd_max(const float *d_X6, int ld6, const float *d_Hm, int ldh, const float *d_w_last, const float *d_b_last,
                      const float *d_vmask, const float *d_frame_w, const int64_t *d_counts, int V, int cap_samples, float slope,
                      const uint8_t *d_ray_drop, const int32_t *d_vs_item, int SR, const float *d_gX7, int ldg7,
                      float *d_gF, int ldgf, float *d_gZ3, int ldgz, float *d_gCF, int ldgcf, float *d_g_w_last, float *d_g_b_last,
                      uint32_t *d_gZ3_max, void *stream);
/* Alpha branch + K-weighted sums transposed, 8 row slots per sample (row = 8 s + k, s < d_counts[HNR_CNT_SAMPLES_VALID] <= cap_samples).  d_aux: per 32-row group
 * 1280 bytes {int32 pid[32]; float w[32]; 1024 bytes unused here}.  Slot with pid >= 0, h = d_H4[row, 0:256]:  y = h . alpha_w + alpha_b - 1;
 * da = w g_sigma[s] sigmoid(y);  d_gZ4[row] = (w gX5[s] + da alpha_w) * (h > 0 ? 1 : slope);  d_g_wagg[row] = softplus(y) g_sigma[s] + h . gX5[s];
 * d_g_alpha_w += da h, d_g_alpha_b += da (atomics).  Empty slots: zeros.  *d_absmax = max(*d_absmax, max |d_gZ4|) (required). */
int hnr_ksum_bwd_rows8(const float *d_H4, const void *d_aux, const float *d_alpha_w, const float *d_alpha_b, const int64_t *d_counts,
                       const float *d_gX5, int ldg5, const float *d_g_sigma, float slope, int cap_samples, float *d_gZ4, float *d_g_wagg,
                       float *d_g_alpha_w, float *d_g_alpha_b, uint32_t *d_absmax, void *stream);
/* d_gX3[row, 256 + e] = sum_n d_dZ3[row, n] d_w30[n, 256 + e] for e < 7, d_gX3[row, 263] = 0, rows < *d_m <= rows_cap; d_dZ3 [rows,256], d_w30 [256,263],
 * d_gX3 [rows,264] (columns 0..255 untouched). */
int hnr_extras_dgrad(const float *d_dZ3, const float *d_w30, const int64_t *d_m, int64_t rows_cap, float *d_gX3, void *stream);
/* p = d_ulist[u], u < *d_u (optional) <= U_cap:  g_color[p] += P8[u, 0:3], g_dir[p] += P8[u, 3:6], g_conf[p] += P8[u, 6]. */
int hnr_point_small_grads(const float *d_P8, const int32_t *d_ulist, int U_cap, const int64_t *d_u, float *d_g_conf, float *d_g_dir, float *d_g_color,
                          void *stream);
/* hnr_point_rows transposed (F = 32), p = d_ids ? d_ids[u] : u, u < *d_n (optional) <= n_cap, E = the forward's row:
 * d_g_emb[p, d] += gE[u, d] + sum_{f<3} 2^f (E[u, c + 1] gE[u, c] - E[u, c] gE[u, c + 1]),  c = 32 + 2 (3 d + f)  (E[c] = sin, E[c + 1] = cos). */
int hnr_point_rows_bwd(const float *d_gE, int ldg, const float *d_E, int lde, const int32_t *d_ids, int n_cap, const int64_t *d_n, float *d_g_emb,
                       void *stream);
/* g[m, n] = (g[m, n] + (d_add && n < n_add ? add[m, n] : 0)) * (y[m, n] > 0 ? 1 : slope), m < *d_m (optional) <= M_cap, n < N; optional
 * *d_absmax = max(*d_absmax, max |g|).  N and the strides multiples of 4; lda >= n_add rounded up to 4. */
int hnr_dleaky_add(float *d_g, int ldg, const float *d_add, int lda, int n_add, const float *d_y, int ldy, int64_t M_cap, const int64_t *d_m, int N,
                   float slope, uint32_t *d_absmax, void *stream);
/* out[s, 0:N] = sum_{v < V} in[v cap + s, 0:N] (added in view order), s < *d_n (optional) <= cap; optional *d_absmax = max(*d_absmax, max |out|). */
int hnr_sum_views(const float *d_in, int ldi, int V, int cap, const int64_t *d_n, int N, float *d_out, int ldo, uint32_t *d_absmax, void *stream);
/* The touched points of the rows m < *d_m <= M_cap with d_row_pid[m] >= 0, without a sort: d_uidx[n_points] = compact index (ascending by point id) or -1;
 * d_ulist[u] = point id and d_seg_start[u] = first entry of its rows in d_row_list, for u < cap (d_seg_start[count] closes the list when count <= cap);
 * *d_count = number of touched points (may exceed cap); d_seg_count[u < cap] = rows of point u; d_row_u[m < M_cap] = compact index of the row's point,
 * `cap` for skipped rows; d_row_list: each point's rows, in any order within its segment.  d_scratch: hnr_unique_points_scratch_elems(n_points) int32. */
int64_t hnr_unique_points_scratch_elems(int n_points);
int hnr_unique_points(const int32_t *d_row_pid, int64_t M_cap, const int64_t *d_m, int n_points, int32_t *d_uidx, int32_t *d_ulist, int cap,
                      int32_t *d_row_u, int32_t *d_count, int32_t *d_scratch, int32_t *d_seg_start, int32_t *d_seg_count, int32_t *d_row_list,
                      void *stream);
/* d_g_conf[0] += sum of d_g_conf_out[i] over the i < n with d_sample_pidx[i] < 0, in a fixed order; d_scratch512: 512 floats. */
int hnr_conf0_grad(const float *d_g_conf_out, const int32_t *d_sample_pidx, int64_t n, float *d_scratch512, float *d_g_conf, void *stream);
/* d_gw0[n, k < 45 ? k : k + 128] = d_g[n, k], n < 64, k < 48: d_g [64,48] -> columns 0..44 and 173..175 of d_gw0 [64,176]. */
int hnr_w0fd_grad(const float *d_g, float *d_gw0, void *stream);
/* d_out[r] = mask[r] > 0 && (d_explicit_flags ? d_explicit_flags[r] : d_lut && d_lut[number of r' < r with mask[r'] > 0]), r < R (one workgroup). */
int hnr_ray_drop_flags(const int8_t *d_ray_mask, int R, const uint8_t *d_lut, const uint8_t *d_explicit_flags, uint8_t *d_out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Dense layers of the TRAINING step on the 16-bit matrix pipe (csrc/h2gemm.hip), fp32 in / fp32 out, the chain's two-term fp16 split
 * arithmetic.  They replace what torch autograd runs for the nn.Linear (+ LeakyReLU) layers of PointAggregator.viewmlp in the reference's
 * train step (models/aggregators/point_aggregators.py:948, :972, :1037, :1199, :1292; loss.backward() at
 * models/mvs_points_volumetric_model.py:111-131).  Every row count is read on the DEVICE: rows = min(M_cap, *d_m) (d_m may be NULL).
 * n_seg > 1: the rows are n_seg SEGMENTS of min(*d_m, seg_stride) rows each, segment v starting at physical row v * seg_stride -- the
 * (view, sample) rows of hnr_proj_rows (row = v * cap_samples + s); n_seg = 1: plain rows.
 *   hnr_h2lin_pack   n_jobs <= 16 weight matrices -> kernel images, two launches for all of them.  Element (n, k) of job j is
 *                    d_W[j][n * rs[j] + k * cs[j]]: (rs, cs) = (ld, 1) packs an nn.Linear weight [N, K], (1, ld) its transpose (input
 *                    gradients: dX = dZ W is the layer "dZ (W^T)^T").  N <= 256, K <= 288; image bytes: hnr_h2lin_packed_bytes(K).
 *   hnr_h2lin        mode 0: C = act(A W^T + bias)  (act != 0: LeakyReLU(slope));
 *                    mode 1: C = (A W^T) * (side > 0 ? 1 : slope)   -- side [M, ld_side] is the stored forward activation: the input
 *                    gradient through a LeakyReLU.  K in {<= 48, <= 64, <= 128, <= 224, <= 256}.  d_absmax (optional): max |C| is
 *                    atomically max-ed into it as a bit pattern (the scale of a later hnr_h2wgrad).
 *   hnr_h2lin_dgrad_bits   mode 1 of hnr_h2lin for the per-neighbour chain (N = 256, whole 32-row tiles: M_cap % 32 == 0): LeakyReLU' comes from the
 *                    SIGN WORDS the training forward leaves (one word per (32-row tile, wave = 64-column group, lane): bit 31 - i = (value i of
 *                    the lane's 32 columns 64 wave + 16 (lane >> 5) + {0..15, 32..47} of row (lane & 31) is > 0)) instead of the stored
 *                    activation.  K = 256 runs the weight-stationary kernel (csrc/h2lin_ws.hip); results equal hnr_h2lin's bit for bit.
 *   hnr_h2wgrad      dW[N, K] (row stride lddw) = dZ[M, N]^T X[M, K], db[N] = column sums of dZ (d_db may be NULL); accumulate != 0 adds.
 *                    d_absmax_z / d_absmax_x: bit patterns of (an upper bound of) max |dZ|, max |X| (hnr_absmax or a producer's output).
 *                    N <= 256, K <= 287.  Deterministic (fixed-order partials, no atomics); d_scratch: hnr_h2wgrad_scratch_bytes(N, K).
 *   hnr_absmax       *d_out = max(*d_out, max |A[0:M, 0:N]|) as a bit pattern. */
int64_t hnr_h2lin_packed_bytes(int K);
int hnr_h2lin_pack(int n_jobs, const float *const *d_W, const int64_t *rs, const int64_t *cs, const int *N, const int *K,
                   const float *const *d_bias /*may be NULL*/, void *const *d_packed, void *stream);
int hnr_h2lin(const float *d_A, int lda, int64_t M_cap, const int64_t *d_m, int n_seg, int64_t seg_stride, const void *d_packed, int N, int K, int mode,
              int act, float slope, const float *d_side, int ld_side, float *d_C, int ldc, uint32_t *d_absmax, void *stream);
int hnr_h2lin_dgrad_bits(const float *d_dZ, int ldz, int64_t M_cap, const int64_t *d_m, const void *d_packed, int N, int K, float slope,
                         const uint32_t *d_side_bits, float *d_C, int ldc, uint32_t *d_absmax, void *stream);
int64_t hnr_h2wgrad_scratch_bytes(int N, int K);
int hnr_h2wgrad(const float *d_dZ, int ldz, const float *d_X, int ldx, int64_t M_cap, const int64_t *d_m, int n_seg, int64_t seg_stride, int N, int K,
                const uint32_t *d_absmax_z, const uint32_t *d_absmax_x, float *d_dW, int lddw, float *d_db, int accumulate,
                void *d_scratch, void *stream);
int hnr_absmax(const float *d_A, int lda, int64_t M_cap, const int64_t *d_m, int n_seg, int64_t seg_stride, int N, uint32_t *d_out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * The whole forward path in ONE call (csrc/render_forward.hip): one pass of NeuralPointsRayMarching.forward + fill_invalid
 * (models/neural_points_volumetric_model.py:257-391, :87-126) over R rays -- query, gather / aggregate (fused chain + fused
 * per-sample MLPs), composite -- with every launch issued here, back to back on the caller's stream.  The reference's three host
 * synchronisations per chunk (query_point_indices_worldcoords.py:645-646, :705; point_aggregators.py:1092) have no counterpart:
 * the kernels read their work sizes from the query's device counters, the intermediate buffers live in the caller's workspace
 * (hnr_render_workspace_bytes) sized for `cap_samples` valid shading samples (R*SR is always enough), and d_status[0] becomes 1 when
 * that capacity was exceeded (the extra samples are dropped; d_status[1] holds the true count's low 32 bits).  K = 8 only.
 * All pointers are device pointers; nothing is allocated, nothing is read back. */
typedef struct {
    int   R, SR, K, D;            /* rays, opt.SR, opt.K (8), opt.z_depth_dim                                          */
    int   tmid_stride;            /* 0: cam->d_tmid is one [D] table; D: [R,D] per-ray tables (train-time jitter)       */
    int   kernel_size[3];
    float radius2;                /* radius_limit^2                                                                    */
    float vsize_z;                /* opt.vsize[2] (ray_dist rule, :331-339)                                            */
    int   raydist_mode_unit;
    int   V;                      /* reference views (0: use_nearest = 0, image branch off)                            */
    int   cap_samples;            /* capacity of the workspace in valid shading samples                                */
    int   knn_order;              /* hnr_query_params.knn_order                                                        */
} hnr_render_params;
typedef struct {
    const float *d_xyz, *d_conf, *d_dir, *d_color;      /* [N,3] [N] [N,3] [N,3]                                       */
    const float *d_point_table; int ldt;                /* [N, ldt >= 256] per-point addend of block1.0                 */
    const float *d_rec;                                 /* optional hnr_point_records image of the four buffers above ([N,12]); NULL: the
                                                           gather reads the four buffers                                */
    /* per-point rotations of an edited scene (hnr_chain_gather_parts); all zero: none                                   */
    const int32_t *d_part;                              /* [N] part index of every point: read when d_rec is NULL, or when rec_parts = 0  */
    const float *d_part_rot;                            /* [n_parts, 9]                                                  */
    int n_parts;                                        /* 0 .. HNR_MAX_PARTS                                            */
    int rec_parts;                                      /* != 0: d_rec was written by hnr_point_records_parts (it holds the part indices) */
} hnr_render_cloud;
typedef struct {
    const void  *d_chain;                               /* hnr_chain_pack                                               */
    const void  *d_mlp_cf, *d_mlp_mw, *d_mlp_mx;        /* hnr_mlp3_pack images: colour feature (4 layers: + the 128 -> 64 colour-feature
                                                           columns of aux_merge_weight_block.0 with its bias), merge weights, mix-up */
    const float *d_mw_last_w, *d_mw_last_b;             /* aux_merge_weight_block.6: [64], [1]                           */
    const float *d_fin_w, *d_fin_b;                     /* color_final_block.0: [3,128], [3]                             */
    float slope;                                        /* LeakyReLU slope                                               */
} hnr_render_weights;
typedef struct { const float *d_campos, *d_camrot, *d_raydir, *d_tmid, *d_bg_color; } hnr_render_camera;
typedef struct {
    const float *d_w2c, *d_intrinsic, *d_campos_nearest; /* [V,4,4] inverse(c2w_nearest), [3,3], [V,3]                  */
    const float *d_featmap; int H, W;                    /* hnr_image_features output [V,H,W,48]                         */
    const float *d_frame_w;                              /* optional [V]                                                 */
    void        *featmap_ready;                          /* optional hipEvent_t: the launch stream waits for it before the first kernel that
                                                            reads d_featmap (the merge stage), so the caller may build the feature map on
                                                            another stream while the query and the per-neighbour chain run            */
} hnr_render_views;
typedef struct {
    float   *d_raycolor, *d_opacity, *d_is_background;   /* [R,3] [R,SR] [R]  (fill_invalid applied)                     */
    float   *d_blend_weight;                             /* optional [R,SR]                                              */
    int8_t  *d_ray_mask;                                 /* [R]                                                          */
    float   *d_decoded;                                  /* [R,SR,4] (sigma, rgb)                                        */
    int32_t *d_sample_pidx; float *d_sample_loc_w; int32_t *d_ray_nsamp;    /* the query outputs, un-padded               */
    int64_t *d_counts;                                   /* [HNR_NCOUNTS]                                                */
    int32_t *d_status;                                   /* [2]                                                          */
    float   *d_weight, *d_conf_coefficient;              /* optional [R,SR,K] (both or neither)                          */
    void   **stage_events;                               /* optional: HNR_RENDER_NSTAGES + 1 hipEvent_t handles recorded at the
                                                            stage boundaries (query, plan, chain_gather, chain, mlp_colorfeat,
                                                            proj_rows, mlp_merge, merge, mlp_mixup, final_color, composite) */
} hnr_render_outputs;
#define HNR_RENDER_NSTAGES 11
int64_t hnr_render_workspace_bytes(const hnr_render_params *p);
int hnr_render_forward(const hnr_grid *grid, const hnr_render_params *p, const hnr_render_cloud *cloud, const hnr_render_weights *weights,
                       const hnr_render_camera *camera, const hnr_render_views *views, void *d_workspace, int64_t workspace_bytes,
                       const hnr_render_outputs *out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * The TRAINING step of the path as two calls (csrc/render_train.hip): hnr_render_train_forward = one pass of NeuralPointsRayMarching.forward in
 * train mode + fill_invalid (models/neural_points_volumetric_model.py:257-427, :87-126: jittered depths through cam->d_tmid with
 * tmid_stride = D, query_point_indices_worldcoords.py:87; patch drop point_aggregators.py:1222-1237; straight-through conf clamp :1422-1424),
 * keeping in the caller's workspace what the backward pass needs; hnr_render_train_backward = what loss.backward() makes torch autograd compute
 * for it (models/mvs_points_volumetric_model.py:111-131; there is no custom autograd.Function in the reference): the gradients of
 * points_embeding / points_conf / points_dir / points_color and of every aggregator parameter of the order-2 hybrid path, from the gradients of
 * coarse_raycolor [R,3] and (optionally) conf_coefficient [R,SR,K].  Every launch is issued by the library on the caller's stream; every work
 * size (valid samples, neighbour rows, touched points) is read from device counters; nothing is allocated, nothing is read back.
 * K = 8, point_features_dim = 32.  The weights are the raw nn.Linear / nn.Conv2d tensors under the reference's names (their kernel images are
 * re-packed every step -- all of them, the backward call's transposed images included, by the FORWARD call: hnr_render_train_backward needs the
 * forward call of the same step, with the same weights and workspace, to have run, as it does for the stored activations).  Weight gradients are OVERWRITTEN, point gradients too ([N,32] [N] [N,3] [N,3], zero
 * outside the batch's points).  Per-point sums are formed in a fixed order: bit-identical gradients run to run.
 *   d_drop_lut [R] u8 (optional): patch-drop pattern indexed by VALID-ray row (drop_patch_rays, point_aggregators.py:14-23, :1225-1233);
 *   d_ray_drop [R] u8 (optional, wins): explicit per-ray flags (a rank's slice of a batch-wide pattern); both are ANDed with ray_mask.
 * `out` as for hnr_render_forward (padded query outputs; d_blend_weight, d_weight, d_conf_coefficient required; stage_events: optional HIP events recorded at the stage boundaries, as in hnr_render_forward -- bench.py reads them);
 * d_status[0] = 1 when cap_samples was exceeded (R * SR always suffices). */
typedef struct {
    int   R, SR, K, D;
    int   tmid_stride;
    int   kernel_size[3];
    float radius2, vsize_z;
    int   raydist_mode_unit;
    int   V, H, W;                /* reference views and their size (V = 0: use_nearest = 0, image branch off)             */
    int   n_points;               /* N                                                                                    */
    int   cap_samples;
    int   knn_order;
    float slope;                  /* LeakyReLU slope                                                                      */
} hnr_train_params;
typedef struct { const float *d_xyz, *d_emb, *d_conf, *d_dir, *d_color; } hnr_train_cloud;          /* [N,3] [N,32] [N] [N,3] [N,3] */
typedef struct { float *d_emb, *d_conf, *d_dir, *d_color; } hnr_train_cloud_grads;
typedef struct {   /* aggregator.{block1.0, block1.2, block3.0, block3.2, alpha_branch.0, color_feature_branch.{0,2,4}, aux_merge_weight_block.{0,2,4,6},
                      color_mixup_block.{0,2,4}, color_final_block.0, aux_block_s1.{0,2}, s2.{0,2}, s3.{0,2}} .weight / .bias (device pointers) */
    const float *block1_0_w, *block1_0_b, *block1_2_w, *block1_2_b, *block3_0_w, *block3_0_b, *block3_2_w, *block3_2_b, *alpha_w, *alpha_b;
    const float *cf_w[3], *cf_b[3], *mw_w[4], *mw_b[4], *mx_w[3], *mx_b[3], *fin_w, *fin_b, *conv_w[6], *conv_b[6];
} hnr_train_weights;           /* the gradient block handed to hnr_render_train_backward has the same layout (its buffers are written)      */
typedef struct { const float *d_w2c, *d_intrinsic, *d_campos_nearest, *d_images /*[V,H,W,3]*/, *d_frame_w /*optional [V]*/; } hnr_train_views;
int64_t hnr_render_train_workspace_bytes(const hnr_train_params *p);
/* STAGE tier (tools only): byte offset / size pairs of the forward pass's intermediate tensors inside the workspace, in the order
 * Xd H1 X3 H3 H4 E Tu X5 sigma T1 T2 CF X6 vmask M1 M2 M3 X7 Y1 Y2 Y3 fm row_pid vs_item fm_scratch (out[2 i], out[2 i + 1]); returns the number of entries or -1.
 * The training-mode counterpart of reading PointAggregator.viewmlp's locals in a debugger (point_aggregators.py:892-1338). */
int hnr_render_train_debug_layout(const hnr_train_params *p, int64_t *out, int max_entries);
/* After hnr_render_train_forward: the batch's touched points inside the workspace -- *d_ids = ascending point ids [*capacity], *d_count = their number
 * (one int64 on the device, already clamped to the capacity).  The reference has no counterpart (autograd's index_select backward writes dense
 * [N, C] gradients, neural_points.py:712-720); a rank's gradient exchange (parallel.PointGradExchange) and a sparse optimiser step read it instead of
 * torch.unique(sample_pidx).  Host pointers only: nothing is launched. */
int hnr_render_train_touched(const hnr_train_params *p, void *d_workspace, int64_t workspace_bytes, const int32_t **d_ids, const int64_t **d_count,
                             int64_t *capacity);
int hnr_render_train_forward(const hnr_grid *grid, const hnr_train_params *p, const hnr_train_cloud *cloud, const hnr_train_weights *weights,
                             const hnr_render_camera *camera, const hnr_train_views *views, const uint8_t *d_drop_lut, const uint8_t *d_ray_drop,
                             void *d_workspace, int64_t workspace_bytes, const hnr_render_outputs *out, void *stream);
int hnr_render_train_backward(const hnr_train_params *p, const hnr_train_cloud *cloud, const hnr_train_weights *weights, const hnr_render_camera *camera,
                              const hnr_train_views *views, void *d_workspace, int64_t workspace_bytes, const hnr_render_outputs *forward_out,
                              const float *d_g_raycolor, const float *d_g_conf_coefficient /*may be NULL*/, const hnr_train_cloud_grads *cloud_grads,
                              const hnr_train_weights *weight_grads, void *stream);
/* ... with the gradient of the expected depth, d_g_depth [R] (may be NULL: hnr_render_train_backward), as a third upstream gradient: the depth a
 * caller forms with hnr_ray_depth from forward_out->d_blend_weight / d_sample_loc_w (the compute_depth branch, neural_points_volumetric_model.py:381-385,
 * supervised by compute_losses' depth term, models/base_rendering_model.py:1209-1215). */
int hnr_render_train_backward_depth(const hnr_train_params *p, const hnr_train_cloud *cloud, const hnr_train_weights *weights, const hnr_render_camera *camera,
                                    const hnr_train_views *views, void *d_workspace, int64_t workspace_bytes, const hnr_render_outputs *forward_out,
                                    const float *d_g_raycolor, const float *d_g_conf_coefficient /*may be NULL*/, const float *d_g_depth /*[R] or NULL*/,
                                    const hnr_train_cloud_grads *cloud_grads, const hnr_train_weights *weight_grads, void *stream);

/* ------------------------------------------------------------------------------------------------
 * "Next" row: hole probing, run/train_ft.py:527-549 (`probe_hole`) + :571-581 (`bloat_inds`).  Per probed frame: a cast
 * ray that found no neighbour although its ground-truth pixel is not background (|gt - bg| > 0.002) marks a hole; every hit ray
 * whose max-opacity sample exceeds opacity_thresh and that lies in the 3x3 neighbourhood of a hole -- or, when far_thresh > 0, whose
 * nearest neighbour is farther than far_thresh while its colour is within 0.1 of the ground truth -- becomes a new point.
 * d_sel [h*w] receives ray id + 1 at the selected pixels (0 elsewhere); the caller compacts it in row-major order.
 * d_pixel_idx [R,2] (x, y) as floats, d_ray_mask [R] float, bg3_host: 3 HOST floats, d_miss_scratch int32[h*w]. */
int hnr_probe_select(const float *d_pixel_idx, const float *d_ray_mask, const float *d_gt, const float *d_raycolor, const float *bg3_host,
                     const float *d_far_dist, const float *d_opacity, int R, int h, int w, float far_thresh, float opacity_thresh,
                     int32_t *d_miss_scratch, int32_t *d_sel, void *stream);

/* ------------------------------------------------------------------------------------------------
 * "Next" row: blur-handling module with pre-defined kernels, models/base_rendering_model.py:677-745
 * (`blur_update_output`, called at mvs_points_volumetric_model.py:145-146).  d_color / d_gt / d_out: [S*S,3] with
 * S = patch_num * patch_size in the dilated-patch ray layout; d_kernels [n_kernels, ks, ks]; per patch the candidate
 * (n_kernels blurred versions, normalised at the borders, + the un-blurred patch as candidate n_kernels) closest in L1 to
 * the ground truth replaces the patch; d_select [patch_num^2] records the choice for the backward.
 * patch_num < 0: the buffers hold -patch_num whole patches packed patch-major (patch, y, x) -- a rank's share of a batch
 * that is sharded over GPUs by whole patches (parallel.shard_patches); d_select then has -patch_num entries. */
int hnr_blur_select(const float *d_color, const float *d_gt, const float *d_kernels, int n_kernels, int kernel_size,
                    int patch_num, int patch_size, float *d_out, int32_t *d_select, void *stream);
int hnr_blur_select_bwd(const float *d_g_out, const float *d_kernels, const int32_t *d_select, int n_kernels, int kernel_size,
                        int patch_num, int patch_size, float *d_g_in, void *stream);

/* "Next" row, learnable blur kernels: models/base_rendering_model.py:827-1020 (`learnable_blur_update_output`,
 * faster_version; called at mvs_points_volumetric_model.py:143-144 when the aggregator returns a blur predictor).
 *   hnr_blur_gray_patches      d_gray [n_patches, 2, ps, ps]: channel 0 = grey ground-truth patch, 1 = grey rendered patch (:886-893),
 *                              the predictor's input; _bwd returns the gradient w.r.t. the rendered colours.
 *   hnr_blur_apply             every patch convolved with ITS kernel d_kernels[patch] (grouped F.conv2d, zero padding ks/2) under
 *                              opt.boundary_mode 0 / 1 / 2 (:915-923); _bwd gives the gradients w.r.t. the colours and the kernels.
 * Ray layout and the patch_num < 0 (patch-major) convention as for hnr_blur_select.  kernel_size odd, <= 15; patch_size <= 16. */
int hnr_blur_gray_patches(const float *d_color, const float *d_gt, int patch_num, int patch_size, float *d_gray, void *stream);
int hnr_blur_gray_patches_bwd(const float *d_g_gray, int patch_num, int patch_size, float *d_g_color, void *stream);
int hnr_blur_apply(const float *d_color, const float *d_kernels, int kernel_size, int patch_num, int patch_size, int boundary_mode,
                   float *d_out, void *stream);
int hnr_blur_apply_bwd(const float *d_g_out, const float *d_color, const float *d_kernels, int kernel_size, int patch_num, int patch_size,
                       int boundary_mode, float *d_g_color, float *d_g_kernels, void *stream);

/* The whole learnable blur module as three launches, for the training step without an autograd graph (train.train_step(learnable_blur=...)):
 * grey patches -> predictor Linear(2 ps^2, 128) LeakyReLU Linear(128, 128) LeakyReLU Linear(128, 128) LeakyReLU Linear(128, ks^2 + e) Sigmoid
 * (point_aggregators.py:1339-1344 without the conv block; e = 1 for kernel_mode 4, 0 for kernel_mode 0) -> normalisation (kernel_norm 0: divide by the
 * sum, 1: softmax, :895-899) -> kernel_mode 4: blend with the identity kernel by the last output and renormalise (:904-909) -> every patch convolved
 * with its kernel under boundary_mode 0 / 1 / 2 (:915-923).  All fp32, plain FMAs in a fixed order, no atomics: two runs give the same bits.
 *   hnr_blur_learn_weights   w[l] [out_l, in_l] row-major and b[l] [out_l] of Linear l = 0..3, nn.Linear's own layout, read through the
 *                            parameters' own pointers (no packed copy: an optimiser that updates in place needs no notification).  The gradient
 *                            block has the same layout and is written, not accumulated.
 *   hnr_blur_learn_forward   one launch.  d_color / d_gt / d_out [rays, 3], ray layout and the patch_num < 0 (patch-major) convention as for
 *                            hnr_blur_select.  d_ws (hnr_blur_learn_workspace_bytes, 16-byte aligned) receives what the backward reads: the grey
 *                            patches, the three hidden activations, the prediction and the final kernels.  d_kernels [n_patches, ks, ks]: optional
 *                            copy of the final kernels (NULL: none).
 *   hnr_blur_learn_backward  two launches.  (a) per patch: d_g_out [rays, 3] through the convolution (gradients w.r.t. the colours and the
 *                            kernel; boundary_mode 2 sends none through the mask term), the kernel gradient through the renormalisation, the
 *                            blend, the normalisation, the sigmoid and the four layers (LeakyReLU's derivative from the sign of its stored output)
 *                            down to the grey rendered patch; d_g_color [rays, 3] = convolution path + grey-patch path; every layer's delta rows
 *                            go to the workspace.  (b) dW_l[o][i] = sum_p delta_l[p][o] a_(l-1)[p][i], db_l[o] = sum_p delta_l[p][o], p ascending,
 *                            one fp32 FMA chain per element.  d_color and the workspace must be what the forward call saw / left.
 * slope: LeakyReLU's negative slope.  kernel_size odd, <= 15; patch_size <= 16.  Not covered: the conv-block predictor
 * (learnable_blur_kernel_conv), which stays with hnr_blur_gray_patches / hnr_blur_apply and torch in between. */
typedef struct {
    int patch_num, patch_size, kernel_size, kernel_mode, kernel_norm, boundary_mode;
    float slope;
} hnr_blur_learn_params;
typedef struct {
    float *w[4];
    float *b[4];
} hnr_blur_learn_weights;
int64_t hnr_blur_learn_workspace_bytes(int n_patches, int patch_size, int kernel_size, int kernel_mode);
int hnr_blur_learn_forward(const hnr_blur_learn_params *prm, const hnr_blur_learn_weights *weights, const float *d_color, const float *d_gt,
                           void *d_ws, int64_t ws_bytes, float *d_out, float *d_kernels, void *stream);
int hnr_blur_learn_backward(const hnr_blur_learn_params *prm, const hnr_blur_learn_weights *weights, const float *d_color, const float *d_g_out,
                            void *d_ws, int64_t ws_bytes, float *d_g_color, const hnr_blur_learn_weights *grads, void *stream);

/* ------------------------------------------------------------------------------------------------
 * "Next" row (second half): the loss terms of the shipped training configurations, value + gradients.
 * BaseRenderingModel.compute_losses, models/base_rendering_model.py: colour item `ray_masked_coarse_raycolor` (:1113-1118:
 * MSE over the rays with ray_mask > 0, 0 when none; `+ 1e-6` per item :1198; `* frame_weight` :1204-1205) and the zero-one
 * regulariser on conf_coefficient (:1228-1240: mean(log v + log(1 - v)), v = clamp(x, eps, 1 - eps)).
 *   d_out4 = {total, colour MSE, zero-one mean, number of valid rays};  total = (mse * w_color + 1e-6) * frame_weight + zo * w_zero_one
 *   d_g_color [R,3], d_g_conf [n_conf]: d total / d input (both NULL = value only).  d_scratch: hnr_shipped_loss_scratch_bytes(). */
int64_t hnr_shipped_loss_scratch_bytes(void);
int hnr_shipped_loss(const float *d_color, const float *d_gt, const int8_t *d_ray_mask, int R, const float *d_conf, int64_t n_conf,
                     float zero_epsilon, float w_color, float w_zero_one, float frame_weight, float *d_out4, float *d_g_color,
                     float *d_g_conf, void *d_scratch, void *stream);
/* The same with d_conf [R, conf_per_ray] holding a row per ray of the batch (the layout hnr_render_train_forward writes): only the rows of rays with
 * ray_mask > 0 enter the mean (and receive a gradient) -- the reference's conf_coefficient holds the R' valid rays only
 * (PointAggregator.forward's return, models/aggregators/point_aggregators.py:1519-1522) -- without a masked copy or a host read of the number of valid rays. */
int hnr_shipped_loss_rows(const float *d_color, const float *d_gt, const int8_t *d_ray_mask, int R, const float *d_conf, int conf_per_ray,
                          float zero_epsilon, float w_color, float w_zero_one, float frame_weight, float *d_out4, float *d_g_color,
                          float *d_g_conf, void *d_scratch, void *stream);
/* ... with the item's frame weight (:1204-1205) read from the device, d_frame_weight[0]: a training step captured in a hipGraph (train.CapturedTrainStep)
 * is replayed for dataset items with different weights. */
int hnr_shipped_loss_rows_fw(const float *d_color, const float *d_gt, const int8_t *d_ray_mask, int R, const float *d_conf, int conf_per_ray,
                             float zero_epsilon, float w_color, float w_zero_one, const float *d_frame_weight, float *d_out4, float *d_g_color,
                             float *d_g_conf, void *d_scratch, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Evaluation of a rendered frame: what the reference's test pass reports per frame, as one fp64 row on the device.
 * Replaces the two test losses of run/test_ft.py:233-243, the 8-bit quantisation of utils/visualizer.py:23-24 (the bytes of the PNGs it
 * writes) and run/evaluate.py:34-97 on those bytes (compare_psnr, structural_similarity, sqrt(mean_squared_error)).
 *   d_image, d_gt_full [h,w,3]: the rendered image and the ground truth scattered the same way (zero where no ray was cast: both count);
 *   d_raycolor, d_gt_rays [R,3], d_ray_mask [R]: the cast rays, for the masked loss (R = 0: all three may be NULL).
 *   A = q(image), B = q(gt_full), q(x) = (uint8) trunc(min(max(x, 0), 1) * 255.0f) in fp32 = (np.clip(x, 0, 1) * 255).astype(np.uint8);
 *   d_img8 / d_gt8 (optional, both or neither) [h,w,3] uint8 receive A and B.
 * d_row[HNR_FM_NCOLS] (fp64; the integers are exact):
 *   HNR_FM_SQERR8     S = sum (A - B)^2 over the n = 3hw values      -> mse8 = S / (65025 n), psnr = 10 log10(1 / mse8), rmse = sqrt(mse8)
 *   HNR_FM_N8         n
 *   HNR_FM_SSIM       structural_similarity(B / 255, A / 255, win_size = win, multichannel): per channel the mean over the (h - win + 1)(w - win + 1)
 *                     windows that lie inside the image of (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)) with the window means
 *                     ux, uy, uxx, uyy, uxy of x = A / 255, y = B / 255, sample covariances vx = NP / (NP - 1) (uxx - ux^2) ..., NP = win^2,
 *                     C1 = (0.01 L)^2, C2 = (0.03 L)^2, L = data_range; then the mean of the three channels.  Window sums exact (integers), the rest
 *                     fp64.  data_range = 2: the value the reference publishes (it hands float images to scikit-image without a data_range, and
 *                     scikit-image then takes the dtype range of floats, -1..1); data_range = 1: the textbook value for images in [0, 1].
 *   HNR_FM_MSE_FULL   mean over 3hw of (image - gt_full)^2, squares in fp32, sum in fp64      (test_ft.py:233-236; psnr = -10 log10)
 *   HNR_FM_MSE_MASKED mean over the rays with ray_mask > 0 of (raycolor - gt_rays)^2, NaN when there is none     (test_ft.py:238-243)
 *   HNR_FM_N_MASKED   number of rays with ray_mask > 0
 * win: odd, 3 <= win <= min(h, w, 31).  Deterministic (no atomics): the same inputs give the same bits.  Stream-ordered, nothing is read back.
 * d_scratch: hnr_frame_metrics_scratch_bytes(h, w, win) bytes (negative: bad shape), private to the call until it has run. */
#define HNR_FM_SQERR8      0
#define HNR_FM_N8          1
#define HNR_FM_SSIM        2
#define HNR_FM_MSE_FULL    3
#define HNR_FM_MSE_MASKED  4
#define HNR_FM_N_MASKED    5
#define HNR_FM_NCOLS       6
int64_t hnr_frame_metrics_scratch_bytes(int h, int w, int win);
int hnr_frame_metrics(const float *d_image, const float *d_gt_full, int h, int w, const float *d_raycolor, const float *d_gt_rays,
                      const int8_t *d_ray_mask, int R, int win, float data_range, double *d_row, uint8_t *d_img8, uint8_t *d_gt8,
                      void *d_scratch, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Multi-GPU training (BASELINE config C5): sparse exchange of the point-buffer gradients of a patch-sharded step.  No reference counterpart
 * (its DataParallel wrapper runs on gpu_ids[0] only, models/neural_points_volumetric_model.py:161-167; autograd writes dense [N, C] gradients).
 *   hnr_point_grad_pack   d_ids / d_count: the batch's touched points (hnr_render_train_touched); d_n_valid: this rank's number of valid rays (one
 *                         float: d_out4[3] of hnr_shipped_loss_rows); the four dense gradients of hnr_render_train_backward.
 *                         d_rec [capacity + 2][40] floats: row 0 = {records, valid rays, overflow flag}; rows 1..capacity = {point id (int32 bits) |
 *                         emb 32 | conf | dir 3 | colour 3}, unused slots id -1; row capacity + 1 = point 0 when the batch did not touch it (the empty
 *                         neighbour slots' d conf_coefficient lands there, neural_points.py:711).
 *   hnr_point_grad_apply  d_all_rec [n_ranks][capacity + 2][40] (ONE all-gather of the ranks' d_rec): rewrites the dense gradients in place as
 *                         sum_r (n_r / n) g_r -- the gradient of the loss's mean over ALL ranks' valid rays -- adding the ranks' rows in rank order (the
 *                         same bits on every rank); only rows some rank touched are written.  d_out2 (optional) = {n, overflow flag of any rank}. */
int hnr_point_grad_pack(const int32_t *d_ids, const int64_t *d_count, int capacity, const float *d_n_valid, const float *d_g_emb, const float *d_g_conf,
                        const float *d_g_dir, const float *d_g_color, float *d_rec, void *stream);
int hnr_point_grad_apply(const float *d_all_rec, int n_ranks, int capacity, float *d_g_emb, float *d_g_conf, float *d_g_dir, float *d_g_color, int n_points,
                         float *d_out2, void *stream);

/* ------------------------------------------------------------------------------------------------
 * "Next" row: voxel down-sampling of the initial point cloud, models/mvs/mvs_utils.py:537-563
 * (`construct_vox_points_closest`, called at run/train_ft.py:164 and :725; needs torch_scatter in the reference).
 *   cell = floor((xyz - space_min) / vox_size)  (fp32 subtract, fp32 divide);  voxels in the lexicographic order of torch.unique(dim=0);
 *   d_centroid [V,3] per-voxel mean (sequential fp32 sum in point-id order), d_grid_idx [V,3] the cells, d_min_idx [V] the point
 *   closest to its voxel's centroid (first one on ties), d_inverse [n] voxel of every point (may be NULL), d_count[0] = V.
 * Output arrays are sized for n voxels.  space_min: 3 host floats.  Synchronises the stream (it reports out-of-range points). */
int64_t hnr_voxel_downsample_scratch_bytes(int64_t n);
int hnr_voxel_downsample(const float *d_xyz, int n, const float *space_min, float vox_size, float *d_centroid, int32_t *d_grid_idx,
                         int32_t *d_min_idx, int32_t *d_inverse, int64_t *d_count, void *d_scratch, int64_t scratch_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * The initial point cloud from posed depth frames (`load_points=2`, run/train_ft.py:687-770).  Stream-ordered, nothing is read back; every fp32
 * operation is rounded on its own in the order given (tests/cloud_init_ref.py restates them).
 *
 * hnr_depth_fuse_frame -- one depth frame: data/scannet_ft_dataset.py:609-642 (read_depth's scaling and range rule, back-projection,
 * `construct_vox_points_xyz`, models/mvs/mvs_utils.py:503-517, on the frame's own bounds) + the torch.cat at :642 as an append at a device count.
 *   d_depth [H,W] uint16 (raw / depth_div) or float32 (metres); Ki [3,3] inverse depth intrinsic, c2w [4,4]: host floats, row-major.
 *   Per pixel (px, py), row-major: d = 0 where d > depth_max or d < depth_min; v = (px*d, py*d, d); cam[c] = (v0*Ki[c][0] + v1*Ki[c][1]) + v2*Ki[c][2];
 *   kept when cam[2] > 0; world[c] = ((cam0*M[c][0] + cam1*M[c][1]) + cam2*M[c][2]) + M[c][3].  The kept points are voxelised with frame_vox_res
 *   cells on their own bounding cube (x 1.05) and the per-voxel centroids (sequential fp32 sum in pixel order / count), in lexicographic cell order,
 *   are written to d_cloud [capacity,3] at d_count[0], which grows by their number.  frame_vox_res <= 0: the kept points themselves, pixel order.
 *   A frame without a kept pixel appends nothing (the reference raises there).  Nothing is written past capacity: d_status[0] |= HNR_CLOUD_OVERFLOW and
 *   d_count[0] keeps counting, so it ends as the capacity the run needed.  d_scratch: hnr_depth_fuse_scratch_bytes(H, W) bytes (negative: bad shape). */
#define HNR_CLOUD_OVERFLOW 1
int64_t hnr_depth_fuse_scratch_bytes(int H, int W);
int hnr_depth_fuse_frame(const void *d_depth, int depth_is_u16, int H, int W, const float *Ki, const float *c2w, float depth_div, float depth_min,
                         float depth_max, int frame_vox_res, float *d_cloud, int64_t capacity, int64_t *d_count, int32_t *d_status, void *d_scratch,
                         int64_t scratch_bytes, void *stream);

/* Range crop (run/train_ft.py:713-716, data/scannet_ft_dataset.py:643-646): d_out = the points of d_xyz[0 : d_n_in[0]] with
 * ranges[0:3] <= p <= ranges[3:6], in their order; d_n_out[0] = their number.  ranges: 6 host floats; ranges[0] <= -99 keeps every point.
 * n_max >= d_n_in[0] sizes the launch, d_out [n_max,3] and the scratch (hnr_range_crop_scratch_bytes(n_max); negative: n_max outside 1 .. 2^30). */
int64_t hnr_range_crop_scratch_bytes(int64_t n_max);
int hnr_range_crop(const float *d_xyz, const int64_t *d_n_in, int64_t n_max, const float *ranges, float *d_out, int64_t *d_n_out, void *d_scratch,
                   int64_t scratch_bytes, void *stream);

/* `nearest_view` (run/train_ft.py:48-57) in one launch: d_view[i] = argmin over the M cameras of
 *   n / 200 + (1.1 - ((ux*rx + uy*ry) + uz*rz)),  d = p - campos, n = sqrt((dx*dx + dy*dy) + dz*dz), u = d / (n + 1e-6), r = camdir;
 * the first strict minimum wins (torch.argmin).  d_xyz [N,3], d_campos / d_camdir [M,3], d_view [N] int32. */
int hnr_nearest_view(const float *d_xyz, int64_t N, const float *d_campos, const float *d_camdir, int M, int32_t *d_view, void *stream);

/* Per-point attributes from the view a point was assigned to: `homo_warp_nongrid` + `extract_from_2d_grid` (models/mvs/mvs_utils.py:299-315, :411-420)
 * and the `dir` branch of `query_embedding` with pointdir_w=True (models/mvs/mvs_points_model.py:239-251), called at run/train_ft.py:759-760.
 *   cam[c] = ((x*w2c[c][0] + y*w2c[c][1]) + z*w2c[c][2]) + w2c[c][3];  q = cam / cam[2];  gx = (q0*K00 + q1*K01) + K02, gy likewise with row 1;
 *   mask = 0 <= gx <= W-1 && 0 <= gy <= H-1 (NaN: 0; no z > 0 test, as in the reference);
 *   d_out_feat [n,C]: bilinear sample of d_feat [C,Hl,Wl] at (gx*(Wl-1)/(W-1), gy*(Hl-1)/(H-1)), zero padding, align_corners=True; zeros where mask = 0;
 *   d_out_dir [n,3], for every point: e = cam - cam_pos_cam, u = e / (|e| + 1e-6), dir[c] = (u0*R[c][0] + u1*R[c][1]) + u2*R[c][2], R = c2w[:3,:3].
 * w2c, c2w [4,4], cam_pos_cam [3] (= (c2w[:,3] @ w2c^T)[:3], computed by the caller as the reference does), K [3,3]: host floats.  Any of the three
 * outputs may be NULL (not all); d_feat / C / Hl / Wl are read only with d_out_feat. */
int hnr_point_view_attrs(const float *d_xyz, int64_t n, const float *w2c, const float *c2w, const float *cam_pos_cam, const float *K, int H, int W,
                         const float *d_feat, int C, int Hl, int Wl, float *d_out_feat, float *d_out_dir, uint8_t *d_out_mask, void *stream);
/* The same with the occlusion flags of hnr_point_occlusion: d_visible [n] uint8 (NULL: hnr_point_view_attrs itself, which forwards here).  Where it is
 * 0 the point is treated as outside the frame -- mask 0, zero features, its direction -- which is what `extract_from_2d_grid` does with the mask
 * `homo_warp_nongrid_occ` has shrunk (models/mvs/mvs_utils.py:363, :411-420). */
int hnr_point_view_attrs_vis(const float *d_xyz, int64_t n, const float *w2c, const float *c2w, const float *cam_pos_cam, const float *K, int H, int W,
                             const float *d_feat, int C, int Hl, int Wl, const uint8_t *d_visible, float *d_out_feat, float *d_out_dir,
                             uint8_t *d_out_mask, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Point embeddings from the MVS init checkpoint: the last stage of the `load_points=2` start of a scene (run/train_ft.py:751-765).  Inference only.
 *
 * hnr_featnet_forward -- `FeatureNet(intermediate=True)` in eval mode, models/mvs/models.py:717-764 (the reference builds it from InPlaceABN):
 *   conv0: 3->8, 8->8 (3x3, stride 1, pad 1); conv1: 8->16 (5x5, stride 2, pad 2), 16->16, 16->16 (3x3); conv2: 16->32 (5x5, stride 2, pad 2), 32->32,
 *   32->32 (3x3); the eight convolutions have no bias and each is followed by y = leaky_relu((x - running_mean) * mul + bias, 0.01) with
 *   mul = rsqrt(running_var + 1e-5) * (|weight| + 1e-5) (the activated batch norm in inference form; mul is folded by whoever packs); `toplayer`: 1x1,
 *   32->32, with bias, no activation, applied to conv2's output.
 *   d_images [V,3,H,W] -> d_x1 [V,8,H,W], d_x2 [V,16,H2,W2], d_x3 [V,32,H4,W4], channels-first (what hnr_point_view_attrs / hnr_point_embed sample),
 *   H2 = (H-1)/2 + 1, H4 = (H2-1)/2 + 1 (integer division), likewise W.  fp32 direct convolution; every output is ONE chain of fused multiply-adds over
 *   (input channel, ky, kx) in that order, zero padding included, so two runs give the same bits.
 *   d_packed [HNR_FEATNET_PACKED_ELEMS]: per convolution, in network order, w [cin][ky][kx][cout] (the transpose of torch's [cout][cin][ky][kx]),
 *   running_mean [cout], mul [cout], bias [cout]; then the toplayer's w [cout][cin] (torch's own layout) and bias [cout].
 *   d_scratch: hnr_featnet_scratch_elems(V, H, W) floats (negative: bad shape).  HNR_ERR_BADARG, before any launch, for a NULL pointer, V < 1,
 *   H < 4 or W < 4 (limits: V <= 4096, H, W <= 32768). */
#define HNR_FEATNET_PACKED_ELEMS 41368
int64_t hnr_featnet_scratch_elems(int V, int H, int W);
int hnr_featnet_forward(const float *d_images, int V, int H, int W, const float *d_packed, float *d_x1, float *d_x2, float *d_x3, float *d_scratch,
                        int64_t scratch_elems, void *stream);

/* hnr_point_embed -- `query_embedding` for the shipped feature string "imgfeat_0_0123 dir_0 point_conf" with shading_feature_mlp_layer0 = 1
 * (models/mvs/mvs_points_model.py:225-259), one view, one launch: projection, mask, direction and samples are those of hnr_point_view_attrs (the same
 * device functions: bit-equal results), the feature maps are one view of hnr_featnet_forward's pyramid for the H x W image d_image [3,H,W]:
 *   row = [x1 8 | x2 16 | x3 32 | colour 3 | dir 3 | conf = 1]  (a point outside the frame: zero features and colour, its direction; it still goes
 *   through premlp, as in the reference);  h = leaky_relu(b0 + row W0^T, 0.01);  d_emb [n,32] = leaky_relu(b1 + h W1^T, 0.01), each sum one chain of
 *   fused multiply-adds starting from the bias, inputs in ascending order.
 *   d_premlp [HNR_PREMLP_PACKED_ELEMS]: W0^T [63][32], b0 [32], W1^T [32][32], b1 [32] (the transposes of nn.Linear's weights).
 *   d_color [n,3], d_dir [n,3]; d_row [n,63] (optional, NULL: not written) is the row premlp saw.  1 <= n <= (2^31 - 1) * 256, 4 <= H, W <= 32768. */
#define HNR_PREMLP_PACKED_ELEMS 3104
int hnr_point_embed(const float *d_xyz, int64_t n, const float *w2c, const float *c2w, const float *cam_pos_cam, const float *K, int H, int W,
                    const float *d_image, const float *d_x1, const float *d_x2, const float *d_x3, const float *d_premlp, float *d_emb, float *d_color,
                    float *d_dir, float *d_row, void *stream);
/* The same with a photometric confidence per point: d_conf [n] (NULL: ones, hnr_point_embed itself) takes the row's last column, as
 * `query_embedding` does when it is handed one (mvs_points_model.py:252-258, from run/train_ft.py:176-180). */
int hnr_point_embed_conf(const float *d_xyz, int64_t n, const float *w2c, const float *c2w, const float *cam_pos_cam, const float *K, int H, int W,
                         const float *d_image, const float *d_x1, const float *d_x2, const float *d_x3, const float *d_premlp, const float *d_conf,
                         float *d_emb, float *d_color, float *d_dir, float *d_row, void *stream);
/* ... and with the occlusion flags of hnr_point_occlusion (`depth_occ = 1`, mvs_points_model.py:203): d_visible [n] uint8 (NULL: hnr_point_embed_conf
 * itself, which forwards here).  Where it is 0 the point is treated as outside the frame: zero features and colour, its direction, and still a row
 * through premlp. */
int hnr_point_embed_vis(const float *d_xyz, int64_t n, const float *w2c, const float *c2w, const float *cam_pos_cam, const float *K, int H, int W,
                        const float *d_image, const float *d_x1, const float *d_x2, const float *d_x3, const float *d_premlp, const float *d_conf,
                        const uint8_t *d_visible, float *d_emb, float *d_color, float *d_dir, float *d_row, void *stream);

/* ------------------------------------------------------------------------------------------------
 * The per-step data path: a device-resident frame bank and the ray batch drawn from it (csrc/frames.hip).  Replaces the dataset item of the
 * reference, data/scannet_ft_dataset.py:736-976 (data/nerf_synth360_ft_dataset.py:643-800), image decoding aside: per step the reference draws pixel
 * coordinates with numpy (:892-949), builds raydir with get_dtu_raydir (data/data_utils.py:57-71), gathers gt_image (:957) and uploads the V nearest
 * frames as float32 (:821-855).  Stream-ordered, nothing is allocated, nothing is read back, at most three launches; every fp32 operation is rounded
 * on its own in the order given and the random words are Philox4x32-10 (tests/frames_ref.py restates all of it; the GPU tests compare bits).
 *
 * hnr_frame_bank -- what stays on the device for one split of a scene:
 *   d_images [F,H,W,3] uint8 (decoded frames) or float32 (images_f32 = 1: the synthetic set's white-composited images, nerf_synth360_ft_dataset.py:536);
 *   d_c2w, d_w2c [F,4,4]; d_intrinsic [3,3], or [F,3,3] with intrinsic_per_frame = 1; d_weight [F] = train_weight_list ** weight_exp (:756-759, :834);
 *   d_angle [F] = vid / total_num_image * 2 pi (:830). */
typedef struct {
    const void *d_images;
    const float *d_c2w, *d_w2c, *d_intrinsic, *d_weight, *d_angle;
    int images_f32, F, H, W, intrinsic_per_frame;
} hnr_frame_bank;

/* hnr_frame_batch_params -- how the pixels of a batch are drawn (scannet_ft_dataset.py:892-949; m = margin = opt.edge_filter):
 *   words w0..w3 = Philox4x32-10(counter = (step low, step high, purpose, index), key = (seed low, seed high));
 *   randint(u, lo, hi) = lo + (((uint64) u * (uint32)(hi - lo)) >> 32);
 *   HNR_FRAMES_RANDOM   size^2 rays; purpose 0, index = ray: px = randint(w0, m, W - m), py = randint(w1, m, H - m)                       (:899-907)
 *   HNR_FRAMES_PATCH    the dilated mode with patch_num = 1, patch_size = size, dilation 1                                               (:893-898)
 *   HNR_FRAMES_DILATED  (patch_num * patch_size)^2 rays; purpose 1, index = patch pi * patch_num + pj: d = randint(w0, dilation_lo, dilation_hi + 1),
 *                       x0 = randint(w1, m, W - m - (patch_size - 1) d), y0 = randint(w2, m, H - m - (patch_size - 1) d); pixel (row a, column b) of
 *                       the patch is (x0 + d b, y0 + d a) at grid position (pi * patch_size + a, pj * patch_size + b), rays row-major       (:917-940)
 *   bg_random           purpose 2, index 0: white when w0 >= 2^31, else black (:964-969); otherwise bg_color
 *   ray (get_dtu_raydir) x = ((px + 0.5) - K02) / K00, y = ((py + 0.5) - K12) / K11, dir[c] = (x R[c][0] + y R[c][1]) + R[c][2], R = c2w[:3,:3];
 *                       dir_norm: dir / (sqrt((dx^2 + dy^2) + dz^2) + 1e-5)
 *   pixels              gt_image = frame[(int) py][(int) px]; uint8 v -> (float) v / 255.0f (a division, as ToTensor); float32 banks are copied
 *   downweight_blurry_feats: frame_weight_nearest = the reference bank's weights (:832-834), ones otherwise. */
#define HNR_FRAMES_RANDOM  0
#define HNR_FRAMES_PATCH   1
#define HNR_FRAMES_DILATED 2
typedef struct {
    int mode, size, patch_num, patch_size, dilation_lo, dilation_hi, margin, dir_norm, bg_random, downweight_blurry_feats;
    float bg_color[3];
    uint64_t seed;
} hnr_frame_batch_params;

/* hnr_frame_batch_out -- the item's tensors; a NULL pointer is an output that is not wanted (nothing is written for it):
 *   per ray       d_raydir [R,3], d_pixel_idx [R,2] (x, y) float32, d_gt_image [R,3]
 *   camera        d_campos [3], d_camrot [3,3], d_c2w [4,4], d_intrinsic [3,3]
 *   views         d_c2w_nearest, d_w2c_nearest [V,4,4], d_campos_nearest [V,3], d_intrinsic_nearest [3,3] (of the first view), d_images_nearest [V,H,W,3]
 *                 float32 (16-byte aligned), d_frame_weight_nearest [V], d_vid_angle_nearest [V]
 *   scalars       d_frame_weight [1], d_bg_color [3], d_frame_row [1] int32, d_patch_table [patch_num^2,3] int32 (d, x0, y0; patch / dilated) */
typedef struct {
    float *d_raydir, *d_pixel_idx, *d_gt_image, *d_campos, *d_camrot, *d_c2w, *d_intrinsic, *d_c2w_nearest, *d_w2c_nearest, *d_campos_nearest,
          *d_intrinsic_nearest, *d_images_nearest, *d_frame_weight_nearest, *d_vid_angle_nearest, *d_frame_weight, *d_bg_color;
    int32_t *d_frame_row, *d_patch_table;
} hnr_frame_batch_out;

/* hnr_frame_batch -- the batch of step d_step[0]: the frame is row d_schedule[d_step[0] % n_schedule] of `target`, its V reference views are rows
 * d_nearest[row * V ..] of `reference` (the same bank, or a test split's train bank; same H, W), and d_step[0] (uint64) advances by one, exactly once.
 * The frame number and the counter are read on the device: the call can be captured in a hipGraph on one stream and replayed.
 * d_scratch: hnr_frame_batch_scratch_bytes(mode, patch_num) bytes (negative: bad arguments), private to the call sequence of one sampler.
 * Ranges that are empty for the frame size (margin, patch reach) and rows outside a bank are HNR_ERR_BADARG / the caller's to validate
 * (the kernels clamp a bad row to 0 rather than read outside the bank). */
int64_t hnr_frame_batch_scratch_bytes(int mode, int patch_num);
int hnr_frame_batch(const hnr_frame_bank *target, const hnr_frame_bank *reference, const int32_t *d_nearest, int V, const hnr_frame_batch_params *p,
                    const int32_t *d_schedule, int n_schedule, uint64_t *d_step, const hnr_frame_batch_out *out, void *d_scratch, int64_t scratch_bytes,
                    void *stream);

/* hnr_frame_item -- the same item for an explicit frame `row` (a host int), no counter, no random words: with d_pixels [n_rays,2] float32 (x, y)
 * those pixels (fractional ones truncate for gt_image, as :957; a pixel outside the frame gets gt_image = 0), with d_pixels = NULL every pixel minus
 * `margin` in scan-line order, n_rays = (W - 2 margin)(H - 2 margin) (`no_crop`, :946-949).  bg_color: 3 host floats.  d_scratch: 16 bytes. */
int hnr_frame_item(const hnr_frame_bank *target, const hnr_frame_bank *reference, const int32_t *d_nearest, int V, int row, const float *d_pixels,
                   int64_t n_rays, int margin, int dir_norm, const float *bg_color, int downweight_blurry_feats, const hnr_frame_batch_out *out,
                   void *d_scratch, int64_t scratch_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Camera paths (csrc/path.hip): the dataset item of a camera that is NOT a row of a frame bank -- a fly-through, an orbit, a viewer's pose -- and
 * the store of a rendered frame into a clip.  The reference's run/render_vid.py is no usable definition (get_dummyrot_item carries no reference
 * views, its rays come from the Blender ray builder applied to an OpenCV pose, the ScanNet dataset has no render_poses), so the behaviour is DEFINED
 * here and restated in tests/path_ref.py.  All three entries: stream-ordered, nothing allocated, nothing read back, no atomics, deterministic,
 * capturable on one stream; every fp32 operation rounded on its own in the order written; HNR_ERR_BADARG before any launch.
 *
 * hnr_pose_views -- the V reference views of Q free cameras among the T = reference->F cameras of a bank: get_nearest_cam_id
 * (data/nerf_synth360_ft_dataset.py:49-74; frames.nearest_by_pose on the host) with every tie decided.  Only d_c2w, d_intrinsic
 * (intrinsic_per_frame), F, H, W of the bank are read.
 *   d_poses [Q,4,4] c2w, d_intrinsic [3,3] or, with intrinsic_per_pose = 1, [Q,3,3]: device memory, read when the kernel runs.
 *   direction   of a camera (c2w, K): the normalised ray of pixel (W / 2, H / 2) (integer halves), the arithmetic of the batch's rays:
 *               x = ((px + 0.5f) - K02) / K00, y = ((py + 0.5f) - K12) / K11, dir[c] = (x R[c][0] + y R[c][1]) + R[c][2],
 *               d = dir / (sqrt((dx^2 + dy^2) + dz^2) + 1e-5f); a train camera's direction is this expression of its own c2w and K.
 *   step 1      score s_t = (tx dx + ty dy) + tz dz; the n1 rows with the largest s, equal scores (-0 = +0) the lower row first (a stable
 *               argsort(-s)).  n1 is the caller's: min(num_times V, floor(T / 10)) in the reference.
 *   step 2      those n1 rows by e_t = sqrt((ax^2 + ay^2) + az^2), a = c2w_t[:3,3] - c2w_q[:3,3], ascending, equal distances in step-1 order.
 *   exclude     d_exclude_row [Q] int32 or NULL: when the FIRST row of step 2 equals d_exclude_row[q] (>= 0) it is skipped (the `is_train` rule).
 *   result      the first V rows that remain -> d_nearest [Q,V] int32.  A NaN score or distance orders last.
 *   limits      1 <= V <= 64, 1 <= T <= 8192, 1 <= Q <= 2^24, V + (d_exclude_row ? 1 : 0) <= n1 <= T.
 * One launch, one workgroup per query; the orders come from a bitonic sort of 64-bit keys (float bits, index) in LDS. */
int hnr_pose_views(const hnr_frame_bank *reference, const float *d_poses, int Q, const float *d_intrinsic, int intrinsic_per_pose,
                   const int32_t *d_exclude_row, int V, int n1, int32_t *d_nearest, void *stream);

/* hnr_path_item -- the dataset item of frame i of a pose table d_poses [P,4,4] (d_intrinsic [3,3], or [P,3,3] with intrinsic_per_pose = 1), into the
 * struct hnr_frame_batch / hnr_frame_item fill; NULL outputs are skipped.  i = d_step[0] % P read on the device, d_step[0] (uint64) advancing by
 * exactly one; with d_step = NULL, i is the explicit host int.  Pose and intrinsic are read from device memory when the kernels run: rewriting the
 * table in place (a viewer, a path generator on the device) changes the next item, the host knows nothing about them.
 *   written     d_campos, d_camrot, d_c2w, d_intrinsic (of pose i); the V views hnr_pose_views picks for it (no exclusion) as d_c2w_nearest,
 *               d_w2c_nearest, d_campos_nearest, d_intrinsic_nearest, d_frame_weight_nearest (the bank's weights with downweight_blurry_feats,
 *               ones otherwise), d_vid_angle_nearest, d_images_nearest float32 (16-byte aligned for a uint8 bank); d_bg_color = bg_color (3 host
 *               floats), d_frame_row = i; d_raydir / d_pixel_idx for every pixel minus `margin` in scan-line order, (W - 2 margin)(H - 2 margin) rays,
 *               H and W the reference bank's.  The arithmetic is hnr_frame_item's: for a pose equal to a bank row's camera the bits are equal.
 *   not written d_gt_image, d_frame_weight, d_patch_table: non-NULL is HNR_ERR_BADARG.
 *   d_scratch   HNR_PATH_SCRATCH_BYTES bytes, private to the call sequence of one sampler.
 * At most three launches. */
#define HNR_PATH_SCRATCH_BYTES 512
int hnr_path_item(const hnr_frame_bank *reference, const float *d_poses, int P, const float *d_intrinsic, int intrinsic_per_pose, int V, int n1,
                  uint64_t *d_step, int i, int margin, int dir_norm, const float *bg_color, int downweight_blurry_feats, const hnr_frame_batch_out *out,
                  void *d_scratch, int64_t scratch_bytes, void *stream);

/* hnr_frame_store -- rendered rays into one frame of a clip: d_color [R,3], d_pixel_idx [R,2] float32 (x, y; truncated), optional d_depth [R] ->
 * any non-NULL combination of d_img8 [h,w,3] uint8 = q(colour), q(x) = (uint8) trunc(min(max(x, 0), 1) * 255.0f) as hnr_frame_metrics quantises
 * (one fp32 product; NaN -> 0), d_image [h,w,3] float32, d_depth_image [h,w] float32 (needs d_depth).  The frame is cleared first, in stream order:
 * pixels no ray reached read 0.  A pixel index outside the frame (or NaN) is dropped; the indices of one call must be distinct pixels.
 * R = 0 only clears.  Replaces torch.zeros + index-put + a separate quantisation per frame. */
int hnr_frame_store(const float *d_color, const float *d_pixel_idx, const float *d_depth, int64_t R, int h, int w, uint8_t *d_img8, float *d_image,
                    float *d_depth_image, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Raw frames to the bank's size (csrc/resize.hip): Pillow's convolution resize for 8-bit images, bit for bit.  Replaces the per-frame
 * `Image.open(...).resize(self.img_wh, Image.LANCZOS)` of data/scannet_ft_dataset.py:742,824 and data/nerf_synth360_ft_dataset.py:531,762, decoding
 * aside (that stays on the host), and the images of nerf_synth360_ft_dataset.py:532-536.  tests/resize_ref.py restates all of it in NumPy;
 * tests/test_resize.py holds that text to PIL.Image.resize, the GPU tests hold the kernels to Pillow.  Not covered: Pillow's box= and reducing_gap=
 * arguments, NEAREST, 16-bit and float images.
 *
 * hnr_resize_coeffs -- HOST function, no GPU call: the tables of one axis, `n_in` -> `n_out` elements, as Pillow's precompute_coeffs +
 * normalize_coeffs_8bpc compute them (double arithmetic, libm):
 *   S = 0.5 (box), 1 (bilinear), 1 (hamming), 2 (bicubic, a = -0.5), 3 (lanczos: sinc(x) sinc(x / 3) on -3 <= x < 3)
 *   scale = n_in / n_out, fs = max(scale, 1), support = S fs, ksize = 2 ceil(support) + 1, ss = 1 / fs; for output xx:
 *   centre = (xx + 0.5) scale, xmin = max((int)(centre - support + 0.5), 0), xmax = min((int)(centre + support + 0.5), n_in) - xmin,
 *   w[x] = filter((x + xmin - centre + 0.5) ss) for x < xmax, divided by their sum in index order (when it is not 0),
 *   coef[xx][x] = (int)(w 2^22 + 0.5) for w >= 0, (int)(w 2^22 - 0.5) otherwise; 0 for xmax <= x < ksize; bounds[xx] = (xmin, xmax).
 * Returns ksize (> 0), or a negative error.  bounds = coef = NULL: only ksize (to size the tables); otherwise both, host memory, coef_elems >= n_out ksize. */
#define HNR_RESIZE_BOX      0
#define HNR_RESIZE_BILINEAR 1
#define HNR_RESIZE_HAMMING  2
#define HNR_RESIZE_BICUBIC  3
#define HNR_RESIZE_LANCZOS  4
int hnr_resize_coeffs(int n_in, int n_out, int filter, int32_t *bounds, int32_t *coef, int64_t coef_elems);

/* hnr_resize_u8 -- N frames d_src [N,h,w,C] uint8 -> d_dst [N,H,W,C] uint8, C = 1, 3 or 4 (channels are independent).  d_src may start at any
 * byte; d_dst may be rows of a larger bank.  Tables: d_bounds_h [W,2], d_coef_h [W,ksize_h] for the width, d_bounds_v [H,2], d_coef_v [H,ksize_v]
 * for the height -- hnr_resize_coeffs' output copied to the device (bounds 8-byte aligned); those of an axis whose size does not change are not read.
 *   pass     out = clip8((2^21 + sum_{x < xmax} in[xmin + x] coef[x]) >> 22): int32 sum, arithmetic shift, clamp to 0 .. 255
 *   order    horizontal first when w != W, its result ROUNDED TO uint8; vertical on that when h != H; neither: a copy
 *   form     HNR_RESIZE_FUSED: one launch, a workgroup per HNR_RESIZE_TILE_W x HNR_RESIZE_TILE_H output pixels, the input footprint and the uint8
 *            intermediate of the tile in LDS (the intermediate never reaches memory); HNR_ERR_BADARG when a tile's footprint (static + dynamic LDS)
 *            exceeds HNR_RESIZE_LDS_BUDGET bytes.  HNR_RESIZE_TWO_PASS: two launches through d_scratch [N,h,W,C], one lane per output byte.  Both give the
 *            same bytes.  HNR_RESIZE_AUTO: fused when the footprint fits, else two-pass; hnr_resize_u8_form tells which (host only, from sizes).
 *   scratch  hnr_resize_u8_scratch_bytes(...) bytes (0 unless both sizes change); read and written by the two-pass form only.
 * Stream-ordered, nothing is allocated or read back; bounds from the tables are clamped, so bad tables cannot reach outside the buffers.
 * Limits: 1 <= N <= 65535, h w and H W <= 2^26, N max(h, H) max(w, W) <= 2^36. */
#define HNR_RESIZE_AUTO     0
#define HNR_RESIZE_FUSED    1
#define HNR_RESIZE_TWO_PASS 2
#define HNR_RESIZE_TILE_W   64
#define HNR_RESIZE_TILE_H   16
#define HNR_RESIZE_LDS_BUDGET 65536
int64_t hnr_resize_u8_scratch_bytes(int N, int h, int w, int C, int H, int W);
int hnr_resize_u8_form(int h, int w, int C, int H, int W, int ksize_h, int ksize_v);
int hnr_resize_u8(const uint8_t *d_src, int N, int h, int w, int C, uint8_t *d_dst, int H, int W, const int32_t *d_bounds_h, const int32_t *d_coef_h,
                  int ksize_h, const int32_t *d_bounds_v, const int32_t *d_coef_v, int ksize_v, int form, void *d_scratch, int64_t scratch_bytes,
                  void *stream);

/* The two element-wise steps of Image.resize on a mode-RGBA image (RGBA -> RGBa, resize the four channels, RGBa -> RGBA), n_pixels x 4 bytes,
 * in place (d_dst = d_src) or not, any byte alignment.  Pillow returns a copy of a SAME-SIZE image before the conversion: a caller skips both steps then
 * (frames.resize_frames does), or colours under partial alpha change:
 *   premultiply    c' = ((t >> 8) + t) >> 8, t = c a + 128; a kept
 *   unpremultiply  c = c' when a is 0 or 255, else min(255 c' / a, 255) with integer division; a kept */
int hnr_rgba_premultiply(const uint8_t *d_src, uint8_t *d_dst, int64_t n_pixels, void *stream);
int hnr_rgba_unpremultiply(const uint8_t *d_src, uint8_t *d_dst, int64_t n_pixels, void *stream);

/* hnr_rgba_compose -- nerf_synth360_ft_dataset.py:532-536 on resized RGBA frames d_rgba [n_pixels,4] uint8: with c, a = (float) u8 / 255.0f,
 * d_black [n,3] = c a, d_white [n,3] = c a + (1 - a), d_alpha [n] = a, d_mask [n] = a > 0.1f ? 1 : 0, float32; any non-NULL subset.  Every operation
 * is rounded on its own in the order divide, multiply, subtract, add: the bits of the torch expressions on the CPU. */
int hnr_rgba_compose(const uint8_t *d_rgba, int64_t n_pixels, float *d_white, float *d_black, float *d_alpha, float *d_mask, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Depth supervision from resident sensor depth (csrc/depth_sup.hip): the per-ray ground-truth depth of a batch, the depth term of the training loss
 * with its gradient, and the depth error of a rendered test frame.  The reference has a `depth_loss_items` branch
 * (models/base_rendering_model.py:1209-1215) but neither of its datasets emits gt_depth or gt_mask, so the behaviour is DEFINED here and restated
 * in tests/depth_sup_ref.py.  All three: one launch, stream-ordered, no allocation, no host read, no atomics, sums in a fixed order (two runs give
 * the same bits), capturable on one stream.  gt_depth = 0 means "no measurement" everywhere.
 *
 * hnr_depth_bank -- the depth frames of a split, beside its hnr_frame_bank (same F, same rows):
 *   d_depth [F,Hd,Wd] uint16 raw sensor values, or float32 metres with depth_f32 = 1; stored as given;
 *   d_depth_intrinsic [3,3] on the device, or NULL: then (Hd, Wd) is the colour frame's (H, W) and a ray reads the texel gt_image reads;
 *   depth_div (raw units per metre, 1000 for ScanNet), depth_min, depth_max: the valid range in metres. */
typedef struct {
    const void *d_depth;
    const float *d_depth_intrinsic;
    int depth_f32, F, Hd, Wd;
    float depth_div, depth_min, depth_max;
} hnr_depth_bank;

/* hnr_frame_depth_rays -- d_gt_depth [R] float32 for the rays of an item, one lane per ray.
 *   frame        row = d_frame_row[0], READ ON THE DEVICE: the word hnr_frame_batch / hnr_frame_item wrote (their d_frame_row output), so the call
 *                follows the batch inside a captured graph.  There is no host-row variant: an explicit item passes its row through that same
 *                device int.  A row outside the bank reads row 0, like the other frame kernels.
 *   value        d = (float) raw / depth_div, a correctly rounded division (read_depth of the reference's dataset); float banks are copied;
 *                d = 0 unless depth_min <= d <= depth_max (so d > depth_max, d < depth_min and a NaN all read 0).
 *   pixel        (px, py) = d_pixel_idx[r] (x, y), the item's pixel_idx.
 *     no depth intrinsic:  (u, v) = ((int) px, (int) py), the texel gt_image reads.
 *     depth intrinsic Kd:  the ray's plane coordinates as the batch kernel forms them, x = ((px + 0.5f) - K02) / K00, y = ((py + 0.5f) - K12) / K11 with
 *                K = d_intrinsic [3,3], the item's colour intrinsic; u = (int) floorf((x * Kd00 + Kd02) + 0.5f), v = (int) floorf((y * Kd11 + Kd12) + 0.5f):
 *                integer pixel = centre, the convention load_init_depth_points unprojects with (scannet_ft_dataset.py:617-633), so supervision and
 *                the initial cloud agree.  Each fp32 operation is rounded on its own in the order written.
 *     (u, v) outside the depth frame: 0.
 *   d_intrinsic may be NULL without a depth intrinsic.  1 <= R <= 2^26. */
int hnr_frame_depth_rays(const hnr_depth_bank *bank, const int32_t *d_frame_row, const float *d_pixel_idx, const float *d_intrinsic, int R,
                         float *d_gt_depth, void *stream);

/* hnr_depth_loss -- the depth term of the training loss, value and gradient, ONE workgroup (batches are a few thousand rays; any 1 <= R <= 2^26 is
 * correct, the 1024 lanes stride over the rays).
 *   m_r = d_ray_mask[r] > 0 && d_gt_depth[r] > 0,  n = sum m_r
 *   L = sum m_r (D_r - d_r)^2 / n, 0 when n = 0: a masked mean like the colour item (the reference's unmasked mean would make the weight depend on
 *       the hit fraction).  Each (D_r - d_r)^2 is formed in fp32 (difference, then square) and the SUM RUNS IN fp64 in a fixed order -- per lane
 *       over r = lane, lane + 1024, ...; an xor butterfly (32, 16, .. 1) over each wave; the sixteen waves in order -- then L = (float)(sum / n).
 *   d_out3 = {L, n, w_depth * L};  d_total[0] += w_depth * L, one fp32 add (skipped when n = 0: the bits of d_total stay) -- d_total is d_out4 of
 *       the hnr_shipped_loss* kernels, queued before this call; NULL: value only.  The term is NOT multiplied by the frame weight: the reference
 *       scales by frame_weight before it adds its depth items (:1204-1215).
 *   d_g_depth[r] = m_r * (D_r - d_r) * ((2 w_depth) / (float) n) -- the scale once in fp32, a correctly rounded division -- and exactly 0 where
 *       m_r = 0 or n = 0; NULL: no gradient.  It is the d_g_depth of hnr_render_train_backward_depth.
 *   w_depth >= 0 and finite.  d_scratch is not used (the reduction stays in LDS) and may be NULL. */
int hnr_depth_loss(const float *d_depth, const float *d_gt_depth, const int8_t *d_ray_mask, int R, float w_depth, float *d_total, float *d_out3,
                   float *d_g_depth, void *d_scratch, void *stream);

/* hnr_depth_metrics -- the depth error of a rendered frame over the rays with a hit and a measurement (m_r as above), ONE workgroup:
 *   d_row [5] fp64 = {n, sum |e|, sum e^2, sum |e| / d, #(max(D / d, d / D) < 1.25)}, e = D - d in fp64 from the fp32 inputs, sums in the fixed
 *   order of hnr_depth_loss.  The threshold is evaluated as D > 0 && D < 1.25 d && d < 1.25 D (exact in fp64). */
#define HNR_DM_N       0
#define HNR_DM_ABS     1
#define HNR_DM_SQ      2
#define HNR_DM_ABSREL  3
#define HNR_DM_D1      4
#define HNR_DM_NCOLS   5
int hnr_depth_metrics(const float *d_depth, const float *d_gt_depth, const int8_t *d_ray_mask, int R, double *d_row, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Patch SSIM term of the training loss (csrc/ssim_loss.hip): L = 1 - SSIM over the ps x ps patches of a patch-sampled batch, value and gradient.
 * The reference carries the term in models/base_rendering_model.py:1120-1143 -- pytorch_msssim's SSIM(win_size=7, win_sigma=1.5, data_range=1,
 * channel=3) (:27) on the dilated patches, `loss = loss + (1 - ssim_module(patch_output_all, patch_gt_all))` -- but parks it behind a
 * pdb.set_trace(), and that package is not part of this project.  The formulas below follow its `_ssim` as far as known; THE DEFINITION HERE IS
 * THE CONTRACT, restated in tests/ssim_loss_ref.py.  Two launches, stream-ordered, no allocation, no host read, no atomics, sums in a fixed
 * order (two runs give the same bits), capturable on one stream.
 *
 *   patches     patch_num > 0 ("grid"): n = patch_num^2 patches tiled over an S x S batch, S = patch_num * patch_size; ray row * S + col is pixel
 *               (row % ps, col % ps) of patch (row / ps) * patch_num + col / ps.  patch_num < 0 ("patch_major", the sign convention of
 *               hnr_blur_select): n = -patch_num whole patches packed (patch, y, x).  7 <= ps = patch_size <= 64, W = ps - 6, n ps^2 <= 2^26.
 *   masking     m = d_ray_mask > 0;  X = m ? d_color : 0,  Y = m ? d_gt : 0  per ray and channel (:1124-1128).
 *   window      g = win[0..6], host memory, read during the call: losses.ssim_window() -- exp(-(i - 3)^2 / (2 * 1.5^2)) normalised to sum 1,
 *               formed in fp32 with the torch ops of the package's _fspecial_gauss_1d.  Each value must lie in [0, 1].
 *   filtering   "valid", separable, per patch and channel, every fp32 operation rounded on its own (no FMA), taps added in ascending i
 *               starting from 0.f:   T_q(y, x) = sum_{i=0..6} g[i] * q(y, x + i)  for q = X, Y, X*X, Y*Y, X*Y (products first),  x < W;
 *               then                 M_q(y, x) = sum_{i=0..6} g[i] * T_q(y + i, x),  y < W.
 *   window      mx = M_X, my = M_Y, exx = M_XX, eyy = M_YY, exy = M_XY;  mxx = mx*mx, myy = my*my, mxy = mx*my;
 *               sx = exx - mxx, sy = eyy - myy, sxy = exy - mxy;  C1 = 1e-4f, C2 = 9e-4f;
 *               A1 = 2*mxy + C1, B1 = (mxx + myy) + C1, A2 = 2*sxy + C2, B2 = (sx + sy) + C2;  l = A1 / B1, cs = A2 / B2,  s = l * cs
 *               (divisions correctly rounded).  No clamping, no nonnegative_ssim.
 *   gradient    a = ds/dmx = ((2*(my - l*mx)) / B1) * cs + l * ((2*(mx*cs - my)) / B2),  b = ds/dexx = -(s / B2),  c = ds/dexy = (2*l) / B2,
 *               each 0 outside the W x W windows;  U_k(y, x) = sum_{i=0..min(6,y)} g[i] * k(y - i, x),  G_k(y, x) = sum_{i=0..min(6,x)} g[i] *
 *               U_k(y, x - i)  for k = a, b, c;  d(sum s)/dX(y, x) = (G_a + (2*X) * G_b) + Y * G_c.
 *   value       N = norm_patches, or n when norm_patches = 0.  sum s runs in fp64 over the fp32 s: per lane over its windows (channel, y, x
 *               ascending), xor butterfly (32 .. 1) over each wave, waves in order, then patches (lane-strided over 64 lanes, butterfly).
 *               SSIM = (float)(sum s / (N 3 W^2)),  L = (float)((n 3 W^2 - sum s) / (N 3 W^2)): 1 - SSIM for N = n, and with N the batch-wide
 *               count the L of the ranks of a patch-sharded batch add up to the whole batch's.  hits = rays with m.  hits = 0: L = 0.
 *   outputs     d_out4 = {L, SSIM, (fw * w_ssim) * L, hits};  d_total[0] += (fw * w_ssim) * L, one fp32 add, skipped (bits untouched) when
 *               hits = 0 (:1117,1144-1145); d_total is d_out4 of the hnr_shipped_loss* kernels queued before, or NULL.  fw = d_frame_weight[0]
 *               (device, one float) when given, else frame_weight: the reference adds the term inside the colour item, before the frame-weight
 *               scaling (:1143,1198,1205).  w_ssim is an absolute weight.
 *               d_g_color [n ps^2, 3]:  v = m ? -((fw * w_ssim) / (float)(N 3 W^2)) * d(sum s)/dX : 0  -- written when accumulate = 0, ADDED in
 *               place (g = g + v, every ray, plain stores: each ray belongs to one patch) when accumulate = 1, e.g. onto d_g_color of
 *               hnr_shipped_loss_rows*; NULL (accumulate = 0): value only.
 *   errors      HNR_ERR_BADARG before anything is queued: patch_size outside 7..64, patch_num = 0, norm_patches < 0 or 0 < norm_patches < n,
 *               w_ssim or frame_weight negative or not finite, a window value outside [0, 1], NULL pointers.
 *   d_scratch   hnr_ssim_loss_scratch_bytes(n) bytes (n = patches of the call), 8-byte aligned. */
int64_t hnr_ssim_loss_scratch_bytes(int n_patches);
int hnr_ssim_loss(const float *d_color, const float *d_gt, const int8_t *d_ray_mask, int patch_num, int patch_size, int norm_patches,
                  const float *win, float w_ssim, float frame_weight, const float *d_frame_weight, float *d_total, float *d_out4,
                  float *d_g_color, int accumulate, void *d_scratch, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Growth schedule, the per-step part: the step's ray-miss loss and the table of the worst frames (prob_mode 0), ONE launch of one workgroup.
 * Replaces the `ray_miss_coarse_raycolor` item of compute_losses (models/base_rendering_model.py:1147-1159) and rank_ray_miss /
 * update_rank_ray_miss (models/mvs_points_volumetric_model.py:154-172), which cost two host synchronisations per step.
 *
 *   L = (sum over the rays with ray_mask == 0, over 3 channels, of (color - gt)^2) / 3   -- l2loss(masked_output, masked_gt) * masked_gt.shape[1];
 *       0 when no ray missed (and for R == 0).  Every difference and square is one rounded fp32 operation; the sums are fp64 in a fixed order
 *       (lane t of 256 takes rays t, t + 256, ...; a butterfly within each wave; the four waves in order); the division by 3 is fp64, rounded
 *       once to fp32.  d_color is the colour the loss kernels were given (the blur module's output when it ran, else coarse_raycolor); the rows
 *       of coarse_raycolor at rays with ray_mask == 0 hold bg_color (composite_kernel, csrc/aggregate.hip, writes it there), so L measures how
 *       far the ground truth of the missed rays is from the background.
 *   n >= 2: d_ids [n] / d_losses [n] are the table (top_ray_miss_ids / top_ray_miss_loss).  If a slot holds d_frame_id[0] its loss becomes
 *       max(L, old); otherwise slot n - 1 is overwritten with (d_frame_id[0], L) -- also when L == 0 or smaller than every entry, as the
 *       reference does.  Then the table is sorted by loss, descending and STABLE (equal losses keep their slot order; torch.sort leaves it open).
 *   n == 1 (prob_num_step == 1): d_losses[0] = max(L, d_losses[0]); d_ids is not touched and may be NULL.
 *   A non-finite L is written to d_miss_out and leaves the table as it was (the reference would carry the NaN into the table).
 *   d_miss_out [2] (may be NULL) = {L, number of missed rays}.  d_frame_id [1] is read on the device (frames.BatchSampler's frame_row).
 * Allocates nothing, reads nothing back, capturable.  HNR_ERR_BADARG, nothing written: n < 1, n > 1024, R < 0, R > 2^24, a NULL pointer other
 * than d_miss_out (and d_ids when n == 1). */
int hnr_ray_miss_rank(const float *d_color /*[R,3]*/, const float *d_gt /*[R,3]*/, const int8_t *d_ray_mask /*[R]*/, int R,
                      const int32_t *d_frame_id /*[1], device*/, int32_t *d_ids /*[n]*/, float *d_losses /*[n]*/, int n,
                      float *d_miss_out /*[2] or NULL: loss, number of missed rays*/, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Geometric-consistency filter of MVS depth maps: the `load_points=0`, `manual_depth_view=1` start of a scene (csrc/geo_filter.hip).  Replaces
 * models/mvs/filter_utils.py:157-297 (`reproject_with_depth_gpu`, `check_geometric_consistency_gpu`, `filter_by_masks_gpu`, `reassign_conf`) and
 * `range_mask_torch` (:146-154), called from run/train_ft.py:105-114: a Python double loop over the views with about 35 full-frame torch ops and
 * three matrix inverses per ordered pair.  Stream-ordered, nothing is allocated, nothing is read back, no atomics: two runs give the same bits.
 * Every fp32 operation below is rounded on its own, in the order written (divisions and the square root correctly rounded);
 * tests/geo_filter_ref.py restates them in NumPy and the GPU tests compare bits.  Depth maps must be finite.
 *
 * hnr_geo_consistency -- one launch for all reference views (workgroups of 32 x 8 pixels; grid z = the reference view).
 *   d_depth [V,H,W]; d_K, d_Kinv [V,3,3]; d_E (world to camera), d_Einv [V,4,4], row-major, on the device (the caller inverts, in fp32).
 *   For the reference view r, pixel (x, y) with d = depth[r][y][x], and every source view s != r in ASCENDING order:
 *     mat3(M, a)[c] = (M[c][0]*a0 + M[c][1]*a1) + M[c][2]*a2;         mat34(T, a)[c] = ((T[c][0]*a0 + T[c][1]*a1) + T[c][2]*a2) + T[c][3];
 *     pair(A, B)[i][j] = ((A[i][0]*B[0][j] + A[i][1]*B[1][j]) + A[i][2]*B[2][j]) + A[i][3]*B[3][j]   (rows 0..2; formed once per workgroup and pair)
 *     p  = mat3(Kinv_r, (x*d, y*d, d));      q  = mat34(pair(E_s, Einv_r), p);      k = mat3(K_s, q);     xs = k0 / k2,  ys = k1 / k2
 *     sd = bilinear sample of depth[s] at (xs, ys), border clamp (grid_sample(align_corners=True, padding_mode='border'), without the round trip
 *          through [-1, 1]):  cx = fmin(fmax(xs, 0), W-1) (a NaN becomes 0), x0 = floor(cx), wx1 = cx - x0, wx0 = (x0 + 1) - cx, likewise y;
 *          sd = (((wx0*wy0)*t00 + (wx1*wy0)*t01) + (wx0*wy1)*t10) + (wx1*wy1)*t11, t_ab = depth[s][min(y0+a, H-1)][min(x0+b, W-1)]
 *     p' = mat3(Kinv_s, (xs*sd, ys*sd, sd)); q' = mat34(pair(E_r, Einv_s), p');     k' = mat3(K_r, q');   xr = k'0 / k'2, yr = k'1 / k'2
 *     ex = xr - x, ey = yr - y;  dist = sqrt(ex*ex + ey*ey);  rel = |q'2 - d| / d;   ok = dist < 1 && rel < 0.01f   (inf / NaN fail both)
 *     count += ok;  sum += ok ? q'2 : 0
 *   d_count [V,H,W] int32 = count;  d_depth_avg [V,H,W] = (sum + d) / (float)(count + 1)   (V = 1: count 0, depth_avg = depth).
 *   HNR_ERR_BADARG, before any launch: a NULL pointer, V < 1 or > 65535, H or W outside 2 .. 32768, V*H*W > 2^30.
 *
 * hnr_geo_filter_select -- final mask, world points, range mask, confidence, ordered compaction (flags, one scan, scatter).
 *   keep = d_conf > conf_thresh && d_points_mask != 0 && (V == 1 || count >= geo_cnsst_num)
 *   cam = (d_cam_xyz[v][y][x][0], d_cam_xyz[v][y][x][1], depth_avg)   (x and y are NOT rescaled to the averaged depth: filter_utils.py:264-265)
 *   world = mat34(Einv_v, cam);  keep &&= ranges[0:3] <= world <= ranges[3:6] unless ranges[0] <= -99 (6 host floats)
 *   conf_table != NULL (opt.default_conf > 1: `reassign_conf`): conf *= conf_table[min(max(count - geo_cnsst_num + 1, 1), 10) - 1]; the caller
 *   computes the ten host floats 1 - 1 / 1.14869^k, k = 1..10, with the reference's own expression.
 *   The kept pixels of all views, views ascending, row-major inside a view (what train_ft.py:133-137 concatenates), go to d_world [capacity,3],
 *   d_cam [capacity,3], d_conf_out [capacity], d_view [capacity] int32.  d_view_counts [V] int64 = kept pixels per view, d_total[0] = their sum (also
 *   beyond capacity: then d_status[0] |= HNR_CLOUD_OVERFLOW -- the caller zeroes the word -- and nothing is written at or past row `capacity`).  d_cam_xyz [V,H,W,3], d_conf [V,H,W],
 *   d_points_mask [V,H,W] uint8.  d_scratch: hnr_geo_filter_select_scratch_bytes(V, H, W) bytes (negative: bad shape).
 *   HNR_ERR_BADARG, before any launch: a NULL pointer (conf_table aside), the shape limits above, capacity < 0, geo_cnsst_num < 0, short scratch. */
int hnr_geo_consistency(const float *d_depth, int V, int H, int W, const float *d_K, const float *d_Kinv, const float *d_E, const float *d_Einv,
                        int32_t *d_count, float *d_depth_avg, void *stream);
int64_t hnr_geo_filter_select_scratch_bytes(int V, int H, int W);
int hnr_geo_filter_select(const float *d_cam_xyz, const float *d_conf, const uint8_t *d_points_mask, const int32_t *d_count, const float *d_depth_avg,
                          int V, int H, int W, const float *d_Einv, float conf_thresh, int geo_cnsst_num, const float *ranges, const float *conf_table,
                          float *d_world, float *d_cam, float *d_conf_out, int32_t *d_view, int64_t capacity, int64_t *d_view_counts, int64_t *d_total,
                          int32_t *d_status, void *d_scratch, int64_t scratch_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Visual-hull masking and the occlusion test of the NeRF-synthetic start of a scene (csrc/hull.hip): `load_points=0`, `depth_occ=1`, a dataset with
 * `alphas` (dev_scripts/w_n360/chair_hybrid.sh, lego_hybrid.sh).  fp32, every operation rounded on its own in the order written; stream-ordered, nothing is allocated,
 * nothing is read back, no float atomics.  HNR_ERR_BADARG, before any launch, for a NULL pointer, a shape outside the limits given or a short scratch.
 *
 * hnr_alpha_pack -- d_alphas [M,H,W] float32 -> d_bits [M,H,Wp] uint32, Wp = (W + 31) / 32: bit (x & 31) of word x >> 5 of a row is alpha > 0.1f (a NaN:
 *   0); the padding bits of a row's last word are 0.  This is all hnr_visual_hull_select needs of an alpha map.  PRECONDITION: alpha >= -0.9 (dataset
 *   alphas are in [0, 1]): with the range mask on, the reference lets a point outside the frame pass because alpha + 1 > 0.1 whatever pixel the clamped
 *   lookup hits, and the kernel does not look.  1 <= M <= 65535, 1 <= H, W <= 32768, M*H < 2^31.
 *
 * hnr_visual_hull_select -- `alpha_masking` (models/mvs/mvs_utils.py:573-607) and the `masking` that follows it (run/train_ft.py:152-158) in one
 *   pass.  d_cams [M,21]: per view rows 0..2 of w2c (12 values, row-major) and K (9).  Per point (x, y, z) and view, views ascending:
 *     cam[q] = ((x*w[q][0] + y*w[q][1]) + z*w[q][2]) + w[q][3];   p[q] = (cam0*K[q][0] + cam1*K[q][1]) + cam2*K[q][2],  q = 0..2
 *     u = floor(p0 / p2), v = floor(p1 / p2)   (correctly rounded divides)
 *     near_far != NULL (two host floats: near - 1 -- formed by the caller in double and rounded to fp32 -- and far):  near - 1 <= cam[2] <= far
 *     range_mask != 0 (opt.alpha_range > 0 or opt.inall_img == 0):  a point with !(0 <= u < W && 0 <= v < H) passes this view
 *     otherwise the bit at (min(max(u, 0), W-1), min(max(v, 0), H-1)); the clamp is done in float before the conversion to int; a u or v that is not
 *     finite reads pixel 0 (the reference's value there is whatever the platform's float -> int64 conversion gives).
 *   A point survives when every view passes; the loop is left at the first failing view.  d_mask [n] uint8 (optional) = survives.  The survivors, in
 *   input order, go to d_out_xyz [capacity,3], d_out_conf [capacity] (from d_conf [n]) and d_out_view [capacity] int32 (from d_view [n]) -- each pair
 *   optional -- by flags, one inclusive scan and a scatter.  d_count[0] = the survivors, also beyond capacity: then d_status[0] |= HNR_CLOUD_OVERFLOW
 *   (the caller zeroes the word) and nothing is written at or past row `capacity`.  1 <= n <= 2^30, capacity >= 0;
 *   d_scratch: hnr_visual_hull_select_scratch_bytes(n) bytes (negative: n outside the limits).
 *
 * hnr_point_occlusion -- the z-buffer test of `homo_warp_nongrid_occ` (models/mvs/mvs_utils.py:333-369) for the n points of ONE view (w2c [4,4], K
 *   [3,3]: host floats).  cam, gx, gy and the frame mask 0 <= gx <= W-1 && 0 <= gy <= H-1 are those of hnr_point_view_attrs, bit for bit (the
 *   reference's `ceil(gx) <= W-1` is the same test).  cell = ceil(gx) * H + ceil(gy), the reference's column-major index; zmin[cell] = the minimum of
 *   cam[2] over the in-frame points of the cell (an integer atomicMin on an order-preserving key of the float: negative depths are legal, and the
 *   result does not depend on the order of arrival);  d_visible [n] uint8 = in frame && cam[2] <= zmin[cell] + tolerate (one fp32 sum; the reference
 *   passes tolerate = 0.1).  n > 0, 2 <= H, W <= 32768, H*W <= 2^24 (the reference forms the cell index in fp32), tolerate >= 0;
 *   d_scratch: hnr_point_occlusion_scratch_bytes(H, W) bytes (negative: bad shape). */
int hnr_alpha_pack(const float *d_alphas, int M, int H, int W, uint32_t *d_bits, void *stream);
int64_t hnr_visual_hull_select_scratch_bytes(int64_t n);
int hnr_visual_hull_select(const float *d_xyz, const float *d_conf, const int32_t *d_view, int64_t n, const uint32_t *d_alpha_bits, const float *d_cams,
                           int M, int H, int W, const float *near_far, int range_mask, uint8_t *d_mask, float *d_out_xyz, float *d_out_conf,
                           int32_t *d_out_view, int64_t capacity, int64_t *d_count, int32_t *d_status, void *d_scratch, int64_t scratch_bytes,
                           void *stream);
int64_t hnr_point_occlusion_scratch_bytes(int H, int W);
int hnr_point_occlusion(const float *d_xyz, int64_t n, const float *w2c, const float *K, int H, int W, float tolerate, uint8_t *d_visible,
                        void *d_scratch, int64_t scratch_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Depth maps from the pretrained MVSNet: the first stage of the `load_points=0`, `manual_depth_view=1` start of a scene (csrc/mvsnet.hip).  Replaces
 * models/depth_estimators/mvsnet.py (`MVSNet(refine=False)` in eval mode, loaded by `MvsPointsModel.load_pretrained_d_est`) and the tail of
 * `MvsPointsModel.gen_points` (models/mvs/mvs_points_model.py:300-341).  Inference only.  All arithmetic is fp32, every intended fused multiply-add is
 * an explicit one, every sum has a fixed order: two runs give the same bits.  Stream-ordered, nothing is allocated, nothing is read back, no atomics.
 * A batch norm is y = (x - running_mean) * mul + bias with mul = weight * rsqrt(running_var + 1e-5), folded by whoever packs (plain BatchNorm: no
 * |weight|, eps on the variance only).  HNR_ERR_BADARG, before any launch, for a NULL pointer, a shape outside the limits given or a short scratch.
 *
 * hnr_mvsnet_feature -- `FeatureNet`, mvsnet.py:7-27: conv + BatchNorm2d + ReLU 3->8, 8->8 (3x3), 8->16 (5x5, stride 2), 16->16, 16->16 (3x3), 16->32
 *   (5x5, stride 2), 32->32 (3x3), pad = kernel / 2, no bias; then `feature`: 3x3, 32->32, with bias, no norm, no activation.
 *   d_images [V,3,H,W] -> d_feat [V,32,h,w], h = ((H-1)/2+1-1)/2+1 (integer division), likewise w.  Direct convolution, one chain of fmaf per output
 *   over (input channel, ky, kx).  d_packed [HNR_MVSNET_FEATURE_PACKED_ELEMS]: per ConvBnReLU, in network order, w [cin][ky][kx][cout], running_mean
 *   [cout], mul [cout], bias [cout]; then `feature`: w [cin][ky][kx][cout], bias [cout].  d_scratch: hnr_mvsnet_feature_scratch_elems(V, H, W) floats
 *   (negative: bad shape).  1 <= V <= 64, 4 <= H, W <= 32768.
 *
 * hnr_mvsnet_cost_volume -- mvsnet.py:109-122 with `homo_warping` (module.py:36-70), one reference view: d_volume [32,D,h,w] =
 *   sum_v f_v^2 / V - (sum_v f_v / V)^2, views ascending, f_v the bilinear sample of d_feat[v] [32,h,w] at the projection of (x, y, depth d_k):
 *     P = d_proj[v] [3,4] (device, row-major): r = (P[c][0]*x + P[c][1]*y) + P[c][2];  q[c] = r[c]*d_k + P[c][3];  px = q0/q2, py = q1/q2;
 *     gx = px / ((w-1)/2) - 1, gy = py / ((h-1)/2) - 1   (the align_corners=True normalisation) ...
 *     ix = ((gx+1)*w - 1)/2, iy = ((gy+1)*h - 1)/2       (... undone as grid_sample's default align_corners=False does: the reference's mismatch,
 *                                                         kept; it moves every sample, the identity view's included)
 *     x0 = floor(ix), y0 = floor(iy); f = (((x0+1-ix)*(y0+1-iy))*t00 + ((ix-x0)*(y0+1-iy))*t01 + ((x0+1-ix)*(iy-y0))*t10) + ((ix-x0)*(iy-y0))*t11,
 *     a tap outside the map is zero; a coordinate that is not finite or not inside (-1, w) x (-1, h) reads nothing and contributes zero.
 *   d_depth_values [D].  1 <= V <= 64, 2 <= h, w <= 8192, 1 <= D <= 4096, D*h*w <= 2^26.
 *
 * hnr_mvsnet_cost_reg -- `CostRegNet`, mvsnet.py:30-70: d_volume [32,D,h,w] -> d_logits [D,h,w].  ConvBnReLU3D 32->8, 8->16 (stride 2), 16->16, 16->32
 *   (stride 2), 32->32, 32->64 (stride 2), 64->64 (3x3x3, pad 1, no bias); ConvTranspose3d (3x3x3, stride 2, pad 1, output_padding 1, no bias) +
 *   BatchNorm3d + ReLU 64->32, 32->16, 16->8, each followed by `skip + y` (the skip is added after the activation); `prob`: 3x3x3, 8->1, with bias.
 *   Direct convolution; a transposed convolution is a gather over the output voxel's parity class (1, 2, 4 or 8 taps per input channel); one chain
 *   of fmaf per output over (input channel, kz, ky, kx).  D, h and w must be multiples of 8 (the skips do not line up otherwise: HNR_ERR_BADARG).
 *   d_packed [HNR_MVSNET_REG_PACKED_ELEMS]: the ten normed layers in network order (conv0 .. conv6, conv7, conv9, conv11), each w [cin][kz][ky][kx][cout],
 *   running_mean [cout], mul [cout], bias [cout]; then `prob`: w [cin][kz][ky][kx], bias [1].  d_scratch: hnr_mvsnet_cost_reg_scratch_elems(D, h, w)
 *   floats (negative: bad shape).  Limits as for the cost volume.
 *
 * hnr_mvsnet_depth_head -- mvsnet.py:126-136, one thread per pixel: m = max_k logit_k, e_k = exp(logit_k - m), S = sum_k e_k (k ascending);
 *   d_depth [h,w] = (sum_k e_k d_k) / S;  i = (sum_k e_k k) / S, idx = (int) i (truncation);  d_conf [h,w] = sum_{k = idx-1 .. idx+2, 0 <= k < D} e_k / S
 *   (the reference's 4 * avg_pool3d over the pad (1, 2), gathered at idx);  d_prob [D,h,w] (optional, NULL: not written) = e_k / S.
 *
 * hnr_mvsnet_depth_points -- mvs_points_model.py:329-337 with manual_std_depth = 0 (`gau_single_sampler`, `depth2point`, mvs_utils.ndc_2_cam):
 *   d = d_depth[sy][sx], sy = min((int)floor(y * ((float)h / H)), h-1), sx likewise (torch's `nearest`);  d_mask [H,W] = near <= d && d <= far;
 *   z = min(max((d - near) / (far - near), 0), 1);  cz = z * (far - near) + near;  cx = ((x / (W-1)) * (W-1)) * cz, cy likewise;
 *   d_cam_xyz [H,W,3][j] = (cx*M[0][j] + cy*M[1][j]) + cz*M[2][j], M = Kt_inv = inverse(K^T) [3,3], host floats (the caller inverts, in fp32);
 *   d_conf_out [H,W] = d_conf[sy][sx].  2 <= H, W <= 32768, 1 <= h <= H, 1 <= w <= W. */
#define HNR_MVSNET_FEATURE_PACKED_ELEMS 40248
#define HNR_MVSNET_REG_PACKED_ELEMS 298297
int64_t hnr_mvsnet_feature_scratch_elems(int V, int H, int W);
int hnr_mvsnet_feature(const float *d_images, int V, int H, int W, const float *d_packed, float *d_feat, float *d_scratch, int64_t scratch_elems,
                       void *stream);
int hnr_mvsnet_cost_volume(const float *d_feat, int V, int h, int w, const float *d_proj, const float *d_depth_values, int D, float *d_volume,
                           void *stream);
int64_t hnr_mvsnet_cost_reg_scratch_elems(int D, int h, int w);
int hnr_mvsnet_cost_reg(const float *d_volume, int D, int h, int w, const float *d_packed, float *d_logits, float *d_scratch, int64_t scratch_elems,
                        void *stream);
int hnr_mvsnet_depth_head(const float *d_logits, const float *d_depth_values, int D, int h, int w, float *d_depth, float *d_conf, float *d_prob,
                          void *stream);
int hnr_mvsnet_depth_points(const float *d_depth, const float *d_conf, int h, int w, int H, int W, float near, float far, const float *Kt_inv,
                            float *d_cam_xyz, float *d_conf_out, uint8_t *d_mask, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Content-aware frame weights (`frame_weights_step5/<scene>_frame_weight_step5.npy`, read at data/scannet_ft_dataset.py:502): RAFT optical flow between
 * consecutive training frames (csrc/raft.hip) and Laplacian-variance blur scores on the flow-aligned overlap (csrc/blur_score.hip).  Replaces
 * raft/demo_content_aware_weights.py:78-184 with raft/core/raft.py, extractor.py, corr.py, update.py, utils/utils.py for the configuration that script
 * runs: the basic model, fp32, eval, test_mode=True, flow_init=None, CorrBlock (radius 4, 4 levels).  Stream-ordered, nothing is allocated, nothing is
 * read back, no float atomics, every sum in a fixed order: two runs give the same bits.  Maps are NCHW.  Every convolution is an implicit GEMM on the
 * f32-input MFMA (a k-ordered fmaf chain per wave; four waves split the input channels of a tile and are added in wave order).
 * Shapes: H, W multiples of 8, 128 .. 4096, h = H/8, w = W/8 with h*w <= 16384 (h, w >= 16: below it the coarsest correlation level has extent 1 and
 * the reference divides by W-1 = 0).  HNR_ERR_BADARG, before any launch, for a NULL pointer, a shape outside these limits or a short scratch.
 *
 * Packed layer (whoever packs folds batch norms and constant factors): w [kh*kw][cinp][cout], cinp = cin rounded up to even (the added row zero),
 *   then bias [cout].  hnr_raft_encoder_packed_elems(): conv1 (7x7, 3->64), then per residual block (64, 64, 96/2, 96, 128/2, 128) conv1, conv2 and, at
 *   stride 2, downsample.0; then conv2 (1x1, 128->256).  hnr_raft_update_packed_elems(): encoder.convc1, convc2, convf1, convf2, conv;
 *   gru.[convz1 | convr1] stacked along cout, convq1, [convz2 | convr2], convq2; flow_head.conv1, conv2; mask.0, 0.25 * mask.2.
 *
 * STAGE tier:
 * hnr_raft_encoder -- `BasicEncoder` (extractor.py:118-192) on d_images [N,3,H,W] (N = 1 or 2; values 0..255: 2(x/255) - 1 is applied here) ->
 *   d_out [N,256,h,w].  norm 0: InstanceNorm2d as constructed there (no affine, no running statistics, eps 1e-5, biased variance, per image and
 *   channel; mean, then the squared deviations, each a strided per-thread sum and an LDS tree);  1: batch norm folded into the packed layers;
 *   2: as 1, then tanh on channels 0..127 and relu on 128..255 (raft.py:111-114: net | inp).
 * hnr_raft_corr_pyramid -- `CorrBlock.__init__` (corr.py:13-27, 53-60): level 0 [h*w][h][w] = fmap1^T fmap2 / 16, then three avg_pool2d(2, 2) (floor on
 *   odd extents), the four levels one after another in d_pyramid [hnr_raft_pyramid_elems(h, w)].
 * hnr_raft_lookup -- `CorrBlock.__call__` (corr.py:29-50) with utils.bilinear_sampler: d_coords [2,h,w] (x, y) -> d_corr [324,h,w]; window index (i, j),
 *   i, j = 0..8: tap x = cx/2^l + (i-4), y = cy/2^l + (j-4) (the reference adds meshgrid(dy, dx) to (x, y)), channel l*81 + i*9 + j; the coordinate
 *   goes through 2v/(W-1) - 1 and back ((g+1)/2)(W-1); bilinear with grid_sample's weight expressions, zero outside.
 * hnr_raft_update -- one iteration of raft.py:122-131 with `BasicUpdateBlock` (update.py:79-136): lookup at d_coords, flow = coords - grid, motion
 *   encoder, SepConvGRU (sigmoid, r*h, tanh and (1-z)h + zq in the convolutions' epilogues; h, inp and the motion features read in place), flow
 *   head, d_coords += delta.  d_net [128,h,w] and d_coords [2,h,w] are updated in place; d_delta [2,h,w] (optional) receives delta_flow; d_mask
 *   [576,h,w] (optional: NULL skips the mask head, which only the last iteration's up-sampling reads) receives 0.25 * mask(net).
 * hnr_raft_upsample -- `upsample_flow` (raft.py:72-83): softmax over the 9 taps of d_mask [9][8][8][h][w], 3x3 unfold of 8 * d_flow [2,h,w] with zero
 *   padding -> d_flow_up [2,8h,8w].
 * hnr_blur_edges -- `detect_blurry` (demo_content_aware_weights.py:78-92) on P grey planes d_gray [P,H,W] uint8 -> d_edges [P,H,W] fp64:
 *   cv2.blur(., (5, 5)) = the 25 taps (an exact integer) * (1/25), then cv2.Laplacian(., CV_64F) = aperture [[0,1,0],[1,-4,1],[0,1,0]], summed
 *   ((up + left) + right) + down - 4 centre; BORDER_REFLECT_101 for both, as OpenCV documents them.  8 <= H, W <= 16384.
 *
 * STABLE tier:
 * hnr_raft_flow -- `RAFT.forward(image1, image2, iters, test_mode=True)`: d_image1 [2,3,H,W] holds both images (d_image2 = d_image1 + 3*H*W),
 *   d_fnet / d_cnet / d_update the packed images above -> d_flow_low [2,h,w] = coords1 - coords0, d_flow_up [2,H,W].  1 <= iters <= 1024.
 * hnr_blur_score_pair -- demo_content_aware_weights.py:147-184 for one pair: d_edge1, d_edge2 [H,W] fp64, d_flow [2,H,W] (flow_up) -> d_row [3] fp64
 *   = (population variance of edge 1, of the warped edge 2, used-pixel count).  Warp: `warp(., flow, mode='nearest')` as torch evaluates it, in
 *   separately rounded fp32 operations: v = x + fx;  g = 2 v / max(W-1, 1) - 1;  i = ((g + 1) W - 1) / 2 (grid_sample without align_corners);
 *   round half to even; outside the frame: 0.  Edge 2 is rounded to fp32 before the warp, as the script does.  A pixel is used where it lies inside
 *   the frame minus `border` pixels on every side and its pick does too.  Sums in fp64: mean first, then squared deviations.  A count of 0 gives the
 *   row (0, 0, 0).  d_pick [H,W] int32 (optional): the picked pixel's index or -1;  d_used [H,W] uint8 (optional).  d_scratch: 8-byte aligned,
 *   hnr_blur_score_pair_scratch_bytes(H, W).  0 <= 2*border < min(H, W). */
int64_t hnr_raft_encoder_packed_elems(void);
int64_t hnr_raft_update_packed_elems(void);
int64_t hnr_raft_encoder_scratch_elems(int N, int H, int W);
int hnr_raft_encoder(const float *d_images, int N, int H, int W, const float *d_packed, int norm, float *d_out, float *d_scratch, int64_t scratch_elems,
                     void *stream);
int64_t hnr_raft_pyramid_elems(int h, int w);
int64_t hnr_raft_pyramid_scratch_elems(int h, int w);
int hnr_raft_corr_pyramid(const float *d_fmap1, const float *d_fmap2, int h, int w, float *d_pyramid, float *d_scratch, int64_t scratch_elems,
                          void *stream);
int hnr_raft_lookup(const float *d_pyramid, const float *d_coords, int h, int w, float *d_corr, void *stream);
int64_t hnr_raft_update_scratch_elems(int h, int w);
int hnr_raft_update(const float *d_packed, const float *d_pyramid, float *d_net, const float *d_inp, float *d_coords, int h, int w, float *d_delta,
                    float *d_mask, float *d_scratch, int64_t scratch_elems, void *stream);
int hnr_raft_upsample(const float *d_flow, const float *d_mask, int h, int w, float *d_flow_up, void *stream);
int64_t hnr_raft_flow_scratch_elems(int H, int W);
int hnr_raft_flow(const float *d_image1, const float *d_image2, int H, int W, const float *d_fnet, const float *d_cnet, const float *d_update, int iters,
                  float *d_flow_low, float *d_flow_up, float *d_scratch, int64_t scratch_elems, void *stream);
int hnr_blur_edges(const uint8_t *d_gray, int P, int H, int W, double *d_edges, void *stream);
int64_t hnr_blur_score_pair_scratch_bytes(int H, int W);
int hnr_blur_score_pair(const double *d_edge1, const double *d_edge2, const float *d_flow, int H, int W, int border, double *d_row, int32_t *d_pick,
                        uint8_t *d_used, void *d_scratch, int64_t scratch_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * LPIPS v0.1 with the AlexNet and the VGG-16 backbone (csrc/lpips.hip): the `lpips` and `vgglpips` columns of report_metrics (run/evaluate.py:41-75,
 * called at run/test_ft.py:260 and run/train_ft.py:437).  Replaces `lpips.LPIPS(net=..., version='0.1')` in eval mode with the package's defaults
 * (lpips=True, spatial=False) and torchvision's `alexnet().features` / `vgg16().features[0:30]`, which evaluate.py runs on PNGs it reads back from
 * disk.  fp32, inference only.  Stream-ordered, nothing is allocated, nothing is read back, no float atomics, every sum in a fixed order: two runs
 * give the same bits.  net: 0 alex, 1 vgg.  Sizes: alex 31 <= h, w <= 4096, vgg 16 <= h, w <= 4096 (below the minimum the last tap has no pixel).
 * HNR_ERR_BADARG, before any launch, for an unknown net, a NULL pointer, a size outside these limits, a d_packed or d_scratch that is not 16-byte
 * aligned, or a short scratch.
 *
 * d_packed [hnr_lpips_packed_elems(net)] floats: ScalingLayer shift [3], scale [3], two zeros; the convolutions in network order, each
 *   w [k*k][cinp][cout] (cinp = cin rounded up to even, the added row zero) then bias [cout]; then the five `lin` layers, [C_k] each.
 *   alex: 3->64 k11 s4 p2 | 64->192 k5 p2 | 192->384 k3 p1 | 384->256 k3 p1 | 256->256 k3 p1, a 3x3/s2 max-pool after the first two; taps after each ReLU.
 *   vgg: thirteen k3 p1 layers 64 64 | 128 128 | 256 256 256 | 512 512 512 | 512 512 512, a 2x2/s2 max-pool between the blocks; taps relu1_2 .. relu5_3.
 * d_scratch: hnr_lpips_scratch_bytes(net, h, w) bytes (negative: bad net or size), the same for every entry below.
 *
 * STAGE tier:
 * hnr_lpips_tap_dims -- dims [5][3] (host) = (C_k, h_k, w_k) of the five taps.
 * hnr_lpips_prepare -- what evaluate.py feeds the network: two [h,w,3] uint8 RGB images -> d_x [2,3,h,w]; per channel float32(b) / 255.0, * 2 - 1.0,
 *   then the ScalingLayer (x - shift) / scale: four separately rounded fp32 operations (a 256-entry table per channel).  bgr != 0: network channel c
 *   reads byte 2 - c (cv2.imread hands evaluate.py BGR and nothing converts it: the published numbers are these).  hnr_lpips_prepare_f32: two float
 *   [3,h,w] images in [-1, 1], channels as given -> the ScalingLayer alone (the package's forward(in0, in1)).
 * hnr_lpips_features -- d_x -> the five taps, d_taps: host array of five device pointers, tap k [2,C_k,h_k,w_k].  Convolution + bias + ReLU is an
 *   implicit GEMM on the f32-input MFMA: one k-ordered chain per output element (input-channel chunk, tap, channel pair), no split sums.
 * hnr_lpips_score -- the five taps -> d_row [6] fp64 = (d, r_0 .. r_4): per pixel n = sqrt(sum_c f^2), g = f / (n + 1e-10),
 *   s = sum_c lin_k[c] (g0 - g1)^2, every term the package's fp32 expression (not the expanded form), the sums over c and the mean r_k of s over
 *   the pixels collected in fp64 in a fixed order; d = sum_k r_k.
 *   Identical taps give exactly 0; a pixel whose features are all zero contributes 0.
 *
 * STABLE tier:
 * hnr_lpips -- prepare, features, score for one pair of 8-bit images (those hnr_frame_metrics leaves) -> d_row [6] fp64.  hnr_lpips_f32: the same
 *   from float images. */
int64_t hnr_lpips_packed_elems(int net);
int64_t hnr_lpips_scratch_bytes(int net, int h, int w);
int hnr_lpips_tap_dims(int net, int h, int w, int *dims);
int hnr_lpips_prepare(const uint8_t *d_img8, const uint8_t *d_gt8, int h, int w, int bgr, const float *d_packed, float *d_x, void *stream);
int hnr_lpips_prepare_f32(const float *d_in0, const float *d_in1, int h, int w, const float *d_packed, float *d_x, void *stream);
int hnr_lpips_features(int net, const float *d_x, int h, int w, const float *d_packed, float *const *d_taps, void *d_scratch, int64_t scratch_bytes,
                       void *stream);
int hnr_lpips_score(int net, const float *const *d_taps, int h, int w, const float *d_packed, double *d_row, void *d_scratch, int64_t scratch_bytes,
                    void *stream);
int hnr_lpips(int net, const uint8_t *d_img8, const uint8_t *d_gt8, int h, int w, int bgr, const float *d_packed, double *d_row, void *d_scratch,
              int64_t scratch_bytes, void *stream);
int hnr_lpips_f32(int net, const float *d_in0, const float *d_in1, int h, int w, const float *d_packed, double *d_row, void *d_scratch,
                  int64_t scratch_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * The optimiser step (csrc/adam.hip): Adam for every tensor of up to HNR_ADAM_MAX_GROUPS parameter groups in ONE launch, behind one single-thread
 * launch that advances the counters and evaluates the learning-rate schedule.  Replaces `self.optimizer.step()` and
 * `self.neural_point_optimizer.step()` of MvsPointsVolumetricModel.backward (models/mvs_points_volumetric_model.py:111-131; both built by
 * setup_optimizer, :94-104: torch.optim.Adam, betas (0.9, 0.999), no weight decay, no amsgrad) and `scheduler.step()` of
 * BaseModel.update_learning_rate (models/base_model.py:148-150) for lr_policy 'iter_exponential_decay' (models/helpers/networks.py:56-61:
 * LambdaLR, lambda_rule(it) = pow(lr_decay_exp, it / lr_decay_iters)).  Stream-ordered; no host value enters a step, nothing is allocated, nothing
 * is read back, no atomics: the launches can be captured in a graph that serves every step, and two runs give the same bits.
 *
 * State the caller owns, all in device memory:
 *   d_counters [2] int64 = {adam_step, sched_it}: Adam's bias-correction count (torch's state['step']) and the schedule's iteration (the number
 *     of scheduler.step() calls so far: iteration n, 1-based, runs with sched_it = n - 1; init_scheduler(total_steps) sets it to total_steps).
 *   d_groups [n_groups][HNR_ADAM_GROUP_DOUBLES] fp64 = {lr0, beta1, beta2, eps, decay_exp, decay_iters} (decay_exp 1, decay_iters 1: constant lr).
 *   d_rows [n_groups][HNR_ADAM_ROW_DOUBLES] fp64, written by the tick = {lr_t, bc1, bc2, lr_t / bc1, sqrt(bc2), 1 - beta1, 1 - beta2, beta2, eps,
 *     step} with lr_t = lr0 * decay_exp^(sched_it_before / decay_iters), bc1 = 1 - beta1^step, bc2 = 1 - beta2^step, step = adam_step after
 *     the increment.
 *   d_tensors [n_tensors] hnr_adam_tensor: parameter, gradient, first and second moment (4-byte aligned, n elements each, not overlapping) and
 *     the tensor's group.  d_chunks [n_chunks][2] int32 = (tensor, chunk within the tensor): one workgroup per HNR_ADAM_CHUNK elements.
 *
 * Element arithmetic: fp32, every operation rounded on its own, divide and sqrt correctly rounded, in the order of torch's _single_tensor_adam;
 * the six scalars are rounded to fp32 once from the fp64 row:
 *     w1 = f32(1 - beta1)  w2 = f32(1 - beta2)  b2 = f32(beta2)  e = f32(eps)  ss = f32(lr_t / bc1)  bs = f32(sqrt(bc2))
 *     m' = m + w1 * (g - m);   v' = (v * b2) + ((w2 * g) * g);   den = (sqrt(v') / bs) + e;   p' = p - ss * (m' / den)
 * Every element is updated, zero gradient or not (Adam's momentum moves it); an element with m = v = g = 0 keeps its bits.  Subnormal
 * intermediates are kept; NaN / inf gradients propagate into m, v and p, as in torch.  16 bytes per lane where p, g, m, v of a tensor are all
 * 16-byte aligned, 4 bytes per lane otherwise.
 *
 * hnr_adam_plan -- HOST only: checks a host copy of the tensor table (HNR_ERR_BADARG for a NULL or misaligned pointer, a negative count, a group
 *   outside [0, n_groups)) and returns the number of chunks; with `chunks` != NULL it also writes the table (chunk_cap entries of two int32).
 *   Upload both tables once; they change only when a pointer does.
 * hnr_adam_step -- the tick launch (counters and rows), then the update launch (reads the tables and d_rows only): one optimiser step; every
 *   argument is checked before the first launch.
 * HNR_ERR_BADARG, before any launch, for a NULL or misaligned pointer, n_groups outside 1..HNR_ADAM_MAX_GROUPS, n_tensors outside
 * 1..HNR_ADAM_MAX_TENSORS or a negative n_chunks. */
#define HNR_ADAM_MAX_GROUPS     4
#define HNR_ADAM_MAX_TENSORS    4096
#define HNR_ADAM_CHUNK          4096
#define HNR_ADAM_GROUP_DOUBLES  6
#define HNR_ADAM_ROW_DOUBLES    10
typedef struct {
    float *p;
    const float *g;
    float *m;
    float *v;
    int64_t n;
    int32_t group;
    int32_t reserved;
} hnr_adam_tensor;
int64_t hnr_adam_plan(const hnr_adam_tensor *tensors, int n_tensors, int n_groups, int32_t *chunks, int64_t chunk_cap);
int hnr_adam_step(int64_t *d_counters, const double *d_groups, int n_groups, double *d_rows, const hnr_adam_tensor *d_tensors, int n_tensors,
                  const int32_t *d_chunks, int64_t n_chunks, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HNR_H */
