"""ctypes binding of libhnr_hip.so (the C ABI declared in include/hnr.h).

There is NO fallback: if the HIP library is missing or a call fails, this raises.  PyTorch only
supplies device memory (`tensor.data_ptr()`) and the current HIP stream.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# HNR_LIB_PATH: another build of the same library (A/B timing of kernel changes); there is no other fallback
LIB_PATH = os.environ.get("HNR_LIB_PATH") or os.path.join(_HERE, "libhnr_hip.so")
NCOUNTS = 9
FEATNET_PACKED_ELEMS = 41368           # HNR_FEATNET_PACKED_ELEMS
PREMLP_PACKED_ELEMS = 3104             # HNR_PREMLP_PACKED_ELEMS
PATH_SCRATCH_BYTES = 512               # HNR_PATH_SCRATCH_BYTES
RESIZE_TILE_W, RESIZE_TILE_H, RESIZE_LDS_BUDGET = 64, 16, 65536       # HNR_RESIZE_TILE_W, HNR_RESIZE_TILE_H, HNR_RESIZE_LDS_BUDGET
RESIZE_FILTERS = dict(box=0, bilinear=1, hamming=2, bicubic=3, lanczos=4)         # HNR_RESIZE_BOX .. HNR_RESIZE_LANCZOS
RESIZE_FORMS = dict(auto=0, fused=1, two_pass=2)                                  # HNR_RESIZE_AUTO .. HNR_RESIZE_TWO_PASS
MVSNET_FEATURE_PACKED_ELEMS = 40248    # HNR_MVSNET_FEATURE_PACKED_ELEMS
MVSNET_REG_PACKED_ELEMS = 298297       # HNR_MVSNET_REG_PACKED_ELEMS
CNT = dict(RAYS_HIT=0, SAMPLES=1, RAYS_VALID=2, NEIGHBOURS=3, CELLS_VISITED=4, CANDIDATES=5, SAMPLES_VALID=6, SAMPLES_SMALL=7, SAMPLES_TINY=8)


class HnrError(RuntimeError):
    pass


class GridParams(ctypes.Structure):
    _fields_ = [("origin", ctypes.c_float * 3), ("cell", ctypes.c_float * 3), ("dims", ctypes.c_int * 3),
                ("query_size", ctypes.c_int * 3), ("P", ctypes.c_int), ("max_o", ctypes.c_int)]


class GridStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in ("n_points", "n_inbounds", "n_occ", "n_dropped_voxels",
                                              "n_cells_over_P", "n_dilated", "n_words", "bytes")]


class QueryParams(ctypes.Structure):
    _fields_ = [("R", ctypes.c_int), ("D", ctypes.c_int), ("SR", ctypes.c_int), ("K", ctypes.c_int),
                ("kernel_size", ctypes.c_int * 3), ("radius2", ctypes.c_float), ("tmid_stride", ctypes.c_int),
                ("pad_outputs", ctypes.c_int), ("knn_order", ctypes.c_int)]


_P = ctypes.c_void_p
_I = ctypes.c_int
_F = ctypes.c_float


class RenderParams(ctypes.Structure):
    _fields_ = [("R", _I), ("SR", _I), ("K", _I), ("D", _I), ("tmid_stride", _I), ("kernel_size", _I * 3), ("radius2", _F), ("vsize_z", _F),
                ("raydist_mode_unit", _I), ("V", _I), ("cap_samples", _I), ("knn_order", _I)]


class RenderCloud(ctypes.Structure):
    _fields_ = [("d_xyz", _P), ("d_conf", _P), ("d_dir", _P), ("d_color", _P), ("d_point_table", _P), ("ldt", _I), ("d_rec", _P),
                ("d_part", _P), ("d_part_rot", _P), ("n_parts", _I), ("rec_parts", _I)]        # per-point rotations (an edited scene); zero: none


class RenderWeights(ctypes.Structure):
    _fields_ = [("d_chain", _P), ("d_mlp_cf", _P), ("d_mlp_mw", _P), ("d_mlp_mx", _P),
                ("d_mw_last_w", _P), ("d_mw_last_b", _P), ("d_fin_w", _P), ("d_fin_b", _P), ("slope", _F)]


class RenderCamera(ctypes.Structure):
    _fields_ = [("d_campos", _P), ("d_camrot", _P), ("d_raydir", _P), ("d_tmid", _P), ("d_bg_color", _P)]


class RenderViews(ctypes.Structure):
    _fields_ = [("d_w2c", _P), ("d_intrinsic", _P), ("d_campos_nearest", _P), ("d_featmap", _P), ("H", _I), ("W", _I), ("d_frame_w", _P), ("featmap_ready", _P)]


class RenderOutputs(ctypes.Structure):
    _fields_ = [("d_raycolor", _P), ("d_opacity", _P), ("d_is_background", _P), ("d_blend_weight", _P), ("d_ray_mask", _P), ("d_decoded", _P),
                ("d_sample_pidx", _P), ("d_sample_loc_w", _P), ("d_ray_nsamp", _P), ("d_counts", _P), ("d_status", _P), ("d_weight", _P),
                ("d_conf_coefficient", _P), ("stage_events", ctypes.POINTER(_P))]


class TrainParams(ctypes.Structure):
    _fields_ = [("R", _I), ("SR", _I), ("K", _I), ("D", _I), ("tmid_stride", _I), ("kernel_size", _I * 3), ("radius2", _F), ("vsize_z", _F),
                ("raydist_mode_unit", _I), ("V", _I), ("H", _I), ("W", _I), ("n_points", _I), ("cap_samples", _I), ("knn_order", _I), ("slope", _F)]


class TrainCloud(ctypes.Structure):
    _fields_ = [("d_xyz", _P), ("d_emb", _P), ("d_conf", _P), ("d_dir", _P), ("d_color", _P)]


class TrainCloudGrads(ctypes.Structure):
    _fields_ = [("d_emb", _P), ("d_conf", _P), ("d_dir", _P), ("d_color", _P)]


# hnr_train_weights in struct order (include/hnr.h): (field stem, the reference's PointAggregator layer -- a string: one pointer; a list: an array of them);
# every stem is two fields, `_w` (the layers' .weight) and then `_b` (their .bias)
_TRAIN_LAYERS = (("block1_0", "block1.0"), ("block1_2", "block1.2"), ("block3_0", "block3.0"), ("block3_2", "block3.2"), ("alpha", "alpha_branch.0"),
                 ("cf", ["color_feature_branch.%d" % l for l in (0, 2, 4)]), ("mw", ["aux_merge_weight_block.%d" % l for l in (0, 2, 4, 6)]),
                 ("mx", ["color_mixup_block.%d" % l for l in (0, 2, 4)]), ("fin", "color_final_block.0"),
                 ("conv", ["aux_block_s%d.%d" % (s, l) for s in (1, 2, 3) for l in (0, 2)]))
# (struct field, parameter name or list of parameter names), the one table train._SLOTS and torch_ops.TRAIN_WEIGHT_NAMES are read from
TRAIN_WEIGHTS = tuple((stem + f, layer + p if isinstance(layer, str) else [l + p for l in layer]) for stem, layer in _TRAIN_LAYERS for f, p in (("_w", ".weight"), ("_b", ".bias")))


class TrainWeights(ctypes.Structure):
    """hnr_train_weights: raw parameter pointers under the reference's names; the gradient block has the same layout."""
    _fields_ = [(f, _P if isinstance(names, str) else _P * len(names)) for f, names in TRAIN_WEIGHTS]


class TrainViews(ctypes.Structure):
    _fields_ = [("d_w2c", _P), ("d_intrinsic", _P), ("d_campos_nearest", _P), ("d_images", _P), ("d_frame_w", _P)]


class FrameBankC(ctypes.Structure):
    """hnr_frame_bank"""
    _fields_ = [("d_images", _P), ("d_c2w", _P), ("d_w2c", _P), ("d_intrinsic", _P), ("d_weight", _P), ("d_angle", _P), ("images_f32", _I), ("F", _I),
                ("H", _I), ("W", _I), ("intrinsic_per_frame", _I)]


class FrameBatchParams(ctypes.Structure):
    _fields_ = [(n, _I) for n in ("mode", "size", "patch_num", "patch_size", "dilation_lo", "dilation_hi", "margin", "dir_norm", "bg_random",
                                  "downweight_blurry_feats")] + [("bg_color", _F * 3), ("seed", ctypes.c_uint64)]


FRAME_OUTPUTS = ("raydir", "pixel_idx", "gt_image", "campos", "camrot", "c2w", "intrinsic", "c2w_nearest", "w2c_nearest", "campos_nearest", "intrinsic_nearest",
                 "images_nearest", "frame_weight_nearest", "vid_angle_nearest", "frame_weight", "bg_color", "frame_row", "patch_table")


class FrameBatchOut(ctypes.Structure):
    _fields_ = [("d_" + n, _P) for n in FRAME_OUTPUTS]


class DepthBankC(ctypes.Structure):
    """hnr_depth_bank"""
    _fields_ = [("d_depth", _P), ("d_depth_intrinsic", _P), ("depth_f32", _I), ("F", _I), ("Hd", _I), ("Wd", _I), ("depth_div", _F), ("depth_min", _F),
                ("depth_max", _F)]


ADAM_MAX_GROUPS, ADAM_MAX_TENSORS, ADAM_CHUNK, ADAM_GROUP_DOUBLES, ADAM_ROW_DOUBLES = 4, 4096, 4096, 6, 10     # HNR_ADAM_*


class AdamTensor(ctypes.Structure):
    """hnr_adam_tensor"""
    _fields_ = [("p", _P), ("g", _P), ("m", _P), ("v", _P), ("n", ctypes.c_int64), ("group", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class BlurLearnParams(ctypes.Structure):
    """hnr_blur_learn_params"""
    _fields_ = [(n, _I) for n in ("patch_num", "patch_size", "kernel_size", "kernel_mode", "kernel_norm", "boundary_mode")] + [("slope", _F)]


class BlurLearnWeights(ctypes.Structure):
    """hnr_blur_learn_weights: Linear l's weight [out, in] and bias; the gradient block has the same layout."""
    _fields_ = [("w", _P * 4), ("b", _P * 4)]


RENDER_STAGES = ("query", "plan_gather", "chain_gather", "chain", "mlp_colorfeat", "proj_rows", "mlp_merge", "merge", "mlp_mixup", "final_color",
                 "composite")

# stage boundaries of the two training calls (their stage_events hook: one more event than stages)
TRAIN_FWD_STAGES = ("pack", "query_plan", "featmap", "gather_table", "chain", "per_sample", "composite")
TRAIN_BWD_STAGES = ("zero_pack", "composite_mixup", "merge_mlp", "proj_conv", "colorfeat", "ksum", "block3", "point_sums", "block1")

# name -> (restype, argtypes); must list every symbol include/hnr.h declares (tests check this)
SIGNATURES = {
    "hnr_version": (ctypes.c_char_p, []),
    "hnr_last_error": (ctypes.c_char_p, []),
    "hnr_points_bounds": (_I, [_P, _I, _P, _P]),
    "hnr_grid_build": (_I, [_P, _I, ctypes.POINTER(GridParams), _P, ctypes.POINTER(_P)]),
    "hnr_grid_free": (_I, [_P]),
    "hnr_grid_get_stats": (_I, [_P, ctypes.POINTER(GridStats)]),
    "hnr_grid_get_params": (_I, [_P, ctypes.POINTER(GridParams)]),
    "hnr_grid_export_dense": (_I, [_P, _P, _P, _P, _P]),
    "hnr_grid_grow": (_I, [_P, _P, _I, _P]),
    "hnr_grid_export_runs": (_I, [_P, _P, _P, _P]),
    "hnr_query_work_elems": (ctypes.c_int64, [_I, _I]),
    "hnr_march_query": (_I, [_P, _P, _P, _P, ctypes.POINTER(QueryParams), _P, _P, _P, _P, _P, _P, _P]),
    "hnr_ray_compact_plan": (_I, [_P, _I, _P, _P, _P, _P]),
    "hnr_ray_compact": (_I, [_P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "hnr_linear_packed_dims": (_I, [_I, _I, ctypes.POINTER(_I), ctypes.POINTER(_I)]),
    "hnr_linear_pack": (_I, [_P, _P, _I, _I, _P, _P, _P]),
    "hnr_linear_f32": (_I, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _F, _P]),
    "hnr_linear_f32_gather_add": (_I, [_P, _I, _P, _P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _F, _P]),
    "hnr_linear_f32_side": (_I, [_P, _I, _P, _P, _P, _P, _I, _I, _I, _P, _I, _I, _I, _I, _I, _F, _P]),
    "hnr_sample_plan": (_I, [_P, _P, _P, _I, _I, _P, _P, _P, _I, _I, _P, _P, _P]),
    "hnr_gather_rows": (_I, [_P] * 5 + [_I] + [_P] * 9 + [_I, _I, _I, _P, _I, _P, _I, _P, _P, _P, _P, _P]),
    "hnr_point_rows": (_I, [_P, _P, _I, _I, _P, _I, _P]),
    "hnr_gather_points": (_I, [_P, ctypes.c_int64] + [_P] * 5 + [_I] + [_P] * 9 + [_P]),
    "hnr_ksum": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _I, _P, _P]),
    "hnr_image_features_scratch_elems": (ctypes.c_int64, [_I, _I, _I]),
    "hnr_image_features": (_I, [_P, _I, _I, _I, ctypes.POINTER(_P), ctypes.POINTER(_P), _F, _P, _P, _P]),
    "hnr_proj_rows": (_I, [_P] * 8 + [_I, _I, _I, _P, _I, _I, _P, _I, _P, _P, _P]),
    "hnr_proj_pixels": (_I, [_P] * 5 + [_I, _I, _I, _I, _P, _P]),
    "hnr_div_probe": (_I, [_P, _P, _I, _P, _P, _P]),
    "hnr_div_probe2": (_I, [_P, _P, _F, _I, _P, _P, _P, _P, _P]),
    "hnr_merge": (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _P, _I, _P, _I, _I, _P, _I, _P, _P, _I, _P]),
    "hnr_chain_packed_bytes": (ctypes.c_int64, []),
    "hnr_chain_workspace_bytes": (ctypes.c_int64, [_I]),
    "hnr_chain_pack": (_I, [_P, _I] + [_P] * 9 + [_P, _P]),
    "hnr_chain_gather": (_I, [_P] * 11 + [_I, _I, _I, _P, _P, _I, _P, _P, _P]),
    "hnr_chain_classes": (_I, []),
    "hnr_chain_plan": (_I, [_P, _P, _P, _I, _I, _I, _P, _I, _P, _P]),
    "hnr_point_records": (_I, [_P, _P, _P, _P, _I, _P, _P]),
    "hnr_chain_gather_rec": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _I, _P, _P, _P]),
    "hnr_point_records_parts": (_I, [_P, _P, _P, _P, _P, _I, _P, _P]),
    "hnr_chain_gather_rec_parts": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _I, _P, _P, _P]),
    "hnr_chain_gather_parts": (_I, [_P] * 6 + [_I] + [_P] * 7 + [_I, _I, _I, _P, _P, _I, _P, _P, _P]),
    "hnr_chain_forward": (_I, [_P, _P, _I, _P, _P, _I, _F, _P, _I, _P, _P, _I, _P]),
    "hnr_mlp3_packed_bytes": (ctypes.c_int64, [_I, ctypes.POINTER(_I)]),
    "hnr_mlp3_pack": (_I, [_I, ctypes.POINTER(_P), ctypes.POINTER(_I), ctypes.POINTER(_I), ctypes.POINTER(_I), ctypes.POINTER(_P), _P, _P]),
    "hnr_mlp3_forward": (_I, [_P, _I, ctypes.c_int64, _P, _I, _I, _I, _P, _I, ctypes.POINTER(_I), ctypes.POINTER(_I), ctypes.POINTER(_I), _F, _P, _P, _I, _P, _I, _P, _I, _P]),
    "hnr_render_workspace_bytes": (ctypes.c_int64, [ctypes.POINTER(RenderParams)]),
    "hnr_render_forward": (_I, [_P, ctypes.POINTER(RenderParams), ctypes.POINTER(RenderCloud), ctypes.POINTER(RenderWeights),
                                ctypes.POINTER(RenderCamera), ctypes.POINTER(RenderViews), _P, ctypes.c_int64, ctypes.POINTER(RenderOutputs), _P]),
    "hnr_merge_stage": (_I, [_P] * 8 + [_I, _I, _I, _P, _P, _I, _P, _P, _P, _P, _I, _I, _F, _P, _I, _P]),
    "hnr_final_color": (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _P, _I, _P, _P]),
    "hnr_mixup_stage": (_I, [_P, _I, _P, _P, _I, _P, _P, _P, _P, _P, _I, _F, _P, _I, _P, _P]),
    "hnr_composite": (_I, [_P] * 8 + [_I, _I, _I, _F, _I, _P, _P, _P, _P, _P]),
    "hnr_ray_depth": (_I, [_P] * 6 + [_I, _I, _P, _P]),
    "hnr_probe_outputs": (_I, [_P] * 10 + [_I, _I, _I, _I] + [_P] * 7 + [_P]),
    "hnr_ray_march": (_I, [_P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P]),
    "hnr_blur_select": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "hnr_blur_select_bwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P]),
    "hnr_shipped_loss_scratch_bytes": (ctypes.c_int64, []),
    "hnr_shipped_loss": (_I, [_P, _P, _P, _I, _P, ctypes.c_int64, _F, _F, _F, _F, _P, _P, _P, _P, _P]),
    "hnr_shipped_loss_rows": (_I, [_P, _P, _P, _I, _P, _I, _F, _F, _F, _F, _P, _P, _P, _P, _P]),
    "hnr_shipped_loss_rows_fw": (_I, [_P, _P, _P, _I, _P, _I, _F, _F, _F, _P, _P, _P, _P, _P, _P]),
    "hnr_frame_metrics_scratch_bytes": (ctypes.c_int64, [_I, _I, _I]),
    "hnr_frame_metrics": (_I, [_P, _P, _I, _I, _P, _P, _P, _I, _I, _F, _P, _P, _P, _P, _P]),
    "hnr_voxel_downsample_scratch_bytes": (ctypes.c_int64, [ctypes.c_int64]),
    "hnr_voxel_downsample": (_I, [_P, _I, ctypes.POINTER(_F), _F, _P, _P, _P, _P, _P, _P, ctypes.c_int64, _P]),
    # initial cloud from depth frames (csrc/cloud_init.hip)
    "hnr_depth_fuse_scratch_bytes": (ctypes.c_int64, [_I, _I]),
    "hnr_depth_fuse_frame": (_I, [_P, _I, _I, _I, ctypes.POINTER(_F), ctypes.POINTER(_F), _F, _F, _F, _I, _P, ctypes.c_int64, _P, _P, _P, ctypes.c_int64, _P]),
    "hnr_range_crop_scratch_bytes": (ctypes.c_int64, [ctypes.c_int64]),
    "hnr_range_crop": (_I, [_P, _P, ctypes.c_int64, ctypes.POINTER(_F), _P, _P, _P, ctypes.c_int64, _P]),
    "hnr_nearest_view": (_I, [_P, ctypes.c_int64, _P, _P, _I, _P, _P]),
    "hnr_point_view_attrs": (_I, [_P, ctypes.c_int64] + [ctypes.POINTER(_F)] * 4 + [_I, _I, _P, _I, _I, _I, _P, _P, _P, _P]),
    "hnr_point_view_attrs_vis": (_I, [_P, ctypes.c_int64] + [ctypes.POINTER(_F)] * 4 + [_I, _I, _P, _I, _I, _I, _P, _P, _P, _P, _P]),
    # point embeddings from the MVS init checkpoint (csrc/featnet.hip)
    "hnr_featnet_scratch_elems": (ctypes.c_int64, [_I, _I, _I]),
    "hnr_featnet_forward": (_I, [_P, _I, _I, _I, _P, _P, _P, _P, _P, ctypes.c_int64, _P]),
    "hnr_point_embed": (_I, [_P, ctypes.c_int64] + [ctypes.POINTER(_F)] * 4 + [_I, _I] + [_P] * 10),
    "hnr_point_embed_conf": (_I, [_P, ctypes.c_int64] + [ctypes.POINTER(_F)] * 4 + [_I, _I] + [_P] * 11),
    "hnr_point_embed_vis": (_I, [_P, ctypes.c_int64] + [ctypes.POINTER(_F)] * 4 + [_I, _I] + [_P] * 12),
    # visual-hull masking and the occlusion test of the synthetic scenes (csrc/hull.hip)
    "hnr_alpha_pack": (_I, [_P, _I, _I, _I, _P, _P]),
    "hnr_visual_hull_select_scratch_bytes": (ctypes.c_int64, [ctypes.c_int64]),
    "hnr_visual_hull_select": (_I, [_P, _P, _P, ctypes.c_int64, _P, _P, _I, _I, _I, ctypes.POINTER(_F), _I, _P, _P, _P, _P, ctypes.c_int64, _P, _P, _P,
                                    ctypes.c_int64, _P]),
    "hnr_point_occlusion_scratch_bytes": (ctypes.c_int64, [_I, _I]),
    "hnr_point_occlusion": (_I, [_P, ctypes.c_int64, ctypes.POINTER(_F), ctypes.POINTER(_F), _I, _I, _F, _P, _P, ctypes.c_int64, _P]),
    # geometric-consistency filter of MVS depth maps (csrc/geo_filter.hip)
    "hnr_geo_consistency": (_I, [_P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "hnr_geo_filter_select_scratch_bytes": (ctypes.c_int64, [_I, _I, _I]),
    "hnr_geo_filter_select": (_I, [_P] * 5 + [_I, _I, _I, _P, _F, _I, ctypes.POINTER(_F), ctypes.POINTER(_F), _P, _P, _P, _P, ctypes.c_int64, _P, _P, _P, _P,
                                   ctypes.c_int64, _P]),
    # depth maps from the pretrained MVSNet (csrc/mvsnet.hip)
    "hnr_mvsnet_feature_scratch_elems": (ctypes.c_int64, [_I, _I, _I]),
    "hnr_mvsnet_feature": (_I, [_P, _I, _I, _I, _P, _P, _P, ctypes.c_int64, _P]),
    "hnr_mvsnet_cost_volume": (_I, [_P, _I, _I, _I, _P, _P, _I, _P, _P]),
    "hnr_mvsnet_cost_reg_scratch_elems": (ctypes.c_int64, [_I, _I, _I]),
    "hnr_mvsnet_cost_reg": (_I, [_P, _I, _I, _I, _P, _P, _P, ctypes.c_int64, _P]),
    "hnr_mvsnet_depth_head": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P]),
    "hnr_mvsnet_depth_points": (_I, [_P, _P, _I, _I, _I, _I, _F, _F, ctypes.POINTER(_F), _P, _P, _P, _P]),
    # content-aware frame weights: RAFT flow (csrc/raft.hip) and blur scores (csrc/blur_score.hip)
    "hnr_raft_encoder_packed_elems": (ctypes.c_int64, []),
    "hnr_raft_update_packed_elems": (ctypes.c_int64, []),
    "hnr_raft_encoder_scratch_elems": (ctypes.c_int64, [_I, _I, _I]),
    "hnr_raft_encoder": (_I, [_P, _I, _I, _I, _P, _I, _P, _P, ctypes.c_int64, _P]),
    "hnr_raft_pyramid_elems": (ctypes.c_int64, [_I, _I]),
    "hnr_raft_pyramid_scratch_elems": (ctypes.c_int64, [_I, _I]),
    "hnr_raft_corr_pyramid": (_I, [_P, _P, _I, _I, _P, _P, ctypes.c_int64, _P]),
    "hnr_raft_lookup": (_I, [_P, _P, _I, _I, _P, _P]),
    "hnr_raft_update_scratch_elems": (ctypes.c_int64, [_I, _I]),
    "hnr_raft_update": (_I, [_P, _P, _P, _P, _P, _I, _I, _P, _P, _P, ctypes.c_int64, _P]),
    "hnr_raft_upsample": (_I, [_P, _P, _I, _I, _P, _P]),
    "hnr_raft_flow_scratch_elems": (ctypes.c_int64, [_I, _I]),
    "hnr_raft_flow": (_I, [_P, _P, _I, _I, _P, _P, _P, _I, _P, _P, _P, ctypes.c_int64, _P]),
    "hnr_blur_edges": (_I, [_P, _I, _I, _I, _P, _P]),
    "hnr_blur_score_pair_scratch_bytes": (ctypes.c_int64, [_I, _I]),
    "hnr_blur_score_pair": (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _P, _P, ctypes.c_int64, _P]),
    # LPIPS with the AlexNet and VGG-16 backbones (csrc/lpips.hip)
    "hnr_lpips_packed_elems": (ctypes.c_int64, [_I]),
    "hnr_lpips_scratch_bytes": (ctypes.c_int64, [_I, _I, _I]),
    "hnr_lpips_tap_dims": (_I, [_I, _I, _I, ctypes.POINTER(_I)]),
    "hnr_lpips_prepare": (_I, [_P, _P, _I, _I, _I, _P, _P, _P]),
    "hnr_lpips_prepare_f32": (_I, [_P, _P, _I, _I, _P, _P, _P]),
    "hnr_lpips_features": (_I, [_I, _P, _I, _I, _P, ctypes.POINTER(_P), _P, ctypes.c_int64, _P]),
    "hnr_lpips_score": (_I, [_I, ctypes.POINTER(_P), _I, _I, _P, _P, _P, ctypes.c_int64, _P]),
    "hnr_lpips": (_I, [_I, _P, _P, _I, _I, _I, _P, _P, _P, ctypes.c_int64, _P]),
    "hnr_lpips_f32": (_I, [_I, _P, _P, _I, _I, _P, _P, _P, ctypes.c_int64, _P]),
    # device-resident frame bank + batch sampler (csrc/frames.hip)
    "hnr_frame_batch_scratch_bytes": (ctypes.c_int64, [_I, _I]),
    "hnr_frame_batch": (_I, [ctypes.POINTER(FrameBankC), ctypes.POINTER(FrameBankC), _P, _I, ctypes.POINTER(FrameBatchParams), _P, _I, _P,
                             ctypes.POINTER(FrameBatchOut), _P, ctypes.c_int64, _P]),
    "hnr_frame_item": (_I, [ctypes.POINTER(FrameBankC), ctypes.POINTER(FrameBankC), _P, _I, _I, _P, ctypes.c_int64, _I, _I, ctypes.POINTER(_F), _I,
                            ctypes.POINTER(FrameBatchOut), _P, ctypes.c_int64, _P]),
    # camera paths: reference views of free poses, the item of a path frame, the store into a clip (csrc/path.hip)
    "hnr_pose_views": (_I, [ctypes.POINTER(FrameBankC), _P, _I, _P, _I, _P, _I, _I, _P, _P]),
    "hnr_path_item": (_I, [ctypes.POINTER(FrameBankC), _P, _I, _P, _I, _I, _I, _P, _I, _I, _I, ctypes.POINTER(_F), _I, ctypes.POINTER(FrameBatchOut), _P,
                           ctypes.c_int64, _P]),
    "hnr_frame_store": (_I, [_P, _P, _P, ctypes.c_int64, _I, _I, _P, _P, _P, _P]),
    # raw frames to the bank's size: Pillow's resize, RGBA mode, compose (csrc/resize.hip)
    "hnr_resize_coeffs": (_I, [_I, _I, _I, _P, _P, ctypes.c_int64]),
    "hnr_resize_u8_scratch_bytes": (ctypes.c_int64, [_I, _I, _I, _I, _I, _I]),
    "hnr_resize_u8_form": (_I, [_I, _I, _I, _I, _I, _I, _I]),
    "hnr_resize_u8": (_I, [_P, _I, _I, _I, _I, _P, _I, _I, _P, _P, _I, _P, _P, _I, _I, _P, ctypes.c_int64, _P]),
    "hnr_rgba_premultiply": (_I, [_P, _P, ctypes.c_int64, _P]),
    "hnr_rgba_unpremultiply": (_I, [_P, _P, ctypes.c_int64, _P]),
    "hnr_rgba_compose": (_I, [_P, ctypes.c_int64, _P, _P, _P, _P, _P]),
    # depth supervision from resident depth frames: per-ray gt_depth, the loss term, the depth metrics row (csrc/depth_sup.hip)
    "hnr_frame_depth_rays": (_I, [ctypes.POINTER(DepthBankC), _P, _P, _P, _I, _P, _P]),
    "hnr_depth_loss": (_I, [_P, _P, _P, _I, _F, _P, _P, _P, _P, _P]),
    "hnr_depth_metrics": (_I, [_P, _P, _P, _I, _P, _P]),
    # patch SSIM term of the training loss, value + gradient (csrc/ssim_loss.hip)
    "hnr_ssim_loss_scratch_bytes": (ctypes.c_int64, [_I]),
    "hnr_ssim_loss": (_I, [_P, _P, _P, _I, _I, _I, ctypes.POINTER(_F), _F, _F, _P, _P, _P, _P, _I, _P, _P]),
    # growth schedule: ray-miss loss + the table of the worst frames, one launch per step (csrc/rank.hip)
    "hnr_ray_miss_rank": (_I, [_P, _P, _P, _I, _P, _P, _P, _I, _P, _P]),
    # the optimiser step: Adam for all parameter groups in one launch + the schedule tick (csrc/adam.hip)
    "hnr_adam_plan": (ctypes.c_int64, [ctypes.POINTER(AdamTensor), _I, _I, ctypes.POINTER(ctypes.c_int32), ctypes.c_int64]),
    "hnr_adam_step": (_I, [_P, _P, _I, _P, _P, _I, _P, ctypes.c_int64, _P]),
    "hnr_blur_gray_patches": (_I, [_P, _P, _I, _I, _P, _P]),
    "hnr_blur_gray_patches_bwd": (_I, [_P, _I, _I, _P, _P]),
    "hnr_blur_apply": (_I, [_P, _P, _I, _I, _I, _I, _P, _P]),
    "hnr_blur_apply_bwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    # the learnable blur module as three launches (train_step(learnable_blur=...))
    "hnr_blur_learn_workspace_bytes": (ctypes.c_int64, [_I, _I, _I, _I]),
    "hnr_blur_learn_forward": (_I, [ctypes.POINTER(BlurLearnParams), ctypes.POINTER(BlurLearnWeights), _P, _P, _P, ctypes.c_int64, _P, _P, _P]),
    "hnr_blur_learn_backward": (_I, [ctypes.POINTER(BlurLearnParams), ctypes.POINTER(BlurLearnWeights), _P, _P, _P, ctypes.c_int64, _P,
                                     ctypes.POINTER(BlurLearnWeights), _P]),
    # backward
    "hnr_composite_bwd": (_I, [_P] * 8 + [_I, _I, _I, _F, _I, _P, _P, _P]),
    "hnr_composite_bwd_depth": (_I, [_P] * 8 + [_I, _I, _I, _F, _I, _P, _P, _P, _P]),
    "hnr_final_color_bwd": (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _I, _P, _P, _I, _P, _I, _P, _P, _P, _P]),
    "hnr_merge_bwd": (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _P, _I, _I, _F, _P, _P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _P, _P, _P]),
    "hnr_proj_rows_bwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _I, _P, _I, _P, _P, _P, _P, _P, ctypes.c_int64, _P]),
    "hnr_sort_rows_scratch_bytes": (ctypes.c_int64, [ctypes.c_int64]),
    "hnr_sort_rows_by_key": (_I, [_P, ctypes.c_int64, _P, _P, _P, ctypes.c_int64, _P]),
    "hnr_segment_sum_rows": (_I, [_P, _I, _P, _I, _P, _P, ctypes.c_int64, _I, _P, ctypes.c_int64, _P]),
    "hnr_image_features_bwd": (_I, [_P, _I, _I, _I, ctypes.POINTER(_P), _F, _P, _P, ctypes.POINTER(_P), ctypes.POINTER(_P), _P]),
    "hnr_image_features_bwd_bbox": (_I, [_P, _I, _I, _I, ctypes.POINTER(_P), _F, _P, _P, ctypes.POINTER(_P), ctypes.POINTER(_P), _P, _P]),
    "hnr_gather_rows_bwd_rows": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P]),
    "hnr_segment_sum_rows_det": (_I, [_P, _I, _P, _P, ctypes.c_int64, _I, _I, _P, _P, ctypes.c_int64, _I, _P]),
    "hnr_segment_sum_rows_csr": (_I, [_P, _I, _P, _P, _P, _I, _I, _P, ctypes.c_int64, _P, _I, _I, _P, ctypes.c_int64, _P, _P]),
    # the glue kernels of the training backward, each alone (tests/test_backward_glue_gpu.py)
    "hnr_final_color_bwd_max": (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _I, _P, _P, _I, _P, _I, _P, _P, _P, _P, _P]),
    "hnr_merge_bwd_max": (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _P, _I, _I, _F, _P, _P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _P, _P, _P, _P]),   # (tests/test_ray_bwd_gpu.py)
    "hnr_ksum_bwd_rows8": (_I, [_P, _P, _P, _P, _P, _P, _I, _P, _F, _I, _P, _P, _P, _P, _P, _P]),
    "hnr_extras_dgrad": (_I, [_P, _P, _P, ctypes.c_int64, _P, _P]),
    "hnr_point_small_grads": (_I, [_P, _P, _I, _P, _P, _P, _P, _P]),
    "hnr_point_rows_bwd": (_I, [_P, _I, _P, _I, _P, _I, _P, _P, _P]),
    "hnr_dleaky_add": (_I, [_P, _I, _P, _I, _I, _P, _I, ctypes.c_int64, _P, _I, _F, _P, _P]),
    "hnr_sum_views": (_I, [_P, _I, _I, _I, _P, _I, _P, _I, _P, _P]),
    "hnr_unique_points_scratch_elems": (ctypes.c_int64, [_I]),
    "hnr_unique_points": (_I, [_P, ctypes.c_int64, _P, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P]),
    "hnr_conf0_grad": (_I, [_P, _P, ctypes.c_int64, _P, _P, _P]),
    "hnr_w0fd_grad": (_I, [_P, _P, _P]),
    "hnr_ray_drop_flags": (_I, [_P, _I, _P, _P, _P, _P]),
    "hnr_probe_select": (_I, [_P, _P, _P, _P, ctypes.POINTER(_F), _P, _P, _I, _I, _I, _F, _F, _P, _P, _P]),
    # training-step dense layers on the 16-bit matrix pipe (csrc/h2gemm.hip)
    "hnr_h2lin_packed_bytes": (ctypes.c_int64, [_I]),
    "hnr_h2lin_pack": (_I, [_I, ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(_I), ctypes.POINTER(_I),
                            ctypes.POINTER(_P), ctypes.POINTER(_P), _P]),
    "hnr_h2lin": (_I, [_P, _I, ctypes.c_int64, _P, _I, ctypes.c_int64, _P, _I, _I, _I, _I, _F, _P, _I, _P, _I, _P, _P]),
    "hnr_h2wgrad_scratch_bytes": (ctypes.c_int64, [_I, _I]),
    "hnr_h2lin_dgrad_bits": (_I, [_P, _I, ctypes.c_int64, _P, _P, _I, _I, _F, _P, _P, _I, _P, _P]),
    "hnr_h2wgrad": (_I, [_P, _I, _P, _I, ctypes.c_int64, _P, _I, ctypes.c_int64, _I, _I, _P, _P, _P, _I, _P, _I, _P, _P]),
    "hnr_absmax": (_I, [_P, _I, ctypes.c_int64, _P, _I, ctypes.c_int64, _I, _P, _P]),
    "hnr_point_grad_pack": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _P, _P]),
    "hnr_point_grad_apply": (_I, [_P, _I, _I, _P, _P, _P, _P, _I, _P, _P]),
    # the training step as two calls (csrc/render_train.hip)
    "hnr_render_train_workspace_bytes": (ctypes.c_int64, [ctypes.POINTER(TrainParams)]),
    "hnr_render_train_debug_layout": (_I, [ctypes.POINTER(TrainParams), ctypes.POINTER(ctypes.c_int64), _I]),
    "hnr_render_train_touched": (_I, [ctypes.POINTER(TrainParams), _P, ctypes.c_int64, ctypes.POINTER(_P), ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_int64)]),
    "hnr_render_train_forward": (_I, [_P, ctypes.POINTER(TrainParams), ctypes.POINTER(TrainCloud), ctypes.POINTER(TrainWeights), ctypes.POINTER(RenderCamera),
                                      ctypes.POINTER(TrainViews), _P, _P, _P, ctypes.c_int64, ctypes.POINTER(RenderOutputs), _P]),
    "hnr_render_train_backward": (_I, [ctypes.POINTER(TrainParams), ctypes.POINTER(TrainCloud), ctypes.POINTER(TrainWeights), ctypes.POINTER(RenderCamera),
                                       ctypes.POINTER(TrainViews), _P, ctypes.c_int64, ctypes.POINTER(RenderOutputs), _P, _P, ctypes.POINTER(TrainCloudGrads),
                                       ctypes.POINTER(TrainWeights), _P]),
    "hnr_render_train_backward_depth": (_I, [ctypes.POINTER(TrainParams), ctypes.POINTER(TrainCloud), ctypes.POINTER(TrainWeights), ctypes.POINTER(RenderCamera),
                                             ctypes.POINTER(TrainViews), _P, ctypes.c_int64, ctypes.POINTER(RenderOutputs), _P, _P, _P,
                                             ctypes.POINTER(TrainCloudGrads), ctypes.POINTER(TrainWeights), _P]),
}

_lib = None


def lib():
    """Load libhnr_hip.so once.  Raises HnrError (never falls back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HnrError(
            "libhnr_hip.so is missing (%s). Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C hybridneuralrendering_amd/csrc`; there is no CPU or PyTorch fallback." % LIB_PATH)
    try:
        L = ctypes.CDLL(LIB_PATH)
    except OSError as e:
        raise HnrError("cannot load %s: %s" % (LIB_PATH, e))
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            raise HnrError("libhnr_hip.so does not export %s (stale build?)" % name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def last_error():
    return lib().hnr_last_error().decode("utf-8", "replace")


def check(rc, what):
    if rc != 0:
        raise HnrError("%s failed (code %d): %s" % (what, rc, last_error()))


def ptr(t):
    """Device pointer of a contiguous CUDA(HIP) tensor as void*."""
    if t is None:
        return None
    if not t.is_cuda:
        raise HnrError("expected a tensor on the GPU, got device=%s" % t.device)
    if not t.is_contiguous():
        raise HnrError("expected a contiguous tensor")
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Strided:
    """Marks a tensor argument of `call` that goes with a leading stride of its own (an lda/ldc operand): no contiguity check."""
    __slots__ = ("t",)

    def __init__(self, t):
        self.t = t


STREAM = object()        # written where the prototype has `void *stream`: the current stream of the call's device
_INT_BITS = {ctypes.c_int: 31, ctypes.c_int64: 63}


def _invoke(name, args, device=None):
    """What the library function returns for `args`, translated as `call` documents, with the arguments' device current."""
    fn = getattr(lib(), name, None) if name in SIGNATURES else None
    if fn is None:
        raise HnrError("libhnr_hip.so has no function %s" % name)
    c, dev, at = list(args), None, -1
    for i, a in enumerate(args):
        if a is None or type(a) in (int, float):
            continue
        if a is STREAM:
            at = i
        elif isinstance(a, (torch.Tensor, Strided)):
            t = a if isinstance(a, torch.Tensor) else a.t
            if not t.is_cuda:
                raise HnrError("%s: argument %d must be a tensor on the GPU, got device=%s" % (name, i, t.device))
            if t is a and not t.is_contiguous():
                raise HnrError("%s: argument %d must be a contiguous tensor (_lib.Strided marks one with a stride of its own)" % (name, i))
            if dev is None:
                dev = t.device
            elif t.device != dev:
                raise HnrError("%s: argument %d is on %s, the tensors before it on %s" % (name, i, t.device, dev))
            c[i] = ctypes.c_void_p(t.data_ptr())
        elif isinstance(a, ctypes.Structure):
            c[i] = ctypes.byref(a)
    if dev is None:
        dev = device
    if dev is None:
        if at >= 0:
            raise HnrError("%s: a stream needs a device: no tensor argument and no device=" % name)
        return fn(*c)
    with torch.cuda.device(dev):
        if at >= 0:
            c[at] = stream()
        return fn(*c)


def call(name, *args, device=None, ok=()):
    """One call into the library; `args` stand one to one in the header's order.  A tensor becomes its device pointer (on the GPU and contiguous;
    `Strided(t)` skips the contiguity check), a ctypes.Structure its byref, None is NULL, STREAM the current stream of the call's device, anything
    else passes through.  The device is the one device of all tensor arguments (`device=` when there is none) and is current during the call.
    Returns the status: 0, or one of `ok`; any other raises HnrError with the library's error text."""
    rc = _invoke(name, args, device)
    if rc not in ok:
        check(rc, name)
    return rc


def size(name, *args, what=None):
    """The value of an entry point that returns a size or a count, not a status (the `*_scratch_bytes`, `*_elems`, `*_packed_*` and
    `*_workspace_bytes` families, hnr_adam_plan, hnr_resize_coeffs, hnr_resize_u8_form, hnr_chain_classes) as an int; arguments as in `call`.
    A negative value (a shape the library refuses) and an int argument outside its C type's range raise HnrError(`what`, or a default text)."""
    types = SIGNATURES[name][1] if name in SIGNATURES else ()
    fits = all(-1 << _INT_BITS[t] <= a < 1 << _INT_BITS[t] for a, t in zip(args, types) if type(a) is int and t in _INT_BITS)
    n = int(_invoke(name, args)) if fits else -1
    if n < 0:
        shown = ", ".join(repr(a) if isinstance(a, (int, float)) else type(a).__name__ for a in args)
        raise HnrError(what or "%s(%s) refused: %s" % (name, shown, last_error() if fits else "an argument is outside its C type's range"))
    return n


def scratch(name, *args, device, dtype=torch.uint8, what=None):
    """A fresh tensor of `size(name, *args)` elements of `dtype` on `device`."""
    return torch.empty((size(name, *args, what=what),), dtype=dtype, device=device)


def require_gpu(t, name, dtype=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise HnrError("%s must be a tensor on the GPU (the HIP path has no CPU fallback)" % name)
    if dtype is not None and t.dtype != dtype:
        raise HnrError("%s must have dtype %s, got %s" % (name, dtype, t.dtype))
    return t.contiguous()


# ---- raw HIP events (profiling hooks of hnr_render_forward: recorded by the library on the launch stream) ------------------
_hip = None


def hip_runtime():
    global _hip
    if _hip is None:
        _hip = ctypes.CDLL("libamdhip64.so")
        _hip.hipEventCreate.argtypes = [ctypes.POINTER(_P)]
        _hip.hipEventDestroy.argtypes = [_P]
        _hip.hipEventSynchronize.argtypes = [_P]
        _hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(_F), _P, _P]
    return _hip


class StageEvents:
    """len(stages) + 1 hipEvent_t handles; elapsed_ms() after the stream has been synchronised."""

    def __init__(self, stages=RENDER_STAGES):
        H = hip_runtime()
        self.stages = tuple(stages)
        self.n = len(self.stages) + 1
        self.arr = (_P * self.n)()
        for i in range(self.n):
            e = _P()
            if H.hipEventCreate(ctypes.byref(e)) != 0:
                raise HnrError("hipEventCreate failed")
            self.arr[i] = e

    def elapsed_ms(self):
        H = hip_runtime()
        out = {}
        for i, name in enumerate(self.stages):
            ms = _F()
            if H.hipEventElapsedTime(ctypes.byref(ms), self.arr[i], self.arr[i + 1]) != 0:
                raise HnrError("hipEventElapsedTime failed (events not recorded / not complete)")
            out[name] = float(ms.value)
        return out

    def __del__(self):
        try:
            H = hip_runtime()
            for i in range(self.n):
                if self.arr[i]:
                    H.hipEventDestroy(self.arr[i])
        except Exception:
            pass
