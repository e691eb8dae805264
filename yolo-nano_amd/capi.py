"""ctypes binding of libyolonano_hip.so (include/yolonano_hip.h).

The product path has NO CPU fallback: if the HIP library is missing or no GPU is
visible, creating a handle raises.  torch is imported first on purpose — it loads
its bundled libamdhip64.so.7, and the library then resolves the same runtime by
soname, so torch tensors' ``data_ptr()`` and torch streams are valid in it.
"""
import ctypes
import os

import numpy as np
import torch  # noqa: F401  (must precede CDLL: shares the HIP runtime)

from . import arch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libyolonano_hip.so")

_vp = ctypes.c_void_p
_i32, _f32 = ctypes.c_int, ctypes.c_float
_i64p = ctypes.POINTER(ctypes.c_int64)

BACKBONE_ID = {"0.5x": 0, "1.0x": 1, "1.5x": 2, "2.0x": 3}


class YnConfig(ctypes.Structure):
    _fields_ = [("input_size", _i32), ("num_classes", _i32), ("num_anchors", _i32),
                ("anchors", _f32 * 18), ("backbone", _i32), ("conf_thresh", _f32), ("nms_thresh", _f32),
                ("diou_nms", _i32), ("max_batch", _i32), ("device", _i32), ("stream", _vp)]


# name -> (restype, argtypes); every symbol include/yolonano_hip.h declares
SIGNATURES = {
    "yn_abi_version": (_i32, []),
    "yn_create": (_i32, [ctypes.POINTER(YnConfig), ctypes.POINTER(_vp)]),
    "yn_destroy": (None, [_vp]),
    "yn_last_error": (ctypes.c_char_p, [_vp]),
    "yn_live_device_memory": (_i32, [_i64p, _i64p]),
    "yn_set_grid": (_i32, [_vp, _i32]),
    "yn_set_grid_rect": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32]),
    "yn_grid_shape": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "yn_set_stream": (_i32, [_vp, _vp]),
    "yn_set_thresholds": (_i32, [_vp, _f32, _f32, _i32]),
    "yn_num_predictions": (_i32, [_vp]),
    "yn_use_graph": (_i32, [_vp, _i32]),
    "yn_synchronize": (_i32, [_vp]),
    "yn_autotune": (_i32, [_vp, _i32]),
    "yn_set_pw_config": (_i32, [_vp, _i32]),
    "yn_tune_save": (_i32, [ctypes.c_char_p, _i32]),
    "yn_tune_load": (_i32, [ctypes.c_char_p, _i32]),
    "yn_allreduce_grads": (_i32, [_vp, _vp]),
    "yn_pw_config_count": (_i32, []),
    "yn_pw_f32_config_count": (_i32, []),
    "yn_unit_chain": (_i32, [_vp, _i32]),
    "yn_chain_pipe": (_i32, [_vp, _i32]),
    "yn_stage_fuse": (_i32, [_vp, _i32, _i32]),
    "yn_pw_pipe": (_i32, [_vp, _i32]),
    "yn_multi_stream": (_i32, [_vp, _i32]),
    "yn_exact_f32": (_i32, [_vp, _i32]),
    "yn_range_status": (_i32, [_vp, ctypes.POINTER(_i32), ctypes.POINTER(_i32)]),
    "yn_fuse_decode": (_i32, [_vp, _i32]),
    "yn_group_launch": (_i32, [_vp, _i32]),
    "yn_down_fuse": (_i32, [_vp, _i32]),
    "yn_tail_fuse": (_i32, [_vp, _i32]),
    "yn_nms_prefilter": (_i32, [_vp, _i32]),
    "yn_nms_sweep": (_i32, [_vp, _i32]),
    "yn_nms_sweep_segments": (_i32, [_vp, _i32, _i32]),
    "yn_nms_stages": (_i32, [_vp, _i32, _i32, _i32] + [_vp] * 10),
    "yn_load_param": (_i32, [_vp, ctypes.c_char_p, _vp, _i64p, _i32]),
    "yn_load_param_dev": (_i32, [_vp, ctypes.c_char_p, _vp, _i64p, _i32]),
    "yn_fold_bn": (_i32, [_vp]),
    "yn_get_folded": (_i32, [_vp, ctypes.c_char_p, _vp, _vp]),
    "yn_forward_raw": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp]),
    "yn_forward_taps": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp]),
    "yn_score_full": (_i32, [_vp, _vp, _vp, _vp, _i32, _vp, _vp]),
    "yn_decode_boxes": (_i32, [_vp, _vp, _i32, _vp]),
    "yn_create_grid": (_i32, [_vp, _i32, _vp, _vp, _vp]),
    "yn_create_grid_rect": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp]),
    "yn_nms": (_i32, [_vp, _vp, _vp, _i32, _f32, _i32, _vp, _vp]),
    "yn_postprocess": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "yn_infer": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "yn_pack_detections": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp]),
    "yn_loss": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "yn_loss_heads": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "yn_train_param_count": (ctypes.c_int64, [_vp]),
    "yn_train_param_offset": (_i32, [_vp, ctypes.c_char_p, _i64p, _i64p]),
    "yn_train_bind": (_i32, [_vp, _vp, _vp, _vp, ctypes.c_int64]),
    "yn_train_step": (_i32, [_vp, _vp, _vp, _i32, _f32, _f32, _f32, _f32, _i32, _vp]),
    "yn_read_param": (_i32, [_vp, ctypes.c_char_p, _vp, ctypes.c_int64]),
    "yn_train_forward": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp]),
    "yn_train_skipped_steps": (_i32, [_vp, _i64p]),
    "yn_train_head_fork": (_i32, [_vp, _i32, ctypes.POINTER(ctypes.c_int)]),
    "yn_train_precision": (_i32, [_vp, _i32]),
    "yn_train_graph": (_i32, [_vp, _i32, _vp]),
    "yn_train_get_loss_scale": (_i32, [_vp, ctypes.POINTER(_f32), ctypes.POINTER(_f32)]),
    "yn_train_set_loss_scale": (_i32, [_vp, _f32, _f32]),
    "yn_make_targets": (_i32, [_vp, _vp, _vp, _i32, _vp, _vp]),
    "yn_preprocess": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "yn_preprocess_batch": (_i32, [_vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp]),
    "yn_preprocess_batch_rect": (_i32, [_vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "yn_train_transform_batch": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp]),
    "yn_mosaic_transform_batch": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp]),
    "yn_nms_merge": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _f32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "yn_ema_update": (_i32, [_vp, _vp, _vp, ctypes.c_int64, ctypes.c_double]),
    "yn_sgd_step": (_i32, [_vp, _vp, _vp, _vp, ctypes.c_int64, _f32, _f32, _f32, _f32, _i32]),
    "yn_op_dwconv3x3": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp]),
    "yn_op_pwconv": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp]),
    "yn_op_pwconv_shuffle": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp]),
    "yn_op_pwconv_group": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp]),
    "yn_op_conv3x3": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp]),
    "yn_op_stem": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp]),
    "yn_op_stem_pool": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp]),
    "yn_op_maxpool3x3s2": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "yn_op_shuffle_block": (_i32, [_vp, ctypes.c_char_p, _vp, _i32, _i32, _i32, _vp]),
    "yn_op_down_unit": (_i32, [_vp, ctypes.c_char_p, _vp, _i32, _i32, _i32, _vp]),
    "yn_op_decode_cand": (_i32, [_vp, _vp, _vp, _vp, _i32, _f32, _vp, _vp, _vp]),
    "yn_op_head_tail": (_i32, [_vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp]),
    "yn_op_nchw_to_nhwc": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "yn_op_nhwc_to_nchw": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "yn_op_h16_conv": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    "yn_op_h16_conv2": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _i32, ctypes.c_int64,
                               _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "yn_op_h16_stem": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "yn_op_h16_maxpool": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "yn_op_h16_stem_pool": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "yn_op_h16_resample": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _i32]),
    "yn_op_h16_gather": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _i32, ctypes.c_int64, _i32, _i32]),
    "yn_op_h16_grad_finish": (_i32, [_vp, _vp, _vp, ctypes.c_int64, _vp, _i32, _i32]),
    "yn_op_h16_loss": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _f32, _vp, _vp, _vp, _vp, ctypes.POINTER(_i32)]),
    "yn_op_h16_bn2": (_i32, [_vp, _vp, _vp, ctypes.c_int64, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "yn_op_h16_bn": (_i32, [_vp, _vp, _vp, ctypes.c_int64, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "yn_op_h16_gemm_stats": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp]),
    "yn_op_h16_bn_unit": (_i32, [_vp, _vp, _vp, _vp, ctypes.c_int64, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "yn_op_f32_conv": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _i32, ctypes.c_int64, _vp, _i32, _vp, _vp, _vp, _vp]),
    "yn_op_f32_bn": (_i32, [_vp, _vp, ctypes.c_int64, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    "yn_op_f32_maxpool": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "yn_op_f32_resample": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _i32]),
    "yn_eval_create": (_i32, [_vp, _i32, ctypes.c_double, ctypes.POINTER(_vp)]),
    "yn_eval_destroy": (None, [_vp]),
    "yn_eval_reset": (_i32, [_vp, _vp]),
    "yn_eval_add": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "yn_eval_finish": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp]),
    "yn_eval_curve": (_i32, [_vp, _vp, _i32, _vp, _vp, ctypes.c_int64]),
    "yn_eval_records": (_i32, [_vp, _vp, _vp, ctypes.c_int64]),
    "yn_eval_size": (_i32, [_vp, _i64p, _i64p]),
    "yn_coco_create": (_i32, [_vp, _i32, _i32, ctypes.POINTER(_vp)]),
    "yn_coco_destroy": (None, [_vp]),
    "yn_coco_reset": (_i32, [_vp, _vp]),
    "yn_coco_add": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "yn_coco_finish": (_i32, [_vp, _vp, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _vp]),
    "yn_coco_matches": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32]),
    "yn_coco_size": (_i32, [_vp, _i64p, _i64p]),
    "yn_kmeans_create": (_i32, [_vp, ctypes.c_int64, _i32, ctypes.POINTER(_vp)]),
    "yn_kmeans_destroy": (None, [_vp]),
    "yn_kmeans_set_boxes": (_i32, [_vp, _vp, _vp, ctypes.c_int64]),
    "yn_kmeans_seed": (_i32, [_vp, _vp, _i32, ctypes.c_int64, _vp, _vp, _vp]),
    "yn_kmeans_set_centroids": (_i32, [_vp, _vp, _vp, _i32]),
    "yn_kmeans_run": (_i32, [_vp, _vp, ctypes.c_double, _i32, _vp, _vp, _vp, _vp]),
    "yn_kmeans_pass": (_i32, [_vp, _vp, _vp, _vp, _vp]),
    "yn_kmeans_assign": (_i32, [_vp, _vp, _vp]),
    "yn_kmeans_stats": (_i32, [_vp, _i64p, _i64p]),
    "yn_resize_batch": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "yn_wbf_merge": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _f32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "yn_wbf_lds_clusters": (_i32, []),
    "yn_wbf_cost": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64]),
    "yn_soft_nms_merge": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _f32, _f32, _vp, _vp, _vp, _vp, _vp]),
    "yn_soft_nms": (_i32, [_vp, _i32, _f32, _f32]),
    "yn_soft_lds_rows": (_i32, []),
    "yn_op_soft_exp": (_i32, [_vp, _vp, _vp, ctypes.c_int64]),
    "yn_merge_soft_tta": (_i32, [_vp, _vp, _i32, _f32, _f32]),
    "yn_merge_soft_slice": (_i32, [_vp, _vp, _i32, _f32, _f32]),
    "yn_merge_soft_fuse": (_i32, [_vp, _vp, _i32, _f32, _f32]),
    "yn_merge_rule_tta": (_i32, [_vp, _vp, _i32, _i32]),
    "yn_merge_rule_slice": (_i32, [_vp, _vp, _i32, _i32]),
    "yn_fuse_create": (_i32, [_vp, _i32, _i32, ctypes.POINTER(_vp)]),
    "yn_fuse_destroy": (None, [_vp]),
    "yn_fuse_open": (_i32, [_vp, _vp, _i32]),
    "yn_fuse_append": (_i32, [_vp, _vp, _i32, _vp, _vp, _f32]),
    "yn_fuse_merge": (_i32, [_vp, _vp, _i32, _i32, _f32, _i32]),
    "yn_fuse_result": (_i32, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_i32)]),
    "yn_fuse_lists": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "yn_tta_create": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, ctypes.POINTER(_vp)]),
    "yn_tta_destroy": (None, [_vp]),
    "yn_tta_infer": (_i32, [_vp, _vp, _vp, _i32, _i32, _f32]),
    "yn_tta_result": (_i32, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_i32)]),
    "yn_tta_forwards": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "yn_slice_create": (_i32, [_vp, _i32, _i32, ctypes.POINTER(_vp)]),
    "yn_slice_destroy": (None, [_vp]),
    "yn_slice_preprocess": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp]),
    "yn_slice_append": (_i32, [_vp, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _f32]),
    "yn_slice_merge": (_i32, [_vp, _vp, _i32, _f32]),
    "yn_slice_infer": (_i32, [_vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _f32, _f32]),
    "yn_slice_result": (_i32, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_i32)]),
    "yn_slice_lists": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "yn_draw_create": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, ctypes.POINTER(_vp)]),
    "yn_draw_destroy": (None, [_vp]),
    "yn_draw_batch": (_i32, [_vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, ctypes.c_int64, _f32]),
    "yn_draw_status": (_i32, [_vp, _vp, _i64p, _i64p, ctypes.POINTER(_i32)]),
    "yn_draw_prims": (_i32, [_vp, _vp, _vp, ctypes.c_int64]),
    "yn_chip_create": (_i32, [_vp, _i32, _vp, _i32, _vp, ctypes.POINTER(_vp)]),
    "yn_chip_destroy": (None, [_vp]),
    "yn_chip_batch": (_i32, [_vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, ctypes.c_int64, _vp, _vp, _vp, _vp]),
    "yn_chip_status": (_i32, [_vp, _vp, _vp]),
    "yn_track_create": (_i32, [_vp, _i32, _i32, _i32, _vp, ctypes.POINTER(_vp)]),
    "yn_track_destroy": (None, [_vp]),
    "yn_track_reset": (_i32, [_vp, _vp, _i32]),
    "yn_track_update": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, ctypes.c_int64, _vp, _vp, _vp]),
    "yn_track_state": (_i32, [_vp, _vp, _i32, _vp, _vp, ctypes.POINTER(_i32)]),
    "yn_track_status": (_i32, [_vp, _vp, _vp]),
    "yn_jpeg_info": (_i32, [_vp, ctypes.c_int64, _vp]),
    "yn_jpeg_coefficients": (_i32, [_vp, ctypes.c_int64, _vp, ctypes.c_int64, _vp, _vp, ctypes.POINTER(_i32)]),
    "yn_jpeg_create": (_i32, [_vp, _i32, ctypes.c_int64, _i32, ctypes.POINTER(_vp)]),
    "yn_jpeg_destroy": (None, [_vp]),
    "yn_jpeg_decode_batch": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, ctypes.POINTER(_i32)]),
    "yn_jpeg_reason": (ctypes.c_char_p, [_vp, _i32]),
    "yn_jpeg_timing": (_i32, [_vp, _vp, _vp]),
    "yn_jpeg_entropy": (_i32, [_vp, _i32, _i32, _i32]),
    "yn_jpeg_entropy_stats": (_i32, [_vp, _vp, _vp, _vp, _vp]),
    "yn_jpeg_device_coefficients": (_i32, [_vp, _vp, _i32, _vp, ctypes.c_int64]),
    "yn_jpeg_entropy_states": (_i32, [_vp, _vp, _i32, _vp, ctypes.c_int64]),
    "yn_jpeg_scan_prepare": (_i32, [_vp, ctypes.c_int64, _vp, ctypes.c_int64, _vp, ctypes.c_int64, _vp]),
    "yn_jpeg_entropy_timing": (_i32, [_vp, _vp, _vp]),
    "yn_jpeg_quant_tables": (_i32, [_i32, _vp]),
    "yn_jpeg_header": (_i32, [_i32, _i32, _i32, _i32, _vp]),
    "yn_jpeg_enc_create": (_i32, [_vp, _i32, ctypes.c_int64, ctypes.POINTER(_vp)]),
    "yn_jpeg_enc_destroy": (None, [_vp]),
    "yn_jpeg_encode_batch": (_i32, [_vp, _vp, _i32, _vp, _vp, _i32, _i32]),
    "yn_jpeg_encode_fetch": (_i32, [_vp, _vp, _vp, _vp, ctypes.c_int64]),
    "yn_jpeg_enc_coefficients": (_i32, [_vp, _vp, _i32, _vp, ctypes.c_int64]),
    "yn_jpeg_enc_guard": (_i32, [_vp, _vp, _vp]),
    "yn_jpeg_enc_timing": (_i32, [_vp, _vp, _vp]),
    "yn_profile_enable": (_i32, [_vp, _i32]),
    "yn_profile_count": (_i32, [_vp]),
    "yn_profile_get": (_i32, [_vp, _i32, ctypes.c_char_p, _i32, ctypes.c_char_p, _i32, ctypes.POINTER(_f32),
                              ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
}

_lib = None


class YnError(RuntimeError):
    pass


class YnRangeError(YnError):
    """yn_infer reported (negative counts / offsets[B]) that an activation left the split-f16 range: the detections of that call are not
    valid.  Call range_status() (clears the flag), switch the handle to exact_f32(True) and run again - YOLONano does this by itself."""


def records_to_host(rec, offsets):
    """(rec [>= total, 6], offsets [B+1]) in yn_pack_detections' layout (device tensors; offsets may already be a host array) -> list of B
    (bboxes [K,4] f32, scores [K] f32, cls_inds [K] i64) numpy triples, fresh and writable: two device-to-host copies."""
    off = offsets if isinstance(offsets, np.ndarray) else offsets.cpu().numpy()
    host = rec[: int(off[-1])].cpu().numpy()
    res = []
    for b in range(len(off) - 1):
        r = host[off[b]:off[b + 1]]
        res.append((r[:, :4].copy(), r[:, 4].copy(), r[:, 5].astype(np.int64)))
    return res


def load_library():
    """dlopen the in-tree HIP library and type every entry point.  Raises if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise YnError("%s is missing — build it with `python -m yolo_nano_amd.build` "
                          "(there is no CPU fallback for the product path)" % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)              # AttributeError if the .so lacks a declared symbol
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def _ptr(t):
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        assert t.is_contiguous(), "tensor must be contiguous"
        return t.data_ptr()
    return t


def tune_save(path, device=0):
    """Write the process-wide autotune table of `device` to `path` (yn_tune_save)."""
    if load_library().yn_tune_save(str(path).encode(), int(device)):
        raise YnError("yn_tune_save(%s) failed" % path)


def tune_load(path, device=0):
    """Adopt the entries of `path` for `device` (yn_tune_load) -> number adopted, -1 if unreadable."""
    return int(load_library().yn_tune_load(str(path).encode(), int(device)))


class Handle:
    """One yn_handle = one device + one stream.  Thin, 1:1 with the C ABI."""

    def __init__(self, input_size, num_classes, anchor_size, backbone="1.0x", conf_thresh=0.001,
                 nms_thresh=0.5, diou_nms=False, max_batch=1, device=None, stream=None):
        self.lib = load_library()
        if backbone not in BACKBONE_ID:
            raise YnError("unknown backbone %r" % (backbone,))
        if not torch.cuda.is_available():
            raise YnError("no MI355X visible: the YOLO-Nano HIP path needs a GPU (no CPU fallback)")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise YnError("device must be a GPU, got %s" % (dev,))
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        flat = [float(v) for wh in anchor_size for v in wh]
        if len(flat) % 6:
            raise YnError("anchor_size must hold 3*A [w,h] pairs")
        self.A = len(flat) // 6
        cfg = YnConfig()
        cfg.input_size, cfg.num_classes, cfg.num_anchors = int(input_size), int(num_classes), self.A
        for i, v in enumerate(flat):
            cfg.anchors[i] = v
        cfg.backbone = BACKBONE_ID[backbone]
        cfg.conf_thresh, cfg.nms_thresh, cfg.diou_nms = float(conf_thresh), float(nms_thresh), int(bool(diou_nms))
        cfg.max_batch, cfg.device = int(max_batch), self.device.index
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream(self.device) if stream is None else stream
            cfg.stream = st.cuda_stream
            h = _vp()
            if self.lib.yn_create(ctypes.byref(cfg), ctypes.byref(h)):
                raise YnError("yn_create: " + self.lib.yn_last_error(None).decode())
        self.h = h
        self._stream_ptr = cfg.stream
        self.C, self.S = int(num_classes), int(input_size)
        self.H = self.W = self.S                                # the canvas; S is None on a rectangular grid (set_grid_rect)
        self.max_batch = max(int(max_batch), 1)
        self.backbone = backbone
        self.head_ch = arch.head_channels(self.C, self.A)

    def close(self):
        if getattr(self, "h", None):
            self.lib.yn_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _torch_stream(self):
        """The stream the handle launches on, as a torch stream object (for record_stream)."""
        if getattr(self, "_ts_ptr", None) != self._stream_ptr or getattr(self, "_ts", None) is None:
            self._ts = torch.cuda.ExternalStream(self._stream_ptr, device=self.device) if self._stream_ptr else torch.cuda.default_stream(self.device)
            self._ts_ptr = self._stream_ptr
        return self._ts

    def _in(self, t, dtype=torch.float32):
        """`t` as a contiguous `dtype` tensor that is safe to hand to the library as a bare pointer.  A converted / compacted COPY would go
        back to torch's caching allocator as soon as the caller's expression ends, while the kernels that read it are still queued on
        the handle's stream (which need not be torch's current one): the copy is tied to that stream with record_stream."""
        c = t if t.dtype == dtype else t.to(dtype)
        c = c.contiguous()
        if c.is_cuda and c.data_ptr() != t.data_ptr():
            c.record_stream(self._torch_stream())
        return c

    def _ck(self, rc, what):
        if rc == 2:                                             # YN_STATUS_RANGE: an earlier yn_infer's range mark has not been acknowledged
            raise YnRangeError("%s: %s" % (what, self.lib.yn_last_error(self.h).decode()))
        if rc:
            raise YnError("%s: %s" % (what, self.lib.yn_last_error(self.h).decode()))

    # ---- configuration
    @property
    def N(self):
        return self.lib.yn_num_predictions(self.h)

    def set_grid(self, S):
        self._ck(self.lib.yn_set_grid(self.h, int(S)), "yn_set_grid")
        self.S = self.H = self.W = int(S)

    def set_grid_rect(self, H, W, side=0, left=0, top=0):
        """The H x W window at (left, top) of a letterboxed side x side square (yn_set_grid_rect; side = 0: the smallest square, centred).
        Boxes stay normalised to the square.  The window that is the whole square is set_grid(side)."""
        self._ck(self.lib.yn_set_grid_rect(self.h, int(H), int(W), int(side), int(left), int(top)), "yn_set_grid_rect")
        H, W, side, left, top = self.shape
        self.H, self.W = H, W
        self.S = side if (H == W == side and left == 0 and top == 0) else None

    @property
    def shape(self):
        """(H, W, side, left, top) of the current grid."""
        v = [ctypes.c_int32() for _ in range(5)]
        self._ck(self.lib.yn_grid_shape(self.h, *[ctypes.addressof(x) for x in v]), "yn_grid_shape")
        return tuple(int(x.value) for x in v)

    def set_stream(self, stream):
        self._ck(self.lib.yn_set_stream(self.h, stream.cuda_stream), "yn_set_stream")
        self._stream_ptr = stream.cuda_stream

    def follow_current_stream(self):
        """Re-home the handle onto torch's current stream of its device when that differs from the one it launches on
        (the old stream is drained first: the activation arena is shared).  The host shim calls this before every forward so
        that `with torch.cuda.stream(s): model(x)` orders the HIP kernels with the torch ops issued on `s`."""
        st = torch.cuda.current_stream(self.device)
        if st.cuda_stream != self._stream_ptr:
            self.set_stream(st)

    def set_thresholds(self, conf, nms, diou=False):
        self._ck(self.lib.yn_set_thresholds(self.h, float(conf), float(nms), int(bool(diou))), "yn_set_thresholds")

    def use_graph(self, on=True):
        self._ck(self.lib.yn_use_graph(self.h, int(bool(on))), "yn_use_graph")

    def autotune(self, on=True):
        self._ck(self.lib.yn_autotune(self.h, int(bool(on))), "yn_autotune")

    def set_pw_config(self, index):
        """Testing aid: pin the pointwise GEMMs to one tile configuration (index < 0: back to the autotuner)."""
        self._ck(self.lib.yn_set_pw_config(self.h, int(index)), "yn_set_pw_config")

    def unit_chain(self, mode=1):
        """One kernel per stride-1 ShuffleV2 unit: 1 = where the map is large enough (default), 0 = never, 2 = always (True = 2);
        bit-identical results either way."""
        self._ck(self.lib.yn_unit_chain(self.h, 2 if mode is True else int(mode)), "yn_unit_chain")

    def chain_pipe(self, mode=1):
        """unit_pipe_kernel (the persistent per-unit tile walk): 1 = by its size rule (default), 0 = never, 2 = also for few tiles; bit-identical."""
        self._ck(self.lib.yn_chain_pipe(self.h, 2 if mode is True else int(mode)), "yn_chain_pipe")

    def stage_fuse(self, mode=1, publish_early=False):
        """stage_pipe_kernel (all but the last stride-1 unit of a stage as ONE persistent launch): 1 = from 256 tiles (default), 0 = never,
        2 = at every size; bit-identical to the per-unit launches."""
        self._ck(self.lib.yn_stage_fuse(self.h, 2 if mode is True else int(mode), int(bool(publish_early))), "yn_stage_fuse")

    def pw_pipe(self, on=True):
        """pw_pipe_kernel among the pointwise autotune candidates (default on)."""
        self._ck(self.lib.yn_pw_pipe(self.h, int(bool(on))), "yn_pw_pipe")

    def multi_stream(self, on=True):
        """Fork independent kernel chains of one forward onto the handle's side streams (default on).  Turn off when several
        handles already run concurrently on their own streams."""
        self._ck(self.lib.yn_multi_stream(self.h, int(bool(on))), "yn_multi_stream")

    def exact_f32(self, on=True):
        """Pin every GEMM-shaped conv to the f32 MFMA (default off: the MFMA-bound layers use split-f16 operands, fp32-class)."""
        self._ck(self.lib.yn_exact_f32(self.h, int(bool(on))), "yn_exact_f32")

    def range_status(self):
        """(weights_exceed_f16, activation_overflow) of the split-f16 range guard (yn_range_status): the first says the handle fell
        back to the f32-MFMA family at fold time; the second that an activation >= 65504 was split since the last call — the
        results of those calls are invalid, re-run them with exact_f32(True).  Synchronises the stream, clears the second flag."""
        w, a = _i32(0), _i32(0)
        self._ck(self.lib.yn_range_status(self.h, ctypes.byref(w), ctypes.byref(a)), "yn_range_status")
        return bool(w.value), bool(a.value)

    def fuse_decode(self, on=True):
        """infer(): last head conv + candidate decode as one kernel (default on; bit-identical outputs either way)."""
        self._ck(self.lib.yn_fuse_decode(self.h, int(on)), "yn_fuse_decode")      # 0 off, 1 when the heads are large enough, 2 always

    def nms_prefilter(self, mode=1):
        """First-chunk prefilter of the per-class NMS: 0 off, 1 for batches of >= 4 images (default), 2 always; same kept sets."""
        self._ck(self.lib.yn_nms_prefilter(self.h, int(mode)), "yn_nms_prefilter")

    def nms_sweep(self, on=True):
        """Spread-out large class segments on nms_sweep_kernel (x-extent broad phase, exact predicate) instead of the dense tiles (default on)."""
        self._ck(self.lib.yn_nms_sweep(self.h, int(bool(on))), "yn_nms_sweep")

    def nms_sweep_segments(self, B, C):
        """Testing aid: segments of the last NMS call (B images, C classes) that nms_sweep_kernel handled."""
        return int(self.lib.yn_nms_sweep_segments(self.h, int(B), int(C)))

    # yn_nms_stages: plan[i] by name (YN_NMS_PLAN_* of the header, in order)
    NMS_PLAN_FIELDS = ("B", "N", "C", "few", "fused", "chunks", "merge", "prefilter", "pre_ranks", "sweep", "sweep_maxn", "sweep_slots",
                       "sweep_split", "resolve_one", "resolve_split", "diou")

    def nms_stages(self, B, N, C):
        """Testing aid: what the NMS chain of the last postprocess / infer / nms_merge call (B, N, C: that call's) left behind, as host
        numpy arrays (yn_nms_stages; synchronises the stream) -> dict: plan (dict of ints by NMS_PLAN_FIELDS), seg_count / seg_off [B, C],
        bucket [B, N] (sorted candidate ids per class at seg_off), sbox [B, N, 4], keep [B, N]; where plan["prefilter"] is set also
        seg_count2 [B, C], bucket2 [B, N], sbox2 [B, N, 4], seg_sparse [B, C] (None otherwise)."""
        B, N, C = int(B), int(N), int(C)
        plan = np.zeros(len(self.NMS_PLAN_FIELDS), np.int32)
        a = {"seg_count": np.zeros((B, C), np.int32), "seg_off": np.zeros((B, C), np.int32), "bucket": np.zeros((B, N), np.int32),
             "sbox": np.zeros((B, N, 4), np.float32), "seg_count2": np.zeros((B, C), np.int32), "bucket2": np.zeros((B, N), np.int32),
             "sbox2": np.zeros((B, N, 4), np.float32), "seg_sparse": np.zeros((B, C), np.int32), "keep": np.zeros((B, N), np.int32)}
        self._ck(self.lib.yn_nms_stages(self.h, B, N, C, plan.ctypes.data, *[v.ctypes.data for v in a.values()]), "yn_nms_stages")
        a["plan"] = dict(zip(self.NMS_PLAN_FIELDS, (int(v) for v in plan)))
        if not a["plan"]["prefilter"]:
            for k in ("seg_count2", "bucket2", "sbox2", "seg_sparse"):
                a[k] = None
        return a

    def down_fuse(self, on=True):
        """Main branch of the stride-2 unit of stage 2 as one kernel (default on; bit-identical outputs either way)."""
        self._ck(self.lib.yn_down_fuse(self.h, int(bool(on))), "yn_down_fuse")

    def tail_fuse(self, on=True):
        """Layers .2-.4 of the detection heads + the decode as one grouped kernel (default on; bit-identical outputs either way)."""
        self._ck(self.lib.yn_tail_fuse(self.h, int(bool(on))), "yn_tail_fuse")

    def group_launch(self, on=True):
        """The three heads' layer k / the three laterals as one grouped launch each (default on; bit-identical outputs either way)."""
        self._ck(self.lib.yn_group_launch(self.h, int(bool(on))), "yn_group_launch")

    def pw_config_count(self):
        return int(self.lib.yn_pw_config_count())

    def pw_f32_config_count(self):
        return int(self.lib.yn_pw_f32_config_count())

    def pw_families(self):
        """The two families of pointwise tile configurations: indices of the f32-MFMA one, indices of the split-f16 one."""
        n, nf = self.pw_config_count(), self.pw_f32_config_count()
        return list(range(nf)), list(range(nf, n))

    def synchronize(self):
        self._ck(self.lib.yn_synchronize(self.h), "yn_synchronize")

    # ---- weights
    def load_param(self, key, value):
        """value: numpy array / CPU tensor (host copy) or a GPU tensor (device copy)."""
        if isinstance(value, torch.Tensor) and value.is_cuda:
            v = value.detach()
            if v.dtype != torch.float32 and v.dtype != torch.int64:
                v = v.float()
            v = v.contiguous()
            shape = (ctypes.c_int64 * max(v.dim(), 1))(*v.shape)
            self._ck(self.lib.yn_load_param_dev(self.h, key.encode(), v.data_ptr(), shape, v.dim()), "yn_load_param_dev(%s)" % key)
            return
        import numpy as np
        a = value.detach().cpu().numpy() if isinstance(value, torch.Tensor) else np.asarray(value)
        if a.dtype != np.int64:
            a = np.ascontiguousarray(a, dtype=np.float32)
        shape = (ctypes.c_int64 * max(a.ndim, 1))(*a.shape)
        self._ck(self.lib.yn_load_param(self.h, key.encode(), a.ctypes.data, shape, a.ndim), "yn_load_param(%s)" % key)

    def load_state_dict(self, sd):
        for k, v in sd.items():
            self.load_param(k, v)

    def fold_bn(self):
        self._ck(self.lib.yn_fold_bn(self.h), "yn_fold_bn")

    def get_folded(self, conv_key, weight_shape):
        import numpy as np
        w = np.empty(weight_shape, dtype=np.float32)
        b = np.empty((weight_shape[0],), dtype=np.float32)
        self._ck(self.lib.yn_get_folded(self.h, conv_key.encode(), w.ctypes.data, b.ctypes.data), "yn_get_folded")
        return w, b

    # ---- network
    def head_shapes(self, B):
        return [(B, self.H // s, self.W // s, self.head_ch) for s in arch.STRIDES]

    def forward_raw(self, x, out=None):
        """x: cuda float32 NCHW [B,3,H,W] (the grid's canvas) -> three NHWC head tensors."""
        B = x.shape[0]
        assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape[1:]) == (3, self.H, self.W), (x.shape, self.H, self.W)
        x = self._in(x)
        if out is None:
            out = [torch.empty(s, dtype=torch.float32, device=x.device) for s in self.head_shapes(B)]
        self._ck(self.lib.yn_forward_raw(self.h, x.data_ptr(), B, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr()), "yn_forward_raw")
        return out

    def forward_taps(self, x):
        """The backbone taps (c3, c4, c5) of ShuffleNetV2.forward, NHWC."""
        B = x.shape[0]
        assert tuple(x.shape[1:]) == (3, self.H, self.W), (x.shape, self.H, self.W)
        ch = arch.STAGE_CH[self.backbone]
        outs = [torch.empty((B, self.H // st, self.W // st, c), dtype=torch.float32, device=x.device) for st, c in zip((8, 16, 32), ch)]
        self._ck(self.lib.yn_forward_taps(self.h, self._in(x).data_ptr(), B, *[o.data_ptr() for o in outs]), "yn_forward_taps")
        return outs

    def score_full(self, heads):
        B = heads[0].shape[0]
        N = self.N
        bbox = torch.empty((B, N, 4), dtype=torch.float32, device=heads[0].device)
        cls = torch.empty((B, N, self.C), dtype=torch.float32, device=heads[0].device)
        self._ck(self.lib.yn_score_full(self.h, _ptr(heads[0]), _ptr(heads[1]), _ptr(heads[2]), B, bbox.data_ptr(), cls.data_ptr()), "yn_score_full")
        return bbox, cls

    def decode_boxes(self, txtytwth):
        t = self._in(txtytwth)
        B = t.shape[0]
        out = torch.empty((B, self.N, 4), dtype=torch.float32, device=t.device)
        self._ck(self.lib.yn_decode_boxes(self.h, t.data_ptr(), B, out.data_ptr()), "yn_decode_boxes")
        return out

    def create_grid(self, S):
        """S: the square input size, or (H, W) of a rectangular canvas (yn_create_grid_rect)."""
        import numpy as np
        H, W = (int(S[0]), int(S[1])) if isinstance(S, (tuple, list)) else (int(S), int(S))
        HW = sum((H // s) * (W // s) for s in arch.STRIDES)
        g = np.empty((1, HW, 1, 2), np.float32)
        st = np.empty((1, HW, self.A, 2), np.float32)
        an = np.empty((1, HW, self.A, 2), np.float32)
        if isinstance(S, (tuple, list)):
            self._ck(self.lib.yn_create_grid_rect(self.h, H, W, g.ctypes.data, st.ctypes.data, an.ctypes.data), "yn_create_grid_rect")
        else:
            self._ck(self.lib.yn_create_grid(self.h, H, g.ctypes.data, st.ctypes.data, an.ctypes.data), "yn_create_grid")
        return g, st, an

    # ---- post-processing
    def nms(self, dets, scores, thresh, diou=False):
        n = int(scores.shape[0])
        keep = torch.empty((max(n, 1),), dtype=torch.int32, device=dets.device)
        cnt = torch.zeros((1,), dtype=torch.int32, device=dets.device)
        self._ck(self.lib.yn_nms(self.h, _ptr(self._in(dets)), _ptr(self._in(scores)), n, float(thresh), int(bool(diou)),
                                 keep.data_ptr(), cnt.data_ptr()), "yn_nms")
        return keep[: int(cnt.item())]

    def alloc_outputs(self, B, N=None, device=None):
        N = self.N if N is None else N
        device = self.device if device is None else device
        return (torch.empty((B, N, 4), dtype=torch.float32, device=device),
                torch.empty((B, N), dtype=torch.float32, device=device),
                torch.empty((B, N), dtype=torch.int32, device=device),
                torch.empty((B, N), dtype=torch.int32, device=device),
                torch.zeros((B,), dtype=torch.int32, device=device))

    def postprocess(self, all_local, all_conf, out=None):
        """all_local [B,N,4], all_conf [B,N,C] cuda float32 -> (boxes, scores, cls, index, count) device buffers"""
        B, N, C = all_conf.shape
        out = self.alloc_outputs(B, N, all_conf.device) if out is None else out
        self._ck(self.lib.yn_postprocess(self.h, _ptr(self._in(all_local)), _ptr(self._in(all_conf)), B, N, C,
                                         *[o.data_ptr() for o in out]), "yn_postprocess")
        return out

    def infer(self, x, out=None):
        B = x.shape[0]
        assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape[1:]) == (3, self.H, self.W), (x.shape, self.H, self.W)
        x = self._in(x)
        out = self.alloc_outputs(B, device=x.device) if out is None else out
        self._ck(self.lib.yn_infer(self.h, x.data_ptr(), B, *[o.data_ptr() for o in out]), "yn_infer")
        return out                                              # out[4] (counts) NEGATIVE = range mark (yn_range_status): check before slicing with it

    def pack_detections(self, out, rec=None, offsets=None):
        """Kept rows of all images of `out` (infer / postprocess outputs) as one record list rec [B*N, 6] = x1,y1,x2,y2,score,class
        (first offsets[B] rows valid) + offsets [B+1] int32, both on the device (yn_pack_detections)."""
        boxes, scores, cls, _, count = out
        B, N = scores.shape
        rec = torch.empty((B * N, 6), dtype=torch.float32, device=scores.device) if rec is None else rec
        offsets = torch.empty((B + 1,), dtype=torch.int32, device=scores.device) if offsets is None else offsets
        self._ck(self.lib.yn_pack_detections(self.h, boxes.data_ptr(), scores.data_ptr(), cls.data_ptr(), count.data_ptr(), B, N,
                                             rec.data_ptr(), offsets.data_ptr()), "yn_pack_detections")
        return rec, offsets

    def detections_to_host(self, out):
        """models/yolo_nano.py:370-376 for a whole batch with two device-to-host copies: -> list of B (bboxes [K,4] f32,
        scores [K] f32, cls_inds [K] i64) numpy triples, fresh and writable."""
        try:
            rec, offsets = self.pack_detections(out)
            off = offsets.cpu().numpy()
            if int(off[-1]) < 0:                                # compact_kernel's range mark, carried through pack_kernel
                raise YnRangeError("yn_infer: an activation exceeded the split-f16 range (|x| >= 65504); results invalid, re-run under exact_f32")
        except YnRangeError:
            self.range_status()                                 # the exception IS the report: acknowledge, so that the flag does not poison later calls
            raise
        return records_to_host(rec, off)

    # ---- training loss
    def loss(self, conf, cls, txtytwth, target, grads=True, out=None):
        """tools.loss + iou_score + decode on the reference's split prediction layout.
        -> (losses [4] device tensor, (g_conf, g_cls, g_txtytwth) or None); out: the three gradient tensors to write into."""
        B = cls.shape[0]
        conf, cls, t, target = (self._in(v) for v in (conf, cls, txtytwth, target))
        losses = torch.empty((4,), dtype=torch.float32, device=cls.device)
        g = (None, None, None)
        if grads:
            g = (torch.empty_like(conf), torch.empty_like(cls), torch.empty_like(t)) if out is None else tuple(out)
            for v, like in zip(g, (conf, cls, t)):
                assert v.is_cuda and v.is_contiguous() and v.dtype == torch.float32 and v.shape == like.shape
        self._ck(self.lib.yn_loss(self.h, conf.data_ptr(), cls.data_ptr(), t.data_ptr(), target.data_ptr(), B, losses.data_ptr(),
                                  _ptr(g[0]), _ptr(g[1]), _ptr(g[2])), "yn_loss")
        return losses, (g if grads else None)

    def loss_heads(self, heads, target, grads=True, out=None):
        """Same, directly on the three raw NHWC head tensors; gradients come back in the head layout (out: the three tensors to write into)."""
        B = heads[0].shape[0]
        target = self._in(target)
        losses = torch.empty((4,), dtype=torch.float32, device=target.device)
        g = [None, None, None]
        if grads:
            g = [torch.empty_like(t) for t in heads] if out is None else list(out)
            for v, like in zip(g, heads):
                assert v.is_cuda and v.is_contiguous() and v.dtype == torch.float32 and v.shape == like.shape
        self._ck(self.lib.yn_loss_heads(self.h, _ptr(heads[0]), _ptr(heads[1]), _ptr(heads[2]), target.data_ptr(), B, losses.data_ptr(),
                                        _ptr(g[0]), _ptr(g[1]), _ptr(g[2])), "yn_loss_heads")
        return losses, (g if grads else None)

    def sgd_step(self, params, grads, momentum_buf, lr, momentum=0.9, weight_decay=5e-4, grad_scale=1.0, first_step=False):
        """In-place SGD on flat float32 buffers (train.py:167-171); grad_scale = 1/world_size after a sum all-reduce."""
        assert params.is_contiguous() and grads.is_contiguous() and momentum_buf.is_contiguous() and params.numel() == grads.numel() == momentum_buf.numel()
        self._ck(self.lib.yn_sgd_step(self.h, params.data_ptr(), grads.data_ptr(), momentum_buf.data_ptr(), params.numel(),
                                      float(lr), float(momentum), float(weight_decay), float(grad_scale), int(bool(first_step))), "yn_sgd_step")

    def preprocess(self, img_u8, rw, rh, left, top, side, mean, std, out=None):
        """ValTransforms on the device: uint8 [h0,w0,3] BGR CUDA tensor -> float32 [3,side,side] (yn_preprocess)."""
        assert img_u8.dtype == torch.uint8 and img_u8.dim() == 3 and img_u8.shape[2] == 3 and img_u8.is_contiguous() and img_u8.is_cuda
        h0, w0 = int(img_u8.shape[0]), int(img_u8.shape[1])
        if out is None:
            out = torch.empty((3, side, side), dtype=torch.float32, device=self.device)
        assert out.is_contiguous() and out.dtype == torch.float32 and out.numel() == 3 * side * side
        m = (ctypes.c_float * 3)(*[float(v) for v in mean])
        sd = (ctypes.c_float * 3)(*[float(v) for v in std])
        self._ck(self.lib.yn_preprocess(self.h, img_u8.data_ptr(), h0, w0, int(rw), int(rh), int(left), int(top), int(side),
                                        ctypes.cast(m, ctypes.c_void_p), ctypes.cast(sd, ctypes.c_void_p), out.data_ptr()), "yn_preprocess")
        return out

    def preprocess_batch(self, imgs_u8, geoms, side, mean, std, out=None):
        """n images in one launch per 32 (yn_preprocess_batch): imgs_u8 = list of uint8 [h0,w0,3] CUDA tensors, geoms = list of
        (rw, rh, left, top) -> float32 [n,3,side,side]."""
        n = len(imgs_u8)
        if out is None:
            out = torch.empty((n, 3, side, side), dtype=torch.float32, device=self.device)
        assert out.is_contiguous() and out.dtype == torch.float32 and out.numel() == n * 3 * side * side
        ptrs = (ctypes.c_void_p * max(n, 1))()
        geom = (ctypes.c_int32 * (6 * max(n, 1)))()
        for i, (im, g) in enumerate(zip(imgs_u8, geoms)):
            assert im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3 and im.is_contiguous() and im.is_cuda
            ptrs[i] = im.data_ptr()
            geom[6 * i:6 * i + 6] = [int(im.shape[0]), int(im.shape[1]), int(g[0]), int(g[1]), int(g[2]), int(g[3])]
        m = (ctypes.c_float * 3)(*[float(v) for v in mean])
        sd = (ctypes.c_float * 3)(*[float(v) for v in std])
        self._ck(self.lib.yn_preprocess_batch(self.h, n, ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(geom, ctypes.c_void_p), int(side),
                                              ctypes.cast(m, ctypes.c_void_p), ctypes.cast(sd, ctypes.c_void_p), out.data_ptr()), "yn_preprocess_batch")
        return out

    def preprocess_batch_rect(self, imgs_u8, geoms, side, window, mean, std, out=None):
        """The window (left, top, W, H) of what preprocess_batch writes for the same arguments (yn_preprocess_batch_rect) -> float32 [n,3,H,W];
        a window that cuts into an image's resized extent is refused."""
        n = len(imgs_u8)
        wl, wt, ww, wh = (int(v) for v in window)
        if out is None:
            out = torch.empty((n, 3, wh, ww), dtype=torch.float32, device=self.device)
        assert out.is_contiguous() and out.dtype == torch.float32 and out.numel() == n * 3 * wh * ww
        ptrs = (ctypes.c_void_p * max(n, 1))()
        geom = (ctypes.c_int32 * (6 * max(n, 1)))()
        for i, (im, g) in enumerate(zip(imgs_u8, geoms)):
            assert im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3 and im.is_contiguous() and im.is_cuda
            ptrs[i] = im.data_ptr()
            geom[6 * i:6 * i + 6] = [int(im.shape[0]), int(im.shape[1]), int(g[0]), int(g[1]), int(g[2]), int(g[3])]
        m = (ctypes.c_float * 3)(*[float(v) for v in mean])
        sd = (ctypes.c_float * 3)(*[float(v) for v in std])
        self._ck(self.lib.yn_preprocess_batch_rect(self.h, n, ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(geom, ctypes.c_void_p), int(side), wl, wt, ww, wh,
                                                   ctypes.cast(m, ctypes.c_void_p), ctypes.cast(sd, ctypes.c_void_p), out.data_ptr()), "yn_preprocess_batch_rect")
        return out

    def train_transform_batch(self, imgs_u8, geom, photo, side, mean, std, out=None):
        """TrainTransforms' pixel work for n frames, one launch per 32 (yn_train_transform_batch): imgs_u8 = list of uint8 [h0,w0,3]
        CUDA tensors, geom = int32 [n,12], photo = float32 [n,7] (the rows the header documents) -> float32 [n,3,side,side]."""
        n = len(imgs_u8)
        geom = np.ascontiguousarray(geom, dtype=np.int32).reshape(n, 12)
        photo = np.ascontiguousarray(photo, dtype=np.float32).reshape(n, 7)
        if out is None:
            out = torch.empty((n, 3, side, side), dtype=torch.float32, device=self.device)
        assert out.is_contiguous() and out.dtype == torch.float32 and out.numel() == n * 3 * side * side
        ptrs = (ctypes.c_void_p * max(n, 1))()
        for i, im in enumerate(imgs_u8):
            assert im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3 and im.is_contiguous() and im.is_cuda
            assert (int(im.shape[0]), int(im.shape[1])) == (int(geom[i, 0]), int(geom[i, 1])), "frame %d does not match its record" % i
            ptrs[i] = im.data_ptr()
        m = (ctypes.c_float * 3)(*[float(v) for v in mean])
        sd = (ctypes.c_float * 3)(*[float(v) for v in std])
        self._ck(self.lib.yn_train_transform_batch(self.h, n, ctypes.cast(ptrs, ctypes.c_void_p), geom.ctypes.data_as(ctypes.c_void_p),
                                                   photo.ctypes.data_as(ctypes.c_void_p), int(side), ctypes.cast(m, ctypes.c_void_p),
                                                   ctypes.cast(sd, ctypes.c_void_p), out.data_ptr()), "yn_train_transform_batch")
        return out

    def mosaic_transform_batch(self, imgs_u8, geom, photo, mosaic_size, side, mean, std, out=None):
        """The pixel work of n mosaic samples (yn_mosaic_transform_batch): imgs_u8 = list of 4n uint8 [h0,w0,3] CUDA tensors (four
        frames per mosaic, in load_mosaic's order), geom = int32 [n,50], photo = float32 [n,7] (the rows the header documents) ->
        float32 [n,3,side,side]."""
        n = len(imgs_u8) // 4
        assert len(imgs_u8) == 4 * n
        geom = np.ascontiguousarray(geom, dtype=np.int32).reshape(n, 50)
        photo = np.ascontiguousarray(photo, dtype=np.float32).reshape(n, 7)
        if out is None:
            out = torch.empty((n, 3, side, side), dtype=torch.float32, device=self.device)
        assert out.is_contiguous() and out.dtype == torch.float32 and out.numel() == n * 3 * side * side
        ptrs = (ctypes.c_void_p * max(4 * n, 1))()
        for i, im in enumerate(imgs_u8):
            assert im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3 and im.is_contiguous() and im.is_cuda
            assert (int(im.shape[0]), int(im.shape[1])) == (int(geom[i // 4, 12 * (i % 4)]), int(geom[i // 4, 12 * (i % 4) + 1])), \
                "frame %d of mosaic %d does not match its record" % (i % 4, i // 4)
            ptrs[i] = im.data_ptr()
        m = (ctypes.c_float * 3)(*[float(v) for v in mean])
        sd = (ctypes.c_float * 3)(*[float(v) for v in std])
        self._ck(self.lib.yn_mosaic_transform_batch(self.h, n, ctypes.cast(ptrs, ctypes.c_void_p), geom.ctypes.data_as(ctypes.c_void_p),
                                                    photo.ctypes.data_as(ctypes.c_void_p), int(mosaic_size), int(side),
                                                    ctypes.cast(m, ctypes.c_void_p), ctypes.cast(sd, ctypes.c_void_p), out.data_ptr()),
                 "yn_mosaic_transform_batch")
        return out

    def resize_batch(self, x, size, flip_pairs=False, out=None):
        """x float32 [B,3,S0,S0] on the device -> [B,3,size,size], with flip_pairs [2B,3,size,size] (image 2b the resize, 2b + 1 its
        horizontal mirror): the library's bilinear resize (yn_resize_batch; align_corners False, no antialias)."""
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3 and x.shape[2] == x.shape[3], tuple(x.shape)
        x = self._in(x)
        B, S0, s = int(x.shape[0]), int(x.shape[2]), int(size)
        nb = 2 * B if flip_pairs else B
        if out is None:
            out = torch.empty((nb, 3, s, s), dtype=torch.float32, device=x.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and out.numel() == nb * 3 * s * s
        self._ck(self.lib.yn_resize_batch(self.h, x.data_ptr(), B, S0, s, int(bool(flip_pairs)), out.data_ptr()), "yn_resize_batch")
        return out

    def nms_merge(self, boxes, scores, cls, num_classes, nms_thresh, diou=False):
        """Per-class NMS over a detection list (TTA merge, utils/misc.py:132-146) -> (boxes [K,4], scores [K], cls [K], index [K])."""
        n = int(boxes.shape[0])
        boxes = self._in(boxes); scores = self._in(scores); cls = self._in(cls, torch.int32)
        ob = torch.empty((max(n, 1), 4), dtype=torch.float32, device=self.device)
        osc = torch.empty((max(n, 1),), dtype=torch.float32, device=self.device)
        oc = torch.empty((max(n, 1),), dtype=torch.int32, device=self.device)
        oi = torch.empty((max(n, 1),), dtype=torch.int32, device=self.device)
        cnt = torch.zeros((1,), dtype=torch.int32, device=self.device)
        self._ck(self.lib.yn_nms_merge(self.h, boxes.data_ptr(), scores.data_ptr(), cls.data_ptr(), n, int(num_classes), float(nms_thresh),
                                       int(bool(diou)), ob.data_ptr(), osc.data_ptr(), oc.data_ptr(), oi.data_ptr(), cnt.data_ptr()), "yn_nms_merge")
        k = int(cnt.item())
        return ob[:k], osc[:k], oc[:k], oi[:k]

    def wbf_merge(self, boxes, scores, cls, num_classes, iou_thresh, expected=1, assign=False):
        """Weighted box fusion over a detection list (yn_wbf_merge) -> (boxes [K,4], scores [K], cls [K], founder row [K],
        votes [K]), with assign=True also the founder row of every input row's cluster [n]."""
        n = int(boxes.shape[0])
        boxes = self._in(boxes); scores = self._in(scores); cls = self._in(cls, torch.int32)
        ob = torch.empty((max(n, 1), 4), dtype=torch.float32, device=self.device)
        osc = torch.empty((max(n, 1),), dtype=torch.float32, device=self.device)
        oc, oi, ov, asg = (torch.empty((max(n, 1),), dtype=torch.int32, device=self.device) for _ in range(4))
        cnt = torch.zeros((1,), dtype=torch.int32, device=self.device)
        self._ck(self.lib.yn_wbf_merge(self.h, boxes.data_ptr(), scores.data_ptr(), cls.data_ptr(), n, int(num_classes), float(iou_thresh),
                                       int(expected), ob.data_ptr(), osc.data_ptr(), oc.data_ptr(), oi.data_ptr(), ov.data_ptr(),
                                       asg.data_ptr() if assign else None, cnt.data_ptr()), "yn_wbf_merge")
        k = int(cnt.item())
        out = (ob[:k], osc[:k], oc[:k], oi[:k], ov[:k])
        return out + (asg[:n],) if assign else out

    def soft_nms_merge(self, boxes, scores, cls, num_classes, method, iou_thresh=0.5, sigma=0.5, score_floor=0.001):
        """Soft-NMS over a detection list (yn_soft_nms_merge) -> (boxes [K,4], scores [K] decayed, cls [K], row [K]), the kept
        rows in ascending row order.  method: SOFT_HARD / SOFT_LINEAR / SOFT_GAUSSIAN or its name."""
        n = int(boxes.shape[0])
        method = soft_method_id(method) if isinstance(method, str) else int(method)
        boxes = self._in(boxes); scores = self._in(scores); cls = self._in(cls, torch.int32)
        ob = torch.empty((max(n, 1), 4), dtype=torch.float32, device=self.device)
        osc = torch.empty((max(n, 1),), dtype=torch.float32, device=self.device)
        oc, oi = (torch.empty((max(n, 1),), dtype=torch.int32, device=self.device) for _ in range(2))
        cnt = torch.zeros((1,), dtype=torch.int32, device=self.device)
        self._ck(self.lib.yn_soft_nms_merge(self.h, boxes.data_ptr(), scores.data_ptr(), cls.data_ptr(), n, int(num_classes), method,
                                            float(iou_thresh), float(sigma), float(score_floor), ob.data_ptr(), osc.data_ptr(), oc.data_ptr(),
                                            oi.data_ptr(), cnt.data_ptr()), "yn_soft_nms_merge")
        k = int(cnt.item())
        return ob[:k], osc[:k], oc[:k], oi[:k]

    def soft_nms(self, method, sigma=0.5, score_floor=0.0):
        """How the NMS inside infer() / postprocess() suppresses from now on (yn_soft_nms): None / SOFT_OFF = the NMS chain as before, else
        "hard" / "linear" / "gaussian" (or SOFT_*) at the handle's nms_thresh.  score_floor: rows at or below it are dropped."""
        method = soft_method_id(method) if method is None or isinstance(method, str) else int(method)
        self._ck(self.lib.yn_soft_nms(self.h, method, float(sigma), float(score_floor)), "yn_soft_nms")

    def soft_exp(self, x):
        """Testing aid (yn_op_soft_exp): E(x), the exp of the gaussian method, elementwise over a float32 tensor."""
        x = self._in(x)
        y = torch.empty_like(x)
        self._ck(self.lib.yn_op_soft_exp(self.h, _ptr(x), _ptr(y), x.numel()), "yn_op_soft_exp")
        return y

    def ema_update(self, ema, model, decay):
        """ema = ema * d + (1 - d) * model, in place (utils/misc.py:83-86); float32 tensors of equal size on this device."""
        assert ema.is_contiguous() and model.is_contiguous() and ema.numel() == model.numel() and ema.dtype == model.dtype == torch.float32
        self._ck(self.lib.yn_ema_update(self.h, ema.data_ptr(), model.data_ptr(), ema.numel(), float(decay)), "yn_ema_update")

    # ---- training labels
    def make_targets(self, label_lists, anchor_size, out=None):
        """tools.multi_gt_creator (tools.py:97-216): list (per image) of [xmin, ymin, xmax, ymax, class] rows ->
        float32 device tensor [B, N, 11].  The (tiny) label table crosses PCIe once; the assignment runs on the GPU."""
        import numpy as np
        B = len(label_lists)
        counts = [len(l) for l in label_lists]
        flat = np.zeros((max(sum(counts), 1), 5), dtype=np.float64)
        if sum(counts):
            flat[:sum(counts)] = np.array([row for l in label_lists for row in l], dtype=np.float64).reshape(-1, 5)
        offs = np.zeros(B + 1, dtype=np.int32)
        offs[1:] = np.cumsum(counts)
        anchors = np.ascontiguousarray(np.array(anchor_size, dtype=np.float64).reshape(-1))
        if anchors.size != 6 * self.A:
            raise YnError("anchor_size must hold %d [w,h] pairs" % (3 * self.A))
        d_flat = torch.from_numpy(flat).to(self.device, non_blocking=True)
        d_offs = torch.from_numpy(offs).to(self.device, non_blocking=True)
        if out is None:
            out = torch.empty((B, self.N, 11), dtype=torch.float32, device=self.device)
        self._ck(self.lib.yn_make_targets(self.h, d_flat.data_ptr(), d_offs.data_ptr(), B, anchors.ctypes.data, out.data_ptr()), "yn_make_targets")
        return out

    # ---- training step
    def train_bind(self):
        """Allocate the flat parameter / gradient / momentum buffers and bind them (parameters = the loaded state dict)."""
        n = int(self.lib.yn_train_param_count(self.h))
        self.flat_params = torch.empty(n, dtype=torch.float32, device=self.device)
        self.flat_grads = torch.empty(n, dtype=torch.float32, device=self.device)
        self.flat_momentum = torch.empty(n, dtype=torch.float32, device=self.device)
        self._ck(self.lib.yn_train_bind(self.h, self.flat_params.data_ptr(), self.flat_grads.data_ptr(), self.flat_momentum.data_ptr(), n), "yn_train_bind")
        return n

    def train_precision(self, dtype="f32"):
        """Arithmetic of train_step: "f32" (the reference's own) or "f16" (fp16 storage + f16 MFMA, fp32 master weights, loss scaling)."""
        self._ck(self.lib.yn_train_precision(self.h, {"f32": 0, "fp32": 0, "f16": 1, "fp16": 1}[dtype]), "yn_train_precision")

    def allreduce_grads(self, nccl_comm):
        """All-reduce(sum) the flat gradient buffer in place over an RCCL communicator (an ncclComm_t as an int / c_void_p) on the
        handle's stream: the torch-free form of the gradient exchange (yn_allreduce_grads)."""
        self._ck(self.lib.yn_allreduce_grads(self.h, ctypes.c_void_p(nccl_comm if isinstance(nccl_comm, int) else nccl_comm.value)), "yn_allreduce_grads")

    def loss_scale(self):
        """(scale, clean steps) of the fp16 step's dynamic loss scale (yn_train_get_loss_scale; synchronises)."""
        s, c = _f32(0), _f32(0)
        self._ck(self.lib.yn_train_get_loss_scale(self.h, ctypes.byref(s), ctypes.byref(c)), "yn_train_get_loss_scale")
        return float(s.value), float(c.value)

    def set_loss_scale(self, scale, clean_steps=0.0):
        """Restore the loss scale (and its clean-step counter) of a checkpoint (yn_train_set_loss_scale)."""
        self._ck(self.lib.yn_train_set_loss_scale(self.h, float(scale), float(clean_steps)), "yn_train_set_loss_scale")

    def skipped_steps(self):
        n = ctypes.c_int64(0)
        self._ck(self.lib.yn_train_skipped_steps(self.h, ctypes.byref(n)), "yn_train_skipped_steps")
        return int(n.value)

    def head_fork(self, force=None):
        """The fp16 step's head-tower fork decision (yn_train_head_fork): None = query, False / True = pin it.  -> -1 undecided, 0, 1."""
        d = ctypes.c_int(-1)
        self._ck(self.lib.yn_train_head_fork(self.h, 0 if force is None else (2 if force else 1), ctypes.byref(d)), "yn_train_head_fork")
        return int(d.value)

    def param_slice(self, key):
        off, num = ctypes.c_int64(), ctypes.c_int64()
        self._ck(self.lib.yn_train_param_offset(self.h, key.encode(), ctypes.byref(off), ctypes.byref(num)), "yn_train_param_offset")
        return slice(off.value, off.value + num.value)

    def train_step(self, x, target, lr=1e-3, momentum=0.9, weight_decay=5e-4, grad_scale=1.0, update=True):
        """-> losses [4] (conf, cls, bbox, iou) device tensor; gradients are left in self.flat_grads."""
        B = x.shape[0]
        x, target = self._in(x), self._in(target)
        losses = torch.empty((4,), dtype=torch.float32, device=x.device)
        self._ck(self.lib.yn_train_step(self.h, x.data_ptr(), target.data_ptr(), B, float(lr), float(momentum), float(weight_decay),
                                        float(grad_scale), int(bool(update)), losses.data_ptr()), "yn_train_step")
        return losses

    def train_forward(self, x):
        """Train-mode forward only (batch statistics; running statistics updated) -> three NHWC float32 raw heads."""
        B = x.shape[0]
        outs = [torch.empty(s, dtype=torch.float32, device=x.device) for s in self.head_shapes(B)]
        self._ck(self.lib.yn_train_forward(self.h, self._in(x).data_ptr(), B, *[o.data_ptr() for o in outs]), "yn_train_forward")
        return outs

    def read_param(self, key, shape):
        import numpy as np
        a = np.empty(shape, dtype=np.float32)
        self._ck(self.lib.yn_read_param(self.h, key.encode(), a.ctypes.data, a.size), "yn_read_param(%s)" % key)
        return a

    # ---- measurement
    def profile_enable(self, on=True):
        self._ck(self.lib.yn_profile_enable(self.h, int(bool(on))), "yn_profile_enable")

    def profile_records(self):
        """[(layer name, kernel symbol, ms, algorithmic flops, algorithmic bytes)] of the last profiled call."""
        n = self.lib.yn_profile_count(self.h)
        recs = []
        name = ctypes.create_string_buffer(96)
        kern = ctypes.create_string_buffer(96)
        ms, fl, by = _f32(), ctypes.c_double(), ctypes.c_double()
        for i in range(n):
            self._ck(self.lib.yn_profile_get(self.h, i, name, 96, kern, 96, ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)), "yn_profile_get")
            recs.append((name.value.decode(), kern.value.decode(), ms.value, fl.value, by.value))
        return recs

    # ---- single operators (NHWC device tensors; weights in torch layout on the device) -----------
    def op_dwconv3x3(self, x, w, bias, stride=1, act=0):
        B, H, W, C = x.shape
        y = torch.empty((B, (H - 1) // stride + 1, (W - 1) // stride + 1, C), dtype=torch.float32, device=x.device)
        self._ck(self.lib.yn_op_dwconv3x3(self.h, _ptr(self._in(x)), B, H, W, C, stride, _ptr(self._in(w)),
                                          _ptr(self._in(bias)) if bias is not None else None, act, y.data_ptr()), "yn_op_dwconv3x3")
        return y

    def op_pwconv(self, x, w, bias, act=0):
        B, H, W, Cin = x.shape
        Cout = w.shape[0]
        y = torch.empty((B, H, W, Cout), dtype=torch.float32, device=x.device)
        self._ck(self.lib.yn_op_pwconv(self.h, _ptr(self._in(x)), B, H, W, Cin, Cout, _ptr(self._in(w)),
                                       _ptr(self._in(bias)) if bias is not None else None, act, y.data_ptr()), "yn_op_pwconv")
        return y

    def op_pwconv_group(self, members, act=0, out=None):
        """Up to three pointwise convs as one grouped launch (yn_op_pwconv_group).  members: [(x, w, bias)], x a contiguous [M, Cin] tensor or
        (wide, off): columns [off, off + Cin) of a contiguous [M, ld] tensor; out: None (new [M, Cout] tensors) or [(wide, off)] per member.
        Returns the output tensors ([M, Cout] views of `wide` where out is given)."""
        n = len(members)
        keep, xs, ws, bs, ys, ret = [], [], [], [], [], []
        in_ld, in_off, Ms, Cin, out_ld, out_off = [], [], [], [], [], []
        Cout = members[0][1].shape[0]
        for p, (x, w, bias) in enumerate(members):
            xt, off = x if isinstance(x, tuple) else (x, 0)
            assert xt.dim() == 2 and xt.is_contiguous() and xt.dtype == torch.float32 and w.shape[0] == Cout
            w, bias = self._in(w), (self._in(bias) if bias is not None else None)
            keep += [w, bias]
            xs.append(xt.data_ptr()); in_ld.append(xt.shape[1]); in_off.append(off); Ms.append(xt.shape[0]); Cin.append(w.shape[1])
            ws.append(w.data_ptr()); bs.append(bias.data_ptr() if bias is not None else 0)
            if out is None:
                yt, yoff = torch.empty((xt.shape[0], Cout), dtype=torch.float32, device=xt.device), 0
            else:
                yt, yoff = out[p]
                assert yt.dim() == 2 and yt.is_contiguous() and yt.dtype == torch.float32 and yt.shape[0] == xt.shape[0]
            ys.append(yt.data_ptr()); out_ld.append(yt.shape[1]); out_off.append(yoff)
            ret.append(yt[:, yoff:yoff + Cout])
        pa = lambda v: (ctypes.c_void_p * n)(*v)
        ia = lambda v: (ctypes.c_int32 * n)(*[int(q) for q in v])
        self._ck(self.lib.yn_op_pwconv_group(self.h, n, pa(xs), ia(in_ld), ia(in_off), ia(Ms), ia(Cin), int(Cout), pa(ws), pa(bs), int(act),
                                             pa(ys), ia(out_ld), ia(out_off)), "yn_op_pwconv_group")
        return ret

    def op_pwconv_shuffle(self, x, passthrough, w, bias, act=0):
        B, H, W, Cin = x.shape
        Cout = w.shape[0]
        y = torch.empty((B, H, W, 2 * Cout), dtype=torch.float32, device=x.device)
        self._ck(self.lib.yn_op_pwconv_shuffle(self.h, self._in(x).data_ptr(), self._in(passthrough).data_ptr(), B, H, W, Cin, Cout,
                                               self._in(w).data_ptr(), _ptr(bias), act, y.data_ptr()), "yn_op_pwconv_shuffle")
        return y

    def op_conv3x3(self, x, w, bias, act=0, x2=None, resample=0):
        B, H, W, Cin = x.shape
        Cout = w.shape[0]
        y = torch.empty((B, H, W, Cout), dtype=torch.float32, device=x.device)
        self._ck(self.lib.yn_op_conv3x3(self.h, _ptr(self._in(x)), _ptr(self._in(x2)) if x2 is not None else None, resample,
                                        B, H, W, Cin, Cout, _ptr(self._in(w)),
                                        _ptr(self._in(bias)) if bias is not None else None, act, y.data_ptr()), "yn_op_conv3x3")
        return y

    def op_stem(self, x_nchw, w, bias, act=0):
        B, _, H, W = x_nchw.shape
        Cout = w.shape[0]
        y = torch.empty((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cout), dtype=torch.float32, device=x_nchw.device)
        self._ck(self.lib.yn_op_stem(self.h, _ptr(self._in(x_nchw)), B, H, W, Cout, _ptr(self._in(w)),
                                     _ptr(self._in(bias)) if bias is not None else None, act, y.data_ptr()), "yn_op_stem")
        return y

    def op_stem_pool(self, x_nchw, w, bias, act=0):
        """The network's fused stem: conv 3x3 s2 + activation + max pool 3x3 s2, NCHW in, pooled NHWC out."""
        B, _, H, W = x_nchw.shape
        Cout = w.shape[0]
        Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        y = torch.empty((B, (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1, Cout), dtype=torch.float32, device=x_nchw.device)
        self._ck(self.lib.yn_op_stem_pool(self.h, _ptr(self._in(x_nchw)), B, H, W, Cout, _ptr(self._in(w)),
                                          _ptr(self._in(bias)) if bias is not None else None, act, y.data_ptr()), "yn_op_stem_pool")
        return y

    def op_maxpool(self, x):
        B, H, W, C = x.shape
        y = torch.empty((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), dtype=torch.float32, device=x.device)
        self._ck(self.lib.yn_op_maxpool3x3s2(self.h, _ptr(self._in(x)), B, H, W, C, y.data_ptr()), "yn_op_maxpool3x3s2")
        return y

    def op_shuffle_block(self, block, x, cout, stride):
        B, H, W, _ = x.shape
        y = torch.empty((B, (H - 1) // stride + 1, (W - 1) // stride + 1, cout), dtype=torch.float32, device=x.device)
        self._ck(self.lib.yn_op_shuffle_block(self.h, block.encode(), _ptr(self._in(x)), B, H, W, y.data_ptr()), "yn_op_shuffle_block")
        return y

    def op_down_unit(self, block, x, cout):
        """A stride-2 block as the one-kernel unit (down_unit_pipe_kernel) on any even map; raises where that kernel does not cover it."""
        B, H, W, _ = x.shape
        y = torch.empty((B, H // 2, W // 2, cout), dtype=torch.float32, device=x.device)
        self._ck(self.lib.yn_op_down_unit(self.h, block.encode(), _ptr(self._in(x)), B, H, W, y.data_ptr()), "yn_op_down_unit")
        return y

    def op_decode_cand(self, heads, conf_thresh):
        """The candidate decode alone on dense raw NHWC heads [B,H,W,A(5+C)] x 3 (decode_kernel<false, KMAX>) ->
        (boxes [B,N,4], best score [B,N], class [B,N] int32, -1 below conf_thresh)."""
        heads = [self._in(t) for t in heads]
        B = heads[0].shape[0]
        for t, hw in zip(heads, self.head_shapes(B)):
            assert t.is_cuda and tuple(t.shape) == hw, (tuple(t.shape), hw)
        boxes, scores, cls, _, _ = self.alloc_outputs(B, device=heads[0].device)
        self._ck(self.lib.yn_op_decode_cand(self.h, heads[0].data_ptr(), heads[1].data_ptr(), heads[2].data_ptr(), B, float(conf_thresh),
                                            boxes.data_ptr(), scores.data_ptr(), cls.data_ptr()), "yn_op_decode_cand")
        return boxes, scores, cls

    def op_head_tail(self, xs):
        """The heads from the output of their layer .1 (xs: three NHWC [B,S/8 (16, 32),same,96] activations) to the candidate arrays, with
        the handle's weights, switches and conf_thresh (yn_op_head_tail) -> (boxes [B,N,4], best score [B,N], class [B,N] int32)."""
        xs = [self._in(t) for t in xs]
        B = xs[0].shape[0]
        for t, s in zip(xs, arch.STRIDES):
            assert t.is_cuda and tuple(t.shape) == (B, self.H // s, self.W // s, arch.NECK_CH), (tuple(t.shape), self.H, self.W, s)
        boxes, scores, cls, _, _ = self.alloc_outputs(B, device=xs[0].device)
        self._ck(self.lib.yn_op_head_tail(self.h, xs[0].data_ptr(), xs[1].data_ptr(), xs[2].data_ptr(), B,
                                          boxes.data_ptr(), scores.data_ptr(), cls.data_ptr()), "yn_op_head_tail")
        return boxes, scores, cls

    def op_h16_conv(self, kind, x, w, bias=None, stride=1, dy=None, gapped=False):
        """One conv kernel of the fp16 training step (+ its two gradient kernels when dy is given): x [B,H,W,Cin] fp32 NHWC,
        kind 0 pw / 1 dw / 2 dense3x3 -> (y, dx, dw) fp32 (dx, dw None without dy)."""
        B, H, W, Cin = x.shape
        Cout = w.shape[0]
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        y = torch.empty((B, Ho, Wo, Cout), dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x) if dy is not None else None
        dw = torch.empty_like(w) if dy is not None else None
        self._ck(self.lib.yn_op_h16_conv(self.h, int(kind), self._in(x).data_ptr(), B, H, W, Cin, int(bool(gapped)), self._in(w).data_ptr(), _ptr(bias),
                                         Cout, int(stride), _ptr(self._in(dy) if dy is not None else None), y.data_ptr(), _ptr(dx), _ptr(dw)), "yn_op_h16_conv")
        return y, dx, dw

    def op_h16_bn(self, y, gamma, beta, act=0, dz=None):
        M, C = y.shape
        z = torch.empty_like(y)
        dy = torch.empty_like(y) if dz is not None else None
        dg = torch.empty((C,), dtype=torch.float32, device=y.device) if dz is not None else None
        db = torch.empty((C,), dtype=torch.float32, device=y.device) if dz is not None else None
        self._ck(self.lib.yn_op_h16_bn(self.h, self._in(y).data_ptr(), _ptr(self._in(dz) if dz is not None else None), M, C, gamma.data_ptr(), beta.data_ptr(),
                                       int(act), z.data_ptr(), _ptr(dy), _ptr(dg), _ptr(db)), "yn_op_h16_bn")
        return z, dy, dg, db

    def op_h16_bn2(self, y, gamma, beta, act=0, dz=None):
        """op_h16_bn with the saved statistics: -> (z, dy, dgamma, dbeta, mean, invstd)."""
        M, C = y.shape
        mk = lambda *shape: torch.empty(shape, dtype=torch.float32, device=y.device)
        z, mean, invstd = torch.empty_like(y), mk(C), mk(C)
        dy, dg, db = (torch.empty_like(y), mk(C), mk(C)) if dz is not None else (None, None, None)
        keep = [self._in(y), self._in(dz) if dz is not None else None]
        self._ck(self.lib.yn_op_h16_bn2(self.h, keep[0].data_ptr(), _ptr(keep[1]), M, C, gamma.data_ptr(), beta.data_ptr(), int(act), z.data_ptr(),
                                        _ptr(dy), _ptr(dg), _ptr(db), mean.data_ptr(), invstd.data_ptr()), "yn_op_h16_bn2")
        return z, dy, dg, db, mean, invstd

    def train_graph(self, enable=None):
        """Switch the fp16 step's hipGraph replay (None: leave); -> number of steps served from a graph so far."""
        n = ctypes.c_int64(0)
        self._ck(self.lib.yn_train_graph(self.h, -1 if enable is None else int(bool(enable)), ctypes.byref(n)), "yn_train_graph")
        return int(n.value)

    def op_h16_gemm_stats(self, kind, x, w, gapped=False, dy=None, y_below=None, mean=None, invstd=None, gamma=None, beta=None, act=0):
        """hgemm with its HColStat epilogue: -> y, sums_fwd (numpy double [2][Cout]) and, with dy, dx, sums_bwd ([2][Cin])."""
        import numpy as np
        B, H, W, Cin = x.shape
        Cout = w.shape[0]
        y = torch.empty((B, H, W, Cout), dtype=torch.float32, device=x.device)
        sf = np.zeros((2, Cout), np.float64)
        dx = torch.empty_like(x) if dy is not None else None
        sb = np.zeros((2, Cin), np.float64) if dy is not None else None
        keep = [self._in(t) if t is not None else None for t in (x, w, dy, y_below, mean, invstd, gamma, beta)]
        self._ck(self.lib.yn_op_h16_gemm_stats(self.h, int(kind), keep[0].data_ptr(), B, H, W, Cin, int(bool(gapped)), keep[1].data_ptr(), Cout, y.data_ptr(),
                                               sf.ctypes.data, _ptr(keep[2]), _ptr(keep[3]), _ptr(keep[4]), _ptr(keep[5]), _ptr(keep[6]), _ptr(keep[7]), int(act),
                                               _ptr(dx), sb.ctypes.data if sb is not None else None), "yn_op_h16_gemm_stats")
        return y, sf, dx, sb

    def op_h16_bn_unit(self, y, passthrough, gamma, beta, act=0, dunit=None):
        """BatchNorm as the last layer of a ShuffleV2 unit: -> unit [M][2C] (and dy, deven, dgamma, dbeta when dunit [M][2C] is given)."""
        M, C = y.shape
        unit = torch.empty((M, 2 * C), dtype=torch.float32, device=y.device)
        mk = lambda *shape: torch.empty(shape, dtype=torch.float32, device=y.device) if dunit is not None else None
        dy, dev, dg, db = mk(M, C), mk(M, C), mk(C), mk(C)
        yc, pc, dc = self._in(y), self._in(passthrough), (self._in(dunit) if dunit is not None else None)
        self._ck(self.lib.yn_op_h16_bn_unit(self.h, yc.data_ptr(), pc.data_ptr(), _ptr(dc), M, C, gamma.data_ptr(), beta.data_ptr(), int(act),
                                            unit.data_ptr(), _ptr(dy), _ptr(dev), _ptr(dg), _ptr(db)), "yn_op_h16_bn_unit")
        return unit, dy, dev, dg, db

    def op_h16_conv2(self, kind, x, w, bias=None, stride=1, dy=None, gapped=False, x_off=0, cin=None, dx=None, dx_off=0, accumulate=False, partial_cap=0,
                     stat=0, below=None, want=("dx", "dw", "dbias")):
        """op_h16_conv with the step's own argument forms (include/yolonano_hip.h): x [B,H,W,x_ld] read at channels [x_off, x_off + cin); `dx`
        given: the tensor [B,H,W,dx_ld] the input gradient is written (accumulate: added) into at [dx_off, dx_off + cin), else a zeroed one like
        the conv's input; stat 1 / 2: the depthwise run kernel's statistics (below = (y_below, mean, invstd, gamma, beta, act) for 2).
        -> dict y and, with dy, those of dx, dw, dbias named in `want`; sums_fwd / sums_bwd (numpy double [2][C])."""
        import numpy as np
        x = self._in(x)
        B, H, W, x_ld = x.shape
        Cin = int(cin) if cin is not None else x_ld - int(x_off)
        Cout = w.shape[0]
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        mk = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)
        out = {"y": mk(B, Ho, Wo, Cout)}
        keep = [self._in(t) if t is not None else None for t in (w, bias, dy)]
        if dy is not None:
            if "dx" in want:
                out["dx"] = torch.zeros((B, H, W, Cin), dtype=torch.float32, device=x.device) if dx is None else dx
            if "dw" in want:
                out["dw"] = torch.empty_like(keep[0])
            if "dbias" in want:
                out["dbias"] = mk(Cout)
        sf = np.zeros((2, Cin), np.float64) if stat == 1 else None
        sb = np.zeros((2, Cin), np.float64) if stat == 2 else None
        bl = [self._in(t) for t in below[:5]] if below is not None else [None] * 5
        act = int(below[5]) if below is not None else 0
        dxt = out.get("dx")
        self._ck(self.lib.yn_op_h16_conv2(self.h, int(kind), x.data_ptr(), B, H, W, Cin, int(bool(gapped)), x_ld, int(x_off), keep[0].data_ptr(), _ptr(keep[1]),
                                          Cout, int(stride), _ptr(keep[2]), int(bool(accumulate)), dxt.shape[3] if dxt is not None else Cin, int(dx_off),
                                          int(partial_cap), int(stat), _ptr(bl[0]), _ptr(bl[1]), _ptr(bl[2]), _ptr(bl[3]), _ptr(bl[4]), act,
                                          out["y"].data_ptr(), _ptr(dxt), _ptr(out.get("dw")), _ptr(out.get("dbias")),
                                          sf.ctypes.data if sf is not None else None, sb.ctypes.data if sb is not None else None), "yn_op_h16_conv2")
        if sf is not None:
            out["sums_fwd"] = sf
        if sb is not None:
            out["sums_bwd"] = sb
        return out

    def op_h16_stem(self, x_nchw, w, bias=None, dy=None):
        """The fp16 step's stem conv over x [B,3,H,W] -> (y [B,Ho,Wo,24], dw like w or None)."""
        x = self._in(x_nchw)
        B, _, H, W = x.shape
        y = torch.empty((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 24), dtype=torch.float32, device=x.device)
        keep = [self._in(t) if t is not None else None for t in (w, bias, dy)]
        dw = torch.empty_like(keep[0]) if dy is not None else None
        self._ck(self.lib.yn_op_h16_stem(self.h, x.data_ptr(), B, H, W, keep[0].data_ptr(), _ptr(keep[1]), _ptr(keep[2]), y.data_ptr(), _ptr(dw)), "yn_op_h16_stem")
        return y, dw

    def op_h16_maxpool(self, x, dy=None):
        """The fp16 step's max pool over x [B,H,W,C]: -> (y, idx uint8 window positions, dx or None)."""
        x = self._in(x)
        B, H, W, C = x.shape
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        y = torch.empty((B, Ho, Wo, C), dtype=torch.float32, device=x.device)
        idx = torch.empty((B, Ho, Wo, C), dtype=torch.uint8, device=x.device)
        dx = torch.empty_like(x) if dy is not None else None
        dyc = self._in(dy) if dy is not None else None
        self._ck(self.lib.yn_op_h16_maxpool(self.h, x.data_ptr(), B, H, W, C, _ptr(dyc), y.data_ptr(), idx.data_ptr(), _ptr(dx)), "yn_op_h16_maxpool")
        return y, idx, dx

    def op_h16_stem_pool(self, y, gamma, beta, act=1, g1=None):
        """The fused stem BatchNorm + activation + max pool of the fp16 step over the conv output y [B,H,W,24] -> dict out, idx, mean, invstd and,
        with g1 (the pooled tensor's gradient), dy, dgamma, dbeta."""
        y = self._in(y)
        B, H, W, C = y.shape
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        mk = lambda *shape: torch.empty(shape, dtype=torch.float32, device=y.device)
        out = {"out": mk(B, Ho, Wo, C), "idx": torch.empty((B, Ho, Wo, C), dtype=torch.uint8, device=y.device), "mean": mk(C), "invstd": mk(C)}
        if g1 is not None:
            out.update(dy=mk(B, H, W, C), dgamma=mk(C), dbeta=mk(C))
        keep = [self._in(t) if t is not None else None for t in (gamma, beta, g1)]
        if C != 24:
            raise YnError("yn_op_h16_stem_pool: the stem has 24 channels")
        self._ck(self.lib.yn_op_h16_stem_pool(self.h, y.data_ptr(), B, H, W, keep[0].data_ptr(), keep[1].data_ptr(), int(act), _ptr(keep[2]),
                                              out["out"].data_ptr(), out["idx"].data_ptr(), out["mean"].data_ptr(), out["invstd"].data_ptr(),
                                              _ptr(out.get("dy")), _ptr(out.get("dgamma")), _ptr(out.get("dbeta"))), "yn_op_h16_stem_pool")
        return out

    def op_h16_resample(self, mode, a, b=None, out=None):
        """hresample_kernel's four modes (as op_f32_resample); modes 2 / 3 add into `out`.  H, W are those of `a`."""
        B, H, W, C = a.shape
        if out is None:
            out = torch.empty_like(a)
        keep = [self._in(a), self._in(b) if b is not None else None]
        self._ck(self.lib.yn_op_h16_resample(self.h, int(mode), keep[0].data_ptr(), _ptr(keep[1]), out.data_ptr(), B, H, W, C), "yn_op_h16_resample")
        return out

    def op_h16_gather(self, src, dst, n, npad, src_off=0, src_cs=1, src_half=None, src_gap=0, dst_off=0, dst_cs=1, dst_half=None, dst_gap=0):
        """hgather_kernel over physical rows src [M,src_ld] -> dst [M,dst_ld] (written in place, returned)."""
        src = self._in(src)
        M, src_ld = src.shape
        dst_ld = dst.shape[1]
        self._ck(self.lib.yn_op_h16_gather(self.h, src.data_ptr(), src_ld, int(src_off), int(src_cs), int(src_ld if src_half is None else src_half), int(src_gap),
                                           dst.data_ptr(), dst_ld, int(dst_off), int(dst_cs), int(dst_ld if dst_half is None else dst_half), int(dst_gap),
                                           M, int(n), int(npad)), "yn_op_h16_gather")
        return dst

    def op_h16_grad_finish(self, g, slots, state, update=0, global_flag=0):
        """hgrad_finish_kernel (+ hscale_update_kernel: update 1 local flag, 2 global_flag) on g [n] (in place), slots [8,n]; state: numpy float32 [5]
        (word 3 is an integer flag: read it through .view(np.uint32)) -> the state afterwards."""
        import numpy as np
        st = np.ascontiguousarray(state, dtype=np.float32).copy()
        assert st.shape == (5,) and slots.shape == (8, g.numel()) and slots.is_contiguous() and g.is_contiguous()
        self._ck(self.lib.yn_op_h16_grad_finish(self.h, g.data_ptr(), slots.data_ptr(), g.numel(), st.ctypes.data, int(update), int(global_flag)), "yn_op_h16_grad_finish")
        return st

    def op_h16_loss(self, heads, target, scale=1.0, grads=True):
        """The fp16 step's loss alone (yn_op_h16_loss): dense fp32 raw heads, staged as fp16 rows of the step's width -> (losses [4] device tensor,
        the three head gradients * scale as dense fp32 or None, the count of pad-column elements of the fp16 gradient rows that are not +0)."""
        heads = [self._in(t) for t in heads]
        B = heads[0].shape[0]
        target = self._in(target)
        losses = torch.empty((4,), dtype=torch.float32, device=target.device)
        g = [torch.empty_like(t) for t in heads] if grads else [None, None, None]
        pad = _i32(-1)
        self._ck(self.lib.yn_op_h16_loss(self.h, heads[0].data_ptr(), heads[1].data_ptr(), heads[2].data_ptr(), target.data_ptr(), B, float(scale),
                                         losses.data_ptr(), _ptr(g[0]), _ptr(g[1]), _ptr(g[2]), ctypes.byref(pad)), "yn_op_h16_loss")
        return losses, (g if grads else None), int(pad.value)

    def op_f32_conv(self, kind, x, w, bias=None, stride=1, dy=None, x_off=0, cin=None, y_ld=None, dx=None, accumulate=False, partial_cap=0,
                    want=("dx", "dw", "dbias")):
        """One conv of the fp32 training step and, with dy, the gradients named in `want`: kind 0 pw / 1 dw / 2 dense3x3 over x [B,H,W,x_ld] fp32
        NHWC, reading channels [x_off, x_off + cin); kind 3 the stem over x NCHW.  -> (y [B,Ho,Wo,y_ld], dx like x, dw like w, dbias); `dx` given:
        the tensor the input gradient is written (accumulate: added) into."""
        stem = int(kind) == 3
        x = self._in(x)
        if stem:
            (B, Cin, H, W), x_ld = x.shape, 0
        else:
            B, H, W, x_ld = x.shape
            Cin = int(cin) if cin is not None else x_ld - int(x_off)
        Cout = w.shape[0]
        y_ld = Cout if y_ld is None else int(y_ld)
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        y = torch.empty((B, Ho, Wo, y_ld), dtype=torch.float32, device=x.device)
        keep = [self._in(t) if t is not None else None for t in (w, bias, dy)]
        if dy is not None and "dx" in want and not stem:
            dx = torch.zeros_like(x) if dx is None else dx
        else:
            dx = None
        dw = torch.empty_like(keep[0]) if dy is not None and "dw" in want else None
        db = torch.empty((Cout,), dtype=torch.float32, device=x.device) if dy is not None and "dbias" in want else None
        self._ck(self.lib.yn_op_f32_conv(self.h, int(kind), x.data_ptr(), B, H, W, Cin, x_ld, int(x_off), keep[0].data_ptr(), _ptr(keep[1]), Cout, int(stride),
                                         y_ld, int(partial_cap), _ptr(keep[2]), int(bool(accumulate)), y.data_ptr(), _ptr(dx), _ptr(dw), _ptr(db)), "yn_op_f32_conv")
        return y, dx, dw, db

    def op_f32_bn(self, y, gamma, beta, act=0, passthrough=None, running=None, dz=None, dz_off=0):
        """Train-mode BatchNorm + activation of the fp32 step over y [M,C]; passthrough [M,C]: the ShuffleV2 unit form (z and dz are [M,2C]).  running =
        (running_mean, running_var), updated in place.  dz [M,dz_ld] is read at channels [dz_off, dz_off + C).
        -> dict z, mean, invstd and, with dz, dy, dgamma, dbeta (unit form: deven)."""
        M, C = y.shape
        unit = passthrough is not None
        mk = lambda *shape: torch.empty(shape, dtype=torch.float32, device=y.device)
        out = {"z": mk(M, 2 * C if unit else C), "mean": mk(C), "invstd": mk(C)}
        if dz is not None:
            out.update(dy=mk(M, C), dgamma=mk(C), dbeta=mk(C))
            if unit:
                out["deven"] = mk(M, C)
        keep = [self._in(t) if t is not None else None for t in (y, gamma, beta, passthrough, dz)]
        rm, rv = running if running is not None else (None, None)
        self._ck(self.lib.yn_op_f32_bn(self.h, keep[0].data_ptr(), M, C, keep[1].data_ptr(), keep[2].data_ptr(), int(act), int(unit), _ptr(keep[3]), _ptr(rm), _ptr(rv),
                                       out["z"].data_ptr(), out["mean"].data_ptr(), out["invstd"].data_ptr(), _ptr(keep[4]),
                                       keep[4].shape[1] if dz is not None else 0, int(dz_off), _ptr(out.get("dy")), _ptr(out.get("deven")),
                                       _ptr(out.get("dgamma")), _ptr(out.get("dbeta"))), "yn_op_f32_bn")
        return out

    def op_f32_maxpool(self, x, dy=None):
        """The step's index-recording 3x3 stride-2 max pool over x [B,H,W,C]: -> (y, idx int32, dx or None)."""
        B, H, W, C = x.shape
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        y = torch.empty((B, Ho, Wo, C), dtype=torch.float32, device=x.device)
        idx = torch.empty((B, Ho, Wo, C), dtype=torch.int32, device=x.device)
        dx = torch.empty_like(x) if dy is not None else None
        keep = [self._in(x), self._in(dy) if dy is not None else None]
        self._ck(self.lib.yn_op_f32_maxpool(self.h, keep[0].data_ptr(), B, H, W, C, y.data_ptr(), idx.data_ptr(), _ptr(keep[1]), _ptr(dx)), "yn_op_f32_maxpool")
        return y, idx, dx

    def op_f32_resample(self, mode, a, b=None, out=None):
        """launch_resample's four modes (include/yolonano_hip.h); modes 2 / 3 add into `out`.  H, W are those of `a`."""
        B, H, W, C = a.shape
        if out is None:
            out = torch.empty_like(a)
        keep = [self._in(a), self._in(b) if b is not None else None]
        self._ck(self.lib.yn_op_f32_resample(self.h, int(mode), keep[0].data_ptr(), _ptr(keep[1]), out.data_ptr(), B, H, W, C), "yn_op_f32_resample")
        return out

    def to_nhwc(self, x):
        B, C, H, W = x.shape
        y = torch.empty((B, H, W, C), dtype=torch.float32, device=x.device)
        self._ck(self.lib.yn_op_nchw_to_nhwc(self.h, _ptr(self._in(x)), B, C, H, W, y.data_ptr()), "yn_op_nchw_to_nhwc")
        return y

    def to_nchw(self, x):
        B, H, W, C = x.shape
        y = torch.empty((B, C, H, W), dtype=torch.float32, device=x.device)
        self._ck(self.lib.yn_op_nhwc_to_nchw(self.h, _ptr(self._in(x)), B, C, H, W, y.data_ptr()), "yn_op_nhwc_to_nchw")
        return y


MERGE_NMS, MERGE_WBF = 0, 1                 # YN_MERGE_NMS / YN_MERGE_WBF
MERGE_RULES = {"nms": MERGE_NMS, "wbf": MERGE_WBF}


def merge_rule_id(merge):
    """"nms" / "wbf" -> YN_MERGE_*; anything else is refused by name."""
    if merge not in MERGE_RULES:
        raise ValueError("merge must be 'nms' or 'wbf', got %r" % (merge,))
    return MERGE_RULES[merge]


SOFT_OFF, SOFT_HARD, SOFT_LINEAR, SOFT_GAUSSIAN = 0, 1, 2, 3      # YN_SOFT_*
SOFT_METHODS = {None: SOFT_OFF, "hard": SOFT_HARD, "linear": SOFT_LINEAR, "gaussian": SOFT_GAUSSIAN}


def soft_method_id(soft):
    """None / "hard" / "linear" / "gaussian" -> YN_SOFT_*; anything else is refused by name."""
    if not (soft is None or isinstance(soft, str)) or soft not in SOFT_METHODS:
        raise ValueError("soft must be None, 'hard', 'linear' or 'gaussian', got %r" % (soft,))
    return SOFT_METHODS[soft]


def check_soft_with_merge(who, merge, soft):
    """Soft-NMS is how the "nms" rule suppresses: it does not combine with merge="wbf"."""
    if soft is not None and merge == "wbf":
        raise ValueError("%s: soft=%r cannot be combined with merge='wbf' (Soft-NMS is a suppression of the 'nms' rule)" % (who, soft))
    return soft_method_id(soft)


class _DeviceView:
    """A region of device memory the library owns, in the form torch.as_tensor adopts without a copy."""

    def __init__(self, ptr, shape, typestr, owner):
        self.owner = owner
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}


class _MergeObject:
    """What Tta and Slice share: the object's lifetime, the (rec, offsets) views of its result and the host arrays of its merge lists.  A subclass
    names its C functions (_destroy, _result, _soft) and sets .obj, .units (its max_batch / max_frames) and .n (the units of the result, None: no
    result)."""

    def close(self):
        if getattr(self, "obj", None):
            getattr(self.lib, self._destroy)(self.obj)
            self.obj = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def merge_soft(self, method, sigma=0.5, score_floor=0.001, handle=None):
        """How the object's MERGE_NMS rule suppresses from now on (yn_merge_soft_tta / _slice / _fuse): None / SOFT_OFF = per-class NMS as
        before, else "hard" / "linear" / "gaussian" (or SOFT_*).  Kept but unused while the rule is MERGE_WBF."""
        h = self.handle if handle is None else handle
        method = soft_method_id(method) if method is None or isinstance(method, str) else int(method)
        h._ck(getattr(self.lib, self._soft)(h.h, self.obj, method, float(sigma), float(score_floor)), self._soft)

    def _result_views(self, total, hint):
        if self.n is None:
            raise YnError("%s: no result (%s first)" % (self._result, hint))
        rec, off, n = _vp(), _vp(), _i32(0)
        if getattr(self.lib, self._result)(self.obj, ctypes.byref(rec), ctypes.byref(off), ctypes.byref(n) if total else None):
            raise YnError("%s: no result" % self._result)
        dev = self.handle.device
        r = torch.as_tensor(_DeviceView(rec.value, (self.units * self.list_capacity, 6), "<f4", self), device=dev)
        o = torch.as_tensor(_DeviceView(off.value, (self.n + 1,), "<i4", self), device=dev)
        return (r, o, int(n.value)) if total else (r, o)

    def _list_arrays(self, n):
        """boxes [n,cap,4], scores [n,cap], cls [n,cap] int32, count [max(n,1)] int32: zeroed host arrays for the lists' read-back"""
        cap = self.list_capacity
        return np.zeros((n, cap, 4), np.float32), np.zeros((n, cap), np.float32), np.zeros((n, cap), np.int32), np.zeros((max(n, 1),), np.int32)


class Tta(_MergeObject):
    """One yn_tta: test-time augmentation for whole batches.  Thin, 1:1 with the C ABI; `handle` gives the device, the anchors per cell
    and the class count, and is the default handle of infer()."""
    _destroy, _result, _soft = "yn_tta_destroy", "yn_tta_result", "yn_merge_soft_tta"

    def __init__(self, handle, scales, flip=True, max_batch=1, list_capacity=8192):
        self.lib = handle.lib
        self.handle = handle
        self.scales = [int(s) for s in scales]
        self.flip, self.max_batch, self.list_capacity = bool(flip), int(max_batch), int(list_capacity)
        self.units = self.max_batch
        self.forwards = len(self.scales) * (2 if self.flip else 1)
        arr = (ctypes.c_int32 * max(len(self.scales), 1))(*self.scales)
        t = _vp()
        handle._ck(self.lib.yn_tta_create(handle.h, ctypes.cast(arr, _vp), len(self.scales), int(self.flip), self.max_batch, self.list_capacity,
                                          ctypes.byref(t)), "yn_tta_create")
        self.obj = t
        self.n = None                                           # images of the result

    def infer(self, x, nms_thresh=0.4, handle=None):
        """x float32 [B,3,S0,S0] on the device: every scale (x flip) forward, the per-image merge and the pack (yn_tta_infer).  Raises
        YnRangeError on the split-f16 range mark, YnError naming the image when a merge list would pass list_capacity."""
        h = self.handle if handle is None else handle
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3 and x.shape[2] == x.shape[3], tuple(x.shape)
        x = h._in(x)
        self.n = None
        h._ck(self.lib.yn_tta_infer(h.h, self.obj, x.data_ptr(), int(x.shape[0]), int(x.shape[2]), float(nms_thresh)), "yn_tta_infer")
        self.n = int(x.shape[0])

    def merge_rule(self, rule, expected=0, handle=None):
        """The merge infer() ends in from now on: MERGE_NMS (default) or MERGE_WBF; expected 0 = the number of forwards (yn_merge_rule_tta)."""
        h = self.handle if handle is None else handle
        h._ck(self.lib.yn_merge_rule_tta(h.h, self.obj, int(rule), int(expected)), "yn_merge_rule_tta")

    def result(self, total=False):
        """(rec [max_batch * list_capacity, 6] float32, offsets [B+1] int32) on the device, in yn_pack_detections' layout: VIEWS of the
        object's buffers, valid until its next infer() (yn_tta_result).  total=True: also offsets[B] as an int (one read-back)."""
        return self._result_views(total, "infer()")

    def forwards_to_host(self, B, handle=None):
        """Testing aid (yn_tta_forwards): the merge lists before the NMS -> (boxes [B,cap,4], scores [B,cap], cls [B,cap] int32,
        count [B] int32, forward_start [forwards,B] int32) numpy arrays."""
        h = self.handle if handle is None else handle
        boxes, scores, cls, count = self._list_arrays(B)
        start = np.zeros((self.forwards, B), np.int32)
        h._ck(self.lib.yn_tta_forwards(h.h, self.obj, boxes.ctypes.data, scores.ctypes.data, cls.ctypes.data, count.ctypes.data, start.ctypes.data),
              "yn_tta_forwards")
        return boxes, scores, cls, count[:B], start


class Slice(_MergeObject):
    """One yn_slice: sliced inference - tiles of large frames, merged per frame.  Thin, 1:1 with the C ABI; `handle` gives the device, the
    anchors per cell and the class count, and is the default handle of every call.  Frames are uint8 [h0,w0,3] CUDA tensors, `tiles` an
    int32 [T,9] table (slicing.tile_table)."""
    _destroy, _result, _soft = "yn_slice_destroy", "yn_slice_result", "yn_merge_soft_slice"

    def __init__(self, handle, max_frames=1, list_capacity=8192):
        self.lib = handle.lib
        self.handle = handle
        self.max_frames, self.list_capacity = int(max_frames), int(list_capacity)
        self.units = self.max_frames
        s = _vp()
        handle._ck(self.lib.yn_slice_create(handle.h, self.max_frames, self.list_capacity, ctypes.byref(s)), "yn_slice_create")
        self.obj = s
        self.n = None                                           # frames of the result
        self.lists = None                                       # (F, T) of the table being appended

    @staticmethod
    def _frames(frames):
        n = len(frames)
        ptrs = (ctypes.c_void_p * max(n, 1))()
        shapes = np.zeros((max(n, 1), 2), np.int32)
        for f, im in enumerate(frames):
            assert im.is_cuda and im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3 and im.is_contiguous(), "frames are contiguous uint8 [h,w,3] on the device"
            ptrs[f] = im.data_ptr()
            shapes[f] = (int(im.shape[0]), int(im.shape[1]))
        return ptrs, shapes

    @staticmethod
    def _table(tiles):
        return np.ascontiguousarray(np.asarray(tiles, dtype=np.int32).reshape(-1, 9))

    def preprocess(self, frames, tiles, side, mean, std, out=None, handle=None):
        """The tile kernel on its own (yn_slice_preprocess) -> float32 [T,3,side,side]."""
        h = self.handle if handle is None else handle
        tiles = self._table(tiles)
        T = len(tiles)
        if out is None:
            out = torch.empty((T, 3, side, side), dtype=torch.float32, device=h.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and out.numel() == T * 3 * side * side
        ptrs, shapes = self._frames(frames)
        m = (ctypes.c_float * 3)(*[float(v) for v in mean])
        sd = (ctypes.c_float * 3)(*[float(v) for v in std])
        h._ck(self.lib.yn_slice_preprocess(h.h, T, ctypes.cast(ptrs, _vp), shapes.ctypes.data, tiles.ctypes.data, int(side), ctypes.cast(m, _vp),
                                           ctypes.cast(sd, _vp), out.data_ptr()), "yn_slice_preprocess")
        return out

    def append(self, shapes, tiles, t0, out, edge_margin=-1.0, handle=None):
        """The kept rows of one infer() over tiles t0 .. t0 + n - 1 (`out` = its five outputs, n = their batch) go to their frames' lists
        (yn_slice_append).  shapes: F rows (h0, w0).  t0 == 0 opens a new table."""
        h = self.handle if handle is None else handle
        boxes, scores, cls, _, count = out
        n, N = int(scores.shape[0]), int(scores.shape[1])
        shapes = np.ascontiguousarray(np.asarray(shapes, dtype=np.int32).reshape(-1, 2))
        tiles = self._table(tiles)
        assert boxes.is_contiguous() and scores.is_contiguous() and cls.is_contiguous() and count.is_contiguous()
        assert boxes.dtype == torch.float32 and scores.dtype == torch.float32 and cls.dtype == torch.int32 and count.dtype == torch.int32
        self.n = None
        h._ck(self.lib.yn_slice_append(h.h, self.obj, len(shapes), shapes.ctypes.data, len(tiles), tiles.ctypes.data, int(t0), n, boxes.data_ptr(),
                                       scores.data_ptr(), cls.data_ptr(), count.data_ptr(), N, float(edge_margin)), "yn_slice_append")
        self.lists = (len(shapes), len(tiles))

    def merge(self, F, nms_thresh=0.5, handle=None):
        """Per-class NMS of the F lists + pack (yn_slice_merge).  Raises YnRangeError on the range mark, YnError naming the frame when a
        list would have passed list_capacity."""
        h = self.handle if handle is None else handle
        self.n = None
        h._ck(self.lib.yn_slice_merge(h.h, self.obj, int(F), float(nms_thresh)), "yn_slice_merge")
        self.n = int(F)

    def infer(self, frames, tiles, mean, std, nms_thresh=0.5, edge_margin=-1.0, handle=None):
        """Every tile through the handle's yn_infer in chunks of its max_batch, the per-frame merge and the pack (yn_slice_infer)."""
        h = self.handle if handle is None else handle
        tiles = self._table(tiles)
        ptrs, shapes = self._frames(frames)
        m = (ctypes.c_float * 3)(*[float(v) for v in mean])
        sd = (ctypes.c_float * 3)(*[float(v) for v in std])
        self.n = None
        self.lists = (len(frames), len(tiles))
        h._ck(self.lib.yn_slice_infer(h.h, self.obj, len(frames), ctypes.cast(ptrs, _vp), shapes.ctypes.data, len(tiles), tiles.ctypes.data,
                                      ctypes.cast(m, _vp), ctypes.cast(sd, _vp), float(nms_thresh), float(edge_margin)), "yn_slice_infer")
        self.n = len(frames)

    def merge_rule(self, rule, expected=0, handle=None):
        """The merge merge() / infer() apply from now on: MERGE_NMS (default) or MERGE_WBF; expected 0 = 1 (yn_merge_rule_slice)."""
        h = self.handle if handle is None else handle
        h._ck(self.lib.yn_merge_rule_slice(h.h, self.obj, int(rule), int(expected)), "yn_merge_rule_slice")

    def result(self, total=False):
        """(rec [max_frames * list_capacity, 6] float32, offsets [F+1] int32) on the device, in yn_pack_detections' layout: VIEWS of the
        object's buffers, valid until its next call (yn_slice_result).  total=True: also offsets[F] as an int (one read-back)."""
        return self._result_views(total, "infer() or merge()")

    def lists_to_host(self, handle=None):
        """Testing aid (yn_slice_lists): the merge lists before the NMS -> (boxes [F,cap,4], scores [F,cap], cls [F,cap] int32,
        count [F] int32, tile_start [T] int32) numpy arrays."""
        h = self.handle if handle is None else handle
        if self.lists is None:
            raise YnError("yn_slice_lists: no table (append() or infer() first)")
        F, T = self.lists
        boxes, scores, cls, count = self._list_arrays(F)
        start = np.zeros((max(T, 1),), np.int32)
        h._ck(self.lib.yn_slice_lists(h.h, self.obj, boxes.ctypes.data, scores.ctypes.data, cls.ctypes.data, count.ctypes.data, start.ctypes.data),
              "yn_slice_lists")
        return boxes, scores, cls, count[:F], start[:T]


class Fuse(_MergeObject):
    """One yn_fuse: record lists fused per unit - ensembles of models, or a TTA result with a sliced one.  Thin, 1:1 with the C ABI."""
    _destroy, _result, _soft = "yn_fuse_destroy", "yn_fuse_result", "yn_merge_soft_fuse"

    def __init__(self, handle, max_units=1, list_capacity=8192):
        self.lib = handle.lib
        self.handle = handle
        self.max_units, self.list_capacity = int(max_units), int(list_capacity)
        self.units = self.max_units
        f = _vp()
        handle._ck(self.lib.yn_fuse_create(handle.h, self.max_units, self.list_capacity, ctypes.byref(f)), "yn_fuse_create")
        self.obj = f
        self.n = None                                           # units of the result
        self.lists = None                                       # units of the open lists

    def open(self, B, handle=None):
        """Empties the B lists (yn_fuse_open)."""
        h = self.handle if handle is None else handle
        self.n = None
        h._ck(self.lib.yn_fuse_open(h.h, self.obj, int(B)), "yn_fuse_open")
        self.lists = int(B)

    def append(self, rec, offsets, weight=1.0, handle=None):
        """(rec, offsets [B+1]) in yn_pack_detections' layout, on the device: unit b's rows go to the end of list b, score * weight
        (yn_fuse_append)."""
        h = self.handle if handle is None else handle
        assert rec.is_cuda and rec.is_contiguous() and rec.dtype == torch.float32 and offsets.is_cuda and offsets.dtype == torch.int32
        self.n = None
        h._ck(self.lib.yn_fuse_append(h.h, self.obj, int(offsets.numel()) - 1, rec.data_ptr(), offsets.data_ptr(), float(weight)), "yn_fuse_append")

    def merge(self, B, rule=MERGE_WBF, thresh=0.55, expected=0, handle=None):
        """One read-back, the merge of the B lists by `rule` and the pack (yn_fuse_merge); expected 0 = the appends since open()."""
        h = self.handle if handle is None else handle
        self.n = None
        h._ck(self.lib.yn_fuse_merge(h.h, self.obj, int(B), int(rule), float(thresh), int(expected)), "yn_fuse_merge")
        self.n = int(B)

    def result(self, total=False):
        """(rec [max_units * list_capacity, 6] float32, offsets [B+1] int32) on the device: VIEWS of the object's buffers, valid until its
        next call (yn_fuse_result)."""
        return self._result_views(total, "merge()")

    def lists_to_host(self, handle=None):
        """Testing aid (yn_fuse_lists): the merge lists -> (boxes [B,cap,4], scores [B,cap], cls [B,cap] int32, count [B] int32)."""
        h = self.handle if handle is None else handle
        if self.lists is None:
            raise YnError("yn_fuse_lists: no lists (open() first)")
        B = self.lists
        boxes, scores, cls, count = self._list_arrays(B)
        h._ck(self.lib.yn_fuse_lists(h.h, self.obj, boxes.ctypes.data, scores.ctypes.data, cls.ctypes.data, count.ctypes.data), "yn_fuse_lists")
        return boxes, scores, cls, count[:B]
