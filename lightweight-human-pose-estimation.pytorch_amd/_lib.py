"""ctypes binding of the C-ABI library (include/lwpose.h).  Fails loudly when the HIP library
is missing: there is no CPU fallback anywhere in the product path."""
import ctypes as C
import os

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, "liblwpose_hip.so")

LWP_OK, LWP_ERR_ARG, LWP_ERR_HIP, LWP_ERR_STATE, LWP_ERR_CAPACITY, LWP_ERR_NOGPU, LWP_ERR_UNBOUND, LWP_ERR_INTERNAL = 0, -1, -2, -3, -4, -5, -6, -7
MEM_HOST, MEM_DEVICE = 0, 1
JPEG_ENTROPY_HOST, JPEG_ENTROPY_DEVICE = 0, 1
JPEG_ENTROPY_MODES = {"host": JPEG_ENTROPY_HOST, "device": JPEG_ENTROPY_DEVICE}
JPEG_SUBSAMPLINGS = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}
F32, BF16, F16 = 0, 1, 2
TRAIN_STAGES, TRAIN_CPM, TRAIN_ALL = 0, 1, 2
TRAIN_SCOPES = {"stages": TRAIN_STAGES, "cpm": TRAIN_CPM, "all": TRAIN_ALL}
KEPT_OUTPUT, KEPT_DEPTHWISE, KEPT_NO_RESIDUAL = 0, 1, 2
PAD_GRAPH, PAD_RAW = 0, 1
PAD_MODES = {"graph": PAD_GRAPH, "raw": PAD_RAW}
BACKWARD_PRECISIONS = {"fp32": F32, "bf16": BF16, "fp16": F16}

EXPORTS = [
    "lwp_version", "lwp_param_count", "lwp_param_spec", "lwp_create", "lwp_destroy", "lwp_last_error",
    "lwp_set_capacity", "lwp_load_weights", "lwp_weights_blob_bytes", "lwp_weights_blob_export",
    "lwp_weights_blob_import", "lwp_forward", "lwp_upsample", "lwp_extract_keypoints", "lwp_group_keypoints",
    "lwp_infer_poses", "lwp_infer_poses_async", "lwp_fetch_poses", "lwp_time_pipeline", "lwp_profile_classes",
    "lwp_synchronize", "lwp_poses_from_maps", "lwp_layer_count", "lwp_layer_info", "lwp_debug_layer_output",
    "lwp_profile_launches", "lwp_debug_time_layer", "lwp_pipeline_submit", "lwp_pipeline_fetch", "lwp_multiscale_accumulate",
    "lwp_preprocess_dims", "lwp_preprocess_u8", "lwp_scale_dims", "lwp_preprocess_scaled_u8", "lwp_debug_layer_variant", "lwp_set_stream", "lwp_preprocess_scaled_f32", "lwp_debug_frames_per_pass", "lwp_debug_post_counts",
    "lwp_debug_f32_to_f16", "lwp_set_skeleton", "lwp_get_skeleton", "lwp_debug_post_counts_ex",
    "lwp_debug_post_generic", "lwp_debug_live_resources", "lwp_debug_graph_fusions",
    "lwp_set_tracking", "lwp_set_unmap", "lwp_reset_tracking", "lwp_get_poses", "lwp_track_poses", "lwp_debug_tracking_near",
    "lwp_preprocess_u8_batch", "lwp_pipeline_submit_u8",
    "lwp_set_overlay", "lwp_get_overlay", "lwp_draw_poses",
    "lwp_train_targets", "lwp_mask_downsample", "lwp_stage_losses", "lwp_time_train_targets", "lwp_time_stage_losses",
    "lwp_train_forward", "lwp_stage_backward", "lwp_stage_grad_count", "lwp_stage_grad_spec", "lwp_profile_stage_backward",
    "lwp_debug_train_activation", "lwp_debug_backward_splits",
    "lwp_stage_adam_group", "lwp_stage_adam_step", "lwp_stage_params_get", "lwp_stage_adam_state_get", "lwp_stage_adam_state_set",
    "lwp_stage_adam_reset", "lwp_time_stage_adam_step",
    "lwp_set_train_scope", "lwp_train_grad_count", "lwp_train_grad_spec", "lwp_train_adam_group", "lwp_train_backward",
    "lwp_debug_train_copy", "lwp_debug_backward_dw_splits", "lwp_debug_dw_grad_sd", "lwp_debug_stem_wgrad",
    "lwp_debug_conv_grad", "lwp_debug_dw_grad", "lwp_debug_loss_grad", "lwp_debug_relu_mask", "lwp_debug_grad_add", "lwp_debug_elu_grad",
    "lwp_debug_pw_fold", "lwp_debug_bn_chain",
    "lwp_augment_batch", "lwp_time_augment_batch",
    "lwp_crowd_masks", "lwp_time_crowd_masks", "lwp_augment_batch_crowd",
    "lwp_coco_eval", "lwp_debug_coco_oks",
    "lwp_coco_open", "lwp_coco_release", "lwp_coco_reset", "lwp_coco_add_maps", "lwp_coco_add_rows", "lwp_coco_counts",
    "lwp_coco_rows", "lwp_coco_finish", "lwp_debug_coco_rows",
    "lwp_jpeg_info", "lwp_debug_jpeg_blocks", "lwp_jpeg_decode_batch", "lwp_time_jpeg_decode_batch",
    "lwp_set_jpeg_entropy", "lwp_debug_jpeg_entropy_batch", "lwp_debug_jpeg_scan", "lwp_time_jpeg_entropy_batch",
    "lwp_jpeg_encode_bound", "lwp_jpeg_encode_batch", "lwp_debug_jpeg_encode_blocks", "lwp_debug_jpeg_encode_header",
    "lwp_time_jpeg_encode_batch", "lwp_debug_jpeg_encode_scan",
    "lwp_set_backward_precision", "lwp_get_backward_precision",
    "lwp_stage_losses_log", "lwp_loss_log_read",
]


class AugmentPlan(C.Structure):
    """lwp_augment_plan of include/lwpose.h: the geometry of one sample of lwp_augment_batch."""
    _fields_ = [("image", C.c_void_p), ("mask", C.c_void_p), ("rs_scale", C.c_double), ("m", C.c_double * 6), ("mem", C.c_int),
                ("src_h", C.c_int), ("src_w", C.c_int), ("rs_h", C.c_int), ("rs_w", C.c_int), ("area", C.c_int),
                ("bound_h", C.c_int), ("bound_w", C.c_int), ("should_crop", C.c_int),
                ("dst_y0", C.c_int), ("dst_y1", C.c_int), ("dst_x0", C.c_int), ("dst_x1", C.c_int),
                ("img_y0", C.c_int), ("img_x0", C.c_int), ("flip", C.c_int),
                ("warp_pad", C.c_ubyte * 3), ("crop_pad", C.c_ubyte * 3)]


class JpegHeader(C.Structure):
    """lwp_jpeg_header of include/lwpose.h: what lwp_jpeg_info reports of one file."""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("components", C.c_int),
                ("h_samp", C.c_int * 3), ("v_samp", C.c_int * 3), ("quant_table", C.c_int * 3),
                ("restart_interval", C.c_int), ("mcus_x", C.c_int), ("mcus_y", C.c_int), ("orientation", C.c_int),
                ("blocks_w", C.c_int * 3), ("blocks_h", C.c_int * 3), ("total_blocks", C.c_int64)]


class CapacityError(RuntimeError):
    """A peak / key-point / connection / pose list overflowed its configured capacity."""


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "lwpose_amd: %s is missing — build it first (python __graft_entry__.py build, or "
            "python lightweight-human-pose-estimation.pytorch_amd/build.py). There is no CPU fallback." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    # Array parameters that callers fill from numpy / torch buffers are c_void_p (they pass the address); scalars keep their exact
    # types and small out-parameters their typed pointers.  tests/test_abi_closure.py holds every list against include/lwpose.h.
    vp, ip, i64p, fp, dp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_double)
    L.lwp_version.restype = C.c_int
    results = [vp, vp, C.c_int, vp, C.c_int, vp]          # counts, key-points and their capacity, entries and theirs, entry counts
    L.lwp_param_count.argtypes = [C.c_int] * 4
    L.lwp_param_spec.argtypes = [C.c_int] * 5 + [C.c_char_p, C.c_int, i64p, ip, ip]
    L.lwp_create.argtypes = [C.c_int] * 6 + [C.POINTER(vp)]
    L.lwp_destroy.argtypes = [vp]
    L.lwp_last_error.argtypes = [vp]
    L.lwp_last_error.restype = C.c_char_p
    L.lwp_set_capacity.argtypes = [vp] + [C.c_int] * 4
    L.lwp_load_weights.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(vp), vp, vp, C.c_int]
    L.lwp_weights_blob_bytes.argtypes = [vp, C.POINTER(C.c_size_t)]
    L.lwp_weights_blob_export.argtypes = [vp, vp, C.c_size_t]
    L.lwp_weights_blob_import.argtypes = [vp, vp, C.c_size_t]
    L.lwp_forward.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp), C.c_int]
    L.lwp_upsample.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int]
    L.lwp_extract_keypoints.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int64, C.c_int64, vp, vp, vp, C.c_int, ip]
    L.lwp_group_keypoints.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, ip]
    L.lwp_infer_poses.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int] + results
    L.lwp_infer_poses_async.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.lwp_fetch_poses.argtypes = [vp] + results
    L.lwp_time_pipeline.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, fp]
    L.lwp_profile_classes.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, fp, ip]
    L.lwp_synchronize.argtypes = [vp]
    L.lwp_poses_from_maps.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int] + results
    L.lwp_profile_launches.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, fp, ip, C.c_int, ip]
    L.lwp_debug_time_layer.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, fp]
    L.lwp_pipeline_submit.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.lwp_pipeline_fetch.argtypes = [vp, C.c_int] + results
    L.lwp_multiscale_accumulate.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, ip, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int]
    L.lwp_preprocess_dims.argtypes = [C.c_int] * 4 + [ip] * 5 + [dp]
    L.lwp_preprocess_u8.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, C.c_double, vp]
    L.lwp_scale_dims.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_int] + [ip] * 5
    L.lwp_preprocess_scaled_u8.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, dp, dp, C.c_double, vp]
    L.lwp_preprocess_scaled_f32.argtypes = L.lwp_preprocess_scaled_u8.argtypes
    L.lwp_layer_count.argtypes = [vp]
    L.lwp_layer_info.argtypes = [vp, C.c_int, C.c_char_p, C.c_int] + [ip] * 6 + [i64p]
    L.lwp_debug_layer_output.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, ip]
    L.lwp_debug_layer_variant.argtypes = [vp, C.c_int, C.c_char_p, C.c_int]
    L.lwp_set_stream.argtypes = [vp, vp, C.c_int]
    L.lwp_debug_frames_per_pass.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.lwp_debug_post_counts.argtypes = [vp, C.c_int] + [C.POINTER(C.c_int)] * 4
    L.lwp_debug_f32_to_f16.argtypes = [vp, vp, C.c_int64]
    L.lwp_set_skeleton.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_double]
    L.lwp_get_skeleton.argtypes = [vp, ip, ip, vp, vp, C.c_int, ip, dp]
    L.lwp_debug_post_counts_ex.argtypes = [vp, C.c_int] + [ip] * 4 + [C.c_int, C.c_int]
    L.lwp_debug_post_generic.argtypes = [vp]
    L.lwp_debug_live_resources.argtypes = [i64p]
    L.lwp_debug_graph_fusions.argtypes = [C.c_int] * 7 + [ip, C.c_char_p, C.c_int, C.c_int, ip]
    L.lwp_set_tracking.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_int, vp, C.c_int]
    L.lwp_set_unmap.argtypes = [vp, C.c_int, C.c_double, C.c_int, C.c_int]
    L.lwp_reset_tracking.argtypes = [vp, C.c_int, C.c_int]
    L.lwp_get_poses.argtypes = [vp, C.c_int] + [vp] * 6 + [C.c_int]
    L.lwp_track_poses.argtypes = [vp, C.c_int, C.c_int] + [vp] * 5 + [ip, C.POINTER(C.c_uint)]
    L.lwp_debug_tracking_near.argtypes = [vp, C.c_int, vp, C.c_int]
    L.lwp_preprocess_u8_batch.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, C.c_double, vp]
    L.lwp_pipeline_submit_u8.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, C.c_double, C.c_int, C.c_int, C.c_int]
    L.lwp_set_overlay.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int]
    L.lwp_get_overlay.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int]
    L.lwp_draw_poses.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, C.c_int]
    L.lwp_train_targets.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, vp, vp]
    L.lwp_mask_downsample.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.lwp_stage_losses.argtypes = [vp, C.POINTER(vp), C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, dp]
    L.lwp_time_train_targets.argtypes = L.lwp_train_targets.argtypes + [C.c_int, fp]
    L.lwp_time_stage_losses.argtypes = L.lwp_stage_losses.argtypes[:-1] + [C.c_int, fp]
    L.lwp_train_forward.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.lwp_stage_backward.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, vp, vp]
    L.lwp_stage_grad_count.argtypes = [C.c_int] * 4 + [i64p]
    L.lwp_stage_grad_spec.argtypes = [C.c_int] * 5 + [C.c_char_p, C.c_int, i64p, ip, i64p]
    L.lwp_profile_stage_backward.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, vp, vp, C.c_int, fp, ip]
    L.lwp_debug_train_activation.argtypes = [vp, C.c_int, vp, C.c_size_t, ip]
    L.lwp_debug_backward_splits.argtypes = [vp, C.c_int]
    L.lwp_stage_adam_group.argtypes = [C.c_int] * 5 + [ip, ip]
    L.lwp_stage_adam_step.argtypes = [vp, vp] + [C.c_double] * 5
    L.lwp_stage_params_get.argtypes = [vp, vp]
    L.lwp_stage_adam_state_get.argtypes = [vp, vp, vp, i64p]
    L.lwp_stage_adam_state_set.argtypes = [vp, vp, vp, C.c_int64]
    L.lwp_stage_adam_reset.argtypes = [vp]
    L.lwp_time_stage_adam_step.argtypes = [vp, vp] + [C.c_double] * 5 + [C.c_int, fp]
    L.lwp_set_train_scope.argtypes = [vp, C.c_int]
    L.lwp_train_grad_count.argtypes = [C.c_int] * 5 + [i64p]
    L.lwp_train_grad_spec.argtypes = [C.c_int] * 6 + [C.c_char_p, C.c_int, i64p, ip, i64p]
    L.lwp_train_adam_group.argtypes = [C.c_int] * 6 + [ip, ip]
    L.lwp_train_backward.argtypes = L.lwp_stage_backward.argtypes + [vp]
    L.lwp_debug_train_copy.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t, ip]
    L.lwp_debug_backward_dw_splits.argtypes = [vp, C.c_int]
    L.lwp_debug_dw_grad_sd.argtypes = [vp, vp, vp, vp] + [C.c_int] * 7 + [vp, vp, vp, ip]
    L.lwp_debug_stem_wgrad.argtypes = [vp, vp, vp] + [C.c_int] * 4 + [vp, vp, ip]
    L.lwp_debug_conv_grad.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp] + [C.c_int] * 12 + [vp, C.c_int, C.c_int, vp, vp, ip]
    L.lwp_debug_dw_grad.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp] + [C.c_int] * 7 + [vp, C.c_int, vp, ip]
    L.lwp_debug_loss_grad.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int, vp, vp, vp] + [C.c_int] * 4 + [C.c_float]
    L.lwp_debug_relu_mask.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int64, C.c_int]
    L.lwp_debug_grad_add.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_int64, C.c_int, C.c_int]
    L.lwp_debug_elu_grad.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_int64, C.c_int]
    L.lwp_debug_pw_fold.argtypes = [vp] * 5 + [C.c_int] * 2
    L.lwp_debug_bn_chain.argtypes = [vp] * 12 + [C.c_int] * 3
    L.lwp_augment_batch.argtypes = [vp, C.POINTER(AugmentPlan)] + [C.c_int] * 4 + [vp, vp, vp]
    L.lwp_time_augment_batch.argtypes = L.lwp_augment_batch.argtypes + [C.c_int, fp]
    L.lwp_crowd_masks.argtypes = [vp] * 6 + [C.c_int, vp, vp]
    L.lwp_time_crowd_masks.argtypes = L.lwp_crowd_masks.argtypes + [C.c_int, fp]
    L.lwp_augment_batch_crowd.argtypes = [vp, C.POINTER(AugmentPlan)] + [C.c_int] * 4 + [vp] * 6
    coco_in = [vp, C.c_int] + [vp] * 9
    L.lwp_coco_eval.argtypes = coco_in + [vp] * 4
    L.lwp_debug_coco_oks.argtypes = coco_in + [C.c_int, ip, ip, vp, C.c_int64, vp, vp, ip]
    L.lwp_coco_open.argtypes = [vp, C.c_int] + [vp] * 6 + [C.c_int]
    L.lwp_coco_release.argtypes = [vp]
    L.lwp_coco_reset.argtypes = [vp]
    L.lwp_coco_add_maps.argtypes = [vp, vp, vp] + [C.c_int] * 6 + [vp]
    L.lwp_coco_add_rows.argtypes = [vp, C.c_int, C.c_int, vp, vp]
    L.lwp_coco_counts.argtypes = [vp, i64p, vp]
    L.lwp_coco_rows.argtypes = [vp, vp, vp, vp, C.c_int64]
    L.lwp_coco_finish.argtypes = [vp] * 5
    L.lwp_debug_coco_rows.argtypes = [vp, C.c_int] + [vp] * 5
    L.lwp_jpeg_info.argtypes = [vp, C.c_size_t, C.POINTER(JpegHeader)]
    L.lwp_debug_jpeg_blocks.argtypes = [vp, C.c_size_t, vp, C.c_size_t, vp]
    L.lwp_jpeg_decode_batch.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(vp)]
    L.lwp_time_jpeg_decode_batch.argtypes = L.lwp_jpeg_decode_batch.argtypes + [C.c_int, fp]
    L.lwp_set_jpeg_entropy.argtypes = [vp, C.c_int, C.c_int]
    L.lwp_debug_jpeg_entropy_batch.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t), C.c_int, C.POINTER(vp), C.POINTER(vp), ip]
    L.lwp_debug_jpeg_scan.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t), vp, C.c_size_t, C.POINTER(C.c_size_t), vp, vp, ip]
    L.lwp_time_jpeg_entropy_batch.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t), C.c_int, C.c_int, fp, ip]
    jpeg_frames = [vp, C.c_int, C.POINTER(vp), C.c_int, ip, ip]          # handle, N, frames, mem, heights, widths
    L.lwp_jpeg_encode_bound.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_size_t)]
    L.lwp_jpeg_encode_batch.argtypes = jpeg_frames + [C.c_int] * 3 + [C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.lwp_debug_jpeg_encode_blocks.argtypes = jpeg_frames + [C.c_int] * 2 + [C.POINTER(vp), vp]
    L.lwp_debug_jpeg_encode_scan.argtypes = [vp, C.c_int, C.POINTER(vp), ip, ip, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t),
                                             C.POINTER(C.c_size_t)]
    L.lwp_debug_jpeg_encode_header.argtypes = [C.c_int] * 5 + [vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.lwp_time_jpeg_encode_batch.argtypes = jpeg_frames + [C.c_int] * 4 + [fp]
    L.lwp_set_backward_precision.argtypes = [vp, C.c_int, C.c_double]
    L.lwp_get_backward_precision.argtypes = [vp, ip, dp]
    L.lwp_stage_losses_log.argtypes = L.lwp_stage_losses.argtypes[:-1] + [C.c_double]
    L.lwp_loss_log_read.argtypes = [vp, dp, i64p, C.c_int]
    for name in EXPORTS:
        if name not in ("lwp_last_error",):
            getattr(L, name).restype = C.c_int
    _lib = L
    return L


def check(rc, handle=None):
    if rc == LWP_OK:
        return
    msg = lib().lwp_last_error(handle)
    msg = msg.decode("utf-8", "replace") if msg else "error %d" % rc
    if rc == LWP_ERR_ARG:
        raise ValueError(msg)
    if rc == LWP_ERR_UNBOUND:
        raise UnboundLocalError(msg)
    if rc == LWP_ERR_CAPACITY:
        raise CapacityError(msg)
    raise RuntimeError("lwpose (%d): %s" % (rc, msg))


def param_spec(nref=1, num_channels=128, num_heatmaps=19, num_pafs=38):
    """[(key, shape tuple, role)] from the library's own table (no GPU needed)."""
    L = lib()
    n = L.lwp_param_count(nref, num_channels, num_heatmaps, num_pafs)
    if n < 0:
        raise ValueError("bad network shape")
    out = []
    name = C.create_string_buffer(256)
    shape = (C.c_int64 * 4)()
    nd, role = C.c_int(), C.c_int()
    for i in range(n):
        check(L.lwp_param_spec(nref, num_channels, num_heatmaps, num_pafs, i, name, 256, shape, C.byref(nd), C.byref(role)))
        out.append((name.value.decode(), tuple(shape[d] for d in range(nd.value)), role.value))
    return out


def stage_grad_spec(nref=1, num_channels=128, num_heatmaps=19, num_pafs=38):
    """([(key, shape tuple, float offset)], total floats) of lwp_stage_backward's gradient array (no GPU needed)."""
    L = lib()
    total = C.c_int64()
    n = L.lwp_stage_grad_count(nref, num_channels, num_heatmaps, num_pafs, C.byref(total))
    if n < 0:
        raise ValueError("bad network shape")
    out = []
    name = C.create_string_buffer(256)
    shape = (C.c_int64 * 4)()
    nd, off = C.c_int(), C.c_int64()
    for i in range(n):
        check(L.lwp_stage_grad_spec(nref, num_channels, num_heatmaps, num_pafs, i, name, 256, shape, C.byref(nd), C.byref(off)))
        out.append((name.value.decode(), tuple(shape[d] for d in range(nd.value)), off.value))
    return out, total.value


def stage_adam_groups(nref=1, num_channels=128, num_heatmaps=19, num_pafs=38):
    """[(key, learning-rate multiplier, weight decay on)] of every gradient-spec entry under train.py:41-55 (no GPU needed)."""
    L = lib()
    spec, _ = stage_grad_spec(nref, num_channels, num_heatmaps, num_pafs)
    mult, wd = C.c_int(), C.c_int()
    out = []
    for i, (key, _, _) in enumerate(spec):
        check(L.lwp_stage_adam_group(nref, num_channels, num_heatmaps, num_pafs, i, C.byref(mult), C.byref(wd)))
        out.append((key, mult.value, bool(wd.value)))
    return out


def train_scope_name(scope):
    """"stages" / "cpm" / "all" of a scope given as ``train_scope`` takes it."""
    sc = train_scope(scope)
    return [k for k, v in TRAIN_SCOPES.items() if v == sc][0]


def train_scope(scope):
    """LWP_TRAIN_* of a scope.  A scope is given by name ("stages" | "cpm" | "all").  The first two may still be given by their
    numbers (TRAIN_STAGES, TRAIN_CPM), as callers written before the scopes had names do; a scope added since has a name only:
    a bare integer that was an error stays one (ValueError), whatever the C enumeration grows to."""
    if scope in TRAIN_SCOPES:
        return TRAIN_SCOPES[scope]
    if scope in (TRAIN_STAGES, TRAIN_CPM):
        return int(scope)
    raise ValueError("train scope must be 'stages', 'cpm' or 'all', got %r" % (scope,))


def _grad_spec_of(sc, nref, num_channels, num_heatmaps, num_pafs):
    L = lib()
    total = C.c_int64()
    n = L.lwp_train_grad_count(sc, nref, num_channels, num_heatmaps, num_pafs, C.byref(total))
    if n < 0:
        raise ValueError("bad network shape")
    out = []
    name = C.create_string_buffer(256)
    shape = (C.c_int64 * 4)()
    nd, off = C.c_int(), C.c_int64()
    for i in range(n):
        check(L.lwp_train_grad_spec(sc, nref, num_channels, num_heatmaps, num_pafs, i, name, 256, shape, C.byref(nd), C.byref(off)))
        out.append((name.value.decode(), tuple(shape[d] for d in range(nd.value)), off.value))
    return out, total.value


def train_grad_spec(scope, nref=1, num_channels=128, num_heatmaps=19, num_pafs=38):
    """``stage_grad_spec`` for a train scope (``train_scope``): in scope "cpm" the ten cpm.* parameters come first, in scope
    "all" the 69 model.* parameters in front of those."""
    return _grad_spec_of(train_scope(scope), nref, num_channels, num_heatmaps, num_pafs)


def train_adam_groups(scope, nref=1, num_channels=128, num_heatmaps=19, num_pafs=38):
    """``stage_adam_groups`` for a train scope: the cpm's conv weights x1 with decay, biases x2 and depthwise weights x1 without;
    the backbone's stem and pointwise weights x1 with decay, depthwise and BatchNorm weights x1 and BatchNorm biases x2 without."""
    L = lib()
    sc = train_scope(scope)
    spec, _ = _grad_spec_of(sc, nref, num_channels, num_heatmaps, num_pafs)
    mult, wd = C.c_int(), C.c_int()
    out = []
    for i, (key, _, _) in enumerate(spec):
        check(L.lwp_train_adam_group(sc, nref, num_channels, num_heatmaps, num_pafs, i, C.byref(mult), C.byref(wd)))
        out.append((key, mult.value, bool(wd.value)))
    return out


class Handle(object):
    """Owns one lwp_handle (one device, one stream)."""

    def __init__(self, device_id=0, nref=1, num_channels=128, num_heatmaps=19, num_pafs=38, dtype=F32):
        self._h = C.c_void_p()
        self.nref, self.num_channels, self.num_heatmaps, self.num_pafs = nref, num_channels, num_heatmaps, num_pafs
        self.device_id = device_id
        check(lib().lwp_create(device_id, nref, num_channels, num_heatmaps, num_pafs, dtype, C.byref(self._h)))

    @property
    def ptr(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().lwp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
