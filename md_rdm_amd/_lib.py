"""ctypes binding of librdm_hip.so (the C ABI in include/rdm_hip.h).

The product path has NO fallback: if the library is missing or a call fails, this raises.
PyTorch only provides device memory (``tensor.data_ptr()``) and the current HIP stream.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librdm_hip.so")
BENCH_LIB_PATH = os.path.join(_HERE, "librdm_bench.so")

c_f32p = C.c_void_p  # all device pointers travel as void*
i32, i64, f32, f64, vp, sz = C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_void_p, C.c_size_t


class ConvDesc(C.Structure):
    """rdm_conv_desc"""
    _fields_ = [(n, i32) for n in ("batch", "in_h", "in_w", "in_c", "in_ld", "out_c", "out_ld", "kh", "kw", "stride_h", "stride_w", "pad_h", "pad_w")]


# The one registry of the C ABI: every public header under include/, and for each function it declares, name: (restype, [argtypes]).
# lib() / bench_lib() bind from it, build.py takes its header dependencies from it, tests/test_abi_cpu.py checks it against the headers.
HEADERS = {
    "rdm_hip.h": {
        # name: (restype, [argtypes])
        "rdm_last_error_string": (C.c_char_p, []),
        "rdm_version": (C.c_int, []),
        "rdm_profile_enable": (None, [i32]),
        "rdm_launch_count": (i64, []),
        "rdm_census_enable": (None, [i32]),
        "rdm_census_reset": (None, []),
        "rdm_census_count": (i32, []),
        "rdm_census_entry": (C.c_int, [i32, C.POINTER(C.c_char_p), C.POINTER(i64)]),
        "rdm_profile_read": (C.c_int, [C.POINTER(f64), C.POINTER(f64), C.POINTER(f64), C.POINTER(i32)]),
        "rdm_profile_kind": (C.c_int, [i32, C.POINTER(C.c_char_p), C.POINTER(f64), C.POINTER(f64), C.POINTER(i32)]),
        "rdm_profile_kind_bytes": (f64, [i32]),
        "rdm_nyu_preprocess_workspace_bytes": (sz, [i32, i32, i32, i32, i32, i32]),
        "rdm_nyu_preprocess": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, sz, vp]),
        "rdm_conv2d_fwd": (C.c_int, [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "rdm_conv2d_dgrad": (C.c_int, [C.POINTER(ConvDesc), vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp]),
        "rdm_conv2d_wgrad": (C.c_int, [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp]),
        "rdm_conv2d_fwd_ex": (C.c_int, [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, vp, vp, i32, vp]),
        "rdm_conv2d_fwd_bnsums": (C.c_int, [C.POINTER(ConvDesc), vp, vp, vp, vp, f64, vp, vp, vp, vp, vp, i32, vp]),
        "rdm_conv3x3_fwd_bnsums_acc": (C.c_int, [C.POINTER(ConvDesc), vp, vp, vp, vp, f64, vp, vp, vp, vp, vp, vp, i32, vp]),
        "rdm_conv2d_dgrad_ex": (C.c_int, [C.POINTER(ConvDesc), vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, i32, vp]),
        "rdm_conv2d_wgrad_ex": (C.c_int, [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, i32, vp]),
        "rdm_conv2d_wgrad_x3": (C.c_int, [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, i32, i32, vp]),
        "rdm_conv1x1_fwd_x6_workspace_bytes": (sz, [i32, i32]),
        "rdm_conv1x1_fwd_x6": (C.c_int, [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, vp, vp, sz, i32, vp]),
        "rdm_conv1x1_dgrad_x3_workspace_bytes": (sz, [i32, i32]),
        "rdm_conv1x1_dgrad_x3": (C.c_int, [C.POINTER(ConvDesc), vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, sz, i32, vp]),
        "rdm_conv3x3_dgrad_x3_workspace_bytes": (sz, [i32]),
        "rdm_conv3x3_dgrad_x3": (C.c_int, [C.POINTER(ConvDesc), vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, sz, i32, vp]),
        "rdm_conv3x3_wino_workspace_bytes": (sz, [i32, i32, i32, i32, i32]),
        "rdm_conv3x3_wino_x6_workspace_bytes": (sz, [i32, i32, i32, i32, i32]),
        "rdm_conv3x3_wino_fwd_x6": (C.c_int, [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, vp, vp, sz, i32, vp]),
        "rdm_conv3x3_wino_fwd": (C.c_int, [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, vp, vp, sz, i32, vp]),
        "rdm_conv3x3_wino_wgrad_workspace_bytes": (sz, [i32, i32, i32, i32]),
        "rdm_conv3x3_wino_wgrad": (C.c_int, [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, sz, vp]),
        "rdm_pack_conv_weight": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, vp]),
        "rdm_unpack_conv_weight": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, vp]),
        "rdm_gemm_bf16": (C.c_int, [vp, i32, i32, vp, vp, vp, i32, vp, vp, i32, i32, i32, i32, vp, sz, vp]),
        "rdm_gemm_bf16_act": (C.c_int, [vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, i32, i32, i32, vp, sz, vp]),
        "rdm_conv3x3_bf16_workspace_bytes": (sz, [i32, i32, i32, i32]),
        "rdm_conv3x3_bf16": (C.c_int, [vp, i32, i32, vp, vp, vp, vp, i32, i32, i32, i32, vp, sz, vp]),
        "rdm_conv3x3_act_bf16_weight_bytes": (sz, [i32]),
        "rdm_conv3x3_act_bf16_pack": (C.c_int, [vp, i32, vp, vp]),
        "rdm_conv3x3_act_bf16_workspace_bytes": (sz, [i32, i32, i32, i32]),
        "rdm_conv3x3_act_bf16": (C.c_int, [vp, i32, i32, vp, vp, i32, i32, i32, i32, vp, sz, vp]),
        "rdm_stem_patches_bf16": (C.c_int, [vp, vp, i32, i32, i32, vp]),
        "rdm_maxpool3s2_bf16": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, vp]),
        "rdm_padavgpool2_bf16": (C.c_int, [vp, i32, vp, vp, vp, i32, i32, i32, i32, vp]),
        "rdm_f32_to_bf16_rows": (C.c_int, [vp, i32, vp, i32, i64, i32, i32, vp]),
        "rdm_pack_conv_weight_bf16": (C.c_int, [vp, vp, i32, i32, i32, i32, vp]),
        "rdm_bn_stats": (C.c_int, [vp, i32, i64, i32, vp, vp, vp]),
        "rdm_bn_finalize": (C.c_int, [vp, vp, f64, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp]),
        "rdm_bn_bwd_reduce": (C.c_int, [vp, i32, vp, i32, vp, vp, i64, i32, vp, vp, vp]),
        "rdm_bn_bwd": (C.c_int, [vp, i32, vp, i32, vp, i32, vp, vp, f64, vp, vp, vp, vp, vp, i64, i32, i32, i32, vp]),
        "rdm_bn_bwd_defer": (C.c_int, [vp, i32, vp, i32, vp, vp, f64, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, vp]),
        "rdm_maxpool3s2_fwd": (C.c_int, [vp, vp, i32, vp, i32, i32, i32, i32, vp]),
        "rdm_maxpool3s2_bwd": (C.c_int, [vp, i32, vp, vp, i32, i32, i32, i32, vp]),
        "rdm_padavgpool2_fwd": (C.c_int, [vp, i32, vp, vp, vp, i32, i32, i32, i32, vp]),
        "rdm_padavgpool2_bwd_workspace_bytes": (sz, [i32]),
        "rdm_padavgpool2_bwd": (C.c_int, [vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, i32, i32, i32, i32, i32, vp, sz, vp]),
        "rdm_net_num_tensors": (C.c_int, []),
        "rdm_net_tensor_name": (C.c_char_p, [i32]),
        "rdm_net_tensor_numel": (i64, [i32]),
        "rdm_net_tensor_is_param": (C.c_int, [i32]),
        "rdm_net_create": (C.c_int, [i32, i32, i32, C.POINTER(vp)]),
        "rdm_net_destroy": (None, [vp]),
        "rdm_net_workspace_bytes": (sz, [vp]),
        "rdm_net_set_option": (C.c_int, [vp, i32, i32]),
        "rdm_net_output_hw": (C.c_int, [vp, C.POINTER(i32), C.POINTER(i32)]),
        "rdm_net_forward": (C.c_int, [vp, vp, C.POINTER(vp), vp, sz, vp, i32, vp]),
        "rdm_net_encoder_output": (C.c_int, [vp, vp, sz, vp, vp]),
        "rdm_net_bf16_weight_bytes": (sz, [vp]),
        "rdm_net_bf16_workspace_bytes": (sz, [vp]),
        "rdm_net_bf16_forward_bytes": (f64, [vp]),
        "rdm_net_bf16_prepare": (C.c_int, [vp, C.POINTER(vp), vp, sz, vp]),
        "rdm_net_forward_bf16": (C.c_int, [vp, vp, C.POINTER(vp), vp, sz, vp, sz, vp, vp]),
        "rdm_net_encoder_output_bf16": (C.c_int, [vp, vp, sz, vp, i32, vp]),
        "rdm_rel_num_tensors": (C.c_int, [i32]),
        "rdm_rel_bf16_weight_bytes": (sz, [i32]),
        "rdm_rel_bf16_prepare": (C.c_int, [i32, C.POINTER(vp), vp, sz, vp]),
        "rdm_rel_bf16_workspace_bytes": (sz, [i32, i32]),
        "rdm_rel_forward_bf16": (C.c_int, [i32, vp, i32, i32, vp, vp, sz, vp, vp]),
        "rdm_rel_bf16_input_nchw": (C.c_int, [vp, i32, vp, i32, vp]),
        "rdm_rel_bf16_train_workspace_bytes": (sz, [i32, i32]),
        "rdm_rel_forward_bf16_train": (C.c_int, [i32, vp, i32, vp, i32, C.POINTER(vp), vp, vp, sz, vp, vp]),
        "rdm_colstats_bf16": (C.c_int, [vp, i32, i32, i32, vp, vp, vp]),
        "rdm_bf16_stats_workspace_bytes": (sz, [i32, i32]),
        "rdm_gemm_bf16_stats": (C.c_int, [vp, i32, i32, vp, vp, vp, i32, vp, i32, i32, i32, vp, vp, vp, sz, vp]),
        "rdm_conv3x3_bf16_stats": (C.c_int, [vp, i32, i32, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, sz, vp]),
        "rdm_wsm_conv_bf16": (C.c_int, [vp, i32, i32, i32, vp, vp, i32, vp, i32, i32, i32, i32, i32, i32, vp]),
        "rdm_wsm_deconv_bf16": (C.c_int, [vp, i32, i32, vp, vp, i32, vp, i32, i32, i32, i32, vp]),
        "rdm_wsm_strip_bf16": (C.c_int, [vp, i32, i32, i32, vp, vp, i32, vp, i32, i32, i32, i32, i32, vp]),
        "rdm_wsm_conv1x1_f32": (C.c_int, [vp, i32, i32, vp, vp, vp, i32, i32, i32, vp]),
        "rdm_net_backward": (C.c_int, [vp, vp, C.POINTER(vp), C.POINTER(vp), vp, sz, i32, i32, vp]),
        "rdm_net_segment_range": (C.c_int, [i32, C.POINTER(i32), C.POINTER(i32)]),
        "rdm_net_num_backward_stages": (C.c_int, []),
        "rdm_net_backward_stage_range": (C.c_int, [i32, C.POINTER(i32), C.POINTER(i32)]),
        "rdm_net_backward_stage": (C.c_int, [vp, vp, C.POINTER(vp), C.POINTER(vp), vp, sz, i32, vp]),
        "rdm_net_buffer": (C.c_int, [vp, C.c_char_p, C.POINTER(i64), C.POINTER(i64)]),
        "rdm_net_route": (C.c_int, [vp, i32, i32, i32, C.POINTER(i32)]),
        "rdm_net_forward_flops": (f64, [vp]),
        "rdm_net_backward_flops": (f64, [vp]),
        "rdm_dorn_fwd": (C.c_int, [vp, vp, vp, i32, i32, i32, vp]),
        "rdm_dorn_bwd": (C.c_int, [vp, vp, vp, i32, i32, i32, vp]),
        "rdm_ordinal_loss_fwd": (C.c_int, [vp, vp, vp, i32, i32, i32, vp]),
        "rdm_ordinal_loss_bwd": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, vp]),
        "rdm_depth2label_sid": (C.c_int, [vp, vp, i64, vp]),
        "rdm_depth2label_sid_ex": (C.c_int, [vp, vp, i64, i32, vp]),
        "rdm_resize_bicubic_f64": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, vp]),
        "rdm_gm_normalize_f64": (C.c_int, [vp, vp, vp, i32, i32, f64, vp]),
        "rdm_decompose_f64": (C.c_int, [vp, vp, i32, i32, vp]),
        "rdm_fine_detail_pred_f32": (C.c_int, [vp, vp, vp, i32, i32, vp]),
        "rdm_fine_detail_pred_bwd": (C.c_int, [vp, vp, vp, i32, i32, vp]),
        "rdm_candidates_matvec_f32": (C.c_int, [vp, vp, vp, i32, i32, i64, vp]),
        "rdm_candidates_matvec_bwd": (C.c_int, [vp, vp, vp, i32, i32, i64, vp]),
        "rdm_split_rows_f32": (C.c_int, [vp, i32, vp, vp, vp, i32, i64, i32, vp]),
        "rdm_frame_split_rows_bytes": (sz, [i32, i32, i32]),
        "rdm_frame_split_rows_f32": (C.c_int, [vp, i32, i32, i32, i32, i32, vp, vp]),
        "rdm_layout_nchw_to_nhwc_f32": (C.c_int, [vp, vp, i32, i32, i32, i32, vp]),
        "rdm_layout_nhwc_to_nchw_f32": (C.c_int, [vp, i32, vp, i32, i32, i32, vp]),
        "rdm_recombine_f64": (C.c_int, [vp, vp, i32, i32, i32, i32, vp]),
        "rdm_recombine_bwd": (C.c_int, [vp, vp, i32, i32, i32, i32, vp]),
        "rdm_predict_tail_f32": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
        "rdm_depth_metrics_f64": (C.c_int, [vp, vp, i64, vp, vp]),
        "rdm_eval_target_metrics_f64": (C.c_int, [vp, vp, i32, i32, i32, i32, vp, vp, vp, i32, vp]),
        "rdm_ratio_grid_lloyd_dense": (C.c_int, [vp, vp, i32, i32, vp, vp, vp]),
        "rdm_ratio_grid_lloyd_paged": (C.c_int, [vp, vp, vp, i32, i32, vp, vp, i32, vp]),
        "rdm_als_workspace_bytes": (sz, [i32, i32, i32, i32, i32]),
        "rdm_als_rank1": (C.c_int, [vp, i32, vp, i32, i32, i32, i32, i32, vp, sz, vp]),
        "rdm_als_rank1_paged": (C.c_int, [vp, vp, vp, i32, i32, vp, vp, i32, vp, sz, vp]),
        "rdm_page_split_f32": (C.c_int, [vp, vp, i32, i32, i32, vp]),
        "rdm_page_reconstruct_f32": (C.c_int, [vp, vp, i32, i32, i32, vp]),
        "rdm_adamw_fused": (C.c_int, [vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, i32, f32, vp]),
    },
    # include/rdm_viz.h: depth-map rendering, part of librdm_hip.so, declared in a header of its own
    "rdm_viz.h": {
        "rdm_viz_rows_u8": (C.c_int, [vp, vp, i32, i32, i32, vp, i32, i32, i32, i32, i32, i32, f64, f64, vp, i32, vp]),
    },
    # include/rdm_eval.h: standard-protocol evaluation, part of librdm_hip.so, declared in a header of its own
    "rdm_eval.h": {
        "rdm_eval_standard_workspace_bytes": (sz, [i32, i32, i32]),
        "rdm_eval_standard_f64": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, f64, f64, C.POINTER(i32), vp, vp, vp, sz, vp]),
    },
    # include/rdm_eval_view.h: the same evaluation for a map that covers a rectangle of the depth frame, declared in a header of its own
    "rdm_eval_view.h": {
        "rdm_eval_standard_view_f64": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, f64, f64, C.POINTER(i32), C.POINTER(f64), vp, vp, vp, sz, vp]),
    },
    # include/rdm_optim.h: gradient accumulation, the squared global norm and the clipped AdamW step, part of librdm_hip.so, declared in a header of its own
    "rdm_optim.h": {
        "rdm_grad_accumulate_f32": (C.c_int, [vp, vp, i64, i32, vp]),
        "rdm_grad_sumsq_workspace_bytes": (sz, [i64]),
        "rdm_grad_sumsq_f64": (C.c_int, [vp, i64, vp, vp, sz, vp]),
        "rdm_adamw_fused_clip": (C.c_int, [vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, i32, f32, vp, i32, f32, vp, vp]),
    },
    # include/rdm_ema.h: the AdamW step that also advances a weight average, and the in-place exchange of two buffers, part of librdm_hip.so, declared in a header of its own
    "rdm_ema.h": {
        "rdm_adamw_fused_ema": (C.c_int, [vp, vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, i32, f32, vp, i32, f32, vp, f32, vp]),
        "rdm_ema_swap_f32": (C.c_int, [vp, vp, i64, vp]),
    },
    # include/rdm_depth.h: metric depth frames (SID scale, view-mapped resample, float32 and 16-bit planes), part of librdm_hip.so, declared in a header of its own
    "rdm_depth.h": {
        "rdm_depth_frames": (C.c_int, [vp, vp, i32, vp, C.POINTER(f64), i32, i32, i32, C.POINTER(f64), i32, f64, vp, vp, vp, i32, vp]),
    },
    # include/rdm_cloud.h: point clouds (unprojection, normals, in-order compaction into PLY vertex records), part of librdm_hip.so, declared in a header of its own
    "rdm_cloud.h": {
        "rdm_depth_cloud": (C.c_int, [vp, vp, i32, i32, i32, C.POINTER(f64), f64, f64, i32, i32, vp, i64, vp, i32, vp]),
    },
    # include/rdm_refine.h: guided depth refinement (joint bilateral filter of a depth frame under its colour frame), part of librdm_hip.so, declared in a header of its own
    "rdm_refine.h": {
        "rdm_depth_refine": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, f64, f64, i32, f64, vp, vp, vp]),
    },
    # include/rdm_mesh.h: triangle faces of a depth frame (depth-edge-aware, in-order compaction into index records whose vertices are rdm_depth_cloud's), part of librdm_hip.so, declared in a header of its own
    "rdm_mesh.h": {
        "rdm_depth_mesh_workspace_bytes": (i64, [i32, i32, i32, i32]),
        "rdm_depth_mesh": (C.c_int, [vp, i32, i32, i32, f64, f64, i32, f64, i32, vp, i64, vp, vp, vp, i64, vp]),
    },
    # include/rdm_warp.h: novel views of a depth frame (z-buffered forward warp through a 64-bit atomic minimum, row-wise hole fill), part of librdm_hip.so, declared in a header of its own
    "rdm_warp.h": {
        "rdm_depth_warp_workspace_bytes": (sz, [i32, i32, i32]),
        "rdm_depth_warp": (C.c_int, [vp, vp, i32, i32, i32, C.POINTER(f64), C.POINTER(f64), vp, i32, f64, f64, i32, i32, i32, i32, vp, vp, vp, vp, vp, sz, vp]),
    },
    # include/rdm_anchor.h: anchored metric depth (cell sums of the log residuals against a sparse metric frame, the fitted scale and the smoothed correction field, the corrected frames), part of librdm_hip.so, declared in a header of its own
    "rdm_anchor.h": {
        "rdm_depth_anchor_cells": (C.c_int, [vp, vp, vp, i32, i32, i32, C.POINTER(f64), i32, f64, f64, f64, vp, vp, vp]),
        "rdm_depth_anchor_field": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, f64, f64, vp, vp, vp, vp]),
        "rdm_depth_frames_corrected": (C.c_int, [vp, vp, i32, vp, C.POINTER(f64), i32, i32, i32, C.POINTER(f64), i32, f64, vp, vp, vp, i32, vp, i32, i32, i32, vp]),
    },
    # include/rdm_fuse.h: multi-frame depth fusion (frames with poses integrated into one TSDF volume in one launch, the volume's zero crossings as oriented points in rdm_cloud.h's records), part of librdm_hip.so, declared in a header of its own
    "rdm_fuse.h": {
        "rdm_tsdf_integrate": (C.c_int, [vp, vp, i32, i32, i32, C.POINTER(f64), vp, i32, f64, f64, f64, f64, i32, i32, i32, C.POINTER(f64), vp, vp, vp, vp]),
        "rdm_tsdf_extract_workspace_bytes": (sz, [i32, i32, i32]),
        "rdm_tsdf_extract": (C.c_int, [vp, vp, vp, i32, i32, i32, C.POINTER(f64), f64, i32, vp, i64, vp, vp, sz, vp]),
    },
    # librdm_bench.so (include/rdm_bench.h): measurement kernels of tools/ and bench_ops.py - not part of the product
    "rdm_bench.h": {
        "rdm_microbench_copy": (C.c_int, [vp, vp, i64, vp]),
        "rdm_microbench_mfma_f32": (C.c_int, [vp, i32, i32, vp]),
        "rdm_microbench_mfma_staged_f32": (C.c_int, [vp, i64, i32, i32, i32, i64, vp]),
        "rdm_microbench_gemm_dma_f32": (C.c_int, [vp, i32, vp, i32, vp, i32, i32, i32, i32, i32, vp]),
        "rdm_microbench_xcd_sync": (C.c_int, [vp, vp, i32, i32, i32, vp, vp]),
    },
}
BENCH_HEADER = "rdm_bench.h"                                 # the one header of librdm_bench.so; every other header is librdm_hip.so's

# rdm_net_option (include/rdm_hip.h), for rdm_net_set_option
NET_OPT_PACKED_3X3, NET_OPT_GRADS_PREZEROED, NET_OPT_DIRECT_3X3, NET_OPT_DETERMINISTIC, NET_OPT_JOIN_PER_SEGMENT = 1, 2, 3, 4, 5
NET_OPT_SPLIT_BWD, NET_OPT_SPLIT_FWD, NET_OPT_GEMM_BF16, NET_OPT_DEFER_NORM1, NET_OPT_PREPACK = 6, 7, 8, 9, 10
NET_OPT_SPLIT_ROWS, NET_OPT_WINO_X6, NET_OPT_FUSE_STATS3 = 11, 12, 13
EVAL_ALIGN = {"none": 0, "median": 1, "logmean": 2}          # RDM_EVAL_ALIGN_* (include/rdm_eval.h)
GRAD_ACC_COPY, GRAD_ACC_ADD, CLIP_MAX_SLOTS = 0, 1, 8        # RDM_GRAD_ACC_*, RDM_CLIP_MAX_SLOTS (include/rdm_optim.h)
DEPTH_OUTSIDE = {"zero": 0, "edge": 1}                       # the `outside` argument of rdm_depth_frames
MESH_FACES = {"i32": 0, "ply": 1}                            # RDM_MESH_FACES_* (include/rdm_mesh.h)
ANCHOR_FIT = {"none": 0, "logmean": 1}                       # RDM_ANCHOR_FIT_* (include/rdm_anchor.h); "median" is formed by md_rdm_amd.anchor from rdm_eval_standard_view_f64
ANCHOR_MAX_CELLS, ANCHOR_MAX_RADIUS = 5120, 96               # RDM_ANCHOR_MAX_CELLS, RDM_ANCHOR_MAX_RADIUS

_lib = None
_bench = None


class RdmError(RuntimeError):
    pass


def _debug_variant_removed(v):
    if int(v) != 0:                                 # bench.py still passes RDM_VARIANT through: 0 is the one configuration there is
        raise RdmError(f"rdm_debug_variant({int(v)}): the development A/B switch was removed - the library has one configuration (0)")


def symbols(header):
    """The function names of one header of HEADERS, in table order."""
    return list(HEADERS[header])


def _bind(L, headers):
    for header in headers:
        for name, (res, args) in HEADERS[header].items():
            fn = getattr(L, name)     # AttributeError here = header/library drift: fail loudly
            fn.restype, fn.argtypes = res, args


def lib():
    """The loaded library; raises (never falls back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RdmError(f"{LIB_PATH} not found - run `python -m md_rdm_amd.build` (hipcc --offload-arch=gfx950). "
                           "There is no CPU/PyTorch fallback for the hot path.")
        L = C.CDLL(LIB_PATH)
        _bind(L, [h for h in HEADERS if h != BENCH_HEADER])
        L.rdm_debug_variant = _debug_variant_removed
        _lib = L
    return _lib


def census():
    """{kernel variant name: launches} recorded since the last rdm_census_reset() (rdm_census_enable(1) must be on)."""
    L = lib()
    out = {}
    for i in range(L.rdm_census_count()):
        name, n = C.c_char_p(), i64()
        check(L.rdm_census_entry(i, C.byref(name), C.byref(n)))
        out[name.value.decode()] = n.value
    return out


def bench_lib():
    """librdm_bench.so, for development tools only (the product never loads it)."""
    global _bench
    if _bench is None:
        lib()                                       # the bench library resolves its support symbols from the product library
        if not os.path.exists(BENCH_LIB_PATH):
            raise RdmError(f"{BENCH_LIB_PATH} not found - run `python -m md_rdm_amd.build`")
        B = C.CDLL(BENCH_LIB_PATH)
        _bind(B, [BENCH_HEADER])
        _bench = B
    return _bench


def check(rc):
    if rc != 0:
        raise RdmError(f"librdm_hip error {rc}: {lib().rdm_last_error_string().decode()}")


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL).  Tensors must be contiguous."""
    if t is None:
        return None
    if not t.is_contiguous():
        raise RdmError("non-contiguous tensor passed to the C ABI")
    return C.c_void_p(t.data_ptr())


def device_depth(depth, who):
    """The depth frame every depth-output call takes, (B,h,w) float32 on the device: (detached contiguous tensor, (B, h, w)).  ``who`` names the
    caller in the error."""
    import torch

    if not isinstance(depth, torch.Tensor) or not depth.is_cuda:
        raise RdmError("%s runs on the MI355X only; there is no CPU fallback" % who)
    if depth.dim() != 3 or depth.dtype != torch.float32 or depth.numel() == 0:
        raise RdmError("depth must be (B,h,w) float32, got %s %s" % (depth.dtype, tuple(depth.shape)))
    return depth.detach().contiguous(), tuple(depth.shape)


def device_rgb(rgb, B, h, w):
    """The colour frame of a (B,h,w) depth frame, (B,h,w,3) uint8 on the device, detached and contiguous; None stays None."""
    import torch

    if rgb is None:
        return None
    if not isinstance(rgb, torch.Tensor) or not rgb.is_cuda:
        raise RdmError("rgb must be on the device; there is no CPU fallback")
    if rgb.dtype != torch.uint8 or tuple(rgb.shape) != (B, h, w, 3):
        raise RdmError("rgb must be (%d,%d,%d,3) uint8, got %s %s" % (B, h, w, rgb.dtype, tuple(rgb.shape)))
    return rgb.detach().contiguous()


def stream():
    """The caller's current HIP stream.  Through the raw query where this torch has it: ``torch.cuda.current_stream()`` builds a Stream object and asks the
    runtime for the device count on the way (hipGetDeviceCount, ~20 us per call on this stack; ~100 C-ABI calls per training step; the host is two steps
    ahead of the GPU in steady state, so this only shortens the first step after a synchronisation - tools/host_pace.py)."""
    import torch

    raw, dev = getattr(torch._C, "_cuda_getCurrentRawStream", None), getattr(torch._C, "_cuda_getDevice", None)
    if raw is not None and dev is not None:
        return C.c_void_p(raw(dev()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
