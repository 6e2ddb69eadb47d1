"""ctypes binding of libnndepth_amd.so (the C-ABI declared in include/nndepth_amd.h).

There is no fallback: if the HIP library is missing the import fails loudly, and every op
refuses non-CUDA (non-HIP) tensors.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NND_LIB") or os.path.join(_HERE, "libnndepth_amd.so")


class NndError(RuntimeError):
    pass


NND_FLAG_CALIBRATE = 1
NND_FLAG_LAST_UPSAMPLE_ONLY = 2  # the refine entry points: only the last iteration's upsampled map


class _SizedDesc(C.Structure):
    """Descriptors start with struct_size = sizeof(the struct) (include/nndepth_amd.h): filled in here, so the
    constructors keep taking the payload fields only."""

    def __init__(self, *args, **kwargs):
        super().__init__(C.sizeof(type(self)), *args, **kwargs)


class UpdateBlockDesc(_SizedDesc):
    _fields_ = [("struct_size", C.c_int32), ("hidden_dim", C.c_int32), ("context_dim", C.c_int32), ("cor_planes", C.c_int32),
                ("flow_channels", C.c_int32), ("mask_channels", C.c_int32), ("gru_kind", C.c_int32),
                ("arithmetic", C.c_int32), ("split_layers", C.c_int32), ("flags", C.c_int32)]


class ConvDesc(C.Structure):
    _fields_ = [("Cout", C.c_int32), ("Cin", C.c_int32), ("KH", C.c_int32), ("KW", C.c_int32), ("stride", C.c_int32)]


class Conv3dDesc(_SizedDesc):
    _fields_ = [("struct_size", C.c_int32), ("Cout", C.c_int32), ("Cin0", C.c_int32), ("Cin1", C.c_int32), ("stride", C.c_int32),
                ("arithmetic", C.c_int32), ("flags", C.c_int32)]


class EncoderDesc(_SizedDesc):
    _fields_ = [("struct_size", C.c_int32), ("output_dim", C.c_int32), ("norm", C.c_int32), ("cnet_dim", C.c_int32),
                ("arithmetic", C.c_int32), ("flags", C.c_int32)]


class RepViTDesc(_SizedDesc):
    _fields_ = [("struct_size", C.c_int32), ("stem_strides", C.c_int32 * 3), ("patch_size", C.c_int32),
                ("down_strides", C.c_int32 * 4), ("channels", C.c_int32 * 4), ("num_blocks", C.c_int32 * 4), ("mixer", C.c_int32 * 4),
                ("ffn_hidden", C.c_int32 * 4), ("cnet_dim", C.c_int32), ("fusion_dim", C.c_int32 * 2), ("flags", C.c_int32)]


class MobileNetV3Desc(_SizedDesc):
    _fields_ = [("struct_size", C.c_int32), ("fnet_dim", C.c_int32), ("cnet_dim", C.c_int32), ("flags", C.c_int32)]


NND_MIDAS_KEEP_PRE = 1


class MidasDesc(_SizedDesc):
    _fields_ = [("struct_size", C.c_int32), ("feature_channels", C.c_int32), ("flags", C.c_int32)]


NND_STEREO_EVAL_MAX_OUTPUTS = 64
NND_STEREO_EVAL_MAX_THRESHOLDS = 8


class StereoEvalOutput(C.Structure):
    _fields_ = [("data", C.c_void_p), ("C", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("reserved", C.c_int32),
                ("stride_b", C.c_int64), ("stride_c", C.c_int64), ("stride_row", C.c_int64)]


class StereoEvalDesc(_SizedDesc):
    _fields_ = [("struct_size", C.c_int32), ("flags", C.c_int32), ("gt", C.c_void_p), ("B", C.c_int32), ("Cg", C.c_int32),
                ("H", C.c_int32), ("W", C.c_int32), ("mask", C.c_void_p), ("mask_h", C.c_int32), ("mask_w", C.c_int32),
                ("gamma", C.c_double), ("max_flow", C.c_float), ("n_above", C.c_int32),
                ("above", C.c_float * NND_STEREO_EVAL_MAX_THRESHOLDS), ("n_below", C.c_int32),
                ("below", C.c_float * NND_STEREO_EVAL_MAX_THRESHOLDS), ("num_outputs", C.c_int32),
                ("outputs", StereoEvalOutput * NND_STEREO_EVAL_MAX_OUTPUTS)]


# name -> (restype, argtypes); mirrors include/nndepth_amd.h one to one
_P = C.c_void_p
_I = C.c_int
SIGNATURES = {
    "nnd_version": (_I, []),
    "nnd_last_error": (C.c_char_p, []),
    "nnd_device_count": (_I, []),
    "nnd_corr1d_pyramid_layout": (_I, [_I, _I, _I, _I, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "nnd_corr1d_build": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "nnd_corr1d_lookup": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "nnd_group_corr_build": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "nnd_group_corr_build_scaled": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, C.c_float, _P]),
    "nnd_group_corr1d_lookup": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "nnd_pyramid_from_level0": (_I, [_P, _I, _I, _I, _I, _P]),
    "nnd_igev_lookup": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "nnd_softargmin_disparity": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "nnd_igev_init_disparity": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "nnd_igev_init_disparity_dev": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "nnd_igev_init_disparity_supported": (_I, [_I, _I]),
    "nnd_igev_init_disparity_chunk": (_I, []),
    "nnd_igev_init_disparity_kernel": (C.c_char_p, [_I, _I, _I, _I, _I]),
    "nnd_convex_upsample": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "nnd_bilinear_sample": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "nnd_agcl_corr_iter": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "nnd_agcl_corr_offset": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "nnd_agcl_corr_offset_nhwc": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "nnd_nchw_to_nhwc": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "nnd_update_block_num_tensors": (_I, [C.POINTER(UpdateBlockDesc)]),
    "nnd_update_block_packed_floats": (C.c_int64, [C.POINTER(UpdateBlockDesc)]),
    "nnd_update_block_pack": (_I, [C.POINTER(UpdateBlockDesc), C.POINTER(_P), _P]),
    "nnd_update_block_workspace_floats": (C.c_int64, [C.POINTER(UpdateBlockDesc), _I, _I, _I]),
    "nnd_update_block_forward": (_I, [C.POINTER(UpdateBlockDesc), _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "nnd_update_block_layer_forward": (_I, [C.POINTER(UpdateBlockDesc), _P, _I, _P, _P, _P, _I, _I, _I, _P]),
    "nnd_update_block_calibration_finish": (_I, [C.POINTER(UpdateBlockDesc), _P, _P, _P]),
    "nnd_update_block_scale_slots": (_I, [C.POINTER(UpdateBlockDesc), C.POINTER(C.c_int64), _I]),
    "nnd_conv2d_calibrate_ex": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "nnd_conv2d_scale_slots_ex": (_I, [_I, _I, _I, _I, _I, C.POINTER(C.c_int64), _I]),
    "nnd_encoder_scale_slots": (_I, [C.POINTER(EncoderDesc), C.POINTER(C.c_int64), _I]),
    "nnd_encoder_scale_name": (C.c_char_p, [C.POINTER(EncoderDesc), _I]),
    "nnd_conv3d_scale_slots": (_I, [C.POINTER(Conv3dDesc), C.POINTER(C.c_int64), _I]),
    "nnd_conv3d_scale_name": (C.c_char_p, [_I]),
    "nnd_scales_read": (_I, [_P, C.POINTER(C.c_int64), _I, _P, _P, _I, _P]),
    "nnd_scales_write": (_I, [_P, C.POINTER(C.c_int64), _I, _P, _I, _P]),
    "nnd_nonfinite_flag": (_I, [_P, C.c_int64, _P, _P]),
    "nnd_encoder_forward2": (_I, [C.POINTER(EncoderDesc), _P, _P, _P, _I, _P, _P, _I, _P, _I, _I, _I, _P]),
    "nnd_pos_enc_sine_add": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "nnd_encoder_calibration_finish": (_I, [C.POINTER(EncoderDesc), _P, _P, _P]),
    "nnd_conv3d_calibration_finish": (_I, [C.POINTER(Conv3dDesc), _P, _P, _P]),
    "nnd_conv2d_packed_floats": (C.c_int64, [_I, _I, _I, _I]),
    "nnd_conv2d_pack": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "nnd_conv2d_forward": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "nnd_conv2d_packed_floats_ex": (C.c_int64, [_I, _I, _I, _I, _I]),
    "nnd_conv2d_pack_ex": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "nnd_conv2d_forward_ex": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "nnd_conv2d_offset_forward": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, C.c_float, _P]),
    "nnd_split_tanh_relu": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "nnd_avg_pool_2x_4x": (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "nnd_resize_bilinear_ac": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, C.c_float, _P]),
    "nnd_resize_nearest_scaled": (_I, [_P, _P, _I, _I, _I, _I, _I, C.c_float, _P]),
    "nnd_mask_upsample_forward": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "nnd_raft_stereo_refine": (_I, [C.POINTER(UpdateBlockDesc), _P, _P, _I, _I, _P, _P, _P, _P, C.c_int64, _P, _P, _P,
                                    _I, _I, _I, _I, _I, _P]),
    "nnd_raft_stereo_group_refine": (_I, [C.POINTER(UpdateBlockDesc), _P, _P, _I, _I, _I, _P, _P, _P, _P, C.c_int64, _P, _P, _P,
                                          _I, _I, _I, _I, _I, _P]),
    "nnd_igev_interleaved_floats": (C.c_int64, [_I, _I, _I, _I, _I]),
    "nnd_igev_interleave_pyramids": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "nnd_igev_interleave_level0_supported": (_I, [_I, _I, _I]),
    "nnd_igev_refine_reads_interleaved": (_I, [_I, _I, _I]),
    "nnd_igev_interleave_level0": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "nnd_igev_stereo_refine": (_I, [C.POINTER(UpdateBlockDesc), _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, C.c_int64, _P, _P, _P,
                                    _I, _I, _I, _I, _I, _P]),
    "nnd_cre_stereo_refine": (_I, [C.POINTER(UpdateBlockDesc), _P, _P, _P, _I, _P, _P, C.c_int64, _P, _P, _P, _P, C.c_int64, _P, _P, _P,
                                   _I, _I, _I, _I, _I, _P]),
    "nnd_conv_packed_floats": (C.c_int64, [C.POINTER(ConvDesc)]),
    "nnd_conv_pack": (_I, [C.POINTER(ConvDesc), _P, _P, _P, _P, _P, _P, C.c_float, _P]),
    "nnd_conv_forward": (_I, [C.POINTER(ConvDesc), _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "nnd_conv_packed_floats_ex": (C.c_int64, [C.POINTER(ConvDesc), _I]),
    "nnd_conv_pack_ex": (_I, [C.POINTER(ConvDesc), _I, _P, _P, _P, _P, _P, _P, C.c_float, _P]),
    "nnd_conv_workspace_floats_ex": (C.c_int64, [C.POINTER(ConvDesc), _I, _I, _I]),
    "nnd_conv_forward_ex": (_I, [C.POINTER(ConvDesc), _I, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "nnd_encoder_num_tensors": (_I, [C.POINTER(EncoderDesc)]),
    "nnd_encoder_packed_floats": (C.c_int64, [C.POINTER(EncoderDesc)]),
    "nnd_encoder_workspace_floats": (C.c_int64, [C.POINTER(EncoderDesc), _I, _I, _I]),
    "nnd_encoder_pack": (_I, [C.POINTER(EncoderDesc), C.POINTER(_P), C.c_float, _P]),
    "nnd_encoder_forward": (_I, [C.POINTER(EncoderDesc), _P, _P, _P, _P, _I, _P, _I, _I, _I, _P]),
    "nnd_repvit_num_tensors": (_I, [C.POINTER(RepViTDesc)]),
    "nnd_repvit_packed_floats": (C.c_int64, [C.POINTER(RepViTDesc)]),
    "nnd_repvit_workspace_floats": (C.c_int64, [C.POINTER(RepViTDesc), _I, _I, _I]),
    "nnd_repvit_pack": (_I, [C.POINTER(RepViTDesc), C.POINTER(_P), _P]),
    "nnd_repvit_forward": (_I, [C.POINTER(RepViTDesc), _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "nnd_repvit_depthwise": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "nnd_repvit_stem": (_I, [_P, _P, _I, _P, _P, _P, _I, _I, _I, _I, _P]),
    "nnd_repvit_pointwise_packed_floats": (C.c_int64, [_I, _I, _I]),
    "nnd_repvit_pointwise_pack": (_I, [_I, _I, _I, _P, _P, _P, _P]),
    "nnd_repvit_pointwise": (_I, [_I, _I, _I, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "nnd_repvit_linear_attention": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "nnd_repvit_upsample_add_relu": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "nnd_mbv3_num_tensors": (_I, [C.POINTER(MobileNetV3Desc)]),
    "nnd_mbv3_packed_floats": (C.c_int64, [C.POINTER(MobileNetV3Desc)]),
    "nnd_mbv3_workspace_floats": (C.c_int64, [C.POINTER(MobileNetV3Desc), _I, _I, _I]),
    "nnd_mbv3_pack": (_I, [C.POINTER(MobileNetV3Desc), C.POINTER(_P), _P]),
    "nnd_mbv3_forward": (_I, [C.POINTER(MobileNetV3Desc), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "nnd_mbv3_depthwise": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "nnd_mbv3_se_partials": (C.c_int64, [_I, _I, _I, _I]),
    "nnd_mbv3_se": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "nnd_mbv3_stem": (_I, [_P, _P, _I, _P, _P, _P, _I, _I, _I, _P]),
    "nnd_mbv3_proj": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "nnd_mbv3_pointwise_packed_floats": (C.c_int64, [_I, _I, _I]),
    "nnd_mbv3_pointwise_pack": (_I, [_I, _I, _I, _P, _P, _P]),
    "nnd_mbv3_pointwise": (_I, [_I, _I, _I, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "nnd_midas_num_tensors": (_I, [C.POINTER(MidasDesc)]),
    "nnd_midas_packed_floats": (C.c_int64, [C.POINTER(MidasDesc)]),
    "nnd_midas_workspace_floats": (C.c_int64, [C.POINTER(MidasDesc), _I, _I, _I]),
    "nnd_midas_workspace_offset": (C.c_int64, [C.POINTER(MidasDesc), _I, _I, _I, _I]),
    "nnd_midas_pack": (_I, [C.POINTER(MidasDesc), C.POINTER(_P), _P]),
    "nnd_midas_forward": (_I, [C.POINTER(MidasDesc), _P, _P, _P, _P, _I, _I, _I, _P]),
    "nnd_midas_up2x_pw_packed_floats": (C.c_int64, [_I, _I]),
    "nnd_midas_up2x_pw_pack": (_I, [_I, _I, _P, _P, _P]),
    "nnd_midas_up2x_pw": (_I, [_I, _I, _P, _P, _P, _I, _I, _I, _P]),
    "nnd_midas_head_packed_floats": (C.c_int64, [_I]),
    "nnd_midas_head_pack": (_I, [_I, _P, _P, _P, _P, _P]),
    "nnd_midas_head": (_I, [_I, _P, _P, _P, _P, _I, _I, _I, _P]),
    "nnd_midas_conv_add": (_I, [_I, _I, _I, _P, _P, _P, _P, _I, _I, _I, _P]),
    "nnd_resize_normalize": (_I, [_P, _I, _P, _I, _I, _I, _I, _I, _I, C.c_float, C.c_float, _P]),
    "nnd_replicate_pad": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "nnd_depth_eval_workspace_bytes": (C.c_int64, [_I]),
    "nnd_depth_eval": (_I, [_P, _P, _P, _I, _I, _I, C.c_float, _P, C.c_int64, _P, _P]),
    "nnd_depth_eval_accumulate": (_I, [_P, _P, _P, _P]),
    "nnd_midas_loss_workspace_bytes": (C.c_int64, [_I, _I, _I]),
    "nnd_midas_loss": (_I, [_P, _P, _P, _I, _I, _I, C.c_int64, C.c_int64, C.c_double, C.c_double, _P, C.c_int64, _P, _P]),
    "nnd_midas_loss_accumulate": (_I, [_P, _P, _P, _P]),
    "nnd_stereo_eval_workspace_bytes": (C.c_int64, [_I]),
    "nnd_stereo_eval": (_I, [C.POINTER(StereoEvalDesc), _P, C.c_int64, _P, _P]),
    "nnd_stereo_eval_accumulate": (_I, [_P, _I, _P, _P]),
    "nnd_min_pool_nearest": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "nnd_view_range_workspace_bytes": (C.c_int64, [_I]),
    "nnd_view_range": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P]),
    "nnd_colorize": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _I, C.c_double, _I, C.c_double, _I, _P, _I, _P, _P]),
    "nnd_pool_abs": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, C.c_float, C.c_float, _P]),
    "nnd_resize_bilinear": (_I, [_P, _I, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, C.c_float, C.c_float, _P]),
    "nnd_depth_inverse": (_I, [_P, _P, C.c_int64, C.c_float, _I, C.c_float, _I, C.c_float, _P]),
    "nnd_disparity_to_depth": (_I, [_P, C.c_int64, _P, _P, _I, C.c_double, _I, C.c_float, _I, C.c_float, _P, _P, _I, _I, _I, _P]),
    "nnd_depth_to_disparity": (_I, [_P, C.c_int64, _P, _I, C.c_double, _I, C.c_double, _P, _I, _I, _I, _P]),
    "nnd_depth_to_points": (_I, [_P, C.c_int64, _P, _P, _I, _P, _I, _I, _I, _P]),
    "nnd_points_compact_workspace_bytes": (C.c_int64, [_I, _I, _I]),
    "nnd_points_compact": (_I, [_P, C.c_int64, _P, _P, _I, _P, _I, _P, _P, _P, _P, C.c_int64, _I, _I, _I, _P]),
    "nnd_lr_consistency": (_I, [_P, C.c_int64, _P, C.c_int64, _I, _I, _I, C.c_float, _P, _P, _I, _I, _I, _P]),
    "nnd_pair_both_views": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "nnd_connected_regions_workspace_bytes": (C.c_int64, [_I, _I, _I]),
    "nnd_connected_regions_tile": (_I, [_I]),
    "nnd_connected_regions": (_I, [_P, C.c_int64, _P, _I, C.c_float, _I, _P, _P, _P, C.c_int64, _I, _I, _I, _P]),
    "nnd_speckle_filter": (_I, [_P, C.c_int64, _P, _I, C.c_float, _I, _I, C.c_float, _P, _P, _P, _P, _P, C.c_int64, _I, _I, _I, _P]),
    "nnd_warp_disparity_limit": (_I, [_I]),
    "nnd_warp_disparity": (_I, [_P, C.c_int64, _P, _I, _I, _I, C.c_float, C.c_float, _P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "nnd_fill_holes_chunk": (_I, []),
    "nnd_fill_holes_workspace_bytes": (C.c_int64, [_I, _I, _I]),
    "nnd_fill_holes": (_I, [_P, C.c_int64, _P, _I, _I, _I, C.c_float, _P, _P, _P, _P, C.c_int64, _I, _I, _I, _P]),
    "nnd_median_filter_limit": (_I, [_I]),
    "nnd_median_filter": (_I, [_P, C.c_int64, _P, _I, _I, _I, _I, C.c_float, _P, _I, C.c_float, _P, _P, _P, _P, _I, _I, _I, _P]),
    "nnd_photometric_limit": (_I, [_I]),
    "nnd_photometric_workspace_bytes": (C.c_int64, [_I, _I, _I]),
    "nnd_synthesize_view": (_I, [_P, _P, C.c_int64, _P, _I, _I, _I, C.c_float, _P, _P, _I, _I, _I, _I, _P]),
    "nnd_photometric_error": (_I, [_P, _P, _P, C.c_int64, _P, _I, _I, _I, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, _P,
                                   _P, _P, _P, _P, _P, C.c_int64, _I, _I, _I, _I, _P]),
    "nnd_loftr_packed_floats": (C.c_int64, [_I, _I]),
    "nnd_loftr_workspace_floats": (C.c_int64, [_I, _I, _I, _I, _I]),
    "nnd_loftr_pack": (_I, [_I, _I, C.POINTER(_P), _P]),
    "nnd_loftr_layer_forward": (_I, [_I, _I, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "nnd_full_attention": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, C.c_int64, C.c_int64, C.c_int64, _P]),
    "nnd_loftr_full_workspace_floats": (C.c_int64, [_I, _I, _I, _I, _I]),
    "nnd_loftr_full_layer_forward": (_I, [_I, _I, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "nnd_conv3d_packed_floats": (C.c_int64, [C.POINTER(Conv3dDesc)]),
    "nnd_conv3d_pack": (_I, [C.POINTER(Conv3dDesc), _P, _P, _P, _P, _P, _P, C.c_float, _P]),
    "nnd_conv3d_forward": (_I, [C.POINTER(Conv3dDesc), _P, _P, _P, _P, _I, _I, _I, _I, C.c_float, _P]),
    "nnd_volume_to_depth_major": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "nnd_depth_major_to_volume": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "nnd_volume_rows_to_depth_major": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "nnd_depth_major_to_volume_rows": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "nnd_volume_upsample2x": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "nnd_volume_gate": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "nnd_profile_conv": (_I, [C.POINTER(UpdateBlockDesc), _P, _P, _I, _I, _I, _I, _I, _P, C.POINTER(C.c_float),
                              C.POINTER(C.c_double)]),
    "nnd_profile_loop_conv": (_I, [C.POINTER(UpdateBlockDesc), _P, _P, _I, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P,
                                   C.POINTER(C.c_float)]),
    "nnd_profile_loop_event_pair": (_I, [C.POINTER(UpdateBlockDesc), _P, _P, _I, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P,
                                         C.POINTER(C.c_float)]),
    "nnd_profile_mfma_peak": (_I, [_I, _I, _P, _P, C.POINTER(C.c_float)]),
    "nnd_profile_mfma16_peak": (_I, [_I, _I, C.c_float, _P, _P, _P, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "nnd_reload_switches": (_I, []),
    "nnd_num_convs": (_I, [C.POINTER(UpdateBlockDesc)]),
    "nnd_conv_name": (C.c_char_p, [C.POINTER(UpdateBlockDesc), _I]),
}


def _load():
    if not os.path.exists(LIB_PATH):
        raise NndError(
            f"{LIB_PATH} not found: build it with `make -C nndepth_amd/csrc` (or __graft_entry__.build()). "
            "nndepth_amd has no CPU / PyTorch fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib.nnd_last_error().decode("utf-8", "replace")
        raise NndError(f"{what or 'nndepth_amd'} failed (status {rc}): {msg}")
