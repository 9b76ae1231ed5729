"""ctypes binding of libcfhip.so (include/cf_hip.h).  No CPU fallback: if the library is missing
or a call fails, this raises - the product path never silently degrades."""
import ctypes as C
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libcfhip.so")

ABI_VERSION = 7      # CF_ABI_VERSION of include/cf_hip.h this binding was written against
CF_MAX_SRC = 4
CF_MAX_GROUPS = 4    # layers per grouped launch (cf_conv3x3_f16x3_grouped, cf_dcn_v2_f16x3_grouped)
ACT_NONE, ACT_RELU, ACT_SIGMOID_CLAMP, ACT_RAW_AND_SIGDEPTH = 0, 1, 2, 3
LAYOUT_NHWC, LAYOUT_NCHW = 0, 1

_f = C.c_void_p  # device pointers travel as integers


class ConvArgs(C.Structure):
    _fields_ = [("src", _f * CF_MAX_SRC), ("src_c", C.c_int32 * CF_MAX_SRC), ("n_src", C.c_int32),
                ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Ho", C.c_int32),
                ("Wo", C.c_int32), ("stride", C.c_int32), ("weight", _f), ("slots", _f),
                ("bias", _f), ("K_pad", C.c_int32), ("N", C.c_int32), ("N_pad", C.c_int32),
                ("residual", _f), ("res_stride", C.c_int32), ("out", _f), ("out2", _f),
                ("out_stride", C.c_int32), ("out_layout", C.c_int32), ("act", C.c_int32),
                ("precise", C.c_int32), ("out_scale", C.c_float), ("in_scale", C.c_float)]


class DcnArgs(C.Structure):
    _fields_ = [("x", _f), ("offmask", _f), ("om_stride", C.c_int32), ("B", C.c_int32),
                ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("weight", _f), ("bias", _f),
                ("N", C.c_int32), ("N_pad", C.c_int32), ("out", _f), ("out_stride", C.c_int32),
                ("act", C.c_int32), ("precise", C.c_int32), ("out_scale", C.c_float),
                ("out_split_bf16", _f), ("split_stride", C.c_int32), ("workspace", _f),
                ("workspace_bytes", C.c_size_t), ("mask_activated", C.c_int32), ("out_mx", _f), ("in_scale", C.c_float),
                ("mx_scale", C.c_float)]


class DcnBwdArgs(C.Structure):
    _fields_ = [("gout", _f), ("weight", _f), ("x", _f), ("offmask", _f), ("B", C.c_int32), ("H", C.c_int32),
                ("W", C.c_int32), ("C", C.c_int32), ("N", C.c_int32), ("gx", _f), ("gom", _f), ("gw", _f), ("gbias", _f),
                ("workspace", _f), ("workspace_bytes", C.c_size_t)]


CF_MAX_HEADS = 12
CF_DEPTH_MAPS_MAX = 8


class HeadTailArgs(C.Structure):
    _fields_ = [("x", _f), ("x_stride", C.c_int32), ("B", C.c_int32), ("H", C.c_int32),
                ("W", C.c_int32), ("n_heads", C.c_int32), ("n_hidden", C.c_int32),
                ("w_hidden", (_f * 2) * CF_MAX_HEADS), ("b_hidden", (_f * 2) * CF_MAX_HEADS),
                ("w_out", _f * CF_MAX_HEADS), ("b_out", _f * CF_MAX_HEADS),
                ("out", _f * CF_MAX_HEADS), ("out2", _f * CF_MAX_HEADS),
                ("c_base", C.c_int32 * CF_MAX_HEADS), ("n_out", C.c_int32 * CF_MAX_HEADS),
                ("act", C.c_int32 * CF_MAX_HEADS)]


class HeadFusedArgs(C.Structure):
    _fields_ = [("tail", HeadTailArgs), ("src", _f * 2), ("src_c", C.c_int32 * 2), ("n_src", C.c_int32),
                ("slots", _f), ("K_pad", C.c_int32), ("w_first", _f * CF_MAX_HEADS),
                ("b_first", _f * CF_MAX_HEADS), ("layout3x3", C.c_int32), ("w_out_perm", _f * CF_MAX_HEADS),
                ("mfma16", C.c_int32), ("mx", C.c_int32), ("first_scale", C.c_float * CF_MAX_HEADS)]


class StemArgs(C.Structure):
    _fields_ = [("x", _f), ("B", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("w_base", _f), ("b_base", _f), ("scale_base", C.c_float),
                ("w_level0", _f), ("b_level0", _f), ("scale_level0", C.c_float),
                ("w_level1", _f), ("b_level1", _f), ("scale_level1", C.c_float),
                ("out", _f), ("out_pool", _f), ("in_scale", C.c_float * 3)]


class StemEarlyArgs(C.Structure):
    _fields_ = [("stem", StemArgs), ("pc", _f), ("pc_h", C.c_int32), ("pc_w", C.c_int32), ("w_base_radar", _f)]


class PackSrc(C.Structure):
    _fields_ = [("channels", C.c_int32), ("stride", C.c_int32), ("c_base", C.c_int32)]


class PackBn(C.Structure):
    _fields_ = [("gamma", _f), ("beta", _f), ("mean", _f), ("var", _f), ("eps", C.c_float)]


class PackConvDesc(C.Structure):
    _fields_ = [("weight", _f), ("bias", _f), ("bn", PackBn),
                ("cout", C.c_int32), ("kh", C.c_int32), ("kw", C.c_int32), ("stride", C.c_int32),
                ("pad", C.c_int32), ("dilation", C.c_int32),
                ("src", C.POINTER(PackSrc)), ("n_src", C.c_int32),
                ("proj_weight", _f), ("proj_bias", _f), ("proj_bn", PackBn), ("proj", PackSrc)]


class PackInfo(C.Structure):
    _fields_ = [("n_pad", C.c_int32), ("k_pad", C.c_int32), ("n_slots", C.c_int32), ("patch", C.c_int32),
                ("out_scale", C.c_float), ("weight_bytes", C.c_size_t)]


class DecodeArgs(C.Structure):
    _fields_ = [("scores", _f), ("inds", _f), ("classes", _f), ("reg", _f), ("wh", _f),
                ("depth", _f), ("rot", _f), ("dim", _f), ("amodal", _f), ("att", _f), ("vel", _f),
                ("B", C.c_int32), ("K", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("out_h", C.c_int32), ("out_w", C.c_int32), ("norm2d", C.c_int32), ("det", _f)]


class SerializeArgs(C.Structure):
    _fields_ = [("post", _f), ("B", C.c_int32), ("K", C.c_int32), ("trans_matrix", _f),
                ("velocity_matrix", _f), ("cs_rot", _f), ("pose_rot", _f), ("rows", _f), ("rotation", _f),
                ("n_samples", C.c_int32), ("sample_ptr", _f), ("sample_frames", _f),
                ("max_per_sample", C.c_int32), ("order", _f), ("counts", _f)]


CF_LOSS_MAX_HEADS = 16
CF_LOSS_STATS = 4 + 4 * CF_LOSS_MAX_HEADS
LOSS_L1, LOSS_L1_UNC, LOSS_BINROT, LOSS_BCE = 0, 1, 2, 3


class LossHead(C.Structure):
    _fields_ = [("kind", C.c_int32), ("channels", C.c_int32), ("map", _f), ("target", _f), ("mask", _f), ("rotbin", _f),
                ("unc", _f), ("weight", C.c_float), ("gmap", _f), ("gunc", _f)]


class LossArgs(C.Structure):
    _fields_ = [("heat", _f), ("heat_gt", _f), ("centers", _f), ("wh", _f), ("mask", _f), ("cls", _f),
                ("B", C.c_int32), ("C", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("M", C.c_int32),
                ("n_heads", C.c_int32), ("out_area", C.c_float), ("heat_weight", C.c_float),
                ("head", LossHead * CF_LOSS_MAX_HEADS), ("losses", _f), ("total", _f), ("layer_mask", _f), ("stats", _f),
                ("workspace", _f), ("workspace_bytes", C.c_size_t), ("grad_out", _f), ("gheat", _f)]


CF_HEAD_TRAIN_MAX_HIDDEN = 2
_HT_LAYERS = CF_HEAD_TRAIN_MAX_HIDDEN + 2


class HeadTrainArgs(C.Structure):
    _fields_ = [("x", _f), ("x2", _f), ("x_stride", C.c_int32), ("c_x", C.c_int32), ("x2_stride", C.c_int32),
                ("c_x2", C.c_int32), ("B", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("n_hidden", C.c_int32),
                ("hidden", C.c_int32), ("n_out", C.c_int32), ("chunk_px", C.c_int32),
                ("weight", _f * _HT_LAYERS), ("bias", _f * _HT_LAYERS), ("y", _f), ("gy", _f),
                ("gw", _f * _HT_LAYERS), ("gb", _f * _HT_LAYERS), ("workspace", _f), ("workspace_bytes", C.c_size_t)]


CF_TARGETS_MAX_OBJS = 128
CF_TARGETS_F = 20
TGT_HAS_AMODAL, TGT_HAS_ATTRIBUTES, TGT_HAS_VELOCITY, TGT_HAS_ALPHA = 1, 2, 4, 8
TGT_HAS_DEPTH, TGT_HAS_DIMENSION, TGT_HAS_LOCATION, TGT_HAS_YAW = 16, 32, 64, 128
TGT_REP3D, TGT_NORM2D, TGT_WRITE_DEPTH, TGT_WRITE_ROT, TGT_FRUSTUM = 1, 2, 4, 8, 16


class TargetsArgs(C.Structure):
    _fields_ = [("ann", _f), ("iann", _f), ("counts", _f), ("trans", _f), ("calib", _f), ("scale", _f), ("pc_dep", _f),
                ("B", C.c_int32), ("M", C.c_int32), ("C", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("flags", C.c_int32), ("max_pc_dist", C.c_float),
                ("heat", _f), ("cls", _f), ("mask", _f), ("trunc_mask", _f), ("wh", _f), ("reg", _f), ("amodal_offset", _f),
                ("dimension", _f), ("depth", _f), ("rotbin", _f), ("rotres", _f), ("att", _f), ("att_mask", _f),
                ("velocity", _f), ("pc_hm", _f), ("t_bboxes", _f), ("t_scores", _f), ("t_centers", _f),
                ("t_heat_centers", _f), ("t_bboxes3d", _f), ("t_rotation", _f), ("t_att", _f), ("t_velocity", _f),
                ("workspace", _f), ("workspace_bytes", C.c_size_t)]


CF_OPTIM_CHUNK = 4096     # elements one workgroup of cf_optim_adamw / cf_optim_sgd owns (cf_optim_chunk_elems() of the library)


class OptimTensor(C.Structure):
    _fields_ = [("param", _f), ("grad", _f), ("state1", _f), ("state2", _f), ("numel", C.c_int64), ("step_base", C.c_int32),
                ("reserved", C.c_int32)]


class OptimChunk(C.Structure):
    _fields_ = [("offset", C.c_int64), ("tensor", C.c_int32), ("reserved", C.c_int32)]


class OptimArgs(C.Structure):
    _fields_ = [("tensors", _f), ("chunks", _f), ("n_tensors", C.c_int32), ("n_chunks", C.c_int32), ("lr", C.c_double),
                ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("wd", C.c_double), ("momentum", C.c_double),
                ("decay", C.c_float), ("step", C.c_int32)]


# every symbol include/cf_hip.h declares: (restype, argtypes)
_i, _d = C.c_int, C.c_double
SYMBOLS = {
    "cf_conv2d_fused": (_i, [C.POINTER(ConvArgs), _f]),
    "cf_conv2d_f16x3": (_i, [C.POINTER(ConvArgs), _f]),
    "cf_conv3x3_f16x3": (_i, [C.POINTER(ConvArgs), _f]),
    "cf_conv3x3_root_f16x3": (_i, [C.POINTER(ConvArgs), C.POINTER(ConvArgs), C.POINTER(C.c_int32), _f]),
    "cf_conv3x3_proj_f16x3": (_i, [C.POINTER(ConvArgs), C.POINTER(C.c_int32), _f]),
    "cf_conv3x3_f16x3_grouped": (_i, [C.POINTER(C.POINTER(ConvArgs)), C.c_int32, _f]),
    "cf_conv3x3_grouped_form": (_i, [C.POINTER(C.POINTER(ConvArgs)), C.c_int32, C.POINTER(C.c_int32)]),
    "cf_conv3x3_tile_form": (_i, [C.c_int32, C.POINTER(C.POINTER(ConvArgs)), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "cf_stem_fused": (_i, [C.POINTER(StemArgs), _f]),
    "cf_stem_fused_early": (_i, [C.POINTER(StemEarlyArgs), _f]),
    "cf_split_bf16": (_i, [_f, _f, C.c_long, _i, _i, _i, _f]),
    "cf_head_fused": (_i, [C.POINTER(HeadFusedArgs), _f]),
    "cf_head_fused_with": (_i, [C.POINTER(HeadFusedArgs), _i, _i, _f]),
    "cf_head_fused_at": (_i, [C.POINTER(HeadFusedArgs), _f, _i, _f]),
    "cf_head_slot_tables": (_i, [_f, _f, _i, _i, _i, _f, _f, _f]),
    "cf_pack_feat_mx": (_i, [_f, _i, _f, C.c_long, _f]),
    "cf_pack_feat_mx_scaled": (_i, [_f, _i, _f, C.c_long, C.c_float, _f]),
    "cf_absmax_f32": (_i, [_f, C.c_long, _i, _i, _f, _f]),
    "cf_dcn_v2_fused": (_i, [C.POINTER(DcnArgs), _f]),
    "cf_dcn_v2_f16x3": (_i, [C.POINTER(DcnArgs), _f]),
    "cf_dcn_v2_workspace_bytes": (C.c_size_t, [_i, _i, _i, _i, _i]),
    "cf_dcn_v2_f16x3_grouped": (_i, [C.POINTER(C.POINTER(DcnArgs)), C.c_int32, _f]),
    "cf_dcn_v2_f16x3_form": (_i, [C.POINTER(C.POINTER(DcnArgs)), C.c_int32, C.POINTER(C.c_int32)]),
    "cf_gemm_tile_form": (_i, [C.c_long, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "cf_dcn_v2_bwd_data": (_i, [C.POINTER(DcnBwdArgs), _f]),
    "cf_dcn_v2_bwd_weight": (_i, [C.POINTER(DcnBwdArgs), _f]),
    "cf_dcn_v2_bwd_workspace_bytes": (C.c_size_t, [_i, _i, _i, _i, _i]),
    "cf_loss_forward": (_i, [C.POINTER(LossArgs), _f]),
    "cf_loss_backward": (_i, [C.POINTER(LossArgs), _f]),
    "cf_loss_workspace_bytes": (C.c_size_t, [_i, _i, _i, _i]),
    "cf_targets_build": (_i, [C.POINTER(TargetsArgs), _f]),
    "cf_targets_workspace_bytes": (C.c_size_t, [_i, _i]),
    "cf_optim_plan": (_i, [C.POINTER(OptimTensor), _i, C.POINTER(OptimChunk), C.c_int64, C.POINTER(C.c_int64)]),
    "cf_optim_adamw": (_i, [C.POINTER(OptimArgs), _f]),
    "cf_optim_sgd": (_i, [C.POINTER(OptimArgs), _f]),
    "cf_optim_chunk_elems": (_i, []),
    "cf_head_train_forward": (_i, [C.POINTER(HeadTrainArgs), _f]),
    "cf_head_backward": (_i, [C.POINTER(HeadTrainArgs), _f]),
    "cf_head_train_workspace_bytes": (C.c_size_t, [_i, _i, _i, _i, _i, _i]),
    "cf_head_bwd_workspace_bytes": (C.c_size_t, [_i, _i, _i, _i, _i, _i]),
    "cf_head_bwd_chunk_px": (_i, [_i, _i, _i, _i]),
    "cf_head_backward_dx": (_i, [C.POINTER(HeadTrainArgs), _f, _i, _f, _i, _f]),
    "cf_head_bwd_dx_workspace_bytes": (C.c_size_t, [_i, _i, _i, _i, _i, _i]),
    "cf_offmask_activate": (_i, [_f, C.c_long, _f]),
    "cf_conv3x3_bwd_workspace_bytes": (C.c_size_t, [_i, _i, _i, _i]),
    "cf_conv3x3_bwd_weight": (_i, [_f, _f, _f, _i, _i, _i, _i, _f, _f, _f, C.c_size_t, _f]),
    "cf_conv3x3_bwd_data": (_i, [_f, _f, _f, _i, _i, _i, _i, _f, _f]),
    "cf_bn_relu_workspace_bytes": (C.c_size_t, [C.c_long, _i]),
    "cf_bn_relu_train_forward": (_i, [_f, _f, _f, _f, _f, _i, C.c_float, C.c_float, C.c_long, _i, _f, _f, _f, _f, C.c_size_t, _f]),
    "cf_bn_relu_backward": (_i, [_f, _f, _f, _f, _f, _f, _i, C.c_long, _i, _f, _f, _f, _f, C.c_size_t, _f]),
    "cf_upsample_dw_bwd_workspace_bytes": (C.c_size_t, [_i, _i, _i, _i, _i]),
    "cf_upsample_dw_bwd": (_i, [_f, _f, _f, _i, _i, _i, _i, _i, _f, _f, _f, C.c_size_t, _f]),
    "cf_upsample_dw": (_i, [_f, _f, _f, _f, _i, _i, _i, _i, _i, _f]),
    "cf_conv_bwd_workspace_bytes": (C.c_size_t, [_i, _i, _i, _i, _i, _i, _i]),
    "cf_conv_bwd_weight": (_i, [_f, _f, _i, _i, _i, _i, _i, _i, _i, _f, _f, C.c_size_t, _f]),
    "cf_conv_bwd_data": (_i, [_f, _f, _i, _i, _i, _i, _i, _i, _i, _f, _f]),
    "cf_bn_act_workspace_bytes": (C.c_size_t, [C.c_long, _i]),
    "cf_bn_act_train_forward": (_i, [_f, _f, _f, _f, _i, _f, _f, _i, C.c_float, C.c_float, C.c_long, _i, _f, _f, _f, _f, C.c_size_t, _f]),
    "cf_bn_act_backward": (_i, [_f, _f, _f, _f, _f, _i, _f, _f, _i, C.c_long, _i, _f, _f, _f, _f, _f, C.c_size_t, _f]),
    "cf_maxpool2x2_bwd": (_i, [_f, _f, _i, _i, _i, _i, _f, _f]),
    "cf_stem_conv_bwd_workspace_bytes": (C.c_size_t, [_i, _i, _i, _i, _i, _i, _i]),
    "cf_stem_conv_forward": (_i, [_f, _f, _f, _i, _i, _i, _i, _i, _i, _i, _f, _f]),
    "cf_stem_conv_bwd_weight": (_i, [_f, _f, _f, _i, _i, _i, _i, _i, _i, _i, _f, _f, C.c_size_t, _f]),
    "cf_stem_conv_bwd_data": (_i, [_f, _f, _i, _i, _i, _i, _i, _i, _i, _f, _f]),
    "cf_maxpool2x2": (_i, [_f, _f, _i, _i, _i, _i, _f]),
    "cf_nchw_to_nhwc4": (_i, [_f, _f, _i, _i, _i, _i, _f]),
    "cf_nhwc_to_nchw": (_i, [_f, _f, _i, _i, _i, _i, _i, _f]),
    "cf_nchw_to_nhwc": (_i, [_f, _f, _i, _i, _i, _i, _i, _i, _f]),
    "cf_radar_ingest": (_i, [_f, _f, _i, _i, _i, _f, _i, _i, _d, _d, _i, _f, _f, _f, _f]),
    "cf_preprocess_images": (_i, [_f, _i, _i, _i, C.POINTER(C.c_double), C.POINTER(C.c_float),
                                 C.POINTER(C.c_float), _i, _i, _f, _f]),
    "cf_augment_workspace_bytes": (C.c_size_t, [_i, _i, _i]),
    "cf_augment_images": (_i, [_f, _i, _i, _i, _f, _f, _f, _f, _f, C.POINTER(C.c_float), C.POINTER(C.c_float), _i, _i, _i, _f,
                              _f, C.c_size_t, _f]),
    "cf_topk_workspace_bytes": (C.c_size_t, [_i, _i]),
    "cf_topk_workspace_bytes_nms": (C.c_size_t, [_i, _i, _i, _i, _i]),
    "cf_topk_peaks": (_i, [_f, _i, _i, _i, _i, _i, _i, _f, _f, _f, _f, _f]),
    "cf_topk_peaks_fused_workspace_bytes": (C.c_size_t, [_i, _i, _i, _i, _i]),
    "cf_topk_peaks_fused": (_i, [_f, _i, _i, _i, _i, _i, _f, _f, _f, _f, _f, _f, _f, _f, _f, _f]),
    "cf_topk_peaks_if_changed": (_i, [_f, _i, _i, _i, _i, _i, _i, _f, _f, _f, _f, _f, _f]),
    "cf_checksum64": (_i, [_f, C.c_long, _f, _f]),
    "cf_frustum_assoc": (_i, [_f, _i, _f, _f, _f, _f, _f, _f, _i, _i, _i, C.c_float, _f, _f, _f, _f]),
    "cf_topk_frustum": (_i, [_f, _i, _i, _f, _f, _f, _f, _f, _f, _i, _i, _i, C.c_float, _f, _f, _f, _f, _f, _f, _f, _f]),
    "cf_pc_hm_direct": (_i, [_f, _i, _i, _i, C.c_float, _f, _f, _f]),
    "cf_radar_roi_expand": (_i, [_f, _f, _f, _i, _i, _i, _f, _f, _i, _i, _i, _f, _f, _f, _f]),
    "cf_pillar_expand": (_i, [_f, _f, _f, _i, _i, _i, _f, _f, _i, _i, _d, _d, _d, _f, _f, _f, _f]),
    "cf_decode_gather": (_i, [C.POINTER(DecodeArgs), _f]),
    "cf_post_process": (_i, [_f, _f, _f, _i, _i, _i, _i, _f, _f]),
    "cf_decode_post": (_i, [C.POINTER(DecodeArgs), _f, _f, _f, _f]),
    "cf_decode_gather_unc": (_i, [C.POINTER(DecodeArgs), _f, _f]),
    "cf_decode_post_unc": (_i, [C.POINTER(DecodeArgs), _f, _f, _f, _f, _f]),
    "cf_depth_maps": (_i, [C.POINTER(_f), C.POINTER(C.c_long), _i, _i, _i, _i, _f, _f]),
    "cf_serialize_nuscenes": (_i, [C.POINTER(SerializeArgs), _f]),
    "cf_serialize_max_candidates": (_i, []),
    "cf_spin_us": (_i, [_i, _f]),
    "cf_last_error": (C.c_char_p, []),
    "cf_pack_conv_f16x3_info": (_i, [C.POINTER(PackConvDesc), C.POINTER(PackInfo)]),
    "cf_pack_conv_f16x3": (_i, [C.POINTER(PackConvDesc), _f, _f, _f, C.POINTER(PackInfo)]),
    "cf_pack_dcn_f16_info": (_i, [_i, _i, C.POINTER(PackInfo)]),
    "cf_pack_dcn_f16": (_i, [_f, _f, C.POINTER(PackBn), _i, _i, _f, _f, C.POINTER(PackInfo)]),
    "cf_abi_version": (_i, []),
}

_lib = None


class CfHipError(RuntimeError):
    pass


def load():
    """Load libcfhip.so (once).  Raises if it has not been built - there is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CfHipError(
                f"{LIB_PATH} is missing: build it with `python -m centerfusiondetect3d_amd.build` "
                "(hipcc, gfx950). The CenterFusion forward has no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        if lib.cf_abi_version() != ABI_VERSION:
            raise CfHipError(f"{LIB_PATH} has ABI version {lib.cf_abi_version()}, this package needs {ABI_VERSION}: "
                             "rebuild it with `python -m centerfusiondetect3d_amd.build`")
        _lib = lib
    return _lib


def check(status, what=""):
    if status != 0:
        msg = load().cf_last_error().decode()
        raise CfHipError(f"{what} failed with status {status}: {msg}")


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def stream_ptr():
    import torch
    return torch.cuda.current_stream().cuda_stream
