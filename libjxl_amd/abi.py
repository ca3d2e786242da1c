"""ctypes binding of the C ABI in include/jxl_hip.h (libjxl_hip.so)."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# JXLHIP_SO: another build of the library (an experiment); default = the product
_SO = os.environ.get("JXLHIP_SO") or os.path.join(_HERE, "csrc", "libjxl_hip.so")
_RUNNER_SO = os.path.join(_HERE, "csrc", "libjxl_threads_hip.so")

KERNEL_COUNT = 8
KERNEL_NAMES = ["prepare", "blocks", "filters", "fused", "epf0", "noise", "splines", "upsample"]
# jxlhip_profile_read_ex: the slots above, then those added since (JXLHIP_KERNEL_PATCHES = 8, JXLHIP_KERNEL_BLEND = 9,
# JXLHIP_KERNEL_TONE_MAP = 10, JXLHIP_KERNEL_BLEND_EC = 11, JXLHIP_KERNEL_DC_UPSAMPLE = 12)
KERNEL_COUNT_EX = 13
KERNEL_NAMES_EX = KERNEL_NAMES + ["patches", "blend", "tone_map", "blend_ec", "dc_upsample"]
ERR_NEED_MORE_INPUT = -9  # JXLHIP_ERR_NEED_MORE_INPUT (jxlhip_decode_codestream_partial)
TONE_MAPPING_CONSTANTS = 18  # JXLHIP_TONE_MAPPING_CONSTANTS
# BlendMode (JXLHIP_BLEND_*) and jxlhip_blend_params::save_slot's "none"
BLEND_REPLACE, BLEND_ADD, BLEND_BLEND, BLEND_ALPHA_WEIGHTED_ADD, BLEND_MUL = range(5)
BLEND_NO_SAVE = 0xFFFFFFFF
MODULAR_I16, MODULAR_I32 = 0, 1  # jxlhip_modular_frame::sample_type / jxlhip_modular_image_planes::sample_type
MODULAR_MAX_RCTS = 2
MODULAR_MAX_EXTRA = 4  # jxlhip_modular_image_channels: extra channels beside the colour
# the sequence calls take frames that need blending on images with extra channels: JXLHIP_SEQUENCE_EXTRA_CHANNELS
# (jxlhip_codestream_sequence_info_ex's flags), JXLHIP_OUT_BLEND_EXTRA_CHANNELS (jxlhip_decode_codestream_next's output_kind)
SEQUENCE_EXTRA_CHANNELS = 1
OUT_BLEND_EXTRA_CHANNELS = 0x200
# PatchBlendMode (JXLHIP_PATCH_*)
PATCH_NONE, PATCH_REPLACE, PATCH_ADD, PATCH_MUL, PATCH_BLEND_ABOVE, PATCH_BLEND_BELOW, PATCH_ALPHA_WEIGHTED_ADD_ABOVE, \
    PATCH_ALPHA_WEIGHTED_ADD_BELOW = range(8)


class JxlHipError(RuntimeError):
    pass


class LoopFilter(C.Structure):
    _fields_ = [("gab", C.c_uint32), ("gab_weights", C.c_float * 6),
                ("epf_iters", C.c_uint32), ("epf_sharp_lut", C.c_float * 8),
                ("epf_channel_scale", C.c_float * 3),
                ("epf_quant_mul", C.c_float),
                ("epf_pass0_sigma_scale", C.c_float),
                ("epf_pass2_sigma_scale", C.c_float),
                ("epf_border_sad_mul", C.c_float)]


class OutputFormat(C.Structure):
    """jxlhip_output_format: FromLinearStage + WriteToOutputStage parameters."""
    _fields_ = [("transfer", C.c_uint32), ("sample_type", C.c_uint32),
                ("num_channels", C.c_uint32), ("bits_per_sample", C.c_uint32),
                ("swap_endianness", C.c_uint32), ("tf_param", C.c_float),
                ("luminances", C.c_float * 3)]


class ToneMapping(C.Structure):
    """jxlhip_tone_mapping"""
    _fields_ = [("orig_intensity_target", C.c_float), ("desired_intensity_target", C.c_float),
                ("luminances", C.c_float * 3), ("orig_transfer", C.c_uint32)]


class Display(C.Structure):
    """jxlhip_display (include/jxl_hip_codestream.h)"""
    _fields_ = [("display_nits", C.c_float), ("primaries", C.c_uint32), ("white_point", C.c_uint32)]


PRIM_SRGB, PRIM_CUSTOM, PRIM_2100, PRIM_P3 = 1, 2, 9, 11
WP_D65, WP_CUSTOM, WP_E, WP_DCI = 1, 2, 10, 11
OUT_XYB_PLANAR, OUT_LINEAR_RGB_F32, OUT_PACKED = 0, 1, 2
TF_LINEAR, TF_SRGB, TF_PQ, TF_709, TF_GAMMA, TF_HLG = 0, 1, 2, 3, 4, 5
SAMPLE_F32, SAMPLE_U8, SAMPLE_U16, SAMPLE_F16 = 0, 1, 2, 3


class BlockCtxMap(C.Structure):
    """jxlhip_block_ctx_map (include/jxl_hip_entropy.h)."""
    _fields_ = [("num_dc_thresholds", C.c_uint32 * 3), ("dc_thresholds", (C.c_int32 * 15) * 3),
                ("num_dc_ctxs", C.c_uint32), ("num_qf_thresholds", C.c_uint32),
                ("qf_thresholds", C.c_uint32 * 15), ("num_ctxs", C.c_uint32), ("ctx_map_size", C.c_uint32),
                ("ctx_map", C.c_uint8 * (3 * 13 * 64))]


QUANT_LIBRARY, QUANT_ID, QUANT_DCT2, QUANT_DCT4, QUANT_DCT4X8, QUANT_AFV, QUANT_DCT, QUANT_RAW = range(8)
NUM_QUANT_TABLES, MAX_DISTANCE_BANDS = 17, 17


class QuantEncoding(C.Structure):
    """jxlhip_quant_encoding: one dequant table's parameters (QuantEncodingInternal)."""
    _fields_ = [("mode", C.c_uint32), ("num_bands", C.c_uint32), ("num_bands_afv_4x4", C.c_uint32),
                ("reserved", C.c_uint32), ("bands", (C.c_float * 17) * 3), ("bands_afv_4x4", (C.c_float * 17) * 3),
                ("weights", (C.c_float * 9) * 3)]


QuantEncodings = QuantEncoding * NUM_QUANT_TABLES


class DcGlobal(C.Structure):
    """jxlhip_dc_global (include/jxl_hip_frame.h)."""
    _fields_ = [("dc_quant", C.c_float * 3), ("global_scale", C.c_int32), ("quant_dc", C.c_int32),
                ("cfl_color_factor", C.c_uint32), ("cfl_base_x", C.c_float), ("cfl_base_b", C.c_float),
                ("ytox_dc", C.c_int32), ("ytob_dc", C.c_int32), ("block_ctx_map", BlockCtxMap)]


class SplineSegment(C.Structure):
    """jxlhip_spline_segment (include/jxl_hip_frame.h)."""
    _fields_ = [("center_x", C.c_float), ("center_y", C.c_float), ("inv_sigma", C.c_float),
                ("sigma_over_4_times_intensity", C.c_float), ("color", C.c_float * 3), ("maximum_distance", C.c_float),
                ("y0", C.c_int32), ("y1", C.c_int32)]


class ImageInfo(C.Structure):
    """jxlhip_image_info (include/jxl_hip_frame.h)."""
    _fields_ = [("xsize", C.c_uint32), ("ysize", C.c_uint32), ("xyb_encoded", C.c_uint32),
                ("num_extra_channels", C.c_uint32), ("ec_dim_shift", C.c_void_p), ("have_animation", C.c_uint32),
                ("have_timecodes", C.c_uint32), ("is_preview", C.c_uint32), ("bits_per_sample", C.c_uint32)]


class BitDepth(C.Structure):
    """jxlhip_bit_depth (include/jxl_hip_frame.h)."""
    _fields_ = [("floating_point_sample", C.c_uint32), ("bits_per_sample", C.c_uint32),
                ("exponent_bits_per_sample", C.c_uint32)]


class ExtraChannel(C.Structure):
    """jxlhip_extra_channel (include/jxl_hip_frame.h)."""
    _fields_ = [("all_default", C.c_uint32), ("type", C.c_uint32), ("bit_depth", BitDepth), ("dim_shift", C.c_uint32),
                ("name_length", C.c_uint32), ("alpha_associated", C.c_uint32), ("spot_color", C.c_float * 4),
                ("cfa_channel", C.c_uint32)]


class ColorEncoding(C.Structure):
    """jxlhip_color_encoding (include/jxl_hip_frame.h)."""
    _fields_ = [("all_default", C.c_uint32), ("want_icc", C.c_uint32), ("color_space", C.c_uint32),
                ("white_point", C.c_uint32), ("primaries", C.c_uint32), ("have_gamma", C.c_uint32),
                ("gamma", C.c_uint32), ("transfer_function", C.c_uint32), ("rendering_intent", C.c_uint32),
                ("white_xy", C.c_int32 * 2), ("primaries_xy", C.c_int32 * 6)]


class ImageHeader(C.Structure):
    """jxlhip_image_header (include/jxl_hip_frame.h)."""
    _fields_ = [("xsize", C.c_uint32), ("ysize", C.c_uint32), ("all_default", C.c_uint32), ("orientation", C.c_uint32),
                ("have_intrinsic_size", C.c_uint32), ("intrinsic_xsize", C.c_uint32), ("intrinsic_ysize", C.c_uint32),
                ("have_preview", C.c_uint32), ("preview_xsize", C.c_uint32), ("preview_ysize", C.c_uint32),
                ("have_animation", C.c_uint32), ("tps_numerator", C.c_uint32), ("tps_denominator", C.c_uint32),
                ("num_loops", C.c_uint32), ("have_timecodes", C.c_uint32), ("bit_depth", BitDepth),
                ("modular_16_bit_buffer_sufficient", C.c_uint32), ("num_extra_channels", C.c_uint32),
                ("xyb_encoded", C.c_uint32), ("color_encoding", ColorEncoding),
                ("tone_mapping_all_default", C.c_uint32), ("intensity_target", C.c_float), ("min_nits", C.c_float),
                ("relative_to_max_display", C.c_uint32), ("linear_below", C.c_float), ("extensions", C.c_uint64),
                ("transform_all_default", C.c_uint32), ("opsin_all_default", C.c_uint32),
                ("inverse_opsin_matrix", C.c_float * 9), ("opsin_biases", C.c_float * 3),
                ("quant_biases", C.c_float * 4), ("custom_weights_mask", C.c_uint32),
                ("upsampling2_weights", C.c_float * 15), ("upsampling4_weights", C.c_float * 55),
                ("upsampling8_weights", C.c_float * 210)]


class FrameHeader(C.Structure):
    """jxlhip_frame_header (include/jxl_hip_frame.h)."""
    _fields_ = [("all_default", C.c_uint32), ("frame_type", C.c_uint32), ("is_modular", C.c_uint32),
                ("color_transform", C.c_uint32), ("flags", C.c_uint64), ("chroma_mode", C.c_uint32 * 3),
                ("upsampling", C.c_uint32), ("group_size_shift", C.c_uint32), ("x_qm_scale", C.c_uint32),
                ("b_qm_scale", C.c_uint32), ("num_passes", C.c_uint32), ("num_downsample", C.c_uint32),
                ("shift", C.c_uint32 * 11), ("downsample", C.c_uint32 * 4), ("last_pass", C.c_uint32 * 4),
                ("dc_level", C.c_uint32), ("custom_size_or_origin", C.c_uint32), ("x0", C.c_int32), ("y0", C.c_int32),
                ("coded_xsize", C.c_uint32), ("coded_ysize", C.c_uint32), ("blend_mode", C.c_uint32),
                ("blend_alpha_channel", C.c_uint32), ("blend_clamp", C.c_uint32), ("blend_source", C.c_uint32),
                ("duration", C.c_uint32), ("timecode", C.c_uint32), ("is_last", C.c_uint32),
                ("save_as_reference", C.c_uint32), ("save_before_color_transform", C.c_uint32),
                ("name_length", C.c_uint32), ("extensions", C.c_uint64), ("lf_all_default", C.c_uint32),
                ("gab_custom", C.c_uint32), ("epf_sharp_custom", C.c_uint32), ("epf_weight_custom", C.c_uint32),
                ("epf_sigma_custom", C.c_uint32), ("lf", LoopFilter), ("epf_pass1_zeroflush", C.c_float),
                ("epf_pass2_zeroflush", C.c_float), ("epf_sigma_for_modular", C.c_float), ("lf_extensions", C.c_uint64),
                ("xsize", C.c_uint32), ("ysize", C.c_uint32), ("xsize_blocks", C.c_uint32), ("ysize_blocks", C.c_uint32),
                ("group_dim", C.c_uint32), ("xsize_groups", C.c_uint32), ("ysize_groups", C.c_uint32),
                ("num_groups", C.c_uint64), ("num_dc_groups", C.c_uint64), ("num_toc_entries", C.c_uint64),
                ("x_dm_multiplier", C.c_float), ("b_dm_multiplier", C.c_float),
                ("num_extra_channels", C.c_uint32), ("ec_upsampling", C.c_uint32 * 4), ("image_bits", C.c_uint32),
                ("ec_blend_mode", C.c_uint32 * 4), ("ec_blend_alpha_channel", C.c_uint32 * 4), ("ec_blend_clamp", C.c_uint32 * 4),
                ("ec_blend_source", C.c_uint32 * 4), ("ec_blend_any", C.c_uint32)]


class CodestreamInfo(C.Structure):
    """jxlhip_codestream_info (include/jxl_hip_codestream.h)."""
    _fields_ = [("xsize", C.c_uint32), ("ysize", C.c_uint32), ("container", C.c_uint32), ("orientation", C.c_uint32),
                ("intensity_target", C.c_float), ("bits_per_sample", C.c_uint32), ("transfer_function", C.c_uint32),
                ("primaries", C.c_uint32), ("white_point", C.c_uint32), ("num_passes", C.c_uint32),
                ("num_groups", C.c_uint32), ("num_dc_groups", C.c_uint32), ("epf_iters", C.c_uint32),
                ("gab", C.c_uint32), ("used_acs", C.c_uint32), ("coeff_type", C.c_uint32), ("modular", C.c_uint32),
                ("num_extra_channels", C.c_uint32), ("alpha_bits", C.c_uint32), ("alpha_premultiplied", C.c_uint32),
                ("luminances", C.c_float * 3), ("gamma", C.c_float), ("icc_size", C.c_uint32), ("grey", C.c_uint32),
                ("upsampling", C.c_uint32)]


class ModularImagePlanes(C.Structure):
    """jxlhip_modular_image_planes (include/jxl_hip_frame.h)."""
    _fields_ = [("planes", C.c_void_p * 3), ("stride_samples", C.c_size_t), ("sample_type", C.c_uint32),
                ("group_rct", C.c_void_p), ("global_rct", C.c_uint16), ("global_tree", C.c_uint32),
                ("global_on_host", C.c_uint32), ("groups_on_device", C.c_uint32), ("groups_on_host", C.c_uint32)]


class ModularFrame(C.Structure):
    """jxlhip_modular_frame (include/jxl_hip.h)."""
    _fields_ = [("xsize", C.c_uint32), ("ysize", C.c_uint32), ("planes", C.c_void_p * 3), ("stride_samples", C.c_size_t),
                ("sample_type", C.c_uint32), ("bits_per_sample", C.c_uint32), ("group_dim", C.c_uint32),
                ("group_rct", C.c_void_p), ("global_rct", C.c_uint16)]


class ModularImageChannels(C.Structure):
    """jxlhip_modular_image_channels (include/jxl_hip_frame.h)."""
    _fields_ = [("num_color", C.c_uint32), ("num_extra", C.c_uint32), ("planes", C.c_void_p * 3),
                ("extra_planes", C.c_void_p * 4), ("extra_bits", C.c_uint32 * 4), ("stride_samples", C.c_size_t),
                ("sample_type", C.c_uint32), ("group_rct", C.c_void_p), ("global_rct", C.c_uint16),
                ("global_tree", C.c_uint32), ("global_on_host", C.c_uint32), ("groups_on_device", C.c_uint32),
                ("groups_on_host", C.c_uint32)]


class ModularChannels(C.Structure):
    """jxlhip_modular_channels (include/jxl_hip.h)."""
    _fields_ = [("xsize", C.c_uint32), ("ysize", C.c_uint32), ("num_color", C.c_uint32), ("planes", C.c_void_p * 3),
                ("alpha_plane", C.c_void_p), ("alpha_bits", C.c_uint32), ("stride_samples", C.c_size_t),
                ("sample_type", C.c_uint32), ("bits_per_sample", C.c_uint32), ("group_dim", C.c_uint32),
                ("group_rct", C.c_void_p), ("global_rct", C.c_uint16)]


class PartialInfo(C.Structure):
    """jxlhip_partial_info"""
    _fields_ = [(n, C.c_uint32) for n in ("complete", "num_passes", "num_groups", "groups_complete", "groups_partial",
                                          "groups_dc_only", "have_ac_global")] + [("bytes_used", C.c_uint64)]


class SequenceInfo(C.Structure):
    """jxlhip_sequence_info"""
    _fields_ = [(n, C.c_uint32) for n in ("have_animation", "tps_numerator", "tps_denominator", "num_loops", "have_timecodes",
                                          "num_coded_frames", "num_displayed_frames")] + [("why", C.c_char_p)]


class SequenceFrame(C.Structure):
    """jxlhip_sequence_frame"""
    _fields_ = [("index", C.c_uint32), ("duration", C.c_uint32), ("timecode", C.c_uint32), ("is_last", C.c_uint32),
                ("name_length", C.c_uint32), ("have_crop", C.c_uint32), ("x0", C.c_int32), ("y0", C.c_int32),
                ("xsize", C.c_uint32), ("ysize", C.c_uint32), ("blend_mode", C.c_uint32), ("blend_source", C.c_uint32),
                ("blend_clamp", C.c_uint32), ("save_as_reference", C.c_uint32), ("coded_frames", C.c_uint32)]


class FrameParams(C.Structure):
    _fields_ = [("xsize", C.c_uint32), ("ysize", C.c_uint32),
                ("coeff_type", C.c_uint32), ("output_kind", C.c_uint32),
                ("global_scale", C.c_int32), ("quant_dc", C.c_int32),
                ("x_dm_multiplier", C.c_float), ("b_dm_multiplier", C.c_float),
                ("quant_biases", C.c_float * 4),
                ("cfl_base_x", C.c_float), ("cfl_base_b", C.c_float),
                ("cfl_color_factor", C.c_uint32),
                ("lf", LoopFilter),
                ("opsin_biases", C.c_float * 3),
                ("inverse_opsin_matrix", C.c_float * 9),
                ("stripe_group_y0", C.c_uint32),
                ("stripe_group_rows", C.c_uint32),
                ("out_format", OutputFormat),
                ("used_acs", C.c_uint32), ("undo_orientation", C.c_uint32)]


class BlendExtraChannel(C.Structure):
    """jxlhip_blend_extra_channel"""
    _fields_ = [("is_alpha", C.c_uint32), ("alpha_associated", C.c_uint32), ("mode", C.c_uint32),
                ("alpha_channel", C.c_uint32), ("clamp", C.c_uint32), ("source", C.c_uint32)]


class BlendExtraParams(C.Structure):
    """jxlhip_blend_extra_params"""
    _fields_ = [("num_extra_channels", C.c_uint32), ("channel", BlendExtraChannel * 4), ("color_alpha_channel", C.c_uint32),
                ("planes", C.c_void_p * 4), ("stride_floats", C.c_size_t)]


class BlendParams(C.Structure):
    """jxlhip_blend_params"""
    _fields_ = [("image_xsize", C.c_uint32), ("image_ysize", C.c_uint32), ("x0", C.c_int32), ("y0", C.c_int32),
                ("mode", C.c_uint32), ("clamp", C.c_uint32), ("source", C.c_uint32), ("save_slot", C.c_uint32)]


class FrameInputs(C.Structure):
    _fields_ = [("coeffs", C.c_void_p * 3),
                ("ac_strategy", C.c_void_p), ("raw_quant", C.c_void_p),
                ("epf_sharpness", C.c_void_p),
                ("ytox_map", C.c_void_p), ("ytob_map", C.c_void_p),
                ("dc", C.c_void_p * 3),
                ("dequant_table", C.c_void_p)]


def make_params(d):
    """dict (libjxl_amd.synth.synth_frame) -> FrameParams."""
    p = FrameParams()
    for k in ("xsize", "ysize", "coeff_type", "output_kind", "global_scale",
              "quant_dc", "x_dm_multiplier", "b_dm_multiplier", "cfl_base_x",
              "cfl_base_b", "cfl_color_factor", "stripe_group_y0",
              "stripe_group_rows"):
        setattr(p, k, d[k])
    p.used_acs = d.get("used_acs", 0)
    p.undo_orientation = d.get("undo_orientation", 0)
    p.quant_biases[:] = d["quant_biases"]
    p.opsin_biases[:] = d["opsin_biases"]
    p.inverse_opsin_matrix[:] = d["inverse_opsin_matrix"]
    p.lf.gab = d["gab"]
    p.lf.gab_weights[:] = d["gab_weights"]
    p.lf.epf_iters = d["epf_iters"]
    p.lf.epf_sharp_lut[:] = d["epf_sharp_lut"]
    p.lf.epf_channel_scale[:] = d["epf_channel_scale"]
    p.lf.epf_quant_mul = d["epf_quant_mul"]
    p.lf.epf_pass0_sigma_scale = d["epf_pass0_sigma_scale"]
    p.lf.epf_pass2_sigma_scale = d["epf_pass2_sigma_scale"]
    p.lf.epf_border_sad_mul = d["epf_border_sad_mul"]
    of = d.get("out_format")
    if of:
        p.out_format.transfer = of.get("transfer", TF_LINEAR)
        p.out_format.sample_type = of.get("sample_type", SAMPLE_F32)
        p.out_format.num_channels = of.get("num_channels", 3)
        p.out_format.bits_per_sample = of.get("bits_per_sample", 0)
        p.out_format.swap_endianness = of.get("swap_endianness", 0)
        p.out_format.tf_param = of.get("tf_param", 0.0)
        p.out_format.luminances[:] = of.get("luminances", (0.2126, 0.7152, 0.0722))
    return p


def library_path():
    return _SO


def runner_library_path():
    return _RUNNER_SO


_lib = None

# every symbol include/jxl_hip.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "jxlhip_covered_blocks_x", "jxlhip_covered_blocks_y",
    "jxlhip_log2_covered_blocks", "jxlhip_quant_table_of_strategy",
    "jxlhip_dequant_table_offset", "jxlhip_status_string", "jxlhip_create", "jxlhip_create_ex", "jxlhip_create_multi",
    "jxlhip_destroy", "jxlhip_last_error", "jxlhip_debug_reload_env", "jxlhip_set_stream",
    "jxlhip_frame_begin", "jxlhip_frame_set_inputs", "jxlhip_upload_side_info",
    "jxlhip_submit_group", "jxlhip_set_alpha", "jxlhip_set_noise", "jxlhip_noise_rng_state", "jxlhip_set_splines", "jxlhip_set_upsampling", "jxlhip_set_dc_only_groups", "jxlhip_set_reference_frame", "jxlhip_set_patches", "jxlhip_set_blending", "jxlhip_set_tone_mapping", "jxlhip_tone_mapping_constants", "jxlhip_canvas_read", "jxlhip_set_blending_extra", "jxlhip_canvas_read_extra", "jxlhip_frame_extra_read", "jxlhip_profile_read_ex", "jxlhip_alpha_staging", "jxlhip_decode_blocks", "jxlhip_halo_rows",
    "jxlhip_halo_export", "jxlhip_halo_import", "jxlhip_decode_filters", "jxlhip_decode_filters_rows", "jxlhip_stripe_begin",
    "jxlhip_stripe_finish", "jxlhip_decode_frame", "jxlhip_decode_modular_frame", "jxlhip_decode_modular_channels",
    "jxlhip_decode_frame_host", "jxlhip_decode_frame_pinned",
    "jxlhip_sync", "jxlhip_export_xyb", "jxlhip_get_sigma",
    "jxlhip_set_concurrency_hint", "jxlhip_debug_prepare_launches", "jxlhip_profile_enable", "jxlhip_profile_read",
    "jxlhip_dequant_tables", "jxlhip_default_dequant_tables", "jxlhip_dequant_dc",
    "jxlhip_dequant_dc_groups",
    # include/jxl_hip_entropy.h
    "jxlhip_ac_pass_decode", "jxlhip_ac_pass_destroy", "jxlhip_ac_pass_max_num_bits",
    "jxlhip_ac_pass_used_orders", "jxlhip_ac_pass_order", "jxlhip_ac_group_decode", "jxlhip_ac_group_decode_sparse",
    "jxlhip_ac_group_decode_submit", "jxlhip_block_ctx_map_decode", "jxlhip_quant_dc_contexts",
    "jxlhip_dequant_encodings_decode", "jxlhip_ac_global_decode", "jxlhip_ac_group_decode_submit_passes",
    "jxlhip_ac_groups_decode_submit", "jxlhip_ac_groups_decode_submit_ex", "jxlhip_num_toc_entries", "jxlhip_toc_decode", "jxlhip_ac_global_decode_at",
    # include/jxl_hip_frame.h
    "jxlhip_frame_header_decode", "jxlhip_dc_global_decode", "jxlhip_noise_lut_decode", "jxlhip_splines_decode",
    "jxlhip_splines_from_quantized", "jxlhip_splines_destroy", "jxlhip_splines_quantized", "jxlhip_splines_segments", "jxlhip_modular_frame_decode", "jxlhip_patches_decode", "jxlhip_patches_from_list", "jxlhip_patches_list", "jxlhip_patches_destroy", "jxlhip_image_header_decode", "jxlhip_icc_decode", "jxlhip_output_opsin_matrix",
    "jxlhip_modular_global_decode", "jxlhip_modular_tree_destroy", "jxlhip_dc_group_decode", "jxlhip_dc_group_decode_staged",
    "jxlhip_modular_ac_group_decode", "jxlhip_modular_ac_group_decode_f32", "jxlhip_modular_extra_channel_f32",
    "jxlhip_modular_groups_are_final", "jxlhip_modular_uses_dc_groups", "jxlhip_modular_finalize",
    "jxlhip_modular_extra_channel_rows_f32", "jxlhip_modular_ac_group_decode_f32_strided", "jxlhip_modular_image_decode",
    "jxlhip_modular_image_decode_channels",
    # include/jxl_hip_codestream.h
    "jxlhip_codestream_basic_info", "jxlhip_decode_codestream", "jxlhip_decode_codestream_extra",
    "jxlhip_codestream_icc_profile", "jxlhip_codestream_phase_ms", "jxlhip_codestream_sequence_info", "jxlhip_codestream_sequence_info_ex",
    "jxlhip_decode_codestream_next", "jxlhip_codestream_set_display", "jxlhip_codestream_display_info",
    "jxlhip_codestream_partial_info", "jxlhip_decode_codestream_partial",
]


def load_library():
    """Loads libjxl_hip.so; raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise JxlHipError(
            f"{_SO} not built: run `python -c 'import __graft_entry__ as g; g.build()'`"
            " (hipcc --offload-arch=gfx950). There is no CPU fallback.")
    L = C.CDLL(_SO)
    vp, sz, u32, i32 = C.c_void_p, C.c_size_t, C.c_uint32, C.c_int
    L.jxlhip_dequant_table_offset.restype = sz
    L.jxlhip_dequant_table_offset.argtypes = [i32, i32]
    L.jxlhip_status_string.restype = C.c_char_p
    L.jxlhip_last_error.restype = C.c_char_p
    L.jxlhip_last_error.argtypes = [vp]
    L.jxlhip_debug_reload_env.restype = None
    L.jxlhip_debug_reload_env.argtypes = []
    L.jxlhip_create.argtypes = [i32, C.POINTER(vp)]
    L.jxlhip_create_ex.argtypes = [i32, vp, C.POINTER(vp)]
    L.jxlhip_create_multi.argtypes = [vp, i32, vp, C.POINTER(vp)]
    L.jxlhip_destroy.argtypes = [vp]
    L.jxlhip_destroy.restype = None
    L.jxlhip_set_stream.argtypes = [vp, vp, i32]
    L.jxlhip_ac_pass_decode.argtypes = [vp, sz, C.POINTER(sz), u32, u32, vp, C.POINTER(vp)]
    L.jxlhip_block_ctx_map_decode.argtypes = [vp, sz, C.POINTER(sz), C.POINTER(BlockCtxMap)]
    L.jxlhip_quant_dc_contexts.argtypes = [C.POINTER(BlockCtxMap), sz, vp * 3, vp]
    L.jxlhip_ac_pass_destroy.argtypes = [vp]
    L.jxlhip_ac_pass_destroy.restype = None
    L.jxlhip_ac_pass_max_num_bits.argtypes = [vp]
    L.jxlhip_ac_pass_max_num_bits.restype = u32
    L.jxlhip_ac_pass_used_orders.argtypes = [vp]
    L.jxlhip_ac_pass_used_orders.restype = u32
    L.jxlhip_ac_group_decode.argtypes = [vp, u32, u32, u32, u32, vp, vp, vp, vp, sz, C.POINTER(sz), u32, u32,
                                         vp * 3, C.POINTER(sz)]
    L.jxlhip_ac_group_decode_sparse.argtypes = [vp, u32, u32, u32, u32, vp, vp, vp, vp, sz, C.POINTER(sz), u32,
                                                vp * 3, u32 * 3, u32 * 3, C.POINTER(sz)]
    L.jxlhip_ac_group_decode_submit.argtypes = [vp, vp, u32, vp, vp, vp, vp, sz, C.POINTER(sz)]
    L.jxlhip_ac_group_decode_submit_passes.argtypes = [vp, u32, vp, vp, u32, vp, vp, vp, vp, vp, vp]
    L.jxlhip_ac_groups_decode_submit.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp]
    L.jxlhip_ac_groups_decode_submit_ex.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.jxlhip_num_toc_entries.argtypes = [u32, u32, u32]
    L.jxlhip_num_toc_entries.restype = u32
    L.jxlhip_toc_decode.argtypes = [vp, sz, C.POINTER(sz), u32, vp, vp, vp]
    L.jxlhip_frame_header_decode.argtypes = [vp, sz, C.POINTER(sz), C.POINTER(ImageInfo), C.POINTER(FrameHeader)]
    L.jxlhip_dc_global_decode.argtypes = [vp, sz, C.POINTER(sz), C.c_uint64, C.POINTER(DcGlobal)]
    L.jxlhip_noise_lut_decode.argtypes = [vp, sz, C.POINTER(sz), C.POINTER(C.c_float)]
    L.jxlhip_splines_decode.argtypes = [vp, sz, C.POINTER(sz), C.c_uint64, C.POINTER(vp)]
    L.jxlhip_splines_from_quantized.argtypes = [u32, vp, vp, vp, vp, i32, C.POINTER(vp)]
    L.jxlhip_splines_destroy.argtypes = [vp]
    L.jxlhip_splines_destroy.restype = None
    L.jxlhip_splines_segments.argtypes = [vp, u32, u32, C.c_float, C.c_float, vp, sz, C.POINTER(sz)]
    L.jxlhip_set_splines.argtypes = [vp, vp]
    L.jxlhip_set_upsampling.argtypes = [vp, u32, C.POINTER(C.c_float), u32, u32]
    L.jxlhip_set_dc_only_groups.argtypes = [vp, vp, C.POINTER(C.c_float)]
    L.jxlhip_patches_decode.argtypes = [vp, sz, C.POINTER(sz), u32, u32, u32, vp, C.POINTER(vp)]
    L.jxlhip_patches_from_list.argtypes = [u32, vp, u32, vp, u32, u32, vp, C.POINTER(vp)]
    L.jxlhip_patches_list.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), vp, vp]
    L.jxlhip_patches_destroy.argtypes = [vp]
    L.jxlhip_modular_frame_decode.argtypes = [vp, sz, C.POINTER(sz), C.POINTER(FrameHeader), vp, sz, C.POINTER(C.c_char_p)]
    L.jxlhip_patches_destroy.restype = None
    L.jxlhip_set_reference_frame.argtypes = [vp, u32, u32, u32, vp, sz, i32]
    L.jxlhip_set_patches.argtypes = [vp, vp]
    L.jxlhip_set_blending.argtypes = [vp, C.POINTER(BlendParams)]
    L.jxlhip_set_tone_mapping.argtypes = [vp, C.POINTER(ToneMapping)]
    L.jxlhip_tone_mapping_constants.argtypes = [C.POINTER(ToneMapping), u32, C.POINTER(C.c_float), sz]
    L.jxlhip_canvas_read.argtypes = [vp, u32, vp, sz, C.POINTER(u32), C.POINTER(u32)]
    L.jxlhip_set_blending_extra.argtypes = [vp, C.POINTER(BlendExtraParams)]
    L.jxlhip_canvas_read_extra.argtypes = [vp, u32, u32, vp, sz, C.POINTER(u32), C.POINTER(u32)]
    L.jxlhip_frame_extra_read.argtypes = [vp, u32, vp, sz]
    L.jxlhip_profile_read_ex.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(u32), u32]
    L.jxlhip_splines_quantized.argtypes = [vp, C.POINTER(u32), C.POINTER(sz), C.POINTER(i32), vp, vp, vp, vp]
    L.jxlhip_modular_global_decode.argtypes = [vp, sz, C.POINTER(sz), C.POINTER(FrameHeader), C.POINTER(vp)]
    L.jxlhip_modular_tree_destroy.argtypes = [vp]
    L.jxlhip_modular_tree_destroy.restype = None
    L.jxlhip_modular_ac_group_decode.argtypes = [vp, C.POINTER(FrameHeader), u32, u32, vp, sz, C.POINTER(sz)]
    L.jxlhip_modular_extra_channel_f32.argtypes = [vp, u32, u32, u32, vp, sz]
    L.jxlhip_modular_groups_are_final.argtypes = [vp]
    L.jxlhip_modular_uses_dc_groups.argtypes = [vp]
    L.jxlhip_modular_finalize.argtypes = [vp, vp, vp]
    L.jxlhip_modular_extra_channel_rows_f32.argtypes = [vp, u32, u32, u32, u32, u32, vp, sz]
    L.jxlhip_modular_ac_group_decode_f32.argtypes = [vp, C.POINTER(FrameHeader), u32, u32, vp, sz, C.POINTER(sz), vp, u32, vp, sz]
    L.jxlhip_dc_group_decode.argtypes = [vp, vp, sz, C.POINTER(sz), C.POINTER(FrameHeader), C.c_uint32,
                                         C.POINTER(vp), C.POINTER(C.c_uint32), vp, vp, vp, vp, vp,
                                         C.POINTER(C.c_uint32)]
    L.jxlhip_dc_group_decode_staged.argtypes = [vp, vp, sz, C.POINTER(sz), C.POINTER(FrameHeader), C.c_uint32,
                                                C.POINTER(vp), C.POINTER(C.c_uint32), vp, vp, vp, vp, vp,
                                                C.POINTER(C.c_uint32), vp, vp]
    L.jxlhip_image_header_decode.argtypes = [vp, sz, C.POINTER(sz), C.POINTER(ExtraChannel), sz,
                                             C.POINTER(ImageHeader)]
    L.jxlhip_output_opsin_matrix.argtypes = [C.POINTER(ImageHeader), C.c_float * 9, C.c_float * 3]
    L.jxlhip_frame_begin.argtypes = [vp, C.POINTER(FrameParams)]
    L.jxlhip_frame_set_inputs.argtypes = [vp, C.POINTER(FrameInputs)]
    L.jxlhip_upload_side_info.argtypes = [vp, vp, vp, vp, vp, vp, vp * 3, vp]
    L.jxlhip_submit_group.argtypes = [vp, u32, vp * 3, sz]
    L.jxlhip_set_alpha.argtypes = [vp, vp, sz]
    L.jxlhip_set_noise.argtypes = [vp, C.POINTER(C.c_float), C.c_uint32, C.c_uint32]
    L.jxlhip_noise_rng_state.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                         C.POINTER(C.c_uint64)]
    L.jxlhip_alpha_staging.argtypes = [vp, C.POINTER(vp), C.POINTER(sz)]
    L.jxlhip_decode_blocks.argtypes = [vp]
    L.jxlhip_halo_rows.argtypes = [vp]
    L.jxlhip_halo_export.argtypes = [vp, i32, vp]
    L.jxlhip_halo_import.argtypes = [vp, i32, vp]
    L.jxlhip_decode_filters.argtypes = [vp, vp, sz, sz]
    L.jxlhip_decode_filters_rows.argtypes = [vp, vp, sz, sz, u32, u32]
    L.jxlhip_stripe_begin.argtypes = [vp, vp, vp]
    L.jxlhip_stripe_finish.argtypes = [vp, vp, vp, vp, sz, sz, u32, u32]
    L.jxlhip_decode_frame.argtypes = [vp, vp, sz, sz]
    L.jxlhip_decode_frame_host.argtypes = [vp, vp, sz, sz]
    L.jxlhip_decode_frame_pinned.argtypes = [vp, C.POINTER(vp), C.POINTER(sz)]
    L.jxlhip_sync.argtypes = [vp]
    L.jxlhip_export_xyb.argtypes = [vp, vp * 3, sz]
    L.jxlhip_get_sigma.argtypes = [vp, C.POINTER(vp), C.POINTER(sz)]
    L.jxlhip_profile_enable.argtypes = [vp, i32]
    L.jxlhip_set_concurrency_hint.argtypes = [vp, i32]
    L.jxlhip_debug_prepare_launches.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.jxlhip_profile_read.argtypes = [vp, C.c_float * KERNEL_COUNT, u32 * KERNEL_COUNT]
    L.jxlhip_default_dequant_tables.argtypes = [vp, vp]
    L.jxlhip_dequant_tables.argtypes = [vp, vp, vp]
    L.jxlhip_dequant_encodings_decode.argtypes = [vp, sz, C.POINTER(sz), vp]
    L.jxlhip_ac_global_decode.argtypes = [vp, sz, u32, u32, u32, vp, vp, C.POINTER(u32), C.POINTER(vp),
                                          C.POINTER(sz)]
    L.jxlhip_dequant_dc.argtypes = [vp, vp * 3, vp * 3, vp, C.c_float, C.c_float, i32]
    L.jxlhip_dequant_dc_groups.argtypes = [vp, vp * 3, vp * 3, vp, C.c_float, C.c_float, i32, vp]
    L.jxlhip_codestream_basic_info.argtypes = [vp, sz, C.POINTER(CodestreamInfo)]
    L.jxlhip_codestream_icc_profile.argtypes = [vp, sz, vp, sz, C.POINTER(sz)]
    L.jxlhip_icc_decode.argtypes = [vp, sz, C.POINTER(sz), vp, sz, C.POINTER(sz)]
    L.jxlhip_decode_codestream.argtypes = [vp, vp, vp, vp, sz, u32, vp, vp, sz, sz, C.POINTER(CodestreamInfo)]
    L.jxlhip_codestream_sequence_info.argtypes = [vp, sz, C.POINTER(CodestreamInfo), C.POINTER(SequenceInfo)]
    L.jxlhip_codestream_sequence_info_ex.argtypes = [vp, sz, u32, C.POINTER(CodestreamInfo), C.POINTER(SequenceInfo)]
    L.jxlhip_decode_codestream_next.argtypes = [vp, vp, vp, vp, sz, C.POINTER(C.c_uint64), u32, vp, vp, sz, sz,
                                                C.POINTER(CodestreamInfo), C.POINTER(SequenceFrame)]
    L.jxlhip_codestream_set_display.argtypes = [vp, C.POINTER(Display)]
    L.jxlhip_codestream_display_info.argtypes = [vp, sz, C.POINTER(Display), C.POINTER(CodestreamInfo), C.POINTER(C.c_char_p)]
    L.jxlhip_codestream_phase_ms.argtypes = [vp, C.POINTER(C.c_double)]
    L.jxlhip_codestream_partial_info.argtypes = [vp, sz, C.POINTER(CodestreamInfo), C.POINTER(PartialInfo)]
    L.jxlhip_decode_codestream_partial.argtypes = [vp, vp, vp, vp, sz, u32, vp, vp, sz, sz, C.POINTER(CodestreamInfo),
                                                   C.POINTER(PartialInfo)]
    L.jxlhip_decode_codestream_extra.argtypes = [vp, vp, vp, vp, sz, u32, vp, vp, sz, sz, C.POINTER(vp), u32, sz,
                                                 C.POINTER(CodestreamInfo)]
    L.jxlhip_modular_ac_group_decode_f32_strided.argtypes = [vp, vp, u32, u32, vp, sz, C.POINTER(sz), vp, u32, vp, vp]
    L.jxlhip_modular_image_decode.argtypes = [vp, sz, C.POINTER(sz), C.POINTER(FrameHeader), vp, vp, C.POINTER(ModularImagePlanes),
                                              C.POINTER(C.c_char_p)]
    L.jxlhip_decode_modular_frame.argtypes = [vp, C.POINTER(ModularFrame), u32, C.POINTER(OutputFormat), vp, sz, u32]
    L.jxlhip_modular_image_decode_channels.argtypes = [vp, sz, C.POINTER(sz), C.POINTER(FrameHeader), vp, vp,
                                                       C.POINTER(ModularImageChannels), C.POINTER(C.c_char_p)]
    L.jxlhip_decode_modular_channels.argtypes = [vp, C.POINTER(ModularChannels), u32, C.POINTER(OutputFormat), vp, sz, u32]
    L.jxlhip_ac_global_decode_at.argtypes = [vp, sz, C.POINTER(sz), u32, u32, u32, vp, vp, C.POINTER(u32), C.POINTER(vp)]
    _lib = L
    return L


def splines_from_quantized(splines, quantization_adjustment=0, L=None):
    """jxlhip_splines_from_quantized: an owned jxlhip_splines* (c_void_p) from quantized splines, each a dict with
    "start" (x, y), "deltas" [(ddx, ddy), ...] (the control-point delta-deltas), "color" (3 x 32 ints) and "sigma" (32
    ints).  Returns (rc, handle); free the handle with splines_destroy."""
    import numpy as np
    L = L or load_library()
    n = len(splines)
    starts = np.array([sp["start"] for sp in splines], np.int32).reshape(-1)
    counts = np.array([len(sp["deltas"]) for sp in splines], np.uint32)
    deltas = np.array([d for sp in splines for d in sp["deltas"]] or [(0, 0)], np.int64).astype(np.int32).reshape(-1)
    dcts = np.array([np.concatenate([np.asarray(sp["color"], np.int64).reshape(96), np.asarray(sp["sigma"], np.int64)])
                     for sp in splines], np.int64).astype(np.int32).reshape(-1)
    h = C.c_void_p()
    rc = L.jxlhip_splines_from_quantized(n, starts.ctypes.data, counts.ctypes.data, deltas.ctypes.data,
                                         dcts.ctypes.data, int(quantization_adjustment), C.byref(h))
    return rc, h


def splines_destroy(handle, L=None):
    (L or load_library()).jxlhip_splines_destroy(handle)


def splines_segments(handle, xsize, ysize, y_to_x=0.0, y_to_b=1.0, L=None):
    """jxlhip_splines_segments: (rc, array of SplineSegment) -- the draw list of the frame."""
    L = L or load_library()
    n = C.c_size_t(0)
    rc = L.jxlhip_splines_segments(handle, xsize, ysize, y_to_x, y_to_b, None, 0, C.byref(n))
    if rc:
        return rc, (SplineSegment * 0)()
    out = (SplineSegment * n.value)()
    rc = L.jxlhip_splines_segments(handle, xsize, ysize, y_to_x, y_to_b, out, n.value, C.byref(n))
    return rc, out


def splines_quantized(handle, L=None):
    """jxlhip_splines_quantized: (quantization_adjustment, [dict(start, deltas, color, sigma), ...])."""
    import numpy as np
    L = L or load_library()
    n, nd, adj = C.c_uint32(0), C.c_size_t(0), C.c_int32(0)
    assert L.jxlhip_splines_quantized(handle, C.byref(n), C.byref(nd), C.byref(adj), None, None, None, None) == 0
    starts = np.zeros(2 * n.value, np.int32)
    counts = np.zeros(n.value, np.uint32)
    deltas = np.zeros(max(1, 2 * nd.value), np.int32)
    dcts = np.zeros(128 * n.value, np.int32)
    assert L.jxlhip_splines_quantized(handle, C.byref(n), C.byref(nd), C.byref(adj), starts.ctypes.data,
                                      counts.ctypes.data, deltas.ctypes.data, dcts.ctypes.data) == 0
    out, k = [], 0
    for i in range(n.value):
        m = int(counts[i])
        out.append(dict(start=(int(starts[2 * i]), int(starts[2 * i + 1])),
                        deltas=[(int(deltas[2 * j]), int(deltas[2 * j + 1])) for j in range(k, k + m)],
                        color=dcts[128 * i:128 * i + 96].reshape(3, 32).tolist(),
                        sigma=dcts[128 * i + 96:128 * i + 128].tolist()))
        k += m
    return adj.value, out


class Patch(C.Structure):
    """jxlhip_patch"""
    _fields_ = [(n, C.c_uint32) for n in ("ref", "ref_x0", "ref_y0", "xsize", "ysize", "x", "y", "mode", "alpha_channel",
                                          "clamp")]


def _ref_sizes(ref_sizes):
    import numpy as np
    a = np.zeros((4, 2), np.uint32)
    for slot, wh in (ref_sizes.items() if isinstance(ref_sizes, dict) else enumerate(ref_sizes)):
        a[slot] = wh
    return a


def patches_decode(data, bit_pos, xsize, ysize, ref_sizes, num_extra_channels=0, L=None):
    """jxlhip_patches_decode at bit `bit_pos` of `data`; xsize / ysize = the frame's padded size, ref_sizes = {slot:
    (xsize, ysize)} or a list of four pairs.  Returns (rc, handle, bit position behind the dictionary); free the handle
    with patches_destroy."""
    L = L or load_library()
    data = bytes(data)
    pos, h = C.c_size_t(bit_pos), C.c_void_p()
    rs = _ref_sizes(ref_sizes)
    rc = L.jxlhip_patches_decode(data, len(data), C.byref(pos), xsize, ysize, num_extra_channels, rs.ctypes.data,
                                 C.byref(h))
    return rc, h, pos.value


def patches_from_list(patches, xsize, ysize, ref_sizes, num_extra_channels=0, ec_blendings=None, L=None):
    """jxlhip_patches_from_list: an owned jxlhip_patches* (c_void_p) from a list of dicts with the fields of
    jxlhip_patch (ref_x0, ref_y0, alpha_channel and clamp default to 0, ref to 0) or an [n, 10] uint32 array in their
    order; ec_blendings: per patch, per extra channel a (mode, alpha_channel, clamp) triple.  Returns (rc, handle); free the handle with patches_destroy."""
    import numpy as np
    L = L or load_library()
    if isinstance(patches, np.ndarray):  # [n, 10] uint32 in the field order of jxlhip_patch
        keep = np.ascontiguousarray(patches, np.uint32)
        assert keep.ndim == 2 and keep.shape[1] == len(Patch._fields_), keep.shape
        arr = (Patch * max(1, len(keep))).from_buffer_copy(keep.tobytes() if len(keep) else bytes(C.sizeof(Patch)))
    else:
        arr = (Patch * max(1, len(patches)))()
        for i, p in enumerate(patches):
            for name, _ in Patch._fields_:
                setattr(arr[i], name, int(p.get(name, 0)))
    ec = np.asarray(ec_blendings if ec_blendings is not None else [], np.uint32).reshape(-1)
    assert ec.size == 3 * len(patches) * num_extra_channels
    rs = _ref_sizes(ref_sizes)
    h = C.c_void_p()
    rc = L.jxlhip_patches_from_list(len(patches), C.addressof(arr), num_extra_channels, ec.ctypes.data if ec.size else None,
                                    xsize, ysize, rs.ctypes.data, C.byref(h))
    return rc, h


def patches_list(handle, L=None):
    """jxlhip_patches_list: (list of patch dicts, num_extra_channels, uses_extra_channels, ec_blendings as an array of
    shape (patches, extra channels, 3))."""
    import numpy as np
    L = L or load_library()
    n, nec, uses = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    assert L.jxlhip_patches_list(handle, C.byref(n), C.byref(nec), C.byref(uses), None, None) == 0
    arr = (Patch * max(1, n.value))()
    ec = np.zeros(max(1, 3 * n.value * nec.value), np.uint32)
    assert L.jxlhip_patches_list(handle, C.byref(n), None, None, C.addressof(arr), ec.ctypes.data) == 0
    out = [{name: int(getattr(arr[i], name)) for name, _ in Patch._fields_} for i in range(n.value)]
    return out, nec.value, bool(uses.value), ec[:3 * n.value * nec.value].reshape(n.value, nec.value, 3)


def patches_destroy(handle, L=None):
    (L or load_library()).jxlhip_patches_destroy(handle)
