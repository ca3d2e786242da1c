/*
 * jxl_hip.h -- C ABI of the MI355X (gfx950) VarDCT decode back-end.
 *
 * This is the drop-in boundary for ONE hot path of libjxl: everything between
 * "quantized AC coefficients + per-block side info are in memory" and "float
 * pixels are in the output buffer":
 *
 *   dequant + chroma-from-luma + LLF-from-DC + variable-size inverse transform
 *   -> [Gaborish] -> [EPF0] [EPF1] [EPF2] -> XYB -> linear RGB
 *
 * Each entry point cites the reference interface (path relative to the libjxl
 * tree) that it replaces.  Plain C: pointers + sizes only, no C++/torch types.
 * All functions return JXLHIP_OK (0) or a negative jxlhip_status; nothing
 * throws; there is NO CPU fallback (a missing device is an error).
 *
 * Coordinate / layout conventions are the reference's own:
 *   - block  = 8x8 px; group = 256x256 px = 32x32 blocks; colour tile = 64x64 px
 *     (lib/jxl/frame_dimensions.h:21-27, lib/jxl/chroma_from_luma.h:28-32)
 *   - channel order c = 0:X 1:Y 2:B
 *   - AC coefficient stream per group and channel: varblocks in raster visit
 *     order of their top-left block, 64*covered_blocks coefficients each, in the
 *     layout of the dequant matrix (rows = short side, lib/jxl/dec_group.cc:221,
 *     334-359; lib/jxl/coeff_order_fwd.h:27-43); group g starts at element
 *     g*65536 (lib/jxl/dec_frame.cc:423, lib/jxl/dct_util.h:23-96)
 */
#ifndef JXL_HIP_H_
#define JXL_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define JXLHIP_EXPORT __attribute__((visibility("default")))
#else
#define JXLHIP_EXPORT
#endif

#define JXLHIP_BLOCK_DIM 8
#define JXLHIP_GROUP_DIM 256
#define JXLHIP_GROUP_DIM_IN_BLOCKS 32
#define JXLHIP_GROUP_COEFFS 65536 /* per channel */
#define JXLHIP_COLOR_TILE_DIM_IN_BLOCKS 8
#define JXLHIP_NUM_STRATEGIES 27
#define JXLHIP_NUM_QUANT_TABLES 17
/* lib/jxl/quant_weights.h:412-417: sum(required_size_x*required_size_y)=2056 */
#define JXLHIP_DEQUANT_TABLE_FLOATS (2056 * 64 * 3)

typedef enum {
  JXLHIP_OK = 0,
  JXLHIP_ERR_INVALID_ARGUMENT = -1,
  JXLHIP_ERR_NO_DEVICE = -2,
  JXLHIP_ERR_OUT_OF_MEMORY = -3,
  JXLHIP_ERR_HIP = -4,         /* a HIP runtime call failed; see last_error */
  JXLHIP_ERR_BAD_STREAM = -5,  /* side info violates a format constraint */
  JXLHIP_ERR_STATE = -6,       /* call sequence error */
  JXLHIP_ERR_UNSUPPORTED = -7, /* valid stream feature outside this back-end */
  JXLHIP_ERR_RANGE = -8,       /* a coefficient does not fit the 16-bit buffers: use JXLHIP_COEFF_I32 */
  JXLHIP_ERR_NEED_MORE_INPUT = -9 /* jxlhip_decode_codestream_partial: the bytes end before anything can be drawn */
} jxlhip_status;

/* ACType, lib/jxl/dct_util.h:23; chosen per frame at lib/jxl/dec_frame.cc:421-431 */
typedef enum { JXLHIP_COEFF_I16 = 0, JXLHIP_COEFF_I32 = 1 } jxlhip_coeff_type;

typedef enum {
  /* 3 planes of xsize*ysize floats (plane stride = out_plane_stride floats):
     the frame after the loop filters, still in XYB (ColorSpace::kXYB output) */
  JXLHIP_OUT_XYB_PLANAR = 0,
  /* interleaved linear RGB float, 3 floats per pixel, row stride in bytes
     given at decode time: what XYBStage + WriteToOutputStage(float) produce
     (lib/jxl/render_pipeline/stage_xyb.cc:42-98, stage_write.cc:334-368) */
  JXLHIP_OUT_LINEAR_RGB_F32 = 1,
  /* interleaved RGB / RGBA samples after the colour-encoding and packing
     stages, as described by jxlhip_frame_params::out_format: what
     FromLinearStage + WriteToOutputStage produce for a buffer output
     (lib/jxl/render_pipeline/stage_from_linear.cc:34-155,
     stage_write.cc:254-700, JxlPixelFormat in include/jxl/types.h).  Row
     stride in bytes given at decode time. */
  JXLHIP_OUT_PACKED = 2
} jxlhip_output_kind;

/* Transfer function FromLinearStage applies (the output ColorEncoding's tf;
 * lib/jxl/cms/transfer_functions-inl.h). */
typedef enum jxlhip_transfer {
  JXLHIP_TF_LINEAR = 0, /* OpLinear: samples stay linear */
  JXLHIP_TF_SRGB = 1,   /* OpRgb: TF_SRGB::EncodedFromDisplay (JXL_HIGH_PRECISION) */
  JXLHIP_TF_PQ = 2,     /* OpPq: TF_PQ(tf_param = intensity target in nits)::EncodedFromDisplay */
  JXLHIP_TF_709 = 3,    /* Op709: TF_709::EncodedFromDisplay */
  JXLHIP_TF_GAMMA = 4,  /* OpGamma: x <= 1e-5 ? 0 : FastPowf(x, tf_param = inverse gamma; DCI: 1/2.6) */
  JXLHIP_TF_HLG = 5     /* OpHlg: HlgOOTF::ToSceneLight(tf_param = intensity target, luminances) on the
                           pixel, then TF_HLG::EncodedFromDisplay per sample */
} jxlhip_transfer;

/* JxlDataType of the output buffer (include/jxl/types.h:40-60). */
typedef enum jxlhip_sample_type {
  JXLHIP_SAMPLE_F32 = 0, /* JXL_TYPE_FLOAT */
  JXLHIP_SAMPLE_U8 = 1,  /* JXL_TYPE_UINT8: x (2^bits-1), ordered dither, clamp, round */
  JXLHIP_SAMPLE_U16 = 2, /* JXL_TYPE_UINT16: x (2^bits-1), clamp, round */
  JXLHIP_SAMPLE_F16 = 3  /* JXL_TYPE_FLOAT16 */
} jxlhip_sample_type;

/* Mirrors the members of jxl::ImageOutput / JxlPixelFormat the write stage
 * reads (lib/jxl/dec_cache.h:70-82). */
typedef struct jxlhip_output_format {
  uint32_t transfer;        /* jxlhip_transfer */
  uint32_t sample_type;     /* jxlhip_sample_type */
  uint32_t num_channels;    /* 3 = RGB, 4 = RGBA (alpha = 1.0: the frame has no alpha channel) */
  uint32_t bits_per_sample; /* U8: 1..8, U16: 1..16; ignored for the float types */
  uint32_t swap_endianness; /* U16 / F16 / F32: byte-swap every sample (JXL_BIG_ENDIAN on this host) */
  float tf_param;           /* PQ, HLG: OutputEncodingInfo::desired_intensity_target; GAMMA: inverse_gamma */
  float luminances[3];      /* HLG: OutputEncodingInfo::luminances, the Y row of the output primaries'
                               RGB->XYZ matrix (dec_xyb.cc:187-211; sRGB: 0.2126, 0.7152, 0.0722) */
} jxlhip_output_format;

/* Mirrors jxl::LoopFilter (lib/jxl/loop_filter.h:20-70); values as decoded. */
typedef struct jxlhip_loop_filter {
  uint32_t gab;          /* LoopFilter::gab */
  float gab_weights[6];  /* gab_{x,y,b}_weight{1,2}: x1,x2,y1,y2,b1,b2 */
  uint32_t epf_iters;    /* 0..3 */
  float epf_sharp_lut[8];
  float epf_channel_scale[3];
  float epf_quant_mul;
  float epf_pass0_sigma_scale;
  float epf_pass2_sigma_scale;
  float epf_border_sad_mul;
} jxlhip_loop_filter;

/* The scalar members of PassesSharedState / PassesDecoderState the hot path
 * reads (lib/jxl/passes_state.h:48-95, lib/jxl/dec_cache.h:86-229). */
typedef struct jxlhip_frame_params {
  uint32_t xsize, ysize;       /* FrameDimensions::xsize/ysize (true size) */
  uint32_t coeff_type;         /* jxlhip_coeff_type */
  uint32_t output_kind;        /* jxlhip_output_kind */
  int32_t global_scale;        /* Quantizer::global_scale_ (quantizer.h:82-85) */
  int32_t quant_dc;            /* Quantizer::quant_dc_ */
  float x_dm_multiplier;       /* 0.8^(x_qm_scale-2), dec_cache.h:161 */
  float b_dm_multiplier;       /* 0.8^(b_qm_scale-2), dec_cache.h:162 */
  float quant_biases[4];       /* OpsinParams::quant_biases (dec_xyb.h:27-33) */
  float cfl_base_x;            /* ColorCorrelation::base_correlation_x_ */
  float cfl_base_b;            /* ColorCorrelation::base_correlation_b_ */
  uint32_t cfl_color_factor;   /* ColorCorrelation::color_factor_ (default 84) */
  jxlhip_loop_filter lf;
  float opsin_biases[3];       /* OpsinParams::opsin_biases (negated biases) */
  /* row-major inverse opsin absorbance matrix ALREADY multiplied by
     255/intensity_target (InitSIMDInverseMatrix, opsin_params.cc:35-45) */
  float inverse_opsin_matrix[9];
  /* Multi-GPU: this context decodes AC-group rows [stripe_group_y0,
     stripe_group_y0+stripe_group_rows) of the frame.  0,0 = whole frame. */
  uint32_t stripe_group_y0;
  uint32_t stripe_group_rows;
  /* output_kind == JXLHIP_OUT_PACKED only */
  jxlhip_output_format out_format;
  /* PassesDecoderState::used_acs (dec_cache.h:120): bit s set = raw strategy s
     occurs in the frame; known once the DC groups are decoded.  A hint: transform
     kernels of families without a set bit are not launched.  0 = unknown (everything
     is launched; a strategy missing from a non-zero mask is NOT decoded). */
  uint32_t used_acs;
  /* ImageMetadata::orientation to UNDO while writing (PassesDecoderState::undo_orientation, dec_cache.h:124;
     WriteToOutputStage's flip_x / flip_y / transpose, stage_write.cc:441-457,486,664-680 -- what JxlDecoder does
     unless JxlDecoderSetKeepOrientation).  0 or 1 = write in coded orientation.  2..8: jxlhip_decode_frame /
     jxlhip_decode_frame_host write DISPLAY orientation; for 5..8 the output is ysize pixels wide and xsize rows
     high (strides refer to that shape).  Interleaved outputs only (JXLHIP_OUT_LINEAR_RGB_F32, JXLHIP_OUT_PACKED;
     the 8-bit dither pattern follows the flipped coordinates like the reference's); not with stripes / several
     devices, not with the split calls (JXLHIP_ERR_UNSUPPORTED). */
  uint32_t undo_orientation;
} jxlhip_frame_params;

/* Device pointers of one frame's inputs.  Same content the reference keeps in
 * PassesSharedState (ac_strategy, raw_quant_field, epf_sharpness, cmap, dc) and
 * in PassesDecoderState::coefficients (ACImage).  All frame-sized planes are
 * dense row-major with row stride xsize_blocks (resp. xsize_tiles) elements
 * and cover the WHOLE frame, also when the context only decodes a stripe;
 * coeffs[c] likewise holds all groups (only the stripe's groups are read). */
typedef struct jxlhip_frame_inputs {
  const void* coeffs[3];        /* int16_t or int32_t [num_groups*65536] */
  const uint8_t* ac_strategy;   /* (raw_strategy<<1)|is_first, ac_strategy.h:187-198 */
  const int32_t* raw_quant;     /* 1..256, valid at first blocks (dec_modular.cc:552) */
  const uint8_t* epf_sharpness; /* 0..7 per block */
  const int8_t* ytox_map;       /* per 64x64 tile */
  const int8_t* ytob_map;
  const float* dc[3];           /* dequantized (+smoothed) DC, per block */
  const float* dequant_table;   /* DequantMatrices::table_ layout, see
                                   jxlhip_dequant_table_offset() */
} jxlhip_frame_inputs;

typedef struct jxlhip_ctx jxlhip_ctx;

/* ---- static geometry helpers (host, no device needed) ------------------- */
/* AcStrategy::covered_blocks_x/y, log2_covered_blocks (ac_strategy.h:148-173) */
JXLHIP_EXPORT int jxlhip_covered_blocks_x(int raw_strategy);
JXLHIP_EXPORT int jxlhip_covered_blocks_y(int raw_strategy);
JXLHIP_EXPORT int jxlhip_log2_covered_blocks(int raw_strategy);
/* kAcStrategyToQuantTableMap (quant_weights.h:337-348) */
JXLHIP_EXPORT int jxlhip_quant_table_of_strategy(int raw_strategy);
/* DequantMatrices::Matrix(kind,c) - table_ (quant_weights.h:364-367); floats */
JXLHIP_EXPORT size_t jxlhip_dequant_table_offset(int raw_strategy, int c);
JXLHIP_EXPORT const char* jxlhip_status_string(int status);

/* ---- context ------------------------------------------------------------ */
/* Replaces the per-decoder state setup of PassesDecoderState::Init
 * (dec_cache.h:153-229).  device = HIP device ordinal. */
JXLHIP_EXPORT int jxlhip_create(int device, jxlhip_ctx** out);
/* JxlMemoryManager (lib/include/jxl/memory_manager.h:45-63), restated so that this header stands alone; the
 * layout is the reference's.  Both callbacks or none (lib/threads/thread_parallel_runner.cc:37-53): exactly
 * one NULL is JXLHIP_ERR_INVALID_ARGUMENT. */
typedef struct JxlMemoryManagerHip {
  void* opaque;
  void* (*alloc)(void* opaque, size_t size);
  void (*free)(void* opaque, void* address);
} JxlMemoryManagerHip;
/* The same with the caller's memory manager: the context object and the pinned staging slots of
 * the entropy decoder (pinned in place with hipHostRegister) come from it; device memory comes from hipMalloc,
 * and the bookkeeping of the C++ containers inside the context from the C++ runtime. */
JXLHIP_EXPORT int jxlhip_create_ex(int device, const JxlMemoryManagerHip* memory_manager, jxlhip_ctx** out);
/* One context over SEVERAL devices of this process ("groups shard across the GPUs of one
 * node"): the frame is cut into contiguous stripes of AC-group rows (the first ysg % ndev stripes one row taller),
 * stripe i lives on devices[i].  A device may be listed more than once (several stripes on one GPU).
 * Supported on a multi context: jxlhip_frame_begin, jxlhip_upload_side_info, jxlhip_submit_group,
 * jxlhip_ac_group(s)_decode_submit[_passes] (a group goes to the device of its stripe),
 * jxlhip_decode_frame (out: device memory of devices[0]; the other stripes arrive by peer copies = the gather),
 * jxlhip_decode_frame_host (every device copies its own stripe to the host rows: no gather), jxlhip_halo_rows,
 * jxlhip_sync, jxlhip_last_error, jxlhip_destroy; everything else is JXLHIP_ERR_UNSUPPORTED.
 * Between the two phases each stripe's LoopFilter::Padding() boundary rows go to its neighbours with
 * hipMemcpyPeerAsync (xGMI when peer access is available), ordered by events only: the host never waits inside
 * a frame.  Replaces GroupBorderAssigner / SaveBorders / LoadBorders across devices
 * (lib/jxl/dec_group_border.cc:68-187) and the data-parallel contract of lib/jxl/base/data_parallel.h:50-78. */
JXLHIP_EXPORT int jxlhip_create_multi(const int* devices, int num_devices,
                                      const JxlMemoryManagerHip* memory_manager, jxlhip_ctx** out);
JXLHIP_EXPORT void jxlhip_destroy(jxlhip_ctx* ctx);
JXLHIP_EXPORT const char* jxlhip_last_error(const jxlhip_ctx* ctx);
/* The library samples its debug / test switches (JXLHIP_WP_GENERAL, JXLHIP_CODESTREAM_VERBOSE, JXLHIP_NO_PIPELINE,
 * JXLHIP_TEST_RANGE_GROUP, JXLHIP_MULTI_INTERIOR_FIRST, JXLHIP_MULTI_FORCE_GATHER, JXLHIP_MAX_PIXELS, the kernels'
 * launch-geometry knobs JXLHIP_FUSED_PC_RH, JXLHIP_FILTER_RH, JXLHIP_BIG_WGS, JXLHIP_R_WGS, and the path switches
 * JXLHIP_FILTERS, JXLHIP_SPARSE_UPLOAD, JXLHIP_FUSE, JXLHIP_MFMA, JXLHIP_STAGE_SLOTS, JXLHIP_PREPARE_ONCE) from the environment when a
 * context is created
 * (jxlhip_create / _ex / _multi) and at their first use before that; a test that changes one of them under a live
 * context calls this to have them read again (the path switches stay as a context was created with them).  Decoding
 * and kernel launches never call getenv (no reference counterpart: libjxl has no run-time switches on this path). */
JXLHIP_EXPORT void jxlhip_debug_reload_env(void);
/* external != 0: all launches go to the caller's hipStream_t `hip_stream`
 * (NULL = the device's default stream, which is what torch's default stream
 * is); external == 0: back to the context's own non-blocking stream. */
JXLHIP_EXPORT int jxlhip_set_stream(jxlhip_ctx* ctx, void* hip_stream,
                                    int external);

/* Replaces PassesDecoderState::InitForAC + PreparePipeline
 * (dec_cache.cc:78-96,117-371): fixes the frame geometry and the stage list
 * and (re)allocates the device intermediates (XYB planes, sigma image, block
 * offset table). */
JXLHIP_EXPORT int jxlhip_frame_begin(jxlhip_ctx* ctx,
                                     const jxlhip_frame_params* params);

/* Zero-copy path: the caller already has the inputs in device memory.
 * One hand-over, any number of decodes: the side-info arrays (ac_strategy, raw_quant, epf_sharpness, ytox_map,
 * ytob_map) are read by the FIRST decode call after this one, which derives the work lists, the sigma image and the
 * strategy-map check from them once (k_prepare); later decode calls of the same hand-over reuse that.  They must not
 * change between decodes unless jxlhip_frame_set_inputs is called again (the same pointers will do).  Coefficients,
 * DC and the dequant table may change from decode to decode: every decode reads them afresh. */
JXLHIP_EXPORT int jxlhip_frame_set_inputs(jxlhip_ctx* ctx,
                                          const jxlhip_frame_inputs* dev);

/* Host-upload path (what a libjxl FrameDecoder would call).
 * Replaces the reads of shared->ac_strategy/raw_quant_field/epf_sharpness/
 * cmap/dc in DecodeGroupImpl (dec_group.cc:275-316).  Host pointers, dense
 * frame-sized planes; copied asynchronously into context-owned HBM.  The work lists, the sigma image and the
 * strategy-map check (k_prepare; ComputeSigma runs per DC group in the reference too, dec_modular.cc:559) are
 * enqueued right behind the copies, once per call: every decode until the next hand-over reuses them. */
JXLHIP_EXPORT int jxlhip_upload_side_info(
    jxlhip_ctx* ctx, const uint8_t* ac_strategy, const int32_t* raw_quant,
    const uint8_t* epf_sharpness, const int8_t* ytox_map,
    const int8_t* ytob_map, const float* const dc[3],
    const float* dequant_table);
/* The frame's alpha channel for 4-channel JXLHIP_OUT_PACKED outputs: a dense host plane of xsize x ysize floats
 * (stride_floats per row; 1.0 = opaque), copied into context-owned HBM.  It is written to the output like a
 * colour channel without the transfer function -- what WriteToOutputStage does with input channel alpha_c
 * (stage_write.cc:350-366); not un-premultiplied.  Without this call (jxlhip_frame_begin resets it) alpha is the
 * opaque 1.0 the reference substitutes (:355-360).  On a multi-device context every stripe takes its own rows.
 * JXLHIP_ERR_UNSUPPORTED on an upsampled frame (jxlhip_set_upsampling). */
JXLHIP_EXPORT int jxlhip_set_alpha(jxlhip_ctx* ctx, const float* host_plane, size_t stride_floats);
/* Photon noise of the current frame (FrameHeader::kNoise, what cjxl --photon_noise_iso writes): lut = NoiseParams::lut,
 * the 8 values DecodeNoise reads (lib/jxl/dec_noise.cc:155-165; jxlhip_noise_lut_decode), and the seed indices of
 * the frame's generators, PassesDecoderState::visible_frame_index / nonvisible_frame_index (dec_cache.h:127-128) as
 * FrameDecoder sets them BEFORE decoding the frame (dec_frame.cc:160-168): a file's only frame is (1, 0).
 * jxlhip_decode_frame then renders what the reference's pipeline does between the loop filters and the XYB stage
 * (dec_cache.cc:205-210): the random planes of PrepareNoiseInput (dec_noise.cc:58-151), ConvolveNoiseStage and
 * AddNoiseStage (render_pipeline/stage_noise.cc:171-310) with the frame's base colour correlation (cfl_base_x /
 * cfl_base_b); every output kind.  A LUT with no entry above 1e-3 adds nothing (noise.h:37-42): the frame then takes
 * exactly the noise-free path.  jxlhip_frame_begin resets it (no noise); frames that never call this are untouched.
 * JXLHIP_ERR_UNSUPPORTED on a multi-device context, for a stripe and with undo_orientation > 1; the split calls
 * (jxlhip_decode_filters[_rows], jxlhip_stripe_finish) refuse a noise frame. */
JXLHIP_EXPORT int jxlhip_set_noise(jxlhip_ctx* ctx, const float lut[8], uint32_t visible_frame_index,
                                   uint32_t nonvisible_frame_index);
/* Splines of the current frame (FrameHeader::kSplines; jxlhip_splines_decode / jxlhip_splines_from_quantized,
 * jxl_hip_frame.h): computes the draw list of Splines::InitializeDrawCache (lib/jxl/splines.cc:657-758) for the
 * frame's size and base colour correlation (cfl_base_x / cfl_base_b) and uploads it into context memory; the object
 * may be destroyed when this returns.  jxlhip_decode_frame then draws the splines where the reference's pipeline has
 * its spline stage, between the loop filters and noise (dec_cache.cc:198-201; DrawSegment, splines.cc:82-127), with
 * every output kind.  NULL or a list without segments: no splines.  jxlhip_frame_begin resets it; frames that never
 * call this are untouched.  JXLHIP_ERR_BAD_STREAM where the reference's draw cache fails (jxlhip_splines_segments);
 * JXLHIP_ERR_UNSUPPORTED on a multi-device context, for a stripe and with undo_orientation > 1; the split calls refuse
 * a spline frame. */
JXLHIP_EXPORT int jxlhip_set_splines(jxlhip_ctx* ctx, const struct jxlhip_splines* splines);
/* A reference frame for patches (what a kReferenceOnly frame with save_as_reference = slot leaves in
 * PassesSharedState::reference_frames, dec_cache.h; the frame must have been saved BEFORE the colour transform, i.e. in
 * XYB): copies the three planes X, Y, B of xsize x ysize floats (stride_floats per row; host memory, or device memory of
 * the context's device when on_device != 0) into context-owned device memory.  The slot (0..3) holds until it is
 * replaced, cleared (xsize == 0 or ysize == 0; planes may then be NULL) or the context is destroyed;
 * jxlhip_frame_begin does not touch it.  Synchronises the context's stream.  Set the slots before
 * jxlhip_set_patches: the uploaded dictionary points into them, and jxlhip_decode_frame answers JXLHIP_ERR_STATE when
 * a slot was set or cleared in between.  JXLHIP_ERR_UNSUPPORTED on a multi-device context. */
JXLHIP_EXPORT int jxlhip_set_reference_frame(jxlhip_ctx* ctx, uint32_t slot, uint32_t xsize, uint32_t ysize,
                                             const float* const planes[3], size_t stride_floats, int on_device);
/* Patches of the current frame (FrameHeader::kPatches; jxlhip_patches_decode / jxlhip_patches_from_list,
 * jxl_hip_frame.h): checks the dictionary against the slots present and the frame's padded size, bins its patches by
 * tile and uploads them; the object may be destroyed when this returns.  jxlhip_decode_frame then blends the patches
 * where the reference's pipeline has its patch stage, behind the loop filters and in front of splines, upsampling and
 * noise (dec_cache.cc:193-197; PatchDictionary::AddOneRow, dec_patch_dictionary.cc:319-357, PerformBlending,
 * blending.cc:42-190), at coded size, in list order, with every output kind.  All eight colour blend modes, as on an
 * image without an alpha channel: kNone keeps the frame, kReplace / kBlendAbove / kBlendBelow take the reference
 * sample, kAdd / kAlphaWeightedAdd* add it, kMul multiplies by it (clamped to [0, 1] with the clamp flag,
 * alpha.cc:82-93).  NULL or a dictionary without patches: the frame takes exactly its plain path.
 * jxlhip_frame_begin resets it; frames that never call this are untouched.  JXLHIP_ERR_INVALID_ARGUMENT for a patch
 * whose slot is empty or smaller than its rectangle, or that leaves the padded frame (the object was made for other
 * slots or another frame); JXLHIP_ERR_UNSUPPORTED for a dictionary that uses extra channels
 * (jxlhip_patches_list), after jxlhip_set_alpha (which refuses a patch frame in turn), on a multi-device context, for
 * a stripe and with undo_orientation > 1; the split calls refuse a patch frame. */
struct jxlhip_patches;
JXLHIP_EXPORT int jxlhip_set_patches(jxlhip_ctx* ctx, const struct jxlhip_patches* patches);
/* Upsampling of the current frame (FrameHeader::upsampling = factor: 2, 4 or 8; what cjxl writes by itself from
 * distance 10 on, and with --resampling).  jxlhip_frame_begin's xsize / ysize are then the CODED size; out_xsize /
 * out_ysize is the size the frame is upsampled and cropped to (the image), with ceil(out / factor) == coded in both
 * directions, JXLHIP_ERR_INVALID_ARGUMENT otherwise.  weights = the 15 / 55 / 210 coded weights of that factor from
 * the image header's transform data (jxlhip_image_header::upsampling{2,4,8}_weights where custom_weights_mask has the
 * factor's bit), NULL = the format's defaults.  jxlhip_decode_frame then renders the reference's upsampling stage
 * (render_pipeline/stage_upsampling.cc) where its pipeline has it (dec_cache.cc:194-218): behind the loop filters and
 * the splines, which are drawn at coded size, in front of noise, which is generated at output size; `out`, its strides
 * and every output kind are those of an out_xsize x out_ysize frame.  Call it before jxlhip_set_splines (the draw list
 * is computed for the upsampled size: JXLHIP_ERR_STATE otherwise, also for a reset to factor 1 behind a draw list made
 * for an upsampled frame).  factor 1 or a new jxlhip_frame_begin resets it;
 * frames that never call this are untouched.  JXLHIP_ERR_UNSUPPORTED on a multi-device context, for a stripe, with
 * undo_orientation > 1 and after jxlhip_set_alpha (which refuses an upsampled frame in turn: extra channels of
 * upsampled frames are outside the back-end); the split calls refuse an upsampled frame. */
JXLHIP_EXPORT int jxlhip_set_upsampling(jxlhip_ctx* ctx, uint32_t factor, const float* weights, uint32_t out_xsize,
                                        uint32_t out_ysize);
/* DC-only groups of the current frame: what FrameDecoder::Flush draws for an AC group none of whose passes has arrived
 * (dec_frame.cc:737-797, dec_group.cc:730-792).  mask = one byte per AC group (num_groups of them, host memory, copied
 * by the call), non-zero = the group has no AC: its 256 x 256 pixels of the three XYB planes are its DC samples
 * upsampled 8x with the format's 25-tap upsampler (render_pipeline/stage_upsampling.cc:147-276; the 5 x 5
 * neighbourhoods read the neighbouring groups' DC and are mirrored at the edges of the DC image only) instead of the
 * inverse transforms of its coefficient slots, which the call's decode zeroes on the device when they are the
 * context's upload buffers (caller-owned coefficients, jxlhip_frame_set_inputs, are read as they are and must be
 * readable; what phase 1 makes of them is overwritten).  weights8 = the 210 coded weights of the 8x upsampler
 * (jxlhip_image_header::upsampling8_weights where custom_weights_mask has bit 2), NULL = the format's defaults.
 * A frame with a mask takes the two-phase route whatever its size; k_dc_upsample8 (JXLHIP_KERNEL_DC_UPSAMPLE) runs
 * between phase 1 and the filter launch, and as the last launch of jxlhip_decode_blocks, so that jxlhip_export_xyb shows
 * its output; Gaborish, EPF and the colour stages follow as usual.  NULL or an all-zero mask: the frame takes exactly
 * the path it takes without this call.  Call it after jxlhip_frame_begin, which resets it.
 * JXLHIP_ERR_UNSUPPORTED (jxlhip_last_error names the case): a multi-device context, a stripe, and a mask together with
 * jxlhip_set_noise, _splines, _patches, _upsampling, _blending or _alpha, whichever comes second (the setters and
 * jxlhip_decode_frame check). */
JXLHIP_EXPORT int jxlhip_set_dc_only_groups(jxlhip_ctx* ctx, const uint8_t* mask, const float* weights8);
/* ---- blending: frame sequences (animations, layers, cropped frames) ----
 * The four slots of jxlhip_set_reference_frame hold one of two things each: the XYB reference frame patches copy from
 * (a frame saved BEFORE the colour transform), or a CANVAS: a frame saved AFTER the colour transform, as float RGB in
 * the output's transfer function at image size (ReferenceFrame::ib_is_in_xyb = false, dec_frame.cc:879).  Storing one
 * kind drops the other; jxlhip_set_reference_frame(slot, 0, 0, ...) clears both; jxlhip_set_patches refuses a patch
 * whose slot holds a canvas ("Patches cannot use frames saved post color transforms", dec_patch_dictionary.cc:70).
 * Canvas memory is the context's and grows as needed.
 *
 * jxlhip_set_blending: the current frame is blended over the canvas of slot `source` at its origin and / or saved
 * (FrameHeader::blending_info, frame_origin, save_as_reference; BlendingStage, render_pipeline/stage_blending.cc).
 * Call it after jxlhip_frame_begin, which resets it; NULL switches it off.  The frame that is blended is the frame's
 * own output (an upsampled frame at its upsampled size), after every render stage it has (patches, splines,
 * upsampling, noise).  With blending on, jxlhip_decode_frame / _host / _pinned take and check `out` and its stride as
 * an image_xsize x image_ysize frame; `out` may be NULL when a save slot is named (a layer nobody displays).  Per
 * canvas pixel: bg = the source canvas (0 when the slot is empty); inside the frame's rectangle clipped to the image
 * the result is PerformBlending's colour mode on an image without an alpha channel (blending.cc:150-184): kReplace and
 * kBlend fg, kAdd and kAlphaWeightedAdd bg + fg, kMul bg * fg with fg clamped to [0, 1] when `clamp` is set; outside
 * it the result is bg.  It goes to the save slot and, through the sample conversion of the output format (dither,
 * clamp, rounding, half floats, byte swap, opaque alpha), to `out`.
 * The reference blends after FromLinearStage, in the ORIGINAL's encoding; this call blends in the transfer function
 * of the caller's output format (JXLHIP_OUT_LINEAR_RGB_F32: linear).  The two agree when the caller asks for the
 * original's transfer function (jxlhip_codestream_info::transfer_function); otherwise the blend is done in another
 * encoding than the reference's.  All frames of a sequence must use the same output transfer function.
 * A full-size kReplace frame at the origin with no save slot launches exactly what it does without this call.
 * JXLHIP_ERR_UNSUPPORTED: multi-device contexts, stripes, undo_orientation > 1, JXLHIP_OUT_XYB_PLANAR, a stream that is
 * being captured into a graph (canvas and staging memory may have to grow), a frame with
 * jxlhip_set_alpha (the extra channels of a blended frame go through jxlhip_set_blending_extra; jxlhip_set_alpha
 * refuses a blended frame in turn), and the split calls on a blended frame.  JXLHIP_ERR_INVALID_ARGUMENT: a bad mode or slot, a source
 * slot that holds an XYB frame ("Trying to blend XYB reference frame"), a source canvas smaller than the image (neither
 * is looked at for a full-size kReplace frame at the origin, which never reads its source), and
 * save_slot == source with a source canvas of another size than the image. */
typedef enum jxlhip_blend_mode {  /* BlendMode, frame_header.h */
  JXLHIP_BLEND_REPLACE = 0,
  JXLHIP_BLEND_ADD = 1,
  JXLHIP_BLEND_BLEND = 2,
  JXLHIP_BLEND_ALPHA_WEIGHTED_ADD = 3,
  JXLHIP_BLEND_MUL = 4
} jxlhip_blend_mode;
#define JXLHIP_BLEND_NO_SAVE 0xFFFFFFFFu
typedef struct jxlhip_blend_params {
  uint32_t image_xsize, image_ysize; /* the canvas: W x H */
  int32_t x0, y0;                    /* FrameHeader::frame_origin */
  uint32_t mode;                     /* jxlhip_blend_mode */
  uint32_t clamp;                    /* BlendingInfo::clamp */
  uint32_t source;                   /* BlendingInfo::source: slot 0..3 */
  uint32_t save_slot;                /* slot 0..3 the blended frame is saved into, or JXLHIP_BLEND_NO_SAVE */
} jxlhip_blend_params;
JXLHIP_EXPORT int jxlhip_set_blending(jxlhip_ctx* ctx, const jxlhip_blend_params* params);
/* Reads the canvas of `slot`: device-to-device into dev_out as interleaved float RGB, stride_floats per row
 * (>= 3 * width), enqueued on the context's stream.  dev_out == NULL only reports the size.  *w = *h = 0 and nothing
 * written when the slot holds no canvas. */
JXLHIP_EXPORT int jxlhip_canvas_read(jxlhip_ctx* ctx, uint32_t slot, float* dev_out, size_t stride_floats, uint32_t* w,
                                     uint32_t* h);
/* ---- blending on an image with extra channels (alpha, depth, ...) ----
 * jxlhip_set_blending_extra: the frame named by the jxlhip_set_blending call in front of it belongs to an image with
 * 1..4 extra channels.  They are blended beside the colour and saved with it: a canvas slot then also holds one planar
 * float plane per extra channel, of the canvas's size, allocated, replaced and cleared with it (an XYB reference frame
 * stored in the slot drops them too).  Per canvas pixel inside the frame's rectangle, in the reference's order
 * (PerformBlending, blending.cc:42-190; alpha.cc:18-93): every extra channel is blended first, with its own mode,
 * alpha_channel and clamp over the plane of its own `source` slot (zeroes when that slot has none), always from the
 * alpha values of BEFORE the blend: kReplace fg, kAdd bg + fg, kMul bg * fg (fg clamped to [0, 1] with the flag), kBlend
 * PerformAlphaBlending's single-channel form (a channel that is its own alpha channel becomes
 * 1 - (1 - fa) * (1 - bga)), kAlphaWeightedAdd bg + fg * fa (its own alpha channel: bg unchanged).  Then the colour,
 * with jxlhip_blend_params' mode, clamp and source and color_alpha_channel here: kBlend and kAlphaWeightedAdd use that
 * channel's alpha (its background from that channel's own source slot), premultiplied or straight by that channel's
 * alpha_associated; a new alpha <= 0 gives black; colour kBlend also writes the new alpha into that channel, over what
 * the channel's own mode gave.  When no channel has is_alpha set, colour kBlend is fg and kAlphaWeightedAdd bg + fg, as
 * without this call.  Outside the rectangle every channel is its own background.  Every operation is float32 in the
 * reference's order, bit for bit.
 * planes[i] = extra channel i of the frame at the FRAME's own size (jxlhip_frame_begin's xsize x ysize; what
 * jxlhip_modular_extra_channel_f32 produces), host memory, stride_floats per row; they are uploaded by this call
 * (like jxlhip_set_alpha's plane).  A 4-channel packed output takes its fourth sample from the blended plane of the
 * first channel with is_alpha set (opaque without one).  jxlhip_frame_begin and every jxlhip_set_blending call reset
 * it; a frame without it behaves exactly as before.
 * JXLHIP_ERR_STATE without jxlhip_set_blending in force.  JXLHIP_ERR_INVALID_ARGUMENT: num_extra_channels outside
 * 1..4, a mode above kMul, an alpha_channel or color_alpha_channel >= num_extra_channels, a source above 3, a NULL
 * plane or a stride below the frame's width, a source slot that holds an XYB reference frame, a source canvas smaller
 * than the image (neither is looked at for a full-size frame at the origin whose colour and extra channels all
 * replace), and -- at jxlhip_decode_frame -- a save slot that is some channel's source with a canvas of another size
 * or another number of extra channels.  JXLHIP_ERR_UNSUPPORTED: whatever jxlhip_set_blending refuses, a frame with
 * jxlhip_set_alpha (neither needed nor allowed here), an upsampled frame, a frame with patches (extra channels of
 * those stay outside the back-end), and a stream that is being captured when staging memory has to grow. */
typedef struct jxlhip_blend_extra_channel {
  uint32_t is_alpha;          /* ExtraChannelInfo::type == kAlpha */
  uint32_t alpha_associated;  /* ExtraChannelInfo::alpha_associated: premultiplied */
  uint32_t mode;              /* jxlhip_blend_mode: FrameHeader::extra_channel_blending_info[i].mode */
  uint32_t alpha_channel;     /* ... .alpha_channel: index of the extra channel that is this one's alpha */
  uint32_t clamp;             /* ... .clamp */
  uint32_t source;            /* ... .source: slot 0..3 */
} jxlhip_blend_extra_channel;
typedef struct jxlhip_blend_extra_params {
  uint32_t num_extra_channels;   /* 1..4 */
  jxlhip_blend_extra_channel channel[4];
  uint32_t color_alpha_channel;  /* FrameHeader::blending_info.alpha_channel */
  const float* planes[4];        /* host planes of the frame's extra channels */
  size_t stride_floats;
} jxlhip_blend_extra_params;
JXLHIP_EXPORT int jxlhip_set_blending_extra(jxlhip_ctx* ctx, const jxlhip_blend_extra_params* params);
/* Reads plane `ec` (0..3) of the canvas of `slot` like jxlhip_canvas_read: device-to-device, stride_floats per row
 * (>= width).  *w = *h = 0 and nothing written when the slot holds no canvas or its canvas no such plane. */
JXLHIP_EXPORT int jxlhip_canvas_read_extra(jxlhip_ctx* ctx, uint32_t slot, uint32_t ec, float* dev_out, size_t stride_floats,
                                           uint32_t* w, uint32_t* h);
/* Reads the blended plane of extra channel `ec` of the current frame, at image size, after jxlhip_decode_frame with
 * jxlhip_set_blending_extra in force: device-to-device, stride_floats per row (>= image_xsize), enqueued on the
 * context's stream.  Valid until the next jxlhip_frame_begin; JXLHIP_ERR_STATE when the frame has no such plane. */
JXLHIP_EXPORT int jxlhip_frame_extra_read(jxlhip_ctx* ctx, uint32_t ec, float* dev_out, size_t stride_floats);
/* ---- tone mapping: a PQ original on a display dimmer than its mastering peak ----
 * jxlhip_set_tone_mapping: the current frame is tone-mapped from orig_intensity_target to desired_intensity_target nits
 * as the reference does behind JxlDecoderSetDesiredIntensityTarget: ToneMappingStage between the XYB stage and
 * FromLinearStage (render_pipeline/stage_tone_mapping.cc, dec_cache.cc:300-318) = the Rec.2408 tone mapper followed by
 * GamutMap with preserve_saturation 0.1 (cms/tone_mapping-inl.h).  Call it after jxlhip_frame_begin, which resets it;
 * NULL switches it off.  luminances = the Y row of the DESTINATION primaries' RGB -> XYZ matrix
 * (OutputEncodingInfo::luminances; jxlhip_output_opsin_matrix reports them); orig_transfer = the ORIGINAL's transfer
 * function (JXLHIP_TF_*).  The destination transfer function is the frame's out_format.transfer, or linear for
 * JXLHIP_OUT_LINEAR_RGB_F32.  With tone mapping on, jxlhip_decode_frame / _host / _pinned run the frame's whole path
 * (patches, splines, upsampling and noise included) into context memory as planar XYB at output size, and one more
 * launch, k_tone_map (JXLHIP_KERNEL_TONE_MAP), writes the caller's output: every format, dither, alpha.
 * When desired >= orig, or the original's transfer function is neither PQ nor HLG, the call succeeds and the frame
 * takes exactly its plain path: the reference adds no stage there.  Frames that never call this are untouched.
 * JXLHIP_ERR_UNSUPPORTED (jxlhip_last_error names the case): an HLG original (the HlgOOTF branch of the stage),
 * JXLHIP_OUT_XYB_PLANAR, multi-device contexts, stripes, undo_orientation > 1, a frame with jxlhip_set_blending (the
 * reference tone-maps behind the blend, in linear light again; jxlhip_set_blending refuses a tone-mapped frame in
 * turn), and the split calls on a tone-mapped frame.  JXLHIP_ERR_INVALID_ARGUMENT: a target that is not positive and
 * finite, non-finite luminances, an orig_transfer outside the enum. */
typedef struct jxlhip_tone_mapping {
  float orig_intensity_target;    /* ImageMetadata::tone_mapping.intensity_target, nits */
  float desired_intensity_target; /* the display's peak, nits */
  float luminances[3];            /* of the destination primaries */
  uint32_t orig_transfer;         /* JXLHIP_TF_* of the original */
} jxlhip_tone_mapping;
JXLHIP_EXPORT int jxlhip_set_tone_mapping(jxlhip_ctx* ctx, const jxlhip_tone_mapping* params);
/* Host-side check of the tone mapper's constants: what k_tone_map would get in its launch arguments for `params` and a
 * destination transfer function dest_transfer (JXLHIP_TF_*), computed as ToneMappingStage's constructor and
 * Rec2408ToneMapperBase's member initialisers do, into out[0 .. n): to_intensity_target,
 * from_desired_intensity_target, source peak, target peak, luminances[3], pq_mastering_min, pq_mastering_range,
 * inv_pq_mastering_range, min_lum, max_lum, ks, inv_one_minus_ks, normalizer, inv_target_peak, 1 - ks,
 * preserve_saturation (n <= JXLHIP_TONE_MAPPING_CONSTANTS = 18).  No device needed.  JXLHIP_ERR_INVALID_ARGUMENT as
 * jxlhip_set_tone_mapping, and for a pair the stage is not built for (an original that is not PQ, desired >= orig). */
#define JXLHIP_TONE_MAPPING_CONSTANTS 18
JXLHIP_EXPORT int jxlhip_tone_mapping_constants(const jxlhip_tone_mapping* params, uint32_t dest_transfer, float* out,
                                                size_t n);
/* Host-side check of the noise generator's jump: the state (s0_[i], s1_[i]) of the 8 lanes of
 * Xorshift128Plus(visible_frame_index, nonvisible_frame_index, x0, y0) (lib/jxl/xorshift128plus-inl.h:46-57) after
 * `fills` calls of Fill, computed as the kernel does (one jump-matrix product, then single steps) into state[2 * i],
 * state[2 * i + 1].  No device needed. */
JXLHIP_EXPORT int jxlhip_noise_rng_state(uint32_t visible_frame_index, uint32_t nonvisible_frame_index, uint32_t x0,
                                         uint32_t y0, uint64_t fills, uint64_t state[16]);
/* A pinned host plane of the current frame's size, owned by the context, for the caller to fill and hand to
 * jxlhip_set_alpha (the copy is then a true asynchronous DMA).  Valid until the next jxlhip_frame_begin of a larger
 * frame or jxlhip_destroy; the previous frame must have been synchronised before it is written again. */
JXLHIP_EXPORT int jxlhip_alpha_staging(jxlhip_ctx* ctx, float** plane, size_t* stride_floats);
/* Replaces GetBlockFromEncoder/GetBlockFromBitstream -> DequantBlock hand-off
 * (dec_group.cc:334-359,662-706): the group's quantized coefficient stream, as
 * produced by DecodeACVarBlock, ncoeffs <= 65536 elements per channel.
 * Thread-safe w.r.t. other groups; copies on a pooled stream. */
JXLHIP_EXPORT int jxlhip_submit_group(jxlhip_ctx* ctx, uint32_t group_idx,
                                      const void* const coeffs[3],
                                      size_t ncoeffs);

/* Phase 1, replaces DecodeGroupImpl's DequantBlock + TransformToPixels for
 * every group of the stripe (dec_group.cc:431-450) and ComputeSigma
 * (epf.cc:39-133).  Result: XYB planes in context memory. */
JXLHIP_EXPORT int jxlhip_decode_blocks(jxlhip_ctx* ctx);

/* Multi-GPU halo hand-off between phase 1 and 2.  Number of rows a stripe
 * needs from each neighbour = LoopFilter::Padding() (loop_filter.h:26-29):
 * the GPU-side replacement of GroupBorderAssigner / SaveBorders / LoadBorders
 * (lib/jxl/dec_group_border.cc:68-187, low_memory_render_pipeline.cc:832-934). */
JXLHIP_EXPORT int jxlhip_halo_rows(const jxlhip_ctx* ctx);
/* The XYB planes are kept block-major (8x8 tiles) in context memory, so halo
 * rows travel through dense staging buffers: dev points to 3 * halo * xsize
 * floats (channel-major, then row, then x) in device memory.
 * export which: 0 = this stripe's first `halo` rows (to send UP),
 *               1 = its last `halo` rows (to send DOWN);
 * import which: 0 = rows received from the stripe ABOVE (placed just above
 *               this stripe), 1 = rows received from BELOW.
 * Both are asynchronous on the context's stream. */
JXLHIP_EXPORT int jxlhip_halo_export(jxlhip_ctx* ctx, int which, float* dev);
JXLHIP_EXPORT int jxlhip_halo_import(jxlhip_ctx* ctx, int which,
                                     const float* dev);

/* Phase 2, replaces the render pipeline stages Gaborish/EPF0/EPF1/EPF2/XYB
 * (+ float WriteToOutput) run by RenderPipeline::InputReady ->
 * ProcessBuffers (low_memory_render_pipeline.cc:832-934) with the
 * SimpleRenderPipeline border semantics (simple_render_pipeline.cc:129-164).
 * out: device pointer; for LINEAR_RGB_F32 out_stride = bytes per row
 * (>= xsize*12), for XYB_PLANAR out_stride = floats per row and the 3 planes
 * are out_plane_stride floats apart.  Rows written: the stripe's rows only
 * (row 0 of `out` = first row of the stripe). */
JXLHIP_EXPORT int jxlhip_decode_filters(jxlhip_ctx* ctx, void* out,
                                        size_t out_stride,
                                        size_t out_plane_stride);
/* Phase 2 for the frame rows [y_begin, y_end) of the stripe only (`out` still names the stripe's first row).  What a
 * stripe with neighbours does while its halo rows travel: the rows whose filter support stays inside the stripe -- all
 * but the first / last block row -- need no halo (the reference hands a group's border rows to its neighbours without
 * waiting for them either, dec_group_border.cc:68-187; stage borders: loop_filter.h:26-29), the two boundary block
 * rows follow once jxlhip_halo_import has run.  y_begin and y_end must be multiples of 8 or the stripe's own first /
 * last row; the pixels do not depend on how the rows are cut. */
JXLHIP_EXPORT int jxlhip_decode_filters_rows(jxlhip_ctx* ctx, void* out, size_t out_stride, size_t out_plane_stride,
                                             uint32_t y_begin, uint32_t y_end);
/* One stripe step in three calls (what libjxl_amd/stripes.py enqueues per rank and frame): jxlhip_stripe_begin = phase 1
 * (jxlhip_decode_blocks) + the stripe's boundary rows into send_up / send_down (jxlhip_halo_export; NULL = no neighbour
 * on that side); the caller then posts its sends / receives and filters the interior rows with
 * jxlhip_decode_filters_rows while they travel; jxlhip_stripe_finish = the neighbours' rows installed
 * (jxlhip_halo_import) + phase 2 of the rows outside [y_interior_begin, y_interior_end) (equal: of every row).
 * Reference: the neighbour hand-off of lib/jxl/dec_group_border.cc:68-187 around the render pipeline. */
JXLHIP_EXPORT int jxlhip_stripe_begin(jxlhip_ctx* ctx, float* send_up, float* send_down);
JXLHIP_EXPORT int jxlhip_stripe_finish(jxlhip_ctx* ctx, const float* recv_up, const float* recv_down, void* out,
                                       size_t out_stride, size_t out_plane_stride, uint32_t y_interior_begin,
                                       uint32_t y_interior_end);

/* Both phases (single GPU).  When the context holds the whole frame (no stripe)
 * and the stage list has at most two EPF passes this runs FUSED
 * (kernels_fused.hip): the filter kernel decodes the DCT8 varblocks of its own
 * window straight from the coefficient stream, those pixels never exist in
 * HBM, and the XYB planes afterwards hold the other strategies' pixels only --
 * jxlhip_export_xyb / jxlhip_halo_export need jxlhip_decode_blocks.
 * JXLHIP_FUSE=0 in the environment forces the two-phase path. */
JXLHIP_EXPORT int jxlhip_decode_frame(jxlhip_ctx* ctx, void* out,
                                      size_t out_stride,
                                      size_t out_plane_stride);

/* The same into HOST memory (the buffer of JxlDecoderSetImageOutBuffer,
 * lib/include/jxl/decode.h:1100-1140; ImageOutput::buffer / stride,
 * lib/jxl/dec_cache.h:70-82): decodes into a context-owned device frame, copies
 * it out with one strided device-to-host transfer and synchronises (returns
 * what jxlhip_sync would).  Strides as for jxlhip_decode_frame, in host terms. */
JXLHIP_EXPORT int jxlhip_decode_frame_host(jxlhip_ctx* ctx, void* host_out,
                                           size_t out_stride,
                                           size_t out_plane_stride);

/* The same into a context-owned PINNED host frame (grown on demand, reused by later frames, freed with the
 * context; taken from the caller's JxlMemoryManager when there is one): returns its address and row stride in
 * bytes once the pixels are there.  The source for a row consumer -- JxlDecoderSetImageOutCallback /
 * JxlDecoderSetMultithreadedImageOutCallback (lib/include/jxl/decode.h:1040-1100; how WriteToOutputStage
 * hands row runs to PixelCallback::run, lib/jxl/render_pipeline/stage_write.cc:662-700): the device-to-host
 * transfer is one DMA into pinned memory and the callbacks then read it in place.  Interleaved outputs
 * (JXLHIP_OUT_LINEAR_RGB_F32, JXLHIP_OUT_PACKED); valid until the next decode call on this context. */
JXLHIP_EXPORT int jxlhip_decode_frame_pinned(jxlhip_ctx* ctx, const void** host_frame, size_t* stride);

JXLHIP_EXPORT int jxlhip_sync(jxlhip_ctx* ctx);

/* ---- regular Modular frames (lossless files): integer planes to pixels ----
 * jxlhip_decode_modular_frame: the device stage behind jxlhip_modular_image_decode (jxl_hip_frame.h), which leaves a
 * lossless frame as three integer planes in coded channel order plus the reversible colour transforms (RCT) that are
 * still to be undone.  The call copies the planes (HOST memory; pinned memory makes the copies true DMAs) and the
 * programs into context-owned device memory on the context's stream and launches ONE kernel, k_modular_emit, which
 * does per pixel what the reference does in InvRCT (modular/transform/rct.cc:29-148) and ModularImageToDecodedRect
 * (dec_modular.cc:75-104,584-586,656-688): widen to int32; undo the pixel's group program, then the global one, each
 * last-listed first, in int32 arithmetic that wraps; v * (float)(1.0 / (2^bits_per_sample - 1)), one IEEE multiply; the
 * sample conversion of the output format.  The samples are the ORIGINAL's, encoded as the original was: no transfer
 * function is applied and out_format->transfer is not read (the whole-file calls check it against the original's,
 * jxl_hip_codestream.h).  A program is the first-listed RCT type | the second-listed type << 8; type 0 .. 41 = 7 *
 * permutation + custom, 0 is the identity.
 * output_kind: JXLHIP_OUT_LINEAR_RGB_F32 (3 floats per pixel, the samples as they are) or JXLHIP_OUT_PACKED with
 * out_format (every sample type, 3 or 4 channels with the opaque alpha, the 8-bit dither, endianness);
 * JXLHIP_OUT_XYB_PLANAR is JXLHIP_ERR_UNSUPPORTED: such a frame has no XYB form.  out / out_stride: device memory, bytes
 * per row, as jxlhip_decode_frame.  undo_orientation: as jxlhip_frame_params (0 or 1 = coded orientation; 2..8 write
 * display orientation, for 5..8 ysize pixels wide and xsize rows high).  Asynchronous like the decode calls: the planes,
 * group_rct and `out` must stay valid until jxlhip_sync.  Needs no jxlhip_frame_begin and leaves the context's frame
 * alone.  JXLHIP_ERR_INVALID_ARGUMENT: a zero size, bits_per_sample outside 1..16, a group_dim that is not 128, 256, 512
 * or 1024, a program with a type above 41, a stride below xsize, a bad output format, stride or alignment.
 * JXLHIP_ERR_UNSUPPORTED on a multi-device context. */
enum { JXLHIP_MODULAR_I16 = 0, JXLHIP_MODULAR_I32 = 1 };
#define JXLHIP_MODULAR_MAX_RCTS 2
typedef struct jxlhip_modular_frame {
  uint32_t xsize, ysize;
  const void* planes[3];      /* host: ysize rows of stride_samples samples, channel order as coded */
  size_t stride_samples;      /* >= xsize */
  uint32_t sample_type;       /* JXLHIP_MODULAR_I16 / JXLHIP_MODULAR_I32 */
  uint32_t bits_per_sample;   /* of the image: 1..16 */
  uint32_t group_dim;         /* 128 << FrameHeader::group_size_shift */
  const uint16_t* group_rct;  /* host: ceil(xsize / group_dim) * ceil(ysize / group_dim) programs, raster order; NULL = all 0 */
  uint16_t global_rct;
} jxlhip_modular_frame;
JXLHIP_EXPORT int jxlhip_decode_modular_frame(jxlhip_ctx* ctx, const jxlhip_modular_frame* frame, uint32_t output_kind,
                                              const jxlhip_output_format* out_format, void* out, size_t out_stride,
                                              uint32_t undo_orientation);
/* jxlhip_decode_modular_channels: the same stage for what jxlhip_modular_image_decode_channels (jxl_hip_frame.h) leaves
 * of an image with an alpha channel and / or a grey image.  jxlhip_decode_modular_frame is this call with num_color = 3
 * and no alpha plane, and that case -- also three colour planes whose alpha cannot reach the output -- is launched as
 * k_modular_emit exactly as before; everything else is the sibling kernel k_modular_planes:
 *   alpha_plane: a fourth integer plane, same rows and sample type as the colour (uploaded as integers: half or a quarter
 *     of a float plane), converted in the kernel with ITS factor, (float)(1.0 / (2^alpha_bits - 1)) -- alpha_bits need
 *     not be bits_per_sample --, and written as the fourth channel of a 4-channel JXLHIP_OUT_PACKED output like a colour
 *     channel, minus the transfer function (stage_write.cc:350-366); never un-premultiplied.  Every other output (three
 *     floats, 3 channels) has no room for it: the plane is neither uploaded nor read.  NULL: the opaque value.
 *   num_color = 1: a grey image -- planes[0] alone, no RCT (a non-zero program is JXLHIP_ERR_INVALID_ARGUMENT), the
 *     sample written to R, G and B, as the reference's pipeline carries a grey image.
 * Everything else as jxlhip_decode_modular_frame.  JXLHIP_ERR_INVALID_ARGUMENT also for num_color outside {1, 3} and
 * alpha_bits outside 1..16 with an alpha plane. */
typedef struct jxlhip_modular_channels {
  uint32_t xsize, ysize;
  uint32_t num_color;         /* 3, or 1 (grey) */
  const void* planes[3];      /* host; planes[1], planes[2] not read when num_color == 1 */
  const void* alpha_plane;    /* host, NULL = none */
  uint32_t alpha_bits;        /* of the alpha channel: 1..16 */
  size_t stride_samples;      /* of every plane, >= xsize */
  uint32_t sample_type;       /* of every plane */
  uint32_t bits_per_sample;   /* of the colour: 1..16 */
  uint32_t group_dim;
  const uint16_t* group_rct;
  uint16_t global_rct;
} jxlhip_modular_channels;
JXLHIP_EXPORT int jxlhip_decode_modular_channels(jxlhip_ctx* ctx, const jxlhip_modular_channels* frame, uint32_t output_kind,
                                                 const jxlhip_output_format* out_format, void* out, size_t out_stride,
                                                 uint32_t undo_orientation);

/* Debug/test taps on context-owned intermediates (device pointers).
 * export_xyb: row-major copy of the phase-1 result, rows [first row of the
 * stripe, + its block-padded height) x xsize_blocks*8 columns, row stride
 * dst_stride floats. */
JXLHIP_EXPORT int jxlhip_export_xyb(jxlhip_ctx* ctx, float* const dst[3],
                                    size_t dst_stride);
JXLHIP_EXPORT int jxlhip_get_sigma(jxlhip_ctx* ctx, float** inv_sigma,
                                   size_t* row_stride);

/* Per-kernel timing with HIP events on the launch stream.  enable!=0 starts
 * recording around every launch of subsequent decode calls;
 * jxlhip_profile_read syncs and returns accumulated milliseconds and launch
 * counts per kernel slot (see JXLHIP_KERNEL_*), then resets. */
enum {
  JXLHIP_KERNEL_PREPARE = 0,  /* block-offset scan, work lists, sigma: once per hand-over of side info; the span of a
                                 decode that reuses them is marked all the same and reads about 0 */
  JXLHIP_KERNEL_BLOCKS = 1,   /* dequant+CfL+LLF+inverse transforms: one launch
                                 per strategy class, overlapped on several
                                 streams; the span covers all of them */
  JXLHIP_KERNEL_FILTERS = 2,  /* Gaborish/EPF/XYB->RGB row march reading the planes (k_filters_fast / k_filters) */
  JXLHIP_KERNEL_FUSED = 3,    /* ... fed from the coefficient stream instead (k_fused: whole frames, see
                                 jxlhip_decode_frame); a frame has a FILTERS or a FUSED span, never both */
  JXLHIP_KERNEL_EPF0 = 4,     /* epf_iters == 3: [Gaborish] + EPF0 into the second plane set (k_epf0); the EPF1 +
                                 EPF2 + output march that follows is the FILTERS span */
  JXLHIP_KERNEL_NOISE = 5,    /* photon noise (jxlhip_set_noise): k_noise_rng + k_noise_emit behind the frame's path */
  JXLHIP_KERNEL_SPLINES = 6,  /* splines (jxlhip_set_splines): k_splines behind the frame's path, in front of noise */
  JXLHIP_KERNEL_UPSAMPLE = 7, /* upsampling (jxlhip_set_upsampling): k_upsample behind the splines, in front of noise */
  JXLHIP_KERNEL_COUNT = 8,    /* the slots jxlhip_profile_read reports: FROZEN at 8, the size of its callers' arrays */
  /* WARNING: the slots from here on equal or exceed JXLHIP_KERNEL_COUNT -- never index an array of
   * JXLHIP_KERNEL_COUNT with them; size arrays with JXLHIP_KERNEL_COUNT_EX and read with jxlhip_profile_read_ex */
  JXLHIP_KERNEL_PATCHES = 8,  /* patches (jxlhip_set_patches): k_patches behind the frame's path, in front of the splines */
  JXLHIP_KERNEL_BLEND = 9,    /* blending (jxlhip_set_blending): k_blend behind the frame's whole path */
  JXLHIP_KERNEL_TONE_MAP = 10, /* tone mapping (jxlhip_set_tone_mapping): k_tone_map behind the frame's whole path */
  JXLHIP_KERNEL_BLEND_EC = 11, /* blending with extra channels (jxlhip_set_blending_extra): k_ec_blend in k_blend's place */
  JXLHIP_KERNEL_DC_UPSAMPLE = 12, /* DC-only groups (jxlhip_set_dc_only_groups): k_dc_upsample8 between phase 1 and the filters */
  JXLHIP_KERNEL_COUNT_EX = 13 /* every slot; grows with each new one (new slots are appended here only) */
};
/* A hint, not a contract: `frames_in_flight` = how many contexts the caller keeps busy on this device at the same time
 * (a pool of decoders over a queue of images; 1 = this context runs alone, the default).  It only moves the frame size
 * from which jxlhip_decode_frame takes the fused kernel: alone, fusing pays from 12 Mpx (a fused wave's head / tail rows
 * against the plane traffic it saves); with several frames in flight the device is bound by HBM
 * traffic, which the fused path has less of, and it pays from 6 Mpx (4K d1.0, three in flight: 83 -> 105 Gpx/s; 1080p
 * stays two-phase: 77 vs 67).  The pixels do not depend on it beyond the rounding difference between the two paths
 * (both within the parity bar).  Nothing like it in libjxl. */
JXLHIP_EXPORT int jxlhip_set_concurrency_hint(jxlhip_ctx* ctx, int frames_in_flight);
/* Debug / test: k_prepare launches this context has enqueued (`launched`) and decode calls that saved one by reusing
 * the lists an earlier decode had used (`reused`) since it was created -- the first decode behind
 * jxlhip_upload_side_info / inside jxlhip_decode_codestream takes up the launch its hand-over enqueued and counts in
 * neither; direct calls only, launches recorded into a hipGraph count in neither.  JXLHIP_PREPARE_ONCE=0 (sampled when the context is created) turns the reuse off: every phase 1 then
 * runs its own k_prepare.  A multi-device context reports the sums over its devices. */
JXLHIP_EXPORT int jxlhip_debug_prepare_launches(const jxlhip_ctx* ctx, uint64_t* launched, uint64_t* reused);
JXLHIP_EXPORT int jxlhip_profile_enable(jxlhip_ctx* ctx, int enable);
JXLHIP_EXPORT int jxlhip_profile_read(jxlhip_ctx* ctx,
                                      float ms[JXLHIP_KERNEL_COUNT],
                                      uint32_t launches[JXLHIP_KERNEL_COUNT]);
/* The call to use from now on: the same for the first `count` slots, count <= JXLHIP_KERNEL_COUNT_EX of the library
 * at hand (JXLHIP_ERR_INVALID_ARGUMENT beyond it).  The caller says how large its arrays are, so later slots need no
 * further variant of this call; jxlhip_profile_read stays as jxlhip_profile_read_ex(..., 8) for compiled callers. */
JXLHIP_EXPORT int jxlhip_profile_read_ex(jxlhip_ctx* ctx, float* ms, uint32_t* launches, uint32_t count);

/* ---- device-side helpers for rows of SURVEY 8(a) outside the two phases -- */
/* a5: DequantMatrices (quant_weights.h:350-428).  One parameter set per
 * quant table (17 of them, QuantTable order: DCT, IDENTITY, DCT2X2, DCT4X4,
 * DCT16X16, DCT32X32, DCT8X16, DCT8X32, DCT16X32, DCT4X8, AFV0, DCT64X64,
 * DCT32X64, DCT128X128, DCT64X128, DCT256X256, DCT128X256) mirroring
 * QuantEncodingInternal (quant_weights.h:57-187) with the values as the
 * decoder holds them (i.e. after Decode's *64 scalings, quant_weights.cc:373-
 * 470).  jxlhip_dequant_encodings_decode (jxl_hip_entropy.h) fills it from the
 * AC-global section. */
typedef enum {
  JXLHIP_QUANT_LIBRARY = 0, /* the default parameters of the table's kind */
  JXLHIP_QUANT_ID = 1,      /* weights[c][0..2] */
  JXLHIP_QUANT_DCT2 = 2,    /* weights[c][0..5] */
  JXLHIP_QUANT_DCT4 = 3,    /* weights[c][0..1] multipliers + bands */
  JXLHIP_QUANT_DCT4X8 = 4,  /* weights[c][0] multiplier + bands */
  JXLHIP_QUANT_AFV = 5,     /* weights[c][0..8] + bands (4x8) + bands_afv_4x4 */
  JXLHIP_QUANT_DCT = 6,     /* bands */
  JXLHIP_QUANT_RAW = 7      /* modular-coded explicit table: NOT supported */
} jxlhip_quant_mode;
#define JXLHIP_NUM_QUANT_TABLES 17
#define JXLHIP_MAX_DISTANCE_BANDS 17
typedef struct jxlhip_quant_encoding {
  uint32_t mode;               /* jxlhip_quant_mode */
  uint32_t num_bands;          /* DctQuantWeightParams::num_distance_bands */
  uint32_t num_bands_afv_4x4;  /* dct_params_afv_4x4 (AFV only) */
  uint32_t reserved;
  float bands[3][JXLHIP_MAX_DISTANCE_BANDS];
  float bands_afv_4x4[3][JXLHIP_MAX_DISTANCE_BANDS];
  float weights[3][9];
} jxlhip_quant_encoding;

/* DequantMatrices::EnsureComputed (quant_weights.cc:163-358,1211-1271): fills a
 * JXLHIP_DEQUANT_TABLE_FLOATS device buffer with the dequant tables of the 17
 * encodings (NULL = all JXLHIP_QUANT_LIBRARY).  Asynchronous on the context's
 * stream like the decode calls; parameters that give a weight outside
 * [1e-8, 1e8) (the reference's "Invalid quantization table",
 * quant_weights.cc:329-339) surface as JXLHIP_ERR_BAD_STREAM from the next
 * jxlhip_sync().  JXLHIP_ERR_UNSUPPORTED for JXLHIP_QUANT_RAW. */
JXLHIP_EXPORT int jxlhip_dequant_tables(jxlhip_ctx* ctx,
                                        const jxlhip_quant_encoding* encodings,
                                        float* table_dev);
/* = jxlhip_dequant_tables(ctx, NULL, table_dev) */
JXLHIP_EXPORT int jxlhip_default_dequant_tables(jxlhip_ctx* ctx,
                                                float* table_dev);
/* a8: DequantDC + AdaptiveDCSmoothing (compressed_dc.cc:128-250), 4:4:4.
 * quant_dc[c]: int32 planes from the modular DC decode (device), dc_out[c]:
 * float planes (device), both xsize_blocks*ysize_blocks dense.
 * dc_quant = DequantMatrices::DCQuant(c) (quant_weights.h:289-299; NULL = the
 * defaults 1/4096, 1/512, 1/256); the step is inv_global_scale / quant_dc *
 * dc_quant[c] (quantizer.h:133-139) with the current frame's global_scale and
 * quant_dc.  cfl_*_dc = ColorCorrelation::YtoXRatio(ytox_dc) / YtoBRatio.
 * smooth != 0 runs AdaptiveDCSmoothing afterwards. */
JXLHIP_EXPORT int jxlhip_dequant_dc(jxlhip_ctx* ctx,
                                    const int32_t* const quant_dc[3],
                                    float* const dc_out[3],
                                    const float dc_quant[3], float cfl_x_dc,
                                    float cfl_b_dc, int smooth);
/* The same with the per-DC-group multiplier 1 / (1 << extra_precision) that
 * DecodeVarDCTDC reads in front of every DC group (dec_modular.cc:443-445) and
 * DequantDC applies to the three factors of that group's rectangle
 * (compressed_dc.cc:207-209) -- NOT to the AdaptiveDCSmoothing thresholds, which
 * use the plain factors (FinalizeDC, dec_frame.cc:344-357).  extra_precision: HOST array,
 * one byte (0..3, as jxlhip_dc_group_decode returns it) per DC group
 * (2048x2048 px) in raster order, ceil(xsize_blocks/256) per row; NULL = all 0. */
JXLHIP_EXPORT int jxlhip_dequant_dc_groups(jxlhip_ctx* ctx,
                                           const int32_t* const quant_dc[3],
                                           float* const dc_out[3],
                                           const float dc_quant[3],
                                           float cfl_x_dc, float cfl_b_dc,
                                           int smooth,
                                           const uint8_t* extra_precision);

#ifdef __cplusplus
}
#endif
#endif /* JXL_HIP_H_ */
