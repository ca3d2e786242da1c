/* jxl_hip_codestream.h -- one call from the bytes of a .jxl file to pixels in HBM (SURVEY.md section 8, row f4:
 * the host front-end in front of the VarDCT back-end, glued).
 *
 * What FrameDecoder does for a plain VarDCT still image, with the same order of operations (libjxl tree, lib/jxl/):
 *   container boxes (jxlc / jxlp)                       decode.cc:1639-1672 (ParseBoxHeader), 1674-2020 (HandleBoxes)
 *   signature, SizeHeader, ImageMetadata, transform data decode.cc:1049-1133  -> jxlhip_image_header_decode
 *   the original's ICC profile                          decode.cc:1101-1130, icc_codec.cc -> jxlhip_icc_decode
 *   FrameHeader, TOC                                    dec_frame.cc:96-189  -> jxlhip_frame_header_decode, jxlhip_toc_decode
 *   ProcessDCGlobal                                     dec_frame.cc:268-302 -> jxlhip_dc_global_decode, jxlhip_modular_global_decode
 *   ProcessDCGroup on the pool                          dec_frame.cc:318-342, 660-680 -> jxlhip_dc_group_decode on the runner
 *   FinalizeDC (DequantDC + AdaptiveDCSmoothing)        dec_frame.cc:344-360, compressed_dc.cc:128-250 -> jxlhip_dequant_dc_groups (device)
 *   ProcessACGlobal                                     dec_frame.cc:372-416 -> jxlhip_ac_global_decode, jxlhip_dequant_tables (device)
 *   ProcessACGroup on the pool                          dec_frame.cc:455-560, 700-760 -> jxlhip_ac_groups_decode_submit
 *   ... its Modular half (extra channels) + FinalizeDecoding  dec_frame.cc:497-530, dec_modular.cc:739-760
 *                                                       -> jxlhip_modular_ac_group_decode[_f32], jxlhip_modular_finalize
 *   the render pipeline                                 dec_cache.cc:117-371 -> jxlhip_decode_frame (device)
 * Taken: any enumerated colour encoding and ICC originals (pixels then linear sRGB, like JxlDecoder without a CMS),
 * grey images, up to four full-resolution integer extra channels (alpha into a 4-channel output, all of them as host
 * planes) incl. the squeeze `cjxl -p` puts on them and palettes without deltas, progressive passes, orientation,
 * photon noise and splines (drawn on the device, jxlhip_set_noise / jxlhip_set_splines), frames upsampled 2x / 4x / 8x
 * (what cjxl writes from distance 10 on and with --resampling; upsampled on the device, jxlhip_set_upsampling, with the
 * image header's custom weights or the format's defaults) of images without extra channels, and the files cjxl writes
 * with patches at its default effort: any number of kReferenceOnly frames -- Modular, XYB, one group, decoded on the
 * host (jxlhip_modular_frame_decode) and handed to jxlhip_set_reference_frame(save_as_reference) -- in front of exactly
 * one regular last frame whose flags may include kPatches (jxlhip_patches_decode, blended on the device,
 * jxlhip_set_patches), of images without extra channels.  The four reference slots of the context are cleared at the
 * start of every call; the info struct describes the visible frame.
 * Also taken: lossless files -- an image that is NOT XYB encoded in one regular Modular frame, what `cjxl -d 0` writes
 * (info->modular = 1): 8..16-bit integer RGB or grey samples with an enumerated colour encoding, up to four extra channels
 * (alpha, depth, ...: full size, integer, at most 16 bits; info reports them as for VarDCT files; alpha_associated is
 * taken and nothing un-premultiplies), any group_size_shift, RCTs (all 42 types, global and per group), palettes without
 * deltas, LZ77.  The first alpha channel is the fourth channel of a 4-channel JXLHIP_OUT_PACKED output (uploaded as an
 * integer plane, converted by the kernel); jxlhip_decode_codestream_extra fills extra_planes with
 * v * (float)(1.0 / (2^bits - 1)) of each channel's own depth, what a VarDCT file's channels get.  Such a frame has a stage path of its own
 * (frame_decode.hip: DecodeModularFrameAt): headers; DC global = the DC dequant bit and the global Modular image; the
 * ModularDC stream of every DC group and the ModularAC stream of every group on the runner (jxlhip_modular_image_decode's
 * stages, jxl_hip_frame.h); the integer planes and RCT programs uploaded and turned into pixels by ONE kernel
 * (jxlhip_decode_modular_channels, jxl_hip.h); jxlhip_sync.  The pixels are the original's samples: out_format->transfer
 * must be the original's (info->transfer_function; JXLHIP_OUT_LINEAR_RGB_F32 wants a linear original), anything else is
 * JXLHIP_ERR_UNSUPPORTED with the reason in jxlhip_last_error -- JxlDecoder without a CMS cannot convert either --, and so
 * are JXLHIP_OUT_XYB_PLANAR and a display (jxlhip_codestream_set_display) with any field set.  jxlhip_codestream_phase_ms
 * reports HEADERS, AC_GROUPS (the host's entropy decode of every group) and KERNELS (upload, kernel, sync); the others 0.
 * A file that has not arrived completely is rendered by jxlhip_decode_codestream_partial below (groups without AC from
 * their DC, upsampled 8x on the device: jxlhip_set_dc_only_groups); the other calls refuse truncated input.
 * Animations, layers, cropped and blended frames go through jxlhip_codestream_sequence_info /
 * jxlhip_decode_codestream_next below (blended on the device, jxlhip_set_blending); the single-frame calls refuse them.
 * Everything this front-end does not decode is refused with JXLHIP_ERR_UNSUPPORTED so that the caller can hand the
 * file to libjxl's CPU decoder: of lossless files, each with a named reason: XYB or YCbCr Modular regular frames, a
 * squeeze on the colour channels (`cjxl -p`), delta palettes, float samples or more than 16 bits, ICC originals, more
 * than four extra channels, a sub-sampled extra channel (dim_shift != 0 or an upsampling factor of its own), float extra
 * channels or ones deeper than 16 bits, a colour or extra-channel blend mode other than kReplace, upsampling != 1, any
 * frame flag, a loop filter, more than one pass, chroma subsampling, previews -- and every lossless file by the sequence calls and the partial call, as before; then
 * animation / layers / any other sequence of frames (single-frame
 * calls; the sequence calls blend images with extra channels too when asked to, and refuse VarDCT
 * reference-only frames, regular frames saved before the colour transform and kSkipProgressive), previews,
 * reference frames of more than one group or with an RCT, squeeze or delta palette, patches on images with extra channels,
 * a last frame that blends (blend_mode other than kReplace) behind a reference frame,
 * chroma subsampling and YCbCr (JPEG recompression), upsampled frames of images with extra channels (alpha included:
 * cjxl downsamples them along with the colour, ec_upsampling != 1, and no stream the test oracle writes has one to
 * check against), extra channels upsampled on their own, cropped frames, DC frames, RAW dequant tables, RCT / delta
 * palettes in the extra channels' Modular streams.
 */
#ifndef JXL_HIP_CODESTREAM_H_
#define JXL_HIP_CODESTREAM_H_

#include <stddef.h>
#include <stdint.h>

#include "jxl_hip.h"
#include "jxl_hip_entropy.h"
#include "jxl_hip_frame.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct jxlhip_codestream_info {
  uint32_t xsize, ysize;       /* image size (= the frame's, after its upsampling) */
  uint32_t container;          /* the bytes were an ISOBMFF container (jxlc / jxlp boxes) */
  uint32_t orientation;        /* 1..8 (ImageMetadata::orientation); see JXLHIP_OUT_UNDO_ORIENTATION */
  float intensity_target;      /* ImageMetadata::tone_mapping.intensity_target */
  uint32_t bits_per_sample;    /* of the ORIGINAL image (metadata; the decode itself is float) */
  uint32_t transfer_function;  /* enumerated colour encoding of the original: CICP code (13 = sRGB, 8 = linear, 16 = PQ, 18 = HLG ...) */
  uint32_t primaries, white_point;
  /* filled by jxlhip_decode_codestream only */
  uint32_t num_passes, num_groups, num_dc_groups;
  uint32_t epf_iters, gab;
  uint32_t used_acs;
  uint32_t coeff_type;         /* JXLHIP_COEFF_I16, or I32 after the JXLHIP_ERR_RANGE redo */
  uint32_t modular;            /* headers: 1 = a lossless file -- the image is not XYB encoded and its one frame is a
                                  regular Modular frame.  The pixels are the original's integer samples:
                                  out_format->transfer must be the one transfer_function above names (a
                                  JXLHIP_OUT_LINEAR_RGB_F32 output wants a linear original), and epf_iters, gab,
                                  used_acs and coeff_type stay 0.  (The word was reserved, and always 0, before lossless
                                  files were taken: the struct's size and every other offset are what they were.) */
  /* headers: the image's extra channels (this front-end takes up to four, full resolution, integer samples) and the
     first one of type alpha: its bit depth (0 = the image has no alpha channel), whether it is premultiplied */
  uint32_t num_extra_channels, alpha_bits, alpha_premultiplied;
  /* headers: the pixels are produced in the image's ORIGINAL colour space (primaries / white_point above; the inverse
     opsin matrix is adapted like OutputEncodingInfo::SetColorEncoding, dec_xyb.cc:180-249).  luminances: the
     luminance weights of that space, for jxlhip_output_format::luminances (HLG OOTF); gamma: the original's gamma
     exponent when its transfer function is a gamma curve (tf_param of JXLHIP_TF_GAMMA), else 0 */
  float luminances[3];
  float gamma;
  /* headers: the original carried an ICC profile of this many bytes (0 = an enumerated colour encoding; fetch it with
     jxlhip_codestream_icc_profile).  The pixels of such an image are LINEAR sRGB (transfer_function 8, primaries /
     white_point 1), grey for a grey profile -- JxlDecoder's output when no CMS is set (dec_xyb.cc:160-164).
     grey: the original is a grey image (R = G = B in every output) */
  uint32_t icc_size, grey;
  /* headers: FrameHeader::upsampling of the frame (1, 2, 4, 8): it is coded at ceil(xsize / upsampling) x
     ceil(ysize / upsampling) and upsampled on the device (jxlhip_set_upsampling); xsize / ysize above and every
     output are the IMAGE size */
  uint32_t upsampling;
} jxlhip_codestream_info;

/* Headers only (no device needed): size and colour metadata of the first frame's image.  JXLHIP_ERR_BAD_STREAM /
 * JXLHIP_ERR_UNSUPPORTED as the decode call would return them for the header part. */
JXLHIP_EXPORT int jxlhip_codestream_basic_info(const uint8_t* data, size_t size, jxlhip_codestream_info* info);

/* ---- the display: peak luminance and output primaries ----
 * jxlhip_codestream_set_display: what JxlDecoderSetDesiredIntensityTarget and JxlDecoderSetOutputColorProfile (with an
 * enumerated encoding) do for an XYB image, sticky on the context and read by jxlhip_decode_codestream, _extra and
 * _next.  NULL resets; with nothing set every call behaves as before.
 *   display_nits            0 = no tone mapping.  Otherwise info->intensity_target reports it (decode.cc:2247) and the
 *                           frames of a PQ original brighter than it are tone-mapped (jxlhip_set_tone_mapping with the
 *                           header's intensity target); other originals and dimmer ones take their plain path.
 *   primaries, white_point  0 = the original's.  Otherwise JXLHIP_PRIM_SRGB / _2100 / _P3 and JXLHIP_WP_D65 / _E / _DCI:
 *                           the inverse opsin matrix and the luminances are re-derived for that space
 *                           (jxlhip_output_opsin_matrix on a copy of the header whose colour encoding names it, as
 *                           OutputEncodingInfo::SetColorEncoding does, dec_xyb.cc:180-249); info->primaries, white_point
 *                           and luminances then describe the output.  Host-only; works without tone mapping as well.
 * The transfer function stays the caller's (out_format).  JXLHIP_ERR_INVALID_ARGUMENT: a negative or non-finite
 * display_nits, a value outside the enums.  JXLHIP_ERR_UNSUPPORTED, from the decode call with the reason in
 * jxlhip_last_error (from jxlhip_codestream_display_info in *why): custom xy as the requested space (refused by the
 * setter itself), an ICC or a grey original with any field set, an HLG original with display_nits set, and a sequence
 * frame that needs blending while display_nits is set (a plain full-frame animation works). */
typedef struct jxlhip_display {
  float display_nits;
  uint32_t primaries;   /* JXLHIP_PRIM_*, 0 = the original's */
  uint32_t white_point; /* JXLHIP_WP_*, 0 = the original's */
} jxlhip_display;
JXLHIP_EXPORT int jxlhip_codestream_set_display(jxlhip_ctx* ctx, const jxlhip_display* display);
/* jxlhip_codestream_basic_info as the decode calls of a context with this display would report it (no device needed:
 * jxlhip_codestream_basic_info takes no context and cannot see the sticky state).  A file only the sequence calls
 * take (an animation, layers) is read as jxlhip_codestream_sequence_info reads it.  *why (may be NULL) = a static string naming the case when the call returns JXLHIP_ERR_UNSUPPORTED, else "". */
JXLHIP_EXPORT int jxlhip_codestream_display_info(const uint8_t* data, size_t size, const jxlhip_display* display,
                                                 jxlhip_codestream_info* info, const char** why);

/* The original's ICC profile (JxlDecoderGetColorAsICCProfile(JXL_COLOR_PROFILE_TARGET_ORIGINAL), decode.cc:2411-2430)
 * of a .jxl file or bare codestream.  *icc_size = its size, 0 for an image with an enumerated colour encoding;
 * icc_capacity 0 only asks for the size, a capacity below the size is JXLHIP_ERR_INVALID_ARGUMENT. */
JXLHIP_EXPORT int jxlhip_codestream_icc_profile(const uint8_t* data, size_t size, uint8_t* icc, size_t icc_capacity,
                                                size_t* icc_size);

/* Decodes the single frame -- VarDCT, or the regular Modular frame of a lossless file -- of a .jxl file or bare codestream into device memory.
 *   alpha                  : an alpha channel of the image is decoded (host, Modular) and written as the fourth
 *                            channel of a 4-channel JXLHIP_OUT_PACKED output; every other output ignores it (its bytes
 *                            are skipped), and a frame without one gives the opaque value.  Not un-premultiplied.
 *   runner / runner_opaque : a JxlParallelRunner (include/jxl/parallel_runner.h; e.g. JxlThreadParallelRunner of
 *                            libjxl_threads_hip.so) for the DC groups and the AC groups; NULL = calling thread
 *   output_kind, out_format: as jxlhip_frame_params (out_format only for JXLHIP_OUT_PACKED; NULL otherwise).
 *                            output_kind | JXLHIP_OUT_UNDO_ORIENTATION writes the pixels in DISPLAY orientation, as
 *                            JxlDecoder does by default (jxlhip_frame_params::undo_orientation = the image's
 *                            orientation: for orientations 5..8 `out` is ysize pixels wide and xsize rows high);
 *                            without the flag the pixels stay in coded orientation (JxlDecoderSetKeepOrientation)
 *   out, out_stride, out_plane_stride : as jxlhip_decode_frame (device pointer)
 * The call returns after the frame is complete (jxlhip_sync included).  The context is left with the frame's
 * inputs resident: jxlhip_decode_frame can re-render (another output format after a new jxlhip_frame_begin needs
 * the inputs again: call this function again). */
#define JXLHIP_OUT_UNDO_ORIENTATION 0x100u
/* jxlhip_decode_codestream_next only: output_kind | JXLHIP_OUT_BLEND_EXTRA_CHANNELS takes frames that need blending on an
 * image with extra channels (see "sequences of frames" below); the other decode calls ignore the bit's meaning and
 * refuse it as a bad output kind. */
#define JXLHIP_OUT_BLEND_EXTRA_CHANNELS 0x200u
JXLHIP_EXPORT int jxlhip_decode_codestream(jxlhip_ctx* ctx, jxlhip_parallel_runner runner, void* runner_opaque,
                                           const uint8_t* data, size_t size, uint32_t output_kind,
                                           const jxlhip_output_format* out_format, void* out, size_t out_stride,
                                           size_t out_plane_stride, jxlhip_codestream_info* info);

/* jxlhip_decode_codestream, and the image's extra channels (alpha, depth, spot colours ...) as float planes in HOST
 * memory -- what JxlDecoderSetExtraChannelBuffer with JXL_TYPE_FLOAT gives (decode.cc:2627; samples v / (2^bits - 1),
 * ModularImageToDecodedRect dec_modular.cc:686-737): extra_planes[e] for extra channel e < num_extra_planes (NULL = not
 * wanted; entries beyond the image's channels are ignored), rows of extra_stride floats (>= xsize), in CODED
 * orientation (JXLHIP_OUT_UNDO_ORIENTATION turns `out` only).  The planes are complete when the call returns.  An
 * alpha channel may be asked for here and ride in a 4-channel `out` at the same time. */
JXLHIP_EXPORT int jxlhip_decode_codestream_extra(jxlhip_ctx* ctx, jxlhip_parallel_runner runner, void* runner_opaque,
                                                 const uint8_t* data, size_t size, uint32_t output_kind,
                                                 const jxlhip_output_format* out_format, void* out, size_t out_stride,
                                                 size_t out_plane_stride, float* const* extra_planes,
                                                 uint32_t num_extra_planes, size_t extra_stride,
                                                 jxlhip_codestream_info* info);

/* Wall-clock milliseconds of the phases of the LAST jxlhip_decode_codestream[_extra] call on this context, ms[0 ..
 * JXLHIP_CODESTREAM_PHASES): what bench.py's `e2e` block prints beside the whole-file rate (the project's own measure is
 * the whole call: tools/djxl_main.cc:392-426, tools/speed_stats.cc:102-121). */
enum {
  JXLHIP_PHASE_HEADERS = 0,        /* container, image / frame header, TOC, DC global, the global Modular tree */
  /* With a runner, the DC groups, AC global and the AC groups are ONE runner call over num_dc_groups + 1 + num_groups
   * work units (the AC groups under a DC group start when its strategy map / quant field are in: DESIGN.md section 4;
   * JXLHIP_NO_PIPELINE=1 restores the three barriers, JXLHIP_CODESTREAM_VERBOSE=1 prints the call's timeline to stderr):
   * DC_GROUPS is then the time until the LAST DC group ended, AC_GROUPS what of the call came after it, AC_GLOBAL ~0. */
  JXLHIP_PHASE_DC_GROUPS = 1,      /* DecodeVarDCTDC + DecodeAcMetadata of every DC group, on the runner */
  JXLHIP_PHASE_AC_GLOBAL = 2,      /* block contexts, dequant encodings, histograms and coefficient orders of every pass */
  JXLHIP_PHASE_SIDE_INFO = 3,      /* frame_begin, side-info uploads, DC dequant + smoothing and dequant tables queued */
  JXLHIP_PHASE_AC_GROUPS = 4,      /* entropy decode of every AC group on the runner + the coefficient uploads queued */
  JXLHIP_PHASE_EXTRA_CHANNELS = 5, /* alpha / extra channels (Modular), 0 when none is asked for */
  JXLHIP_PHASE_KERNELS = 6,        /* jxlhip_decode_frame + jxlhip_sync: what is left of uploads and kernels */
  JXLHIP_CODESTREAM_PHASES = 7
};
JXLHIP_EXPORT int jxlhip_codestream_phase_ms(const jxlhip_ctx* ctx, double* ms);

/* ---- partial files: what a viewer shows before all of a file has arrived --------------------------------------------
 * jxlhip_decode_codestream_partial renders the picture JxlDecoderFlushImage gives for the first `size` bytes of a file
 * (FrameDecoder::Flush, dec_frame.cc:737-797).  The picture is a function of the set of COMPLETE sections alone:
 *   - a section counts only when all its bytes are inside `size`; one cut in the middle is ignored;
 *   - pass p of an AC group counts only when passes 0 .. p-1 of that group do (dec_frame.cc:625-635);
 *   - a group with k >= 1 passes is decoded from those k (jxlhip_ac_group_decode_submit_passes); a group with none --
 *     every group when the AC-global section is missing -- is drawn from its DC upsampled 8x
 *     (jxlhip_set_dc_only_groups, with the image header's upsampling8_weights when it carries custom ones);
 *   - Gaborish, EPF and the colour stages run over everything as usual; every pixel is written.
 * JXLHIP_ERR_NEED_MORE_INPUT where JxlDecoderFlushImage returns JXL_DEC_ERROR: the headers, the TOC, DC global or any
 * DC group is incomplete, and always for a frame of one section that is not complete.  A complete file takes exactly
 * the path of jxlhip_decode_codestream and gives the same bytes (info->complete = 1).  The sticky display state
 * (jxlhip_codestream_set_display) is honoured.  Arguments as jxlhip_decode_codestream.
 * JXLHIP_ERR_UNSUPPORTED with the reason in jxlhip_last_error: whatever jxlhip_decode_codestream refuses; for an
 * incomplete file also frames with noise, splines, patches or upsampling, and a 4-channel output of an image with extra
 * channels (a 3-channel output of such an image is fine: the extra channels' bytes are skipped).
 * jxlhip_decode_codestream, _extra and _next keep answering truncated input as before (JXLHIP_ERR_BAD_STREAM). */
typedef struct jxlhip_partial_info {
  uint32_t complete;        /* every section present: the call did exactly what jxlhip_decode_codestream does */
  uint32_t num_passes, num_groups;
  uint32_t groups_complete, groups_partial /* 1..num_passes-1 passes */, groups_dc_only;
  uint32_t have_ac_global;
  uint64_t bytes_used;      /* end of the last complete section that was drawn (an offset into the codestream) */
} jxlhip_partial_info;
/* Host only, no device: what the decode call below would draw from these bytes.  info may be NULL. */
JXLHIP_EXPORT int jxlhip_codestream_partial_info(const uint8_t* data, size_t size, jxlhip_codestream_info* info,
                                                 jxlhip_partial_info* partial);
JXLHIP_EXPORT int jxlhip_decode_codestream_partial(jxlhip_ctx* ctx, jxlhip_parallel_runner runner, void* runner_opaque,
                                                   const uint8_t* data, size_t size, uint32_t output_kind,
                                                   const jxlhip_output_format* out_format, void* out, size_t out_stride,
                                                   size_t out_plane_stride, jxlhip_codestream_info* info,
                                                   jxlhip_partial_info* partial);

/* ---- sequences of frames: animations, layers, cropped and blended frames --------------------------------------------
 * jxlhip_codestream_basic_info and jxlhip_decode_codestream[_extra] above keep refusing every file with more than one
 * visible frame.  The two calls below take them: they walk every frame of the file up front (header, TOC, skip the
 * sections) and decode them in order, blending on the device (jxlhip_set_blending): the canvas stays in the context's
 * slots between calls and makes no host round trip.
 * A DISPLAYED frame is what the reference's coalescing decoder reports (decode.cc:1346-1356): a regular frame with
 * is_last or duration > 0, blended over whatever its zero-duration layers and earlier frames left in its source slot.
 * Refused up front with JXLHIP_ERR_UNSUPPORTED and a named reason (jxlhip_last_error of the decode call): previews,
 * Modular regular frames (lossless files included: an image that is not XYB encoded is refused at its header), VarDCT kReferenceOnly frames, DC frames and kUseDcFrame, kSkipProgressive, regular frames
 * saved before the colour transform; on an image with extra channels a frame with patches, an upsampled frame and
 * extra channels upsampled on their own; a frame that needs blending while display_nits is set; and everything the
 * single-frame calls refuse per frame.
 * Images with extra channels (alpha, depth, ...): the caller asks for them -- JXLHIP_SEQUENCE_EXTRA_CHANNELS to
 * jxlhip_codestream_sequence_info_ex, JXLHIP_OUT_BLEND_EXTRA_CHANNELS in jxlhip_decode_codestream_next's output_kind.
 * Without the flags both calls refuse a frame that NeedsBlending on such an image ("a frame that needs blending on an
 * image with extra channels"), exactly as they did before the flags existed: the answers of the existing calls to
 * existing arguments do not change.  With them a frame that
 * NeedsBlending (blending.cc:23-40: a crop, or a blend
 * mode other than kReplace on the colour or on any extra channel) or that a later frame reads has its extra channels
 * decoded (Modular, host) and blended and saved beside the colour on the device (jxlhip_set_blending_extra): kBlend and
 * kAlphaWeightedAdd with the real alpha, straight or premultiplied (alpha_premultiplied), every extra channel with its
 * own mode and source slot.  A 4-channel packed `out` then carries the BLENDED alpha of the image's first alpha
 * channel.  A plain full kReplace frame that nothing reads takes the single-frame path (jxlhip_set_alpha). */
typedef struct jxlhip_sequence_info {
  uint32_t have_animation, tps_numerator, tps_denominator, num_loops, have_timecodes; /* AnimationHeader */
  uint32_t num_coded_frames;     /* every frame of the file, reference-only frames and layers included */
  uint32_t num_displayed_frames; /* calls of jxlhip_decode_codestream_next until is_last */
  const char* why;               /* a static string: which case, when the call returns JXLHIP_ERR_UNSUPPORTED; else "" */
} jxlhip_sequence_info;

/* Headers only (no device needed): fills *info like jxlhip_codestream_basic_info (upsampling: the first displayed
 * frame's) and *seq.  JXLHIP_ERR_BAD_STREAM for a file that ends inside the walk (a frame's sections included);
 * JXLHIP_ERR_UNSUPPORTED with seq->why naming the case (the other fields of *seq are then 0). */
JXLHIP_EXPORT int jxlhip_codestream_sequence_info(const uint8_t* data, size_t size, jxlhip_codestream_info* info,
                                                  jxlhip_sequence_info* seq);
/* The same with flags: JXLHIP_SEQUENCE_EXTRA_CHANNELS = frames that need blending on an image with extra channels are
 * taken (decode them with JXLHIP_OUT_BLEND_EXTRA_CHANNELS).  flags == 0 is jxlhip_codestream_sequence_info; any other bit
 * is JXLHIP_ERR_INVALID_ARGUMENT. */
#define JXLHIP_SEQUENCE_EXTRA_CHANNELS 1u
JXLHIP_EXPORT int jxlhip_codestream_sequence_info_ex(const uint8_t* data, size_t size, uint32_t flags,
                                                     jxlhip_codestream_info* info, jxlhip_sequence_info* seq);

typedef struct jxlhip_sequence_frame {
  uint32_t index;               /* of the displayed frame, from 0 */
  uint32_t duration, timecode;  /* AnimationFrame (ticks of tps_numerator / tps_denominator per second) */
  uint32_t is_last;
  uint32_t name_length;
  /* the displayed frame's own rectangle and blending (FrameHeader): the whole image when not cropped */
  uint32_t have_crop;
  int32_t x0, y0;
  uint32_t xsize, ysize;
  uint32_t blend_mode, blend_source, blend_clamp, save_as_reference;
  uint32_t coded_frames;        /* coded frames this call decoded (reference-only frames and layers included) */
} jxlhip_sequence_frame;

/* The next displayed frame of a file.  *cursor == 0 starts a sequence: the four slots of the context are cleared.
 * Each call decodes the coded frames from the cursor up to and including the next displayed frame -- reference-only
 * Modular frames into their slots (as jxlhip_decode_codestream), zero-duration layers blended into theirs -- writes the
 * displayed frame at IMAGE size into `out` (arguments as jxlhip_decode_codestream; blended frames refuse
 * JXLHIP_OUT_UNDO_ORIENTATION with orientations above 1 and JXLHIP_OUT_XYB_PLANAR), fills *frame and advances *cursor.
 * The context remembers the cursor it expects: any other non-zero value, and a call after the frame with is_last, is
 * JXLHIP_ERR_STATE.  Pass the same bytes to every call of a sequence.
 * A frame is saved only when a later frame of the file reads its slot before the slot is overwritten (it blends with
 * that source, colour or any extra channel, or carries a patch dictionary): cjxl gives every frame of an animation save_as_reference = 1 whether it
 * is used or not, and a plain full-frame animation takes exactly the single-frame path per frame.
 * Blending happens in the transfer function of out_format (jxlhip_set_blending): it matches the reference when that is
 * the original's (info->transfer_function).  Noise frames get the reference's seed counters (dec_frame.cc:160-168) as
 * the walk has counted them.  jxlhip_codestream_phase_ms covers the last call. */
JXLHIP_EXPORT int jxlhip_decode_codestream_next(jxlhip_ctx* ctx, jxlhip_parallel_runner runner, void* runner_opaque,
                                                const uint8_t* data, size_t size, uint64_t* cursor, uint32_t output_kind,
                                                const jxlhip_output_format* out_format, void* out, size_t out_stride,
                                                size_t out_plane_stride, jxlhip_codestream_info* info,
                                                jxlhip_sequence_frame* frame);

#ifdef __cplusplus
}
#endif
#endif /* JXL_HIP_CODESTREAM_H_ */
