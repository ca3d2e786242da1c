// codestream.hip -- jxlhip_codestream_basic_info / jxlhip_decode_codestream (include/jxl_hip_codestream.h): the
// whole-file calls.  The container (codestream_plan.h), the headers, the reference frames, the display set-up, the walk
// over a sequence and the plan of a partial file; each frame's decode is frame_decode.hip (FrameDecoder,
// lib/jxl/dec_frame.cc:96-189 around it).
#include "codestream_plan.h"
#include "frame_decode.h"
#include "modular_image.h"

namespace {

// A kReferenceOnly frame (what cjxl writes in front of a frame with patches: the sheet its dictionary copies from):
// decoded on the host into h->refs[save_as_reference]; *pos moves from the first bit behind its frame header to the
// header of the next frame.
int ReadReferenceFrame(const uint8_t* cs, size_t n, const jxlhip_frame_header& fh, size_t* pos, ParsedHeaders* h) {
  if (!fh.is_modular || fh.num_toc_entries != 1) {
    h->why = fh.is_modular ? "a reference frame of more than one section" : "a reference frame coded in VarDCT";
    return JXLHIP_ERR_UNSUPPORTED;
  }
  if (fh.save_as_reference > 3) return JXLHIP_ERR_BAD_STREAM;
  uint64_t off = 0, total = 0;
  uint32_t sz = 0;
  int rc = jxlhip_toc_decode(cs, n, pos, 1, &off, &sz, &total);
  if (rc) return rc;
  const size_t base = *pos / 8;
  if (total > n - base) return JXLHIP_ERR_BAD_STREAM;
  ReferenceFrame& r = h->refs[fh.save_as_reference];
  r.xsize = r.ysize = 0;
  const size_t plane = (size_t)fh.xsize * fh.ysize;
  if (fh.xsize > fh.group_dim || fh.ysize > fh.group_dim) {
    h->why = "a Modular frame of more than one group";
    return JXLHIP_ERR_UNSUPPORTED;
  }
  r.xyb.assign(3 * plane, 0.0f);
  float* const planes[3] = {r.xyb.data(), r.xyb.data() + plane, r.xyb.data() + 2 * plane};
  size_t spos = 0;
  if ((rc = jxlhip_modular_frame_decode(cs + base + off, sz, &spos, &fh, planes, fh.xsize, &h->why))) return rc;
  r.xsize = fh.xsize;
  r.ysize = fh.ysize;
  *pos = (base + (size_t)total) * 8;
  return JXLHIP_OK;
}

// image header + the reference frames + the visible frame's header + the eligibility rules of this back-end.
// lossless: the caller takes a lossless file (an image that is not XYB encoded, in one regular Modular frame:
// h->modular); the partial call does not, and the sequence calls have a walk of their own.
int ParseHeaders(const uint8_t* cs, size_t n, ParsedHeaders* h, bool lossless) {
  size_t pos = 0;
  jxlhip_image_info info{};
  int rc = ParseImagePart(cs, n, h, &pos, &info, false, lossless);
  if (rc) return rc;
  const jxlhip_image_header& ih = h->ih;
  // any number of kReferenceOnly frames, then exactly one regular frame, the last of the file: every other sequence
  // (animation, layers, DC frames) is outside this front-end
  for (;;) {
    rc = jxlhip_frame_header_decode(cs, n, &pos, &info, &h->fh);
    if (rc) return rc;
    if (h->fh.frame_type != JXLHIP_FRAME_REFERENCE_ONLY || h->fh.is_last) break;
    if ((rc = ReadReferenceFrame(cs, n, h->fh, &pos, h))) return rc;
  }
  const jxlhip_frame_header& fh = h->fh;
  if (h->modular) {  // the frame-level cases of the lossless path, each by name (ModularImageChannelsRefusal)
    for (const ReferenceFrame& r : h->refs)
      if (r.xsize != 0) return h->why = "a lossless file with reference frames", JXLHIP_ERR_UNSUPPORTED;
    if (!fh.is_last) return h->why = "a lossless file of more than one frame", JXLHIP_ERR_UNSUPPORTED;
    if (const char* what = ModularImageChannelsRefusal(&fh)) return h->why = what, JXLHIP_ERR_UNSUPPORTED;
    if (fh.xsize != ih.xsize || fh.ysize != ih.ysize) return JXLHIP_ERR_UNSUPPORTED;
    h->frame_bit_pos = pos;
    return JXLHIP_OK;
  }
  // (patches would have to blend the extra channels as well: refused for now)
  if ((fh.flags & JXLHIP_FLAG_PATCHES) && ih.num_extra_channels != 0) {
    h->why = "patches on an image with extra channels";
    return JXLHIP_ERR_UNSUPPORTED;
  }
  // a last frame that blends over a saved frame (kAdd, kBlend, kMul, ... with blend_source naming a filled slot) is a
  // layer, not a patch frame: the reference blends it (blending.cc:23-40), this front-end would decode it as kReplace
  for (const ReferenceFrame& r : h->refs)
    if (r.xsize != 0 && fh.blend_mode != 0) {
      h->why = "a frame that blends over a reference frame";
      return JXLHIP_ERR_UNSUPPORTED;
    }
  if (fh.is_modular || fh.color_transform != JXLHIP_CT_XYB || fh.frame_type != JXLHIP_FRAME_REGULAR ||
      (fh.flags & JXLHIP_FLAG_USE_DC_FRAME) ||
      fh.chroma_mode[0] || fh.chroma_mode[1] || fh.chroma_mode[2] || fh.dc_level != 0 || fh.custom_size_or_origin ||
      !fh.is_last)
    return JXLHIP_ERR_UNSUPPORTED;
  // upsampling 2 / 4 / 8 (jxlhip_set_upsampling): the colour channels only -- an image with extra channels has them
  // downsampled along with the colour, and the back-end upsamples none
  const uint32_t ups = fh.upsampling;
  if ((ups != 1 && ups != 2 && ups != 4 && ups != 8) || (ups != 1 && ih.num_extra_channels != 0) ||
      fh.xsize != (ih.xsize + ups - 1) / ups || fh.ysize != (ih.ysize + ups - 1) / ups)
    return JXLHIP_ERR_UNSUPPORTED;
  for (uint32_t i = 0; i < ih.num_extra_channels; i++)
    if (fh.ec_upsampling[i] != 1) return JXLHIP_ERR_UNSUPPORTED;
  h->frame_bit_pos = pos;
  return JXLHIP_OK;
}

void FillInfo(const ParsedHeaders& h, bool container, jxlhip_codestream_info* info) {
  memset(info, 0, sizeof(*info));
  info->xsize = h.ih.xsize;
  info->ysize = h.ih.ysize;
  info->container = container ? 1u : 0u;
  info->orientation = h.ih.orientation;
  info->intensity_target = h.display_nits > 0.0f ? h.display_nits : h.ih.intensity_target;  // (decode.cc:2247)
  info->bits_per_sample = h.ih.bit_depth.bits_per_sample;
  info->transfer_function = h.ih.color_encoding.all_default ? 13u : h.ih.color_encoding.transfer_function;
  info->primaries = h.ih.color_encoding.all_default ? 1u : h.ih.color_encoding.primaries;
  info->white_point = h.ih.color_encoding.all_default ? 1u : h.ih.color_encoding.white_point;
  info->icc_size = (uint32_t)h.icc_size;
  info->grey = !h.ih.color_encoding.all_default && h.ih.color_encoding.color_space == JXLHIP_CS_GRAY;
  if (h.ih.color_encoding.want_icc) info->transfer_function = 8u, info->primaries = 1u, info->white_point = 1u;  // linear sRGB
  for (int i = 0; i < 3; i++) info->luminances[i] = h.luminances[i];
  info->gamma = h.ih.color_encoding.have_gamma ? (float)h.ih.color_encoding.gamma * 1e-7f : 0.0f;
  info->num_extra_channels = h.ih.num_extra_channels;
  if (h.alpha_index >= 0) {
    info->alpha_bits = h.extra[h.alpha_index].bit_depth.bits_per_sample;
    info->alpha_premultiplied = h.extra[h.alpha_index].alpha_associated;
  }
  info->upsampling = h.fh.upsampling;
  info->modular = h.modular ? 1u : 0u;
}

// jxlhip_codestream_set_display applied to the parsed headers: the matrix and luminances of the requested space, the
// header's colour encoding naming it (FillInfo then describes the output), the display's peak.  *why names a refusal.
int CheckDisplay(const jxlhip_display& d) {
  if (!(d.display_nits >= 0.0f) || !std::isfinite(d.display_nits)) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (d.primaries == JXLHIP_PRIM_CUSTOM || d.white_point == JXLHIP_WP_CUSTOM) return JXLHIP_ERR_UNSUPPORTED;
  if (d.primaries != 0 && d.primaries != JXLHIP_PRIM_SRGB && d.primaries != JXLHIP_PRIM_2100 && d.primaries != JXLHIP_PRIM_P3)
    return JXLHIP_ERR_INVALID_ARGUMENT;
  if (d.white_point != 0 && d.white_point != JXLHIP_WP_D65 && d.white_point != JXLHIP_WP_E && d.white_point != JXLHIP_WP_DCI)
    return JXLHIP_ERR_INVALID_ARGUMENT;
  return JXLHIP_OK;
}
int ApplyDisplay(const jxlhip_display& d, ParsedHeaders* h, const char** why) {
  *why = "";
  if (d.display_nits == 0.0f && d.primaries == 0 && d.white_point == 0) return JXLHIP_OK;
  // (a lossless file's samples are the original's: nothing between them and the output could take a display into account)
  if (h->modular) return *why = "a display set for a lossless (Modular) file", JXLHIP_ERR_UNSUPPORTED;
  int rc = CheckDisplay(d);
  if (rc) {
    if (rc == JXLHIP_ERR_UNSUPPORTED) *why = "custom xy as the requested output space";
    return rc;
  }
  jxlhip_color_encoding& ce = h->ih.color_encoding;
  if (ce.want_icc) return *why = "a display set for an ICC original (the reference needs a CMS there)", JXLHIP_ERR_UNSUPPORTED;
  if (!ce.all_default && ce.color_space == JXLHIP_CS_GRAY) return *why = "a display set for a grey original", JXLHIP_ERR_UNSUPPORTED;
  if (ce.all_default) {  // spell the defaults out: sRGB, D65, relative intent
    ce.all_default = 0;
    ce.color_space = JXLHIP_CS_RGB;
    ce.white_point = JXLHIP_WP_D65;
    ce.primaries = JXLHIP_PRIM_SRGB;
    ce.have_gamma = 0;
    ce.transfer_function = 13;
    ce.rendering_intent = 1;
  }
  if (d.display_nits > 0.0f && !ce.have_gamma && ce.transfer_function == 18)
    return *why = "display_nits set for an HLG original (the HlgOOTF branch is not in the back-end)", JXLHIP_ERR_UNSUPPORTED;
  if (d.primaries != 0 || d.white_point != 0) {
    if (d.primaries) ce.primaries = d.primaries;
    if (d.white_point) ce.white_point = d.white_point;
    if ((rc = jxlhip_output_opsin_matrix(&h->ih, h->inv_matrix, h->luminances))) return rc;
  }
  h->display_nits = d.display_nits;
  return JXLHIP_OK;
}
int ApplyDisplay(jxlhip_ctx* c, ParsedHeaders* h) {
  const jxlhip_display d{c->display_nits, c->display_primaries, c->display_white_point};
  const char* why = "";
  const int rc = ApplyDisplay(d, h, &why);
  return rc ? Fail(c, rc, "%s", why[0] ? why : "the display cannot be applied to this image") : JXLHIP_OK;
}

}  // namespace

int jxlhip_codestream_basic_info(const uint8_t* data, size_t size, jxlhip_codestream_info* info) {
  if (!data || !info) return JXLHIP_ERR_INVALID_ARGUMENT;
  CodestreamBytes b;
  int rc = b.Open(data, size);
  if (rc) return rc;
  ParsedHeaders h;
  try {
    if ((rc = ParseHeaders(b.cs, b.n, &h, true))) return rc;
  } catch (const std::bad_alloc&) {
    return JXLHIP_ERR_OUT_OF_MEMORY;
  }
  FillInfo(h, b.container, info);
  return JXLHIP_OK;
}

int jxlhip_codestream_set_display(jxlhip_ctx* c, const jxlhip_display* d) {
  if (!c) return JXLHIP_ERR_INVALID_ARGUMENT;
  JXLHIP_NO_MULTI(c);
  if (d) {
    const int rc = CheckDisplay(*d);
    if (rc == JXLHIP_ERR_UNSUPPORTED) return Fail(c, rc, "custom xy as the requested output space");
    if (rc) return Fail(c, rc, "display: %g nits, primaries %u, white point %u", d->display_nits, d->primaries, d->white_point);
  }
  c->display_nits = d ? d->display_nits : 0.0f;
  c->display_primaries = d ? d->primaries : 0;
  c->display_white_point = d ? d->white_point : 0;
  return JXLHIP_OK;
}

namespace {
void FillSequenceInfo(Sequence& s, bool container, jxlhip_codestream_info* info, jxlhip_sequence_info* seq);
}

int jxlhip_codestream_display_info(const uint8_t* data, size_t size, const jxlhip_display* display, jxlhip_codestream_info* info,
                                   const char** why_out) {
  const char* why = "";
  if (why_out) *why_out = why;
  if (!data || !info) return JXLHIP_ERR_INVALID_ARGUMENT;
  CodestreamBytes b;
  int rc = b.Open(data, size);
  if (rc) return rc;
  // a single-frame file as jxlhip_codestream_basic_info reads it; what that refuses, as the walk of the sequence calls does
  try {
    ParsedHeaders h;
    Sequence s;
    rc = ParseHeaders(b.cs, b.n, &h, true);
    const bool sequence = rc == JXLHIP_ERR_UNSUPPORTED;
    if (sequence && (rc = WalkSequence(b.cs, b.n, &s)) == JXLHIP_ERR_UNSUPPORTED) why = s.h.why;
    if (!rc && display) rc = ApplyDisplay(*display, sequence ? &s.h : &h, &why);
    if (rc) {
      if (why_out) *why_out = why;
      return rc;
    }
    if (sequence) FillSequenceInfo(s, b.container, info, nullptr);
    else FillInfo(h, b.container, info);
  } catch (const std::bad_alloc&) {
    return JXLHIP_ERR_OUT_OF_MEMORY;
  }
  return JXLHIP_OK;
}

int jxlhip_codestream_icc_profile(const uint8_t* data, size_t size, uint8_t* icc, size_t icc_capacity, size_t* icc_size) {
  if (!data || !icc_size || (icc_capacity && !icc)) return JXLHIP_ERR_INVALID_ARGUMENT;
  *icc_size = 0;
  try {
    CodestreamBytes b;
    size_t pos = 0;
    int rc = b.Open(data, size);
    if (rc) return rc;
    jxlhip_image_header ih;
    if ((rc = jxlhip_image_header_decode(b.cs, b.n, &pos, nullptr, 0, &ih))) return rc;
    if (!ih.color_encoding.want_icc) return JXLHIP_OK;
    return jxlhip_icc_decode(b.cs, b.n, &pos, icc_capacity ? icc : nullptr, icc_capacity, icc_size);
  } catch (const std::bad_alloc&) {
    return JXLHIP_ERR_OUT_OF_MEMORY;
  }
}

int jxlhip_codestream_phase_ms(const jxlhip_ctx* c, double* ms) {
  if (!c || !ms) return JXLHIP_ERR_INVALID_ARGUMENT;
  for (int i = 0; i < JXLHIP_CODESTREAM_PHASES; i++) ms[i] = c->cs_phase_ms[i];
  return JXLHIP_OK;
}

namespace {

// ---- what the three decoding entry points (a file's one frame, the next frame of a sequence, a partial file) share

// The header-controlled sizes of a frame drive host allocations (side info of up to 2^22 groups): an allocation failure
// must come back as a status, not as an exception through the C boundary (the reference returns an error too).
template <class Impl>
int GuardedDecode(jxlhip_ctx* c, Impl impl) {
  try {
    const int rc = impl();
    // an early return may leave uploads of a frame queued: nothing of it may still be in flight when the caller frees
    // its buffers
    if (rc != JXLHIP_OK && c && !c->multi && c->stream) (void)hipStreamSynchronize(c->stream);
    return rc;
  } catch (const std::bad_alloc&) {
    return c ? Fail(c, JXLHIP_ERR_OUT_OF_MEMORY, "host allocation failed while decoding the codestream") : JXLHIP_ERR_OUT_OF_MEMORY;
  }
}

struct DecodeCall {
  FrameCall fc;  // (Check: the part that is the same for every frame of every entry point)
  PhaseClock clock;
  bool verbose = false;
  // The flag bits off output_kind (`flags`: the ones the call `func` takes), the argument check, no multi-device context
  int Check(jxlhip_ctx* c, const char* func, const void* data, uint32_t flags, jxlhip_parallel_runner runner, void* runner_opaque,
            uint32_t output_kind, const jxlhip_output_format* out_format, void* out, size_t out_stride, size_t out_plane_stride) {
    const uint32_t kind = output_kind & ~flags;
    if (!c || !data || !out || kind > JXLHIP_OUT_PACKED || (kind == JXLHIP_OUT_PACKED && !out_format)) return JXLHIP_ERR_INVALID_ARGUMENT;
    if (c->multi) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "%s is not available on a multi-device context", func);  // (JXLHIP_NO_MULTI)
    fc.runner = runner;
    fc.runner_opaque = runner_opaque;
    fc.output_kind = kind;
    fc.undo_orientation = (output_kind & JXLHIP_OUT_UNDO_ORIENTATION) != 0;
    fc.out_format = out_format;
    fc.out = out;
    fc.out_stride = out_stride;
    fc.out_plane_stride = out_plane_stride;
    return JXLHIP_OK;
  }
  // clear_slots: one file's reference frames never reach the next.  The phase clock and the verbose switch.
  int Begin(jxlhip_ctx* c, bool clear_slots) {
    for (uint32_t slot = 0; clear_slots && slot < 4; slot++) {
      const int cleared = jxlhip_set_reference_frame(c, slot, 0, 0, nullptr, 0, 0);
      if (cleared) return cleared;
    }
    clock.Start(c->cs_phase_ms);
    verbose = jxlhip_env::Get().codestream_verbose.load(std::memory_order_relaxed);
    g_upload_wait_on.store(verbose);
    return JXLHIP_OK;
  }
};

// a decoded kReferenceOnly frame into its slot of the context
int SetReferenceSlot(jxlhip_ctx* c, uint32_t slot, const ReferenceFrame& r) {
  const size_t plane = (size_t)r.xsize * r.ysize;
  const float* const planes[3] = {r.xyb.data(), r.xyb.data() + plane, r.xyb.data() + 2 * plane};
  return jxlhip_set_reference_frame(c, slot, r.xsize, r.ysize, planes, r.xsize, 0);
}

int DecodeCodestreamImpl(jxlhip_ctx* c, jxlhip_parallel_runner runner, void* runner_opaque, const uint8_t* data,
                         size_t size, uint32_t output_kind, const jxlhip_output_format* out_format, void* out,
                         size_t out_stride, size_t out_plane_stride, float* const* extra_planes,
                         uint32_t num_extra_planes, size_t extra_stride, jxlhip_codestream_info* info_out) {
  DecodeCall call;
  int rc = call.Check(c, __func__, data, JXLHIP_OUT_UNDO_ORIENTATION, runner, runner_opaque, output_kind, out_format, out, out_stride, out_plane_stride);
  if (rc || (rc = call.Begin(c, true))) return rc;
  CodestreamBytes b;
  if ((rc = b.Open(data, size))) return Fail(c, rc, "not a JPEG XL codestream or container");
  ParsedHeaders h;
  if ((rc = ParseHeaders(b.cs, b.n, &h, true)))
    return Fail(c, rc, rc == JXLHIP_ERR_UNSUPPORTED ? (h.why[0] ? h.why : "stream uses features outside the VarDCT back-end") : "invalid headers");
  if ((rc = ApplyDisplay(c, &h))) return rc;
  FrameCall& fc = call.fc;
  fc.extra_planes = extra_planes;
  fc.num_extra_planes = num_extra_planes;
  fc.extra_stride = extra_stride;
  if (h.modular) {  // a lossless file: a stage path of its own (frame_decode.hip)
    jxlhip_codestream_info info;
    FillInfo(h, b.container, &info);
    if ((rc = DecodeModularFrameAt(c, b.cs, b.n, h, fc, call.clock, &info))) return rc;
    if (info_out) *info_out = info;
    return JXLHIP_OK;
  }
  for (uint32_t slot = 0; slot < 4; slot++)
    if (h.refs[slot].xsize != 0 && (rc = SetReferenceSlot(c, slot, h.refs[slot]))) return rc;
  jxlhip_codestream_info info;
  FillInfo(h, b.container, &info);
  fc.out_xsize = h.ih.xsize;
  fc.out_ysize = h.ih.ysize;
  if ((rc = DecodeFrameAt(c, b.cs, b.n, h, h.fh, h.frame_bit_pos, fc, call.clock, call.verbose, &info, nullptr))) return rc;
  if (info_out) *info_out = info;
  return JXLHIP_OK;
}

}  // namespace

int jxlhip_decode_codestream(jxlhip_ctx* c, jxlhip_parallel_runner runner, void* runner_opaque, const uint8_t* data,
                             size_t size, uint32_t output_kind, const jxlhip_output_format* out_format, void* out,
                             size_t out_stride, size_t out_plane_stride, jxlhip_codestream_info* info_out) {
  return jxlhip_decode_codestream_extra(c, runner, runner_opaque, data, size, output_kind, out_format, out, out_stride,
                                        out_plane_stride, nullptr, 0, 0, info_out);
}
int jxlhip_decode_codestream_extra(jxlhip_ctx* c, jxlhip_parallel_runner runner, void* runner_opaque, const uint8_t* data,
                                   size_t size, uint32_t output_kind, const jxlhip_output_format* out_format, void* out,
                                   size_t out_stride, size_t out_plane_stride, float* const* extra_planes,
                                   uint32_t num_extra_planes, size_t extra_stride, jxlhip_codestream_info* info_out) {
  if (num_extra_planes && !extra_planes) return JXLHIP_ERR_INVALID_ARGUMENT;
  return GuardedDecode(c, [&] {
    return DecodeCodestreamImpl(c, runner, runner_opaque, data, size, output_kind, out_format, out, out_stride, out_plane_stride,
                                extra_planes, num_extra_planes, extra_stride, info_out);
  });
}

// ---- sequences of frames (jxlhip_codestream_sequence_info, jxlhip_decode_codestream_next) -----------------------------

namespace {

void FillSequenceInfo(Sequence& s, bool container, jxlhip_codestream_info* info, jxlhip_sequence_info* seq) {
  ParsedHeaders& h = s.h;
  for (const SeqFrame& f : s.frames)
    if (f.displayed) {
      h.fh = f.fh;
      break;
    }
  FillInfo(h, container, info);
  if (!seq) return;
  memset(seq, 0, sizeof(*seq));
  seq->have_animation = h.ih.have_animation;
  if (h.ih.have_animation) {
    seq->tps_numerator = h.ih.tps_numerator;
    seq->tps_denominator = h.ih.tps_denominator;
    seq->num_loops = h.ih.num_loops;
    seq->have_timecodes = h.ih.have_timecodes;
  }
  seq->num_coded_frames = (uint32_t)s.frames.size();
  seq->num_displayed_frames = s.displayed;
  seq->why = "";
}

int SequenceNextImpl(jxlhip_ctx* c, jxlhip_parallel_runner runner, void* runner_opaque, const uint8_t* data, size_t size,
                     uint64_t* cursor, uint32_t output_kind, const jxlhip_output_format* out_format, void* out, size_t out_stride,
                     size_t out_plane_stride, jxlhip_codestream_info* info_out, jxlhip_sequence_frame* frame_out) {
  const bool blend_extra = (output_kind & JXLHIP_OUT_BLEND_EXTRA_CHANNELS) != 0;
  if (!cursor) return JXLHIP_ERR_INVALID_ARGUMENT;
  DecodeCall call;
  int rc = call.Check(c, __func__, data, JXLHIP_OUT_UNDO_ORIENTATION | JXLHIP_OUT_BLEND_EXTRA_CHANNELS, runner, runner_opaque, output_kind,
                      out_format, out, out_stride, out_plane_stride);
  if (rc) return rc;
  if (*cursor != 0 && (!c->seq_open || *cursor != c->seq_expect)) {
    return Fail(c, JXLHIP_ERR_STATE, c->seq_open ? "cursor %llu is not the one this context expects (%llu)"
                                                 : "cursor %llu, but no sequence is open on this context (the last frame was decoded, or none was started)",
                (unsigned long long)*cursor, (unsigned long long)c->seq_expect);
  }
  const bool start = *cursor == 0;
  c->seq_open = false;  // (until this call has succeeded)
  if ((rc = call.Begin(c, start))) return rc;  // (one file's frames never reach the next)
  CodestreamBytes bytes;
  if ((rc = bytes.Open(data, size))) return Fail(c, rc, "not a JPEG XL codestream or container");
  const uint8_t* const cs = bytes.cs;
  const size_t n = bytes.n;
  Sequence s;
  if ((rc = WalkSequence(cs, n, &s, blend_extra)))
    return Fail(c, rc, rc == JXLHIP_ERR_UNSUPPORTED ? (s.h.why[0] ? s.h.why : "stream uses features outside the VarDCT back-end") : "invalid headers");
  if ((rc = ApplyDisplay(c, &s.h))) return rc;
  size_t i = 0;
  if (!start) {
    while (i < s.frames.size() && s.frames[i].header_bit / 8 != *cursor) i++;
    if (i == s.frames.size()) return Fail(c, JXLHIP_ERR_STATE, "cursor %llu is no frame of these bytes", (unsigned long long)*cursor);
  }
  jxlhip_codestream_info info;
  FillSequenceInfo(s, bytes.container, &info, nullptr);
  const uint32_t W = s.h.ih.xsize, H = s.h.ih.ysize;
  uint32_t coded = 0;
  for (;; i++) {
    SeqFrame& f = s.frames[i];
    const jxlhip_frame_header& fh = f.fh;
    coded++;
    if (fh.frame_type == JXLHIP_FRAME_REFERENCE_ONLY) {
      size_t pos = f.toc_bit;
      if ((rc = ReadReferenceFrame(cs, n, fh, &pos, &s.h)))
        return Fail(c, rc, rc == JXLHIP_ERR_UNSUPPORTED ? (s.h.why[0] ? s.h.why : "a reference frame outside the Modular front-end") : "invalid reference frame");
      if ((rc = SetReferenceSlot(c, fh.save_as_reference, s.h.refs[fh.save_as_reference]))) return rc;
      continue;
    }
    // a layer nothing reads and nobody sees leaves no trace
    if (!f.displayed && !f.save) continue;
    FrameCall fc = call.fc;
    fc.out = f.displayed ? out : nullptr;
    fc.out_xsize = fh.custom_size_or_origin ? fh.coded_xsize : W;
    fc.out_ysize = fh.custom_size_or_origin ? fh.coded_ysize : H;
    fc.noise_visible = f.visible;
    fc.noise_nonvisible = f.nonvisible;
    jxlhip_blend_params b{};
    if (f.blends || f.save) {
      b.image_xsize = W;
      b.image_ysize = H;
      b.x0 = fh.custom_size_or_origin ? fh.x0 : 0;
      b.y0 = fh.custom_size_or_origin ? fh.y0 : 0;
      b.mode = fh.blend_mode;
      b.clamp = fh.blend_clamp;
      b.source = f.blends ? fh.blend_source : 0;
      b.save_slot = f.save ? fh.save_as_reference : JXLHIP_BLEND_NO_SAVE;
      if (b.source > 3 || (f.save && fh.save_as_reference > 3)) return Fail(c, JXLHIP_ERR_BAD_STREAM, "blend source / save slot out of range");
      fc.blend = &b;
      if (s.h.display_nits > 0.0f)
        return Fail(c, JXLHIP_ERR_UNSUPPORTED, "a sequence frame that needs blending while display_nits is set (tone mapping behind a blend is not in the back-end)");
    }
    s.h.fh = fh;
    if ((rc = DecodeFrameAt(c, cs, n, s.h, fh, f.toc_bit, fc, call.clock, call.verbose, &info, nullptr))) return rc;
    if (f.displayed) break;
  }
  const SeqFrame& f = s.frames[i];
  info.upsampling = f.fh.upsampling;
  if (info_out) *info_out = info;
  if (frame_out) {
    memset(frame_out, 0, sizeof(*frame_out));
    frame_out->index = f.display_index;
    frame_out->duration = f.fh.duration;
    frame_out->timecode = f.fh.timecode;
    frame_out->is_last = f.fh.is_last;
    frame_out->name_length = f.fh.name_length;
    frame_out->have_crop = f.fh.custom_size_or_origin;
    frame_out->x0 = f.fh.custom_size_or_origin ? f.fh.x0 : 0;
    frame_out->y0 = f.fh.custom_size_or_origin ? f.fh.y0 : 0;
    frame_out->xsize = f.fh.custom_size_or_origin ? f.fh.coded_xsize : W;
    frame_out->ysize = f.fh.custom_size_or_origin ? f.fh.coded_ysize : H;
    frame_out->blend_mode = f.fh.blend_mode;
    frame_out->blend_source = f.fh.blend_source;
    frame_out->blend_clamp = f.fh.blend_clamp;
    frame_out->save_as_reference = f.fh.save_as_reference;
    frame_out->coded_frames = coded;
  }
  *cursor = f.end_bit / 8;
  c->seq_expect = *cursor;
  c->seq_open = !f.fh.is_last;
  return JXLHIP_OK;
}

}  // namespace

int jxlhip_codestream_sequence_info(const uint8_t* data, size_t size, jxlhip_codestream_info* info, jxlhip_sequence_info* seq) {
  return jxlhip_codestream_sequence_info_ex(data, size, 0, info, seq);
}

int jxlhip_codestream_sequence_info_ex(const uint8_t* data, size_t size, uint32_t flags, jxlhip_codestream_info* info,
                                       jxlhip_sequence_info* seq) {
  if (!data || !info || !seq || (flags & ~(uint32_t)JXLHIP_SEQUENCE_EXTRA_CHANNELS)) return JXLHIP_ERR_INVALID_ARGUMENT;
  try {
    CodestreamBytes b;
    int rc = b.Open(data, size);
    if (rc) return rc;
    Sequence s;
    memset(seq, 0, sizeof(*seq));
    seq->why = "";
    if ((rc = WalkSequence(b.cs, b.n, &s, (flags & JXLHIP_SEQUENCE_EXTRA_CHANNELS) != 0))) {
      if (rc == JXLHIP_ERR_UNSUPPORTED) seq->why = s.h.why[0] ? s.h.why : "stream uses features outside the VarDCT back-end";
      return rc;
    }
    FillSequenceInfo(s, b.container, info, seq);
    return JXLHIP_OK;
  } catch (const std::bad_alloc&) {
    return JXLHIP_ERR_OUT_OF_MEMORY;
  }
}

int jxlhip_decode_codestream_next(jxlhip_ctx* c, jxlhip_parallel_runner runner, void* runner_opaque, const uint8_t* data,
                                  size_t size, uint64_t* cursor, uint32_t output_kind, const jxlhip_output_format* out_format,
                                  void* out, size_t out_stride, size_t out_plane_stride, jxlhip_codestream_info* info_out,
                                  jxlhip_sequence_frame* frame_out) {
  return GuardedDecode(c, [&] {
    return SequenceNextImpl(c, runner, runner_opaque, data, size, cursor, output_kind, out_format, out, out_stride, out_plane_stride,
                            info_out, frame_out);
  });
}

// ---- partial files (jxlhip_codestream_partial_info, jxlhip_decode_codestream_partial) --------------------------------

namespace {

// Which sections of the visible frame lie completely inside the n bytes (FrameDecoder::Flush's view of the file,
// dec_frame.cc:737-797; a pass counts only behind the passes before it, :625-635).  JXLHIP_ERR_NEED_MORE_INPUT where the
// reference's flush fails: the TOC, DC global or a DC group is incomplete, or the frame has one section and is not whole.
int PlanPartial(const uint8_t* cs, size_t n, const ParsedHeaders& h, PartialPlan* plan) {
  const jxlhip_frame_header& fh = h.fh;
  if (fh.num_groups > (1u << 22) || fh.num_passes == 0 || fh.num_passes > 11) return JXLHIP_ERR_UNSUPPORTED;
  const uint32_t ng = (uint32_t)fh.num_groups, ndc = (uint32_t)fh.num_dc_groups, np = fh.num_passes;
  const uint32_t ntoc = (uint32_t)fh.num_toc_entries;
  std::vector<uint64_t> off(ntoc);
  std::vector<uint32_t> sz(ntoc);
  uint64_t total = 0;
  size_t pos = h.frame_bit_pos;
  if (jxlhip_toc_decode(cs, n, &pos, ntoc, off.data(), sz.data(), &total)) return JXLHIP_ERR_NEED_MORE_INPUT;
  const size_t base = pos / 8;
  if (base > n) return JXLHIP_ERR_NEED_MORE_INPUT;
  jxlhip_partial_info& pi = plan->info;
  memset(&pi, 0, sizeof(pi));
  pi.num_passes = np;
  pi.num_groups = ng;
  plan->passes_of.assign(ng, 0);
  if (total <= n - base) {
    pi.complete = 1;
    pi.groups_complete = ng;
    pi.have_ac_global = 1;
    pi.bytes_used = base + total;
    plan->passes_of.assign(ng, (uint8_t)np);
    return JXLHIP_OK;
  }
  if (ntoc == 1) return JXLHIP_ERR_NEED_MORE_INPUT;
  if (ntoc != 2 + ndc + (uint64_t)np * ng) return JXLHIP_ERR_BAD_STREAM;
  uint64_t used = 0;
  auto have = [&](uint32_t i) {
    const uint64_t end = base + off[i] + sz[i];
    if (end > n) return false;
    used = std::max(used, end);
    return true;
  };
  for (uint32_t i = 0; i <= ndc; i++)
    if (!have(i)) return JXLHIP_ERR_NEED_MORE_INPUT;
  pi.have_ac_global = have(1 + ndc) ? 1u : 0u;
  for (uint32_t g = 0; g < ng; g++) {
    uint32_t k = 0;
    while (pi.have_ac_global && k < np && have(2 + ndc + k * ng + g)) k++;
    plan->passes_of[g] = (uint8_t)k;
    if (k == np) pi.groups_complete++;
    else if (k) pi.groups_partial++;
    else pi.groups_dc_only++;
  }
  pi.bytes_used = used;
  return JXLHIP_OK;
}

// container, headers and the plan; *why names a refusal
int ReadPartial(const uint8_t* data, size_t size, CodestreamBytes* b, ParsedHeaders* h, PartialPlan* plan, const char** why) {
  *why = "";
  int rc = b->Open(data, size, true);
  if (rc) return rc;
  // headers that end early do not parse: which of the two it is only more bytes can tell
  rc = ParseHeaders(b->cs, b->n, h, false);
  if (rc == JXLHIP_ERR_BAD_STREAM) return JXLHIP_ERR_NEED_MORE_INPUT;
  if (rc == JXLHIP_ERR_UNSUPPORTED) *why = h->why[0] ? h->why : "stream uses features outside the VarDCT back-end";
  if (rc) return rc;
  if ((rc = PlanPartial(b->cs, b->n, *h, plan)) == JXLHIP_ERR_UNSUPPORTED) *why = "frame too large";
  return rc;
}

}  // namespace

int jxlhip_codestream_partial_info(const uint8_t* data, size_t size, jxlhip_codestream_info* info, jxlhip_partial_info* partial) {
  if (!data || !partial) return JXLHIP_ERR_INVALID_ARGUMENT;
  try {
    CodestreamBytes b;
    ParsedHeaders h;
    PartialPlan plan;
    const char* why;
    const int rc = ReadPartial(data, size, &b, &h, &plan, &why);
    if (rc) return rc;
    if (info) FillInfo(h, b.container, info);
    *partial = plan.info;
    return JXLHIP_OK;
  } catch (const std::bad_alloc&) {
    return JXLHIP_ERR_OUT_OF_MEMORY;
  }
}

static int DecodePartialImpl(jxlhip_ctx* c, jxlhip_parallel_runner runner, void* runner_opaque, const uint8_t* data, size_t size,
                             uint32_t output_kind, const jxlhip_output_format* out_format, void* out, size_t out_stride,
                             size_t out_plane_stride, jxlhip_codestream_info* info_out, jxlhip_partial_info* partial_out) {
  DecodeCall call;
  int rc = call.Check(c, __func__, data, JXLHIP_OUT_UNDO_ORIENTATION, runner, runner_opaque, output_kind, out_format, out, out_stride, out_plane_stride);
  if (rc) return rc;
  FrameCall& fc = call.fc;
  CodestreamBytes b;
  ParsedHeaders h;
  PartialPlan plan;
  const char* why;
  rc = ReadPartial(data, size, &b, &h, &plan, &why);
  if (rc == JXLHIP_ERR_NEED_MORE_INPUT) return Fail(c, rc, "the headers, the TOC, DC global or a DC group is incomplete");
  if (rc) return Fail(c, rc, "%s", why[0] ? why : "not a JPEG XL codestream or container");
  if (plan.info.complete) {  // exactly what jxlhip_decode_codestream does
    if ((rc = jxlhip_decode_codestream(c, runner, runner_opaque, data, size, output_kind, out_format, out, out_stride, out_plane_stride, info_out)))
      return rc;
    if (partial_out) *partial_out = plan.info;
    return JXLHIP_OK;
  }
  const jxlhip_frame_header& fh = h.fh;
  // FrameDecoder::Flush draws none of these on a partial frame the way the whole frame has them: named follow-ups
  if (fh.flags & JXLHIP_FLAG_NOISE) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "a partial file of a frame with noise");
  if (fh.flags & JXLHIP_FLAG_SPLINES) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "a partial file of a frame with splines");
  if (fh.flags & JXLHIP_FLAG_PATCHES) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "a partial file of a frame with patches");
  if (fh.upsampling != 1) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "a partial file of an upsampled frame");
  if (h.ih.num_extra_channels != 0 && fc.output_kind == JXLHIP_OUT_PACKED && out_format->num_channels == 4)
    return Fail(c, JXLHIP_ERR_UNSUPPORTED, "a partial file of an image with extra channels into a 4-channel output");
  if ((rc = call.Begin(c, true))) return rc;
  if ((rc = ApplyDisplay(c, &h))) return rc;
  jxlhip_codestream_info info;
  FillInfo(h, b.container, &info);
  fc.out_xsize = h.ih.xsize;
  fc.out_ysize = h.ih.ysize;
  fc.partial = &plan;
  if ((rc = DecodeFrameAt(c, b.cs, b.n, h, h.fh, h.frame_bit_pos, fc, call.clock, call.verbose, &info, nullptr))) return rc;
  if (info_out) *info_out = info;
  if (partial_out) *partial_out = plan.info;
  return JXLHIP_OK;
}

int jxlhip_decode_codestream_partial(jxlhip_ctx* c, jxlhip_parallel_runner runner, void* runner_opaque, const uint8_t* data,
                                     size_t size, uint32_t output_kind, const jxlhip_output_format* out_format, void* out,
                                     size_t out_stride, size_t out_plane_stride, jxlhip_codestream_info* info_out,
                                     jxlhip_partial_info* partial_out) {
  return GuardedDecode(c, [&] {
    return DecodePartialImpl(c, runner, runner_opaque, data, size, output_kind, out_format, out, out_stride, out_plane_stride, info_out,
                             partial_out);
  });
}
