// sequence_walk.h -- the host-only part of the codestream front-end that looks at headers and nothing else: the image
// part of a file (ParseImagePart) and the walk over every frame of it (WalkSequence: header, TOC, skip the sections, the
// refusals of the sequence calls, which frames are displayed, which must be saved, the noise counters).  No device and no
// HIP header: codestream.hip includes it, and so does tests/fuzz/fuzz_sequence.cc, which runs this very code under
// -fsanitize=address,undefined over damaged files.
#ifndef JXLHIP_SEQUENCE_WALK_H_
#define JXLHIP_SEQUENCE_WALK_H_

#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/jxl_hip_codestream.h"

namespace jxlhip {

// a kReferenceOnly frame in front of the visible one: what it leaves in its slot (ParseHeaders decodes it)
struct ReferenceFrame {
  uint32_t xsize = 0, ysize = 0;  // 0: the slot is empty
  std::vector<float> xyb;         // three dense planes
};

struct ParsedHeaders {
  jxlhip_image_header ih;
  jxlhip_frame_header fh;  // of the visible frame
  ReferenceFrame refs[4];
  const char* why = "";    // JXLHIP_ERR_UNSUPPORTED from a reference frame: which case
  size_t frame_bit_pos;  // first bit after the frame header (= the TOC)
  jxlhip_extra_channel extra[4];
  int alpha_index;       // first extra channel of type alpha, -1 = none
  float inv_matrix[9];   // inverse opsin matrix into the ORIGINAL colour space (unscaled), jxlhip_output_opsin_matrix
  float luminances[3];   // luminance weights of that space
  size_t icc_size;       // size of the original's ICC profile (0 = an enumerated colour encoding)
  float display_nits = 0.0f;  // jxlhip_codestream_set_display: the display's peak when the frames are tone-mapped to it (0: not)
  bool modular = false;  // a lossless file: the image is not XYB encoded and its one frame is a regular Modular frame
};

// the image header, the ICC profile, the extra channels' eligibility and the colour set-up; *pos_out = the first frame
// header, *info_out = what the frame headers' conditions read from the image header.  sequence: the caller walks every
// frame of the file (WalkSequence) and takes animations.  lossless: the caller takes an image that is not XYB encoded (a
// lossless file: jxlhip_codestream_basic_info, jxlhip_decode_codestream[_extra]); h->modular then says it is one, and
// the image-level cases that path refuses are named in h->why.
inline int ParseImagePart(const uint8_t* cs, size_t n, ParsedHeaders* h, size_t* pos_out, jxlhip_image_info* info_out, bool sequence,
                          bool lossless = false) {
  size_t pos = 0;
  int rc = jxlhip_image_header_decode(cs, n, &pos, h->extra, 4, &h->ih);
  if (rc) return rc;
  const jxlhip_image_header& ih = h->ih;
  h->icc_size = 0;
  if (sequence && ih.have_preview) h->why = "a preview";
  if (!ih.xyb_encoded && !lossless) return JXLHIP_ERR_UNSUPPORTED;
  h->modular = !ih.xyb_encoded;
  if (h->modular) {  // the samples are the original's integers: what the Modular path cannot turn into pixels
    auto refuse = [&](const char* why) {
      h->why = why;
      return JXLHIP_ERR_UNSUPPORTED;
    };
    const jxlhip_color_encoding& ce = ih.color_encoding;
    if (ih.have_preview) return refuse("a lossless file with a preview");
    if (ih.have_animation) return refuse("a lossless animation");
    // extra channels (alpha, depth, ...): integer planes like the colour, up to four as on the VarDCT path
    if (ih.num_extra_channels > 4) return refuse("a lossless image with more than four extra channels");
    for (uint32_t i = 0; i < ih.num_extra_channels; i++) {
      const jxlhip_extra_channel& e = h->extra[i];
      if (e.dim_shift != 0) return refuse("a lossless image with a sub-sampled extra channel");
      if (e.bit_depth.floating_point_sample || e.bit_depth.bits_per_sample == 0 || e.bit_depth.bits_per_sample > 16)
        return refuse("a lossless image with a float extra channel or one of more than 16 bits");
    }
    if (ih.bit_depth.floating_point_sample || ih.bit_depth.bits_per_sample == 0 || ih.bit_depth.bits_per_sample > 16)
      return refuse("a lossless image of float samples or more than 16 bits");
    if (ce.want_icc) return refuse("a lossless image with an ICC profile");
    if (!ce.all_default && ce.color_space != JXLHIP_CS_RGB && ce.color_space != JXLHIP_CS_GRAY) return refuse("a lossless image in a colour space other than RGB or grey");
  }
  if (ih.num_extra_channels > 4 || ih.have_preview || (ih.have_animation && !sequence)) return JXLHIP_ERR_UNSUPPORTED;
  // an ICC original: the coded profile sits between the image header and the frame; it has to be decoded to find
  // its end (jxlhip_codestream_icc_profile hands it out).  Pixels: linear sRGB, like the reference without a CMS
  if (ih.color_encoding.want_icc && (rc = jxlhip_icc_decode(cs, n, &pos, nullptr, 0, &h->icc_size))) return rc;
  // extra channels (alpha, depth, ...): full-resolution integer samples; the Modular front-end decodes them all,
  // the back-end writes the first alpha channel
  h->alpha_index = -1;
  uint8_t dim_shift[4] = {0, 0, 0, 0};
  for (uint32_t i = 0; i < ih.num_extra_channels; i++) {
    const jxlhip_extra_channel& e = h->extra[i];
    if (e.dim_shift != 0 || e.bit_depth.floating_point_sample || e.bit_depth.bits_per_sample == 0 ||
        e.bit_depth.bits_per_sample > 24)
      return JXLHIP_ERR_UNSUPPORTED;
    if (e.type == JXLHIP_EC_ALPHA && h->alpha_index < 0) h->alpha_index = (int)i;
  }
  // Colour: the pixels come out in the image's ORIGINAL colour space, like JxlDecoder's default -- the inverse opsin
  // matrix is adapted to the original's primaries / white point as OutputEncodingInfo::SetColorEncoding does
  // (dec_xyb.cc:180-249); the caller applies the original's transfer function through out_format (the info struct
  // says which).  ICC and grey originals are outside this front-end.
  if (h->modular) {  // (no XYB stage: the matrix is not used; the luminances are sRGB's, for the info struct)
    static const float kIdentity[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, kLuminances[3] = {0.2126f, 0.7152f, 0.0722f};
    memcpy(h->inv_matrix, kIdentity, sizeof(kIdentity));
    memcpy(h->luminances, kLuminances, sizeof(kLuminances));
  } else if ((rc = jxlhip_output_opsin_matrix(&ih, h->inv_matrix, h->luminances))) {
    return rc;
  }
  jxlhip_image_info info{};
  info.xsize = ih.xsize;
  info.ysize = ih.ysize;
  info.xyb_encoded = ih.xyb_encoded;
  info.num_extra_channels = ih.num_extra_channels;
  info.ec_dim_shift = dim_shift;
  info.bits_per_sample = ih.bit_depth.bits_per_sample;
  info.have_animation = ih.have_animation;  // (0 unless `sequence`)
  info.have_timecodes = ih.have_animation ? ih.have_timecodes : 0;
  info.ec_dim_shift = nullptr;  // (all 0, checked above; the array above does not outlive this call)
  *pos_out = pos;
  *info_out = info;
  return JXLHIP_OK;
}

struct SeqFrame {
  jxlhip_frame_header fh;
  size_t header_bit = 0;  // first bit of the frame header (byte-aligned)
  size_t toc_bit = 0;     // first bit behind it
  size_t end_bit = 0;     // first bit behind the frame's sections
  bool displayed = false;
  bool blends = false;    // NeedsBlending (blending.cc:23-40)
  bool save = false;      // a later frame reads its slot before the slot is overwritten
  uint32_t visible = 0, nonvisible = 0;  // the reference's counters while it decodes this frame (dec_frame.cc:160-168)
  uint32_t display_index = 0;
};

struct Sequence {
  ParsedHeaders h;
  std::vector<SeqFrame> frames;
  uint32_t displayed = 0;
};

// FrameHeader::CanBeReferenced (frame_header.h:373-379)
inline bool CanBeReferenced(const jxlhip_frame_header& fh) {
  return !fh.is_last && fh.frame_type != JXLHIP_FRAME_DC && (fh.duration == 0 || fh.save_as_reference != 0);
}

// Every frame of the file: header, TOC, skip the sections.  JXLHIP_ERR_UNSUPPORTED with s->h.why for what the sequence
// calls refuse, JXLHIP_ERR_BAD_STREAM for a file that ends inside the walk.
// blend_extra: the caller takes frames that need blending on an image with extra channels (JXLHIP_SEQUENCE_EXTRA_CHANNELS
// / JXLHIP_OUT_BLEND_EXTRA_CHANNELS); without it they are refused, as before those flags existed.
inline int WalkSequence(const uint8_t* cs, size_t n, Sequence* s, bool blend_extra = false) {
  ParsedHeaders& h = s->h;
  size_t pos = 0;
  jxlhip_image_info info{};
  int rc = ParseImagePart(cs, n, &h, &pos, &info, true);
  if (rc) return rc;
  const jxlhip_image_header& ih = h.ih;
  auto refuse = [&](const char* why) {
    h.why = why;
    return JXLHIP_ERR_UNSUPPORTED;
  };
  uint32_t visible = 0, nonvisible = 0;
  for (;;) {
    if (s->frames.size() >= (1u << 20)) return refuse("more than 2^20 coded frames");
    SeqFrame f;
    f.header_bit = pos;
    if ((rc = jxlhip_frame_header_decode(cs, n, &pos, &info, &f.fh))) return rc;
    f.toc_bit = pos;
    const jxlhip_frame_header& fh = f.fh;
    if (fh.frame_type == JXLHIP_FRAME_DC || fh.dc_level != 0) return refuse("a DC frame");
    if (fh.flags & JXLHIP_FLAG_USE_DC_FRAME) return refuse("a frame that uses a DC frame");
    if (fh.frame_type == JXLHIP_FRAME_SKIP_PROGRESSIVE) return refuse("a kSkipProgressive frame");
    if (fh.num_toc_entries == 0 || fh.num_toc_entries > (1u << 24)) return refuse("frame too large");
    if (fh.frame_type == JXLHIP_FRAME_REFERENCE_ONLY) {
      if (!fh.is_modular) return refuse("a reference frame coded in VarDCT");
      if (fh.num_toc_entries != 1) return refuse("a reference frame of more than one section");
      if (fh.xsize > fh.group_dim || fh.ysize > fh.group_dim) return refuse("a Modular frame of more than one group");
    } else {
      if (fh.is_modular) return refuse("a Modular regular frame");
      if (fh.color_transform != JXLHIP_CT_XYB || fh.chroma_mode[0] || fh.chroma_mode[1] || fh.chroma_mode[2])
        return refuse("a frame that is not XYB, or chroma-subsampled");
      if (CanBeReferenced(fh) && fh.save_before_color_transform) return refuse("a regular frame saved before the colour transform");
      if ((fh.flags & JXLHIP_FLAG_PATCHES) && ih.num_extra_channels != 0) return refuse("patches on an image with extra channels");
      const uint32_t ups = fh.upsampling;
      const uint32_t fw = fh.custom_size_or_origin ? fh.coded_xsize : ih.xsize, fhh = fh.custom_size_or_origin ? fh.coded_ysize : ih.ysize;
      if ((ups != 1 && ups != 2 && ups != 4 && ups != 8) || (ups != 1 && ih.num_extra_channels != 0) ||
          fh.xsize != (fw + ups - 1) / ups || fh.ysize != (fhh + ups - 1) / ups)
        return refuse("an upsampled frame on an image with extra channels, or an upsampling factor outside 1, 2, 4, 8");
      for (uint32_t i = 0; i < ih.num_extra_channels && i < 4; i++)
        if (fh.ec_upsampling[i] != 1) return refuse("extra channels upsampled on their own");
      f.blends = fh.custom_size_or_origin || fh.blend_mode != JXLHIP_BLEND_REPLACE || fh.ec_blend_any;  // NeedsBlending
      if (f.blends && ih.num_extra_channels != 0 && !blend_extra)
        return refuse("a frame that needs blending on an image with extra channels");
      f.displayed = fh.is_last || fh.duration > 0;
    }
    if (f.displayed) {
      visible++;
      nonvisible = 0;
      f.display_index = s->displayed++;
    } else {
      nonvisible++;
    }
    f.visible = visible;
    f.nonvisible = nonvisible;
    // the TOC, to find the end of the frame
    const uint32_t ntoc = (uint32_t)fh.num_toc_entries;
    std::vector<uint64_t> off(ntoc);
    std::vector<uint32_t> sz(ntoc);
    uint64_t total = 0;
    if ((rc = jxlhip_toc_decode(cs, n, &pos, ntoc, off.data(), sz.data(), &total))) return rc;
    const size_t base = pos / 8;
    if (total > n - base) return JXLHIP_ERR_BAD_STREAM;
    pos = (base + (size_t)total) * 8;
    f.end_bit = pos;
    s->frames.push_back(f);
    if (fh.is_last) break;
  }
  if (s->displayed == 0) return JXLHIP_ERR_BAD_STREAM;  // (is_last is a regular frame's: cannot happen)
  // which regular frames must be saved: a later frame reads the slot (it blends with that source, or carries a patch
  // dictionary, which may name any slot) before -- or while -- the slot is overwritten
  for (size_t i = 0; i < s->frames.size(); i++) {
    SeqFrame& f = s->frames[i];
    if (f.fh.frame_type != JXLHIP_FRAME_REGULAR || !CanBeReferenced(f.fh)) continue;
    const uint32_t slot = f.fh.save_as_reference;
    for (size_t j = i + 1; j < s->frames.size() && !f.save; j++) {
      const SeqFrame& g = s->frames[j];
      if (g.fh.frame_type == JXLHIP_FRAME_REGULAR && g.blends) {
        bool reads = g.fh.blend_source == slot;  // (... or an extra channel does: each has a source of its own)
        for (uint32_t e = 0; e < ih.num_extra_channels && e < 4; e++) reads = reads || g.fh.ec_blend_source[e] == slot;
        if (reads) f.save = true;
      }
      if (g.fh.frame_type == JXLHIP_FRAME_REGULAR && (g.fh.flags & JXLHIP_FLAG_PATCHES)) f.save = true;
      if (CanBeReferenced(g.fh) && g.fh.save_as_reference == slot) break;
    }
    // (A saved frame of an image with extra channels takes them into its slot: jxlhip_set_blending_extra.)
  }
  return JXLHIP_OK;
}

}  // namespace jxlhip
#endif
