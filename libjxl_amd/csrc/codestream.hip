// codestream.hip -- jxlhip_codestream_basic_info / jxlhip_decode_codestream (include/jxl_hip_codestream.h):
// the host front-end pieces (entropy.cc, modular.inc) and the device back-end glued into the order of
// operations of FrameDecoder (lib/jxl/dec_frame.cc:96-189, 268-416, 573-760) for ONE plain VarDCT still frame.
#include <functional>

#include "context.h"
#include "sequence_walk.h"

namespace {

// ---- container (decode.cc:1639-1672 ParseBoxHeader, 1674-2020 HandleBoxes): the codestream is the
// payload of the one jxlc box, or the concatenation of the jxlp payloads (4-byte big-endian index in
// front of each, bit 31 = last) in index order.  Out-of-order jxlp boxes are put in order.
// partial (jxlhip_decode_codestream_partial): the file may end anywhere -- a box cut short gives the payload that is there
// and ends the walk, and bytes that are the beginning of a signature are JXLHIP_ERR_NEED_MORE_INPUT.
int ExtractCodestream(const uint8_t* data, size_t size, std::vector<uint8_t>* storage, const uint8_t** cs,
                      size_t* cs_size, bool* container, bool partial = false) {
  static const uint8_t kSig[12] = {0, 0, 0, 0xC, 'J', 'X', 'L', ' ', 0xD, 0xA, 0x87, 0xA};
  *container = false;
  if (size >= 2 && data[0] == 0xFF && data[1] == 0x0A) {
    *cs = data;
    *cs_size = size;
    return JXLHIP_OK;
  }
  if (partial && size < 12 && (size == 0 || (size == 1 && data[0] == 0xFF) || memcmp(data, kSig, size) == 0))
    return JXLHIP_ERR_NEED_MORE_INPUT;
  if (size < 12 || memcmp(data, kSig, 12) != 0) return JXLHIP_ERR_BAD_STREAM;
  *container = true;
  struct Part {
    uint32_t index;
    const uint8_t* p;
    size_t n;
  };
  std::vector<Part> parts;
  bool have_jxlc = false, have_last = false;
  size_t pos = 0;
  bool cut = false;  // (partial) the box at hand ends behind the file
  while (pos < size && !cut) {
    if (size - pos < 8) {
      if (partial) break;
      return JXLHIP_ERR_BAD_STREAM;
    }
    uint64_t box = ((uint64_t)data[pos] << 24) | ((uint64_t)data[pos + 1] << 16) | ((uint64_t)data[pos + 2] << 8) | data[pos + 3];
    const uint8_t* type = data + pos + 4;
    size_t header = 8;
    if (box == 1) {  // 64-bit size follows
      if (size - pos < 16) {
        if (partial) break;
        return JXLHIP_ERR_BAD_STREAM;
      }
      box = 0;
      for (int i = 0; i < 8; i++) box = (box << 8) | data[pos + 8 + i];
      header = 16;
    }
    uint64_t payload;
    if (box == 0) payload = size - pos - header;  // runs to the end of the file
    else if (box < header) return JXLHIP_ERR_BAD_STREAM;
    else if (box - header > size - pos - header) {
      if (!partial) return JXLHIP_ERR_BAD_STREAM;
      payload = size - pos - header;
      cut = true;
    } else payload = box - header;
    const uint8_t* p = data + pos + header;
    if (!memcmp(type, "jxlc", 4)) {
      if (have_jxlc || !parts.empty()) return JXLHIP_ERR_BAD_STREAM;  // "there can only be one jxlc box"
      have_jxlc = true;
      parts.push_back({0u, p, (size_t)payload});
    } else if (!memcmp(type, "jxlp", 4)) {
      if (cut && payload < 4) break;
      if (have_jxlc || payload < 4) return JXLHIP_ERR_BAD_STREAM;
      const uint32_t idx = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
      if (idx & 0x80000000u) {
        if (have_last) return JXLHIP_ERR_BAD_STREAM;
        have_last = true;
      }
      parts.push_back({idx & 0x7FFFFFFFu, p + 4, (size_t)payload - 4});
    }
    // ftyp, jxll, Exif, xml, jumb, brob, jbrd ...: not pixels
    pos += header + payload;
  }
  if (parts.empty()) return partial ? JXLHIP_ERR_NEED_MORE_INPUT : JXLHIP_ERR_BAD_STREAM;
  if (parts.size() == 1 && have_jxlc) {
    *cs = parts[0].p;
    *cs_size = parts[0].n;
    return JXLHIP_OK;
  }
  std::sort(parts.begin(), parts.end(), [](const Part& a, const Part& b) { return a.index < b.index; });
  for (size_t i = 0; i < parts.size(); i++)
    if (parts[i].index != i) return JXLHIP_ERR_BAD_STREAM;  // duplicate or missing jxlp index
  size_t total = 0;
  for (const Part& q : parts) total += q.n;
  storage->resize(total);
  size_t at = 0;
  for (const Part& q : parts) {
    memcpy(storage->data() + at, q.p, q.n);
    at += q.n;
  }
  *cs = storage->data();
  *cs_size = total;
  return JXLHIP_OK;
}

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

// image header + the reference frames + the visible frame's header + the eligibility rules of this back-end
int ParseHeaders(const uint8_t* cs, size_t n, ParsedHeaders* h) {
  size_t pos = 0;
  jxlhip_image_info info{};
  int rc = ParseImagePart(cs, n, h, &pos, &info, false);
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

// The Modular parts of the AC-group sections on the runner (extra channels; FrameDecoder::ProcessACGroup's second
// half, dec_frame.cc:497-530)
struct ModularGroupsJob {
  jxlhip_modular_tree* tree;
  const jxlhip_frame_header* fh;
  uint32_t num_groups, num_passes;
  const uint8_t* const* sections;
  const size_t* sizes;
  const size_t* start_bits;
  // the samples go straight into float planes (jxlhip_modular_ac_group_decode_f32), or -- collect -- into the handle's
  // image when its transforms need every group first (jxlhip_modular_groups_are_final == 0)
  bool collect;
  uint32_t ec_bits[4], image_bits;
  float* planes[4];
  size_t strides[4];
  std::atomic<int> status{JXLHIP_OK};
};
int ModularGroupsInit(void*, size_t) { return 0; }
void ModularGroupsFunc(void* opaque, uint32_t g, size_t) {
  ModularGroupsJob* j = static_cast<ModularGroupsJob*>(opaque);
  if (j->status.load(std::memory_order_relaxed) != JXLHIP_OK) return;
  for (uint32_t p = 0; p < j->num_passes; p++) {
    const size_t i = (size_t)p * j->num_groups + g;
    size_t pos = j->start_bits[i];
    const int rc = j->collect ? jxlhip_modular_ac_group_decode(j->tree, j->fh, g, p, j->sections[i], j->sizes[i], &pos)
                              : jxlhip_modular_ac_group_decode_f32_strided(j->tree, j->fh, g, p, j->sections[i], j->sizes[i],
                                                                           &pos, j->ec_bits, j->image_bits, j->planes,
                                                                           j->strides);
    if (rc != JXLHIP_OK) {
      int expected = JXLHIP_OK;
      j->status.compare_exchange_strong(expected, rc);
      return;
    }
  }
}

// jxlhip_decode_codestream_partial: which sections of the frame are inside the bytes (PlanPartial)
struct PartialPlan {
  jxlhip_partial_info info{};
  std::vector<uint8_t> passes_of;  // per AC group: how many leading passes are complete (0 = drawn from its DC)
};

// jxlhip_decode_codestream_partial: the AC groups of an incomplete frame, each with the passes the plan counts
struct PartialGroupsJob {
  jxlhip_ctx* c;
  const PartialPlan* plan;
  uint32_t num_groups;
  jxlhip_ac_pass* const* passes;
  const uint32_t* shifts;
  const uint8_t* acs;
  const int32_t* raw_quant;
  const uint8_t* quant_dc;
  const uint8_t* const* sections;
  const size_t* sizes;
  std::atomic<int> status{JXLHIP_OK};
};
void PartialGroupsFunc(void* opaque, uint32_t g, size_t) {
  PartialGroupsJob* j = static_cast<PartialGroupsJob*>(opaque);
  const uint32_t k = j->plan->passes_of[g];
  if (k == 0 || j->status.load(std::memory_order_relaxed) != JXLHIP_OK) return;
  const jxlhip_ac_pass* pp[11];
  const uint8_t* data[11];
  size_t sizes[11], pos[11];
  for (uint32_t p = 0; p < k; p++) {
    pp[p] = j->passes[p];
    data[p] = j->sections[(size_t)p * j->num_groups + g];
    sizes[p] = j->sizes[(size_t)p * j->num_groups + g];
    pos[p] = 0;
  }
  const int rc = jxlhip_ac_group_decode_submit_passes(j->c, k, pp, j->shifts, g, j->acs, j->raw_quant, j->quant_dc, data, sizes, pos);
  if (rc != JXLHIP_OK) {
    int expected = JXLHIP_OK;
    j->status.compare_exchange_strong(expected, rc);
  }
}

// extra channels from the handle's image to float planes (jxlhip_modular_extra_channel_rows_f32), 64 rows per task
struct ExtraRowsJob {
  const jxlhip_modular_tree* tree;
  uint32_t ec_bits[4], image_bits, ysize, tasks_per_channel;
  float* planes[4];
  size_t strides[4];
  std::atomic<int> status{JXLHIP_OK};
};
void ExtraRowsFunc(void* opaque, uint32_t t, size_t) {
  ExtraRowsJob* j = static_cast<ExtraRowsJob*>(opaque);
  const uint32_t e = t / j->tasks_per_channel, y0 = (t % j->tasks_per_channel) * 64;
  if (!j->planes[e]) return;
  const int rc = jxlhip_modular_extra_channel_rows_f32(j->tree, e, j->ec_bits[e], j->image_bits, y0,
                                                       std::min(j->ysize, y0 + 64), j->planes[e], j->strides[e]);
  if (rc != JXLHIP_OK) {
    int expected = JXLHIP_OK;
    j->status.compare_exchange_strong(expected, rc);
  }
}

struct DcJob {
  const jxlhip_modular_tree* tree;
  const jxlhip_frame_header* fh;
  const uint8_t* const* sections;
  const size_t* sizes;
  int32_t* qdc[3];
  uint8_t* precision;
  uint8_t* acs;
  int32_t* raw_quant;
  uint8_t* sharp;
  int8_t* ytox;
  int8_t* ytob;
  uint32_t* used_acs;
  // the block contexts of a group's rectangle (jxlhip_quant_dc_contexts), by the thread that decoded it
  const jxlhip_block_ctx_map* ctx_map = nullptr;
  uint8_t* qctx = nullptr;
  // task `ndc`, beside the DC groups: the AC-global section (FrameDecoder::ProcessACGlobal, dec_frame.cc:372-416).  A
  // dozen DC groups keep a dozen threads busy for milliseconds each; the section that follows them in the file needs
  // nothing of theirs but the set of strategies in use -- which only limits the coefficient orders worth keeping, so
  // it is read with every strategy marked and runs on one of the idle threads meanwhile
  uint32_t ndc = 0;
  const uint8_t* ag_data = nullptr;
  size_t ag_size = 0;
  uint32_t ag_groups = 0, ag_passes = 0;
  jxlhip_quant_encoding* ag_enc = nullptr;
  uint32_t* ag_num_hist = nullptr;
  jxlhip_ac_pass** ag_pass_handles = nullptr;
  int ag_status = JXLHIP_OK;
  std::atomic<int> status{JXLHIP_OK};
  // (the pipelined call) a group's strategy map / quant field / block contexts are complete: its AC groups may start
  void (*block_info_hook)(void* opaque, uint32_t g) = nullptr;
  void* hook_opaque = nullptr;
  // JXLHIP_CODESTREAM_VERBOSE=1: when each task ran (ms from the runner call) and on which thread
  std::chrono::steady_clock::time_point t0;
  std::vector<float>* timeline = nullptr;  // [task] = {start, end, thread}
};
constexpr uint32_t kEveryStrategy = (1u << 27) - 1;  // AcStrategy::kNumValidStrategies bits
int DcInit(void*, size_t) { return 0; }
void DcUnit(void* opaque, uint32_t g, size_t thread);
void DcFunc(void* opaque, uint32_t g, size_t thread) {
  DcJob* j = static_cast<DcJob*>(opaque);
  if (j->timeline) {
    const double a = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - j->t0).count();
    std::vector<float>* tl = j->timeline;
    DcUnit(opaque, g, thread);
    const double b = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - j->t0).count();
    (*tl)[3 * g] = (float)a, (*tl)[3 * g + 1] = (float)b, (*tl)[3 * g + 2] = (float)thread;
    return;
  }
  DcUnit(opaque, g, thread);
}
void DcUnit(void* opaque, uint32_t g, size_t) {
  DcJob* j = static_cast<DcJob*>(opaque);
  if (g == j->ndc && j->ag_data) {
    size_t bits = 0;
    j->ag_status = jxlhip_ac_global_decode(j->ag_data, j->ag_size, j->ag_groups, j->ag_passes, kEveryStrategy, j->ctx_map, j->ag_enc,
                                           j->ag_num_hist, j->ag_pass_handles, &bits);
    return;
  }
  if (j->status.load(std::memory_order_relaxed) != JXLHIP_OK) return;
  size_t pos = 0;
  uint32_t prec = 0;
  struct Ready {  // jxlhip_dc_group_decode_staged's callback: the block contexts of the rectangle, then the caller's hook
    DcJob* j;
    uint32_t g;
    int rc = JXLHIP_OK;
    static void Call(void* opaque) {
      Ready* r = static_cast<Ready*>(opaque);
      DcJob* j = r->j;
      if (j->qctx) {
        const uint32_t xsb = j->fh->xsize_blocks, ysb = j->fh->ysize_blocks, gd = j->fh->group_dim;  // (a DC group covers gd x gd blocks)
        const uint32_t xdg = (xsb + gd - 1) / gd, x0 = (r->g % xdg) * gd, y0 = (r->g / xdg) * gd;
        const uint32_t rw = std::min(gd, xsb - x0), rh = std::min(gd, ysb - y0);
        for (uint32_t y = y0; y < y0 + rh && r->rc == JXLHIP_OK; y++) {
          const size_t at = (size_t)y * xsb + x0;
          const int32_t* q3[3] = {j->qdc[0] + at, j->qdc[1] + at, j->qdc[2] + at};
          r->rc = jxlhip_quant_dc_contexts(j->ctx_map, rw, q3, j->qctx + at);
        }
      }
      if (r->rc == JXLHIP_OK && j->block_info_hook) j->block_info_hook(j->hook_opaque, r->g);
    }
  } ready{j, g};
  int rc = jxlhip_dc_group_decode_staged(j->tree, j->sections[g], j->sizes[g], &pos, j->fh, g, j->qdc, &prec, j->acs, j->raw_quant,
                                         j->sharp, j->ytox, j->ytob, j->used_acs, Ready::Call, &ready);
  j->precision[g] = (uint8_t)prec;
  if (rc == JXLHIP_OK) rc = ready.rc;
  if (rc != JXLHIP_OK) {
    int expected = JXLHIP_OK;
    j->status.compare_exchange_strong(expected, rc);
  }
}

struct PassHandles {
  jxlhip_ac_pass* p[11] = {nullptr};
  ~PassHandles() {
    for (auto* q : p)
      if (q) jxlhip_ac_pass_destroy(q);
  }
};

// ---- DC groups, AC global and AC groups in ONE runner call.  A DC group is a serial Modular stream (milliseconds on one
// core), a frame has a dozen of them and they end at different times; the AC groups under a DC group need nothing but
// that group's strategy / quant-field / context rectangles and the AC-global section.  So the frame is a pool of work
// units -- ndc DC groups, AC global, ng AC groups -- and the runner's ndc + 1 + ng tasks are TICKETS: a ticket takes
// the next unclaimed DC-phase unit if there is one (the largest sections first), else the next READY AC group (those
// of finished DC groups, largest first), else waits for a DC group to finish.  Any execution order of the tickets
// completes: the DC-phase units never wait, and a ticket only waits while every DC-phase unit is claimed, i.e. running
// on another thread.  (FrameDecoder runs ProcessDCGroup, ProcessACGlobal and ProcessACGroup as three barriers,
// dec_frame.cc:596-703: the threads of the third stand idle through the first.)
struct PipelineJob {
  DcJob dc;
  GroupsJob ac;
  uint32_t ndc = 0, ng = 0;
  std::vector<uint32_t> dc_order;                 // DC-phase units, first to last: AC global, then DC groups by bytes
  std::vector<std::vector<uint32_t>> ac_of_dc;    // the AC groups under each DC group, largest section first
  std::atomic<uint32_t> dc_next{0};
  std::vector<uint32_t> ready;                    // AC groups that may run, in the order they became ready
  std::atomic<uint32_t> ready_end{0}, ready_next{0};
  std::mutex mu;
  std::condition_variable cv;
  bool ag_done = false;                           // (under mu)
  std::vector<uint32_t> waiting_for_ag;           // DC groups finished before AC global (under mu)
  std::atomic<bool> stop{false};                  // a unit failed: the tickets drain
  std::atomic<bool> ac_range{false};              // a coefficient left the 16-bit range: AC groups stop, DC groups go on
  std::chrono::steady_clock::time_point t_call;   // when the runner was called; dc_end_us: when the last DC-phase unit ended
  std::atomic<int64_t> dc_end_us{0};
  void Publish(uint32_t g) {                      // (under mu)
    uint32_t e = ready_end.load(std::memory_order_relaxed);
    for (uint32_t a : ac_of_dc[g]) ready[e++] = a;
    ready_end.store(e, std::memory_order_release);
  }
  // DcJob::block_info_hook: DC group g's rectangles are in (its sharpness channel is still being decoded)
  static void BlockInfoReady(void* opaque, uint32_t g) {
    PipelineJob* j = static_cast<PipelineJob*>(opaque);
    {
      std::lock_guard<std::mutex> lock(j->mu);
      if (j->ag_done) j->Publish(g);
      else j->waiting_for_ag.push_back(g);
    }
    j->cv.notify_all();
  }
};
int PipelineInit(void* opaque, size_t num_threads) { return GroupsInit(&static_cast<PipelineJob*>(opaque)->ac, num_threads); }
void PipelineFunc(void* opaque, uint32_t, size_t thread) {
  PipelineJob* j = static_cast<PipelineJob*>(opaque);
  const uint32_t u = j->dc_next.fetch_add(1, std::memory_order_relaxed);
  if (u <= j->ndc) {
    const uint32_t g = j->dc_order[u];
    DcFunc(&j->dc, g, thread);
    {
      const int64_t now = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - j->t_call).count();
      int64_t seen = j->dc_end_us.load(std::memory_order_relaxed);
      while (seen < now && !j->dc_end_us.compare_exchange_weak(seen, now, std::memory_order_relaxed)) {
      }
    }
    bool failed;
    {
      std::lock_guard<std::mutex> lock(j->mu);
      failed = g == j->ndc ? j->dc.ag_status != JXLHIP_OK : j->dc.status.load() != JXLHIP_OK;
      if (failed) {
        j->stop.store(true);
      } else if (g == j->ndc) {
        j->ag_done = true;
        for (uint32_t d : j->waiting_for_ag) j->Publish(d);
        j->waiting_for_ag.clear();
      }  // (a DC group published its AC groups from inside the call: BlockInfoReady)
    }
    j->cv.notify_all();
    return;
  }
  for (;;) {
    if (j->stop.load(std::memory_order_relaxed) || j->ac_range.load(std::memory_order_relaxed)) return;
    uint32_t i = j->ready_next.load(std::memory_order_relaxed);
    if (i < j->ready_end.load(std::memory_order_acquire)) {
      if (!j->ready_next.compare_exchange_weak(i, i + 1, std::memory_order_relaxed)) continue;
      GroupsOne(&j->ac, j->ready[i], thread);
      const int st = j->ac.status.load(std::memory_order_relaxed);
      // set under the mutex, like the DC branch: a ticket between its predicate check and its cv.wait must not
      // miss the wake-up
      if (st == JXLHIP_ERR_RANGE) {
        {
          std::lock_guard<std::mutex> lock(j->mu);
          j->ac_range.store(true);
        }
        j->cv.notify_all();
      } else if (st != JXLHIP_OK) {
        {
          std::lock_guard<std::mutex> lock(j->mu);
          j->stop.store(true);
        }
        j->cv.notify_all();
      }
      return;
    }
    if (i >= j->ng) return;  // (every AC group has been handed out)
    std::unique_lock<std::mutex> lock(j->mu);
    j->cv.wait(lock, [&] {
      return j->stop.load() || j->ac_range.load() || j->ready_next.load() < j->ready_end.load(std::memory_order_acquire);
    });
  }
}

}  // namespace

int jxlhip_codestream_basic_info(const uint8_t* data, size_t size, jxlhip_codestream_info* info) {
  if (!data || !info) return JXLHIP_ERR_INVALID_ARGUMENT;
  std::vector<uint8_t> storage;
  const uint8_t* cs = nullptr;
  size_t n = 0;
  bool container = false;
  int rc = ExtractCodestream(data, size, &storage, &cs, &n, &container);
  if (rc) return rc;
  ParsedHeaders h;
  try {
    if ((rc = ParseHeaders(cs, n, &h))) return rc;
  } catch (const std::bad_alloc&) {
    return JXLHIP_ERR_OUT_OF_MEMORY;
  }
  FillInfo(h, container, info);
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
  std::vector<uint8_t> storage;
  const uint8_t* cs = nullptr;
  size_t n = 0;
  bool container = false;
  int rc = ExtractCodestream(data, size, &storage, &cs, &n, &container);
  if (rc) return rc;
  // a single-frame file as jxlhip_codestream_basic_info reads it; what that refuses, as the walk of the sequence calls does
  try {
    ParsedHeaders h;
    Sequence s;
    rc = ParseHeaders(cs, n, &h);
    const bool sequence = rc == JXLHIP_ERR_UNSUPPORTED;
    if (sequence && (rc = WalkSequence(cs, n, &s)) == JXLHIP_ERR_UNSUPPORTED) why = s.h.why;
    if (!rc && display) rc = ApplyDisplay(*display, sequence ? &s.h : &h, &why);
    if (rc) {
      if (why_out) *why_out = why;
      return rc;
    }
    if (sequence) FillSequenceInfo(s, container, info, nullptr);
    else FillInfo(h, container, info);
  } catch (const std::bad_alloc&) {
    return JXLHIP_ERR_OUT_OF_MEMORY;
  }
  return JXLHIP_OK;
}

int jxlhip_codestream_icc_profile(const uint8_t* data, size_t size, uint8_t* icc, size_t icc_capacity, size_t* icc_size) {
  if (!data || !icc_size || (icc_capacity && !icc)) return JXLHIP_ERR_INVALID_ARGUMENT;
  *icc_size = 0;
  try {
    std::vector<uint8_t> storage;
    const uint8_t* cs = nullptr;
    size_t n = 0, pos = 0;
    bool container = false;
    int rc = ExtractCodestream(data, size, &storage, &cs, &n, &container);
    if (rc) return rc;
    jxlhip_image_header ih;
    if ((rc = jxlhip_image_header_decode(cs, n, &pos, nullptr, 0, &ih))) return rc;
    if (!ih.color_encoding.want_icc) return JXLHIP_OK;
    return jxlhip_icc_decode(cs, n, &pos, icc_capacity ? icc : nullptr, icc_capacity, icc_size);
  } catch (const std::bad_alloc&) {
    return JXLHIP_ERR_OUT_OF_MEMORY;
  }
}

static int DecodeCodestreamImpl(jxlhip_ctx* c, jxlhip_parallel_runner runner, void* runner_opaque, const uint8_t* data,
                                size_t size, uint32_t output_kind, const jxlhip_output_format* out_format, void* out,
                                size_t out_stride, size_t out_plane_stride, float* const* extra_planes,
                                uint32_t num_extra_planes, size_t extra_stride, jxlhip_codestream_info* info_out);

// The header-controlled sizes below drive host allocations (side info of up to 2^22 groups): an allocation failure
// must come back as a status, not as an exception through the C boundary (the reference returns an error too).
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
  try {
    const int rc = DecodeCodestreamImpl(c, runner, runner_opaque, data, size, output_kind, out_format, out, out_stride,
                                        out_plane_stride, extra_planes, num_extra_planes, extra_stride, info_out);
    // an early return may leave uploads of this frame queued: nothing of it may still be in flight when the
    // caller frees its buffers
    if (rc != JXLHIP_OK && c && !c->multi && c->stream) (void)hipStreamSynchronize(c->stream);
    return rc;
  } catch (const std::bad_alloc&) {
    return c ? Fail(c, JXLHIP_ERR_OUT_OF_MEMORY, "host allocation failed while decoding the codestream") : JXLHIP_ERR_OUT_OF_MEMORY;
  }
}

// wall-clock of the phases of the last jxlhip_decode_codestream on a context (jxlhip_codestream_phase_ms)
struct PhaseClock {
  double* ms;
  std::chrono::steady_clock::time_point t;
  explicit PhaseClock(double* out) : ms(out), t(std::chrono::steady_clock::now()) {
    for (int i = 0; i < JXLHIP_CODESTREAM_PHASES; i++) ms[i] = 0.0;
  }
  void Mark(int phase) {
    const auto now = std::chrono::steady_clock::now();
    ms[phase] += std::chrono::duration<double, std::milli>(now - t).count();
    t = now;
  }
};

int jxlhip_codestream_phase_ms(const jxlhip_ctx* c, double* ms) {
  if (!c || !ms) return JXLHIP_ERR_INVALID_ARGUMENT;
  for (int i = 0; i < JXLHIP_CODESTREAM_PHASES; i++) ms[i] = c->cs_phase_ms[i];
  return JXLHIP_OK;
}

// what the caller of one frame's decode wants (DecodeFrameAt)
struct FrameCall {
  jxlhip_parallel_runner runner = nullptr;
  void* runner_opaque = nullptr;
  uint32_t output_kind = 0;      // without JXLHIP_OUT_UNDO_ORIENTATION
  bool undo_orientation = false;
  const jxlhip_output_format* out_format = nullptr;
  void* out = nullptr;           // (NULL: a blended frame that is only saved)
  size_t out_stride = 0, out_plane_stride = 0;
  float* const* extra_planes = nullptr;
  uint32_t num_extra_planes = 0;
  size_t extra_stride = 0;
  uint32_t out_xsize = 0, out_ysize = 0;  // the size an upsampled frame comes out at: the image's, or a cropped frame's own
  uint32_t noise_visible = 1, noise_nonvisible = 0;  // PassesDecoderState::visible_frame_index / nonvisible_frame_index
  const jxlhip_blend_params* blend = nullptr;
  // an incomplete file (a plain frame of more than one section): the sections the plan counts are decoded, the
  // groups without AC are drawn from their DC (jxlhip_set_dc_only_groups); nullptr = every section is there
  const PartialPlan* partial = nullptr;
};
static int DecodeFrameAt(jxlhip_ctx* c, const uint8_t* cs, size_t n, const ParsedHeaders& h, const jxlhip_frame_header& fh,
                         size_t frame_bit_pos, const FrameCall& fc, PhaseClock& clock, bool verbose, jxlhip_codestream_info* info_p,
                         size_t* end_bit_pos);

static int DecodeCodestreamImpl(jxlhip_ctx* c, jxlhip_parallel_runner runner, void* runner_opaque, const uint8_t* data,
                                size_t size, uint32_t output_kind, const jxlhip_output_format* out_format, void* out,
                                size_t out_stride, size_t out_plane_stride, float* const* extra_planes,
                                uint32_t num_extra_planes, size_t extra_stride, jxlhip_codestream_info* info_out) {
  const bool undo_orientation = (output_kind & JXLHIP_OUT_UNDO_ORIENTATION) != 0;
  output_kind &= ~(uint32_t)JXLHIP_OUT_UNDO_ORIENTATION;
  if (!c || !data || !out || output_kind > JXLHIP_OUT_PACKED || (output_kind == JXLHIP_OUT_PACKED && !out_format))
    return JXLHIP_ERR_INVALID_ARGUMENT;
  JXLHIP_NO_MULTI(c);
  // one file's reference frames never reach the next
  for (uint32_t slot = 0; slot < 4; slot++) {
    const int cleared = jxlhip_set_reference_frame(c, slot, 0, 0, nullptr, 0, 0);
    if (cleared) return cleared;
  }
  PhaseClock clock(c->cs_phase_ms);
  const bool verbose = jxlhip_env::Get().codestream_verbose.load(std::memory_order_relaxed);
  g_upload_wait_on.store(verbose);
  std::vector<uint8_t> storage;
  const uint8_t* cs = nullptr;
  size_t n = 0;
  bool container = false;
  int rc = ExtractCodestream(data, size, &storage, &cs, &n, &container);
  if (rc) return Fail(c, rc, "not a JPEG XL codestream or container");
  ParsedHeaders h;
  if ((rc = ParseHeaders(cs, n, &h)))
    return Fail(c, rc, rc == JXLHIP_ERR_UNSUPPORTED ? (h.why[0] ? h.why : "stream uses features outside the VarDCT back-end") : "invalid headers");
  if ((rc = ApplyDisplay(c, &h))) return rc;
  for (uint32_t slot = 0; slot < 4; slot++) {
    const ReferenceFrame& r = h.refs[slot];
    if (r.xsize == 0) continue;
    const size_t plane = (size_t)r.xsize * r.ysize;
    const float* const planes[3] = {r.xyb.data(), r.xyb.data() + plane, r.xyb.data() + 2 * plane};
    if ((rc = jxlhip_set_reference_frame(c, slot, r.xsize, r.ysize, planes, r.xsize, 0))) return rc;
  }
  jxlhip_codestream_info info;
  FillInfo(h, container, &info);
  FrameCall fc;
  fc.runner = runner;
  fc.runner_opaque = runner_opaque;
  fc.output_kind = output_kind;
  fc.undo_orientation = undo_orientation;
  fc.out_format = out_format;
  fc.out = out;
  fc.out_stride = out_stride;
  fc.out_plane_stride = out_plane_stride;
  fc.extra_planes = extra_planes;
  fc.num_extra_planes = num_extra_planes;
  fc.extra_stride = extra_stride;
  fc.out_xsize = h.ih.xsize;
  fc.out_ysize = h.ih.ysize;
  if ((rc = DecodeFrameAt(c, cs, n, h, h.fh, h.frame_bit_pos, fc, clock, verbose, &info, nullptr))) return rc;
  if (info_out) *info_out = info;
  return JXLHIP_OK;
}

// One VarDCT frame of a file: from the first bit behind its frame header (the TOC) to the pixels (FrameCall::out; with
// FrameCall::blend, blended over a canvas and / or saved, jxlhip_set_blending).  *end_bit_pos (may be NULL) = the first
// bit behind its sections: the next frame's header.
static int DecodeFrameAt(jxlhip_ctx* c, const uint8_t* cs, size_t n, const ParsedHeaders& h, const jxlhip_frame_header& fh,
                         size_t frame_bit_pos, const FrameCall& fc, PhaseClock& clock, bool verbose, jxlhip_codestream_info* info_p,
                         size_t* end_bit_pos) {
  jxlhip_codestream_info& info = *info_p;
  const jxlhip_parallel_runner runner = fc.runner;
  void* const runner_opaque = fc.runner_opaque;
  const uint32_t output_kind = fc.output_kind;
  const bool undo_orientation = fc.undo_orientation;
  const jxlhip_output_format* const out_format = fc.out_format;
  float* const* const extra_planes = fc.extra_planes;
  const uint32_t num_extra_planes = fc.num_extra_planes;
  const size_t extra_stride = fc.extra_stride;
  int rc;
  const jxlhip_image_header& ih = h.ih;
  if (fh.num_groups > (1u << 22) || fh.num_passes == 0 || fh.num_passes > 11)
    return Fail(c, JXLHIP_ERR_UNSUPPORTED, "frame too large");
  {
    // a few header bytes can claim 2^38 pixels: bound what is allocated before looking at the sections
    // (JXLHIP_MAX_PIXELS, default 2^30 = four 16K frames' worth; each 8x8 block needs ~40 bytes of host side info)
    const uint64_t max_px = jxlhip_env::Get().max_pixels.load(std::memory_order_relaxed);
    if ((uint64_t)fh.xsize_blocks * fh.ysize_blocks * 64u > max_px)
      return Fail(c, JXLHIP_ERR_UNSUPPORTED, "frame of %ux%u blocks exceeds JXLHIP_MAX_PIXELS", fh.xsize_blocks, fh.ysize_blocks);
  }
  const uint32_t ng = (uint32_t)fh.num_groups, ndc = (uint32_t)fh.num_dc_groups, np = fh.num_passes;
  const uint32_t xsb = fh.xsize_blocks, ysb = fh.ysize_blocks;
  const size_t nb = (size_t)xsb * ysb;
  const size_t nt = (size_t)((xsb + 7) / 8) * ((ysb + 7) / 8);

  // ---- table of contents
  size_t pos = frame_bit_pos;
  const uint32_t ntoc = (uint32_t)fh.num_toc_entries;
  std::vector<uint64_t> off(ntoc);
  std::vector<uint32_t> sz(ntoc);
  uint64_t total = 0;
  if ((rc = jxlhip_toc_decode(cs, n, &pos, ntoc, off.data(), sz.data(), &total))) return Fail(c, rc, "invalid TOC");
  const size_t base = pos / 8;
  if (total > n - base && !fc.partial) return Fail(c, JXLHIP_ERR_BAD_STREAM, "truncated frame: %llu section bytes, %zu present",
                                                   (unsigned long long)total, n - base);
  auto sec = [&](uint32_t i) { return cs + base + off[i]; };
  const bool single = ntoc == 1;

  // ---- DC global: quantizer, block context map, colour correlation; the global modular tree
  jxlhip_dc_global dcg;
  size_t spos = 0;  // bit position inside section 0 (the only section of a single-section frame)
  // the patch dictionary leads the section (dec_frame.cc:272-288), the splines bundle follows (:289-293);
  // jxlhip_dc_global_decode reads on from behind them
  std::unique_ptr<jxlhip_patches, void (*)(jxlhip_patches*)> patches(nullptr, jxlhip_patches_destroy);
  if (fh.flags & JXLHIP_FLAG_PATCHES) {
    uint32_t ref_sizes[4][2];
    // what the slots hold; a canvas (a sequence's saved frame) with its size, so that the dictionary decodes and
    // jxlhip_set_patches names the refusal ("saved after the colour transform")
    for (int slot = 0; slot < 4; slot++) {
      ref_sizes[slot][0] = c->slots.ref_w[slot] ? c->slots.ref_w[slot] : c->slots.canvas_w[slot];
      ref_sizes[slot][1] = c->slots.ref_h[slot] ? c->slots.ref_h[slot] : c->slots.canvas_h[slot];
    }
    jxlhip_patches* pt = nullptr;
    if ((rc = jxlhip_patches_decode(sec(0), sz[0], &spos, fh.xsize_blocks * 8, fh.ysize_blocks * 8, 0, ref_sizes, &pt)))
      return Fail(c, rc, "invalid patch dictionary");
    patches.reset(pt);
    uint32_t count = 0;
    if ((rc = jxlhip_patches_list(pt, &count, nullptr, nullptr, nullptr, nullptr))) return Fail(c, rc, "invalid patch dictionary");
    if (count == 0) patches.reset();  // an empty dictionary: the frame takes its plain path
  }
  std::unique_ptr<jxlhip_splines, void (*)(jxlhip_splines*)> splines(nullptr, jxlhip_splines_destroy);
  if (fh.flags & JXLHIP_FLAG_SPLINES) {
    jxlhip_splines* sp = nullptr;
    if ((rc = jxlhip_splines_decode(sec(0), sz[0], &spos, (uint64_t)fh.xsize * fh.ysize, &sp)))
      return Fail(c, rc, "invalid splines");
    splines.reset(sp);
  }
  float noise_lut[8] = {0};
  if (fh.flags & JXLHIP_FLAG_NOISE) {
    size_t npos = spos;
    if ((rc = jxlhip_noise_lut_decode(sec(0), sz[0], &npos, noise_lut))) return Fail(c, rc, "invalid noise parameters");
  }
  if ((rc = jxlhip_dc_global_decode(sec(0), sz[0], &spos, fh.flags & ~(uint64_t)(JXLHIP_FLAG_SPLINES | JXLHIP_FLAG_PATCHES), &dcg)))
    return Fail(c, rc, "invalid DC global section");
  jxlhip_modular_tree* tree_raw = nullptr;
  if ((rc = jxlhip_modular_global_decode(sec(0), sz[0], &spos, &fh, &tree_raw)))
    return Fail(c, rc, "invalid modular global section");
  struct TreeOwner {
    jxlhip_modular_tree* t;
    ~TreeOwner() { jxlhip_modular_tree_destroy(t); }
  } tree{tree_raw};

  clock.Mark(JXLHIP_PHASE_HEADERS);
  // ---- the back-end's frame parameters (what PassesDecoderState::Init / InitForAC derive); used_acs follows the DC groups
  jxlhip_frame_params p{};
  p.xsize = fh.xsize;
  p.ysize = fh.ysize;
  p.output_kind = output_kind;
  p.undo_orientation = undo_orientation ? ih.orientation : 0;
  p.global_scale = dcg.global_scale;
  p.quant_dc = dcg.quant_dc;
  p.x_dm_multiplier = fh.x_dm_multiplier;
  p.b_dm_multiplier = fh.b_dm_multiplier;
  memcpy(p.quant_biases, ih.quant_biases, sizeof(p.quant_biases));
  p.cfl_base_x = dcg.cfl_base_x;
  p.cfl_base_b = dcg.cfl_base_b;
  p.cfl_color_factor = dcg.cfl_color_factor;
  p.lf = fh.lf;
  memcpy(p.opsin_biases, ih.opsin_biases, sizeof(p.opsin_biases));
  {
    const float scale = 255.0f / ih.intensity_target;  // OpsinParams::Init, opsin_params.cc:35-45
    for (int i = 0; i < 9; i++) p.inverse_opsin_matrix[i] = h.inv_matrix[i] * scale;
  }
  if (out_format) p.out_format = *out_format;

  // an alpha channel is decoded only when the output has room for it; its bytes sit behind the coefficients of
  // every AC-group section and are skipped otherwise
  // (a frame that is blended or saved hands ALL its extra channels to jxlhip_set_blending_extra instead: below)
  const bool blend_ec = fc.blend && ih.num_extra_channels != 0;
  const bool want_alpha = !blend_ec && h.alpha_index >= 0 && output_kind == JXLHIP_OUT_PACKED && out_format->num_channels == 4;
  // the caller's host planes for the extra channels (jxlhip_decode_codestream_extra)
  float* user_plane[4] = {nullptr, nullptr, nullptr, nullptr};
  bool want_planes = false;
  for (uint32_t i = 0; i < ih.num_extra_channels && i < num_extra_planes && i < 4; i++) {
    user_plane[i] = extra_planes[i];
    want_planes |= user_plane[i] != nullptr;
  }
  if (want_planes && extra_stride < ih.xsize) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "extra_stride below the image width");
  // the planes of a blended frame, at the FRAME's size (a cropped frame's channels are as small as its colour)
  std::vector<float> blend_planes;
  size_t plane_stride = extra_stride;
  if (blend_ec) {
    if (want_planes) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "the caller's extra-channel planes on a blended frame");
    const size_t plane = (size_t)fh.xsize * fh.ysize;
    blend_planes.resize(ih.num_extra_channels * plane);
    for (uint32_t i = 0; i < ih.num_extra_channels; i++) user_plane[i] = blend_planes.data() + i * plane;
    plane_stride = fh.xsize;
    want_planes = true;
  }
  const bool want_modular = want_alpha || want_planes;
  std::vector<size_t> end_bits(want_modular ? (size_t)np * ng : 0, 0);
  std::vector<const uint8_t*> asec((size_t)np * ng);
  std::vector<size_t> asz((size_t)np * ng);
  std::vector<uint32_t> shifts(np);
  for (uint32_t ps = 0; ps < np; ps++) shifts[ps] = fh.shift[ps];
  if (!single) {
    for (uint32_t ps = 0; ps < np; ps++)
      for (uint32_t g = 0; g < ng; g++) {
        asec[(size_t)ps * ng + g] = sec(2 + ndc + ps * ng + g);
        asz[(size_t)ps * ng + g] = sz[2 + ndc + ps * ng + g];
      }
  }

  // ---- DC groups on the runner: quantized DC + the AC metadata (strategy map, quant field, sharpness, cmaps); with a
  // runner, AC global and the AC groups (16-bit coefficients, optimistically) in the same call: PipelineJob
  std::vector<int32_t> qdc(3 * nb), raw_quant(nb);
  std::vector<uint8_t> acs(nb), sharp(nb), prec(ndc), qctx(nb);
  std::vector<int8_t> ytox(nt), ytob(nt);
  uint32_t used_acs = 0;
  jxlhip_quant_encoding enc[JXLHIP_NUM_QUANT_TABLES];
  uint32_t num_hist = 0;
  PassHandles passes;
  bool ac_global_done = false;
  int ac_i16_status = JXLHIP_ERR_STATE;  // != STATE: the AC groups went through the pipelined call as 16-bit coefficients, with this result
  double ac_tail_ms = 0;                 // how long the pipelined call went on after its last DC-phase unit
  {
    PipelineJob pj;
    DcJob& job = pj.dc;
    job.tree = tree.t;
    job.fh = &fh;
    for (int ch = 0; ch < 3; ch++) job.qdc[ch] = qdc.data() + ch * nb;
    job.precision = prec.data();
    job.acs = acs.data();
    job.raw_quant = raw_quant.data();
    job.sharp = sharp.data();
    job.ytox = ytox.data();
    job.ytob = ytob.data();
    job.used_acs = &used_acs;
    job.ndc = ndc;
    if (single) {
      uint32_t p0 = 0;
      rc = jxlhip_dc_group_decode(tree.t, sec(0), sz[0], &spos, &fh, 0, job.qdc, &p0, job.acs, job.raw_quant, job.sharp,
                                  job.ytox, job.ytob, &used_acs);
      prec[0] = (uint8_t)p0;
      if (rc) return Fail(c, rc, "invalid DC group");
    } else {
      std::vector<const uint8_t*> dsec(ndc);
      std::vector<size_t> dsz(ndc);
      for (uint32_t g = 0; g < ndc; g++) {
        dsec[g] = sec(1 + g);
        dsz[g] = sz[1 + g];
      }
      job.sections = dsec.data();
      job.sizes = dsz.data();
      job.ctx_map = &dcg.block_ctx_map;
      job.qctx = qctx.data();
      if (runner && fc.partial) {  // the DC groups alone: AC global may not be there, and the AC groups follow the plan
        if (runner(runner_opaque, &job, DcInit, DcFunc, 0, ndc) != 0) return Fail(c, JXLHIP_ERR_STATE, "parallel runner failed");
      } else if (runner) {
        // (the AC-global section rides along as one more unit: DcJob)
        job.ag_data = sec(1 + ndc);
        job.ag_size = sz[1 + ndc];
        job.ag_groups = ng;
        job.ag_passes = np;
        job.ag_enc = enc;
        job.ag_num_hist = &num_hist;
        job.ag_pass_handles = passes.p;
        std::vector<float> timeline;
        if (verbose) {
          timeline.assign(3 * (size_t)(ndc + 1), 0.0f);
          job.timeline = &timeline;
          job.t0 = std::chrono::steady_clock::now();
          fprintf(stderr, "[codestream] %.2f ms from the headers to the runner call (frame-level arrays, frame_begin)\n",
                  std::chrono::duration<double, std::milli>(job.t0 - clock.t).count());
        }
        // the frame on the back-end BEFORE the call: the AC groups submit their coefficients from inside it
        p.coeff_type = JXLHIP_COEFF_I16;
        p.used_acs = 0;
        const bool pipelined = !jxlhip_env::Get().no_pipeline.load(std::memory_order_relaxed) && (rc = jxlhip_frame_begin(c, &p)) == JXLHIP_OK && (rc = EnsureUploadBuffers(c)) == JXLHIP_OK;
        if (rc) return rc;
        if (pipelined) {
          pj.ndc = ndc;
          pj.ng = ng;
          job.block_info_hook = PipelineJob::BlockInfoReady;
          job.hook_opaque = &pj;
          GroupsJob& gj = pj.ac;
          gj.c = c;
          gj.num_passes = np;
          gj.num_groups = ng;
          gj.passes = passes.p;  // (filled in by the AC-global unit before the first AC group is published)
          gj.shifts = shifts.data();
          gj.acs = acs.data();
          gj.raw_quant = raw_quant.data();
          gj.quant_dc = qctx.data();
          gj.sections = asec.data();
          gj.sizes = asz.data();
          gj.end_bits = want_modular ? end_bits.data() : nullptr;
          gj.sparse = SparseEligible(c, np);
          if (verbose) {
            gj.timeline.assign(3 * (size_t)ng, 0.0f);
            gj.t0 = job.t0;
          }
          // DC-phase units: AC global first (short, and every AC group waits for it), then the DC groups by bytes
          std::vector<uint64_t> key(ndc);
          for (uint32_t g = 0; g < ndc; g++) key[g] = ((uint64_t)std::min<size_t>(dsz[g], 0xFFFFFFFFu) << 32) | (uint32_t)~g;
          std::sort(key.begin(), key.end(), std::greater<uint64_t>());
          pj.dc_order.push_back(ndc);
          for (uint32_t g = 0; g < ndc; g++) pj.dc_order.push_back(~(uint32_t)key[g]);
          // the AC groups under each DC group (8 x 8 of them, dec_frame.cc:318-360 / frame_dimensions.h), largest first
          const uint32_t xsg = (fh.xsize + 255) / 256, xdg = (fh.xsize_blocks + fh.group_dim - 1) / fh.group_dim;
          pj.ac_of_dc.resize(ndc);
          {
            std::vector<uint64_t> akey(ng);
            for (uint32_t g = 0; g < ng; g++) {
              uint64_t bytes = 0;
              for (uint32_t ps = 0; ps < np; ps++) bytes += asz[(size_t)ps * ng + g];
              akey[g] = (std::min<uint64_t>(bytes, 0xFFFFFFFFu) << 32) | (uint32_t)~g;
            }
            std::sort(akey.begin(), akey.end(), std::greater<uint64_t>());
            for (uint32_t t = 0; t < ng; t++) {
              const uint32_t g = ~(uint32_t)akey[t];
              const uint32_t d = (g / xsg / 8) * xdg + (g % xsg) / 8;
              if (d >= ndc) return Fail(c, JXLHIP_ERR_STATE, "AC group %u under no DC group", g);
              pj.ac_of_dc[d].push_back(g);
            }
          }
          pj.ready.resize(ng);
          pj.t_call = std::chrono::steady_clock::now();
          if (runner(runner_opaque, &pj, PipelineInit, PipelineFunc, 0, ndc + 1 + ng) != 0) return Fail(c, JXLHIP_ERR_STATE, "parallel runner failed");
          // (the phase report: what of the call followed the last DC group is the AC groups' own time)
          ac_tail_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - pj.t_call).count() - pj.dc_end_us.load() * 1e-3;
          for (SparseBatch& sb : gj.batch) {  // what the threads still hold
            const int frc = SparseFlush(c, &sb);
            if (frc != JXLHIP_OK) {
              int expected = JXLHIP_OK;
              gj.status.compare_exchange_strong(expected, frc);
            }
          }
          ac_i16_status = gj.status.load();
          if (verbose) GroupsTimelineReport(gj);
        } else {
          if (runner(runner_opaque, &job, DcInit, DcFunc, 0, ndc + 1) != 0) return Fail(c, JXLHIP_ERR_STATE, "parallel runner failed");
        }
        ac_global_done = true;
        if (verbose) {
          fprintf(stderr, "[codestream] runner call: %.2f ms; DC-phase units (start-end ms @thread):",
                  std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - job.t0).count());
          for (uint32_t g = 0; g <= ndc; g++) {
            fprintf(stderr, " %s%.2f-%.2f@%d", g == ndc ? "acglobal:" : "", timeline[3 * g], timeline[3 * g + 1], (int)timeline[3 * g + 2]);
          }
          fprintf(stderr, "\n");
        }
      } else {
        for (uint32_t g = 0; g < ndc; g++) DcFunc(&job, g, 0);
      }
      if ((rc = job.status.load())) return Fail(c, rc, "invalid DC group");
      if (ac_global_done && job.ag_status) return Fail(c, job.ag_status, "invalid AC global section");
    }
  }
  clock.Mark(JXLHIP_PHASE_DC_GROUPS);
  if (ac_tail_ms > 0) {
    c->cs_phase_ms[JXLHIP_PHASE_DC_GROUPS] -= ac_tail_ms;
    c->cs_phase_ms[JXLHIP_PHASE_AC_GROUPS] += ac_tail_ms;
  }
  if (single) {
    const int32_t* qdc3[3] = {qdc.data(), qdc.data() + nb, qdc.data() + 2 * nb};
    if ((rc = jxlhip_quant_dc_contexts(&dcg.block_ctx_map, nb, qdc3, qctx.data()))) return rc;
  }

  // ---- AC global: dequant encodings, histograms and coefficient orders of every pass (unless it rode along above)
  if (single) {
    rc = jxlhip_ac_global_decode_at(sec(0), sz[0], &spos, ng, np, used_acs, &dcg.block_ctx_map, enc, &num_hist, passes.p);
  } else if (!ac_global_done && (!fc.partial || fc.partial->info.have_ac_global)) {
    size_t bits = 0;
    rc = jxlhip_ac_global_decode(sec(1 + ndc), sz[1 + ndc], ng, np, used_acs, &dcg.block_ctx_map, enc, &num_hist, passes.p, &bits);
  }
  if (rc) return Fail(c, rc, "invalid AC global section");
  clock.Mark(JXLHIP_PHASE_AC_GLOBAL);
  p.used_acs = used_acs;

  // ---- coefficient type: 16-bit buffers optimistically (jxl_hip_entropy.h), int32 when a value does not fit
  for (uint32_t ct = JXLHIP_COEFF_I16; ct <= JXLHIP_COEFF_I32; ct++) {
    const bool ac_in_pipeline = ct == JXLHIP_COEFF_I16 && ac_i16_status != JXLHIP_ERR_STATE;
    if (ac_in_pipeline && ac_i16_status == JXLHIP_ERR_RANGE) continue;  // redo with int32 buffers
    if (ac_in_pipeline && ac_i16_status != JXLHIP_OK) return ac_i16_status;
    p.coeff_type = ct;
    if (ac_in_pipeline) {  // the frame began before the pipelined call; what the DC groups found out since:
      c->p.used_acs = used_acs;
      c->f.used_acs = used_acs & 0x7FFFFFFu;
    } else {
      if ((rc = jxlhip_frame_begin(c, &p))) return rc;
      if ((rc = EnsureUploadBuffers(c))) return rc;
    }
    const jxlhip_frame_inputs& in = c->up_inputs;
    hipStream_t st = c->stream;
    // side info; the DC planes are produced on the device straight into the upload slab
    HIPCHK(c, hipMemcpyAsync((void*)in.ac_strategy, acs.data(), nb, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync((void*)in.raw_quant, raw_quant.data(), nb * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync((void*)in.epf_sharpness, sharp.data(), nb, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync((void*)in.ytox_map, ytox.data(), nt, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync((void*)in.ytob_map, ytob.data(), nt, hipMemcpyHostToDevice, st));
    if ((rc = c->qdc_dev.Reserve(c, 3 * nb))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->qdc_dev, qdc.data(), 3 * nb * sizeof(int32_t), hipMemcpyHostToDevice, st));
    {
      const int32_t* q3[3] = {c->qdc_dev, c->qdc_dev + nb, c->qdc_dev + 2 * nb};
      float* d3[3] = {(float*)in.dc[0], (float*)in.dc[1], (float*)in.dc[2]};
      const float cscale = 1.0f / (float)dcg.cfl_color_factor;  // ColorCorrelation::YtoXRatio / YtoBRatio
      const float cfl_x = dcg.cfl_base_x + (float)dcg.ytox_dc * cscale;
      const float cfl_b = dcg.cfl_base_b + (float)dcg.ytob_dc * cscale;
      const int smooth = !(fh.flags & JXLHIP_FLAG_SKIP_ADAPTIVE_DC_SMOOTHING);
      if ((rc = jxlhip_dequant_dc_groups(c, q3, d3, dcg.dc_quant, cfl_x, cfl_b, smooth, prec.data()))) return rc;
    }
    // (without AC global no coefficient is dequantised: phase 1 runs over zeroes with the default tables)
    const bool have_enc = !fc.partial || fc.partial->info.have_ac_global;
    if ((rc = have_enc ? jxlhip_dequant_tables(c, enc, (float*)in.dequant_table) : jxlhip_default_dequant_tables(c, (float*)in.dequant_table))) return rc;
    ApplyInputs(c, &in);
    c->have_inputs = true;
    c->blocks_done = false;
    DropPrepared(c);  // (new maps, and used_acs above)
    if (fc.partial) {  // in front of the prepare: a frame with DC-only groups is two-phase
      std::vector<uint8_t> mask(ng);
      for (uint32_t g = 0; g < ng; g++) mask[g] = fc.partial->passes_of[g] == 0;
      if ((rc = jxlhip_set_dc_only_groups(c, mask.data(), (ih.custom_weights_mask & 4u) ? ih.upsampling8_weights : nullptr))) return rc;
    }
    if ((rc = PrepareAhead(c, (fh.flags & JXLHIP_FLAG_NOISE) || splines || patches || fh.upsampling > 1))) return rc;  // under the AC groups' entropy decode instead of in front of the frame's kernels
    clock.Mark(JXLHIP_PHASE_SIDE_INFO);
    // AC groups on the runner: entropy decode into pinned staging slots + uploads
    if (ac_in_pipeline) {
      rc = JXLHIP_OK;  // (decoded and submitted inside the pipelined call)
    } else if (fc.partial) {  // every group the passes it has
      PartialGroupsJob pg;
      pg.c = c;
      pg.plan = fc.partial;
      pg.num_groups = ng;
      pg.passes = passes.p;
      pg.shifts = shifts.data();
      pg.acs = acs.data();
      pg.raw_quant = raw_quant.data();
      pg.quant_dc = qctx.data();
      pg.sections = asec.data();
      pg.sizes = asz.data();
      if (runner) {
        if (runner(runner_opaque, &pg, ModularGroupsInit, PartialGroupsFunc, 0, ng) != 0) return Fail(c, JXLHIP_ERR_STATE, "parallel runner failed");
      } else {
        for (uint32_t g = 0; g < ng; g++) PartialGroupsFunc(&pg, g, 0);
      }
      rc = pg.status.load();
    } else if (single) {
      const uint8_t* d1[11];
      size_t s1[11], b1[11];
      // one section: the AC group follows AC global at the current bit position (one pass)
      d1[0] = sec(0);
      s1[0] = sz[0];
      b1[0] = spos;
      const jxlhip_ac_pass* pp[11];
      for (uint32_t i = 0; i < np; i++) pp[i] = passes.p[i];
      rc = jxlhip_ac_group_decode_submit_passes(c, 1, pp, shifts.data(), 0, acs.data(), raw_quant.data(), qctx.data(), d1, s1, b1);
      if (want_modular) end_bits[0] = b1[0];
    } else {
      const jxlhip_ac_pass* pp[11];
      for (uint32_t i = 0; i < np; i++) pp[i] = passes.p[i];
      rc = jxlhip_ac_groups_decode_submit_ex(c, runner, runner_opaque, np, pp, shifts.data(), acs.data(), raw_quant.data(),
                                             qctx.data(), asec.data(), asz.data(), want_modular ? end_bits.data() : nullptr);
    }
    clock.Mark(JXLHIP_PHASE_AC_GROUPS);
    if (rc == JXLHIP_ERR_RANGE && ct == JXLHIP_COEFF_I16) continue;  // redo with int32 buffers
    if (rc) return rc;
    info.coeff_type = ct;
    break;
  }
  if (want_modular) {  // (the coefficient uploads of the last groups are still in flight)
    // The alpha channel of an RGBA output goes into the context's pinned plane (uploaded by jxlhip_set_alpha), the
    // channels the caller asked for into its planes: by the groups' threads when the channels are larger than a group
    // and final group by group, from the handle's image otherwise
    float* alpha = nullptr;
    size_t astride = 0;
    if (want_alpha && (rc = jxlhip_alpha_staging(c, &alpha, &astride))) return rc;
    ModularGroupsJob job;
    job.collect = !jxlhip_modular_groups_are_final(tree.t);
    const bool in_groups = !job.collect && (fh.xsize > fh.group_dim || fh.ysize > fh.group_dim);
    for (uint32_t i = 0; i < 4; i++) {
      job.ec_bits[i] = i < ih.num_extra_channels ? h.extra[i].bit_depth.bits_per_sample : 8;
      const bool is_alpha = want_alpha && (int)i == h.alpha_index;
      job.planes[i] = is_alpha ? alpha : user_plane[i];
      job.strides[i] = is_alpha ? astride : plane_stride;
    }
    job.image_bits = ih.bit_depth.bits_per_sample;
    job.tree = tree.t;
    job.fh = &fh;
    job.num_groups = ng;
    job.num_passes = single ? 1 : np;
    const uint8_t* s0 = sec(0);
    const size_t z0 = sz[0];
    job.sections = single ? &s0 : asec.data();
    job.sizes = single ? &z0 : asz.data();
    job.start_bits = end_bits.data();
    if (runner && !single) {
      if (runner(runner_opaque, &job, ModularGroupsInit, ModularGroupsFunc, 0, ng) != 0)
        return Fail(c, JXLHIP_ERR_STATE, "parallel runner failed");
    } else {
      for (uint32_t g = 0; g < ng; g++) ModularGroupsFunc(&job, g, 0);
    }
    if ((rc = job.status.load()))
      return Fail(c, rc, rc == JXLHIP_ERR_UNSUPPORTED ? "extra channels coded with Modular features outside this front-end"
                                                       : "invalid Modular data in an AC group");
    if (!in_groups) {
      // the global image's transforms (a squeeze pyramid: every level spread over the runner), then the samples as
      // floats, 64 rows per task
      if ((rc = jxlhip_modular_finalize(tree.t, runner, runner_opaque))) return Fail(c, rc, "extra channels: undoing the transforms");
      ExtraRowsJob rows;
      rows.tree = tree.t;
      rows.image_bits = job.image_bits;
      rows.ysize = fh.ysize;  // (the image's, except for a cropped frame of a sequence)
      rows.tasks_per_channel = (fh.ysize + 63) / 64;
      for (uint32_t i = 0; i < 4; i++) {
        rows.ec_bits[i] = job.ec_bits[i];
        rows.planes[i] = i < ih.num_extra_channels ? job.planes[i] : nullptr;
        rows.strides[i] = job.strides[i];
      }
      const uint32_t tasks = 4 * rows.tasks_per_channel;
      if (runner) {
        if (runner(runner_opaque, &rows, ModularGroupsInit, ExtraRowsFunc, 0, tasks) != 0)
          return Fail(c, JXLHIP_ERR_STATE, "parallel runner failed");
      } else {
        for (uint32_t t = 0; t < tasks; t++) ExtraRowsFunc(&rows, t, 0);
      }
      if ((rc = rows.status.load())) return Fail(c, rc, "extra channel");
    }
    if (want_alpha) {
      if (user_plane[h.alpha_index])  // the caller wants the alpha plane as well
        for (uint32_t y = 0; y < ih.ysize; y++)
          memcpy(user_plane[h.alpha_index] + (size_t)y * extra_stride, alpha + (size_t)y * astride, (size_t)ih.xsize * sizeof(float));
      if ((rc = jxlhip_set_alpha(c, alpha, astride))) return rc;
    }
  }
  clock.Mark(JXLHIP_PHASE_EXTRA_CHANNELS);
  // an upsampled frame: the image header's weights for the factor, or the format's defaults (in front of the splines:
  // their draw list is made for the upsampled size)
  if (fh.upsampling != 1) {
    const uint32_t bit = fh.upsampling == 2 ? 1u : fh.upsampling == 4 ? 2u : 4u;
    const float* coded = fh.upsampling == 2 ? ih.upsampling2_weights : fh.upsampling == 4 ? ih.upsampling4_weights : ih.upsampling8_weights;
    if ((rc = jxlhip_set_upsampling(c, fh.upsampling, (ih.custom_weights_mask & bit) ? coded : nullptr, fc.out_xsize, fc.out_ysize))) return rc;
  }
  // photon noise: a file's only visible frame is visible frame 1 (FrameDecoder::InitFrame counts it before decoding,
  // dec_frame.cc:160-168); a sequence counts its frames (WalkSequence)
  if ((fh.flags & JXLHIP_FLAG_NOISE) && (rc = jxlhip_set_noise(c, noise_lut, fc.noise_visible, fc.noise_nonvisible))) return rc;
  if (patches && (rc = jxlhip_set_patches(c, patches.get()))) return rc;
  if (splines && (rc = jxlhip_set_splines(c, splines.get()))) return rc;
  if (fc.blend && (rc = jxlhip_set_blending(c, fc.blend))) return rc;
  if (blend_ec) {  // the extra channels are blended and saved beside the colour (ExtraChannelInfo, extra_channel_blending_info)
    jxlhip_blend_extra_params e{};
    e.num_extra_channels = ih.num_extra_channels;
    e.color_alpha_channel = fh.blend_alpha_channel;
    e.stride_floats = plane_stride;
    for (uint32_t i = 0; i < ih.num_extra_channels; i++) {
      e.channel[i].is_alpha = h.extra[i].type == JXLHIP_EC_ALPHA;
      e.channel[i].alpha_associated = h.extra[i].alpha_associated;
      e.channel[i].mode = fh.ec_blend_mode[i];
      e.channel[i].alpha_channel = fh.ec_blend_alpha_channel[i];
      e.channel[i].clamp = fh.ec_blend_clamp[i];
      e.channel[i].source = fh.ec_blend_source[i];
      e.planes[i] = user_plane[i];
    }
    if (e.color_alpha_channel >= e.num_extra_channels) return Fail(c, JXLHIP_ERR_BAD_STREAM, "the colour's alpha channel %u of %u extra channels", e.color_alpha_channel, e.num_extra_channels);
    for (uint32_t i = 0; i < e.num_extra_channels; i++)
      if (e.channel[i].alpha_channel >= e.num_extra_channels || e.channel[i].source > 3 || e.channel[i].mode > JXLHIP_BLEND_MUL)
        return Fail(c, JXLHIP_ERR_BAD_STREAM, "blending info of extra channel %u out of range", i);
    if ((rc = jxlhip_set_blending_extra(c, &e))) return rc;
  }
  if (h.display_nits > 0.0f) {  // JxlDecoderSetDesiredIntensityTarget: the stage exists for a PQ original brighter than the display
    const jxlhip_color_encoding& ce = ih.color_encoding;
    jxlhip_tone_mapping tm{};
    tm.orig_intensity_target = ih.intensity_target;
    tm.desired_intensity_target = h.display_nits;
    for (int i = 0; i < 3; i++) tm.luminances[i] = h.luminances[i];
    tm.orig_transfer = (!ce.all_default && !ce.have_gamma && ce.transfer_function == 16) ? JXLHIP_TF_PQ
                       : (!ce.all_default && !ce.have_gamma && ce.transfer_function == 18) ? JXLHIP_TF_HLG
                                                                                            : JXLHIP_TF_SRGB;
    if ((rc = jxlhip_set_tone_mapping(c, &tm))) return rc;
  }
  if ((rc = jxlhip_decode_frame(c, fc.out, fc.out_stride, fc.out_plane_stride))) return rc;
  if ((rc = jxlhip_sync(c))) return rc;
  clock.Mark(JXLHIP_PHASE_KERNELS);
  info.num_passes = np;
  info.num_groups = ng;
  info.num_dc_groups = ndc;
  info.epf_iters = fh.lf.epf_iters;
  info.gab = fh.lf.gab;
  info.used_acs = used_acs;
  if (end_bit_pos) *end_bit_pos = (base + (size_t)total) * 8;
  return JXLHIP_OK;
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
  const bool undo_orientation = (output_kind & JXLHIP_OUT_UNDO_ORIENTATION) != 0;
  const bool blend_extra = (output_kind & JXLHIP_OUT_BLEND_EXTRA_CHANNELS) != 0;
  output_kind &= ~(uint32_t)(JXLHIP_OUT_UNDO_ORIENTATION | JXLHIP_OUT_BLEND_EXTRA_CHANNELS);
  if (!c || !data || !out || !cursor || output_kind > JXLHIP_OUT_PACKED || (output_kind == JXLHIP_OUT_PACKED && !out_format))
    return JXLHIP_ERR_INVALID_ARGUMENT;
  JXLHIP_NO_MULTI(c);
  if (*cursor != 0 && (!c->seq_open || *cursor != c->seq_expect)) {
    return Fail(c, JXLHIP_ERR_STATE, c->seq_open ? "cursor %llu is not the one this context expects (%llu)"
                                                 : "cursor %llu, but no sequence is open on this context (the last frame was decoded, or none was started)",
                (unsigned long long)*cursor, (unsigned long long)c->seq_expect);
  }
  const bool start = *cursor == 0;
  c->seq_open = false;  // (until this call has succeeded)
  if (start) {  // one file's frames never reach the next
    for (uint32_t slot = 0; slot < 4; slot++) {
      const int cleared = jxlhip_set_reference_frame(c, slot, 0, 0, nullptr, 0, 0);
      if (cleared) return cleared;
    }
  }
  PhaseClock clock(c->cs_phase_ms);
  const bool verbose = jxlhip_env::Get().codestream_verbose.load(std::memory_order_relaxed);
  g_upload_wait_on.store(verbose);
  std::vector<uint8_t> storage;
  const uint8_t* cs = nullptr;
  size_t n = 0;
  bool container = false;
  int rc = ExtractCodestream(data, size, &storage, &cs, &n, &container);
  if (rc) return Fail(c, rc, "not a JPEG XL codestream or container");
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
  FillSequenceInfo(s, container, &info, nullptr);
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
      const ReferenceFrame& r = s.h.refs[fh.save_as_reference];
      const size_t plane = (size_t)r.xsize * r.ysize;
      const float* const planes[3] = {r.xyb.data(), r.xyb.data() + plane, r.xyb.data() + 2 * plane};
      if ((rc = jxlhip_set_reference_frame(c, fh.save_as_reference, r.xsize, r.ysize, planes, r.xsize, 0))) return rc;
      continue;
    }
    // a layer nothing reads and nobody sees leaves no trace
    if (!f.displayed && !f.save) continue;
    FrameCall fc;
    fc.runner = runner;
    fc.runner_opaque = runner_opaque;
    fc.output_kind = output_kind;
    fc.undo_orientation = undo_orientation;
    fc.out_format = out_format;
    fc.out = f.displayed ? out : nullptr;
    fc.out_stride = out_stride;
    fc.out_plane_stride = out_plane_stride;
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
    if ((rc = DecodeFrameAt(c, cs, n, s.h, fh, f.toc_bit, fc, clock, verbose, &info, nullptr))) return rc;
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
    std::vector<uint8_t> storage;
    const uint8_t* cs = nullptr;
    size_t n = 0;
    bool container = false;
    int rc = ExtractCodestream(data, size, &storage, &cs, &n, &container);
    if (rc) return rc;
    Sequence s;
    memset(seq, 0, sizeof(*seq));
    seq->why = "";
    if ((rc = WalkSequence(cs, n, &s, (flags & JXLHIP_SEQUENCE_EXTRA_CHANNELS) != 0))) {
      if (rc == JXLHIP_ERR_UNSUPPORTED) seq->why = s.h.why[0] ? s.h.why : "stream uses features outside the VarDCT back-end";
      return rc;
    }
    FillSequenceInfo(s, container, info, seq);
    return JXLHIP_OK;
  } catch (const std::bad_alloc&) {
    return JXLHIP_ERR_OUT_OF_MEMORY;
  }
}

int jxlhip_decode_codestream_next(jxlhip_ctx* c, jxlhip_parallel_runner runner, void* runner_opaque, const uint8_t* data,
                                  size_t size, uint64_t* cursor, uint32_t output_kind, const jxlhip_output_format* out_format,
                                  void* out, size_t out_stride, size_t out_plane_stride, jxlhip_codestream_info* info_out,
                                  jxlhip_sequence_frame* frame_out) {
  try {
    const int rc = SequenceNextImpl(c, runner, runner_opaque, data, size, cursor, output_kind, out_format, out, out_stride,
                                    out_plane_stride, info_out, frame_out);
    // an early return may leave uploads of a frame queued: nothing of it may still be in flight when the caller frees
    // its buffers
    if (rc != JXLHIP_OK && c && !c->multi && c->stream) (void)hipStreamSynchronize(c->stream);
    return rc;
  } catch (const std::bad_alloc&) {
    return c ? Fail(c, JXLHIP_ERR_OUT_OF_MEMORY, "host allocation failed while decoding the codestream") : JXLHIP_ERR_OUT_OF_MEMORY;
  }
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
int ReadPartial(const uint8_t* data, size_t size, std::vector<uint8_t>* storage, const uint8_t** cs, size_t* n, bool* container,
                ParsedHeaders* h, PartialPlan* plan, const char** why) {
  *why = "";
  int rc = ExtractCodestream(data, size, storage, cs, n, container, true);
  if (rc) return rc;
  // headers that end early do not parse: which of the two it is only more bytes can tell
  rc = ParseHeaders(*cs, *n, h);
  if (rc == JXLHIP_ERR_BAD_STREAM) return JXLHIP_ERR_NEED_MORE_INPUT;
  if (rc == JXLHIP_ERR_UNSUPPORTED) *why = h->why[0] ? h->why : "stream uses features outside the VarDCT back-end";
  if (rc) return rc;
  if ((rc = PlanPartial(*cs, *n, *h, plan)) == JXLHIP_ERR_UNSUPPORTED) *why = "frame too large";
  return rc;
}

}  // namespace

int jxlhip_codestream_partial_info(const uint8_t* data, size_t size, jxlhip_codestream_info* info, jxlhip_partial_info* partial) {
  if (!data || !partial) return JXLHIP_ERR_INVALID_ARGUMENT;
  try {
    std::vector<uint8_t> storage;
    const uint8_t* cs = nullptr;
    size_t n = 0;
    bool container = false;
    ParsedHeaders h;
    PartialPlan plan;
    const char* why;
    const int rc = ReadPartial(data, size, &storage, &cs, &n, &container, &h, &plan, &why);
    if (rc) return rc;
    if (info) FillInfo(h, container, info);
    *partial = plan.info;
    return JXLHIP_OK;
  } catch (const std::bad_alloc&) {
    return JXLHIP_ERR_OUT_OF_MEMORY;
  }
}

static int DecodePartialImpl(jxlhip_ctx* c, jxlhip_parallel_runner runner, void* runner_opaque, const uint8_t* data, size_t size,
                             uint32_t output_kind, const jxlhip_output_format* out_format, void* out, size_t out_stride,
                             size_t out_plane_stride, jxlhip_codestream_info* info_out, jxlhip_partial_info* partial_out) {
  const bool undo_orientation = (output_kind & JXLHIP_OUT_UNDO_ORIENTATION) != 0;
  const uint32_t kind = output_kind & ~(uint32_t)JXLHIP_OUT_UNDO_ORIENTATION;
  if (!c || !data || !out || kind > JXLHIP_OUT_PACKED || (kind == JXLHIP_OUT_PACKED && !out_format)) return JXLHIP_ERR_INVALID_ARGUMENT;
  JXLHIP_NO_MULTI(c);
  std::vector<uint8_t> storage;
  const uint8_t* cs = nullptr;
  size_t n = 0;
  bool container = false;
  ParsedHeaders h;
  PartialPlan plan;
  const char* why;
  int rc = ReadPartial(data, size, &storage, &cs, &n, &container, &h, &plan, &why);
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
  if (h.ih.num_extra_channels != 0 && kind == JXLHIP_OUT_PACKED && out_format->num_channels == 4)
    return Fail(c, JXLHIP_ERR_UNSUPPORTED, "a partial file of an image with extra channels into a 4-channel output");
  for (uint32_t slot = 0; slot < 4; slot++)
    if ((rc = jxlhip_set_reference_frame(c, slot, 0, 0, nullptr, 0, 0))) return rc;
  PhaseClock clock(c->cs_phase_ms);
  const bool verbose = jxlhip_env::Get().codestream_verbose.load(std::memory_order_relaxed);
  g_upload_wait_on.store(verbose);
  if ((rc = ApplyDisplay(c, &h))) return rc;
  jxlhip_codestream_info info;
  FillInfo(h, container, &info);
  FrameCall fc;
  fc.runner = runner;
  fc.runner_opaque = runner_opaque;
  fc.output_kind = kind;
  fc.undo_orientation = undo_orientation;
  fc.out_format = out_format;
  fc.out = out;
  fc.out_stride = out_stride;
  fc.out_plane_stride = out_plane_stride;
  fc.out_xsize = h.ih.xsize;
  fc.out_ysize = h.ih.ysize;
  fc.partial = &plan;
  if ((rc = DecodeFrameAt(c, cs, n, h, h.fh, h.frame_bit_pos, fc, clock, verbose, &info, nullptr))) return rc;
  if (info_out) *info_out = info;
  if (partial_out) *partial_out = plan.info;
  return JXLHIP_OK;
}

int jxlhip_decode_codestream_partial(jxlhip_ctx* c, jxlhip_parallel_runner runner, void* runner_opaque, const uint8_t* data,
                                     size_t size, uint32_t output_kind, const jxlhip_output_format* out_format, void* out,
                                     size_t out_stride, size_t out_plane_stride, jxlhip_codestream_info* info_out,
                                     jxlhip_partial_info* partial_out) {
  try {
    const int rc = DecodePartialImpl(c, runner, runner_opaque, data, size, output_kind, out_format, out, out_stride,
                                     out_plane_stride, info_out, partial_out);
    // (as jxlhip_decode_codestream_extra: nothing of an abandoned frame may still be in flight)
    if (rc != JXLHIP_OK && c && !c->multi && c->stream) (void)hipStreamSynchronize(c->stream);
    return rc;
  } catch (const std::bad_alloc&) {
    return c ? Fail(c, JXLHIP_ERR_OUT_OF_MEMORY, "host allocation failed while decoding the codestream") : JXLHIP_ERR_OUT_OF_MEMORY;
  }
}
