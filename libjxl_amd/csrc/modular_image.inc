// modular_image.inc -- a regular Modular frame on the host (jxlhip_modular_image_decode[_channels],
// include/jxl_hip_frame.h; the stages of modular_image.h).  Textually included by entropy.cc behind modular.inc, whose decode loop, transforms and
// global image (ModularFull) it uses.  Host code, written from the format as the libjxl tree implements it (lib/jxl/):
//   FrameDecoder::ProcessDCGlobal / ProcessDCGroup / ProcessACGroup of a Modular frame   dec_frame.cc:268-342,455-530
//   ModularFrameDecoder::DecodeGlobalInfo / DecodeGroup                                  dec_modular.cc:207-316,330-425
//   Transform (RCT) and its inverse                                                      modular/transform/transform.cc:36-90, rct.cc:29-148
// What the reference does behind them -- FinalizeDecoding's undo of the global transforms and ModularImageToDecodedRect's
// int -> float (dec_modular.cc:564-632,739-790) -- is split between this file and the device: see the header.
#include "modular_image.h"

namespace jxlhip {

struct ModularImage {
  jxlhip_modular_tree tree;  // the global tree, and in tree.full the global image: the colour channels (three, or one
                             // of a grey image), then the image's extra channels
  jxlhip_frame_header fh;
  jxlhip_modular_image_channels* out = nullptr;
  uint32_t nch = 3;  // num_color + num_extra
  // the global list stays with the host: the groups collect into tree.full (int32) and ModularImageFinish undoes it.
  // Otherwise a group writes its samples straight into the planes.
  bool collect = false;
  std::atomic<uint32_t> on_device{0}, on_host{0};
  std::atomic<bool> range{false};
};

namespace {

// channel c of the global image: a colour plane, or behind them an extra channel's
void* PlaneOf(const jxlhip_modular_image_channels& o, uint32_t c) {
  return c < o.num_color ? o.planes[c] : o.extra_planes[c - o.num_color];
}

// the caller's struct against the frame header (the header has passed ModularImageChannelsRefusal)
bool BadChannels(const jxlhip_frame_header* fh, const jxlhip_modular_image_channels& o) {
  if (!o.group_rct || o.stride_samples < fh->xsize || o.sample_type > JXLHIP_MODULAR_I32 || (o.num_color != 1 && o.num_color != 3) ||
      o.num_extra != fh->num_extra_channels)
    return true;
  for (uint32_t c = 0; c < o.num_color + o.num_extra; c++)
    if (!PlaneOf(o, c)) return true;
  for (uint32_t e = 0; e < o.num_extra; e++)
    if (o.extra_bits[e] == 0 || o.extra_bits[e] > 16) return true;
  return false;
}

// rows of int32 samples into the caller's planes; false: a sample does not fit 16 bits
bool StoreRows(const jxlhip_modular_image_channels& o, uint32_t c, uint32_t x0, uint32_t y0, const ModularChannel& ch) {
  bool fits = true;
  void* const plane = PlaneOf(o, c);
  for (uint32_t y = 0; y < ch.h; y++) {
    const int32_t* in = ch.Row(y);
    const size_t at = (size_t)(y0 + y) * o.stride_samples + x0;
    if (o.sample_type == JXLHIP_MODULAR_I32) {
      memcpy((int32_t*)plane + at, in, ch.w * sizeof(int32_t));
    } else {
      int16_t* d = (int16_t*)plane + at;
      int32_t bad = 0;
      for (uint32_t x = 0; x < ch.w; x++) {
        d[x] = (int16_t)in[x];
        bad |= in[x] ^ (int32_t)d[x];
      }
      fits = fits && bad == 0;
    }
  }
  return fits;
}

}  // namespace

static const char* FrameRefusal(const jxlhip_frame_header* fh, bool extra_channels) {
  if (!fh->is_modular) return "a VarDCT frame";
  if (fh->frame_type != JXLHIP_FRAME_REGULAR || fh->dc_level != 0) return "a Modular frame that is not a regular frame";
  if (fh->color_transform == JXLHIP_CT_XYB) return "an XYB Modular regular frame";
  if (fh->color_transform != JXLHIP_CT_NONE) return "a YCbCr Modular regular frame";
  if (fh->chroma_mode[0] || fh->chroma_mode[1] || fh->chroma_mode[2]) return "a chroma-subsampled Modular frame";
  if (fh->flags != 0) return "a Modular regular frame with flags (noise, patches, splines, a DC frame)";
  if (fh->lf.gab || fh->lf.epf_iters) return "a Modular regular frame with a loop filter";
  if (fh->upsampling != 1) return "an upsampled Modular regular frame";
  if (fh->num_passes != 1) return "a Modular regular frame of more than one pass";
  if (fh->num_extra_channels != 0 && !extra_channels) return "a Modular regular frame of an image with extra channels";
  if (fh->custom_size_or_origin) return "a cropped Modular regular frame";
  if (!extra_channels) return nullptr;
  if (fh->num_extra_channels > JXLHIP_MODULAR_MAX_EXTRA) return "a Modular regular frame of an image with more than four extra channels";
  for (uint32_t i = 0; i < fh->num_extra_channels; i++)
    if (fh->ec_upsampling[i] != 1) return "a Modular regular frame with a sub-sampled extra channel";
  // (one full-size frame: blending it over the empty canvas is the reference's business)
  if (fh->blend_mode != JXLHIP_BLEND_REPLACE) return "a Modular regular frame whose colour blend mode is not kReplace";
  if (fh->ec_blend_any) return "a Modular regular frame with an extra-channel blend mode other than kReplace";
  return nullptr;
}

const char* ModularImageRefusal(const jxlhip_frame_header* fh) { return FrameRefusal(fh, false); }
const char* ModularImageChannelsRefusal(const jxlhip_frame_header* fh) { return FrameRefusal(fh, true); }

int ModularImageBegin(const uint8_t* data, size_t size, size_t* bit_pos, const jxlhip_frame_header* fh,
                      jxlhip_modular_image_channels* out, ModularImage** image, const char** why) {
  auto refuse = [&](const char* what) {
    if (why) *why = what;
    return JXLHIP_ERR_UNSUPPORTED;
  };
  if (why) *why = "";
  if (!data || !bit_pos || !fh || !out || !image) return JXLHIP_ERR_INVALID_ARGUMENT;
  *image = nullptr;
  if (const char* what = ModularImageChannelsRefusal(fh)) return refuse(what);
  if (fh->xsize == 0 || fh->ysize == 0 || fh->num_groups == 0 || fh->num_groups > (1u << 22) || BadChannels(fh, *out))
    return JXLHIP_ERR_INVALID_ARGUMENT;
  const uint32_t nch = out->num_color + out->num_extra;
  if ((uint64_t)fh->xsize * fh->ysize * nch > ((uint64_t)1 << 32)) return JXLHIP_ERR_OUT_OF_MEMORY;
  try {
    std::unique_ptr<ModularImage> m(new ModularImage);
    m->fh = *fh;
    m->out = out;
    m->nch = nch;
    out->global_rct = 0;
    out->global_tree = out->global_on_host = out->groups_on_device = out->groups_on_host = 0;
    memset(out->group_rct, 0, (size_t)fh->num_groups * sizeof(uint16_t));
    BitReader br(data, size, *bit_pos);
    if (!br.Read(1)) {  // DequantMatrices::DecodeDC (quant_weights.cc:513-528): read, checked and of no use to this frame
      for (int i = 0; i < 3; i++) {
        float v;
        if (!ReadF16(&br, &v)) return kBad;
        if (v * (1.0f / 128.0f) < 1e-8f) return kBad;
      }
    }
    if (!br.Healthy()) return kBad;
    if (br.Read(1)) {
      const uint64_t limit = std::min<uint64_t>(1u << 22, 1024 + (uint64_t)fh->xsize * fh->ysize * nch / 16);
      const int rc = DecodeMaTree(&br, (size_t)limit, &m->tree);
      if (rc == JXLHIP_ERR_UNSUPPORTED) return refuse("the MA tree of the Modular frame");
      if (rc) return rc;
      out->global_tree = 1;
    }
    m->tree.full = std::make_shared<ModularFull>();
    ModularFull& f = *m->tree.full;
    f.group_dim = fh->group_dim;
    f.xsg = fh->xsize_groups;
    f.num_groups = (uint32_t)fh->num_groups;
    f.num_dc_groups = (uint32_t)fh->num_dc_groups;
    f.image_bits = fh->image_bits;
    f.ch.resize(nch);
    const bool large = fh->xsize > fh->group_dim || fh->ysize > fh->group_dim;
    for (ModularChannel& c : f.ch) {
      if (large) c.Shape(fh->xsize, fh->ysize);  // left to the groups
      else c.Resize(fh->xsize, fh->ysize);
    }
    ModularStreamOptions opt;
    opt.rct = opt.lz77 = true;
    opt.leave_rcts = out->num_color == 3;  // (a grey image has no three colour channels: its lists are undone here)
    opt.channels = nch;
    const char* where = "a Modular feature outside this front-end";
    const int rc = ModularDecodeImage(&br, f.ch, 0, &m->tree, fh->group_dim, fh->image_bits, &f.pending, nullptr, true, &where, &opt);
    if (rc == JXLHIP_ERR_UNSUPPORTED) return refuse(where);
    if (rc) return rc;
    if (f.pending.squeeze.present) return refuse("a squeeze on the colour channels");
    if (!br.Healthy()) return kBad;
    if (opt.left) out->global_rct = opt.program;
    // (a one-group frame whose list the host had to undo is complete by now: ModularDecodeImage has undone it)
    out->global_on_host = opt.transforms && !opt.left;
    m->collect = !f.pending.palettes.empty();
    *bit_pos = br.BitsConsumed();
    *image = m.release();
    return kOk;
  } catch (const std::bad_alloc&) {
    return JXLHIP_ERR_OUT_OF_MEMORY;
  }
}

// ModularFrameDecoder::DecodeGroup (dec_modular.cc:330-425) over the rectangle (x0, y0, dim x dim) with the shift bracket
// [min_shift, max_shift]
static int ModularImageGroup(ModularImage* m, uint32_t x0, uint32_t y0, uint32_t dim, int min_shift, int max_shift,
                             uint32_t stream_id, int64_t group, const uint8_t* data, size_t size, size_t* bit_pos) {
  try {
    ModularFull& f = *m->tree.full;
    std::vector<ModularChannel> gi;
    std::vector<uint32_t> which;
    ModularStreamOptions opt;
    opt.rct = opt.lz77 = true;
    opt.leave_rcts = !m->collect && m->out->num_color == 3;
    opt.channels = m->nch;
    const int rc = ModularGroupRects(&m->tree, x0, y0, dim, min_shift, max_shift, stream_id, data, size, bit_pos, &gi, &which, &opt);
    if (rc || gi.empty()) return rc;
    if (m->collect) {
      ModularGroupCopy(f, x0, y0, gi, which);
    } else {
      // without pending global transforms the list is the image's channels, all of them in every group
      if (group < 0 || which.size() != m->nch) return kBad;
      for (uint32_t c = 0; c < m->nch; c++)
        if (which[c] != c) return kBad;
      for (uint32_t c = 0; c < m->nch; c++)
        if (!StoreRows(*m->out, c, x0, y0, gi[c])) m->range.store(true, std::memory_order_relaxed);
      if (opt.left) m->out->group_rct[group] = opt.program;
    }
    if (opt.left && opt.program) m->on_device.fetch_add(1, std::memory_order_relaxed);
    if (opt.transforms && !opt.left) m->on_host.fetch_add(1, std::memory_order_relaxed);
    return kOk;
  } catch (const std::bad_alloc&) {
    return JXLHIP_ERR_OUT_OF_MEMORY;
  }
}

int ModularImageDcGroup(ModularImage* m, uint32_t dc_group, const uint8_t* data, size_t size, size_t* bit_pos) {
  if (!m || !data || !bit_pos || dc_group >= m->fh.num_dc_groups) return JXLHIP_ERR_INVALID_ARGUMENT;
  const uint32_t dim = m->fh.group_dim * 8, xdg = (m->fh.xsize + dim - 1) / dim;
  // (channels of shift 3 and more: only a squeeze makes any, and that is refused -- the stream is empty)
  return ModularImageGroup(m, (dc_group % xdg) * dim, (dc_group / xdg) * dim, dim, 3, 1000,
                           1 + (uint32_t)m->fh.num_dc_groups + dc_group, -1, data, size, bit_pos);
}

int ModularImageAcGroup(ModularImage* m, uint32_t group, const uint8_t* data, size_t size, size_t* bit_pos) {
  if (!m || !data || !bit_pos || group >= m->fh.num_groups) return JXLHIP_ERR_INVALID_ARGUMENT;
  const ModularFull& f = *m->tree.full;
  int min_shift, max_shift;
  DownsamplingBracket(&m->fh, 0, &min_shift, &max_shift);
  return ModularImageGroup(m, (group % f.xsg) * f.group_dim, (group / f.xsg) * f.group_dim, f.group_dim, min_shift, max_shift,
                           1 + 3 * f.num_dc_groups + 17 + group, (int64_t)group, data, size, bit_pos);
}

int ModularImageFinish(ModularImage* m) {
  if (!m) return JXLHIP_ERR_INVALID_ARGUMENT;
  try {
    ModularFull& f = *m->tree.full;
    const bool in_full = m->collect || (m->fh.xsize <= m->fh.group_dim && m->fh.ysize <= m->fh.group_dim);
    if (m->collect) {
      f.AllocateLarge();  // (a frame none of whose groups carried anything)
      const int rc = UndoPalettes(f.ch, f.pending.palettes, &f.pending.nb_meta, f.image_bits);
      if (rc) return rc;
    }
    if (in_full) {
      if (f.pending.nb_meta != 0 || f.ch.size() != m->nch) return kBad;
      for (uint32_t c = 0; c < m->nch; c++) {
        const ModularChannel& ch = f.ch[c];
        if (ch.w != m->fh.xsize || ch.h != m->fh.ysize || ch.px.size() != (size_t)ch.w * ch.h) return kBad;
        if (!StoreRows(*m->out, c, 0, 0, ch)) m->range.store(true);
      }
    }
    m->out->groups_on_device = m->on_device.load();
    m->out->groups_on_host = m->on_host.load();
    return m->range.load() ? JXLHIP_ERR_RANGE : kOk;
  } catch (const std::bad_alloc&) {
    return JXLHIP_ERR_OUT_OF_MEMORY;
  }
}

void ModularImageDestroy(ModularImage* m) { delete m; }

}  // namespace jxlhip

namespace {
struct ModularImageJob {
  jxlhip::ModularImage* m;
  const uint8_t* base;
  const uint64_t* off;
  const uint32_t* sz;
  uint32_t ndc, ng;
  std::atomic<int> status{JXLHIP_OK};
};
int ModularImageJobInit(void*, size_t) { return 0; }
void ModularImageJobFunc(void* opaque, uint32_t t, size_t) {
  ModularImageJob* j = static_cast<ModularImageJob*>(opaque);
  if (j->status.load(std::memory_order_relaxed) != JXLHIP_OK) return;
  size_t pos = 0;
  const uint32_t s = t < j->ndc ? 1 + t : 2 + t;  // (section 1 + ndc is AC global: empty in a Modular frame)
  const int rc = t < j->ndc ? jxlhip::ModularImageDcGroup(j->m, t, j->base + j->off[s], j->sz[s], &pos)
                            : jxlhip::ModularImageAcGroup(j->m, t - j->ndc, j->base + j->off[s], j->sz[s], &pos);
  int expected = JXLHIP_OK;
  if (rc != JXLHIP_OK) j->status.compare_exchange_strong(expected, rc);
}
}  // namespace

int jxlhip_modular_image_decode_channels(const uint8_t* data, size_t size, size_t* bit_pos, const jxlhip_frame_header* fh,
                                         jxlhip_parallel_runner runner, void* runner_opaque,
                                         jxlhip_modular_image_channels* channels, const char** why) {
  if (why) *why = "";
  if (!data || !bit_pos || !fh || !channels) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (const char* what = jxlhip::ModularImageChannelsRefusal(fh)) {
    if (why) *why = what;
    return JXLHIP_ERR_UNSUPPORTED;
  }
  if (fh->num_toc_entries == 0 || fh->num_toc_entries > (1u << 24) || jxlhip::BadChannels(fh, *channels)) return JXLHIP_ERR_INVALID_ARGUMENT;
  try {
    const uint32_t ntoc = (uint32_t)fh->num_toc_entries, ndc = (uint32_t)fh->num_dc_groups, ng = (uint32_t)fh->num_groups;
    if (ntoc != 1 && ntoc != 2 + (uint64_t)ndc + ng) return JXLHIP_ERR_INVALID_ARGUMENT;
    std::vector<uint64_t> off(ntoc);
    std::vector<uint32_t> sz(ntoc);
    uint64_t total = 0;
    size_t pos = *bit_pos;
    int rc = jxlhip_toc_decode(data, size, &pos, ntoc, off.data(), sz.data(), &total);
    if (rc) return rc;
    const size_t base = pos / 8;
    if (total > size - base) return kBad;
    jxlhip::ModularImage* raw = nullptr;
    size_t spos = 0;
    if ((rc = jxlhip::ModularImageBegin(data + base + off[0], sz[0], &spos, fh, channels, &raw, why))) return rc;
    std::unique_ptr<jxlhip::ModularImage, void (*)(jxlhip::ModularImage*)> m(raw, jxlhip::ModularImageDestroy);
    if (ntoc == 1) {  // one section: the DC group, (AC global: nothing,) the AC group follow at the bit position
      if ((rc = jxlhip::ModularImageDcGroup(raw, 0, data + base + off[0], sz[0], &spos))) return rc;
      if ((rc = jxlhip::ModularImageAcGroup(raw, 0, data + base + off[0], sz[0], &spos))) return rc;
    } else {
      ModularImageJob job{raw, data + base, off.data(), sz.data(), ndc, ng};
      if (runner) {
        if (runner(runner_opaque, &job, ModularImageJobInit, ModularImageJobFunc, 0, ndc + ng) != 0) return JXLHIP_ERR_STATE;
      } else {
        for (uint32_t t = 0; t < ndc + ng; t++) ModularImageJobFunc(&job, t, 0);
      }
      if ((rc = job.status.load())) return rc;
    }
    if ((rc = jxlhip::ModularImageFinish(raw))) return rc;
    *bit_pos = (base + (size_t)total) * 8;
    return kOk;
  } catch (const std::bad_alloc&) {
    return JXLHIP_ERR_OUT_OF_MEMORY;
  }
}

// the three-plane entry: an RGB image without extra channels through the entry above
int jxlhip_modular_image_decode(const uint8_t* data, size_t size, size_t* bit_pos, const jxlhip_frame_header* fh,
                                jxlhip_parallel_runner runner, void* runner_opaque, jxlhip_modular_image_planes* planes,
                                const char** why) {
  if (why) *why = "";
  if (!data || !bit_pos || !fh || !planes) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (const char* what = jxlhip::ModularImageRefusal(fh)) {
    if (why) *why = what;
    return JXLHIP_ERR_UNSUPPORTED;
  }
  jxlhip_modular_image_channels ch{};
  ch.num_color = 3;
  for (int c = 0; c < 3; c++) ch.planes[c] = planes->planes[c];
  ch.stride_samples = planes->stride_samples;
  ch.sample_type = planes->sample_type;
  ch.group_rct = planes->group_rct;
  const int rc = jxlhip_modular_image_decode_channels(data, size, bit_pos, fh, runner, runner_opaque, &ch, why);
  planes->global_rct = ch.global_rct;
  planes->global_tree = ch.global_tree;
  planes->global_on_host = ch.global_on_host;
  planes->groups_on_device = ch.groups_on_device;
  planes->groups_on_host = ch.groups_on_host;
  return rc;
}
