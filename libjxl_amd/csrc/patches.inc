// patches.inc -- patches in the host front-end (included by entropy.cc, behind the entropy decoder it uses): the
// dictionary at the head of a patch frame's DC-global section, and the same object from a caller's list.
//
// Replaces (behaviour, not code): lib/jxl/dec_patch_dictionary.cc -- PatchDictionary::Decode (:31-178) with the contexts
// of lib/jxl/patch_dictionary_internal.h and UsesAlpha / UsesClamp (dec_patch_dictionary.h:72-80).  The patch tree of
// ComputePatchTree is not built: the back-end bins the patches by tile (jxlhip_set_patches).

struct jxlhip_patches {
  uint32_t num_extra_channels = 0;
  bool uses_extra_channels = false;
  std::vector<jxlhip_patch> patches;
  std::vector<uint32_t> ec;  // per patch and extra channel: mode, alpha_channel, clamp
};

namespace {

// patch_dictionary_internal.h:12-24
enum : uint32_t {
  kPatNumRefPatchCtx = 0,
  kPatReferenceFrameCtx,
  kPatSizeCtx,
  kPatReferencePositionCtx,
  kPatPositionCtx,
  kPatBlendModeCtx,
  kPatOffsetCtx,
  kPatCountCtx,
  kPatAlphaChannelCtx,
  kPatClampCtx,
  kPatCtxs
};
constexpr uint32_t kPatNumBlendModes = 8, kPatMaxReferenceFrames = 4;

inline bool PatUsesAlpha(uint32_t mode) { return mode >= JXLHIP_PATCH_BLEND_ABOVE && mode < kPatNumBlendModes; }
inline bool PatUsesClamp(uint32_t mode) { return PatUsesAlpha(mode) || mode == JXLHIP_PATCH_MUL; }

struct PatLimits {
  uint64_t max_ref_patches, max_patches, max_blendings;
  PatLimits(uint64_t xsize, uint64_t ysize) {
    max_ref_patches = 1024 + xsize * ysize / 4;  // "about 66 bytes per pixel" (:50-55)
    max_patches = max_ref_patches * 4;
    max_blendings = max_patches * 4;
  }
};

// what Decode checks of one reference rectangle (:66-84); the slot sizes stand for the reference frames
bool PatRefOk(uint64_t ref, uint64_t x0, uint64_t y0, uint64_t xs, uint64_t ys, const uint32_t ref_sizes[4][2]) {
  if (ref >= kPatMaxReferenceFrames || ref_sizes[ref][0] == 0 || ref_sizes[ref][1] == 0) return false;
  return x0 + xs <= ref_sizes[ref][0] && y0 + ys <= ref_sizes[ref][1];
}

// one blending (:137-164): false where Decode fails; the object's uses_extra_channels follows the image, not the
// decoder's flag: an alpha mode counts when the image has extra channels (without them PerformBlending falls back to
// kAdd / kReplace, blending.cc:150-184), an extra channel counts with every mode but kNone
bool PatBlendingOk(jxlhip_patches* s, uint32_t j, uint32_t mode, uint32_t alpha_channel) {
  if (mode >= kPatNumBlendModes) return false;
  if (PatUsesAlpha(mode) && s->num_extra_channels > 0) s->uses_extra_channels = true;
  if (mode != JXLHIP_PATCH_NONE && j > 0) s->uses_extra_channels = true;
  if (PatUsesAlpha(mode) && s->num_extra_channels > 1 && alpha_channel >= s->num_extra_channels) return false;
  return true;
}

}  // namespace

int jxlhip_patches_decode(const uint8_t* data, size_t size, size_t* bit_pos, uint32_t xsize, uint32_t ysize,
                          uint32_t num_extra_channels, const uint32_t ref_sizes[4][2], jxlhip_patches** out) {
  if (!data || !bit_pos || !ref_sizes || !out) return JXLHIP_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  try {
    BitReader br(data, size, *bit_pos);
    EntropyCode code;
    int rc = DecodeEntropyCode(&br, kPatCtxs, &code, /*disallow_lz77=*/false, 0);
    if (rc) return rc;
    if (!br.Healthy()) return kBad;
    SymbolReader reader(&code, &br);
    if (!reader.Ok()) return JXLHIP_ERR_OUT_OF_MEMORY;
    const std::vector<uint8_t>& cmap = code.context_map;
    auto read_num = [&](uint32_t ctx) -> uint64_t { return reader.ReadHybridUint(cmap[ctx], &br); };
    std::unique_ptr<jxlhip_patches> s(new jxlhip_patches);
    s->num_extra_channels = num_extra_channels;
    const PatLimits lim(xsize, ysize);
    const uint64_t stride = (uint64_t)num_extra_channels + 1;
    const uint64_t num_ref_patch = read_num(kPatNumRefPatchCtx);
    if (num_ref_patch > lim.max_ref_patches) return kBad;
    uint64_t total = 0, next_size = 1;
    for (uint64_t id = 0; id < num_ref_patch; id++) {
      const uint64_t ref = read_num(kPatReferenceFrameCtx);
      if (ref >= kPatMaxReferenceFrames || ref_sizes[ref][0] == 0 || ref_sizes[ref][1] == 0) return kBad;
      const uint64_t rx = read_num(kPatReferencePositionCtx), ry = read_num(kPatReferencePositionCtx);
      const uint64_t xs = read_num(kPatSizeCtx) + 1, ys = read_num(kPatSizeCtx) + 1;
      if (!PatRefOk(ref, rx, ry, xs, ys, ref_sizes)) return kBad;
      uint64_t count = read_num(kPatCountCtx);
      if (count > lim.max_patches) return kBad;
      count++;
      total += count;
      if (total > lim.max_patches) return kBad;
      if (next_size < total) next_size = std::min(next_size * 2, lim.max_patches);
      if (next_size * stride > lim.max_blendings) return kBad;
      if (!br.Healthy() || reader.Corrupt()) return kBad;  // (nothing is allocated for counts read past the end)
      for (uint64_t i = 0; i < count; i++) {
        jxlhip_patch p{};
        p.ref = (uint32_t)ref;
        p.ref_x0 = (uint32_t)rx;
        p.ref_y0 = (uint32_t)ry;
        p.xsize = (uint32_t)xs;
        p.ysize = (uint32_t)ys;
        uint64_t x, y;
        if (i == 0) {
          x = read_num(kPatPositionCtx);
          y = read_num(kPatPositionCtx);
        } else {
          const jxlhip_patch& last = s->patches.back();
          const int64_t dx = SplUnpackSigned((uint32_t)read_num(kPatOffsetCtx));
          if (dx < 0 && (uint64_t)-dx > last.x) return kBad;
          x = (uint64_t)((int64_t)last.x + dx);
          const int64_t dy = SplUnpackSigned((uint32_t)read_num(kPatOffsetCtx));
          if (dy < 0 && (uint64_t)-dy > last.y) return kBad;
          y = (uint64_t)((int64_t)last.y + dy);
        }
        if (x + xs > xsize || y + ys > ysize) return kBad;
        p.x = (uint32_t)x;
        p.y = (uint32_t)y;
        for (uint32_t j = 0; j < stride; j++) {
          const uint32_t mode = (uint32_t)read_num(kPatBlendModeCtx);
          if (mode >= kPatNumBlendModes) return kBad;
          uint32_t alpha = 0, clamp = 0;
          if (PatUsesAlpha(mode) && num_extra_channels > 1) alpha = (uint32_t)read_num(kPatAlphaChannelCtx);
          if (!PatBlendingOk(s.get(), j, mode, alpha)) return kBad;
          if (PatUsesClamp(mode)) clamp = read_num(kPatClampCtx) != 0;
          if (j == 0) {
            p.mode = mode;
            p.alpha_channel = alpha;
            p.clamp = clamp;
          } else {
            s->ec.insert(s->ec.end(), {mode, alpha, clamp});
          }
        }
        s->patches.push_back(p);
        if (!br.Healthy() || reader.Corrupt()) return kBad;
      }
    }
    if (!br.Healthy() || reader.Corrupt() || !reader.FinalStateOk()) return kBad;
    *bit_pos = br.BitsConsumed();
    *out = s.release();
    return kOk;
  } catch (const std::bad_alloc&) {
    return JXLHIP_ERR_OUT_OF_MEMORY;
  }
}

int jxlhip_patches_from_list(uint32_t num_patches, const jxlhip_patch* patches, uint32_t num_extra_channels,
                             const uint32_t* ec_blendings, uint32_t xsize, uint32_t ysize,
                             const uint32_t ref_sizes[4][2], jxlhip_patches** out) {
  if (!out || !ref_sizes || (num_patches && (!patches || (num_extra_channels && !ec_blendings))))
    return JXLHIP_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  const PatLimits lim(xsize, ysize);
  if (num_patches > lim.max_patches || (uint64_t)num_patches * (num_extra_channels + 1ull) > lim.max_blendings) return kBad;
  try {
    std::unique_ptr<jxlhip_patches> s(new jxlhip_patches);
    s->num_extra_channels = num_extra_channels;
    for (uint32_t i = 0; i < num_patches; i++) {
      const jxlhip_patch& p = patches[i];
      if (p.xsize == 0 || p.ysize == 0 || !PatRefOk(p.ref, p.ref_x0, p.ref_y0, p.xsize, p.ysize, ref_sizes)) return kBad;
      if ((uint64_t)p.x + p.xsize > xsize || (uint64_t)p.y + p.ysize > ysize) return kBad;
      if (!PatBlendingOk(s.get(), 0, p.mode, p.alpha_channel)) return kBad;
      for (uint32_t j = 0; j < num_extra_channels; j++) {
        const uint32_t* e = ec_blendings + 3 * ((size_t)i * num_extra_channels + j);
        if (!PatBlendingOk(s.get(), j + 1, e[0], e[1])) return kBad;
      }
    }
    s->patches.assign(patches, patches + num_patches);
    for (jxlhip_patch& p : s->patches) p.clamp = PatUsesClamp(p.mode) && p.clamp;  // (as Decode: read only for those modes)
    s->ec.assign(ec_blendings, ec_blendings + 3 * (size_t)num_patches * num_extra_channels);
    *out = s.release();
    return kOk;
  } catch (const std::bad_alloc&) {
    return JXLHIP_ERR_OUT_OF_MEMORY;
  }
}

int jxlhip_patches_list(const jxlhip_patches* s, uint32_t* num_patches, uint32_t* num_extra_channels,
                        uint32_t* uses_extra_channels, jxlhip_patch* patches, uint32_t* ec_blendings) {
  if (!s || !num_patches) return JXLHIP_ERR_INVALID_ARGUMENT;
  *num_patches = (uint32_t)s->patches.size();
  if (num_extra_channels) *num_extra_channels = s->num_extra_channels;
  if (uses_extra_channels) *uses_extra_channels = s->uses_extra_channels;
  if (patches && !s->patches.empty()) memcpy(patches, s->patches.data(), s->patches.size() * sizeof(jxlhip_patch));
  if (ec_blendings && !s->ec.empty()) memcpy(ec_blendings, s->ec.data(), s->ec.size() * sizeof(uint32_t));
  return kOk;
}

void jxlhip_patches_destroy(jxlhip_patches* s) { delete s; }
