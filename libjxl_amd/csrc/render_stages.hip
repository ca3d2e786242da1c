// render_stages.hip -- the render stages of a frame (noise, splines, patches, upsampling, DC-only groups, blending, tone
// mapping): their setters (StageState / SlotState, context.h) and the decode paths that run them around DecodeFrameCoded.
#include <math.h>
#include "context.h"
#include "upsampling_constants.inc"

// Photon noise of the current frame (FrameHeader::kNoise): NoiseParams::lut and the seed indices of
// PassesDecoderState; frame_begin resets to "no noise".  A LUT without an entry above 1e-3 is recorded as no noise,
// as AddNoiseStage skips it (noise.h:37-42).
int jxlhip_set_noise(jxlhip_ctx* c, const float lut[8], uint32_t visible_frame_index, uint32_t nonvisible_frame_index) {
  if (!c || !lut) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (c->multi) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "noise on a multi-device context");
  if (!c->have_frame) return Fail(c, JXLHIP_ERR_STATE, "set_noise before frame_begin");
  if (c->f.group_y0 != 0 || c->f.group_rows != c->f.ysg) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "noise with stripes");
  if (c->p.undo_orientation > 1) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "noise with undo_orientation %u", c->p.undo_orientation);
  if (c->st.dc_only.on) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "noise on a frame with DC-only groups");
  bool any = false;
  for (int i = 0; i < 8; i++) any = any || fabsf(lut[i]) > 1e-3f;
  c->st.noise.on = false;
  if (!any) return JXLHIP_OK;
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->st.noise.jump) {
    static const std::vector<uint32_t> table = [] {
      std::vector<uint32_t> t((size_t)kNoiseSegs * kNoiseJumpWords);
      NoiseJumpTable(t.data());
      return t;
    }();
    const int rc = c->st.noise.jump.Reserve(c, table.size());
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->st.noise.jump, table.data(), table.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  }
  memcpy(c->st.noise.lut, lut, sizeof(c->st.noise.lut));
  c->st.noise.visible = visible_frame_index;
  c->st.noise.nonvisible = nonvisible_frame_index;
  c->st.noise.on = true;
  return JXLHIP_OK;
}

// std::llround of a float as the reference's x86-64 build evaluates it: out-of-range and NaN arguments give INT64_MIN
static int64_t SplineRound(float v) { return fabsf(v) < 9.0e18f ? (int64_t)llroundf(v) : INT64_MIN; }

// Splines of the current frame (FrameHeader::kSplines): the draw list of Splines::InitializeDrawCache for the frame's
// size and base colour correlation, binned by 64 x 16 tile for k_splines; frame_begin resets to "no splines".
int jxlhip_set_splines(jxlhip_ctx* c, const jxlhip_splines* s) {
  if (!c) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (c->multi) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "splines on a multi-device context");
  if (!c->have_frame) return Fail(c, JXLHIP_ERR_STATE, "set_splines before frame_begin");
  if (c->f.group_y0 != 0 || c->f.group_rows != c->f.ysg) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "splines with stripes");
  if (c->p.undo_orientation > 1) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "splines with undo_orientation %u", c->p.undo_orientation);
  c->st.splines.on = false;
  if (!s) return JXLHIP_OK;
  if (c->st.dc_only.on) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "splines on a frame with DC-only groups");
  const uint32_t W = c->f.xsize, H = c->f.ysize;
  // an upsampled frame: the draw cache is made for the upsampled size (dec_frame.cc:304-308), the stage draws the
  // rows and columns of the coded frame
  const uint32_t DW = (uint32_t)OutCols(c), DH = c->st.ups.factor > 1 ? c->st.ups.ysize : H;
  HIPCHK(c, hipSetDevice(c->device));
  SplineStage& st = c->st.splines;
  size_t n = 0;
  int rc = st.tiles.WaitHostFree(c);
  if (rc) return rc;
  rc = jxlhip_splines_segments(s, DW, DH, c->p.cfl_base_x, c->p.cfl_base_b, nullptr, 0, &n);
  if (rc) return Fail(c, rc, "invalid splines");
  std::vector<jxlhip_spline_segment> segs(n);
  if (n && (rc = jxlhip_splines_segments(s, DW, DH, c->p.cfl_base_x, c->p.cfl_base_b, segs.data(), n, &n))) return Fail(c, rc, "invalid splines");
  // bin by tile: the column span of DrawSegment (splines.cc:116-125) clipped to the frame, the row span as computed
  std::vector<SplineSeg>& hs = st.host_segs;
  hs.clear();
  std::vector<TileRect> rects;
  for (const jxlhip_spline_segment& g : segs) {
    const int64_t start = SplineRound(g.center_x - g.maximum_distance);
    const int64_t end = SplineRound(g.center_x + g.maximum_distance);
    if (end < 0 || start >= (int64_t)W || g.y1 <= g.y0 || g.y0 >= (int64_t)H) continue;
    SplineSeg d;
    d.cx = g.center_x;
    d.cy = g.center_y;
    d.inv_sigma = g.inv_sigma;
    d.s4i = g.sigma_over_4_times_intensity;
    for (int k = 0; k < 3; k++) d.color[k] = g.color[k];
    d.y0 = g.y0;
    d.y1 = (int32_t)std::min<int64_t>(g.y1, (int64_t)H);
    d.x0 = (int32_t)std::max<int64_t>(start, 0);
    d.x1 = (int32_t)std::min<int64_t>(end, (int64_t)W - 1);
    d.pad = 0.0f;
    hs.push_back(d);
    rects.push_back({(uint32_t)d.x0, (uint32_t)d.y0, (uint32_t)d.x1 + 1, (uint32_t)d.y1});  // (x1 is the last column)
  }
  if (!BinTiles(rects.data(), rects.size(), W, H, &st.tiles.host)) return Fail(c, JXLHIP_ERR_OUT_OF_MEMORY, "spline draw list too long");
  if (st.tiles.host.entries == 0) return JXLHIP_OK;  // nothing reaches the frame: the spline-free path
  if ((rc = st.segs.Reserve(c, hs.size()))) return rc;
  HIPCHK(c, hipMemcpyAsync(st.segs, hs.data(), hs.size() * sizeof(SplineSeg), hipMemcpyHostToDevice, c->stream));
  if ((rc = st.tiles.Upload(c, c->stream))) return rc;
  c->st.splines.on = true;
  return JXLHIP_OK;
}

// A reference frame for patches: three XYB planes into slot `slot` of the context (dense, xsize floats per row).
int jxlhip_set_reference_frame(jxlhip_ctx* c, uint32_t slot, uint32_t xsize, uint32_t ysize, const float* const planes[3],
                               size_t stride_floats, int on_device) {
  if (!c || slot > 3) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (c->multi) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "reference frames on a multi-device context");
  c->slots.ref_serial++;  // (an uploaded dictionary points into the slots: DecodeFrameFeatures refuses it from here on)
  c->seq_open = false;  // (a sequence of jxlhip_decode_codestream_next must not go on over slots emptied behind its back)
  c->slots.canvas_w[slot] = c->slots.canvas_h[slot] = 0;  // (a slot holds one kind: an XYB frame drops the canvas)
  c->slots.canvas_nec[slot] = 0;                     // (... and its extra-channel planes)
  if (xsize == 0 || ysize == 0) {  // cleared; the memory stays for the next frame of the slot
    c->slots.ref_w[slot] = c->slots.ref_h[slot] = 0;
    return JXLHIP_OK;
  }
  if (!planes || !planes[0] || !planes[1] || !planes[2]) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "null reference plane");
  if (stride_floats < xsize) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "reference stride %zu < xsize", stride_floats);
  HIPCHK(c, hipSetDevice(c->device));
  c->slots.ref_w[slot] = c->slots.ref_h[slot] = 0;
  const size_t plane = (size_t)xsize * ysize;
  HIPCHK(c, hipStreamSynchronize(c->stream));  // an earlier frame's k_patches may still read the slot
  const int rc = c->slots.ref_planes[slot].Reserve(c, 3 * plane);
  if (rc) return rc;
  for (int k = 0; k < 3; k++)
    HIPCHK(c, hipMemcpy2DAsync(c->slots.ref_planes[slot] + k * plane, xsize * sizeof(float), planes[k], stride_floats * sizeof(float),
                               xsize * sizeof(float), ysize, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // (the caller's planes are free when this returns)
  c->slots.ref_w[slot] = xsize;
  c->slots.ref_h[slot] = ysize;
  return JXLHIP_OK;
}

// Patches of the current frame (FrameHeader::kPatches): the dictionary as records of k_patches, binned by 64 x 16 tile
// in dictionary order; frame_begin resets to "no patches".
int jxlhip_set_patches(jxlhip_ctx* c, const jxlhip_patches* s) {
  if (!c) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (c->multi) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "patches on a multi-device context");
  if (!c->have_frame) return Fail(c, JXLHIP_ERR_STATE, "set_patches before frame_begin");
  if (c->f.group_y0 != 0 || c->f.group_rows != c->f.ysg) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "patches with stripes");
  if (c->p.undo_orientation > 1) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "patches with undo_orientation %u", c->p.undo_orientation);
  c->st.patches.on = false;
  if (!s) return JXLHIP_OK;
  uint32_t n = 0, nec = 0, uses_ec = 0;
  int rc = jxlhip_patches_list(s, &n, &nec, &uses_ec, nullptr, nullptr);
  if (rc) return Fail(c, rc, "invalid patch dictionary");
  if (n == 0) return JXLHIP_OK;  // nothing reaches the frame: the plain path
  if (c->st.dc_only.on) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "patches on a frame with DC-only groups");
  if (uses_ec) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "patches that blend extra channels");
  if (c->fp.alpha) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "patches on a frame with alpha (they would have to blend it)");
  std::vector<jxlhip_patch> list(n);
  if ((rc = jxlhip_patches_list(s, &n, nullptr, nullptr, list.data(), nullptr))) return Fail(c, rc, "invalid patch dictionary");
  const uint32_t W = c->f.xsize, H = c->f.ysize;
  const uint64_t WP = ((uint64_t)W + 7) & ~7ull, HP = ((uint64_t)H + 7) & ~7ull;  // FrameDimensions::xsize_padded
  HIPCHK(c, hipSetDevice(c->device));
  PatchStage& st = c->st.patches;
  if ((rc = st.tiles.WaitHostFree(c))) return rc;
  std::vector<PatchRec>& hr = st.host_recs;
  hr.clear();
  std::vector<TileRect> rects;
  for (uint32_t i = 0; i < n; i++) {
    const jxlhip_patch& p = list[i];
    if (p.ref <= 3 && c->slots.canvas_w[p.ref] != 0)
      return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "patch %u: slot %u holds a frame saved after the colour transform", i, p.ref);
    if (p.ref > 3 || c->slots.ref_w[p.ref] == 0) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "patch %u: reference slot %u is empty", i, p.ref);
    const uint32_t rw = c->slots.ref_w[p.ref], rh = c->slots.ref_h[p.ref];
    if (p.xsize == 0 || p.ysize == 0 || (uint64_t)p.ref_x0 + p.xsize > rw || (uint64_t)p.ref_y0 + p.ysize > rh)
      return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "patch %u: %ux%u at (%u, %u) leaves the %ux%u frame of slot %u", i, p.xsize,
                  p.ysize, p.ref_x0, p.ref_y0, rw, rh, p.ref);
    if ((uint64_t)p.x + p.xsize > WP || (uint64_t)p.y + p.ysize > HP)
      return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "patch %u: %ux%u at (%u, %u) leaves the frame", i, p.xsize, p.ysize, p.x, p.y);
    if (p.mode > 7) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "patch %u: blend mode %u", i, p.mode);
    if (p.mode == JXLHIP_PATCH_NONE || p.x >= W || p.y >= H) continue;  // the frame keeps its samples
    PatchRec r;
    r.x0 = (int32_t)p.x;
    r.y0 = (int32_t)p.y;
    r.x1 = (int32_t)std::min<uint64_t>((uint64_t)p.x + p.xsize, W);
    r.y1 = (int32_t)std::min<uint64_t>((uint64_t)p.y + p.ysize, H);
    r.src = c->slots.ref_planes[p.ref] + (size_t)p.ref_y0 * rw + p.ref_x0;
    r.stride = rw;
    r.plane = rw * rh;
    // PerformBlending's colour modes without an alpha channel (blending.cc:150-184)
    r.op = p.mode == JXLHIP_PATCH_MUL ? (p.clamp ? kPatchOpMulClamp : kPatchOpMul)
           : (p.mode == JXLHIP_PATCH_ADD || p.mode >= JXLHIP_PATCH_ALPHA_WEIGHTED_ADD_ABOVE) ? kPatchOpAdd : kPatchOpReplace;
    r.pad = 0;
    hr.push_back(r);
    rects.push_back({(uint32_t)r.x0, (uint32_t)r.y0, (uint32_t)r.x1, (uint32_t)r.y1});
  }
  if (!BinTiles(rects.data(), rects.size(), W, H, &st.tiles.host)) return Fail(c, JXLHIP_ERR_OUT_OF_MEMORY, "patch list too long");
  if (st.tiles.host.entries == 0) return JXLHIP_OK;
  if ((rc = st.recs.Reserve(c, hr.size()))) return rc;
  HIPCHK(c, hipMemcpyAsync(st.recs, hr.data(), hr.size() * sizeof(PatchRec), hipMemcpyHostToDevice, c->stream));
  if ((rc = st.tiles.Upload(c, c->stream))) return rc;
  c->st.patches.ref_serial = c->slots.ref_serial;
  c->st.patches.on = true;
  return JXLHIP_OK;
}

// Upsampling of the current frame (FrameHeader::upsampling): the factor, its kernels (UpsamplingStage's constructor on
// the coded or the default weights) and the size the frame comes out at; frame_begin resets to "not upsampled".
int jxlhip_set_upsampling(jxlhip_ctx* c, uint32_t factor, const float* weights, uint32_t out_xsize, uint32_t out_ysize) {
  if (!c) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (c->multi) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "upsampling on a multi-device context");
  if (!c->have_frame) return Fail(c, JXLHIP_ERR_STATE, "set_upsampling before frame_begin");
  if (factor != 1 && factor != 2 && factor != 4 && factor != 8) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "upsampling factor %u", factor);
  if (factor == 1) {
    // (a draw list made for the upsampled size must not outlive it)
    if (c->st.ups.factor > 1 && c->st.splines.on) return Fail(c, JXLHIP_ERR_STATE, "set_upsampling after set_splines (the draw list depends on it)");
    c->st.ups.factor = 1;
    return JXLHIP_OK;
  }
  if (c->f.group_y0 != 0 || c->f.group_rows != c->f.ysg) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "upsampling with stripes");
  if (c->p.undo_orientation > 1) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "upsampling with undo_orientation %u", c->p.undo_orientation);
  if (c->fp.alpha) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "alpha on an upsampled frame");
  if (c->st.splines.on) return Fail(c, JXLHIP_ERR_STATE, "set_upsampling after set_splines (the draw list depends on it)");
  if (c->st.dc_only.on) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "upsampling on a frame with DC-only groups");
  if (out_xsize == 0 || out_ysize == 0 || (out_xsize + factor - 1) / factor != c->f.xsize || (out_ysize + factor - 1) / factor != c->f.ysize)
    return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "a %ux%u frame upsampled %ux does not give %ux%u", c->f.xsize, c->f.ysize,
                factor, out_xsize, out_ysize);
  HIPCHK(c, hipSetDevice(c->device));
  const float* coded = weights ? weights : factor == 2 ? kUpsampling2Weights : factor == 4 ? kUpsampling4Weights : kUpsampling8Weights;
  UpsampleKernels(factor, coded, c->st.ups.weights_host);
  const int rc = c->st.ups.weights.Reserve(c, 64 * 25);
  if (rc) return rc;
  // (a pageable source: staged by the runtime when hipMemcpyAsync returns, the next frame may overwrite it)
  HIPCHK(c, hipMemcpyAsync(c->st.ups.weights, c->st.ups.weights_host, sizeof(float) * factor * factor * 25, hipMemcpyHostToDevice, c->stream));
  c->st.ups.factor = factor;
  c->st.ups.xsize = out_xsize;
  c->st.ups.ysize = out_ysize;
  return JXLHIP_OK;
}

// DC-only groups of the current frame (FrameDecoder::Flush on a group without AC, dec_frame.cc:737-797): the mask and
// the 8x kernels go up here; the decode calls zero the groups' coefficient slots and launch k_dc_upsample8 behind
// phase 1 (LaunchDcOnly); frame_begin resets to "none".
int jxlhip_set_dc_only_groups(jxlhip_ctx* c, const uint8_t* mask, const float* weights8) {
  if (!c) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (c->multi) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "DC-only groups on a multi-device context");
  if (!c->have_frame) return Fail(c, JXLHIP_ERR_STATE, "set_dc_only_groups before frame_begin");
  c->st.dc_only.on = false;
  const size_t ng = (size_t)c->f.xsg * c->f.ysg;
  bool any = false;
  for (size_t g = 0; mask && g < ng; g++) any = any || mask[g] != 0;
  if (!any) return JXLHIP_OK;  // the frame's own path, untouched
  if (c->f.group_y0 != 0 || c->f.group_rows != c->f.ysg) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "DC-only groups with stripes");
  const char* other = c->st.noise.on ? "noise" : c->st.splines.on ? "splines" : c->st.patches.on ? "patches" : c->st.ups.factor > 1 ? "upsampling"
                      : c->st.blend.on ? "blending" : c->fp.alpha ? "alpha" : nullptr;
  if (other) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "DC-only groups on a frame with %s", other);
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = c->st.dc_only.mask.Reserve(c, ng)) || (rc = c->st.dc_only.weights.Reserve(c, 25 * 64))) return rc;
  float kernels[64 * 25], tap_major[25 * 64];
  UpsampleKernels(8, weights8 ? weights8 : kUpsampling8Weights, kernels);
  DcUpsampleWeights(kernels, tap_major);
  c->st.dc_only.host.assign(mask, mask + ng);
  // (pageable sources: staged by the runtime when hipMemcpyAsync returns)
  HIPCHK(c, hipMemcpyAsync(c->st.dc_only.mask, c->st.dc_only.host.data(), ng, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->st.dc_only.weights, tap_major, sizeof(tap_major), hipMemcpyHostToDevice, c->stream));
  c->st.dc_only.on = true;
  return JXLHIP_OK;
}

// Blending of the current frame (FrameHeader::blending_info, frame_origin, save_as_reference): recorded here, carried
// out by DecodeFrameBlended; frame_begin resets to "not blended".
int jxlhip_set_blending(jxlhip_ctx* c, const jxlhip_blend_params* b) {
  if (!c) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (c->multi) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "blending on a multi-device context");
  if (!c->have_frame) return Fail(c, JXLHIP_ERR_STATE, "set_blending before frame_begin");
  c->st.blend.on = false;
  c->st.blend_ec.on = false;
  if (!b) return JXLHIP_OK;
  if (c->st.dc_only.on) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "blending on a frame with DC-only groups");
  if (c->f.group_y0 != 0 || c->f.group_rows != c->f.ysg) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "blending with stripes");
  if (c->p.undo_orientation > 1) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "blending with undo_orientation %u", c->p.undo_orientation);
  if (c->p.output_kind == JXLHIP_OUT_XYB_PLANAR)
    return Fail(c, JXLHIP_ERR_UNSUPPORTED, "blending with planar XYB output (canvases are frames saved after the colour transform)");
  if (c->fp.alpha) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "blending on a frame with alpha (blending extra channels is not in the back-end)");
  if (c->st.tone_map.on) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "blending on a tone-mapped frame (tone mapping behind a blend is not in the back-end)");
  if (b->image_xsize == 0 || b->image_ysize == 0 || b->image_xsize > (1u << 19) || b->image_ysize > (1u << 19))
    return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "image size %ux%u out of range", b->image_xsize, b->image_ysize);
  if (b->x0 < -(1 << 30) || b->x0 > (1 << 30) || b->y0 < -(1 << 30) || b->y0 > (1 << 30))
    return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "frame origin (%d, %d) out of range", b->x0, b->y0);
  if (b->mode > JXLHIP_BLEND_MUL) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "blend mode %u", b->mode);
  if (b->source > 3 || (b->save_slot > 3 && b->save_slot != JXLHIP_BLEND_NO_SAVE))
    return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "blend source slot %u / save slot %u", b->source, b->save_slot);
  c->st.blend.p = *b;
  c->st.blend.on = true;
  return JXLHIP_OK;
}

// rows of w floats, device to device on c->stream (strides in floats)
static int CopyRows(jxlhip_ctx* c, float* dst, size_t dst_stride, const float* src, size_t src_stride, size_t w, size_t h) {
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpy2DAsync(dst, dst_stride * sizeof(float), src, src_stride * sizeof(float), w * sizeof(float), h, hipMemcpyDeviceToDevice, c->stream));
  return JXLHIP_OK;
}

int jxlhip_canvas_read(jxlhip_ctx* c, uint32_t slot, float* dev_out, size_t stride_floats, uint32_t* w, uint32_t* h) {
  if (!c || slot > 3 || !w || !h) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (c->multi) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "canvases on a multi-device context");
  *w = c->slots.canvas_w[slot];
  *h = c->slots.canvas_h[slot];
  if (!dev_out || *w == 0) return JXLHIP_OK;
  if (stride_floats < 3 * (size_t)*w) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "canvas stride %zu < 3 * %u", stride_floats, *w);
  return CopyRows(c, dev_out, stride_floats, c->slots.canvas[slot], CanvasStride(*w), 3 * (size_t)*w, *h);
}


// What DecodeFrameBlended and jxlhip_set_blending_extra both need to know about a blended frame of an image with extra
// channels: whether the colour's mode comes to "replace" (PerformBlending's copy(fg)), and whether nothing of any
// source is read at all (a full-size frame at the origin whose colour and extra channels all replace).
static bool EcHasAlpha(const jxlhip_blend_extra_params& e) {
  for (uint32_t i = 0; i < e.num_extra_channels; i++)
    if (e.channel[i].is_alpha) return true;
  return false;
}
static bool EcSourcesDead(const jxlhip_ctx* c, const jxlhip_blend_extra_params& e) {
  const jxlhip_blend_params& b = c->st.blend.p;
  const bool full = b.x0 == 0 && b.y0 == 0 && OutCols(c) == b.image_xsize && OutRows(c) == b.image_ysize;
  bool replaces = b.mode == JXLHIP_BLEND_REPLACE || (b.mode == JXLHIP_BLEND_BLEND && !EcHasAlpha(e));
  for (uint32_t i = 0; i < e.num_extra_channels; i++) replaces = replaces && e.channel[i].mode == JXLHIP_BLEND_REPLACE;
  return full && replaces;
}
// the source slots of the extra channels, as DecodeFrameBlended checks the colour's
static int CheckEcSources(jxlhip_ctx* c, const jxlhip_blend_extra_params& e) {
  if (EcSourcesDead(c, e)) return JXLHIP_OK;
  const uint32_t W = c->st.blend.p.image_xsize, H = c->st.blend.p.image_ysize;
  for (uint32_t i = 0; i < e.num_extra_channels; i++) {
    const uint32_t s = e.channel[i].source;
    if (c->slots.ref_w[s] != 0)
      return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "blend source slot %u of extra channel %u holds an XYB reference frame", s, i);
    if (c->slots.canvas_w[s] != 0 && (c->slots.canvas_w[s] < W || c->slots.canvas_h[s] < H))
      return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "the %ux%u canvas of slot %u (extra channel %u) is smaller than the %ux%u image",
                  c->slots.canvas_w[s], c->slots.canvas_h[s], s, i, W, H);
  }
  return JXLHIP_OK;
}

// The extra channels of the current blended frame (FrameHeader::extra_channel_blending_info, ExtraChannelInfo):
// recorded and uploaded here, carried out by DecodeFrameBlended with k_ec_blend; frame_begin and set_blending reset.
int jxlhip_set_blending_extra(jxlhip_ctx* c, const jxlhip_blend_extra_params* e) {
  if (!c || !e) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (c->multi) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "blending on a multi-device context");
  if (!c->have_frame) return Fail(c, JXLHIP_ERR_STATE, "set_blending_extra before frame_begin");
  c->st.blend_ec.on = false;
  if (!c->st.blend.on) return Fail(c, JXLHIP_ERR_STATE, "set_blending_extra without set_blending on this frame");
  if (c->fp.alpha) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "set_blending_extra on a frame with set_alpha (the alpha channel is one of the planes here)");
  if (c->st.ups.factor > 1) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "extra channels of an upsampled frame");
  if (c->st.patches.on) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "extra channels of a frame with patches (they would have to blend them)");
  const uint32_t n = e->num_extra_channels;
  if (n == 0 || n > 4) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "%u extra channels (1..4)", n);
  if (e->color_alpha_channel >= n) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "colour alpha channel %u of %u", e->color_alpha_channel, n);
  const size_t fw = c->f.xsize, fh = c->f.ysize;
  for (uint32_t i = 0; i < n; i++) {
    const jxlhip_blend_extra_channel& ch = e->channel[i];
    if (ch.mode > JXLHIP_BLEND_MUL) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "extra channel %u: blend mode %u", i, ch.mode);
    if (ch.alpha_channel >= n) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "extra channel %u: alpha channel %u of %u", i, ch.alpha_channel, n);
    if (ch.source > 3) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "extra channel %u: blend source slot %u", i, ch.source);
    if (!e->planes[i]) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "extra channel %u: null plane", i);
  }
  if (e->stride_floats < fw) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "extra channel stride %zu < xsize", e->stride_floats);
  int rc = CheckEcSources(c, *e);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  // staged like the colour: (x0 mod 4) floats into rows padded to four pixels (kernels_blend_ec.hip)
  const size_t lead = (size_t)(c->st.blend.p.x0 - (c->st.blend.p.x0 & ~3));
  const size_t stride = EcStride((uint32_t)(lead + fw));
  const size_t need = n * fh * stride;
  if (need > c->st.blend_ec.stage.n) {
    if (Capturing(c->stream)) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "blending while the stream is being captured");
    HIPCHK(c, hipStreamSynchronize(c->stream));  // an earlier launch may still read the planes
    if ((rc = c->st.blend_ec.stage.Reserve(c, need))) return rc;
    // (the padding is read, never used: zeroed once so that nothing reads memory nobody wrote)
    HIPCHK(c, hipMemsetAsync(c->st.blend_ec.stage, 0, need * sizeof(float), c->stream));
  }
  for (uint32_t i = 0; i < n; i++)
    HIPCHK(c, hipMemcpy2DAsync(c->st.blend_ec.stage + i * fh * stride + lead, stride * sizeof(float), e->planes[i],
                               e->stride_floats * sizeof(float), fw * sizeof(float), fh, hipMemcpyHostToDevice, c->stream));
  c->st.blend_ec.stage_stride = stride;
  c->st.blend_ec.p = *e;
  for (int i = 0; i < 4; i++) c->st.blend_ec.p.planes[i] = nullptr;
  c->st.blend_ec.on = true;
  return JXLHIP_OK;
}

int jxlhip_canvas_read_extra(jxlhip_ctx* c, uint32_t slot, uint32_t ec, float* dev_out, size_t stride_floats, uint32_t* w, uint32_t* h) {
  if (!c || slot > 3 || ec > 3 || !w || !h) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (c->multi) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "canvases on a multi-device context");
  const bool have = c->slots.canvas_w[slot] != 0 && ec < c->slots.canvas_nec[slot];
  *w = have ? c->slots.canvas_w[slot] : 0;
  *h = have ? c->slots.canvas_h[slot] : 0;
  if (!dev_out || !have) return JXLHIP_OK;
  if (stride_floats < *w) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "plane stride %zu < %u", stride_floats, *w);
  const size_t es = EcStride(*w);
  return CopyRows(c, dev_out, stride_floats, c->slots.canvas_ec[slot] + (size_t)ec * *h * es, es, *w, *h);
}

int jxlhip_frame_extra_read(jxlhip_ctx* c, uint32_t ec, float* dev_out, size_t stride_floats) {
  if (!c || !dev_out || ec > 3) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (c->multi) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "canvases on a multi-device context");
  if (ec >= c->st.blend_ec.frame_n) return Fail(c, JXLHIP_ERR_STATE, "the current frame has no blended plane of extra channel %u", ec);
  const uint32_t w = c->st.blend_ec.frame_w, h = c->st.blend_ec.frame_h;
  if (stride_floats < w) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "plane stride %zu < %u", stride_floats, w);
  const size_t es = EcStride(w);
  return CopyRows(c, dev_out, stride_floats, c->st.blend_ec.frame_planes + (size_t)ec * h * es, es, w, h);
}

// ToneMappingStage's constructor for `t` (stage_tone_mapping.cc:33-64): 1 = the Rec.2408 tone mapper is built, 0 = no
// stage (the frame's plain path), else the error (with its reason in c->err when c is given)
static int ToneMappingKind(jxlhip_ctx* c, const jxlhip_tone_mapping* t) {
  if (!(t->orig_intensity_target > 0.0f) || !(t->desired_intensity_target > 0.0f) || !std::isfinite(t->orig_intensity_target) ||
      !std::isfinite(t->desired_intensity_target))
    return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "tone mapping: intensity targets %g -> %g", t->orig_intensity_target, t->desired_intensity_target);
  for (int i = 0; i < 3; i++)
    if (!std::isfinite(t->luminances[i])) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "tone mapping: luminance %d is not finite", i);
  if (t->orig_transfer > JXLHIP_TF_HLG) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "tone mapping: orig_transfer %u", t->orig_transfer);
  if (t->desired_intensity_target == t->orig_intensity_target) return 0;
  if (t->orig_transfer == JXLHIP_TF_PQ) return t->desired_intensity_target < t->orig_intensity_target ? 1 : 0;
  if (t->orig_transfer == JXLHIP_TF_HLG)
    return Fail(c, JXLHIP_ERR_UNSUPPORTED, "tone mapping of an HLG original (the HlgOOTF branch is not in the back-end)");
  return 0;
}

// Tone mapping of the current frame (JxlDecoderSetDesiredIntensityTarget): recorded here, carried out by
// DecodeFrameToneMapped; frame_begin resets to "not tone-mapped".
int jxlhip_set_tone_mapping(jxlhip_ctx* c, const jxlhip_tone_mapping* t) {
  if (!c) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (c->multi) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "tone mapping on a multi-device context");
  if (!c->have_frame) return Fail(c, JXLHIP_ERR_STATE, "set_tone_mapping before frame_begin");
  c->st.tone_map.on = false;
  if (!t) return JXLHIP_OK;
  const int kind = ToneMappingKind(c, t);
  if (kind <= 0) return kind;
  if (c->f.group_y0 != 0 || c->f.group_rows != c->f.ysg) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "tone mapping with stripes");
  if (c->p.undo_orientation > 1) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "tone mapping with undo_orientation %u", c->p.undo_orientation);
  if (c->p.output_kind == JXLHIP_OUT_XYB_PLANAR)
    return Fail(c, JXLHIP_ERR_UNSUPPORTED, "tone mapping with planar XYB output (the stage works on linear RGB)");
  if (c->st.blend.on) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "tone mapping on a blended frame (tone mapping behind a blend is not in the back-end)");
  const bool dest_pq = c->p.output_kind == JXLHIP_OUT_PACKED && c->p.out_format.transfer == JXLHIP_TF_PQ;
  ToneMapHostConstants(t->orig_intensity_target, t->desired_intensity_target, t->luminances, dest_pq, &c->st.tone_map.k);
  c->st.tone_map.on = true;
  return JXLHIP_OK;
}

int jxlhip_tone_mapping_constants(const jxlhip_tone_mapping* t, uint32_t dest_transfer, float* out, size_t n) {
  if (!t || !out || n > kToneMapConstants || dest_transfer > JXLHIP_TF_HLG) return JXLHIP_ERR_INVALID_ARGUMENT;
  const int kind = ToneMappingKind(nullptr, t);
  if (kind != 1) return JXLHIP_ERR_INVALID_ARGUMENT;
  ToneMapConstants k;
  ToneMapHostConstants(t->orig_intensity_target, t->desired_intensity_target, t->luminances, dest_transfer == JXLHIP_TF_PQ, &k);
  memcpy(out, &k, n * sizeof(float));
  return JXLHIP_OK;
}

int jxlhip_noise_rng_state(uint32_t visible_frame_index, uint32_t nonvisible_frame_index, uint32_t x0, uint32_t y0,
                           uint64_t fills, uint64_t state[16]) {
  if (!state) return JXLHIP_ERR_INVALID_ARGUMENT;
  NoiseStateAfter(visible_frame_index, nonvisible_frame_index, x0, y0, fills, state);
  return JXLHIP_OK;
}

// jxlhip_set_dc_only_groups, in front of phase 1: the coefficient slots of the masked groups are zeroed (the context's
// upload buffer only: nothing was submitted into them, and phase 1 must not read what an earlier frame left), runs of
// neighbouring groups with one memset each
int jxlhip::ZeroDcOnlySlots(jxlhip_ctx* c) {
  if (!c->st.dc_only.on || c->f.coeffs[0] != c->up_coeffs[0] || !c->up_coeffs[0]) return JXLHIP_OK;
  const size_t ng = (size_t)c->f.xsg * c->f.ysg, slot = 3 * (size_t)JXLHIP_GROUP_COEFFS * c->up_esz;
  if (c->up_groups != ng) return Fail(c, JXLHIP_ERR_STATE, "the upload buffers were laid out for another frame");
  for (size_t g = 0; g < ng;) {
    if (!c->st.dc_only.host[g]) {
      g++;
      continue;
    }
    size_t e = g;
    while (e < ng && c->st.dc_only.host[e]) e++;
    HIPCHK(c, hipMemsetAsync((char*)c->up_coeffs[0] + g * slot, 0, (e - g) * slot, c->stream));
    g = e;
  }
  return JXLHIP_OK;
}
// ... and behind it: k_dc_upsample8 writes the masked groups' tiles of the planes
int jxlhip::LaunchDcOnly(jxlhip_ctx* c) {
  if (!c->st.dc_only.on) return JXLHIP_OK;
  if (!LaunchDcUpsample8(c->f, c->st.dc_only.mask, c->st.dc_only.weights, c->stream))
    return Fail(c, JXLHIP_ERR_UNSUPPORTED, "DC-only groups: a stripe, or planes beyond 32-bit indices");
  ProfMark(c, JXLHIP_KERNEL_DC_UPSAMPLE);
  HIPCHK(c, hipGetLastError());
  return JXLHIP_OK;
}

// A frame with splines, upsampling and / or photon noise (jxlhip_set_splines, jxlhip_set_upsampling, jxlhip_set_noise;
// whole frames, coded orientation): the frame's own path -- fused or two-phase, whatever DecodeFrameCoded picks for it --
// writes the filtered frame as planar XYB into context memory; the render stages the reference's pipeline has between
// the loop filters and the XYB stage follow in its order (dec_cache.cc:194-218): splines at coded size, upsampling,
// noise at output size, and the last launch writes the caller's output:
//   splines only  k_splines draws every tile and emits;
//   noise only    k_noise_rng + k_noise_emit (kernels_noise.hip);
//   upsampling    k_upsample emits; with noise it writes planar XYB at output size and the noise launches emit;
//   splines in front of either: k_splines draws the tiles with segments back into the planes.
// Noise behind upsampling is the noise of a frame of the output size: PrepareNoiseInput seeds one generator per
// group_dim tile in OUTPUT coordinates and fills it clipped to the image (dec_noise.cc:120-151).
static int DecodeFrameFeatures(jxlhip_ctx* c, const OutTarget& t) {
  const bool ups = c->st.ups.factor > 1;
  int rc = CheckOutArgs(c, t, OutCols(c), OutRows(c));
  if (rc) return rc;
  const DevFrame& f = c->f;
  if (f.group_y0 != 0 || f.group_rows != f.ysg || c->p.undo_orientation > 1)
    return Fail(c, JXLHIP_ERR_UNSUPPORTED, "noise / splines / upsampling need a whole frame in coded orientation");
  if (c->st.patches.on && c->st.patches.ref_serial != c->slots.ref_serial)  // (in front of every launch of the frame)
    return Fail(c, JXLHIP_ERR_STATE, "set_reference_frame after set_patches (the uploaded dictionary points into the slots)");
  HIPCHK(c, hipSetDevice(c->device));
  // the filtered frame at coded size (cns x f.ysize per plane), and the frame the noise launches work on (W x H)
  const uint32_t cns = (f.xsize + 63u) & ~63u;
  const size_t cplane = (size_t)cns * f.ysize;
  const uint32_t W = (uint32_t)OutCols(c), H = (uint32_t)OutRows(c);
  const uint32_t ns = (W + 63u) & ~63u;
  const size_t nplane = (size_t)ns * H;
  if (ups && (rc = c->st.ups.planes.Reserve(c, 3 * cplane))) return rc;
  if ((!ups || c->st.noise.on) && (rc = c->st.noise.buf.Reserve(c, (c->st.noise.on ? 6 : 3) * nplane))) return rc;
  float* coded = ups ? c->st.ups.planes : c->st.noise.buf;
  if ((rc = DecodeFrameCoded(c, MakeTarget(c, JXLHIP_OUT_XYB_PLANAR, c->p.out_format, coded, cns, cplane)))) return rc;
  const uint32_t kind = t.kind;
  const FilterParams& fp = t.fp;
  ProfBegin(c);
  auto tiled = [&](auto* a, const TileList& tiles) {  // PatchArgs / SplineArgs: the coded frame, drawn in place, and the list
    a->xsize = f.xsize;
    a->ysize = f.ysize;
    a->xyb = a->xyb_out = coded;
    a->ns = cns;
    a->nplane = cplane;
    tiles.Fill(a);
  };
  if (c->st.patches.on) {
    PatchArgs A{};
    tiled(&A, c->st.patches.tiles);
    A.recs = c->st.patches.recs;
    if (!LaunchPatches(A, fp, (int)kind, /*in_place=*/c->st.splines.on || c->st.noise.on || ups, c->stream))
      return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "patches output kind %u", kind);
    ProfMark(c, JXLHIP_KERNEL_PATCHES);
  }
  if (c->st.splines.on) {
    SplineArgs S{};
    tiled(&S, c->st.splines.tiles);
    S.segs = c->st.splines.segs;
    if (!LaunchSplines(S, fp, (int)kind, /*in_place=*/c->st.noise.on || ups, c->stream))
      return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "splines output kind %u", kind);
    ProfMark(c, JXLHIP_KERNEL_SPLINES);
  }
  if (ups) {
    UpsampleArgs U{};
    U.cw = f.xsize;
    U.ch = f.ysize;
    U.xsize = W;
    U.ysize = H;
    U.n = c->st.ups.factor;
    U.xyb = coded;
    U.ns = cns;
    U.nplane = cplane;
    U.weights = c->st.ups.weights;
    if (!LaunchUpsample(U, fp, (int)kind, c->st.noise.on ? (float*)c->st.noise.buf : nullptr, ns, nplane, c->stream))
      return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "upsampling output kind %u", kind);
    ProfMark(c, JXLHIP_KERNEL_UPSAMPLE);
  }
  if (c->st.noise.on) {
    NoiseArgs N{};
    N.xsize = W;
    N.ysize = H;
    N.xsg = (W + 255u) / 256u;
    N.ysg = (H + 255u) / 256u;
    N.visible = c->st.noise.visible;
    N.nonvisible = c->st.noise.nonvisible;
    memcpy(N.lut, c->st.noise.lut, sizeof(N.lut));
    N.ytox = c->p.cfl_base_x;  // ColorCorrelation::YtoXRatio(0) / YtoBRatio(0) (chroma_from_luma.h:51-57)
    N.ytob = c->p.cfl_base_b;
    N.xyb = c->st.noise.buf;
    N.rnd = c->st.noise.buf + 3 * nplane;
    N.ns = ns;
    N.nplane = nplane;
    N.jump = c->st.noise.jump;
    if (!LaunchNoise(N, fp, (int)kind, c->stream)) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "noise output kind %u", kind);
    ProfMark(c, JXLHIP_KERNEL_NOISE);
  }
  HIPCHK(c, hipGetLastError());
  return JXLHIP_OK;
}

int jxlhip::DecodeFrameOwnPath(jxlhip_ctx* c, const OutTarget& t) {
  return c->st.RenderStagesOn() ? DecodeFrameFeatures(c, t) : DecodeFrameCoded(c, t);
}

// A blended frame (jxlhip_set_blending): the frame's whole path -- DecodeFrameCoded or DecodeFrameFeatures, whatever it
// would take without blending -- writes packed float RGB in the caller's transfer function into blend_stage, and
// k_blend (kernels_blend.hip) blends that over the source canvas into the save slot and / or the caller's buffer,
// which is image-sized.  The canvas never leaves the device.  With jxlhip_set_blending_extra the launch is k_ec_blend
// (kernels_blend_ec.hip), which blends and saves the image's extra channels beside the colour.
int jxlhip::DecodeFrameBlended(jxlhip_ctx* c, void* out, size_t out_stride) {
  const jxlhip_blend_params& b = c->st.blend.p;
  const DevFrame& f = c->f;
  // (set_blending has checked these; set_alpha, set_upsampling .. may have been called since)
  if (f.group_y0 != 0 || f.group_rows != f.ysg || c->p.undo_orientation > 1 || c->p.output_kind == JXLHIP_OUT_XYB_PLANAR)
    return Fail(c, JXLHIP_ERR_UNSUPPORTED, "blending needs a whole frame in coded orientation and an interleaved output");
  if (c->fp.alpha) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "blending on a frame with alpha");
  const bool ec = c->st.blend_ec.on;
  const jxlhip_blend_extra_params& e = c->st.blend_ec.p;
  const uint32_t nec = ec ? e.num_extra_channels : 0;
  if (ec && (c->st.ups.factor > 1 || c->st.patches.on))
    return Fail(c, JXLHIP_ERR_UNSUPPORTED, "extra channels of an upsampled frame or of a frame with patches");
  const uint32_t W = b.image_xsize, H = b.image_ysize;
  const bool save = b.save_slot != JXLHIP_BLEND_NO_SAVE;
  if (!out && !save) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "null output and no save slot");
  int rc;
  OutTarget t = MakeTarget(c, out, out_stride, 0);  // the caller's: what the blend launch writes
  if (out && (rc = CheckOutArgs(c, t, W, H))) return rc;
  if (Capturing(c->stream))  // (canvas and staging memory may have to grow: a synchronise and an allocation)
    return Fail(c, JXLHIP_ERR_UNSUPPORTED, "blending while the stream is being captured");
  const int64_t fw = (int64_t)OutCols(c), fh = (int64_t)OutRows(c);
  const uint32_t op = b.mode == JXLHIP_BLEND_MUL ? (b.clamp ? kPatchOpMulClamp : kPatchOpMul)
                      : (b.mode == JXLHIP_BLEND_ADD || b.mode == JXLHIP_BLEND_ALPHA_WEIGHTED_ADD) ? kPatchOpAdd : kPatchOpReplace;
  const bool full = b.x0 == 0 && b.y0 == 0 && fw == W && fh == H;
  // a full frame that replaces never reads its source: whatever the slot holds is no concern of this frame.  (With
  // extra channels "replaces" means the colour AND every channel: a full frame whose colour replaces while a channel
  // blends has the colour's slot checked too although the colour does not read it, as BlendingStage's constructor does.)
  const bool bg_dead = ec ? EcSourcesDead(c, e) : full && op == kPatchOpReplace;
  if (!bg_dead && c->slots.ref_w[b.source] != 0)
    return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "blend source slot %u holds an XYB reference frame", b.source);
  const bool have_src = !bg_dead && c->slots.canvas_w[b.source] != 0;
  if (have_src && (c->slots.canvas_w[b.source] < W || c->slots.canvas_h[b.source] < H))
    return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "the %ux%u canvas of slot %u is smaller than the %ux%u image",
                c->slots.canvas_w[b.source], c->slots.canvas_h[b.source], b.source, W, H);
  const bool in_place = save && have_src && b.save_slot == b.source;
  if (in_place && (c->slots.canvas_w[b.source] != W || c->slots.canvas_h[b.source] != H))
    return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "save_slot == source with a %ux%u canvas and a %ux%u image",
                c->slots.canvas_w[b.source], c->slots.canvas_h[b.source], W, H);
  // the extra channels: each from the plane of its own source slot (zeroes when the slot has none); a slot that is
  // saved into while one of its planes is read must already have the layout it is given
  bool ec_src[4] = {false, false, false, false};
  bool ec_in_place = true;
  if (ec) {
    if ((rc = CheckEcSources(c, e))) return rc;
    for (uint32_t i = 0; i < nec; i++) {
      const uint32_t s = e.channel[i].source;
      ec_src[i] = !bg_dead && c->slots.canvas_w[s] != 0 && i < c->slots.canvas_nec[s];
      ec_in_place = ec_in_place && ec_src[i] && save && s == b.save_slot;
      if (save && ec_src[i] && s == b.save_slot && (c->slots.canvas_w[s] != W || c->slots.canvas_h[s] != H || c->slots.canvas_nec[s] != nec))
        return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT,
                    "save_slot == source of extra channel %u with a %ux%u canvas of %u extra channels and a %ux%u image of %u", i,
                    c->slots.canvas_w[s], c->slots.canvas_h[s], c->slots.canvas_nec[s], W, H, nec);
    }
  }
  const bool in_place_all = in_place && ec_in_place;  // (without extra channels: in_place)
  // a full frame that replaces and is not saved: today's path and launches, nothing else
  if (!ec && full && op == kPatchOpReplace && !save) return DecodeFrameOwnPath(c, t);
  HIPCHK(c, hipSetDevice(c->device));
  BlendArgs A{};
  A.W = W;
  A.H = H;
  A.rx0 = (int32_t)std::max<int64_t>(b.x0, 0);
  A.ry0 = (int32_t)std::max<int64_t>(b.y0, 0);
  A.rx1 = (int32_t)std::min<int64_t>((int64_t)b.x0 + fw, W);
  A.ry1 = (int32_t)std::min<int64_t>((int64_t)b.y0 + fh, H);
  const bool empty = A.rx1 <= A.rx0 || A.ry1 <= A.ry0;
  if (empty) A.rx0 = A.rx1 = A.ry0 = A.ry1 = 0;
  A.op = op;
  // the frame itself, staged: (x0 mod 4) pixels into rows padded to four pixels (see kernels_blend.hip).  A frame that
  // lies wholly outside the image is still decoded: its stream errors must surface as they do without blending.
  const int32_t xa = b.x0 & ~3;  // (rounds down, also below zero)
  const size_t lead = (size_t)(b.x0 - xa);
  const size_t stage_stride = CanvasStride((uint32_t)(lead + (size_t)fw));
  if ((rc = c->st.blend.stage.Reserve(c, (size_t)fh * stage_stride))) return rc;
  jxlhip_output_format stage_fmt = c->p.out_format;  // float RGB in the caller's transfer function: no dither, no alpha
  stage_fmt.sample_type = JXLHIP_SAMPLE_F32;
  stage_fmt.num_channels = 3;
  stage_fmt.swap_endianness = 0;
  rc = DecodeFrameOwnPath(c, MakeTarget(c, c->p.output_kind, stage_fmt, c->st.blend.stage + 3 * lead, stage_stride * sizeof(float), 0));
  if (rc) return rc;
  A.fg = c->st.blend.stage;
  A.fg_xa = xa;
  A.fg_y0 = b.y0;
  A.fg_stride = stage_stride;
  if (have_src) {
    A.src = c->slots.canvas[b.source];
    A.src_stride = CanvasStride(c->slots.canvas_w[b.source]);
  }
  if (save) {
    const uint32_t s = b.save_slot;
    if (!in_place) {
      const size_t need = (size_t)H * CanvasStride(W);
      if (need > c->slots.canvas[s].n) HIPCHK(c, hipStreamSynchronize(c->stream));  // an earlier launch may still read the slot
      if ((rc = c->slots.canvas[s].Reserve(c, need))) return rc;
    }
    A.dst = c->slots.canvas[s];
    A.dst_stride = CanvasStride(W);
  }
  A.dst_all = in_place_all ? 0u : 1u;
  // the caller's buffer or another slot is written everywhere; a frame blended into its own source slot -- the source of
  // its colour and of every extra channel -- only under its rectangle
  if (out || !in_place_all) {
    A.gx0 = 0;
    A.gx1 = (W + 3) / 4;
    A.y0 = 0;
    A.y1 = H;
  } else {
    A.gx0 = (uint32_t)A.rx0 / 4;
    A.gx1 = ((uint32_t)A.rx1 + 3) / 4;
    A.y0 = (uint32_t)A.ry0;
    A.y1 = (uint32_t)A.ry1;
  }
  FilterParams& fp = t.fp;
  fp.fmt.transfer = JXLHIP_TF_LINEAR;  // the samples are encoded already: neither the HLG OOTF nor the curve runs twice
  BlendEcArgs E{};
  if (ec) {
    const size_t es = EcStride(W), plane = (size_t)H * es;
    // where the blended planes go: the save slot's, or the frame's own
    DevBuf<float>& planes = save ? c->slots.canvas_ec[b.save_slot] : c->st.blend_ec.frame_buf;
    if ((size_t)nec * plane > planes.n) HIPCHK(c, hipStreamSynchronize(c->stream));  // an earlier launch may still read them
    if ((rc = planes.Reserve(c, (size_t)nec * plane))) return rc;
    E.num_ec = nec;
    E.has_alpha = EcHasAlpha(e) ? 1u : 0u;
    E.color_mode = b.mode;
    E.color_clamp = b.clamp;
    E.color_alpha = e.color_alpha_channel;
    E.out_alpha = -1;
    E.fg_stride = c->st.blend_ec.stage_stride;
    E.dst_stride = es;
    for (uint32_t i = 0; i < nec; i++) {
      const jxlhip_blend_extra_channel& ch = e.channel[i];
      E.mode[i] = ch.mode;
      E.clamp[i] = ch.clamp;
      E.alpha[i] = ch.alpha_channel;
      E.premul[i] = ch.alpha_associated ? 1u : 0u;
      if (ch.is_alpha && E.out_alpha < 0) E.out_alpha = (int32_t)i;
      E.fg[i] = c->st.blend_ec.stage + (size_t)i * (size_t)fh * E.fg_stride;
      if (ec_src[i]) {
        const uint32_t s = ch.source;
        E.src_stride[i] = EcStride(c->slots.canvas_w[s]);
        E.src[i] = c->slots.canvas_ec[s] + (size_t)i * c->slots.canvas_h[s] * E.src_stride[i];
      }
      E.dst[i] = planes + (size_t)i * plane;
    }
    if (E.out_alpha >= 0) {  // the fourth sample of a packed output: read back from the blended plane
      fp.alpha = E.dst[E.out_alpha];
      fp.alpha_stride = (uint32_t)es;
    }
    c->st.blend_ec.frame_planes = planes;
    c->st.blend_ec.frame_n = nec;
    c->st.blend_ec.frame_w = W;
    c->st.blend_ec.frame_h = H;
  }
  // (a layer wholly outside the image that is blended into its own source slot visits nothing: no launch, no span)
  if (A.gx1 > A.gx0 && A.y1 > A.y0) {
    ProfBegin(c);
    if (ec) {
      E.B = A;
      if (!LaunchBlendEc(E, fp, out ? (int)c->p.output_kind : 0, c->stream)) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "blend launch arguments");
      ProfMark(c, JXLHIP_KERNEL_BLEND_EC);
    } else {
      if (!LaunchBlend(A, fp, out ? (int)c->p.output_kind : 0, c->stream)) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "blend launch arguments");
      ProfMark(c, JXLHIP_KERNEL_BLEND);
    }
    HIPCHK(c, hipGetLastError());
  }
  if (save) {
    const uint32_t s = b.save_slot;
    c->slots.canvas_w[s] = W;
    c->slots.canvas_h[s] = H;
    c->slots.canvas_nec[s] = nec;
    if (c->slots.ref_w[s] != 0) {  // (a slot holds one kind: the canvas drops the XYB frame, and a dictionary that points into it)
      c->slots.ref_w[s] = c->slots.ref_h[s] = 0;
      c->slots.ref_serial++;
    }
  }
  return JXLHIP_OK;
}

// A tone-mapped frame (jxlhip_set_tone_mapping): the frame's whole path -- DecodeFrameCoded or DecodeFrameFeatures,
// whatever it would take without tone mapping -- writes planar XYB at output size into tm_planes, and k_tone_map
// (kernels_tonemap.hip) writes the caller's output from that.
int jxlhip::DecodeFrameToneMapped(jxlhip_ctx* c, void* out, size_t out_stride) {
  const DevFrame& f = c->f;
  // (set_tone_mapping has checked these; set_blending refuses a tone-mapped frame)
  if (f.group_y0 != 0 || f.group_rows != f.ysg || c->p.undo_orientation > 1 || c->p.output_kind == JXLHIP_OUT_XYB_PLANAR || c->st.blend.on)
    return Fail(c, JXLHIP_ERR_UNSUPPORTED, "tone mapping needs a whole unblended frame in coded orientation and an interleaved output");
  const uint32_t W = (uint32_t)OutCols(c), H = (uint32_t)OutRows(c);
  const OutTarget t = MakeTarget(c, out, out_stride, 0);
  int rc = CheckOutArgs(c, t, W, H);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const uint32_t ns = (W + 63u) & ~63u;
  const size_t nplane = (size_t)ns * H;
  if (3 * nplane > 0xFFFFFFFFull)
    return Fail(c, JXLHIP_ERR_UNSUPPORTED, "tone mapping of a frame whose three planes exceed 2^32 samples (k_tone_map indexes with 32 bits)");
  if (3 * nplane > c->st.tone_map.planes.n && Capturing(c->stream))  // (a synchronise and an allocation)
    return Fail(c, JXLHIP_ERR_UNSUPPORTED, "tone mapping while the stream is being captured and its planes have to grow");
  if ((rc = c->st.tone_map.planes.Reserve(c, 3 * nplane))) return rc;
  if ((rc = DecodeFrameOwnPath(c, MakeTarget(c, JXLHIP_OUT_XYB_PLANAR, c->p.out_format, c->st.tone_map.planes, ns, nplane)))) return rc;
  ToneMapArgs A{};
  A.xsize = W;
  A.ysize = H;
  A.xyb = c->st.tone_map.planes;
  A.ns = ns;
  A.nplane = (uint32_t)nplane;
  A.k = c->st.tone_map.k;
  ProfBegin(c);
  if (!LaunchToneMap(A, t.fp, (int)t.kind, c->stream)) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "tone map launch arguments");
  ProfMark(c, JXLHIP_KERNEL_TONE_MAP);
  HIPCHK(c, hipGetLastError());
  return JXLHIP_OK;
}

// ---- a regular Modular frame (lossless files): the host's integer planes and RCT programs onto the device, k_modular_emit
// or -- an alpha plane, a grey frame -- k_modular_planes (kernels_modular.hip) into the caller's output, through the
// orientation staging frame when undo_orientation asks.
int jxlhip_decode_modular_frame(jxlhip_ctx* c, const jxlhip_modular_frame* f, uint32_t output_kind, const jxlhip_output_format* out_format,
                                void* out, size_t out_stride, uint32_t undo_orientation) {
  if (!c || !f) return JXLHIP_ERR_INVALID_ARGUMENT;
  jxlhip_modular_channels m{};  // three colour planes, no alpha: k_modular_emit's launch
  m.xsize = f->xsize;
  m.ysize = f->ysize;
  m.num_color = 3;
  for (int ch = 0; ch < 3; ch++) m.planes[ch] = f->planes[ch];
  m.stride_samples = f->stride_samples;
  m.sample_type = f->sample_type;
  m.bits_per_sample = f->bits_per_sample;
  m.group_dim = f->group_dim;
  m.group_rct = f->group_rct;
  m.global_rct = f->global_rct;
  return jxlhip_decode_modular_channels(c, &m, output_kind, out_format, out, out_stride, undo_orientation);
}

int jxlhip_decode_modular_channels(jxlhip_ctx* c, const jxlhip_modular_channels* m, uint32_t output_kind,
                                   const jxlhip_output_format* out_format, void* out, size_t out_stride, uint32_t undo_orientation) {
  if (!c || !m) return JXLHIP_ERR_INVALID_ARGUMENT;
  JXLHIP_NO_MULTI(c);
  if (output_kind == JXLHIP_OUT_XYB_PLANAR) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "planar XYB of a Modular frame that is not XYB");
  if (output_kind > JXLHIP_OUT_PACKED || (output_kind == JXLHIP_OUT_PACKED && !out_format) || undo_orientation > 8)
    return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "bad output kind / orientation");
  if (m->num_color != 1 && m->num_color != 3) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "bad Modular frame: %u colour planes", m->num_color);
  const uint32_t nc = m->num_color;
  if (m->alpha_plane && (m->alpha_bits == 0 || m->alpha_bits > 16)) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "bad Modular frame: %u alpha bits", m->alpha_bits);
  if (m->xsize == 0 || m->ysize == 0 || m->xsize > (1u << 19) || m->ysize > (1u << 19) || !m->planes[0] || (nc == 3 && (!m->planes[1] || !m->planes[2])) ||
      m->stride_samples < m->xsize || m->sample_type > JXLHIP_MODULAR_I32 || m->bits_per_sample == 0 || m->bits_per_sample > 16)
    return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "bad Modular frame: %ux%u, %u bits, sample type %u, stride %zu", m->xsize, m->ysize,
                m->bits_per_sample, m->sample_type, m->stride_samples);
  uint32_t shift = 0;
  while (shift < 11 && (1u << shift) != m->group_dim) shift++;
  if (shift < 7 || shift > 10) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "group dimension %u", m->group_dim);
  jxlhip_output_format fmt{};
  if (output_kind == JXLHIP_OUT_PACKED) {  // (as jxlhip_frame_begin; the transfer function is not read)
    fmt = *out_format;
    const uint32_t max_bits = fmt.sample_type == JXLHIP_SAMPLE_U8 ? 8 : 16;
    if (fmt.sample_type > JXLHIP_SAMPLE_F16 || (fmt.num_channels != 3 && fmt.num_channels != 4) || fmt.swap_endianness > 1 ||
        ((fmt.sample_type == JXLHIP_SAMPLE_U8 || fmt.sample_type == JXLHIP_SAMPLE_U16) && (fmt.bits_per_sample == 0 || fmt.bits_per_sample > max_bits)))
      return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "bad output format");
  }
  const uint32_t W = m->xsize, H = m->ysize;
  const uint32_t xsg = ((W - 1) >> shift) + 1, ysg = ((H - 1) >> shift) + 1;
  const size_t ng = (size_t)xsg * ysg;
  auto bad_program = [](uint32_t p) { return (p & 0xFFu) > 41u || (p >> 8) > 41u; };
  bool bad = bad_program(m->global_rct);
  for (size_t g = 0; m->group_rct && g < ng; g++) bad = bad || bad_program(m->group_rct[g]);
  if (bad) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "an RCT type above 41");
  if (nc == 1) {  // one colour plane: there is nothing an RCT could run over
    bool any = m->global_rct != 0;
    for (size_t g = 0; m->group_rct && g < ng; g++) any = any || m->group_rct[g] != 0;
    if (any) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "an RCT program on a grey (one-plane) Modular frame");
  }
  // the alpha plane goes up only when it reaches the output: the fourth channel of a packed format
  const bool alpha = m->alpha_plane && output_kind == JXLHIP_OUT_PACKED && out_format->num_channels == 4;
  const uint32_t np = nc + (alpha ? 1u : 0u);
  // the target: the caller's buffer, or -- undo_orientation -- the staging frame k_orient reads
  OutTarget t{output_kind, fmt, FilterParams{}};
  const size_t bpp = OutPixelBytes(output_kind, fmt);
  const bool oriented = undo_orientation > 1, transposed = undo_orientation >= 5;
  t.fp.out = out;
  t.fp.out_stride = out_stride;
  t.fp.fmt = fmt;
  int rc;
  if ((rc = CheckOutArgs(c, t, transposed ? H : W, transposed ? W : H))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if (oriented) {
    const size_t row = ((size_t)W * bpp + 255) & ~(size_t)255;
    if ((rc = c->orient_dev.Reserve(c, (size_t)H * row))) return rc;
    t.fp.out = c->orient_dev;
    t.fp.out_stride = row;
  }
  if (output_kind == JXLHIP_OUT_PACKED) {
    const bool is_int = fmt.sample_type == JXLHIP_SAMPLE_U8 || fmt.sample_type == JXLHIP_SAMPLE_U16;
    t.fp.sample_mul = is_int ? (float)((1u << fmt.bits_per_sample) - 1u) : 1.0f;  // stage_write.cc:528
    t.fp.dither = c->tables + kTabDither;
  }
  {  // the 8-bit dither pattern follows the flipped coordinates (jxlhip_frame_begin)
    const uint32_t o = undo_orientation;
    const bool fx = o == 2 || o == 3 || o == 7 || o == 8, fy = o == 3 || o == 4 || o == 6 || o == 7;
    t.fp.dither_x0 = fx ? (int32_t)W - 1 : 0;
    t.fp.dither_xs = fx ? -1 : 1;
    t.fp.dither_y0 = fy ? (int32_t)H - 1 : 0;
    t.fp.dither_ys = fy ? -1 : 1;
  }
  // the planes and the programs onto the device: rows padded to 64 samples, planes to 256 bytes
  const size_t ssz = m->sample_type == JXLHIP_MODULAR_I16 ? 2 : 4;
  const uint32_t ns = (W + 63u) & ~63u;
  const size_t plane_bytes = ((size_t)ns * H * ssz + 255) & ~(size_t)255;
  if ((np * plane_bytes > c->modular_dev.n || ng > c->modular_rct_dev.n) && Capturing(c->stream))  // (a synchronise and an allocation)
    return Fail(c, JXLHIP_ERR_UNSUPPORTED, "a Modular frame while the stream is being captured and its planes have to grow");
  if ((rc = c->modular_dev.Reserve(c, np * plane_bytes))) return rc;
  if ((rc = c->modular_rct_dev.Reserve(c, ng))) return rc;
  ModularPlanesArgs B{};
  ModularEmitArgs& A = B.e;
  for (uint32_t ch = 0; ch < np; ch++) {
    uint8_t* dst = c->modular_dev + ch * plane_bytes;
    const void* src = ch < nc ? m->planes[ch] : m->alpha_plane;
    HIPCHK(c, hipMemcpy2DAsync(dst, (size_t)ns * ssz, src, m->stride_samples * ssz, (size_t)W * ssz, H, hipMemcpyHostToDevice, c->stream));
    if (ch < nc) A.plane[ch] = dst;
    else B.alpha = dst;
  }
  B.num_color = nc;
  if (alpha) B.alpha_factor = (float)(1.0 / (double)((1u << m->alpha_bits) - 1u));
  if (m->group_rct) HIPCHK(c, hipMemcpyAsync(c->modular_rct_dev, m->group_rct, ng * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
  else HIPCHK(c, hipMemsetAsync(c->modular_rct_dev, 0, ng * sizeof(uint16_t), c->stream));
  A.xsize = W;
  A.ysize = H;
  A.ns = ns;
  A.sample_type = m->sample_type;
  A.group_shift = shift;
  A.xsg = xsg;
  A.group_rct = c->modular_rct_dev;
  A.global_rct = m->global_rct;
  A.factor = (float)(1.0 / (double)((1u << m->bits_per_sample) - 1u));  // dec_modular.cc:584-586
  if (!LaunchModularPlanes(B, t.fp, (int)output_kind, c->stream)) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "Modular emit launch arguments");
  HIPCHK(c, hipGetLastError());
  if (oriented) {
    if (!LaunchOrient(c->orient_dev, t.fp.out_stride, W, H, (uint32_t)bpp, undo_orientation, out, out_stride, c->stream))
      return Fail(c, JXLHIP_ERR_UNSUPPORTED, "undo_orientation %u with %zu-byte pixels", undo_orientation, bpp);
    HIPCHK(c, hipGetLastError());
  }
  return JXLHIP_OK;
}
