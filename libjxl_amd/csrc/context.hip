// context.hip -- the C ABI of include/jxl_hip.h: context, frame set-up, the
// two decode phases, halo regions, profiling.  Host code only;
// kernels live in kernels_*.hip.  No CPU fallback: every entry point that needs
// a device fails with JXLHIP_ERR_NO_DEVICE / JXLHIP_ERR_HIP when there is none.
// The render stages (their setters and decode paths) are render_stages.hip, the input hand-off is handover.hip, the
// multi-device parent multi.hip, the whole-file decoder codestream.hip.
#include <math.h>
#include <stdarg.h>
#include <stdlib.h>
#include <new>

#include "context.h"
#include "dither_pattern.inc"
#include "phase1_plan.h"

extern "C" __attribute__((visibility("default"))) void jxlhip_debug_reload_env(void) {
  std::lock_guard<std::mutex> lock(jxlhip_env::g.mu);
  jxlhip_env::LoadLocked();
}

int jxlhip::Fail(jxlhip_ctx* c, int code, const char* fmt, ...) {
  if (c) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(c->err, sizeof(c->err), fmt, ap);
    va_end(ap);
  }
  return code;
}

namespace {

// Counter blocks (kCountStride u32 each) of phase 1 (LaunchPhase1): direct calls alternate between blocks 0 and 1; a
// phase 1 recorded into a hipGraph uses kCaptureBlock, a block no direct call ever touches -- a replay dirties its block
// behind the host's back, and the host's "clean" flags describe blocks 0 / 1 only (round 5 put captured frames on
// block 0, round 6 still the split calls: a replay between two direct calls left k_prepare starting on non-zero counters).
constexpr int kCaptureBlock = 2;
constexpr int kCountBlocks = 3;

void ProfPush(jxlhip_ctx* c) {
  c->marks.emplace_back();
  (void)c->marks.back().ev.Create(hipEventDefault);
  (void)hipEventRecord(c->marks.back().ev, c->stream);
}

}  // namespace

void jxlhip::ProfBegin(jxlhip_ctx* c) {
  if (c->profiling) ProfPush(c);
}
// closes the span [previous mark, now) for `slot` and opens the next one (the last mark's slot_after stays -1: nothing
// starts there)
void jxlhip::ProfMark(jxlhip_ctx* c, int slot) {
  if (!c->profiling || c->marks.empty()) return;
  c->marks.back().slot_after = slot;
  ProfPush(c);
}

// ---- static helpers -------------------------------------------------------
int jxlhip_covered_blocks_x(int s) {
  return (s >= 0 && s < JXLHIP_NUM_STRATEGIES) ? kCoveredX[s] : 0;
}
int jxlhip_covered_blocks_y(int s) {
  return (s >= 0 && s < JXLHIP_NUM_STRATEGIES) ? kCoveredY[s] : 0;
}
int jxlhip_log2_covered_blocks(int s) {
  if (s < 0 || s >= JXLHIP_NUM_STRATEGIES) return -1;
  int n = kCoveredX[s] * kCoveredY[s], l = 0;
  while ((1 << l) < n) l++;
  return l;
}
int jxlhip_quant_table_of_strategy(int s) {
  return (s >= 0 && s < JXLHIP_NUM_STRATEGIES) ? kQuantKind[s] : -1;
}
size_t jxlhip_dequant_table_offset(int s, int c) {
  if (s < 0 || s >= JXLHIP_NUM_STRATEGIES || c < 0 || c > 2) return (size_t)-1;
  const int kind = kQuantKind[s];
  return DequantOffset(s) + (size_t)c * 64u * kKindShort[kind] * kKindLong[kind];
}
const char* jxlhip_status_string(int status) {
  switch (status) {
    case JXLHIP_OK: return "ok";
    case JXLHIP_ERR_INVALID_ARGUMENT: return "invalid argument";
    case JXLHIP_ERR_NO_DEVICE: return "no HIP device";
    case JXLHIP_ERR_OUT_OF_MEMORY: return "out of device memory";
    case JXLHIP_ERR_HIP: return "HIP runtime error";
    case JXLHIP_ERR_BAD_STREAM: return "side info violates a format constraint";
    case JXLHIP_ERR_STATE: return "call sequence error";
    case JXLHIP_ERR_UNSUPPORTED: return "stream feature outside this back-end";
    case JXLHIP_ERR_RANGE: return "coefficient outside the 16-bit range: redo the frame with JXLHIP_COEFF_I32";
    case JXLHIP_ERR_NEED_MORE_INPUT: return "the bytes end before anything can be drawn";
    default: return "unknown status";
  }
}

// ---- context ----------------------------------------------------------------
jxlhip_ctx* jxlhip::NewCtx(const JxlMemoryManagerHip* mm) {
  JxlMemoryManagerHip m{};
  if (mm) m = *mm;
  void* mem = m.alloc ? m.alloc(m.opaque, sizeof(jxlhip_ctx)) : malloc(sizeof(jxlhip_ctx));
  if (!mem) return nullptr;
  jxlhip_ctx* c = new (mem) jxlhip_ctx();
  c->mm = m;
  return c;
}
void jxlhip::DeleteCtx(jxlhip_ctx* c) {
  const JxlMemoryManagerHip m = c->mm;
  c->~jxlhip_ctx();
  if (m.free) m.free(m.opaque, c);
  else free(c);
}

int jxlhip_create(int device, jxlhip_ctx** out) { return jxlhip_create_ex(device, nullptr, out); }

int jxlhip_create_ex(int device, const JxlMemoryManagerHip* memory_manager, jxlhip_ctx** out) {
  if (!out) return JXLHIP_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  // both callbacks or none (lib/threads/thread_parallel_runner.cc:37-53, lib/jxl/memory_manager_internal.h)
  if (memory_manager && ((memory_manager->alloc == nullptr) != (memory_manager->free == nullptr)))
    return JXLHIP_ERR_INVALID_ARGUMENT;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return JXLHIP_ERR_NO_DEVICE;
  if (device < 0 || device >= ndev) return JXLHIP_ERR_INVALID_ARGUMENT;
  jxlhip_ctx* c = NewCtx(memory_manager);
  if (!c) return JXLHIP_ERR_OUT_OF_MEMORY;
  c->device = device;
  {  // the debug / test switches follow the environment as it is when a context is created (and at no other time)
    std::lock_guard<std::mutex> lock(jxlhip_env::g.mu);
    jxlhip_env::LoadLocked();
    const jxlhip_env::Switches& s = jxlhip_env::g;
    c->generic_filters = s.generic_filters.load();
    c->sparse_upload = s.sparse_upload.load();
    c->fuse = s.fuse.load();
    c->mfma = s.mfma.load();
    c->prepare_once = s.prepare_once.load();
    const int ss = s.stage_slots.load();
    if (ss != jxlhip_env::Switches::kUnset) {  // whole chunks, at least the first allocation
      const int v = (ss + kStageChunk - 1) / kStageChunk * kStageChunk;
      c->stage_cap = v < kStageSlotsFirst ? kStageSlotsFirst : (v > kStageSlots ? kStageSlots : v);
    }
  }
  auto fail = [&](int code) {
    jxlhip_destroy(c);
    return code;
  };
  if (hipSetDevice(device) != hipSuccess) return fail(JXLHIP_ERR_HIP);
  if (c->own_stream.Create() != hipSuccess) return fail(JXLHIP_ERR_HIP);
  c->stream = c->own_stream;
  for (int i = 0; i < kPoolStreams; i++) {
    if (c->pool[i].Create() != hipSuccess || c->pool_ev[i].Create() != hipSuccess) return fail(JXLHIP_ERR_HIP);
  }
  if (c->frame_ev.Create() != hipSuccess) return fail(JXLHIP_ERR_HIP);
  if (c->counts.Reserve(c, (size_t)kCountStride * kCountBlocks) || c->error_flag.Reserve(c, 2) ||
      c->tables.Reserve(c, kTabFloats) || c->quant_enc.Reserve(c, JXLHIP_NUM_QUANT_TABLES))
    return fail(JXLHIP_ERR_OUT_OF_MEMORY);
  if (hipMemset(c->error_flag, 0, sizeof(int32_t) * 2) != hipSuccess ||
      hipMemcpy(c->tables + kTabWc, kWcHost, sizeof(float) * (kTabResample - kTabWc), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(c->tables + kTabResample, kResampleUpHost, sizeof(float) * (kTabDither - kTabResample), hipMemcpyHostToDevice) !=
          hipSuccess ||
      hipMemcpy(c->tables + kTabDither, kDitherPattern, sizeof(float) * (kTabMfma32 - kTabDither), hipMemcpyHostToDevice) !=
          hipSuccess)
    return fail(JXLHIP_ERR_HIP);
  {
    float mfma_tab[kTabFloats - kTabMfma32];
    MfmaDct32Constants(mfma_tab);
    MfmaDct16Constants(mfma_tab + (kTabMfma16 - kTabMfma32));
    if (hipMemcpy(c->tables + kTabMfma32, mfma_tab, sizeof(mfma_tab), hipMemcpyHostToDevice) != hipSuccess)
      return fail(JXLHIP_ERR_HIP);
  }
  *out = c;
  return JXLHIP_OK;
}

// What is synchronisation happens here; the release is the owners' (~jxlhip_ctx in DeleteCtx).
void jxlhip_destroy(jxlhip_ctx* c) {
  if (!c) return;
  if (c->multi) return MultiDestroy(c);
  (void)hipSetDevice(c->device);
  if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
  for (int i = 0; i < kPoolStreams; i++)
    if (c->pool[i]) (void)hipStreamSynchronize(c->pool[i]);
  for (int i = 0; i < kStageSlots; i++)
    if (c->stage_ev[i] && c->stage_state[i] == 2) (void)hipEventSynchronize(c->stage_ev[i]);
  DeleteCtx(c);
}

const char* jxlhip_last_error(const jxlhip_ctx* c) { return c ? c->err : ""; }

int jxlhip_set_stream(jxlhip_ctx* c, void* hip_stream, int external) {
  if (!c) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (c->multi) return jxlhip_set_stream(c->multi->kids[0].ctx, hip_stream, external);  // the frame's consumer is on devices[0]
  const hipStream_t st = external ? (hipStream_t)hip_stream : c->own_stream;
  // the zeroing of the next frame's counter block is ordered on the OLD stream only: a new stream starts with a memset
  // -- and with a prepare of its own: the lists the old stream's k_prepare writes are ordered on that stream only
  if (st != c->stream) {
    c->counts_clean[0] = c->counts_clean[1] = false;
    DropPrepared(c);
  }
  c->stream = st;
  return JXLHIP_OK;
}

// ---- frame set-up -------------------------------------------------------------
int jxlhip_frame_begin(jxlhip_ctx* c, const jxlhip_frame_params* p) {
  if (c && p && p->undo_orientation > 8) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "undo_orientation %u", p->undo_orientation);
  if (!c || !p) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (c->multi) return MultiFrameBegin(c, p);
  if (p->xsize == 0 || p->ysize == 0 || p->xsize > (1u << 19) || p->ysize > (1u << 19))
    return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "frame size %ux%u out of range", p->xsize,
                p->ysize);
  if (p->coeff_type > JXLHIP_COEFF_I32 || p->output_kind > JXLHIP_OUT_PACKED)
    return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "bad coeff_type/output_kind");
  if (p->output_kind == JXLHIP_OUT_PACKED) {
    const jxlhip_output_format& o = p->out_format;
    const uint32_t max_bits = o.sample_type == JXLHIP_SAMPLE_U8 ? 8 : 16;
    if (o.transfer > JXLHIP_TF_HLG || o.sample_type > JXLHIP_SAMPLE_F16 ||
        ((o.transfer == JXLHIP_TF_PQ || o.transfer == JXLHIP_TF_GAMMA || o.transfer == JXLHIP_TF_HLG) &&
         !(o.tf_param > 0.0f)) ||
        (o.num_channels != 3 && o.num_channels != 4) || o.swap_endianness > 1 ||
        ((o.sample_type == JXLHIP_SAMPLE_U8 || o.sample_type == JXLHIP_SAMPLE_U16) &&
         (o.bits_per_sample == 0 || o.bits_per_sample > max_bits)))
      return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "bad output format");
  }
  if (p->global_scale <= 0 || p->quant_dc <= 0 || p->cfl_color_factor == 0)
    return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "bad quantizer parameters");
  if (p->lf.gab > 1 || p->lf.epf_iters > 3)
    return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "bad loop filter parameters");
  HIPCHK(c, hipSetDevice(c->device));
  // a new frame: the geometry, the constants and the buffers k_prepare reads and writes may all change below
  DropPrepared(c);
  c->capture_seen = false;
  DevFrame f{};
  f.xsize = p->xsize;
  f.ysize = p->ysize;
  f.xsb = (p->xsize + 7) / 8;
  f.ysb = (p->ysize + 7) / 8;
  f.xsg = (p->xsize + 255) / 256;
  f.ysg = (p->ysize + 255) / 256;
  f.xtiles = (f.xsb + 7) / 8;
  f.group_y0 = p->stripe_group_y0;
  f.group_rows = p->stripe_group_rows ? p->stripe_group_rows : f.ysg - f.group_y0;
  f.used_acs = p->used_acs & 0x7FFFFFFu;
  if (f.group_y0 >= f.ysg || f.group_y0 + f.group_rows > f.ysg)
    return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "stripe [%u,+%u) outside %u group rows",
                f.group_y0, f.group_rows, f.ysg);
  f.y0 = f.group_y0 * 256;
  f.y1 = (f.group_y0 + f.group_rows) * 256;
  if (f.y1 > f.ysize) f.y1 = f.ysize;
  f.fy0 = f.y0;
  f.fy1 = f.y1;
  f.band_g0 = f.group_y0;
  f.band_g1 = f.group_y0 + f.group_rows;
  static const uint32_t kEpfPad[4] = {0, 2, 3, 6};  // loop_filter.h:26-29
  f.halo = kEpfPad[p->lf.epf_iters] + p->lf.gab;
  f.coeff_type = p->coeff_type;
  f.inv_global_scale = (float)(1.0 * 65536 / p->global_scale);   // quantizer.h:82-85
  f.quant_scale = (float)(p->global_scale * (1.0 / 65536));
  f.x_dm = p->x_dm_multiplier;
  f.b_dm = p->b_dm_multiplier;
  memcpy(f.biases, p->quant_biases, sizeof(f.biases));
  f.cfl_base_x = p->cfl_base_x;
  f.cfl_base_b = p->cfl_base_b;
  f.color_scale = 1.0f / (float)p->cfl_color_factor;
  // XYB planes, block-major: the stripe's block rows plus one tile row above
  // and below for the halo rows (halo <= 7 < 8)
  const uint32_t rows_blocks = (f.group_y0 + f.group_rows) * 32 > f.ysb
                                   ? f.ysb * 8 - f.y0
                                   : f.group_rows * 256;
  f.tile_stride = (f.xsb + 1) & ~1u;
  f.plane_y0 = (int32_t)f.y0 - 8;
  f.plane_tile_rows = rows_blocks / 8 + 2;
  const size_t plane_floats = (size_t)f.plane_tile_rows * f.tile_stride * 64;
  int rc;
  if ((rc = c->planes.Reserve(c, 3 * plane_floats))) return rc;
  for (int ch = 0; ch < 3; ch++) f.xyb[ch] = c->planes + ch * plane_floats;
  if (p->lf.epf_iters == 3 && (rc = c->planes2.Reserve(c, 3 * plane_floats))) return rc;
  if ((rc = c->inv_sigma.Reserve(c, (size_t)f.xsb * f.ysb))) return rc;
  f.inv_sigma = c->inv_sigma;
  f.error_flag = c->error_flag;
  // work lists, worst case per class
  const size_t cells = (size_t)f.xsg * f.group_rows * 1024;
  size_t total = 0;
  size_t offs[kNumClasses];
  for (int k = 0; k < kNumClasses; k++) {
    offs[k] = total;
    const size_t m = cells / ClassMinCovered(k);
    c->max_items[k] = (uint32_t)m;
    total += m;
  }
  // +64: transform kernels fetch their list entry before they know the count
  if ((rc = c->lists.Reserve(c, total + 64))) return rc;
  for (int k = 0; k < kNumClasses; k++) c->wl.list[k] = c->lists + offs[k];
  c->wl.count = c->counts;
  // stage parameters, computed as the reference stages do
  FilterParams fp{};
  for (int ch = 0; ch < 3; ch++) {
    float w0 = 1.0f, w1 = p->lf.gab_weights[2 * ch], w2 = p->lf.gab_weights[2 * ch + 1];
    const float div = w0 + 4 * (w1 + w2);  // stage_gaborish.cc:36-53
    const float mul = 1.0f / div;
    fp.gab_w[ch][0] = w0 * mul;
    fp.gab_w[ch][1] = w1 * mul;
    fp.gab_w[ch][2] = w2 * mul;
    fp.ch_scale[ch] = p->lf.epf_channel_scale[ch];
    fp.opsin_bias[ch] = p->opsin_biases[ch];
    fp.cbrt_bias[ch] = cbrtf(p->opsin_biases[ch]);  // dec_xyb.cc:158-161
  }
  // stage_epf.cc:98-115,237-255,428-446
  fp.sm[0] = (float)(p->lf.epf_pass0_sigma_scale * 1.65);
  fp.sm[1] = 1.65f;
  fp.sm[2] = (float)(p->lf.epf_pass2_sigma_scale * 1.65);
  for (int i = 0; i < 3; i++) fp.bsm[i] = fp.sm[i] * p->lf.epf_border_sad_mul;
  memcpy(fp.minv, p->inverse_opsin_matrix, sizeof(fp.minv));
  for (int j = 0; j < 3; j++)
    for (int k = 0; k < 4; k++) fp.mcol[j][k] = fp.minv[3 * (k % 3) + j];
  for (int ch = 0; ch < 3; ch++) {
    fp.xyb_bias[ch] = -fp.cbrt_bias[ch];
    fp.xyb_bias[3 + ch] = fp.opsin_bias[ch];
  }
  if (p->output_kind == JXLHIP_OUT_PACKED) {
    fp.fmt = p->out_format;
    const bool is_int = fp.fmt.sample_type == JXLHIP_SAMPLE_U8 || fp.fmt.sample_type == JXLHIP_SAMPLE_U16;
    fp.sample_mul = is_int ? (float)((1u << fp.fmt.bits_per_sample) - 1u) : 1.0f;  // stage_write.cc:528
    fp.dither = c->tables + kTabDither;
    // TF_PQ's display_scaling_factor_to_10000_nits_ (transfer_functions-inl.h:146-148)
    fp.tf_scale = fp.fmt.transfer == JXLHIP_TF_PQ ? fp.fmt.tf_param * (1.0f / 10000.0f) : fp.fmt.tf_param;
    fp.hlg_exponent = 0.0f;
    if (fp.fmt.transfer == JXLHIP_TF_HLG) {
      // HlgOOTF::ToSceneLight + HlgOOTF_Base (cms/tone_mapping-inl.h:113-119, tone_mapping.h:120-126)
      const float gamma = (1 / 1.2f) * powf(1.111f, -log2f(fp.fmt.tf_param / 1000.f));
      const float e = gamma - 1;
      if (e < -0.01f || 0.01f < e) fp.hlg_exponent = e;
    }
  }
  memcpy(c->lut.v, p->lf.epf_sharp_lut, sizeof(c->lut.v));
  {
    // undo_orientation: the kernels write coded orientation into a staging frame (DecodeFrame below), only the
    // 8-bit dither pattern has to follow the flipped coordinates already
    const uint32_t o = p->undo_orientation;
    const bool fx = o == 2 || o == 3 || o == 7 || o == 8, fy = o == 3 || o == 4 || o == 6 || o == 7;
    fp.dither_x0 = fx ? (int32_t)p->xsize - 1 : 0;
    fp.dither_xs = fx ? -1 : 1;
    fp.dither_y0 = fy ? (int32_t)p->ysize - 1 : 0;
    fp.dither_ys = fy ? -1 : 1;
  }
  c->fp = fp;
  c->f = f;
  c->p = *p;
  {
    const int rc = BeginHandover(c);
    if (rc) return rc;
    c->handover_fresh = true;
  }
  c->have_frame = true;
  c->have_inputs = false;
  c->blocks_done = false;
  c->st.ResetFrame();
  return JXLHIP_OK;
}

void jxlhip::ApplyInputs(jxlhip_ctx* c, const jxlhip_frame_inputs* in) {
  c->f.coef_stride64 = in == &c->up_inputs ? 3072u : 1024u;
  for (int ch = 0; ch < 3; ch++) {
    c->f.coeffs[ch] = in->coeffs[ch];
    c->f.dc[ch] = in->dc[ch];
  }
  c->f.acs = in->ac_strategy;
  c->f.raw_quant = in->raw_quant;
  c->f.sharp = in->epf_sharpness;
  c->f.ytox = in->ytox_map;
  c->f.ytob = in->ytob_map;
  c->f.dequant = in->dequant_table;
}

int jxlhip_frame_set_inputs(jxlhip_ctx* c, const jxlhip_frame_inputs* in) {
  if (!c || !in) return JXLHIP_ERR_INVALID_ARGUMENT;
  JXLHIP_NO_MULTI(c);  // device pointers belong to one device: use the host-upload path
  if (!c->have_frame) return Fail(c, JXLHIP_ERR_STATE, "frame_set_inputs before frame_begin");
  for (int ch = 0; ch < 3; ch++)
    if (!in->coeffs[ch] || !in->dc[ch])
      return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "null coeffs/dc pointer");
  if (!in->ac_strategy || !in->raw_quant || !in->ytox_map || !in->ytob_map ||
      !in->dequant_table || (c->p.lf.epf_iters > 0 && !in->epf_sharpness))
    return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "null side-info pointer");
  if (((uintptr_t)in->dequant_table & 15) || ((uintptr_t)in->coeffs[0] & 15) ||
      ((uintptr_t)in->coeffs[1] & 15) || ((uintptr_t)in->coeffs[2] & 15))
    return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "coeffs/dequant_table must be 16-byte aligned");
  ApplyInputs(c, in);
  c->have_inputs = true;
  c->blocks_done = false;
  DropPrepared(c);  // (lazily prepared: the caller's arrays are first read by the first decode)
  return JXLHIP_OK;
}

int jxlhip_alpha_staging(jxlhip_ctx* c, float** plane, size_t* stride_floats) {
  if (!c || !plane || !stride_floats) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!c->have_frame) return Fail(c, JXLHIP_ERR_STATE, "alpha_staging before frame_begin");
  const size_t need = (size_t)c->f.xsize * c->f.ysize;
  if (need * sizeof(float) > c->alpha_host.bytes) {
    if (c->alpha_host.p) {
      const int rc = jxlhip_sync(c);  // nothing may still be reading the old plane
      if (rc) return rc;
    }
    if (c->alpha_host.Alloc(&c->mm, need * sizeof(float))) return Fail(c, JXLHIP_ERR_OUT_OF_MEMORY, "pinned alpha plane");
  }
  *plane = (float*)c->alpha_host.p;
  *stride_floats = c->f.xsize;
  return JXLHIP_OK;
}

// The alpha channel of the current frame for 4-channel packed outputs (what reaches WriteToOutputStage as
// input channel alpha_c, stage_write.cc:350-366); frame_begin resets to "opaque".
int jxlhip_set_alpha(jxlhip_ctx* c, const float* host_plane, size_t stride_floats) {
  if (!c || !host_plane) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!c->have_frame) return Fail(c, JXLHIP_ERR_STATE, "set_alpha before frame_begin");
  if (c->st.ups.factor > 1) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "alpha on an upsampled frame");
  if (c->st.patches.on) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "alpha on a frame with patches (they would have to blend it)");
  if (c->st.blend.on) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "alpha on a blended frame (blending extra channels is not in the back-end)");
  if (c->st.dc_only.on) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "alpha on a frame with DC-only groups");
  if (c->multi) {  // every stripe takes its own rows of the plane
    for (MultiChild& k : c->multi->kids) {
      const int rc = jxlhip_set_alpha(k.ctx, host_plane, stride_floats);
      if (rc) return MultiCheck(c, k.ctx, rc);
    }
    return JXLHIP_OK;
  }
  const size_t w = c->f.xsize, y0 = c->f.y0, rows = c->f.y1 - c->f.y0;
  if (stride_floats < w) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "alpha stride %zu < xsize", stride_floats);
  HIPCHK(c, hipSetDevice(c->device));
  const int rc = c->alpha_dev.Reserve(c, w * rows);
  if (rc) return rc;
  // the rows of this context's stripe; the kernels index the plane by IMAGE row: the base pointer is that of row 0
  HIPCHK(c, hipMemcpy2DAsync(c->alpha_dev, w * sizeof(float), host_plane + y0 * stride_floats, stride_floats * sizeof(float),
                             w * sizeof(float), rows, hipMemcpyHostToDevice, c->stream));
  c->fp.alpha = c->alpha_dev - y0 * w;
  c->fp.alpha_stride = (uint32_t)w;
  return JXLHIP_OK;
}

// ---- decode -------------------------------------------------------------------
bool jxlhip::Capturing(hipStream_t st) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(st, &cap);
  return cap == hipStreamCaptureStatusActive;
}

namespace {

// Phase 1 over the context's whole stripe (DevFrame::band_g0 / band_g1 = its group rows, set by jxlhip_frame_begin), in
// two steps: "prepare" (EnqueuePrepare: the counter-block zeroing, the cell_info fill of a fused stripe, k_prepare) and
// "blocks" (the transform kernels, which only READ the list lengths).
//
// Prepare once per hand-over.  k_prepare reads side info and frame constants only -- ac_strategy, raw_quant,
// epf_sharpness, ytox_map, ytob_map, the geometry, the stripe, used_acs, coef_stride64, `fused`, the quantizer scale and
// the sharpness LUT -- never a coefficient, and its outputs (work lists and their lengths, cell_info, inv_sigma, the
// error flag) are a function of those, up to the order inside a list.  So a DIRECT phase 1 whose key -- `fused` and the
// hand-over generation -- matches the prepare the context remembers launches the blocks on the remembered counter block
// and no k_prepare: a progressive pass, a second output format, a loop that refreshes coefficients only.  The reference
// has this work in the same place: ComputeSigma runs when a DC group's AC metadata is decoded (dec_modular.cc:559), not
// per AC pass.  jxlhip_upload_side_info and jxlhip_decode_codestream enqueue the prepare right behind their side-info
// copies (PrepareAhead), under the host's entropy decode; the zero-copy jxlhip_frame_set_inputs stays lazy.
// Who writes what a prepare leaves behind, and so who ends the prepared state (DropPrepared / EnqueuePrepare):
//   work lists   k_prepare only; the buffer is (re)allocated by jxlhip_frame_begin
//   counters     the memset / LaunchZeroU32 below, k_prepare (its atomics on its own block, zero_counts on the other);
//                allocated once by jxlhip_create_ex
//   cell_info    k_prepare and the 0xFF fill below; reserved by EnqueuePrepare itself
//   inv_sigma    k_prepare only; reserved by jxlhip_frame_begin
//   error flag   k_prepare raises [0] (k_dequant_tables [1]); jxlhip_sync clears it when it reports it
//   the inputs   jxlhip_frame_set_inputs, jxlhip_upload_side_info, jxlhip_decode_codestream (with its used_acs update)
// -> jxlhip_frame_begin, those three hand-overs, jxlhip_set_stream to another stream (the prepare is ordered on the old
// one), a jxlhip_sync that reports JXLHIP_ERR_BAD_STREAM (the next decode must raise the flag again) and any HIP error
// inside a phase 1 drop the state; jxlhip_set_concurrency_hint and whatever else moves WantFused change the key.
// JXLHIP_PREPARE_ONCE=0: every phase 1 prepares.
//
// Every prepare takes its work-list counter block here.  Direct calls alternate between blocks 0 and 1: a block gets a
// memset only when it is not marked clean, and the k_prepare of one call zeroes the block the next PREPARE will use
// (DevFrame::zero_counts) -- no memset launch per frame.  Under stream capture -- the caller records the frame's
// launches into a hipGraph and replays it (bench.py's `graph_replay`: the command processor's ~5-8 us per dependent
// launch are paid once per graph instead) -- nothing is reused: the captured frame carries its own k_prepare, every
// replay must find the SAME block zeroed by a node of the graph itself, and must not touch a block the direct calls
// keep a "clean" flag for: kCaptureBlock, zeroed by a kernel (see LaunchZeroU32: no memset node at the root of a frame
// graph).  A replay rewrites the shared lists behind the host's back: once a context has seen a capture, its direct
// calls prepare every time until the next jxlhip_frame_begin.
// fused: 0 = two-phase, 1 = the whole frame through the fused kernel, 2 = a STRIPE through it (the DCT8 cells of
// the stripe's first / last block row are decoded into the planes as well: they are the halo rows its neighbours pull)
// the frame as both steps of phase 1 see it
DevFrame Phase1Frame(const jxlhip_ctx* c, int fused) {
  DevFrame f = c->f;
  f.fused = (uint32_t)fused;
  f.cell_info = c->cell_info;
  // DCT32X32 / DCT16X16 on the matrix cores: the rule is PickMfma's (phase1_plan.h)
  const Phase1Mfma m = PickMfma(f.used_acs, (uint64_t)f.xsize * f.ysize, c->mfma);
  f.mfma32 = m.mfma32 ? c->tables + kTabMfma32 : nullptr;
  f.mfma16 = m.mfma16 ? c->tables + kTabMfma16 : nullptr;
  return f;
}

// The prepare step on c->stream; *block = the counter block it counted into.  A direct one becomes the context's
// prepared state when everything was enqueued without an error.
int EnqueuePrepare(jxlhip_ctx* c, int fused, bool capturing, int* block_out) {
  hipStream_t st = c->stream;
  c->prepared = false;  // (what the last prepare left is overwritten from here on; a replay will overwrite this one's)
  c->prepared_ahead = false;
  if (capturing) c->capture_seen = true;
  int rc;
  if (fused && (rc = c->cell_info.Reserve(c, (size_t)c->f.xsb * c->f.ysb))) return rc;
  const int block = capturing ? kCaptureBlock : c->counts_slot;
  uint32_t* counts = c->counts + (size_t)block * kCountStride;
  if (capturing) {
    LaunchZeroU32(counts, (uint32_t)kCountStride, st);
    HIPCHK(c, hipGetLastError());
  } else {
    if (!c->counts_clean[block]) HIPCHK(c, hipMemsetAsync(counts, 0, sizeof(uint32_t) * kCountStride, st));
    // From here on the block is in use: whatever happens below (a failed launch after k_prepare ran), it must not be
    // taken for clean by the next prepare.  Block ^ 1 becomes clean only when the launch that zeroes it succeeded.
    c->counts_clean[block] = false;
  }
  DevFrame f = Phase1Frame(c, fused);
  f.zero_counts = capturing ? nullptr : c->counts + (size_t)(block ^ 1) * kCountStride;
  if (fused == 2)  // a stripe: every cell "from the planes" until k_prepare says otherwise (whole frames: k_prepare writes every cell)
    HIPCHK(c, hipMemsetAsync(c->cell_info, 0xFF, sizeof(uint2) * (size_t)f.xsb * f.ysb, st));
  WorkLists wl = c->wl;
  wl.count = counts;
  ProfBegin(c);
  LaunchPrepare(f, wl, c->p.lf.epf_iters > 0, c->p.lf.epf_quant_mul, c->lut, st);
  ProfMark(c, JXLHIP_KERNEL_PREPARE);
  HIPCHK(c, hipGetLastError());
  *block_out = block;
  if (capturing) return JXLHIP_OK;
  c->counts_clean[block ^ 1] = true;
  c->counts_slot = block ^ 1;
  c->prepares_launched++;
  if (c->prepare_once && !c->capture_seen) {
    c->prepared = true;
    c->prepared_fused = fused;
    c->prepared_block = block;
    c->prepared_gen = c->handover_gen;
  }
  return JXLHIP_OK;
}

int LaunchPhase1(jxlhip_ctx* c, int fused = 0, const FilterParams* emit = nullptr) {
  hipStream_t st = c->stream;
  const bool capturing = Capturing(st);
  int block;
  if (!capturing && c->prepared && c->prepared_fused == fused && c->prepared_gen == c->handover_gen) {
    block = c->prepared_block;
    if (!c->prepared_ahead) c->prepares_reused++;
    c->prepared_ahead = false;
    ProfBegin(c);
    ProfMark(c, JXLHIP_KERNEL_PREPARE);  // (the span is still there: about 0, nothing was launched)
  } else {
    const int rc = EnqueuePrepare(c, fused, capturing, &block);
    if (rc) return rc;
  }
  const DevFrame f = Phase1Frame(c, fused);
  WorkLists wl = c->wl;
  wl.count = c->counts + (size_t)block * kCountStride;
  const uint32_t cells = f.xsg * f.group_rows * 1024u;
  LaunchBlocks(f, wl, cells, c->tables + kTabWc, c->tables + kTabResample, st, emit);
  ProfMark(c, JXLHIP_KERNEL_BLOCKS);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    c->prepared = false;
    return Fail(c, e == hipErrorOutOfMemory ? JXLHIP_ERR_OUT_OF_MEMORY : JXLHIP_ERR_HIP, "phase 1: %s", hipGetErrorString(e));
  }
  return JXLHIP_OK;
}

// epf_iters = 3: [Gaborish] + EPF0 into the second plane set -- from the fused producer's slab (k_fused_pc0) or from
// the planes (k_epf0) -- then EPF1 + EPF2 + output from there.  *declined: the EPF0 march does not take the geometry,
// nothing was launched.
int LaunchEpf0Then12(jxlhip_ctx* c, const DevFrame& f, const OutTarget& t, bool fused, bool* declined) {
  const FilterParams& fp = t.fp;
  float* dst[3];
  const size_t plane_floats = (size_t)f.plane_tile_rows * f.tile_stride * 64;
  for (int ch = 0; ch < 3; ch++) dst[ch] = c->planes2 + ch * plane_floats;
  const int gab = (int)c->p.lf.gab;
  *declined = !(fused ? LaunchFusedEpf0(f, fp, gab, dst, c->stream) : LaunchEpf0(f, fp, gab, dst, c->stream));
  if (*declined) return JXLHIP_OK;
  ProfMark(c, JXLHIP_KERNEL_EPF0);
  DevFrame f2 = f;
  for (int ch = 0; ch < 3; ch++) f2.xyb[ch] = dst[ch];
  f2.linear_stride = f.tile_stride * 32u;
  if (!LaunchFiltersFast(f2, fp, 0, 2, (int)t.kind, c->stream))
    return Fail(c, JXLHIP_ERR_STATE, "EPF1 + EPF2 march refused a frame the EPF0 march accepted");
  return JXLHIP_OK;
}

// phase 2 for pixel rows [fy0, fy1) of the stripe
int LaunchFiltersRows(jxlhip_ctx* c, const OutTarget& t, uint32_t fy0, uint32_t fy1, bool fused = false) {
  const FilterParams& fp = t.fp;
  DevFrame f = c->f;
  f.fy0 = fy0;
  f.fy1 = fy1;
  f.fused = fused ? 1u : 0u;
  f.cell_info = c->cell_info;
  ProfBegin(c);
  if (fused && c->p.lf.epf_iters == 3) {
    bool declined;
    const int rc = LaunchEpf0Then12(c, f, t, true, &declined);
    if (rc) return rc;
    if (declined) return Fail(c, JXLHIP_ERR_STATE, "fused EPF0 kernel refused a frame FusedEpf0Supported accepted");
    ProfMark(c, JXLHIP_KERNEL_FILTERS);
      HIPCHK(c, hipGetLastError());
    return JXLHIP_OK;
  }
  if (fused) {
    if (!LaunchFused(f, fp, (int)c->p.lf.gab, (int)c->p.lf.epf_iters, (int)t.kind, c->stream))
      return Fail(c, JXLHIP_ERR_STATE, "fused kernel refused a frame FusedSupported accepted");
    ProfMark(c, JXLHIP_KERNEL_FUSED);
      HIPCHK(c, hipGetLastError());
    return JXLHIP_OK;
  }
  bool fast = false;
  if (!c->generic_filters && fy1 > fy0 && c->p.lf.epf_iters == 3 && c->planes2) {
    bool declined;  // (then the generic kernel below)
    const int rc = LaunchEpf0Then12(c, f, t, false, &declined);
    if (rc) return rc;
    fast = !declined;
  } else if (!c->generic_filters && fy1 > fy0) {
    fast = LaunchFiltersFast(f, fp, (int)c->p.lf.gab, (int)c->p.lf.epf_iters, (int)t.kind, c->stream);
  }
  if (!fast && LaunchFilters(f, fp, (int)c->p.lf.gab, (int)c->p.lf.epf_iters, (int)t.kind, c->stream) != 0)
    return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "unsupported filter configuration");
  ProfMark(c, JXLHIP_KERNEL_FILTERS);
  HIPCHK(c, hipGetLastError());
  return JXLHIP_OK;
}

// Does this frame (or stripe of it) go through the fused kernel (kernels_fused.hip)?  auto: with a filter, frames
// of 12 Mpx and more (see jxlhip_ctx::fuse); without one the fused wave has no halo rows to pay for and wins at 4K as
// well (95.8 vs 83.4 Gpx/s); never when the caller's used_acs says the frame has no DCT8 block -- then the slab is
// only a detour (configs[4]: 76.1 vs 79.6 Gpx/s).  Packed outputs: the two-phase filter kernel has the formats djxl
// writes most (8-bit sRGB RGB / RGBA, 16-bit sRGB RGB) fixed at compile time, the fused kernel only the general
// per-sample format path -- measured at 8K d1.0: 0.42 ms two-phase against 0.74 - 0.82 ms fused
// (profiles/r03_packed_paths.txt).  kind, fmt: what the path would write (OutTarget).
bool WantFused(const jxlhip_ctx* c, uint32_t kind, const jxlhip_output_format& fmt) {
  const DevFrame& f = c->f;
  if (c->st.dc_only.on) return false;  // (the fused kernel decodes DCT8 cells from the coefficient stream and never sees the planes)
  // alone a context fuses from 12 Mpx; with several frames in flight on the device (jxlhip_set_concurrency_hint) the
  // step is bound by HBM traffic and the fused path, which moves less, pays from 6 Mpx (profiles/r04_path_choice.txt)
  const uint64_t min_px = c->concurrency > 1 ? (6ull << 20) : (12ull << 20);
  const bool big = (uint64_t)f.xsize * f.ysize >= min_px || (c->p.lf.gab == 0 && c->p.lf.epf_iters == 0);
  const bool has_dct8 = f.used_acs == 0 || (f.used_acs & 1u);
  const bool packed_fixed = kind == JXLHIP_OUT_PACKED && FastFixedFormat(fmt);
  if (c->p.lf.epf_iters == 3) {
    // three EPF iterations: EPF0 marches from the fused producer's slab (k_fused_pc0), the rest as before; whole frames
    // only, and only with several frames in flight on the device (jxlhip_set_concurrency_hint): the producer / consumer
    // form has half the marching waves of k_epf0 per CU and is slower on its own (8K d1.0: the EPF0 launch 0.33 against
    // 0.23 ms, the step 0.651 against 0.623 ms of kernels), but it moves the DCT8 share's 24 bytes per pixel less, and a
    // device kept busy by other frames is bound by traffic: 64.8 -> 67.0 Gpx/s with three in flight
    // (profiles/r04_epf3_fused.txt)
    const bool many = c->concurrency > 1 && (uint64_t)f.xsize * f.ysize >= (6ull << 20);
    return (c->fuse > 0 || (c->fuse < 0 && many && has_dct8)) && !c->generic_filters && c->planes2 &&
           f.group_y0 == 0 && f.group_rows == f.ysg && FusedEpf0Supported(f, (int)c->p.lf.gab);
  }
  return (c->fuse > 0 || (c->fuse < 0 && big && has_dct8 && !packed_fixed)) && !c->generic_filters &&
         FusedSupported(f, (int)c->p.lf.gab, (int)c->p.lf.epf_iters, (int)kind);
}

int BeginDecode(jxlhip_ctx* c) {
  if (!c->have_frame || !c->have_inputs)
    return Fail(c, JXLHIP_ERR_STATE, "decode needs frame_begin + inputs");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  {
    std::lock_guard<std::mutex> lock(c->pool_mu);
    for (int i = 0; i < kPoolStreams; i++) {
      if (!c->pool_dirty[i]) continue;
      HIPCHK(c, hipEventRecord(c->pool_ev[i], c->pool[i]));
      HIPCHK(c, hipStreamWaitEvent(st, c->pool_ev[i], 0));
      c->pool_dirty[i] = false;
    }
  }
  if (c->sp_any.load() && c->f.coeffs[0] == c->up_coeffs[0]) {
    // the groups that came up as non-zero lists: their offset table, then zero + scatter into the dense upload
    // buffer, behind the uploads.  (Idempotent: a second decode of the same frame repeats it.)
    const size_t ng = (size_t)c->f.xsg * c->f.ysg;
    const int par = (int)(c->frame_serial & 1u);
    int rc;
    if ((rc = c->sp_off_dev.Reserve(c, ng))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->sp_off_dev, c->sp_off_host[par].p, ng * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipEventRecord(c->sp_off_ev[par], st));
    c->sp_off_pending[par] = true;
    LaunchExpandSparse(c->sp_dev, c->sp_off_dev, (int16_t*)c->up_coeffs[0], c->f.group_y0 * c->f.xsg, c->f.group_rows * c->f.xsg, st);
  }
  return JXLHIP_OK;
}


}  // namespace

int jxlhip::CheckOutArgs(jxlhip_ctx* c, const OutTarget& t, size_t cols, size_t rows) {
  const size_t out_stride = t.fp.out_stride;
  if (!t.fp.out) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "null output");
  if (t.kind == JXLHIP_OUT_LINEAR_RGB_F32) {
    if (out_stride < cols * 12 || (out_stride & 3))
      return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "RGB row stride %zu too small", out_stride);
  } else if (t.kind == JXLHIP_OUT_PACKED) {
    const size_t ssz = OutSampleBytes(t.fmt);
    if (out_stride < cols * OutPixelBytes(t.kind, t.fmt) || (out_stride % ssz) || ((uintptr_t)t.fp.out % ssz))
      return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "packed row stride %zu / alignment invalid", out_stride);
  } else if (out_stride < cols || t.fp.out_plane_stride < out_stride * (rows - 1) + cols) {
    return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "XYB strides too small");
  }
  return JXLHIP_OK;
}

int jxlhip::PrepareAhead(jxlhip_ctx* c, bool render_stages) {
  if (!c->prepare_once || c->capture_seen || !c->have_frame || !c->have_inputs || Capturing(c->stream)) return JXLHIP_OK;
  // the mode the context would pick now: a whole frame goes through jxlhip_decode_frame (1 or 0), a stripe through the
  // split calls (2 or 0).  A decode that wants another one -- the split calls on a whole frame, a render stage that
  // changes the output kind -- prepares again: correct, and one launch.
  const bool stripe = c->f.group_y0 != 0 || c->f.group_rows != c->f.ysg;
  // (DecodeFrameFeatures and DecodeFrameToneMapped pass a planar target down)
  const bool planar = render_stages || c->st.RenderStagesOn() || c->st.tone_map.on;
  const int fused = WantFused(c, planar ? JXLHIP_OUT_XYB_PLANAR : c->p.output_kind, c->p.out_format) ? (stripe ? 2 : 1) : 0;
  int block;
  const int rc = EnqueuePrepare(c, fused, false, &block);
  c->prepared_ahead = rc == JXLHIP_OK && c->prepared;
  return rc;
}

int jxlhip_debug_prepare_launches(const jxlhip_ctx* c, uint64_t* launched, uint64_t* reused) {
  if (!c || !launched || !reused) return JXLHIP_ERR_INVALID_ARGUMENT;
  *launched = *reused = 0;
  if (c->multi) {
    for (const MultiChild& k : c->multi->kids) {
      *launched += k.ctx->prepares_launched;
      *reused += k.ctx->prepares_reused;
    }
    return JXLHIP_OK;
  }
  *launched = c->prepares_launched;
  *reused = c->prepares_reused;
  return JXLHIP_OK;
}

int jxlhip_decode_blocks(jxlhip_ctx* c) {
  if (!c) return JXLHIP_ERR_INVALID_ARGUMENT;
  JXLHIP_NO_MULTI(c);
  int rc = BeginDecode(c);
  if (rc) return rc;
  // A STRIPE of a frame (what jxlhip_create_multi / libjxl_amd.stripes run per device) takes the fused kernel
  // by the whole-frame rule: its DCT8 blocks are decoded inside the filter march, except that those of its
  // first / last block row ALSO reach the planes -- the halo rows the neighbours pull with jxlhip_halo_export.
  // A whole frame through the split calls stays two-phase (the taps read the planes).
  const bool stripe = c->f.group_y0 != 0 || c->f.group_rows != c->f.ysg;
  c->blocks_fused = stripe && WantFused(c, c->p.output_kind, c->p.out_format);
  if ((rc = ZeroDcOnlySlots(c))) return rc;
  rc = LaunchPhase1(c, c->blocks_fused ? 2 : 0);
  if (rc) return rc;
  if ((rc = LaunchDcOnly(c))) return rc;  // (the last launch of phase 1: jxlhip_export_xyb shows its output)
  c->blocks_done = true;
  return JXLHIP_OK;
}

int jxlhip_halo_rows(const jxlhip_ctx* c) {
  if (!c || !c->have_frame) return JXLHIP_ERR_STATE;
  return (int)c->f.halo;
}

static int HaloCopy(jxlhip_ctx* c, int which, float* dev, bool to_dense) {
  if (!c || !dev || which < 0 || which > 1) return JXLHIP_ERR_INVALID_ARGUMENT;
  JXLHIP_NO_MULTI(c);
  if (!c->have_frame) return Fail(c, JXLHIP_ERR_STATE, "halo copy before frame_begin");
  const DevFrame& f = c->f;
  const uint32_t stripe_rows = f.y1 - f.y0;
  if (f.halo > stripe_rows)
    return Fail(c, JXLHIP_ERR_STATE, "stripe of %u rows is shorter than the %u-row halo",
                stripe_rows, f.halo);
  if (f.halo == 0) return JXLHIP_OK;
  int y_first;
  if (to_dense) y_first = which == 0 ? (int)f.y0 : (int)(f.y1 - f.halo);
  else y_first = which == 0 ? (int)f.y0 - (int)f.halo : (int)f.y1;
  if (y_first < 0 || y_first + (int)f.halo > (int)f.ysize)
    return Fail(c, JXLHIP_ERR_STATE, "no neighbouring stripe on that side");
  HIPCHK(c, hipSetDevice(c->device));
  LaunchRowsCopy(f, dev, y_first, (int)f.halo, (int)f.xsize, f.xsize,
                 (size_t)f.halo * f.xsize, 3, to_dense, c->stream);
  HIPCHK(c, hipGetLastError());
  return JXLHIP_OK;
}

int jxlhip_halo_export(jxlhip_ctx* c, int which, float* dev) {
  if (c && !c->blocks_done) return Fail(c, JXLHIP_ERR_STATE, "halo_export before decode_blocks");
  return HaloCopy(c, which, dev, true);
}

int jxlhip_halo_import(jxlhip_ctx* c, int which, const float* dev) {
  return HaloCopy(c, which, const_cast<float*>(dev), false);
}

int jxlhip_decode_filters(jxlhip_ctx* c, void* out, size_t out_stride, size_t out_plane_stride) {
  if (!c) return JXLHIP_ERR_INVALID_ARGUMENT;
  return jxlhip_decode_filters_rows(c, out, out_stride, out_plane_stride, c->f.y0, c->f.y1);
}

int jxlhip_decode_filters_rows(jxlhip_ctx* c, void* out, size_t out_stride, size_t out_plane_stride, uint32_t y_begin,
                               uint32_t y_end) {
  if (!c) return JXLHIP_ERR_INVALID_ARGUMENT;
  JXLHIP_NO_MULTI(c);
  if (!c->blocks_done) return Fail(c, JXLHIP_ERR_STATE, "decode_filters before decode_blocks");
  if (c->p.undo_orientation > 1) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "undo_orientation with the split calls");
  if (c->st.noise.on) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "noise with the split calls (jxlhip_decode_frame takes it)");
  if (c->st.splines.on) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "splines with the split calls (jxlhip_decode_frame takes them)");
  if (c->st.patches.on) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "patches with the split calls (jxlhip_decode_frame takes them)");
  if (c->st.ups.factor > 1) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "upsampling with the split calls (jxlhip_decode_frame takes it)");
  if (c->st.blend.on) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "blending with the split calls (jxlhip_decode_frame takes it)");
  if (c->st.tone_map.on) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "tone mapping with the split calls (jxlhip_decode_frame takes it)");
  const OutTarget t = MakeTarget(c, out, out_stride, out_plane_stride);
  int rc = CheckOutArgs(c, t, c->f.xsize, c->f.y1 - c->f.y0);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const bool whole = y_begin == c->f.y0 && y_end == c->f.y1;
  if (!whole) {
    if (y_begin == y_end && y_begin >= c->f.y0 && y_end <= c->f.y1) return JXLHIP_OK;  // (an edge stripe has no boundary rows on its outer side)
    if (y_begin < c->f.y0 || y_end > c->f.y1 || y_begin > y_end ||
        ((y_begin & 7u) && y_begin != c->f.y0) || ((y_end & 7u) && y_end != c->f.y1))
      return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "rows [%u, %u) of a stripe [%u, %u): block-row multiples inside it only", y_begin,
                  y_end, c->f.y0, c->f.y1);
    if (c->p.lf.epf_iters == 3) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "row ranges with epf_iters = 3 (two marches over a second plane set)");
  }
  return LaunchFiltersRows(c, t, y_begin, y_end, c->blocks_fused);
}

// ---- one stripe step in three calls (round 5) ----------------------------------------------------
// What a rank of the striped decode (libjxl_amd/stripes.py: one process per GPU) enqueues around its halo exchange was
// seven to nine C calls per frame -- phase 1, two exports, up to three row ranges of phase 2, two imports -- each
// through the host language's FFI: on a 16K frame over 8 GPUs a rank's kernels take ~170 us, and the host must not take
// as long to enqueue them.  jxlhip_stripe_begin = phase 1 + both exports; [the caller posts its sends / receives, then
// jxlhip_decode_filters_rows for the interior]; jxlhip_stripe_finish = both imports + the boundary block rows.
// send_* / recv_* = dense [3][halo][xsize] device buffers, nullptr = no neighbour on that side.
int jxlhip_stripe_begin(jxlhip_ctx* c, float* send_up, float* send_down) {
  int rc = jxlhip_decode_blocks(c);
  if (rc) return rc;
  if (send_up && (rc = jxlhip_halo_export(c, 0, send_up))) return rc;
  if (send_down && (rc = jxlhip_halo_export(c, 1, send_down))) return rc;
  return JXLHIP_OK;
}

// y_interior_begin / _end: the rows jxlhip_decode_filters_rows has filtered already between the two calls (equal:
// none -- everything is filtered here, behind the imports)
int jxlhip_stripe_finish(jxlhip_ctx* c, const float* recv_up, const float* recv_down, void* out, size_t out_stride,
                         size_t out_plane_stride, uint32_t y_interior_begin, uint32_t y_interior_end) {
  if (!c) return JXLHIP_ERR_INVALID_ARGUMENT;
  int rc;
  if (recv_up && (rc = jxlhip_halo_import(c, 0, recv_up))) return rc;
  if (recv_down && (rc = jxlhip_halo_import(c, 1, recv_down))) return rc;
  if (y_interior_begin >= y_interior_end) return jxlhip_decode_filters(c, out, out_stride, out_plane_stride);
  if ((rc = jxlhip_decode_filters_rows(c, out, out_stride, out_plane_stride, c->f.y0, y_interior_begin))) return rc;
  return jxlhip_decode_filters_rows(c, out, out_stride, out_plane_stride, y_interior_end, c->f.y1);
}

// Both phases, each over the whole stripe.
int jxlhip_decode_frame(jxlhip_ctx* c, void* out, size_t out_stride, size_t out_plane_stride) {
  if (!c) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (c->multi) return out ? MultiDecodeFrame(c, out, nullptr, out_stride, out_plane_stride) : JXLHIP_ERR_INVALID_ARGUMENT;
  if (!c->have_frame) return Fail(c, JXLHIP_ERR_STATE, "decode needs frame_begin + inputs");
  if (c->st.tone_map.on) return DecodeFrameToneMapped(c, out, out_stride);
  if (c->st.blend.on) return DecodeFrameBlended(c, out, out_stride);
  if (c->p.undo_orientation <= 1 || c->st.RenderStagesOn()) return DecodeFrameOwnPath(c, MakeTarget(c, out, out_stride, out_plane_stride));
  // undo_orientation: coded orientation into a staging frame, k_orient into the caller's buffer
  const DevFrame& f = c->f;
  const size_t bpp = OutPixelBytes(c);
  if (!out || bpp == 0) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "undo_orientation needs an interleaved output");
  if (f.group_y0 != 0 || f.group_rows != f.ysg) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "undo_orientation with stripes");
  const bool transposed = c->p.undo_orientation >= 5;
  const size_t need = (size_t)(transposed ? f.ysize : f.xsize) * bpp;
  if (out_stride < need) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "row stride %zu too small for the oriented frame", out_stride);
  HIPCHK(c, hipSetDevice(c->device));
  const size_t row = ((size_t)f.xsize * bpp + 255) & ~(size_t)255;
  int rc;
  if ((rc = c->orient_dev.Reserve(c, (size_t)f.ysize * row))) return rc;
  if ((rc = DecodeFrameCoded(c, MakeTarget(c, c->orient_dev, row, 0)))) return rc;
  if (!LaunchOrient(c->orient_dev, row, f.xsize, f.ysize, (uint32_t)bpp, c->p.undo_orientation, out, out_stride, c->stream))
    return Fail(c, JXLHIP_ERR_UNSUPPORTED, "undo_orientation %u with %zu-byte pixels", c->p.undo_orientation, bpp);
  HIPCHK(c, hipGetLastError());
  return JXLHIP_OK;
}

int jxlhip::DecodeFrameCoded(jxlhip_ctx* c, const OutTarget& t) {
  const DevFrame& f = c->f;
  c->blocks_fused = false;
  int rc = BeginDecode(c);
  if (rc) return rc;
  rc = CheckOutArgs(c, t, f.xsize, f.y1 - f.y0);  // (always at coded size here)
  if (rc) return rc;
  // A frame of DCT32X32 varblocks only, no loop filter, linear float RGB out (BASELINE configs[4]): the matrix-core
  // class kernel applies the opsin inverse and writes the pixels itself (kernels_mfma.hip, EMIT) -- no XYB planes,
  // no second kernel.  used_acs is the caller's promise; k_prepare reports any other strategy it meets.
  if (c->mfma != 0 && f.used_acs == (1u << 5) && c->p.lf.gab == 0 && c->p.lf.epf_iters == 0 &&
      t.kind == JXLHIP_OUT_LINEAR_RGB_F32 && !c->generic_filters && !c->st.dc_only.on) {
    rc = LaunchPhase1(c, 0, &t.fp);
    c->blocks_done = false;  // nothing in the planes
    return rc;
  }
  // Whole frame on this context: the fused kernel decodes the DCT8 blocks inside the filter march (kernels_fused.hip;
  // WantFused says when).  The split calls (jxlhip_decode_blocks / _filters) stay two-phase: a stripe's halo rows must
  // exist in the planes for its neighbours.
  if (WantFused(c, t.kind, t.fmt) && f.group_y0 == 0 && f.group_rows == f.ysg) {
    if ((rc = LaunchPhase1(c, 1))) return rc;
    c->blocks_done = false;  // the planes do not hold the whole frame
    return LaunchFiltersRows(c, t, f.y0, f.y1, true);
  }
  // (a frame with DC-only groups always comes here: WantFused; k_dc_upsample8 between phase 1 and the filters)
  if ((rc = ZeroDcOnlySlots(c))) return rc;
  if ((rc = LaunchPhase1(c))) return rc;
  if ((rc = LaunchDcOnly(c))) return rc;
  c->blocks_done = true;
  return LaunchFiltersRows(c, t, f.y0, f.y1);
}

// The boundary handing over a HOST buffer (what JxlDecoderSetImageOutBuffer gives libjxl): both phases
// into a context-owned device frame, one strided device-to-host copy, synchronised.
int jxlhip_decode_frame_host(jxlhip_ctx* c, void* host_out, size_t out_stride, size_t out_plane_stride) {
  if (!c || !host_out) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (c->multi) {
    const int rc = MultiDecodeFrame(c, nullptr, host_out, out_stride, out_plane_stride);
    return rc ? rc : MultiSync(c);
  }
  if (!c->have_frame) return Fail(c, JXLHIP_ERR_STATE, "decode needs frame_begin + inputs");
  const DevFrame& f = c->f;
  const bool transposed = c->p.undo_orientation >= 5;  // the oriented frame is ysize wide, xsize high
  const size_t rows = transposed ? f.xsize : BufRows(c);  // (an upsampled or blended frame is never transposed)
  const size_t cols = transposed ? f.ysize : BufCols(c);
  const bool planar = c->p.output_kind == JXLHIP_OUT_XYB_PLANAR;
  const size_t row_bytes = cols * (planar ? 4 : OutPixelBytes(c));
  const size_t host_row = planar ? out_stride * 4 : out_stride;
  if (host_row < row_bytes) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "host row stride %zu too small", out_stride);
  const size_t dev_row = (row_bytes + 255) & ~(size_t)255;
  const size_t planes = planar ? 3 : 1;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = c->host_frame_dev.Reserve(c, planes * rows * dev_row))) return rc;
  rc = planar ? jxlhip_decode_frame(c, c->host_frame_dev, dev_row / 4, rows * dev_row / 4)
              : jxlhip_decode_frame(c, c->host_frame_dev, dev_row, 0);
  if (rc) return rc;
  for (size_t pl = 0; pl < planes; pl++)
    HIPCHK(c, hipMemcpy2DAsync((char*)host_out + pl * out_plane_stride * 4, host_row, c->host_frame_dev + pl * rows * dev_row,
                               dev_row, row_bytes, rows, hipMemcpyDeviceToHost, c->stream));
  return jxlhip_sync(c);
}

int jxlhip_decode_frame_pinned(jxlhip_ctx* c, const void** host_frame, size_t* stride) {
  if (!c || !host_frame || !stride) return JXLHIP_ERR_INVALID_ARGUMENT;
  const jxlhip_frame_params& p = c->p;
  if (p.output_kind == JXLHIP_OUT_XYB_PLANAR) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "pinned frames are interleaved outputs");
  const bool transposed = p.undo_orientation >= 5;
  // (a multi-device parent's c->f is its first child's stripe: the whole frame there, and no stage is ever on)
  const size_t rows = transposed ? p.xsize : c->multi ? p.ysize : BufRows(c);
  const size_t cols = transposed ? p.ysize : BufCols(c);
  const size_t row_bytes = cols * OutPixelBytes(c);
  const size_t pitch = (row_bytes + 63) & ~(size_t)63;
  if (rows * pitch > c->pinned_frame.bytes) {
    if (c->pinned_frame.p) {
      int rc0 = jxlhip_sync(c);  // nothing may still be writing the old frame
      if (rc0) return rc0;
    }
    if (c->pinned_frame.Alloc(&c->mm, rows * pitch)) return Fail(c, JXLHIP_ERR_OUT_OF_MEMORY, "pinned frame of %zu bytes", rows * pitch);
  }
  const int rc = jxlhip_decode_frame_host(c, c->pinned_frame.p, pitch, 0);
  if (rc) return rc;
  *host_frame = c->pinned_frame.p;
  *stride = pitch;
  return JXLHIP_OK;
}

int jxlhip_sync(jxlhip_ctx* c) {
  if (!c) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (c->multi) return MultiSync(c);
  HIPCHK(c, hipSetDevice(c->device));
  int32_t flag[2] = {0, 0};
  HIPCHK(c, hipMemcpyAsync(flag, c->error_flag, sizeof(flag), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (flag[0] || flag[1]) {
    // the flag is k_prepare's to raise: the next decode of the same inputs prepares again and reports the map again
    DropPrepared(c);
    HIPCHK(c, hipMemsetAsync(c->error_flag, 0, sizeof(flag), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return Fail(c, JXLHIP_ERR_BAD_STREAM,
                flag[0] ? "AC strategy map violates the group/stream constraints "
                          "(dec_modular.cc:539-549, dec_group.cc:359)"
                        : "dequant table weight out of range (quant_weights.cc:329-339)");
  }
  return JXLHIP_OK;
}

// ---- taps ------------------------------------------------------------------------
int jxlhip_export_xyb(jxlhip_ctx* c, float* const dst[3], size_t dst_stride) {
  if (!c || !dst || !dst[0] || !dst[1] || !dst[2]) return JXLHIP_ERR_INVALID_ARGUMENT;
  JXLHIP_NO_MULTI(c);
  if (!c->have_frame) return Fail(c, JXLHIP_ERR_STATE, "no frame");
  if (!c->blocks_done || c->blocks_fused)
    return Fail(c, JXLHIP_ERR_STATE, "export_xyb needs a two-phase jxlhip_decode_blocks (a fused decode -- jxlhip_decode_frame, or "
                                     "a stripe of a frame of 12 Mpx and more -- leaves DCT8 blocks out of the planes; JXLHIP_FUSE=0)");
  const DevFrame& f = c->f;
  const int rows = (int)(f.plane_tile_rows - 2) * 8;
  if (dst_stride < (size_t)f.xsb * 8) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "stride too small");
  HIPCHK(c, hipSetDevice(c->device));
  // the three destination planes may be separate allocations: one launch each
  for (int ch = 0; ch < 3; ch++) {
    DevFrame g = f;
    g.xyb[0] = f.xyb[ch];
    LaunchRowsCopy(g, dst[ch], (int)f.y0, rows, (int)f.xsb * 8, dst_stride, 0, 1, true, c->stream);
  }
  HIPCHK(c, hipGetLastError());
  return JXLHIP_OK;
}

int jxlhip_get_sigma(jxlhip_ctx* c, float** inv_sigma, size_t* row_stride) {
  if (!c || !inv_sigma || !row_stride) return JXLHIP_ERR_INVALID_ARGUMENT;
  JXLHIP_NO_MULTI(c);
  if (!c->have_frame) return Fail(c, JXLHIP_ERR_STATE, "no frame");
  *inv_sigma = c->f.inv_sigma;
  *row_stride = c->f.xsb;
  return JXLHIP_OK;
}

int jxlhip_set_concurrency_hint(jxlhip_ctx* c, int frames_in_flight) {
  if (!c || frames_in_flight < 1) return JXLHIP_ERR_INVALID_ARGUMENT;
  c->concurrency = frames_in_flight;
  if (c->multi)
    for (MultiChild& k : c->multi->kids) k.ctx->concurrency = frames_in_flight;
  return JXLHIP_OK;
}

int jxlhip_profile_enable(jxlhip_ctx* c, int enable) {
  if (!c) return JXLHIP_ERR_INVALID_ARGUMENT;
  JXLHIP_NO_MULTI(c);
  c->profiling = enable != 0;
  return JXLHIP_OK;
}

int jxlhip_profile_read(jxlhip_ctx* c, float ms[JXLHIP_KERNEL_COUNT],
                        uint32_t launches[JXLHIP_KERNEL_COUNT]) {
  return jxlhip_profile_read_ex(c, ms, launches, JXLHIP_KERNEL_COUNT);
}

int jxlhip_profile_read_ex(jxlhip_ctx* c, float* ms, uint32_t* launches, uint32_t count) {
  if (!c || !ms || !launches || count > JXLHIP_KERNEL_COUNT_EX) return JXLHIP_ERR_INVALID_ARGUMENT;
  JXLHIP_NO_MULTI(c);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < (int)count; i++) {
    ms[i] = 0;
    launches[i] = 0;
  }
  for (size_t i = 0; i + 1 < c->marks.size(); i++) {
    const int slot = c->marks[i].slot_after;
    if (slot >= 0 && slot < (int)count) {
      float t = 0;
      if (hipEventElapsedTime(&t, c->marks[i].ev, c->marks[i + 1].ev) == hipSuccess) {
        ms[slot] += t;
        launches[slot]++;
      }
    }
  }
  c->marks.clear();
  return JXLHIP_OK;
}

// ---- a5 / a8 ------------------------------------------------------------------------
// Library encodings -> the parameters they stand for (DequantMatrices::Library,
// quant_weights.cc:532-1188; data in format_constants.inc).  The AFV library entry
// takes its 4x8 and 4x4 band parameters from the DCT4X8 and DCT4X4 entries.
static void ResolveLibrary(int kind, jxlhip_quant_encoding* e) {
  static const uint32_t kModeOfLib[6] = {JXLHIP_QUANT_DCT,  JXLHIP_QUANT_ID,     JXLHIP_QUANT_DCT2,
                                         JXLHIP_QUANT_DCT4, JXLHIP_QUANT_DCT4X8, JXLHIP_QUANT_AFV};
  const QuantLibEntry& l = kQuantLib[kind];
  memset(e, 0, sizeof(*e));
  e->mode = kModeOfLib[l.mode];
  const QuantLibEntry& b = l.mode == 5 ? kQuantLib[9] : l;
  e->num_bands = (uint32_t)b.nb;
  for (int c = 0; c < 3; c++) {
    for (int i = 0; i < 8; i++) e->bands[c][i] = b.bands[c][i];
    for (int i = 0; i < 9; i++) e->weights[c][i] = l.w[c][i];
  }
  if (l.mode == 5) {
    e->num_bands_afv_4x4 = (uint32_t)kQuantLib[3].nb;
    for (int c = 0; c < 3; c++)
      for (int i = 0; i < 8; i++) e->bands_afv_4x4[c][i] = kQuantLib[3].bands[c][i];
  }
}

int jxlhip_dequant_tables(jxlhip_ctx* c, const jxlhip_quant_encoding* enc, float* table_dev) {
  if (!c || !table_dev) return JXLHIP_ERR_INVALID_ARGUMENT;
  JXLHIP_NO_MULTI(c);
  static const uint32_t kSingleBlockKinds = 0x60F;  // kinds whose matrix is one 8x8 block
  for (int k = 0; k < JXLHIP_NUM_QUANT_TABLES; k++) {
    jxlhip_quant_encoding* e = &c->quant_enc_host[k];
    if (!enc || enc[k].mode == JXLHIP_QUANT_LIBRARY) {
      ResolveLibrary(k, e);
      continue;
    }
    *e = enc[k];
    if (e->mode == JXLHIP_QUANT_RAW)
      return Fail(c, JXLHIP_ERR_UNSUPPORTED, "kQuantModeRAW dequant tables are modular-coded");
    const bool has_bands = e->mode == JXLHIP_QUANT_DCT || e->mode == JXLHIP_QUANT_DCT4 ||
                           e->mode == JXLHIP_QUANT_DCT4X8 || e->mode == JXLHIP_QUANT_AFV;
    if (e->mode > JXLHIP_QUANT_RAW || (e->mode != JXLHIP_QUANT_DCT && !((kSingleBlockKinds >> k) & 1)) ||
        (has_bands && (e->num_bands < 1 || e->num_bands > JXLHIP_MAX_DISTANCE_BANDS)) ||
        (e->mode == JXLHIP_QUANT_AFV &&
         (e->num_bands_afv_4x4 < 1 || e->num_bands_afv_4x4 > JXLHIP_MAX_DISTANCE_BANDS)))
      return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "malformed quant encoding");
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(c->quant_enc, c->quant_enc_host, sizeof(c->quant_enc_host), hipMemcpyHostToDevice,
                           c->stream));
  LaunchDequantTables(table_dev, c->quant_enc, c->error_flag + 1, c->stream);
  HIPCHK(c, hipGetLastError());
  return JXLHIP_OK;
}

int jxlhip_default_dequant_tables(jxlhip_ctx* c, float* table_dev) {
  return jxlhip_dequant_tables(c, nullptr, table_dev);
}

int jxlhip_dequant_dc(jxlhip_ctx* c, const int32_t* const quant_dc[3], float* const dc_out[3],
                      const float dc_quant[3], float cfl_x_dc, float cfl_b_dc, int smooth) {
  return jxlhip_dequant_dc_groups(c, quant_dc, dc_out, dc_quant, cfl_x_dc, cfl_b_dc, smooth, nullptr);
}

int jxlhip_dequant_dc_groups(jxlhip_ctx* c, const int32_t* const quant_dc[3], float* const dc_out[3],
                             const float dc_quant[3], float cfl_x_dc, float cfl_b_dc, int smooth,
                             const uint8_t* extra_precision) {
  if (!c || !quant_dc || !dc_out) return JXLHIP_ERR_INVALID_ARGUMENT;
  JXLHIP_NO_MULTI(c);
  if (!c->have_frame) return Fail(c, JXLHIP_ERR_STATE, "dequant_dc before frame_begin");
  for (int ch = 0; ch < 3; ch++)
    if (!quant_dc[ch] || !dc_out[ch]) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "null plane");
  HIPCHK(c, hipSetDevice(c->device));
  const DevFrame& f = c->f;
  static const float kDefaultDcQuant[3] = {1.0f / 4096.0f, 1.0f / 512.0f, 1.0f / 256.0f};
  const float* dq = dc_quant ? dc_quant : kDefaultDcQuant;
  float mul_dc[3];
  for (int ch = 0; ch < 3; ch++)
    mul_dc[ch] = (f.inv_global_scale / (float)c->p.quant_dc) * dq[ch];  // quantizer.h:133-139
  const size_t n = (size_t)f.xsb * f.ysb;
  int rc;
  if ((rc = c->dc_tmp.Reserve(c, 3 * n))) return rc;
  float* tmp[3] = {c->dc_tmp, c->dc_tmp + n, c->dc_tmp + 2 * n};
  const uint8_t* prec_dev = nullptr;
  if (extra_precision) {
    // at most a few dozen bytes (one per 2048x2048-pixel DC group): staged behind the DC scratch
    const size_t ndc = (size_t)((f.xsb + 255) / 256) * ((f.ysb + 255) / 256);
    bool any = false;
    for (size_t i = 0; i < ndc; i++) {
      if (extra_precision[i] > 3) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "extra_precision > 3");
      any |= extra_precision[i] != 0;
    }
    if (any) {
      if ((rc = c->dc_prec.Reserve(c, ndc))) return rc;
      HIPCHK(c, hipMemcpyAsync(c->dc_prec, extra_precision, ndc, hipMemcpyHostToDevice, c->stream));
      // the source may be a short-lived host array: the copy is pageable, hence already staged by
      // the runtime when hipMemcpyAsync returns
      prec_dev = c->dc_prec;
    }
  }
  LaunchDequantDC(f.xsb, f.ysb, quant_dc, dc_out, tmp, mul_dc, cfl_x_dc, cfl_b_dc, smooth, prec_dev,
                  c->stream);
  HIPCHK(c, hipGetLastError());
  return JXLHIP_OK;
}

