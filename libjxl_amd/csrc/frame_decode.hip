// frame_decode.hip -- ONE VarDCT frame of a file (DecodeFrameAt, frame_decode.h): the host front-end pieces (entropy.cc,
// modular.inc) and the device back-end glued into the order of operations of FrameDecoder (lib/jxl/dec_frame.cc:268-416,
// 573-760), as a list of stages over one per-frame state (FrameDecode); the jobs the stages put on the caller's runner.
#include "frame_decode.h"

#include "codestream_plan.h"
#include "modular_image.h"

namespace jxlhip {
namespace {

// the first error of a job's tasks wins
void KeepFirst(std::atomic<int>& status, int rc) {
  int expected = JXLHIP_OK;
  if (rc != JXLHIP_OK) status.compare_exchange_strong(expected, rc);
}
int NoInit(void*, size_t) { return 0; }

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
    KeepFirst(j->status, rc);
    if (rc != JXLHIP_OK) return;
  }
}

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
  KeepFirst(j->status, jxlhip_ac_group_decode_submit_passes(j->c, k, pp, j->shifts, g, j->acs, j->raw_quant, j->quant_dc, data, sizes, pos));
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
  KeepFirst(j->status, jxlhip_modular_extra_channel_rows_f32(j->tree, e, j->ec_bits[e], j->image_bits, y0,
                                                             std::min(j->ysize, y0 + 64), j->planes[e], j->strides[e]));
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
  KeepFirst(j->status, rc == JXLHIP_OK ? ready.rc : rc);
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
      if (st != JXLHIP_OK) {
        {
          std::lock_guard<std::mutex> lock(j->mu);
          (st == JXLHIP_ERR_RANGE ? j->ac_range : j->stop).store(true);
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

// ---- the back-end's frame parameters (what PassesDecoderState::Init / InitForAC derive); used_acs follows the DC groups
jxlhip_frame_params MakeFrameParams(const ParsedHeaders& h, const jxlhip_frame_header& fh, const jxlhip_dc_global& dcg,
                                    const FrameCall& fc) {
  const jxlhip_image_header& ih = h.ih;
  jxlhip_frame_params p{};
  p.xsize = fh.xsize;
  p.ysize = fh.ysize;
  p.output_kind = fc.output_kind;
  p.undo_orientation = fc.undo_orientation ? ih.orientation : 0;
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
  const float scale = 255.0f / ih.intensity_target;  // OpsinParams::Init, opsin_params.cc:35-45
  for (int i = 0; i < 9; i++) p.inverse_opsin_matrix[i] = h.inv_matrix[i] * scale;
  if (fc.out_format) p.out_format = *fc.out_format;
  return p;
}

// What one frame's decode holds from its TOC to its kernels; the stages below run in the order DecodeFrameAt lists them.
struct FrameDecode {
  jxlhip_ctx* const c;
  const uint8_t* const cs;
  const size_t n;
  const ParsedHeaders& h;
  const jxlhip_image_header& ih;
  const jxlhip_frame_header& fh;
  const FrameCall& fc;
  PhaseClock& clock;
  const bool verbose;

  uint32_t ng = 0, ndc = 0, np = 0;
  size_t nb = 0, nt = 0;  // 8x8 blocks; 64x64 colour-correlation tiles
  // the section table: logical section i is sz[i] bytes at sec(i); asec / asz: the AC-group sections, [pass * ng + group]
  std::vector<uint64_t> off;
  std::vector<uint32_t> sz;
  uint64_t total = 0;
  size_t base = 0;
  bool single = false;
  size_t spos = 0;  // bit position inside section 0 (the only section of a single-section frame)
  std::vector<const uint8_t*> asec;
  std::vector<size_t> asz;
  std::vector<uint32_t> shifts;
  const uint8_t* sec(uint32_t i) const { return cs + base + off[i]; }

  // DC global and what leads it
  jxlhip_dc_global dcg;
  std::unique_ptr<jxlhip_patches, void (*)(jxlhip_patches*)> patches{nullptr, jxlhip_patches_destroy};
  std::unique_ptr<jxlhip_splines, void (*)(jxlhip_splines*)> splines{nullptr, jxlhip_splines_destroy};
  std::unique_ptr<jxlhip_modular_tree, void (*)(jxlhip_modular_tree*)> tree{nullptr, jxlhip_modular_tree_destroy};
  float noise_lut[8] = {0};
  jxlhip_frame_params p{};

  // where the extra channels go (PlanExtraChannels)
  bool blend_ec = false, want_alpha = false, want_planes = false, want_modular = false;
  float* user_plane[4] = {nullptr, nullptr, nullptr, nullptr};  // the caller's host planes (jxlhip_decode_codestream_extra), or blend_planes
  std::vector<float> blend_planes;
  size_t plane_stride = 0;
  std::vector<size_t> end_bits;  // per AC-group section: the bit behind its coefficients, where its Modular part begins

  // the host side info the DC groups fill; AC global
  std::vector<int32_t> qdc, raw_quant;
  std::vector<uint8_t> acs, sharp, prec, qctx;
  std::vector<int8_t> ytox, ytob;
  uint32_t used_acs = 0;
  jxlhip_quant_encoding enc[JXLHIP_NUM_QUANT_TABLES];
  uint32_t num_hist = 0;
  PassHandles passes;
  bool ac_global_done = false;
  int ac_i16_status = JXLHIP_ERR_STATE;  // != STATE: the AC groups went through the pipelined call as 16-bit coefficients, with this result
  double ac_tail_ms = 0;                 // how long the pipelined call went on after its last DC-phase unit

  // The n tasks of a job on the caller's runner; one after the other without one, or when the caller says `serial`
  int RunJob(void* job, int (*init)(void*, size_t), void (*func)(void*, uint32_t, size_t), uint32_t tasks, bool serial = false) {
    if (fc.runner && !serial)
      return fc.runner(fc.runner_opaque, job, init, func, 0, tasks) != 0 ? Fail(c, JXLHIP_ERR_STATE, "parallel runner failed") : JXLHIP_OK;
    for (uint32_t t = 0; t < tasks; t++) func(job, t, 0);
    return JXLHIP_OK;
  }

  int ReadToc(size_t frame_bit_pos);
  int ReadDcGlobal();
  int PlanExtraChannels();
  int RunDcPhase();
  int RunDcWithAcGlobal(PipelineJob* pj);
  int RunPipelined(PipelineJob* pj);
  int ReadAcGlobal();
  int UploadSideInfo(uint32_t ct, bool ac_in_pipeline);
  int DecodeAcGroups();
  int DecodeExtraChannels();
  int SetRenderStages();
};

// ---- table of contents
int FrameDecode::ReadToc(size_t frame_bit_pos) {
  if (fh.num_groups > (1u << 22) || fh.num_passes == 0 || fh.num_passes > 11)
    return Fail(c, JXLHIP_ERR_UNSUPPORTED, "frame too large");
  // a few header bytes can claim 2^38 pixels: bound what is allocated before looking at the sections
  // (JXLHIP_MAX_PIXELS, default 2^30 = four 16K frames' worth; each 8x8 block needs ~40 bytes of host side info)
  const uint64_t max_px = jxlhip_env::Get().max_pixels.load(std::memory_order_relaxed);
  if ((uint64_t)fh.xsize_blocks * fh.ysize_blocks * 64u > max_px)
    return Fail(c, JXLHIP_ERR_UNSUPPORTED, "frame of %ux%u blocks exceeds JXLHIP_MAX_PIXELS", fh.xsize_blocks, fh.ysize_blocks);
  ng = (uint32_t)fh.num_groups, ndc = (uint32_t)fh.num_dc_groups, np = fh.num_passes;
  nb = (size_t)fh.xsize_blocks * fh.ysize_blocks;
  nt = (size_t)((fh.xsize_blocks + 7) / 8) * ((fh.ysize_blocks + 7) / 8);
  size_t pos = frame_bit_pos;
  const uint32_t ntoc = (uint32_t)fh.num_toc_entries;
  off.resize(ntoc);
  sz.resize(ntoc);
  const int rc = jxlhip_toc_decode(cs, n, &pos, ntoc, off.data(), sz.data(), &total);
  if (rc) return Fail(c, rc, "invalid TOC");
  base = pos / 8;
  if (total > n - base && !fc.partial) return Fail(c, JXLHIP_ERR_BAD_STREAM, "truncated frame: %llu section bytes, %zu present",
                                                   (unsigned long long)total, n - base);
  single = ntoc == 1;
  return JXLHIP_OK;
}

// ---- DC global: quantizer, block context map, colour correlation; the global modular tree
int FrameDecode::ReadDcGlobal() {
  int rc;
  // the patch dictionary leads the section (dec_frame.cc:272-288), the splines bundle follows (:289-293);
  // jxlhip_dc_global_decode reads on from behind them
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
  if (fh.flags & JXLHIP_FLAG_SPLINES) {
    jxlhip_splines* sp = nullptr;
    if ((rc = jxlhip_splines_decode(sec(0), sz[0], &spos, (uint64_t)fh.xsize * fh.ysize, &sp)))
      return Fail(c, rc, "invalid splines");
    splines.reset(sp);
  }
  if (fh.flags & JXLHIP_FLAG_NOISE) {
    size_t npos = spos;
    if ((rc = jxlhip_noise_lut_decode(sec(0), sz[0], &npos, noise_lut))) return Fail(c, rc, "invalid noise parameters");
  }
  if ((rc = jxlhip_dc_global_decode(sec(0), sz[0], &spos, fh.flags & ~(uint64_t)(JXLHIP_FLAG_SPLINES | JXLHIP_FLAG_PATCHES), &dcg)))
    return Fail(c, rc, "invalid DC global section");
  jxlhip_modular_tree* tree_raw = nullptr;
  if ((rc = jxlhip_modular_global_decode(sec(0), sz[0], &spos, &fh, &tree_raw)))
    return Fail(c, rc, "invalid modular global section");
  tree.reset(tree_raw);
  return JXLHIP_OK;
}

// Which extra channels are decoded and where they go; the section lists and the side-info arrays of the phases that follow
int FrameDecode::PlanExtraChannels() {
  // an alpha channel is decoded only when the output has room for it; its bytes sit behind the coefficients of
  // every AC-group section and are skipped otherwise
  // (a frame that is blended or saved hands ALL its extra channels to jxlhip_set_blending_extra instead: SetRenderStages)
  blend_ec = fc.blend && ih.num_extra_channels != 0;
  want_alpha = !blend_ec && h.alpha_index >= 0 && fc.output_kind == JXLHIP_OUT_PACKED && fc.out_format->num_channels == 4;
  for (uint32_t i = 0; i < ih.num_extra_channels && i < fc.num_extra_planes && i < 4; i++) {
    user_plane[i] = fc.extra_planes[i];
    want_planes |= user_plane[i] != nullptr;
  }
  if (want_planes && fc.extra_stride < ih.xsize) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "extra_stride below the image width");
  // the planes of a blended frame, at the FRAME's size (a cropped frame's channels are as small as its colour)
  plane_stride = fc.extra_stride;
  if (blend_ec) {
    if (want_planes) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "the caller's extra-channel planes on a blended frame");
    const size_t plane = (size_t)fh.xsize * fh.ysize;
    blend_planes.resize(ih.num_extra_channels * plane);
    for (uint32_t i = 0; i < ih.num_extra_channels; i++) user_plane[i] = blend_planes.data() + i * plane;
    plane_stride = fh.xsize;
    want_planes = true;
  }
  want_modular = want_alpha || want_planes;
  end_bits.assign(want_modular ? (size_t)np * ng : 0, 0);
  asec.resize((size_t)np * ng);
  asz.resize((size_t)np * ng);
  shifts.assign(fh.shift, fh.shift + np);
  for (size_t i = 0; !single && i < (size_t)np * ng; i++) {
    asec[i] = sec(2 + ndc + (uint32_t)i);
    asz[i] = sz[2 + ndc + i];
  }
  qdc.resize(3 * nb), raw_quant.resize(nb);
  acs.resize(nb), sharp.resize(nb), prec.resize(ndc), qctx.resize(nb);
  ytox.resize(nt), ytob.resize(nt);
  return JXLHIP_OK;
}

// ---- DC groups on the runner: quantized DC + the AC metadata (strategy map, quant field, sharpness, cmaps); with a
// runner, AC global and the AC groups (16-bit coefficients, optimistically) in the same call: PipelineJob
int FrameDecode::RunDcPhase() {
  int rc;
  PipelineJob pj;
  DcJob& job = pj.dc;
  job.tree = tree.get();
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
  std::vector<const uint8_t*> dsec(ndc);
  std::vector<size_t> dsz(ndc);
  if (single) {
    uint32_t p0 = 0;
    rc = jxlhip_dc_group_decode(tree.get(), sec(0), sz[0], &spos, &fh, 0, job.qdc, &p0, job.acs, job.raw_quant, job.sharp,
                                job.ytox, job.ytob, &used_acs);
    prec[0] = (uint8_t)p0;
    if (rc) return Fail(c, rc, "invalid DC group");
  } else {
    for (uint32_t g = 0; g < ndc; g++) {
      dsec[g] = sec(1 + g);
      dsz[g] = sz[1 + g];
    }
    job.sections = dsec.data();
    job.sizes = dsz.data();
    job.ctx_map = &dcg.block_ctx_map;
    job.qctx = qctx.data();
    // without a runner, and for a partial file, the DC groups alone: AC global may not be there, and the AC groups follow the plan
    rc = fc.runner && !fc.partial ? RunDcWithAcGlobal(&pj) : RunJob(&job, NoInit, DcFunc, ndc);
    if (rc) return rc;
    if ((rc = job.status.load())) return Fail(c, rc, "invalid DC group");
    if (ac_global_done && job.ag_status) return Fail(c, job.ag_status, "invalid AC global section");
  }
  return JXLHIP_OK;  // (the job and its threads' buffers go inside the DC phase's time: the caller marks it)
}

// The DC groups with a runner: the AC-global section rides along as one more unit (DcJob), and so do -- unless
// JXLHIP_NO_PIPELINE -- the AC groups (RunPipelined)
int FrameDecode::RunDcWithAcGlobal(PipelineJob* pj) {
  DcJob& job = pj->dc;
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
  int rc = JXLHIP_OK;
  const bool pipelined = !jxlhip_env::Get().no_pipeline.load(std::memory_order_relaxed) && (rc = jxlhip_frame_begin(c, &p)) == JXLHIP_OK && (rc = EnsureUploadBuffers(c)) == JXLHIP_OK;
  if (rc) return rc;
  if ((rc = pipelined ? RunPipelined(pj) : RunJob(&job, NoInit, DcFunc, ndc + 1))) return rc;
  ac_global_done = true;
  if (verbose) {
    fprintf(stderr, "[codestream] runner call: %.2f ms; DC-phase units (start-end ms @thread):",
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - job.t0).count());
    for (uint32_t g = 0; g <= ndc; g++) {
      fprintf(stderr, " %s%.2f-%.2f@%d", g == ndc ? "acglobal:" : "", timeline[3 * g], timeline[3 * g + 1], (int)timeline[3 * g + 2]);
    }
    fprintf(stderr, "\n");
  }
  return JXLHIP_OK;
}

// The single runner call (PipelineJob): ndc + 1 + ng tickets
int FrameDecode::RunPipelined(PipelineJob* pj) {
  pj->ndc = ndc;
  pj->ng = ng;
  pj->dc.block_info_hook = PipelineJob::BlockInfoReady;
  pj->dc.hook_opaque = pj;
  GroupsJob& gj = pj->ac;
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
    gj.t0 = pj->dc.t0;
  }
  uint32_t stray = 0;
  if (!PlanTickets(ndc, ng, np, pj->dc.sizes, asz.data(), fh.xsize, fh.xsize_blocks, fh.group_dim, &pj->dc_order, &pj->ac_of_dc, &stray))
    return Fail(c, JXLHIP_ERR_STATE, "AC group %u under no DC group", stray);
  pj->ready.resize(ng);
  pj->t_call = std::chrono::steady_clock::now();
  const int rc = RunJob(pj, PipelineInit, PipelineFunc, ndc + 1 + ng);
  if (rc) return rc;
  // (the phase report: what of the call followed the last DC group is the AC groups' own time)
  ac_tail_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - pj->t_call).count() - pj->dc_end_us.load() * 1e-3;
  for (SparseBatch& sb : gj.batch) KeepFirst(gj.status, SparseFlush(c, &sb));  // what the threads still hold
  ac_i16_status = gj.status.load();
  if (verbose) GroupsTimelineReport(gj);
  return JXLHIP_OK;
}

// ---- AC global: dequant encodings, histograms and coefficient orders of every pass (unless it rode along in the DC phase)
int FrameDecode::ReadAcGlobal() {
  int rc = JXLHIP_OK;
  if (single) {  // (the block contexts a DC group's thread makes otherwise: DcJob)
    const int32_t* qdc3[3] = {qdc.data(), qdc.data() + nb, qdc.data() + 2 * nb};
    if ((rc = jxlhip_quant_dc_contexts(&dcg.block_ctx_map, nb, qdc3, qctx.data()))) return rc;
    rc = jxlhip_ac_global_decode_at(sec(0), sz[0], &spos, ng, np, used_acs, &dcg.block_ctx_map, enc, &num_hist, passes.p);
  } else if (!ac_global_done && (!fc.partial || fc.partial->info.have_ac_global)) {
    size_t bits = 0;
    rc = jxlhip_ac_global_decode(sec(1 + ndc), sz[1 + ndc], ng, np, used_acs, &dcg.block_ctx_map, enc, &num_hist, passes.p, &bits);
  }
  if (rc) return Fail(c, rc, "invalid AC global section");
  clock.Mark(JXLHIP_PHASE_AC_GLOBAL);
  p.used_acs = used_acs;
  return JXLHIP_OK;
}

// The frame on the back-end with coefficient type ct, and the side info of the DC phase on the stream
int FrameDecode::UploadSideInfo(uint32_t ct, bool ac_in_pipeline) {
  int rc;
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
  return JXLHIP_OK;
}

// AC groups on the runner: entropy decode into pinned staging slots + uploads
int FrameDecode::DecodeAcGroups() {
  const jxlhip_ac_pass* pp[11];
  for (uint32_t i = 0; i < np; i++) pp[i] = passes.p[i];
  if (fc.partial) {  // every group the passes it has
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
    const int rc = RunJob(&pg, NoInit, PartialGroupsFunc, ng);
    return rc ? rc : pg.status.load();
  }
  if (single) {
    // one section: the AC group follows AC global at the current bit position (one pass)
    const uint8_t* d1[11] = {sec(0)};
    size_t s1[11] = {sz[0]}, b1[11] = {spos};
    const int rc = jxlhip_ac_group_decode_submit_passes(c, 1, pp, shifts.data(), 0, acs.data(), raw_quant.data(), qctx.data(), d1, s1, b1);
    if (want_modular) end_bits[0] = b1[0];
    return rc;
  }
  return jxlhip_ac_groups_decode_submit_ex(c, fc.runner, fc.runner_opaque, np, pp, shifts.data(), acs.data(), raw_quant.data(),
                                           qctx.data(), asec.data(), asz.data(), want_modular ? end_bits.data() : nullptr);
}

// The Modular extra channels (the coefficient uploads of the last groups are still in flight).
// The alpha channel of an RGBA output goes into the context's pinned plane (uploaded by jxlhip_set_alpha), the
// channels the caller asked for into its planes: by the groups' threads when the channels are larger than a group
// and final group by group, from the handle's image otherwise
int FrameDecode::DecodeExtraChannels() {
  int rc;
  float* alpha = nullptr;
  size_t astride = 0;
  if (want_alpha && (rc = jxlhip_alpha_staging(c, &alpha, &astride))) return rc;
  ModularGroupsJob job;
  job.collect = !jxlhip_modular_groups_are_final(tree.get());
  const bool in_groups = !job.collect && (fh.xsize > fh.group_dim || fh.ysize > fh.group_dim);
  for (uint32_t i = 0; i < 4; i++) {
    job.ec_bits[i] = i < ih.num_extra_channels ? h.extra[i].bit_depth.bits_per_sample : 8;
    const bool is_alpha = want_alpha && (int)i == h.alpha_index;
    job.planes[i] = is_alpha ? alpha : user_plane[i];
    job.strides[i] = is_alpha ? astride : plane_stride;
  }
  job.image_bits = ih.bit_depth.bits_per_sample;
  job.tree = tree.get();
  job.fh = &fh;
  job.num_groups = ng;
  job.num_passes = single ? 1 : np;
  const uint8_t* s0 = sec(0);
  const size_t z0 = sz[0];
  job.sections = single ? &s0 : asec.data();
  job.sizes = single ? &z0 : asz.data();
  job.start_bits = end_bits.data();
  if ((rc = RunJob(&job, NoInit, ModularGroupsFunc, ng, single))) return rc;
  if ((rc = job.status.load()))
    return Fail(c, rc, rc == JXLHIP_ERR_UNSUPPORTED ? "extra channels coded with Modular features outside this front-end"
                                                     : "invalid Modular data in an AC group");
  if (!in_groups) {
    // the global image's transforms (a squeeze pyramid: every level spread over the runner), then the samples as
    // floats, 64 rows per task
    if ((rc = jxlhip_modular_finalize(tree.get(), fc.runner, fc.runner_opaque))) return Fail(c, rc, "extra channels: undoing the transforms");
    ExtraRowsJob rows;
    rows.tree = tree.get();
    rows.image_bits = job.image_bits;
    rows.ysize = fh.ysize;  // (the image's, except for a cropped frame of a sequence)
    rows.tasks_per_channel = (fh.ysize + 63) / 64;
    for (uint32_t i = 0; i < 4; i++) {
      rows.ec_bits[i] = job.ec_bits[i];
      rows.planes[i] = i < ih.num_extra_channels ? job.planes[i] : nullptr;
      rows.strides[i] = job.strides[i];
    }
    if ((rc = RunJob(&rows, NoInit, ExtraRowsFunc, 4 * rows.tasks_per_channel))) return rc;
    if ((rc = rows.status.load())) return Fail(c, rc, "extra channel");
  }
  if (want_alpha) {
    if (user_plane[h.alpha_index])  // the caller wants the alpha plane as well
      for (uint32_t y = 0; y < ih.ysize; y++)
        memcpy(user_plane[h.alpha_index] + (size_t)y * fc.extra_stride, alpha + (size_t)y * astride, (size_t)ih.xsize * sizeof(float));
    if ((rc = jxlhip_set_alpha(c, alpha, astride))) return rc;
  }
  return JXLHIP_OK;
}

// The render stages of the frame, in the order the back-end runs them
int FrameDecode::SetRenderStages() {
  int rc;
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
  return JXLHIP_OK;
}

}  // namespace

int DecodeFrameAt(jxlhip_ctx* c, const uint8_t* cs, size_t n, const ParsedHeaders& h, const jxlhip_frame_header& fh,
                  size_t frame_bit_pos, const FrameCall& fc, PhaseClock& clock, bool verbose, jxlhip_codestream_info* info_p,
                  size_t* end_bit_pos) {
  jxlhip_codestream_info& info = *info_p;
  FrameDecode d{c, cs, n, h, h.ih, fh, fc, clock, verbose};
  int rc;
  if ((rc = d.ReadToc(frame_bit_pos))) return rc;
  if ((rc = d.ReadDcGlobal())) return rc;
  clock.Mark(JXLHIP_PHASE_HEADERS);
  d.p = MakeFrameParams(h, fh, d.dcg, fc);
  if ((rc = d.PlanExtraChannels())) return rc;
  if ((rc = d.RunDcPhase())) return rc;
  clock.Mark(JXLHIP_PHASE_DC_GROUPS);
  if (d.ac_tail_ms > 0) {  // what of the pipelined call followed its last DC-phase unit is the AC groups' own time
    c->cs_phase_ms[JXLHIP_PHASE_DC_GROUPS] -= d.ac_tail_ms;
    c->cs_phase_ms[JXLHIP_PHASE_AC_GROUPS] += d.ac_tail_ms;
  }
  if ((rc = d.ReadAcGlobal())) return rc;
  // ---- coefficient type: 16-bit buffers optimistically (jxl_hip_entropy.h), int32 when a value does not fit
  for (uint32_t ct = JXLHIP_COEFF_I16; ct <= JXLHIP_COEFF_I32; ct++) {
    // (the 16-bit attempt of the pipelined call: decoded and submitted inside it)
    const bool ac_in_pipeline = ct == JXLHIP_COEFF_I16 && d.ac_i16_status != JXLHIP_ERR_STATE;
    if (ac_in_pipeline && d.ac_i16_status == JXLHIP_ERR_RANGE) continue;  // redo with int32 buffers
    if (ac_in_pipeline && d.ac_i16_status != JXLHIP_OK) return d.ac_i16_status;
    if ((rc = d.UploadSideInfo(ct, ac_in_pipeline))) return rc;
    rc = ac_in_pipeline ? JXLHIP_OK : d.DecodeAcGroups();
    clock.Mark(JXLHIP_PHASE_AC_GROUPS);
    if (rc == JXLHIP_ERR_RANGE && ct == JXLHIP_COEFF_I16) continue;  // redo with int32 buffers
    if (rc) return rc;
    info.coeff_type = ct;
    break;
  }
  if (d.want_modular && (rc = d.DecodeExtraChannels())) return rc;
  clock.Mark(JXLHIP_PHASE_EXTRA_CHANNELS);
  if ((rc = d.SetRenderStages())) return rc;
  if ((rc = jxlhip_decode_frame(c, fc.out, fc.out_stride, fc.out_plane_stride))) return rc;
  if ((rc = jxlhip_sync(c))) return rc;
  clock.Mark(JXLHIP_PHASE_KERNELS);
  info.num_passes = d.np;
  info.num_groups = d.ng;
  info.num_dc_groups = d.ndc;
  info.epf_iters = fh.lf.epf_iters;
  info.gab = fh.lf.gab;
  info.used_acs = d.used_acs;
  if (end_bit_pos) *end_bit_pos = (d.base + (size_t)d.total) * 8;
  return JXLHIP_OK;
}


// ---- the one frame of a lossless file: a regular Modular frame.  No VarDCT part: DC global is the DC dequant bit and
// the global Modular image, a DC group is its ModularDC stream, AC global is empty, an AC group is its ModularAC stream.
// The entropy decode stays on the host (an MA-tree context per sample, an ANS state per stream: serial inside a group,
// parallel over the groups on the runner); what it leaves -- three integer planes and the RCTs still to undo -- goes to
// the device for one streaming kernel.
namespace {

struct ModularGroupsJob2 {
  ModularImage* image;
  const FrameDecode* d;
  std::atomic<int> status{JXLHIP_OK};
};
void ModularImageGroupsFunc(void* opaque, uint32_t t, size_t) {
  ModularGroupsJob2* j = static_cast<ModularGroupsJob2*>(opaque);
  if (j->status.load(std::memory_order_relaxed) != JXLHIP_OK) return;
  const FrameDecode& d = *j->d;
  size_t pos = 0;
  // (section 1 + ndc is AC global)
  const int rc = t < d.ndc ? ModularImageDcGroup(j->image, t, d.sec(1 + t), d.sz[1 + t], &pos)
                           : ModularImageAcGroup(j->image, t - d.ndc, d.sec(2 + t), d.sz[2 + t], &pos);
  KeepFirst(j->status, rc);
}

// the output's transfer function a lossless file has to be asked for in: the original's (JXLHIP_TF_*)
uint32_t OriginalTransfer(const jxlhip_color_encoding& ce) {
  if (ce.all_default) return JXLHIP_TF_SRGB;
  if (ce.have_gamma) return JXLHIP_TF_GAMMA;
  switch (ce.transfer_function) {
    case 1: return JXLHIP_TF_709;
    case 8: return JXLHIP_TF_LINEAR;
    case 13: return JXLHIP_TF_SRGB;
    case 16: return JXLHIP_TF_PQ;
    case 17: return JXLHIP_TF_GAMMA;
    case 18: return JXLHIP_TF_HLG;
    default: return ~0u;
  }
}

}  // namespace

int DecodeModularFrameAt(jxlhip_ctx* c, const uint8_t* cs, size_t n, const ParsedHeaders& h, const FrameCall& fc, PhaseClock& clock,
                         jxlhip_codestream_info* info) {
  const jxlhip_image_header& ih = h.ih;
  const jxlhip_frame_header& fh = h.fh;
  if (fc.output_kind == JXLHIP_OUT_XYB_PLANAR) return Fail(c, JXLHIP_ERR_UNSUPPORTED, "planar XYB of a lossless (Modular) file, which is not XYB");
  // the pixels are the original's samples: nothing on this path converts between transfer functions (JxlDecoder without a
  // CMS cannot either)
  const uint32_t original = OriginalTransfer(ih.color_encoding);
  const uint32_t asked = fc.output_kind == JXLHIP_OUT_PACKED ? fc.out_format->transfer : (uint32_t)JXLHIP_TF_LINEAR;
  if (asked != original)
    return Fail(c, JXLHIP_ERR_UNSUPPORTED, "a lossless (Modular) file comes out in its original's transfer function only (JXLHIP_TF_* %u asked, %u coded)",
                asked, original);
  // the channels: three colour planes, or the one of a grey image; behind them the image's extra channels.  The first
  // alpha channel goes to the device when the output has a fourth channel for it; the others are decoded, as they must
  // be, into ordinary memory and handed to the caller as float planes where asked for (jxlhip_decode_codestream_extra)
  const jxlhip_color_encoding& ce = ih.color_encoding;
  const uint32_t num_color = !ce.all_default && ce.color_space == JXLHIP_CS_GRAY ? 1 : 3, nec = ih.num_extra_channels;
  const bool want_alpha = h.alpha_index >= 0 && fc.output_kind == JXLHIP_OUT_PACKED && fc.out_format->num_channels == 4;
  float* user_plane[4] = {nullptr, nullptr, nullptr, nullptr};
  bool want_planes = false;
  for (uint32_t i = 0; i < nec && i < fc.num_extra_planes && i < 4; i++) {
    user_plane[i] = fc.extra_planes[i];
    want_planes = want_planes || user_plane[i];
  }
  if (want_planes && fc.extra_stride < ih.xsize) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "extra_stride below the image width");
  FrameDecode d{c, cs, n, h, ih, fh, fc, clock, false};
  int rc;
  if ((rc = d.ReadToc(h.frame_bit_pos))) return rc;
  if (!d.single && d.off.size() != 2 + (size_t)d.ndc + d.ng) return Fail(c, JXLHIP_ERR_BAD_STREAM, "section count of a Modular frame");
  // pinned planes (rows of a multiple of 64 samples) and programs: int16 when the image header says 16-bit buffers do
  const uint32_t stride = (fh.xsize + 63u) & ~63u;
  HIPCHK(c, hipSetDevice(c->device));
  for (uint32_t type = ih.modular_16_bit_buffer_sufficient ? JXLHIP_MODULAR_I16 : JXLHIP_MODULAR_I32; type <= JXLHIP_MODULAR_I32; type++) {
    const size_t ssz = type == JXLHIP_MODULAR_I16 ? 2 : 4;
    const size_t plane = ((size_t)stride * fh.ysize * ssz + 255) & ~(size_t)255;
    const uint32_t dev_planes = num_color + (want_alpha ? 1u : 0u);
    const size_t need = dev_planes * plane + (size_t)d.ng * sizeof(uint16_t);
    if (need > c->modular_host.bytes) {
      if ((rc = jxlhip_sync(c))) return rc;  // (nothing may still be reading the old planes)
      if (c->modular_host.Alloc(&c->mm, need)) return Fail(c, JXLHIP_ERR_OUT_OF_MEMORY, "pinned Modular planes of %zu bytes", need);
    }
    uint8_t* base = static_cast<uint8_t*>(c->modular_host.p);
    jxlhip_modular_image_channels pl{};
    pl.num_color = num_color;
    pl.num_extra = nec;
    for (uint32_t ch = 0; ch < num_color; ch++) pl.planes[ch] = base + ch * plane;
    std::vector<uint8_t> others;  // the extra channels that do not go to the device
    others.resize((size_t)(nec - (want_alpha ? 1u : 0u)) * plane);
    for (uint32_t e = 0, k = 0; e < nec; e++) {
      pl.extra_planes[e] = want_alpha && (int)e == h.alpha_index ? base + num_color * plane : others.data() + (k++) * plane;
      pl.extra_bits[e] = h.extra[e].bit_depth.bits_per_sample;
    }
    pl.stride_samples = stride;
    pl.sample_type = type;
    pl.group_rct = reinterpret_cast<uint16_t*>(base + dev_planes * plane);
    // ---- DC global: the DC dequant bit, the global tree, the global Modular image
    const char* why = "";
    ModularImage* raw = nullptr;
    d.spos = 0;
    if ((rc = ModularImageBegin(d.sec(0), d.sz[0], &d.spos, &fh, &pl, &raw, &why)))
      return Fail(c, rc, "%s", rc == JXLHIP_ERR_UNSUPPORTED && why[0] ? why : "invalid DC global section of a Modular frame");
    std::unique_ptr<ModularImage, void (*)(ModularImage*)> image(raw, ModularImageDestroy);
    clock.Mark(JXLHIP_PHASE_HEADERS);
    // ---- ModularDC per DC group, ModularAC per group: on the runner
    if (d.single) {
      if ((rc = ModularImageDcGroup(raw, 0, d.sec(0), d.sz[0], &d.spos)) || (rc = ModularImageAcGroup(raw, 0, d.sec(0), d.sz[0], &d.spos)))
        return Fail(c, rc, "invalid Modular group");
    } else {
      ModularGroupsJob2 job{raw, &d};
      if ((rc = d.RunJob(&job, NoInit, ModularImageGroupsFunc, d.ndc + d.ng))) return rc;
      if ((rc = job.status.load()))
        return Fail(c, rc, rc == JXLHIP_ERR_UNSUPPORTED ? "a Modular group with a delta palette or a squeeze" : "invalid Modular group");
    }
    rc = ModularImageFinish(raw);
    clock.Mark(JXLHIP_PHASE_AC_GROUPS);
    if (rc == JXLHIP_ERR_RANGE && type == JXLHIP_MODULAR_I16) continue;  // (the header's promise did not hold: int32 planes)
    if (rc) return Fail(c, rc, "invalid Modular frame");
    // ---- the caller's extra-channel planes: v * (float)(1.0 / (2^bits - 1)) with the channel's own depth, what
    // jxlhip_modular_extra_channel_f32 gives a VarDCT file's channels (dec_modular.cc:726-731)
    for (uint32_t e = 0; e < nec && e < 4; e++) {
      if (!user_plane[e]) continue;
      const float factor = (float)(1.0 / (double)((1u << pl.extra_bits[e]) - 1u));
      for (uint32_t y = 0; y < fh.ysize; y++) {
        float* to = user_plane[e] + (size_t)y * fc.extra_stride;
        if (type == JXLHIP_MODULAR_I16) {
          const int16_t* from = static_cast<const int16_t*>(pl.extra_planes[e]) + (size_t)y * stride;
          for (uint32_t x = 0; x < fh.xsize; x++) to[x] = (float)from[x] * factor;
        } else {
          const int32_t* from = static_cast<const int32_t*>(pl.extra_planes[e]) + (size_t)y * stride;
          for (uint32_t x = 0; x < fh.xsize; x++) to[x] = (float)from[x] * factor;
        }
      }
    }
    // ---- upload, k_modular_emit or k_modular_planes, sync
    jxlhip_modular_channels m{};
    m.xsize = fh.xsize;
    m.ysize = fh.ysize;
    m.num_color = num_color;
    for (uint32_t ch = 0; ch < num_color; ch++) m.planes[ch] = pl.planes[ch];
    if (want_alpha) {
      m.alpha_plane = pl.extra_planes[h.alpha_index];
      m.alpha_bits = pl.extra_bits[h.alpha_index];
    }
    m.stride_samples = stride;
    m.sample_type = type;
    m.bits_per_sample = ih.bit_depth.bits_per_sample;
    m.group_dim = fh.group_dim;
    m.group_rct = pl.group_rct;
    m.global_rct = pl.global_rct;
    if ((rc = jxlhip_decode_modular_channels(c, &m, fc.output_kind, fc.out_format, fc.out, fc.out_stride, fc.undo_orientation ? ih.orientation : 0)))
      return rc;
    if ((rc = jxlhip_sync(c))) return rc;
    clock.Mark(JXLHIP_PHASE_KERNELS);
    break;
  }
  info->num_passes = d.np;
  info->num_groups = d.ng;
  info->num_dc_groups = d.ndc;
  return JXLHIP_OK;
}

}  // namespace jxlhip
