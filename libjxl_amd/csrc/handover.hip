// handover.hip -- how a frame's inputs reach the device (include/jxl_hip.h, jxl_hip_entropy.h): the upload buffers and
// the side info, jxlhip_submit_group, the pinned staging slots, the sparse arena, and the AC groups on the caller's
// runner (jxlhip_ac_groups_decode_submit).  Host code only.
#include <functional>

#include "context.h"

// A new hand-over of a frame's data begins (jxlhip_frame_begin, and jxlhip_upload_side_info: the same frame may be
// handed over again without a new frame_begin).  Frames may follow each other without a jxlhip_sync: the group
// uploads travel on the pool streams into buffers the previous decode's kernels (main stream) may still be reading,
// so the pool streams wait for everything queued on the main stream; the sparse arena and its offset table start empty.
int jxlhip::BeginHandover(jxlhip_ctx* c) {
  const DevFrame& f = c->f;
  c->frame_serial++;
  c->sp_any.store(false);
  c->sp_arena_used.store(0);
  if (c->sparse_upload && f.coeff_type == JXLHIP_COEFF_I16) {
    const size_t ng = (size_t)f.xsg * f.ysg;
    const int par = (int)(c->frame_serial & 1u);
    if (SparseTableItems(c) < ng) {
      for (int i = 0; i < 2; i++) {
        if (c->sp_off_pending[i]) (void)hipEventSynchronize(c->sp_off_ev[i]);
        c->sp_off_pending[i] = false;
        if (c->sp_off_host[i].Alloc(&c->mm, ng * 4)) return Fail(c, JXLHIP_ERR_OUT_OF_MEMORY, "sparse offset table");
        HIPCHK(c, c->sp_off_ev[i].Create());
      }
    }
    // the table of two hand-overs ago has long been copied; make sure before it is overwritten
    if (c->sp_off_pending[par]) HIPCHK(c, hipEventSynchronize(c->sp_off_ev[par]));
    c->sp_off_pending[par] = false;
    memset(c->sp_off_host[par].p, 0xFF, ng * 4);
  }
  if (c->up_coeffs[0]) {
    HIPCHK(c, hipEventRecord(c->frame_ev, c->stream));
    for (int i = 0; i < kPoolStreams; i++) HIPCHK(c, hipStreamWaitEvent(c->pool[i], c->frame_ev, 0));
  }
  return JXLHIP_OK;
}

// lays the side-info slab out; returns total bytes
static size_t SideLayout(const DevFrame& f, size_t off[9]) {
  const size_t nb = (size_t)f.xsb * f.ysb;
  const size_t nt = (size_t)f.xtiles * ((f.ysb + 7) / 8);
  size_t pos = 0;
  auto take = [&](size_t bytes) {
    const size_t o = pos;
    pos += (bytes + 255) & ~(size_t)255;
    return o;
  };
  off[0] = take(nb);                   // acs
  off[1] = take(nb * 4);               // raw_quant
  off[2] = take(nb);                   // sharpness
  off[3] = take(nt);                   // ytox
  off[4] = take(nt);                   // ytob
  off[5] = take(nb * 4);               // dc x
  off[6] = take(nb * 4);               // dc y
  off[7] = take(nb * 4);               // dc b
  off[8] = take(sizeof(float) * JXLHIP_DEQUANT_TABLE_FLOATS);
  return pos;
}

int jxlhip::EnsureUploadBuffers(jxlhip_ctx* c) {
  const DevFrame& f = c->f;
  const size_t esz = f.coeff_type == JXLHIP_COEFF_I16 ? 2 : 4;
  // one buffer, [group][channel][65536]: a group's three channels are contiguous, so the
  // staging slot of jxlhip_ac_group_decode_submit goes up with ONE copy (three copies per group
  // = ~400 hipMemcpyAsync calls per 4K frame were a 4.5 ms serial floor: the runtime serialises
  // them whatever thread they come from)
  const size_t cbytes = (size_t)f.xsg * f.ysg * 3 * JXLHIP_GROUP_COEFFS * esz;
  int rc;
  if ((rc = c->up_coeff_slab.Reserve(c, cbytes))) {
    c->up_coeffs[0] = c->up_coeffs[1] = c->up_coeffs[2] = nullptr;
    return rc;
  }
  c->up_coeffs[0] = c->up_coeff_slab;
  if (c->sparse_upload && esz == 2) {  // the landing zone of the sparse hand-off (see SubmitSparse)
    // (never cleared: k_expand_sparse reads only what the offset table points at, and those bytes were uploaded.
    // A hipMemset here runs on the NULL stream, unordered against the uploads on the non-blocking pool streams: it
    // once landed AFTER the first batch and turned a frame into its DC image.)
    if ((rc = c->sp_dev.Reserve(c, (size_t)f.xsg * f.ysg * 3 * JXLHIP_GROUP_COEFFS * 2))) return rc;
  }
  c->up_groups = f.xsg * f.ysg;
  c->up_esz = esz;
  c->up_coeffs[1] = (char*)c->up_coeffs[0] + (size_t)JXLHIP_GROUP_COEFFS * esz;
  c->up_coeffs[2] = (char*)c->up_coeffs[0] + 2 * (size_t)JXLHIP_GROUP_COEFFS * esz;
  size_t off[9];
  const size_t sbytes = SideLayout(f, off);
  if ((rc = c->up_side.Reserve(c, sbytes))) return rc;
  jxlhip_frame_inputs in{};
  for (int ch = 0; ch < 3; ch++) {
    in.coeffs[ch] = c->up_coeffs[ch];
    in.dc[ch] = (const float*)(c->up_side + off[5 + ch]);
  }
  in.ac_strategy = c->up_side + off[0];
  in.raw_quant = (const int32_t*)(c->up_side + off[1]);
  in.epf_sharpness = c->up_side + off[2];
  in.ytox_map = (const int8_t*)(c->up_side + off[3]);
  in.ytob_map = (const int8_t*)(c->up_side + off[4]);
  in.dequant_table = (const float*)(c->up_side + off[8]);
  c->up_inputs = in;
  return JXLHIP_OK;
}

int jxlhip_upload_side_info(jxlhip_ctx* c, const uint8_t* ac_strategy, const int32_t* raw_quant,
                            const uint8_t* epf_sharpness, const int8_t* ytox_map,
                            const int8_t* ytob_map, const float* const dc[3],
                            const float* dequant_table) {
  if (!c) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (c->multi) {
    for (MultiChild& k : c->multi->kids) {
      const int rc = jxlhip_upload_side_info(k.ctx, ac_strategy, raw_quant, epf_sharpness, ytox_map, ytob_map, dc, dequant_table);
      if (rc) return MultiCheck(c, k.ctx, rc);
    }
    return JXLHIP_OK;
  }
  if (!c->have_frame) return Fail(c, JXLHIP_ERR_STATE, "upload_side_info before frame_begin");
  if (!ac_strategy || !raw_quant || !ytox_map || !ytob_map || !dc || !dc[0] || !dc[1] ||
      !dc[2] || !dequant_table || (c->p.lf.epf_iters > 0 && !epf_sharpness))
    return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "null side-info pointer");
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = EnsureUploadBuffers(c))) return rc;
  // frame_begin has just started this frame's hand-over (serial, sparse table parity, arena): starting another one
  // here would advance the serial twice per frame -- the double-buffered offset table would then sit on ONE parity
  // and wait for the previous frame's copy every time -- and would drop groups submitted before the side info.  Only
  // a frame handed over AGAIN (a second upload_side_info without a frame_begin) starts over.
  if (c->handover_fresh) c->handover_fresh = false;
  else if ((rc = BeginHandover(c))) return rc;
  const DevFrame& f = c->f;
  const size_t nb = (size_t)f.xsb * f.ysb;
  const size_t nt = (size_t)f.xtiles * ((f.ysb + 7) / 8);
  const jxlhip_frame_inputs& in = c->up_inputs;
  hipStream_t st = c->stream;
  HIPCHK(c, hipMemcpyAsync((void*)in.ac_strategy, ac_strategy, nb, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync((void*)in.raw_quant, raw_quant, nb * 4, hipMemcpyHostToDevice, st));
  if (epf_sharpness)
    HIPCHK(c, hipMemcpyAsync((void*)in.epf_sharpness, epf_sharpness, nb, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync((void*)in.ytox_map, ytox_map, nt, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync((void*)in.ytob_map, ytob_map, nt, hipMemcpyHostToDevice, st));
  for (int ch = 0; ch < 3; ch++)
    HIPCHK(c, hipMemcpyAsync((void*)in.dc[ch], dc[ch], nb * 4, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync((void*)in.dequant_table, dequant_table,
                           sizeof(float) * JXLHIP_DEQUANT_TABLE_FLOATS, hipMemcpyHostToDevice, st));
  ApplyInputs(c, &in);
  c->have_inputs = true;
  c->blocks_done = false;
  DropPrepared(c);
  return PrepareAhead(c);  // behind the copies, under whatever the caller does until it decodes
}

// JXLHIP_CODESTREAM_VERBOSE: the longest single wait of the upload path during one AC phase, microseconds
// [0] a pinned slot (AcquireSlot), [1] one hipMemcpyAsync call, [2] one hipEventRecord call
static std::atomic<int64_t> g_upload_wait_us[3];
std::atomic<bool> jxlhip::g_upload_wait_on{false};
struct UploadWaitClock {
  int which;
  std::chrono::steady_clock::time_point t0;
  explicit UploadWaitClock(int w) : which(w) {
    if (g_upload_wait_on.load(std::memory_order_relaxed)) t0 = std::chrono::steady_clock::now();
  }
  ~UploadWaitClock() {
    if (!g_upload_wait_on.load(std::memory_order_relaxed)) return;
    const int64_t us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    int64_t seen = g_upload_wait_us[which].load(std::memory_order_relaxed);
    while (seen < us && !g_upload_wait_us[which].compare_exchange_weak(seen, us, std::memory_order_relaxed)) {
    }
  }
};

static int jxlhip_submit_group_ev(jxlhip_ctx* c, uint32_t group_idx, const void* const coeffs[3],
                                  size_t ncoeffs, hipEvent_t done);

int jxlhip_submit_group(jxlhip_ctx* c, uint32_t group_idx, const void* const coeffs[3],
                        size_t ncoeffs) {
  return jxlhip_submit_group_ev(c, group_idx, coeffs, ncoeffs, nullptr);
}

// `done` (optional) is recorded behind the three copies on the slot's stream
static int jxlhip_submit_group_ev(jxlhip_ctx* c, uint32_t group_idx, const void* const coeffs[3],
                                  size_t ncoeffs, hipEvent_t done) {
  if (!c || !coeffs) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (c->multi) {
    if (!c->have_frame) return Fail(c, JXLHIP_ERR_STATE, "submit_group before frame_begin");
    const int o = MultiOwner(c, group_idx);
    if (o < 0) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "bad group %u", group_idx);
    jxlhip_ctx* k = c->multi->kids[o].ctx;
    return MultiCheck(c, k, jxlhip_submit_group_ev(k, group_idx, coeffs, ncoeffs, done));
  }
  if (!c->have_frame) return Fail(c, JXLHIP_ERR_STATE, "submit_group before frame_begin");
  const DevFrame& f = c->f;
  if (group_idx >= f.xsg * f.ysg || ncoeffs > JXLHIP_GROUP_COEFFS || !coeffs[0] || !coeffs[1] ||
      !coeffs[2])
    return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "bad group %u / ncoeffs %zu", group_idx, ncoeffs);
  const size_t esz = f.coeff_type == JXLHIP_COEFF_I16 ? 2 : 4;
  int slot;
  {
    // only the bookkeeping is serialised: the copies themselves are issued concurrently by the
    // runner's threads (with the lock around them, ~400 hipMemcpyAsync calls per 4K frame were
    // a 4.5 ms serial floor of the whole upload path).  A thread issues its three copies and
    // then its event on ONE stream in program order, so the event still follows its copies
    // however other threads' calls interleave on that stream.
    std::lock_guard<std::mutex> lock(c->pool_mu);
    if (hipSetDevice(c->device) != hipSuccess) return JXLHIP_ERR_HIP;
    // (re)sized for THIS frame's group count and coefficient type: a context reused for a larger
    // frame or another coefficient type must not write past the previous frame's allocation
    if (!c->up_coeffs[0] || c->up_groups != f.xsg * f.ysg || c->up_esz != esz) {
      int rc = EnsureUploadBuffers(c);
      if (rc) return rc;
    }
    slot = (int)(c->pool_next++ % kPoolStreams);
    c->pool_dirty[slot] = true;
  }
  if (hipSetDevice(c->device) != hipSuccess) return JXLHIP_ERR_HIP;
  const size_t chan = (size_t)JXLHIP_GROUP_COEFFS * esz;
  char* dst0 = (char*)c->up_coeffs[0] + (size_t)group_idx * 3 * chan;
  if ((const char*)coeffs[1] == (const char*)coeffs[0] + chan && (const char*)coeffs[2] == (const char*)coeffs[0] + 2 * chan) {
    // the three channels sit in one staging slot: one copy up to the last used coefficient
    hipError_t e;
    {
      UploadWaitClock w(1);
      e = hipMemcpyAsync(dst0, coeffs[0], 2 * chan + ncoeffs * esz, hipMemcpyHostToDevice, c->pool[slot]);
    }
    if (e != hipSuccess) return Fail(c, JXLHIP_ERR_HIP, "submit_group: %s", hipGetErrorString(e));
  } else {
    for (int ch = 0; ch < 3; ch++) {
      hipError_t e = hipMemcpyAsync(dst0 + ch * chan, coeffs[ch], ncoeffs * esz, hipMemcpyHostToDevice, c->pool[slot]);
      if (e != hipSuccess) return Fail(c, JXLHIP_ERR_HIP, "submit_group: %s", hipGetErrorString(e));
    }
  }
  if (done && hipEventRecord(done, c->pool[slot]) != hipSuccess)
    return Fail(c, JXLHIP_ERR_HIP, "submit_group: event record failed");
  return JXLHIP_OK;
}

// ---- sparse hand-off ------------------------------------------------------------------------------------------
// A single-pass, 16-bit group crosses PCIe as its NON-ZERO coefficients: 16 header bytes (three counts) + one
// (position << 16 | value) word per non-zero, the three channels' lists back to back -- nine out of ten
// coefficients of a d1.0 frame are zero, and the dense stream is 384 KB per group whatever it holds (8K: 196 MB per
// frame).  The compact groups of one runner thread are collected in a staging slot and go up TOGETHER: one
// hipMemcpyAsync costs ~15 us inside the runtime whatever thread issues it, serialised -- 510 per-group copies
// were an 8 ms floor under an 8K frame however many threads decoded.  sp_dev is a per-frame bump arena;
// sp_off_host[parity][g] says where group g's header landed (0xFFFFFFFF: handed over densely); BeginDecode uploads
// that table and k_expand_sparse rebuilds the dense block stream (zero + scatter) behind the uploads.
// entries per channel (X, Y, B), one slot's worth in total: the luma list can take EVERY coefficient of the group (a
// noise patch at d1.0 has 45 000 non-zero luma coefficients in a group), the chroma lists a quarter each
static constexpr uint32_t kSparseCap[3] = {16382u, 65536u, 16382u};
static constexpr size_t kSparseStride = 3u * (size_t)JXLHIP_GROUP_COEFFS * 2u;     // arena bytes per group, worst case

static int AcquireSlot(jxlhip_ctx* c, size_t slot_bytes, int* out);
static void ReleaseSlot(jxlhip_ctx* c, int slot, bool uploaded);


// the batch goes up as one copy through a pinned staging slot; its groups' headers are entered into the offset table
int jxlhip::SparseFlush(jxlhip_ctx* c, SparseBatch* b) {
  if (b->n == 0) return JXLHIP_OK;
  int slot = -1;
  int rc;
  {
    UploadWaitClock w(0);
    rc = AcquireSlot(c, kSparseStride, &slot);
  }
  if (rc) return rc;
  memcpy(c->stage[slot], b->buf.data(), b->used);
  const size_t bytes = (b->used + 255) & ~(size_t)255;
  const size_t off = c->sp_arena_used.fetch_add(bytes);
  int stream;
  {
    std::lock_guard<std::mutex> lock(c->pool_mu);
    stream = (int)(c->pool_next++ % kPoolStreams);
    c->pool_dirty[stream] = true;
  }
  if (off + bytes > c->sp_dev.n) rc = Fail(c, JXLHIP_ERR_STATE, "sparse arena overflow");
  if (!rc && hipSetDevice(c->device) != hipSuccess) rc = JXLHIP_ERR_HIP;
  if (!rc) {
    hipError_t e;
    {
      UploadWaitClock w(1);
      e = hipMemcpyAsync(c->sp_dev + off, c->stage[slot], b->used, hipMemcpyHostToDevice, c->pool[stream]);
    }
    if (e != hipSuccess) {
      rc = Fail(c, JXLHIP_ERR_HIP, "sparse submit: %s", hipGetErrorString(e));
    } else {
      UploadWaitClock w(2);
      if (hipEventRecord(c->stage_ev[slot], c->pool[stream]) != hipSuccess) rc = Fail(c, JXLHIP_ERR_HIP, "sparse submit: event record failed");
    }
  }
  if (!rc) {
    uint32_t* table = (uint32_t*)c->sp_off_host[c->frame_serial & 1u].p;
    for (int i = 0; i < b->n; i++) table[b->group[i]] = (uint32_t)((off + b->at[i]) >> 4);
    c->sp_any.store(true);
  }
  ReleaseSlot(c, slot, rc == JXLHIP_OK);
  b->used = 0;
  b->n = 0;
  return rc;
}

// One group, single pass, decoded into `scratch` (kSparseStride bytes) and appended to the batch.
// JXLHIP_ERR_RANGE: not representable (a chroma channel with more than kSparseCap non-zeros, a value outside 16 bits):
// the caller hands the group over densely.
static int SparseAppend(jxlhip_ctx* c, SparseBatch* b, uint8_t* scratch, const jxlhip_ac_pass* pass, uint32_t shift,
                        uint32_t group_idx, const uint8_t* ac_strategy, const int32_t* raw_quant, const uint8_t* quant_dc,
                        const uint8_t* data, size_t size, size_t* bit_pos) {
  const DevFrame& f = c->f;
  uint32_t* const ent[3] = {(uint32_t*)(scratch + 16), (uint32_t*)(scratch + 16) + kSparseCap[0],
                            (uint32_t*)(scratch + 16) + kSparseCap[0] + kSparseCap[1]};
  uint32_t cnt[3] = {0, 0, 0};
  size_t pos = *bit_pos, ncoeffs = 0;
  int rc = jxlhip_ac_group_decode_sparse(pass, f.xsb, f.ysb, group_idx % f.xsg, group_idx / f.xsg, ac_strategy, raw_quant, quant_dc,
                                         data, size, &pos, shift, ent, kSparseCap, cnt, &ncoeffs);
  if (rc) return rc;
  *bit_pos = pos;
  const size_t bytes = 16 + 4 * ((size_t)cnt[0] + cnt[1] + cnt[2]);
  if (b->buf.size() < kSparseStride) b->buf.resize(kSparseStride);
  if (b->n && (b->used + bytes > kSparseStride || b->n == kBatchGroups)) {
    if ((rc = SparseFlush(c, b))) return rc;
  }
  uint8_t* dst = b->buf.data() + b->used;
  uint32_t* hdr = (uint32_t*)dst;
  hdr[0] = cnt[0], hdr[1] = cnt[1], hdr[2] = cnt[2], hdr[3] = 0;
  memcpy(dst + 16, ent[0], (size_t)cnt[0] * 4);
  memcpy(dst + 16 + (size_t)cnt[0] * 4, ent[1], (size_t)cnt[1] * 4);
  memcpy(dst + 16 + ((size_t)cnt[0] + cnt[1]) * 4, ent[2], (size_t)cnt[2] * 4);
  b->group[b->n] = group_idx;
  b->at[b->n] = (uint32_t)b->used;
  b->n++;
  b->used += (bytes + 15) & ~(size_t)15;
  return JXLHIP_OK;
}

bool jxlhip::SparseEligible(const jxlhip_ctx* c, uint32_t num_passes) {
  return c->sparse_upload && num_passes == 1 && c->f.coeff_type == JXLHIP_COEFF_I16 && c->sp_dev &&
         c->sp_dev.n >= (size_t)c->f.xsg * c->f.ysg * kSparseStride && SparseTableItems(c) >= (size_t)c->f.xsg * c->f.ysg;
}

static int SubmitPassesImpl(jxlhip_ctx* c, uint32_t num_passes, const jxlhip_ac_pass* const* passes, const uint32_t* shifts,
                            uint32_t group_idx, const uint8_t* ac_strategy, const int32_t* raw_quant, const uint8_t* quant_dc,
                            const uint8_t* const* data, const size_t* sizes, size_t* bit_pos, bool allow_sparse,
                            std::vector<uint8_t>* dense_scratch = nullptr);

// f1: entropy-decode all passes of one AC group into a pinned staging slot and
// queue its upload.  The slot is reused only after its copies completed.
int jxlhip_ac_group_decode_submit_passes(jxlhip_ctx* c, uint32_t num_passes,
                                         const jxlhip_ac_pass* const* passes, const uint32_t* shifts,
                                         uint32_t group_idx, const uint8_t* ac_strategy,
                                         const int32_t* raw_quant, const uint8_t* quant_dc,
                                         const uint8_t* const* data, const size_t* sizes,
                                         size_t* bit_pos) {
  if (!c || !passes || !ac_strategy || !raw_quant || !data || !sizes || !bit_pos || num_passes == 0 ||
      num_passes > 11)
    return JXLHIP_ERR_INVALID_ARGUMENT;
  for (uint32_t p = 0; p < num_passes; p++)
    if (!passes[p] || !data[p] || (shifts && shifts[p] > 3)) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!c->have_frame) return Fail(c, JXLHIP_ERR_STATE, "ac_group_decode_submit before frame_begin");
  if (c->multi) {
    const int o = MultiOwner(c, group_idx);
    if (o < 0) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "bad group %u", group_idx);
    jxlhip_ctx* k = c->multi->kids[o].ctx;
    return MultiCheck(c, k, jxlhip_ac_group_decode_submit_passes(k, num_passes, passes, shifts, group_idx, ac_strategy,
                                                                              raw_quant, quant_dc, data, sizes, bit_pos));
  }
  return SubmitPassesImpl(c, num_passes, passes, shifts, group_idx, ac_strategy, raw_quant, quant_dc, data, sizes, bit_pos, true);
}

// A free pinned staging slot (state 1 = owned by the caller); blocks while all are in flight / owned.
static int AcquireSlot(jxlhip_ctx* c, size_t slot_bytes, int* out) {
  int slot = -1;
  std::unique_lock<std::mutex> lock(c->stage_mu);
  if (hipSetDevice(c->device) != hipSuccess) return JXLHIP_ERR_HIP;
  // kStageChunk more slots (the chunk after the ones there are), free
  auto grow = [&]() -> int {
    const int k = c->stage_count / kStageChunk;
    if (c->stage_count + kStageChunk > c->stage_cap)
      return Fail(c, JXLHIP_ERR_OUT_OF_MEMORY, "pinned staging: the cap of %d slots (JXLHIP_STAGE_SLOTS) is reached", c->stage_cap);
    // the events first, then the chunk, and only then is anything published: a failure half way leaves nothing
    // behind that a later grow() would overwrite (an event that exists already is simply kept)
    for (int i = c->stage_count; i < c->stage_count + kStageChunk; i++)
      if (c->stage_ev[i].Create() != hipSuccess)
        return Fail(c, JXLHIP_ERR_HIP, "event creation failed");
    if (c->stage_chunk[k].Alloc(&c->mm, (size_t)kStageChunk * c->stage_bytes) != JXLHIP_OK)
      return Fail(c, JXLHIP_ERR_OUT_OF_MEMORY, "pinned staging allocation failed");
    void* chunk = c->stage_chunk[k].p;
    for (int i = c->stage_count; i < c->stage_count + kStageChunk; i++) {
      c->stage[i] = (char*)chunk + (size_t)(i - c->stage_count) * c->stage_bytes;
      c->stage_state[i] = 0;
    }
    c->stage_count += kStageChunk;
    return JXLHIP_OK;
  };
  if (c->stage_bytes < slot_bytes) {
    // (re)allocation: only when no thread owns a slot
    c->stage_cv.wait(lock, [&] {
      for (int i = 0; i < c->stage_count; i++)
        if (c->stage_state[i] == 1) return false;
      return true;
    });
    if (c->stage_bytes < slot_bytes) {
      for (int i = 0; i < c->stage_count; i++) {
        if (c->stage_state[i] == 2) (void)hipEventSynchronize(c->stage_ev[i]);
        c->stage[i] = nullptr;
        c->stage_state[i] = 0;
      }
      for (PinnedBuf& chunk : c->stage_chunk) chunk.Free();
      c->stage_bytes = slot_bytes;
      c->stage_count = 0;
      static_assert(kStageSlotsFirst % kStageChunk == 0 && kStageSlots % kStageChunk == 0, "whole chunks");
      while (c->stage_count < kStageSlotsFirst) {
        const int rc = grow();
        if (rc) return rc;
      }
    }
  }
  while (slot < 0) {
    int pending = -1;
    for (int i = 0; i < c->stage_count && slot < 0; i++) {
      if (c->stage_state[i] == 0) slot = i;
      else if (c->stage_state[i] == 2) {
        if (hipEventQuery(c->stage_ev[i]) == hipSuccess) slot = i;
        else if (pending < 0) pending = i;
      }
    }
    if (slot >= 0) break;
    if (c->stage_count < c->stage_cap) {  // nothing free: more slots rather than a wait
      slot = c->stage_count;
      const int rc = grow();
      if (rc) return rc;
    } else if (pending >= 0) {  // every slot is in flight: wait for one upload, without keeping the others out
      hipEvent_t ev = c->stage_ev[pending];
      lock.unlock();
      const hipError_t e = hipEventSynchronize(ev);
      lock.lock();
      if (e != hipSuccess) return JXLHIP_ERR_HIP;
    } else {  // every slot is owned by another decoding thread
      c->stage_cv.wait(lock);
    }
  }
  c->stage_state[slot] = 1;
  *out = slot;
  return JXLHIP_OK;
}

static void ReleaseSlot(jxlhip_ctx* c, int slot, bool uploaded) {
  {
    std::lock_guard<std::mutex> lock(c->stage_mu);
    c->stage_state[slot] = uploaded ? 2 : 0;
  }
  c->stage_cv.notify_all();
}

static int SubmitPassesImpl(jxlhip_ctx* c, uint32_t num_passes, const jxlhip_ac_pass* const* passes, const uint32_t* shifts,
                            uint32_t group_idx, const uint8_t* ac_strategy, const int32_t* raw_quant, const uint8_t* quant_dc,
                            const uint8_t* const* data, const size_t* sizes, size_t* bit_pos, bool allow_sparse,
                            std::vector<uint8_t>* dense_scratch) {
  const DevFrame& f = c->f;
  if (group_idx >= f.xsg * f.ysg) return Fail(c, JXLHIP_ERR_INVALID_ARGUMENT, "bad group %u", group_idx);
  const size_t esz = f.coeff_type == JXLHIP_COEFF_I16 ? 2 : 4;
  const size_t slot_bytes = 3 * (size_t)JXLHIP_GROUP_COEFFS * esz;
  int rc = JXLHIP_ERR_RANGE;
  if (allow_sparse && SparseEligible(c, num_passes)) {  // one group = one batch (callers that submit groups one by one)
    SparseBatch b;
    std::vector<uint8_t> scratch(kSparseStride);
    rc = SparseAppend(c, &b, scratch.data(), passes[0], shifts ? shifts[0] : 0, group_idx, ac_strategy, raw_quant, quant_dc,
                      data[0], sizes[0], &bit_pos[0]);
    const int rf = SparseFlush(c, &b);
    if (rc == JXLHIP_OK) rc = rf;
  }
  if (rc == JXLHIP_ERR_RANGE) {
    // the dense form: decoded into the caller's (or a local) heap buffer; a pinned staging slot is held only for the
    // copy into it and the submit -- a textured group decodes for milliseconds, and with the slots held that long the
    // 33rd such group of a frame waited for the first to finish
    std::vector<uint8_t> local;
    std::vector<uint8_t>& buf = dense_scratch ? *dense_scratch : local;
    if (buf.size() < slot_bytes) buf.resize(slot_bytes);
    char* base = (char*)buf.data();
    void* const ch[3] = {base, base + (size_t)JXLHIP_GROUP_COEFFS * esz, base + 2 * (size_t)JXLHIP_GROUP_COEFFS * esz};
    size_t ncoeffs = 0;
    memset(base, 0, slot_bytes);  // coefficients are accumulated (dec_group.cc:527-531)
    rc = JXLHIP_OK;
    for (uint32_t p = 0; p < num_passes && rc == JXLHIP_OK; p++)
      rc = jxlhip_ac_group_decode(passes[p], f.xsb, f.ysb, group_idx % f.xsg, group_idx / f.xsg, ac_strategy,
                                  raw_quant, quant_dc, data[p], sizes[p], &bit_pos[p], shifts ? shifts[p] : 0,
                                  f.coeff_type, ch, &ncoeffs);
    if (rc == JXLHIP_OK) {
      int slot = -1;
      {
        UploadWaitClock w(0);
        rc = AcquireSlot(c, slot_bytes, &slot);
      }
      if (rc) return rc;
      char* pinned = (char*)c->stage[slot];
      const size_t chan = (size_t)JXLHIP_GROUP_COEFFS * esz;
      memcpy(pinned, base, 2 * chan + ncoeffs * esz);  // (what jxlhip_submit_group_ev sends up in one copy)
      const void* const src[3] = {pinned, pinned + chan, pinned + 2 * chan};
      rc = jxlhip_submit_group_ev(c, group_idx, src, ncoeffs, c->stage_ev[slot]);
      ReleaseSlot(c, slot, rc == JXLHIP_OK);
    }
  }
  if (rc == JXLHIP_ERR_BAD_STREAM) return Fail(c, rc, "AC group %u: invalid entropy-coded data", group_idx);
  return rc;
}

namespace jxlhip {
int GroupsInit(void* opaque, size_t num_threads) {
  GroupsJob* j = static_cast<GroupsJob*>(opaque);
  if (j->sparse) {
    j->batch.assign(num_threads ? num_threads : 1, SparseBatch());
    j->scratch.assign(num_threads ? num_threads : 1, std::vector<uint8_t>());
  }
  j->dense.assign(num_threads ? num_threads : 1, std::vector<uint8_t>());
  j->test_range_group = jxlhip_env::Get().test_range_group.load(std::memory_order_relaxed);
  return 0;
}
// A section this large carries more non-zeros than a chroma list of the sparse form takes (kSparseCap; the stream above:
// every group that overflowed had 32 000 bytes or more, none below 34 300 fitted with much to spare): decoded densely
// straight away instead of finding that out three quarters of the way through the sparse attempt.
static constexpr size_t kDenseFirstBytes = 30000;
void GroupsFuncBody(GroupsJob* j, uint32_t g, size_t thread);
// one group, with its entry in the timeline (keyed by group) when one is kept
void GroupsOne(GroupsJob* j, uint32_t g, size_t thread) {
  if (j->timeline.empty()) return GroupsFuncBody(j, g, thread);
  const double a = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - j->t0).count();
  GroupsFuncBody(j, g, thread);
  const double b = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - j->t0).count();
  j->timeline[3 * (size_t)g] = (float)a, j->timeline[3 * (size_t)g + 1] = (float)b, j->timeline[3 * (size_t)g + 2] = (float)thread;
}
void GroupsFunc(void* opaque, uint32_t task, size_t thread) {
  GroupsJob* j = static_cast<GroupsJob*>(opaque);
  GroupsOne(j, j->order.empty() ? task : j->order[task], thread);
}
void GroupsFuncBody(GroupsJob* j, uint32_t g, size_t thread) {
  if (j->status.load(std::memory_order_relaxed) != JXLHIP_OK) return;
  const DevFrame& f = j->c->f;
  const uint32_t gy = g / f.xsg;
  if (gy < f.group_y0 || gy >= f.group_y0 + f.group_rows) return;  // another rank's stripe
  const uint8_t* data[11];
  size_t sizes[11], pos[11];
  for (uint32_t p = 0; p < j->num_passes; p++) {
    data[p] = j->sections[(size_t)p * j->num_groups + g];
    sizes[p] = j->sizes[(size_t)p * j->num_groups + g];
    pos[p] = 0;
  }
  int rc = JXLHIP_ERR_RANGE;
  if ((int64_t)g == j->test_range_group && f.coeff_type == JXLHIP_COEFF_I16) {
    int expected = JXLHIP_OK;
    j->status.compare_exchange_strong(expected, JXLHIP_ERR_RANGE);
    return;
  }
  if (j->sparse && thread < j->batch.size() && sizes[0] < kDenseFirstBytes) {
    if (j->scratch[thread].empty()) j->scratch[thread].resize(kSparseStride);
    rc = SparseAppend(j->c, &j->batch[thread], j->scratch[thread].data(), j->passes[0], j->shifts ? j->shifts[0] : 0, g, j->acs,
                      j->raw_quant, j->quant_dc, data[0], sizes[0], &pos[0]);
    if (rc == JXLHIP_ERR_BAD_STREAM) Fail(j->c, rc, "AC group %u: invalid entropy-coded data", g);
  }
  if (rc == JXLHIP_ERR_RANGE)
    rc = SubmitPassesImpl(j->c, j->num_passes, j->passes, j->shifts, g, j->acs, j->raw_quant, j->quant_dc, data, sizes, pos, false,
                          thread < j->dense.size() ? &j->dense[thread] : nullptr);
  if (rc != JXLHIP_OK) {
    int expected = JXLHIP_OK;
    j->status.compare_exchange_strong(expected, rc);
  } else if (j->end_bits) {
    for (uint32_t p = 0; p < j->num_passes; p++) j->end_bits[(size_t)p * j->num_groups + g] = pos[p];
  }
}
}  // namespace jxlhip

// (JXLHIP_CODESTREAM_VERBOSE) per thread: first start, last end, busy time; and the longest task
void jxlhip::GroupsTimelineReport(const GroupsJob& job) {
  const double total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - job.t0).count();
  struct Th { float first = 1e9f, last = 0, busy = 0; int n = 0; };
  std::vector<Th> th(1024);
  int used = 0;
  float longest = 0, first_min = 1e9f, first_max = 0, last_min = 1e9f, busy_min = 1e9f, busy_max = 0;
  for (uint32_t t = 0; t < job.num_groups; t++) {
    const float a = job.timeline[3 * (size_t)t], b = job.timeline[3 * (size_t)t + 1];
    if (b <= 0) continue;
    Th& h = th[std::min<size_t>((size_t)job.timeline[3 * (size_t)t + 2], 1023)];
    h.first = std::min(h.first, a), h.last = std::max(h.last, b), h.busy += b - a, h.n++;
    longest = std::max(longest, b - a);
  }
  for (const Th& h : th) {
    if (!h.n) continue;
    used++;
    first_min = std::min(first_min, h.first), first_max = std::max(first_max, h.first), last_min = std::min(last_min, h.last);
    busy_min = std::min(busy_min, h.busy), busy_max = std::max(busy_max, h.busy);
  }
  fprintf(stderr, "[codestream] longest single wait in the upload path: pinned slot %.2f ms, hipMemcpyAsync %.2f ms, hipEventRecord %.2f ms\n",
          g_upload_wait_us[0].exchange(0) * 1e-3, g_upload_wait_us[1].exchange(0) * 1e-3, g_upload_wait_us[2].exchange(0) * 1e-3);
  fprintf(stderr, "[codestream] AC groups: %.2f ms after the runner call began, on %d threads; first group started at %.2f, last thread started at "
          "%.2f, first finished at %.2f; busy per thread %.2f .. %.2f ms; longest group %.2f ms\n", total, used, first_min, first_max, last_min,
          busy_min, busy_max, longest);
}

int jxlhip_ac_groups_decode_submit(jxlhip_ctx* c, jxlhip_parallel_runner runner, void* runner_opaque,
                                   uint32_t num_passes, const jxlhip_ac_pass* const* passes,
                                   const uint32_t* shifts, const uint8_t* ac_strategy,
                                   const int32_t* raw_quant, const uint8_t* quant_dc,
                                   const uint8_t* const* sections, const size_t* sizes) {
  return jxlhip_ac_groups_decode_submit_ex(c, runner, runner_opaque, num_passes, passes, shifts, ac_strategy, raw_quant, quant_dc,
                                           sections, sizes, nullptr);
}

int jxlhip_ac_groups_decode_submit_ex(jxlhip_ctx* c, jxlhip_parallel_runner runner, void* runner_opaque,
                                      uint32_t num_passes, const jxlhip_ac_pass* const* passes,
                                      const uint32_t* shifts, const uint8_t* ac_strategy,
                                      const int32_t* raw_quant, const uint8_t* quant_dc,
                                      const uint8_t* const* sections, const size_t* sizes, size_t* end_bits) {
  if (!c || !passes || !ac_strategy || !raw_quant || !sections || !sizes || num_passes == 0 || num_passes > 11)
    return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!c->have_frame) return Fail(c, JXLHIP_ERR_STATE, "ac_groups_decode_submit before frame_begin");
  if (c->multi) {  // every child takes the groups of its stripe (GroupsFunc skips the others)
    for (MultiChild& kid : c->multi->kids) {
      jxlhip_ctx* k = kid.ctx;
      const int rc = jxlhip_ac_groups_decode_submit_ex(k, runner, runner_opaque, num_passes, passes, shifts, ac_strategy, raw_quant,
                                                       quant_dc, sections, sizes, end_bits);
      if (rc) return MultiCheck(c, k, rc);
    }
    return JXLHIP_OK;
  }
  GroupsJob job;
  job.c = c;
  job.num_passes = num_passes;
  job.num_groups = c->f.xsg * c->f.ysg;
  job.passes = passes;
  job.shifts = shifts;
  job.acs = ac_strategy;
  job.raw_quant = raw_quant;
  job.quant_dc = quant_dc;
  job.sections = sections;
  job.sizes = sizes;
  job.end_bits = end_bits;
  job.sparse = SparseEligible(c, num_passes);
  if (runner && job.num_groups > 1) {
    std::vector<uint64_t> key(job.num_groups);  // (bytes over all passes) << 32 | ~group: sorted descending = largest first, ties in group order
    for (uint32_t g = 0; g < job.num_groups; g++) {
      uint64_t bytes = 0;
      for (uint32_t p = 0; p < num_passes; p++) bytes += sizes[(size_t)p * job.num_groups + g];
      key[g] = (std::min<uint64_t>(bytes, 0xFFFFFFFFu) << 32) | (uint32_t)~g;
    }
    std::sort(key.begin(), key.end(), std::greater<uint64_t>());
    job.order.resize(job.num_groups);
    for (uint32_t t = 0; t < job.num_groups; t++) job.order[t] = ~(uint32_t)key[t];
  }
  const bool verbose = jxlhip_env::Get().codestream_verbose.load(std::memory_order_relaxed);
  if (verbose) {
    job.timeline.assign(3 * (size_t)job.num_groups, 0.0f);
    job.t0 = std::chrono::steady_clock::now();
  }
  if (runner) {
    if (runner(runner_opaque, &job, GroupsInit, GroupsFunc, 0, job.num_groups) != 0)
      return Fail(c, JXLHIP_ERR_STATE, "parallel runner failed");
    if (verbose) GroupsTimelineReport(job);
  } else {
    GroupsInit(&job, 1);
    for (uint32_t g = 0; g < job.num_groups; g++) GroupsFunc(&job, g, 0);
  }
  for (SparseBatch& b : job.batch) {  // what the threads still hold
    const int rc = SparseFlush(c, &b);
    if (rc != JXLHIP_OK) {
      int expected = JXLHIP_OK;
      job.status.compare_exchange_strong(expected, rc);
    }
  }
  return job.status.load();
}

int jxlhip_ac_group_decode_submit(jxlhip_ctx* c, const jxlhip_ac_pass* pass, uint32_t group_idx,
                                  const uint8_t* ac_strategy, const int32_t* raw_quant,
                                  const uint8_t* quant_dc, const uint8_t* data, size_t size,
                                  size_t* bit_pos) {
  return jxlhip_ac_group_decode_submit_passes(c, 1, &pass, nullptr, group_idx, ac_strategy, raw_quant,
                                              quant_dc, &data, &size, bit_pos);
}

