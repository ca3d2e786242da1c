// context.h -- what the host units (context.hip, render_stages.hip, handover.hip, multi.hip, codestream.hip) share: struct jxlhip_ctx, the
// owner types of what it holds, Fail / HIPCHK, and the internal functions the units call across each other.  Not a
// public header: nothing here is part of the C ABI.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <vector>

#include "../../include/jxl_hip_codestream.h"
#include "../../include/jxl_hip_entropy.h"
#include "kernels.h"
#include "tile_bins.h"
#include "env_switches.h"  // (the switches themselves live in entropy.cc: that file is also built alone, by the fuzz harnesses)

namespace jxlhip {

int Fail(jxlhip_ctx* c, int code, const char* fmt, ...);

#define HIPCHK(c, call)                                                              \
  do {                                                                               \
    hipError_t e_ = (call);                                                          \
    if (e_ != hipSuccess)                                                            \
      return Fail(c, e_ == hipErrorOutOfMemory ? JXLHIP_ERR_OUT_OF_MEMORY           \
                                               : JXLHIP_ERR_HIP,                     \
                  "%s: %s", #call, hipGetErrorString(e_));                           \
  } while (0)

// ---- owners: each releases in its destructor and never waits; whoever replaces a buffer something may still be using
// synchronises first (jxlhip_destroy, jxlhip_alpha_staging, jxlhip_decode_frame_pinned, BeginHandover)

// Device memory, n elements of T.  Never shrunk, and never cleared on growth (EnsureUploadBuffers says why).
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  operator T*() const { return p; }
  int Reserve(jxlhip_ctx* c, size_t need) {
    if (need <= n && p) return JXLHIP_OK;
    if (p) HIPCHK(c, hipFree(p));
    p = nullptr;
    n = 0;
    HIPCHK(c, hipMalloc((void**)&p, need * sizeof(T)));
    n = need;
    return JXLHIP_OK;
  }
};

// Pinned host memory: from the caller's JxlMemoryManager when there is one (pinned in place with hipHostRegister:
// "caller owns the host memory, the library pins it"), else hipHostMalloc.  `mm` is the context's copy of
// the memory manager: it is declared in front of every PinnedBuf of the context and so outlives them.
struct PinnedBuf {
  void* p = nullptr;
  size_t bytes = 0;
  const JxlMemoryManagerHip* mm = nullptr;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  ~PinnedBuf() { Free(); }
  // replaces what is held; JXLHIP_ERR_OUT_OF_MEMORY (and empty) when it cannot
  int Alloc(const JxlMemoryManagerHip* m, size_t need) {
    Free();
    mm = m;
    if (mm->alloc) {
      p = mm->alloc(mm->opaque, need);
      if (!p) return JXLHIP_ERR_OUT_OF_MEMORY;
      if (hipHostRegister(p, need, hipHostRegisterDefault) != hipSuccess) {
        mm->free(mm->opaque, p);
        p = nullptr;
        return JXLHIP_ERR_OUT_OF_MEMORY;
      }
    } else if (hipHostMalloc(&p, need, hipHostMallocDefault) != hipSuccess) {
      p = nullptr;
      return JXLHIP_ERR_OUT_OF_MEMORY;
    }
    bytes = need;
    return JXLHIP_OK;
  }
  void Free() {
    if (!p) return;
    if (mm->alloc) {
      (void)hipHostUnregister(p);
      mm->free(mm->opaque, p);
    } else {
      (void)hipHostFree(p);
    }
    p = nullptr;
    bytes = 0;
  }
};

struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
  ~Event() {
    if (e) (void)hipEventDestroy(e);
  }
  operator hipEvent_t() const { return e; }
  hipError_t Create(unsigned flags = hipEventDisableTiming) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
};

struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(const Stream&) = delete;
  ~Stream() {
    if (s) (void)hipStreamDestroy(s);
  }
  operator hipStream_t() const { return s; }
  hipError_t Create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
};

constexpr int kPoolStreams = 8;
// pinned staging buffers of jxlhip_ac_group_decode_submit (0.4 / 0.8 MB each): kStageSlotsFirst at first use, one more
// whenever a thread would otherwise have to wait for an upload to finish, up to kStageSlots.  (An upload is microseconds
// of PCIe, but the runtime now and then sits on a queued copy for 10-30 ms -- profiles/r04_e2e_waits.txt -- and with 32
// slots for 64 decoding threads that stall became every thread's.)
constexpr int kStageSlots = 128, kStageSlotsFirst = 32;
// (slots are pinned kStageChunk at a time: one hipHostMalloc of 12 MB takes a tenth of the time of 32 of 0.4 MB, and a
// context's first frame -- all a one-shot tool ever decodes -- waited for them)
constexpr int kStageChunk = 32;

// jxlhip_ctx::tables, in floats: the coefficients of kWcHost, kResampleUpHost, the dither pattern, and the constants of
// the two matrix-core transforms (MfmaDct32Constants, MfmaDct16Constants)
constexpr size_t kTabWc = 0, kTabResample = kTabWc + 512, kTabDither = kTabResample + 64, kTabMfma32 = kTabDither + 1024,
                 kTabMfma16 = kTabMfma32 + 2048, kTabFloats = kTabMfma16 + 256;
static_assert(kTabFloats == 3904, "the layout the kernels were measured with");

// jxlhip_profile_enable: ONE event between consecutive launches (it ends the span of the launch before it and starts
// the span of the one after: rounds 1-5 recorded two, and the pass inflated every launch by ~9 %)
struct ProfMarkRec {
  Event ev;
  int slot_after = -1;  // kernel slot of the span that STARTS at this event; < 0: none (the end of a group of launches)
};

// jxlhip_create_multi: what a PARENT context keeps per child (multi.hip).  The halo staging and the output stripe live
// on the child's device.
struct MultiChild {
  jxlhip_ctx* ctx = nullptr;
  uint32_t group_y0 = 0, group_rows = 0;  // its stripe of the current frame
  DevBuf<float> halo_send[2], halo_recv[2];  // dense [3][halo][xsize] staging (0: up, 1: down)
  DevBuf<uint8_t> stripe_out;  // its output stripe when the frame goes to another device / the host
  Event ev_halo[2], ev_pull[2], ev_done;
};
struct MultiState {
  std::vector<MultiChild> kids;
};

// What jxlhip_set_splines / jxlhip_set_patches keep around a tile-binned list (tile_bins.h).  The host copies -- `host`
// and the stage's records, which go up in front of it on the same stream -- stay alive until `ev` says the upload is done.
struct TileList {
  DevBuf<uint32_t> dev;
  TileBins host;
  Event ev;
  bool pending = false;
  int WaitHostFree(jxlhip_ctx* c) {  // until the previous upload no longer reads the host copies
    if (pending) HIPCHK(c, hipEventSynchronize(ev));
    pending = false;
    return JXLHIP_OK;
  }
  int Upload(jxlhip_ctx* c, hipStream_t st) {
    if (const int rc = dev.Reserve(c, host.words.size())) return rc;
    HIPCHK(c, hipMemcpyAsync(dev, host.words.data(), host.words.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPCHK(c, ev.Create());
    HIPCHK(c, hipEventRecord(ev, st));
    pending = true;
    return JXLHIP_OK;
  }
  template <typename Args>  // SplineArgs / PatchArgs
  void Fill(Args* a) const {
    a->tiles_x = host.tiles_x;
    a->num_active = host.num_active;
    a->tile_start = dev;
    a->tile_idx = dev + host.num_tiles + 1;
    a->active = dev + host.num_tiles + 1 + host.entries;
  }
};

// ---- the render stages of the current frame, one struct per stage (render_stages.hip).  `on`, ups.factor and
// blend_ec.frame_n are per frame (StageState::ResetFrame); the buffers, host copies and events outlive frames.
// jxlhip_set_noise: photon noise; buf = the filtered frame as planar XYB + the random planes (kernels_noise.hip),
// jump = the generator's jump matrices (uploaded once)
struct NoiseStage {
  bool on = false;
  float lut[8] = {0};
  uint32_t visible = 0, nonvisible = 0;
  DevBuf<float> buf;
  DevBuf<uint32_t> jump;
};
// jxlhip_set_splines: the draw list, binned by 64 x 16 tile (kernels_splines.hip)
struct SplineStage {
  bool on = false;
  DevBuf<SplineSeg> segs;
  std::vector<SplineSeg> host_segs;
  TileList tiles;
};
// jxlhip_set_patches: the dictionary, binned by 64 x 16 tile (kernels_patches.hip).  The records point into the
// reference slots: ref_serial = SlotState::ref_serial at the dictionary's upload.
struct PatchStage {
  bool on = false;
  uint64_t ref_serial = 0;
  DevBuf<PatchRec> recs;
  std::vector<PatchRec> host_recs;
  TileList tiles;
};
// jxlhip_set_upsampling: the frame is upsampled by `factor` (1 = not) to xsize x ysize; planes = the filtered frame as
// planar XYB at CODED size (kernels_upsample.hip; noise.buf then holds the upsampled planes + the random planes at
// output size), weights = the factor's kernels (UpsampleKernels), weights_host the copy their upload reads
struct UpsampleStage {
  uint32_t factor = 1, xsize = 0, ysize = 0;
  DevBuf<float> planes, weights;
  float weights_host[64 * 25] = {0};
};
// jxlhip_set_dc_only_groups: the AC groups that are drawn from their DC; mask = one byte per group, weights = the 8x
// kernels as k_dc_upsample8 loads them (DcUpsampleWeights), host = the host copy of the mask (which coefficient slots
// ZeroDcOnlySlots zeroes)
struct DcOnlyStage {
  bool on = false;
  DevBuf<uint8_t> mask;
  DevBuf<float> weights;
  std::vector<uint8_t> host;
};
// jxlhip_set_blending: the frame is blended over a canvas and / or saved; stage = the frame's own output in front of
// k_blend (DecodeFrameBlended)
struct BlendStage {
  bool on = false;
  jxlhip_blend_params p{};
  DevBuf<float> stage;
};
// jxlhip_set_blending_extra: the frame's image has extra channels, which are blended and saved with the colour
// (set_blending resets `on` as well).  stage = the frame's own planes in front of k_ec_blend (uploaded by the call:
// p.num_extra_channels planes of f.ysize rows of stage_stride floats, the samples (x0 mod 4) floats in); frame_buf = the
// blended planes of a frame that is not saved; frame_planes = where the current frame's blended planes are (the save
// slot's or frame_buf; jxlhip_frame_extra_read), frame_n of them, 0 = none.
struct BlendEcStage {
  bool on = false;
  jxlhip_blend_extra_params p{};  // (its plane pointers are the caller's and not kept)
  DevBuf<float> stage, frame_buf;
  size_t stage_stride = 0;
  const float* frame_planes = nullptr;
  uint32_t frame_n = 0, frame_w = 0, frame_h = 0;
};
// jxlhip_set_tone_mapping: k = k_tone_map's constants, planes = the frame's own output as planar XYB at output size in
// front of it (DecodeFrameToneMapped)
struct ToneMapStage {
  bool on = false;
  ToneMapConstants k{};
  DevBuf<float> planes;
};
struct StageState {
  NoiseStage noise;
  SplineStage splines;
  PatchStage patches;
  UpsampleStage ups;
  DcOnlyStage dc_only;
  BlendStage blend;
  BlendEcStage blend_ec;
  ToneMapStage tone_map;
  void ResetFrame() {  // jxlhip_frame_begin: no stage is on
    noise.on = splines.on = patches.on = dc_only.on = blend.on = blend_ec.on = tone_map.on = false;
    ups.factor = 1;
    blend_ec.frame_n = 0;
  }
  // some stage between the loop filters and the XYB stage is on: the frame goes through DecodeFrameFeatures
  bool RenderStagesOn() const { return noise.on || splines.on || patches.on || ups.factor > 1; }
};

// The four slots (jxlhip_set_reference_frame, DecodeFrameBlended's save_slot); a slot holds one kind.  ref_planes[s] =
// a reference frame patches copy from: three dense XYB planes of ref_w x ref_h floats (0: empty); ref_serial =
// set_reference_frame calls so far.  canvas[s] = a canvas: interleaved float RGB in the output's transfer function,
// CanvasStride(canvas_w) floats per row (rows padded to four pixels: k_blend's 16-byte vectors), canvas_w x canvas_h (0:
// none); canvas_ec[s] = its canvas_nec[s] extra channels: planar planes of canvas_h rows of EcStride(canvas_w) floats.
struct SlotState {
  DevBuf<float> ref_planes[4];
  uint32_t ref_w[4] = {0, 0, 0, 0}, ref_h[4] = {0, 0, 0, 0};
  uint64_t ref_serial = 0;
  DevBuf<float> canvas[4];
  uint32_t canvas_w[4] = {0, 0, 0, 0}, canvas_h[4] = {0, 0, 0, 0};
  DevBuf<float> canvas_ec[4];
  uint32_t canvas_nec[4] = {0, 0, 0, 0};
};

// Where and as what a decode path writes (never read from c->p): the output kind (JXLHIP_OUT_*), the packed format,
// and the context's FilterParams with out, the strides, fmt and sample_mul of that.
struct OutTarget {
  uint32_t kind;
  jxlhip_output_format fmt;
  FilterParams fp;
};

}  // namespace jxlhip

using namespace jxlhip;

struct jxlhip_ctx {
  JxlMemoryManagerHip mm{};                            // jxlhip_create_ex / _multi: who allocated this object
  // jxlhip_create_multi: the context is a PARENT over one child context per device (a device may be
  // listed more than once); frame-level calls fan out to the children, each of which decodes a stripe
  // of group rows.  A parent owns no device memory of its own except the halo staging in there.
  std::unique_ptr<MultiState> multi;
  int device = 0;
  Stream own_stream;
  hipStream_t stream = nullptr;  // the one launches go to
  char err[512] = {0};
  bool have_frame = false;
  bool have_inputs = false;
  bool blocks_done = false;
  // Direct phase-1 launches alternate between counter blocks 0 and 1: k_prepare of frame N zeroes the block frame N + 1
  // will use (DevFrame::zero_counts) -- no memset launch per frame.  clean[b]: block b is all zero.
  int counts_slot = 0;
  bool counts_clean[2] = {false, false};
  // The prepared state (LaunchPhase1): k_prepare's outputs -- work lists, counters, cell_info, inv_sigma, the error
  // flag -- are a function of the side info and the frame constants only, so one prepare serves every direct phase 1 of
  // the same hand-over.  prepared: a prepare has been enqueued on `stream` with this key (the `fused` mode 0 / 1 / 2 and
  // the hand-over generation) on counter block prepared_block.  DropPrepared says who ends it.
  bool prepare_once = true;  // JXLHIP_PREPARE_ONCE=0: every phase 1 prepares
  bool prepared = false;
  bool prepared_ahead = false;  // ... by PrepareAhead, and no decode has used it yet (the first one is no "reuse")
  int prepared_fused = 0;
  int prepared_block = 0;
  uint64_t prepared_gen = 0;
  uint64_t handover_gen = 0;  // advances with every hand-over of side info and whatever else k_prepare reads
  bool capture_seen = false;  // a phase 1 of this frame was recorded into a graph: its replays rewrite the shared lists
                              // behind the host's back, direct calls prepare every time until the next frame_begin
  // direct calls only (jxlhip_debug_prepare_launches): k_prepare launches, and phase 1s that saved one -- a decode that
  // takes up the prepare its hand-over enqueued ahead is neither
  uint64_t prepares_launched = 0, prepares_reused = 0;
  double cs_phase_ms[8] = {};  // jxlhip_codestream_phase_ms
  int concurrency = 1;  // jxlhip_set_concurrency_hint: contexts the caller keeps busy on this device at a time
  bool handover_fresh = false;  // frame_begin started the hand-over and upload_side_info has not been called since
  bool blocks_fused = false;  // jxlhip_decode_blocks ran in fused-stripe mode: the planes lack the inner DCT8 blocks
  jxlhip_frame_params p{};
  DevFrame f{};
  FilterParams fp{};
  SharpLut lut{};
  // context-owned device memory
  DevBuf<float> planes;  // 3 planes
  DevBuf<unsigned char> orient_dev;  // undo_orientation: the frame in coded orientation (jxlhip_decode_frame)
  DevBuf<float> planes2;  // epf_iters == 3: EPF0 output, the EPF1 + EPF2 march's input (kernels_epf0.hip)
  DevBuf<float> inv_sigma;
  DevBuf<WorkItem> lists;
  DevBuf<uint32_t> counts;    // kNumClasses
  DevBuf<int32_t> error_flag; // [0] stream error, [1] table status
  DevBuf<float> tables;       // kTabFloats: see kTabWc
  DevBuf<jxlhip_quant_encoding> quant_enc;  // device: the 17 resolved encodings of the last table build
  jxlhip_quant_encoding quant_enc_host[JXLHIP_NUM_QUANT_TABLES];
  WorkLists wl{};
  uint32_t max_items[kNumClasses] = {0};
  // upload path
  DevBuf<uint8_t> up_coeff_slab;
  void* up_coeffs[3] = {nullptr, nullptr, nullptr};  // the three channels of group 0 inside up_coeff_slab
  uint32_t up_groups = 0;  // geometry the upload buffers were laid out for
  size_t up_esz = 0;
  DevBuf<uint8_t> up_side;  // one slab: acs, quant, sharp, ytox, ytob, dc*3, dequant
  jxlhip_frame_inputs up_inputs{};
  // sparse coefficient hand-off (jxlhip_ac_group_decode_submit, single-pass 16-bit frames): a group's non-zero
  // coefficients go up as (position << 16 | value) words into sp_dev + group * kSparseStride; BeginDecode expands the
  // groups whose sp_mode byte is set into the dense upload buffer (k_expand_sparse)
  bool sparse_upload = true;  // JXLHIP_SPARSE_UPLOAD=0 turns it off
  DevBuf<uint8_t> sp_dev;
  uint32_t frame_serial = 0;
  std::atomic<bool> sp_any{false};
  std::atomic<size_t> sp_arena_used{0};   // sp_dev is a per-frame bump arena: a staging slot's worth of groups per copy
  PinnedBuf sp_off_host[2];  // per frame parity: arena offset / 16 of every group's header (uint32_t),
                             // 0xFFFFFFFF = the group was handed over densely
  Event sp_off_ev[2];        // "the copy of sp_off_host[parity] has executed"
  bool sp_off_pending[2] = {false, false};
  DevBuf<uint32_t> sp_off_dev;
  Stream pool[kPoolStreams];
  Event pool_ev[kPoolStreams];
  Event frame_ev;  // jxlhip_frame_begin: "everything queued for the previous frame", see there
  bool pool_dirty[kPoolStreams] = {false};
  std::mutex pool_mu;
  uint32_t pool_next = 0;
  // entropy-decode staging: pinned host buffers (3 channels x 65536 coefficients
  // each), reused round-robin; stage_ev[i] fires when slot i's upload is done
  void* stage[kStageSlots] = {nullptr};
  Event stage_ev[kStageSlots];
  int stage_state[kStageSlots] = {0};  // 0 free, 1 owned by a decoding thread, 2 upload queued (stage_ev)
  int stage_count = 0;                 // slots allocated so far (<= stage_cap), kStageChunk at a time
  int stage_cap = kStageSlots;         // JXLHIP_STAGE_SLOTS (read at jxlhip_create): pinned host memory per context is at
                                       // most stage_cap x 0.8 MB -- several contexts per device share the host's lockable memory
  PinnedBuf stage_chunk[kStageSlots / kStageChunk];  // the allocations the slots are carved from
  size_t stage_bytes = 0;
  std::mutex stage_mu;
  std::condition_variable stage_cv;
  // dc scratch
  DevBuf<float> dc_tmp;
  DevBuf<uint8_t> dc_prec;  // per-DC-group extra_precision of jxlhip_dequant_dc_groups
  DevBuf<uint8_t> host_frame_dev;  // jxlhip_decode_frame_host: the device frame in front of the D2H copy
  PinnedBuf pinned_frame;  // jxlhip_decode_frame_pinned: context-owned pinned host frame
  DevBuf<float> alpha_dev;  // jxlhip_set_alpha: the frame's alpha plane (xsize floats per row)
  PinnedBuf alpha_host;  // jxlhip_alpha_staging: pinned plane the caller fills
  DevBuf<int32_t> qdc_dev;  // jxlhip_decode_codestream: the quantized DC planes on their way to jxlhip_dequant_dc_groups
  // jxlhip_decode_modular_frame: the three integer planes and the per-group RCT programs on the device; the pinned
  // planes and programs a lossless file's host decode fills (jxlhip_decode_codestream)
  DevBuf<uint8_t> modular_dev;
  DevBuf<uint16_t> modular_rct_dev;
  PinnedBuf modular_host;
  StageState st;  // the render stages of the current frame (jxlhip_frame_begin: ResetFrame)
  SlotState slots;  // the four reference / canvas slots: they outlive frames
  // jxlhip_codestream_set_display: sticky on the context (0 = not set), read by the whole-file decode calls
  float display_nits = 0.0f;
  uint32_t display_primaries = 0, display_white_point = 0;
  // jxlhip_decode_codestream_next: a sequence is open and this is the cursor the next call must bring
  bool seq_open = false;
  uint64_t seq_expect = 0;
  bool generic_filters = false;  // JXLHIP_FILTERS=generic: LDS kernel for every stage list
  int mfma = -1;                 // DCT32X32 / DCT16X16 on the matrix cores (kernels_mfma.hip; the 16x16 rule is in
                                 // LaunchPhase1).  -1 (default): when the caller's
                                 // used_acs says DCT32X32 is the only class of the row-per-lane 32-point family in
                                 // the frame (the class kernel then is a launch of its own anyway; measured on c5:
                                 // 219 -> 193 us); on mixed frames the butterflies inside the merged launch win
                                 // (c3: blocks 95 -> 105 us with a separate MFMA launch).  JXLHIP_MFMA=0 / 1 forces.
  int fuse = -1;                 // the fused kernel (kernels_fused.hip) in jxlhip_decode_frame.  -1 (default): for
                                 // frames of 12 Mpx and more -- a fused wave pays its halo rows and a fill per 8 rows,
                                 // which only amortises when the frame gives every resident wave enough rows (8K d1.0:
                                 // fused 89.9 vs 80 Gpx/s two-phase; 6144x3456: 88.5 vs 77.4; 5120x2880: 87.5 vs 82.2;
                                 // 4K: 71.2 vs 80.3; 1024^2: 16.9 vs 18.3; profiles/r02_fused_rows_sweep*.txt,
                                 // r02_fused_size_threshold.txt).  JXLHIP_FUSE=0 / 1 forces.
  DevBuf<uint2> cell_info;       // fused mode: per-cell coefficient offset + quant / CfL word (k_prepare)
  // profiling
  bool profiling = false;
  std::vector<ProfMarkRec> marks;
};

namespace jxlhip {

// entries of the sparse offset tables (both parities are allocated together)
inline size_t SparseTableItems(const jxlhip_ctx* c) { return std::min(c->sp_off_host[0].bytes, c->sp_off_host[1].bytes) / 4; }

// bytes of one sample of a packed output format
inline size_t OutSampleBytes(const jxlhip_output_format& o) {
  return o.sample_type == JXLHIP_SAMPLE_U8 ? 1 : (o.sample_type == JXLHIP_SAMPLE_F32 ? 4 : 2);
}
// bytes of one interleaved output pixel (0: planar XYB)
inline size_t OutPixelBytes(uint32_t kind, const jxlhip_output_format& o) {
  if (kind == JXLHIP_OUT_LINEAR_RGB_F32) return 12;
  return kind == JXLHIP_OUT_PACKED ? (size_t)o.num_channels * OutSampleBytes(o) : 0;
}
inline size_t OutPixelBytes(const jxlhip_ctx* c) { return OutPixelBytes(c->p.output_kind, c->p.out_format); }

// columns / rows of what jxlhip_decode_frame writes in coded orientation: the context's stripe of the frame, or the
// size an upsampled frame (jxlhip_set_upsampling: whole frames only) comes out at
inline size_t OutCols(const jxlhip_ctx* c) { return c->st.ups.factor > 1 ? c->st.ups.xsize : c->f.xsize; }
inline size_t OutRows(const jxlhip_ctx* c) { return c->st.ups.factor > 1 ? c->st.ups.ysize : c->f.y1 - c->f.y0; }
// ... and of what the caller's buffer holds: the image when the frame is blended (jxlhip_set_blending)
inline size_t BufCols(const jxlhip_ctx* c) { return c->st.blend.on ? c->st.blend.p.image_xsize : OutCols(c); }
inline size_t BufRows(const jxlhip_ctx* c) { return c->st.blend.on ? c->st.blend.p.image_ysize : OutRows(c); }

// A target of `kind` and (packed) `fmt` at out; MakeTarget(c, out, ..): the one jxlhip_frame_begin was given.
inline OutTarget MakeTarget(const jxlhip_ctx* c, uint32_t kind, const jxlhip_output_format& fmt, void* out, size_t out_stride,
                            size_t out_plane_stride) {
  OutTarget t{kind, fmt, c->fp};
  t.fp.out = out;
  t.fp.out_stride = out_stride;
  t.fp.out_plane_stride = out_plane_stride;
  if (kind == JXLHIP_OUT_PACKED) {  // (as jxlhip_frame_begin)
    const bool is_int = fmt.sample_type == JXLHIP_SAMPLE_U8 || fmt.sample_type == JXLHIP_SAMPLE_U16;
    t.fp.fmt = fmt;
    t.fp.sample_mul = is_int ? (float)((1u << fmt.bits_per_sample) - 1u) : 1.0f;
  }
  return t;
}
inline OutTarget MakeTarget(const jxlhip_ctx* c, void* out, size_t out_stride, size_t out_plane_stride) {
  return MakeTarget(c, c->p.output_kind, c->p.out_format, out, out_stride, out_plane_stride);
}

// context.hip
jxlhip_ctx* NewCtx(const JxlMemoryManagerHip* mm);
void DeleteCtx(jxlhip_ctx* c);
void ApplyInputs(jxlhip_ctx* c, const jxlhip_frame_inputs* in);
// Ends the prepared state and starts a new hand-over generation: whatever k_prepare reads may have changed (every
// caller is listed at LaunchPhase1).
inline void DropPrepared(jxlhip_ctx* c) {
  c->prepared = false;
  c->handover_gen++;
}
// The side info of the current hand-over is queued on c->stream: enqueues its prepare right behind it, in the mode the
// context would decode it with now (jxlhip_upload_side_info, jxlhip_decode_codestream).  render_stages: the caller
// knows that splines, upsampling or noise will be set for this frame (its own path then writes planar XYB).
int PrepareAhead(jxlhip_ctx* c, bool render_stages = false);
bool Capturing(hipStream_t st);
void ProfBegin(jxlhip_ctx* c), ProfMark(jxlhip_ctx* c, int slot);
// cols x rows: what the call writes -- the stripe at coded size, or an upsampled frame (OutCols / OutRows)
int CheckOutArgs(jxlhip_ctx* c, const OutTarget& t, size_t cols, size_t rows);
// both phases over the whole stripe at coded size, without any render stage
int DecodeFrameCoded(jxlhip_ctx* c, const OutTarget& t);

// render_stages.hip
int ZeroDcOnlySlots(jxlhip_ctx* c), LaunchDcOnly(jxlhip_ctx* c);  // jxlhip_set_dc_only_groups: in front of phase 1, behind it
// the frame's own path: DecodeFrameFeatures when a render stage is on (StageState::RenderStagesOn), else DecodeFrameCoded
int DecodeFrameOwnPath(jxlhip_ctx* c, const OutTarget& t);
int DecodeFrameBlended(jxlhip_ctx* c, void* out, size_t out_stride);
int DecodeFrameToneMapped(jxlhip_ctx* c, void* out, size_t out_stride);

// multi.hip
void MultiDestroy(jxlhip_ctx* c);
int MultiFrameBegin(jxlhip_ctx* c, const jxlhip_frame_params* p);
int MultiOwner(const jxlhip_ctx* c, uint32_t group_idx);
int MultiDecodeFrame(jxlhip_ctx* c, void* out_dev, void* host_out, size_t out_stride, size_t out_plane_stride);
int MultiSync(jxlhip_ctx* c);
int MultiCheck(jxlhip_ctx* c, jxlhip_ctx* child, int rc);
#define JXLHIP_NO_MULTI(c)                                                                                   \
  do {                                                                                                       \
    if ((c) && (c)->multi)                                                                                   \
      return Fail((c), JXLHIP_ERR_UNSUPPORTED, "%s is not available on a multi-device context", __func__); \
  } while (0)

// handover.hip
constexpr int kBatchGroups = 96;
struct SparseBatch {  // what one runner thread has collected (in its own heap buffer: a pinned staging slot is only
  std::vector<uint8_t> buf;  // held for the moment of the copy -- more threads than slots must not starve each other)
  size_t used = 0;
  int n = 0;
  uint32_t group[kBatchGroups];
  uint32_t at[kBatchGroups];  // byte offset of the group's header inside the slot
};
struct GroupsJob {
  jxlhip_ctx* c;
  uint32_t num_passes, num_groups;
  const jxlhip_ac_pass* const* passes;
  const uint32_t* shifts;
  const uint8_t* acs;
  const int32_t* raw_quant;
  const uint8_t* quant_dc;
  const uint8_t* const* sections;
  const size_t* sizes;
  size_t* end_bits = nullptr;
  std::atomic<int> status{JXLHIP_OK};
  // the runner's task t is group order[t]: the sections with the most bytes first.  A group's decode time follows its
  // bytes (r = 0.98 on the 8K d1.0 stream of tests/data) and a textured patch takes five times the mean: handed out
  // last, one such group is the tail the whole frame waits for
  std::vector<uint32_t> order;
  // JXLHIP_CODESTREAM_VERBOSE=1: per task {start ms, end ms, thread}
  std::vector<float> timeline;
  std::chrono::steady_clock::time_point t0;
  // sparse hand-off: one open staging slot + one decode scratch per runner thread
  bool sparse = false;
  std::vector<SparseBatch> batch;
  std::vector<std::vector<uint8_t>> scratch;
  std::vector<std::vector<uint8_t>> dense;  // per runner thread: where a group that goes up densely is decoded
  // test hook (JXLHIP_TEST_RANGE_GROUP=g, read by GroupsInit): group g reports a coefficient beyond 16 bits on the
  // 16-bit attempt -- no stream libjxl's encoder writes at ordinary settings does, and the redo with int32 buffers
  // (through the single runner call and through the three barriers) has to be reachable by a test
  int64_t test_range_group = -1;
};
extern std::atomic<bool> g_upload_wait_on;  // JXLHIP_CODESTREAM_VERBOSE: the upload-wait clock runs
int BeginHandover(jxlhip_ctx* c);
int EnsureUploadBuffers(jxlhip_ctx* c);
bool SparseEligible(const jxlhip_ctx* c, uint32_t num_passes);
int SparseFlush(jxlhip_ctx* c, SparseBatch* b);
int GroupsInit(void* opaque, size_t num_threads);
void GroupsOne(GroupsJob* j, uint32_t g, size_t thread);
void GroupsTimelineReport(const GroupsJob& job);

}  // namespace jxlhip
