// frame_decode.h -- what codestream.hip needs of frame_decode.hip: one VarDCT frame of a file, from its TOC to the pixels.
#ifndef JXLHIP_FRAME_DECODE_H_
#define JXLHIP_FRAME_DECODE_H_

#include "context.h"
#include "sequence_walk.h"

namespace jxlhip {

// jxlhip_decode_codestream_partial: which sections of the frame are inside the bytes (PlanPartial)
struct PartialPlan {
  jxlhip_partial_info info{};
  std::vector<uint8_t> passes_of;  // per AC group: how many leading passes are complete (0 = drawn from its DC)
};

// wall-clock of the phases of the last jxlhip_decode_codestream on a context (jxlhip_codestream_phase_ms)
struct PhaseClock {
  double* ms = nullptr;
  std::chrono::steady_clock::time_point t;
  void Start(double* out) {
    ms = out;
    t = std::chrono::steady_clock::now();
    for (int i = 0; i < JXLHIP_CODESTREAM_PHASES; i++) ms[i] = 0.0;
  }
  void Mark(int phase) {
    const auto now = std::chrono::steady_clock::now();
    ms[phase] += std::chrono::duration<double, std::milli>(now - t).count();
    t = now;
  }
};

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

// One VarDCT frame of a file: from the first bit behind its frame header (the TOC) to the pixels (FrameCall::out; with
// FrameCall::blend, blended over a canvas and / or saved, jxlhip_set_blending).  *end_bit_pos (may be NULL) = the first
// bit behind its sections: the next frame's header.
int DecodeFrameAt(jxlhip_ctx* c, const uint8_t* cs, size_t n, const ParsedHeaders& h, const jxlhip_frame_header& fh,
                  size_t frame_bit_pos, const FrameCall& fc, PhaseClock& clock, bool verbose, jxlhip_codestream_info* info_p,
                  size_t* end_bit_pos);


// The one frame of a lossless file (ParsedHeaders::modular: a regular Modular frame of an image that is not XYB
// encoded), from its TOC to the pixels: the host decode of its sections into pinned integer planes
// (modular_image.h), their upload and k_modular_emit or k_modular_planes (jxlhip_decode_modular_channels), jxlhip_sync.
// An alpha channel goes up as a fourth integer plane; extra-channel planes the caller asked for are filled on the host.
int DecodeModularFrameAt(jxlhip_ctx* c, const uint8_t* cs, size_t n, const ParsedHeaders& h, const FrameCall& fc, PhaseClock& clock,
                         jxlhip_codestream_info* info);

}  // namespace jxlhip

#endif  // JXLHIP_FRAME_DECODE_H_
