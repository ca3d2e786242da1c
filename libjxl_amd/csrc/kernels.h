// kernels.h -- host-callable launchers of the HIP kernels (internal).
#ifndef JXLHIP_KERNELS_H_
#define JXLHIP_KERNELS_H_

#include "dev_common.h"

namespace jxlhip {

struct WorkLists {
  WorkItem* list[kNumClasses];
  uint32_t* count;  // kCountStride counters (classes + unit tickets), zeroed before k_prepare
};

struct SharpLut {
  float v[8];
};

// Stage parameters of phase 2, precomputed on the host exactly as the
// reference stages do in their constructors / per-row prologues.
struct FilterParams {
  float gab_w[3][3];     // per channel: normalised w0, w1, w2 (stage_gaborish.cc:36-53)
  float ch_scale[3];     // epf_channel_scale
  float sm[3], bsm[3];   // per EPF stage: sigma multiplier inside / on 8x8 borders
  float opsin_bias[3];   // OpsinParams::opsin_biases
  float cbrt_bias[3];    // cbrt(opsin_biases)
  float minv[9];         // inverse opsin matrix * 255/intensity_target
  float xyb_bias[6];     // -cbrt_bias[0..2], opsin_bias[0..2] (filters_march.h)
  float mcol[3][4];      // its columns, wrapped: (m[j], m[3+j], m[6+j], m[j]) (filters_march.h)
  void* out;
  size_t out_stride;        // RGB / packed: bytes per row; XYB: floats per row
  size_t out_plane_stride;  // XYB only
  // JXLHIP_OUT_PACKED: FromLinearStage + WriteToOutputStage parameters
  jxlhip_output_format fmt;
  float sample_mul;         // 2^bits_per_sample - 1
  float tf_scale;           // PQ: intensity_target / 10000; GAMMA: inverse gamma
  float hlg_exponent;       // HLG: HlgOOTF exponent (gamma - 1), 0 = OOTF not applied
  const float* dither;      // 32x32 pattern (device)
  // dither coordinates = (dither_x0 + dither_xs * x, dither_y0 + dither_ys * y): the reference dithers AFTER
  // undo_orientation's flips (stage_write.cc:486-492): identity = (0, 1, 0, 1)
  int32_t dither_x0, dither_xs, dither_y0, dither_ys;
  // 4-channel packed output: the frame's alpha channel (floats, image coordinates, alpha_stride floats per row);
  // nullptr = the opaque 1.0 the reference substitutes (stage_write.cc:355-360)
  const float* alpha;
  uint32_t alpha_stride;
};

void LaunchPrepare(const DevFrame& f, const WorkLists& wl, int with_sigma, float epf_quant_mul,
                   const SharpLut& lut, hipStream_t st);
// The transform kernels (k_transform_8, the row-per-lane families R16 / R32 or their merged k_transform_r, family A,
// the matrix-core classes, the large kinds), back to back on `st`; `cells` = block cells of the stripe (bounds the
// unit count).  emit: see LaunchMfma32 (nullptr: every class writes the XYB planes).
void LaunchBlocks(const DevFrame& f, const WorkLists& wl, uint32_t cells, const float* wc,
                  const float* resample, hipStream_t st, const FilterParams* emit = nullptr);
// Returns 0, or -1 when the (gab, epf_iters, output_kind) combination is invalid.
int LaunchFilters(const DevFrame& f, const FilterParams& p, int gab, int epf_iters,
                  int output_kind, hipStream_t st);

// Register/DPP kernel for stage lists with at most one EPF pass; returns false
// when the configuration is not covered (caller falls back to LaunchFilters).
bool LaunchFiltersFast(const DevFrame& f, const FilterParams& p, int gab, int epf_iters,
                       int output_kind, hipStream_t st);
// the packed formats LaunchFiltersFast has a kernel with the format fixed at compile time for
bool FastFixedFormat(const jxlhip_output_format& o);

// epf_iters = 3 (kernels_epf0.hip): [Gaborish] + EPF0 from f.xyb into a second plane set; the EPF1 + EPF2 march
// (LaunchFiltersFast with gab = 0, epf_iters = 2 on those planes) follows.  false: geometry not covered.
bool LaunchEpf0(const DevFrame& f, const FilterParams& p, int gab, float* const dst[3], hipStream_t st);

// Sparse coefficient hand-off (kernels_tables.hip k_expand_sparse): group g of [g0, g0 + n) whose entry in `offsets`
// is not 0xFFFFFFFF is expanded from `sparse + 16 * offsets[g]` -- three counts + pad, then the (position << 16 |
// value) lists of the three channels back to back -- into the dense int16 block stream `dense`
// ([group][channel][65536], zero-filled first)
void LaunchExpandSparse(const uint8_t* sparse, const uint32_t* offsets, int16_t* dense, uint32_t g0, uint32_t n, hipStream_t st);

// undo_orientation (kernels_tables.hip k_orient): coded xsize x ysize pixels of bytes_per_pixel -> display orientation
bool LaunchOrient(const void* src, size_t src_stride, uint32_t xsize, uint32_t ysize, uint32_t bytes_per_pixel,
                  uint32_t orientation, void* dst, size_t dst_stride, hipStream_t st);

// Matrix-core 32x32 IDCT (kernels_mfma.hip), opt-in through DevFrame::mfma32
void MfmaDct32Constants(float* host /* 2048 floats */);
void MfmaDct16Constants(float* host /* 256 floats */);
// emit != nullptr: the frame is DCT32X32 only and has no loop filter -- the kernel writes linear float RGB to
// emit->out itself (rows f.y0 .. f.y1) instead of XYB planes.  grid: workgroups of four waves (Phase1Plan::mfma32 / 16)
void LaunchMfma32(const DevFrame& f, const WorkLists& wl, uint32_t grid, hipStream_t st, const FilterParams* emit = nullptr);
// Matrix-core 16x16 IDCT, opt-in through DevFrame::mfma16
void LaunchMfma16(const DevFrame& f, const WorkLists& wl, uint32_t grid, hipStream_t st);

// Fused kernel (kernels_fused.hip): the row march fed from the coefficient stream (DCT8 decoded by the
// filter wave itself, other classes copied from the planes).  FusedSupported: frames it takes --
// decided before k_prepare, which routes the DCT8 blocks (DevFrame::fused).
bool FusedSupported(const DevFrame& f, int gab, int epf_iters, int output_kind);
bool LaunchFused(const DevFrame& f, const FilterParams& p, int gab, int epf_iters, int output_kind,
                 hipStream_t st);
// epf_iters = 3 in fused mode (kernels_fused_epf0.hip): [Gaborish] + EPF0 marched from the producer's slab into the
// second plane set, as LaunchEpf0 does from the planes; FusedEpf0Supported: whole frames it takes (decided before
// k_prepare, like FusedSupported)
bool FusedEpf0Supported(const DevFrame& f, int gab);
bool LaunchFusedEpf0(const DevFrame& f, const FilterParams& p, int gab, float* const dst[3], hipStream_t st);
// compute units of the device the calling thread has current (hipDeviceAttributeMultiprocessorCount, cached): what the
// generation-filling launch geometries are sized from (256 on a whole MI355X, fewer on a CPX / DPX partition)
unsigned DeviceCus();
// Rows per chunk of a row march whose launch is `wgx` columns of workgroups over `rows` rows, `resident` of them on
// the device at a time.  Every workgroup costs its chunk height plus `overhead` row steps and all of a launch take
// the same time, so the launch runs in ceil(workgroups / resident) generations: the height among first, first + step,
// .. last that minimises generations * cost instead of leaving a mostly empty last generation (the lowest on a tie).
inline int ChunkRows(unsigned wgx, unsigned rows, unsigned resident, int first, int last, int step, int overhead) {
  int best = 64;
  double best_cost = 1e30;
  for (int rh = first; rh <= last; rh += step) {
    const unsigned wgs = wgx * ((rows + rh - 1) / rh);
    const unsigned gens = (wgs + resident - 1) / resident;
    const double cost = (double)gens * (rh + overhead);
    if (cost < best_cost) {
      best_cost = cost;
      best = rh;
    }
  }
  return best;
}

// Photon noise (kernels_noise.hip).  The fill sequence of a group's generator is cut into segments of kNoiseSegFills
// fills; kNoiseSegs segments cover the longest one (3 planes x 256 rows x 16 fills).
constexpr uint32_t kNoiseSegFills = 128;
constexpr uint32_t kNoiseSegs = (3u * 256u * 16u + kNoiseSegFills - 1) / kNoiseSegFills;
constexpr uint32_t kNoiseJumpWords = 128 * 4;  // one 128x128-bit matrix: 128 columns of 4 words
struct NoiseArgs {
  uint32_t xsize, ysize, xsg, ysg;
  uint32_t visible, nonvisible;  // PassesDecoderState::visible_frame_index / nonvisible_frame_index
  float lut[8];                  // NoiseParams::lut
  float ytox, ytob;              // ColorCorrelation::YtoXRatio(0) / YtoBRatio(0)
  const float* xyb;              // the filtered frame: 3 planes, ns floats per row, nplane floats apart
  float* rnd;                    // the random planes, same layout
  uint32_t ns;                   // a multiple of 64
  size_t nplane;                 // a multiple of 64
  const uint32_t* jump;          // kNoiseSegs x kNoiseJumpWords (NoiseJumpTable)
};
// host: the jump matrices M^(j * kNoiseSegFills) of one Xorshift128+ lane, columns of (s0 lo, s0 hi, s1 lo, s1 hi)
void NoiseJumpTable(uint32_t* host /* kNoiseSegs * kNoiseJumpWords */);
// host: the 8 lanes' (s0, s1) of Xorshift128Plus(visible, nonvisible, x0, y0) after `fills` fills, through the same
// jump matrices the kernel uses
void NoiseStateAfter(uint32_t visible, uint32_t nonvisible, uint32_t x0, uint32_t y0, uint64_t fills, uint64_t state[16]);
// k_noise_rng + k_noise_emit: random planes, ConvolveNoise, AddNoise on N.xyb, then the output tail of `output_kind`
// into p.out (whole frames only); false for a bad output kind
bool LaunchNoise(const NoiseArgs& N, const FilterParams& p, int output_kind, hipStream_t st);

// Splines (kernels_splines.hip).  The frame is cut into 64 x 16 tiles; tile t draws the segments
// segs[tile_idx[tile_start[t] .. tile_start[t + 1])] in that (increasing) order.
struct SplineSeg {       // SplineSegment (splines.h:95-101) with its spans; 48 bytes
  float cx, cy, inv_sigma, s4i;
  float color[3];
  int32_t y0, y1;        // rows [y0, y1), inside the frame
  int32_t x0, x1;        // columns [x0, x1] = [llround(cx - maximum_distance), llround(cx + maximum_distance)] clipped
  float pad;
};
struct SplineArgs {
  uint32_t xsize, ysize, tiles_x;
  uint32_t num_active;     // tiles with segments (draw-in-place covers only these)
  const float* xyb;        // the filtered frame: 3 planes, ns floats per row, nplane floats apart
  float* xyb_out;          // draw-in-place: where the drawn planes go (same layout; may be xyb)
  uint32_t ns;
  size_t nplane;
  const SplineSeg* segs;
  const uint32_t* tile_start;  // tiles + 1 entries
  const uint32_t* tile_idx;
  const uint32_t* active;      // num_active tile indices
};
// k_splines: in_place = false: draw every tile and write the output tail of `output_kind` into p.out; true: draw the
// active tiles back into S.xyb_out (planar XYB, for the noise launches).  False for a bad output kind.
bool LaunchSplines(const SplineArgs& S, const FilterParams& p, int output_kind, bool in_place, hipStream_t st);

// Patches (kernels_patches.hip).  The frame is cut into 64 x 16 tiles; tile t blends the records
// recs[tile_idx[tile_start[t] .. tile_start[t + 1])] in that (increasing) order -- the order of the dictionary, which
// GetPatchesForRow restores for every row (dec_patch_dictionary.cc:309-312).
enum : uint32_t { kPatchOpReplace = 0, kPatchOpAdd = 1, kPatchOpMul = 2, kPatchOpMulClamp = 3 };
struct PatchRec {          // one placement, 40 bytes
  int32_t x0, y0, x1, y1;  // its rectangle in the frame, [x0, x1) x [y0, y1), clipped to the frame
  const float* src;        // the reference sample that goes to (x0, y0): plane X of its slot
  uint32_t stride, plane;  // of the slot: floats per row, floats between planes
  uint32_t op;             // kPatchOp*: what PerformBlending's colour mode comes to without an alpha channel
  uint32_t pad;
};
struct PatchArgs {
  uint32_t xsize, ysize, tiles_x;
  uint32_t num_active;     // tiles with records (blend-in-place covers only these)
  const float* xyb;        // the filtered frame: 3 planes, ns floats per row, nplane floats apart
  float* xyb_out;          // blend-in-place: where the planes go (same layout; may be xyb)
  uint32_t ns;
  size_t nplane;
  const PatchRec* recs;
  const uint32_t* tile_start;  // tiles + 1 entries
  const uint32_t* tile_idx;
  const uint32_t* active;      // num_active tile indices
};
// records one LDS batch of k_patches holds (a tile with more is blended in several batches)
constexpr uint32_t kPatchBatch = 128;
// k_patches: in_place = false: blend every tile and write the output tail of `output_kind` into p.out; true: blend the
// active tiles back into A.xyb_out (planar XYB, for the launches that follow).  False for a bad output kind.
bool LaunchPatches(const PatchArgs& A, const FilterParams& p, int output_kind, bool in_place, hipStream_t st);

// Blending (kernels_blend.hip).  Canvases are interleaved float RGB, rows padded to four pixels (CanvasStride); a
// thread takes one group of four pixels.
inline size_t CanvasStride(uint32_t xsize) { return 3 * (((size_t)xsize + 3) & ~(size_t)3); }  // floats per row
struct BlendArgs {
  uint32_t W, H;               // the canvas = the image
  int32_t rx0, ry0, rx1, ry1;  // the frame's rectangle clipped to the canvas, [rx0, rx1) x [ry0, ry1) (may be empty)
  uint32_t gx0, gx1, y0, y1;   // what the launch visits: 4-pixel groups [gx0, gx1) of rows [y0, y1)
  uint32_t op;                 // kPatchOp*: what PerformBlending's colour mode comes to without an alpha channel
  uint32_t dst_all;            // write dst in every visited group (else only in those that touch the rectangle)
  const float* fg;             // the staged frame: canvas pixel (x, y) is at fg + (y - fg_y0) * fg_stride + 3 * (x - fg_xa)
  int32_t fg_xa, fg_y0;        // fg_xa = the frame's x origin rounded DOWN to a multiple of 4, fg_y0 its y origin
  size_t fg_stride;            // floats per staged row, a multiple of 12; fg is 16-byte aligned
  const float* src;            // the source canvas (src_stride floats per row), nullptr = zeroes
  size_t src_stride;
  float* dst;                  // the slot saved into (may be src), nullptr = none
  size_t dst_stride;
};
// k_blend: output_kind 0 = the caller's output is not written, else JXLHIP_OUT_LINEAR_RGB_F32 / JXLHIP_OUT_PACKED into
// p.out at canvas coordinates (p.fmt.transfer must be the identity: the samples are encoded already).  False for a bad
// kind, op or region.
bool LaunchBlend(const BlendArgs& A, const FilterParams& p, int output_kind, hipStream_t st);

// Blending on an image with extra channels (kernels_blend_ec.hip).  The colour canvas is BlendArgs' (B.op is not read:
// the colour's BlendMode is color_mode here); every extra channel is a planar float plane whose rows are padded to
// four pixels (EcStride), in the staged frame (x0 mod 4) pixels in like the colour.
inline size_t EcStride(uint32_t xsize) { return ((size_t)xsize + 3) & ~(size_t)3; }  // floats per row
struct BlendEcArgs {
  BlendArgs B;
  uint32_t num_ec;                 // 1..4
  uint32_t has_alpha;              // some extra channel is of type alpha (PerformBlending's has_alpha)
  uint32_t color_mode, color_clamp, color_alpha;  // BlendingInfo of the colour: jxlhip_blend_mode, clamp, alpha_channel
  uint32_t mode[4], clamp[4], alpha[4];           // ... of every extra channel
  uint32_t premul[4];              // ExtraChannelInfo::alpha_associated of channel i (read where i is somebody's alpha channel)
  int32_t out_alpha;               // the channel whose blended plane the packed tail reads back as alpha (p.alpha), -1: none
  const float* fg[4];              // staged planes: canvas pixel (x, y) at fg[i] + (y - B.fg_y0) * fg_stride + (x - B.fg_xa)
  size_t fg_stride;                // floats per staged row, a multiple of 4
  const float* src[4];             // the plane of channel i in ITS source slot (src_stride[i] floats per row), nullptr = zeroes
  size_t src_stride[4];
  float* dst[4];                   // where the blended plane goes: the save slot's plane (may be any src) or the frame's own
  size_t dst_stride;               // plane (jxlhip_frame_extra_read); never nullptr for i < num_ec
};
// k_ec_blend: as LaunchBlend.  With out_alpha >= 0 and a 4-channel packed output p.alpha must be dst[out_alpha]: a thread
// stores its four blended alpha samples and the output stage reads them back.  False for a bad kind, mode or region.
bool LaunchBlendEc(const BlendEcArgs& A, const FilterParams& p, int output_kind, hipStream_t st);

// Tone mapping (kernels_tonemap.hip).  What ToneMappingStage's constructor and Rec2408ToneMapperBase's member
// initialisers compute for a PQ original (stage_tone_mapping.cc:43-63, cms/tone_mapping.h:82-97), in the order
// jxlhip_tone_mapping_constants reports them.
struct ToneMapConstants {
  float to_intensity_target, from_desired_intensity_target;  // 10000 / orig and desired / 10000 for a PQ destination, else 1
  float source_peak, target_peak;                            // source_range_[1], target_range_[1]
  float lum[3];                                              // the destination primaries' luminances
  float pq_mastering_min, pq_mastering_range, inv_pq_mastering_range;
  float min_lum, max_lum, ks, inv_one_minus_ks;
  float normalizer, inv_target_peak;
  float one_minus_ks;                                        // 1 - ks, which P evaluates per call
  float preserve_saturation;                                 // GamutMap's default, 0.1
};
constexpr uint32_t kToneMapConstants = sizeof(ToneMapConstants) / sizeof(float);  // 18
struct ToneMapArgs {
  uint32_t xsize, ysize;  // the frame at output size
  const float* xyb;       // 3 planes, ns floats per row (even, >= xsize rounded up to 2), nplane floats apart (even); 8-byte aligned
  uint32_t ns;
  uint32_t nplane;        // 3 * nplane < 2^32: the kernel indexes with 32 bits
  ToneMapConstants k;
};
// host: the constants for a PQ original of `orig` nits shown at `desired` nits (desired < orig); dest_pq: the
// destination transfer function is PQ
void ToneMapHostConstants(float orig, float desired, const float luminances[3], bool dest_pq, ToneMapConstants* k);
// k_tone_map: XYB -> linear RGB, the tone mapper, the gamut map and the output tail of `output_kind`
// (JXLHIP_OUT_LINEAR_RGB_F32 / JXLHIP_OUT_PACKED) into p.out.  False for another kind or bad geometry.
bool LaunchToneMap(const ToneMapArgs& A, const FilterParams& p, int output_kind, hipStream_t st);

// A regular Modular frame (kernels_modular.hip): three integer planes, the RCT programs the host left, the scale.
struct ModularEmitArgs {
  uint32_t xsize, ysize;
  const void* plane[3];        // device, 16-byte aligned: rows of ns samples of sample_type, channel order as coded
  uint32_t ns;                 // a multiple of 8, >= xsize rounded up to 8
  uint32_t sample_type;        // JXLHIP_MODULAR_I16 / JXLHIP_MODULAR_I32
  uint32_t group_shift, xsg;   // groups of (1 << group_shift) pixels (7 .. 10), xsg of them to the row
  const uint16_t* group_rct;   // device: per group, the first-listed RCT type | the second-listed << 8 (0 = none)
  uint32_t global_rct;         // the same for the whole frame, undone behind the group's
  float factor;                // (float)(1.0 / (2^bits_per_sample - 1))
};
// k_modular_emit: inverse RCTs, int -> float and the output tail of `output_kind` (JXLHIP_OUT_LINEAR_RGB_F32 /
// JXLHIP_OUT_PACKED; p.fmt.transfer is not read: the tail runs with the identity) into p.out.  False for another kind or
// bad geometry / alignment.
bool LaunchModularEmit(const ModularEmitArgs& A, const FilterParams& p, int output_kind, hipStream_t st);
// The same frame with an integer alpha plane and / or ONE colour plane (a grey image): k_modular_planes, the sibling of
// k_modular_emit for the two cases that kernel cannot express.
struct ModularPlanesArgs {
  ModularEmitArgs e;     // num_color == 1: plane[0] alone is read, and every program must be 0 (group_rct may be NULL)
  uint32_t num_color;    // 3, or 1: the sample goes to R, G and B
  const void* alpha;     // device, 16-byte aligned, rows of e.ns samples of e.sample_type; NULL = the opaque value
  float alpha_factor;    // (float)(1.0 / (2^alpha_bits - 1))
};
// Three colour planes without an alpha plane that reaches the output (none, or an output without a fourth channel) are
// k_modular_emit's launch, unchanged; everything else is k_modular_planes.  False as LaunchModularEmit.
bool LaunchModularPlanes(const ModularPlanesArgs& A, const FilterParams& p, int output_kind, hipStream_t st);

// Upsampling (kernels_upsample.hip).  The coded frame is cut into 64 x 16 tiles; every coded pixel gives n x n output
// pixels, each a 25-tap sum over its 5 x 5 neighbourhood clamped to the neighbourhood's range.
struct UpsampleArgs {
  uint32_t cw, ch;         // the coded frame: ceil(xsize / n) x ceil(ysize / n)
  uint32_t xsize, ysize;   // the output (= image) size
  uint32_t n;              // 2, 4, 8
  const float* xyb;        // the filtered coded frame: 3 planes, ns floats per row, nplane floats apart
  uint32_t ns;
  size_t nplane;
  const float* weights;    // device: n * n kernels of 25 taps (UpsampleKernels)
};
// host: the 15 / 55 / 210 coded weights of factor n expanded to its n * n kernels of 25 taps
void UpsampleKernels(uint32_t n, const float* coded, float* kernels /* n * n * 25 */);
// k_upsample: planes_out == nullptr: upsample and write the output tail of `output_kind` into p.out; else upsample
// into planar XYB at output resolution (planes_ns floats per row, planes_nplane apart, for the noise launches).  False
// for a bad output kind, factor or size pair.
bool LaunchUpsample(const UpsampleArgs& U, const FilterParams& p, int output_kind, float* planes_out, uint32_t planes_ns,
                    size_t planes_nplane, hipStream_t st);

// DC-only groups (kernels_dc_upsample.hip): the DC samples of the AC groups whose mask byte is set, upsampled 8x into
// their 8 x 8 tiles of the three block-major XYB planes of f (whole frames only).
// host: the 64 kernels of 25 taps (UpsampleKernels(8, ...)) in the order the kernel loads them: [tap][kernel]
void DcUpsampleWeights(const float* kernels /* 64 * 25 */, float* tap_major /* 25 * 64 */);
// k_dc_upsample8: mask = f.xsg * f.ysg bytes (device), weights = DcUpsampleWeights' table (device).  False for a stripe
// and for planes beyond 32-bit float indices.
bool LaunchDcUpsample8(const DevFrame& f, const uint8_t* mask, const float* weights, hipStream_t st);

// block-major plane rows <-> dense row-major staging
void LaunchZeroU32(uint32_t* p, uint32_t n, hipStream_t st);  // (kernels_tables.hip: a kernel, for captured graphs)
void LaunchRowsCopy(const DevFrame& f, float* dense, int y_first, int nrows, int ncols,
                    size_t dense_stride, size_t dense_plane, int nch, bool to_dense,
                    hipStream_t st);

// a5 / a8 helpers
void LaunchDequantTables(float* table, const jxlhip_quant_encoding* enc_dev, int32_t* status,
                         hipStream_t st);
void LaunchDequantDC(uint32_t xsb, uint32_t ysb, const int32_t* const q[3], float* const dc[3],
                     float* const tmp[3], const float mul_dc[3], float cfl_x, float cfl_b,
                     int smooth, const uint8_t* extra_precision, hipStream_t st);

}  // namespace jxlhip
#endif
