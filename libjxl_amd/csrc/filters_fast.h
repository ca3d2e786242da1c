// filters_fast.h -- k_filters_fast, phase 2 as a register row march: [Gaborish] [EPF1] [EPF2] XYB->RGB (every
// stream below distance ~3, i.e. the BASELINE d1.0 configuration; with three EPF iterations this kernel runs
// the EPF1 + EPF2 + output part behind k_epf0, kernels_epf0.hip), written for the CDNA4 wavefront instead of LDS:
//
//   * one wave = 128 adjacent pixel COLUMNS (each lane owns an aligned PAIR of
//     columns), marching down the rows of its band.  Two pixels per lane turn
//     the filter arithmetic into packed fp32 (v_pk_add/mul/fma_f32: two results
//     per VALU issue) and halve the cross-lane traffic per pixel;
//   * horizontal neighbours inside the pair are free, the two outside it come
//     from the neighbouring LANE through DPP wave_shr/wave_shl (no LDS, no
//     barrier);
//   * vertical neighbours come from a sliding window of rows kept in registers
//     (rings of 8 / 4 slots, slot = row & 7 / & 3, resolved at compile time by
//     unrolling the row loop 8x);
//   * input rows are prefetched in bursts of four rows = whole 128-byte lines of
//     the block-major planes (one 8-byte load per lane, row and channel; the row
//     base is scalar), output rows leave as 24-byte non-temporal RGB stores.
//
// The kernel is written against its VALU ISSUE count (SQ counters of round 1: 218 VALU instructions
// per row step and wave, the SIMDs' VALU ports 57 % busy at 2 waves per SIMD -- issue-bound, not
// latency-bound).  Round 2 brought the row step to ~118 VALU instructions (tools/isa_loops.py on the
// -S listing): channel-summed difference images before the plus-shaped sums, weights through the
// packed FMA's [0, 1] output clamp, XYB -> RGB on pixel pairs with per-half matrix rows picked by
// op_sel, DPP operands folded into VOP2 instructions (v_add/v_sub/v_fmac ..._dpp), one 8-slot input
// ring instead of prefetch + input rings (no register copies between rings), SGPR-based addressing
// for every load and store, a running output-row pointer, part of the wave-uniform constants kept in
// VGPRs (the loop wanted more than 102 SGPRs).  Measured on MI355X (8K d1.0, JXLHIP_DEBUG
// ablations): arithmetic alone 135 -> 94 us; with the plane reads 127-137 us; whole kernel 215-235 us
// (866 MB: 3.9 TB/s, where a device copy moves 4.8-5.0) -- what remains is the block-major read
// path and the mixed read / write stream, not arithmetic.  Tried and measured
// without gain: 3 workgroups per CU, deeper single-row prefetch (see kAhead), routing the RGB row
// through LDS so that every store instruction writes whole 64-byte lines.
//
// EPF1 (lib/jxl/render_pipeline/stage_epf.cc:225-367) is evaluated through an
// regrouping of the reference's sums: with Du(x,y) = sum_c scale_c |p_c(x,y-1) - p_c(x,y)|
// and Dl(x,y) = sum_c scale_c |p_c(x-1,y) - p_c(x,y)|, the four SADs of pixel (x,y) are the
// plus-shaped sums  PV(x,y), PH(x,y), PH(x+1,y), PV(x,y+1)  of Du / Dl -- the reference's 15
// non-negative terms per SAD in another association (per channel first there, per position first
// here), each plus-sum computed once per pixel instead of four times.
//
// Border rule (simple_render_pipeline.cc:129-164): stages read their input
// mirrored at the true image edge.  Gaborish of the mirrored input IS the
// mirrored Gaborish output (symmetric kernel, commutative pair sums), so halo
// lanes/rows outside the image simply run on mirrored input; this kernel is
// only used when no stage follows an EPF stage, where that identity is all
// that is needed.  Where EPF2 follows EPF1 the one out-of-image column / row it reads is the mirror = the edge pixel
// itself (Lane::fix_*).  Frames narrower or lower than 16 px use the generic kernel (kernels_filters.hip).
//
// The kernel template and its launch live here; the translation units kernels_filters_fast*.hip instantiate it, each
// for the output forms it is named for (JXLHIP_FIXED_FORMATS below says which unit compiles which fixed format).
#ifndef JXLHIP_FILTERS_FAST_H_
#define JXLHIP_FILTERS_FAST_H_

#include <stdlib.h>

#include "env_switches.h"
#include "filters_march.h"

namespace jxlhip {

// One launch entry per translation unit besides kernels_filters_fast.hip (LaunchFiltersFast, kernels.h: the float and
// planar outputs): the general packed format (in two units; LaunchFastGeneral takes every stage list and passes on
// those with EPF2), and the fixed formats of each FastUnit.  The fixed ones return false when p.fmt is none of theirs;
// all of them when (gab, epf_iters) is not a stage list of the march.
bool LaunchFastGeneral(const DevFrame& f, const FilterParams& p, int gab, int epf_iters, hipStream_t st);
bool LaunchFastGeneralEpf2(const DevFrame& f, const FilterParams& p, int gab, hipStream_t st);
bool LaunchFastFixedInt(const DevFrame& f, const FilterParams& p, int gab, int epf_iters, hipStream_t st);
bool LaunchFastFixedBe16(const DevFrame& f, const FilterParams& p, int gab, int epf_iters, hipStream_t st);
bool LaunchFastFixedFp(const DevFrame& f, const FilterParams& p, int gab, int epf_iters, hipStream_t st);

namespace {

template <int GAB, int EPF>
struct FastGeom {
  static constexpr int HX = GAB + (EPF >= 1 ? 2 : 0) + (EPF == 2 ? 1 : 0);  // halo rows / columns each side
  static constexpr int HXP = (HX + 1) & ~1;       // in whole column pairs
  static constexpr int USE = 128 - 2 * HXP;       // output columns per wave
};

template <int GAB, int EPF, int OUTK, int FMT, bool EDGE, int SRC>
__device__ __forceinline__ void March(const DevFrame& f, const FilterParams& P, Lane& L, int y_begin,
                                      int y_end) {
  constexpr int HX = FastGeom<GAB, EPF>::HX;
  const int H = (int)f.ysize;
  // rows: input rows r = y_begin - HX .. y_end + HX - 1; the pipeline emits
  // row r - HX at step r.
  const int r_first = y_begin - HX;
  const int r_last = y_end + HX - 1;
  // the prefetcher runs kAhead rows ahead: clamp to the last row this
  // context holds (plane rows cover [y0 - halo, y1_padded + halo))
  const int plane_last = f.plane_y0 + (int)f.plane_tile_rows * 8 - 1;
  int prefetch_last_row = r_last;
  // mirrored rows always fall inside the plane; direct rows must too
  if (prefetch_last_row > plane_last && prefetch_last_row < H) prefetch_last_row = plane_last;
  State s;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    // rows r_first .. r_first + kAhead - 1 are in flight when the first step runs; the slots of the
    // (not yet existing) rows above them start as zero like the other rings
    const bool fetch = k < kAhead;
    int pr = r_first + k;
    pr = pr > prefetch_last_row ? prefetch_last_row : pr;
    const uint32_t off = SrcRowOffset<SRC>(f, Mirror1(pr, H));
    LaneOffset(L.byte_off);
#pragma unroll
    for (int c = 0; c < 3; c++) {
      if (fetch) s.x[c][k] = LoadPair<EDGE>((const char*)f.xyb[c] + off, L);
      else s.x[c][k] = v2f{0.0f, 0.0f};
    }
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
      s.hs[c][k] = v2f{0.0f, 0.0f};
      s.g[c][k] = v2f{0.0f, 0.0f};
      s.e[c][k] = v2f{0.0f, 0.0f};
    }
    s.du[k] = v2f{0.0f, 0.0f};
    s.dl[k] = v2f{0.0f, 0.0f};
    s.pv[k] = v2f{0.0f, 0.0f};
    s.ph[k] = v2f{0.0f, 0.0f};
    s.dv[k] = v2f{0.0f, 0.0f};
  }
  float inv_sigma_blk = -1.0f, inv_sigma_blk2 = -1.0f;
  const XybConsts KC = MakeXybConsts(P);
  // output row of step r is row r - HX: a running pointer instead of a 64-bit product per row
  const size_t out_row_bytes = OUTK == JXLHIP_OUT_XYB_PLANAR ? P.out_stride * 4 : P.out_stride;
  char* out_row = (char*)P.out + (ptrdiff_t)(r_first - HX - (int)f.y0) * (ptrdiff_t)out_row_bytes;
#define JXLHIP_STEP(K)                                                                                         \
  Step<GAB, EPF, OUTK, FMT, K, EDGE, SRC>(s, r + K, f, P, L, prefetch_last_row, y_begin, y_end,             \
                                               inv_sigma_blk, inv_sigma_blk2, out_row, KC);                  \
  out_row += out_row_bytes
  for (int r = r_first; r <= r_last; r += 8) {
    JXLHIP_STEP(0);
    JXLHIP_STEP(1);
    JXLHIP_STEP(2);
    JXLHIP_STEP(3);
    if (r + 4 > r_last) break;
    JXLHIP_STEP(4);
    JXLHIP_STEP(5);
    JXLHIP_STEP(6);
    JXLHIP_STEP(7);
  }
#undef JXLHIP_STEP
}

template <int GAB, int EPF, int OUTK, int FMT, int SRC = SRC_PLANES>
__global__ __launch_bounds__(256, EPF == 2 ? 2 : 3) void k_filters_fast(DevFrame f, FilterParams P, int RH) {
  using G = FastGeom<GAB, EPF>;
  constexpr int HXP = G::HXP, USE = G::USE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float __attribute__((address_space(3)))* dither_lds = nullptr;
  if constexpr (OUTK == JXLHIP_OUT_PACKED) {  // before any wave leaves: whole-workgroup barrier
    __shared__ float s_dither[1024];
    if (P.fmt.sample_type == JXLHIP_SAMPLE_U8) {  // uniform
      for (int i = threadIdx.x; i < 1024; i += 256) s_dither[i] = P.dither[i];
      __syncthreads();
    }
    dither_lds = (const float __attribute__((address_space(3)))*)s_dither;
  }
  const int strip = blockIdx.x * 4 + wave;
  const int W = (int)f.xsize;
  const int x_first = strip * USE;  // first output column of the wave (even)
  if (x_first >= W) return;
  const int y_begin = (int)f.fy0 + blockIdx.y * RH;
  const int y_end = min(y_begin + RH, (int)f.fy1);
  if (y_begin >= y_end) return;
  Lane L;
  L.gx = x_first - HXP + 2 * lane;
  L.dither = dither_lds;
  // the lane's two columns, mirrored into the image, always fall into one
  // aligned pair of plane columns (the planes are allocated in whole 8x8
  // tiles, so column W exists when W is odd)
  const int m0 = MirrorF(L.gx, W), m1 = MirrorF(L.gx + 1, W);
  const int base = m0 & ~1;
  L.sel0 = m0 & 1;
  L.sel1 = m1 & 1;
  L.byte_off = SRC == SRC_LINEAR ? (uint32_t)base * 4u : ((uint32_t)(base >> 3) * 64u + (uint32_t)(base & 7)) * 4u;
  const bool edge = x_first - HXP < 0 || x_first - HXP + 128 > W;  // wave-uniform
  const bool lane_in = lane >= HXP / 2 && lane < 64 - HXP / 2;
  L.out0 = lane_in && L.gx < W;
  L.out1 = lane_in && L.gx + 1 < W;
  const int gxc = L.gx < 0 ? 0 : (L.gx >= W ? W - 1 : L.gx);
  L.sx4 = (uint32_t)(gxc >> 3) * 4u;
  L.out_off = (uint32_t)(L.gx < 0 ? 0 : L.gx) * (OUTK == JXLHIP_OUT_LINEAR_RGB_F32 ? 12u : 4u);
  const int ix = gxc & 7;
  // columns gx, gx+1 (gx even inside the image): only gx can be a block's
  // first column and only gx+1 its last
  L.mul = v2f{ix == 0 ? P.bsm[1] : P.sm[1], ix == 6 ? P.bsm[1] : P.sm[1]};
  L.mul2 = v2f{ix == 0 ? P.bsm[2] : P.sm[2], ix == 6 ? P.bsm[2] : P.sm[2]};
  L.fix_left = L.gx == -2;
  L.fix_right_even = L.gx == W;       // only reached when W is even (gx is even)
  L.fix_right_odd = L.gx == W - 1;    // W odd
  if (edge) March<GAB, EPF, OUTK, FMT, true, SRC>(f, P, L, y_begin, y_end);
  else March<GAB, EPF, OUTK, FMT, false, SRC>(f, P, L, y_begin, y_end);
}

// Rows per wave: ChunkRows (kernels.h) over every height from 16 to 512 with two workgroups resident per compute unit;
// a wave costs RH + 2 * HX row steps plus ~6 of prologue.  JXLHIP_FILTER_RH (sampled when a context is created,
// env_switches.h) overrides, here and in LaunchEpf0 (kernels_epf0.hip): at three EPF iterations both marches are cut
// at the forced height.
template <int GAB, int EPF, int OUTK, int FMT = -1>
void LaunchFastT(const DevFrame& f, const FilterParams& p, hipStream_t st) {
  using G = FastGeom<GAB, EPF>;
  const unsigned strips = (f.xsize + G::USE - 1) / G::USE;
  const unsigned wgx = (strips + 3) / 4;
  const int forced = jxlhip_env::Get().filter_rh.load(std::memory_order_relaxed);
  const int RH = forced > 0 ? forced : ChunkRows(wgx, f.fy1 - f.fy0, DeviceCus() * 2u, 16, 512, 1, 2 * G::HX + 6);
  const dim3 grid(wgx, (f.fy1 - f.fy0 + RH - 1) / RH);
  if constexpr (GAB == 0 && EPF == 2) {
    if (f.linear_stride) {  // the input is k_epf0's row-major plane set
      hipLaunchKernelGGL((k_filters_fast<GAB, EPF, OUTK, FMT, SRC_LINEAR>), grid, dim3(256), 0, st, f, p, RH);
      return;
    }
  }
  hipLaunchKernelGGL((k_filters_fast<GAB, EPF, OUTK, FMT>), grid, dim3(256), 0, st, f, p, RH);
}

// Packed formats with a kernel of their own (the format fixed at compile time): what djxl writes most -- 8-bit sRGB
// for PNG / PPM, 16-bit sRGB -- 16-bit sRGB RGBA and the BIG-ENDIAN 16-bit forms (PNG / PNM are big-endian), float
// sRGB / linear (PFM, NPY, API clients), half-float RGBA (HDR canvases), 16-bit PQ (HDR PNG).  Everything else takes
// the kernel that reads the format from its launch parameters -- at twice the time (per-sample wave-uniform branches,
// 256 VGPRs and spills; profiles/r03_packed_fixed_formats.txt).
// X(transfer, sample type, channels, swap endianness, unit): the ONE list -- FastFixedFormat, the dispatch and the
// translation unit that compiles a format's kernels (kernels_filters_fast_<unit>.hip; six stage lists plus the
// row-major-source form each, the units balanced by compile time) all follow from it.
enum FastUnit : int { kFastInt, kFastBe16, kFastFp };
#define JXLHIP_FIXED_FORMATS(X)                                  \
  X(JXLHIP_TF_SRGB, JXLHIP_SAMPLE_U8, 3, 0, kFastInt)            \
  X(JXLHIP_TF_SRGB, JXLHIP_SAMPLE_U8, 4, 0, kFastInt)            \
  X(JXLHIP_TF_SRGB, JXLHIP_SAMPLE_U16, 3, 0, kFastInt)           \
  X(JXLHIP_TF_SRGB, JXLHIP_SAMPLE_U16, 4, 0, kFastInt)           \
  X(JXLHIP_TF_SRGB, JXLHIP_SAMPLE_U16, 3, 1, kFastBe16)          \
  X(JXLHIP_TF_SRGB, JXLHIP_SAMPLE_U16, 4, 1, kFastBe16)          \
  X(JXLHIP_TF_PQ, JXLHIP_SAMPLE_U16, 3, 1, kFastBe16)            \
  X(JXLHIP_TF_PQ, JXLHIP_SAMPLE_U16, 4, 1, kFastBe16)            \
  X(JXLHIP_TF_SRGB, JXLHIP_SAMPLE_F32, 3, 0, kFastFp)            \
  X(JXLHIP_TF_SRGB, JXLHIP_SAMPLE_F32, 4, 0, kFastFp)            \
  X(JXLHIP_TF_LINEAR, JXLHIP_SAMPLE_F32, 4, 0, kFastFp)          \
  X(JXLHIP_TF_SRGB, JXLHIP_SAMPLE_F16, 4, 0, kFastFp)            \
  X(JXLHIP_TF_LINEAR, JXLHIP_SAMPLE_F16, 4, 0, kFastFp)

inline bool IsFormat(const jxlhip_output_format& o, int tf, int st, int nc, int sw) {
  return (int)o.transfer == tf && (int)o.sample_type == st && (int)o.num_channels == nc && (o.swap_endianness != 0) == (sw != 0);
}

// the six stage lists (gab, epf_iters) the march is instantiated for; (0, 0), no loop filter: the same row march is a
// streaming block-major -> RGB conversion
#define JXLHIP_STAGE_LISTS(X) X(0, 0) X(1, 0) X(0, 1) X(1, 1) X(0, 2) X(1, 2)

// unit UNIT's fixed formats: launches and returns true when p.fmt is one of them
template <int UNIT, int GAB, int EPF>
bool LaunchFixedT(const DevFrame& f, const FilterParams& p, hipStream_t st) {
#define JXLHIP_TRY(TF, ST, NC, SW, U)                                               \
  if constexpr (U == UNIT) {                                                        \
    if (IsFormat(p.fmt, TF, ST, NC, SW)) {                                          \
      LaunchFastT<GAB, EPF, JXLHIP_OUT_PACKED, FormatId(TF, ST, NC, SW)>(f, p, st); \
      return true;                                                                  \
    }                                                                               \
  }
  JXLHIP_FIXED_FORMATS(JXLHIP_TRY)
#undef JXLHIP_TRY
  return false;
}
template <int UNIT>
bool LaunchFixedUnit(const DevFrame& f, const FilterParams& p, int gab, int epf_iters, hipStream_t st) {
#define JXLHIP_FAST(G, E) \
  if (gab == G && epf_iters == E) return LaunchFixedT<UNIT, G, E>(f, p, st);
  JXLHIP_STAGE_LISTS(JXLHIP_FAST)
#undef JXLHIP_FAST
  return false;
}

}  // namespace
}  // namespace jxlhip
#endif  // JXLHIP_FILTERS_FAST_H_
