// kernels_fused.hip -- the loop-filter row march fed straight from the coefficient stream.
//
// Round 1's two phases move the frame's XYB planes through HBM twice (12 B/px written by the
// transform kernels, 12 B/px read by the filter kernel: 0.8 of the 1.5 GB an 8K frame moved).  Here
// the filter wave decodes the varblocks of its own 128-column window itself, one block row (8 pixel
// rows) at a time, into a 12 KB per-wave LDS slab and marches over the slab -- those pixels never
// exist in HBM.  What a wave can decode alone without holding more than 8 rows is the single-block
// class that dominates a d1.0 frame, DCT8 (45 % of the area, row-per-lane: 8 lanes per block,
// register transposes, as k_transform_8); every other varblock is still decoded by the class-sorted
// kernels of phase 1 into the block-major planes, and the wave copies those cells' tiles into its
// slab with LDS-DMA loads (global_load_lds_dword: HBM -> LDS without passing through registers).
//
//   wave window : 16 whole block columns [112 k - 8, 112 k + 120): 8 halo columns either side of the
//                 112 output columns (the march needs <= 4), so that the window is made of whole
//                 varblock cells; neighbouring windows share two block columns, decoded by both
//   per group of 8 rows (r = 0 mod 8):
//     Fill      : cell info of the 16 cells (k_prepare left coefficient offset + quant / CfL word of
//                 every DCT8 block in DevFrame::cell_info; other cells say "from the planes");
//                 LDS-DMA of the plane cells (24 instructions per 8 cells); DCT8 cells in steps of 8
//                 blocks: dequant + CfL + IDCT x transpose x IDCT, two ds_write_b128 per channel
//     8 x Step  : the row march of filters_march.h with SRC_LDS (ds_read_b64 per channel and row)
//   mirroring   : columns through the lane's (mirrored) slab address; rows by the slab row index
//                 (a group of 8 rows always lies in one block row: frames with 1..3 rows in their
//                 last block row go to the two-phase path)
//
// The reference semantics are those of the two-phase path (simple_render_pipeline.cc:129-164,
// loop_filter.h:26-29); the parity tests run both.
#include "fused_pc.h"

namespace jxlhip {

namespace {

// INTERIOR (wave-uniform, chosen by the kernel): the chunk starts and ends on block rows and touches neither the frame's
// top nor its bottom -- every row step then knows its place in the block row, whether it writes, and that no row is a
// mirror row at COMPILE time (filters_march.h, StepKnown): the scalar bookkeeping of the generic step, a third of the
// marching wave's instruction issues, is gone.  The first whole group is peeled: its first HX steps still complete rows
// of the chunk above (not written here), every later step of the chunk writes.
template <int GAB, int EPF, int OUTK, int FMT, bool EDGE, bool INTERIOR, int NB = 2>
__device__ __forceinline__ void MarchPC(const DevFrame& f, const FilterParams& P, Lane& L, StripLdsT<NB>* w, int bc0,
                                        int y_begin, int y_end) {
  constexpr int HX = MarchGeom<GAB, EPF>::HX;
  constexpr int KI = INTERIOR ? (int)kStepInterior : 0;                  // a step that writes nothing
  constexpr int KE = INTERIOR ? (int)(kStepInterior | kStepEmit) : 0;   // a step that writes its row
  constexpr int KF = INTERIOR ? (int)kStepFirst : 0;
  const int H = (int)f.ysize;
  const int r_first = HX ? y_begin - 8 : y_begin;
  const int r_last = y_end + HX - 1;
  const int nb_last = (H - 1) >> 3;
  const int G = PcGroups<HX>(y_begin, y_end);
  State s;
#pragma unroll
  for (int k = 0; k < 8; k++)
#pragma unroll
    for (int c = 0; c < 3; c++) s.x[c][k] = v2f{0.0f, 0.0f};
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
  float sigma_last = -1.0f;
  const XybConsts KC = MakeXybConsts(P);
  const size_t out_row_bytes = OUTK == JXLHIP_OUT_XYB_PLANAR ? P.out_stride * 4 : P.out_stride;
  char* out_row = (char*)P.out + (ptrdiff_t)(r_first - HX - (int)f.y0) * (ptrdiff_t)out_row_bytes;
  const float __attribute__((address_space(3)))* const slab0 = L.slab;
  // the lane's cell inside the window, for the inv_sigma row the producer leaves in LDS
  const LdsF* sig0 = (const LdsF*)w->sigma[0] + ((int)(L.sx4 >> 2) - bc0);
  int i = 0;
  auto enter_group = [&](int g) -> float {  // after the barrier that publishes buffer g % NB
    const int b = NB == 2 ? (g & 1) : g % NB;
    L.slab = slab0 + b * (3 * kSlabPlaneFloats);
    return EPF ? sig0[b * 16] : 0.0f;
  };
#define JXLHIP_PSTEPK(K, KN)                                                                                          \
  Step<GAB, EPF, OUTK, FMT, K, EDGE, SRC_LDS, KN>(s, r + K, f, P, L, 0, y_begin, y_end, inv_sigma_blk,         \
                                                  inv_sigma_blk2, out_row, KC, slab_y0, sigma_pre, sigma_prev);       \
  out_row += out_row_bytes
// a whole group of 8 rows starting at image row r (a multiple of 8): steps 0 .. HX-1 take KLOW, the others KHIGH
#define JXLHIP_PGROUP(KLOW, KHIGH)                                                       \
  {                                                                                      \
    const int slab_y0 = GroupBlockRow(r, nb_last) * 8;                                   \
    const float sigma_prev = sigma_last;                                                 \
    const float sigma_pre = enter_group(i);                                              \
    sigma_last = sigma_pre;                                                              \
    {                                                                                    \
      const int row0 = INTERIOR ? 0 : Mirror1(r, H) - slab_y0;                           \
      _Pragma("unroll") for (int c = 0; c < 3; c++) s.x[c][0] = LdsPair<EDGE>(L, c, row0); \
    }                                                                                    \
    JXLHIP_PSTEPK(0, (0 < HX ? (KLOW) : (KHIGH)));                                       \
    JXLHIP_PSTEPK(1, (1 < HX ? (KLOW) : (KHIGH)));                                       \
    JXLHIP_PSTEPK(2, (2 < HX ? (KLOW) : (KHIGH)));                                       \
    JXLHIP_PSTEPK(3, (3 < HX ? (KLOW) : (KHIGH)));                                       \
    JXLHIP_PSTEPK(4, (KHIGH));                                                           \
    JXLHIP_PSTEPK(5, (KHIGH));                                                           \
    JXLHIP_PSTEPK(6, (KHIGH));                                                           \
    JXLHIP_PSTEPK(7, (KHIGH));                                                           \
    i++;                                                                                 \
  }
  PcBarrierMarch();  // fill(0)
  if constexpr (HX > 0) {  // the last HX rows of the block row above
    const int r = r_first;
    const int slab_y0 = GroupBlockRow(r, nb_last) * 8;
    const float sigma_prev = sigma_last;
    const float sigma_pre = enter_group(i);
    sigma_last = sigma_pre;
    {
      const int row0 = INTERIOR ? 8 - HX : Mirror1(r + 8 - HX, H) - slab_y0;
#pragma unroll
      for (int c = 0; c < 3; c++) s.x[c][8 - HX] = LdsPair<EDGE>(L, c, row0);
    }
    out_row += (8 - HX) * out_row_bytes;
    if constexpr (HX >= 4) { JXLHIP_PSTEPK(4, KI); }
    if constexpr (HX >= 3) { JXLHIP_PSTEPK(5, KI); }
    if constexpr (HX >= 2) { JXLHIP_PSTEPK(6, KI); }
    JXLHIP_PSTEPK(7, KI);
    i++;
    PcBarrierMarch();  // a whole group always follows
  }
  int r = HX ? y_begin : r_first;
  if constexpr (INTERIOR) {
    JXLHIP_PGROUP(KI | KF, KE | KF)
    if (i < G) PcBarrierMarch();
    for (r += 8; r < y_end; r += 8) {
      JXLHIP_PGROUP(KE, KE)
      if (i < G) PcBarrierMarch();
    }
  } else {
    for (; r_last - r >= HX; r += 8) {
      JXLHIP_PGROUP(0, 0)
      if (i < G) PcBarrierMarch();
    }
  }
  if (HX > 0 && (INTERIOR || r <= r_last)) {  // the first HX rows of the block row below
    const int slab_y0 = GroupBlockRow(r, nb_last) * 8;
    const float sigma_prev = sigma_last;
    const float sigma_pre = enter_group(i);
    sigma_last = sigma_pre;
    {
      const int row0 = INTERIOR ? 0 : Mirror1(r, H) - slab_y0;
#pragma unroll
      for (int c = 0; c < 3; c++) s.x[c][0] = LdsPair<EDGE>(L, c, row0);
    }
    JXLHIP_PSTEPK(0, KE);
    if constexpr (HX >= 2) { JXLHIP_PSTEPK(1, KE); }
    if constexpr (HX >= 3) { JXLHIP_PSTEPK(2, KE); }
    if constexpr (HX >= 4) { JXLHIP_PSTEPK(3, KE); }
  }
#undef JXLHIP_PGROUP
#undef JXLHIP_PSTEPK
}

// blockIdx.x is dispatched round-robin over the 8 XCDs: logical workgroup = (xcd, slot) -> xcd * per + slot, so
// that an XCD's L2 sees neighbouring windows of the same rows (they share two block columns of coefficients and
// plane tiles); the grid is padded to a multiple of 8
template <int GAB, int EPF, int OUTK, int FMT, typename CT>
__global__ __launch_bounds__(128, kPcWaves) void k_fused_pc(DevFrame f, FilterParams P, int RH, int strips, int nwg) {
  __shared__ StripLds lds;
  const int lane = threadIdx.x & 63;
  const int wave = (int)(threadIdx.x >> 6);  // 0 marches, 1 produces
  const float __attribute__((address_space(3)))* dither_lds = nullptr;
  if constexpr (OUTK == JXLHIP_OUT_PACKED) {
    __shared__ float s_dither[1024];
    if (P.fmt.sample_type == JXLHIP_SAMPLE_U8) {  // uniform
      for (int i = threadIdx.x; i < 1024; i += 128) s_dither[i] = P.dither[i];
      __syncthreads();
    }
    dither_lds = (const float __attribute__((address_space(3)))*)s_dither;
  }
  const int per = (int)gridDim.x >> 3;
  const int logical = ((int)blockIdx.x & 7) * per + ((int)blockIdx.x >> 3);
  if (logical >= nwg) return;
  const int strip = logical % strips, chunk = logical / strips;
  const int W = (int)f.xsize;
  const int x_first = strip * kFusedUse;
  const int y_begin = (int)f.fy0 + chunk * RH;
  const int y_end = min(y_begin + RH, (int)f.fy1);
  if (x_first >= W || y_begin >= y_end) return;  // (both waves)
  const int x0 = x_first - kFusedHalo;
  const int bc0 = x0 >> 3;
  const FrameArgs fa = (FrameArgs)__builtin_amdgcn_kernarg_segment_ptr();
  if (wave == 1) {
    __builtin_amdgcn_s_setprio(kProducerPrio);
    if constexpr (sizeof(CT) == 2) ProducePC2<MarchGeom<GAB, EPF>::HX>(fa, &lds, bc0, y_begin, y_end, ((int)f.ysize - 1) >> 3);
    else
      ProducePC<MarchGeom<GAB, EPF>::HX, CT>(fa, &lds, bc0, y_begin, y_end, ((int)f.ysize - 1) >> 3);
    return;
  }
  Lane L;
  L.gx = x0 + 2 * lane;
  L.dither = dither_lds;
  const int m0 = MirrorF(L.gx, W), m1 = MirrorF(L.gx + 1, W);
  int base = (m0 & ~1) - x0;
  base = base < 0 ? 0 : (base > kSlabCols - 2 ? kSlabCols - 2 : base);
  L.sel0 = m0 & 1;
  L.sel1 = m1 & 1;
  L.byte_off = 0;
  L.slab = (const float __attribute__((address_space(3)))*)lds.slab[0] + base;
  const bool edge = x0 < 0 || x0 + kSlabCols > W;
  const bool lane_in = lane >= kFusedHalo / 2 && lane < 64 - kFusedHalo / 2;
  L.out0 = lane_in && L.gx < W;
  L.out1 = lane_in && L.gx + 1 < W;
  const int gxc = L.gx < 0 ? 0 : (L.gx >= W ? W - 1 : L.gx);
  L.sx4 = (uint32_t)(gxc >> 3) * 4u;
  L.out_off = (uint32_t)(L.gx < 0 ? 0 : L.gx) * (OUTK == JXLHIP_OUT_LINEAR_RGB_F32 ? 12u : 4u);
  const int ix = gxc & 7;
  L.mul = v2f{ix == 0 ? P.bsm[1] : P.sm[1], ix == 6 ? P.bsm[1] : P.sm[1]};
  L.mul2 = v2f{ix == 0 ? P.bsm[2] : P.sm[2], ix == 6 ? P.bsm[2] : P.sm[2]};
  L.fix_left = L.gx == -2;
  L.fix_right_even = L.gx == W;
  L.fix_right_odd = L.gx == W - 1;
  // a chunk of whole block rows that needs no mirror row: the march with its row bookkeeping resolved at compile time
  const bool interior = (y_begin & 7) == 0 && ((y_end - y_begin) & 7) == 0 && y_begin >= 8 &&
                        y_end + 8 <= (int)f.ysize;
  if (interior) {
    if (edge) MarchPC<GAB, EPF, OUTK, FMT, true, true>(f, P, L, &lds, bc0, y_begin, y_end);
    else MarchPC<GAB, EPF, OUTK, FMT, false, true>(f, P, L, &lds, bc0, y_begin, y_end);
  } else {
    if (edge) MarchPC<GAB, EPF, OUTK, FMT, true, false>(f, P, L, &lds, bc0, y_begin, y_end);
    else MarchPC<GAB, EPF, OUTK, FMT, false, false>(f, P, L, &lds, bc0, y_begin, y_end);
  }
}

template <int GAB, int EPF, int OUTK, int FMT = -1>
void LaunchFusedPcT(const DevFrame& f, const FilterParams& p, hipStream_t st) {
  const unsigned strips = (f.xsize + kFusedUse - 1) / kFusedUse;
  const int RH = FusedRowsPC(strips, f.fy1 - f.fy0);
  const unsigned nwg = strips * ((f.fy1 - f.fy0 + RH - 1) / RH);
  const dim3 grid((nwg + 7) & ~7u);
  if (f.coeff_type == JXLHIP_COEFF_I16)
    hipLaunchKernelGGL((k_fused_pc<GAB, EPF, OUTK, FMT, int16_t>), grid, dim3(128), 0, st, f, p, RH, (int)strips, (int)nwg);
  else
    hipLaunchKernelGGL((k_fused_pc<GAB, EPF, OUTK, FMT, int32_t>), grid, dim3(128), 0, st, f, p, RH, (int)strips, (int)nwg);
}

}  // namespace

// Frames the fused kernel takes (decided before k_prepare: it routes the DCT8 blocks).
bool FusedSupported(const DevFrame& f, int gab, int epf_iters, int output_kind) {
  (void)gab;
  if (epf_iters > 2) return false;                 // EPF0: k_epf0 + the EPF1 + EPF2 march (kernels_epf0.hip)
  // Packed outputs stay two-phase: their emit code doubles the march's instruction count, and k_fused_pc has the march
  // on half of a workgroup's waves (8K d1.0: sRGB RGBA8 0.50 ms fused against 0.42 ms two-phase,
  // profiles/r03_packed_paths.txt).  (Rounds 2-5 also shipped a single-wave fused kernel for the general packed
  // formats; removed in round 6 with the other never-default forms.)
  if (output_kind == JXLHIP_OUT_PACKED) return false;
  if (f.xsize < 16 || f.ysize < 16) return false;  // multiply mirrored columns / rows
  const uint32_t tail = f.ysize & 7u;
  if (tail >= 1 && tail <= 3) return false;        // mirror rows below the frame leave the last block row
  if ((f.fy0 & 7u) != 0) return false;
  if ((uint64_t)f.plane_tile_rows * f.tile_stride * 256u >= (1ull << 32)) return false;
  // the producing wave addresses coefficients as buffer base + 32-bit byte offset (PcIssue)
  if ((uint64_t)f.xsg * f.ysg * f.coef_stride64 * 64u * (f.coeff_type == JXLHIP_COEFF_I16 ? 2u : 4u) >= (1ull << 32)) return false;
  return true;
}

bool LaunchFused(const DevFrame& f, const FilterParams& p, int gab, int epf_iters, int output_kind, hipStream_t st) {
  if (!FusedSupported(f, gab, epf_iters, output_kind)) return false;
#define JXLHIP_FUSED_PCX(G, E)                                    \
  if (gab == G && epf_iters == E) {                               \
    if (output_kind == 0) LaunchFusedPcT<G, E, 0>(f, p, st);      \
    else LaunchFusedPcT<G, E, 1>(f, p, st);                       \
    return true;                                                  \
  }
  JXLHIP_FUSED_PCX(1, 1)
  JXLHIP_FUSED_PCX(0, 0)
  JXLHIP_FUSED_PCX(0, 1)
  JXLHIP_FUSED_PCX(1, 0)
  JXLHIP_FUSED_PCX(0, 2)
  JXLHIP_FUSED_PCX(1, 2)
#undef JXLHIP_FUSED_PCX
  return false;
}

}  // namespace jxlhip
