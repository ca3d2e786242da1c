// fused_pc.h -- what the producer / consumer fused kernels share: k_fused_pc (kernels_fused.hip) and k_fused_pc0
// (kernels_fused_epf0.hip, the epf_iters = 3 form).  The window and slab geometry, the double-buffered LDS slab, the
// producing wave (ProducePC / ProducePC2), the barriers that join it with the marching wave, and the chunk height of
// a launch.  See kernels_fused.hip for the design.
#ifndef JXLHIP_FUSED_PC_H_
#define JXLHIP_FUSED_PC_H_

#include <stdlib.h>

#include <type_traits>

#include "blocks_common.h"
#include "env_switches.h"
#include "filters_march.h"

// The producing wave runs at a raised wave priority (s_setprio): the marching wave waits for it at every block row's
// barrier, and at equal priority the SIMD's arbiter lets the (longer, never-waiting) marches of OTHER windows take the
// issue slots a producer needs to finish its block row (8K d1.0: k_fused_pc 203.5 -> 196 us, profiles/r04_setprio.txt).
static constexpr int kProducerPrio = 3;

namespace jxlhip {

namespace {

typedef __attribute__((address_space(3))) float LdsF;
typedef __attribute__((address_space(3))) uint32_t LdsU;

static constexpr int kFusedHalo = 8;                      // window columns in front of the first output column
static constexpr int kFusedUse = kSlabCols - 2 * kFusedHalo;  // 112 output columns per wave

// The fill steps read their frame parameters (coefficient / DC / table / plane pointers, quantizer
// scalars) from the KERNARG SEGMENT at the point of use instead of keeping them in SGPRs for the whole
// march: the march alone wants the ~100 SGPRs a wave has, and what does not fit is spilled to VGPR
// lanes and read back with v_readlane_b32 -- 14 VALU issues per row step in the first version of this
// kernel.  (DevFrame is the kernel's first by-value argument: offset 0 of the segment.)  The pointer
// is laundered through an empty asm so that the loads are not hoisted out of the row loop again.
typedef const DevFrame __attribute__((address_space(4))) * FrameArgs;
__device__ __forceinline__ FrameArgs Fresh(FrameArgs q) {
  asm volatile("" : "+s"(q));
  return q;
}

// What a wave knows about the block row it fills next: the cell info of its 16 cells (lanes 0..15)
// and, once that load has returned, which cells it decodes itself / copies from the planes.
struct NextRow {
  int nb;        // block row, -1 = none
  uint2 ci;      // lanes 0..15: cell info
  uint32_t m8;   // wave-uniform: DCT8 cells
  uint32_t mp;   // wave-uniform: cells whose tiles come from the planes
};

__device__ __forceinline__ void NextRowRequest(FrameArgs fa, NextRow& n, int nb, int bc0) {
  const FrameArgs f = Fresh(fa);
  const int lane = threadIdx.x & 63;
  const int c16 = bc0 + (lane & 15);
  n.nb = nb;
  n.ci = make_uint2(kCellFromPlanes, 0u);
  if (nb >= 0 && lane < 16 && c16 >= 0 && c16 < (int)f->xsb) n.ci = f->cell_info[(size_t)nb * f->xsb + c16];
}
__device__ __forceinline__ void NextRowMasks(FrameArgs fa, NextRow& n, int bc0) {
  const FrameArgs f = Fresh(fa);
  const int lane = threadIdx.x & 63;
  const int c16 = bc0 + (lane & 15);
  const bool valid_cell = n.nb >= 0 && lane < 16 && c16 >= 0 && c16 < (int)f->xsb;
  const bool is_dct8 = valid_cell && n.ci.x != kCellFromPlanes;
  n.m8 = (uint32_t)__ballot(is_dct8) & 0xffffu;
  n.mp = (uint32_t)__ballot(valid_cell && !is_dct8) & 0xffffu;
}

// Plane cells of block row n.nb, slab rows 2k and 2k+1, all three channels: three LDS-DMA
// instructions of 1 KB (global_load_lds_dwordx4: lane l brings 16 bytes = columns 4 (l & 31) ..
// of row 2k + (l >> 5); the LDS destination of a wave instruction is contiguous, which two
// consecutive 128-float slab rows are).  Called when rows 2k, 2k+1 of the CURRENT block row have
// been consumed: the copy overlaps the march over the remaining rows.
__device__ __forceinline__ void DmaPlaneRows(FrameArgs fa, LdsF* slab, const NextRow& n, int bc0, int k) {
  if (n.mp == 0) return;  // wave-uniform
  const FrameArgs f = Fresh(fa);
  const int lane = threadIdx.x & 63;
  const int cell = (lane & 31) >> 1;
  if ((n.mp >> cell) & 1u) {
    const int row = 2 * k + (lane >> 5);
    const size_t at = ((size_t)(n.nb - (f->plane_y0 >> 3)) * f->tile_stride + (size_t)(bc0 + cell)) * 64u + row * 8 + (lane & 1) * 4;
#pragma unroll
    for (int ch = 0; ch < 3; ch++)
      __builtin_amdgcn_global_load_lds(f->xyb[ch] + at, slab + ch * kSlabPlaneFloats + 2 * k * kSlabCols, 16, 0, 0);
  }
}

// The rest of a block row's fill: the last two plane rows and the DCT8 cells -- the row-per-lane scheme
// of k_transform_8 (kernels_blocks.hip), 8 blocks per step: dequant + CfL, IDCT, register transpose,
// IDCT, two ds_write_b128 per channel.  nb: block row (inside the frame), bc0: block column of slab
// column 0 (-1 at the left edge; cells outside the frame are skipped: no lane reads their columns).
template <typename CT>
__device__ __forceinline__ void FinishSlab(FrameArgs fa, LdsF* slab, LdsU* list, const NextRow& n, int bc0, int first_plane_k) {
  const FrameArgs f = Fresh(fa);
  const int lane = threadIdx.x & 63;
  const int nb = n.nb;
  // every row of the previous block row has been read (this wave's own ds_write stay in order behind
  // the reads; the DMA writes come through the vector memory path: wait for the reads explicitly)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  for (int k = first_plane_k; k < 4; k++) DmaPlaneRows(fa, slab, n, bc0, k);
  const uint32_t m8 = n.m8;
                           // ~50 % busy; a wave cannot overlap its own fill with its own march, and registers + LDS
                           // cap the SIMD at three waves)
  if (m8) {  // wave-uniform
    const bool is_dct8 = lane < 16 && ((m8 >> lane) & 1u);
    if (is_dct8) {
      const uint32_t rank = __builtin_popcount(m8 & ((1u << lane) - 1u));
      list[rank * 4 + 0] = (uint32_t)lane;
      list[rank * 4 + 1] = n.ci.x;
      list[rank * 4 + 2] = n.ci.y;
    }
    const int n8 = __builtin_popcount(m8);
    const int j = lane >> 3;  // matrix row (input), pixel row (output)
    const bool bit3 = (lane & 8) != 0;
    for (int first = 0; first < n8; first += 8) {
      const int b = first + (lane & 7);
      const bool valid = b < n8;
      const int bb = valid ? b : n8 - 1;
      const int cell = (int)list[bb * 4 + 0];
      WorkItem it;
      it.pos = ((uint32_t)nb << 16) | (uint32_t)(bc0 + cell);
      it.off = list[bb * 4 + 1];
      it.qc = list[bb * 4 + 2];
      it.pad = 0;
      const size_t elem = (size_t)it.off * 64u + (size_t)j * 8u;
      const size_t dc_at = (size_t)nb * f->xsb + (size_t)(bc0 + cell);
      Dct8Row<CT> rows[3];
      float dcv[3];
      float tab[3][8];
#pragma unroll
      for (int c = 0; c < 3; c++) {
        rows[c].Load(f->coeffs[c], elem);
        dcv[c] = f->dc[c][dc_at];
      }
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const float4 t0 = *(const float4*)(f->dequant + c * 64 + j * 8);
        const float4 t1 = *(const float4*)(f->dequant + c * 64 + j * 8 + 4);
        tab[c][0] = t0.x, tab[c][1] = t0.y, tab[c][2] = t0.z, tab[c][3] = t0.w;
        tab[c][4] = t1.x, tab[c][5] = t1.y, tab[c][6] = t1.z, tab[c][7] = t1.w;
      }
      BlockHdr h;  // MakeHdr (blocks_common.h) on the kernarg copy of the frame
      {
        const int quant = (int)(it.qc & 0xffffu);
        const float sq = f->inv_global_scale / (float)quant;  // dec_group.cc:164
        h.sx = sq * f->x_dm;
        h.sy = sq;
        h.sb = sq * f->b_dm;
        h.x_cc = f->cfl_base_x + (float)(int8_t)((it.qc >> 16) & 0xffu) * f->color_scale;
        h.b_cc = f->cfl_base_b + (float)(int8_t)(it.qc >> 24) * f->color_scale;
      }
      const float bias0 = f->biases[0], bias1 = f->biases[1], bias2 = f->biases[2], bias3 = f->biases[3];
      int32_t q[8];
      float vy[8];
      rows[1].Unpack(q);
#pragma unroll
      for (int k = 0; k < 8; k++) vy[k] = AdjustQuantBias(q[k], bias1, bias3) * (tab[1][k] * h.sy);
#pragma unroll
      for (int ci3 = 0; ci3 < 3; ci3++) {
        const int c = ci3 == 0 ? 1 : (ci3 == 1 ? 0 : 2);
        float v[8];
        if (c == 1) {
#pragma unroll
          for (int k = 0; k < 8; k++) v[k] = vy[k];
        } else {
          const float sc = c == 0 ? h.sx : h.sb;
          const float cc = c == 0 ? h.x_cc : h.b_cc;
          rows[c].Unpack(q);
#pragma unroll
          for (int k = 0; k < 8; k++) {
            const float d = AdjustQuantBias(q[k], c == 0 ? bias0 : bias2, bias3) * (tab[c][k] * sc);
            v[k] = __builtin_fmaf(cc, vy[k], d);
          }
        }
        if (j == 0) v[0] = dcv[c];
        IdctReg<8>(v);
        Transpose8Lanes(v, bit3);
        IdctReg<8>(v);
        if (valid) {
          typedef float f4v __attribute__((ext_vector_type(4)));
          typedef f4v __attribute__((address_space(3))) * P4;
          LdsF* dst = slab + c * kSlabPlaneFloats + j * kSlabCols + cell * 8;
          *(P4)dst = f4v{v[0], v[1], v[2], v[3]};
          *(P4)(dst + 4) = f4v{v[4], v[5], v[6], v[7]};
        }
      }
    }
  }
  // the LDS-DMA loads count in vmcnt; this wave's ds_write / ds_read stay in order by themselves
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// block row the 8 rows of the group starting at row r come from (also when they are mirror rows: see the header)
__device__ __forceinline__ int GroupBlockRow(int r, int nb_last) {
  const int nb = r < 0 ? 0 : (r >> 3);
  return nb > nb_last ? nb_last : nb;
}

// ------------------------------------------------------------------------------------------------
// k_fused_pc: the same window march with the two halves of the work on two WAVES of a workgroup.
//
// On gfx9 (gfx950 included) a wave has ONE counter, vmcnt, for its vector-memory loads AND stores, and it
// retires in issue order: waiting for a load that was issued behind N output stores waits for the write
// acknowledgements of those N stores first.  The single-wave kernel above waits like that once or twice per
// block row (the inv_sigma load, the vmcnt(0) that ends a fill) -- every group of 8 rows pays the latency of its
// own output stores on top of its loads, and the fill can only start when the march has let go of the slab.
// Here
//   wave 0 (march)  : reads its rows and its inv_sigma values from LDS, computes, stores pixels.  It issues NO
//                     vector-memory load, so it never waits on vmcnt: the stores just queue.
//   wave 1 (produce): fills block row i+1 into the other half of a double-buffered slab (cell info, LDS-DMA of
//                     the plane cells, in-wave DCT8 decode, inv_sigma row) while wave 0 marches over block row i.
//                     It issues no store, so its vmcnt waits cover loads only.
// One s_barrier per block row joins the two (fill(i) done / march(i-1) done).  Workgroup = 128 threads = one
// window; six workgroups per CU (three waves per SIMD by registers, 24.7 KB of LDS each).
static constexpr int kPcWaves = 3;   // waves per SIMD the kernels below are compiled for (<= 168 VGPRs)
static constexpr int kPcPerCu = 6;   // windows resident per CU
template <int NB>
struct __attribute__((aligned(16))) StripLdsT {
  float slab[NB][3 * kSlabPlaneFloats];  // [buffer][channel][row 0..7][column 0..127]
  float sigma[NB][16];                   // [buffer][cell]: inv_sigma of the block row's 16 cells (columns clamped into the frame)
  uint32_t list[NB - 1][16 * 4];         // per producer: the DCT8 cells of the block row being filled
};
typedef StripLdsT<2> StripLds;

// groups of 8 rows a window chunk [y_begin, y_end) walks over: [head (HX rows of the block row above)] + whole
// groups + [tail (HX rows of the block row below)]; group i starts at image row r_first + 8 i
template <int HX>
__device__ __forceinline__ int PcGroups(int y_begin, int y_end) {
  const int whole = (y_end - y_begin + 7) >> 3;
  const bool tail = HX > 0 && y_begin + 8 * whole <= y_end + HX - 1;
  return (HX > 0 ? 1 : 0) + whole + (tail ? 1 : 0);
}

__device__ __forceinline__ void PcBarrierProducer() {
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
__device__ __forceinline__ void PcBarrierMarch() {  // no vmcnt: the output stores stay in flight
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

template <int HX, typename CT>
__device__ __forceinline__ void ProducePC(FrameArgs fa, StripLds* w, int bc0, int y_begin, int y_end, int nb_last) {
  const int lane = threadIdx.x & 63;
  const int r_first = HX ? y_begin - 8 : y_begin;
  const int G = PcGroups<HX>(y_begin, y_end);
  auto sigma_request = [&](int nb) -> float {
    const FrameArgs f = Fresh(fa);
    const int xsb = (int)f->xsb;
    int col = bc0 + (lane & 15);
    col = col < 0 ? 0 : (col >= xsb ? xsb - 1 : col);
    return lane < 16 ? f->inv_sigma[(size_t)nb * xsb + col] : 0.0f;
  };
  NextRow nx;
  int nb = GroupBlockRow(r_first, nb_last);
  NextRowRequest(fa, nx, nb, bc0);
  float sg = sigma_request(nb);
  for (int i = 0; i < G; i++) {
    NextRowMasks(fa, nx, bc0);  // needs the cell info: the first wait of this fill
    const NextRow cur = nx;
    const float sg_cur = sg;
    if (i + 1 < G) {  // the next block row's cell info / sigma travel while this one is decoded
      nb = GroupBlockRow(r_first + 8 * (i + 1), nb_last);
      NextRowRequest(fa, nx, nb, bc0);
      sg = sigma_request(nb);
    }
    LdsF* slab = (LdsF*)w->slab[(i & 1)];
    FinishSlab<CT>(fa, slab, (LdsU*)w->list[0], cur, bc0, 0);  // four plane row pairs by LDS-DMA + the DCT8 cells; ends on vmcnt(0)
    if (lane < 16) ((LdsF*)w->sigma[i & 1])[lane] = sg_cur;
    PcBarrierProducer();
  }
}

// The producer as a software pipeline (16-bit coefficients): the coefficient rows and DC values of block row
// g+1 are requested -- into a second set of registers -- BEFORE block row g is decoded, and block row g+2's cell
// info with them, so that a fill is the decode arithmetic plus LDS writes and the vmcnt(0) in front of the
// barrier finds loads that have had the whole decode to arrive.  (ProducePC above starts every fill with two
// dependent round trips: cell info, then coefficients.)
//
// These loads are issued through inline asm on purpose: for a load it knows, the compiler places the s_waitcnt
// itself, and across this loop's control flow it falls back to vmcnt(0) in front of the first use -- which would
// wait for the prefetch that was just issued.  An asm load's result is "ready" as far as the compiler is concerned;
// the ONLY wait is the vmcnt(0) of PcBarrierProducer, and every loaded register is first used behind it (the two
// register sets alternate through a loop unrolled by two: no copies).
typedef uint32_t u4v __attribute__((ext_vector_type(4)));
typedef uint32_t u2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u4v AsmLoad4(const void* p) {
  u4v r;
  asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(r) : "v"(p) : "memory");
  return r;
}
__device__ __forceinline__ u2v AsmLoad2(const void* p) {
  u2v r;
  asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(r) : "v"(p) : "memory");
  return r;
}
__device__ __forceinline__ uint32_t AsmLoad1(const void* p) {
  uint32_t r;
  asm volatile("global_load_dword %0, %1, off" : "=v"(r) : "v"(p) : "memory");
  return r;
}

struct PcStepRegs {  // one decode step = up to 8 DCT8 cells, lane = (cell of the step: bits 0-2, matrix row: bits 3-5)
  u4v rows[3];       // the lane's row of 8 coefficients, per channel
  uint32_t dcv[3];   // DC of the lane's block (float bits)
  uint32_t qc;
  int cell;          // window cell 0..15 of the lane's block
};
struct PcGroupRegs {
  PcStepRegs st[2];
  int n8;       // DCT8 cells of the block row (wave-uniform)
  uint32_t mp;  // cells copied from the planes (wave-uniform)
  int nb;       // block row
};
struct PcNext {  // cell info + inv_sigma of a block row, as requested (valid behind the next barrier)
  u2v ci;
  uint32_t sg;
  int nb;
};

// Frame constants of the producing wave, read ONCE from the kernarg segment (round 5).  Rounds 2-4 re-read every field
// at its point of use (Fresh above): right for the single-wave kernel, whose march wants every SGPR -- but the
// producing wave of k_fused_pc runs no march, and each re-read was an s_load + s_waitcnt lgkmcnt(0) in the middle of
// the fill (19 scalar round trips per block row).  The wave's ~35 SGPRs of constants stay resident instead, and every
// load is SGPR base + 32-bit lane offset (no 64-bit VALU address arithmetic: 32 v_lshl_add_u64 per decode step before).
struct PcK {
  const char* coef[3];
  const char* dc[3];
  const char* cell_info;
  const char* inv_sigma;
  const float* xyb[3];
  int xsb;
  uint32_t tile_stride;
  int plane_tile_row0;
  float inv_global_scale, x_dm, b_dm, cfl_base_x, cfl_base_b, color_scale;
  float bias[4];
};
__device__ __forceinline__ PcK MakePcK(FrameArgs f) {
  PcK k;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    k.coef[c] = (const char*)f->coeffs[c];
    k.dc[c] = (const char*)f->dc[c];
    k.xyb[c] = f->xyb[c];
  }
  k.cell_info = (const char*)f->cell_info;
  k.inv_sigma = (const char*)f->inv_sigma;
  k.xsb = (int)f->xsb;
  k.tile_stride = f->tile_stride;
  k.plane_tile_row0 = f->plane_y0 >> 3;
  k.inv_global_scale = f->inv_global_scale;
  k.x_dm = f->x_dm;
  k.b_dm = f->b_dm;
  k.cfl_base_x = f->cfl_base_x;
  k.cfl_base_b = f->cfl_base_b;
  k.color_scale = f->color_scale;
#pragma unroll
  for (int i = 0; i < 4; i++) k.bias[i] = f->biases[i];
  return k;
}
// loads at SGPR base + unsigned 32-bit lane offset; no compiler-placed wait (see above)
__device__ __forceinline__ u4v AsmLoad4S(const char* base, uint32_t off) {
  u4v r;
  asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(r) : "v"(off), "s"(base) : "memory");
  return r;
}
__device__ __forceinline__ u2v AsmLoad2S(const char* base, uint32_t off) {
  u2v r;
  asm volatile("global_load_dwordx2 %0, %1, %2" : "=v"(r) : "v"(off), "s"(base) : "memory");
  return r;
}
__device__ __forceinline__ uint32_t AsmLoad1S(const char* base, uint32_t off) {
  uint32_t r;
  asm volatile("global_load_dword %0, %1, %2" : "=v"(r) : "v"(off), "s"(base) : "memory");
  return r;
}

// "These registers are defined HERE": placed right behind the wait (s_waitcnt vmcnt(0) / the barrier) that the data of
// the asm loads above has landed at.  An asm load's result looks ready to the compiler from the load on, and nothing but
// a data dependency keeps it from scheduling a plain VALU use of the register above the (volatile, but register-free)
// wait -- it did exactly that with the first build of this round (a v_cmp of the cell info in front of the prologue's
// s_waitcnt: a memory fault).  Volatile asm statements keep their order, so every use below depends on the wait.
__device__ __forceinline__ void PcLanded(PcNext& n) { asm volatile("" : "+v"(n.ci), "+v"(n.sg)); }
__device__ __forceinline__ void PcLanded(PcGroupRegs& R) {
#pragma unroll
  for (int s = 0; s < 2; s++)
#pragma unroll
    for (int c = 0; c < 3; c++) asm volatile("" : "+v"(R.st[s].rows[c]), "+v"(R.st[s].dcv[c]));
}

__device__ __forceinline__ void PcRequest(const PcK& K, PcNext& n, int nb, int bc0) {
  const int lane = threadIdx.x & 63;
  int col = bc0 + (lane & 15);
  col = col < 0 ? 0 : (col >= K.xsb ? K.xsb - 1 : col);  // lanes 16..63 and cells outside the frame: any valid address
  const uint32_t cell = (uint32_t)(nb * K.xsb + col);  // (whole-frame cell index: < 2^26)
  n.nb = nb;
  n.ci = AsmLoad2S(K.cell_info, cell * 8u);
  n.sg = AsmLoad1S(K.inv_sigma, cell * 4u);
}

// n's registers are valid (a barrier has passed since PcRequest): masks, the DCT8 list, and the loads of the block
// row's coefficient rows / DC values into R
__device__ __forceinline__ void PcIssue(const PcK& K, LdsU* list, const PcNext& n, int bc0, PcGroupRegs& R) {
  const int lane = threadIdx.x & 63;
  const int c16 = bc0 + (lane & 15);
  const bool valid_cell = lane < 16 && c16 >= 0 && c16 < K.xsb;
  const bool is_dct8 = valid_cell && n.ci.x != kCellFromPlanes;
  const uint32_t m8 = (uint32_t)__ballot(is_dct8) & 0xffffu;
  R.mp = (uint32_t)__ballot(valid_cell && !is_dct8) & 0xffffu;
  R.n8 = __builtin_popcount(m8);
  R.nb = n.nb;
  if (m8 == 0) return;  // wave-uniform
  if (is_dct8) {
    const uint32_t rank = __builtin_popcount(m8 & ((1u << lane) - 1u));
    list[rank * 4 + 0] = (uint32_t)lane;
    list[rank * 4 + 1] = n.ci.x;
    list[rank * 4 + 2] = n.ci.y;
  }
  const int j = lane >> 3;
#pragma unroll
  for (int s = 0; s < 2; s++) {
    if (s * 8 < R.n8) {  // wave-uniform
      const int b = s * 8 + (lane & 7);
      const int bb = b < R.n8 ? b : R.n8 - 1;
      const int cell = (int)list[bb * 4 + 0];
      const uint32_t off = list[bb * 4 + 1];
      R.st[s].qc = list[bb * 4 + 2];
      R.st[s].cell = cell;
      // 16-bit coefficients: 128 bytes per block, 16 per matrix row (the offset stays below 2^32: a channel's
      // coefficient buffer is frame pixels x 2 bytes)
      const uint32_t elem_bytes = off * 128u + (uint32_t)j * 16u;
      const uint32_t dc_bytes = (uint32_t)(n.nb * K.xsb + bc0 + cell) * 4u;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        R.st[s].rows[c] = AsmLoad4S(K.coef[c], elem_bytes);
        R.st[s].dcv[c] = AsmLoad1S(K.dc[c], dc_bytes);
      }
    }
  }
}

// Plane cells of block row nb, the four slab row pairs, all three channels: twelve LDS-DMA instructions of 1 KB
// (DmaPlaneRows above, with the producer's resident constants)
__device__ __forceinline__ void PcDmaPlanes(const PcK& K, LdsF* slab, uint32_t mp, int nb, int bc0) {
  if (mp == 0) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  const int cell = (lane & 31) >> 1;
  if ((mp >> cell) & 1u) {
    const uint32_t tile = (uint32_t)(nb - K.plane_tile_row0) * K.tile_stride + (uint32_t)(bc0 + cell);
    const uint32_t at0 = tile * 64u + (uint32_t)(lane >> 5) * 8u + (uint32_t)(lane & 1) * 4u;  // floats; < 2^30 (FusedSupported)
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
      for (int ch = 0; ch < 3; ch++)
        __builtin_amdgcn_global_load_lds(K.xyb[ch] + (at0 + 16u * k), slab + ch * kSlabPlaneFloats + 2 * k * kSlabCols, 16, 0, 0);
  }
}

__device__ __forceinline__ void PcDecode(const PcK& K, LdsF* slab, const PcGroupRegs& R, const float (&tab)[3][8]) {
  const int lane = threadIdx.x & 63;
  const int j = lane >> 3;
  const bool bit3 = (lane & 8) != 0;
#pragma unroll
  for (int s = 0; s < 2; s++) {
    if (s * 8 < R.n8) {  // wave-uniform
      const PcStepRegs& T = R.st[s];
      const bool valid = s * 8 + (lane & 7) < R.n8;
      float sx, sy, sb, x_cc, b_cc;
      {
        const int quant = (int)(T.qc & 0xffffu);
        const float sq = K.inv_global_scale / (float)quant;  // dec_group.cc:164
        sx = sq * K.x_dm;
        sy = sq;
        sb = sq * K.b_dm;
        x_cc = K.cfl_base_x + (float)(int8_t)((T.qc >> 16) & 0xffu) * K.color_scale;
        b_cc = K.cfl_base_b + (float)(int8_t)(T.qc >> 24) * K.color_scale;
      }
      const float bias0 = K.bias[0], bias1 = K.bias[1], bias2 = K.bias[2], bias3 = K.bias[3];
      auto unpack = [](const u4v r, int32_t* q) {
        const uint32_t wv[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
          q[2 * i] = (int32_t)(int16_t)(wv[i] & 0xffffu);
          q[2 * i + 1] = (int32_t)wv[i] >> 16;
        }
      };
      int32_t q[8];
      float vy[8];
      unpack(T.rows[1], q);
#pragma unroll
      for (int k = 0; k < 8; k++) vy[k] = AdjustQuantBias(q[k], bias1, bias3) * (tab[1][k] * sy);
      typedef float f4v __attribute__((ext_vector_type(4)));
      typedef f4v __attribute__((address_space(3))) * P4;
#pragma unroll
      for (int ci3 = 0; ci3 < 3; ci3++) {
        const int c = ci3 == 0 ? 1 : (ci3 == 1 ? 0 : 2);
        float v[8];
        if (c == 1) {
#pragma unroll
          for (int k = 0; k < 8; k++) v[k] = vy[k];
        } else {
          const float sc = c == 0 ? sx : sb;
          const float cc = c == 0 ? x_cc : b_cc;
          unpack(T.rows[c], q);
#pragma unroll
          for (int k = 0; k < 8; k++) {
            const float d = AdjustQuantBias(q[k], c == 0 ? bias0 : bias2, bias3) * (tab[c][k] * sc);
            v[k] = __builtin_fmaf(cc, vy[k], d);
          }
        }
        if (j == 0) v[0] = __uint_as_float(T.dcv[c]);
        IdctReg<8>(v);
        Transpose8Lanes(v, bit3);
        IdctReg<8>(v);
        LdsF* dst = slab + c * kSlabPlaneFloats + j * kSlabCols + T.cell * 8;
        if (valid) {
          *(P4)dst = f4v{v[0], v[1], v[2], v[3]};
          *(P4)(dst + 4) = f4v{v[4], v[5], v[6], v[7]};
        }
      }
    }
  }
}

template <int HX>
__device__ __forceinline__ void ProducePC2(FrameArgs fa, StripLds* w, int bc0, int y_begin, int y_end, int nb_last) {
  const int lane = threadIdx.x & 63;
  const int r_first = HX ? y_begin - 8 : y_begin;
  const int G = PcGroups<HX>(y_begin, y_end);
  const PcK K = MakePcK(fa);
  // this lane's 8 entries of the three DCT8 dequant matrices, once per wave (DequantLane, dec_group.cc:115-153)
  float tab[3][8];
  {
    const int j = lane >> 3;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const float4 t0 = *(const float4*)(fa->dequant + c * 64 + j * 8);
      const float4 t1 = *(const float4*)(fa->dequant + c * 64 + j * 8 + 4);
      tab[c][0] = t0.x, tab[c][1] = t0.y, tab[c][2] = t0.z, tab[c][3] = t0.w;
      tab[c][4] = t1.x, tab[c][5] = t1.y, tab[c][6] = t1.z, tab[c][7] = t1.w;
    }
  }
  LdsU* list = (LdsU*)w->list[0];
  auto group_nb = [&](int g) { return GroupBlockRow(r_first + 8 * (g < G ? g : G - 1), nb_last); };
  PcGroupRegs A, B;
  PcNext n0, n1;
  uint32_t sg_a = 0, sg_b = 0;
  // prologue: block row 0's loads and block row 1's cell info, then everything has landed
  PcRequest(K, n0, group_nb(0), bc0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  PcLanded(n0);
  PcIssue(K, list, n0, bc0, A);
  sg_a = n0.sg;
  PcRequest(K, n1, group_nb(1), bc0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  PcLanded(A);
  PcLanded(n1);
  // one fill: CUR holds block row g (loaded behind an earlier barrier), NXT receives block row g+1,
  // nn = cell info of block row g+1 (valid), refilled with block row g+2's
  auto body = [&](int g, PcGroupRegs& CUR, PcGroupRegs& NXT, uint32_t& sg_cur, uint32_t& sg_nxt, PcNext& nn) {
    LdsF* slab = (LdsF*)w->slab[(g & 1)];  // free: the march left it before the previous barrier
    // the plane cells of block row g first: of everything this fill waits for at its barrier, these copies were the last
    // to be issued (behind the list round trip of PcIssue) -- now they have the whole decode to land
    PcDmaPlanes(K, slab, CUR.mp, CUR.nb, bc0);
    PcIssue(K, list, nn, bc0, NXT);     // block row g+1 (the last block row again behind the end: harmless)
    sg_nxt = nn.sg;
    PcRequest(K, nn, group_nb(g + 2), bc0);
    PcDecode(K, slab, CUR, tab);
    if (lane < 16) ((LdsU*)w->sigma[g & 1])[lane] = sg_cur;
    PcBarrierProducer();
    PcLanded(NXT);
    PcLanded(nn);
  };
  for (int g = 0; g < G; g += 2) {
    body(g, A, B, sg_a, sg_b, n1);
    if (g + 1 < G) body(g + 1, B, A, sg_b, sg_a, n1);
  }
}

// rows per window chunk: a multiple of 8 that fills whole generations of resident workgroups (6 per CU); a chunk costs
// its rows + 2 x HX marched rows + two more block-row fills
int FusedRowsPC(unsigned strips, unsigned rows, unsigned per_cu = kPcPerCu) {
  const int forced = jxlhip_env::Get().fused_pc_rh.load(std::memory_order_relaxed);  // experiments / tests: rows per window chunk
  if (forced > 0) return (forced + 7) & ~7;
  return ChunkRows(strips, rows, DeviceCus() * per_cu, 16, 1024, 8, 6 + 16);
}

}  // namespace
}  // namespace jxlhip
#endif  // JXLHIP_FUSED_PC_H_
