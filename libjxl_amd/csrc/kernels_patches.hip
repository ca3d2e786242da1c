// kernels_patches.hip -- patches (FrameHeader::kPatches) on gfx950: the render pipeline's patch stage, every patch of the
// dictionary blended into the frame in dictionary order, followed by the caller's output tail.
//
// Replaces (behaviour, not code): lib/jxl/dec_patch_dictionary.cc:286-357 (GetPatchesForRow, AddOneRow),
// lib/jxl/blending.cc:42-190 (PerformBlending, the colour channels of an image without an alpha channel),
// lib/jxl/alpha.cc:82-93 (PerformMulBlending) and lib/jxl/render_pipeline/stage_patches.cc.
//
// One kernel, k_patches, behind the frame's normal filter path, which has written the filtered frame as planar XYB.
// A block of 256 threads takes one 64 x 16 tile (a thread = one column, rows r, r + 4, r + 8, r + 12; a wave = four
// whole rows of the tile, so the row test of a record is the same for all its lanes).  The host bins the dictionary by
// tile (PatchArgs: a CSR list per tile, in increasing patch order); the block stages its tile's records through LDS in
// batches of kPatchBatch and every thread walks them in order: for the pixels it owns inside a record's rectangle it
// reads the reference sample of X, Y and B and applies the record's operation -- one IEEE operation per sample, so the
// result is that of the reference's row loops bit for bit.  Two forms:
//   blend-and-emit  (nothing behind the patches) every tile of the frame, then the output tail of the filter kernels
//                   (emit.h): planar XYB, linear float RGB or any packed format with dither;
//   blend-in-place  (splines, upsampling or noise follow) only the tiles with records; writes the XYB planes back.
// A tile writes its own pixels only: the in-place form has no race between workgroups.
#include "dev_common.h"
#include "emit.h"
#include "kernels.h"

namespace jxlhip {

namespace {

constexpr int kTW = 64, kTH = 16, kRowsPerThread = kTH / (256 / kTW);

// Clamp (base/common.h: Clamp1(x, 0, 1)); a NaN passes, as there
__device__ __forceinline__ float Clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

// One sample: every result is a single IEEE operation on (bg, fg), chosen by selects -- no branch inside the record loop
__device__ __forceinline__ float Blend(uint32_t op, float bg, float fg) {
  const float sum = bg + fg;
  const float prod = bg * (op == kPatchOpMulClamp ? Clamp01(fg) : fg);
  return op == kPatchOpReplace ? fg : (op == kPatchOpAdd ? sum : prod);
}

template <int OUTK, bool INPLACE>
__global__ __launch_bounds__(256) void k_patches(PatchArgs A, FilterParams P) {
  __shared__ PatchRec rec[kPatchBatch];
  const uint32_t tile = INPLACE ? A.active[blockIdx.x] : blockIdx.y * A.tiles_x + blockIdx.x;
  const uint32_t ty = tile / A.tiles_x, tx = tile - ty * A.tiles_x;
  const int W = (int)A.xsize, H = (int)A.ysize;
  const int x = (int)tx * kTW + (int)(threadIdx.x & (kTW - 1));
  const int yb = (int)ty * kTH + (int)(threadIdx.x / kTW);
  const bool xin = x < W;
  float v[kRowsPerThread][3];
#pragma unroll
  for (int k = 0; k < kRowsPerThread; k++) {
    const int y = yb + 4 * k;
    if (xin && y < H) {
      const size_t o = (size_t)y * A.ns + x;
      v[k][0] = A.xyb[o];
      v[k][1] = A.xyb[o + A.nplane];
      v[k][2] = A.xyb[o + 2 * A.nplane];
    } else {
      v[k][0] = v[k][1] = v[k][2] = 0.0f;
    }
  }
  const uint32_t s0 = A.tile_start[tile], s1 = A.tile_start[tile + 1];
  for (uint32_t base = s0; base < s1; base += kPatchBatch) {
    const uint32_t n = min(kPatchBatch, s1 - base);
    __syncthreads();  // (the previous batch is done with)
    if (threadIdx.x < n) rec[threadIdx.x] = A.recs[A.tile_idx[base + threadIdx.x]];
    __syncthreads();
    if (!xin) continue;
#pragma unroll 1
    for (uint32_t j = 0; j < n; j++) {
      const PatchRec r = rec[j];  // (one LDS read of the whole record, the same address in every lane)
      // the rows of a wave are the same for all its lanes: a record that misses them, or whose columns hold none of the
      // lanes, is skipped by the whole wave
      bool hit[kRowsPerThread], any = false;
#pragma unroll
      for (int k = 0; k < kRowsPerThread; k++) {
        const int y = yb + 4 * k;
        hit[k] = y >= r.y0 && y < r.y1;  // (x1 <= W, y1 <= H)
        any = any || hit[k];
      }
      if (!any || x < r.x0 || x >= r.x1) continue;
      // all twelve reference samples are requested before the first is used (a row outside the rectangle reads the
      // rectangle's first row instead, a sample that exists and is cached): one memory latency per record, not twelve
      const float* src = r.src + (x - r.x0);
      const uint32_t op = r.op;
      float fg[kRowsPerThread][3];
#pragma unroll
      for (int k = 0; k < kRowsPerThread; k++) {
        const float* s = src + (hit[k] ? (size_t)(yb + 4 * k - r.y0) * r.stride : 0);
        fg[k][0] = s[0];
        fg[k][1] = s[r.plane];
        fg[k][2] = s[2 * (size_t)r.plane];
      }
#pragma unroll
      for (int k = 0; k < kRowsPerThread; k++) {
#pragma unroll
        for (int c = 0; c < 3; c++) v[k][c] = hit[k] ? Blend(op, v[k][c], fg[k][c]) : v[k][c];
      }
    }
  }
  if (!xin) return;
#pragma unroll
  for (int k = 0; k < kRowsPerThread; k++) {
    const int y = yb + 4 * k;
    if (y >= H) break;
    if constexpr (INPLACE) {
      const size_t o = (size_t)y * A.ns + x;
      A.xyb_out[o] = v[k][0];
      A.xyb_out[o + A.nplane] = v[k][1];
      A.xyb_out[o + 2 * A.nplane] = v[k][2];
    } else if constexpr (OUTK == JXLHIP_OUT_XYB_PLANAR) {
      float* d = (float*)P.out + (size_t)y * P.out_stride + x;
      d[0] = v[k][0];
      d[P.out_plane_stride] = v[k][1];
      d[2 * P.out_plane_stride] = v[k][2];
    } else {
      float rgb[3];
      XybToRgb(v[k][0], v[k][1], v[k][2], P, rgb);
      if constexpr (OUTK == JXLHIP_OUT_LINEAR_RGB_F32) {
        float* d = (float*)((char*)P.out + (size_t)y * P.out_stride) + 3 * (size_t)x;
        d[0] = rgb[0];
        d[1] = rgb[1];
        d[2] = rgb[2];
      } else {
        StorePackedPixel<FmtSel<-1>>(P, P.dither, (char*)P.out + (size_t)y * P.out_stride, x, y, rgb);
      }
    }
  }
}

}  // namespace

bool LaunchPatches(const PatchArgs& A, const FilterParams& p, int output_kind, bool in_place, hipStream_t st) {
  if (output_kind < 0 || output_kind > 2 || A.xsize == 0 || A.ysize == 0) return false;
  if (in_place) {
    if (A.num_active) hipLaunchKernelGGL((k_patches<0, true>), dim3(A.num_active), dim3(256), 0, st, A, p);
    return true;
  }
  const dim3 grid(A.tiles_x, (A.ysize + kTH - 1) / kTH);
  if (output_kind == JXLHIP_OUT_XYB_PLANAR)
    hipLaunchKernelGGL((k_patches<JXLHIP_OUT_XYB_PLANAR, false>), grid, dim3(256), 0, st, A, p);
  else if (output_kind == JXLHIP_OUT_LINEAR_RGB_F32)
    hipLaunchKernelGGL((k_patches<JXLHIP_OUT_LINEAR_RGB_F32, false>), grid, dim3(256), 0, st, A, p);
  else
    hipLaunchKernelGGL((k_patches<JXLHIP_OUT_PACKED, false>), grid, dim3(256), 0, st, A, p);
  return true;
}

}  // namespace jxlhip
