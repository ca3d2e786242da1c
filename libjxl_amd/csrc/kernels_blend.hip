// kernels_blend.hip -- frame blending (FrameHeader::blending_info, custom_size_or_origin) on gfx950: the render
// pipeline's last stage in front of the output, a decoded frame blended over a saved canvas at its origin, and the
// blended frame saved for the frames that follow.
//
// Replaces (behaviour, not code): lib/jxl/render_pipeline/stage_blending.cc (ProcessRow, ProcessPaddingRow),
// lib/jxl/blending.cc:42-190 (PerformBlending, the colour channels of an image without extra channels: a frame of an
// image with alpha or other extra channels goes to k_ec_blend, kernels_blend_ec.hip, which has this kernel's geometry),
// lib/jxl/alpha.cc:82-93 (PerformMulBlending) and the save of dec_frame.cc:870-885 for frames saved after the colour
// transform.
//
// One kernel, k_blend, behind the frame's whole path, which has written the frame as packed float RGB in the output's
// transfer function into context staging memory (jxlhip_decode_frame, DecodeFrameBlended).  The kernel is elementwise
// and memory-bound: a thread takes four horizontally adjacent canvas pixels = 12 floats = three 16-byte vectors of the
// canvas, of the staged frame and of the slot it saves into; the grid is capped (256 groups of a row per block, the blocks stride over the rows: 32-bit index arithmetic only).  Canvas
// rows and staged rows are padded to four pixels, and the staged frame starts (x0 mod 4) pixels into its rows, so that
// a canvas vector and the staged vector under it are both 16-byte aligned whatever the origin.  Per sample the result
// is one IEEE operation on (bg, fg) inside the frame's rectangle and bg outside, so it equals the reference's row
// loops bit for bit.  No LDS.
//
// What a launch reads and writes is decided on the host (BlendArgs):
//   region   the 4-pixel groups and rows it visits: the whole canvas when the caller's output or another slot is
//            written, only the groups under the rectangle when the frame is blended into its own source slot
//   src      the source canvas; nullptr = empty slot = zeroes.  Not read where the rectangle covers a group and the
//            mode replaces.
//   dst      the slot saved into (may be src: a thread reads its own twelve floats before it writes them and touches
//            nothing else); nullptr = not saved
//   P.out    the caller's output at canvas coordinates, through emit.h's packing with the transfer function forced to
//            identity by the host (the samples are already encoded); OUTK 0 = none
#include <algorithm>

#include "dev_common.h"
#include "emit.h"
#include "kernels.h"

namespace jxlhip {

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));  // the caller's rows are only sample-aligned

// Clamp (base/common.h: Clamp1(x, 0, 1)); a NaN passes, as there
__device__ __forceinline__ float Clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

// One sample: a single IEEE operation on (bg, fg), chosen by selects on the launch-uniform op
__device__ __forceinline__ float Blend(uint32_t op, float bg, float fg) {
  const float sum = bg + fg;
  const float prod = bg * (op == kPatchOpMulClamp ? Clamp01(fg) : fg);
  return op == kPatchOpReplace ? fg : (op == kPatchOpAdd ? sum : prod);
}

template <int OUTK>
__global__ __launch_bounds__(256) void k_blend(BlendArgs A, FilterParams P) {
  // blockIdx.x: 256 groups of a row; blockIdx.y: the first of the rows this block takes, gridDim.y apart
  const uint32_t g = A.gx0 + blockIdx.x * 256u + threadIdx.x;
  if (g >= A.gx1) return;
  const uint32_t op = A.op;
#pragma unroll 1
  for (uint32_t yy = A.y0 + blockIdx.y; yy < A.y1; yy += gridDim.y) {
    const int y = (int)yy;
    // x is the same in every turn, but what the general packed tail derives from it (dither columns, store addresses
    // of every sample type) must not be hoisted out of the loop and held in registers: 100 VGPRs instead of 60
    int x = (int)(4 * g);
    asm volatile("" : "+v"(x));
    const bool row_in = y >= A.ry0 && y < A.ry1;
    bool in[4], any_in = false, all_in = true;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      in[k] = row_in && x + k >= A.rx0 && x + k < A.rx1;
      any_in = any_in || in[k];
      all_in = all_in && in[k];
    }
    float bg[12], fg[12], v[12];
    if (A.src && !(all_in && op == kPatchOpReplace)) {
      const f4* s = (const f4*)(A.src + (size_t)y * A.src_stride + 12 * (size_t)g);
      const f4 a = s[0], b = s[1], c = s[2];
#pragma unroll
      for (int k = 0; k < 4; k++) bg[k] = a[k], bg[4 + k] = b[k], bg[8 + k] = c[k];
    } else {
#pragma unroll
      for (int k = 0; k < 12; k++) bg[k] = 0.0f;  // (zeroes_ of the reference's stage)
    }
    if (any_in) {
      // (x - fg_xa is a non-negative multiple of 4 here, and the group lies inside the padded staged row)
      const f4* s = (const f4*)(A.fg + (size_t)(y - A.fg_y0) * A.fg_stride + 3 * (size_t)(x - A.fg_xa));
      const f4 a = s[0], b = s[1], c = s[2];
#pragma unroll
      for (int k = 0; k < 4; k++) fg[k] = a[k], fg[4 + k] = b[k], fg[8 + k] = c[k];
#pragma unroll
      for (int k = 0; k < 12; k++) v[k] = in[k / 3] ? Blend(op, bg[k], fg[k]) : bg[k];
    } else {
#pragma unroll
      for (int k = 0; k < 12; k++) v[k] = bg[k];
    }
    if (A.dst && (A.dst_all || any_in)) {
      f4* d = (f4*)(A.dst + (size_t)y * A.dst_stride + 12 * (size_t)g);
      d[0] = f4{v[0], v[1], v[2], v[3]};
      d[1] = f4{v[4], v[5], v[6], v[7]};
      d[2] = f4{v[8], v[9], v[10], v[11]};
    }
    if constexpr (OUTK != 0) {
      char* row = (char*)P.out + (size_t)y * P.out_stride;
      const int W = (int)A.W;
      if (x + 3 < W) {
        if constexpr (OUTK == JXLHIP_OUT_LINEAR_RGB_F32) {
          f4u* d = (f4u*)(row + 12 * (size_t)x);
          __builtin_nontemporal_store(f4u{v[0], v[1], v[2], v[3]}, d);
          __builtin_nontemporal_store(f4u{v[4], v[5], v[6], v[7]}, d + 1);
          __builtin_nontemporal_store(f4u{v[8], v[9], v[10], v[11]}, d + 2);
        } else {
          StorePackedPair<FmtSel<-1>>(P, P.dither, row, x, y, v, v + 3);
          StorePackedPair<FmtSel<-1>>(P, P.dither, row, x + 2, y, v + 6, v + 9);
        }
      } else {
#pragma unroll
        for (int k = 0; k < 3; k++) {
          if (x + k >= W) break;
          if constexpr (OUTK == JXLHIP_OUT_LINEAR_RGB_F32) {
            float* d = (float*)row + 3 * (size_t)(x + k);
            d[0] = v[3 * k];
            d[1] = v[3 * k + 1];
            d[2] = v[3 * k + 2];
          } else {
            StorePackedPixel<FmtSel<-1>>(P, P.dither, row, x + k, y, v + 3 * k);
          }
        }
      }
    }
  }
}

}  // namespace

bool LaunchBlend(const BlendArgs& A, const FilterParams& p, int output_kind, hipStream_t st) {
  if (output_kind < 0 || output_kind > 2 || A.W == 0 || A.H == 0 || A.op > kPatchOpMulClamp) return false;
  if (A.gx1 <= A.gx0 || A.y1 <= A.y0) return true;  // nothing to visit
  if (A.gx1 > (A.W + 3) / 4 || A.y1 > A.H) return false;
  // memory-bound: at most eight blocks per compute unit; a block takes 256 groups of a row and strides over the rows
  const unsigned bx = (A.gx1 - A.gx0 + 255) / 256;
  const unsigned by = std::min<unsigned>(A.y1 - A.y0, std::max<unsigned>(1u, DeviceCus() * 8 / bx));
  const dim3 blocks(bx, by);
  if (output_kind == 0)
    hipLaunchKernelGGL((k_blend<0>), blocks, dim3(256), 0, st, A, p);
  else if (output_kind == JXLHIP_OUT_LINEAR_RGB_F32)
    hipLaunchKernelGGL((k_blend<JXLHIP_OUT_LINEAR_RGB_F32>), blocks, dim3(256), 0, st, A, p);
  else
    hipLaunchKernelGGL((k_blend<JXLHIP_OUT_PACKED>), blocks, dim3(256), 0, st, A, p);
  return true;
}

}  // namespace jxlhip
