// kernels_splines.hip -- splines (FrameHeader::kSplines) on gfx950: the render pipeline's spline stage, DrawSegments
// on every pixel of the frame, followed by the caller's output tail.
//
// Replaces (behaviour, not code): lib/jxl/splines.cc:82-127 (DrawSegment), :173-182 (DrawSegments) and
// lib/jxl/render_pipeline/stage_splines.cc; FastErff (lib/jxl/base/fast_math-inl.h:129-157).
//
// One kernel, k_splines, behind the frame's normal filter path, which has written the filtered frame as planar XYB.
// A block of 256 threads takes one 64 x 16 tile (a thread = one column, rows r, r + 4, r + 8, r + 12).  The host
// bins the frame's segments by tile (SplineArgs: a CSR list per tile, in increasing segment order -- the order in
// which DrawSegments adds them to any one row); the block stages its tile's records through LDS in chunks and adds
// each segment whose row span holds the pixel's row and whose column span [llround(cx - d), llround(cx + d)] holds
// its column, accumulating into the pixel's value one segment after another as the reference does.  Two forms:
//   draw-and-emit  (no noise) every tile of the frame, then the output tail of the filter kernels (emit.h): planar
//                  XYB, linear float RGB or any packed format with dither and alpha;
//   draw-in-place  (noise follows) only the tiles with segments; writes the XYB planes back for k_noise_rng /
//                  k_noise_emit.
#include "dev_common.h"
#include "emit.h"
#include "kernels.h"

namespace jxlhip {

namespace {

constexpr int kTW = 64, kTH = 16, kRowsPerThread = kTH / (256 / kTW), kChunk = 128;

// FastErff (fast_math-inl.h:129-157), one lane: 1 - 1 / (((a|x| + b)|x| + c)|x| + d)|x| + 1)^4 with x's sign
__device__ __forceinline__ float FastErf(float x) {
  const bool le0 = x <= 0.0f;
  const float ax = __builtin_fabsf(x);
  const float d1 = __builtin_fmaf(ax, 7.77394369e-02f, 2.05260015e-04f);
  const float d2 = __builtin_fmaf(d1, ax, 2.32120216e-01f);
  const float d3 = __builtin_fmaf(d2, ax, 2.77820801e-01f);
  const float d4 = __builtin_fmaf(d3, ax, 1.0f);
  const float d5 = d4 * d4;
  const float inv = 1.0f / d5;
  const float r = __builtin_fmaf(-inv, inv, 1.0f);
  return le0 ? -r : r;
}

template <int OUTK, bool INPLACE>
__global__ __launch_bounds__(256) void k_splines(SplineArgs S, FilterParams P) {
  __shared__ SplineSeg seg[kChunk];
  const uint32_t tile = INPLACE ? S.active[blockIdx.x] : blockIdx.y * S.tiles_x + blockIdx.x;
  const uint32_t ty = tile / S.tiles_x, tx = tile - ty * S.tiles_x;
  const int W = (int)S.xsize, H = (int)S.ysize;
  const int x = (int)tx * kTW + (int)(threadIdx.x & (kTW - 1));
  const int yb = (int)ty * kTH + (int)(threadIdx.x / kTW);
  const bool xin = x < W;
  float v[kRowsPerThread][3];
#pragma unroll
  for (int k = 0; k < kRowsPerThread; k++) {
    const int y = yb + 4 * k;
    if (xin && y < H) {
      const size_t o = (size_t)y * S.ns + x;
      v[k][0] = S.xyb[o];
      v[k][1] = S.xyb[o + S.nplane];
      v[k][2] = S.xyb[o + 2 * S.nplane];
    } else {
      v[k][0] = v[k][1] = v[k][2] = 0.0f;
    }
  }
  const uint32_t s0 = S.tile_start[tile], s1 = S.tile_start[tile + 1];
  const float fx = (float)x;
  for (uint32_t base = s0; base < s1; base += kChunk) {
    const uint32_t n = min((uint32_t)kChunk, s1 - base);
    __syncthreads();  // (the previous chunk is done with)
    if (threadIdx.x < n) seg[threadIdx.x] = S.segs[S.tile_idx[base + threadIdx.x]];
    __syncthreads();
    if (!xin) continue;
#pragma unroll 1
    for (uint32_t j = 0; j < n; j++) {
      const SplineSeg& g = seg[j];
      if (x < g.x0 || x > g.x1) continue;
      const float dx = fx - g.cx;
#pragma unroll
      for (int k = 0; k < kRowsPerThread; k++) {
        const int y = yb + 4 * k;
        if (y < g.y0 || y >= g.y1) continue;  // (y1 <= H)
        // DrawSegment (:82-110)
        const float dy = (float)y - g.cy;
        const float d = __builtin_sqrtf(__builtin_fmaf(dx, dx, dy * dy));
        const float f = FastErf(__builtin_fmaf(d, 0.5f, 0.353553391f) * g.inv_sigma) -
                        FastErf(__builtin_fmaf(d, 0.5f, -0.353553391f) * g.inv_sigma);
        const float li = g.s4i * (f * f);
        v[k][0] = __builtin_fmaf(g.color[0], li, v[k][0]);
        v[k][1] = __builtin_fmaf(g.color[1], li, v[k][1]);
        v[k][2] = __builtin_fmaf(g.color[2], li, v[k][2]);
      }
    }
  }
  if (!xin) return;
#pragma unroll
  for (int k = 0; k < kRowsPerThread; k++) {
    const int y = yb + 4 * k;
    if (y >= H) break;
    if constexpr (INPLACE) {
      const size_t o = (size_t)y * S.ns + x;
      S.xyb_out[o] = v[k][0];
      S.xyb_out[o + S.nplane] = v[k][1];
      S.xyb_out[o + 2 * S.nplane] = v[k][2];
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

bool LaunchSplines(const SplineArgs& S, const FilterParams& p, int output_kind, bool in_place, hipStream_t st) {
  if (output_kind < 0 || output_kind > 2 || S.xsize == 0 || S.ysize == 0) return false;
  if (in_place) {
    if (S.num_active) hipLaunchKernelGGL((k_splines<0, true>), dim3(S.num_active), dim3(256), 0, st, S, p);
    return true;
  }
  const dim3 grid(S.tiles_x, (S.ysize + kTH - 1) / kTH);
  if (output_kind == JXLHIP_OUT_XYB_PLANAR)
    hipLaunchKernelGGL((k_splines<JXLHIP_OUT_XYB_PLANAR, false>), grid, dim3(256), 0, st, S, p);
  else if (output_kind == JXLHIP_OUT_LINEAR_RGB_F32)
    hipLaunchKernelGGL((k_splines<JXLHIP_OUT_LINEAR_RGB_F32, false>), grid, dim3(256), 0, st, S, p);
  else
    hipLaunchKernelGGL((k_splines<JXLHIP_OUT_PACKED, false>), grid, dim3(256), 0, st, S, p);
  return true;
}

}  // namespace jxlhip
