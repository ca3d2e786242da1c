// kernels_upsample.hip -- upsampled frames (FrameHeader::upsampling = 2, 4, 8) on gfx950: the render pipeline's
// upsampling stage on the three XYB planes, followed by the caller's output tail.
//
// Replaces (behaviour, not code): lib/jxl/render_pipeline/stage_upsampling.cc:51-84 (the expansion of the coded weights
// to N x N kernels of 5 x 5 taps), :147-276 (the neighbourhood's minimum / maximum, the 25-tap sum, the clamp) and the
// pipeline's border of 2 pixels mirrored at the edge of the CODED frame (lib/jxl/image_ops.h:184-196).
//
// One kernel, k_upsample<N, OUTK>, behind the frame's normal filter path (and k_splines, draw-in-place), which has
// written the filtered frame as planar XYB at coded size.  A block of 256 threads takes one 64 x 16 tile of CODED
// pixels: the tile plus its 2-pixel border of the three planes goes into LDS (mirrored at the coded frame's edge,
// repeatedly for frames narrower than the border); a thread = one coded column, rows r, r + 4, r + 8, r + 12.  For each
// of its coded pixels the thread keeps the 3 x 25 samples in registers and loops over the N x N output pixels: the
// kernel index is the same for the whole wave, and the table is read through the constant address space, so the 2 x 25
// weights of an output pair arrive in SGPRs (s_load_dwordx16 + x8 + x1 per kernel in the ISA; the only vector loads
// left are the tile's).  The sum is the reference's: three accumulators over taps i, i + 1, i + 2, fused
// multiply-adds, (acc1 + acc2) + acc0, clamped to the neighbourhood's range.  The outputs are computed and stored two
// at a time (x even: 24 bytes of float RGB as 16 + 8, 8 of RGBA8, 8 per plane of planar XYB).  A lane's N outputs of a
// row are contiguous and so are the wave's 64 * N, but ONE store instruction of the wave covers 2 pixels of every N:
// all of each cache line at N = 2, half of it at N = 4, a quarter at N = 8; the line is completed by the next
// iterations of the same wave.  Two forms:
//   upsample-and-emit  (no noise) the output tail of the filter kernels (emit.h) at output resolution, cropped to the
//                      image size: planar XYB, linear float RGB or any packed format with dither;
//   upsample-to-planes (noise follows) planar XYB at output resolution for k_noise_rng / k_noise_emit: the same kernel
//                      with the planar output pointed at context memory.
#include <algorithm>

#include "dev_common.h"
#include "emit.h"
#include "kernels.h"

namespace jxlhip {

namespace {

constexpr int kTW = 64, kTH = 16, kLW = kTW + 4, kLH = kTH + 4;

// the kernels' table read through the constant address space: with a wave-uniform index the compiler then fetches
// the weights with scalar loads into SGPRs (through a plain global pointer it issues one vector load per lane, all
// 64 lanes on one address: the stores through P.out could alias it)
typedef const float __attribute__((address_space(4))) * ConstF;

__device__ __forceinline__ int MirrorN(int x, int n) {  // image_ops.h:184-196
  while (x < 0 || x >= n) x = x < 0 ? -x - 1 : 2 * n - 1 - x;
  return x;
}

template <int N, int OUTK>
__global__ __launch_bounds__(256) void k_upsample(UpsampleArgs U, FilterParams P) {
  __shared__ float t[3][kLH * kLW];
  const int tx0 = blockIdx.x * kTW, ty0 = blockIdx.y * kTH;
  const int CW = (int)U.cw, CH = (int)U.ch, W = (int)U.xsize, H = (int)U.ysize;
  for (int i = threadIdx.x; i < kLH * kLW; i += 256) {
    const int ly = i / kLW, lx = i - ly * kLW;
    const size_t o = (size_t)MirrorN(ty0 - 2 + ly, CH) * U.ns + MirrorN(tx0 - 2 + lx, CW);
    t[0][i] = U.xyb[o];
    t[1][i] = U.xyb[o + U.nplane];
    t[2][i] = U.xyb[o + 2 * U.nplane];
  }
  __syncthreads();
  const int lx = threadIdx.x & (kTW - 1);
  const int cx = tx0 + lx;
  if (cx >= CW) return;
  const ConstF wt = (ConstF)U.weights;  // (written by a copy that is complete before the launch; never by a kernel)
#pragma unroll 1
  for (int ly = threadIdx.x / kTW; ly < kTH; ly += 256 / kTW) {
    const int cy = ty0 + ly;
    if (cy >= CH) break;
    float v[3][25], lo[3], hi[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
#pragma unroll
      for (int i = 0; i < 25; i++) v[c][i] = t[c][(ly + i / 5) * kLW + lx + i % 5];
      lo[c] = hi[c] = v[c][0];
#pragma unroll
      for (int i = 1; i < 25; i++) {
        lo[c] = __builtin_fminf(lo[c], v[c][i]);
        hi[c] = __builtin_fmaxf(hi[c], v[c][i]);
      }
    }
#pragma unroll 1
    for (int oy = 0; oy < N; oy++) {
      const int y = cy * N + oy;
      if (y >= H) break;
      // two output pixels at a time: their samples are neighbours in every interleaved output (x is even)
#pragma unroll 1
      for (int ox = 0; ox < N; ox += 2) {
        const int x = cx * N + ox;
        if (x >= W) break;  // the crop to the image size
        const ConstF k = wt + (oy * N + ox) * 25;  // (wave-uniform: kernels ox and ox + 1)
        float r[2][3];
#pragma unroll
        for (int j = 0; j < 2; j++) {
#pragma unroll
          for (int c = 0; c < 3; c++) {
            // UpsamplingStage::ProcessRowImpl (stage_upsampling.cc:249-261)
            float a0 = v[c][0] * k[25 * j], a1 = v[c][1] * k[25 * j + 1], a2 = v[c][2] * k[25 * j + 2];
#pragma unroll
            for (int i = 3; i < 24; i += 3) {
              a0 = __builtin_fmaf(v[c][i], k[25 * j + i], a0);
              a1 = __builtin_fmaf(v[c][i + 1], k[25 * j + i + 1], a1);
              a2 = __builtin_fmaf(v[c][i + 2], k[25 * j + i + 2], a2);
            }
            a0 = __builtin_fmaf(v[c][24], k[25 * j + 24], a0);
            r[j][c] = __builtin_fminf(__builtin_fmaxf((a1 + a2) + a0, lo[c]), hi[c]);
          }
        }
        const bool pair = x + 1 < W;
        if constexpr (OUTK == JXLHIP_OUT_XYB_PLANAR) {
          typedef float f2 __attribute__((ext_vector_type(2), aligned(4)));
          float* d = (float*)P.out + (size_t)y * P.out_stride + x;
#pragma unroll
          for (int c = 0; c < 3; c++) {
            if (pair) *(f2*)(d + c * P.out_plane_stride) = f2{r[0][c], r[1][c]};  // (the noise launches read it back: cached)
            else d[c * P.out_plane_stride] = r[0][c];
          }
        } else {
          float rgb0[3], rgb1[3];
          XybToRgb(r[0][0], r[0][1], r[0][2], P, rgb0);
          XybToRgb(r[1][0], r[1][1], r[1][2], P, rgb1);
          char* row = (char*)P.out + (size_t)y * P.out_stride;
          if constexpr (OUTK == JXLHIP_OUT_LINEAR_RGB_F32) {
            float* d = (float*)row + 3 * (size_t)x;
            if (pair) {  // 24 bytes as 16 + 8 (emit.h StorePackedPair says why not 12 + 12)
              typedef float f2 __attribute__((ext_vector_type(2), aligned(4)));
              typedef float f4 __attribute__((ext_vector_type(4), aligned(4)));
              __builtin_nontemporal_store(f4{rgb0[0], rgb0[1], rgb0[2], rgb1[0]}, (f4*)d);
              asm volatile("" ::: "memory");
              __builtin_nontemporal_store(f2{rgb1[1], rgb1[2]}, (f2*)(d + 4));
            } else {
              d[0] = rgb0[0];
              d[1] = rgb0[1];
              d[2] = rgb0[2];
            }
          } else if (pair) {
            StorePackedPair<FmtSel<-1>>(P, P.dither, row, x, y, rgb0, rgb1);
          } else {
            StorePackedPixel<FmtSel<-1>>(P, P.dither, row, x, y, rgb0);
          }
        }
      }
    }
  }
}

template <int N>
void LaunchN(const UpsampleArgs& U, const FilterParams& p, int output_kind, hipStream_t st) {
  const dim3 grid((U.cw + kTW - 1) / kTW, (U.ch + kTH - 1) / kTH);
  if (output_kind == JXLHIP_OUT_XYB_PLANAR)
    hipLaunchKernelGGL((k_upsample<N, JXLHIP_OUT_XYB_PLANAR>), grid, dim3(256), 0, st, U, p);
  else if (output_kind == JXLHIP_OUT_LINEAR_RGB_F32)
    hipLaunchKernelGGL((k_upsample<N, JXLHIP_OUT_LINEAR_RGB_F32>), grid, dim3(256), 0, st, U, p);
  else
    hipLaunchKernelGGL((k_upsample<N, JXLHIP_OUT_PACKED>), grid, dim3(256), 0, st, U, p);
}

}  // namespace

// UpsamplingStage's constructor (stage_upsampling.cc:58-83): the coded weights are the upper triangle of a symmetric
// matrix of 5N/2 x 5N/2 entries, the top-left quarter of the N x N kernels; the other quarters are its mirror images
void UpsampleKernels(uint32_t n, const float* coded, float* kernels) {
  const uint32_t h = n / 2;
  for (uint32_t ky = 0; ky < h; ky++)
    for (uint32_t kx = 0; kx < h; kx++) {
      float* k0 = kernels + (ky * n + kx) * 25;
      float* k1 = kernels + (ky * n + (n - 1 - kx)) * 25;
      float* k2 = kernels + ((n - 1 - ky) * n + kx) * 25;
      float* k3 = kernels + ((n - 1 - ky) * n + (n - 1 - kx)) * 25;
      for (uint32_t py = 0; py < 5; py++)
        for (uint32_t px = 0; px < 5; px++) {
          const uint32_t j = 5 * ky + py, i = 5 * kx + px;
          const uint32_t my = std::min(i, j), mx = std::max(i, j);
          const float w = coded[5 * h * my - my * (my - 1) / 2 + mx - my];
          k0[py * 5 + px] = w;
          k1[py * 5 + (4 - px)] = w;
          k2[(4 - py) * 5 + px] = w;
          k3[(4 - py) * 5 + (4 - px)] = w;
        }
    }
}

bool LaunchUpsample(const UpsampleArgs& U, const FilterParams& p, int output_kind, float* planes_out, uint32_t planes_ns,
                    size_t planes_nplane, hipStream_t st) {
  if (output_kind < 0 || output_kind > 2 || U.cw == 0 || U.ch == 0) return false;
  if ((U.xsize + U.n - 1) / U.n != U.cw || (U.ysize + U.n - 1) / U.n != U.ch) return false;  // (every store is inside W x H)
  FilterParams q = p;
  if (planes_out) {
    q.out = planes_out;
    q.out_stride = planes_ns;
    q.out_plane_stride = planes_nplane;
    output_kind = JXLHIP_OUT_XYB_PLANAR;
  }
  if (U.n == 2) LaunchN<2>(U, q, output_kind, st);
  else if (U.n == 4) LaunchN<4>(U, q, output_kind, st);
  else if (U.n == 8) LaunchN<8>(U, q, output_kind, st);
  else return false;
  return true;
}

}  // namespace jxlhip
