// kernels_dc_upsample.hip -- DC-only groups of a partially received frame (jxlhip_set_dc_only_groups) on gfx950: the DC
// samples of an AC group none of whose passes has arrived, upsampled 8x into the group's tiles of the three XYB planes.
//
// Replaces (behaviour, not code): lib/jxl/dec_group.cc:730-792 (DecodeGroupImpl's draw of a group without AC: the
// group's DC rectangle with two samples of border, real neighbours across group borders, mirrored at the edges of the
// DC image, through PassesDecoderState::upsampler8x) and lib/jxl/render_pipeline/stage_upsampling.cc:147-276 (the
// neighbourhood's minimum / maximum, the 25-tap sum, the clamp).
//
// One kernel, k_dc_upsample8, between phase 1 and the filter launch.  A DC sample becomes one 8 x 8 tile of the
// block-major planes: 64 floats, 256 contiguous bytes, its output pixel (ox, oy) at float oy * 8 + ox -- the index of
// the kernel that makes it.  16 lanes take a tile: lane l of them owns floats 4l .. 4l + 3, so its four kernels are
// 4l .. 4l + 3 and its 4 x 25 weights are 25 aligned float4 of the tap-major table (DcUpsampleWeights), loaded once
// and kept in registers (they differ by lane: no SGPRs as in k_upsample).  A wave takes four horizontally adjacent
// tiles per step, so every store instruction of a wave writes 1 KB contiguous per plane: eight whole 128-byte lines,
// each written once, by one instruction.  A workgroup of four waves takes kBand DC rows of one masked group: the rows
// plus the two-sample border of the three DC planes go into LDS (5.2 KB), mirrored at the edge of the DC image
// (repeatedly for images narrower than the border); the 16 lanes of a tile read the same 25 addresses (a broadcast),
// the four tiles of a wave four neighbouring ones.  The sum is the reference's: three accumulators over taps i, i + 1,
// i + 2, fused multiply-adds, (acc1 + acc2) + acc0, clamped to the neighbourhood's range.  Unmasked groups are not
// touched: their workgroups leave at once.  Indices are 32-bit (LaunchDcUpsample8 refuses planes beyond them).
#include "dev_common.h"
#include "kernels.h"

namespace jxlhip {

namespace {

constexpr int kBand = 8;  // DC rows per workgroup: a group's 32 rows give four workgroups (2040 on an 8K frame)
constexpr int kLW = 32 + 4, kLH = kBand + 4;

struct DcUpsampleArgs {
  uint32_t xsb, ysb, xsg;     // the DC image, groups per row
  uint32_t tile_stride;       // tiles per tile row of the planes
  uint32_t tile_row0;         // tile row of block row 0
  uint32_t plane_floats;      // floats between the planes of xyb
  const float* dc[3];         // xsb floats per row
  float* xyb;                 // plane X
  const uint8_t* mask;        // one byte per group
  const float* weights;       // [25][64], 16-byte aligned
};

__device__ __forceinline__ int MirrorN(int x, int n) {  // image_ops.h:184-196
  while (x < 0 || x >= n) x = x < 0 ? -x - 1 : 2 * n - 1 - x;
  return x;
}

typedef float f4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void k_dc_upsample8(DcUpsampleArgs A) {
  __shared__ float t[3][kLH * kLW];
  const uint32_t g = blockIdx.x;
  if (A.mask[g] == 0) return;  // (the whole workgroup)
  const int XS = (int)A.xsb, YS = (int)A.ysb;
  const int bx0 = (int)(g % A.xsg) * 32, by0 = (int)(g / A.xsg) * 32 + (int)blockIdx.y * kBand;
  if (by0 >= YS) return;
  const int gw = min(32, XS - bx0), gh = min(kBand, YS - by0);
  for (int i = threadIdx.x; i < kLH * kLW; i += 256) {
    const int ly = i / kLW, lx = i - ly * kLW;
    const uint32_t o = (uint32_t)MirrorN(by0 - 2 + ly, YS) * A.xsb + (uint32_t)MirrorN(bx0 - 2 + lx, XS);
    t[0][i] = A.dc[0][o];
    t[1][i] = A.dc[1][o];
    t[2][i] = A.dc[2][o];
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = lane >> 4, l = lane & 15;
  f4 w[25];  // w[i] = tap i of kernels 4l .. 4l + 3
#pragma unroll
  for (int i = 0; i < 25; i++) w[i] = ((const f4*)A.weights)[i * 16 + l];
  __syncthreads();
  const int nq = (gw + 3) >> 2;  // steps of four tiles per DC row
#pragma unroll 1
  for (int it = wave; it < gh * nq; it += 4) {
    const int ry = it / nq, tx = (it - ry * nq) * 4 + q;
    const bool active = tx < gw;
    const int lx = active ? tx : 0;  // (a lane beyond the row computes tile 0 again and stores nothing)
    const uint32_t tile = ((uint32_t)(by0 + ry) + A.tile_row0) * A.tile_stride + (uint32_t)(bx0 + tx);
#pragma unroll 1
    for (int c = 0; c < 3; c++) {
      const float* tc = &t[c][ry * kLW + lx];
      float v[25];
#pragma unroll
      for (int i = 0; i < 25; i++) v[i] = tc[(i / 5) * kLW + i % 5];
      float lo = v[0], hi = v[0];
#pragma unroll
      for (int i = 1; i < 25; i++) {
        lo = __builtin_fminf(lo, v[i]);
        hi = __builtin_fmaxf(hi, v[i]);
      }
      // UpsamplingStage::ProcessRowImpl (stage_upsampling.cc:249-261), four kernels at a time
      f4 a0 = v[0] * w[0], a1 = v[1] * w[1], a2 = v[2] * w[2];
#pragma unroll
      for (int i = 3; i < 24; i += 3) {
        a0 = __builtin_elementwise_fma(f4{v[i], v[i], v[i], v[i]}, w[i], a0);
        a1 = __builtin_elementwise_fma(f4{v[i + 1], v[i + 1], v[i + 1], v[i + 1]}, w[i + 1], a1);
        a2 = __builtin_elementwise_fma(f4{v[i + 2], v[i + 2], v[i + 2], v[i + 2]}, w[i + 2], a2);
      }
      a0 = __builtin_elementwise_fma(f4{v[24], v[24], v[24], v[24]}, w[24], a0);
      const f4 s = (a1 + a2) + a0;
      f4 r;
      r.x = __builtin_fminf(__builtin_fmaxf(s.x, lo), hi);
      r.y = __builtin_fminf(__builtin_fmaxf(s.y, lo), hi);
      r.z = __builtin_fminf(__builtin_fmaxf(s.z, lo), hi);
      r.w = __builtin_fminf(__builtin_fmaxf(s.w, lo), hi);
      if (active) *(f4*)(A.xyb + ((uint32_t)c * A.plane_floats + tile * 64u + 4u * (uint32_t)l)) = r;
    }
  }
}

}  // namespace

void DcUpsampleWeights(const float* kernels, float* tap_major) {
  for (int k = 0; k < 64; k++)
    for (int i = 0; i < 25; i++) tap_major[i * 64 + k] = kernels[k * 25 + i];
}

bool LaunchDcUpsample8(const DevFrame& f, const uint8_t* mask, const float* weights, hipStream_t st) {
  if (f.group_y0 != 0 || f.group_rows != f.ysg || f.plane_y0 != -8 || f.linear_stride != 0) return false;  // whole frames
  const size_t plane = (size_t)f.plane_tile_rows * f.tile_stride * 64;
  if (f.xyb[1] != f.xyb[0] + plane || f.xyb[2] != f.xyb[0] + 2 * plane) return false;
  if (3 * plane >= ((size_t)1 << 32) || (size_t)f.xsb * f.ysb >= ((size_t)1 << 32)) return false;  // 32-bit indices
  if (f.ysb + 1 > f.plane_tile_rows || f.xsb > f.tile_stride) return false;                          // every tile inside the planes
  if (((uintptr_t)f.xyb[0] & 15) || ((uintptr_t)weights & 15)) return false;
  DcUpsampleArgs A;
  A.xsb = f.xsb;
  A.ysb = f.ysb;
  A.xsg = f.xsg;
  A.tile_stride = f.tile_stride;
  A.tile_row0 = 1;
  A.plane_floats = (uint32_t)plane;
  for (int c = 0; c < 3; c++) A.dc[c] = f.dc[c];
  A.xyb = f.xyb[0];
  A.mask = mask;
  A.weights = weights;
  hipLaunchKernelGGL(k_dc_upsample8, dim3(f.xsg * f.ysg, 32 / kBand), dim3(256), 0, st, A);
  return true;
}

}  // namespace jxlhip
