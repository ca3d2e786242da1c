// kernels_blend_ec.hip -- frame blending on an image with extra channels (alpha, depth, ...) on gfx950: what
// kernels_blend.hip does for the colour alone, with the extra channels blended beside it and the two blend modes that
// mean something only with alpha, kBlend and kAlphaWeightedAdd, in full.
//
// Replaces (behaviour, not code): lib/jxl/blending.cc:42-190 (PerformBlending, all of it), lib/jxl/alpha.cc:18-93
// (PerformAlphaBlending in both forms, PerformAlphaWeightedAdd, PerformMulBlending),
// lib/jxl/render_pipeline/stage_blending.cc (ProcessRow, ProcessPaddingRow: every extra channel has a source slot of
// its own) and the save of dec_frame.cc:870-885, which saves the extra channels with the colour.
//
// One kernel, k_ec_blend, with k_blend's geometry: a thread takes four horizontally adjacent canvas pixels, the colour
// as three 16-byte vectors each of source canvas, staged frame and save slot, and every extra channel (up to four) as
// one more vector of its source plane and one of its staged plane.  The planes are planar float, rows padded to four
// pixels (EcStride); the staged ones start (x0 mod 4) pixels in, like the staged colour, so every vector is 16-byte
// aligned at any origin.  The grid is LaunchBlend's.  No LDS.
//
// Per pixel inside the frame's rectangle, in the reference's order:
//   1. every extra channel's background and foreground are read first: the alpha every blend below sees is the one
//      from BEFORE the blend;
//   2. extra channel i is blended with its own (mode, alpha_channel, clamp): kReplace fg, kAdd bg + fg, kMul
//      bg * fg (fg clamped with the flag), kBlend = PerformAlphaBlending's single-channel form (the channel that is
//      its own alpha channel becomes 1 - (1 - fa) * (1 - bga)), kAlphaWeightedAdd = bg + fg * fa (its own alpha
//      channel: bg);
//   3. the colour is blended with the colour's BlendingInfo; kBlend and kAlphaWeightedAdd take the alpha of
//      color_alpha, whose background comes from THAT channel's source slot, premultiplied or straight by that channel's
//      alpha_associated; new_a <= 0 gives a reciprocal of 0; colour kBlend writes new_a over whatever step 2 left in
//      the alpha channel (blend_weighted's output row is tmp.Row(3 + alpha));
//   4. without a channel of type alpha, colour kBlend is fg and kAlphaWeightedAdd bg + fg.
// Outside the rectangle every channel is its own background; an empty slot is zeroes.  Every expression is float32 in
// the reference's operation order (the unit is built with -ffp-contract=off; 1.f / new_a is the correctly rounded
// division), so the result equals the reference's row loops bit for bit.
//
// Modes, clamps, alpha indices and premultiplied flags are launch arguments: the branches on them are scalar, and an
// alpha channel is picked out of the four vectors with selects on its index, never by indexing registers.  A thread
// reads every extra-channel sample it has before it stores the first blended plane, and its colour samples before it
// stores colour; colour canvases and planes share no memory, so the save slot may be the source of the colour or of any
// channel.  (Reading the colour behind the planes' stores keeps its 24 floats from being live beside the planes' 32: 94 /
// 96 / 111 VGPRs, four to five waves per SIMD, instead of 102 / 105 / 123.)
// A 4-channel packed output takes its fourth sample from the blended plane of the image's first alpha channel: the
// thread has just stored those four samples (dst[out_alpha]), and emit.h reads them back through FilterParams::alpha
// as it reads a frame's alpha plane anywhere else.
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

// the four samples of plane `i` (launch-uniform, 0..3) out of four planes' worth that live in registers: selects on the
// index, never an indexed register
__device__ __forceinline__ void PickFour(uint32_t i, const float (&s)[4][4], float (&out)[4]) {
#pragma unroll
  for (int k = 0; k < 4; k++) out[k] = i == 0 ? s[0][k] : (i == 1 ? s[1][k] : (i == 2 ? s[2][k] : s[3][k]));
}

// What a blend takes from its alpha channel, for four pixels (alpha.cc:18-65): the foreground alpha after the clamp,
// the background alpha, and -- for kBlend -- the new alpha and, in the straight form, its reciprocal (0 where the new
// alpha is not positive; 1.f / new_a is the correctly rounded division)
struct AlphaTerms {
  float fa[4], bga[4], new_a[4], rnew_a[4];
};
__device__ __forceinline__ void MakeAlphaTerms(uint32_t ai, bool clamp, bool blend, bool straight, const float (&efg)[4][4],
                                               const float (&ebg)[4][4], AlphaTerms& t) {
  PickFour(ai, efg, t.fa);
  PickFour(ai, ebg, t.bga);
  if (clamp) {
#pragma unroll
    for (int k = 0; k < 4; k++) t.fa[k] = Clamp01(t.fa[k]);
  }
#pragma unroll
  for (int k = 0; k < 4; k++) t.new_a[k] = t.rnew_a[k] = 0.0f;
  if (blend) {
#pragma unroll
    for (int k = 0; k < 4; k++) t.new_a[k] = 1.f - (1.f - t.fa[k]) * (1.f - t.bga[k]);
    if (straight) {
#pragma unroll
      for (int k = 0; k < 4; k++) t.rnew_a[k] = t.new_a[k] > 0 ? 1.f / t.new_a[k] : 0.f;
    }
  }
}

// One channel's four samples blended (blending.cc:58-184 with alpha.cc's row loops): every branch is on a launch
// argument and encloses the loop over the pixels.  self: the channel is its own alpha channel.
__device__ __forceinline__ void BlendFour(uint32_t mode, bool clamp, bool self, bool premul, const float (&b)[4],
                                          const float (&f)[4], const AlphaTerms& t, float (&r)[4]) {
  if (mode == JXLHIP_BLEND_REPLACE) {
#pragma unroll
    for (int k = 0; k < 4; k++) r[k] = f[k];
  } else if (mode == JXLHIP_BLEND_ADD) {
#pragma unroll
    for (int k = 0; k < 4; k++) r[k] = b[k] + f[k];
  } else if (mode == JXLHIP_BLEND_MUL) {
    if (clamp) {
#pragma unroll
      for (int k = 0; k < 4; k++) r[k] = b[k] * Clamp01(f[k]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++) r[k] = b[k] * f[k];
    }
  } else if (mode == JXLHIP_BLEND_BLEND) {
    if (self) {
#pragma unroll
      for (int k = 0; k < 4; k++) r[k] = t.new_a[k];
    } else if (premul) {
#pragma unroll
      for (int k = 0; k < 4; k++) r[k] = f[k] + b[k] * (1.f - t.fa[k]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++) r[k] = (f[k] * t.fa[k] + b[k] * t.bga[k] * (1.f - t.fa[k])) * t.rnew_a[k];
    }
  } else {  // kAlphaWeightedAdd
    if (self) {
#pragma unroll
      for (int k = 0; k < 4; k++) r[k] = b[k];
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++) r[k] = b[k] + f[k] * t.fa[k];
    }
  }
}

template <int OUTK>
__global__ __launch_bounds__(256) void k_ec_blend(BlendEcArgs E, FilterParams P) {
  const BlendArgs& A = E.B;
  // blockIdx.x: 256 groups of a row; blockIdx.y: the first of the rows this block takes, gridDim.y apart
  const uint32_t g = A.gx0 + blockIdx.x * 256u + threadIdx.x;
  if (g >= A.gx1) return;
  // (step 4: what the colour's mode comes to without a channel of type alpha)
  const uint32_t cm = E.has_alpha ? E.color_mode
                                  : (E.color_mode == JXLHIP_BLEND_BLEND              ? (uint32_t)JXLHIP_BLEND_REPLACE
                                     : E.color_mode == JXLHIP_BLEND_ALPHA_WEIGHTED_ADD ? (uint32_t)JXLHIP_BLEND_ADD
                                                                                       : E.color_mode);
#pragma unroll 1
  for (uint32_t yy = A.y0 + blockIdx.y; yy < A.y1; yy += gridDim.y) {
    const int y = (int)yy;
    // (as in k_blend: what the packed tail derives from x must not be hoisted out of the loop and held in registers)
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
    // ---- 1. the extra channels' samples, background and foreground: the alpha every blend below sees
    float ebg[4][4], efg[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      f4 a = f4{0.0f, 0.0f, 0.0f, 0.0f};  // (zeroes_ of the reference's stage)
      if ((uint32_t)i < E.num_ec && E.src[i]) a = *(const f4*)(E.src[i] + (size_t)y * E.src_stride[i] + 4 * (size_t)g);
#pragma unroll
      for (int k = 0; k < 4; k++) ebg[i][k] = a[k];
    }
    // (x - fg_xa is a non-negative multiple of 4 where any_in, and the group lies inside the padded staged rows)
    const size_t frow = (size_t)(y - A.fg_y0), fcol = (size_t)(x - A.fg_xa);
    // what the colour takes from its alpha channel
    const bool color_premul = (E.color_alpha == 0   ? E.premul[0]
                               : E.color_alpha == 1 ? E.premul[1]
                               : E.color_alpha == 2 ? E.premul[2]
                                                    : E.premul[3]) != 0;
    AlphaTerms ct;
    if (any_in) {
#pragma unroll
      for (int i = 0; i < 4; i++) {
        f4 a = f4{0.0f, 0.0f, 0.0f, 0.0f};
        if ((uint32_t)i < E.num_ec) a = *(const f4*)(E.fg[i] + frow * E.fg_stride + fcol);
#pragma unroll
        for (int k = 0; k < 4; k++) efg[i][k] = a[k];
      }
      MakeAlphaTerms(E.color_alpha, E.color_clamp != 0, cm == JXLHIP_BLEND_BLEND, !color_premul, efg, ebg, ct);
    }
    // ---- 2. the extra channels, each with its own mode and the PRE-blend alpha of its alpha channel; stored at once (a
    // plane of the save slot can only be the source of the same channel, and all of those have been read)
#pragma unroll
    for (int i = 0; i < 4; i++) {
      if ((uint32_t)i >= E.num_ec) continue;
      float ev[4];
#pragma unroll
      for (int k = 0; k < 4; k++) ev[k] = ebg[i][k];
      if (any_in) {
        float r[4];
        if (cm == JXLHIP_BLEND_BLEND && E.color_alpha == (uint32_t)i) {
          // (colour kBlend writes the new alpha into its alpha channel, over this channel's own result: step 3)
#pragma unroll
          for (int k = 0; k < 4; k++) r[k] = ct.new_a[k];
        } else {
          const uint32_t mode = E.mode[i], ai = E.alpha[i];
          const bool clamp = E.clamp[i] != 0, self = ai == (uint32_t)i;
          const bool premul = (ai == 0 ? E.premul[0] : ai == 1 ? E.premul[1] : ai == 2 ? E.premul[2] : E.premul[3]) != 0;
          AlphaTerms t;
          MakeAlphaTerms(ai, clamp, mode == JXLHIP_BLEND_BLEND, !self && !premul, efg, ebg, t);
          BlendFour(mode, clamp, self, premul, ebg[i], efg[i], t, r);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) ev[k] = in[k] ? r[k] : ev[k];
      }
      if (A.dst_all || any_in) *(f4*)(E.dst[i] + (size_t)y * E.dst_stride + 4 * (size_t)g) = f4{ev[0], ev[1], ev[2], ev[3]};
    }
    // ---- 3. the colour (its canvases share no memory with the planes: read only now, to keep the registers few)
    float v[12];
    if (A.src && !(all_in && cm == JXLHIP_BLEND_REPLACE)) {
      const f4* s = (const f4*)(A.src + (size_t)y * A.src_stride + 12 * (size_t)g);
      const f4 a = s[0], b = s[1], c = s[2];
#pragma unroll
      for (int k = 0; k < 4; k++) v[k] = a[k], v[4 + k] = b[k], v[8 + k] = c[k];
    } else {
#pragma unroll
      for (int k = 0; k < 12; k++) v[k] = 0.0f;
    }
    if (any_in) {
      const f4* s = (const f4*)(A.fg + frow * A.fg_stride + 3 * fcol);
      const f4 fa4 = s[0], fb4 = s[1], fc4 = s[2];
      float fg[12];
#pragma unroll
      for (int k = 0; k < 4; k++) fg[k] = fa4[k], fg[4 + k] = fb4[k], fg[8 + k] = fc4[k];
#pragma unroll
      for (int c = 0; c < 3; c++) {
        float b[4], f[4], r[4];
#pragma unroll
        for (int k = 0; k < 4; k++) b[k] = v[3 * k + c], f[k] = fg[3 * k + c];
        BlendFour(cm, E.color_clamp != 0, false, color_premul, b, f, ct, r);
#pragma unroll
        for (int k = 0; k < 4; k++) v[3 * k + c] = in[k] ? r[k] : b[k];
      }
    }
    // ---- the colour's stores: the save slot, then the caller's output
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

bool LaunchBlendEc(const BlendEcArgs& E, const FilterParams& p, int output_kind, hipStream_t st) {
  const BlendArgs& A = E.B;
  if (output_kind < 0 || output_kind > 2 || A.W == 0 || A.H == 0 || E.num_ec == 0 || E.num_ec > 4 || E.color_mode > JXLHIP_BLEND_MUL ||
      E.color_alpha >= E.num_ec || E.out_alpha >= (int32_t)E.num_ec)
    return false;
  for (uint32_t i = 0; i < E.num_ec; i++)
    if (E.mode[i] > JXLHIP_BLEND_MUL || E.alpha[i] >= E.num_ec || !E.fg[i] || !E.dst[i]) return false;
  if (output_kind == JXLHIP_OUT_PACKED && p.fmt.num_channels == 4 && E.out_alpha >= 0 &&
      (p.alpha != E.dst[E.out_alpha] || p.alpha_stride != E.dst_stride))
    return false;
  if (A.gx1 <= A.gx0 || A.y1 <= A.y0) return true;  // nothing to visit
  if (A.gx1 > (A.W + 3) / 4 || A.y1 > A.H) return false;
  // memory-bound: at most eight blocks per compute unit; a block takes 256 groups of a row and strides over the rows
  const unsigned bx = (A.gx1 - A.gx0 + 255) / 256;
  const unsigned by = std::min<unsigned>(A.y1 - A.y0, std::max<unsigned>(1u, DeviceCus() * 8 / bx));
  const dim3 blocks(bx, by);
  if (output_kind == 0)
    hipLaunchKernelGGL((k_ec_blend<0>), blocks, dim3(256), 0, st, E, p);
  else if (output_kind == JXLHIP_OUT_LINEAR_RGB_F32)
    hipLaunchKernelGGL((k_ec_blend<JXLHIP_OUT_LINEAR_RGB_F32>), blocks, dim3(256), 0, st, E, p);
  else
    hipLaunchKernelGGL((k_ec_blend<JXLHIP_OUT_PACKED>), blocks, dim3(256), 0, st, E, p);
  return true;
}

}  // namespace jxlhip
