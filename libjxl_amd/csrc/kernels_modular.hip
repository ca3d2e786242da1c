// kernels_modular.hip -- the device stage of a regular Modular frame (jxlhip_decode_modular_frame) on gfx950: the three
// integer planes the host front-end leaves (jxlhip_modular_image_decode) become the caller's pixels.
//
// Replaces (behaviour, not code): what is left of lib/jxl/modular/transform/rct.cc (InvRCT, :29-148) once the host has
// decided which transform lists stay (include/jxl_hip_frame.h says how), and ModularImageToDecodedRect's int -> float of a
// frame that is not XYB (lib/jxl/dec_modular.cc:75-104,584-586,656-688: one IEEE multiply by
// (float)(1.0 / (2^bits - 1))).  The samples are the original's, encoded as the original was: the output tail is emit.h's
// sample conversion (PackSamples) with the IDENTITY transfer -- LaunchModularEmit hands it a format whose transfer is
// JXLHIP_TF_LINEAR.
//
// One kernel, k_modular_emit.  Pure streaming: a lane owns a run of kRun = 8 consecutive pixels of a row, read with
// 16-byte loads -- one per plane of int16 samples, two of int32 (taken as two pieces of four pixels) --, a block 2048
// columns, and the blocks of a grid column stride over the rows.  Group dimensions are multiples of 128, so a run lies in
// ONE group: its RCT program (and the global one) is fetched and taken apart once per run.  A run that crosses the right
// edge of the frame is the scalar tail: sample by sample, pixel by pixel.  No LDS, no scratch, at most 64 registers
// (eight waves to the SIMD; tests/test_modular_kernel_resources.py).  Per pixel: widen to int32; undo the group's
// program, then the global one, each last-listed first, in arithmetic that wraps; convert; pack.  Instantiations per
// sample type: float RGB (96 contiguous bytes per run), the general packed tail FmtSel<-1> (pairs of pixels through
// StorePackedPair), and 8-bit RGB / RGBA with the format fixed at compile time and the run stored as 24 / 32 contiguous
// bytes (taken when the output rows are 4-byte aligned).
// Below it k_modular_planes: the same stage for frames with an integer alpha plane and for grey frames
// (jxlhip_decode_modular_channels); RGB without alpha stays k_modular_emit's.
#include "dev_common.h"
#include "emit.h"
#include "kernels.h"

namespace jxlhip {

namespace {

constexpr int kRun = 8;
constexpr int kRunsPerBlock = 256;
constexpr unsigned kMaxGridRows = 1024;

// InvRCT (rct.cc:68-94) on a run, in place: type = 7 * permutation + custom.  The type is the same for the whole run
// (and, away from group borders, the whole wave): it is taken apart once, and the pixels go through straight-line code --
// selects on values that are constant over the run instead of a branch per pixel.
template <int N>
__device__ __forceinline__ void InvRctRun(uint32_t type, int32_t (&s)[3][N]) {
  const uint32_t perm = type / 7u, custom = type - 7u * perm;
  // the three results go to channels perm % 3, (perm + 1 + perm / 3) % 3, (perm + 2 - perm / 3) % 3
  const uint32_t hi = perm >= 3 ? 1u : 0u, t0 = perm - 3u * hi;
  uint32_t t1 = t0 + 1u + hi;
  t1 = t1 >= 3 ? t1 - 3u : t1;
  if (custom == 6) {  // YCoCg
#pragma unroll
    for (int i = 0; i < N; i++) {
      const uint32_t first = (uint32_t)s[0][i], second = (uint32_t)s[1][i], third = (uint32_t)s[2][i];
      const uint32_t tmp = first - (uint32_t)((int32_t)third >> 1);
      const uint32_t b = third + tmp;
      const uint32_t c = tmp - (uint32_t)((int32_t)second >> 1);
      const uint32_t a = c + second;
#pragma unroll
      for (uint32_t o = 0; o < 3; o++) s[o][i] = (int32_t)(t0 == o ? a : (t1 == o ? b : c));
    }
  } else {
    const uint32_t add3 = (custom & 1u) ? ~0u : 0u, how = custom >> 1;
    const uint32_t add_first = how == 1 ? ~0u : 0u, add_avg = how == 2 ? ~0u : 0u;
#pragma unroll
    for (int i = 0; i < N; i++) {
      const uint32_t a = (uint32_t)s[0][i], second = (uint32_t)s[1][i], third = (uint32_t)s[2][i];
      const uint32_t c = third + (a & add3);
      const uint32_t b = second + (a & add_first) + ((uint32_t)((int32_t)(a + c) >> 1) & add_avg);
#pragma unroll
      for (uint32_t o = 0; o < 3; o++) s[o][i] = (int32_t)(t0 == o ? a : (t1 == o ? b : c));
    }
  }
}

// the group's program, then the global one, each last-listed first
template <int N>
__device__ __forceinline__ void UndoPrograms(uint32_t group_prog, uint32_t global_prog, int32_t (&s)[3][N]) {
  const uint32_t types = (group_prog >> 8) | ((group_prog & 0xFFu) << 8) | ((global_prog >> 8) << 16) | ((global_prog & 0xFFu) << 24);
#pragma unroll 1
  for (uint32_t k = 0; k < 32 && (types >> k) != 0; k += 8) {
    const uint32_t type = (types >> k) & 0xFFu;
    if (type != 0) InvRctRun(type, s);
  }
}

// S: int16_t / int32_t planes.  FMT: the packed format fixed at compile time (FormatId), -1 = read from the launch parameters.
// (amdgpu_waves_per_eu(8) = 64 registers: left alone, the scheduler spreads a run's dither-table addresses and format
// selects over up to 190 -- for a kernel that waits on memory and is hidden by nothing but its resident waves)
template <typename S, int OUTK, int FMT>
__global__ __launch_bounds__(kRunsPerBlock) __attribute__((amdgpu_waves_per_eu(8))) void k_modular_emit(ModularEmitArgs A, FilterParams P) {
  typedef uint32_t u2 __attribute__((ext_vector_type(2), aligned(4)));
  typedef uint32_t u4 __attribute__((ext_vector_type(4), aligned(4)));
  typedef int32_t i4 __attribute__((ext_vector_type(4)));
  typedef int16_t s8 __attribute__((ext_vector_type(8)));
  const uint32_t x0 = (uint32_t)kRun * (blockIdx.x * kRunsPerBlock + threadIdx.x);
  if (x0 >= A.xsize) return;
  const bool whole = x0 + kRun <= A.xsize;
  const uint32_t gx = x0 >> A.group_shift;
  const S* const pl0 = (const S*)A.plane[0];
  const S* const pl1 = (const S*)A.plane[1];
  const S* const pl2 = (const S*)A.plane[2];
  for (uint32_t y = blockIdx.y; y < A.ysize; y += gridDim.y) {
    const uint32_t prog = A.group_rct[(size_t)(y >> A.group_shift) * A.xsg + gx];
    const size_t o = (size_t)y * A.ns + x0;  // (A.ns is a multiple of 8: a run starts at a 16-byte boundary)
    char* const orow = (char*)P.out + (size_t)y * P.out_stride;
    if (!whole) {  // the scalar tail: sample by sample, pixel by pixel, the columns the frame still has
      for (uint32_t x = x0; x < A.xsize; x++) {
        const size_t at = o + (x - x0);
        int32_t t[3][1] = {{(int32_t)pl0[at]}, {(int32_t)pl1[at]}, {(int32_t)pl2[at]}};
        UndoPrograms(prog, A.global_rct, t);
        const float rgb[3] = {(float)t[0][0] * A.factor, (float)t[1][0] * A.factor, (float)t[2][0] * A.factor};
        if constexpr (OUTK == JXLHIP_OUT_LINEAR_RGB_F32) {
          uint32_t* d = (uint32_t*)orow + 3u * (size_t)x;
          d[0] = __float_as_uint(rgb[0]);
          d[1] = __float_as_uint(rgb[1]);
          d[2] = __float_as_uint(rgb[2]);
        } else {
          StorePackedPixel<FmtSel<FMT>>(P, P.dither, orow, (int)x, (int)y, rgb);
        }
      }
      continue;
    }
    // a run of int32 samples is taken in two pieces of four pixels (16 bytes per plane each, like the one piece of an
    // int16 run): half the samples are in registers at a time
    constexpr int kPiece = sizeof(S) == 2 ? kRun : kRun / 2;
    constexpr int kNc = (FMT >> 5) & 1 ? 4 : 3;  // (the fixed formats)
    uint32_t w8[2 * kNc];                        // ... their run: 24 / 32 contiguous bytes
#pragma unroll
    for (int k = 0; k < 2 * kNc; k++) w8[k] = 0;
#pragma unroll
    for (int h = 0; h < kRun / kPiece; h++) {
      int32_t s[3][kPiece];
      if constexpr (sizeof(S) == 2) {
        const s8 a = __builtin_nontemporal_load((const s8*)(pl0 + o));
        const s8 b = __builtin_nontemporal_load((const s8*)(pl1 + o));
        const s8 c = __builtin_nontemporal_load((const s8*)(pl2 + o));
#pragma unroll
        for (int i = 0; i < kPiece; i++) s[0][i] = a[i], s[1][i] = b[i], s[2][i] = c[i];
      } else {
        const i4 a = __builtin_nontemporal_load((const i4*)(pl0 + o) + h);
        const i4 b = __builtin_nontemporal_load((const i4*)(pl1 + o) + h);
        const i4 c = __builtin_nontemporal_load((const i4*)(pl2 + o) + h);
#pragma unroll
        for (int i = 0; i < kPiece; i++) s[0][i] = a[i], s[1][i] = b[i], s[2][i] = c[i];
      }
      UndoPrograms(prog, A.global_rct, s);
      const uint32_t xp = x0 + (uint32_t)(h * kPiece);  // the piece's first column
      if constexpr (OUTK == JXLHIP_OUT_LINEAR_RGB_F32) {  // 12 contiguous bytes per pixel
        uint32_t* d = (uint32_t*)orow + 3u * (size_t)xp;
#pragma unroll
        for (int k = 0; k < 3 * kPiece / 4; k++) {  // word 4k + j of the piece is sample (4k + j) % 3 of pixel (4k + j) / 3
          u4 w;
#pragma unroll
          for (int j = 0; j < 4; j++) w[j] = __float_as_uint((float)s[(4 * k + j) % 3][(4 * k + j) / 3] * A.factor);
          __builtin_nontemporal_store(w, (u4*)d + k);
        }
      } else if constexpr (FMT < 0) {
#pragma unroll
        for (int i = 0; i < kPiece; i += 2) {
          const float p0[3] = {(float)s[0][i] * A.factor, (float)s[1][i] * A.factor, (float)s[2][i] * A.factor};
          const float p1[3] = {(float)s[0][i + 1] * A.factor, (float)s[1][i + 1] * A.factor, (float)s[2][i + 1] * A.factor};
          // (the column goes through an empty asm statement: one pair's dither-table addresses and loads cannot be
          // hoisted over the pairs before it -- the run would hold all of them at once, in twice the registers)
          int xi = (int)xp + i;
          asm volatile("" : "+v"(xi)::"memory");
          StorePackedPair<FmtSel<FMT>>(P, P.dither, orow, xi, (int)y, p0, p1);
        }
      } else {  // 8-bit samples, 3 or 4 to the pixel
        static_assert(((FMT >> 3) & 3) == JXLHIP_SAMPLE_U8, "the fixed formats are the 8-bit ones");
        uint32_t* const d = (uint32_t*)(orow + (size_t)x0 * kNc);
#pragma unroll
        for (int j = 0; j < kPiece; j++) {  // byte kNc * i + ch of the run is sample ch of pixel i
          const int i = h * kPiece + j;
          const float rgb[3] = {(float)s[0][j] * A.factor, (float)s[1][j] * A.factor, (float)s[2][j] * A.factor};
          uint32_t q[4];
          int xi = (int)x0 + i;
          asm volatile("" : "+v"(xi)::"memory");  // (as above)
          PackSamples<FmtSel<FMT>>(P, P.dither, xi, (int)y, rgb, q);
#pragma unroll
          for (int ch = 0; ch < kNc; ch++) w8[(kNc * i + ch) / 4] |= q[ch] << (8 * ((kNc * i + ch) % 4));
          // a 16-byte piece of the run goes out as soon as its last byte is in; an RGB run ends on 8 bytes
          if ((kNc * (i + 1)) / 16 > (kNc * i) / 16) {
            const int k = 4 * ((kNc * (i + 1)) / 16 - 1);
            __builtin_nontemporal_store(u4{w8[k], w8[k + 1], w8[k + 2], w8[k + 3]}, (u4*)(d + k));
          }
          if (kNc == 3 && i == kRun - 1) __builtin_nontemporal_store(u2{w8[4], w8[5]}, (u2*)(d + 4));
        }
      }
    }
  }
}

template <typename S>
bool LaunchTyped(const ModularEmitArgs& A, const FilterParams& p, int output_kind, dim3 grid, hipStream_t st) {
  const jxlhip_output_format& o = p.fmt;
  const bool rows4 = (((uintptr_t)p.out | p.out_stride) & 3u) == 0;
  const bool u8 = output_kind == JXLHIP_OUT_PACKED && o.sample_type == JXLHIP_SAMPLE_U8 && o.swap_endianness == 0 && rows4;
  if (output_kind == JXLHIP_OUT_LINEAR_RGB_F32)
    hipLaunchKernelGGL((k_modular_emit<S, JXLHIP_OUT_LINEAR_RGB_F32, -1>), grid, dim3(kRunsPerBlock), 0, st, A, p);
  else if (u8 && o.num_channels == 3)
    hipLaunchKernelGGL((k_modular_emit<S, JXLHIP_OUT_PACKED, FormatId(JXLHIP_TF_LINEAR, JXLHIP_SAMPLE_U8, 3)>), grid, dim3(kRunsPerBlock), 0, st, A, p);
  else if (u8 && o.num_channels == 4)
    hipLaunchKernelGGL((k_modular_emit<S, JXLHIP_OUT_PACKED, FormatId(JXLHIP_TF_LINEAR, JXLHIP_SAMPLE_U8, 4)>), grid, dim3(kRunsPerBlock), 0, st, A, p);
  else if (output_kind == JXLHIP_OUT_PACKED)
    hipLaunchKernelGGL((k_modular_emit<S, JXLHIP_OUT_PACKED, -1>), grid, dim3(kRunsPerBlock), 0, st, A, p);
  else
    return false;
  return true;
}

// ---- k_modular_planes: the sibling of k_modular_emit for the two cases that kernel cannot express -- an integer ALPHA
// plane beside the colour (a fourth 16-byte load per piece; converted with a factor of its own, (float)(1.0 / (2^alpha_bits
// - 1)); packed like a colour channel minus the transfer function: emit.h's forms that take the alpha sample) and a GREY
// image (NC = 1: one colour plane, no programs, the sample replicated into R, G and B as the reference's pipeline carries
// it).  Same shape and budget: a lane owns a run of 8 pixels that never straddles a group, the scalar tail takes the
// right edge, no LDS, no scratch, at most 64 registers.  Three colour planes without alpha never come here.
template <typename S, int NC, bool ALPHA, int OUTK, int FMT>
__global__ __launch_bounds__(kRunsPerBlock) __attribute__((amdgpu_waves_per_eu(8))) void k_modular_planes(ModularPlanesArgs B, FilterParams P) {
  static_assert(NC == 1 || NC == 3, "one colour plane or three");
  static_assert(NC == 1 || ALPHA, "three planes without alpha are k_modular_emit's");
  static_assert(!(ALPHA && OUTK == JXLHIP_OUT_LINEAR_RGB_F32), "three floats have no room for alpha");
  typedef uint32_t u2 __attribute__((ext_vector_type(2), aligned(4)));
  typedef uint32_t u4 __attribute__((ext_vector_type(4), aligned(4)));
  typedef int32_t i4 __attribute__((ext_vector_type(4)));
  typedef int16_t s8 __attribute__((ext_vector_type(8)));
  const ModularEmitArgs& A = B.e;
  const uint32_t x0 = (uint32_t)kRun * (blockIdx.x * kRunsPerBlock + threadIdx.x);
  if (x0 >= A.xsize) return;
  const bool whole = x0 + kRun <= A.xsize;
  const uint32_t gx = x0 >> A.group_shift;
  const S* const pl0 = (const S*)A.plane[0];
  const S* const pl1 = (const S*)A.plane[NC == 3 ? 1 : 0];
  const S* const pl2 = (const S*)A.plane[NC == 3 ? 2 : 0];
  const S* const pa = (const S*)B.alpha;
  for (uint32_t y = blockIdx.y; y < A.ysize; y += gridDim.y) {
    uint32_t prog = 0;
    if constexpr (NC == 3) prog = A.group_rct[(size_t)(y >> A.group_shift) * A.xsg + gx];
    const size_t o = (size_t)y * A.ns + x0;  // (A.ns is a multiple of 8: a run starts at a 16-byte boundary)
    char* const orow = (char*)P.out + (size_t)y * P.out_stride;
    if (!whole) {  // the scalar tail
      for (uint32_t x = x0; x < A.xsize; x++) {
        const size_t at = o + (x - x0);
        float rgb[3];
        if constexpr (NC == 3) {
          int32_t t[3][1] = {{(int32_t)pl0[at]}, {(int32_t)pl1[at]}, {(int32_t)pl2[at]}};
          UndoPrograms(prog, A.global_rct, t);
          rgb[0] = (float)t[0][0] * A.factor, rgb[1] = (float)t[1][0] * A.factor, rgb[2] = (float)t[2][0] * A.factor;
        } else {
          rgb[0] = rgb[1] = rgb[2] = (float)(int32_t)pl0[at] * A.factor;
        }
        float alpha = 1.0f;
        if constexpr (ALPHA) alpha = (float)(int32_t)pa[at] * B.alpha_factor;
        if constexpr (OUTK == JXLHIP_OUT_LINEAR_RGB_F32) {
          uint32_t* d = (uint32_t*)orow + 3u * (size_t)x;
          d[0] = __float_as_uint(rgb[0]);
          d[1] = __float_as_uint(rgb[1]);
          d[2] = __float_as_uint(rgb[2]);
        } else {
          StorePackedPixel<FmtSel<FMT>>(P, P.dither, orow, (int)x, (int)y, rgb, alpha);
        }
      }
      continue;
    }
    constexpr int kPiece = sizeof(S) == 2 ? kRun : kRun / 2;  // (as k_modular_emit: 16 bytes per plane and piece)
    constexpr int kNc = (FMT >> 5) & 1 ? 4 : 3;
    // (three colour planes through the general tail fill the 64 registers on their own -- k_modular_emit's is at 64 --:
    // there the alpha samples come pair by pair, one 4- or 8-byte load behind each pair's column fence, instead of a
    // 16-byte load per piece that would sit in registers through the whole piece)
    constexpr bool kAlphaPerPair = ALPHA && NC == 3 && FMT < 0 && OUTK == JXLHIP_OUT_PACKED;
    uint32_t w8[2 * kNc];
#pragma unroll
    for (int k = 0; k < 2 * kNc; k++) w8[k] = 0;
#pragma unroll
    for (int h = 0; h < kRun / kPiece; h++) {
      int32_t s[NC][kPiece], sa[kPiece];
      if constexpr (sizeof(S) == 2) {
        const s8 a = __builtin_nontemporal_load((const s8*)(pl0 + o));
#pragma unroll
        for (int i = 0; i < kPiece; i++) s[0][i] = a[i];
        if constexpr (NC == 3) {
          const s8 b = __builtin_nontemporal_load((const s8*)(pl1 + o));
          const s8 c = __builtin_nontemporal_load((const s8*)(pl2 + o));
#pragma unroll
          for (int i = 0; i < kPiece; i++) s[NC - 2][i] = b[i], s[NC - 1][i] = c[i];
        }
        if constexpr (ALPHA && !kAlphaPerPair) {
          const s8 d = __builtin_nontemporal_load((const s8*)(pa + o));
#pragma unroll
          for (int i = 0; i < kPiece; i++) sa[i] = d[i];
        }
      } else {
        const i4 a = __builtin_nontemporal_load((const i4*)(pl0 + o) + h);
#pragma unroll
        for (int i = 0; i < kPiece; i++) s[0][i] = a[i];
        if constexpr (NC == 3) {
          const i4 b = __builtin_nontemporal_load((const i4*)(pl1 + o) + h);
          const i4 c = __builtin_nontemporal_load((const i4*)(pl2 + o) + h);
#pragma unroll
          for (int i = 0; i < kPiece; i++) s[NC - 2][i] = b[i], s[NC - 1][i] = c[i];
        }
        if constexpr (ALPHA && !kAlphaPerPair) {
          const i4 d = __builtin_nontemporal_load((const i4*)(pa + o) + h);
#pragma unroll
          for (int i = 0; i < kPiece; i++) sa[i] = d[i];
        }
      }
      if constexpr (NC == 3) UndoPrograms(prog, A.global_rct, s);
      // pixel i of the piece: its three colour samples (a grey sample three times) and its alpha
      auto colour = [&](int i, float* rgb) {
#pragma unroll
        for (int ch = 0; ch < 3; ch++) rgb[ch] = (float)s[NC == 3 ? ch : 0][i] * A.factor;
      };
      auto alpha_of = [&](int i) { return ALPHA ? (float)sa[i] * B.alpha_factor : 1.0f; };
      const uint32_t xp = x0 + (uint32_t)(h * kPiece);  // the piece's first column
      if constexpr (OUTK == JXLHIP_OUT_LINEAR_RGB_F32) {  // 12 contiguous bytes per pixel
        uint32_t* d = (uint32_t*)orow + 3u * (size_t)xp;
#pragma unroll
        for (int k = 0; k < 3 * kPiece / 4; k++) {  // word 4k + j of the piece is sample (4k + j) % 3 of pixel (4k + j) / 3
          u4 w;
#pragma unroll
          for (int j = 0; j < 4; j++) w[j] = __float_as_uint((float)s[NC == 3 ? (4 * k + j) % 3 : 0][(4 * k + j) / 3] * A.factor);
          __builtin_nontemporal_store(w, (u4*)d + k);
        }
      } else if constexpr (FMT < 0) {
#pragma unroll
        for (int i = 0; i < kPiece; i += 2) {
          float p0[3], p1[3];
          colour(i, p0);
          colour(i + 1, p1);
          int xi = (int)xp + i;
          asm volatile("" : "+v"(xi)::"memory");  // (as k_modular_emit: one pair's dither addresses at a time)
          if constexpr (kAlphaPerPair) {
            typedef S pair_t __attribute__((ext_vector_type(2)));
            const pair_t d = __builtin_nontemporal_load((const pair_t*)(pa + (size_t)y * A.ns + (uint32_t)xi));
            StorePackedPair<FmtSel<FMT>>(P, P.dither, orow, xi, (int)y, p0, p1, (float)(int32_t)d[0] * B.alpha_factor,
                                         (float)(int32_t)d[1] * B.alpha_factor);
          } else {
            StorePackedPair<FmtSel<FMT>>(P, P.dither, orow, xi, (int)y, p0, p1, alpha_of(i), alpha_of(i + 1));
          }
        }
      } else {  // 8-bit samples, 3 or 4 to the pixel: the run as 24 / 32 contiguous bytes
        static_assert(((FMT >> 3) & 3) == JXLHIP_SAMPLE_U8, "the fixed formats are the 8-bit ones");
        uint32_t* const d = (uint32_t*)(orow + (size_t)x0 * kNc);
#pragma unroll
        for (int j = 0; j < kPiece; j++) {  // byte kNc * i + ch of the run is sample ch of pixel i
          const int i = h * kPiece + j;
          float rgb[3];
          colour(j, rgb);
          uint32_t q[4];
          int xi = (int)x0 + i;
          asm volatile("" : "+v"(xi)::"memory");  // (as above)
          PackSamples<FmtSel<FMT>>(P, P.dither, xi, (int)y, rgb, alpha_of(j), q);
#pragma unroll
          for (int ch = 0; ch < kNc; ch++) w8[(kNc * i + ch) / 4] |= q[ch] << (8 * ((kNc * i + ch) % 4));
          if ((kNc * (i + 1)) / 16 > (kNc * i) / 16) {  // a 16-byte piece of the run goes out as soon as it is full
            const int k = 4 * ((kNc * (i + 1)) / 16 - 1);
            __builtin_nontemporal_store(u4{w8[k], w8[k + 1], w8[k + 2], w8[k + 3]}, (u4*)(d + k));
          }
          if (kNc == 3 && i == kRun - 1) __builtin_nontemporal_store(u2{w8[4], w8[5]}, (u2*)(d + 4));
        }
      }
    }
  }
}

// The launch table: every k_modular_planes instantiation, one X per line -- sample type, colour planes, alpha, output
// kind, format (-1 = the general packed tail, which takes every sample type, 3 or 4 channels, dither and endianness).
// {int16, int32} x {grey, grey + alpha, RGB + alpha}; the float kind drops alpha, so only grey comes here for it; the
// fixed 8-bit tails for what users hit: RGB + alpha to RGBA8 from both sample types, and 8-bit grey images (int16
// planes) to RGB8 / RGBA8.  A case without a fixed tail of its own goes through the general one.
constexpr int kRgb8 = FormatId(JXLHIP_TF_LINEAR, JXLHIP_SAMPLE_U8, 3), kRgba8 = FormatId(JXLHIP_TF_LINEAR, JXLHIP_SAMPLE_U8, 4);
#define JXLHIP_MODULAR_PLANES_KERNELS(X)               \
  X(int16_t, 1, false, JXLHIP_OUT_LINEAR_RGB_F32, -1)  \
  X(int32_t, 1, false, JXLHIP_OUT_LINEAR_RGB_F32, -1)  \
  X(int16_t, 1, false, JXLHIP_OUT_PACKED, -1)          \
  X(int32_t, 1, false, JXLHIP_OUT_PACKED, -1)          \
  X(int16_t, 1, true, JXLHIP_OUT_PACKED, -1)           \
  X(int32_t, 1, true, JXLHIP_OUT_PACKED, -1)           \
  X(int16_t, 3, true, JXLHIP_OUT_PACKED, -1)           \
  X(int32_t, 3, true, JXLHIP_OUT_PACKED, -1)           \
  X(int16_t, 3, true, JXLHIP_OUT_PACKED, kRgba8)       \
  X(int32_t, 3, true, JXLHIP_OUT_PACKED, kRgba8)       \
  X(int16_t, 1, false, JXLHIP_OUT_PACKED, kRgb8)       \
  X(int16_t, 1, false, JXLHIP_OUT_PACKED, kRgba8)      \
  X(int16_t, 1, true, JXLHIP_OUT_PACKED, kRgba8)

struct PlanesKernel {
  uint32_t sample_type, num_color;
  bool alpha;
  int output_kind, fmt;
  void (*kernel)(ModularPlanesArgs, FilterParams);
};
#define JXLHIP_X(S, NC, ALPHA, OUTK, FMT) \
  {sizeof(S) == 2 ? JXLHIP_MODULAR_I16 : JXLHIP_MODULAR_I32, NC, ALPHA, OUTK, FMT, k_modular_planes<S, NC, ALPHA, OUTK, FMT>},
const PlanesKernel kPlanesKernels[] = {JXLHIP_MODULAR_PLANES_KERNELS(JXLHIP_X)};
#undef JXLHIP_X

}  // namespace

bool LaunchModularEmit(const ModularEmitArgs& A, const FilterParams& fp, int output_kind, hipStream_t st) {
  if (A.xsize == 0 || A.ysize == 0 || A.ns < ((A.xsize + 7u) & ~7u) || (A.ns & 7u) || A.group_shift < 7 || A.group_shift > 10 ||
      A.xsg != ((A.xsize - 1) >> A.group_shift) + 1 || !A.plane[0] || !A.plane[1] || !A.plane[2] || !A.group_rct || !fp.out ||
      A.sample_type > JXLHIP_MODULAR_I32)
    return false;
  for (int c = 0; c < 3; c++)
    if ((uintptr_t)A.plane[c] & 15u) return false;
  if (output_kind == JXLHIP_OUT_LINEAR_RGB_F32 && ((((uintptr_t)fp.out | fp.out_stride) & 3u) != 0)) return false;
  FilterParams p = fp;
  p.fmt.transfer = JXLHIP_TF_LINEAR;  // the identity hand-over: the samples are encoded already
  const uint32_t runs = (A.xsize + kRun - 1) / kRun;
  const dim3 grid((runs + kRunsPerBlock - 1) / kRunsPerBlock, std::min(A.ysize, kMaxGridRows));
  return A.sample_type == JXLHIP_MODULAR_I16 ? LaunchTyped<int16_t>(A, p, output_kind, grid, st)
                                             : LaunchTyped<int32_t>(A, p, output_kind, grid, st);
}

bool LaunchModularPlanes(const ModularPlanesArgs& B, const FilterParams& fp, int output_kind, hipStream_t st) {
  const ModularEmitArgs& A = B.e;
  if (B.num_color != 1 && B.num_color != 3) return false;
  // an alpha plane reaches the output only through a fourth packed channel
  const bool alpha = B.alpha && output_kind == JXLHIP_OUT_PACKED && fp.fmt.num_channels == 4;
  if (B.num_color == 3 && !alpha) return LaunchModularEmit(A, fp, output_kind, st);
  if (A.xsize == 0 || A.ysize == 0 || A.ns < ((A.xsize + 7u) & ~7u) || (A.ns & 7u) || A.group_shift < 7 || A.group_shift > 10 ||
      A.xsg != ((A.xsize - 1) >> A.group_shift) + 1 || !fp.out || A.sample_type > JXLHIP_MODULAR_I32)
    return false;
  for (uint32_t c = 0; c < B.num_color; c++)
    if (!A.plane[c] || ((uintptr_t)A.plane[c] & 15u)) return false;
  if (alpha && ((uintptr_t)B.alpha & 15u)) return false;
  if (B.num_color == 3 ? !A.group_rct : A.global_rct != 0) return false;  // (a grey frame has no programs at all)
  if (output_kind == JXLHIP_OUT_LINEAR_RGB_F32 && ((((uintptr_t)fp.out | fp.out_stride) & 3u) != 0)) return false;
  if (output_kind != JXLHIP_OUT_LINEAR_RGB_F32 && output_kind != JXLHIP_OUT_PACKED) return false;
  FilterParams p = fp;
  p.fmt.transfer = JXLHIP_TF_LINEAR;  // the identity hand-over: the samples are encoded already
  // the fixed 8-bit tails want rows they can store 16 bytes at a time into; everything else is the general tail's
  const jxlhip_output_format& o = p.fmt;
  const bool rows4 = (((uintptr_t)p.out | p.out_stride) & 3u) == 0;
  int fmt = -1;
  if (output_kind == JXLHIP_OUT_PACKED && o.sample_type == JXLHIP_SAMPLE_U8 && o.swap_endianness == 0 && rows4)
    fmt = o.num_channels == 4 ? kRgba8 : kRgb8;
  const PlanesKernel* k = nullptr;
  for (int pass = 0; pass < 2 && !k; pass++, fmt = -1)
    for (const PlanesKernel& e : kPlanesKernels)
      if (e.sample_type == A.sample_type && e.num_color == B.num_color && e.alpha == alpha && e.output_kind == output_kind && e.fmt == fmt) {
        k = &e;
        break;
      }
  if (!k) return false;
  ModularPlanesArgs args = B;
  if (!alpha) args.alpha = nullptr;
  const uint32_t runs = (A.xsize + kRun - 1) / kRun;
  const dim3 grid((runs + kRunsPerBlock - 1) / kRunsPerBlock, std::min(A.ysize, kMaxGridRows));
  hipLaunchKernelGGL(k->kernel, grid, dim3(kRunsPerBlock), 0, st, args, p);
  return true;
}

}  // namespace jxlhip
