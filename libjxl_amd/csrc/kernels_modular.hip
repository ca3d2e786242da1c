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

}  // namespace jxlhip
