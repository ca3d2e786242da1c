// kernels_tonemap.hip -- tone mapping (jxlhip_set_tone_mapping) on gfx950: the render pipeline's ToneMappingStage for
// a PQ original shown on a display dimmer than its mastering peak, followed by the caller's output tail.
//
// Replaces (behaviour, not code): lib/jxl/render_pipeline/stage_tone_mapping.cc (ToneMappingStage::ProcessRow),
// lib/jxl/cms/tone_mapping-inl.h (Rec2408ToneMapper::ToneMap, GamutMap), lib/jxl/cms/tone_mapping.h
// (Rec2408ToneMapperBase's members: ToneMapConstants below) and TF_PQ's two directions at an intensity target of 1
// (lib/jxl/cms/transfer_functions-inl.h:145-208).
//
// One kernel, k_tone_map, behind the frame's whole path, which has written the frame as planar XYB at output size into
// context memory (the form every feature launch writes when something follows it).  Elementwise: a lane owns two
// horizontally adjacent pixels of a row (one 8-byte load per plane: a wave reads 512 contiguous bytes of each; the pair
// goes out through StorePackedPair's wide stores), a block 512 columns, and the blocks of a grid column stride over
// the rows.  No LDS, no scratch; the constants travel in the launch arguments and stay wave-uniform.  Instantiations:
// float RGB, the general packed tail FmtSel<-1>, and 8-bit sRGB RGB / RGBA with the tail fixed at compile time.
//
// Arithmetic: every operation is the reference's single-lane one -- explicit fmaf where it uses MulAdd, IEEE square
// root and IEEE division everywhere it divides or takes a root (the two PQ rationals included) -- so the stage itself is
// bit-equal to tests/tone_mapping_model.py on the same linear pixels; what differs from the reference behind it is
// emit.h's sRGB / PQ curve alone.
#include "dev_common.h"
#include "emit.h"
#include "kernels.h"

#include <math.h>

namespace jxlhip {

namespace {

constexpr int kPairsPerBlock = 256;
constexpr unsigned kMaxGridRows = 1024;

// EvalRationalPolynomial of degree 4/4 with the division the reference's FastDivision comes to (Div).
// JXLHIP_TONEMAP_RCP=1 (a measurement build, never the product's: DESIGN section 3 "Tone mapping" has what each form
// measured) takes emit.h's Rational44 instead: the same Horner scheme, times the hardware's 1-ulp v_rcp_f32.
#ifndef JXLHIP_TONEMAP_RCP
#define JXLHIP_TONEMAP_RCP 0
#endif
__device__ __forceinline__ float Rational44Div(float x, const float* p, const float* q) {
#if JXLHIP_TONEMAP_RCP
  return Rational44(x, p, q);
#else
  float yp = p[4], yq = q[4];
#pragma unroll
  for (int i = 3; i >= 0; i--) {
    yp = __builtin_fmaf(yp, x, p[i]);
    yq = __builtin_fmaf(yq, x, q[i]);
  }
  return yp / yq;
#endif
}

// TF_PQ(1.0)::EncodedFromDisplay (transfer_functions-inl.h:172-207)
__device__ __forceinline__ float PqEncodedFromDisplay1(float v) {
  const float kP[5] = {1.351392e-02f, -1.095778e+00f, 5.522776e+01f, 1.492516e+02f, 4.838434e+01f};
  const float kQ[5] = {1.012416e+00f, 2.016708e+01f, 9.263710e+01f, 1.120607e+02f, 2.590418e+01f};
  const float kPlo[5] = {9.863406e-06f, 3.881234e-01f, 1.352821e+02f, 6.889862e+04f, -2.864824e+05f};
  const float kQlo[5] = {3.371868e+01f, 1.477719e+03f, 1.608477e+04f, -4.389884e+04f, -2.072546e+05f};
  const float x = __builtin_fabsf(v);
  const float r = __builtin_sqrtf(__builtin_sqrtf(x * (1.0f * (1.0f / 10000.0f))));
  const float mag = x < 1e-4f ? Rational44Div(r, kPlo, kQlo) : Rational44Div(r, kP, kQ);
  return __builtin_copysignf(__builtin_fabsf(mag), v);
}

// TF_PQ(1.0)::DisplayFromEncoded (transfer_functions-inl.h:145-168): a 4/4 rational in x + x * x
__device__ __forceinline__ float PqDisplayFromEncoded1(float v) {
  const float kP[5] = {2.62975656e-04f, -6.23553089e-03f, 7.38602301e-01f, 2.64553172e+00f, 5.50034862e-01f};
  const float kQ[5] = {4.21350107e+02f, -4.28736818e+02f, 1.74364667e+02f, -3.39078883e+01f, 2.67718770e+00f};
  const float x = __builtin_fabsf(v);
  const float xpxx = __builtin_fmaf(x, x, x);
  const float mag = Rational44Div(xpxx, kP, kQ) * 10000.0f;
  return __builtin_copysignf(__builtin_fabsf(mag), v);
}

// Min / Max as one lane evaluates them: (b < a) ? b : a and (a < b) ? b : a
__device__ __forceinline__ float MinF(float a, float b) { return b < a ? b : a; }
__device__ __forceinline__ float MaxF(float a, float b) { return a < b ? b : a; }

// ToneMappingStage::ProcessRow on one pixel of linear RGB (stage_tone_mapping.cc:88-109)
__device__ __forceinline__ void ToneMapPixel(const ToneMapConstants& K, float* rgb) {
#pragma unroll
  for (int c = 0; c < 3; c++) rgb[c] = rgb[c] * K.to_intensity_target;
  {  // Rec2408ToneMapper::ToneMap (tone_mapping-inl.h:40-72)
    const float lum = K.source_peak * __builtin_fmaf(K.lum[0], rgb[0], __builtin_fmaf(K.lum[1], rgb[1], K.lum[2] * rgb[2]));
    const float npq = MinF(1.0f, (PqEncodedFromDisplay1(lum) - K.pq_mastering_min) * K.inv_pq_mastering_range);
    float e2 = npq;
    if (!(npq < K.ks)) {  // P (:83-96)
      const float t = (npq - K.ks) * K.inv_one_minus_ks;
      const float t2 = t * t;
      const float t3 = t2 * t;
      const float a = __builtin_fmaf(2.0f, t3, __builtin_fmaf(-3.0f, t2, 1.0f));
      const float b = t3 + __builtin_fmaf(-2.0f, t2, t);
      const float m = __builtin_fmaf(-2.0f, t3, 3.0f * t2) * K.max_lum;
      e2 = __builtin_fmaf(a, K.ks, __builtin_fmaf(b, K.one_minus_ks, m));
    }
    const float om = 1.0f - e2;
    const float om2 = om * om;
    const float om4 = om2 * om2;
    const float e3 = __builtin_fmaf(K.min_lum, om4, e2);
    const float e4 = __builtin_fmaf(e3, K.pq_mastering_range, K.pq_mastering_min);
    const float d4 = PqDisplayFromEncoded1(e4);
    const float new_lum = MinF(K.target_peak, d4 < 0.0f ? 0.0f : d4);
    const bool use_cap = lum <= 1e-6f;
    const float ratio = new_lum / MaxF(lum, 1e-6f);
    const float cap = new_lum * K.inv_target_peak;
    const float mul = ratio * K.normalizer;
#pragma unroll
    for (int c = 0; c < 3; c++) rgb[c] = use_cap ? cap : rgb[c] * mul;
  }
  {  // GamutMap (tone_mapping-inl.h:139-187)
    const float lum = __builtin_fmaf(K.lum[0], rgb[0], __builtin_fmaf(K.lum[1], rgb[1], K.lum[2] * rgb[2]));
    float mix_sat = 0.0f, mix_lum = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const float val = rgb[c];
      const float vmg = val - lum;
      const float inv = 1.0f / (vmg == 0.0f ? 1.0f : vmg);
      const float vov = val * inv;
      mix_sat = vmg >= 0.0f ? mix_sat : MaxF(mix_sat, vov);
      mix_lum = MaxF(mix_lum, vmg <= 0.0f ? mix_sat : vov - inv);
    }
    const float mix = MinF(MaxF(0.0f, __builtin_fmaf(K.preserve_saturation, mix_sat - mix_lum, mix_lum)), 1.0f);
#pragma unroll
    for (int c = 0; c < 3; c++) rgb[c] = __builtin_fmaf(mix, lum - rgb[c], rgb[c]);
    const float max_clr = MaxF(MaxF(1.0f, rgb[0]), MaxF(rgb[1], rgb[2]));
    const float norm = 1.0f / max_clr;
#pragma unroll
    for (int c = 0; c < 3; c++) rgb[c] = rgb[c] * norm;
  }
#pragma unroll
  for (int c = 0; c < 3; c++) rgb[c] = rgb[c] * K.from_desired_intensity_target;
}

// FMT: the packed format fixed at compile time (FormatId), -1 = read from the launch parameters
template <int OUTK, int FMT>
__global__ __launch_bounds__(kPairsPerBlock) void k_tone_map(ToneMapArgs A, FilterParams P) {
  typedef float f2 __attribute__((ext_vector_type(2)));
  typedef uint32_t u2 __attribute__((ext_vector_type(2), aligned(4)));
  typedef uint32_t u4 __attribute__((ext_vector_type(4), aligned(4)));
  const uint32_t x = 2u * (blockIdx.x * kPairsPerBlock + threadIdx.x);
  if (x >= A.xsize) return;
  const bool pair = x + 1 < A.xsize;  // (an odd width: the last pixel of a row is alone)
  for (uint32_t y = blockIdx.y; y < A.ysize; y += gridDim.y) {
    // rows are A.ns floats apart, a multiple of 64: column x + 1 exists in memory even when it is not in the frame.
    // 32-bit offsets: LaunchToneMap refuses planes whose last sample lies at or beyond 2^32 floats
    const uint32_t o = y * A.ns + x;
    const f2 vx = *(const f2*)(A.xyb + o);
    const f2 vy = *(const f2*)(A.xyb + (o + A.nplane));
    const f2 vb = *(const f2*)(A.xyb + (o + 2u * A.nplane));
    float p0[3], p1[3];
    XybToRgb(vx.x, vy.x, vb.x, P, p0);
    XybToRgb(vx.y, vy.y, vb.y, P, p1);
    ToneMapPixel(A.k, p0);
    ToneMapPixel(A.k, p1);
    char* orow = (char*)P.out + (size_t)y * P.out_stride;
    if constexpr (OUTK == JXLHIP_OUT_LINEAR_RGB_F32) {
      uint32_t* d = (uint32_t*)orow + 3u * x;
      if (pair) {  // 16 + 8 bytes (see StorePackedPair)
        __builtin_nontemporal_store(u4{__float_as_uint(p0[0]), __float_as_uint(p0[1]), __float_as_uint(p0[2]), __float_as_uint(p1[0])},
                                    (u4*)d);
        asm volatile("" ::: "memory");
        __builtin_nontemporal_store(u2{__float_as_uint(p1[1]), __float_as_uint(p1[2])}, (u2*)(d + 4));
      } else {
        d[0] = __float_as_uint(p0[0]);
        d[1] = __float_as_uint(p0[1]);
        d[2] = __float_as_uint(p0[2]);
      }
    } else {
      if (pair) StorePackedPair<FmtSel<FMT>>(P, P.dither, orow, (int)x, (int)y, p0, p1);
      else StorePackedPixel<FmtSel<FMT>>(P, P.dither, orow, (int)x, (int)y, p0);
    }
  }
}

// Rec2408ToneMapperBase::InvEOTF = TF_PQ_Base::EncodedFromDisplay(1.0, .) (cms/transfer_functions.h:107-119)
float PqInvEotfHost(float luminance) {
  constexpr double kM1 = 2610.0 / 16384, kM2 = (2523.0 / 4096) * 128, kC1 = 3424.0 / 4096, kC2 = (2413.0 / 4096) * 32,
                   kC3 = (2392.0 / 4096) * 32;
  double d = luminance;
  if (d == 0.0) return 0.0f;
  const double sign = d;
  d = fabs(d);
  const double xp = pow(d * (double)(1.0f * (1.0f / 10000.0f)), kM1);
  const double e = pow((kC1 + xp * kC2) / (1.0 + xp * kC3), kM2);
  return copysignf((float)e, (float)sign);
}

}  // namespace

void ToneMapHostConstants(float orig, float desired, const float luminances[3], bool dest_pq, ToneMapConstants* k) {
  // ToneMappingStage's constructor (stage_tone_mapping.cc:43-63): source range {0, orig}, target range {0, desired}
  k->to_intensity_target = dest_pq ? 10000.f / orig : 1.f;
  k->from_desired_intensity_target = dest_pq ? desired / 10000.f : 1.f;
  k->source_peak = orig;
  k->target_peak = desired;
  for (int i = 0; i < 3; i++) k->lum[i] = luminances[i];
  // Rec2408ToneMapperBase's members (tone_mapping.h:82-97)
  k->pq_mastering_min = PqInvEotfHost(0.0f);
  const float pq_mastering_max = PqInvEotfHost(orig);
  k->pq_mastering_range = pq_mastering_max - k->pq_mastering_min;
  k->inv_pq_mastering_range = 1.0f / k->pq_mastering_range;
  k->min_lum = (PqInvEotfHost(0.0f) - k->pq_mastering_min) * k->inv_pq_mastering_range;
  k->max_lum = (PqInvEotfHost(desired) - k->pq_mastering_min) * k->inv_pq_mastering_range;
  k->ks = 1.5f * k->max_lum - 0.5f;
  k->inv_one_minus_ks = 1.0f / std::max(1e-6f, 1.0f - k->ks);
  k->normalizer = orig / desired;
  k->inv_target_peak = 1.f / desired;
  k->one_minus_ks = 1.0f - k->ks;  // (P evaluates Sub(Set(1), ks) per call)
  k->preserve_saturation = 0.1f;
}

bool LaunchToneMap(const ToneMapArgs& A, const FilterParams& p, int output_kind, hipStream_t st) {
  if (A.xsize == 0 || A.ysize == 0 || A.ns < ((A.xsize + 1u) & ~1u) || (A.ns & 1u) || (A.nplane & 1u) ||
      (uint64_t)A.nplane < (uint64_t)A.ns * A.ysize || 3ull * A.nplane > 0xFFFFFFFFull || !A.xyb || !p.out)
    return false;
  const uint32_t pairs = (A.xsize + 1u) / 2u;
  const dim3 grid((pairs + kPairsPerBlock - 1) / kPairsPerBlock, std::min(A.ysize, kMaxGridRows));
  // 8-bit sRGB RGB / RGBA (any bit depth up to 8: the depth is a launch parameter) have the tail fixed at compile time:
  // through the general tail's per-sample branches the launch took 0.262 ms at 8K against 0.187 ms as float RGB
  const jxlhip_output_format& o = p.fmt;
  const bool srgb8 = output_kind == JXLHIP_OUT_PACKED && o.transfer == JXLHIP_TF_SRGB && o.sample_type == JXLHIP_SAMPLE_U8 &&
                     o.swap_endianness == 0;
  if (output_kind == JXLHIP_OUT_LINEAR_RGB_F32)
    hipLaunchKernelGGL((k_tone_map<JXLHIP_OUT_LINEAR_RGB_F32, -1>), grid, dim3(kPairsPerBlock), 0, st, A, p);
  else if (srgb8 && o.num_channels == 3)
    hipLaunchKernelGGL((k_tone_map<JXLHIP_OUT_PACKED, FormatId(JXLHIP_TF_SRGB, JXLHIP_SAMPLE_U8, 3)>), grid, dim3(kPairsPerBlock), 0, st, A, p);
  else if (srgb8 && o.num_channels == 4)
    hipLaunchKernelGGL((k_tone_map<JXLHIP_OUT_PACKED, FormatId(JXLHIP_TF_SRGB, JXLHIP_SAMPLE_U8, 4)>), grid, dim3(kPairsPerBlock), 0, st, A, p);
  else if (output_kind == JXLHIP_OUT_PACKED)
    hipLaunchKernelGGL((k_tone_map<JXLHIP_OUT_PACKED, -1>), grid, dim3(kPairsPerBlock), 0, st, A, p);
  else
    return false;
  return true;
}

}  // namespace jxlhip
