// kernels_noise.hip -- photon noise (FrameHeader::kNoise) on gfx950: the random planes of PrepareNoiseInput and the
// render pipeline stages ConvolveNoiseStage + AddNoiseStage, followed by the caller's output tail.
//
// Replaces (behaviour, not code): lib/jxl/dec_noise.cc:58-151 (RandomImage / Random3Planes / PrepareNoiseInput),
// lib/jxl/xorshift128plus-inl.h:28-86, lib/jxl/render_pipeline/stage_noise.cc:72-310 and lib/jxl/noise.h:20-42.
//
// Two launches behind the frame's normal filter path, which has written the filtered frame as planar XYB:
//   k_noise_rng   one Xorshift128+ per AC group, 8 lanes of 64 bits, seeded through SplitMix64 with
//                 (visible_frame_index, nonvisible_frame_index, gx * 256, gy * 256).  The reference runs it serially:
//                 plane 0, 1, 2, each row by row with ceil(w / 16) fills of 16 floats per row, w x h being the group
//                 clipped to the TRUE image size.  The generator is linear over GF(2), so the state after n fills is
//                 M^n s0: the fill sequence of a group is cut into segments of kNoiseSegFills fills, a thread = one
//                 (group, lane, segment) jumps to its segment with one 128x128-bit matrix-vector product (the
//                 matrices M^(j * kNoiseSegFills) are built on the host, NoiseJumpTable) and runs the segment's fills,
//                 storing its two floats of each fill where the serial order puts them.
//   k_noise_emit  per 64 x 16 tile: the three random planes with a 2-pixel border mirrored at the true image edge into
//                 LDS, the 5x5 convolution, AddNoise on the XYB samples, then the output tail of the filter kernels
//                 (emit.h): planar XYB, linear float RGB or any packed format with dither and alpha.
#include <algorithm>
#include <vector>

#include "dev_common.h"
#include "emit.h"
#include "kernels.h"

namespace jxlhip {

namespace {

constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;

__host__ __device__ inline uint64_t SplitMix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// one Fill of one lane (xorshift128plus-inl.h:61-84): returns the 64 random bits, advances (a, b) = (s0_[i], s1_[i])
__host__ __device__ inline uint64_t XorshiftStep(uint64_t& a, uint64_t& b) {
  const uint64_t bits = a + b;
  uint64_t t = a;
  a = b;
  t ^= t << 23;
  b = t ^ b ^ (t >> 18) ^ (b >> 5);
  return bits;
}

// Xorshift128Plus(seed1..seed4) (xorshift128plus-inl.h:46-57): the state of `lane`
__host__ __device__ inline void NoiseSeed(uint32_t s1, uint32_t s2, uint32_t s3, uint32_t s4, uint32_t lane,
                                          uint64_t& a, uint64_t& b) {
  a = SplitMix64(((uint64_t)s1 << 32) + s2 + kGolden);
  b = SplitMix64(((uint64_t)s3 << 32) + s4 + kGolden);
  for (uint32_t i = 0; i < lane; i++) {
    a = SplitMix64(a);
    b = SplitMix64(b);
  }
}

__device__ __forceinline__ int MirrorN(int x, int n) {  // image_ops.h:184-196
  while (x < 0 || x >= n) x = x < 0 ? -x - 1 : 2 * n - 1 - x;
  return x;
}

// ---- the random planes --------------------------------------------------------------------------------------------
// block = 8 groups x 8 lanes (threadIdx.x & 7 = lane); blockIdx.x = segment (the jump matrix is uniform per block),
// blockIdx.y = block of 8 groups
__global__ __launch_bounds__(64) void k_noise_rng(NoiseArgs N) {
  const uint32_t lane = threadIdx.x & 7u;
  const uint32_t g = blockIdx.y * 8u + (threadIdx.x >> 3);
  const uint32_t seg = blockIdx.x;
  if (g >= N.xsg * N.ysg) return;
  const uint32_t gx = g % N.xsg, gy = g / N.xsg;
  const uint32_t w = min(256u, N.xsize - gx * 256u), h = min(256u, N.ysize - gy * 256u);
  const uint32_t fills = (w + 15u) / 16u;  // per row (dec_noise.cc:74-96: ceil(w / 16))
  const uint32_t total = 3u * h * fills;
  const uint32_t n0 = seg * kNoiseSegFills;
  if (n0 >= total) return;
  uint64_t a, b;
  NoiseSeed(N.visible, N.nonvisible, gx * 256u, gy * 256u, lane, a, b);
  if (seg) {  // (a, b) = M^n0 (a, b): XOR of the columns of the set state bits
    const uint32_t* m = N.jump + (size_t)seg * kNoiseJumpWords;
    const uint32_t v[4] = {(uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32)};
    uint32_t o[4] = {0, 0, 0, 0};
    for (int k = 0; k < 128; k++) {
      const uint32_t mask = 0u - ((v[k >> 5] >> (k & 31)) & 1u);
#pragma unroll
      for (int i = 0; i < 4; i++) o[i] ^= m[4 * k + i] & mask;
    }
    a = (uint64_t)o[0] | ((uint64_t)o[1] << 32);
    b = (uint64_t)o[2] | ((uint64_t)o[3] << 32);
  }
  const uint32_t steps = min(kNoiseSegFills, total - n0);
  const uint32_t row = n0 / fills;
  uint32_t cx = n0 - row * fills;
  uint32_t p = row / h, r = row - p * h;
  const size_t group0 = (size_t)gy * 256u * N.ns + gx * 256u;
  float* dst = N.rnd + p * N.nplane + group0 + (size_t)r * N.ns;
  for (uint32_t s = 0; s < steps; s++) {
    const uint64_t bits = XorshiftStep(a, b);
    // batch32[2 * lane] / [2 * lane + 1] = low / high half (dec_noise.cc:79-95); 1.0 + 23 random mantissa bits
    const float lo = __uint_as_float(((uint32_t)bits >> 9) | 0x3F800000u);
    const float hi = __uint_as_float(((uint32_t)(bits >> 32) >> 9) | 0x3F800000u);
    const uint32_t x = cx * 16u + 2u * lane;
    if (x + 1u < w) {
      *(float2*)(dst + x) = make_float2(lo, hi);  // (ns, nplane and x are even: 8-byte aligned)
    } else if (x < w) {
      dst[x] = lo;
    }
    if (++cx == fills) {
      cx = 0;
      dst += N.ns;
      if (++r == h) {
        r = 0;
        p++;
        dst = N.rnd + p * N.nplane + group0;
      }
    }
  }
}

// ---- convolution + AddNoise + output ------------------------------------------------------------------------------
constexpr int kTW = 64, kTH = 16, kLW = kTW + 4, kLH = kTH + 4;

// ConvolveNoiseStage::ProcessRow (stage_noise.cc:269-296), its order of additions
__device__ __forceinline__ float ConvNoise(const float* c) {
  float others = 0.0f;
#pragma unroll
  for (int i = -2; i <= 2; i++) {
    others = others + c[-2 * kLW + i];
    others = others + c[-1 * kLW + i];
    others = others + c[1 * kLW + i];
    others = others + c[2 * kLW + i];
  }
  others = others + c[-2];
  others = others + c[-1];
  others = others + c[1];
  others = others + c[2];
  return __builtin_fmaf(others, 0.16f, c[0] * -3.84f);
}

// StrengthEvalLut + NoiseStrength (stage_noise.cc:55-133): the LUT interpolated at x, clamped to [0, 1]
__device__ __forceinline__ float NoiseStrength(const NoiseArgs& N, float x) {
  const float scaled = __builtin_fmaxf(0.0f, x * 6.0f);
  float fl = __builtin_floorf(scaled);
  float fr = scaled - fl;
  if (scaled >= 7.0f) {
    fl = 6.0f;
    fr = 1.0f;
  }
  const int i = (int)fl;
  // lut[i], lut[i + 1] by selects (a dynamic index into the kernel argument would go through scratch)
  float low = N.lut[0], high = N.lut[1];
#pragma unroll
  for (int k = 1; k < 7; k++) {
    low = i == k ? N.lut[k] : low;
    high = i == k ? N.lut[k + 1] : high;
  }
  const float v = __builtin_fmaf(high - low, fr, low);
  return __builtin_fmaxf(__builtin_fminf(v, 1.0f), 0.0f);
}

template <int OUTK>
__global__ __launch_bounds__(256) void k_noise_emit(NoiseArgs N, FilterParams P) {
  __shared__ float t[3][kLH * kLW];
  const int tx0 = blockIdx.x * kTW, ty0 = blockIdx.y * kTH;
  const int W = (int)N.xsize, H = (int)N.ysize;
  for (int i = threadIdx.x; i < kLH * kLW; i += 256) {
    const int ly = i / kLW, lx = i - ly * kLW;
    const size_t o = (size_t)MirrorN(ty0 - 2 + ly, H) * N.ns + MirrorN(tx0 - 2 + lx, W);
    t[0][i] = N.rnd[o];
    t[1][i] = N.rnd[o + N.nplane];
    t[2][i] = N.rnd[o + 2 * N.nplane];
  }
  __syncthreads();
  const int lx = threadIdx.x & (kTW - 1);
  const int x = tx0 + lx;
  if (x >= W) return;
#pragma unroll 1
  for (int ly = threadIdx.x / kTW; ly < kTH; ly += 256 / kTW) {
    const int y = ty0 + ly;
    if (y >= H) break;
    const int c0 = (ly + 2) * kLW + lx + 2;
    // AddNoiseStage::ProcessRow + AddNoiseToRGB (stage_noise.cc:136-222)
    const float rnd_r = ConvNoise(&t[0][c0]) * 0.22f;
    const float rnd_g = ConvNoise(&t[1][c0]) * 0.22f;
    const float rnd_c = ConvNoise(&t[2][c0]) * 0.22f;
    const size_t o = (size_t)y * N.ns + x;
    float vx = N.xyb[o], vy = N.xyb[o + N.nplane], vb = N.xyb[o + 2 * N.nplane];
    const float str_g = NoiseStrength(N, (vy - vx) * 0.5f);
    const float str_r = NoiseStrength(N, (vy + vx) * 0.5f);
    const float red = str_r * __builtin_fmaf(0.0078125f, rnd_r, 0.9921875f * rnd_c);
    const float green = str_g * __builtin_fmaf(0.0078125f, rnd_g, 0.9921875f * rnd_c);
    const float rg = red + green;
    vx = __builtin_fmaf(N.ytox, rg, red - green) + vx;
    vy = vy + rg;
    vb = __builtin_fmaf(N.ytob, rg, vb);
    if constexpr (OUTK == JXLHIP_OUT_XYB_PLANAR) {
      float* d = (float*)P.out + (size_t)y * P.out_stride + x;
      d[0] = vx;
      d[P.out_plane_stride] = vy;
      d[2 * P.out_plane_stride] = vb;
    } else {
      float rgb[3];
      XybToRgb(vx, vy, vb, P, rgb);
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

// 128x128 matrices over GF(2) on the state (a, b): column k = the image of state bit k (a: 0..63, b: 64..127)
struct Gf2Mat {
  uint64_t col[128][2];
};

void Apply(const Gf2Mat& m, const uint64_t v[2], uint64_t out[2]) {
  uint64_t o0 = 0, o1 = 0;
  for (int k = 0; k < 128; k++)
    if ((v[k >> 6] >> (k & 63)) & 1u) {
      o0 ^= m.col[k][0];
      o1 ^= m.col[k][1];
    }
  out[0] = o0;
  out[1] = o1;
}

Gf2Mat Mul(const Gf2Mat& x, const Gf2Mat& y) {
  Gf2Mat r;
  for (int k = 0; k < 128; k++) Apply(x, y.col[k], r.col[k]);
  return r;
}

// the matrices M^(j * kNoiseSegFills), j = 0 .. kNoiseSegs - 1, built once per process
const std::vector<Gf2Mat>& JumpMatrices() {
  static const std::vector<Gf2Mat> mats = [] {
    Gf2Mat m;
    for (int k = 0; k < 128; k++) {
      uint64_t a = k < 64 ? 1ull << k : 0, b = k < 64 ? 0 : 1ull << (k - 64);
      (void)XorshiftStep(a, b);
      m.col[k][0] = a;
      m.col[k][1] = b;
    }
    static_assert((kNoiseSegFills & (kNoiseSegFills - 1)) == 0, "segment length: a power of two");
    for (uint32_t n = 1; n < kNoiseSegFills; n *= 2) m = Mul(m, m);
    std::vector<Gf2Mat> v(kNoiseSegs);
    for (int k = 0; k < 128; k++) {
      v[0].col[k][0] = k < 64 ? 1ull << k : 0;
      v[0].col[k][1] = k < 64 ? 0 : 1ull << (k - 64);
    }
    for (uint32_t j = 1; j < kNoiseSegs; j++) v[j] = Mul(m, v[j - 1]);
    return v;
  }();
  return mats;
}

}  // namespace

void NoiseJumpTable(uint32_t* host) {
  const std::vector<Gf2Mat>& mats = JumpMatrices();
  for (uint32_t j = 0; j < kNoiseSegs; j++)
    for (int k = 0; k < 128; k++) {
      uint32_t* d = host + (size_t)j * kNoiseJumpWords + 4 * k;
      d[0] = (uint32_t)mats[j].col[k][0];
      d[1] = (uint32_t)(mats[j].col[k][0] >> 32);
      d[2] = (uint32_t)mats[j].col[k][1];
      d[3] = (uint32_t)(mats[j].col[k][1] >> 32);
    }
}

void NoiseStateAfter(uint32_t visible, uint32_t nonvisible, uint32_t x0, uint32_t y0, uint64_t fills,
                     uint64_t state[16]) {
  const std::vector<Gf2Mat>& mats = JumpMatrices();
  const uint64_t j = std::min<uint64_t>(fills / kNoiseSegFills, kNoiseSegs - 1);
  for (uint32_t lane = 0; lane < 8; lane++) {
    uint64_t s[2], o[2];
    NoiseSeed(visible, nonvisible, x0, y0, lane, s[0], s[1]);
    Apply(mats[j], s, o);
    for (uint64_t i = j * kNoiseSegFills; i < fills; i++) (void)XorshiftStep(o[0], o[1]);
    state[2 * lane] = o[0];
    state[2 * lane + 1] = o[1];
  }
}

bool LaunchNoise(const NoiseArgs& N, const FilterParams& p, int output_kind, hipStream_t st) {
  if (output_kind < 0 || output_kind > 2 || N.xsize == 0 || N.ysize == 0) return false;
  const uint32_t ngroups = N.xsg * N.ysg;
  hipLaunchKernelGGL(k_noise_rng, dim3(kNoiseSegs, (ngroups + 7) / 8), dim3(64), 0, st, N);
  const dim3 grid((N.xsize + kTW - 1) / kTW, (N.ysize + kTH - 1) / kTH);
  if (output_kind == JXLHIP_OUT_XYB_PLANAR)
    hipLaunchKernelGGL(k_noise_emit<JXLHIP_OUT_XYB_PLANAR>, grid, dim3(256), 0, st, N, p);
  else if (output_kind == JXLHIP_OUT_LINEAR_RGB_F32)
    hipLaunchKernelGGL(k_noise_emit<JXLHIP_OUT_LINEAR_RGB_F32>, grid, dim3(256), 0, st, N, p);
  else
    hipLaunchKernelGGL(k_noise_emit<JXLHIP_OUT_PACKED>, grid, dim3(256), 0, st, N, p);
  return true;
}

}  // namespace jxlhip
