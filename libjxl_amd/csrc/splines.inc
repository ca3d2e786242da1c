// splines.inc -- splines in the host front-end (included by entropy.cc, behind the entropy decoder it uses):
// the bundle at the head of a spline frame's DC-global section and the draw list the device kernel consumes.
//
// Replaces (behaviour, not code): lib/jxl/splines.cc -- Splines::Decode (:600-642), DecodeAllStartingPoints
// (:250-285), QuantizedSpline::Decode (:534-583) and Dequantize (:439-532), Splines::InitializeDrawCache (:657-758)
// with DrawCentripetalCatmullRomSpline (:300-342), ForEachEquallySpacedPoint (:351-383), SegmentsFromPoints
// (:185-209), ContinuousIDCT (:55-79) and ComputeSegments (:129-171); FastCosf (lib/jxl/base/fast_math-inl.h:97-126).
// Arithmetic follows the reference's single-lane evaluation: fmaf where it has MulAdd, sequential accumulation in the
// IDCT, IEEE sqrtf and division, float everywhere it has float.

#include <cmath>
#include <utility>

struct jxlhip_splines {
  struct Quantized {
    int64_t x0, y0;                                 // the starting point
    std::vector<std::pair<int64_t, int64_t>> dd;    // control-point delta-deltas
    int32_t color[3][32];
    int32_t sigma[32];
  };
  int32_t quant_adjust = 0;
  std::vector<Quantized> splines;
};

namespace {

// Splines contexts (splines.h:35-43)
enum : uint32_t { kSplQuantAdjCtx = 0, kSplStartCtx, kSplNumCtx, kSplNumPointsCtx, kSplPointsCtx, kSplDctCtx, kSplCtxs };
constexpr int64_t kSplinePosLimit = 1 << 23;
constexpr int64_t kSplineDeltaLimit = 1 << 30;
constexpr uint64_t kSplineMaxControlPoints = 1u << 20;
constexpr float kSplSqrt2 = 1.41421356237f;    // kSqrt2 (dct_scales.h:15)
constexpr float kSplSqrt0_5 = 0.70710678118f;  // kSqrt0_5
constexpr double kSplPi = 3.14159265358979323846264338327950288;
constexpr float kSplChannelWeight[4] = {0.0042f, 0.075f, 0.07f, .3333f};  // X, Y, B, sigma

inline int64_t SplUnpackSigned(uint32_t v) { return (int64_t)(v >> 1) ^ -(int64_t)(v & 1u); }
inline bool SplPosOk(int64_t x, int64_t y) {
  return x < kSplinePosLimit && x > -kSplinePosLimit && y < kSplinePosLimit && y > -kSplinePosLimit;
}
inline bool SplPosOkF(float x, float y) {
  const float lim = (float)kSplinePosLimit;
  return x < lim && x > -lim && y < lim && y > -lim;
}

// the per-spline checks QuantizedSpline::Decode applies to its values
bool SplDeltaOk(int64_t a, int64_t b) {
  return a < kSplineDeltaLimit && a > -kSplineDeltaLimit && b < kSplineDeltaLimit && b > -kSplineDeltaLimit;
}

float SplInvAdjustedQuant(int32_t adjustment) {
  return adjustment >= 0 ? 1.f / (1.f + .125f * (float)adjustment) : (1.f - .125f * (float)adjustment);
}

// std::llround as the reference's x86-64 build evaluates it: out-of-range and NaN arguments give INT64_MIN
int64_t SplRound(float v) {
  if (!(fabsf(v) < 9.0e18f)) return INT64_MIN;
  return (int64_t)llroundf(v);
}

struct SplPoint {
  float x, y;
};

// FastCosf (fast_math-inl.h:97-126), one lane
float SplFastCos(float x) {
  const float pi2 = (float)(kSplPi * 2.0f), pi2_inv = (float)(0.5f / kSplPi);
  const float npi2 = floorf(x * pi2_inv) * pi2;
  const float xmodpi2 = x - npi2;
  const float x_pi = std::min(xmodpi2, pi2 - xmodpi2);
  const bool above_pihalf = x_pi >= (float)(kSplPi / 2.0f);
  const float x_pihalf = above_pihalf ? (float)kSplPi - x_pi : x_pi;
  const float xs = x_pihalf * 0.25f;
  const float x2 = xs * xs;
  const float x4 = x2 * x2;
  const float pre = fmaf(x4, (float)0.06960438, fmaf(x2, (float)-0.84087373, (float)1.68179268));
  const float s1 = fmaf(pre, pre, (float)-1.414213562);
  const float s2 = fmaf(s1, s1, -1.0f);
  return above_pihalf ? -s2 : s2;
}

// ContinuousIDCT (:55-79): the DCT-III of 32 values at t, rescaled so that {x, 0, ..., 0} gives x
float SplIdct(const float dct[32], float t) {
  const float tandhalf = t + 0.5f;
  float result = 0.0f;
  for (int i = 0; i < 32; i++) {
    const float mult = (float)(kSplPi / 32 * i);
    const float local = dct[i] * SplFastCos(mult * tandhalf);
    result = fmaf(kSplSqrt2, local, result);
  }
  return result;
}

struct SplSpline {
  std::vector<SplPoint> points;
  float color[3][32];
  float sigma[32];
};

// QuantizedSpline::Dequantize (:439-532); false where the reference fails
bool SplDequantize(const jxlhip_splines::Quantized& q, int32_t adjust, float y_to_x, float y_to_b,
                   uint64_t image_size, uint64_t* total_area, SplSpline* out) {
  const uint64_t area_limit = std::min<uint64_t>(1024 * image_size + (1ull << 32), 1ull << 42);
  out->points.clear();
  out->points.reserve(q.dd.size() + 1);
  const float px = roundf((float)q.x0), py = roundf((float)q.y0);
  if (!SplPosOkF(px, py)) return false;
  int64_t cx = (int64_t)px, cy = (int64_t)py;
  out->points.push_back({(float)cx, (float)cy});
  int64_t dx = 0, dy = 0;
  uint64_t manhattan = 0;
  for (const auto& d : q.dd) {
    dx += d.first;
    dy += d.second;
    manhattan += (uint64_t)(std::llabs(dx) + std::llabs(dy));
    if (manhattan > area_limit) return false;
    if (!SplPosOk(dx, dy)) return false;
    cx += dx;
    cy += dy;
    if (!SplPosOk(cx, cy)) return false;
    out->points.push_back({(float)cx, (float)cy});
  }
  const float inv_quant = SplInvAdjustedQuant(adjust);
  for (int c = 0; c < 3; c++)
    for (int i = 0; i < 32; i++) {
      const float inv_dct_factor = i == 0 ? kSplSqrt0_5 : 1.0f;
      out->color[c][i] = (float)q.color[c][i] * inv_dct_factor * kSplChannelWeight[c] * inv_quant;
    }
  for (int i = 0; i < 32; i++) {
    out->color[0][i] += y_to_x * out->color[1][i];
    out->color[2][i] += y_to_b * out->color[1][i];
  }
  // the area estimate (not taking kChannelWeight into account, as the reference)
  uint64_t color[3] = {0, 0, 0};
  for (int c = 0; c < 3; c++)
    for (int i = 0; i < 32; i++) color[c] += (uint64_t)ceilf(inv_quant * (float)std::abs(q.color[c][i]));
  color[0] += (uint64_t)ceilf(fabsf(y_to_x)) * color[1];
  color[2] += (uint64_t)ceilf(fabsf(y_to_b)) * color[1];
  const uint64_t max_color = std::max({color[1], color[0], color[2]});
  // CeilLog2Nonzero(1 + max_color) = the bit length of max_color
  const uint64_t logcolor = std::max<uint64_t>(1, max_color ? 64 - (uint64_t)__builtin_clzll(max_color) : 0);
  const float weight_limit =
      ceilf(sqrtf(((float)area_limit / (float)logcolor) / (float)std::max<uint64_t>(1, manhattan)));
  uint64_t width_estimate = 0;
  for (int i = 0; i < 32; i++) {
    const float inv_dct_factor = i == 0 ? kSplSqrt0_5 : 1.0f;
    out->sigma[i] = (float)q.sigma[i] * inv_dct_factor * kSplChannelWeight[3] * inv_quant;
    const float weight_f = ceilf(inv_quant * (float)std::abs(q.sigma[i]));
    const uint64_t weight = (uint64_t)std::min(weight_limit, std::max(1.0f, weight_f));
    width_estimate += weight * weight * logcolor;
  }
  *total_area += width_estimate * manhattan;
  return *total_area <= area_limit;
}

// DrawCentripetalCatmullRomSpline (:300-342): 16 points per span
void SplCatmullRom(std::vector<SplPoint> p, std::vector<SplPoint>* result) {
  if (p.empty()) return;
  if (p.size() == 1) {
    result->push_back(p[0]);
    return;
  }
  constexpr int kNumPoints = 16;
  const SplPoint first = {p[0].x + (p[0].x - p[1].x), p[0].y + (p[0].y - p[1].y)};
  const size_t n = p.size();
  const SplPoint last = {p[n - 1].x + (p[n - 1].x - p[n - 2].x), p[n - 1].y + (p[n - 1].y - p[n - 2].y)};
  p.insert(p.begin(), first);
  p.push_back(last);
  for (size_t start = 0; start + 3 < p.size(); start++) {
    const SplPoint* q = &p[start];
    result->push_back(q[1]);
    float d[3], t[4];
    t[0] = 0;
    for (int k = 0; k < 3; k++) {
      d[k] = sqrtf(hypotf(q[k + 1].x - q[k].x, q[k + 1].y - q[k].y));
      t[k + 1] = t[k] + d[k];
    }
    for (int i = 1; i < kNumPoints; i++) {
      const float tt = d[0] + ((float)i / kNumPoints) * d[1];
      SplPoint a[3], b[2];
      for (int k = 0; k < 3; k++) {
        const float f = (tt - t[k]) / d[k];
        a[k] = {q[k].x + f * (q[k + 1].x - q[k].x), q[k].y + f * (q[k + 1].y - q[k].y)};
      }
      for (int k = 0; k < 2; k++) {
        const float f = (tt - t[k]) / (d[k] + d[k + 1]);
        b[k] = {a[k].x + f * (a[k + 1].x - a[k].x), a[k].y + f * (a[k + 1].y - a[k].y)};
      }
      const float f = (tt - t[1]) / d[1];
      result->push_back({b[0].x + f * (b[1].x - b[0].x), b[0].y + f * (b[1].y - b[0].y)});
    }
  }
  result->push_back(p[p.size() - 2]);
}

// ForEachEquallySpacedPoint (:351-383) at kDesiredRenderingDistance = 1: (point, distance to the previous one)
void SplEquallySpaced(const std::vector<SplPoint>& pts, std::vector<std::pair<SplPoint, float>>* out) {
  SplPoint current = pts.front();
  out->push_back({current, 1.0f});
  size_t next = 0;
  while (next != pts.size()) {
    SplPoint previous = current;
    float from_previous = 0.f;
    for (;;) {
      if (next == pts.size()) {
        out->push_back({previous, from_previous});
        return;
      }
      const float vx = pts[next].x - previous.x, vy = pts[next].y - previous.y;
      const float to_next = sqrtf(vx * vx + vy * vy);
      if (from_previous + to_next >= 1.0f) {
        const float f = (1.0f - from_previous) / to_next;
        current = {previous.x + f * vx, previous.y + f * vy};
        out->push_back({current, 1.0f});
        break;
      }
      from_previous += to_next;
      previous = pts[next];
      ++next;
    }
  }
}

// ComputeSegments (:129-171) with kDistanceExp = 5
void SplComputeSegment(int64_t ysize, SplPoint center, float intensity, const float color[3], float sigma,
                       std::vector<jxlhip_spline_segment>* segs) {
  if (!(std::isfinite(sigma) && sigma != 0.0f && std::isfinite(1.0f / sigma) && std::isfinite(intensity))) return;
  constexpr float kDistanceExp = 5;  // JXL_HIGH_PRECISION, the reference's default build (common.h:15-17)
  float max_color = 0.01f;
  for (int c = 0; c < 3; c++) max_color = std::max(max_color, fabsf(color[c] * intensity));
  const float maximum_distance = sqrtf(-2.0f * sigma * sigma * (logf(0.1f) * kDistanceExp - logf(max_color)));
  int64_t y0 = SplRound(center.y - maximum_distance);
  y0 = std::max<int64_t>(y0, 0);
  int64_t y1 = SplRound(center.y + maximum_distance);
  y1 = y1 == INT64_MIN ? y1 : y1 + 1;
  y1 = std::min<int64_t>(y1, ysize);
  if (y1 <= y0) return;
  jxlhip_spline_segment s;
  s.center_x = center.x;
  s.center_y = center.y;
  s.inv_sigma = 1.0f / sigma;
  s.sigma_over_4_times_intensity = .25f * sigma * intensity;
  for (int c = 0; c < 3; c++) s.color[c] = color[c];
  s.maximum_distance = maximum_distance;
  s.y0 = (int32_t)y0;
  s.y1 = (int32_t)y1;
  segs->push_back(s);
}

int SplDecodeDct(SymbolReader* reader, BitReader* br, const std::vector<uint8_t>& cmap, int32_t dct[32]) {
  for (int i = 0; i < 32; i++) {
    const int64_t v = SplUnpackSigned(reader->ReadHybridUint(cmap[kSplDctCtx], br));
    if (v == INT32_MIN) return kBad;  // "the weird number in spline DCT"
    dct[i] = (int32_t)v;
  }
  return kOk;
}

}  // namespace

extern "C" {

int jxlhip_splines_decode(const uint8_t* data, size_t size, size_t* bit_pos, uint64_t num_pixels,
                          jxlhip_splines** out) {
  if (!data || !bit_pos || !out) return JXLHIP_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  try {
    BitReader br(data, size, *bit_pos);
    EntropyCode code;
    int rc = DecodeEntropyCode(&br, kSplCtxs, &code, /*disallow_lz77=*/false, 0);
    if (rc) return rc;
    if (!br.Healthy()) return kBad;
    SymbolReader reader(&code, &br);
    if (!reader.Ok()) return JXLHIP_ERR_OUT_OF_MEMORY;
    const std::vector<uint8_t>& cmap = code.context_map;
    std::unique_ptr<jxlhip_splines> s(new jxlhip_splines);
    uint64_t num_splines = reader.ReadHybridUint(cmap[kSplNumCtx], &br);
    const uint64_t max_control_points = std::min<uint64_t>(kSplineMaxControlPoints, num_pixels / 2);
    if (num_splines > max_control_points || num_splines + 1 > max_control_points) return kBad;
    num_splines++;
    s->splines.resize(num_splines);
    int64_t last_x = 0, last_y = 0;
    for (uint64_t i = 0; i < num_splines; i++) {  // DecodeAllStartingPoints
      const uint32_t dx = reader.ReadHybridUint(cmap[kSplStartCtx], &br);
      const uint32_t dy = reader.ReadHybridUint(cmap[kSplStartCtx], &br);
      const int64_t x = i ? SplUnpackSigned(dx) + last_x : (int64_t)dx;
      const int64_t y = i ? SplUnpackSigned(dy) + last_y : (int64_t)dy;
      if (!SplPosOk(x, y)) return kBad;
      s->splines[i].x0 = x;
      s->splines[i].y0 = y;
      last_x = x;
      last_y = y;
      if (!br.Healthy()) return kBad;
    }
    s->quant_adjust = (int32_t)SplUnpackSigned(reader.ReadHybridUint(cmap[kSplQuantAdjCtx], &br));
    uint64_t total_points = num_splines;
    for (auto& q : s->splines) {  // QuantizedSpline::Decode
      const uint64_t n = reader.ReadHybridUint(cmap[kSplNumPointsCtx], &br);
      if (n > max_control_points) return kBad;
      total_points += n;
      if (total_points > max_control_points) return kBad;
      q.dd.resize(n);
      for (auto& d : q.dd) {
        d.first = SplUnpackSigned(reader.ReadHybridUint(cmap[kSplPointsCtx], &br));
        d.second = SplUnpackSigned(reader.ReadHybridUint(cmap[kSplPointsCtx], &br));
        if (!SplDeltaOk(d.first, d.second)) return kBad;
      }
      for (auto& c : q.color)
        if ((rc = SplDecodeDct(&reader, &br, cmap, c))) return rc;
      if ((rc = SplDecodeDct(&reader, &br, cmap, q.sigma))) return rc;
      if (!br.Healthy() || reader.Corrupt()) return kBad;
    }
    if (!br.Healthy() || reader.Corrupt() || !reader.FinalStateOk()) return kBad;
    if (s->splines.empty()) return kBad;  // "decoded splines but got none"
    *bit_pos = br.BitsConsumed();
    *out = s.release();
    return kOk;
  } catch (const std::bad_alloc&) {
    return JXLHIP_ERR_OUT_OF_MEMORY;
  }
}

int jxlhip_splines_from_quantized(uint32_t num_splines, const int32_t* starts, const uint32_t* num_deltas,
                                  const int32_t* deltas, const int32_t* dcts, int32_t quantization_adjustment,
                                  jxlhip_splines** out) {
  if (!out || (num_splines && (!starts || !num_deltas || !dcts))) return JXLHIP_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (num_splines == 0) return kBad;
  try {
    std::unique_ptr<jxlhip_splines> s(new jxlhip_splines);
    s->quant_adjust = quantization_adjustment;
    s->splines.resize(num_splines);
    size_t k = 0;
    for (uint32_t i = 0; i < num_splines; i++) {
      auto& q = s->splines[i];
      q.x0 = starts[2 * i];
      q.y0 = starts[2 * i + 1];
      if (!SplPosOk(q.x0, q.y0)) return kBad;
      if (num_deltas[i] && !deltas) return JXLHIP_ERR_INVALID_ARGUMENT;
      q.dd.resize(num_deltas[i]);
      for (auto& d : q.dd) {
        d.first = deltas[2 * k];
        d.second = deltas[2 * k + 1];
        k++;
        if (!SplDeltaOk(d.first, d.second)) return kBad;
      }
      const int32_t* v = dcts + (size_t)128 * i;
      for (int j = 0; j < 128; j++)
        if (v[j] == INT32_MIN) return kBad;
      for (int c = 0; c < 3; c++) memcpy(q.color[c], v + 32 * c, sizeof(q.color[c]));
      memcpy(q.sigma, v + 96, sizeof(q.sigma));
    }
    *out = s.release();
    return kOk;
  } catch (const std::bad_alloc&) {
    return JXLHIP_ERR_OUT_OF_MEMORY;
  }
}

void jxlhip_splines_destroy(jxlhip_splines* s) { delete s; }

int jxlhip_splines_quantized(const jxlhip_splines* s, uint32_t* num_splines, size_t* num_deltas,
                             int32_t* quantization_adjustment, int32_t* starts, uint32_t* counts, int32_t* deltas,
                             int32_t* dcts) {
  if (!s || !num_splines || !num_deltas) return JXLHIP_ERR_INVALID_ARGUMENT;
  *num_splines = (uint32_t)s->splines.size();
  size_t k = 0;
  for (size_t i = 0; i < s->splines.size(); i++) {
    const auto& q = s->splines[i];
    if (starts) {
      starts[2 * i] = (int32_t)q.x0;
      starts[2 * i + 1] = (int32_t)q.y0;
    }
    if (counts) counts[i] = (uint32_t)q.dd.size();
    for (const auto& d : q.dd) {
      if (deltas) {
        deltas[2 * k] = (int32_t)d.first;
        deltas[2 * k + 1] = (int32_t)d.second;
      }
      k++;
    }
    if (dcts) {
      for (int c = 0; c < 3; c++) memcpy(dcts + 128 * i + 32 * c, q.color[c], sizeof(q.color[c]));
      memcpy(dcts + 128 * i + 96, q.sigma, sizeof(q.sigma));
    }
  }
  *num_deltas = k;
  if (quantization_adjustment) *quantization_adjustment = s->quant_adjust;
  return kOk;
}

int jxlhip_splines_segments(const jxlhip_splines* s, uint32_t xsize, uint32_t ysize, float y_to_x, float y_to_b,
                            jxlhip_spline_segment* out, size_t cap, size_t* count) {
  if (!s || !count || (cap && !out)) return JXLHIP_ERR_INVALID_ARGUMENT;
  *count = 0;
  try {
    // Splines::InitializeDrawCache: dequantise every spline first (the area estimate runs over all of them) ...
    std::vector<SplSpline> splines(s->splines.size());
    uint64_t total_area = 0;
    for (size_t i = 0; i < splines.size(); i++) {
      if (!SplDequantize(s->splines[i], s->quant_adjust, y_to_x, y_to_b, (uint64_t)xsize * ysize, &total_area,
                         &splines[i]))
        return kBad;
      const auto& p = splines[i].points;
      for (size_t j = 1; j < p.size(); j++)
        if (p[j].x == p[j - 1].x && p[j].y == p[j - 1].y) return kBad;  // identical successive control points
    }
    // (a total area above min(8 * pixels + 2^25, 2^30) is only a warning in the reference)
    std::vector<jxlhip_spline_segment> segs;
    std::vector<SplPoint> inter;
    std::vector<std::pair<SplPoint, float>> draw;
    for (const SplSpline& sp : splines) {
      inter.clear();
      draw.clear();
      SplCatmullRom(sp.points, &inter);
      SplEquallySpaced(inter, &draw);
      const float arc_length = (float)(draw.size() - 2) * 1.0f + draw.back().second;
      if (arc_length <= 0.f) continue;  // this spline would have no effect
      const float inv_arc_length = 1.0f / arc_length;
      int k = 0;
      for (const auto& pd : draw) {  // SegmentsFromPoints
        const float progress = std::min(1.f, ((float)k * 1.0f) * inv_arc_length);
        ++k;
        float color[3];
        for (int c = 0; c < 3; c++) color[c] = SplIdct(sp.color[c], (float)(32 - 1) * progress);
        const float sigma = SplIdct(sp.sigma, (float)(32 - 1) * progress);
        SplComputeSegment(ysize, pd.first, pd.second, color, sigma, &segs);
      }
    }
    *count = segs.size();
    if (out) memcpy(out, segs.data(), std::min(cap, segs.size()) * sizeof(jxlhip_spline_segment));
    return kOk;
  } catch (const std::bad_alloc&) {
    return JXLHIP_ERR_OUT_OF_MEMORY;
  }
}

}  // extern "C"
