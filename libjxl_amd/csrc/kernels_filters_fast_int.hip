// kernels_filters_fast_int.hip -- the phase-2 row march (filters_fast.h) for the packed formats fixed at compile time
// that JXLHIP_FIXED_FORMATS assigns to kFastInt: the little-endian integer formats (8-bit and 16-bit sRGB, RGB and RGBA).
#include "filters_fast.h"

namespace jxlhip {

bool LaunchFastFixedInt(const DevFrame& f, const FilterParams& p, int gab, int epf_iters, hipStream_t st) {
  return LaunchFixedUnit<kFastInt>(f, p, gab, epf_iters, st);
}

}  // namespace jxlhip
