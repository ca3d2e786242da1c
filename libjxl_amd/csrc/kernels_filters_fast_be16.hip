// kernels_filters_fast_be16.hip -- the phase-2 row march (filters_fast.h) for the packed formats fixed at compile time
// that JXLHIP_FIXED_FORMATS assigns to kFastBe16: the big-endian 16-bit formats (sRGB and PQ, RGB and RGBA).
#include "filters_fast.h"

namespace jxlhip {

bool LaunchFastFixedBe16(const DevFrame& f, const FilterParams& p, int gab, int epf_iters, hipStream_t st) {
  return LaunchFixedUnit<kFastBe16>(f, p, gab, epf_iters, st);
}

}  // namespace jxlhip
