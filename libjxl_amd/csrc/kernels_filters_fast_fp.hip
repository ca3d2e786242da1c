// kernels_filters_fast_fp.hip -- the phase-2 row march (filters_fast.h) for the packed formats fixed at compile time
// that JXLHIP_FIXED_FORMATS assigns to kFastFp: the float and half-float formats (sRGB and linear).
#include "filters_fast.h"

namespace jxlhip {

bool LaunchFastFixedFp(const DevFrame& f, const FilterParams& p, int gab, int epf_iters, hipStream_t st) {
  return LaunchFixedUnit<kFastFp>(f, p, gab, epf_iters, st);
}

}  // namespace jxlhip
