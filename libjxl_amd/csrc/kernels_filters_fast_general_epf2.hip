// kernels_filters_fast_general_epf2.hip -- the phase-2 row march (filters_fast.h) for the general packed output (see
// kernels_filters_fast_general.hip), the stage lists that end in EPF1 + EPF2, from either row source.
#include "filters_fast.h"

namespace jxlhip {

bool LaunchFastGeneralEpf2(const DevFrame& f, const FilterParams& p, int gab, hipStream_t st) {
  if (gab == 0) LaunchFastT<0, 2, JXLHIP_OUT_PACKED, -1>(f, p, st);
  else if (gab == 1) LaunchFastT<1, 2, JXLHIP_OUT_PACKED, -1>(f, p, st);
  return gab == 0 || gab == 1;
}

}  // namespace jxlhip
