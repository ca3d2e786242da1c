// kernels_filters_fast_general.hip -- the phase-2 row march (filters_fast.h) for the general packed output: the format
// is read from the launch parameters at run time (every packed format without a kernel of its own; 256 VGPRs).  The
// stage lists without EPF2; those with it compile as long again: kernels_filters_fast_general_epf2.hip.
#include "filters_fast.h"

namespace jxlhip {

bool LaunchFastGeneral(const DevFrame& f, const FilterParams& p, int gab, int epf_iters, hipStream_t st) {
  if (epf_iters == 2) return LaunchFastGeneralEpf2(f, p, gab, st);
#define JXLHIP_FAST(G, E)                                    \
  if (gab == G && epf_iters == E) {                          \
    LaunchFastT<G, E, JXLHIP_OUT_PACKED, -1>(f, p, st);      \
    return true;                                             \
  }
  JXLHIP_FAST(0, 0)
  JXLHIP_FAST(1, 0)
  JXLHIP_FAST(0, 1)
  JXLHIP_FAST(1, 1)
#undef JXLHIP_FAST
  return false;
}

}  // namespace jxlhip
