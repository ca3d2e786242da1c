// kernels_filters_fast.hip -- the entry point of the phase-2 row march (filters_fast.h) and its kernels for the float
// RGB and planar XYB outputs; the packed outputs are compiled in kernels_filters_fast_{general,general_epf2,int,be16,fp}.hip.
#include "filters_fast.h"

namespace jxlhip {

bool FastFixedFormat(const jxlhip_output_format& o) {
#define JXLHIP_IS(TF, ST, NC, SW, U) \
  if (IsFormat(o, TF, ST, NC, SW)) return true;
  JXLHIP_FIXED_FORMATS(JXLHIP_IS)
#undef JXLHIP_IS
  return false;
}

bool LaunchFiltersFast(const DevFrame& f, const FilterParams& p, int gab, int epf_iters,
                       int output_kind, hipStream_t st) {
  if (epf_iters > 2) return false;  // three iterations: LaunchEpf0 (kernels_epf0.hip) first, then this with (0, 2)
  if (f.xsize < 16 || f.ysize < 16) return false;  // multiply mirrored columns / rows: generic kernel
  // row offsets inside a plane are 32-bit
  if ((uint64_t)f.plane_tile_rows * f.tile_stride * 256u >= (1ull << 32)) return false;
  if (f.linear_stride && !(gab == 0 && epf_iters == 2)) return false;
  if (gab < 0 || gab > 1 || epf_iters < 0) return false;
  if (output_kind == JXLHIP_OUT_PACKED &&
      (LaunchFastFixedInt(f, p, gab, epf_iters, st) || LaunchFastFixedBe16(f, p, gab, epf_iters, st) ||
       LaunchFastFixedFp(f, p, gab, epf_iters, st)))
    return true;
  if (output_kind != 0 && output_kind != 1) return LaunchFastGeneral(f, p, gab, epf_iters, st);
#define JXLHIP_FAST(G, E)                                  \
  if (gab == G && epf_iters == E) {                        \
    if (output_kind == 0) LaunchFastT<G, E, 0>(f, p, st);  \
    else LaunchFastT<G, E, 1>(f, p, st);                   \
    return true;                                           \
  }
  JXLHIP_STAGE_LISTS(JXLHIP_FAST)
#undef JXLHIP_FAST
  return false;
}

}  // namespace jxlhip
