// work_classes.h -- the work classes of phase 1 and their strategy tables.  No HIP header: dev_common.h includes it for
// the kernels, phase1_plan.h for the launch plan and its stand-alone checker.
#ifndef JXLHIP_WORK_CLASSES_H_
#define JXLHIP_WORK_CLASSES_H_

#include <stdint.h>

namespace jxlhip {

// Work classes: one compacted varblock list per class, built by k_prepare, so
// that every wave of the transform kernels runs ONE strategy.
static constexpr int kNumSpecial = 9;
static constexpr int kNumMedium = 11;
enum WorkClass : int {
  kClsDct8 = 0,      // strategy 0
  kClsSpecial0 = 1,  // kNumSpecial single-block kinds follow, see kSpecialStrategy
  kClsMedium0 = kClsSpecial0 + kNumSpecial,  // kNumMedium kinds, see kMediumStrategy
  kClsLarge = kClsMedium0 + kNumMedium,      // 21..26 (any side >= 128)
  kNumClasses = kClsLarge + 1
};
// counter block of one band: the list length of class c lives at
// count[c * kCounterPad] -- one 128-byte line per counter, so that the ~20
// atomics every k_prepare workgroup issues do not all serialise on one line
static constexpr int kCounterPad = 32;
static_assert(kNumClasses <= 32, "counter block layout");
static constexpr uint8_t kSpecialStrategy[kNumSpecial] = {1, 2, 3, 12, 13, 14, 15, 16, 17};
// medium class index -> strategy (16x8 .. 64x64)
static constexpr uint8_t kMediumStrategy[kNumMedium] = {6, 7, 4, 8, 9, 10, 11, 5, 18, 19, 20};

}  // namespace jxlhip
#endif
