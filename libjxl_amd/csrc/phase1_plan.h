// phase1_plan.h -- which phase-1 kernels a frame launches, with what grid, and which role a workgroup of the merged
// launch plays: the one definition that the host (LaunchBlocksT, Phase1Frame), the device (k_transform_r) and the tests
// share.  No HIP header: kernels_blocks.hip, kernels_mfma.hip and context.hip include it, and so does
// tests/fuzz/check_phase1_plan.cc, which runs this very code under -fsanitize=address,undefined and answers the
// Python restatement of tests/phase1_plan.py.
#ifndef JXLHIP_PHASE1_PLAN_H_
#define JXLHIP_PHASE1_PLAN_H_

#include <stdint.h>

#include "work_classes.h"

#ifdef __HIP__
#define JXLHIP_PLAN_HD __host__ __device__ __forceinline__
#else
#define JXLHIP_PLAN_HD inline
#endif

namespace jxlhip {

// ---- families -----------------------------------------------------------------------------------------------------
// Families: kernels whose workgroups take "unit u of the family" from blockIdx.x; which class list and which unit of
// it that is follows from the class counters on the device (PickUnit).  The host never learns the list lengths; it
// bounds the unit count by cells/64 + N and caps the grid at a few resident generations, the workgroups loop.
struct FamilyEntry {
  int cls;
  int unit_varblocks;
};
template <int N>
struct Family {
  FamilyEntry e[N];
};
template <int N, int M>
constexpr Family<N> FamilySlice(const FamilyEntry (&all)[M], int first) {
  static_assert(N <= M, "");
  Family<N> f{};
  for (int i = 0; i < N; i++) f.e[i] = all[first + i];
  return f;
}

// A: 64x64, 64x32, 32x64 (long units first); A1: one varblock per task for every class of the family
static constexpr FamilyEntry kFamilyA[3] = {{kClsMedium0 + 8, 1}, {kClsMedium0 + 9, 2}, {kClsMedium0 + 10, 2}};
static constexpr FamilyEntry kFamilyA1[3] = {{kClsMedium0 + 8, 1}, {kClsMedium0 + 9, 1}, {kClsMedium0 + 10, 1}};
// R: 16x8 .. 32x32, row-per-lane, 4 waves x (64 / S) varblocks per unit, long units first so that the drain ends on
// short ones.  Its first five entries are R32 (longer side 32: twice the registers per lane), its last three R16
// (longer side 16); merged, the (few, long, register-heavy) L = 32 units come first: on a mixed frame their
// single-generation latency (~27 us as a launch of its own) disappears behind the L = 16 bulk, at the price of the
// L = 16 units running at the L = 32 occupancy.
static constexpr FamilyEntry kFamilyR[8] = {{kClsMedium0 + 7, 8},  {kClsMedium0 + 5, 16}, {kClsMedium0 + 6, 16},
                                            {kClsMedium0 + 3, 32}, {kClsMedium0 + 4, 32}, {kClsMedium0 + 2, 16},
                                            {kClsMedium0 + 0, 32}, {kClsMedium0 + 1, 32}};
static constexpr int kNumR32 = 5, kNumR16 = 3;
static constexpr Family<kNumR32> kFamilyR32 = FamilySlice<kNumR32>(kFamilyR, 0);
static constexpr Family<kNumR16> kFamilyR16 = FamilySlice<kNumR16>(kFamilyR, kNumR32);
static_assert(kMediumStrategy[8] == 18 && kMediumStrategy[9] == 19 && kMediumStrategy[10] == 20 &&
              kMediumStrategy[7] == 5 && kMediumStrategy[5] == 10 && kMediumStrategy[6] == 11 &&
              kMediumStrategy[2] == 4 && kMediumStrategy[3] == 8 && kMediumStrategy[4] == 9 &&
              kMediumStrategy[0] == 6 && kMediumStrategy[1] == 7, "class table mismatch");

// ---- the matrix cores ---------------------------------------------------------------------------------------------
struct Phase1Mfma {
  bool mfma32, mfma16;  // DCT32X32 / DCT16X16 leave the row-per-lane families for kernels_mfma.hip
};
constexpr uint64_t kMfma16MinPixels = 16u << 20;
// mfma_switch: JXLHIP_MFMA (> 0 both classes, 0 neither, < 0 this rule).  DCT32X32 goes when it is the only class of
// the 32-point row-per-lane family in the frame (the class kernel then is a launch of its own anyway).  DCT16X16: the
// same rule against the 16-point row-per-lane family (16x8, 8x16), only when no 32-point class pulls the merged launch
// in anyway, and on frames of 16 Mpx and more (measured, all-DCT16X16 frames: 8K blocks 132 -> 118 us, 16x16 + 32x32
// 176 -> 161 us; 4K 33.6 -> 37.6 us: the butterflies stay; on the mixed c3 frame a launch of its own costs
// 97 -> 117 us, like DCT32X32)
inline Phase1Mfma PickMfma(uint32_t used_acs, uint64_t pixels, int mfma_switch) {
  constexpr uint32_t kOthers32 = (1u << 8) | (1u << 9) | (1u << 10) | (1u << 11);  // 32x8 .. 16x32
  constexpr uint32_t kOthers16 = (1u << 6) | (1u << 7);
  Phase1Mfma m;
  const bool lone32 = (used_acs & (1u << 5)) && !(used_acs & kOthers32);
  m.mfma32 = mfma_switch > 0 || (mfma_switch < 0 && lone32);
  const bool lone16 = (used_acs & (1u << 4)) && !(used_acs & (kOthers16 | kOthers32)) &&
                      (!(used_acs & (1u << 5)) || m.mfma32) && pixels >= kMfma16MinPixels;
  m.mfma16 = mfma_switch > 0 || (mfma_switch < 0 && lone16);
  return m;
}

// ---- the launches -------------------------------------------------------------------------------------------------
// caps: residency of the kernel (workgroups per CU by LDS / registers) x 256 CUs x 2 generations
constexpr uint32_t kCapGridA = 1536;    // k_transform_a
constexpr uint32_t kCapBig = 512;       // the 64-point role of k_transform_r
constexpr uint32_t kCapGridR16 = 4096;  // k_transform_r16, the row-per-lane role of k_transform_r
constexpr uint32_t kCapGridR32 = 3072;  // k_transform_r32 (units of 128 blocks)
constexpr uint32_t kCapGridLarge = 512;
constexpr uint32_t kCapMfma32 = 2048;
constexpr uint32_t kCapMfma16 = 4096;
constexpr int kKnobMax = 4096;          // JXLHIP_BIG_WGS / JXLHIP_R_WGS: anything outside [1, kKnobMax] = the built-in caps
constexpr uint32_t kUnitCells = 64;     // a unit is bounded by 64 block cells

// DCT8: steps of 8 blocks per wave, blocks per 256-thread workgroup (Dct8Rows)
constexpr int Dct8Steps(bool int16) { return int16 ? 4 : 2; }
constexpr uint32_t Dct8PerWg(bool int16) { return 4u * Dct8Steps(int16) * 8u; }

struct Phase1Inputs {
  uint32_t cells;       // block cells of the stripe
  uint32_t used_acs;    // jxlhip_frame_params::used_acs (0 = unknown: every family may have work)
  uint32_t coeff_type;  // JXLHIP_COEFF_I16 (0) / I32
  uint32_t fused;       // DevFrame::fused
  uint32_t xsb;
  bool mfma32, mfma16;  // PickMfma
  int big_wgs, r_wgs;   // JXLHIP_BIG_WGS / JXLHIP_R_WGS as read (experiments and tests/test_gpu_phase1_loops.py: fewer
                        // workgroups, so that each one walks many units)
};

// The grid of every launch, 0 = the launch does not happen.
struct Phase1Plan {
  uint32_t transform_a, transform_8, transform_r16, transform_r32, large, mfma32, mfma16;
  // the merged launch: transform_r = special_wgs + big_wgs + r_wgs + dct8_wgs, in the order of the grid (RoleOf deals
  // the part behind the special head)
  uint32_t transform_r, special_wgs, big_wgs, r_wgs, dct8_wgs;
};

inline Phase1Plan PlanPhase1(const Phase1Inputs& in) {
  auto min_u = [](uint32_t a, uint32_t b) { return a < b ? a : b; };
  // used_acs (when the caller knows it) says which families have work at all
  auto any = [&](uint32_t strategies) { return in.used_acs == 0 || (in.used_acs & strategies) != 0; };
  auto bits = [](int first, int last) { return (2u << last) - (1u << first); };
  const uint32_t cells = in.cells, units = cells / kUnitCells;
  const bool big_set = in.big_wgs >= 1 && in.big_wgs <= kKnobMax;
  const bool r_set = in.r_wgs >= 1 && in.r_wgs <= kKnobMax;
  uint32_t grid_a = min_u(units + 3, kCapGridA);
  uint32_t grid_r16 = min_u(units + 3, kCapGridR16);
  uint32_t grid_r32 = min_u(units / 2 + 5, kCapGridR32);
  if (big_set) grid_a = min_u(grid_a, (uint32_t)in.big_wgs);
  if (r_set) {
    grid_r16 = min_u(grid_r16, (uint32_t)in.r_wgs);
    grid_r32 = min_u(grid_r32, (uint32_t)in.r_wgs);
  }
  const bool need_r16 = any(bits(6, 7)) || (!in.mfma16 && any(1u << 4));
  const bool need_r32 = any(bits(8, 11)) || (!in.mfma32 && any(1u << 5));
  const bool merged = need_r16 && need_r32;
  const bool have_big = any(bits(18, 20));
  // worst cases: all cells special (3 tasks per 64 blocks, 4 tasks per workgroup) or all DCT8
  const bool specials = any(bits(1, 3) | bits(12, 17));
  const uint32_t bound_s = specials ? (cells / 64 + kNumSpecial) * 3 / 4 + 1 : 0;
  // fused == 2 (a stripe): only the DCT8 cells of the two block rows its neighbours pull are on the list
  const uint32_t cells_8 = in.fused == 0 ? cells : (in.fused == 2 ? 2u * in.xsb : 0u);
  const uint32_t per_wg = Dct8PerWg(in.coeff_type == 0);
  const uint32_t bound_8 = (any(1u << 0) && cells_8) ? (cells_8 + per_wg - 1) / per_wg : 0;

  Phase1Plan p{};
  if (merged) {
    // -10 us per 8K d1.0 frame against two launches, -15 us more with family A inside; the single-block classes ride
    // along (specials at the head, DCT8 workgroups alternating with the other classes' persistent ones).
    // (round 6, again: the 16-point classes in a launch of their own -- 93 VGPRs, no LDS, five waves per SIMD, where inside
    // this launch they run at three: all-DCT16X16 frames 159 against 115 us -- cost 9 us more per frame on both the d1 mix
    // and genuine-content shares, profiles/r06_transform_overread.txt; the single launch stays)
    p.big_wgs = have_big ? min_u(grid_a, big_set ? (uint32_t)in.big_wgs : kCapBig) : 0u;
    p.special_wgs = specials ? bound_s + kNumSpecial : 0u;
    p.r_wgs = grid_r16;
    p.dct8_wgs = bound_8;
    p.transform_r = p.special_wgs + p.big_wgs + p.r_wgs + p.dct8_wgs;
  } else {
    if (have_big) p.transform_a = grid_a;
    p.transform_8 = (bound_s > bound_8 ? bound_s : bound_8) + (specials ? kNumSpecial : 0);
    if (need_r16) p.transform_r16 = grid_r16;
    if (need_r32) p.transform_r32 = grid_r32;
  }
  if (in.mfma32 && any(1u << 5)) p.mfma32 = min_u(cells / 16 / 4 + 1, kCapMfma32);  // varblocks / 4 waves
  if (in.mfma16 && any(1u << 4)) p.mfma16 = min_u(cells / 4 / 4 + 1, kCapMfma16);
  if (cells >= 256 && any(bits(21, 26))) p.large = min_u(cells / 128, kCapGridLarge);
  return p;
}

// ---- the roles of the merged launch -------------------------------------------------------------------------------
enum Phase1RoleKind : uint32_t { kRoleIdle, kRoleDct8, kRoleBig, kRoleRowLane };
struct Phase1Role {
  Phase1RoleKind kind;
  uint32_t idx;  // workgroup of its kind: < d8 (DCT8), < big_wgs, < r_wgs
};
// Workgroup i behind the special head of k_transform_r.
// The DCT8 workgroups (short, LDS-free, the bulk of a d1.0 frame) alternate with the persistent workgroups of the
// other classes in the dispatch order, so that the two kinds run side by side from the first wave on -- as two
// launches the second waits for the first's tail, which on frames of a few Mpx is most of it (1080p: blocks 39 -> ? us;
// the two-stream form pays ~40 us of fork / join events instead).
// The launch is sized for a frame of nothing but DCT8 (dct8_wgs); k_prepare's count says how many of those workgroups
// have work (need8).  On genuine content -- a few per cent DCT8 -- thousands of empty workgroups between the
// persistent ones cost more than the DCT8 blocks themselves: then only the ones with work alternate and the surplus
// sits at the end of the grid, leaving at once (two-phase, real-content shares: 8K 257 -> 200 us, 4K 61 -> 51 us).
// With a quarter or more of the bound in use (the d1 mix: 45 %) the old placement stays: there the empty workgroups
// between the later persistent ones HELP (4K 39 vs 45 us; profiles/r03_dct8_workgroup_roles.txt).
JXLHIP_PLAN_HD Phase1Role RoleOf(uint32_t i, uint32_t big_wgs, uint32_t r_wgs, uint32_t dct8_wgs, uint32_t need8) {
  const uint32_t np = big_wgs + r_wgs;
  const uint32_t d8 = need8 * 4 < dct8_wgs ? need8 : dct8_wgs;
  const uint32_t pairs = np < d8 ? np : d8;
  bool is_dct8;
  uint32_t idx;
  if (i < 2 * pairs) {
    is_dct8 = (i & 1u) != 0;
    idx = i >> 1;
  } else {
    is_dct8 = d8 > np;
    idx = i - pairs;
    if (idx >= (is_dct8 ? d8 : np)) return {kRoleIdle, 0};
  }
  if (is_dct8) return {kRoleDct8, idx};
  if (idx < big_wgs) return {kRoleBig, idx};
  return {kRoleRowLane, idx - big_wgs};
}

}  // namespace jxlhip
#endif
