// check_phase1_plan.cc -- libjxl_amd/csrc/phase1_plan.h alone, in a stand-alone program (tests/test_phase1_launch_plan.py
// builds it with -fsanitize=address,undefined).
//   (a) RoleOf deals every role index of the merged launch exactly once, DCT8 and persistent workgroups alternating;
//   (b) every plan's merged grid is the sum of its parts, and no stand-alone family launch goes with it;
//   (c) lines of "cells used_acs coeff_type fused xsb pixels mfma_switch big_wgs r_wgs" on stdin: PickMfma and PlanPhase1
//       of each as one line of key=value pairs; no input: the caps and the family tables.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../libjxl_amd/csrc/phase1_plan.h"

using namespace jxlhip;

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                           \
    }                                                                    \
  } while (0)

// (a)
static long CheckRoles(uint32_t big_wgs, uint32_t r_wgs, uint32_t dct8_wgs, uint32_t need8) {
  const uint32_t np = big_wgs + r_wgs, total = np + dct8_wgs;
  std::vector<int> big(big_wgs, 0), row(r_wgs, 0), d8_hit(dct8_wgs, 0);
  uint32_t d8 = 0;  // DCT8 workgroups with a role = 1 + the largest index dealt
  std::vector<Phase1Role> roles(total);
  for (uint32_t i = 0; i < total; i++) {
    const Phase1Role r = roles[i] = RoleOf(i, big_wgs, r_wgs, dct8_wgs, need8);
    switch (r.kind) {
      case kRoleIdle: break;
      case kRoleDct8:
        CHECK(r.idx < dct8_wgs);
        d8_hit[r.idx]++;
        d8 = std::max(d8, r.idx + 1);
        break;
      case kRoleBig:
        CHECK(r.idx < big_wgs);
        big[r.idx]++;
        break;
      case kRoleRowLane:
        CHECK(r.idx < r_wgs);
        row[r.idx]++;
        break;
      default: CHECK(!"kind");
    }
  }
  for (int n : big) CHECK(n == 1);
  for (int n : row) CHECK(n == 1);
  CHECK(d8 >= need8 && d8 <= dct8_wgs);
  for (uint32_t k = 0; k < dct8_wgs; k++) CHECK(d8_hit[k] == (k < d8 ? 1 : 0));
  // today's order: pairs of (persistent, DCT8) from the first workgroup on
  for (uint32_t i = 0; i < 2 * std::min(np, d8); i++) {
    const Phase1RoleKind k = roles[i].kind;
    CHECK(i & 1 ? k == kRoleDct8 : (k == kRoleBig || k == kRoleRowLane));
    CHECK(roles[i].idx == (k == kRoleRowLane ? i / 2 - big_wgs : i / 2));
  }
  return total;
}

static long SweepRoles() {
  long n = 0;
  for (uint32_t big_wgs : {0u, 1u, 2u, 7u, 512u})
    for (uint32_t r_wgs : {1u, 2u, 5u, 99u, 4096u})
      for (uint32_t dct8_wgs : {0u, 1u, 3u, 4u, 5u, 100u, 4097u}) {
        const long q = dct8_wgs / 4;
        for (long need8 : {0l, 1l, q - 1, q, q + 1, (long)dct8_wgs})
          n += CheckRoles(big_wgs, r_wgs, dct8_wgs, (uint32_t)std::min<long>(std::max(need8, 0l), dct8_wgs));
      }
  return n;
}

// (b)
static void CheckPlan(const Phase1Plan& p) {
  CHECK(p.transform_r == (p.r_wgs ? p.special_wgs + p.big_wgs + p.r_wgs + p.dct8_wgs : 0));
  if (p.transform_r) {
    CHECK(!p.transform_a && !p.transform_8 && !p.transform_r16 && !p.transform_r32);
  } else {
    CHECK(!p.special_wgs && !p.big_wgs && !p.dct8_wgs);
    CHECK(!(p.transform_r16 && p.transform_r32));
  }
}

static long SweepPlans() {
  long n = 0;
  const uint32_t masks[] = {0u, 1u, 1u << 4, 1u << 5, (1u << 4) | (1u << 5), (1u << 6) | (1u << 8), (1u << 27) - 1,
                            (1u << 18) | (1u << 4) | (1u << 9) | 2u, (1u << 21) | (1u << 7) | (1u << 11) | 1u};
  for (uint32_t cells : {0u, 64u, 1024u, 6144u, 16384u, 262144u, 1u << 22})
    for (uint32_t used : masks)
      for (uint32_t coeff_type : {0u, 1u})
        for (uint32_t fused : {0u, 1u, 2u})
          for (int mfma : {-1, 0, 1})
            for (int big : {INT32_MIN, 0, 1, 2, 4096, 5000})
              for (int r : {INT32_MIN, 1, 7, 4096, 4097}) {
                const Phase1Mfma m = PickMfma(used, (uint64_t)cells * 64, mfma);
                CheckPlan(PlanPhase1({cells, used, coeff_type, fused, 40u, m.mfma32, m.mfma16, big, r}));
                n++;
              }
  return n;
}

// (c)
template <int N>
static void PrintFamily(const char* name, const FamilyEntry (&fam)[N]) {
  printf("%s=", name);
  for (int i = 0; i < N; i++)
    printf("%s%d:%d", i ? "," : "", (int)kMediumStrategy[fam[i].cls - kClsMedium0], fam[i].unit_varblocks);
  printf("\n");
}

static void PrintTables() {
  printf("grid_a=%u\nbig_cap=%u\ngrid_r16=%u\ngrid_r32=%u\ngrid_l=%u\nmfma32=%u\nmfma16=%u\n", kCapGridA, kCapBig,
         kCapGridR16, kCapGridR32, kCapGridLarge, kCapMfma32, kCapMfma16);
  printf("knob_max=%d\nunit_cells=%u\nmfma16_min_pixels=%llu\n", kKnobMax, kUnitCells, (unsigned long long)kMfma16MinPixels);
  PrintFamily("kFamilyA", kFamilyA);
  PrintFamily("kFamilyA1", kFamilyA1);
  PrintFamily("kFamilyR", kFamilyR);
  PrintFamily("kFamilyR16", kFamilyR16.e);
  PrintFamily("kFamilyR32", kFamilyR32.e);
}

int main() {
  const long roles = SweepRoles(), plans = SweepPlans();
  fprintf(stderr, "roles=%ld plans=%ld\n", roles, plans);
  unsigned cells, used, coeff_type, fused, xsb;
  unsigned long long pixels;
  int mfma, big, r;
  long lines = 0;
  while (scanf("%u %u %u %u %u %llu %d %d %d", &cells, &used, &coeff_type, &fused, &xsb, &pixels, &mfma, &big, &r) == 9) {
    const Phase1Mfma m = PickMfma(used, pixels, mfma);
    const Phase1Plan p = PlanPhase1({cells, used, coeff_type, fused, xsb, m.mfma32, m.mfma16, big, r});
    CheckPlan(p);
    printf("pick32=%d pick16=%d a=%u t8=%u r16=%u r32=%u large=%u mfma32=%u mfma16=%u r=%u special_wgs=%u big_wgs=%u "
           "r_wgs=%u dct8_wgs=%u\n", m.mfma32, m.mfma16, p.transform_a, p.transform_8, p.transform_r16, p.transform_r32,
           p.large, p.mfma32, p.mfma16, p.transform_r, p.special_wgs, p.big_wgs, p.r_wgs, p.dct8_wgs);
    lines++;
  }
  if (!lines) PrintTables();
  return 0;
}
