"""The launch rule of phase 1 (libjxl_amd/csrc/phase1_plan.h: PickMfma, PlanPhase1), restated once for the tests.
Test infrastructure: test_gpu_phase1_loops.py asserts turn counts with launch_plan(), spectrum.py's frames pick their
launch with launch_of().  tests/test_phase1_launch_plan.py holds every table and launch_plan() itself to the compiled
header (tests/fuzz/check_phase1_plan.cc) on the CPU; nothing here needs a compiler."""
import numpy as np

# Grid caps of PlanPhase1, in workgroups
CAPS = dict(grid_a=1536, big_cap=512, grid_r16=4096, grid_r32=3072, grid_l=512, mfma32=2048, mfma16=4096)
# (strategy, varblocks per unit) in PickUnit's order: kFamilyA1 / kFamilyA, kFamilyR, kFamilyR16, kFamilyR32
FAMILY_A = {0: [(18, 1), (19, 1), (20, 1)], 1: [(18, 1), (19, 2), (20, 2)]}  # by coefficient type
FAMILY_R = [(5, 8), (10, 16), (11, 16), (8, 32), (9, 32), (4, 16), (6, 32), (7, 32)]
FAMILY_R32, FAMILY_R16 = FAMILY_R[:5], FAMILY_R[5:]
KNOB_UNSET = -(1 << 31)   # jxlhip_env::Switches::kUnset


class Launch:
    """One persistent launch (or role of the merged launch): `units` dealt round-robin to `workers`."""

    def __init__(self, units, workers, per_class):
        self.units, self.workers, self.per_class = int(units), int(workers), dict(per_class)

    @property
    def min_turns(self):  # turns every worker takes
        return self.units // self.workers

    @property
    def max_turns(self):
        return -(-self.units // self.workers)

    def workers_with(self, turns):  # how many workers take at least `turns` turns
        return max(0, min(self.workers, self.units - (turns - 1) * self.workers))

    def __repr__(self):
        return "Launch(%d units / %d workers, %s)" % (self.units, self.workers, self.per_class)


def strategy_counts(acs):
    acs = np.asarray(acs)
    return np.bincount(acs[(acs & 1) == 1] >> 1, minlength=27)


def _knob(v):
    return int(v) if v is not None and 1 <= int(v) <= 4096 else None  # anything else: the built-in value


def row_lane_launch(used, mfma32, mfma16):
    """need_r16 / need_r32 / merged; used(*strategies): whether the frame holds any of them; mfma32 / mfma16: DCT32X32 /
    DCT16X16 leave the row-per-lane families for the matrix-core kernels."""
    need_r16 = used(6, 7) or (not mfma16 and used(4))
    need_r32 = used(8, 9, 10, 11) or (not mfma32 and used(5))
    return dict(need_r16=need_r16, need_r32=need_r32, merged=need_r16 and need_r32)


def launch_of(used_acs, mfma):
    """row_lane_launch from the frame's used_acs and JXLHIP_MFMA (0 / 1)."""
    return row_lane_launch(lambda *ss: any(used_acs >> s & 1 for s in ss), mfma, mfma)


def pick_mfma(used, pixels, mfma):
    """(mfma32, mfma16) by PickMfma; mfma: JXLHIP_MFMA as a bool, None = unset (the context's own rule)."""
    lone32 = used(5) and not used(8, 9, 10, 11)
    mfma32 = lone32 if mfma is None else mfma
    lone16 = used(4) and not used(6, 7, 8, 9, 10, 11) and (not used(5) or mfma32) and pixels >= (16 << 20)
    return mfma32, (lone16 if mfma is None else mfma)


def launch_plan(acs, xsize, ysize, coeff_type=0, big_wgs=None, r_wgs=None, mfma=None, group_rows=None, caps=CAPS):
    """{kernel: Launch} of one jxlhip_decode_blocks call, by the rule of PlanPhase1: "a" (k_transform_a, or the
    64-point role of k_transform_r), "r" (the row-per-lane role of k_transform_r) or "r16" / "r32" (the stand-alone
    kernels), "large", "mfma32" / "mfma16" (workers = waves).  `acs`: the strategy map of the rows decoded (the whole
    frame, or the stripe of `group_rows` group rows), or its 27 strategy counts; big_wgs / r_wgs / mfma: the values of
    JXLHIP_BIG_WGS / JXLHIP_R_WGS / JXLHIP_MFMA (None = unset)."""
    n = np.asarray(acs) if np.ndim(acs) == 1 else strategy_counts(acs)
    used = lambda *ss: any(n[s] for s in ss)  # noqa: E731
    xsg, ysg = (xsize + 255) // 256, (ysize + 255) // 256
    cells = xsg * (group_rows or ysg) * 1024
    units = cells // 64
    mfma32, mfma16 = pick_mfma(used, xsize * ysize, None if mfma is None else int(mfma) != 0)
    big, rw = _knob(big_wgs), _knob(r_wgs)
    grid_a = min(units + 3, caps["grid_a"], big or (1 << 30))
    grid_r16 = min(units + 3, caps["grid_r16"], rw or (1 << 30))
    grid_r32 = min(units // 2 + 5, caps["grid_r32"], rw or (1 << 30))
    grid_l = min(max(cells // 128, 1), caps["grid_l"])
    need = row_lane_launch(used, mfma32, mfma16)
    merged = need["merged"]

    def family(entries, skip=()):
        return {s: -(-int(n[s]) // vb) for s, vb in entries if s not in skip and n[s]}

    skip = ((5,) if mfma32 else ()) + ((4,) if mfma16 else ())
    plan = {}
    if used(18, 19, 20):
        per = family(FAMILY_A[coeff_type])
        plan["a"] = Launch(sum(per.values()), min(grid_a, big or caps["big_cap"]) if merged else grid_a, per)
    if merged:
        per = family(FAMILY_R, skip)
        plan["r"] = Launch(sum(per.values()), grid_r16, per)
    elif need["need_r16"]:
        per = family(FAMILY_R16, skip)
        plan["r16"] = Launch(sum(per.values()), grid_r16, per)
    elif need["need_r32"]:
        per = family(FAMILY_R32, skip)
        plan["r32"] = Launch(sum(per.values()), grid_r32, per)
    if mfma32 and used(5):
        plan["mfma32"] = Launch(n[5], 4 * min(cells // 16 // 4 + 1, caps["mfma32"]), {5: int(n[5])})
    if mfma16 and used(4):
        plan["mfma16"] = Launch(n[4], 4 * min(cells // 4 // 4 + 1, caps["mfma16"]), {4: int(n[4])})
    if cells >= 256 and used(21, 22, 23, 24, 25, 26):
        per = {s: int(n[s]) for s in range(21, 27) if n[s]}
        plan["large"] = Launch(sum(per.values()), grid_l, per)
    plan["merged"] = merged
    return plan
