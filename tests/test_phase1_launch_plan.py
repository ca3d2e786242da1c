"""CPU checks of the launch rule restated in tests/test_gpu_phase1_loops.py (launch_plan, CAPS): the caps are the ones
in the source text of LaunchBlocksT and LaunchMfma32 / LaunchMfma16, and the cases' "really loops" assertions fail when a
cap exceeds the unit count -- so a retuned cap cannot quietly turn the loop tests into one-turn tests."""
import os
import re

import numpy as np
import pytest

from libjxl_amd import synth
import test_gpu_phase1_loops as loops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libjxl_amd", "csrc")


def function_text(path, name):
    """The definition of `name` (a function at namespace scope, closing brace in column 0)."""
    text = open(os.path.join(CSRC, path)).read()
    m = re.search(r"^(?:static )?void %s\([^;{]*\{.*?^\}" % name, text, re.S | re.M)
    assert m, "%s not found in %s" % (name, path)
    return m.group(0)


def one(pattern, text, what):
    found = re.findall(pattern, text)
    assert len(found) == 1, "%s: %r matches %d times -- update the pattern here and CAPS in test_gpu_phase1_loops.py" % (
        what, pattern, len(found))
    return int(found[0])


def test_caps_of_the_loop_tests_are_the_ones_in_the_launchers():
    """CAPS of tests/test_gpu_phase1_loops.py == the grid caps in the source.  If this fails after a cap was retuned:
    update CAPS there, and re-derive the turn counts in that module's docstring and DESIGN.md section 6."""
    blocks = function_text("kernels_blocks.hip", "LaunchBlocksT")
    m32 = function_text("kernels_mfma.hip", "LaunchMfma32")
    m16 = function_text("kernels_mfma.hip", "LaunchMfma16")
    source = dict(
        grid_a=one(r"grid_a = units \+ 3 < (\d+)u \? units \+ 3 : \1u;", blocks, "grid_a"),
        grid_r16=one(r"grid_r16 = units \+ 3 < (\d+)u \? units \+ 3 : \1u;", blocks, "grid_r16"),
        grid_r32=one(r"grid_r32 = units / 2 \+ 5 < (\d+)u \? units / 2 \+ 5 : \1u;", blocks, "grid_r32"),
        grid_l=one(r"grid_l = cells / 128 < (\d+)u \? \(cells / 128 \? cells / 128 : 1\) : \1u;", blocks, "grid_l"),
        big_cap=one(r"big_cap = big_set \? \(uint32_t\)big_env : (\d+)u;", blocks, "big_cap"),
        mfma32=one(r"grid = cells / 16 / 4 \+ 1;[^\n]*\n\s*if \(grid > (\d+)u\) grid = \1u;", m32, "LaunchMfma32"),
        mfma16=one(r"grid = cells / 4 / 4 \+ 1;[^\n]*\n\s*if \(grid > (\d+)u\) grid = \1u;", m16, "LaunchMfma16"))
    assert source == loops.CAPS, "retuned cap: update CAPS in tests/test_gpu_phase1_loops.py (source %r)" % (source,)
    # the knobs: [1, 4096], anything else the built-in value; units = cells / 64
    assert one(r"big_set = big_env >= 1 && big_env <= (\d+);", blocks, "JXLHIP_BIG_WGS range") == 4096
    assert one(r"if \(r_env >= 1 && r_env <= (\d+)\)", blocks, "JXLHIP_R_WGS range") == 4096
    assert one(r"const uint32_t units = cells / (\d+);", blocks, "units") == 64


def test_unit_tables_are_the_family_tables_of_the_kernels():
    text = open(os.path.join(CSRC, "kernels_blocks.hip")).read()
    medium = re.search(r"kMediumStrategy\[\w*\]\s*=\s*\{([^}]*)\}", open(os.path.join(CSRC, "dev_common.h")).read())
    assert medium, "kMediumStrategy not found"
    strategy = [int(v) for v in medium.group(1).split(",")]

    def table(name):
        m = re.search(r"FamilyEntry %s\[\d+\] = \{(.*?)\};" % name, text, re.S)
        assert m, name
        return [(strategy[int(i)], int(vb)) for i, vb in re.findall(r"\{kClsMedium0 \+ (\d+), (\d+)\}", m.group(1))]

    assert table("kFamilyA1") == loops.FAMILY_A[0]
    assert table("kFamilyA") == loops.FAMILY_A[1]
    assert table("kFamilyR") == loops.FAMILY_R
    assert table("kFamilyR16") == loops.FAMILY_R16
    assert table("kFamilyR32") == loops.FAMILY_R32


def test_launch_plan_on_a_map_counted_by_hand():
    """520x300 (3 x 2 groups: 6144 cells, 96 units): 5 varblocks of 64x64, 3 of 64x32, 40 of 16x8, 20 of 32x8."""
    acs = np.zeros((38, 65), np.uint8)
    acs[0, :5], acs[1, :3], acs[2, :40], acs[3, :20] = (18 << 1) | 1, (19 << 1) | 1, (6 << 1) | 1, (8 << 1) | 1
    p = loops.launch_plan(acs, 520, 300, 0)
    assert p["merged"] and (p["a"].units, p["a"].workers) == (8, 99) and (p["r"].units, p["r"].workers) == (3, 99)
    assert p["r"].per_class == {8: 1, 6: 2}
    p = loops.launch_plan(acs, 520, 300, 1, big_wgs="2", r_wgs="5000")
    assert (p["a"].units, p["a"].workers, p["a"].min_turns, p["a"].max_turns) == (7, 2, 3, 4)
    assert p["a"].workers_with(4) == 1 and p["a"].workers_with(3) == 2 and p["a"].workers_with(5) == 0
    assert p["r"].workers == 99  # out of range: the built-in value
    acs[3, :20] = 1  # DCT8 instead of 32x8: one row-per-lane family only -> the stand-alone kernels
    p = loops.launch_plan(acs, 520, 300, 0, big_wgs="2", r_wgs="1")
    assert not p["merged"] and p["a"].workers == 2 and (p["r16"].units, p["r16"].workers) == (2, 1) and "r32" not in p
    acs[2, :40] = (5 << 1) | 1  # DCT32X32 alone in its family: the matrix cores, 4 waves per workgroup
    p = loops.launch_plan(acs, 520, 300, 0)
    assert "r32" not in p and (p["mfma32"].units, p["mfma32"].workers) == (40, 4 * 97)
    assert loops.launch_plan(acs, 520, 300, 0, mfma="0")["r32"].units == 5
    acs[4, :3] = (21 << 1) | 1
    assert (lambda l: (l.units, l.workers))(loops.launch_plan(acs, 520, 300, 0)["large"]) == (3, 48)
    assert loops.launch_plan(acs[:32], 520, 300, 0, group_rows=1)["large"].workers == 24


RAISED = {k: 1 << 20 for k in loops.CAPS}


def _acs(size, mix, seed, **kw):
    return synth.synth_frame(*size, mix=mix, gab=False, epf_iters=0, seed=seed, **kw)[1]["ac_strategy"].numpy()


def test_small_cases_loop_and_their_assertions_bite():
    """The loop requirements of the small cases hold on the CPU (the strategy map does not need a device).  Their
    workgroup counts come from a knob or from the frame's group count (units + 3), not from a cap: the assertions fail
    when the frame has fewer units instead -- here, a much smaller frame."""
    for ct in (0, 1):
        kw = loops.I32 if ct else {}
        loops.loops_a(_acs(loops.SIZE_A, loops.MIX_A, loops.SEED_A[ct], **kw), ct)
        with pytest.raises(AssertionError):
            loops.loops_a(_acs((504, 392), loops.MIX_A, loops.SEED_A[ct], **kw), ct)
    for size, mix in (((1024, 1024), {19: 1}), ((1021, 765), loops.MIX_B)):
        loops.loops_b(_acs(size, mix, 41), size, 0)
        with pytest.raises(AssertionError, match="a third of the workers"):
            loops.loops_b(_acs((size[0] // 2, size[1] // 2), mix, 41), size, 0)
    for mix, kernel in ((loops.MIX_C, "r"), (loops.MIX_C16, "r16"), (loops.MIX_C32, "r32")):
        mix = {**mix, 0: 1} if kernel == "r" else mix
        acs = _acs(loops.SIZE_C, mix, 61)
        for k in loops.KNOBS_C:
            loops.loops_c(acs, loops.SIZE_C, 0, kernel, k)
        with pytest.raises(AssertionError, match="every worker"):
            loops.loops_c(_acs((120, 96), mix, 61), loops.SIZE_C, 0, kernel, "1")


def test_knob_free_cases_fail_their_loop_assertion_under_raised_caps():
    """The cases whose workgroup count IS a cap (3072x3072 and up): with the caps raised past the unit counts their
    "really loops" assertions fail, with the caps of the source they hold."""
    def bites(check, *args):
        check(*args)
        with pytest.raises(AssertionError, match="should take"):
            check(*args, caps=RAISED)

    acs = _acs((3072, 3072), loops.MIX_B, 41)
    bites(loops.loops_b, acs, (3072, 3072), 1)
    bites(loops.loops_c, _acs(loops.SIZE_8K, loops.MIX_C, 63), loops.SIZE_8K, 0, "r", None)
    bites(loops.loops_c, _acs(loops.SIZE_8K, loops.MIX_C16, 63), loops.SIZE_8K, 0, "r16", None)
    bites(loops.loops_d, _acs((4096, 2048), {21: 1, 22: 1, 23: 1}, 71), (4096, 2048), 0, 2)
    bites(loops.loops_d, _acs((4096, 4096), {s: 1 for s in range(21, 27)}, 71), (4096, 4096), 0, 2)
    bites(loops.loops_e, _acs(loops.SIZE_8K, synth.MIX_DCT32, 81), loops.SIZE_8K, 0, "mfma32", 3)
    bites(loops.loops_e, _acs((4096, 4096), {4: 1.0}, 77), (4096, 4096), 1, "mfma16", 4)
    bites(loops.loops_f, _acs(loops.SIZE_8K, loops.real4k_mix(), 0x4A584C))
