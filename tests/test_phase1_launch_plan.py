"""CPU checks of the launch rule of phase 1.  libjxl_amd/csrc/phase1_plan.h is the rule; tests/fuzz/check_phase1_plan.cc
includes it into a stand-alone program built with -fsanitize=address,undefined, which checks that RoleOf deals every
role of the merged launch exactly once and that every plan's grid is the sum of its parts, and prints the caps, the
family tables and the plan of any frame.  The restatement the GPU tests use (tests/phase1_plan.py: CAPS, FAMILY_*,
launch_plan) is held to that output; and the cases' "really loops" assertions fail when a cap exceeds the unit count --
so a retuned cap cannot quietly turn the loop tests into one-turn tests."""
import itertools
import os
import subprocess

import numpy as np
import pytest

from libjxl_amd import synth
import phase1_plan as plan
import test_gpu_phase1_loops as loops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """run(text) -> (stdout, stderr) of the compiled checker, which has passed its own sweeps."""
    out = str(tmp_path_factory.mktemp("phase1_plan") / "check_phase1_plan")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "fuzz", "check_phase1_plan.cc"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(text=""):
        r = subprocess.run([out], input=text, capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, (r.stdout[-500:], r.stderr[-4000:])
        return r.stdout, r.stderr
    return run


@pytest.fixture(scope="module")
def tables(checker):
    out, err = checker()
    return dict(line.split("=") for line in out.split()), dict(kv.split("=") for kv in err.split())


def test_roles_and_grids_under_asan_ubsan(tables):
    """The checker's own sweeps ran (they end the program on the first failure): every role index of the merged launch
    dealt exactly once over 5 x 5 x 7 x 6 geometries, the merged grid the sum of its parts over 34020 plans."""
    _, swept = tables
    assert int(swept["roles"]) >= 5 * 5 * 7 * 6 * 2 and int(swept["plans"]) >= 34020


def test_caps_of_the_loop_tests_are_the_ones_in_the_launchers(tables):
    """CAPS of tests/phase1_plan.py == the grid caps of phase1_plan.h.  If this fails after a cap was retuned: update
    CAPS there, and re-derive the turn counts in test_gpu_phase1_loops.py's docstring and DESIGN.md section 6."""
    printed, _ = tables
    source = {k: int(printed[k]) for k in plan.CAPS}
    assert source == loops.CAPS, "retuned cap: update CAPS in tests/phase1_plan.py (source %r)" % (source,)
    # the knobs: [1, 4096], anything else the built-in value; units = cells / 64
    assert int(printed["knob_max"]) == 4096 and int(printed["unit_cells"]) == 64
    assert int(printed["mfma16_min_pixels"]) == 16 << 20


def test_unit_tables_are_the_family_tables_of_the_kernels(tables):
    printed, _ = tables

    def table(name):
        return [tuple(int(v) for v in e.split(":")) for e in printed[name].split(",")]

    assert table("kFamilyA1") == loops.FAMILY_A[0]
    assert table("kFamilyA") == loops.FAMILY_A[1]
    assert table("kFamilyR") == loops.FAMILY_R
    assert table("kFamilyR16") == loops.FAMILY_R16
    assert table("kFamilyR32") == loops.FAMILY_R32


def _counts(mix, xsize, ysize):
    """Strategy counts of a frame that holds every strategy of `mix` (launch_plan and PlanPhase1 read only which are
    there; the numbers follow the area shares)."""
    covered = np.array(synth.COVERED_X, np.int64) * np.array(synth.COVERED_Y, np.int64)
    blocks = ((xsize + 7) // 8) * ((ysize + 7) // 8)
    n = np.zeros(27, np.int64)
    for s, share in mix.items():
        n[s] = max(1, int(blocks * share / sum(mix.values())) // int(covered[s]))
    return n


def test_launch_plan_agrees_with_the_compiled_plan(checker):
    """launch_plan() == PlanPhase1 over PickMfma on `merged`, on which launches happen and on every worker count."""
    hand = {18: 5, 19: 3, 6: 40, 8: 20}   # test_launch_plan_on_a_map_counted_by_hand
    mixes = [{s: 1} for s in range(27)] + [loops.MIX_A, loops.MIX_B, loops.MIX_C, loops.MIX_C16, loops.MIX_C32,
                                          loops.real4k_mix(), hand]
    knobs = (None, 1, 2, 4096, 5000)
    cases, lines = [], []
    for mix, (xs, ys) in itertools.product(mixes, ((264, 264), (520, 300), (1000, 776), (4096, 4096))):
        n = _counts(mix, xs, ys)
        used = sum(1 << s for s in range(27) if n[s])
        cells = ((xs + 255) // 256) * ((ys + 255) // 256) * 1024
        for ct, mfma, big, r in itertools.product((0, 1), (None, 0, 1), knobs, knobs):
            cases.append((n, xs, ys, ct, big, r, mfma))
            lines.append("%d %d %d 0 %d %d %d %d %d" % (
                cells, used, ct, (xs + 7) // 8, xs * ys, -1 if mfma is None else mfma,
                plan.KNOB_UNSET if big is None else big, plan.KNOB_UNSET if r is None else r))
    out, _ = checker("\n".join(lines) + "\n")
    answers = out.splitlines()
    assert len(answers) == len(cases) == 34 * 4 * 2 * 3 * 25
    for (n, xs, ys, ct, big, r, mfma), line in zip(cases, answers):
        c = {k: int(v) for k, v in (kv.split("=") for kv in line.split())}
        p = plan.launch_plan(n, xs, ys, ct, big_wgs=big, r_wgs=r, mfma=mfma)
        used = lambda *ss: any(n[s] for s in ss)  # noqa: E731
        assert (bool(c["pick32"]), bool(c["pick16"])) == plan.pick_mfma(used, xs * ys, None if mfma is None else bool(mfma))
        want = {"merged": p["merged"]}
        want.update({k: v.workers for k, v in p.items() if k != "merged"})
        got = {"merged": c["r"] != 0}
        got.update({k: v for k, v in (("a", c["big_wgs"] if c["r"] else c["a"]), ("r", c["r_wgs"]), ("r16", c["r16"]),
                                      ("r32", c["r32"]), ("large", c["large"]), ("mfma32", 4 * c["mfma32"]),
                                      ("mfma16", 4 * c["mfma16"])) if v})
        assert got == want, (line, (xs, ys, ct, big, r, mfma), p)
        assert c["r"] == c["special_wgs"] + c["big_wgs"] + c["r_wgs"] + c["dct8_wgs"]


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
