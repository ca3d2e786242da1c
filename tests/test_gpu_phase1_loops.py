"""The persistent phase-1 loops past their first turn.

Every phase-1 kernel (kernels_blocks.hip, kernels_mfma.hip) is a persistent launch: the host caps the grid
(PlanPhase1, phase1_plan.h) and a workgroup -- a wave, on the matrix cores -- walks units u, u + workers, ...,
reusing its LDS and carrying state from one varblock to the next (FamilyALoop16: the APrefetch registers, the hc / hn
header swap, the request for varblock k + 1 in front of varblock k's stores; k_transform_mfma32 / 16: the Staged
prefetch; UnitDispatch: the barrier in front of the LDS reuse; k_large: the llf / dcs tiles).  At the sizes of the
other parity tests no workgroup takes a second turn.  Here every case

  1. first PROVES that it loops: launch_plan() restates the launch rule (units per kernel from the strategy map and
     the coefficient type, workgroups from the caps and the knobs) and the case asserts its minimum turn count before
     it decodes, so that a retuned cap or a changed synth cannot quietly make it a one-turn test
     (tests/phase1_plan.py holds the restatement; tests/test_phase1_launch_plan.py pins its caps, its family tables
     and its plans to the compiled libjxl_amd/csrc/phase1_plan.h through tests/fuzz/check_phase1_plan.cc, on the
     CPU, and checks that the assertions bite);
  2. compares with the oracle at the bar of test_gpu_parity.py (TIGHT);
  3. compares, bit for bit, with the same frame decoded in a geometry where no workgroup takes a second turn
     (JXLHIP_BIG_WGS / JXLHIP_R_WGS unset at the small sizes; k_large: the frame decoded in stripes): how varblocks
     are dealt to workgroups does not enter any varblock's arithmetic.

Turn counts (launch_plan: units / workers; "a/b" = every worker takes at least a turns, some take b):
  A  1000x776 mixed, merged k_transform_r   int16, seed 5: 39 tasks (13 + 18 + 8); BIG_WGS 1 -> 39, 2 -> 19/20, 3 -> 13,
                                             7 -> 5/6.  int32, seed 10: 27 units (15 + 20/2 + 3/2); 1 -> 27, 2 -> 13/14,
                                             3 -> 9, 7 -> 3/4
  B  k_transform_a   1024x1024 all 64x32     512 / 259: 253 workgroups take two turns
                     1021x765 18/19/20       306 / 195: 111 take two turns
                     1029x781 18/19/20       int16 290 tasks, int32 184 units: BIG_WGS 1 -> all, 3 -> 96/97 and 61/62
                                             (unset: 323 workgroups, one turn: the comparison geometry)
                     3072x3072 18/19/20      int16 3636 / 1536 = 2/3 turns, int32 2246 / 1536: 710 take two
  C  row-per-lane    1000x776, 8 classes + DCT8   139 units: R_WGS 1 -> 139, 2 -> 69/70, 5 -> 27/28 (k_transform_r)
                     1000x776, {4, 6, 7}     187 units (k_transform_r16);  {5, 8 .. 11}: 92 units (k_transform_r32)
                     7680x4320, 8 classes    6731 / 4096: 2635 workgroups take two turns
                     7680x4320, {4, 6, 7}    7946 / 4096: 3850 take two
  D  k_large         4096x2048 {21, 22, 23}  911 / 512: 399 take two;  4096x4096 {21 .. 26}: 1582 / 512 = 3/4 turns
                     (stripes of two group rows: 191 .. 228 items / 256 workgroups)
  E  matrix cores    7680x4320 all DCT32X32  32400 / 8192 waves = 3/4 turns;  4096x4096 all DCT16X16: 65536 / 16384 = 4
  F  7680x4320, the shares of real_4k_d1.npz: 64-point family 1803 tasks / 512 = 3/4 turns, no knob
(what the helper printed when the module was written; the assertions below hold the minimum, not the exact count)
"""
import os

import numpy as np
import pytest
import torch

import frames
from libjxl_amd import VarDctDecoder, synth

pytestmark = pytest.mark.gpu

TIGHT = 2e-5     # test_gpu_parity.py: what the kernels are held to (relative to the range)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32 = dict(coeff_type=1, amp=200000.0, decay=3.0)   # coefficients that need 32 bits, as in test_gpu_parity.py

# ---- the launch rule, restated: tests/phase1_plan.py (held to libjxl_amd/csrc/phase1_plan.h by test_phase1_launch_plan.py)
from phase1_plan import CAPS, FAMILY_A, FAMILY_R, FAMILY_R16, FAMILY_R32, Launch, launch_plan, strategy_counts  # noqa: E402,F401


def require_turns(launch, every=None, third=None, what=""):
    """every: each worker takes at least that many turns; third: at least a third of the workers take that many."""
    print("loops %s: %r -> %d..%d turns" % (what, launch, launch.min_turns, launch.max_turns))
    if every is not None:
        assert launch.min_turns >= every, (what, launch, "every worker should take >= %d turns" % every)
    if third is not None:
        assert 3 * launch.workers_with(third) >= launch.workers, \
            (what, launch, "a third of the workers should take >= %d turns" % third)


def require_one_turn(launch, what=""):
    assert launch.max_turns <= 1, (what, launch, "the comparison geometry must not loop")


# ---- the cases' frames and their loop requirements (also called, with raised caps, by test_phase1_launch_plan.py) ----
MIX_A = {18: 4, 19: 2, 20: 2, 4: 2, 6: 1, 7: 1, 5: 2, 10: 1, 11: 1, 8: 1, 9: 1, 0: 2,
         **{s: 0.2 for s in (1, 2, 3, 12, 13, 14, 15, 16, 17)}}
SIZE_A, SEED_A, KNOBS_A = (1000, 776), {0: 5, 1: 10}, ("1", "2", "3", "7", None)  # seeds by coefficient type: see loops_a
MIX_B = {18: 2, 19: 1, 20: 1}
MIX_C = {4: 3, 6: 2, 7: 2, 5: 1, 10: 1, 11: 1, 8: 1, 9: 1}  # all eight row-per-lane classes
MIX_C16 = {4: 1, 6: 1, 7: 1}
MIX_C32 = {5: 1, 8: 1, 9: 1, 10: 1, 11: 1}
SIZE_C, KNOBS_C = (1000, 776), ("1", "2", "5", None)
SIZE_8K = (7680, 4320)


def loops_a(acs, coeff_type, caps=CAPS):
    """Case A: the merged launch with all three 64-point classes; the stated minimum (>= 5 turns at 7 workgroups,
    >= 13 at 3) is for one varblock per task, i.e. int16.  int32 units hold two 64x32 / 32x64 varblocks (kFamilyA),
    so a frame has about 2/3 as many units as tasks: there the minimum is >= 13 turns at 2, >= 9 at 3 and >= 3 at 7,
    and a two-varblock class must have an odd count (a unit whose second slot is empty).  Seed 5 gives 13 / 18 / 8
    varblocks -- both even -- so the int32 case takes seed 10: 15 / 20 / 3, i.e. 15 + 10 + 2 = 27 units."""
    n = strategy_counts(acs)
    assert n[18] and n[19] and n[20], n[18:21]
    assert any(n[s] for s in (4, 6, 7)) and any(n[s] for s in (5, 8, 9, 10, 11)) and n[0]
    assert any(n[s] for s in (1, 2, 3, 12, 13, 14, 15, 16, 17))
    if coeff_type:
        assert n[19] % 2 or n[20] % 2, n[18:21]
    want = {"7": 3, "3": 9, "2": 13, "1": 27} if coeff_type else {"7": 5, "3": 13, "2": 19, "1": 39}
    for k in KNOBS_A:
        p = launch_plan(acs, *SIZE_A, coeff_type, big_wgs=k, caps=caps)
        assert p["merged"]
        if k is None:
            require_one_turn(p["a"], "A unset")
            require_one_turn(p["r"], "A unset")
        else:
            assert p["a"].workers == int(k)
            require_turns(p["a"], every=want[k], what="A BIG_WGS=%s" % k)


def loops_b(acs, size, coeff_type, knob=None, every=None, caps=CAPS):
    """Case B: k_transform_a as a launch of its own; knob-free, a third of the workgroups take a second turn."""
    p = launch_plan(acs, *size, coeff_type, big_wgs=knob, caps=caps)
    assert not p["merged"] and "r16" not in p and "r32" not in p
    if every is not None:
        require_turns(p["a"], every=every, what="B %r BIG_WGS=%s" % (size, knob))
    else:
        require_turns(p["a"], third=2, what="B %r" % (size,))
    return p["a"]


def loops_c(acs, size, coeff_type, kernel, knob, caps=CAPS):
    """Case C: the row-per-lane units; >= 10 turns with one workgroup (>= 5 with 2, >= 2 with 5: the same units),
    knob-free at 8K a third of the workgroups take a second turn."""
    p = launch_plan(acs, *size, coeff_type, r_wgs=knob, caps=caps)
    assert kernel in p, (kernel, p)
    if knob is None and size == SIZE_C:
        require_one_turn(p[kernel], "C unset")
    elif knob is None:
        require_turns(p[kernel], third=2, what="C %r" % (size,))
    else:
        assert p[kernel].workers == int(knob)
        require_turns(p[kernel], every={"1": 10, "2": 5, "5": 2}[knob], what="C %s R_WGS=%s" % (kernel, knob))
    return p[kernel]


def loops_d(acs, size, coeff_type, stripe_rows, caps=CAPS):
    """Case D: k_large takes a second turn on a third of its workgroups; no stripe of `stripe_rows` group rows does."""
    p = launch_plan(acs, *size, coeff_type, caps=caps)
    require_turns(p["large"], third=2, what="D %r" % (size,))
    ysg = (size[1] + 255) // 256
    for g0 in range(0, ysg, stripe_rows):
        s = launch_plan(acs[g0 * 32:(g0 + stripe_rows) * 32], *size, coeff_type, group_rows=stripe_rows, caps=caps)
        require_one_turn(s["large"], "D stripe %d" % g0)


def loops_e(acs, size, coeff_type, kernel, every, caps=CAPS):
    p = launch_plan(acs, *size, coeff_type, caps=caps)
    assert kernel in p and "r16" not in p and "r32" not in p and not p["merged"], p  # the context's own rule chose it
    require_turns(p[kernel], every=every, what="E " + kernel)


def loops_f(acs, caps=CAPS):
    p = launch_plan(acs, *SIZE_8K, 0, caps=caps)
    assert p["merged"]
    require_turns(p["a"], every=3, what="F 64-point family")
    assert len(p["a"].per_class) == 3, p["a"]


def real4k_mix():
    """Area shares of the strategies in a genuine d1.0 stream (tests/data/real_4k_d1.npz): 42 % 64x64, 32 % 32x32, ..."""
    acs = np.load(os.path.join(ROOT, "tests", "data", "real_4k_d1.npz"))["ac_strategy"]
    n = np.bincount(acs.ravel() >> 1, minlength=27)
    return {int(s): float(v) for s, v in enumerate(n) if v}


# ---- decoding -------------------------------------------------------------------------------------------------------
def to_dev(t):
    return {k: ([x.cuda() for x in v] if isinstance(v, list) else v.cuda()) for k, v in t.items()}


def rel_err(got, ref):
    scale = max(1.0, float(np.abs(ref).max()))
    return float(np.abs(got.astype(np.float64) - ref).max()) / scale


@pytest.fixture(scope="module")
def dq():
    d = VarDctDecoder(0)
    p, _ = synth.synth_frame(8, 8, mix=synth.MIX_DCT8)
    d.begin_frame(p)
    t = d.default_dequant_tables()
    d.sync()
    yield t
    d.close()


def setenv(monkeypatch, **kw):
    for k, v in kw.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))


def decode(params, devt, dq, monkeypatch, frame=False, **env):
    """The phase-1 planes [3 arrays] (frame=False) or decode_frame's output under the environment `env`; a context of
    its own, since a context samples the switches when it is created."""
    setenv(monkeypatch, **env)
    d = VarDctDecoder(0)
    try:
        d.begin_frame(params)
        d.set_inputs(devt, dq)
        if frame:
            out = d.decode_frame()
            d.sync()
            return out.cpu().numpy()
        d.decode_blocks()
        d.sync()
        return d.export_xyb()
    finally:
        d.close()


def first_varblock(diff_at, acs):
    """(by, bx, strategy) of the varblock that holds the first differing sample (for the failure message)."""
    if not len(diff_at):
        return None
    y, x = int(diff_at[0][0]) // 8, int(diff_at[0][1]) // 8
    acs = np.asarray(acs)
    s = int(acs[y, x]) >> 1
    while x > 0 and not acs[y, x] & 1 and (acs[y, x - 1] >> 1) == s:
        x -= 1
    while y > 0 and not acs[y, x] & 1 and (acs[y - 1, x] >> 1) == s:
        y -= 1
    return (y, x, s)


def check_planes(outs, base, ref, acs):
    """outs: {knob: planes}; each within TIGHT of the oracle and bit-equal to outs[base]."""
    for k, got in outs.items():
        for c in range(3):
            assert rel_err(got[c], ref[c]) <= TIGHT, \
                (k, c, rel_err(got[c], ref[c]), first_varblock(np.argwhere(np.abs(got[c] - ref[c]) > 1e-3), acs))
    for k, got in outs.items():
        for c in range(3):
            assert np.array_equal(got[c], outs[base][c]), \
                (k, c, first_varblock(np.argwhere(got[c] != outs[base][c]), acs))


# ---- A: the 64-point family inside the merged launch ------------------------------------------------------------------
@pytest.mark.parametrize("coeff_type", [0, 1])
def test_big_wgs_family_a_in_the_merged_launch_loops(dq, oracle, coeff_type, monkeypatch):
    """FamilyALoop16 (int16) / UnitDispatch<kFamilyA> with two-varblock units (int32) on the first JXLHIP_BIG_WGS
    workgroups of k_transform_r: one workgroup walks every task across both class boundaries; two, three and seven
    give strides where the current and the prefetched varblock differ in class, and last turns right after a class
    change.  Ragged frame, every role of the merged grid present."""
    params, t, fr = frames.make_case(*SIZE_A, mix=MIX_A, gab=False, epf_iters=0, seed=SEED_A[coeff_type], **(I32 if coeff_type else {}))
    acs = t["ac_strategy"].numpy()
    loops_a(acs, coeff_type)
    devt = to_dev(t)
    outs = {k: decode(params, devt, dq, monkeypatch, JXLHIP_BIG_WGS=k) for k in KNOBS_A}
    check_planes(outs, None, fr.decode_groups(), acs)


@pytest.mark.parametrize("fuse", ["1", "0"])
def test_big_wgs_family_a_loops_in_front_of_both_filter_paths(dq, oracle, fuse, monkeypatch):
    """The same frame through decode_frame with Gaborish + EPF1: phase 1 in front of the fused kernel and of the
    two-phase filter march."""
    params, t, fr = frames.make_case(*SIZE_A, mix=MIX_A, gab=True, epf_iters=1, seed=SEED_A[0])
    acs = t["ac_strategy"].numpy()
    loops_a(acs, 0)
    devt = to_dev(t)
    outs = {k: decode(params, devt, dq, monkeypatch, frame=True, JXLHIP_FUSE=fuse, JXLHIP_BIG_WGS=k) for k in KNOBS_A}
    ref = fr.decode(threads=4)
    for k, got in outs.items():
        assert rel_err(got, ref) <= TIGHT, (k, np.argwhere(np.abs(got - ref) > 1e-3)[:5])
    for k, got in outs.items():
        assert np.array_equal(got, outs[None]), (k, np.argwhere(got != outs[None])[:5])


# ---- B: k_transform_a as a launch of its own --------------------------------------------------------------------------
@pytest.mark.parametrize("size,mix,coeff_type", [((1024, 1024), {19: 1}, 0), ((1021, 765), MIX_B, 0),
                                                 ((3072, 3072), MIX_B, 0), ((3072, 3072), MIX_B, 1)])
def test_big_wgs_unset_k_transform_a_loops_on_its_own_grid(dq, oracle, size, mix, coeff_type, monkeypatch):
    """No row-per-lane class in the frame: k_transform_a, grid_a = min(units + 3, 1536) workgroups, and more 64-point
    tasks than that.  (1021x765 rather than 1029x781 for the knob-free case with class changes: the grid follows the
    frame's GROUPS, 20 of them at 1029x781 -- 323 workgroups for 311 tasks, one turn; 12 groups at 1021x765.)
    Compared with JXLHIP_BIG_WGS = 128 and 1, which deal the same varblocks differently."""
    params, t, fr = frames.make_case(*size, mix=mix, gab=False, epf_iters=0, seed=41, **(I32 if coeff_type else {}))
    acs = t["ac_strategy"].numpy()
    loops_b(acs, size, coeff_type)
    knobs = (None, "128") + (("1",) if size[0] < 3072 else ())
    for k in knobs[1:]:
        assert loops_b(acs, size, coeff_type, knob=k, every=1).workers == int(k)
    devt = to_dev(t)
    outs = {k: decode(params, devt, dq, monkeypatch, JXLHIP_BIG_WGS=k) for k in knobs}
    check_planes(outs, None, fr.decode_groups(), acs)


@pytest.mark.parametrize("coeff_type", [0, 1])
def test_big_wgs_caps_the_grid_of_k_transform_a(dq, oracle, coeff_type, monkeypatch):
    """1029x781 with 64x64, 64x32 and 32x64 only: one workgroup walks every task, three take ~100 turns each with
    class changes; unset, no workgroup takes a second turn."""
    size = (1029, 781)
    params, t, fr = frames.make_case(*size, mix=MIX_B, gab=False, epf_iters=0, seed=43, **(I32 if coeff_type else {}))
    acs = t["ac_strategy"].numpy()
    n = strategy_counts(acs)
    assert n[18] and n[19] and n[20], n[18:21]
    require_one_turn(loops_b(acs, size, coeff_type, every=0), "B unset")
    tasks = loops_b(acs, size, coeff_type, knob="1", every=100).units
    loops_b(acs, size, coeff_type, knob="3", every=tasks // 3)
    devt = to_dev(t)
    outs = {k: decode(params, devt, dq, monkeypatch, JXLHIP_BIG_WGS=k) for k in ("1", "3", None)}
    check_planes(outs, None, fr.decode_groups(), acs)


# ---- C: the row-per-lane units -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("coeff_type", [0, 1])
@pytest.mark.parametrize("mix,kernel", [(MIX_C, "r"), (MIX_C16, "r16"), (MIX_C32, "r32")], ids=["r", "r16", "r32"])
def test_r_wgs_row_per_lane_units_loop(dq, oracle, mix, kernel, coeff_type, monkeypatch):
    """JXLHIP_R_WGS workgroups for the row-per-lane families: with one, a single workgroup of k_transform_r runs 32-,
    16- and 8-point LDS transposes back to back through the same allocation (RowLaneUnit<..., true>), and the
    stand-alone kernels k_transform_r16 / _r32 walk all their classes in one workgroup.  DCT8 cells (the mix's own, or
    synth's fill where nothing else fits) ride along.  (No mix here leaves DCT32X32 or DCT16X16 alone in its family, so
    the context's rule keeps every class on the butterflies without JXLHIP_MFMA = 0.)"""
    mix = {**mix, 0: 1} if kernel == "r" else mix
    params, t, fr = frames.make_case(*SIZE_C, mix=mix, gab=False, epf_iters=0, seed=61, **(I32 if coeff_type else {}))
    acs = t["ac_strategy"].numpy()
    n = strategy_counts(acs)
    want = [s for s, _ in {"r": FAMILY_R, "r16": FAMILY_R16, "r32": FAMILY_R32}[kernel]]
    assert all(n[s] for s in want), n
    for k in KNOBS_C:
        unit = loops_c(acs, SIZE_C, coeff_type, kernel, k)
        assert set(unit.per_class) == set(want)
    devt = to_dev(t)
    outs = {k: decode(params, devt, dq, monkeypatch, JXLHIP_R_WGS=k) for k in KNOBS_C}
    check_planes(outs, None, fr.decode_groups(), acs)


@pytest.fixture(scope="module", params=["r", "r16"])
def frame_8k_row_lane(request, oracle):
    mix = MIX_C if request.param == "r" else MIX_C16
    params, t, fr = frames.make_case(*SIZE_8K, mix=mix, gab=False, epf_iters=0, seed=63)
    return request.param, params, t, fr


def test_r_wgs_unset_row_per_lane_units_loop_at_8k(dq, frame_8k_row_lane, monkeypatch):
    """Knob-free at full size: more row-per-lane units than the 4096 workgroups of grid_r16.  The comparison geometry
    is JXLHIP_R_WGS = 1024 (every workgroup loops, over other units)."""
    kernel, params, t, fr = frame_8k_row_lane
    acs = t["ac_strategy"].numpy()
    loops_c(acs, SIZE_8K, 0, kernel, None)
    assert launch_plan(acs, *SIZE_8K, 0, r_wgs="1024")[kernel].workers == 1024
    devt = to_dev(t)
    outs = {k: decode(params, devt, dq, monkeypatch, JXLHIP_R_WGS=k) for k in (None, "1024")}
    check_planes(outs, None, fr.decode_groups(), acs)


# ---- D: k_large ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coeff_type", [0, 1])
@pytest.mark.parametrize("size,mix", [((4096, 2048), {21: 1, 22: 1, 23: 1}), ((4096, 4096), {s: 1 for s in range(21, 27)})])
def test_k_large_items_loop(dq, oracle, size, mix, coeff_type, monkeypatch):
    """k_large: item += gridDim.x with the llf / dcs tiles reused per item; more 128x64 .. 256x256 varblocks than the
    512 workgroups of grid_l.  There is no geometry knob: the comparison is the same frame decoded in stripes of two
    group rows, each with fewer items than workgroups (its rows must equal the whole frame's bit for bit).
    JXLHIP_FUSE = 0: a stripe of a frame of 12 Mpx and more would otherwise leave its DCT8 cells to the fused kernel."""
    params, t, fr = frames.make_case(*size, mix=mix, gab=False, epf_iters=0, seed=71, **(I32 if coeff_type else {}))
    acs = t["ac_strategy"].numpy()
    loops_d(acs, size, coeff_type, stripe_rows=2)
    devt = to_dev(t)
    whole = decode(params, devt, dq, monkeypatch, JXLHIP_FUSE="0")
    ref = fr.decode_groups()
    for c in range(3):
        assert rel_err(whole[c], ref[c]) <= TIGHT, (c, first_varblock(np.argwhere(np.abs(whole[c] - ref[c]) > 1e-3), acs))
    for g0 in range(0, (size[1] + 255) // 256, 2):
        part = decode(dict(params, stripe_group_y0=g0, stripe_group_rows=2), devt, dq, monkeypatch, JXLHIP_FUSE="0")
        for c in range(3):
            rows = whole[c][g0 * 256:g0 * 256 + part[c].shape[0]]
            assert np.array_equal(part[c], rows), (g0, c, first_varblock(np.argwhere(part[c] != rows), acs[g0 * 32:]))


# ---- E: the matrix-core kernels ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frame_8k_dct32(oracle):
    return frames.make_case(*SIZE_8K, mix=synth.MIX_DCT32, gab=False, epf_iters=0, seed=81)


@pytest.mark.parametrize("gab,epf", [(0, 0), (1, 1)])
def test_mfma32_int16_waves_loop_at_8k(dq, frame_8k_dct32, gab, epf, monkeypatch):
    """k_transform_mfma32<int16_t> (the context's own rule: DCT32X32 alone among the 32-point classes): 32400
    varblocks over 8192 waves, the Staged prefetch carried over three or four turns.  Without filters it is the EMIT
    form, with Gaborish + EPF1 the plane-writing one.  Against the butterflies only "not equal": the rule engaged."""
    params, t, _ = frame_8k_dct32
    params = dict(params, gab=gab, epf_iters=epf)
    fr = frames.oracle_frame(params, t, __import__("oracle").default_dequant_tables())
    loops_e(t["ac_strategy"].numpy(), SIZE_8K, 0, "mfma32", every=3)
    devt = to_dev(t)
    ref = fr.decode(threads=8)
    outs = {m: decode(params, devt, dq, monkeypatch, frame=True, JXLHIP_MFMA=m) for m in (None, "0")}
    assert rel_err(outs[None], ref) <= TIGHT, np.argwhere(np.abs(outs[None] - ref) > 1e-3)[:5]
    assert rel_err(outs["0"], ref) <= TIGHT
    assert not np.array_equal(outs[None], outs["0"])


def test_mfma16_int32_waves_loop_at_16_mpx(dq, oracle, monkeypatch):
    """The int32 form of test_all_dct16_frame_of_16_mpx_takes_the_matrix_cores_by_default: k_transform_mfma16<int32_t>,
    65536 varblocks over 16384 waves."""
    size = (4096, 4096)
    params, t, fr = frames.make_case(*size, mix={4: 1.0}, gab=False, epf_iters=0, seed=77, **I32)
    assert int(t["coeffs"][1].abs().max()) > 32767
    loops_e(t["ac_strategy"].numpy(), size, 1, "mfma16", every=4)
    devt = to_dev(t)
    ref = fr.decode(threads=8)
    outs = {m: decode(params, devt, dq, monkeypatch, frame=True, JXLHIP_MFMA=m) for m in (None, "0")}
    assert rel_err(outs[None], ref) <= TIGHT, np.argwhere(np.abs(outs[None] - ref) > 1e-3)[:5]
    assert rel_err(outs["0"], ref) <= TIGHT
    assert not np.array_equal(outs[None], outs["0"])


# ---- F: the genuine shares -----------------------------------------------------------------------------------------------
def test_genuine_shares_at_8k_loop_in_the_64_point_family(dq, oracle, monkeypatch):
    """The workload README quotes (the strategy shares of a genuine d1.0 stream, 8K, int16, Gaborish + EPF1, default
    switches) against the oracle: >= 3 turns per workgroup in the 64-point family with class changes, no knob set."""
    params, t, fr = frames.make_case(*SIZE_8K, mix=real4k_mix(), gab=True, epf_iters=1)
    loops_f(t["ac_strategy"].numpy())
    for k in ("JXLHIP_BIG_WGS", "JXLHIP_R_WGS", "JXLHIP_MFMA", "JXLHIP_FUSE"):
        monkeypatch.delenv(k, raising=False)
    got = decode(params, to_dev(t), dq, monkeypatch, frame=True)
    ref = fr.decode(threads=8)
    assert rel_err(got, ref) <= TIGHT, np.argwhere(np.abs(got - ref) > 1e-3)[:5]
