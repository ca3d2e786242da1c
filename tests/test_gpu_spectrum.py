"""Every inverse transform over its WHOLE spectrum, on every launch that implements it, against the libjxl reference
decoder with its own dequant tables.

synth.synth_frame's default spectrum leaves the upper band of every transform at zero (45 % to 83 % of a strategy's
positions on the frames of test_gpu_parity.py::test_blocks_each_strategy), so those frames cannot see a wrong dequant
entry, IDCT row / column or transpose there.  The frames of spectrum.py put energy everywhere: flat frames (decay 0)
and impulse frames (one non-zero per varblock and channel, or up to four diagonals in the large ones), the latter in
one amplitude class per frame: "large" (every impulse of the same dequantised amplitude, so every position is of the
size of the frame's range; split into several frames for 128x128 and larger) and "small" (+1 .. -300).  Every frame
runs here.  test_spectrum_model.py shows on the CPU that the frames meet their population conditions, that the oracle
equals the reference on them bit for bit, that one table entry raised by 1 % moves the "large" frames decoded here by
>= 5x the bar at four named positions of every strategy (at every position of four strategies), and that a doubled
entry moves the flat frames by as much; a 1 % fault under a small value, or on a flat frame, is below the bar.

Each case builds its own decoder under its switches, asserts from used_acs which launch LaunchBlocksT takes
(spectrum.launch_of restates the rule), decodes once and compares per channel: max|got_c - want_c| <= 2e-5 *
max(max|want_c|, 1e-3) (frames.check_channels).  It prints "WORST <path> <strategy> <kind> c0 c1 c2"."""
import os

import numpy as np
import pytest
import torch

import frames
import spectrum as sp
from frames import check_channels

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)
ALONE = {"JXLHIP_FUSE": "0", "JXLHIP_MFMA": "0"}
MFMA = {"JXLHIP_FUSE": "0", "JXLHIP_MFMA": "1"}
MERGED_IMPULSE = list(range(4, 12)) + [18, 19, 20]


def kinds(s):
    """"flat" and the impulse frames of strategy s ("large", or "large0" .. where the class is split, and "small")."""
    return ["flat"] + list(sp.amplitudes(s))


TYPE = {0: "i16", 1: "i32"}


@pytest.fixture(scope="module")
def ref(oracle):
    if not oracle.ref_available():
        pytest.fail("oracle/_ref/libjxl_ref.so missing: run __graft_entry__.build() in the build container")
    oracle.ref_lib()
    return oracle


def to_dev(t):
    return {k: ([x.cuda() for x in v] if isinstance(v, list) else v.cuda()) for k, v in t.items()}


def reference(ref, params, t):
    return sp.reference_frame(ref, params, t).decode_ref(threads=THREADS)


def case_of(kind, s, coeff_type, **kw):
    """(params, tensors) of the flat or impulse frame, its population conditions checked on the frame itself."""
    merged = kw.get("merged", False)
    if kind == "flat":
        params, t = sp.flat_case(s, coeff_type, **kw)
        sp.check_flat_values(t, coeff_type)
        sp.check_flat_population(t, s)
    else:
        params, t = sp.impulse_case(s, coeff_type, kind, **kw)
        sp.check_impulse_population(params, t, s, coeff_type, kind, exact=not merged)
    return params, t


def decoder(env, monkeypatch):
    from libjxl_amd import VarDctDecoder
    for k in ("JXLHIP_FUSE", "JXLHIP_FILTERS", "JXLHIP_MFMA", "JXLHIP_FUSED_PC_RH", "JXLHIP_SPARSE_UPLOAD"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return VarDctDecoder(0)


def decode_planes(params, t, env, monkeypatch):
    """decode_blocks + export_xyb under `env`: the phase-1 XYB planes, (3, ysize, xsize)."""
    d = decoder(env, monkeypatch)
    try:
        d.begin_frame(params)
        d.set_inputs(to_dev(t), d.default_dequant_tables())
        d.decode_blocks()
        d.sync()
        return np.stack([p[:params["ysize"], :params["xsize"]] for p in d.export_xyb()])
    finally:
        d.close()


def decode_frame(params, t, env, monkeypatch):
    """decode_frame under `env`: (output, profile slots, whether the planes hold the whole frame afterwards).  A
    two-phase decode leaves every block in the XYB planes and jxlhip_export_xyb hands them out; a fused one
    (k_fused_pc, k_fused_pc0: the DCT8 blocks never reach the planes) and the class kernel that writes the pixels
    itself leave them incomplete, and the export is refused."""
    from libjxl_amd import abi
    d = decoder(env, monkeypatch)
    try:
        d.begin_frame(params)
        d.set_inputs(to_dev(t), d.default_dequant_tables())
        d.profile(True)
        o = d.decode_frame().cpu().numpy()
        d.sync()
        slots = d.profile_read()
        try:
            d.export_xyb()
            whole = True
        except abi.JxlHipError:
            whole = False
        return o, slots, whole
    finally:
        d.close()


def name(s, kind, coeff_type):
    return "%d %s_%s" % (s, kind, TYPE[coeff_type])


# ---- alone: k_transform_8, k_transform_r16 / _r32 (RowLaneUnit<..., false>), k_transform_a, k_large ------------------------
@pytest.mark.parametrize("coeff_type", [0, 1])
@pytest.mark.parametrize("s,kind", [(s, k) for s in sp.STRATEGIES for k in kinds(s)])
def test_alone(ref, s, kind, coeff_type, monkeypatch):
    """One strategy (flat: with DCT8 filler) through the launches of its own class: the row-per-lane families are not
    merged, so k_transform_8, k_transform_r16 or _r32, k_transform_a and k_large run as separate kernels."""
    params, t = case_of(kind, s, coeff_type)
    launch = sp.launch_of(params["used_acs"], mfma=0)
    assert not launch["merged"] and sp.used_set(params) <= {s, 0}
    assert launch["need_r16"] == (s in (4, 6, 7)) and launch["need_r32"] == (s in (5, 8, 9, 10, 11))
    got = decode_planes(params, t, ALONE, monkeypatch)
    check_channels("alone", name(s, kind, coeff_type), got, reference(ref, params, t), axis=0)


# ---- merged: SpecialWorkgroup, Dct8Rows, RowLaneUnit<..., true>, FamilyALoop16 / MediumUnit inside k_transform_r -----------
@pytest.mark.parametrize("coeff_type", [0, 1])
@pytest.mark.parametrize("s,kind", [(s, k) for s in range(21) for k in (kinds(s) if s in MERGED_IMPULSE else ["flat"])])
def test_merged(ref, s, kind, coeff_type, monkeypatch):
    """The same strategy with a small share of 16x8 and 32x8 varblocks: both row-per-lane families have work, so one
    k_transform_r launch carries the single-block classes, DCT8, the LDS-staged 64-point classes (FamilyALoop16 for
    int16, MediumUnit for int32) and the row-per-lane units that transpose through LDS.  Impulse form: the filler
    varblocks carry zeros."""
    params, t = case_of(kind, s, coeff_type, merged=True)
    assert sp.launch_of(params["used_acs"], mfma=0)["merged"] and {s, 6, 8} <= sp.used_set(params)
    got = decode_planes(params, t, ALONE, monkeypatch)
    check_channels("merged", name(s, kind, coeff_type), got, reference(ref, params, t), axis=0)


# ---- matrix cores -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coeff_type", [0, 1])
@pytest.mark.parametrize("merged", [False, True], ids=["alone", "merged"])
@pytest.mark.parametrize("kind", kinds(4))
@pytest.mark.parametrize("s", [4, 5])
def test_matrix_cores(ref, s, kind, merged, coeff_type, monkeypatch):
    """JXLHIP_MFMA=1: DCT16X16 / DCT32X32 leave the row-per-lane families for k_transform_mfma16 / _mfma32, next to
    the unmerged launches (alone) or to k_transform_r (merged: the filler keeps both families busy).  The planes
    differ from the butterflies' (a dense product rounds differently): the matrix cores really ran."""
    params, t = case_of(kind, s, coeff_type, merged=merged)
    assert sp.launch_of(params["used_acs"], mfma=1)["merged"] == merged and s in sp.used_set(params)
    want = reference(ref, params, t)
    got = decode_planes(params, t, MFMA, monkeypatch)
    check_channels("mfma_merged" if merged else "mfma_alone", name(s, kind, coeff_type), got, want, axis=0)
    assert not np.array_equal(got, decode_planes(params, t, ALONE, monkeypatch))


@pytest.mark.parametrize("coeff_type", [0, 1])
@pytest.mark.parametrize("kind", kinds(5))
def test_dct32_only_frame_written_by_the_class_kernel(ref, kind, coeff_type, monkeypatch):
    """All DCT32X32, no loop filter, linear RGB out: k_transform_mfma32<EMIT> applies the opsin inverse and writes the
    pixels itself -- no filter kernel runs.  Against the reference's RGB."""
    params, t = sp.dct32_only_flat(coeff_type) if kind == "flat" else sp.dct32_only_impulse(coeff_type, kind)
    assert params["used_acs"] == 1 << 5 and params["output_kind"] == 1 and not params["gab"] and not params["epf_iters"]
    (sp.check_flat_population(t, 5) if kind == "flat" else sp.check_impulse_population(params, t, 5, coeff_type, kind, True))
    got, slots, whole = decode_frame(params, t, MFMA, monkeypatch)
    assert "blocks" in slots and "filters" not in slots and "fused" not in slots and not whole, slots
    check_channels("mfma32_emit", name(5, kind, coeff_type), got, reference(ref, params, t), axis=2)


# ---- fused: the DCT8 decode inside k_fused_pc / k_fused_pc0 ----------------------------------------------------------------
def fused_case(ref, params, t, path, label, monkeypatch):
    epf = params["epf_iters"]
    got, slots, whole = decode_frame(params, t, {"JXLHIP_FUSE": "1"}, monkeypatch)
    check_channels(path, label, got, reference(ref, params, t), axis=2)
    assert not whole  # the fused producer ran: the DCT8 blocks are not in the planes
    if epf == 3:  # k_fused_pc0 feeds the EPF1 + EPF2 march: the two-phase decode (k_epf0) bit for bit
        assert "epf0" in slots, slots
        two, _, two_whole = decode_frame(params, t, {"JXLHIP_FUSE": "0"}, monkeypatch)
        assert two_whole  # ... and that one really was the two-phase path
        assert np.array_equal(got, two), np.argwhere(got != two)[:5]
    else:
        assert "fused" in slots and "filters" not in slots, slots


@pytest.mark.parametrize("coeff_type", [0, 1])
@pytest.mark.parametrize("gab,epf", [(0, 0), (1, 1), (1, 3)])
@pytest.mark.parametrize("kind", kinds(0))
def test_fused_dct8(ref, kind, gab, epf, coeff_type, monkeypatch):
    """JXLHIP_FUSE=1, every block DCT8: the producer of k_fused_pc (k_fused_pc0 at three EPF iterations) decodes them
    itself; linear RGB against the reference."""
    params, t = case_of(kind, 0, coeff_type, gab=bool(gab), epf=epf, output_kind=1)
    assert sp.used_set(params) == {0}
    fused_case(ref, params, t, "fused_g%de%d" % (gab, epf), name(0, kind, coeff_type), monkeypatch)


@pytest.mark.parametrize("coeff_type", [0, 1])
def test_fused_every_strategy(ref, coeff_type, monkeypatch):
    """A flat frame of every strategy through k_fused_pc: DCT8 in the producer, the other classes copied from the
    planes the block kernels wrote."""
    params, t = sp.flat_case(0, coeff_type, gab=True, epf=1, output_kind=1, size=sp.FUSED_MIX_SIZE, mix_all=True,
                             seed=sp.FUSED_MIX_SEED)
    sp.check_flat_values(t, coeff_type)
    used = sp.used_set(params)
    assert 0 in used and len(used) >= 12 and sp.launch_of(params["used_acs"], mfma=0)["merged"]
    sp.check_flat_population(t, 0)  # (the other classes have their own frames above; here they come from the planes)
    fused_case(ref, params, t, "fused_mix_g1e1", "all flat_" + TYPE[coeff_type], monkeypatch)


# ---- hand-over: dense fallback and sparse groups in one frame ------------------------------------------------------------------
def test_handover_mixes_dense_and_sparse_groups(ref, monkeypatch):
    """jxlhip_ac_group_decode_submit on a flat int16 frame whose full group holds more non-zeros in X and B than a
    chroma list of the sparse form takes (it goes up densely) while the clipped groups stay sparse: the pixels of the
    device-resident decode, bit for bit, and within the bar of the reference."""
    params, t = sp.handover_case()
    dense = sp.handover_group_kinds(t)
    assert dense.any() and not dense.all(), dense.tolist()
    d = decoder({"JXLHIP_SPARSE_UPLOAD": "1"}, monkeypatch)
    d2 = decoder({"JXLHIP_SPARSE_UPLOAD": "1"}, monkeypatch)
    try:
        dq = d.default_dequant_tables()
        d.begin_frame(params)
        d.set_inputs(to_dev(t), dq)
        want = d.decode_frame().clone()
        d.sync()
        fr = sp.reference_frame(ref, params, t)
        check_channels("handover", "all flat_i16", want.cpu().numpy(), fr.decode_ref(threads=THREADS), axis=2)

        d2.begin_frame(params)
        h = frames.entropy_decode_submit(d2, t, dq.cpu().numpy(), fr, threads=4)
        got = d2.decode_frame()
        d2.sync()
        d2.L.jxlhip_ac_pass_destroy(h)
        assert torch.equal(got, want), torch.nonzero(got != want)[:5].tolist()
    finally:
        d.close()
        d2.close()
