"""Every kernel path at the off-default frame parameters and side info of frames.PARAM_SETS, against the libjxl
reference decoder with its own dequant tables (as run_case of test_gpu_vs_reference.py).

The bar is per channel: max|got_c - want_c| <= 2e-5 * max(max|want_c|, 1e-3).  The bar of the other modules divides
by max(1, max|want|) over all channels, which holds a channel of small magnitude (X: ~0.02) to ~1e-3 of its own
range.  test_frame_params_parity.py shows that every knob of every set moves some channel by >= 50x this bar, and
that the oracle equals the reference bit for bit at every set.  Each test prints the worst per-channel error it saw
("WORST <path> <set> <c0> <c1> <c2>", relative to the channel's magnitude)."""
import os

import numpy as np
import pytest
import torch

import frames
from frames import check_channels, per_channel_err  # noqa: F401  (shared with test_gpu_spectrum.py)

pytestmark = pytest.mark.gpu

TIGHT = frames.TIGHT
THREADS = min(16, os.cpu_count() or 1)
SIZE = (520, 300)
SETS = sorted(frames.PARAM_SETS)
DEQUANT_SETS = ["quant_hi", "quant_lo", "cfl", "qfield_1", "coeff_i16", "coeff_i32"]  # knobs that reach the planes


@pytest.fixture(scope="module")
def ref(oracle):
    if not oracle.ref_available():
        pytest.fail("oracle/_ref/libjxl_ref.so missing: run __graft_entry__.build() in the build container")
    oracle.ref_lib()
    return oracle


def to_dev(t):
    return {k: ([x.cuda() for x in v] if isinstance(v, list) else v.cuda()) for k, v in t.items()}


def reference(ref, params, t):
    return frames.oracle_frame(params, t, ref.ref_default_dequant_tables()).decode_ref(threads=THREADS)


def decode(params, t, env, monkeypatch):
    """One decoder created under the environment switches `env`; returns (output as numpy, profile slots)."""
    from libjxl_amd import VarDctDecoder
    for k in ("JXLHIP_FUSE", "JXLHIP_FILTERS", "JXLHIP_MFMA", "JXLHIP_FUSED_PC_RH"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    d = VarDctDecoder(0)
    try:
        d.begin_frame(params)
        d.set_inputs(to_dev(t), d.default_dequant_tables())
        d.profile(True)
        o = d.decode_frame().cpu().numpy()
        d.sync()
        return o, d.profile_read()
    finally:
        d.close()


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("path", ["two_phase", "generic"])
def test_row_march_and_generic_kernel(ref, name, path, monkeypatch):
    """JXLHIP_FUSE=0: k_prepare + the block kernels + the two-phase row march (k_epf0 first at three EPF
    iterations); JXLHIP_FILTERS=generic: the generic LDS filter kernel instead of the march."""
    params, t, _ = frames.make_param_case(*SIZE, name)
    env = {"JXLHIP_FUSE": "0"} if path == "two_phase" else {"JXLHIP_FILTERS": "generic"}
    got, slots = decode(params, t, env, monkeypatch)
    check_channels(path, name, got, reference(ref, params, t), axis=2)
    assert "fused" not in slots, slots
    if frames.PARAM_SETS[name]["epf"] or frames.PARAM_SETS[name]["gab"]:
        assert "filters" in slots or "epf0" in slots, slots


@pytest.mark.parametrize("name", SETS)
def test_fused_kernels(ref, name, monkeypatch):
    """JXLHIP_FUSE=1: k_fused_pc at 0-2 EPF iterations, k_fused_pc0 + the EPF1/EPF2 march at three.  Row-chunking
    (JXLHIP_FUSED_PC_RH) changes no sample, and at three iterations the fused path equals the two-phase path (k_epf0)
    bit for bit, as test_gpu_parity.py holds them at the defaults."""
    params, t, _ = frames.make_param_case(*SIZE, name)
    epf = frames.PARAM_SETS[name]["epf"]
    got, slots = decode(params, t, {"JXLHIP_FUSE": "1", "JXLHIP_FUSED_PC_RH": "0"}, monkeypatch)
    check_channels("fused_pc0" if epf == 3 else "fused_pc", name, got, reference(ref, params, t), axis=2)
    if epf == 3:
        assert "epf0" in slots, slots
        two, _ = decode(params, t, {"JXLHIP_FUSE": "0"}, monkeypatch)
        assert np.array_equal(got, two), np.argwhere(got != two)[:5]
    else:
        assert "fused" in slots and "filters" not in slots, slots
    chunked, _ = decode(params, t, {"JXLHIP_FUSE": "1", "JXLHIP_FUSED_PC_RH": "24"}, monkeypatch)
    assert np.array_equal(got, chunked), np.argwhere(got != chunked)[:5]


@pytest.mark.parametrize("name", DEQUANT_SETS)
def test_mfma_planes(ref, name, monkeypatch):
    """JXLHIP_MFMA=1: DCT16X16 / DCT32X32 varblocks through the matrix-core kernels; the phase-1 XYB planes
    (export_xyb) against the reference's planes (no filters, XYB output)."""
    from libjxl_amd import VarDctDecoder
    xs, ys = 1000, 520
    params, t, _ = frames.make_param_case(xs, ys, name, gab=False, epf_iters=0, output_kind=0)
    acs = t["ac_strategy"].numpy()
    assert {4, 5} <= set((acs[(acs & 1) == 1] >> 1).tolist())
    want = reference(ref, params, t)
    planes = {}
    for mfma in ("1", "0"):
        monkeypatch.setenv("JXLHIP_MFMA", mfma)
        d = VarDctDecoder(0)
        try:
            d.begin_frame(params)
            d.set_inputs(to_dev(t), d.default_dequant_tables())
            d.decode_blocks()
            d.sync()
            planes[mfma] = np.stack([p[:ys, :xs] for p in d.export_xyb()])
        finally:
            d.close()
    check_channels("mfma", name, planes["1"], want, axis=0)
    check_channels("blocks", name, planes["0"], want, axis=0)
    assert not np.array_equal(planes["1"], planes["0"])  # the matrix cores really ran: they round differently


PACKED = {
    "srgb_rgba8": dict(transfer=1, sample_type=1, num_channels=4, bits_per_sample=8),      # fixed-format march
    "srgb_rgb16": dict(transfer=1, sample_type=2, num_channels=3, bits_per_sample=16),     # fixed-format march
    "pq_rgb16": dict(transfer=2, sample_type=2, num_channels=3, bits_per_sample=16, tf_param=1000.0),  # general
    "linear_f32": dict(transfer=0, sample_type=0, num_channels=3),                         # general
}


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("fmt", sorted(PACKED))
def test_packed_output(ref, name, fmt, monkeypatch):
    """FromLinearStage + WriteToOutputStage fused into the march: the fixed-format instantiations and the general
    per-sample path, at the LSB bars of test_gpu_vs_reference.py (float output: the per-channel bar)."""
    from libjxl_amd import VarDctDecoder
    of = PACKED[fmt]
    it = 1000.0 if of["transfer"] == 2 else (80.0 if of["transfer"] else 255.0)
    params, t, _ = frames.make_param_case(*SIZE, name, output_kind=2, out_format=of, intensity_target=it)
    for k in ("JXLHIP_FUSE", "JXLHIP_FILTERS", "JXLHIP_MFMA"):
        monkeypatch.delenv(k, raising=False)
    d = VarDctDecoder(0)
    try:
        d.begin_frame(params)
        d.set_inputs(to_dev(t), d.default_dequant_tables())
        got = d.decode_frame().cpu().numpy()
        d.sync()
    finally:
        d.close()
    want = reference(ref, params, t)
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize
    if of["sample_type"] == 0:
        check_channels("packed_" + fmt, name, got, want, axis=2)
        return
    if of["sample_type"] == 2:  # (the decoder hands 16-bit samples back in an int16 tensor)
        got, want = got.view(np.uint16), want.view(np.uint16)
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    if "coeffs" in frames.PARAM_SETS[name]["knobs"]:
        # Next to a block with a +-32767 / 2^24 coefficient the float pipeline works on values ~1e8 times the usual
        # ones: an in-range sample there can be the difference of such values, and its error is 2e-5 of THEIR
        # magnitude (the per-channel bar of the float outputs), far more than an LSB.  The LSB bar holds elsewhere.
        near = near_huge(reference(ref, dict(params, output_kind=1), t), 16.0, 8)  # (H, W): d[near] is (n, channels)
        print("WORST packed_%s %s next to the extreme blocks (%.1f%% of the samples): max %d" %
              (fmt, name, 100 * near.mean(), d[near].max()))
        d = d[~near]
    print("WORST packed_%s %s max %d frac %.2e" % (fmt, name, d.max(), (d != 0).mean()))
    if fmt == "srgb_rgba8":
        assert d.max() <= 1 and (d != 0).mean() < 1e-3, (d.max(), (d != 0).mean())
        assert (got[..., 3] == 255).all()
    elif fmt == "srgb_rgb16":
        assert d.max() <= max(2, int(TIGHT * 8 * 65536))
    else:  # PQ's slope near zero (~1e3 at 1e-4) amplifies the float pipeline's 2e-5
        assert d.max() <= 140 and (d > 8).mean() < 2e-3, (d.max(), (d > 8).mean())


def near_huge(linear_rgb, limit, radius):
    """Pixels within `radius` of one whose linear RGB exceeds `limit` in magnitude (the loop filters' reach)."""
    m = np.abs(linear_rgb).max(axis=2) > limit
    for axis in (0, 1):
        acc = m.copy()
        for r in range(1, radius + 1):
            acc |= np.roll(m, r, axis=axis) | np.roll(m, -r, axis=axis)
        m = acc
    return m


STRIPE_SETS = ["quant_hi", "cfl", "opsin", "lf_g2", "lf_g3", "qfield_1"]


@pytest.mark.parametrize("fuse", ["1", "0"])
@pytest.mark.parametrize("name", STRIPE_SETS)
def test_stripe_step_in_three_calls_equals_whole_frame(ref, name, fuse, monkeypatch):
    """jxlhip_stripe_begin / jxlhip_decode_filters_rows / jxlhip_stripe_finish on three stripes of one device (as
    test_gpu_parity.py runs them; at three EPF iterations without the early interior call, which that path does not
    offer): bit-equal to the whole frame, which is within the bar of the reference."""
    from libjxl_amd import VarDctDecoder
    monkeypatch.setenv("JXLHIP_FUSE", fuse)
    xs, ys = 600, 1100
    params, t, _ = frames.make_param_case(xs, ys, name, mix=None)
    devt = to_dev(t)
    d0 = VarDctDecoder(0)
    d0.begin_frame(params)
    dq = d0.default_dequant_tables()
    d0.set_inputs(devt, dq)
    whole = d0.decode_frame().clone()
    d0.sync()
    d0.close()
    check_channels("stripes_fuse" + fuse, name, whole.cpu().numpy(), reference(ref, params, t), axis=2)
    parts = [(0, 2), (2, 1), (3, 2)]
    decs, bufs, outs = [], [], []
    try:
        for (g0, gr) in parts:
            d = VarDctDecoder(0)
            decs.append(d)
            d.begin_frame(dict(params, stripe_group_y0=g0, stripe_group_rows=gr))
            d.set_inputs(devt, dq)
            h = d.halo_rows()
            mk = lambda: torch.full((3, h, xs), float("nan"), dtype=torch.float32, device="cuda")  # noqa: E731
            up, dn = g0 > 0, g0 + gr < 5
            b = dict(up=mk() if up and h else None, dn=mk() if dn and h else None)
            d.stripe_begin(b["up"], b["dn"])
            out = d.alloc_output()
            y0, y1 = d.stripe_rows()
            rows = (y0 + 8 if up else y0, y1 - 8 if dn else y1)
            interior = frames.PARAM_SETS[name]["epf"] < 3
            if interior:
                d.decode_filters(out, rows=rows)
            bufs.append(b), outs.append((out, rows if interior else None))
        torch.cuda.synchronize()
        for i, d in enumerate(decs):
            d.stripe_finish(outs[i][0], bufs[i - 1]["dn"] if i > 0 else None,
                            bufs[i + 1]["up"] if i + 1 < len(decs) else None, outs[i][1])
            d.sync()
        got = torch.cat([o for o, _ in outs], dim=0)
        assert torch.equal(got, whole)
    finally:
        for d in decs:
            d.close()


@pytest.mark.parametrize("smooth", [0, 1])
@pytest.mark.parametrize("name", ["quant_hi", "quant_lo"])
def test_dequant_dc(ref, name, smooth):
    """jxlhip_dequant_dc takes its step from the frame's global_scale and quant_dc (quantizer.h:133-139): against the
    reference's DequantDC (+ AdaptiveDCSmoothing), bit for bit."""
    import ctypes as C
    from libjxl_amd import VarDctDecoder
    xs, ys = 333, 270
    params, _, _ = frames.make_param_case(xs, ys, name)
    xsb, ysb = (xs + 7) // 8, (ys + 7) // 8
    rng = np.random.default_rng(4 + smooth)
    yy, xx = np.mgrid[0:ysb, 0:xsb]
    q = [(200 * np.sin(xx * 0.05 + c) * np.cos(yy * 0.04) + rng.integers(-3, 4, (ysb, xsb))).astype(np.int32)
         for c in range(3)]
    inv_gs = np.float32(65536.0 / params["global_scale"])
    mul = np.array([np.float32(inv_gs / np.float32(params["quant_dc"])) * np.float32(v)
                    for v in (1 / 4096.0, 1 / 512.0, 1 / 256.0)], np.float32)
    want = ref.ref_dequant_dc(q, mul, 0.1, 0.9, smooth)
    d = VarDctDecoder(0)
    try:
        d.begin_frame(params)
        qd = [torch.from_numpy(a).cuda() for a in q]
        od = [torch.empty((ysb, xsb), dtype=torch.float32, device="cuda") for _ in range(3)]
        rc = d.L.jxlhip_dequant_dc(d.ctx, (C.c_void_p * 3)(*[a.data_ptr() for a in qd]),
                                   (C.c_void_p * 3)(*[a.data_ptr() for a in od]), None, 0.1, 0.9, smooth)
        assert rc == 0
        d.sync()
        for c in range(3):
            assert np.array_equal(od[c].cpu().numpy(), want[c]), c
    finally:
        d.close()


def test_automatic_fused_rule_at_12_mpx(ref, monkeypatch):
    """No switches: a 4096x3072 frame (12.6 Mpx) with DCT8 blocks and float RGB output takes the fused kernel by the
    context's own rule.  The quantisation, CfL, opsin and loop-filter sets at once."""
    names = ("quant_hi", "cfl", "opsin", "lf_g1")
    params, t, _ = frames.make_param_case(4096, 3072, names, mix=None)
    got, slots = decode(params, t, {}, monkeypatch)
    assert "fused" in slots and "filters" not in slots, slots
    check_channels("auto_fused", "+".join(names), got, reference(ref, params, t), axis=2)
