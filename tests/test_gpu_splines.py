"""Splines on the device (jxlhip_set_splines, kernels_splines.hip).

  - genuine spline streams (the reference encoder's custom splines, oracle.feature_stream("splines")) through
    jxlhip_decode_codestream against the reference's public JxlDecoder (oracle/_ref/libjxl_dec_ref.so), as float and
    as 8-bit output;
  - the kernel alone on synthetic frames: (splines on) == tests/spline_model.py's drawing on the (splines off) XYB
    planes, over every stage list and both routings, and with noise behind it (tests/noise_model.py);
  - packed output with alpha, a context reused after a spline frame, and the refused configurations."""
import ctypes as C

import numpy as np
import pytest

from libjxl_amd import abi, synth

import noise_model
import spline_model as sm
from test_splines_front_end import built_sets, path, spline

TIGHT = 2e-5
LUT = [0.05, 0.12, 0.3, 0.45, 0.6, 0.75, 0.9, 1.0]
# (size, distance): at distance 1.0 the encoder writes no splines above about a megapixel
STREAMS = [((600, 400), 1.0), ((777, 333), 1.0), ((2200, 520), 3.0), ((13, 200), 1.0), ((600, 400), 3.0),
           ((777, 333), 3.0)]


@pytest.fixture(scope="module")
def L():
    return abi.load_library()


@pytest.fixture(scope="module")
def ref(oracle):
    if not oracle.ref_available():
        pytest.skip("oracle/_ref not available")
    oracle.ref_lib()
    return oracle


@pytest.fixture(scope="module")
def jxl_ref():
    import os
    import sys
    import test_seam
    sys.path.insert(0, os.path.join(test_seam.ROOT, "integration"))
    import build_seam
    try:
        ref_so, _ = build_seam.build()
    except RuntimeError as e:
        pytest.skip(str(e))
    return test_seam, test_seam.load(ref_so)


def _decode_stream(L, cs, xs, ys, workers, sample, channels):
    import torch
    from libjxl_amd import VarDctDecoder
    R = C.CDLL(abi.runner_library_path())
    R.JxlThreadParallelRunnerCreate.restype = C.c_void_p
    R.JxlThreadParallelRunnerCreate.argtypes = [C.c_void_p, C.c_size_t]
    R.JxlThreadParallelRunnerDestroy.argtypes = [C.c_void_p]
    pool = R.JxlThreadParallelRunnerCreate(None, workers) if workers else None
    runner = C.cast(R.JxlThreadParallelRunner, C.c_void_p) if workers else None
    dec = VarDctDecoder(0)
    try:
        info = abi.CodestreamInfo()
        assert L.jxlhip_codestream_basic_info(cs, len(cs), C.byref(info)) == 0
        assert info.transfer_function == 13  # sRGB
        if sample == abi.SAMPLE_F32:
            fmt = abi.OutputFormat(abi.TF_SRGB, abi.SAMPLE_F32, channels, 32, 0, 0.0, info.luminances)
            out = torch.full((ys, xs, channels), -7.0, dtype=torch.float32, device="cuda")
            stride = xs * 4 * channels
        else:
            fmt = abi.OutputFormat(abi.TF_SRGB, abi.SAMPLE_U8, channels, 8, 0, 0.0, info.luminances)
            out = torch.zeros((ys, xs, channels), dtype=torch.uint8, device="cuda")
            stride = xs * channels
        rc = L.jxlhip_decode_codestream(dec.ctx, runner, pool, cs, len(cs), 2, C.byref(fmt), out.data_ptr(), stride,
                                        0, None)
        assert rc == 0, L.jxlhip_last_error(dec.ctx)
        return out.cpu().numpy()
    finally:
        dec.close()
        if pool:
            R.JxlThreadParallelRunnerDestroy(pool)


@pytest.mark.gpu
@pytest.mark.parametrize("workers", [0, 6])
@pytest.mark.parametrize("size,distance", STREAMS)
def test_spline_stream_matches_jxldecoder(L, ref, jxl_ref, size, distance, workers):
    ts, RL = jxl_ref
    xs, ys = size
    cs = ref.feature_stream("splines", xsize=xs, ysize=ys, seed=5, distance=distance)
    want = ts.jxl_decode(RL, cs)  # (JxlDecoder takes the stream, the narrow one included)
    assert want.shape == (ys, xs, 3)
    got = _decode_stream(L, cs, xs, ys, workers, abi.SAMPLE_F32, 3)
    scale = max(1.0, float(np.abs(want).max()))
    assert float(np.abs(got - want).max()) / scale <= TIGHT


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("size,distance", [((600, 400), 1.0), ((2200, 520), 3.0), ((13, 200), 1.0)])
def test_spline_stream_as_8_bit(L, ref, jxl_ref, size, distance, channels):
    ts, RL = jxl_ref
    xs, ys = size
    cs = ref.feature_stream("splines", xsize=xs, ysize=ys, seed=5, distance=distance)
    want = np.round(np.clip(ts.jxl_decode(RL, cs), 0.0, 1.0) * 255.0)
    got = _decode_stream(L, cs, xs, ys, 0, abi.SAMPLE_U8, channels)
    assert np.abs(got[..., :3].astype(np.float32) - want).max() <= 1.0
    if channels == 4:
        assert np.all(got[..., 3] == 255)  # no alpha channel: opaque


def _decode(dec, params, t, dq, splines=None, noise=None, alpha=None):
    dec.begin_frame(params)
    dec.set_inputs(t, dq)
    if alpha is not None:
        dec.set_alpha(alpha)
    if noise is not None:
        dec.set_noise(*noise)
    if splines is not None:
        dec.set_splines(splines)
    out = dec.decode_frame()
    dec.sync()
    return out.cpu().numpy()


def _sets(xs, ys, names):
    s = built_sets(xs, ys)
    return [sp for n in names for sp in s[n]]


# (xsize, ysize, gab, epf_iters, sets): every stage list; 4096x3072 = 12 Mpx takes the fused routing
KERNEL_CASES = [(61, 70, g, e, ("edge", "tiny", "large")) for g in (0, 1) for e in (0, 1, 2, 3)] + \
               [(300, 520, g, e, ("edge", "tiny")) for g in (0, 1) for e in (0, 1, 2, 3)] + \
               [(300, 520, 1, 1, ("large",)), (4096, 3072, 1, 1, ("edge", "tiny"))]


@pytest.mark.gpu
@pytest.mark.parametrize("xs,ys,gab,epf,names", KERNEL_CASES)
def test_spline_kernel_matches_the_numpy_restatement(xs, ys, gab, epf, names):
    from libjxl_amd import VarDctDecoder
    params, t = synth.synth_frame(xs, ys, device="cuda", output_kind=0, gab=bool(gab), epf_iters=epf)
    params["cfl_base_x"] = 0.0625  # a non-zero YtoX ratio
    sets = _sets(xs, ys, names)
    dec = VarDctDecoder(0)
    try:
        dq = dec.default_dequant_tables()
        off = _decode(dec, params, t, dq)
        on = _decode(dec, params, t, dq, splines=sets)
    finally:
        dec.close()
    segs = sm.segments(sets, 0, xs, ys, 0.0625, params["cfl_base_b"])
    want = sm.draw(off, segs)
    assert np.abs(want - off).max() > 1e-3  # the splines are there
    err = float(np.abs(on - want).max())
    assert err <= 1e-5, err


@pytest.mark.gpu
@pytest.mark.parametrize("xs,ys,gab,epf", [(61, 70, 1, 2), (300, 520, 0, 1), (4096, 3072, 1, 1)])
def test_splines_then_noise(xs, ys, gab, epf):
    from libjxl_amd import VarDctDecoder
    params, t = synth.synth_frame(xs, ys, device="cuda", output_kind=0, gab=bool(gab), epf_iters=epf)
    params["cfl_base_x"] = 0.0625
    sets = _sets(xs, ys, ("edge", "tiny"))
    dec = VarDctDecoder(0)
    try:
        dq = dec.default_dequant_tables()
        off = _decode(dec, params, t, dq)
        on = _decode(dec, params, t, dq, splines=sets, noise=(LUT, 1, 0))
    finally:
        dec.close()
    drawn = sm.draw(off, sm.segments(sets, 0, xs, ys, 0.0625, params["cfl_base_b"]))
    want = noise_model.add_noise(drawn, LUT, 0.0625, params["cfl_base_b"], visible=1)
    err = float(np.abs(on - want).max())
    assert err <= 1e-5, err


@pytest.mark.gpu
def test_packed_rgba8_with_alpha_agrees_with_the_float_output():
    from libjxl_amd import VarDctDecoder
    xs, ys = 300, 200
    fmt = dict(transfer=abi.TF_SRGB, sample_type=abi.SAMPLE_U8, num_channels=4, bits_per_sample=8)
    p_lin, t = synth.synth_frame(xs, ys, device="cuda", output_kind=1, gab=True, epf_iters=1)
    p_8, _ = synth.synth_frame(xs, ys, device="cuda", output_kind=2, gab=True, epf_iters=1, out_format=fmt)
    alpha = np.random.default_rng(3).random((ys, xs), dtype=np.float32)
    sets = _sets(xs, ys, ("edge", "tiny"))
    dec = VarDctDecoder(0)
    try:
        dq = dec.default_dequant_tables()
        lin = _decode(dec, p_lin, t, dq, splines=sets)
        lin_plain = _decode(dec, p_lin, t, dq)
        out8 = _decode(dec, p_8, t, dq, splines=sets, alpha=alpha)
        out8_plain = _decode(dec, p_8, t, dq, alpha=alpha)
    finally:
        dec.close()
    assert np.abs(lin - lin_plain).max() > 1e-3
    c = np.clip(lin, 0, 1)
    srgb = np.where(c <= 0.0031308, c * 12.92, 1.055 * np.power(c, 1 / 2.4) - 0.055) * 255.0
    assert np.abs(out8[..., :3].astype(np.float32) - srgb).max() <= 1.6
    assert np.array_equal(out8[..., 3], out8_plain[..., 3])  # alpha untouched by the splines


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1])
def test_splines_outside_the_frame_take_the_plain_path(kind):
    """A draw list whose segments all miss the frame's columns (and a spline of one control point) leaves the frame
    bit-identical to no splines."""
    from libjxl_amd import VarDctDecoder
    params, t = synth.synth_frame(300, 520, device="cuda", output_kind=kind, gab=True, epf_iters=2)
    far = [spline(*path([(5000, 10), (5200, 400)])), spline((150, 200), [])]
    dec = VarDctDecoder(0)
    try:
        dq = dec.default_dequant_tables()
        plain = _decode(dec, params, t, dq)
        missed = _decode(dec, params, t, dq, splines=far)
    finally:
        dec.close()
    assert np.array_equal(plain, missed)


@pytest.mark.gpu
def test_a_frame_after_a_spline_frame_is_untouched():
    from libjxl_amd import VarDctDecoder
    params, t = synth.synth_frame(600, 400, device="cuda", output_kind=1, gab=True, epf_iters=1)
    fresh = VarDctDecoder(0)
    used = VarDctDecoder(0)
    try:
        want = _decode(fresh, params, t, fresh.default_dequant_tables())
        dq = used.default_dequant_tables()
        drawn = _decode(used, params, t, dq, splines=_sets(600, 400, ("edge", "tiny")))
        got = _decode(used, params, t, dq)
    finally:
        fresh.close()
        used.close()
    assert np.abs(drawn - want).max() > 1e-3
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_refused_configurations(L):
    import torch
    from libjxl_amd import VarDctDecoder
    rc, h = abi.splines_from_quantized(_sets(300, 520, ("edge",)))
    assert rc == 0
    try:
        ctx = C.c_void_p()
        devs = (C.c_int * 2)(0, 0)
        assert L.jxlhip_create_multi(devs, 2, None, C.byref(ctx)) == 0
        try:
            assert L.jxlhip_set_splines(ctx, h) == -7
            assert b"multi-device" in L.jxlhip_last_error(ctx)
        finally:
            L.jxlhip_destroy(ctx)
        dec = VarDctDecoder(0)
        try:
            params, t = synth.synth_frame(300, 520, device="cuda", output_kind=1, gab=True, epf_iters=1)
            dec.begin_frame(dict(params, stripe_group_y0=1, stripe_group_rows=1))
            assert L.jxlhip_set_splines(dec.ctx, h) == -7
            assert b"stripes" in L.jxlhip_last_error(dec.ctx)
            dec.begin_frame(dict(params, undo_orientation=6))
            assert L.jxlhip_set_splines(dec.ctx, h) == -7
            assert b"undo_orientation" in L.jxlhip_last_error(dec.ctx)
            dq = dec.default_dequant_tables()
            dec.begin_frame(params)
            dec.set_inputs(t, dq)
            dec.set_splines(h)
            dec.decode_blocks()
            out = torch.empty((520, 300, 3), dtype=torch.float32, device="cuda")
            assert L.jxlhip_decode_filters(dec.ctx, C.c_void_p(out.data_ptr()), 300 * 12, 0) == -7
            assert b"split calls" in L.jxlhip_last_error(dec.ctx)
            assert L.jxlhip_decode_filters_rows(dec.ctx, C.c_void_p(out.data_ptr()), 300 * 12, 0, 0, 256) == -7
            dec.decode_frame(out)  # ... while jxlhip_decode_frame takes the same frame
            dec.sync()
        finally:
            dec.close()
    finally:
        abi.splines_destroy(h)
