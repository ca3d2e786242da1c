"""Upsampled frames on the device (jxlhip_set_upsampling, kernels_upsample.hip).

  - genuine streams (the reference encoder resamples by itself from distance 10 on: oracle.feature_stream(f, ...,
    distance >= 10) has FrameHeader::upsampling == 2) through jxlhip_decode_codestream against the reference's public
    JxlDecoder (oracle/_ref/libjxl_dec_ref.so), as float and as 8-bit output: plain frames, with noise, with splines,
    progressive;
  - the kernel alone on synthetic frames: (upsampling on) == tests/upsampling_model.py on the (upsampling off) XYB
    planes, for N = 2, 4, 8, default and custom weights, full and cropped output sizes, every output kind and both
    routings, and with splines in front and noise behind it (tests/spline_model.py, tests/noise_model.py);
  - genuine streams beyond the encoder's own choice (oracle.feature_stream's resampling and custom_weights_seed,
    tests/stream_chain.py; committed under tests/golden/render_stage_streams): N = 4 and 8 with the default tables, N = 2, 4 and 8 with custom ones, cropped and not, of
    several sections and of one, against JxlDecoder; tests/test_render_stage_streams.py holds the model to the same
    streams on the CPU and shows what a misread weight expansion or a missing clamp costs there;
  - the kernel against the model on planted step edges (tests/planted_frames.py), where for every one of the N x N
    output phases both ends of the clamp are asserted to decide;
  - a context reused after an upsampled frame, factor 1, and the refused configurations."""
import ctypes as C

import numpy as np
import pytest

from libjxl_amd import abi, synth

import noise_model
import planted_frames as pf
import spline_model as sm
import stream_chain as sc
import upsampling_model as um
from test_splines_front_end import built_sets

TIGHT = 2e-5
LUT = [0.05, 0.12, 0.3, 0.45, 0.6, 0.75, 0.9, 1.0]
# (feature, size, distance): every one has upsampling == 2, default weights, Gaborish + EPF
STREAMS = [("plain", (600, 400), 12), ("plain", (777, 333), 10), ("plain", (13, 200), 15), ("plain", (2200, 520), 12),
           ("noise", (600, 400), 12), ("noise", (777, 333), 16), ("splines", (600, 400), 12),
           ("progressive", (600, 400), 12)]


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


def _decode_stream(L, cs, xs, ys, workers, sample, channels, ups=2):
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
        assert (info.xsize, info.ysize, info.upsampling) == (xs, ys, ups)
        if sample == abi.SAMPLE_F32:
            fmt = abi.OutputFormat(abi.TF_SRGB, abi.SAMPLE_F32, channels, 32, 0, 0.0, info.luminances)
            out = torch.full((ys, xs, channels), -7.0, dtype=torch.float32, device="cuda")
            stride = xs * 4 * channels
        else:
            fmt = abi.OutputFormat(abi.TF_SRGB, abi.SAMPLE_U8, channels, 8, 0, 0.0, info.luminances)
            out = torch.zeros((ys, xs, channels), dtype=torch.uint8, device="cuda")
            stride = xs * channels
        got = abi.CodestreamInfo()
        rc = L.jxlhip_decode_codestream(dec.ctx, runner, pool, cs, len(cs), 2, C.byref(fmt), out.data_ptr(), stride,
                                        0, C.byref(got))
        assert rc == 0, L.jxlhip_last_error(dec.ctx)
        assert (got.xsize, got.ysize, got.upsampling) == (xs, ys, ups)
        return out.cpu().numpy()
    finally:
        dec.close()
        if pool:
            R.JxlThreadParallelRunnerDestroy(pool)


@pytest.mark.gpu
@pytest.mark.parametrize("workers", [0, 6])
@pytest.mark.parametrize("feature,size,distance", STREAMS)
def test_upsampled_stream_matches_jxldecoder(L, ref, jxl_ref, feature, size, distance, workers):
    ts, RL = jxl_ref
    xs, ys = size
    cs = ref.feature_stream(feature, xsize=xs, ysize=ys, seed=5, distance=distance)
    want = ts.jxl_decode(RL, cs)
    assert want.shape == (ys, xs, 3)
    got = _decode_stream(L, cs, xs, ys, workers, abi.SAMPLE_F32, 3)
    scale = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got - want).max()) / scale
    print("%s %dx%d d%g workers %d: max|diff| / scale = %.3e" % (feature, xs, ys, distance, workers, err))
    assert err <= TIGHT


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("feature,size,distance", [("plain", (600, 400), 12), ("plain", (2200, 520), 12),
                                                   ("noise", (600, 400), 12)])
def test_upsampled_stream_as_8_bit(L, ref, jxl_ref, feature, size, distance, channels):
    ts, RL = jxl_ref
    xs, ys = size
    cs = ref.feature_stream(feature, xsize=xs, ysize=ys, seed=5, distance=distance)
    want = np.round(np.clip(ts.jxl_decode(RL, cs), 0.0, 1.0) * 255.0)
    got = _decode_stream(L, cs, xs, ys, 0, abi.SAMPLE_U8, channels)
    err = float(np.abs(got[..., :3].astype(np.float32) - want).max())
    print("%s %dx%d 8-bit x%d: max level difference %g" % (feature, xs, ys, channels, err))
    assert err <= 1.0
    if channels == 4:
        assert np.all(got[..., 3] == 255)  # no alpha channel: opaque


@pytest.fixture(scope="module")
def knob_streams(jxl_ref):
    """name -> (the committed stream, JxlDecoder's picture) of stream_chain.UPSAMPLING_STREAMS: decoded once, never
    modified.  (tests/test_render_stage_streams.py holds the committed files to what the reference encoder writes.)"""
    ts, RL = jxl_ref
    done = {}

    def get(name):
        if name not in done:
            cs = sc.golden_stream(name)
            want = ts.jxl_decode(RL, cs)
            want.setflags(write=False)
            done[name] = (cs, want)
        return done[name]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("workers", [0, 6])
@pytest.mark.parametrize("name", list(sc.UPSAMPLING_STREAMS))
def test_4x_8x_and_custom_weight_streams_match_jxldecoder(L, knob_streams, name, workers):
    """Reaches, and would fail without: the (ky, kx) indexing, the triangular index and the mirrored quarters of
    UpsampleKernels at h = 2 and 4 (N = 4, 8), and the custom tables of all three factors from the image header to the
    kernel (test_render_stage_streams.py: with the default tables instead these pictures are off by 10 bars and more)."""
    kw = sc.UPSAMPLING_STREAMS[name]
    cs, want = knob_streams(name)
    xs, ys = kw["xsize"], kw["ysize"]
    assert want.shape == (ys, xs, 3)
    got = _decode_stream(L, cs, xs, ys, workers, abi.SAMPLE_F32, 3, ups=kw["resampling"])
    scale = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got - want).max()) / scale
    print("UPS-GPU %s workers %d: max|diff| / scale = %.3e" % (name, workers, err))
    assert err <= TIGHT


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n2_custom", "n4_custom_crop", "n8_custom"])
def test_custom_weight_streams_as_8_bit(L, knob_streams, name):
    kw = sc.UPSAMPLING_STREAMS[name]
    cs, ref_px = knob_streams(name)
    want = np.round(np.clip(ref_px, 0.0, 1.0) * 255.0)
    got = _decode_stream(L, cs, kw["xsize"], kw["ysize"], 0, abi.SAMPLE_U8, 3, ups=kw["resampling"])
    err = float(np.abs(got.astype(np.float32) - want).max())
    print("UPS-GPU8 %s: max level difference %g" % (name, err))
    assert err <= 1.0


# ---- the kernel against the model -----------------------------------------------------------------------------------

def _decode(dec, params, t, dq, ups=None, splines=None, noise=None):
    """ups = (factor, (W, H), weights)"""
    dec.begin_frame(params)
    dec.set_inputs(t, dq)
    if ups is not None:
        dec.set_upsampling(*ups)
    if noise is not None:
        dec.set_noise(*noise)
    if splines is not None:
        dec.set_splines(splines)
    out = dec.decode_frame()
    dec.sync()
    return out.cpu().numpy()


def _custom_weights(n, seed):
    """Random weights around the defaults (a kernel still sums to about one, so the clamp rarely decides)."""
    rng = np.random.default_rng(seed)
    w = um.default_weights(n)
    return (w + rng.standard_normal(w.size).astype(np.float32) * np.float32(0.02)).astype(np.float32)


def _xyb_to_rgb(xyb, params):
    """XybToRgb (dec_xyb-inl.h:38-86) in float64 on float32 XYB planes [3, H, W] -> [H, W, 3]."""
    x, y, b = [xyb[c].astype(np.float64) for c in range(3)]
    bias = np.array(params["opsin_biases"], np.float32)
    cb = np.cbrt(bias.astype(np.float32)).astype(np.float32).astype(np.float64)
    mixed = [(y + x - cb[0]) ** 3 + float(bias[0]), (y - x - cb[1]) ** 3 + float(bias[1]), (b - cb[2]) ** 3 + float(bias[2])]
    m = np.array(params["inverse_opsin_matrix"], np.float32).astype(np.float64).reshape(3, 3)
    return np.stack([m[r, 0] * mixed[0] + m[r, 1] * mixed[1] + m[r, 2] * mixed[2] for r in range(3)], axis=-1)


def _srgb8(lin):
    c = np.clip(lin, 0, 1)
    return np.where(c <= 0.0031308, c * 12.92, 1.055 * np.power(c, 1 / 2.4) - 0.055) * 255.0


KERNEL_CASES = [(cw, ch, n, custom, crop) for (cw, ch) in ((61, 70), (300, 520), (7, 5)) for n in (2, 4, 8)
                for custom in (False, True) for crop in (False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("cw,ch,n,custom,crop", KERNEL_CASES)
def test_upsample_kernel_matches_the_numpy_restatement(cw, ch, n, custom, crop):
    from libjxl_amd import VarDctDecoder
    W, H = (n * cw - (n - 1), n * ch - (n - 1)) if crop else (n * cw, n * ch)
    weights = _custom_weights(n, cw + n) if custom else None
    fmt = dict(transfer=abi.TF_SRGB, sample_type=abi.SAMPLE_U8, num_channels=4, bits_per_sample=8)
    kw = dict(device="cuda", gab=True, epf_iters=1)
    p0, t = synth.synth_frame(cw, ch, output_kind=0, **kw)
    p1, _ = synth.synth_frame(cw, ch, output_kind=1, **kw)
    p2, _ = synth.synth_frame(cw, ch, output_kind=2, out_format=fmt, **kw)
    ups = (n, (W, H), weights)
    dec = VarDctDecoder(0)
    try:
        dq = dec.default_dequant_tables()
        off = _decode(dec, p0, t, dq)
        on = _decode(dec, p0, t, dq, ups=ups)
        lin = _decode(dec, p1, t, dq, ups=ups)
        out8 = _decode(dec, p2, t, dq, ups=ups)
    finally:
        dec.close()
    assert off.shape == (3, ch, cw) and on.shape == (3, H, W) and lin.shape == (H, W, 3) and out8.shape == (H, W, 4)
    want = um.upsample(off, n, weights, (W, H))
    err = float(np.abs(on - want).max())
    print("coded %dx%d N=%d custom=%d crop=%d: planar XYB max|diff| = %.3e" % (cw, ch, n, custom, crop, err))
    assert err <= 1e-5, err
    # linear RGB: the conversion of the device's own upsampled planes (checked above), evaluated in float64.  What is
    # left is the float32 rounding of XybToRgb: a cube and a 3-term dot product with coefficients below 12, a few
    # 2^-24 of the largest term each: 1e-5 of the range holds it with a margin of 5 and more
    rgb = _xyb_to_rgb(on, p1)
    scale = max(1.0, float(np.abs(rgb).max()))
    err = float(np.abs(lin - rgb).max()) / scale
    print("  linear RGB max|diff| / scale = %.3e" % err)
    assert err <= 1e-5, err
    # packed: against the float output, as tests/test_gpu_splines.py does
    assert np.abs(out8[..., :3].astype(np.float32) - _srgb8(lin)).max() <= 1.6
    assert np.all(out8[..., 3] == 255)


@pytest.mark.gpu
@pytest.mark.parametrize("custom", [False, True])
@pytest.mark.parametrize("n", [2, 4, 8])
@pytest.mark.parametrize("cw,ch", [(61, 70), (7, 5)])
def test_both_ends_of_the_clamp_on_planted_step_edges(cw, ch, n, custom):
    """Step edges between two levels (rows, columns and a checkerboard of blocks; inside the one block of 7x5): the
    kernels' negative lobes overshoot on both sides.  Asserted from the model before the comparison: in every one of
    the N x N output phases the lower and the upper end of k_upsample's clamp each change a value (by more than ten
    bars, not by a rounding), and without the clamp the model is 50 bars and more away."""
    from libjxl_amd import VarDctDecoder
    weights = _custom_weights(n, cw + n) if custom else None
    params, t = pf.step_frame(cw, ch, device="cuda")
    dec = VarDctDecoder(0)
    try:
        dq = dec.default_dequant_tables()
        off = _decode(dec, params, t, dq)
        on = _decode(dec, params, t, dq, ups=(n, (n * cw, n * ch), weights))
    finally:
        dec.close()
    assert off.shape == (3, ch, cw) and on.shape == (3, n * ch, n * cw)
    want = um.upsample(off, n, weights)
    free = um.upsample(off, n, weights, clamp=False)
    for oy in range(n):
        for ox in range(n):
            a, b = want[:, oy::n, ox::n], free[:, oy::n, ox::n]
            assert (b < a - 1e-4).any() and (b > a + 1e-4).any(), (oy, ox)
    assert np.abs(free - want).max() >= 50 * 1e-5
    err = float(np.abs(on - want).max())
    print("UPS-PLANTED coded %dx%d N=%d custom=%d: max|diff| = %.3e (the clamp moves %.3e)" % (
        cw, ch, n, custom, err, float(np.abs(free - want).max())))
    assert err <= 1e-5, err


@pytest.mark.gpu
def test_upsample_behind_the_fused_routing():
    """Coded 4096 x 3072 (12 Mpx: the frame's own path is the fused kernel) upsampled 2x; the model on three strips of
    coded rows (top, middle, bottom: the strips in the middle carry two more rows on each side than are compared)."""
    from libjxl_amd import VarDctDecoder
    cw, ch, n = 4096, 3072, 2
    p0, t = synth.synth_frame(cw, ch, device="cuda", output_kind=0, gab=True, epf_iters=1)
    dec = VarDctDecoder(0)
    try:
        dq = dec.default_dequant_tables()
        off = _decode(dec, p0, t, dq)
        dec.profile(True)
        on = _decode(dec, p0, t, dq, ups=(n, (n * cw - 1, n * ch), None))
        slots = dec.profile_read()
    finally:
        dec.close()
    assert "fused" in slots and "upsample" in slots and "filters" not in slots, slots
    assert on.shape == (3, n * ch, n * cw - 1)
    for a, b in ((0, 40), (1500, 1540), (ch - 40, ch)):
        lo, hi = max(a - 2, 0), min(b + 2, ch)
        want = um.upsample(off[:, lo:hi], n)[:, (a - lo) * n:(b - lo) * n, :n * cw - 1]
        err = float(np.abs(on[:, a * n:b * n] - want).max())
        print("coded rows [%d, %d): max|diff| = %.3e" % (a, b, err))
        assert err <= 1e-5, err


@pytest.mark.gpu
@pytest.mark.parametrize("cw,ch,n,crop", [(61, 70, 2, True), (300, 520, 2, False), (61, 70, 4, False), (37, 29, 8, True)])
def test_splines_then_upsampling_then_noise(cw, ch, n, crop):
    """The reference's stage order (dec_cache.cc:194-218): splines at coded size, upsampling, noise at output size."""
    from libjxl_amd import VarDctDecoder
    W, H = (n * cw - (n - 1), n * ch - 1) if crop else (n * cw, n * ch)
    params, t = synth.synth_frame(cw, ch, device="cuda", output_kind=0, gab=True, epf_iters=2)
    params["cfl_base_x"] = 0.0625
    s = built_sets(cw, ch)
    sets = s["edge"] + s["tiny"]
    ups = (n, (W, H), None)
    dec = VarDctDecoder(0)
    try:
        dq = dec.default_dequant_tables()
        off = _decode(dec, params, t, dq)
        both = _decode(dec, params, t, dq, ups=ups, splines=sets, noise=(LUT, 1, 0))
        only_splines = _decode(dec, params, t, dq, ups=ups, splines=sets)
        only_noise = _decode(dec, params, t, dq, ups=ups, noise=(LUT, 1, 0))
    finally:
        dec.close()
    drawn = sm.draw(off, sm.segments(sets, 0, cw, ch, 0.0625, params["cfl_base_b"]))
    assert np.abs(drawn - off).max() > 1e-3  # the splines are there
    up = um.upsample(drawn, n, None, (W, H))
    err = float(np.abs(only_splines - up).max())
    print("splines -> upsample: %.3e" % err)
    assert err <= 1e-5, err
    want = noise_model.add_noise(up, LUT, 0.0625, params["cfl_base_b"], visible=1)
    assert np.abs(want - up).max() > 1e-3  # the noise is there
    err = float(np.abs(both - want).max())
    print("splines -> upsample -> noise: %.3e" % err)
    assert err <= 1e-5, err
    want = noise_model.add_noise(um.upsample(off, n, None, (W, H)), LUT, 0.0625, params["cfl_base_b"], visible=1)
    err = float(np.abs(only_noise - want).max())
    print("upsample -> noise: %.3e" % err)
    assert err <= 1e-5, err


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [1, 2])
def test_noise_behind_upsampling_in_the_interleaved_outputs(kind):
    """k_noise_emit writes the caller's output of an upsampled frame: linear RGB / RGBA8 against the planar result."""
    from libjxl_amd import VarDctDecoder
    cw, ch, n = 300, 200, 2
    fmt = dict(transfer=abi.TF_SRGB, sample_type=abi.SAMPLE_U8, num_channels=4, bits_per_sample=8)
    p0, t = synth.synth_frame(cw, ch, device="cuda", output_kind=0, gab=True, epf_iters=1)
    pk, _ = synth.synth_frame(cw, ch, device="cuda", output_kind=kind, gab=True, epf_iters=1, out_format=fmt if kind == 2 else None)
    ups = (n, (n * cw - 1, n * ch - 1), None)
    dec = VarDctDecoder(0)
    try:
        dq = dec.default_dequant_tables()
        planar = _decode(dec, p0, t, dq, ups=ups, noise=(LUT, 1, 0))
        out = _decode(dec, pk, t, dq, ups=ups, noise=(LUT, 1, 0))
    finally:
        dec.close()
    rgb = _xyb_to_rgb(planar, p0)
    if kind == 1:
        assert float(np.abs(out - rgb).max()) / max(1.0, float(np.abs(rgb).max())) <= 1e-5
    else:
        assert out.shape == (n * ch - 1, n * cw - 1, 4)
        assert np.abs(out[..., :3].astype(np.float32) - _srgb8(rgb)).max() <= 1.6
        assert np.all(out[..., 3] == 255)


@pytest.mark.gpu
def test_host_frame_of_an_upsampled_frame(L):
    """jxlhip_decode_frame_host sizes its rows and columns from the output."""
    from libjxl_amd import VarDctDecoder
    cw, ch, n = 61, 70, 2
    W, H = n * cw - 1, n * ch
    params, t = synth.synth_frame(cw, ch, device="cuda", output_kind=1, gab=True, epf_iters=1)
    dec = VarDctDecoder(0)
    try:
        dq = dec.default_dequant_tables()
        want = _decode(dec, params, t, dq, ups=(n, (W, H), None))
        host = np.full((H, W, 3), -7.0, np.float32)
        assert L.jxlhip_decode_frame_host(dec.ctx, host.ctypes.data, W * 12, 0) == 0, L.jxlhip_last_error(dec.ctx)
        assert L.jxlhip_decode_frame_host(dec.ctx, host.ctypes.data, W * 12 - 4, 0) == -1
    finally:
        dec.close()
    assert np.array_equal(host, want)


# ---- state ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_a_frame_after_an_upsampled_frame_is_untouched():
    from libjxl_amd import VarDctDecoder
    params, t = synth.synth_frame(600, 400, device="cuda", output_kind=1, gab=True, epf_iters=1)
    fresh = VarDctDecoder(0)
    used = VarDctDecoder(0)
    try:
        want = _decode(fresh, params, t, fresh.default_dequant_tables())
        dq = used.default_dequant_tables()
        up = _decode(used, params, t, dq, ups=(4, (2400, 1597), None))
        got = _decode(used, params, t, dq)
        # factor 1 resets within a frame
        used.begin_frame(params)
        used.set_inputs(t, dq)
        used.set_upsampling(2, (1200, 800))
        used.set_upsampling(1, None)
        reset = used.decode_frame()
        used.sync()
        reset = reset.cpu().numpy()
    finally:
        fresh.close()
        used.close()
    assert up.shape == (1597, 2400, 3)
    assert np.array_equal(got, want)
    assert np.array_equal(reset, want)


@pytest.mark.gpu
def test_refused_configurations(L):
    import torch
    from libjxl_amd import VarDctDecoder
    ctx = C.c_void_p()
    devs = (C.c_int * 2)(0, 0)
    assert L.jxlhip_create_multi(devs, 2, None, C.byref(ctx)) == 0
    try:
        assert L.jxlhip_set_upsampling(ctx, 2, None, 600, 1040) == -7
        assert b"multi-device" in L.jxlhip_last_error(ctx)
    finally:
        L.jxlhip_destroy(ctx)
    dec = VarDctDecoder(0)
    try:
        params, t = synth.synth_frame(300, 520, device="cuda", output_kind=1, gab=True, epf_iters=1)
        assert L.jxlhip_set_upsampling(dec.ctx, 2, None, 600, 1040) == -6  # before frame_begin
        dec.begin_frame(dict(params, stripe_group_y0=1, stripe_group_rows=1))
        assert L.jxlhip_set_upsampling(dec.ctx, 2, None, 600, 1040) == -7
        assert b"stripes" in L.jxlhip_last_error(dec.ctx)
        dec.begin_frame(dict(params, undo_orientation=6))
        assert L.jxlhip_set_upsampling(dec.ctx, 2, None, 600, 1040) == -7
        assert b"undo_orientation" in L.jxlhip_last_error(dec.ctx)
        dq = dec.default_dequant_tables()
        dec.begin_frame(params)
        dec.set_inputs(t, dq)
        # the size pair (ceil(out / factor) must be the coded 300 x 520) and the factor
        for factor, w, h in ((2, 601, 1040), (2, 600, 1038), (2, 598, 1040), (4, 1200, 2076), (4, 1201, 2080), (8, 2400, 4152), (8, 2400, 4161), (2, 0, 0)):
            assert L.jxlhip_set_upsampling(dec.ctx, factor, None, w, h) == -1, (factor, w, h)
        for factor in (0, 3, 16):
            assert L.jxlhip_set_upsampling(dec.ctx, factor, None, 300 * factor, 520 * factor) == -1
        assert L.jxlhip_set_upsampling(dec.ctx, 4, None, 1197, 2080) == 0
        # alpha on an upsampled frame, either way round
        alpha = np.ones((520, 300), np.float32)
        assert L.jxlhip_set_alpha(dec.ctx, alpha.ctypes.data, 300) == -7
        assert b"alpha" in L.jxlhip_last_error(dec.ctx)
        dec.begin_frame(params)
        dec.set_inputs(t, dq)
        dec.set_alpha(alpha)
        assert L.jxlhip_set_upsampling(dec.ctx, 2, None, 600, 1040) == -7
        assert b"alpha" in L.jxlhip_last_error(dec.ctx)
        # behind a draw list made for the upsampled size neither the factor nor a reset to 1 is taken
        dec.begin_frame(params)
        dec.set_inputs(t, dq)
        dec.set_upsampling(2, (600, 1040))
        dec.set_splines(built_sets(300, 520)["edge"])
        assert L.jxlhip_set_upsampling(dec.ctx, 1, None, 0, 0) == -6
        assert L.jxlhip_set_upsampling(dec.ctx, 4, None, 1200, 2080) == -6
        assert b"set_splines" in L.jxlhip_last_error(dec.ctx)
        # the split calls
        dec.begin_frame(params)
        dec.set_inputs(t, dq)
        dec.set_upsampling(2, (600, 1040))
        dec.decode_blocks()
        out = torch.empty((1040, 600, 3), dtype=torch.float32, device="cuda")
        assert L.jxlhip_decode_filters(dec.ctx, C.c_void_p(out.data_ptr()), 600 * 12, 0) == -7
        assert b"split calls" in L.jxlhip_last_error(dec.ctx)
        assert L.jxlhip_decode_filters_rows(dec.ctx, C.c_void_p(out.data_ptr()), 600 * 12, 0, 0, 256) == -7
        # an output sized for the coded frame is too small
        assert L.jxlhip_decode_frame(dec.ctx, C.c_void_p(out.data_ptr()), 300 * 12, 0) == -1
        dec.decode_frame(out)  # ... while jxlhip_decode_frame takes the frame at its output size
        dec.sync()
    finally:
        dec.close()
