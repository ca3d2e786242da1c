"""Photon noise on the device (jxlhip_set_noise, kernels_noise.hip).

  - genuine noise streams (the reference encoder's kNoise frames, oracle.feature_stream("noise")) through
    jxlhip_decode_codestream against the reference's public JxlDecoder (oracle/_ref/libjxl_dec_ref.so);
  - the kernels alone on synthetic frames: (noise on) == numpy restatement of RNG + ConvolveNoise + AddNoise applied
    to the (noise off) XYB planes (tests/noise_model.py), over every stage list and both routings (two-phase, fused);
  - packed output with alpha, the silent LUT, a context reused after a noise frame, and the refused configurations;
  - genuine streams with a CHOSEN LUT (not monotone, one entry zero), plain and behind 4x upsampling, and of an original
    bright enough to fill the LUT's upper intervals and the branch at 7 and beyond (tests/stream_chain.py; their CPU
    twins, with the populations and the fault injection, are tests/test_render_stage_streams.py);
  - the kernel against the model on planted frames (tests/planted_frames.py) whose (y - x) / 2 and (y + x) / 2 sit below
    zero, on both sides of every knot, inside every interval and above 7 / 6, under a LUT with entries outside [0, 1]:
    every branch of NoiseStrength, both ends of its clamp included, with the counts asserted on the device's planes."""
import ctypes as C

import numpy as np
import pytest

from libjxl_amd import abi, synth

import noise_model
import planted_frames as pf
import stream_chain as sc

TIGHT = 2e-5
LUT = [0.05, 0.12, 0.3, 0.45, 0.6, 0.75, 0.9, 1.0]


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


@pytest.mark.gpu
@pytest.mark.parametrize("workers", [0, 6])
@pytest.mark.parametrize("size,distance", [((600, 400), 1.0), ((777, 333), 1.0), ((2200, 520), 1.0), ((13, 200), 1.0),
                                           ((600, 400), 3.0), ((777, 333), 3.0)])
def test_noise_stream_matches_jxldecoder(L, ref, jxl_ref, size, distance, workers):
    import torch
    from libjxl_amd import VarDctDecoder
    ts, RL = jxl_ref
    xs, ys = size
    cs = ref.feature_stream("noise", xsize=xs, ysize=ys, seed=5, distance=distance)
    want = ts.jxl_decode(RL, cs)
    assert want.shape == (ys, xs, 3)
    R = C.CDLL(abi.runner_library_path())
    R.JxlThreadParallelRunnerCreate.restype = C.c_void_p
    R.JxlThreadParallelRunnerCreate.argtypes = [C.c_void_p, C.c_size_t]
    R.JxlThreadParallelRunnerDestroy.argtypes = [C.c_void_p]
    pool = R.JxlThreadParallelRunnerCreate(None, workers) if workers else None
    runner = C.cast(R.JxlThreadParallelRunner, C.c_void_p) if workers else None
    dec = VarDctDecoder(0)
    try:
        # JxlDecoder's float output is in the original's colour space (sRGB): the packed path with that transfer
        info = abi.CodestreamInfo()
        assert L.jxlhip_codestream_basic_info(cs, len(cs), C.byref(info)) == 0
        assert info.transfer_function == 13  # sRGB
        fmt = abi.OutputFormat(abi.TF_SRGB, abi.SAMPLE_F32, 3, 32, 0, 0.0, info.luminances)
        out = torch.full((ys, xs, 3), -7.0, dtype=torch.float32, device="cuda")
        rc = L.jxlhip_decode_codestream(dec.ctx, runner, pool, cs, len(cs), 2, C.byref(fmt), out.data_ptr(), xs * 12, 0,
                                        None)
        assert rc == 0, L.jxlhip_last_error(dec.ctx)
        got = out.cpu().numpy()
        scale = max(1.0, float(np.abs(want).max()))
        assert float(np.abs(got - want).max()) / scale <= TIGHT
    finally:
        dec.close()
        if pool:
            R.JxlThreadParallelRunnerDestroy(pool)


@pytest.fixture(scope="module")
def chosen(jxl_ref):
    """name -> (the committed stream, JxlDecoder's picture) of stream_chain.NOISE_STREAMS: decoded once, never
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
@pytest.mark.parametrize("name", list(sc.NOISE_STREAMS))
def test_chosen_lut_stream_matches_jxldecoder(L, chosen, name, workers):
    """The LUT of stream_chain.NOISE_LUT: in gamut (intervals 0..2) at 2e-5, plain and at output size
    behind 4x upsampling; the original times 30 (intervals 3..6 and the branch at 7 and beyond), plain and behind 2x, at
    stream_chain.BRIGHT_BAR -- a bar from the CPU tier, not from this kernel.  Measured on an MI355X: noise 1.84e-5,
    noise_n4 1.69e-5, bright 5.5e-5, bright_n2 7.2e-5 (0 and 6 workers alike).  The device's planes are within 1.5 ulp of
    the model's; dark, saturated samples, which strong noise makes, carry such an ulp to 1e-5 of the range through the
    colour conversion (DESIGN.md section 6 says how the LUT's amplitude was chosen with that in view)."""
    from test_gpu_upsampling import _decode_stream
    kw = sc.NOISE_STREAMS[name]
    cs, want = chosen(name)
    xs, ys = kw["xsize"], kw["ysize"]
    assert want.shape == (ys, xs, 3)
    got = _decode_stream(L, cs, xs, ys, workers, abi.SAMPLE_F32, 3, ups=kw.get("resampling", 1))
    bar = sc.BRIGHT_BAR if name.startswith("bright") else TIGHT
    scale = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got - want).max()) / scale
    print("NOISE-GPU %s workers %d: max|diff| / scale = %.3e (scale %.3f, bar %.1e)" % (name, workers, err, scale, bar))
    assert err <= bar


def _decode(dec, params, t, dq, noise=None, alpha=None):
    dec.begin_frame(params)
    dec.set_inputs(t, dq)
    if alpha is not None:
        dec.set_alpha(alpha)
    if noise is not None:
        dec.set_noise(*noise)
    out = dec.decode_frame()
    dec.sync()
    return out.cpu().numpy()


# (xsize, ysize, gab, epf_iters, visible_frame_index): every stage list; 4096x3072 = 12 Mpx takes the fused routing
KERNEL_CASES = [(61, 70, g, e, 1 + (g + e) % 2) for g in (0, 1) for e in (0, 1, 2, 3)] + \
               [(300, 520, g, e, 2 - (g + e) % 2) for g in (0, 1) for e in (0, 1, 2, 3)] + \
               [(4096, 3072, 1, 1, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("xs,ys,gab,epf,vis", KERNEL_CASES)
def test_noise_kernel_matches_the_numpy_restatement(xs, ys, gab, epf, vis):
    from libjxl_amd import VarDctDecoder
    params, t = synth.synth_frame(xs, ys, device="cuda", output_kind=0, gab=bool(gab), epf_iters=epf)
    params["cfl_base_x"] = 0.0625  # a non-zero YtoX ratio: AddNoise's X term
    dec = VarDctDecoder(0)
    try:
        dq = dec.default_dequant_tables()
        off = _decode(dec, params, t, dq)
        on = _decode(dec, params, t, dq, noise=(LUT, vis, 0))
    finally:
        dec.close()
    want = noise_model.add_noise(off, LUT, 0.0625, params["cfl_base_b"], visible=vis)
    assert np.abs(on - off).max() > 1e-3  # the noise is there
    err = float(np.abs(on - want).max())
    assert err <= 1e-5, err


# (xsize, ysize, visible, nonvisible frame index): one group; the group seams; both indices in the seed
PLANTED_CASES = [(128, 64, 1, 0), (300, 520, 2, 0), (61, 70, 3, 2), (61, 70, 1, 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("xs,ys,vis,nonvis", PLANTED_CASES)
def test_every_branch_of_noise_strength_on_planted_frames(xs, ys, vis, nonvis):
    """Reaches, and would fail without: max(0, .) (arguments below zero), each of the six selects and both LUT entries
    of every interval (values on both sides of every knot and inside every interval), scaled >= 7 (values on both sides
    of 7 / 6 and far above), and both ends of the clamp to [0, 1] (LUT entries -0.2, -0.1, 1.2, 1.3)."""
    from libjxl_amd import VarDctDecoder
    params, t = pf.noise_frame(xs, ys, device="cuda")
    params["cfl_base_x"] = 0.0625
    lut = pf.NOISE_CLAMP_LUT
    dec = VarDctDecoder(0)
    try:
        dq = dec.default_dequant_tables()
        off = _decode(dec, params, t, dq)
        on = _decode(dec, params, t, dq, noise=(lut, vis, nonvis))
    finally:
        dec.close()
    # the population, on the device's own noise-free planes: a block is 64 pixels
    for what, counts in pf.noise_population(off).items():
        assert min(counts) >= 64, (what, counts)
    # ... and from the model: each end of the clamp decides
    for v in ((off[1] - off[0]) * np.float32(0.5), (off[1] + off[0]) * np.float32(0.5)):
        raw = noise_model.strength(lut, v, clamp=False)
        assert int((raw < 0).sum()) >= 64 and int((raw > 1).sum()) >= 64
        assert np.abs(noise_model.strength(lut, v) - raw).max() > 0.1
    want = noise_model.add_noise(off, lut, 0.0625, params["cfl_base_b"], visible=vis, nonvisible=nonvis)
    assert np.abs(on - off).max() > 1e-3  # the noise is there
    if nonvis:  # ... and the second index is in the seed
        assert np.abs(want - noise_model.add_noise(off, lut, 0.0625, params["cfl_base_b"], visible=vis)).max() > 1e-3
    err = float(np.abs(on - want).max())
    print("NOISE-PLANTED %dx%d frame indices (%d, %d): max|diff| = %.3e" % (xs, ys, vis, nonvis, err))
    assert err <= 1e-5, err


@pytest.mark.gpu
def test_packed_rgba8_with_alpha_agrees_with_the_float_output():
    from libjxl_amd import VarDctDecoder
    xs, ys = 300, 200
    fmt = dict(transfer=abi.TF_SRGB, sample_type=abi.SAMPLE_U8, num_channels=4, bits_per_sample=8)
    p_lin, t = synth.synth_frame(xs, ys, device="cuda", output_kind=1, gab=True, epf_iters=1)
    p_8, _ = synth.synth_frame(xs, ys, device="cuda", output_kind=2, gab=True, epf_iters=1, out_format=fmt)
    alpha = np.random.default_rng(3).random((ys, xs), dtype=np.float32)
    dec = VarDctDecoder(0)
    try:
        dq = dec.default_dequant_tables()
        lin = _decode(dec, p_lin, t, dq, noise=(LUT, 1, 0))
        lin_plain = _decode(dec, p_lin, t, dq)
        out8 = _decode(dec, p_8, t, dq, noise=(LUT, 1, 0), alpha=alpha)
        out8_plain = _decode(dec, p_8, t, dq, alpha=alpha)
    finally:
        dec.close()
    assert np.abs(lin - lin_plain).max() > 1e-3
    c = np.clip(lin, 0, 1)
    srgb = np.where(c <= 0.0031308, c * 12.92, 1.055 * np.power(c, 1 / 2.4) - 0.055) * 255.0
    assert np.abs(out8[..., :3].astype(np.float32) - srgb).max() <= 1.6
    assert np.array_equal(out8[..., 3], out8_plain[..., 3])  # alpha untouched by the noise


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1])
def test_a_silent_lut_is_bit_identical_to_no_noise(kind):
    from libjxl_amd import VarDctDecoder
    params, t = synth.synth_frame(300, 520, device="cuda", output_kind=kind, gab=True, epf_iters=2)
    dec = VarDctDecoder(0)
    try:
        dq = dec.default_dequant_tables()
        plain = _decode(dec, params, t, dq)
        silent = _decode(dec, params, t, dq, noise=([0.0009, -0.001, 0.0, 0.0005, 0.0, 0.0, 0.001, 0.0], 1, 0))
    finally:
        dec.close()
    assert np.array_equal(plain, silent)


@pytest.mark.gpu
def test_a_frame_after_a_noise_frame_is_untouched():
    from libjxl_amd import VarDctDecoder
    params, t = synth.synth_frame(600, 400, device="cuda", output_kind=1, gab=True, epf_iters=1)
    fresh = VarDctDecoder(0)
    used = VarDctDecoder(0)
    try:
        want = _decode(fresh, params, t, fresh.default_dequant_tables())
        dq = used.default_dequant_tables()
        noisy = _decode(used, params, t, dq, noise=(LUT, 1, 0))
        got = _decode(used, params, t, dq)
    finally:
        fresh.close()
        used.close()
    assert np.abs(noisy - want).max() > 1e-3
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_refused_configurations(L):
    import torch
    from libjxl_amd import VarDctDecoder
    lut = (C.c_float * 8)(*LUT)
    # several devices (a device may be listed twice)
    ctx = C.c_void_p()
    devs = (C.c_int * 2)(0, 0)
    assert L.jxlhip_create_multi(devs, 2, None, C.byref(ctx)) == 0
    try:
        assert L.jxlhip_set_noise(ctx, lut, 1, 0) == -7
        assert b"multi-device" in L.jxlhip_last_error(ctx)
    finally:
        L.jxlhip_destroy(ctx)
    dec = VarDctDecoder(0)
    try:
        # a stripe of the frame
        params, t = synth.synth_frame(300, 520, device="cuda", output_kind=1, gab=True, epf_iters=1)
        striped = dict(params, stripe_group_y0=1, stripe_group_rows=1)
        dec.begin_frame(striped)
        assert L.jxlhip_set_noise(dec.ctx, lut, 1, 0) == -7
        assert b"stripes" in L.jxlhip_last_error(dec.ctx)
        # undo_orientation
        dec.begin_frame(dict(params, undo_orientation=6))
        assert L.jxlhip_set_noise(dec.ctx, lut, 1, 0) == -7
        assert b"undo_orientation" in L.jxlhip_last_error(dec.ctx)
        # the split calls
        dq = dec.default_dequant_tables()
        dec.begin_frame(params)
        dec.set_inputs(t, dq)
        dec.set_noise(LUT, 1, 0)
        dec.decode_blocks()
        out = torch.empty((520, 300, 3), dtype=torch.float32, device="cuda")
        assert L.jxlhip_decode_filters(dec.ctx, C.c_void_p(out.data_ptr()), 300 * 12, 0) == -7
        assert b"split calls" in L.jxlhip_last_error(dec.ctx)
        assert L.jxlhip_decode_filters_rows(dec.ctx, C.c_void_p(out.data_ptr()), 300 * 12, 0, 0, 256) == -7
        # ... while jxlhip_decode_frame takes the same frame
        dec.decode_frame(out)
        dec.sync()
    finally:
        dec.close()
