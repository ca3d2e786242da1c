"""Tone mapping on the device (jxlhip_set_tone_mapping, libjxl_amd/csrc/kernels_tonemap.hip).

Kernel against model, on one decoder and one path: the frame is decoded once as linear float and once with tone
mapping; expected = tests/tone_mapping_model.py (held bit for bit to the reference's JxlDecoder by
tests/test_tone_mapping_model.py) applied to the device's OWN linear output and pushed through oracle.pack_output;
actual = the device's tone-mapped output.  What is measured is k_tone_map and nothing in front of it.

Sizes: the smallest at which an elementwise pair-per-lane kernel can go wrong -- 263 x 137 (odd width: the last pixel of
a row is alone), 16 x 8 (less than a wave), 72 x 40, and 16 x 1100 (more rows than grid rows: the row loop) -- with
padded row strides in a sentinel-filled buffer.  Frames: the planted frame (tone_mapping_model.planted_frame: black,
above the source peak, greys, negative components, saturated colours) and a MIX_D1 frame.  Routings: the plain frame,
and noise + splines + 2x upsampling in front (noise + splines alone where the format carries alpha, which an upsampled
frame cannot).

Bars (tone_mapping_model.GPU_BARS, with what was seen on an MI355X): see there.  Every decoder here is created under
JXLHIP_FUSE=0, as in tests/test_gpu_output_encoding.py: both decodes then share XybToRgb on the same planes."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import output_sweep as S
import tone_mapping_model as tm
from libjxl_amd import abi, synth

pytestmark = pytest.mark.gpu

SWITCHES = ("JXLHIP_FUSE", "JXLHIP_FILTERS", "JXLHIP_MFMA", "JXLHIP_FUSED_PC_RH", "JXLHIP_FILTER_RH")
SENTINEL = 0xA5
PAD = 20
SIZES = [(263, 137), (72, 40), (16, 8)]
ORIG = tm.ORIG_NITS
NOISE = ([0.02, 0.03, 0.05, 0.05, 0.04, 0.03, 0.02, 0.02], 1, 0)
FORMATS = tm.gpu_cases()  # (name, output kind, format, desired nits, luminances)


@functools.lru_cache(maxsize=None)
def inputs(frame, size):
    if frame == "planted":
        return tm.planted_frame(*size, device="cuda")
    return synth.synth_frame(*size, mix=synth.MIX_D1, device="cuda")


@functools.lru_cache(maxsize=None)
def alpha_plane(size):
    rng = np.random.default_rng(size[0] * 1000 + size[1])
    a = rng.random((size[1], size[0])).astype(np.float32)
    a[0, :4] = (0.0, 1.0, 0.5, 0.25)
    return a


@pytest.fixture(scope="module")
def dec():
    from libjxl_amd import VarDctDecoder
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ["JXLHIP_FUSE"] = "0"
    try:
        d = VarDctDecoder(0)
        d.dq = d.default_dequant_tables()
    finally:
        os.environ.pop("JXLHIP_FUSE", None)
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v
    yield d
    d.close()


def coded_size(size, features):
    return ((size[0] + 1) // 2, (size[1] + 1) // 2) if "ups" in features else size


def run(dec, frame, size, kind, f, features=(), tone=None, alpha=False, gab=1, epf=1):
    """One decode at output size `size`; the whole sentinel-filled buffer comes back as (H, stride) uint8."""
    cs = coded_size(size, features)
    base, t = inputs(frame, cs)
    dec.begin_frame(dict(base, gab=gab, epf_iters=epf, output_kind=kind, out_format=f))
    dec.set_inputs(t, dec.dq)
    if "ups" in features:
        dec.set_upsampling(2, size)
    if "splines" in features:
        from test_splines_front_end import built_sets
        dec.set_splines(built_sets(*size)["tiny"])
    if "noise" in features:
        dec.set_noise(*NOISE)
    if alpha:
        dec.set_alpha(alpha_plane(size))
    if tone is not None:
        dec.set_tone_mapping(ORIG, tone[0], tone[1])
    dec.profile(True)
    bpp = 12 if kind == 1 else f["num_channels"] * {0: 4, 1: 1, 2: 2, 3: 2}[f["sample_type"]]
    row_bytes = size[0] * bpp
    raw = torch.full((size[1], row_bytes + PAD), SENTINEL, dtype=torch.uint8, device="cuda")
    rc = dec.L.jxlhip_decode_frame(dec.ctx, C.c_void_p(raw.data_ptr()), row_bytes + PAD, 0)
    assert rc == 0, dec.L.jxlhip_last_error(dec.ctx)
    dec.sync()
    raw = raw.cpu().numpy()
    S.check_padding(raw, row_bytes, SENTINEL)
    return np.ascontiguousarray(raw[:, :row_bytes]), dec.profile_read()


def as_f32(body, size):
    return body.view(np.float32).reshape(size[1], size[0], 3)


@pytest.mark.parametrize("features", [(), ("noise", "splines", "ups")], ids=["plain", "features"])
@pytest.mark.parametrize("frame", ["planted", "d1"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("case", FORMATS, ids=lambda c: c[0])
def test_kernel_against_model(oracle, dec, case, size, frame, features):
    name, kind, f, desired, lum = case
    has_alpha = f is not None and f["num_channels"] == 4
    if has_alpha:
        features = tuple(x for x in features if x != "ups")  # (alpha on an upsampled frame is outside the back-end)
    if size == (16, 8) and features:
        features = tuple(x for x in features if x != "splines")  # (an 8 x 4 coded frame is smaller than any spline set)
    lin_body, slots = run(dec, frame, size, 1, None, features)
    assert "tone_map" not in slots, slots
    lin = as_f32(lin_body, size)
    got_body, slots = run(dec, frame, size, kind, f, features, tone=(desired, lum), alpha=has_alpha)
    assert slots.get("tone_map", (0, 0))[1] == 1, slots
    for feat, slot in (("noise", "noise"), ("splines", "splines"), ("ups", "upsample")):
        assert (slot in slots) == (feat in features), slots
    dest_pq = f is not None and f["transfer"] == abi.TF_PQ
    k = tm.constants(ORIG, desired, lum, dest_pq)
    if frame == "planted" and size != (16, 8) and not features:
        assert tm.population_problems(lin, k) == []
    mapped = tm.tone_map(lin, k)
    if kind == 1:
        got = as_f32(got_body, size)
        res = tm.compare_f32(got, mapped)
    else:
        want = oracle.pack_output(f, mapped)
        got = S.rows_of(f, np.ascontiguousarray(got_body), size[0])[0]
        res = tm.compare_packed(f, got, want)
        if has_alpha:  # the tail's alpha: exactly what the same tail writes without tone mapping
            plain_body, _ = run(dec, frame, size, kind, f, features, alpha=True)
            plain = S.rows_of(f, np.ascontiguousarray(plain_body), size[0])[0]
            assert np.array_equal(got[..., 3], plain[..., 3]) and len(np.unique(got[..., 3])) > 16
    print("WORST tone_map %s %dx%d %s %s %s" % (name, size[0], size[1], frame, "+".join(features) or "plain", res))
    tm.check_bar(name, res)


def test_state_and_refusals(dec):
    """frame_begin resets; desired >= orig and a non-PQ original launch nothing new (by the profile slots); every
    refusal with its reason."""
    L = dec.L
    size = (72, 40)
    lum = S.SRGB_LUMINANCES
    plain, slots = run(dec, "d1", size, 1, None)
    assert "tone_map" not in slots
    mapped, slots = run(dec, "d1", size, 1, None, tone=(250.0, lum))
    assert slots["tone_map"][1] == 1 and not np.array_equal(mapped, plain)
    again, slots = run(dec, "d1", size, 1, None)  # frame_begin has reset it
    assert "tone_map" not in slots and np.array_equal(again, plain)
    for desired in (1000.0, 4000.0):  # the reference adds no stage
        same, slots = run(dec, "d1", size, 1, None, tone=(desired, lum))
        assert "tone_map" not in slots and np.array_equal(same, plain)

    def begin(**kw):
        base, t = inputs("d1", size)
        dec.begin_frame(dict(base, **kw))
        dec.set_inputs(t, dec.dq)

    def setter(orig=1000.0, desired=250.0, tf=abi.TF_PQ, lums=lum):
        t = abi.ToneMapping(orig, desired, (C.c_float * 3)(*lums), tf)
        return L.jxlhip_set_tone_mapping(dec.ctx, C.byref(t)), L.jxlhip_last_error(dec.ctx)

    begin(output_kind=1)
    assert setter(tf=abi.TF_SRGB)[0] == 0  # an sRGB original: no stage, no error
    rc, why = setter(tf=abi.TF_HLG)
    assert rc == -7 and b"HLG" in why
    for bad in (dict(orig=0.0), dict(desired=-1.0), dict(orig=float("inf")), dict(desired=float("nan")), dict(tf=6),
                dict(lums=(float("nan"), 0.5, 0.5))):
        assert setter(**bad)[0] == -1, bad
    # NULL switches it off
    assert setter()[0] == 0 and L.jxlhip_set_tone_mapping(dec.ctx, None) == 0
    out = dec.decode_frame()
    dec.sync()
    assert np.array_equal(out.cpu().numpy().view(np.uint8).reshape(size[1], -1), plain)
    # the split calls
    begin(output_kind=1)
    assert setter()[0] == 0
    dec.decode_blocks()
    o = dec.alloc_output()
    rc = L.jxlhip_decode_filters(dec.ctx, C.c_void_p(o.data_ptr()), size[0] * 12, 0)
    assert rc == -7 and b"tone mapping with the split calls" in L.jxlhip_last_error(dec.ctx)
    # planar XYB, orientation, stripes
    begin(output_kind=0)
    rc, why = setter()
    assert rc == -7 and b"planar XYB" in why
    begin(output_kind=1, undo_orientation=6)
    rc, why = setter()
    assert rc == -7 and b"undo_orientation" in why
    base, t = inputs("d1", (72, 520))
    dec.begin_frame(dict(base, output_kind=1, stripe_group_y0=1, stripe_group_rows=1))
    rc, why = setter()
    assert rc == -7 and b"stripes" in why
    # blending, both ways round
    begin(output_kind=1)
    dec.set_blending(size, (0, 0), abi.BLEND_ADD, save_slot=1)
    rc, why = setter()
    assert rc == -7 and b"blended frame" in why
    begin(output_kind=1)
    assert setter()[0] == 0
    b = abi.BlendParams(size[0], size[1], 0, 0, abi.BLEND_ADD, 0, 0, 1)
    assert L.jxlhip_set_blending(dec.ctx, C.byref(b)) == -7 and b"tone-mapped frame" in L.jxlhip_last_error(dec.ctx)
    # before frame_begin, and a multi-device context
    from libjxl_amd import VarDctDecoder
    fresh = VarDctDecoder(0)
    try:
        t = abi.ToneMapping(1000.0, 250.0, (C.c_float * 3)(*lum), abi.TF_PQ)
        assert L.jxlhip_set_tone_mapping(fresh.ctx, C.byref(t)) == -6
    finally:
        fresh.close()
    devs = (C.c_int * 2)(0, 0)
    multi = C.c_void_p()
    assert L.jxlhip_create_multi(devs, 2, None, C.byref(multi)) == 0
    try:
        t = abi.ToneMapping(1000.0, 250.0, (C.c_float * 3)(*lum), abi.TF_PQ)
        assert L.jxlhip_set_tone_mapping(multi, C.byref(t)) == -7 and b"multi-device" in L.jxlhip_last_error(multi)
    finally:
        L.jxlhip_destroy(multi)


def test_profile_slot_layout():
    assert abi.KERNEL_COUNT == 8 and abi.KERNEL_NAMES_EX[10] == "tone_map" and abi.KERNEL_COUNT_EX >= 11


# ---- whole files against JxlDecoder ------------------------------------------------------------------------------------

# (name, primaries asked of both decoders, the reference's transfer function, JXLHIP_TF_*)
DESTINATIONS = [("pq-rec2100", "rec2100", "pq", abi.TF_PQ), ("srgb-rec2100", "rec2100", "srgb", abi.TF_SRGB),
                ("srgb-srgb", "srgb", "srgb", abi.TF_SRGB), ("linear-srgb", "srgb", "linear", abi.TF_LINEAR)]


@pytest.fixture(scope="module")
def files(oracle):
    import sys
    if not oracle.ref_available():
        pytest.skip("oracle/_ref not available")
    oracle.ref_lib()
    import test_seam
    sys.path.insert(0, os.path.join(test_seam.ROOT, "integration"))
    import build_seam
    prebuilt = [os.path.join(build_seam.B.OUT, n) for n in ("libjxl_dec_ref.so", "libjxl_dec_hip.so")]
    if not build_seam.available() and not all(os.path.exists(p) for p in prebuilt):
        pytest.skip("reference tree not present and no prebuilt seam libraries")
    RL = test_seam.load(build_seam.build()[0])
    cs = oracle.RealStream(263, 137, seed=12, original="rec2100pq").codestream.tobytes()
    R, runner, pool = test_seam.hip_runner()
    yield RL, cs, runner, pool
    R.JxlThreadParallelRunnerDestroy(pool)


def decode_file(dec, cs, tf, runner=None, pool=None, through_next=False):
    """float RGB of the file in transfer function tf (its PQ curve at the original's 1000 nits, as the reference's)."""
    L = dec.L
    f = abi.OutputFormat(tf, abi.SAMPLE_F32, 3, 32, 0, ORIG if tf == abi.TF_PQ else 0.0, (C.c_float * 3)(*S.SRGB_LUMINANCES))
    out = torch.full((137, 263, 3), -7.0, dtype=torch.float32, device="cuda")
    info = abi.CodestreamInfo()
    if through_next:
        cursor, fr = C.c_uint64(0), abi.SequenceFrame()
        rc = L.jxlhip_decode_codestream_next(dec.ctx, runner, pool, cs, len(cs), C.byref(cursor), 2, C.byref(f), out.data_ptr(),
                                             263 * 12, 0, C.byref(info), C.byref(fr))
        assert rc == 0 and fr.is_last == 1, L.jxlhip_last_error(dec.ctx)
    else:
        rc = L.jxlhip_decode_codestream(dec.ctx, runner, pool, cs, len(cs), 2, C.byref(f), out.data_ptr(), 263 * 12, 0, C.byref(info))
        assert rc == 0, L.jxlhip_last_error(dec.ctx)
    return out.cpu().numpy(), info


@pytest.mark.parametrize("workers", [0, 6])
@pytest.mark.parametrize("dest", DESTINATIONS, ids=lambda d: d[0])
@pytest.mark.parametrize("desired", [250.0, 100.0])
def test_whole_file_against_jxldecoder(dec, files, desired, dest, workers):
    """jxlhip_codestream_set_display + jxlhip_decode_codestream (and _next) == JxlDecoder with
    JxlDecoderSetDesiredIntensityTarget + JxlDecoderSetOutputColorProfile, within tm.FILE_BARS; the same file's plain
    error (no tone mapping, same primaries and curve) is measured beside it."""
    RL, cs, runner, pool = files
    name, prim, ref_tf, tf = dest
    run_with = (runner, pool) if workers else (None, None)
    enc = tm.color_encoding(prim, ref_tf)
    try:
        dec.set_display(0.0, prim)
        got_plain, info = decode_file(dec, cs, tf, *run_with)
        assert info.intensity_target == ORIG and info.primaries == tm.PRIMARIES[prim]
        want_plain, _ = tm.jxl_decode_display(RL, cs, None, enc)
        dec.set_display(desired, prim)
        dec.profile(True)
        dec.profile_read()  # (drops the spans of earlier decodes)
        got, info = decode_file(dec, cs, tf, *run_with)
        assert dec.profile_read()["tone_map"][1] == 1
        assert info.intensity_target == desired and info.primaries == tm.PRIMARIES[prim]
        got_next, _ = decode_file(dec, cs, tf, *run_with, through_next=True)
        assert np.array_equal(got_next, got)
        want, _ = tm.jxl_decode_display(RL, cs, desired, enc)
    finally:
        dec.set_display()
    err_plain = float(np.abs(got_plain - want_plain).max())
    err = float(np.abs(got - want).max())
    print("FILE %s %g nits workers=%d: tone-mapped max|diff| %.3e, plain %.3e (range %.3f)" % (
        name, desired, workers, err, err_plain, float(np.abs(want).max())))
    if tf == abi.TF_LINEAR:
        assert err_plain <= 2e-5 * max(1.0, float(np.abs(want_plain).max()))  # the project's bar for linear pixels
    assert err <= tm.FILE_BARS[name, desired], (err, tm.FILE_BARS[name, desired])


def test_display_state(dec, files):
    """Sticky until NULL; a display at least as bright as the original launches nothing new; refusals with their reason."""
    RL, cs, runner, pool = files
    L = dec.L
    try:
        plain, info = decode_file(dec, cs, abi.TF_LINEAR)
        dec.set_display(250.0)
        a, _ = decode_file(dec, cs, abi.TF_LINEAR)
        b, _ = decode_file(dec, cs, abi.TF_LINEAR)  # sticky
        assert np.array_equal(a, b) and not np.array_equal(a, plain)
        assert L.jxlhip_codestream_set_display(dec.ctx, None) == 0
        c, info = decode_file(dec, cs, abi.TF_LINEAR)
        assert np.array_equal(c, plain) and info.intensity_target == ORIG
        for nits in (1000.0, 4000.0):
            dec.set_display(nits)
            dec.profile(True)
            dec.profile_read()  # (drops the spans of earlier decodes)
            d, info = decode_file(dec, cs, abi.TF_LINEAR)
            assert "tone_map" not in dec.profile_read() and np.array_equal(d, plain) and info.intensity_target == nits
        for bad, rc in ((abi.Display(-1.0, 0, 0), -1), (abi.Display(float("nan"), 0, 0), -1), (abi.Display(0.0, 5, 0), -1),
                        (abi.Display(0.0, 0, 3), -1), (abi.Display(0.0, abi.PRIM_CUSTOM, 0), -7), (abi.Display(0.0, 0, abi.WP_CUSTOM), -7)):
            assert L.jxlhip_codestream_set_display(dec.ctx, C.byref(bad)) == rc
        assert b"custom xy" in L.jxlhip_last_error(dec.ctx)
    finally:
        dec.set_display()


def test_rows_beyond_the_grid(oracle, dec):
    """16 x 1100: more rows than the launch has grid rows (1024), so the row-stride loop of k_tone_map takes a second
    turn for rows 1024 .. 1099; bit-equal to the model like every other linear-float run."""
    size = (16, 1100)
    lin = as_f32(run(dec, "planted", size, 1, None)[0], size)
    got = as_f32(run(dec, "planted", size, 1, None, tone=(250.0, S.SRGB_LUMINANCES))[0], size)
    k = tm.constants(ORIG, 250.0, S.SRGB_LUMINANCES, False)
    want = tm.tone_map(lin, k)
    assert not np.array_equal(got[1024:], lin[1024:])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- multi-frame files through jxlhip_decode_codestream_next ---------------------------------------------------------

def next_frames(dec, cs, count, tf=abi.TF_LINEAR, size=(263, 137), runner=None, pool=None):
    L = dec.L
    w, h = size
    f = abi.OutputFormat(tf, abi.SAMPLE_F32, 3, 32, 0, ORIG if tf == abi.TF_PQ else 0.0, (C.c_float * 3)(*S.SRGB_LUMINANCES))
    cursor, frames, infos = C.c_uint64(0), [], []
    for k in range(count):
        out = torch.full((h, w, 3), -7.0, dtype=torch.float32, device="cuda")
        info, fr = abi.CodestreamInfo(), abi.SequenceFrame()
        rc = L.jxlhip_decode_codestream_next(dec.ctx, runner, pool, cs, len(cs), C.byref(cursor), 2, C.byref(f), out.data_ptr(),
                                             w * 12, 0, C.byref(info), C.byref(fr))
        assert rc == 0, (k, L.jxlhip_last_error(dec.ctx))
        assert fr.index == k and fr.is_last == int(k == count - 1)
        frames.append(out.cpu().numpy())
        infos.append(info)
    return frames, infos


@pytest.mark.parametrize("workers", [0, 6])
def test_three_frame_pq_animation_through_next(oracle, dec, files, workers):
    """A three-frame full-kReplace animation of Rec.2100 PQ frames (tone_mapping_model.with_animation +
    layer_streams.splice) with the sticky display: every frame is tone-mapped (one k_tone_map launch per frame) and
    equals JxlDecoder's frame with the same two calls within tm.ANIMATION_BAR."""
    RL, _, runner, pool = files
    streams = [oracle.RealStream(263, 137, seed=s, original="rec2100pq").codestream.tobytes() for s in (12, 5, 9)]
    cs = tm.splice_animation(dec.L, tm.with_animation(dec.L, streams[0]), streams, [3, 2, 5])
    want = tm.jxl_decode_frames_display(RL, cs, 250.0, tm.color_encoding("srgb", "linear"))
    plain = tm.jxl_decode_frames_display(RL, cs, None, tm.color_encoding("srgb", "linear"))
    assert len(want) == 3
    try:
        dec.set_display(250.0, "srgb")
        dec.profile(True)
        dec.profile_read()
        got, infos = next_frames(dec, cs, 3, runner=runner if workers else None, pool=pool if workers else None)
        assert dec.profile_read()["tone_map"][1] == 3
    finally:
        dec.set_display()
    worst = 0.0
    for k in range(3):
        assert infos[k].intensity_target == 250.0 and infos[k].primaries == 1
        assert float(np.abs(want[k] - plain[k]).max()) > 0.05
        worst = max(worst, float(np.abs(got[k] - want[k]).max()))
    print("FILE animation-3 250 nits workers=%d: tone-mapped max|diff| %.3e" % (workers, worst))
    assert worst <= tm.ANIMATION_BAR


def test_srgb_animation_with_a_display(oracle, dec, files):
    """The oracle's own animation (an sRGB original): P3 output primaries on every frame, and display_nits that leaves
    each frame on its plain path (no stage for an sRGB original), against JxlDecoder at the project's 2e-5."""
    RL, _, runner, pool = files
    cs = oracle.feature_stream("animation")
    enc = tm.color_encoding("p3", "linear")
    want = tm.jxl_decode_frames_display(RL, cs, 100.0, enc)
    h, w = want[0].shape[:2]
    try:
        dec.set_display(100.0, "p3")
        dec.profile(True)
        dec.profile_read()
        got, infos = next_frames(dec, cs, len(want), size=(w, h), runner=runner, pool=pool)
        assert "tone_map" not in dec.profile_read()
    finally:
        dec.set_display()
    orig = tm.jxl_decode_frames_display(RL, cs)
    for k in range(len(want)):
        assert infos[k].intensity_target == 100.0 and infos[k].primaries == 11
        assert float(np.abs(want[k] - orig[k]).max()) > 1e-3  # the primaries show
        assert float(np.abs(got[k] - want[k]).max()) <= 2e-5 * max(1.0, float(np.abs(want[k]).max()))


def test_blended_sequence_frame_refused_with_display_nits(oracle, dec):
    """A sequence frame that needs blending while display_nits is set; the primaries alone are taken."""
    import layer_streams as ls
    L = dec.L
    fs = lambda n, size=(203, 137), seed=5: oracle.feature_stream(n, xsize=size[0], ysize=size[1], seed=seed, distance=1.0)  # noqa: E731
    cs = ls.splice(L, fs("animation"), [dict(stream=fs("plain"), duration=3, save_as_reference=1),
                                        dict(stream=fs("plain", (72, 40), 7), crop=(37, 21), mode=ls.ADD, source=1, duration=2)])
    f = abi.OutputFormat(abi.TF_LINEAR, abi.SAMPLE_F32, 3, 32, 0, 0.0, (C.c_float * 3)(*S.SRGB_LUMINANCES))
    out = torch.empty((137, 203, 3), dtype=torch.float32, device="cuda")
    try:
        dec.set_display(100.0)
        cursor = C.c_uint64(0)
        rc = L.jxlhip_decode_codestream_next(dec.ctx, None, None, cs, len(cs), C.byref(cursor), 2, C.byref(f), out.data_ptr(),
                                             203 * 12, 0, None, None)
        assert rc == -7 and b"needs blending while display_nits is set" in L.jxlhip_last_error(dec.ctx)
        dec.set_display(0.0, "p3")
        got, infos = next_frames(dec, cs, 2, size=(203, 137))
        assert infos[1].primaries == 11
    finally:
        dec.set_display()


# ---- the command-line tool -------------------------------------------------------------------------------------------

def test_djxl_hip_with_display_flags(oracle, files, tmp_path):
    """tools/djxl_hip.py --display_nits 250 --output_primaries srgb on the 1000-nit Rec.2100 PQ stream == JxlDecoder with
    the same two calls: .npy (linear float) within the whole-file bar, .ppm (8-bit, the original's PQ curve at the
    original's 1000 nits) at most one level apart; --frames with a display on the three-frame PQ animation."""
    import subprocess
    import sys
    RL, cs, _, _ = files
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "pq.jxl"
    src.write_bytes(cs)
    flags = ["--display_nits", "250", "--output_primaries", "srgb", "--threads", "4"]

    def tool(*args):
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "djxl_hip.py"), *args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]

    tool(str(src), str(tmp_path / "out.npy"), *flags)
    want, _ = tm.jxl_decode_display(RL, cs, 250.0, tm.color_encoding("srgb", "linear"))
    got = np.load(tmp_path / "out.npy")
    err = float(np.abs(got - want).max())
    print("FILE djxl_hip npy 250 nits srgb: max|diff| %.3e" % err)
    assert err <= tm.FILE_BARS["linear-srgb", 250.0]
    tool(str(src), str(tmp_path / "out.ppm"), *flags)
    want_pq, _ = tm.jxl_decode_display(RL, cs, 250.0, tm.color_encoding("srgb", "pq"))
    raw = (tmp_path / "out.ppm").read_bytes()
    px = np.frombuffer(raw[len(raw) - 263 * 137 * 3:], np.uint8).reshape(137, 263, 3).astype(np.int32)
    want8 = np.clip(np.rint(want_pq * 255.0), 0, 255).astype(np.int32)  # (undithered: the tool's samples are dithered by < 1 level)
    assert int(np.abs(px - want8).max()) <= 1
    streams = [oracle.RealStream(263, 137, seed=s, original="rec2100pq").codestream.tobytes() for s in (12, 5, 9)]
    L = abi.load_library()
    anim = tm.splice_animation(L, tm.with_animation(L, streams[0]), streams, [3, 2, 5])
    (tmp_path / "anim.jxl").write_bytes(anim)
    tool(str(tmp_path / "anim.jxl"), str(tmp_path / "f.npy"), "--frames", *flags)
    wants = tm.jxl_decode_frames_display(RL, anim, 250.0, tm.color_encoding("srgb", "linear"))
    for k in range(3):
        assert float(np.abs(np.load(tmp_path / ("f-%03d.npy" % k)) - wants[k]).max()) <= tm.ANIMATION_BAR
