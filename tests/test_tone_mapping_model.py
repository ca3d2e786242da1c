"""The tone-mapping model (tests/tone_mapping_model.py) against the reference's public JxlDecoder, on the CPU, before
any GPU is involved, and the host part of jxlhip_set_tone_mapping against the model.

Model against reference: the input is the reference's OWN linear output of the file (JxlDecoderSetOutputColorProfile
with a linear encoding of the destination primaries), the expected output its tone-mapped output
(JxlDecoderSetDesiredIntensityTarget on top).  Streams: oracle.RealStream(original="rec2100pq"), 1000 nits, at
263 x 137 and 72 x 40; desired 250 and 100 nits; destinations PQ Rec.2100, sRGB-curve Rec.2100, sRGB-curve sRGB
primaries, and linear (both primaries).

Measured first, as the model was written: on the one-lane build of the reference the model is BIT-EQUAL for the linear
destinations (every sample of all eight frames), so that test is array_equal.  For the encoded destinations the
reference's FromLinearStage follows; the model's output goes through oracle.pack_output (the restatement of that
stage, held byte for byte to the reference by tests/test_reference_parity.py), and that too is bit-equal.

Population: every case (desired x destination) has pixels on both sides of the knee start ks at each size -- with one
exception named in the test: the 72 x 40 frame has none below the 100-nit knee, nor below any knee under a PQ destination (its darkest pixel is 37 nits, that knee
starts near 25; seeds 1 .. 200 were tried), the 263 x 137 one has 240.  The planted frame, at 263 x 137 and 72 x 40,
(tone_mapping_model.planted_frame, the reference FrameDecoder's pixels for it) carries black, luminance above the
source peak, greys, negative components and components above 1 behind the mapping."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from libjxl_amd import abi

import output_sweep as S
import tone_mapping_model as tm

SIZES = [(263, 137), (72, 40)]
SEED = 12
ORIG = 1000.0
DESIRED = [250.0, 100.0]
# (name, primaries, transfer function of the reference, JXLHIP_TF_*)
DESTINATIONS = [("pq-rec2100", "rec2100", "pq", abi.TF_PQ), ("srgb-rec2100", "rec2100", "srgb", abi.TF_SRGB),
                ("srgb-srgb", "srgb", "srgb", abi.TF_SRGB), ("linear-rec2100", "rec2100", "linear", abi.TF_LINEAR),
                ("linear-srgb", "srgb", "linear", abi.TF_LINEAR)]


@pytest.fixture(scope="module")
def kit(oracle):
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
    L = abi.load_library()
    streams, linear, lums = {}, {}, {}
    for size in SIZES:
        cs = oracle.RealStream(*size, seed=SEED, original="rec2100pq").codestream.tobytes()
        streams[size] = cs
        for prim in ("rec2100", "srgb"):
            lin, nits = tm.jxl_decode_display(RL, cs, None, tm.color_encoding(prim, "linear"))
            assert nits == ORIG and lin.shape == (size[1], size[0], 3)
            lin.setflags(write=False)
            linear[size, prim] = lin
    # the destination primaries' luminances: the header with the requested space named in it
    a = np.frombuffer(streams[SIZES[0]], np.uint8)
    for prim, code in (("rec2100", 9), ("srgb", 1)):
        ih, pos = abi.ImageHeader(), C.c_size_t(0)
        assert L.jxlhip_image_header_decode(a.ctypes.data, len(a), C.byref(pos), None, 0, C.byref(ih)) == 0
        ih.color_encoding.primaries = code
        m, lum = (C.c_float * 9)(), (C.c_float * 3)()
        assert L.jxlhip_output_opsin_matrix(C.byref(ih), m, lum) == 0
        lums[prim] = tuple(lum)
    return L, RL, streams, linear, lums


def expected(oracle, tf, mapped):
    """The model's linear output through FromLinearStage's restatement, as float samples."""
    if tf == abi.TF_LINEAR:
        return mapped
    return oracle.pack_output(S.fmt(tf, abi.SAMPLE_F32, 3, par=ORIG if tf == abi.TF_PQ else 0.0), mapped)


@pytest.mark.parametrize("dest", DESTINATIONS, ids=lambda d: d[0])
@pytest.mark.parametrize("desired", DESIRED)
def test_model_equals_the_reference(oracle, kit, desired, dest):
    L, RL, streams, linear, lums = kit
    name, prim, ref_tf, tf = dest
    k = tm.constants(ORIG, desired, lums[prim], tf == abi.TF_PQ)
    for size in SIZES:
        lin = linear[size, prim]
        want, nits = tm.jxl_decode_display(RL, streams[size], desired, tm.color_encoding(prim, ref_tf))
        assert nits == desired  # (decode.cc:2247: the basic info reports the display's peak)
        plain, _ = tm.jxl_decode_display(RL, streams[size], None, tm.color_encoding(prim, ref_tf))
        assert float(np.abs(want - plain).max()) > 0.05  # the two calls change the reference's output
        got = expected(oracle, tf, tm.tone_map(lin, k))
        ne = got.view(np.uint32) != want.view(np.uint32)
        print("MODEL %s %g nits %dx%d: %d of %d samples differ, worst %.2f ulp" % (
            name, desired, size[0], size[1], int(ne.sum()), ne.size, float(S.ulp_distance(got, want).max())))
        assert not ne.any()
        _, npq = tm.normalized_pq(lin, k)
        below, above = int((npq < k[tm.K_KS]).sum()), int((npq >= k[tm.K_KS]).sum())
        # both sides of the knee in every case at every size -- but for the one the stream cannot give: no 72 x 40
        # frame of this encoder's procedural image (seeds 1 .. 200) has a pixel under the 100-nit knee, which starts
        # near 25 nits (the darkest pixel of seed 12 is 37 nits).  The planted frame straddles it at both sizes
        # (test_planted_frame_population).  Under a PQ destination the stage first multiplies the pixel by 10000 / orig
        # = 10, which lifts that frame above the 250-nit knee (near 115 nits) as well.
        if not (size == (72, 40) and (desired == 100.0 or tf == abi.TF_PQ)):
            assert below > 0, (size, desired, below)
        assert above > 0, (size, desired, above)


def _planted(oracle, size):
    import frames
    params, t = tm.planted_frame(*size, gab=0, epf_iters=0)
    fr = frames.oracle_frame(params, t, oracle.default_dequant_tables())
    lin = fr.decode_ref(threads=1) if oracle.ref_available() else fr.decode(threads=1)
    lin.setflags(write=False)
    return lin


@pytest.fixture(scope="module")
def planted(oracle):
    return _planted(oracle, (263, 137))


@pytest.fixture(scope="module")
def planted_small(oracle):
    return _planted(oracle, (72, 40))


@pytest.mark.parametrize("desired", DESIRED)
@pytest.mark.parametrize("lum", [S.SRGB_LUMINANCES, (0.2627002, 0.677998, 0.0593017)], ids=["srgb", "rec2100"])
def test_planted_frame_population(planted, planted_small, desired, lum):
    for dest_pq in (False, True):
        k = tm.constants(ORIG, desired, lum, dest_pq)
        for lin in (planted, planted_small):
            assert tm.population_problems(lin, k) == []
            assert np.isfinite(tm.tone_map(lin, k)).all()


@pytest.mark.parametrize("orig,desired", [(1000.0, 250.0), (1000.0, 100.0), (4000.0, 203.0), (10000.0, 48.0), (255.0, 254.0)])
@pytest.mark.parametrize("dest", [abi.TF_LINEAR, abi.TF_SRGB, abi.TF_PQ])
def test_host_constants_equal_the_model_bit_for_bit(orig, desired, dest):
    L = abi.load_library()
    lum = (0.2627002, 0.677998, 0.0593017)
    t = abi.ToneMapping(orig, desired, (C.c_float * 3)(*lum), abi.TF_PQ)
    out = (C.c_float * abi.TONE_MAPPING_CONSTANTS)()
    assert L.jxlhip_tone_mapping_constants(C.byref(t), dest, out, abi.TONE_MAPPING_CONSTANTS) == 0
    got, want = np.array(out[:], np.float32), tm.constants(orig, desired, lum, dest == abi.TF_PQ)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
    assert want[tm.K_KS] < 1 and want[tm.K_PQMIN] == 0 and want[tm.K_MINLUM] == 0


def test_host_constants_refusals():
    L = abi.load_library()
    out = (C.c_float * 18)()

    def rc(orig=1000.0, desired=250.0, tf=abi.TF_PQ, dest=0, n=18, lum=(0.2, 0.7, 0.1)):
        t = abi.ToneMapping(orig, desired, (C.c_float * 3)(*lum), tf)
        return L.jxlhip_tone_mapping_constants(C.byref(t), dest, out, n)

    assert rc() == 0 and rc(n=3) == 0
    for bad in (dict(orig=0.0), dict(desired=0.0), dict(desired=float("nan")), dict(orig=float("inf")), dict(tf=6),
                dict(tf=abi.TF_HLG), dict(tf=abi.TF_SRGB), dict(desired=1000.0), dict(desired=2000.0), dict(dest=6),
                dict(n=19), dict(lum=(float("inf"), 0.0, 0.0))):
        assert rc(**bad) == -1, bad
    assert L.jxlhip_tone_mapping_constants(None, 0, out, 18) == -1


@pytest.mark.parametrize("fault", tm.FAULTS)
def test_the_gpu_tiers_bars_see_every_fault(oracle, planted, fault):
    """Each fault, put into the model alone, moves the frames of the GPU tier's cases by at least 5x the bar that tier
    holds the kernel to (tone_mapping_model.GPU_BARS): float samples by 5x the ulp bar (and at least one ulp), integer
    and half-float samples by 5 codes / steps or 5x the share cap.  A bar too loose to see a fault fails here.  The
    frames are the tier's two, as the reference's FrameDecoder decodes them on the CPU."""
    import frames
    from libjxl_amd import synth
    params, t = synth.synth_frame(263, 137, mix=synth.MIX_D1)
    fr = frames.oracle_frame(params, t, oracle.default_dequant_tables())
    d1 = fr.decode_ref(threads=1) if oracle.ref_available() else fr.decode(threads=1)
    for name, kind, f, desired, lum in tm.gpu_cases():
        dest_pq = f is not None and f["transfer"] == abi.TF_PQ
        if fault == "no_to_intensity_target" and not dest_pq:
            continue  # (the factor is 1 for every other destination: there is nothing to drop)
        k = tm.constants(ORIG, desired, lum, dest_pq)
        bar = tm.GPU_BARS[name]
        for frame, lin in (("planted", planted), ("d1", d1)):
            good, bad = tm.tone_map(lin, k), tm.tone_map(lin, k, fault=fault)
            if kind == 1:
                res = tm.compare_f32(bad, good)
                seen = res["ulp"] >= max(1.0, 5 * bar["ulp"])
            else:
                res = tm.compare_packed(f, oracle.pack_output(f, bad), oracle.pack_output(f, good))
                seen = res["maxdiff"] >= max(1, 5 * bar["maxdiff"]) or (bar["share"] > 0 and res["share"] >= 5 * bar["share"])
            print("FAULT %s %s %s: %s" % (fault, name, frame, res))
            # the planted frame is built to see everything.  The MIX_D1 frame must see a fault wherever its pixels can:
            # under a PQ destination the stage scales it by 10000 / orig = 10 first, which puts every pixel of it at
            # 910 nits and more -- on the flat end of the knee spline (slope 0 at t = 1), where moving ks moves nothing
            if frame == "planted" or not (dest_pq and fault == "ks_moved"):
                assert seen, (name, fault, frame, res)


# ---- the display, header-only ---------------------------------------------------------------------------------------

def _display_info(L, cs, nits=0.0, prim=0, wp=0):
    info, why = abi.CodestreamInfo(), C.c_char_p()
    d = abi.Display(nits, prim, wp)
    rc = L.jxlhip_codestream_display_info(cs, len(cs), C.byref(d), C.byref(info), C.byref(why))
    return rc, info, (why.value or b"").decode()


def test_display_info_reports_the_output(oracle):
    if not oracle.ref_available():
        pytest.skip("oracle/_ref not available")
    L = abi.load_library()
    cs = oracle.RealStream(72, 40, seed=3, original="rec2100pq").codestream.tobytes()
    rc, plain, _ = _display_info(L, cs)
    assert rc == 0 and (plain.intensity_target, plain.primaries, plain.white_point, plain.transfer_function) == (1000.0, 9, 1, 16)
    rc, info, _ = _display_info(L, cs, 250.0)
    assert rc == 0 and info.intensity_target == 250.0 and info.primaries == 9 and list(info.luminances) == list(plain.luminances)
    rc, info, _ = _display_info(L, cs, 250.0, abi.PRIM_SRGB, abi.WP_D65)
    assert rc == 0 and (info.intensity_target, info.primaries, info.white_point, info.transfer_function) == (250.0, 1, 1, 16)
    assert [np.float32(v) for v in info.luminances] == [np.float32(v) for v in S.SRGB_LUMINANCES]
    rc, info, _ = _display_info(L, cs, 0.0, abi.PRIM_P3, 0)
    assert rc == 0 and info.intensity_target == 1000.0 and info.primaries == 11 and abs(sum(info.luminances) - 1) < 1e-5
    p3 = oracle.RealStream(72, 40, seed=3, original="p3").codestream.tobytes()
    basic = abi.CodestreamInfo()
    assert L.jxlhip_codestream_basic_info(p3, len(p3), C.byref(basic)) == 0
    assert list(info.luminances) == list(basic.luminances)  # rec2100 -> P3 names the space a P3 original has


@pytest.mark.parametrize("original,asked", [("p3", abi.PRIM_SRGB), ("rec2100pq", abi.PRIM_SRGB), ("srgb8", abi.PRIM_P3),
                                            ("srgb8", abi.PRIM_2100)])
def test_primaries_alone_give_the_references_matrix(oracle, original, asked):
    """The matrix and luminances of a header whose colour encoding names the requested space (what
    jxlhip_codestream_set_display derives them from) against the matrix the REFERENCE decoder derived for a stream whose
    original IS that space -- all these streams code the default opsin matrix, so the two must agree bit for bit after
    the 255 / intensity_target scale, the comparison tests/test_codestream.py uses for the original's own space."""
    if not oracle.ref_available():
        pytest.skip("oracle/_ref not available")
    L = abi.load_library()
    twin = {abi.PRIM_SRGB: "srgb8", abi.PRIM_P3: "p3", abi.PRIM_2100: "rec2100pq"}[asked]
    rs, want = oracle.RealStream(72, 40, seed=3, original=original), oracle.RealStream(72, 40, seed=3, original=twin)
    cs = np.ascontiguousarray(rs.codestream)
    ih, pos = abi.ImageHeader(), C.c_size_t(0)
    assert L.jxlhip_image_header_decode(cs.ctypes.data, len(cs), C.byref(pos), None, 0, C.byref(ih)) == 0
    ih.color_encoding.all_default, ih.color_encoding.color_space = 0, 0
    ih.color_encoding.primaries, ih.color_encoding.white_point = asked, abi.WP_D65
    if ih.color_encoding.transfer_function == 0:
        ih.color_encoding.transfer_function = 13
    m, lum = (C.c_float * 9)(), (C.c_float * 3)()
    assert L.jxlhip_output_opsin_matrix(C.byref(ih), m, lum) == 0
    scale = np.float32(255.0) / np.float32({"rec2100pq": 1000.0}.get(twin, 255.0))  # the twin's intensity target
    mine = np.array([np.float32(v) * scale for v in m], np.float32)
    assert np.array_equal(mine, np.array(want.frame_params.inverse_opsin_matrix, np.float32))
    rc, info, _ = _display_info(L, rs.codestream.tobytes(), 0.0, asked, abi.WP_D65)
    assert rc == 0 and list(info.luminances) == list(lum)


def test_display_refusals(oracle):
    if not oracle.ref_available():
        pytest.skip("oracle/_ref not available")
    L = abi.load_library()
    pq = oracle.RealStream(72, 40, seed=3, original="rec2100pq").codestream.tobytes()
    grey = oracle.RealStream(72, 40, seed=3, original="gray8").codestream.tobytes()
    rc, _, why = _display_info(L, pq, 0.0, abi.PRIM_CUSTOM)
    assert rc == -7 and "custom xy" in why
    rc, _, why = _display_info(L, pq, 0.0, 0, abi.WP_CUSTOM)
    assert rc == -7 and "custom xy" in why
    for nits, prim in ((250.0, 0), (0.0, abi.PRIM_P3)):
        rc, _, why = _display_info(L, grey, nits, prim)
        assert rc == -7 and "grey original" in why
    assert _display_info(L, grey)[0] == 0  # nothing set: exactly as before
    for bad in ((-1.0, 0, 0), (float("inf"), 0, 0), (0.0, 7, 0), (0.0, 0, 4)):
        assert _display_info(L, pq, *bad)[0] == -1, bad


def test_display_refused_for_an_icc_original(oracle):
    """An ICC original with any field of the display set: the reference needs a CMS there."""
    if not oracle.ref_available():
        pytest.skip("oracle/_ref not available")
    from test_icc import make_profile
    L = abi.load_library()
    cs = oracle.RealStream(96, 72, seed=4, distance=2.0, icc=make_profile(False, 64)).codestream.tobytes()
    rc, info, _ = _display_info(L, cs)
    assert rc == 0 and info.icc_size > 0  # nothing set: exactly as before
    for nits, prim, wp in ((250.0, 0, 0), (0.0, abi.PRIM_P3, 0), (0.0, 0, abi.WP_E)):
        rc, _, why = _display_info(L, cs, nits, prim, wp)
        assert rc == -7 and "ICC original" in why, (nits, prim, wp, why)


def test_display_info_reads_sequence_files(oracle):
    """jxlhip_codestream_display_info on a file only the sequence calls take (an animation): what
    jxlhip_codestream_sequence_info reports, with the display applied."""
    if not oracle.ref_available():
        pytest.skip("oracle/_ref not available")
    L = abi.load_library()
    cs = oracle.feature_stream("animation")
    basic = abi.CodestreamInfo()
    assert L.jxlhip_codestream_basic_info(cs, len(cs), C.byref(basic)) == -7
    rc, info, _ = _display_info(L, cs, 100.0, abi.PRIM_P3, abi.WP_D65)
    seq_info, seq = abi.CodestreamInfo(), abi.SequenceInfo()
    assert L.jxlhip_codestream_sequence_info(cs, len(cs), C.byref(seq_info), C.byref(seq)) == 0
    assert rc == 0 and (info.xsize, info.ysize) == (seq_info.xsize, seq_info.ysize)
    assert info.intensity_target == 100.0 and info.primaries == 11 and list(info.luminances) != list(seq_info.luminances)


def test_animation_header_rewriter(oracle):
    """tone_mapping_model.with_animation + splice_animation: a three-frame Rec.2100 PQ animation the reference accepts,
    its frames the single streams' own pixels (full kReplace frames, bit for bit)."""
    if not oracle.ref_available():
        pytest.skip("oracle/_ref not available")
    import test_seam
    sys.path.insert(0, os.path.join(test_seam.ROOT, "integration"))
    import build_seam
    prebuilt = [os.path.join(build_seam.B.OUT, n) for n in ("libjxl_dec_ref.so", "libjxl_dec_hip.so")]
    if not build_seam.available() and not all(os.path.exists(p) for p in prebuilt):
        pytest.skip("reference tree not present and no prebuilt seam libraries")
    RL = test_seam.load(build_seam.build()[0])
    L = abi.load_library()
    streams = [oracle.RealStream(72, 40, seed=s, original="rec2100pq").codestream.tobytes() for s in (12, 5, 9)]
    cs = tm.splice_animation(L, tm.with_animation(L, streams[0]), streams, [3, 2, 5])
    frames = tm.jxl_decode_frames_display(RL, cs)
    assert len(frames) == 3
    for got, one in zip(frames, streams):
        assert np.array_equal(got, tm.jxl_decode_display(RL, one)[0])
    info, seq = abi.CodestreamInfo(), abi.SequenceInfo()
    assert L.jxlhip_codestream_sequence_info(cs, len(cs), C.byref(info), C.byref(seq)) == 0
    assert (seq.have_animation, seq.num_displayed_frames, info.intensity_target, info.transfer_function) == (1, 3, 1000.0, 16)
