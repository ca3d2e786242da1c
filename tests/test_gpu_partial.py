"""Files that end early through jxlhip_decode_codestream_partial against the reference's flushed picture
(JxlDecoderFlushImage on the same bytes, tests/partial_ref.py): three multi-section oracle streams (plain and progressive 600x400, plain 2200x520) cut
  (a) right behind the last DC group          (b) behind AC global, no AC group
  (c) in the middle of an AC section about half-way through (of pass 0: groups without AC beside groups with it)
  (d) one byte short of the end                (e) not at all
and the progressive one also behind pass 0 of every group and inside a section of pass 1; as float RGB within 2e-5 of
the reference (normalised as in tests/test_gpu_patches.py, no pixel left out) and as 8-bit sRGB within one level,
with 0 and 6 workers.  (e) equals jxlhip_decode_codestream bit for bit.  Then a file with custom upsampling weights (its
own 8x table draws the DC-only groups), display orientation, and the refusals."""
import ctypes as C

import numpy as np
import pytest

from libjxl_amd import abi

import partial_ref as pr
import stream_chain as sc

TIGHT = 2e-5
NEED_MORE_INPUT = -9
UNDO = 0x100


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
    return pr.load_reference()


def _cuts(s, size):
    """name -> length"""
    dc_end = max(s.end(i) for i in range(1 + s.ndc))
    ag_end = s.end(1 + s.ndc)
    ac = [(p, g) for p in range(s.np) for g in range(s.ng)]
    assert dc_end < ag_end < min(s.end(s.ac(p, g)) for p, g in ac)  # the file order the cuts assume
    # (c): the section of pass 0 that holds the byte half-way through pass 0 -- half-way through the AC groups of a file
    # of one pass, and in a progressive file the half-way point at which groups WITHOUT any AC are still left
    target = (ag_end + max(s.end(s.ac(0, g)) for g in range(s.ng))) // 2
    mid = [s.ac(0, g) for g in range(s.ng) if s.end(s.ac(0, g)) - s.size[s.ac(0, g)] <= target < s.end(s.ac(0, g))]
    assert len(mid) == 1
    cuts = {"a": dc_end, "b": ag_end, "c": s.end(mid[0]) - s.size[mid[0]] // 2, "d": size - 1, "e": size}
    if s.np > 1:
        cuts["pass0"] = max(s.end(s.ac(0, g)) for g in range(s.ng))
        one = s.ac(1, s.ng // 2)
        cuts["in_pass1"] = s.end(one) - s.size[one] // 2
        assert cuts["pass0"] < cuts["in_pass1"]
    return cuts


CASES = [(key, cut) for key in pr.STREAMS for cut in ("a", "b", "c", "d", "e") + (("pass0", "in_pass1") if key[0] == "progressive" else ())]


@pytest.fixture(scope="module")
def flushed(L, ref, jxl_ref):
    """(stream, cut) -> (the file, the length, the reference's flushed picture): computed once, never modified."""
    ts, RL = jxl_ref
    out = {}
    for key in pr.STREAMS:
        cs = pr.stream(ref, key)
        s = pr.Sections(L, cs)
        for cut, n in _cuts(s, len(cs)).items():
            ok, want = pr.flush(ts, RL, cs[:n])
            assert ok and want.shape == (key[2], key[1], 3) and not (want == pr.SENTINEL).any()
            want.setflags(write=False)
            out[(key, cut)] = (cs, n, want, s.expect(n))
    return out


def _runner(workers):
    R = C.CDLL(abi.runner_library_path())
    R.JxlThreadParallelRunnerCreate.restype = C.c_void_p
    R.JxlThreadParallelRunnerCreate.argtypes = [C.c_void_p, C.c_size_t]
    R.JxlThreadParallelRunnerDestroy.argtypes = [C.c_void_p]
    pool = R.JxlThreadParallelRunnerCreate(None, workers) if workers else None
    return R, pool, C.cast(R.JxlThreadParallelRunner, C.c_void_p) if workers else None


def _decode(L, dec, cs, n, shape, sample=abi.SAMPLE_F32, channels=3, workers=0, whole_call=False, kind=2, tf=abi.TF_SRGB):
    """(rc, pixels, jxlhip_partial_info) of the first n bytes; whole_call: through jxlhip_decode_codestream instead"""
    import torch
    R, pool, runner = _runner(workers)
    try:
        lum = (C.c_float * 3)(0.2126, 0.7152, 0.0722)
        if sample == abi.SAMPLE_F32:
            fmt = abi.OutputFormat(tf, abi.SAMPLE_F32, channels, 32, 0, 0.0, lum)
            out = torch.full(shape + (channels,), -7.0, dtype=torch.float32, device="cuda")
        else:
            fmt = abi.OutputFormat(tf, abi.SAMPLE_U8, channels, 8, 0, 0.0, lum)
            out = torch.zeros(shape + (channels,), dtype=torch.uint8, device="cuda")
        stride = shape[1] * channels * out.element_size()
        pi, info = abi.PartialInfo(), abi.CodestreamInfo()
        if whole_call:
            rc = L.jxlhip_decode_codestream(dec.ctx, runner, pool, cs, n, kind, C.byref(fmt), out.data_ptr(), stride, 0, C.byref(info))
        else:
            rc = L.jxlhip_decode_codestream_partial(dec.ctx, runner, pool, cs, n, kind, C.byref(fmt), out.data_ptr(), stride, 0,
                                                    C.byref(info), C.byref(pi))
        return rc, out.cpu().numpy(), pi
    finally:
        if pool:
            R.JxlThreadParallelRunnerDestroy(pool)


@pytest.fixture(scope="module")
def dec():
    from libjxl_amd import VarDctDecoder
    d = VarDctDecoder(0)
    yield d
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("workers", [0, 6])
@pytest.mark.parametrize("key,cut", CASES)
def test_partial_file_matches_the_flushed_picture(L, dec, flushed, key, cut, workers):
    cs, n, want, expect = flushed[(key, cut)]
    rc, got, pi = _decode(L, dec, cs, n, want.shape[:2], workers=workers)
    assert rc == 0, L.jxlhip_last_error(dec.ctx)
    assert (pi.complete, pi.groups_complete, pi.groups_partial, pi.groups_dc_only, pi.have_ac_global, pi.bytes_used) == expect
    if cut in ("a", "b", "c"):
        assert pi.groups_dc_only > 0
    if cut == "c":
        assert pi.groups_dc_only < pi.num_groups  # ... beside groups that have AC
    if cut in ("a", "b"):
        assert pi.groups_dc_only == pi.num_groups and pi.have_ac_global == (cut == "b")
    if cut in ("pass0", "in_pass1"):
        assert pi.groups_partial > 0
    assert pi.complete == (cut == "e")
    assert not (got == -7.0).any()  # every sample written
    scale = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got - want).max()) / scale
    print("PARTIAL %s %dx%d cut %s (%d of %d bytes; %d/%d/%d groups) workers %d: max|diff| / scale = %.3e" % (
        key[0], key[1], key[2], cut, n, len(cs), pi.groups_complete, pi.groups_partial, pi.groups_dc_only, workers, err))
    assert err <= TIGHT


@pytest.mark.gpu
@pytest.mark.parametrize("key,cut", CASES)
def test_partial_file_as_8_bit(L, dec, flushed, key, cut):
    cs, n, want, _ = flushed[(key, cut)]
    want8 = np.round(np.clip(want, 0.0, 1.0) * 255.0)
    rc, got, pi = _decode(L, dec, cs, n, want.shape[:2], sample=abi.SAMPLE_U8)
    assert rc == 0, L.jxlhip_last_error(dec.ctx)
    err = float(np.abs(got.astype(np.float32) - want8).max())
    print("PARTIAL8 %s %dx%d cut %s: max level difference %g" % (key[0], key[1], key[2], cut, err))
    assert err <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("workers", [0, 6])
def test_partial_file_with_custom_upsampling_weights(L, dec, ref, jxl_ref, workers):
    """A 600x400 file that is NOT upsampled but carries custom upsampling weights (custom_weights_mask = 7), cut
    behind AC global and in the middle of its AC groups: the DC-only groups are drawn with the file's own 8x table
    (kernels_dc_upsample.hip), as JxlDecoderFlushImage draws them.  With the default table the picture is far off:
    the same cut of the same image coded without custom weights differs by 10 bars and more."""
    ts, RL = jxl_ref
    kw = dict(xsize=600, ysize=400, seed=5, distance=1.0)
    cs = sc.golden_stream("partial_custom")  # (= ref.feature_stream("plain", custom_weights_seed=3, **kw))
    info = abi.CodestreamInfo()
    assert L.jxlhip_codestream_basic_info(cs, len(cs), C.byref(info)) == 0 and info.upsampling == 1
    plain = ref.feature_stream("plain", **kw)
    assert len(cs) > len(plain)  # the three tables are in the image header
    s, s_plain = pr.Sections(L, cs), pr.Sections(L, plain)
    cuts, cuts_plain = _cuts(s, len(cs)), _cuts(s_plain, len(plain))
    for cut in ("b", "c"):
        n = cuts[cut]
        ok, want = pr.flush(ts, RL, cs[:n])
        assert ok and want.shape == (400, 600, 3) and not (want == pr.SENTINEL).any()
        rc, got, pi = _decode(L, dec, cs, n, (400, 600), workers=workers)
        assert rc == 0, L.jxlhip_last_error(dec.ctx)
        assert pi.groups_dc_only > 0 and (pi.groups_dc_only < pi.num_groups) == (cut == "c")
        scale = max(1.0, float(np.abs(want).max()))
        err = float(np.abs(got - want).max()) / scale
        print("PARTIAL custom weights cut %s workers %d (%d of %d groups DC only): max|diff| / scale = %.3e" % (
            cut, workers, pi.groups_dc_only, pi.num_groups, err))
        assert err <= TIGHT
        if cut == "b":  # every group DC only, in both files
            ok, other = pr.flush(ts, RL, plain[:cuts_plain[cut]])
            assert ok and float(np.abs(want - other).max()) / scale >= 10 * TIGHT


@pytest.mark.gpu
@pytest.mark.parametrize("key", pr.STREAMS)
def test_a_complete_file_is_the_single_frame_call_bit_for_bit(L, dec, flushed, key):
    cs, n, want, _ = flushed[(key, "e")]
    for sample in (abi.SAMPLE_F32, abi.SAMPLE_U8):
        rc, got, pi = _decode(L, dec, cs, n, want.shape[:2], sample=sample, workers=6)
        rc2, got2, _ = _decode(L, dec, cs, n, want.shape[:2], sample=sample, workers=6, whole_call=True)
        assert rc == 0 and rc2 == 0 and pi.complete == 1
        assert np.array_equal(got, got2)
    # ... which still refuses the file one byte short, as before
    rc, _, _ = _decode(L, dec, cs, n - 1, want.shape[:2], whole_call=True)
    assert rc == -5 and b"truncated frame" in L.jxlhip_last_error(dec.ctx)


@pytest.mark.gpu
def test_need_more_input_before_the_dc_groups_and_for_one_section(L, dec, ref, flushed):
    cs, n, want, _ = flushed[(pr.STREAMS[0], "a")]
    for m in (0, 1, 40, n // 2, n - 1):
        rc, got, _ = _decode(L, dec, cs, m, want.shape[:2])
        assert rc == NEED_MORE_INPUT, (m, rc)
        assert b"incomplete" in L.jxlhip_last_error(dec.ctx)
    one = pr.stream(ref, pr.ONE_SECTION)
    rc, _, _ = _decode(L, dec, one, len(one) - 1, (13, 200))
    assert rc == NEED_MORE_INPUT
    rc, _, pi = _decode(L, dec, one, len(one), (13, 200))
    assert rc == 0 and pi.complete == 1
    # the context is usable afterwards
    rc, got, _ = _decode(L, dec, cs, n, want.shape[:2])
    assert rc == 0 and float(np.abs(got - want).max()) <= TIGHT * max(1.0, float(np.abs(want).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("orientation", [6])
def test_display_orientation_of_a_partial_file(L, dec, ref, jxl_ref, orientation, monkeypatch):
    """A coded-orientation stream (ImageMetadata::orientation = 6) cut behind half its AC groups, with
    JXLHIP_OUT_UNDO_ORIENTATION: the flushed picture comes out turned, like JxlDecoder's."""
    ts, RL = jxl_ref
    monkeypatch.setenv("JXR_ORIENTATION", str(orientation))
    rs = ref.RealStream(seed=12, xsize=456, ysize=280, distance=1.0, speed_tier=3)
    monkeypatch.delenv("JXR_ORIENTATION")
    cs = rs.codestream.tobytes()
    info = abi.CodestreamInfo()
    assert L.jxlhip_codestream_basic_info(cs, len(cs), C.byref(info)) == 0 and info.orientation == orientation
    s = pr.Sections(L, cs)
    assert s.ng == 4 and s.np == 1
    n = sorted(s.end(s.ac(0, g)) for g in range(4))[1]  # two of the four groups
    ok, want = pr.flush(ts, RL, cs[:n])
    assert ok and want.shape == (456, 280, 3) and not (want == pr.SENTINEL).any()
    tf = {13: abi.TF_SRGB, 8: abi.TF_LINEAR}[info.transfer_function]
    rc, got, pi = _decode(L, dec, cs, n, (456, 280), kind=2 | UNDO, tf=tf, workers=6)
    assert rc == 0, L.jxlhip_last_error(dec.ctx)
    assert (pi.groups_complete, pi.groups_dc_only) == (2, 2)
    err = float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max()))
    print("PARTIAL orientation %d: max|diff| / scale = %.3e" % (orientation, err))
    assert err <= TIGHT


@pytest.mark.gpu
def test_refusals_by_name(L, dec, ref):
    def refused(cs, n, shape, why, channels=3, sample=abi.SAMPLE_F32):
        rc, _, _ = _decode(L, dec, cs, n, shape, sample=sample, channels=channels)
        assert rc == -7, (why, rc, L.jxlhip_last_error(dec.ctx))
        assert why.encode() in L.jxlhip_last_error(dec.ctx), (why, L.jxlhip_last_error(dec.ctx))

    # a frame with a render stage the partial path does not draw, one byte short of its end
    for feature, why in (("noise", "a partial file of a frame with noise"), ("splines", "a partial file of a frame with splines"),
                         ("patches", "a partial file of a frame with patches")):
        cs = ref.feature_stream(feature, xsize=600, ysize=400, seed=5, distance=1.0)
        refused(cs, len(cs) - 1, (400, 600), why)
        # ... and whole it is what the single-frame call makes of it
        rc, got, pi = _decode(L, dec, cs, len(cs), (400, 600))
        rc2, got2, _ = _decode(L, dec, cs, len(cs), (400, 600), whole_call=True)
        assert rc == 0 and rc2 == 0 and pi.complete and np.array_equal(got, got2)
    cs = ref.feature_stream("plain", xsize=600, ysize=400, seed=5, distance=12)
    refused(cs, len(cs) - 1, (400, 600), "a partial file of an upsampled frame")
    # files the single-frame call refuses, with its reason
    cs = ref.feature_stream("animation", xsize=600, ysize=400, seed=5, distance=1.0)
    rc, _, _ = _decode(L, dec, cs, len(cs), (400, 600), whole_call=True)
    assert rc == -7
    why = L.jxlhip_last_error(dec.ctx)
    rc, _, _ = _decode(L, dec, cs, len(cs), (400, 600))
    assert rc == -7 and L.jxlhip_last_error(dec.ctx) == why
    cs = ref.feature_stream("modular", xsize=600, ysize=400, seed=5, distance=1.0)
    rc, _, _ = _decode(L, dec, cs, len(cs) - 1, (400, 600))
    assert rc == -7
    # an image with an alpha channel: three channels are fine (the channel's bytes are skipped), four are not
    rs = ref.RealStream(xsize=520, ysize=300, alpha_bits=8, original="srgb8")
    cs = rs.codestream.tobytes()
    refused(cs, len(cs) - 1, (300, 520), "a partial file of an image with extra channels into a 4-channel output", channels=4,
            sample=abi.SAMPLE_U8)
    rc, got, pi = _decode(L, dec, cs, len(cs) - 1, (300, 520), sample=abi.SAMPLE_U8)
    assert rc == 0 and not pi.complete, L.jxlhip_last_error(dec.ctx)
    rc2, whole, _ = _decode(L, dec, cs, len(cs), (300, 520), sample=abi.SAMPLE_U8)
    assert rc2 == 0
    full = pi.groups_complete and np.abs(got.astype(int) - whole.astype(int))
    # the groups that were complete are the whole file's away from the others (the last group is the one cut)
    assert pi.groups_complete + pi.groups_partial + pi.groups_dc_only == pi.num_groups and pi.groups_complete >= 1
    assert int(full[:200, :200].max()) == 0
    # bad arguments
    assert L.jxlhip_decode_codestream_partial(dec.ctx, None, None, cs, len(cs), 2, None, 1, 0, 0, None, None) == -1


@pytest.mark.gpu
def test_djxl_hip_allow_partial_files(flushed, tmp_path):
    """tools/djxl_hip.py --allow_partial_files on the plain 600x400 file cut in the middle of its AC groups: the
    flushed picture as .ppm within one level, and the three group counts on its standard output."""
    import os
    import subprocess
    import sys
    key = pr.STREAMS[0]
    cs, n, want, expect = flushed[(key, "c")]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, dst = tmp_path / "cut.jxl", tmp_path / "cut.ppm"
    src.write_bytes(cs[:n])
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "djxl_hip.py"), str(src), str(dst), "--allow_partial_files",
                        "--threads", "4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "partial file: %d group(s) complete, %d partial, %d DC only" % expect[1:4] in r.stdout, r.stdout
    raw = dst.read_bytes()
    px = np.frombuffer(raw[len(raw) - 600 * 400 * 3:], np.uint8).reshape(400, 600, 3).astype(np.int32)
    want8 = np.clip(np.rint(want * 255.0), 0, 255).astype(np.int32)
    assert int(np.abs(px - want8).max()) <= 1
