"""The host front-end of lossless files with extra channels and of grey lossless files
(jxlhip_modular_image_decode_channels, libjxl_amd/csrc/modular_image.inc) against the reference decoder, without a device.

Streams: the genuine files of tests/golden/lossless_channels/, written by the reference's two lossless encoders (the
effort-1 encoder enc_fast_lossless.cc: e1_*; the full encoder at its default effort: e7_*); manifest.json says what each is
and records the counters the front-end reports for it.  What the encoders turned out to write: the effort-1 encoder puts
its YCoCg into the GLOBAL list (global_rct = 6, every group's list empty), and the full encoder gives an image of one group
a global RCT too -- so one file, e7_rgba8_g128_300x270 (the full encoder with 128-pixel groups,
`cjxl -d 0 --modular_group_size=0`), is there to keep per-GROUP programs beside an alpha plane: 9 groups, type 6 each.
e7_rgba8_2ec_140x90 says modular_16_bit_buffer_sufficient while its 16-bit depth channel does not fit: the int16 decode is
JXLHIP_ERR_RANGE and the int32 one is taken, as the whole-file call does.

For every file: every plane the entry returns -- the colour planes through the numpy model of the device stage
(tests/lossless_channels_model.py), each extra channel as it is -- must EQUAL round(reference float x (2^bits - 1)) of the
reference's JxlDecoder, with no runner and with six workers, in int16 and int32 planes.  Then the conditions on the inputs,
the refusals by name, truncation, and jxlhip_codestream_basic_info."""
import ctypes as C

import numpy as np
import pytest

import lossless_channels_model as lm
from libjxl_amd import abi
from test_modular_front_end import sections_end
from test_seam import hip_runner, jxl_decode, libs, load, ref  # noqa: F401  (fixtures)

FILES = sorted(lm.manifest())


@pytest.fixture(scope="module")
def L():
    return abi.load_library()


@pytest.fixture(scope="module")
def wanted(libs):
    """Per file: the reference's integers -- colour [H, W, 3] and one [H, W] per extra channel -- and its 4-channel floats."""
    RL = load(libs[0])
    out = {}
    for name, m in lm.manifest().items():
        cs = lm.fixture(name)
        px = jxl_decode(RL, cs, channels=4)
        assert px.shape == (m["ysize"], m["xsize"], 4)
        colour = np.rint(px[..., :3].astype(np.float64) * ((1 << m["bits"]) - 1)).astype(np.int32)
        extras = []
        for e, bits in enumerate(m["extra_bits"]):
            _, plane = jxl_decode(RL, cs, channels=4, extra_channel=e)
            extras.append((np.rint(plane.astype(np.float64) * ((1 << bits) - 1)).astype(np.int32), plane))
        out[name] = (colour, extras, px)
    return out


def check(o, m, want, name):
    colour, extras, _ = want
    s = lm.samples(list(o["planes"]), o["fh"].group_dim, o["group_rct"], o["global_rct"])
    assert len(s) == (1 if m["channels"][0] == "grey" else 3)
    if len(s) == 1:
        s = s * 3
    assert np.array_equal(np.stack(s, -1), colour), name
    assert len(o["extras"]) == len(extras) == len(m["extra_bits"])
    for e, (ints, _) in enumerate(extras):
        assert np.array_equal(o["extras"][e].astype(np.int32), ints), (name, e)
    assert (o["padding"] == -12345).all() and o["end_bit"] == 8 * len(lm.fixture(name))
    assert o["groups_on_device"] == int((o["group_rct"] != 0).sum())
    got = {k: int(o[k]) for k in ("groups_on_device", "groups_on_host", "global_on_host", "global_rct")}
    assert got == {k: m[k] for k in got}, name  # (the manifest's record)


@pytest.mark.parametrize("name", FILES)
def test_every_plane_equals_the_reference_decoder(L, wanted, name):
    m, cs = lm.manifest()[name], lm.fixture(name)
    R, runner, pool = hip_runner()  # six workers
    try:
        first = None
        for kw in (dict(), dict(runner=runner, runner_opaque=pool)):
            rc, why, a = lm.host_decode(L, abi, cs, sample_type=abi.MODULAR_I16, **kw)
            assert rc == (0 if m["int16"] else -8), (name, rc, why)  # JXLHIP_ERR_RANGE: a plane that does not fit 16 bits
            if rc == 0:
                assert a["planes"].dtype == np.int16
                check(a, m, wanted[name], name)
            rc, why, b = lm.host_decode(L, abi, cs, sample_type=abi.MODULAR_I32, **kw)
            assert rc == 0 and b["planes"].dtype == np.int32, (name, rc, why)
            check(b, m, wanted[name], name)
            if m["int16"]:
                assert np.array_equal(a["planes"], b["planes"]) and np.array_equal(a["extras"], b["extras"])
            first = first or b
            assert np.array_equal(first["planes"], b["planes"]) and np.array_equal(first["group_rct"], b["group_rct"])
    finally:
        R.JxlThreadParallelRunnerDestroy(pool)


def test_the_files_cover_what_they_are_there_for():
    man = lm.manifest()
    alpha = {n: m for n, m in man.items() if "alpha" in m["channels"]}
    # a group program left for the device on an image with alpha; a global one too
    assert any(m["groups_on_device"] >= 1 and m["channels"][:3] == ["r", "g", "b"] for m in alpha.values())
    assert any(m["global_rct"] != 0 for m in alpha.values())
    # the collecting path (a global list the host undoes once every group is in) with four channels and more
    assert any(m["global_on_host"] and len(m["channels"]) == 4 for m in man.values())
    assert any(m["global_on_host"] and len(m["channels"]) == 5 for m in man.values())
    # grey with and without alpha; int32 planes; both encoders; more than one group; per-channel bit depths
    assert any(m["channels"] == ["grey"] for m in man.values()) and any(m["channels"] == ["grey", "alpha"] for m in man.values())
    assert any(not m["int16"] for m in man.values())
    assert {m["encoder"] for m in man.values()} == {"fast_lossless", "full"}
    assert any(m["extra_bits"] == [8, 16] and m["bits"] == 8 for m in man.values())
    assert all(m["bytes"] <= 165274 for m in man.values())  # (no file larger than the largest tests/golden/ held before)


def test_the_numpy_model_gives_the_reference_floats(L, wanted):
    """tests/lossless_channels_model.py held to JxlDecoder's 4-channel float output, bit for bit, on every file."""
    for name, m in lm.manifest().items():
        rc, _, o = lm.host_decode(L, abi, lm.fixture(name), sample_type=abi.MODULAR_I32)
        assert rc == 0
        ai = lm.alpha_index(o)
        got = lm.emit_rgba_f32(list(o["planes"]), m["bits"], None if ai is None else o["extras"][ai],
                               0 if ai is None else m["extra_bits"][ai], o["fh"].group_dim, o["group_rct"], o["global_rct"])
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), wanted[name][2].view(np.uint32)), name
        for e, (_, plane) in enumerate(wanted[name][1]):  # the other extra channels: the same multiply
            mine = o["extras"][e].astype(np.float32) * np.float32(1.0 / ((1 << m["extra_bits"][e]) - 1))
            assert np.array_equal(mine.view(np.uint32), plane.view(np.uint32)), (name, e)


def test_refusals_by_name(L):
    cs = lm.fixture("e7_rgba8_2ec_140x90")

    def refused(edit, **kw):
        rc, why, _ = lm.host_decode(L, abi, cs, sample_type=abi.MODULAR_I32, fh_edit=edit, **kw)
        assert rc == -7, rc
        return why

    def set_to(**changes):
        def edit(fh):
            for k, v in changes.items():
                if isinstance(v, tuple):
                    getattr(fh, k)[v[0]] = v[1]
                else:
                    setattr(fh, k, v)
        return edit

    assert "sub-sampled extra channel" in refused(set_to(ec_upsampling=(1, 2)))  # (dim_shift != 0 in the image header)
    assert "more than four extra channels" in refused(set_to(num_extra_channels=5), num_extra=4)
    assert "extra-channel blend mode" in refused(set_to(ec_blend_mode=(0, abi.BLEND_BLEND), ec_blend_any=1))
    assert "colour blend mode" in refused(set_to(blend_mode=abi.BLEND_ADD))
    assert "XYB" in refused(set_to(color_transform=0)) and "upsampled" in refused(set_to(upsampling=2))
    # the three-plane entry keeps refusing an image with extra channels, by name
    rc, ih, extra, fh, pos = lm.headers(L, abi, cs)
    assert rc == 0 and fh.num_extra_channels == 2
    planes, rct, pl = np.zeros((3, 90, 140), np.int32), np.zeros(int(fh.num_groups), np.uint16), abi.ModularImagePlanes()
    for c in range(3):
        pl.planes[c] = planes[c].ctypes.data
    pl.stride_samples, pl.sample_type, pl.group_rct = 140, abi.MODULAR_I32, rct.ctypes.data
    why, p = C.c_char_p(), C.c_size_t(pos)
    assert L.jxlhip_modular_image_decode(cs, len(cs), C.byref(p), C.byref(fh), None, None, C.byref(pl), C.byref(why)) == -7
    assert b"extra channels" in why.value
    fh.num_extra_channels = 1
    assert L.jxlhip_modular_image_decode(cs, len(cs), C.byref(p), C.byref(fh), None, None, C.byref(pl), C.byref(why)) == -7
    assert b"extra channels" in why.value
    # bad arguments of the new entry: the channel counts must be the frame's, every plane there, the depths 1..16
    for kw in (dict(num_extra=1),):
        rc, _, _ = lm.host_decode(L, abi, cs, sample_type=abi.MODULAR_I32, **kw)
        assert rc == -1


def test_the_whole_file_calls_name_the_image_level_cases(L):
    """dim_shift != 0, float or deep extra channels and a fifth extra channel sit in the IMAGE header, which only the
    whole-file calls read: jxlhip_codestream_basic_info takes every fixture and still declines by status what it cannot
    name without a context (tests/test_gpu_lossless_channels.py reads the names through jxlhip_last_error)."""
    for name, m in lm.manifest().items():
        cs = lm.fixture(name)
        info = abi.CodestreamInfo()
        assert L.jxlhip_codestream_basic_info(cs, len(cs), C.byref(info)) == 0, name
        assert info.modular == 1 and (info.xsize, info.ysize) == (m["xsize"], m["ysize"])
        assert info.grey == (m["channels"][0] == "grey") and info.bits_per_sample == m["bits"]
        assert info.num_extra_channels == len(m["extra_bits"])
        assert info.alpha_bits == (m["extra_bits"][0] if "alpha" in m["channels"] else 0) and info.alpha_premultiplied == 0
        seq = abi.SequenceInfo()
        assert L.jxlhip_codestream_sequence_info(cs, len(cs), C.byref(info), C.byref(seq)) == -7
        part = abi.PartialInfo()
        assert L.jxlhip_codestream_partial_info(cs, len(cs), C.byref(info), C.byref(part)) == -7


def test_truncation_at_every_section_boundary_is_a_bad_stream(L):
    for name in ("e1_rgba8_300x270", "e7_rgba8_g128_300x270"):
        cs = lm.fixture(name)
        rc, ih, extra, fh, pos = lm.headers(L, abi, cs)
        assert rc == 0
        ends = sections_end(L, cs, pos, fh)
        assert ends[-1] == len(cs) and len(ends) == fh.num_toc_entries > 1
        for end in ends:
            rc, _, _ = lm.host_decode(L, abi, cs[:end - 1])
            assert rc == -5, (name, end, rc)
        rc, _, _ = lm.host_decode(L, abi, cs + b"\0" * 3)  # (bytes behind the frame are not the frame's)
        assert rc == 0


def test_damaged_files_under_asan_ubsan(tmp_path):
    """tests/fuzz/fuzz_modular_channels.cc: the host sources compiled with g++ -fsanitize=address,undefined into a program
    of their own, which sends damaged copies of the files through jxlhip_modular_image_decode_channels.  Every byte of the
    two smallest files is complemented in turn; of the others every stride-th byte, the strides primes so that the positions
    fall into every section at varying depths; every bit of each file's first 64 bytes is flipped.  The runs must end clean."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "fuzz_modular_channels")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-DJXLHIP_NO_DEVICE", os.path.join(root, "tests", "fuzz", "fuzz_modular_channels.cc"),
           os.path.join(root, "libjxl_amd", "csrc", "entropy.cc"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for stride, names in ((1, ["e1_rgba8_palette_130x70", "e7_rgba8_1x1"]), (53, ["e1_greya16_70x50"]), (211, ["e7_rgba8_2ec_140x90"]),
                          (1009, ["e7_rgba8_g128_300x270"]), (173, ["e7_grey8_129x257"])):
        paths = [os.path.join(lm.GOLDEN, n + ".jxl") for n in names]
        r = subprocess.run([out, str(stride)] + paths, capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, (names, r.stdout[-500:], r.stderr[-4000:])
        ok, rejected = map(int, r.stdout.split())
        total = sum(-(-os.path.getsize(p) // stride) + min(512, 8 * os.path.getsize(p)) for p in paths)
        assert ok + rejected == total and rejected > total // 4 and ok > 0, (names, ok, rejected)
