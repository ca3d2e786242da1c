"""Lossless files with an alpha channel and grey lossless files on the device: k_modular_planes alone
(jxlhip_decode_modular_channels) against the numpy model (tests/lossless_channels_model.py) on planted planes, and the
genuine files of tests/golden/lossless_channels/ through jxlhip_decode_codestream against the reference's JxlDecoder.

Kernel alone.  Frames of 1x1, 7x3, 8x1, 9x2 (the scalar tail alone, one whole run, a run and its tail), 129x130 in
128-pixel groups (a group seam in both directions), 2049x2 (the block seam at 2048 columns) and 9x1025 (a second turn of
the row loop behind the 1024-row grid cap), each with int16 and int32 planes and as grey, grey + alpha and RGB + alpha;
all four group dimensions; two-RCT group and global programs beside an alpha plane; padded plane rows; canaries behind
every output row and behind the buffer.  4-channel float output is bit-equal to the model; 8-bit output of 8-bit samples
(the dither cannot decide anything) equals the integers, through the fixed RGB8 / RGBA8 tails (rows at 4-byte aligned
addresses) and through the general tail (a row base at an odd address); u16, f16, dithered 8-bit output of deeper samples,
big-endian and 3-channel outputs equal oracle.pack_output of the model's samples with the identity transfer byte for byte.
Alpha takes any value of ITS depth: 8-bit alpha beside 16-bit colour (12-bit in int16 planes) and the reverse.  The alpha
column of the yardstick: pack_output packs three colour channels, and alpha is packed like a colour channel minus the
transfer function, which is the identity here -- so it is pack_output's channel 0 of an image that holds the alpha
samples, moved by (5, 7) pixels for 8-bit samples because channel c reads the 32x32 dither table at (x + 23c, y + 13c)
(stage_write.cc:263-284) and 69 = 5, 39 = 7 mod 32.

Whole files: every fixture with 0 and 6 workers; 4-channel float bit-equal to JxlDecoder (both sides do one float32
multiply per sample); RGBA8 of the 8-bit files equal to round(255 x) and 16-bit RGBA of the 16-bit file equal to
round(65535 x) (its 8-bit output is dithered: the kernel tests hold that to the yardstick); the extra-channel planes of
e7_rgba8_2ec_140x90; three files back to back on one context; tools/djxl_hip.py.  On the parent commit the RGBA and
grey files are refused (-7) at the image header and the RGB control decodes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lossless_channels_model as lm
import output_sweep as S
from libjxl_amd import VarDctDecoder, abi
from test_gpu_modular import coded_planes, decode_file, linear, programs
from test_seam import hip_runner, jxl_decode, libs, load, ref  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5
SIZES = [(1, 1), (7, 3), (8, 1), (9, 2), (129, 130), (2049, 2), (9, 1025)]
KINDS = ["grey", "grey_alpha", "rgb_alpha"]
SSZ = {0: 4, 1: 1, 2: 2, 3: 2}


@pytest.fixture(scope="module")
def dec():
    d = VarDctDecoder(0)
    yield d
    d.close()


def emit(dec, colour, bits, alpha, alpha_bits, gd, group_rct, global_rct, kind, f=None, orient=0, in_pad=0, out_pad=24, base_off=0,
         expect=0, num_color=None):
    """jxlhip_decode_modular_channels on [nc, H, W] colour planes and an [H, W] alpha plane (or None); returns the
    [H', W', channels] output after checking the canaries in front of the buffer, behind every row and behind the buffer."""
    L = dec.L
    nc, h, w = colour.shape
    fill = 0x55AA if colour.dtype == np.int32 else 0x55A
    host = np.full((nc + 1, h, w + in_pad), fill, colour.dtype)
    host[:nc, :, :w] = colour
    m = abi.ModularChannels()
    m.xsize, m.ysize, m.num_color = w, h, nc if num_color is None else num_color
    for c in range(nc):
        m.planes[c] = host[c].ctypes.data
    if alpha is not None:
        host[nc, :, :w] = alpha
        m.alpha_plane, m.alpha_bits = host[nc].ctypes.data, alpha_bits
    m.stride_samples = w + in_pad
    m.sample_type = abi.MODULAR_I16 if colour.dtype == np.int16 else abi.MODULAR_I32
    m.bits_per_sample, m.group_dim = bits, gd
    rct = None if group_rct is None else np.ascontiguousarray(group_rct, np.uint16)
    m.group_rct = None if rct is None else rct.ctypes.data
    m.global_rct = int(global_rct)
    of = None
    if f is not None:
        of = abi.OutputFormat(f["transfer"], f["sample_type"], f["num_channels"], f["bits_per_sample"], f["swap_endianness"],
                              f["tf_param"], f["luminances"])
    ssz = 4 if kind == 1 else SSZ[f["sample_type"]]
    bpp = 12 if kind == 1 else f["num_channels"] * ssz
    ow, oh = (h, w) if orient >= 5 else (w, h)
    stride = ow * bpp + out_pad
    stride += -stride % ssz
    head, tail = 256 + base_off, 256
    assert base_off % ssz == 0
    buf = torch.full((head + oh * stride + tail,), SENTINEL, dtype=torch.uint8, device="cuda")
    rc = L.jxlhip_decode_modular_channels(dec.ctx, C.byref(m), kind, C.byref(of) if of else None, buf.data_ptr() + head, stride, orient)
    assert rc == expect, (rc, L.jxlhip_last_error(dec.ctx))
    assert L.jxlhip_sync(dec.ctx) == 0
    raw = buf.cpu().numpy()
    if expect:
        assert (raw == SENTINEL).all()
        return None
    assert (raw[:head] == SENTINEL).all() and (raw[head + oh * stride:] == SENTINEL).all(), "bytes outside the buffer touched"
    rows = raw[head:head + oh * stride].reshape(oh, stride)
    S.check_padding(rows, ow * bpp, SENTINEL)
    dt = np.float32 if kind == 1 else {0: np.float32, 1: np.uint8, 2: np.uint16, 3: np.uint16}[f["sample_type"]]
    return np.ascontiguousarray(rows[:, :ow * bpp]).view(dt).reshape(oh, ow, 3 if kind == 1 else f["num_channels"])


def yardstick(oracle, f, rgba):
    """oracle.pack_output with the identity transfer for the colour, and for a fourth channel the alpha column (see the
    module's text).  rgba: the model's [H, W, 4] float32 samples."""
    f = linear(f)
    out = oracle.pack_output(f, np.ascontiguousarray(rgba[..., :3]))
    if f["num_channels"] == 4:
        h, w = rgba.shape[:2]
        dx, dy = (5, 7) if f["sample_type"] == abi.SAMPLE_U8 else (0, 0)
        moved = np.zeros((h + dy, w + dx, 3), np.float32)
        moved[dy:, dx:, 0] = rgba[..., 3]
        out[..., 3] = oracle.pack_output(dict(f, num_channels=3), moved)[dy:, dx:, 0]
    return out


def same_bytes(a, b):
    """Every byte equal (byte-swapped floats are NaNs as often as not: no float comparison)."""
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def planted(kind, w, h, gd, dtype, rng, bits=8, alpha_bits=8, two=False, global_rct=0):
    """Planes as an encoder would have left them, the programs (none for a grey frame), and the model's [H, W, 4]
    float32 samples."""
    nc = 1 if kind.startswith("grey") else 3
    global_rct = global_rct if nc == 3 else 0
    img = rng.integers(0, 1 << bits, (nc, h, w))
    img[:, : h // 2 + 1, : w // 3 + 1] = rng.integers(0, 2, (nc, 1, 1)) * ((1 << bits) - 1)  # (a flat corner: both ends)
    alpha = None
    if kind.endswith("alpha"):
        alpha = rng.integers(0, 1 << alpha_bits, (h, w))
        alpha[: h // 3 + 1] = 0  # fully transparent, fully opaque, and everything between
        alpha[h // 3 + 1: 2 * h // 3 + 1, : w // 2 + 1] = (1 << alpha_bits) - 1
        alpha = alpha.astype(dtype)
    if nc == 3:
        group_rct = programs(w, h, gd, rng, two=two)
        planes = coded_planes(img, gd, group_rct, global_rct, dtype)
    else:
        group_rct, planes = None, img.astype(dtype)
    want = lm.emit_rgba_f32(list(planes), bits, alpha, alpha_bits, gd, group_rct, global_rct)
    ints = np.rint(want[..., :3].astype(np.float64) * ((1 << bits) - 1)).astype(np.int64)
    assert np.array_equal(ints, np.broadcast_to(img, (3, h, w)).transpose(1, 2, 0))  # (the model undoes what was done)
    return planes, alpha, group_rct, global_rct, want


def check_8bit_case(oracle, dec, kind, w, h, gd, dtype, rng, in_pad, two=False, global_rct=0):
    planes, alpha, group_rct, global_rct, want = planted(kind, w, h, gd, dtype, rng, two=two, global_rct=global_rct)
    args = (dec, planes, 8, alpha, 8, gd, group_rct, global_rct)
    got = emit(*args, 2, S.fmt(abi.TF_SRGB, abi.SAMPLE_F32, 4), in_pad=in_pad)  # (the transfer function is not read)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (kind, dtype, np.argwhere(got != want)[:3])
    ints = np.rint(want.astype(np.float64) * 255).astype(np.uint8)
    for nch in (4, 3):
        f = S.fmt(abi.TF_SRGB, abi.SAMPLE_U8, nch)
        # rows at 4-byte aligned addresses -- the fixed tails store a run as 32 / 24 contiguous bytes -- and a row base
        # and stride at odd addresses: the general tail
        for out_pad, base_off in ((24 + -(w * nch) % 4, 0), (7 + (w * nch) % 2, 1)):
            got = emit(*args, 2, f, in_pad=in_pad, out_pad=out_pad, base_off=base_off)
            assert np.array_equal(got, ints[..., :nch]), (kind, dtype, nch, base_off)
            assert same_bytes(got, yardstick(oracle, f, want))
    got = emit(*args, 1, in_pad=in_pad)  # three floats: a grey sample three times; alpha has no room there
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want[..., :3]).view(np.uint32))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_kernel_is_bit_equal_to_the_model(oracle, dec, size, kind):
    w, h = size
    gd = 128 if size == (129, 130) else 256
    rng = np.random.default_rng(w * 1000 + h + len(kind))
    for dtype, in_pad in ((np.int16, 0), (np.int32, 5), (np.int16, 3)):
        check_8bit_case(oracle, dec, kind, w, h, gd, dtype, rng, in_pad)


@pytest.mark.parametrize("gd", [128, 256, 512, 1024])
def test_kernel_group_dimensions_and_two_rct_programs(oracle, dec, gd):
    """RGB + alpha with a program of two RCTs in every group and a global program of two on top, in every group size."""
    rng = np.random.default_rng(gd)
    for dtype in (np.int16, np.int32):
        check_8bit_case(oracle, dec, "rgb_alpha", 257, 130, gd, dtype, rng, 0, two=True, global_rct=6 | (9 << 8))
    check_8bit_case(oracle, dec, "grey_alpha", 257, 130, gd, np.int16, rng, 0)


FORMATS = [S.fmt(abi.TF_SRGB, abi.SAMPLE_U8, 4), S.fmt(abi.TF_PQ, abi.SAMPLE_U8, 3, par=1000.0), S.fmt(abi.TF_SRGB, abi.SAMPLE_U8, 4, bits=5),
           S.fmt(abi.TF_SRGB, abi.SAMPLE_U16, 4), S.fmt(abi.TF_709, abi.SAMPLE_U16, 4, swap=1), S.fmt(abi.TF_SRGB, abi.SAMPLE_U16, 3, bits=10),
           S.fmt(abi.TF_SRGB, abi.SAMPLE_F16, 4), S.fmt(abi.TF_HLG, abi.SAMPLE_F16, 4, swap=1, par=1000.0),
           S.fmt(abi.TF_SRGB, abi.SAMPLE_F32, 4, swap=1), S.fmt(abi.TF_LINEAR, abi.SAMPLE_F32, 3)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("depths", [(8, "deep"), ("deep", 8), ("deep", "deep"), (10, 10)], ids=str)
def test_kernel_depths_and_every_sample_type(oracle, dec, kind, depths):
    """Colour and alpha depths of their own -- `deep` is 16 bits in int32 planes and 12 in int16 planes, which hold no
    more -- into every sample type, 3 and 4 channels, both endiannesses: the yardstick, every byte equal."""
    w, h, gd = 129, 130, 128
    for dtype, deep in ((np.int16, 12), (np.int32, 16)):
        bits, alpha_bits = (deep if d == "deep" else d for d in depths)
        rng = np.random.default_rng(bits * 100 + alpha_bits + len(kind))
        # (two RCTs and a global one widen 12-bit samples past int16: the int16 planes carry one RCT per group)
        planes, alpha, group_rct, global_rct, want = planted(kind, w, h, gd, dtype, rng, bits, alpha_bits, two=dtype == np.int32, global_rct=1)
        for f in FORMATS:
            got = emit(dec, planes, bits, alpha, alpha_bits, gd, group_rct, global_rct, 2, f)
            assert same_bytes(got, yardstick(oracle, f, want)), (kind, dtype, depths, S.fmt_id(f))
            if alpha is not None and f["num_channels"] == 4 and f["sample_type"] == abi.SAMPLE_U16 and f["bits_per_sample"] == alpha_bits \
                    and not f["swap_endianness"]:
                assert np.array_equal(got[..., 3], alpha)  # (a 16-bit sample of an alpha of as many bits: the integer)


@pytest.mark.parametrize("o", [5, 8])
def test_kernel_orientations(oracle, dec, o):
    """undo_orientation through the staging frame and k_orient; the 8-bit dither follows the flipped coordinates."""
    w, h, gd = 257, 130, 256
    rng = np.random.default_rng(o)
    planes, alpha, group_rct, _, want = planted("rgb_alpha", w, h, gd, np.int16, rng, 10, 8)
    fx, fy = o in (2, 3, 7, 8), o in (3, 4, 6, 7)
    flipped = want[:, ::-1] if fx else want
    flipped = np.ascontiguousarray(flipped[::-1] if fy else flipped)
    for f in (S.fmt(abi.TF_SRGB, abi.SAMPLE_F32, 4), S.fmt(abi.TF_SRGB, abi.SAMPLE_U8, 4), S.fmt(abi.TF_SRGB, abi.SAMPLE_U16, 4)):
        got = emit(dec, planes, 10, alpha, 8, gd, group_rct, 0, 2, f, orient=o)
        assert same_bytes(got, np.ascontiguousarray(yardstick(oracle, f, flipped).swapaxes(0, 1))), (o, S.fmt_id(f))


def test_kernel_refusals(dec):
    grey, alpha = np.zeros((1, 9, 17), np.int16), np.zeros((9, 17), np.int16)
    f = S.fmt(abi.TF_SRGB, abi.SAMPLE_U8, 4)
    emit(dec, grey, 8, alpha, 8, 128, np.array([6], np.uint16), 0, 2, f, expect=-1)  # an RCT on one plane
    assert b"grey" in dec.L.jxlhip_last_error(dec.ctx)
    emit(dec, grey, 8, alpha, 8, 128, None, 6, 2, f, expect=-1)
    emit(dec, grey, 8, alpha, 0, 128, None, 0, 2, f, expect=-1)  # alpha depths outside 1..16
    emit(dec, grey, 8, alpha, 17, 128, None, 0, 2, f, expect=-1)
    emit(dec, grey, 8, alpha, 8, 128, None, 0, 2, f, num_color=2, expect=-1)
    emit(dec, grey, 8, alpha, 8, 128, None, 0, 0, f, expect=-7)  # planar XYB


# ---- whole files -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def files(libs):
    """name -> (codestream, manifest entry, the reference JxlDecoder's 4-channel float pixels), decoded once."""
    RL = load(libs[0])
    return {name: (lm.fixture(name), m, jxl_decode(RL, lm.fixture(name), channels=4)) for name, m in lm.manifest().items()}


def check_file(dec, name, cs, m, want, runner=None, pool=None):
    shape = want.shape[:2]
    got, info = decode_file(dec, cs, S.fmt(abi.TF_SRGB, abi.SAMPLE_F32, 4), shape, runner, pool)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
    assert info.modular == 1 and info.num_extra_channels == len(m["extra_bits"]) and info.grey == (m["channels"][0] == "grey")
    if "alpha" not in m["channels"]:
        assert (want[..., 3] == 1.0).all()
    if m["bits"] == 8 and (m["extra_bits"] or [8])[0] == 8:
        got8, _ = decode_file(dec, cs, S.fmt(abi.TF_SRGB, abi.SAMPLE_U8, 4), shape, runner, pool)
        assert np.array_equal(got8, np.rint(want.astype(np.float64) * 255).astype(np.uint8)), name
        got8, _ = decode_file(dec, cs, S.fmt(abi.TF_SRGB, abi.SAMPLE_U8, 3), shape, runner, pool)
        assert np.array_equal(got8, np.rint(want[..., :3].astype(np.float64) * 255).astype(np.uint8)), name
    else:
        got16, _ = decode_file(dec, cs, S.fmt(abi.TF_SRGB, abi.SAMPLE_U16, 4), shape, runner, pool)
        assert np.array_equal(got16.view(np.uint16), np.rint(want.astype(np.float64) * 65535).astype(np.uint16)), name


@pytest.mark.parametrize("workers", [0, 6])
def test_whole_files_equal_the_reference_decoder(dec, files, workers):
    R, runner, pool = hip_runner() if workers else (None, None, None)
    try:
        for name, (cs, m, want) in files.items():
            check_file(dec, name, cs, m, want, runner, pool)
    finally:
        if pool:
            R.JxlThreadParallelRunnerDestroy(pool)


@pytest.mark.parametrize("name", ["e1_rgba8_300x270", "e1_grey8_261x131", "e1_rgb8_300x270"])
def test_files_the_parent_refused_and_the_control(dec, files, name):
    """RGBA and grey lossless files were JXLHIP_ERR_UNSUPPORTED (-7) at the image header before this path took them; the
    RGB control decodes before and after."""
    check_file(dec, name, *files[name])


def test_extra_channel_planes_of_a_lossless_file(dec, libs):
    name = "e7_rgba8_2ec_140x90"
    cs, RL = lm.fixture(name), load(libs[0])
    want = [jxl_decode(RL, cs, channels=4, extra_channel=e) for e in (0, 1)]
    h, w = want[0][0].shape[:2]
    f = S.fmt(abi.TF_SRGB, abi.SAMPLE_F32, 4)
    of = abi.OutputFormat(f["transfer"], f["sample_type"], f["num_channels"], f["bits_per_sample"], f["swap_endianness"], f["tf_param"],
                          f["luminances"])
    out = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    stride = w + 3
    planes = np.full((2, h, stride), -7.0, np.float32)
    ptrs = (C.c_void_p * 2)(planes[0].ctypes.data, planes[1].ctypes.data)
    info = abi.CodestreamInfo()
    rc = dec.L.jxlhip_decode_codestream_extra(dec.ctx, None, None, cs, len(cs), 2, C.byref(of), out.data_ptr(), w * 16, 0, ptrs, 2, stride,
                                              C.byref(info))
    assert rc == 0, dec.L.jxlhip_last_error(dec.ctx)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want[0][0].view(np.uint32))
    for e in (0, 1):
        assert np.array_equal(planes[e, :, :w].view(np.uint32), want[e][1].view(np.uint32)), e
        assert (planes[e, :, w:] == -7.0).all()
    assert info.num_extra_channels == 2 and info.alpha_bits == 8


def test_lossless_rgba_vardct_alpha_and_lossless_rgb_back_to_back(ref, files):
    """No alpha pointer or plane of one file survives into the next: each file gives the bytes it gives alone."""
    cs = {"a": files["e1_rgba8_300x270"][0], "m": files["e1_rgb8_300x270"][0],
          "v": ref.RealStream(seed=31, xsize=300, ysize=270, alpha_bits=8, distance=1.0, speed_tier=3).codestream.tobytes()}
    f = S.fmt(abi.TF_SRGB, abi.SAMPLE_U8, 4)
    alone = {}
    for name in cs:
        d = VarDctDecoder(0)
        alone[name], _ = decode_file(d, cs[name], f, (270, 300))
        d.close()
    assert (alone["m"][..., 3] == 255).all() and len(np.unique(alone["a"][..., 3])) > 2 and len(np.unique(alone["v"][..., 3])) > 2
    for order in ("avmavm", "mvamva"):
        d = VarDctDecoder(0)
        for name in order:
            got, info = decode_file(d, cs[name], f, (270, 300))
            assert np.array_equal(got, alone[name]), (order, name)
        d.close()


@pytest.mark.parametrize("name", ["e7_rgba8_300x270", "e7_grey8_129x257"])
def test_djxl_hip_writes_the_reference_pixels(files, tmp_path, name):
    cs, m, want = files[name]
    h, w = want.shape[:2]
    grey = m["channels"][0] == "grey"
    src, dst = tmp_path / (name + ".jxl"), tmp_path / (name + (".ppm" if grey else ".pam"))  # (what the tool writes for VarDCT files of the kind)
    src.write_bytes(cs)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "djxl_hip.py"), str(src), str(dst)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    data = dst.read_bytes()
    ints = np.rint(want.astype(np.float64) * 255).astype(np.uint8)
    if grey:
        head = b"P6\n%d %d\n255\n" % (w, h)
        assert data.startswith(head)
        assert np.array_equal(np.frombuffer(data[len(head):], np.uint8).reshape(h, w, 3), ints[..., :3])
    else:
        head = b"P7\nWIDTH %d\nHEIGHT %d\nDEPTH 4\nMAXVAL 255\nTUPLTYPE RGB_ALPHA\nENDHDR\n" % (w, h)
        assert data.startswith(head), data[:80]
        assert np.array_equal(np.frombuffer(data[len(head):], np.uint8).reshape(h, w, 4), ints)
