"""Lossless files on the device: k_modular_emit alone against the numpy model (tests/modular_model.py) on synthetic
planes, and whole files against the reference decoder.

Kernel alone (jxlhip_decode_modular_frame): frames of 1x1, 3x5, 17x9, 129x127, 257x130 and 891x765 with groups of 128,
256, 512 and 1024 pixels -- one run, the scalar tail alone, several blocks of runs, widths that are no multiple of the
8-pixel run, group borders inside a wave --, all 42 RCT types at once (891x765 in 128-pixel groups has 42 of them, and
a two-RCT global program on top), two RCTs in a group's program, int16 and int32 planes, 8 / 10 / 12 / 16-bit samples,
padded plane rows, and canary bytes behind every output row and behind the buffer.  float RGB and 8-bit samples are
held bit-equal to the model (an 8-bit sample of an 8-bit image IS the integer the planes hold); u16, f16, dithered 8-bit
output of deeper samples, four channels, big-endian samples and the eight orientations go through
tests/output_sweep.py's yardstick (oracle.pack_output) with the identity transfer: every byte equal, that file's bar for
the linear encoding.

Whole files (jxlhip_decode_codestream): the seven streams of tests/test_modular_front_end.py plus the one whose groups
keep an RCT for the device, with 0 and 6 workers: float output bit-equal to JxlDecoder's pixels (both sides do ONE float32
multiply by float32(1 / 255)), 8-bit output equal to round(255 x) of them; a lossless and a VarDCT file back to back on
one context in both orders; tools/djxl_hip.py writes the reference's 8-bit pixels."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import modular_model as mm
import output_sweep as S
from libjxl_amd import VarDctDecoder, abi
from test_seam import hip_runner, jxl_decode, libs, load, ref  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5
SIZES = [(1, 1), (3, 5), (17, 9), (129, 127), (257, 130), (891, 765)]
GROUP_DIMS = [128, 256, 512, 1024]


@pytest.fixture(scope="module")
def dec():
    d = VarDctDecoder(0)
    yield d
    d.close()


def programs(w, h, gd, rng, two=False):
    """One program per group: every group another type, cycling through all 42 (a second RCT on top with `two`)."""
    ng = -(-w // gd) * -(-h // gd)
    p = (np.arange(ng) % 42).astype(np.uint16)
    if two:
        p |= (rng.integers(1, 42, ng).astype(np.uint16) << 8)
    return p


def coded_planes(img, gd, group_rct, global_rct, dtype):
    """The planes an encoder that applied these programs would have left: the global RCTs first-listed first, then each
    group's.  img: [3, H, W] integer samples."""
    p = [np.array(c, np.int32) for c in img]
    for t in (global_rct & 0xFF, global_rct >> 8):
        p = mm.forward_rct(p, t)
    h, w = p[0].shape
    xsg = -(-w // gd)
    for g, prog in enumerate(group_rct):
        ys = slice((g // xsg) * gd, min(h, (g // xsg + 1) * gd))
        xs = slice((g % xsg) * gd, min(w, (g % xsg + 1) * gd))
        q = [c[ys, xs].copy() for c in p]  # (copies: a permutation returns its inputs)
        for t in (int(prog) & 0xFF, int(prog) >> 8):
            q = mm.forward_rct(q, t)
        for c in range(3):
            p[c][ys, xs] = q[c]
    out = np.stack(p)
    if dtype == np.int16:
        assert np.abs(out).max() < 32768
    return out.astype(dtype)


def emit(dec, planes, bits, gd, group_rct, global_rct, kind, f=None, orient=0, in_pad=0, out_pad=24, expect=0):
    """jxlhip_decode_modular_frame on [3, H, W] int16 / int32 planes; returns the [H', W', channels] output after checking
    the canaries behind every row and behind the buffer."""
    L = dec.L
    _, h, w = planes.shape
    host = np.full((3, h, w + in_pad), 0x55AA if planes.dtype == np.int32 else 0x55A, planes.dtype)
    host[:, :, :w] = planes
    m = abi.ModularFrame()
    m.xsize, m.ysize = w, h
    for c in range(3):
        m.planes[c] = host[c].ctypes.data
    m.stride_samples = w + in_pad
    m.sample_type = abi.MODULAR_I16 if planes.dtype == np.int16 else abi.MODULAR_I32
    m.bits_per_sample = bits
    m.group_dim = gd
    rct = None if group_rct is None else np.ascontiguousarray(group_rct, np.uint16)
    m.group_rct = None if rct is None else rct.ctypes.data
    m.global_rct = int(global_rct)
    of = None
    if f is not None:
        of = abi.OutputFormat(f["transfer"], f["sample_type"], f["num_channels"], f["bits_per_sample"], f["swap_endianness"],
                              f["tf_param"], f["luminances"])
    bpp = 12 if kind == 1 else f["num_channels"] * {0: 4, 1: 1, 2: 2, 3: 2}[f["sample_type"]]
    ow, oh = (h, w) if orient >= 5 else (w, h)
    ssz = 4 if kind == 1 else {0: 4, 1: 1, 2: 2, 3: 2}[f["sample_type"]]
    stride = ow * bpp + out_pad
    stride += -stride % ssz
    tail = 256
    buf = torch.full((oh * stride + tail,), SENTINEL, dtype=torch.uint8, device="cuda")
    rc = L.jxlhip_decode_modular_frame(dec.ctx, C.byref(m), kind, C.byref(of) if of else None, buf.data_ptr(), stride, orient)
    assert rc == expect, (rc, L.jxlhip_last_error(dec.ctx))
    assert L.jxlhip_sync(dec.ctx) == 0
    raw = buf.cpu().numpy()
    if expect:
        assert (raw == SENTINEL).all()
        return None
    assert (raw[oh * stride:] == SENTINEL).all(), "bytes behind the buffer touched"
    rows = raw[:oh * stride].reshape(oh, stride)
    S.check_padding(rows, ow * bpp, SENTINEL)
    dt = np.float32 if kind == 1 else {0: np.float32, 1: np.uint8, 2: np.uint16, 3: np.uint16}[f["sample_type"]]
    nc = 3 if kind == 1 else f["num_channels"]
    return np.ascontiguousarray(rows[:, :ow * bpp]).view(dt).reshape(oh, ow, nc)


def linear(f):
    return dict(f, transfer=abi.TF_LINEAR)


@pytest.mark.parametrize("gd", GROUP_DIMS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_kernel_float_and_8bit_are_bit_equal_to_the_model(oracle, dec, size, gd):
    w, h = size
    rng = np.random.default_rng(w * 1000 + h + gd)
    img = rng.integers(0, 256, (3, h, w))
    img[:, : h // 2 + 1, : w // 3 + 1] = rng.integers(0, 2, (3, 1, 1)) * 255  # (a flat corner: codes 0 and 255)
    group_rct = programs(w, h, gd, rng)
    global_rct = 6 | (9 << 8)  # a 43rd choice, of two RCTs, behind every group's
    for dtype, pad in ((np.int16, 0), (np.int32, 5), (np.int16, 3)):
        planes = coded_planes(img, gd, group_rct, global_rct, dtype)
        want = mm.emit_f32(planes, 8, gd, group_rct, global_rct)
        assert np.array_equal(np.rint(want * 255).astype(np.int64), img.transpose(1, 2, 0))  # (the model undoes what was done)
        got = emit(dec, planes, 8, gd, group_rct, global_rct, 1, in_pad=pad)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (dtype, np.argwhere(got != want)[:3])
        f = S.fmt(abi.TF_SRGB, abi.SAMPLE_F32, 3)  # (the transfer function is not read: the samples are encoded already)
        got = emit(dec, planes, 8, gd, group_rct, global_rct, 2, f, in_pad=pad)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        for nc in (3, 4):
            f = S.fmt(abi.TF_SRGB, abi.SAMPLE_U8, nc)
            # rows that are 4-byte aligned -- the run goes out as 24 / 32 contiguous bytes -- and rows at odd addresses
            for out_pad in (24 + -(w * nc) % 4, 7 + (w * nc) % 2):
                got = emit(dec, planes, 8, gd, group_rct, global_rct, 2, f, in_pad=pad, out_pad=out_pad)
                assert np.array_equal(got[..., :3], img.transpose(1, 2, 0).astype(np.uint8)), (dtype, nc, out_pad)
                assert np.array_equal(got, oracle.pack_output(linear(f), want))


def test_kernel_wraps_like_the_reference_on_any_int32(dec):
    """Planes that hold ANY int32 (sums that wrap, >> 1 of negative values) under two-RCT programs in every group."""
    w, h, gd = 257, 130, 128
    rng = np.random.default_rng(7)
    planes = rng.integers(-2 ** 31, 2 ** 31, (3, h, w)).astype(np.int32)
    planes[:, :4, :40] = np.array([-2 ** 31, 2 ** 31 - 1, -1, 0, 1, -2 ** 31 + 1, 2 ** 31 - 2, 12345], np.int32).repeat(5)
    group_rct = programs(w, h, gd, rng, two=True)
    group_rct[:2] = [41 | (41 << 8), 6 | (6 << 8)]
    for global_rct in (0, 13, 20 | (34 << 8)):
        want = mm.emit_f32(planes, 16, gd, group_rct, global_rct)
        got = emit(dec, planes, 16, gd, group_rct, global_rct, 1)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # no programs at all (NULL): the samples as they are
    got = emit(dec, planes, 12, gd, None, 0, 1)
    assert np.array_equal(got.view(np.uint32), mm.emit_f32(planes, 12, gd).view(np.uint32))


@pytest.mark.parametrize("bits", [8, 10, 12, 16])
def test_kernel_bit_depths_and_every_sample_type(oracle, dec, bits):
    """Samples of 8 .. 16 bits into every sample type (an 8-bit output of deeper samples is where the dither decides),
    3 and 4 channels, both endiannesses: oracle.pack_output with the identity transfer, every byte equal."""
    w, h, gd = 129, 127, 128
    rng = np.random.default_rng(bits)
    img = rng.integers(0, 1 << bits, (3, h, w))
    img[:, :9, :9] = 0
    img[:, -9:, -9:] = (1 << bits) - 1
    group_rct = programs(w, h, gd, rng, two=True)
    dtype = np.int16 if bits <= 12 else np.int32
    planes = coded_planes(img, gd, group_rct, 1, dtype)
    lin = mm.emit_f32(planes, bits, gd, group_rct, 1)
    assert np.array_equal(np.rint(lin.astype(np.float64) * ((1 << bits) - 1)).astype(np.int64), img.transpose(1, 2, 0))
    for f in [S.fmt(abi.TF_SRGB, abi.SAMPLE_U8, 3), S.fmt(abi.TF_PQ, abi.SAMPLE_U8, 4, par=1000.0), S.fmt(abi.TF_SRGB, abi.SAMPLE_U8, 3, bits=5),
              S.fmt(abi.TF_SRGB, abi.SAMPLE_U16, 3), S.fmt(abi.TF_709, abi.SAMPLE_U16, 4, swap=1), S.fmt(abi.TF_SRGB, abi.SAMPLE_U16, 3, bits=10),
              S.fmt(abi.TF_SRGB, abi.SAMPLE_F16, 3), S.fmt(abi.TF_HLG, abi.SAMPLE_F16, 4, swap=1, par=1000.0),
              S.fmt(abi.TF_SRGB, abi.SAMPLE_F32, 4), S.fmt(abi.TF_LINEAR, abi.SAMPLE_F32, 3, swap=1)]:
        got = emit(dec, planes, bits, gd, group_rct, 1, 2, f)
        S.compare(linear(f), got, oracle.pack_output(linear(f), lin), lin)
        if f["sample_type"] == abi.SAMPLE_U16 and f["bits_per_sample"] == bits and not f["swap_endianness"]:
            assert np.array_equal(got[..., :3], img.transpose(1, 2, 0))  # (a 16-bit sample of a `bits`-bit image: the integer)


@pytest.mark.parametrize("o", range(2, 9))
def test_kernel_orientations(oracle, dec, o):
    """undo_orientation: the frame goes through the staging frame and k_orient; the 8-bit dither follows the FLIPPED
    coordinates (the reference dithers after its flips and before its transposed write: tests/test_gpu_output_encoding.py)."""
    w, h, gd = 257, 130, 256
    rng = np.random.default_rng(o)
    img = rng.integers(0, 1024, (3, h, w))
    group_rct = programs(w, h, gd, rng)
    planes = coded_planes(img, gd, group_rct, 0, np.int16)
    lin = mm.emit_f32(planes, 10, gd, group_rct, 0)
    fx, fy, tr = o in (2, 3, 7, 8), o in (3, 4, 6, 7), o >= 5
    flipped = lin[:, ::-1] if fx else lin
    flipped = np.ascontiguousarray(flipped[::-1] if fy else flipped)
    got = emit(dec, planes, 10, gd, group_rct, 0, 1, orient=o)
    want = flipped.swapaxes(0, 1) if tr else flipped
    assert np.array_equal(got, want)
    for f in (S.fmt(abi.TF_SRGB, abi.SAMPLE_U8, 3), S.fmt(abi.TF_SRGB, abi.SAMPLE_U16, 4), S.fmt(abi.TF_SRGB, abi.SAMPLE_F16, 3)):
        got = emit(dec, planes, 10, gd, group_rct, 0, 2, f, orient=o)
        want = oracle.pack_output(linear(f), flipped)
        S.compare(linear(f), got, np.ascontiguousarray(want.swapaxes(0, 1)) if tr else want, want)


def test_kernel_refusals(dec):
    planes = np.zeros((3, 9, 17), np.int16)
    f = S.fmt(abi.TF_SRGB, abi.SAMPLE_U8, 3)
    emit(dec, planes, 8, 128, None, 0, 0, f, expect=-7)  # planar XYB
    assert b"XYB" in dec.L.jxlhip_last_error(dec.ctx)
    emit(dec, planes, 8, 96, None, 0, 2, f, expect=-1)  # a group dimension the format does not have
    emit(dec, planes, 17, 128, None, 0, 2, f, expect=-1)
    emit(dec, planes, 0, 128, None, 0, 2, f, expect=-1)
    emit(dec, planes, 8, 128, np.array([42], np.uint16), 0, 2, f, expect=-1)  # an RCT type above 41
    emit(dec, planes, 8, 128, None, 42 << 8, 2, f, expect=-1)
    emit(dec, planes, 8, 128, None, 0, 2, f, orient=9, expect=-1)


# ---- whole files -----------------------------------------------------------------------------------------------------

STREAMS = [dict(xsize=1, ysize=1), dict(xsize=17, ysize=9), dict(xsize=256, ysize=256), dict(xsize=257, ysize=255),
           dict(xsize=600, ysize=400), dict(xsize=1030, ysize=520), dict(xsize=2100, ysize=300),
           dict(xsize=1030, ysize=520, seed=6, gain=4.0)]  # (the one whose groups keep an RCT for the device)


@pytest.fixture(scope="module")
def files(ref, libs):
    """(codestream, the reference JxlDecoder's float pixels) per stream, decoded once."""
    RL = load(libs[0])
    out = []
    for kw in STREAMS:
        cs = ref.feature_stream("modular", **dict(dict(seed=5, distance=1.0), **kw))
        out.append((cs, jxl_decode(RL, cs)))
    return out


def decode_file(dec, cs, f, shape, runner=None, pool=None, kind=2, flags=0, expect=0):
    L = dec.L
    h, w = shape
    of = abi.OutputFormat(f["transfer"], f["sample_type"], f["num_channels"], f["bits_per_sample"], f["swap_endianness"],
                          f["tf_param"], f["luminances"])
    dt = {0: torch.float32, 1: torch.uint8, 2: torch.int16, 3: torch.int16}[f["sample_type"]]
    out = torch.zeros((h, w, f["num_channels"]), dtype=dt, device="cuda")
    info = abi.CodestreamInfo()
    rc = L.jxlhip_decode_codestream(dec.ctx, runner, pool, cs, len(cs), kind | flags, C.byref(of), out.data_ptr(),
                                    w * f["num_channels"] * out.element_size(), 0, C.byref(info))
    assert rc == expect, (rc, L.jxlhip_last_error(dec.ctx))
    return out.cpu().numpy(), info


@pytest.mark.parametrize("workers", [0, 6])
def test_whole_files_equal_the_reference_decoder(dec, files, workers):
    R, runner, pool = hip_runner() if workers else (None, None, None)
    try:
        kept = 0
        for (cs, want), kw in zip(files, STREAMS):
            h, w = want.shape[:2]
            got, info = decode_file(dec, cs, S.fmt(abi.TF_SRGB, abi.SAMPLE_F32, 3), (h, w), runner, pool)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), kw
            assert info.modular == 1 and (info.xsize, info.ysize) == (w, h) and info.num_passes == 1
            assert info.epf_iters == 0 and info.gab == 0 and info.used_acs == 0 and info.coeff_type == 0
            got8, _ = decode_file(dec, cs, S.fmt(abi.TF_SRGB, abi.SAMPLE_U8, 3), (h, w), runner, pool)
            assert np.array_equal(got8, np.rint(want * 255).astype(np.uint8)), kw
            ms = (C.c_double * 7)()
            assert dec.L.jxlhip_codestream_phase_ms(dec.ctx, ms) == 0
            assert ms[1] == 0 and ms[2] == 0 and ms[3] == 0 and ms[5] == 0 and ms[0] > 0 and ms[6] > 0
            kept += kw.get("gain") is not None
        assert kept == 1
    finally:
        if pool:
            R.JxlThreadParallelRunnerDestroy(pool)


def test_whole_file_refusals_and_orientation(dec, files):
    cs, want = files[4]
    h, w = want.shape[:2]
    # another transfer function than the original's: nothing on this path converts
    decode_file(dec, cs, S.fmt(abi.TF_LINEAR, abi.SAMPLE_F32, 3), (h, w), expect=-7)
    assert b"transfer function" in dec.L.jxlhip_last_error(dec.ctx)
    decode_file(dec, cs, S.fmt(abi.TF_SRGB, abi.SAMPLE_F32, 3), (h, w), kind=1, expect=-7)  # (JXLHIP_OUT_LINEAR_RGB_F32 is linear)
    decode_file(dec, cs, S.fmt(abi.TF_SRGB, abi.SAMPLE_F32, 3), (h, w), kind=0, expect=-7)
    assert b"XYB" in dec.L.jxlhip_last_error(dec.ctx)
    # a display on the context: refused for these files, and gone again afterwards
    d = abi.Display(203.0, 0, 0)
    assert dec.L.jxlhip_codestream_set_display(dec.ctx, C.byref(d)) == 0
    decode_file(dec, cs, S.fmt(abi.TF_SRGB, abi.SAMPLE_U8, 3), (h, w), expect=-7)
    assert b"display" in dec.L.jxlhip_last_error(dec.ctx)
    assert dec.L.jxlhip_codestream_set_display(dec.ctx, None) == 0
    # the orientation flag (these streams are orientation 1: the same bytes)
    got, _ = decode_file(dec, cs, S.fmt(abi.TF_SRGB, abi.SAMPLE_U8, 4), (h, w), flags=0x100)
    assert np.array_equal(got[..., :3], np.rint(want * 255).astype(np.uint8)) and (got[..., 3] == 255).all()


def test_lossless_and_vardct_files_back_to_back_leave_no_state(ref, files):
    cs_m, want = files[4]
    cs_v = ref.feature_stream("plain", xsize=600, ysize=400, seed=5, distance=1.0)
    f = S.fmt(abi.TF_SRGB, abi.SAMPLE_U8, 3)
    alone = {}
    for name, cs in (("m", cs_m), ("v", cs_v)):
        d = VarDctDecoder(0)
        alone[name], _ = decode_file(d, cs, f, (400, 600))
        d.close()
    assert np.array_equal(alone["m"], np.rint(want * 255).astype(np.uint8))
    for order in ("mvmv", "vmvm"):
        d = VarDctDecoder(0)
        for name in order:
            got, info = decode_file(d, cs_m if name == "m" else cs_v, f, (400, 600))
            assert np.array_equal(got, alone[name]), (order, name)
            assert info.modular == (name == "m")
        d.close()


def test_djxl_hip_writes_the_reference_pixels(files, tmp_path):
    cs, want = files[4]
    src, dst = tmp_path / "lossless.jxl", tmp_path / "lossless.ppm"
    src.write_bytes(cs)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "djxl_hip.py"), str(src), str(dst)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    data = dst.read_bytes()
    assert data.startswith(b"P6\n600 400\n255\n")
    px = np.frombuffer(data[len(b"P6\n600 400\n255\n"):], np.uint8).reshape(400, 600, 3)
    assert np.array_equal(px, np.rint(want * 255).astype(np.uint8))
