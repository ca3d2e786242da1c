"""Blending on images with extra channels on the device (jxlhip_set_blending_extra, jxlhip_canvas_read_extra,
jxlhip_frame_extra_read, kernels_blend_ec.hip): k_ec_blend against tests/alpha_blending_model.py bit for bit, the alpha of
packed outputs, layered files against the reference's JxlDecoder, and the refused configurations.

The kernel tests use synthetic frames like tests/test_gpu_blending.py: a canvas-sized frame A is saved into a slot with
its extra-channel planes, frame B is decoded with blending on.  Colour and planes -- the caller's buffer, the saved canvas
and the frame's own planes -- must each be BIT-EQUAL to the model applied to the SAME decoder's direct float output of A
and B and to the planes handed in.

Smallest shapes that can still go wrong: canvases 201, 202 and 203 wide (every W mod 4 tail) and 67 high, a 72 x 40 frame
at origins with x0 mod 4 = 1, 0, 2, 3, one negative and one crossing the right and the bottom edge.  The planes hold
values below 0 and above 1, exact zeroes and ones, and a region where the frame's and the canvas's alpha are both 0."""
import ctypes as C
import itertools

import numpy as np
import pytest

from libjxl_amd import abi, synth

import alpha_blending_model as am
import output_sweep as osw
from test_gpu_blending import SENTINEL, float_format, same

WIDTHS = (201, 202, 203)
H = 67
FW, FH = 72, 40
ORIGINS = [(37, 21), (-20, -9), (170, 50), (43, 3)]  # x0 mod 4 = 1, 0, 2, 3
SRGB_F32 = osw.fmt(abi.TF_SRGB, abi.SAMPLE_F32, 3)
SRGB_F32_RGBA = osw.fmt(abi.TF_SRGB, abi.SAMPLE_F32, 4)
SRGB_U8_RGBA = osw.fmt(abi.TF_SRGB, abi.SAMPLE_U8, 4)
# the caller's output: none (the frame is only saved), float RGB, packed float RGB, packed float RGBA
OUTS = {"save-only": (2, SRGB_F32), "linear": (1, None), "srgb": (2, SRGB_F32), "rgba": (2, SRGB_F32_RGBA)}
ALPHA, OTHER = dict(is_alpha=1), dict(is_alpha=0)


def configs(clamp, premul):
    """The extra channels of a frame: (info, ec, the colour's alpha channel).  One, two and four channels with mixed
    modes; a channel that is no alpha blended with kBlend through the alpha channel; an image whose extra channels are
    none of type alpha; an alpha channel that is not channel 0."""
    a = dict(ALPHA, alpha_associated=premul)
    o = dict(OTHER, alpha_associated=premul)  # (read only where the channel is named as somebody's alpha channel)
    return [
        ([a], [dict(mode=am.BLEND, alpha_channel=0, clamp=clamp)], 0),
        ([a, OTHER], [dict(mode=am.ADD), dict(mode=am.BLEND, alpha_channel=0, clamp=clamp)], 0),
        ([a, OTHER, OTHER, a], [dict(mode=am.BLEND, alpha_channel=0), dict(mode=am.ALPHA_WEIGHTED_ADD, alpha_channel=0, clamp=clamp),
                                dict(mode=am.MUL, clamp=clamp), dict(mode=am.BLEND, alpha_channel=3, clamp=clamp)], 3),
        ([OTHER, o], [dict(mode=am.BLEND, alpha_channel=1, clamp=clamp), dict(mode=am.ALPHA_WEIGHTED_ADD, alpha_channel=1)], 1),
        ([OTHER, a], [dict(mode=am.MUL), dict(mode=am.REPLACE)], 1),
    ]


def make_planes(seed, h, w, zero):
    """Four planes [4, h, w]: uniform in [-0.3, 1.3], a block of exact ones, and exact zeroes in `zero` = (y0, y1, x0, x1)."""
    p = np.random.default_rng(seed).uniform(-0.3, 1.3, (4, h, w)).astype(np.float32)
    p[:, h - 12:h - 4, 4:30] = 1.0
    y0, y1, x0, x1 = zero
    p[:, y0:y1, x0:x1] = 0.0
    p.setflags(write=False)
    return p


class Bench:
    """One decoder, the synthetic frames and planes, and the decoder's direct outputs of the frames (computed once per
    format, read-only)."""

    def __init__(self):
        from libjxl_amd import VarDctDecoder
        self.dec = VarDctDecoder(0)
        self.dq = self.dec.default_dequant_tables()
        self.inputs, self.planes, self.direct_cache = {}, {}, {}
        for w in WIDTHS:
            for name, seed in (("A", 11), ("A2", 12)):
                self.inputs[(name, w)] = synth.synth_frame(w, H, device="cuda", seed=seed + w, gab=True, epf_iters=1)
                # (zero under the first rows and columns of a frame at (37, 21))
                self.planes[(name, w)] = make_planes(seed + w, H, w, (21, 33, 37, 52))
        # (brighter and rougher: some per cent of its samples above 1 and below 0, so that kMul's clamp shows)
        self.inputs["B"] = synth.synth_frame(FW, FH, device="cuda", seed=13, gab=True, epf_iters=1, intensity_target=60.0, amp=30.0)
        self.planes["B"] = make_planes(13, FH, FW, (0, 10, 0, 12))

    def close(self):
        self.dec.close()

    def begin(self, name, kind, f):
        self.dec.begin_frame(dict(self.inputs[name][0], output_kind=kind, out_format=f))
        self.dec.set_inputs(self.inputs[name][1], self.dq)

    def direct(self, name, kind, f):
        """The frame decoded without blending, as float RGB in f's transfer function."""
        ff = float_format(f)
        key = (name, kind, None if ff is None else (ff["transfer"], ff["tf_param"]))
        if key not in self.direct_cache:
            self.begin(name, kind, ff)
            out = self.dec.decode_frame()
            self.dec.sync()
            a = out.cpu().numpy()
            a.setflags(write=False)
            self.direct_cache[key] = a
        return self.direct_cache[key]

    def save(self, name, w, n, kind, f, slot, info=None):
        """Canvas frame `name` of width w with its first n planes saved into `slot`, written nowhere else."""
        self.begin((name, w), kind, f)
        self.dec.set_blending((w, H), (0, 0), abi.BLEND_REPLACE, False, 0, slot)
        self.dec.set_blending_extra(self.planes[(name, w)][:n], info or [OTHER] * n)
        assert self.dec.decode_frame(out=False) is None

    def blend(self, w, origin, color, ec, info, kind, f, source, ec_sources, save_slot, out=True):
        """Frame B blended over the canvas; returns the caller's region of a sentinel-filled buffer with padded rows (None
        without a buffer)."""
        import torch
        self.begin("B", kind, f)
        self.dec.set_blending((w, H), origin, color["mode"], color["clamp"], source, save_slot)
        chans = [dict(i, **e, source=s) for i, e, s in zip(info, ec, ec_sources)]
        self.dec.set_blending_extra(self.planes["B"][:len(ec)], chans, color["alpha_channel"])
        if not out:
            assert self.dec.decode_frame(out=False) is None
            self.dec.sync()
            return None
        like = self.dec.alloc_output()
        shape, dt = tuple(like.shape), like.dtype
        assert shape[:2] == (H, w)
        s = SENTINEL[np.dtype(str(dt).split(".")[1])]
        buf = torch.full((shape[0] + 1, shape[1] + 5, shape[2]), s, dtype=dt, device="cuda")
        self.dec.decode_frame(buf[:shape[0], :shape[1]])
        self.dec.sync()
        raw = buf.cpu().numpy()
        assert np.all(raw[:shape[0], shape[1]:] == s) and np.all(raw[shape[0]:] == s)  # the padding is the caller's
        return np.ascontiguousarray(raw[:shape[0], :shape[1]])

    def canvas(self, slot):
        t = self.dec.read_canvas(slot)
        return None if t is None else t.cpu().numpy()

    def canvas_planes(self, slot, n):
        got = [self.dec.read_canvas_extra(slot, i) for i in range(n)]
        assert self.dec.read_canvas_extra(slot, n) is None if n < 4 else True
        return np.stack([g.cpu().numpy() for g in got])

    def frame_planes(self, n):
        return np.stack([self.dec.read_frame_extra(i).cpu().numpy() for i in range(n)])


@pytest.fixture(scope="module")
def bench():
    b = Bench()
    yield b
    b.close()


def first_alpha(info):
    return next((i for i, c in enumerate(info) if c["is_alpha"]), None)


# ---- the kernel against the model -----------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("out", sorted(OUTS))
@pytest.mark.parametrize("w", WIDTHS)
def test_kernel_is_bit_equal_to_the_model(bench, w, out):
    """Every colour mode x clamp x {straight, premultiplied} with EVERY channel configuration (the four with a channel of
    type alpha, and the one without as one more run), the origins cycling over the 100 combinations, each saved into the
    source slot, into another slot, not saved, and with the extra channels' source another slot than the colour's."""
    k, f = OUTS[out]
    a, a2, b = bench.direct(("A", w), k, f), bench.direct(("A2", w), k, f), bench.direct("B", k, f)
    pa, pa2, pb = bench.planes[("A", w)], bench.planes[("A2", w)], bench.planes["B"]
    dec = bench.dec
    seen_overrides = 0
    with_alpha = set()
    for idx, (mode, clamp, premul, cfg) in enumerate(itertools.product(am.MODES, (0, 1), (0, 1), range(5))):
        info, ec, ca = configs(clamp, premul)[cfg]
        n = len(ec)
        if first_alpha(info) is not None:
            with_alpha.add((mode, clamp, premul))
        origin = ORIGINS[idx % 4]
        color = dict(mode=mode, clamp=clamp, alpha_channel=ca)
        for how in ("same", "other", "none", "alpha-other"):
            if out == "save-only" and how == "none":
                continue
            src = idx % 4
            src2 = (src + 2) % 4
            save = {"same": src, "other": (src + 1) % 4, "none": None, "alpha-other": src}[how]
            ec_src = [src2 if how == "alpha-other" else src] * n
            for slot in range(4):
                dec.set_reference_frame(slot, None)
            bench.save("A", w, n, k, f, src)
            if how == "alpha-other":
                bench.save("A2", w, n, k, f, src2)
            bg_ec = pa2[:n] if how == "alpha-other" else pa[:n]
            want, wantp = am.blend(a, list(bg_ec), b, pb[:n], origin, color, ec, info)
            got = bench.blend(w, origin, color, ec, info, k, f, src, ec_src, save, out=out != "save-only")
            what = (mode, clamp, premul, cfg, origin, how)
            if out == "rgba":
                fa = first_alpha(info)
                assert same(np.ascontiguousarray(got[..., :3]), want), what
                # the fourth sample: the blended plane of the first alpha channel, opaque without one
                assert same(np.ascontiguousarray(got[..., 3]), wantp[fa] if fa is not None else np.ones((H, w), np.float32)), what
            elif got is not None:
                assert same(got, want), what  # (every canvas pixel written: the sentinel is no value of the model's)
            assert same(bench.frame_planes(n), wantp), what
            if save is not None:
                assert same(bench.canvas(save), want), what
                assert same(bench.canvas_planes(save, n), wantp), what
            if save != src:
                assert same(bench.canvas(src), a) and same(bench.canvas_planes(src, n), pa[:n]), what  # read only
            if how == "alpha-other":
                assert same(bench.canvas(src2), a2) and same(bench.canvas_planes(src2, n), pa2[:n]), what
            if mode == am.BLEND and first_alpha(info) is not None:
                seen_overrides += int(not np.array_equal(
                    wantp[ca], am.blend(a, list(bg_ec), b, pb[:n], origin, dict(color, mode=am.ADD), ec, info)[1][ca]))
    assert seen_overrides > 0  # colour kBlend wrote its new alpha over a channel's own result somewhere
    assert len(with_alpha) == 20  # every colour mode x clamp x {straight, premultiplied} met an image with an alpha channel


@pytest.mark.gpu
def test_the_inputs_are_worth_the_test(bench):
    w = 203
    k, f = OUTS["srgb"]
    a, b = bench.direct(("A", w), k, f), bench.direct("B", k, f)
    pa, pb = bench.planes[("A", w)], bench.planes["B"]
    assert float(pb.min()) < 0.0 and float(pb.max()) > 1.0 and float(pa.min()) < 0.0 and float(pa.max()) > 1.0
    assert np.all(pa[0, 21:31, 37:49] == 0.0) and np.all(pb[0, :10, :12] == 0.0)  # both alphas 0: rnew_a = 0
    assert np.any(pa == 1.0) and np.any(pb == 1.0)
    for premul in (0, 1):
        info, ec0, ca = configs(0, premul)[0]
        _, ec1, _ = configs(1, premul)[0]
        for mode in (am.BLEND, am.ALPHA_WEIGHTED_ADD):
            r0 = am.blend(a, [pa[0]], b, pb[:1], (37, 21), dict(mode=mode, clamp=0, alpha_channel=0), ec0, info)
            r1 = am.blend(a, [pa[0]], b, pb[:1], (37, 21), dict(mode=mode, clamp=1, alpha_channel=0), ec1, info)
            assert not np.array_equal(r0[0], r1[0]), (premul, mode)  # the clamp changes the colour
        assert not np.array_equal(r0[1], r1[1])                      # ... and the alpha
    # straight and premultiplied differ, and the zero-alpha region of a straight blend is black
    s = am.blend(a, [pa[0]], b, pb[:1], (37, 21), dict(mode=am.BLEND, clamp=0, alpha_channel=0), *configs(0, 0)[0][1::-1])
    p = am.blend(a, [pa[0]], b, pb[:1], (37, 21), dict(mode=am.BLEND, clamp=0, alpha_channel=0), *configs(0, 1)[0][1::-1])
    assert not np.array_equal(s[0], p[0]) and np.all(s[0][21:31, 37:49] == 0.0) and np.all(np.isfinite(s[0]))


@pytest.mark.gpu
def test_empty_slots_are_zeroes_and_a_chain_blends_in_place(bench):
    w = 203
    k, f = OUTS["srgb"]
    dec = bench.dec
    a, b = bench.direct(("A", w), k, f), bench.direct("B", k, f)
    pa, pb = bench.planes[("A", w)], bench.planes["B"]
    info, ec, ca = configs(1, 0)[1]
    color = dict(mode=am.BLEND, clamp=1, alpha_channel=ca)
    for slot in range(4):
        dec.set_reference_frame(slot, None)
    # nothing in slot 2: colour and planes blend over zeroes, and the whole canvas is written
    want = am.blend(None, [None, None], b, pb[:2], (37, 21), color, ec, info, size=(w, H))
    got = bench.blend(w, (37, 21), color, ec, info, k, f, 2, [2, 2], 2)
    assert same(got, want[0]) and same(bench.canvas(2), want[0]) and same(bench.canvas_planes(2, 2), want[1])
    # three blends into their own source slot, the last without a caller's buffer: only the rectangle is visited
    bench.save("A", w, 2, k, f, 1)
    c1 = am.blend(a, list(pa[:2]), b, pb[:2], (37, 21), color, ec, info)
    g1 = bench.blend(w, (37, 21), color, ec, info, k, f, 1, [1, 1], 1)
    c2 = am.blend(c1[0], list(c1[1]), b, pb[:2], (-20, -9), color, ec, info)
    g2 = bench.blend(w, (-20, -9), color, ec, info, k, f, 1, [1, 1], 1)
    c3 = am.blend(c2[0], list(c2[1]), b, pb[:2], (170, 50), color, ec, info)
    assert bench.blend(w, (170, 50), color, ec, info, k, f, 1, [1, 1], 1, out=False) is None
    assert same(g1, c1[0]) and same(g2, c2[0])
    assert same(bench.canvas(1), c3[0]) and same(bench.canvas_planes(1, 2), c3[1]) and same(bench.frame_planes(2), c3[1])
    assert bench.canvas(0) is None and bench.canvas(3) is None and dec.read_canvas_extra(0, 0) is None


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 4])
def test_packed_u8_alpha_goes_through_the_output_stage(bench, oracle, which):
    """RGBA u8: the colour bytes are the oracle's sample conversion of the blended colour (transfer function off: the
    samples were encoded before the blend), the alpha bytes what the output stage makes of the blended alpha plane
    handed in as a frame's alpha (jxlhip_set_alpha: dither at canvas coordinates, clamp, rounding)."""
    w = 203
    f = SRGB_U8_RGBA
    dec = bench.dec
    a, b = bench.direct(("A", w), 2, f), bench.direct("B", 2, f)
    pa, pb = bench.planes[("A", w)], bench.planes["B"]
    info, ec, ca = configs(1, 0)[which]
    n = len(ec)
    color = dict(mode=am.BLEND, clamp=1, alpha_channel=ca)
    bench.save("A", w, n, 2, f, 0)
    want, wantp = am.blend(a, list(pa[:n]), b, pb[:n], (43, 3), color, ec, info)
    got = bench.blend(w, (43, 3), color, ec, info, 2, f, 0, [0] * n, 0)
    assert got.dtype == np.uint8 and got.shape == (H, w, 4)
    rgb = oracle.pack_output(dict(f, transfer=abi.TF_LINEAR), want)
    assert np.array_equal(got[..., :3], rgb[..., :3])
    bench.begin(("A", w), 2, f)
    dec.set_alpha(wantp[first_alpha(info)])
    ref = dec.decode_frame()
    dec.sync()
    assert np.array_equal(got[..., 3], ref.cpu().numpy()[..., 3])
    assert len(np.unique(got[..., 3])) > 50  # a real plane, not the opaque value


@pytest.mark.gpu
def test_blend_ec_launch_is_profiled_in_its_own_slot(bench):
    w = 203
    k, f = OUTS["srgb"]
    dec = bench.dec
    info, ec, ca = configs(0, 0)[0]
    bench.save("A", w, 1, k, f, 0)
    dec.profile(True)
    try:
        bench.blend(w, (37, 21), dict(mode=am.BLEND, clamp=0, alpha_channel=0), ec, info, k, f, 0, [0], 0)
        slots = dec.profile_read()
        assert slots["blend_ec"][1] == 1 and "blend" not in slots, slots
    finally:
        dec.profile(False)
    assert abi.KERNEL_NAMES_EX[11] == "blend_ec" and abi.KERNEL_COUNT_EX >= 12 and abi.KERNEL_COUNT == 8


# ---- state and refusals of the context calls --------------------------------------------------------------------------

@pytest.mark.gpu
def test_set_blending_extra_state_and_refusals(bench):
    w = 203
    k, f = OUTS["srgb"]
    dec, L = bench.dec, bench.dec.L
    planes = np.ascontiguousarray(bench.planes["B"][:2])

    def params(n=2, color_alpha=0, **over):
        e = abi.BlendExtraParams()
        e.num_extra_channels = n
        e.color_alpha_channel = color_alpha
        e.stride_floats = over.pop("stride", FW)
        for i in range(min(n, 4)):
            e.planes[i] = planes[i % 2].ctypes.data
            e.channel[i].is_alpha = int(i == 0)
        for key, (i, v) in over.items():
            setattr(e.channel[i], key, v)
        return e

    def call(e):
        return L.jxlhip_set_blending_extra(dec.ctx, C.byref(e))

    for slot in range(4):
        dec.set_reference_frame(slot, None)
    # without set_blending on the frame; frame_begin and set_blending(NULL) reset
    bench.begin("B", k, f)
    assert call(params()) == -6 and b"without set_blending" in L.jxlhip_last_error(dec.ctx)
    dec.set_blending((w, H), (37, 21), abi.BLEND_BLEND, False, 0, None)
    assert call(params()) == 0
    dec.set_blending(None)
    assert call(params()) == -6
    dec.set_blending((w, H), (37, 21), abi.BLEND_BLEND, False, 0, None)
    assert call(params()) == 0
    bench.begin("B", k, f)  # (a new frame_begin resets blending and the extra channels with it)
    dec.image_size = None
    out = dec.decode_frame()
    dec.sync()
    assert same(out.cpu().numpy(), bench.direct("B", k, f))
    assert L.jxlhip_frame_extra_read(dec.ctx, 0, C.c_void_p(out.data_ptr()), w) == -6
    # bad arguments
    dec.set_blending((w, H), (37, 21), abi.BLEND_BLEND, False, 0, None)
    for bad in (params(0), params(5), params(color_alpha=2), params(mode=(1, 5)), params(alpha_channel=(0, 2)),
                params(source=(1, 4)), params(stride=FW - 1)):
        assert call(bad) == -1, L.jxlhip_last_error(dec.ctx)
    null = params()
    null.planes[1] = None
    assert call(null) == -1
    assert L.jxlhip_set_blending_extra(dec.ctx, None) == -1
    # a source slot that holds an XYB frame, a source canvas smaller than the image
    sheet = (np.random.default_rng(3).standard_normal((3, 18, 20)) * 0.2).astype(np.float32)
    dec.set_reference_frame(2, sheet)
    assert call(params(source=(1, 2))) == -1 and b"XYB reference frame" in L.jxlhip_last_error(dec.ctx)
    bench.save("A", 201, 2, k, f, 3)
    bench.begin("B", k, f)
    dec.set_blending((w, H), (37, 21), abi.BLEND_BLEND, False, 0, None)
    assert call(params(source=(1, 3))) == -1 and b"smaller" in L.jxlhip_last_error(dec.ctx)
    # set_alpha is neither needed nor allowed; upsampled frames and frames with patches stay outside
    assert call(params()) == 0
    assert L.jxlhip_set_alpha(dec.ctx, planes[0].ctypes.data, FW) == -7
    bench.begin("B", k, f)
    dec.set_upsampling(2, (143, 80))
    dec.set_blending((w, H), (37, 21), abi.BLEND_BLEND, False, 0, None)
    assert call(params()) == -7 and b"upsampled" in L.jxlhip_last_error(dec.ctx)
    dec.set_reference_frame(2, sheet)
    bench.begin("B", k, f)
    dec.set_patches([dict(ref=2, ref_x0=2, ref_y0=1, xsize=12, ysize=9, x=30, y=20, mode=2, alpha_channel=0, clamp=0)])
    dec.set_blending((w, H), (37, 21), abi.BLEND_BLEND, False, 0, None)
    assert call(params()) == -7 and b"patches" in L.jxlhip_last_error(dec.ctx)
    # a multi-device context
    ctx = C.c_void_p()
    assert L.jxlhip_create_multi((C.c_int * 2)(0, 0), 2, None, C.byref(ctx)) == 0
    try:
        wv, hv = C.c_uint32(), C.c_uint32()
        assert L.jxlhip_set_blending_extra(ctx, C.byref(params())) == -7
        assert L.jxlhip_canvas_read_extra(ctx, 0, 0, None, 0, C.byref(wv), C.byref(hv)) == -7
    finally:
        L.jxlhip_destroy(ctx)
    # canvas_read_extra: bad slot / channel / stride
    wv, hv = C.c_uint32(), C.c_uint32()
    assert L.jxlhip_canvas_read_extra(dec.ctx, 4, 0, None, 0, C.byref(wv), C.byref(hv)) == -1
    assert L.jxlhip_canvas_read_extra(dec.ctx, 3, 4, None, 0, C.byref(wv), C.byref(hv)) == -1
    assert L.jxlhip_canvas_read_extra(dec.ctx, 3, 1, C.c_void_p(out.data_ptr()), 200, C.byref(wv), C.byref(hv)) == -1
    assert (wv.value, hv.value) == (201, H)
    dec.sync()


@pytest.mark.gpu
def test_a_slot_given_an_xyb_frame_loses_its_planes(bench):
    k, f = OUTS["linear"]
    dec = bench.dec
    sheet = (np.random.default_rng(3).standard_normal((3, 18, 20)) * 0.2).astype(np.float32)
    bench.save("A", 202, 3, k, f, 1)
    assert same(bench.canvas_planes(1, 3), bench.planes[("A", 202)][:3]) and same(bench.canvas(1), bench.direct(("A", 202), k, f))
    dec.set_reference_frame(1, sheet)
    assert bench.canvas(1) is None and all(dec.read_canvas_extra(1, i) is None for i in range(4))
    # ... and a canvas saved without extra channels has none
    bench.save("A", 202, 2, k, f, 1)
    bench.begin(("A", 202), k, f)
    dec.set_blending((202, H), (0, 0), abi.BLEND_REPLACE, False, 0, 1)
    dec.decode_frame(out=False)
    assert bench.canvas(1) is not None and dec.read_canvas_extra(1, 0) is None
    dec.set_reference_frame(1, None)


# ---- files, through jxlhip_decode_codestream_next ---------------------------------------------------------------------

TIGHT = 2e-5


@pytest.fixture(scope="module")
def kit(oracle):
    """test_alpha_blending_model's files, and JxlDecoder's coalesced RGBA frames of them, computed once."""
    import layer_streams as ls
    import test_alpha_blending_model as tm
    k = tm.make_kit(oracle)
    files = {name: tm.build_case(k, name)[0] for name in sorted(tm.CASES)}
    truth = {}
    for name, cs in files.items():
        truth[name] = ls.jxl_decode_frames(k[1], cs, channels=4)
        for px, _ in truth[name]:
            px.setflags(write=False)
    return k[0], k[1], files, truth, k[2]


def next_frames(L, dec, cs, sample, workers=0):
    """Every displayed frame of a file as RGBA through jxlhip_decode_codestream_next: [(pixels, abi.SequenceFrame)]."""
    import torch
    from test_gpu_patches import _runner
    R, pool, runner = _runner(workers)
    try:
        info, seq = abi.CodestreamInfo(), abi.SequenceInfo()
        assert L.jxlhip_codestream_sequence_info_ex(cs, len(cs), abi.SEQUENCE_EXTRA_CHANNELS, C.byref(info), C.byref(seq)) == 0, seq.why
        tf = {8: abi.TF_LINEAR, 13: abi.TF_SRGB}[info.transfer_function]  # the blend happens in the original's encoding
        st = abi.SAMPLE_F32 if sample == "f32" else abi.SAMPLE_U8
        fmt = abi.OutputFormat(tf, st, 4, 32 if sample == "f32" else 8, 0, 0.0, info.luminances)
        out = torch.full((info.ysize, info.xsize, 4), 77, dtype=torch.float32 if sample == "f32" else torch.uint8, device="cuda")
        cursor, got = C.c_uint64(0), []
        for k in range(seq.num_displayed_frames):
            fr = abi.SequenceFrame()
            rc = L.jxlhip_decode_codestream_next(dec.ctx, runner, pool, cs, len(cs), C.byref(cursor), 2 | abi.OUT_BLEND_EXTRA_CHANNELS,
                                                 C.byref(fmt), out.data_ptr(), info.xsize * 4 * out.element_size(), 0, None, C.byref(fr))
            assert rc == 0, L.jxlhip_last_error(dec.ctx)
            assert fr.index == k and fr.is_last == int(k + 1 == seq.num_displayed_frames)
            got.append((out.cpu().numpy(), fr))
        assert cursor.value == len(cs)
        return got
    finally:
        if pool:
            R.JxlThreadParallelRunnerDestroy(pool)


@pytest.mark.gpu
@pytest.mark.parametrize("workers", [0, 6])
def test_file_frames_match_jxldecoder(kit, workers):
    """Bound: TIGHT relative to the frame's range and 1 level at 8 bit, as tests/test_gpu_blending.py's files.  Measured on
    an MI355X, all files, both worker counts: colour max|diff| / scale 1.3e-6 .. 2.6e-6, alpha 0, at most 1 level at 8
    bit ("Blending with extra channels")."""
    from libjxl_amd import VarDctDecoder
    L, RL, files, truth, _ = kit
    dec = VarDctDecoder(0)
    worst = [0.0, 0.0]
    try:
        for name in sorted(files):
            got = next_frames(L, dec, files[name], "f32", workers)
            got8 = next_frames(L, dec, files[name], "u8", workers)
            assert len(got) == len(truth[name]) == 1
            for k, ((px, fr), (px8, _), (want, head)) in enumerate(zip(got, got8, truth[name])):
                scale = max(1.0, float(np.abs(want).max()))
                err = float(np.abs(px - want).max()) / scale
                erra = float(np.abs(px[..., 3] - want[..., 3]).max())
                # (the alpha planes are decoded losslessly on the host and blended with the reference's arithmetic)
                assert erra == 0.0, (name, k)
                err8 = float(np.abs(px8.astype(np.float32) - np.round(np.clip(want, 0.0, 1.0) * 255.0)).max())
                print("%s frame %d workers %d: max|diff| / scale = %.3e (alpha %.3e), 8-bit levels %g" % (name, k, workers, err, erra, err8))
                worst = [max(worst[0], err), max(worst[1], err8)]
                assert err <= TIGHT, (name, k)
                assert err8 <= 1.0, (name, k)
                assert (fr.duration, fr.timecode, fr.is_last, fr.name_length) == (head["duration"], head["timecode"], head["is_last"],
                                                                                  head["name_length"]), (name, k)
                # (coalescing, JxlDecoder reports the image's size; jxlhip_sequence_frame the frame's own rectangle)
                assert (head["xsize"], head["ysize"]) == (203, 67) and (fr.xsize, fr.ysize) == (72, 40) and fr.have_crop == 1, (name, k)
    finally:
        dec.close()
    print("worst over the files, workers %d: %.3e relative, %g levels at 8 bit" % (workers, worst[0], worst[1]))


@pytest.mark.gpu
def test_sequence_saves_the_planes_and_still_refuses(kit):
    import torch
    import alpha_layer_streams as als
    from libjxl_amd import VarDctDecoder
    L, RL, files, truth, streams = kit
    s8 = streams[8]
    fmt = abi.OutputFormat(abi.TF_SRGB, abi.SAMPLE_F32, 4, 32, 0, 0.0, (C.c_float * 3)(0.2126, 0.7152, 0.0722))
    out = torch.empty((67, 203, 4), dtype=torch.float32, device="cuda")

    def call(dec, data, cursor, frame=None, kind=2 | abi.OUT_BLEND_EXTRA_CHANNELS):
        return L.jxlhip_decode_codestream_next(dec.ctx, None, None, data, len(data), C.byref(cursor), kind, C.byref(fmt), out.data_ptr(),
                                               203 * 16, 0, None, frame)

    def why(data, flags=abi.SEQUENCE_EXTRA_CHANNELS):
        info, seq = abi.CodestreamInfo(), abi.SequenceInfo()
        return L.jxlhip_codestream_sequence_info_ex(data, len(data), flags, C.byref(info), C.byref(seq)), seq.why or b""

    dec = VarDctDecoder(0)
    try:
        # the chain: frames 1 and 2 are blended into slot 1 with their alpha; the last frame leaves the slot as it was
        cs = files["chain-of-three"]
        cursor, fr = C.c_uint64(0), abi.SequenceFrame()
        dec.profile(True)
        assert call(dec, cs, cursor, C.byref(fr)) == 0, L.jxlhip_last_error(dec.ctx)
        slots = dec.profile_read()
        dec.profile(False)
        assert slots["blend_ec"][1] == 4 and "blend" not in slots, slots
        assert (fr.coded_frames, fr.is_last, fr.have_crop, fr.x0, fr.y0, fr.blend_mode, fr.blend_source) == (4, 1, 1, 170, 50, 2, 1)
        assert dec.read_canvas(1) is not None and dec.read_canvas_extra(1, 0) is not None and dec.read_canvas_extra(1, 1) is None
        assert float(dec.read_canvas_extra(1, 0).min()) == 0.0 and float(dec.read_canvas_extra(1, 0).max()) == 1.0
        # a caller that does not ask for it gets the refusal it always got, from both calls
        needs = b"a frame that needs blending on an image with extra channels"
        assert why(cs, 0) == (-7, needs) and why(cs)[0] == 0 and why(cs, 2)[0] == -1
        assert call(dec, cs, C.c_uint64(0), kind=2) == -7 and needs in L.jxlhip_last_error(dec.ctx)
        # the single-frame calls keep refusing a sequence
        assert L.jxlhip_decode_codestream(dec.ctx, None, None, cs, len(cs), 2, C.byref(fmt), out.data_ptr(), 203 * 16, 0, None) == -7
        # patches and upsampling on an image with extra channels, with their reasons
        a, b = s8["A"], s8["B"]
        import layer_streams as ls
        assert why(ls.splice(L, a, [dict(stream=a, save_as_reference=1), dict(stream=a, flags_or=2)])) == \
            (-7, b"patches on an image with extra channels")
        rc, reason = why(als.splice_ec(L, a, [dict(stream=a, save_as_reference=1), dict(stream=b, crop=(37, 21), source=1, upsampling=2)]))
        assert rc == -7 and b"upsampled frame on an image with extra channels" in reason
        # tone mapping behind a blend
        try:
            dec.set_display(100.0)
            assert call(dec, files["blend-8-clamp0"], C.c_uint64(0)) == -7
            assert b"needs blending while display_nits is set" in L.jxlhip_last_error(dec.ctx)
        finally:
            dec.set_display()
    finally:
        dec.close()


# ---- the command-line tool -------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_djxl_hip_frames_writes_rgba(kit, tmp_path):
    """tools/djxl_hip.py --frames OUT.pam on a layered still with alpha: one RGBA file, colour and blended alpha at most
    one level from JxlDecoder's coalesced frame."""
    import os
    import subprocess
    import sys
    from test_djxl import read_pam
    L, RL, files, truth, _ = kit
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "layers.jxl"
    src.write_bytes(files["chain-of-three"])
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "djxl_hip.py"), str(src), str(tmp_path / "f.pam"), "--frames",
                        "--threads", "4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    px, mx = read_pam(str(tmp_path / "f-000.pam"))
    want = truth["chain-of-three"][0][0]
    assert mx == 255 and px.shape == (67, 203, 4) and not os.path.exists(tmp_path / "f-001.pam")
    want8 = np.clip(np.rint(want * 255.0), 0, 255).astype(np.int32)  # (undithered: the tool's samples are dithered by < 1 level)
    assert int(np.abs(px.astype(np.int32) - want8).max()) <= 1
    assert len(np.unique(px[..., 3])) >= 5  # a real alpha plane
