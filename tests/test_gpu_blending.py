"""Blending on the device (jxlhip_set_blending, jxlhip_canvas_read, kernels_blend.hip): canvas slots, k_blend against
tests/blending_model.py, the packing of the blended frame, the frame's own render stages in front of the blend, and the
refused configurations.

The kernel tests use synthetic frames: frame A, canvas-sized, is saved into a slot; frame B is decoded with blending on.
The caller's buffer and the saved canvas must each be BIT-EQUAL to the model applied to the SAME decoder's direct packed
float outputs of A and B -- every blended sample is one IEEE operation, and the frame's own path is the same launches
both times.

Smallest shapes that can still go wrong: a 203 x 137 canvas (no multiple of 4, 16 or 64; 51 four-pixel groups of which
the last holds three pixels; more than one workgroup), frames of 72 x 40 and 9 x 5 at origins inside, at (0, 0), negative,
overhanging right and bottom and wholly outside, and a 260 x 150 frame that covers the canvas from (-30, -7)."""
import ctypes as C

import numpy as np
import pytest

from libjxl_amd import abi, synth

import blending_model as bm
import output_sweep as osw

W, H = 203, 137
ORIGINS = [(0, 0), (37, 21), (-20, -9), (170, 120), (210, 0)]
PLACEMENTS = [(name, o) for name in ("B", "S") for o in ORIGINS] + [("L", (-30, -7))]
FRAME_SIZES = {"A": (W, H), "A2": (W, H), "B": (72, 40), "S": (9, 5), "L": (260, 150)}
SEEDS = {"A": 11, "A2": 12, "B": 13, "S": 14, "L": 15}
SRGB_F32 = osw.fmt(abi.TF_SRGB, abi.SAMPLE_F32, 3)
KINDS = {"linear": (1, None), "srgb": (2, SRGB_F32)}
SENTINEL = {np.dtype(np.float32): -7.0, np.dtype(np.uint8): 0xA5, np.dtype(np.int16): 0x5A5A}


def float_format(f):
    """The format the frame is staged in: float RGB in f's transfer function."""
    return None if f is None else dict(f, sample_type=abi.SAMPLE_F32, num_channels=3, bits_per_sample=0, swap_endianness=0)


class Bench:
    """One decoder, the synthetic frames, and the decoder's direct outputs of them (computed once per format, read-only)."""

    def __init__(self):
        from libjxl_amd import VarDctDecoder
        self.dec = VarDctDecoder(0)
        self.dq = self.dec.default_dequant_tables()
        self.inputs = {}
        self.direct_cache = {}
        for name, (w, h) in FRAME_SIZES.items():
            # (frames B, S, L brighter and rougher: some per cent of their samples above 1 and below 0, so that kMul's
            # clamp shows)
            kw = {} if name in ("A", "A2") else dict(intensity_target=60.0, amp=30.0)
            self.inputs[name] = synth.synth_frame(w, h, device="cuda", seed=SEEDS[name], gab=True, epf_iters=1, **kw)

    def close(self):
        self.dec.close()

    def params(self, name, kind, f):
        p = dict(self.inputs[name][0], output_kind=kind, out_format=f)
        return p

    def begin(self, name, kind, f, stages=None):
        dec = self.dec
        dec.begin_frame(self.params(name, kind, f))
        dec.set_inputs(self.inputs[name][1], self.dq)
        for call, args in (stages or []):
            getattr(dec, call)(*args)

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

    def save(self, name, kind, f, slot):
        """Frame `name` (canvas-sized) saved into `slot` and not written anywhere else."""
        self.begin(name, kind, f)
        self.dec.set_blending((W, H), (0, 0), abi.BLEND_REPLACE, False, 0, slot)
        assert self.dec.decode_frame(out=False) is None

    def blend(self, name, kind, f, origin, mode, clamp, source, save_slot, stages=None, image=(W, H)):
        """Frame `name` blended into a sentinel-filled buffer with padded rows; returns the caller's region."""
        import torch
        self.begin(name, kind, f, stages)
        self.dec.set_blending(image, origin, mode, clamp, source, save_slot)
        like = self.dec.alloc_output()
        shape, dt = tuple(like.shape), like.dtype
        assert shape[:2] == (image[1], image[0])
        s = SENTINEL[np.dtype(str(dt).split(".")[1])]
        buf = torch.full((shape[0] + 1, shape[1] + 5, shape[2]), s, dtype=dt, device="cuda")
        self.dec.decode_frame(buf[:shape[0], :shape[1]])
        self.dec.sync()
        raw = buf.cpu().numpy()
        # the row padding and the row behind the last one are the caller's
        assert np.all(raw[:shape[0], shape[1]:] == s) and np.all(raw[shape[0]:] == s)
        return np.ascontiguousarray(raw[:shape[0], :shape[1]])

    def canvas(self, slot):
        t = self.dec.read_canvas(slot)
        return None if t is None else t.cpu().numpy()


@pytest.fixture(scope="module")
def bench():
    b = Bench()
    yield b
    b.close()


def same(got, want):
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- the kernel against the model -----------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["linear", "srgb"])
@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("mode", bm.MODES)
def test_blend_kernel_is_bit_equal_to_the_model(bench, mode, clamp, kind):
    k, f = KINDS[kind]
    a = bench.direct("A", k, f)
    for i, (name, origin) in enumerate(PLACEMENTS):
        fg = bench.direct(name, k, f)
        want = bm.blend(a, fg, origin, mode, clamp)
        for how in ("same", "other", "none"):
            src = i % 4
            save = {"same": src, "other": (src + 1) % 4, "none": None}[how]
            bench.save("A", k, f, src)
            if save is not None and save != src:
                bench.dec.set_reference_frame(save, None)
            got = bench.blend(name, k, f, origin, mode, clamp, src, save)
            what = (name, origin, how)
            assert same(got, want), what  # (every canvas pixel written: the sentinel is no value of the model's)
            if save is not None:
                assert same(bench.canvas(save), want), what
            if save != src:
                assert same(bench.canvas(src), a), what  # the source slot is read only
    # the inputs are worth the test: the frame shows, and the clamp matters
    fg = bench.direct("B", k, f)
    assert float(fg.max()) > 1.0 and float(fg.min()) < 0.0
    assert not np.array_equal(bm.blend(a, fg, (37, 21), bm.MUL, True), bm.blend(a, fg, (37, 21), bm.MUL, False))
    assert not np.array_equal(bm.blend(a, fg, (37, 21), mode, clamp), a)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", bm.MODES)
def test_empty_source_is_zeroes(bench, mode):
    k, f = KINDS["srgb"]
    for slot in range(4):
        bench.dec.set_reference_frame(slot, None)
    for name, origin in PLACEMENTS:
        fg = bench.direct(name, k, f)
        want = bm.blend(None, fg, origin, mode, True, size=(W, H))
        bench.dec.set_reference_frame(2, None)
        assert bench.canvas(2) is None
        assert same(bench.blend(name, k, f, origin, mode, True, 2, None), want), (name, origin)
        assert bench.canvas(2) is None  # not saved
        # saved into the empty source slot itself: the whole canvas is written, zeroes outside the rectangle
        assert same(bench.blend(name, k, f, origin, mode, True, 2, 2), want), (name, origin)
        assert same(bench.canvas(2), want), (name, origin)


@pytest.mark.gpu
def test_chain_of_three_blends(bench):
    k, f = KINDS["srgb"]
    a, b, s = (bench.direct(n, k, f) for n in ("A", "B", "S"))
    for slot in range(4):
        bench.dec.set_reference_frame(slot, None)
    bench.save("A", k, f, 1)
    want1 = bm.blend(a, b, (37, 21), bm.ADD)
    got1 = bench.blend("B", k, f, (37, 21), bm.ADD, False, 1, 1)
    want2 = bm.blend(want1, b, (-20, -9), bm.MUL, True)
    got2 = bench.blend("B", k, f, (-20, -9), bm.MUL, True, 1, 2)
    want3 = bm.blend(want2, s, (170, 120), bm.ADD)
    got3 = bench.blend("S", k, f, (170, 120), bm.ADD, False, 2, 2)
    assert same(got1, want1) and same(got2, want2) and same(got3, want3)
    assert same(bench.canvas(1), want1) and same(bench.canvas(2), want3)
    assert bench.canvas(0) is None and bench.canvas(3) is None
    # a layer nobody displays: blended into its slot without an output buffer
    bench.begin("S", k, f)
    bench.dec.set_blending((W, H), (0, 0), abi.BLEND_ADD, False, 2, 2)
    bench.dec.decode_frame(out=False)
    assert same(bench.canvas(2), bm.blend(want3, s, (0, 0), bm.ADD))


@pytest.mark.gpu
def test_a_second_canvas_replaces_the_first(bench):
    k, f = KINDS["linear"]
    bench.save("A", k, f, 0)
    bench.save("A2", k, f, 0)
    assert same(bench.canvas(0), bench.direct("A2", k, f))
    assert not np.array_equal(bench.direct("A", k, f), bench.direct("A2", k, f))


@pytest.mark.gpu
def test_blend_launch_is_profiled_and_full_replace_launches_nothing_more(bench):
    k, f = KINDS["srgb"]
    dec = bench.dec
    bench.save("A", k, f, 0)
    dec.profile(True)
    try:
        bench.blend("B", k, f, (37, 21), bm.ADD, False, 0, 0)
        slots = dec.profile_read()
        assert slots["blend"][1] == 1, slots
        # a layer wholly outside the image, blended into its own source slot without a caller's buffer: nothing is
        # visited, nothing is launched, and no span is reported
        before = bench.canvas(0)
        bench.begin("B", k, f)
        dec.set_blending((W, H), (210, 0), abi.BLEND_ADD, False, 0, 0)
        dec.decode_frame(out=False)
        assert "blend" not in dec.profile_read() and same(bench.canvas(0), before)
        # full frame, kReplace / kBlend, no save slot: exactly the launches of the frame without blending
        bench.begin("A", k, f)
        dec.decode_frame()
        plain = dec.profile_read()
        for mode in (bm.REPLACE, bm.BLEND):
            got = bench.blend("A", k, f, (0, 0), mode, False, 0, None)
            slots = dec.profile_read()
            assert "blend" not in slots and {n: v[1] for n, v in slots.items()} == {n: v[1] for n, v in plain.items()}, slots
            assert same(got, bench.direct("A", k, f))
    finally:
        dec.profile(False)
    # the first eight slots are what jxlhip_profile_read reports, as before
    assert abi.KERNEL_COUNT == 8 and abi.KERNEL_NAMES_EX[9] == "blend" and abi.KERNEL_COUNT_EX >= 10


# ---- packing ----------------------------------------------------------------------------------------------------------

PACKED = osw.FIXED_LIST + [osw.GENERAL_LIST[0], osw.GENERAL_LIST[2]]


def _native(raw):
    return raw.view(np.uint16) if raw.dtype == np.int16 else raw


@pytest.mark.gpu
@pytest.mark.parametrize("f", PACKED, ids=osw.fmt_id)
def test_blended_frame_is_packed_like_the_output_stage(bench, oracle, f):
    """The caller's bytes = the oracle's sample conversion (dither at canvas coordinates, clamp, rounding, half floats,
    byte swap, opaque alpha) of the blended float frame with the transfer function switched off: the samples were
    encoded before the blend."""
    a, b = bench.direct("A", 2, f), bench.direct("B", 2, f)
    bench.save("A", 2, f, 3)
    assert same(bench.canvas(3), a)
    for origin, mode, save in (((37, 21), bm.ADD, 3), ((-20, -9), bm.MUL, None), ((170, 120), bm.REPLACE, 0)):
        bench.save("A", 2, f, 3)
        blended = bm.blend(a, b, origin, mode, True)
        got = _native(bench.blend("B", 2, f, origin, mode, True, 3, save))
        want = oracle.pack_output(dict(f, transfer=abi.TF_LINEAR), blended)
        assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (origin, mode)
        if save is not None:
            assert same(bench.canvas(save), blended)


@pytest.mark.gpu
@pytest.mark.parametrize("f", PACKED, ids=osw.fmt_id)
def test_saving_a_full_replace_frame_does_not_change_its_bytes(bench, f):
    dec = bench.dec
    for slot in range(4):
        dec.set_reference_frame(slot, None)
    bench.begin("A", 2, f)
    plain = dec.decode_frame()
    dec.sync()
    plain = plain.cpu().numpy()
    got = bench.blend("A", 2, f, (0, 0), bm.REPLACE, False, 1, 2)
    assert np.array_equal(got.view(np.uint8), plain.view(np.uint8))
    assert same(bench.canvas(2), bench.direct("A", 2, f))


# ---- the frame's own stages in front of the blend -----------------------------------------------------------------------

def _stage_cases():
    from test_splines_front_end import built_sets
    lut = [0.05, 0.12, 0.3, 0.45, 0.6, 0.75, 0.9, 1.0]
    sets = built_sets(72, 40)
    sheet = (np.random.default_rng(3).standard_normal((3, 18, 20)) * 0.2).astype(np.float32)
    patches = [dict(ref=3, ref_x0=2, ref_y0=1, xsize=12, ysize=9, x=30, y=20, mode=2, alpha_channel=0, clamp=0),
               dict(ref=3, ref_x0=0, ref_y0=0, xsize=5, ysize=4, x=67, y=36, mode=1, alpha_channel=0, clamp=0)]
    return {"noise": ("B", [("set_noise", (lut, 3, 2))], None),
            "splines": ("B", [("set_splines", (sets["edge"] + sets["tiny"],))], None),
            "patches": ("B", [("set_patches", (patches,))], sheet),
            "upsampling": ("B", [("set_upsampling", (2, (143, 80)))], None)}


@pytest.mark.gpu
@pytest.mark.parametrize("stage", ["noise", "splines", "patches", "upsampling"])
def test_render_stages_run_in_front_of_the_blend(bench, stage):
    k, f = KINDS["srgb"]
    name, stages, sheet = _stage_cases()[stage]
    dec = bench.dec
    for slot in range(4):
        dec.set_reference_frame(slot, None)
    if sheet is not None:
        dec.set_reference_frame(3, sheet)  # an XYB frame in slot 3, the canvas in slot 0
    a, plain = bench.direct("A", k, f), bench.direct(name, k, f)
    bench.begin(name, k, float_format(f), stages)
    fg = dec.decode_frame()
    dec.sync()
    fg = fg.cpu().numpy()
    assert fg.shape == ((80, 143, 3) if stage == "upsampling" else plain.shape)
    if stage != "upsampling":
        assert np.abs(fg - plain).max() > 1e-3  # the stage is there
    dec.profile(True)
    try:
        bench.save("A", k, f, 0)
        dec.profile_read()
        for origin, mode in (((37, 21), bm.ADD), ((-20, -9), bm.REPLACE), ((100, 70), bm.MUL)):
            bench.save("A", k, f, 0)
            got = bench.blend(name, k, f, origin, mode, False, 0, 0, stages)
            slots = dec.profile_read()
            want = bm.blend(a, fg, origin, mode, False)
            assert same(got, want), (stage, origin)
            assert same(bench.canvas(0), want), (stage, origin)
            assert {"noise": "noise", "splines": "splines", "patches": "patches", "upsampling": "upsample"}[stage] in slots
    finally:
        dec.profile(False)


# ---- state and refusals -----------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_slots_hold_one_kind_at_a_time(bench):
    L = bench.dec.L
    k, f = KINDS["linear"]
    dec = bench.dec
    sheet = (np.random.default_rng(3).standard_normal((3, 18, 20)) * 0.2).astype(np.float32)
    for slot in range(4):
        dec.set_reference_frame(slot, None)
    bench.save("A", k, f, 1)
    assert bench.canvas(1) is not None
    # set_patches refuses a slot that holds a canvas
    rc, h = abi.patches_from_list([dict(ref=1, ref_x0=0, ref_y0=0, xsize=2, ysize=2, x=1, y=1, mode=2, alpha_channel=0,
                                        clamp=0)], 72, 40, {1: (W, H)}, L=L)
    assert rc == 0
    try:
        bench.begin("B", k, f)
        assert L.jxlhip_set_patches(dec.ctx, h) == -1 and b"after the colour transform" in L.jxlhip_last_error(dec.ctx)
        # an XYB frame stored in the slot drops the canvas; a canvas saved into it drops the XYB frame
        dec.set_reference_frame(1, sheet)
        assert bench.canvas(1) is None
        # ... and an XYB frame is no blend source
        bench.begin("B", k, f)
        dec.set_blending((W, H), (0, 0), abi.BLEND_ADD, False, 1, None)
        out = dec.alloc_output()
        assert L.jxlhip_decode_frame(dec.ctx, *dec._out_args(out)) == -1
        assert b"XYB reference frame" in L.jxlhip_last_error(dec.ctx)
        bench.save("A", k, f, 1)
        bench.begin("B", k, f)
        assert L.jxlhip_set_patches(dec.ctx, h) == -1 and b"after the colour transform" in L.jxlhip_last_error(dec.ctx)
        # set_reference_frame(slot, nothing) clears a canvas
        dec.set_reference_frame(1, None)
        assert bench.canvas(1) is None
        bench.begin("B", k, f)
        assert L.jxlhip_set_patches(dec.ctx, h) == -1 and b"empty" in L.jxlhip_last_error(dec.ctx)
    finally:
        abi.patches_destroy(h, L)


@pytest.mark.gpu
def test_frame_begin_and_null_switch_blending_off(bench):
    k, f = KINDS["linear"]
    dec = bench.dec
    bench.save("A", k, f, 0)
    b = bench.direct("B", k, f)
    bench.begin("B", k, f)
    dec.set_blending((W, H), (37, 21), abi.BLEND_ADD, False, 0, 0)
    dec.set_blending(None)
    out = dec.decode_frame()
    dec.sync()
    assert same(out.cpu().numpy(), b)
    bench.begin("B", k, f)
    dec.set_blending((W, H), (37, 21), abi.BLEND_ADD, False, 0, 0)
    bench.begin("B", k, f)  # (a new frame_begin resets it)
    dec.image_size = None
    out = dec.decode_frame()
    dec.sync()
    assert same(out.cpu().numpy(), b)
    assert same(bench.canvas(0), bench.direct("A", k, f))


@pytest.mark.gpu
def test_host_frame_path_is_image_sized(bench):
    k, f = KINDS["srgb"]
    dec, L = bench.dec, bench.dec.L
    a, b = bench.direct("A", k, f), bench.direct("B", k, f)
    bench.save("A", k, f, 0)
    bench.begin("B", k, f)
    dec.set_blending((W, H), (170, 120), abi.BLEND_ADD, False, 0, None)
    host = np.full((H, W + 2, 3), -7.0, np.float32)
    assert L.jxlhip_decode_frame_host(dec.ctx, host.ctypes.data, (W + 2) * 12, 0) == 0, L.jxlhip_last_error(dec.ctx)
    assert same(np.ascontiguousarray(host[:, :W]), bm.blend(a, b, (170, 120), bm.ADD)) and np.all(host[:, W:] == -7.0)
    assert L.jxlhip_decode_frame_host(dec.ctx, host.ctypes.data, W * 12 - 4, 0) == -1  # too small for the IMAGE


@pytest.mark.gpu
def test_refused_configurations(bench):
    import torch
    L, dec = bench.dec.L, bench.dec
    k, f = KINDS["srgb"]
    bp = abi.BlendParams(W, H, 0, 0, abi.BLEND_ADD, 0, 0, abi.BLEND_NO_SAVE)
    ctx = C.c_void_p()
    devs = (C.c_int * 2)(0, 0)
    assert L.jxlhip_create_multi(devs, 2, None, C.byref(ctx)) == 0
    try:
        w, h = C.c_uint32(), C.c_uint32()
        assert L.jxlhip_set_blending(ctx, C.byref(bp)) == -7 and b"multi-device" in L.jxlhip_last_error(ctx)
        assert L.jxlhip_canvas_read(ctx, 0, None, 0, C.byref(w), C.byref(h)) == -7
    finally:
        L.jxlhip_destroy(ctx)
    from libjxl_amd import VarDctDecoder
    fresh = VarDctDecoder(0)
    try:
        assert L.jxlhip_set_blending(fresh.ctx, C.byref(bp)) == -6  # before frame_begin
    finally:
        fresh.close()
    for slot in range(4):
        dec.set_reference_frame(slot, None)
    big, t = synth.synth_frame(300, 520, device="cuda", output_kind=1, gab=True, epf_iters=1)
    dec.begin_frame(dict(big, stripe_group_y0=1, stripe_group_rows=1))
    assert L.jxlhip_set_blending(dec.ctx, C.byref(bp)) == -7 and b"stripes" in L.jxlhip_last_error(dec.ctx)
    dec.begin_frame(dict(big, undo_orientation=6))
    assert L.jxlhip_set_blending(dec.ctx, C.byref(bp)) == -7 and b"undo_orientation" in L.jxlhip_last_error(dec.ctx)
    dec.begin_frame(dict(big, output_kind=0))
    assert L.jxlhip_set_blending(dec.ctx, C.byref(bp)) == -7 and b"planar XYB" in L.jxlhip_last_error(dec.ctx)
    # alpha on a blended frame, either way round
    rgba = osw.fmt(abi.TF_SRGB, abi.SAMPLE_U8, 4)
    alpha = np.ones((40, 72), np.float32)
    bench.begin("B", 2, rgba)
    dec.set_alpha(alpha)
    assert L.jxlhip_set_blending(dec.ctx, C.byref(bp)) == -7 and b"alpha" in L.jxlhip_last_error(dec.ctx)
    bench.begin("B", 2, rgba)
    assert L.jxlhip_set_blending(dec.ctx, C.byref(bp)) == 0
    assert L.jxlhip_set_alpha(dec.ctx, alpha.ctypes.data, 72) == -7 and b"blended frame" in L.jxlhip_last_error(dec.ctx)
    # the split calls
    bench.begin("B", k, f)
    assert L.jxlhip_set_blending(dec.ctx, C.byref(bp)) == 0
    dec.decode_blocks()
    out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    assert L.jxlhip_decode_filters(dec.ctx, C.c_void_p(out.data_ptr()), W * 12, 0) == -7
    assert b"split calls" in L.jxlhip_last_error(dec.ctx)
    assert L.jxlhip_decode_filters_rows(dec.ctx, C.c_void_p(out.data_ptr()), W * 12, 0, 0, 40) == -7
    assert L.jxlhip_stripe_finish(dec.ctx, None, None, C.c_void_p(out.data_ptr()), W * 12, 0, 0, 0) == -7
    # bad arguments
    bench.begin("B", k, f)
    for bad in (abi.BlendParams(0, H, 0, 0, 1, 0, 0, 0), abi.BlendParams(W, H, 0, 0, 5, 0, 0, 0),
                abi.BlendParams(W, H, 0, 0, 1, 0, 4, 0), abi.BlendParams(W, H, 0, 0, 1, 0, 0, 4)):
        assert L.jxlhip_set_blending(dec.ctx, C.byref(bad)) == -1
    # neither an output nor a save slot; an output too small for the image; a source canvas smaller than the image
    assert L.jxlhip_set_blending(dec.ctx, C.byref(bp)) == 0
    assert L.jxlhip_decode_frame(dec.ctx, None, 0, 0) == -1
    assert L.jxlhip_decode_frame(dec.ctx, C.c_void_p(out.data_ptr()), W * 12 - 4, 0) == -1
    bench.save("A", k, f, 0)
    bench.begin("B", k, f)
    larger = abi.BlendParams(W + 1, H, 0, 0, abi.BLEND_ADD, 0, 0, abi.BLEND_NO_SAVE)
    assert L.jxlhip_set_blending(dec.ctx, C.byref(larger)) == 0
    out2 = torch.empty((H, W + 1, 3), dtype=torch.float32, device="cuda")
    assert L.jxlhip_decode_frame(dec.ctx, C.c_void_p(out2.data_ptr()), (W + 1) * 12, 0) == -1
    assert b"smaller" in L.jxlhip_last_error(dec.ctx)
    # ... while a larger source canvas serves a smaller image (read only)
    a, b = bench.direct("A", k, f), bench.direct("B", k, f)
    got = bench.blend("B", k, f, (37, 21), bm.ADD, False, 0, 1, image=(W - 3, H - 2))
    want = bm.blend(a, b, (37, 21), bm.ADD, size=(W - 3, H - 2))
    assert same(got, want) and same(bench.canvas(1), want) and same(bench.canvas(0), a)
    # canvas_read: bad slot, bad stride
    w, h = C.c_uint32(), C.c_uint32()
    assert L.jxlhip_canvas_read(dec.ctx, 4, None, 0, C.byref(w), C.byref(h)) == -1
    assert L.jxlhip_canvas_read(dec.ctx, 0, C.c_void_p(out.data_ptr()), 3 * W - 1, C.byref(w), C.byref(h)) == -1
    assert (w.value, h.value) == (W, H)
    dec.sync()


# ---- files, through jxlhip_decode_codestream_next ---------------------------------------------------------------------

TIGHT = 2e-5


@pytest.fixture(scope="module")
def kit(oracle):
    """(L, the reference's JxlDecoder library, the files by name): spliced at test time (tests/layer_streams.py), the
    truth is always JxlDecoder on the same bytes, computed once."""
    import os
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
    import layer_streams as ls
    L = abi.load_library()
    fs = lambda name, size=(W, H), seed=5: oracle.feature_stream(name, xsize=size[0], ysize=size[1], seed=seed, distance=1.0)  # noqa: E731
    anim, a, a2, b = fs("animation"), fs("plain"), fs("plain", seed=9), fs("plain", (72, 40), 7)
    nb, nfull = fs("noise", (72, 40), 7), fs("noise", seed=11)
    files = {
        "oracle-animation": anim,
        # full kReplace saved, a crop with kAdd, a crop with kMul and clamp: each blended into its own source slot
        "animation-3": ls.splice(L, anim, [dict(stream=a, duration=3, save_as_reference=1),
                                           dict(stream=b, crop=(37, 21), mode=ls.ADD, source=1, duration=2, save_as_reference=1),
                                           dict(stream=b, crop=(170, 120), mode=ls.MUL, clamp=1, source=1, duration=5)]),
        # a layered still: two zero-duration layers (the second at a negative origin, with noise: non-visible frame 2),
        # then the one displayed frame
        "layers": ls.splice(L, a, [dict(stream=a, save_as_reference=1),
                                   dict(stream=nb, crop=(-20, -9), mode=ls.ADD, source=1, save_as_reference=1),
                                   dict(stream=b, crop=(100, 70), mode=ls.ADD, source=1)]),
        # a noise frame second: visible frame 2
        "noise-second": ls.splice(L, anim, [dict(stream=a2, duration=1, save_as_reference=1), dict(stream=nfull, duration=2)]),
    }
    truth = {}
    for name, cs in files.items():
        truth[name] = ls.jxl_decode_frames(RL, cs)  # (raises when the reference does not accept the file)
        for px, _ in truth[name]:
            px.setflags(write=False)
    assert [len(truth[n]) for n in ("oracle-animation", "animation-3", "layers", "noise-second")] == [1, 3, 1, 2]
    return L, files, truth, dict(modular=fs("modular"), plain=a,
                                 xyb_saved=ls.splice(L, a, [dict(stream=a, save_as_reference=1, save_before_color_transform=1),
                                                            dict(stream=a)]))


def _next_frames(L, dec, cs, sample, workers=0):
    """Every displayed frame of a file through jxlhip_decode_codestream_next: [(pixels, abi.SequenceFrame)]."""
    import torch
    from test_gpu_patches import _runner
    R, pool, runner = _runner(workers)
    try:
        info, seq = abi.CodestreamInfo(), abi.SequenceInfo()
        assert L.jxlhip_codestream_sequence_info(cs, len(cs), C.byref(info), C.byref(seq)) == 0
        assert info.transfer_function == 13  # sRGB: the blend happens in the original's encoding
        st = abi.SAMPLE_F32 if sample == "f32" else abi.SAMPLE_U8
        fmt = abi.OutputFormat(abi.TF_SRGB, st, 3, 32 if sample == "f32" else 8, 0, 0.0, info.luminances)
        out = torch.full((info.ysize, info.xsize, 3), 77, dtype=torch.float32 if sample == "f32" else torch.uint8, device="cuda")
        cursor, got = C.c_uint64(0), []
        for k in range(seq.num_displayed_frames):
            fr = abi.SequenceFrame()
            rc = L.jxlhip_decode_codestream_next(dec.ctx, runner, pool, cs, len(cs), C.byref(cursor), 2, C.byref(fmt), out.data_ptr(),
                                                 info.xsize * 3 * out.element_size(), 0, None, C.byref(fr))
            assert rc == 0, L.jxlhip_last_error(dec.ctx)
            assert fr.index == k and fr.is_last == int(k + 1 == seq.num_displayed_frames)
            got.append((out.cpu().numpy(), fr))
        assert cursor.value == len(cs)
        # a call after the last frame, and a cursor the context does not expect
        assert L.jxlhip_decode_codestream_next(dec.ctx, runner, pool, cs, len(cs), C.byref(cursor), 2, C.byref(fmt), out.data_ptr(),
                                               info.xsize * 3 * out.element_size(), 0, None, None) == -6
        return got
    finally:
        if pool:
            R.JxlThreadParallelRunnerDestroy(pool)


@pytest.mark.gpu
@pytest.mark.parametrize("workers", [0, 6])
@pytest.mark.parametrize("name", ["oracle-animation", "animation-3", "layers", "noise-second"])
def test_file_frames_match_jxldecoder(kit, name, workers):
    from libjxl_amd import VarDctDecoder
    L, files, truth, _ = kit
    dec = VarDctDecoder(0)
    try:
        got = _next_frames(L, dec, files[name], "f32", workers)
        got8 = _next_frames(L, dec, files[name], "u8", workers)
    finally:
        dec.close()
    assert len(got) == len(truth[name])
    for k, ((px, fr), (px8, _), (want, head)) in enumerate(zip(got, got8, truth[name])):
        scale = max(1.0, float(np.abs(want).max()))
        err = float(np.abs(px - want).max()) / scale
        err8 = float(np.abs(px8.astype(np.float32) - np.round(np.clip(want, 0.0, 1.0) * 255.0)).max())
        print("%s frame %d workers %d: max|diff| / scale = %.3e, 8-bit levels %g" % (name, k, workers, err, err8))
        assert err <= TIGHT, (name, k)
        assert err8 <= 1.0, (name, k)
        assert (fr.duration, fr.timecode, fr.is_last, fr.name_length) == (head["duration"], head["timecode"], head["is_last"],
                                                                          head["name_length"]), (name, k)


@pytest.mark.gpu
def test_sequence_state_and_refusals(kit):
    import torch
    from libjxl_amd import VarDctDecoder
    L, files, truth, bad = kit
    cs = files["animation-3"]
    fmt = abi.OutputFormat(abi.TF_SRGB, abi.SAMPLE_F32, 3, 32, 0, 0.0, (C.c_float * 3)(0.2126, 0.7152, 0.0722))
    out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")

    def call(dec, data, cursor, frame=None):
        return L.jxlhip_decode_codestream_next(dec.ctx, None, None, data, len(data), C.byref(cursor), 2, C.byref(fmt), out.data_ptr(),
                                               W * 12, 0, None, frame)

    dec = VarDctDecoder(0)
    try:
        cursor, fr = C.c_uint64(0), abi.SequenceFrame()
        assert call(dec, cs, C.c_uint64(1234)) == -6 and b"no sequence is open" in L.jxlhip_last_error(dec.ctx)
        assert call(dec, cs, cursor, C.byref(fr)) == 0
        assert (fr.index, fr.duration, fr.have_crop, fr.xsize, fr.ysize, fr.save_as_reference, fr.coded_frames) == (0, 3, 0, W, H, 1, 1)
        assert dec.read_canvas(1) is not None  # frame 1 blends over it
        assert call(dec, cs, C.c_uint64(cursor.value + 1)) == -6 and b"expects" in L.jxlhip_last_error(dec.ctx)
        # (the sequence is still open at the cursor it expects; start again all the same)
        cursor = C.c_uint64(0)
        assert call(dec, cs, cursor) == 0 and call(dec, cs, cursor, C.byref(fr)) == 0
        assert (fr.index, fr.have_crop, fr.x0, fr.y0, fr.xsize, fr.ysize, fr.blend_mode, fr.blend_source) == (1, 1, 37, 21, 72, 40, 1, 1)
        # cursor 0 clears the slots: a second file never sees the first file's canvas
        c2 = C.c_uint64(0)
        assert call(dec, bad["plain"], c2) == 0 and c2.value == len(bad["plain"])
        assert all(dec.read_canvas(s) is None for s in range(4))
        assert np.abs(out.cpu().numpy() - truth["animation-3"][0][0]).max() <= TIGHT * 2  # (the same plain frame)
        # the old sequence is gone with it
        assert call(dec, cs, cursor) == -6
        # ... and so is a sequence whose slots the caller empties behind its back (it would blend over zeroes)
        c3 = C.c_uint64(0)
        assert call(dec, cs, c3) == 0
        dec.set_reference_frame(3, None)
        assert call(dec, cs, c3) == -6 and b"no sequence is open" in L.jxlhip_last_error(dec.ctx)
        c3 = C.c_uint64(0)
        assert call(dec, cs, c3) == 0
        assert L.jxlhip_decode_codestream(dec.ctx, None, None, bad["plain"], len(bad["plain"]), 2, C.byref(fmt), out.data_ptr(),
                                          W * 12, 0, None) == 0
        assert call(dec, cs, c3) == -6
        # refusals, with their reasons
        assert call(dec, bad["modular"], C.c_uint64(0)) == -7  # (the oracle's Modular stream is not even XYB: refused at the image header)
        assert call(dec, bad["xyb_saved"], C.c_uint64(0)) == -7 and b"before the colour transform" in L.jxlhip_last_error(dec.ctx)
        # the single-frame calls still refuse the oracle's animation
        anim = files["oracle-animation"]
        assert L.jxlhip_codestream_basic_info(anim, len(anim), C.byref(abi.CodestreamInfo())) == -7
        assert L.jxlhip_decode_codestream(dec.ctx, None, None, anim, len(anim), 2, C.byref(fmt), out.data_ptr(), W * 12, 0, None) == -7
        # a plain full-frame animation pays nothing for blending: frame 0 of "noise-second" is saved by its header
        # (save_as_reference = 1) but nothing reads the slot
        cursor = C.c_uint64(0)
        dec.profile(True)
        assert call(dec, files["noise-second"], cursor) == 0
        assert "blend" not in dec.profile_read() and dec.read_canvas(1) is None
        dec.profile(False)
    finally:
        dec.close()


@pytest.mark.gpu
def test_a_full_replace_frame_never_looks_at_its_source(bench):
    """A full-size kReplace frame with a save slot does not read slot `source`: an XYB frame there (a file with a Modular
    reference frame in slot 0 and a saved full frame) or a smaller canvas is no concern of it."""
    k, f = KINDS["srgb"]
    dec = bench.dec
    sheet = (np.random.default_rng(3).standard_normal((3, 18, 20)) * 0.2).astype(np.float32)
    for slot in range(4):
        dec.set_reference_frame(slot, None)
    dec.set_reference_frame(0, sheet)
    bench.save("A", k, f, 1)  # (source = 0)
    assert same(bench.canvas(1), bench.direct("A", k, f))
    got = bench.blend("B", k, f, (0, 0), bm.REPLACE, False, 1, 2, image=(72, 40))  # a 72 x 40 canvas in slot 2
    assert same(got, bench.direct("B", k, f))
    got = bench.blend("A", k, f, (0, 0), bm.BLEND, False, 2, 2)  # source = save = the smaller canvas: replaced
    assert same(got, bench.direct("A", k, f)) and same(bench.canvas(2), bench.direct("A", k, f))
    dec.set_reference_frame(0, None)


@pytest.mark.gpu
@pytest.mark.parametrize("workers", [0, 6])
def test_full_frame_sequence_with_alpha(kit, oracle, workers):
    """Three full kReplace frames of an image with an alpha channel, each with a save_as_reference nothing reads: the
    displayed frame comes out with its alpha, as JxlDecoder gives it."""
    import torch
    import layer_streams as ls
    import test_seam
    from libjxl_amd import VarDctDecoder
    from test_gpu_patches import _runner
    L = kit[0]
    import os
    import sys
    sys.path.insert(0, os.path.join(test_seam.ROOT, "integration"))
    import build_seam
    RL = test_seam.load(build_seam.build()[0])
    al = [oracle.RealStream(seed=s, xsize=W, ysize=H, alpha_bits=8).codestream.tobytes() for s in (3, 6)]
    cs = ls.splice(L, al[0], [dict(stream=al[0], save_as_reference=1), dict(stream=al[0], save_as_reference=2), dict(stream=al[1])])
    want = ls.jxl_decode_frames(RL, cs, channels=4)
    assert len(want) == 1 and float(want[0][0][..., 3].min()) < 1.0  # a real alpha plane
    info, seq = abi.CodestreamInfo(), abi.SequenceInfo()
    assert L.jxlhip_codestream_sequence_info(cs, len(cs), C.byref(info), C.byref(seq)) == 0
    assert (seq.num_coded_frames, seq.num_displayed_frames, info.num_extra_channels) == (3, 1, 1)
    tf = {8: abi.TF_LINEAR, 13: abi.TF_SRGB}[info.transfer_function]
    fmt = abi.OutputFormat(tf, abi.SAMPLE_F32, 4, 32, 0, 0.0, info.luminances)
    out = torch.full((H, W, 4), 77, dtype=torch.float32, device="cuda")
    R, pool, runner = _runner(workers)
    dec = VarDctDecoder(0)
    try:
        cursor, fr = C.c_uint64(0), abi.SequenceFrame()
        rc = L.jxlhip_decode_codestream_next(dec.ctx, runner, pool, cs, len(cs), C.byref(cursor), 2, C.byref(fmt), out.data_ptr(),
                                             W * 16, 0, None, C.byref(fr))
        assert rc == 0, L.jxlhip_last_error(dec.ctx)
        assert (fr.is_last, fr.coded_frames, cursor.value) == (1, 3, len(cs))
        assert all(dec.read_canvas(s) is None for s in range(4))  # nothing was saved
    finally:
        dec.close()
        if pool:
            R.JxlThreadParallelRunnerDestroy(pool)
    got = out.cpu().numpy()
    err = float(np.abs(got - want[0][0]).max()) / max(1.0, float(np.abs(want[0][0]).max()))
    print("alpha sequence, workers %d: max|diff| / scale = %.3e" % (workers, err))
    assert err <= TIGHT
