"""DC-only groups on the device (jxlhip_set_dc_only_groups, kernels_dc_upsample.hip), the kernel alone: synthetic
frames through the split call with a mask, jxlhip_export_xyb against
  - tests/upsampling_model.py's N = 8 path on the frame's DC planes, in the masked groups;
  - the unmasked decode of the same frame in the others, bit for bit
over the smallest shapes at which it can go wrong (a 1 x 1 DC image; two DC columns over three group rows, the last
eight rows high; a last group column one block wide over a last group row one block high; widths across a block edge),
four masks, default and custom weights.  The model is float32 in the reference's order of operations, so bit-equality
is the expectation; the bar is the 1e-5 tests/test_gpu_upsampling.py puts on k_upsample against the same model, and a
test without a GPU shows that the bar sees a kernel that mirrors at group edges or drops the clamp.  Then the timing
slot, a context reused, and the refused configurations."""
import ctypes as C

import numpy as np
import pytest

from libjxl_amd import abi, synth

import upsampling_model as um

BAR = 1e-5
SHAPES = [(8, 8), (16, 520), (520, 264), (261, 264), (262, 264), (263, 264), (264, 264)]
MASKS = ["all", "corner", "checker", "all_but_one"]
LUT = [0.05, 0.12, 0.3, 0.45, 0.6, 0.75, 0.9, 1.0]


def _groups(xs, ys):
    return (ys + 255) // 256, (xs + 255) // 256


def _mask(name, xs, ys):
    ysg, xsg = _groups(xs, ys)
    gy, gx = np.mgrid[0:ysg, 0:xsg]
    if name == "all":
        return np.ones((ysg, xsg), bool)
    if name == "corner":
        return (gy == ysg - 1) & (gx == xsg - 1)
    if name == "checker":
        return (gx + gy) % 2 == 0
    return ~((gy == 0) & (gx == 0)) if ysg * xsg > 1 else np.ones((ysg, xsg), bool)  # all but one


def _custom_weights(seed):
    """Random weights around the defaults; the coded form is the upper triangle of a symmetric matrix."""
    rng = np.random.default_rng(seed)
    w = um.default_weights(8)
    return (w + rng.standard_normal(w.size).astype(np.float32) * np.float32(0.02)).astype(np.float32)


def _dc_planes(t):
    return np.stack([d.cpu().numpy() for d in t["dc"]]).astype(np.float32)


def _pixel_mask(mask, xs, ys):
    ysb, xsb = (ys + 7) // 8, (xs + 7) // 8
    y, x = np.mgrid[0:ysb * 8, 0:xsb * 8]
    return mask[y // 256, x // 256]


def _rel(got, want):
    """per channel: max|got - want| / max(max|want|, 1e-3)"""
    g, w = got.reshape(3, -1).astype(np.float64), want.reshape(3, -1).astype(np.float64)
    return float((np.abs(g - w).max(axis=1) / np.maximum(np.abs(w).max(axis=1), 1e-3)).max())


def _ulps(got, want):
    def key(a):  # float32 -> integers ordered like the floats
        i = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int(np.abs(key(got) - key(want)).max())


def _upsample_variant(planes, weights, clamp=True, group=None):
    """um.upsample's N = 8 arithmetic with a fault built in: clamp = False drops the clamp to the neighbourhood's range;
    group = 32 mirrors at the edges of every 32 x 32 group of DC samples instead of the image's."""
    if group is not None:
        nc, ch, cw = planes.shape
        out = np.zeros((nc, 8 * ch, 8 * cw), np.float32)
        for y0 in range(0, ch, group):
            for x0 in range(0, cw, group):
                out[:, 8 * y0:8 * (y0 + group), 8 * x0:8 * (x0 + group)] = _upsample_variant(
                    planes[:, y0:y0 + group, x0:x0 + group], weights, clamp)
        return out
    if clamp:
        return um.upsample(planes, 8, weights)
    nc, ch, cw = planes.shape
    k = um.kernels(8, um.default_weights(8) if weights is None else weights)
    ys = np.array([um._mirror(i, ch) for i in range(-2, ch + 2)])
    xs = np.array([um._mirror(i, cw) for i in range(-2, cw + 2)])
    p = planes[:, ys][:, :, xs]
    taps = [p[:, i // 5:i // 5 + ch, i % 5:i % 5 + cw] for i in range(25)]
    out = np.zeros((nc, 8 * ch, 8 * cw), np.float32)
    for o in range(64):
        acc = [taps[i] * k[o][i] for i in range(3)]
        for i in range(3, 24, 3):
            for a in range(3):
                acc[a] = um._fma(taps[i + a], k[o][i + a], acc[a])
        acc[0] = um._fma(taps[24], k[o][24], acc[0])
        out[:, o // 8::8, o % 8::8] = (acc[1] + acc[2]) + acc[0]
    return out


def test_the_bar_sees_group_edge_mirroring_and_a_dropped_clamp():
    """No GPU: both faults, applied to the model, exceed the bar by a wide margin on the frames the GPU test uses."""
    for xs, ys in ((520, 264), (16, 520)):
        _, t = synth.synth_frame(xs, ys, device="cpu", gab=True, epf_iters=1)
        dc = _dc_planes(t)
        good = um.upsample(dc, 8, None)
        edge = _rel(_upsample_variant(dc, None, group=32), good)
        unclamped = _rel(_upsample_variant(dc, None, clamp=False), good)
        print("%dx%d: mirrored at group edges %.3e, without the clamp %.3e (bar %.0e)" % (xs, ys, edge, unclamped, BAR))
        assert edge > 100 * BAR and unclamped > 100 * BAR
    # (the model's own variant with neither fault is the model)
    assert np.array_equal(_upsample_variant(dc, None), good)


@pytest.fixture(scope="module")
def bench():
    from libjxl_amd import VarDctDecoder

    class Bench:
        def __init__(self):
            self.dec = VarDctDecoder(0)
            self.dq = self.dec.default_dequant_tables()
            self.frames = {}

        def frame(self, xs, ys):
            """(params, tensors, DC planes, the unmasked phase-1 planes): made once per shape, never modified"""
            if (xs, ys) not in self.frames:
                params, t = synth.synth_frame(xs, ys, device="cuda", gab=True, epf_iters=1, mix=synth.MIX_ALL)
                off = self.planes(params, t, None, None)
                off.setflags(write=False)
                self.frames[(xs, ys)] = (params, t, _dc_planes(t), off)
            return self.frames[(xs, ys)]

        def planes(self, params, t, mask, weights):
            d = self.dec
            d.begin_frame(params)
            d.set_inputs(t, self.dq)
            d.set_dc_only_groups(mask, weights)
            d.decode_blocks()
            return np.stack(d.export_xyb())

    b = Bench()
    yield b
    b.dec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("custom", [False, True])
@pytest.mark.parametrize("mask_name", MASKS)
@pytest.mark.parametrize("xs,ys", SHAPES)
def test_masked_groups_are_the_model_and_the_others_untouched(bench, xs, ys, mask_name, custom):
    params, t, dc, off = bench.frame(xs, ys)
    mask = _mask(mask_name, xs, ys)
    weights = _custom_weights(xs + ys) if custom else None
    got = bench.planes(params, t, mask, weights)
    assert got.shape == off.shape == (3, dc.shape[1] * 8, dc.shape[2] * 8)
    want = um.upsample(dc, 8, weights)
    pm = _pixel_mask(mask, xs, ys)
    assert pm.any()
    assert np.array_equal(got[:, ~pm], off[:, ~pm])  # bit for bit
    g, w = got[:, pm], want[:, pm]
    err, ulps = _rel(g, w), _ulps(g, w)
    print("DCUP %dx%d mask %s custom %d: max rel %.3e, %d ulp(s)" % (xs, ys, mask_name, custom, err, ulps))
    assert err <= BAR, (err, ulps)
    if mask.sum() < mask.size or not custom:
        assert not np.array_equal(got[:, pm], off[:, pm])  # the stage ran: phase 1's own pixels are gone


@pytest.mark.gpu
def test_an_empty_mask_is_the_plain_path_and_the_slot_is_12(bench):
    params, t, dc, off = bench.frame(520, 264)
    assert np.array_equal(bench.planes(params, t, np.zeros(_groups(520, 264), bool), None), off)
    assert abi.KERNEL_NAMES_EX[12] == "dc_upsample" and abi.KERNEL_COUNT_EX >= 13 and abi.KERNEL_COUNT == 8
    d = bench.dec
    for mask, launches in ((None, 0), (_mask("checker", 520, 264), 1)):
        d.begin_frame(params)
        d.set_inputs(t, bench.dq)
        d.set_dc_only_groups(mask)
        d.profile(True)
        d.decode_frame()
        prof = d.profile_read()
        d.profile(False)
        assert ("dc_upsample" in prof) == bool(launches), prof
        if launches:
            assert prof["dc_upsample"][1] == 1 and "fused" not in prof and "filters" in prof
    # the frozen call reports its eight slots and knows nothing of the new one
    ms, n = (C.c_float * 8)(), (C.c_uint32 * 8)()
    assert d.L.jxlhip_profile_read(d.ctx, ms, n) == 0


@pytest.mark.gpu
def test_whole_frame_decode_equals_the_split_calls_and_a_new_frame_resets(bench):
    """jxlhip_decode_frame with a mask = decode_blocks + decode_filters with it; the next frame_begin forgets the mask."""
    params, t, dc, off = bench.frame(520, 264)
    d = bench.dec
    mask = _mask("checker", 520, 264)
    d.begin_frame(params)
    d.set_inputs(t, bench.dq)
    d.set_dc_only_groups(mask)
    whole = d.decode_frame().cpu().numpy()
    d.decode_blocks()
    split = d.alloc_output()
    d.decode_filters(split)
    d.sync()
    assert np.array_equal(whole, split.cpu().numpy())
    d.begin_frame(params)
    d.set_inputs(t, bench.dq)
    plain = d.decode_frame().cpu().numpy()
    d.sync()
    assert not np.array_equal(whole, plain)
    pm = _pixel_mask(mask, 520, 264)[:264, :520]
    far = np.zeros_like(pm)  # inside an unmasked group, further from the masked ones than the filters reach: the plain frame
    far[8:248, 264:504] = True
    assert not pm[far].any() and np.array_equal(whole[far], plain[far])


@pytest.mark.gpu
def test_refused_configurations(bench):
    L, d = bench.dec.L, bench.dec
    params, t, dc, off = bench.frame(520, 264)
    ones = np.ones(6, np.uint8)
    ctx = C.c_void_p()
    assert L.jxlhip_create_multi((C.c_int * 2)(0, 0), 2, None, C.byref(ctx)) == 0
    try:
        assert L.jxlhip_set_dc_only_groups(ctx, ones.ctypes.data, None) == -7 and b"multi-device" in L.jxlhip_last_error(ctx)
    finally:
        L.jxlhip_destroy(ctx)
    from libjxl_amd import VarDctDecoder
    fresh = VarDctDecoder(0)
    try:
        assert L.jxlhip_set_dc_only_groups(fresh.ctx, ones.ctypes.data, None) == -6  # before frame_begin
    finally:
        fresh.close()
    d.begin_frame(dict(params, stripe_group_y0=1, stripe_group_rows=1))
    assert L.jxlhip_set_dc_only_groups(d.ctx, ones.ctypes.data, None) == -7 and b"stripes" in L.jxlhip_last_error(d.ctx)
    spline = [dict(start=(100, 100), deltas=[(8, 0), (0, 0)], color=[[0] * 32 for _ in range(3)], sigma=[4] + [0] * 31)]
    spline[0]["color"][1][0] = 3
    ref = np.zeros((3, 16, 16), np.float32)
    patch = [dict(ref=0, xsize=8, ysize=8, x=8, y=8, mode=abi.PATCH_ADD)]
    rgba = dict(transfer=abi.TF_SRGB, sample_type=abi.SAMPLE_U8, num_channels=4, bits_per_sample=8)
    others = {
        "noise": lambda: d.set_noise(LUT),
        "splines": lambda: d.set_splines(spline),
        "patches": lambda: d.set_patches(patch),
        "upsampling": lambda: d.set_upsampling(8, (520 * 8, 264 * 8)),
        "blending": lambda: d.set_blending((520, 264)),
        "alpha": lambda: d.set_alpha(np.ones((264, 520), np.float32)),
    }
    d.set_reference_frame(0, ref)
    try:
        for name, call in others.items():
            p = dict(params, output_kind=2, out_format=rgba) if name == "alpha" else params
            # the mask first, the other stage second
            d.begin_frame(p)
            d.set_dc_only_groups(ones)
            with pytest.raises(abi.JxlHipError, match="%s on a frame with DC-only groups" % name):
                call()
            # ... and the other way round
            d.begin_frame(p)
            call()
            with pytest.raises(abi.JxlHipError, match="DC-only groups on a frame with %s" % name):
                d.set_dc_only_groups(ones)
            # an empty mask refuses nothing
            d.set_dc_only_groups(np.zeros(6, np.uint8))
    finally:
        d.set_reference_frame(0, None)
