"""Patches on the device (jxlhip_set_reference_frame, jxlhip_set_patches, kernels_patches.hip).

  - genuine patch files (oracle.feature_stream("patches"): a kReferenceOnly Modular frame + a VarDCT frame with kPatches)
    through jxlhip_decode_codestream against the reference's public JxlDecoder, as float and as 8-bit output;
  - the kernel alone on synthetic frames with synthetic reference frames: (patches on) must be BIT-EQUAL to
    tests/patches_model.py on the (patches off) planar XYB of the same decoder -- every blend is one IEEE operation, and
    the frame's own path is the same launch both times -- over both routings, every mode, order-dependent overlaps,
    more records per tile than one LDS batch, and with splines, upsampling and noise behind it;
  - state that must not leak between frames and files, and the refused configurations."""
import ctypes as C

import numpy as np
import pytest

from libjxl_amd import abi, synth

import noise_model
import patches_model as pm
import spline_model as sm
import upsampling_model as um
from test_patches_front_end import Walk
from test_splines_front_end import built_sets

TIGHT = 2e-5
LUT = [0.05, 0.12, 0.3, 0.45, 0.6, 0.75, 0.9, 1.0]
STREAMS = [((600, 400), 1.0), ((333, 277), 2.0), ((261, 200), 3.0), ((600, 400), 8.0), ((1030, 520), 1.0)]
BATCH = 128  # kPatchBatch (kernels.h): records one LDS batch of k_patches holds


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
    prebuilt = [os.path.join(build_seam.B.OUT, n) for n in ("libjxl_dec_ref.so", "libjxl_dec_hip.so")]
    if not build_seam.available() and not all(os.path.exists(p) for p in prebuilt):
        pytest.skip("reference tree not present and no prebuilt seam libraries")
    ref_so, _ = build_seam.build()  # (a compile or link failure fails the tests: it must not skip them)
    return test_seam, test_seam.load(ref_so)


@pytest.fixture(scope="module")
def streams(L, ref, jxl_ref):
    """Per (size, distance): the file, and JxlDecoder's float pixels for it -- computed once, never modified."""
    ts, RL = jxl_ref
    out = {}
    for size, d in STREAMS:
        cs = ref.feature_stream("patches", xsize=size[0], ysize=size[1], seed=5, distance=d)
        w = Walk(L, cs)  # a stream without patches cannot pass unnoticed
        assert len(w.frames) == 2 and w.frames[0][0].frame_type == 2 and w.frames[1][0].flags & 2
        want = ts.jxl_decode(RL, cs)
        assert want.shape == (size[1], size[0], 3)
        want.setflags(write=False)
        out[(size, d)] = (cs, want)
    return out


def _runner(workers):
    R = C.CDLL(abi.runner_library_path())
    R.JxlThreadParallelRunnerCreate.restype = C.c_void_p
    R.JxlThreadParallelRunnerCreate.argtypes = [C.c_void_p, C.c_size_t]
    R.JxlThreadParallelRunnerDestroy.argtypes = [C.c_void_p]
    pool = R.JxlThreadParallelRunnerCreate(None, workers) if workers else None
    return R, pool, C.cast(R.JxlThreadParallelRunner, C.c_void_p) if workers else None


def _decode_file(L, dec, cs, xs, ys, sample, channels, workers=0):
    import torch
    R, pool, runner = _runner(workers)
    try:
        info = abi.CodestreamInfo()
        assert L.jxlhip_codestream_basic_info(cs, len(cs), C.byref(info)) == 0
        assert (info.xsize, info.ysize, info.transfer_function) == (xs, ys, 13)  # the visible frame; sRGB
        if sample == abi.SAMPLE_F32:
            fmt = abi.OutputFormat(abi.TF_SRGB, abi.SAMPLE_F32, channels, 32, 0, 0.0, info.luminances)
            out = torch.full((ys, xs, channels), -7.0, dtype=torch.float32, device="cuda")
        else:
            fmt = abi.OutputFormat(abi.TF_SRGB, abi.SAMPLE_U8, channels, 8, 0, 0.0, info.luminances)
            out = torch.zeros((ys, xs, channels), dtype=torch.uint8, device="cuda")
        rc = L.jxlhip_decode_codestream(dec.ctx, runner, pool, cs, len(cs), 2, C.byref(fmt), out.data_ptr(),
                                        xs * channels * out.element_size(), 0, None)
        assert rc == 0, L.jxlhip_last_error(dec.ctx)
        return out.cpu().numpy()
    finally:
        if pool:
            R.JxlThreadParallelRunnerDestroy(pool)


@pytest.mark.gpu
@pytest.mark.parametrize("workers", [0, 6])
@pytest.mark.parametrize("size,distance", STREAMS)
def test_patch_file_matches_jxldecoder(L, streams, size, distance, workers):
    from libjxl_amd import VarDctDecoder
    cs, want = streams[(size, distance)]
    dec = VarDctDecoder(0)
    try:
        got = _decode_file(L, dec, cs, size[0], size[1], abi.SAMPLE_F32, 3, workers)
    finally:
        dec.close()
    scale = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got - want).max()) / scale
    print("patches %dx%d d%g workers %d: max|diff| / scale = %.3e" % (size[0], size[1], distance, workers, err))
    assert err <= TIGHT


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("size,distance", [((600, 400), 1.0), ((261, 200), 3.0), ((600, 400), 8.0)])
def test_patch_file_as_8_bit(L, streams, size, distance, channels):
    from libjxl_amd import VarDctDecoder
    cs, want = streams[(size, distance)]
    want8 = np.round(np.clip(want, 0.0, 1.0) * 255.0)
    dec = VarDctDecoder(0)
    try:
        got = _decode_file(L, dec, cs, size[0], size[1], abi.SAMPLE_U8, channels)
    finally:
        dec.close()
    err = float(np.abs(got[..., :3].astype(np.float32) - want8).max())
    print("patches %dx%d d%g 8-bit x%d: max level difference %g" % (size[0], size[1], distance, channels, err))
    assert err <= 1.0
    if channels == 4:
        assert np.all(got[..., 3] == 255)  # no alpha channel: opaque


# ---- the kernel against the model -----------------------------------------------------------------------------------

def sheets():
    """Four reference frames of different sizes, samples well outside [0, 1] (the clamp of kMul must show)."""
    rng = np.random.default_rng(11)
    return {slot: (rng.standard_normal((3, h, w)) * 0.7).astype(np.float32)
            for slot, (w, h) in {0: (20, 18), 1: (128, 48), 2: (7, 33), 3: (1, 1)}.items()}


def patch(slot, rx, ry, w, h, x, y, mode=pm.ADD, clamp=0):
    return dict(ref=slot, ref_x0=rx, ref_y0=ry, xsize=w, ysize=h, x=x, y=y, mode=mode, alpha_channel=0, clamp=clamp)


def edge_set(W, H):
    """The smallest rectangles that can go wrong, for any frame from 13 pixels wide."""
    PW = (W + 7) & ~7
    out = [patch(0, 3, 4, 1, 1, 5, 7, pm.REPLACE),                       # 1 x 1
           patch(0, 0, 0, 3, 2, W - 3, H - 2, pm.ADD),                   # ends on the last column and row
           patch(0, 16, 15, 4, 3, 2, 40, pm.REPLACE),                    # the far corner of its sheet
           patch(2, 0, 0, 7, 33, 4, 60, pm.MUL, 1),                      # crosses tile rows
           patch(3, 0, 0, 1, 1, 0, 0, pm.ADD),                           # slot 3, the first pixel
           patch(1, 100, 30, 6, 9, 6, 100, pm.ADD),
           patch(0, 5, 5, PW - W + 2, 3, W - 2, 90, pm.REPLACE)]         # into the padding behind the last column
    if W >= 128:
        out += [patch(1, 14, 5, 100, 40, 30, 10, pm.ADD),                # several tiles in both directions
                patch(1, 0, 0, 128, 48, W - 128, H - 48, pm.MUL)]
    return out


def crowded_tile(x0, y0):
    """300 overlapping 3 x 3 patches inside the tile at (x0, y0): more than two LDS batches, in an order that matters."""
    rng = np.random.default_rng(5)
    modes = [(pm.ADD, 0), (pm.REPLACE, 0), (pm.MUL, 0), (pm.MUL, 1)]
    out = []
    for i in range(300):
        m, c = modes[int(rng.integers(0, 4))] if i % 3 else (pm.ADD, 0)
        out.append(patch(int(rng.integers(0, 2)), int(rng.integers(0, 17)), int(rng.integers(0, 15)), 3, 3,
                         x0 + int(rng.integers(0, 10)), y0 + int(rng.integers(0, 13)), m, c))
    return out


def _decode(dec, params, t, dq, patches=None, ups=None, splines=None, noise=None):
    dec.begin_frame(params)
    dec.set_inputs(t, dq)
    if ups is not None:
        dec.set_upsampling(*ups)
    if noise is not None:
        dec.set_noise(*noise)
    if patches is not None:
        dec.set_patches(patches)
    if splines is not None:
        dec.set_splines(splines)
    out = dec.decode_frame()
    dec.sync()
    return out.cpu().numpy()


def _decoder(refs=None):
    from libjxl_amd import VarDctDecoder
    dec = VarDctDecoder(0)
    for slot, planes in (refs or {}).items():
        dec.set_reference_frame(slot, planes)
    return dec


def _xyb_to_rgb(xyb, params):
    """XybToRgb (dec_xyb-inl.h:38-86) in float64 on float32 XYB planes [3, H, W] -> [H, W, 3]."""
    x, y, b = [xyb[c].astype(np.float64) for c in range(3)]
    bias = np.array(params["opsin_biases"], np.float32)
    cb = np.cbrt(bias.astype(np.float32)).astype(np.float32).astype(np.float64)
    mixed = [(y + x - cb[0]) ** 3 + float(bias[0]), (y - x - cb[1]) ** 3 + float(bias[1]), (b - cb[2]) ** 3 + float(bias[2])]
    m = np.array(params["inverse_opsin_matrix"], np.float32).astype(np.float64).reshape(3, 3)
    return np.stack([m[r, 0] * mixed[0] + m[r, 1] * mixed[1] + m[r, 2] * mixed[2] for r in range(3)], axis=-1)


def _srgb8(lin):
    c = np.clip(lin, 0, 1)
    return np.where(c <= 0.0031308, c * 12.92, 1.055 * np.power(c, 1 / 2.4) - 0.055) * 255.0


@pytest.mark.gpu
@pytest.mark.parametrize("fuse", ["0", "1"])
@pytest.mark.parametrize("xs,ys,gab,epf", [(261, 200, 1, 1), (13, 200, 1, 1), (600, 400, 1, 1), (600, 400, 1, 3)])
def test_patch_kernel_is_bit_equal_to_the_numpy_restatement(monkeypatch, xs, ys, gab, epf, fuse):
    monkeypatch.setenv("JXLHIP_FUSE", fuse)
    refs = sheets()
    params, t = synth.synth_frame(xs, ys, device="cuda", output_kind=0, gab=bool(gab), epf_iters=epf)
    patches = edge_set(xs, ys) + crowded_tile(64 if xs > 128 else 0, 16)
    dec = _decoder(refs)
    try:
        dq = dec.default_dequant_tables()
        off = _decode(dec, params, t, dq)
        dec.profile(True)
        on = _decode(dec, params, t, dq, patches=patches)
        slots = dec.profile_read()
        empty = _decode(dec, params, t, dq, patches=[])
    finally:
        dec.close()
    assert slots["patches"][1] == 1, slots
    if epf <= 2:  # both routings of the frame's own path (the fused kernel takes frames from 16 pixels wide)
        assert ("fused" in slots) == (fuse == "1" and xs >= 16) and ("filters" in slots) != ("fused" in slots), slots
    want = pm.apply(off, patches, refs)
    assert np.abs(want - off).max() > 0.1  # the patches are there
    assert np.array_equal(on, want), float(np.abs(on - want).max())
    assert np.array_equal(empty, off)  # an empty dictionary: the plain path


@pytest.mark.gpu
@pytest.mark.parametrize("mode", range(8))
@pytest.mark.parametrize("clamp", [0, 1])
def test_every_mode_one_at_a_time(mode, clamp):
    xs, ys = 261, 200
    refs = sheets()
    params, t = synth.synth_frame(xs, ys, device="cuda", output_kind=0, gab=True, epf_iters=1)
    patches = [dict(p, mode=mode, clamp=clamp) for p in edge_set(xs, ys)]
    dec = _decoder(refs)
    try:
        dq = dec.default_dequant_tables()
        off = _decode(dec, params, t, dq)
        on = _decode(dec, params, t, dq, patches=patches)
    finally:
        dec.close()
    want = pm.apply(off, patches, refs)
    assert np.array_equal(on, want)
    assert np.array_equal(want, off) == (mode == pm.NONE)


ORDERED = [((pm.REPLACE, 0), (pm.ADD, 0)), ((pm.ADD, 0), (pm.REPLACE, 0)), ((pm.MUL, 0), (pm.ADD, 0)),
           ((pm.MUL, 1), (pm.ADD, 0)), ((pm.MUL, 1), (pm.MUL, 0))]


@pytest.mark.gpu
@pytest.mark.parametrize("first,second", ORDERED)
def test_overlapping_patches_are_blended_in_list_order(first, second):
    xs, ys = 261, 200
    refs = sheets()
    params, t = synth.synth_frame(xs, ys, device="cuda", output_kind=0, gab=True, epf_iters=1)
    a = patch(0, 0, 0, 12, 10, 58, 10, *first)   # across the border of two tiles, overlapping in 8 x 6 pixels
    b = patch(1, 40, 8, 12, 10, 62, 14, *second)
    dec = _decoder(refs)
    try:
        dq = dec.default_dequant_tables()
        off = _decode(dec, params, t, dq)
        ab = _decode(dec, params, t, dq, patches=[a, b])
        ba = _decode(dec, params, t, dq, patches=[b, a])
    finally:
        dec.close()
    assert np.array_equal(ab, pm.apply(off, [a, b], refs))
    assert np.array_equal(ba, pm.apply(off, [b, a], refs))
    assert not np.array_equal(ab, ba)  # swapping the two changes the result


@pytest.mark.gpu
def test_more_records_in_a_tile_than_one_lds_batch():
    """300 records in one tile: three batches are staged (a kernel that stopped after the first would leave 172 out)."""
    xs, ys = 261, 200
    refs = sheets()
    params, t = synth.synth_frame(xs, ys, device="cuda", output_kind=0, gab=True, epf_iters=1)
    patches = crowded_tile(128, 32)
    in_tile = [p for p in patches if 128 <= p["x"] and p["x"] + 3 <= 192 and 32 <= p["y"] and p["y"] + 3 <= 48]
    assert len(in_tile) == 300 > 2 * BATCH
    dec = _decoder(refs)
    try:
        dq = dec.default_dequant_tables()
        off = _decode(dec, params, t, dq)
        on = _decode(dec, params, t, dq, patches=patches)
    finally:
        dec.close()
    assert np.array_equal(on, pm.apply(off, patches, refs))
    assert not np.array_equal(on, pm.apply(off, patches[:BATCH], refs))
    assert not np.array_equal(on, pm.apply(off, patches[:2 * BATCH], refs))


@pytest.mark.gpu
def test_float_rgb_and_packed_outputs():
    xs, ys = 261, 200
    refs = sheets()
    fmt = dict(transfer=abi.TF_SRGB, sample_type=abi.SAMPLE_U8, num_channels=4, bits_per_sample=8)
    kw = dict(device="cuda", gab=True, epf_iters=1)
    p0, t = synth.synth_frame(xs, ys, output_kind=0, **kw)
    p1, _ = synth.synth_frame(xs, ys, output_kind=1, **kw)
    p2, _ = synth.synth_frame(xs, ys, output_kind=2, out_format=fmt, **kw)
    # (small amplitudes: the frame stays inside the range the 8-bit comparison resolves)
    small = {s: (v * np.float32(0.05)).astype(np.float32) for s, v in refs.items()}
    patches = [p for p in edge_set(xs, ys) if p["mode"] == pm.ADD]
    dec = _decoder(small)
    try:
        dq = dec.default_dequant_tables()
        off = _decode(dec, p0, t, dq)
        lin = _decode(dec, p1, t, dq, patches=patches)
        out8 = _decode(dec, p2, t, dq, patches=patches)
    finally:
        dec.close()
    rgb = _xyb_to_rgb(pm.apply(off, patches, small), p1)
    assert np.abs(rgb - _xyb_to_rgb(off, p1)).max() > 1e-3
    scale = max(1.0, float(np.abs(rgb).max()))
    err = float(np.abs(lin - rgb).max()) / scale
    print("linear RGB max|diff| / scale = %.3e" % err)
    assert err <= 1e-5, err
    assert np.abs(out8[..., :3].astype(np.float32) - _srgb8(lin)).max() <= 1.6
    assert np.all(out8[..., 3] == 255)


# ---- with the stages behind it ----------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("fuse", ["0", "1"])
def test_patches_then_splines_upsampling_noise(monkeypatch, fuse):
    """The reference's stage order (dec_cache.cc:193-218): patches, splines at coded size, upsampling, noise."""
    monkeypatch.setenv("JXLHIP_FUSE", fuse)
    cw, ch, n = 261, 200, 2
    W, H = n * cw - 1, n * ch
    refs = sheets()
    params, t = synth.synth_frame(cw, ch, device="cuda", output_kind=0, gab=True, epf_iters=2)
    params["cfl_base_x"] = 0.0625
    s = built_sets(cw, ch)
    sets = s["edge"] + s["tiny"]
    patches = edge_set(cw, ch)
    ups = (n, (W, H), None)
    dec = _decoder(refs)
    try:
        dq = dec.default_dequant_tables()
        off = _decode(dec, params, t, dq)
        with_splines = _decode(dec, params, t, dq, patches=patches, splines=sets)
        with_noise = _decode(dec, params, t, dq, patches=patches, noise=(LUT, 1, 0))
        with_ups_noise = _decode(dec, params, t, dq, patches=patches, ups=ups, noise=(LUT, 1, 0))
        dec.profile(True)
        everything = _decode(dec, params, t, dq, patches=patches, ups=ups, splines=sets, noise=(LUT, 1, 0))
        slots = dec.profile_read()
    finally:
        dec.close()
    assert all(k in slots for k in ("patches", "splines", "upsample", "noise")), slots
    blended = pm.apply(off, patches, refs)
    drawn = sm.draw(blended, sm.segments(sets, 0, cw, ch, 0.0625, params["cfl_base_b"]))
    assert np.abs(drawn - blended).max() > 1e-3
    for name, got, want in (
            ("patches -> splines", with_splines, drawn),
            ("patches -> noise", with_noise, noise_model.add_noise(blended, LUT, 0.0625, params["cfl_base_b"], visible=1)),
            ("patches -> upsampling -> noise", with_ups_noise,
             noise_model.add_noise(um.upsample(blended, n, None, (W, H)), LUT, 0.0625, params["cfl_base_b"], visible=1)),
            ("patches -> splines -> upsampling -> noise", everything,
             noise_model.add_noise(um.upsample(drawn, n, None, (W, H)), LUT, 0.0625, params["cfl_base_b"], visible=1))):
        err = float(np.abs(got - want).max())
        print("%s: %.3e" % (name, err))
        assert err <= 1e-5, (name, err)


# ---- state ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_a_frame_after_a_patch_frame_is_untouched():
    refs = sheets()
    params, t = synth.synth_frame(600, 400, device="cuda", output_kind=1, gab=True, epf_iters=1)
    fresh, used = _decoder(), _decoder(refs)
    try:
        want = _decode(fresh, params, t, fresh.default_dequant_tables())
        dq = used.default_dequant_tables()
        blended = _decode(used, params, t, dq, patches=edge_set(600, 400))
        got = _decode(used, params, t, dq)
    finally:
        fresh.close()
        used.close()
    assert np.abs(blended - want).max() > 1e-3
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_files_do_not_leak_into_each_other(L, ref, streams):
    from libjxl_amd import VarDctDecoder
    cs, _ = streams[((261, 200), 3.0)]
    plain = ref.feature_stream("plain", xsize=261, ysize=200, seed=5, distance=3.0)
    fresh, used = VarDctDecoder(0), VarDctDecoder(0)
    try:
        want_plain = _decode_file(L, fresh, plain, 261, 200, abi.SAMPLE_F32, 3)
        first = _decode_file(L, used, cs, 261, 200, abi.SAMPLE_F32, 3)
        again = _decode_file(L, used, cs, 261, 200, abi.SAMPLE_F32, 3)
        got_plain = _decode_file(L, used, plain, 261, 200, abi.SAMPLE_F32, 3)
        # the slots were cleared at the start of the plain file's call: a dictionary for slot 3 finds nothing there
        params, t = synth.synth_frame(64, 48, device="cuda", output_kind=0)
        used.begin_frame(params)
        rc, h = abi.patches_from_list([patch(3, 0, 0, 2, 2, 1, 1)], 64, 48, {3: (18, 18)}, L=L)
        assert rc == 0
        assert L.jxlhip_set_patches(used.ctx, h) == -1 and b"empty" in L.jxlhip_last_error(used.ctx)
        abi.patches_destroy(h, L)
    finally:
        fresh.close()
        used.close()
    assert np.array_equal(first, again)
    assert np.array_equal(got_plain, want_plain)


@pytest.mark.gpu
def test_slots_are_validated_by_every_set_patches(L):
    """A patch whose slot is empty, or smaller than its rectangle since the slot was replaced, is
    JXLHIP_ERR_INVALID_ARGUMENT (-1): the dictionary object was checked against other slots than the context holds."""
    refs = sheets()
    params, t = synth.synth_frame(261, 200, device="cuda", output_kind=0, gab=True, epf_iters=1)
    p = patch(1, 100, 30, 6, 9, 6, 100)
    dec = _decoder(refs)
    try:
        dq = dec.default_dequant_tables()
        off = _decode(dec, params, t, dq)
        assert np.array_equal(_decode(dec, params, t, dq, patches=[p]), pm.apply(off, [p], refs))
        rc, h = abi.patches_from_list([p], 264, 200, {1: (128, 48)}, L=L)
        assert rc == 0
        try:
            smaller = refs[1][:, :20, :50].copy()
            dec.set_reference_frame(1, smaller)  # replaced by a smaller sheet
            dec.begin_frame(params)
            assert L.jxlhip_set_patches(dec.ctx, h) == -1 and b"leaves" in L.jxlhip_last_error(dec.ctx)
            dec.set_reference_frame(1, None)     # cleared
            assert L.jxlhip_set_patches(dec.ctx, h) == -1 and b"empty" in L.jxlhip_last_error(dec.ctx)
            # a slot set between set_patches and the decode: the uploaded records point into the old slot
            dec.set_reference_frame(1, refs[1])
            dec.begin_frame(params)
            dec.set_inputs(t, dq)
            assert L.jxlhip_set_patches(dec.ctx, h) == 0
            dec.set_reference_frame(0, refs[0])
            out = dec.alloc_output()
            a = dec._out_args(out)
            assert L.jxlhip_decode_frame(dec.ctx, *a) == -6 and b"set_reference_frame" in L.jxlhip_last_error(dec.ctx)
            assert L.jxlhip_set_patches(dec.ctx, h) == 0  # set again: taken
            assert L.jxlhip_decode_frame(dec.ctx, *a) == 0
            dec.sync()
            assert np.array_equal(out.cpu().numpy(), pm.apply(off, [p], refs))
            # a smaller sheet in the same slot serves the patches that fit it
            dec.set_reference_frame(1, smaller)
            q = patch(1, 40, 10, 6, 9, 6, 100)
            assert np.array_equal(_decode(dec, params, t, dq, patches=[q]), pm.apply(off, [q], {1: smaller}))
        finally:
            abi.patches_destroy(h, L)
    finally:
        dec.close()


@pytest.mark.gpu
def test_refused_configurations(L):
    import torch
    refs = sheets()
    sizes = {s: (v.shape[2], v.shape[1]) for s, v in refs.items()}
    rc, h = abi.patches_from_list(edge_set(300, 520), 304, 520, sizes, L=L)
    assert rc == 0
    # a dictionary that uses extra channels: an alpha mode on an image with alpha; an extra channel that is blended
    rc, h_alpha = abi.patches_from_list([patch(0, 0, 0, 2, 2, 1, 1, pm.BLEND_ABOVE)], 304, 520, sizes, 1, [[[0, 0, 0]]], L=L)
    assert rc == 0
    rc, h_ec = abi.patches_from_list([patch(0, 0, 0, 2, 2, 1, 1, pm.ADD)], 304, 520, sizes, 1, [[[pm.ADD, 0, 0]]], L=L)
    assert rc == 0
    try:
        ctx = C.c_void_p()
        devs = (C.c_int * 2)(0, 0)
        assert L.jxlhip_create_multi(devs, 2, None, C.byref(ctx)) == 0
        try:
            assert L.jxlhip_set_patches(ctx, h) == -7
            assert b"multi-device" in L.jxlhip_last_error(ctx)
            one = np.zeros((3, 2, 2), np.float32)
            ptrs = (C.c_void_p * 3)(*[one[k].ctypes.data for k in range(3)])
            assert L.jxlhip_set_reference_frame(ctx, 0, 2, 2, ptrs, 2, 0) == -7
        finally:
            L.jxlhip_destroy(ctx)
        dec = _decoder(refs)
        try:
            params, t = synth.synth_frame(300, 520, device="cuda", output_kind=1, gab=True, epf_iters=1)
            assert L.jxlhip_set_patches(dec.ctx, h) == -6  # before frame_begin
            dec.begin_frame(dict(params, stripe_group_y0=1, stripe_group_rows=1))
            assert L.jxlhip_set_patches(dec.ctx, h) == -7
            assert b"stripes" in L.jxlhip_last_error(dec.ctx)
            dec.begin_frame(dict(params, undo_orientation=6))
            assert L.jxlhip_set_patches(dec.ctx, h) == -7
            assert b"undo_orientation" in L.jxlhip_last_error(dec.ctx)
            dq = dec.default_dequant_tables()
            dec.begin_frame(params)
            dec.set_inputs(t, dq)
            for bad in (h_alpha, h_ec):
                assert L.jxlhip_set_patches(dec.ctx, bad) == -7
                assert b"extra channels" in L.jxlhip_last_error(dec.ctx)
            # alpha on a patch frame, either way round
            alpha = np.ones((520, 300), np.float32)
            dec.set_patches(h)
            assert L.jxlhip_set_alpha(dec.ctx, alpha.ctypes.data, 300) == -7
            assert b"patches" in L.jxlhip_last_error(dec.ctx)
            fmt = dict(transfer=abi.TF_SRGB, sample_type=abi.SAMPLE_U8, num_channels=4, bits_per_sample=8)
            p8, _ = synth.synth_frame(300, 520, device="cuda", output_kind=2, gab=True, epf_iters=1, out_format=fmt)
            dec.begin_frame(p8)
            dec.set_inputs(t, dq)
            dec.set_alpha(alpha)
            assert L.jxlhip_set_patches(dec.ctx, h) == -7
            assert b"alpha" in L.jxlhip_last_error(dec.ctx)
            # bad arguments of the slots
            one = np.zeros((3, 2, 2), np.float32)
            ptrs = (C.c_void_p * 3)(*[one[k].ctypes.data for k in range(3)])
            assert L.jxlhip_set_reference_frame(dec.ctx, 4, 2, 2, ptrs, 2, 0) == -1
            assert L.jxlhip_set_reference_frame(dec.ctx, 0, 2, 2, ptrs, 1, 0) == -1
            assert L.jxlhip_set_reference_frame(dec.ctx, 0, 2, 2, None, 2, 0) == -1
            dec.set_reference_frame(0, refs[0])
            # the split calls
            dec.begin_frame(params)
            dec.set_inputs(t, dq)
            dec.set_patches(h)
            dec.decode_blocks()
            out = torch.empty((520, 300, 3), dtype=torch.float32, device="cuda")
            assert L.jxlhip_decode_filters(dec.ctx, C.c_void_p(out.data_ptr()), 300 * 12, 0) == -7
            assert b"split calls" in L.jxlhip_last_error(dec.ctx)
            assert L.jxlhip_decode_filters_rows(dec.ctx, C.c_void_p(out.data_ptr()), 300 * 12, 0, 0, 256) == -7
            dec.decode_frame(out)  # ... while jxlhip_decode_frame takes the same frame
            dec.sync()
        finally:
            dec.close()
    finally:
        for x in (h, h_alpha, h_ec):
            abi.patches_destroy(x, L)


@pytest.mark.gpu
def test_device_planes_as_a_reference_frame():
    """set_reference_frame from device memory (on_device = 1) gives what the host copy gives."""
    import torch
    refs = sheets()
    params, t = synth.synth_frame(261, 200, device="cuda", output_kind=0, gab=True, epf_iters=1)
    patches = edge_set(261, 200)
    a, b = _decoder(refs), _decoder({s: torch.from_numpy(v).cuda() for s, v in refs.items()})
    try:
        want = _decode(a, params, t, a.default_dequant_tables(), patches=patches)
        got = _decode(b, params, t, b.default_dequant_tables(), patches=patches)
    finally:
        a.close()
        b.close()
    assert np.array_equal(got, want)
