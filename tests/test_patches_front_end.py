"""Patches in the host front-end (CPU): the files cjxl writes for images with repeated glyphs
(oracle.feature_stream("patches")) -- a kReferenceOnly Modular frame that holds the glyph sheet, then the visible
VarDCT frame with FrameHeader::kPatches -- through jxlhip_modular_frame_decode and jxlhip_patches_decode, on through the
DC-global fields; bytes to pixels without a device (the product's parsers, the C oracle's filters, tests/patches_model.py)
against the reference's JxlDecoder; the list round trip; every rejection; truncation; and the same inputs through a
stand-alone sanitizer build (tests/fuzz/fuzz_patches.cc)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from libjxl_amd import abi

import patches_model as pm

FLAG_PATCHES = 2
BAD, UNSUPPORTED = -5, -7
TIGHT = 2e-5
# together: epf_iters 1, 2 and 3
STREAMS = [((600, 400), 1.0), ((333, 277), 2.0), ((261, 200), 3.0), ((600, 400), 8.0)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref(oracle):
    if not oracle.ref_available():
        pytest.skip("oracle/_ref not available")
    oracle.ref_lib()
    return oracle


@pytest.fixture(scope="module")
def L():
    return abi.load_library()


@pytest.fixture(scope="module")
def jxl_ref():
    import sys
    import test_seam
    sys.path.insert(0, os.path.join(test_seam.ROOT, "integration"))
    import build_seam
    prebuilt = [os.path.join(build_seam.B.OUT, n) for n in ("libjxl_dec_ref.so", "libjxl_dec_hip.so")]
    if not build_seam.available() and not all(os.path.exists(p) for p in prebuilt):
        pytest.skip("reference tree not present and no prebuilt seam libraries")
    ref_so, _ = build_seam.build()  # (a compile or link failure fails the tests: it must not skip them)
    return test_seam, test_seam.load(ref_so)


class Walk:
    """The frames of a patches file as the product's header parsers see them."""

    def __init__(self, L, cs):
        self.cs = cs = np.frombuffer(cs, np.uint8)
        base, n = cs.ctypes.data, len(cs)
        self.ih, pos = abi.ImageHeader(), C.c_size_t(0)
        assert L.jxlhip_image_header_decode(base, n, C.byref(pos), None, 0, C.byref(self.ih)) == 0
        ih = self.ih
        self.info = abi.ImageInfo(ih.xsize, ih.ysize, ih.xyb_encoded, 0, None, 0, 0, 0, ih.bit_depth.bits_per_sample)
        self.frames = []  # (frame header, sections)
        while True:
            fh = abi.FrameHeader()
            assert L.jxlhip_frame_header_decode(base, n, C.byref(pos), C.byref(self.info), C.byref(fh)) == 0
            nt = int(fh.num_toc_entries)
            off, sz, total = np.zeros(nt, np.uint64), np.zeros(nt, np.uint32), C.c_uint64(0)
            assert L.jxlhip_toc_decode(base, n, C.byref(pos), nt, off.ctypes.data, sz.ctypes.data, C.byref(total)) == 0
            start = pos.value // 8
            self.frames.append((fh, [cs[start + int(o): start + int(o) + int(s)].copy() for o, s in zip(off, sz)]))
            pos = C.c_size_t((start + total.value) * 8)
            if fh.is_last:
                break
        assert pos.value == 8 * n  # the file ends with its last frame

    def reference_frame(self, L, data=None, fh=None):
        """(rc, planes [3, h, w], bits consumed, message) of jxlhip_modular_frame_decode on frame 0's section."""
        fh0, sections = self.frames[0]
        fh = fh0 if fh is None else fh
        s0 = sections[0] if data is None else data
        s0 = np.ascontiguousarray(s0) if len(s0) else np.zeros(1, np.uint8)
        size = len(sections[0]) if data is None else len(data)
        planes = np.zeros((3, fh0.ysize, fh0.xsize), np.float32)
        ptrs = (C.c_void_p * 3)(*[planes[k].ctypes.data for k in range(3)])
        pos, why = C.c_size_t(0), C.c_char_p()
        rc = L.jxlhip_modular_frame_decode(s0.ctypes.data, size, C.byref(pos), C.byref(fh), ptrs, fh0.xsize, C.byref(why))
        return rc, planes, pos.value, (why.value or b"").decode()

    def ref_sizes(self):
        fh0 = self.frames[0][0]
        return {int(fh0.save_as_reference): (int(fh0.xsize), int(fh0.ysize))}

    def dictionary(self, L, data=None):
        """(rc, handle, end bit) of jxlhip_patches_decode on the head of frame 1's DC-global section."""
        fh1, sections = self.frames[1]
        d = sections[0].tobytes() if data is None else bytes(data)
        return abi.patches_decode(d, 0, fh1.xsize_blocks * 8, fh1.ysize_blocks * 8, self.ref_sizes(), L=L)


@pytest.fixture(scope="module")
def walks(L, ref):
    return {(size, d): Walk(L, ref.feature_stream("patches", xsize=size[0], ysize=size[1], seed=5, distance=d))
            for size, d in STREAMS}


@pytest.mark.parametrize("size,distance", STREAMS)
def test_frame_walk_on_the_genuine_streams(L, walks, size, distance):
    w = walks[(size, distance)]
    assert len(w.frames) == 2
    fh0, sec0 = w.frames[0]
    fh1, sec1 = w.frames[1]
    assert (fh0.frame_type, fh0.is_modular, fh0.color_transform, fh0.flags, fh0.upsampling) == (2, 1, 0, 0, 1)
    assert fh0.custom_size_or_origin and not fh0.is_last and fh0.save_before_color_transform and len(sec0) == 1
    assert (fh1.frame_type, fh1.is_modular, fh1.is_last) == (0, 0, 1) and fh1.flags & FLAG_PATCHES
    assert (fh1.xsize, fh1.ysize) == size and fh1.lf.gab and fh1.lf.epf_iters == {1.0: 1, 2.0: 2, 3.0: 2, 8.0: 3}[distance]
    # frame 0: planes of the header's size, its single section consumed exactly
    rc, planes, bits, why = w.reference_frame(L)
    assert rc == 0, why
    assert planes.shape == (3, fh0.ysize, fh0.xsize) and (bits + 7) // 8 == len(sec0[0])
    assert np.abs(planes).max() > 0.1 and np.isfinite(planes).all()
    # frame 1: dictionary, DC-global fields, Modular global info consume the DC-global section exactly
    s0 = sec1[0]
    rc, h, end = w.dictionary(L)
    assert rc == 0
    try:
        dcg, pos = abi.DcGlobal(), C.c_size_t(end)
        assert L.jxlhip_dc_global_decode(s0.ctypes.data, len(s0), C.byref(pos), fh1.flags & ~FLAG_PATCHES, C.byref(dcg)) == 0
        assert dcg.global_scale > 0 and dcg.quant_dc > 0
        tree = C.c_void_p()
        assert L.jxlhip_modular_global_decode(s0.ctypes.data, len(s0), C.byref(pos), C.byref(fh1), C.byref(tree)) == 0
        L.jxlhip_modular_tree_destroy(tree)
        assert (pos.value + 7) // 8 == len(s0)
        # the flag itself is still refused by the DC-global decode
        p2 = C.c_size_t(end)
        assert L.jxlhip_dc_global_decode(s0.ctypes.data, len(s0), C.byref(p2), fh1.flags, C.byref(abi.DcGlobal())) == UNSUPPORTED
        lst, nec, uses_ec, _ = abi.patches_list(h, L)
        assert len(lst) > 100 and nec == 0 and not uses_ec
        for p in lst:
            assert p["x"] + p["xsize"] <= size[0] and p["y"] + p["ysize"] <= size[1]
            assert p["ref"] == fh0.save_as_reference
            assert p["ref_x0"] + p["xsize"] <= fh0.xsize and p["ref_y0"] + p["ysize"] <= fh0.ysize
            assert p["mode"] == pm.ADD  # what the encoder writes (enc_patch_dictionary.cc:776-780)
    finally:
        abi.patches_destroy(h, L)


def _filtered_xyb(L, w):
    """Frame 1 of a walk through the product's host parsers and entropy decoder into the C oracle: planar XYB behind
    the loop filters (the chain of tests/test_front_end_chain.py, the DC-global fields read from behind the
    dictionary)."""
    import oracle as O
    fh, sections = w.frames[1]
    ih = w.ih
    s0 = sections[0]
    rc, h, end = w.dictionary(L)
    assert rc == 0
    patches = abi.patches_list(h, L)[0]
    abi.patches_destroy(h, L)
    dcg, dpos = abi.DcGlobal(), C.c_size_t(end)
    assert L.jxlhip_dc_global_decode(s0.ctypes.data, len(s0), C.byref(dpos), fh.flags & ~FLAG_PATCHES, C.byref(dcg)) == 0
    tree = C.c_void_p()
    assert L.jxlhip_modular_global_decode(s0.ctypes.data, len(s0), C.byref(dpos), C.byref(fh), C.byref(tree)) == 0
    xsb, ysb, ng, ndc = fh.xsize_blocks, fh.ysize_blocks, int(fh.num_groups), int(fh.num_dc_groups)
    qdc = [np.zeros(xsb * ysb, np.int32) for _ in range(3)]
    acs, rq, sharp = np.zeros(xsb * ysb, np.uint8), np.zeros(xsb * ysb, np.int32), np.zeros(xsb * ysb, np.uint8)
    cw, chh = (xsb + 7) // 8, (ysb + 7) // 8
    ytox, ytob = np.zeros(cw * chh, np.int8), np.zeros(cw * chh, np.int8)
    used, prec = C.c_uint32(0), []
    try:
        for g in range(ndc):
            d = sections[1 + g]
            gp, ep = C.c_size_t(0), C.c_uint32(0)
            ptrs = (C.c_void_p * 3)(*[q.ctypes.data for q in qdc])
            assert L.jxlhip_dc_group_decode(tree, d.ctypes.data, len(d), C.byref(gp), C.byref(fh), g, ptrs, C.byref(ep),
                                            acs.ctypes.data, rq.ctypes.data, sharp.ctypes.data, ytox.ctypes.data,
                                            ytob.ctypes.data, C.byref(used)) == 0
            prec.append(ep.value)
    finally:
        L.jxlhip_modular_tree_destroy(tree)
    assert ndc == 1
    qctx = np.zeros(xsb * ysb, np.uint8)
    qp = (C.c_void_p * 3)(*[q.ctypes.data for q in qdc])
    assert L.jxlhip_quant_dc_contexts(C.byref(dcg.block_ctx_map), xsb * ysb, qp, qctx.ctypes.data) == 0
    f32 = np.float32
    inv_quant_dc = (f32(65536.0) / f32(dcg.global_scale)) / f32(dcg.quant_dc)
    mul_dc = [f32(inv_quant_dc * f32(dcg.dc_quant[c])) for c in range(3)]
    scale = f32(1.0) / f32(dcg.cfl_color_factor)
    dc = O.ref_dequant_dc([q.reshape(ysb, xsb) for q in qdc], mul_dc,
                          float(f32(dcg.cfl_base_x) + f32(dcg.ytox_dc) * scale),
                          float(f32(dcg.cfl_base_b) + f32(dcg.ytob_dc) * scale),
                          not (fh.flags & 128), mul=float(f32(1.0) / f32(1 << prec[0])))
    glob = sections[1 + ndc]
    encs = abi.QuantEncodings()
    nh, bits, hs = C.c_uint32(0), C.c_size_t(0), (C.c_void_p * fh.num_passes)()
    assert L.jxlhip_ac_global_decode(glob.ctypes.data, len(glob), ng, fh.num_passes, used.value,
                                     C.byref(dcg.block_ctx_map), C.byref(encs), C.byref(nh), hs, C.byref(bits)) == 0
    coeffs = [np.zeros(ng * 65536, np.int32) for _ in range(3)]
    try:
        xsg = int(fh.xsize_groups)
        for g in range(ng):
            ptrs = (C.c_void_p * 3)(*[o[g * 65536:].ctypes.data for o in coeffs])
            for ps in range(fh.num_passes):
                d = sections[2 + ndc + ps * ng + g]
                gp, cnt = C.c_size_t(0), C.c_size_t(0)
                assert L.jxlhip_ac_group_decode(hs[ps], xsb, ysb, g % xsg, g // xsg, acs.ctypes.data, rq.ctypes.data,
                                                qctx.ctypes.data, d.ctypes.data, len(d), C.byref(gp), fh.shift[ps], 1,
                                                ptrs, C.byref(cnt)) == 0
    finally:
        for hh in hs:
            L.jxlhip_ac_pass_destroy(hh)
    p = O.FrameParams()
    p.xsize, p.ysize, p.coeff_type, p.output_kind = fh.xsize, fh.ysize, 1, 0  # planar XYB behind the loop filters
    p.global_scale, p.quant_dc = dcg.global_scale, dcg.quant_dc
    p.x_dm_multiplier, p.b_dm_multiplier = fh.x_dm_multiplier, fh.b_dm_multiplier
    p.quant_biases[:] = ih.quant_biases[:]
    p.cfl_base_x, p.cfl_base_b, p.cfl_color_factor = dcg.cfl_base_x, dcg.cfl_base_b, dcg.cfl_color_factor
    C.memmove(C.byref(p.lf), C.byref(fh.lf), C.sizeof(fh.lf))
    p.opsin_biases[:] = ih.opsin_biases[:]
    s = f32(255.0) / f32(ih.intensity_target)
    p.inverse_opsin_matrix[:] = [float(f32(v) * s) for v in ih.inverse_opsin_matrix]
    p.used_acs = used.value
    table = O.dequant_tables(encs)
    assert table is not None
    fr = O.Frame(p, coeffs, acs, rq, sharp, ytox, ytob, [np.ascontiguousarray(d) for d in dc], table)
    return fr, fr.decode(threads=4), patches


@pytest.mark.parametrize("size,distance", STREAMS)
def test_bytes_to_pixels_without_a_device(L, ref, jxl_ref, walks, size, distance):
    """Proves the Modular frame decode and the dictionary decode before any GPU run: the product's reference planes
    and dictionary, blended by the numpy model into the oracle's filtered XYB, give JxlDecoder's pixels."""
    import oracle as O
    ts, RL = jxl_ref
    w = walks[(size, distance)]
    want = ts.jxl_decode(RL, w.cs.tobytes())
    assert want.shape == (size[1], size[0], 3)
    fr, xyb, patches = _filtered_xyb(L, w)
    rc, sheet, _, why = w.reference_frame(L)
    assert rc == 0, why
    blended = pm.apply(xyb, patches, {int(w.frames[0][0].save_as_reference): sheet})
    assert np.abs(blended - xyb).max() > 0.05  # the patches carry the glyphs: without them the test could not pass
    linear = fr.xyb_to_rgb([np.ascontiguousarray(blended[c]) for c in range(3)])
    got = O.pack_output(dict(transfer=abi.TF_SRGB, sample_type=abi.SAMPLE_F32, num_channels=3, bits_per_sample=32), linear)
    scale = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got - want).max()) / scale
    without = O.pack_output(dict(transfer=abi.TF_SRGB, sample_type=abi.SAMPLE_F32, num_channels=3, bits_per_sample=32),
                            fr.xyb_to_rgb([np.ascontiguousarray(xyb[c]) for c in range(3)]))
    print("max error / range: %.3g (without the patches: %.3g)" % (err, float(np.abs(without - want).max()) / scale))
    assert err <= TIGHT


def test_list_round_trip(L, walks):
    w = walks[STREAMS[1]]
    rc, h, _ = w.dictionary(L)
    assert rc == 0
    lst, nec, uses_ec, ec = abi.patches_list(h, L)
    abi.patches_destroy(h, L)
    fh1 = w.frames[1][0]
    rc, h2 = abi.patches_from_list(lst, fh1.xsize_blocks * 8, fh1.ysize_blocks * 8, w.ref_sizes(), L=L)
    assert rc == 0
    try:
        lst2, nec2, uses2, _ = abi.patches_list(h2, L)
    finally:
        abi.patches_destroy(h2, L)
    assert lst2 == lst and nec2 == nec == 0 and uses2 == uses_ec
    # with extra channels: the per-channel blendings round-trip, and they decide uses_extra_channels
    some = [dict(p, mode=pm.REPLACE) for p in lst[:3]]
    for ec_modes, uses in (([[0, 0, 0], [0, 0, 0]], False), ([[0, 0, 0], [2, 0, 0]], True)):
        rc, h3 = abi.patches_from_list(some, 600, 400, w.ref_sizes(), num_extra_channels=2, ec_blendings=[ec_modes] * 3, L=L)
        assert rc == 0
        got, nec3, uses3, ec3 = abi.patches_list(h3, L)
        abi.patches_destroy(h3, L)
        assert got == some and nec3 == 2 and uses3 == uses and ec3.tolist() == [ec_modes] * 3
    # an alpha mode uses the extra channels exactly when the image has some; the clamp flag is kept where it is coded
    for nec_in, uses in ((0, False), (1, True)):
        rc, h4 = abi.patches_from_list([dict(some[0], mode=pm.BLEND_ABOVE, clamp=1), dict(some[1], mode=pm.ADD, clamp=1)], 600, 400,
                                       w.ref_sizes(), num_extra_channels=nec_in, ec_blendings=[[[0, 0, 0]] * nec_in] * 2, L=L)
        assert rc == 0
        got, _, uses4, _ = abi.patches_list(h4, L)
        abi.patches_destroy(h4, L)
        assert uses4 == uses and got[0]["clamp"] == 1 and got[1]["clamp"] == 0
    rc, h5 = abi.patches_from_list([], 600, 400, {}, L=L)  # an empty dictionary
    assert rc == 0 and abi.patches_list(h5, L)[0] == []
    abi.patches_destroy(h5, L)


GOOD = dict(ref=1, ref_x0=2, ref_y0=3, xsize=5, ysize=4, x=10, y=20, mode=pm.ADD)
REFS = {1: (18, 19)}


@pytest.mark.parametrize("change,why", [
    (dict(ref=4), "reference id >= 4"),
    (dict(ref=2), "an empty slot"),
    (dict(ref_x0=14), "a rectangle outside the reference frame (x)"),
    (dict(ref_y0=16), "a rectangle outside the reference frame (y)"),
    (dict(x=60), "a patch outside the frame (x)"),
    (dict(y=45), "a patch outside the frame (y)"),
    (dict(mode=8), "blend mode >= 8"),
    (dict(xsize=0), "an empty rectangle (sizes are coded minus one)"),
])
def test_rejections_through_the_list(L, change, why):
    rc, h = abi.patches_from_list([GOOD], 64, 48, REFS, L=L)
    assert rc == 0
    abi.patches_destroy(h, L)
    rc, h = abi.patches_from_list([GOOD, dict(GOOD, **change)], 64, 48, REFS, L=L)
    assert rc == BAD and not h.value, why


def test_rejections_that_need_extra_channels_or_counts(L):
    # alpha channel out of range: read (and checked) only with more than one extra channel
    ecb = [[[0, 0, 0], [0, 0, 0]]]
    rc, h = abi.patches_from_list([dict(GOOD, mode=pm.BLEND_ABOVE, alpha_channel=1)], 64, 48, REFS, 2, ecb, L=L)
    assert rc == 0
    abi.patches_destroy(h, L)
    assert abi.patches_from_list([dict(GOOD, mode=pm.BLEND_ABOVE, alpha_channel=2)], 64, 48, REFS, 2, ecb, L=L)[0] == BAD
    assert abi.patches_from_list([dict(GOOD, mode=pm.REPLACE)], 64, 48, REFS, 2, [[[0, 0, 0], [6, 2, 0]]], L=L)[0] == BAD
    assert abi.patches_from_list([dict(GOOD, mode=pm.REPLACE)], 64, 48, REFS, 2, [[[0, 0, 0], [9, 0, 0]]], L=L)[0] == BAD
    # too many patches: 4 * (1024 + pixels / 4) of them at the most, and a quarter as many per extra channel and one
    one = dict(ref=1, xsize=1, ysize=1, x=0, y=0, mode=pm.ADD)
    cap = 4 * (1024 + 8 * 8 // 4)
    rc, h = abi.patches_from_list([one] * cap, 8, 8, REFS, L=L)
    assert rc == 0
    abi.patches_destroy(h, L)
    assert abi.patches_from_list([one] * (cap + 1), 8, 8, REFS, L=L)[0] == BAD
    n = cap * 4 // 5 + 1  # blendings = patches * (1 + 4 extra channels) > 4 * cap
    assert abi.patches_from_list([one] * n, 8, 8, REFS, 4, [[[0, 0, 0]] * 4] * n, L=L)[0] == BAD


class Bits:
    """LSB-first bit writer for hand-made dictionaries."""

    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, nbits):
        assert 0 <= value < (1 << nbits) or nbits == 0
        self.v |= value << self.n
        self.n += nbits

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8 + 4, "little")  # (the readers may look a few bytes ahead)


HEADER_BITS = 38


def handmade_dictionary(values, tokens=(0, 1, 2, 3)):
    """A patch dictionary whose hybrid-uint values are `values`, in stream order, every context on one prefix-coded
    histogram: LZ77 off; a simple context map with 0 bits per entry; prefix codes; split_exponent 0 (token 0 = 0, token
    t = the values of t bits, t - 1 of them raw); an alphabet of 16 tokens of which the four in `tokens` (ascending)
    have codes, each 2 bits long."""
    assert list(tokens) == sorted(tokens) and len(tokens) == 4
    b = Bits()
    b.put(0, 1)              # LZ77 off
    b.put(1, 1), b.put(0, 2)  # simple context map, 0 bits per entry
    b.put(1, 1)              # prefix codes
    b.put(0, 4)              # split_exponent 0: msb_in_token and lsb_in_token take 0 bits
    b.put(1, 1), b.put(3, 4), b.put(7, 3)  # alphabet size 7 + (1 << 3) + 1 = 16
    b.put(1, 2), b.put(3, 2)  # simple code, 4 symbols
    for t in tokens:
        b.put(t, 4)
    b.put(0, 1)              # ... all of length 2
    assert b.n == HEADER_BITS
    for v in values:
        token = v.bit_length()
        code = tokens.index(token)
        b.put((code >> 1) & 1, 1), b.put(code & 1, 1)  # canonical code, first bit first
        if token > 1:
            b.put(v - (1 << (token - 1)), token - 1)
    return b.bytes()


def test_rejections_through_a_handmade_stream(L):
    """The decoder's own checks, on streams written here: a valid dictionary first (the writer is right), then the
    failures a list cannot express -- a negative coordinate after a delta -- and those it can, through the stream."""
    refs = {1: (6, 6)}
    # 1 reference patch: slot 1, rectangle (0, 1) 2x3, 2 placements: (4, 5) kReplace; delta (-4, +2) -> (0, 7) kMul + clamp
    good = [1, 1, 0, 1, 1, 2, 1, 4, 5, pm.REPLACE, 7, 4, pm.MUL, 1]
    rc, h, end = abi.patches_decode(handmade_dictionary(good), 0, 16, 16, refs, L=L)
    assert rc == 0
    lst = abi.patches_list(h, L)[0]
    abi.patches_destroy(h, L)
    assert lst == [dict(ref=1, ref_x0=0, ref_y0=1, xsize=2, ysize=3, x=4, y=5, mode=pm.REPLACE, alpha_channel=0, clamp=0),
                   dict(ref=1, ref_x0=0, ref_y0=1, xsize=2, ysize=3, x=0, y=7, mode=pm.MUL, alpha_channel=0, clamp=1)]
    assert end == HEADER_BITS + sum(2 + max(0, v.bit_length() - 1) for v in good)

    def rc_of(values, xsize=16, ysize=16, r=refs, nec=0):
        rc, h, _ = abi.patches_decode(handmade_dictionary(values), 0, xsize, ysize, r, nec, L=L)
        assert rc != 0 and not h.value
        return rc
    assert rc_of([1, 1, 0, 1, 1, 2, 1, 3, 5, pm.REPLACE, 7, 4, pm.REPLACE]) == BAD   # x = 3 - 4
    assert rc_of([1, 1, 0, 1, 1, 2, 1, 4, 1, pm.REPLACE, 1, 3, pm.REPLACE]) == BAD   # y = 1 - 2
    assert rc_of([1, 4] + good[2:]) == BAD                                            # reference id >= 4
    assert rc_of([1, 2] + good[2:]) == BAD                                            # an empty slot
    assert rc_of([1, 1, 5] + good[3:]) == BAD                                         # x0 + xsize > 6
    assert rc_of([1, 1, 0, 4] + good[4:]) == BAD                                      # y0 + ysize > 6
    assert rc_of(good, xsize=5) == BAD and rc_of(good, ysize=9) == BAD                # a patch outside the frame
    assert rc_of([1, 1, 0, 1, 1, 2, 0, 4, 5, pm.BLEND_ABOVE, 2, 0, 0, 0], nec=2) == BAD  # alpha channel 2 of 2
    # too many reference patches for an 8 x 8 frame: 1024 + pixels / 4 = 1040 at the most -- and exactly that many pass
    # this check (the stream then ends: BAD all the same, but only after 1040 is accepted and 1041 is not)
    few = (0, 1, 2, 11)
    ok_head = handmade_dictionary([1040, 1, 0, 0, 0, 0, 0, 0, 0, pm.ADD], few)
    rc, h, _ = abi.patches_decode(ok_head + bytes(4096), 0, 8, 8, refs, L=L)
    assert rc == BAD and not h.value  # (the second reference patch names slot 0, which is empty)
    assert abi.patches_decode(handmade_dictionary([1041], few), 0, 8, 8, refs, L=L)[0] == BAD
    # too many patches: 4 * 1040 = 4160 placements at the most, a count of 4161 (coded minus one) fails
    many = (0, 1, 2, 13)
    assert abi.patches_decode(handmade_dictionary([1, 1, 0, 0, 0, 0, 4160], many), 0, 8, 8, refs, L=L)[0] == BAD


UNSUPPORTED_HEADERS = [
    (dict(num_groups=2), "more than one group"),
    (dict(flags=1), "flags"),
    (dict(upsampling=2), "upsampled"),
    (dict(num_passes=2), "more than one pass"),
    (dict(save_before_color_transform=0), "behind the colour transform"),
    (dict(num_extra_channels=1), "extra channels"),
    (dict(color_transform=1), "not XYB"),
    (dict(gab=1), "loop filter"),
    (dict(epf_iters=1), "loop filter"),
]


@pytest.mark.parametrize("change,message", UNSUPPORTED_HEADERS)
def test_reference_frames_outside_the_front_end(L, walks, change, message):
    w = walks[STREAMS[2]]
    fh = abi.FrameHeader()
    C.memmove(C.byref(fh), C.byref(w.frames[0][0]), C.sizeof(fh))
    for k, v in change.items():
        setattr(fh.lf if k in ("gab", "epf_iters") else fh, k, v)
    rc, _, _, why = w.reference_frame(L, fh=fh)
    assert rc == UNSUPPORTED and message in why, why


def modular_frame_with_transform(kind):
    """The head of a Modular frame's only section, written bit by bit, up to a transform the front-end does not take:
    default DC quant, no global tree, a group header with a local tree, the default WP header and ONE transform."""
    b = Bits()
    b.put(1, 1)  # DequantMatrices::DecodeDC: all default
    b.put(0, 1)  # no global tree
    b.put(0, 1)  # GroupHeader::use_global_tree = 0
    b.put(1, 1)  # weighted::Header all default
    b.put(1, 2)  # nb_transforms: selector 1 = one transform
    if kind == "rct":
        b.put(0, 2)      # TransformId::kRCT
    elif kind == "squeeze":
        b.put(2, 2)      # TransformId::kSqueeze
    else:                # a palette with delta entries (lossy)
        b.put(1, 2)      # TransformId::kPalette
        b.put(0, 2), b.put(0, 3)    # begin_c = 0
        b.put(0, 2)                 # num_c = 1
        b.put(0, 2), b.put(16, 8)   # nb_colors = 16
        b.put(1, 2), b.put(2, 8)    # nb_deltas = 1 + 2
        b.put(0, 4)                 # predictor Zero
    return np.frombuffer(b.bytes() + bytes(32), np.uint8).copy()


@pytest.mark.parametrize("kind", ["rct", "squeeze", "delta_palette"])
def test_reference_frames_with_a_transform_outside_the_front_end(L, walks, kind):
    w = walks[STREAMS[2]]
    rc, _, _, why = w.reference_frame(L, data=modular_frame_with_transform(kind))
    assert rc == UNSUPPORTED and "transform" in why, (rc, why)


def test_a_palette_without_deltas_is_not_refused_as_a_transform(L, walks):
    """The control of the test above: the same bits with nb_deltas = 0 pass the group header (the stream then ends: BAD)."""
    w = walks[STREAMS[2]]
    b = Bits()
    for v, n in ((1, 1), (0, 1), (0, 1), (1, 1), (1, 2), (1, 2), (0, 2), (0, 3), (0, 2), (0, 2), (16, 8), (0, 2), (0, 4)):
        b.put(v, n)
    rc, _, _, why = w.reference_frame(L, data=np.frombuffer(b.bytes(), np.uint8).copy())
    assert rc == BAD and why == "", (rc, why)


def test_a_vardct_frame_is_no_reference_frame(L, walks):
    w = walks[STREAMS[2]]
    fh1, sections = w.frames[1]
    planes = np.zeros((3, fh1.ysize, fh1.xsize), np.float32)
    ptrs = (C.c_void_p * 3)(*[planes[k].ctypes.data for k in range(3)])
    pos = C.c_size_t(0)
    s0 = sections[0]
    assert L.jxlhip_modular_frame_decode(s0.ctypes.data, len(s0), C.byref(pos), C.byref(fh1), ptrs, fh1.xsize, None) == -1


@pytest.mark.parametrize("size,distance", STREAMS)
def test_truncation_at_every_byte(L, walks, size, distance):
    w = walks[(size, distance)]
    s0 = w.frames[0][1][0]
    for n in range(len(s0)):
        rc, _, _, _ = w.reference_frame(L, data=s0[:n].copy())
        assert rc == BAD, n
    rc, h, end = w.dictionary(L)
    abi.patches_destroy(h, L)
    bundle = w.frames[1][1][0][:(end + 7) // 8].tobytes()
    for n in range(len(bundle)):
        rc, h, _ = abi.patches_decode(bundle[:n], 0, w.frames[1][0].xsize_blocks * 8, w.frames[1][0].ysize_blocks * 8,
                                      w.ref_sizes(), L=L)
        assert rc == BAD and not h.value, n


def test_whole_files_report_the_visible_frame(L, walks, ref):
    """jxlhip_codestream_basic_info walks the frames (no device needed): a patches file is accepted and described by
    its visible frame; other multi-frame files stay outside."""
    for (size, d), w in walks.items():
        info = abi.CodestreamInfo()
        assert L.jxlhip_codestream_basic_info(w.cs.ctypes.data, len(w.cs), C.byref(info)) == 0
        assert (info.xsize, info.ysize, info.upsampling) == (size[0], size[1], 1)
    cs = ref.feature_stream("animation", xsize=64, ysize=48, seed=5)
    assert L.jxlhip_codestream_basic_info(cs, len(cs), C.byref(abi.CodestreamInfo())) == UNSUPPORTED
    # a damaged reference frame fails the file
    w = walks[STREAMS[2]]
    cs = w.cs.copy()
    at = len(cs) - sum(len(s) for s in w.frames[1][1]) - 200  # inside frame 0's section
    cs[at: at + 20] ^= 0x5A
    assert L.jxlhip_codestream_basic_info(cs.ctypes.data, len(cs), C.byref(abi.CodestreamInfo())) != 0


def test_damaged_patch_files_under_asan_ubsan(ref, walks, tmp_path):
    """tests/fuzz/fuzz_patches.cc: frame 0 and the dictionary of the four streams, truncated at every byte and with
    every single bit flipped, in a stand-alone program built with -fsanitize=address,undefined."""
    out = str(tmp_path / "fuzz_patches")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-DJXLHIP_NO_DEVICE", os.path.join(ROOT, "tests", "fuzz", "fuzz_patches.cc"),
           os.path.join(ROOT, "libjxl_amd", "csrc", "entropy.cc"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    paths = []
    for i, w in enumerate(walks.values()):
        paths.append(str(tmp_path / ("p%d.jxl" % i)))
        with open(paths[-1], "wb") as f:
            f.write(w.cs.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([out] + paths, capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-4000:])
    ok, rejected = map(int, r.stdout.split())
    assert rejected > ok > 0  # the damage is real, and a flipped sample or offset bit still decodes
