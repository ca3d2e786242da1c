"""The frame-header rewriter for images with extra channels (tests/alpha_layer_streams.py) and the alpha blending model
(tests/alpha_blending_model.py) against the reference's public JxlDecoder, on the CPU, before any kernel is trusted:
every coded frame of a spliced layered still is decoded alone as a one-frame file (float RGBA in the original's
encoding), the model blends them through the reference's slots, and the result must equal JxlDecoder's coalesced frame
of the spliced file BIT FOR BIT, colour and alpha.

Shapes: a 203 x 67 canvas (no multiple of 4) and 72 x 40 layers at origins inside, negative, and crossing the right and
the bottom edge.  The alpha planes have five levels (0, 1 and three between) with zeroes in the corners, so layers and
canvas overlap where both alphas are 0: the rnew_a = 0 branch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from libjxl_amd import abi

import alpha_blending_model as am

W, H = 203, 67
INFO = {8: [dict(is_alpha=1, alpha_associated=0)], 16: [dict(is_alpha=1, alpha_associated=0)],
        "premul": [dict(is_alpha=1, alpha_associated=1)]}
A_BLEND = [dict(mode=am.BLEND, alpha_channel=0)]


def cases():
    """name -> (image header: 8 | 16 | "premul", frames); a frame names its stream by key ("A", "A2": canvases, "B", "B2":
    72 x 40 layers) and carries splice_ec's fields."""
    c = {}
    base = dict(stream="A", save_as_reference=1)
    for bits in (8, "premul"):
        for clamp in (0, 1):
            c["blend-%s-clamp%d" % (bits, clamp)] = (bits, [base, dict(stream="B", crop=(37, 21), mode=am.BLEND, clamp=clamp, source=1,
                                                                       ec=[dict(mode=am.BLEND, clamp=clamp, alpha_channel=0)])])
    c["weighted-add"] = (8, [base, dict(stream="B", crop=(37, 21), mode=am.ALPHA_WEIGHTED_ADD, source=1, ec=A_BLEND)])
    c["weighted-add-clamp-alpha-weighted-add"] = (8, [base, dict(stream="B", crop=(37, 21), mode=am.ALPHA_WEIGHTED_ADD, clamp=1, source=1,
                                                                 ec=[dict(mode=am.ALPHA_WEIGHTED_ADD, alpha_channel=0)])])
    c["mul-clamp"] = (8, [base, dict(stream="B", crop=(37, 21), mode=am.MUL, clamp=1, source=1, ec=[dict(mode=am.MUL, clamp=1)])])
    c["mul"] = (8, [base, dict(stream="B", crop=(37, 21), mode=am.MUL, source=1, ec=A_BLEND)])
    # the alpha channel's own mode beside a colour that does not override it
    for name, mode in (("blend", am.BLEND), ("add", am.ADD), ("replace", am.REPLACE)):
        c["alpha-" + name] = (8, [base, dict(stream="B", crop=(37, 21), mode=am.ADD, source=1, ec=[dict(mode=mode, alpha_channel=0)])])
    # ... and beside colour kBlend, which writes the new alpha over it
    c["blend-over-alpha-add"] = (8, [base, dict(stream="B", crop=(37, 21), mode=am.BLEND, source=1, ec=[dict(mode=am.ADD)])])
    for origin in ((-20, -9), (170, 50)):
        c["blend-at-%d,%d" % origin] = (8, [base, dict(stream="B", crop=origin, mode=am.BLEND, source=1, ec=A_BLEND)])
        c["premul-at-%d,%d" % origin] = ("premul", [base, dict(stream="B", crop=origin, mode=am.BLEND, source=1, ec=A_BLEND)])
    c["empty-source"] = (8, [base, dict(stream="B", crop=(37, 21), mode=am.BLEND, source=2, ec=A_BLEND)])
    c["chain-of-three"] = (8, [base, dict(stream="B", crop=(37, 21), mode=am.BLEND, source=1, ec=A_BLEND, save_as_reference=1),
                               dict(stream="B2", crop=(-20, -9), mode=am.BLEND, source=1, ec=A_BLEND, save_as_reference=1),
                               dict(stream="B", crop=(170, 50), mode=am.BLEND, source=1, ec=A_BLEND)])
    c["alpha-from-another-slot"] = (8, [base, dict(stream="A2", save_as_reference=2),
                                        dict(stream="B", crop=(37, 21), mode=am.BLEND, source=1,
                                             ec=[dict(mode=am.BLEND, alpha_channel=0, source=2)])])
    c["sixteen-bit"] = (16, [base, dict(stream="B", crop=(37, 21), mode=am.BLEND, source=1, ec=A_BLEND)])
    return c


CASES = cases()


def seam_library(oracle):
    """The reference's JxlDecoder library (integration/build_seam.py), or a skip where it cannot exist."""
    if not oracle.ref_available():
        pytest.skip("oracle/_ref not available")
    oracle.ref_lib()
    import test_seam
    sys.path.insert(0, os.path.join(test_seam.ROOT, "integration"))
    import build_seam
    prebuilt = [os.path.join(build_seam.B.OUT, n) for n in ("libjxl_dec_ref.so", "libjxl_dec_hip.so")]
    if not build_seam.available() and not all(os.path.exists(p) for p in prebuilt):
        pytest.skip("reference tree not present and no prebuilt seam libraries")
    return test_seam.load(build_seam.build()[0])


def make_kit(oracle):
    """(L, RL, streams[header][key], pixels[header][key] = (colour, planes) of the stream decoded alone by JxlDecoder)."""
    import alpha_layer_streams as als
    import layer_streams as ls
    RL = seam_library(oracle)
    L = abi.load_library()
    streams, pixels = {}, {}
    for bits in (8, 16):
        s = {k: oracle.RealStream(seed=seed, xsize=w, ysize=h, alpha_bits=bits, alpha_levels=5).codestream.tobytes()
             for k, (w, h, seed) in dict(A=(W, H, 3), A2=(W, H, 6), B=(72, 40, 7), B2=(72, 40, 9)).items()}
        streams[bits] = s
        pixels[bits] = {}
        for k, cs in s.items():
            px = ls.jxl_decode_frames(RL, cs, channels=4)[0][0]
            pair = (np.ascontiguousarray(px[..., :3]), np.ascontiguousarray(px[..., 3])[None])
            for a in pair:
                a.setflags(write=False)
            pixels[bits][k] = pair
    # premultiplied at file level: the 16-bit streams (their channel info is not all_default) with the bit set; a
    # frame's own samples do not depend on it
    streams["premul"] = {k: als.set_alpha_associated(cs) for k, cs in streams[16].items()}
    pixels["premul"] = pixels[16]
    return L, RL, streams, pixels


@pytest.fixture(scope="module")
def kit(oracle):
    return make_kit(oracle)


def build_case(kit, name):
    """(the spliced file, the model's frames with their pixels, the header key)."""
    import alpha_layer_streams as als
    L, RL, streams, pixels = kit
    header, frames = CASES[name]
    cs = als.splice_ec(L, streams[header]["A"], [dict(f, stream=streams[header][f["stream"]]) for f in frames])
    return cs, [dict(f, pixels=pixels[header][f["stream"]]) for f in frames], header


def same(got, want):
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_the_alpha_planes_are_worth_the_test(kit):
    _, _, _, pixels = kit
    for bits in (8, 16):
        a, b = pixels[bits]["A"][1][0], pixels[bits]["B"][1][0]
        for p in (a, b):
            assert float(p.min()) == 0.0 and float(p.max()) == 1.0 and np.any((p > 0.0) & (p < 1.0))
        # the layer at (37, 21) over the canvas: pixels where both alphas are 0 (rnew_a = 0), and pixels where they are not
        under = a[21:61, 37:109]
        assert np.any((under == 0.0) & (b == 0.0)) and np.any((under > 0.0) & (b > 0.0)) and np.any((under == 0.0) & (b > 0.0))


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_equals_the_reference_on_a_spliced_file(kit, name):
    import layer_streams as ls
    L, RL, streams, pixels = kit
    cs, frames, header = build_case(kit, name)
    got = ls.jxl_decode_frames(RL, cs, channels=4)  # (raises when the reference does not accept the file)
    assert len(got) == 1 and got[0][1]["is_last"] == 1
    color, planes = am.blend_sequence(frames, (W, H), INFO[header])
    px = got[0][0]
    assert same(np.ascontiguousarray(px[..., :3]), color), float(np.abs(px[..., :3] - color).max())
    assert same(np.ascontiguousarray(px[..., 3]), planes[0]), float(np.abs(px[..., 3] - planes[0]).max())
    assert not np.array_equal(color, pixels[header]["A"][0])  # the layer shows


def test_premultiplied_and_straight_differ(kit):
    """The premultiplied files are no copies of the straight ones: the bit reaches the blend."""
    a = am.blend_sequence(build_case(kit, "blend-premul-clamp0")[1], (W, H), INFO["premul"])[0]
    b = am.blend_sequence(build_case(kit, "blend-premul-clamp0")[1], (W, H), INFO[16])[0]
    assert not np.array_equal(a, b)


def test_the_header_bit_is_reported(kit):
    L, RL, streams, _ = kit
    for key, want in ((16, 0), ("premul", 1)):
        cs = streams[key]["A"]
        info = abi.CodestreamInfo()
        assert L.jxlhip_codestream_basic_info(cs, len(cs), C.byref(info)) == 0
        assert (info.alpha_bits, info.alpha_premultiplied) == (16, want)
    assert streams["premul"]["A"] != streams[16]["A"] and len(streams["premul"]["A"]) == len(streams[16]["A"])
