"""The frame-header rewriter (tests/layer_streams.py) and the blending model (tests/blending_model.py) against the
reference's public JxlDecoder, on the CPU, before any GPU is involved: a canvas stream and a small stream are decoded
each on its own, as float in the original's encoding, and blended by the model; the result must equal JxlDecoder's
decode of the spliced two-layer file BIT FOR BIT -- every mode, with and without clamp, an empty source, and origins
inside, at (0, 0), negative, overhanging right and bottom, and wholly outside."""
import os
import sys

import numpy as np
import pytest

from libjxl_amd import abi

import blending_model as bm

W, H = 203, 137
ORIGINS = [(37, 21), (0, 0), (-20, -9), (170, 120), (210, 0)]
CASES = [(bm.REPLACE, 0), (bm.ADD, 0), (bm.MUL, 0), (bm.MUL, 1), (bm.BLEND, 0), (bm.ALPHA_WEIGHTED_ADD, 0)]


@pytest.fixture(scope="module")
def kit(oracle):
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
    L = abi.load_library()
    canvas = oracle.feature_stream("plain", xsize=W, ysize=H, seed=5, distance=1.0)
    small = oracle.feature_stream("plain", xsize=72, ysize=40, seed=7, distance=1.0)
    a, b = test_seam.jxl_decode(RL, canvas), test_seam.jxl_decode(RL, small)
    assert a.shape == (H, W, 3) and b.shape == (40, 72, 3)
    a.setflags(write=False)
    b.setflags(write=False)
    return L, RL, canvas, small, a, b


@pytest.mark.parametrize("origin", ORIGINS)
@pytest.mark.parametrize("mode,clamp", CASES)
def test_model_equals_the_reference_on_a_spliced_file(kit, mode, clamp, origin):
    import layer_streams as ls
    L, RL, canvas, small, a, b = kit
    # a zero-duration layer saved into slot 1, then the displayed frame blended over it
    cs = ls.splice(L, canvas, [dict(stream=canvas, save_as_reference=1),
                               dict(stream=small, crop=origin, mode=mode, clamp=clamp, source=1)])
    frames = ls.jxl_decode_frames(RL, cs)  # (raises when the reference does not accept the file)
    assert len(frames) == 1 and frames[0][1]["is_last"] == 1
    want = bm.blend(a, b, origin, mode, clamp)
    assert np.array_equal(frames[0][0].view(np.uint32), want.view(np.uint32)), float(np.abs(frames[0][0] - want).max())
    if origin != (210, 0) and mode != bm.MUL:
        assert not np.array_equal(want, a)  # the frame shows


@pytest.mark.parametrize("mode,clamp", CASES)
def test_empty_source_is_zeroes(kit, mode, clamp):
    import layer_streams as ls
    L, RL, canvas, small, a, b = kit
    cs = ls.splice(L, canvas, [dict(stream=canvas, save_as_reference=1),
                               dict(stream=small, crop=(37, 21), mode=mode, clamp=clamp, source=2)])  # nothing is in slot 2
    got = ls.jxl_decode_frames(RL, cs)[0][0]
    want = bm.blend(None, b, (37, 21), mode, clamp, size=(W, H))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_a_chain_of_three(kit):
    import layer_streams as ls
    L, RL, canvas, small, a, b = kit
    cs = ls.splice(L, canvas, [dict(stream=canvas, save_as_reference=1),
                               dict(stream=small, crop=(-20, -9), mode=bm.ADD, source=1, save_as_reference=1),
                               dict(stream=small, crop=(170, 120), mode=bm.MUL, clamp=1, source=1)])
    got = ls.jxl_decode_frames(RL, cs)[0][0]
    want = bm.blend(bm.blend(a, b, (-20, -9), bm.ADD), b, (170, 120), bm.MUL, True)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
