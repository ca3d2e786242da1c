"""The frame-level inputs synth.synth_frame keeps at one value (global_scale, quant_dc, the qm scales, CfL, opsin, the
loop-filter fields) and the side info it keeps in narrow ranges, set away from those values (frames.PARAM_SETS).

CPU tier: at every set the C oracle equals the libjxl reference bit for bit through both of the reference's executors,
as test_reference_parity.py holds it at the defaults; every knob of every set moves the decoded frame by far more than
the GPU tier's bar (test_gpu_frame_params.py), so a kernel that ignored the knob would fail there; and the sigma
boundary cells of the quant-field sets really exist."""
import numpy as np
import pytest

import frames

SIZE = (520, 300)
SETS = sorted(frames.PARAM_SETS)
GPU_BAR = 2e-5   # test_gpu_frame_params.py: per channel, relative to the channel's own magnitude
TEETH = 50 * GPU_BAR


@pytest.fixture(scope="module")
def ref(oracle):
    if not oracle.ref_available():
        pytest.skip("oracle/_ref not built and the reference tree absent")
    oracle.ref_lib()
    return oracle


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def channel_scale(img):
    """max|img_c| per channel of a (H, W, 3) frame, floored like the GPU bar."""
    return np.maximum(np.abs(img).reshape(-1, 3).max(axis=0), 1e-3)


@pytest.mark.parametrize("name", SETS)
def test_oracle_bit_exact_with_reference(ref, name):
    _, _, fr = frames.make_param_case(*SIZE, name)
    o = fr.decode(threads=4)
    assert np.isfinite(o).all()
    assert np.array_equal(bits(o), bits(fr.decode_ref(threads=4)))
    assert np.array_equal(bits(o), bits(fr.decode_ref(threads=1, simple_pipeline=True)))


@pytest.mark.parametrize("name", ["cfl", "opsin", "quant_hi"])
def test_oracle_bit_exact_with_reference_planar_xyb(ref, name):
    # the IDCT planes without filters (what the MFMA tests of the GPU tier compare)
    _, _, fr = frames.make_param_case(*SIZE, name, gab=False, epf_iters=0, output_kind=0)
    assert np.array_equal(bits(fr.decode()), bits(fr.decode_ref()))


@pytest.mark.parametrize("name", SETS)
def test_teeth_every_knob_moves_the_frame(oracle, name):
    """Each knob set back to synth's default moves at least one channel by >= 1e-3 of its magnitude (50x the GPU
    bar).  A knob that only the DC dequantisation reads is checked on jxlhip_dequant_dc's reference instead."""
    s = frames.PARAM_SETS[name]
    _, _, fr = frames.make_param_case(*SIZE, name)
    want = fr.decode(threads=4)
    scale = channel_scale(want)
    for k in s["knobs"]:
        if k in frames.DC_ONLY_KNOBS:
            continue
        _, _, fr1 = frames.make_param_case(*SIZE, name, revert=(k,))
        moved = np.abs(fr1.decode(threads=4).astype(np.float64) - want).reshape(-1, 3).max(axis=0) / scale
        assert moved.max() >= TEETH, (name, k, moved.tolist())


def dc_mul(params):
    inv_gs = np.float32(65536.0 / params["global_scale"])
    return np.array([np.float32(inv_gs / np.float32(params["quant_dc"])) * np.float32(v)
                     for v in (1 / 4096.0, 1 / 512.0, 1 / 256.0)], np.float32)


@pytest.mark.parametrize("name", ["quant_hi", "quant_lo"])
def test_teeth_dc_dequant_knobs(ref, name):
    """global_scale and quant_dc set the DC step (quantizer.h:133-139): each moves the reference's DequantDC."""
    rng = np.random.default_rng(8)
    q = [rng.integers(-300, 300, size=(23, 31)).astype(np.int32) for _ in range(3)]
    p, _, _ = frames.make_param_case(8, 8, name)
    want = ref.ref_dequant_dc(q, dc_mul(p), 0.0, 0.0, 1)
    for k in ("global_scale", "quant_dc"):
        p1, _, _ = frames.make_param_case(8, 8, name, revert=(k,))
        got = ref.ref_dequant_dc(q, dc_mul(p1), 0.0, 0.0, 1)
        for c in range(3):
            assert np.abs(got[c] - want[c]).max() >= TEETH * np.abs(want[c]).max(), (k, c)


@pytest.mark.parametrize("name", ["qfield_1", "qfield_3"])
def test_sigma_boundary_cells_exist(oracle, name):
    """The custom sharpness LUT puts some cells' inv_sigma on kMinSigma and on the floats either side of it (the
    copy-or-filter decision of the EPF stages, stage_epf.cc); the quant field reaches raw_quant 1 and 256 under
    every sharpness value."""
    params, t, fr = frames.make_param_case(*SIZE, name)
    s = fr.compute_sigma()
    k = frames.K_MIN_SIGMA
    below, _, above = frames.min_sigma_targets()
    assert below == np.nextafter(k, np.float32(-np.inf))  # the float just below
    for v in (below, k, above):
        assert (s == v).any(), v
    # the float just above kMinSigma is no quotient 1 / sigma of a float sigma: above is the nearest one
    up1 = np.nextafter(k, np.float32(0))
    assert above == np.nextafter(up1, np.float32(0))
    sig = (np.float32(1 / -3.9052429).view(np.int32) + np.arange(-1000, 1000, dtype=np.int32)).view(np.float32)
    assert not (np.float32(1) / sig == up1).any()
    # the same values from the formula in numpy
    cells = frames.min_sigma_cells(params["global_scale"], params["epf_quant_mul"])
    got = [frames.inv_sigma_f32(params["global_scale"], params["epf_quant_mul"], qv, np.float32(params["epf_sharp_lut"][sv]))
           for (qv, _), sv in zip(cells, frames.MIN_SIGMA_SHARPNESS)]
    assert got == frames.min_sigma_targets()
    acs, q, sh = t["ac_strategy"].numpy(), t["raw_quant"].numpy(), t["epf_sharpness"].numpy()
    first = (acs & 1) == 1
    for qv in (1, 256):
        assert set(sh[first & (q == qv)].tolist()) == set(range(8)), qv


def test_extreme_coefficients_present(oracle):
    _, t, _ = frames.make_param_case(*SIZE, "coeff_i16")
    for c in range(3):
        a = t["coeffs"][c].numpy()
        assert a.max() == 32767 and a.min() == -32768
    _, t, _ = frames.make_param_case(*SIZE, "coeff_i32")
    for c in range(3):
        a = t["coeffs"][c].numpy().astype(np.int64)
        big = a[np.abs(a) > (1 << 24)]
        assert len(big) and (big.astype(np.float32).astype(np.int64) != big).any()  # not exact in f32


def test_cfl_maps_span_int8(oracle):
    _, t, _ = frames.make_param_case(*SIZE, "cfl")
    for k in ("ytox_map", "ytob_map"):
        m = t[k].numpy()
        assert m.min() == -128 and m.max() == 127


def test_default_make_case_is_unchanged(oracle):
    """frames.make_case still hands back synth_frame's frame, untouched (the product inputs bench.py draws)."""
    from libjxl_amd import synth
    p, t, _ = frames.make_case(264, 136, mix=synth.MIX_ALL, gab=True, epf_iters=1, seed=5)
    p0, t0 = synth.synth_frame(264, 136, mix=synth.MIX_ALL, gab=True, epf_iters=1, seed=5)
    assert p == p0
    for k in t:
        a, b = (t[k], t0[k]) if isinstance(t[k], list) else ([t[k]], [t0[k]])
        assert all(np.array_equal(x.numpy(), y.numpy()) for x, y in zip(a, b)), k
