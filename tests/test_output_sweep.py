"""tests/output_sweep.py on the CPU: the sweep frame meets its population conditions for every format of the grid (on
the restatement's own linear decode; tests/test_gpu_output_encoding.py checks them again on the device's), and the
comparison function of the GPU tests rejects each kind of fault it is there to catch."""
import functools

import numpy as np
import pytest

import output_sweep as S
from libjxl_amd import abi

STAGE_LISTS = [(g, e) for g in (0, 1) for e in (0, 1, 2, 3) if (g, e) != (1, 3)] + [(1, 3)]


@functools.lru_cache(maxsize=None)
def linear(oracle, size, variant, gab, epf):
    _, _, fr = S.sweep_case(*size, variant, gab=bool(gab), epf_iters=epf, output_kind=1)
    lin = fr.decode()
    lin.setflags(write=False)
    return lin


@pytest.mark.parametrize("variant", [S.SIGNED, S.NONNEG])
def test_main_frame_meets_the_population_conditions(oracle, variant):
    lin = linear(oracle, S.MAIN_SIZE, variant, 0, 0)
    for f in S.format_grid():
        if S.variant_of(f) == variant:
            assert S.population_problems(f, lin, variant) == [], S.fmt_id(f)
    if variant == S.NONNEG:
        assert not (lin < 0).any() and not np.signbit(lin).any()


@pytest.mark.parametrize("gab,epf", STAGE_LISTS)
def test_kernel_frame_meets_the_population_conditions_behind_every_stage_list(oracle, gab, epf):
    """The loop filters move the planted values (Gaborish the rim of a block, an EPF pass a few ulps of its interior):
    the clusters are wide enough to keep both sides of every branch point populated."""
    for f in S.GENERAL_LIST + S.FIXED_LIST:
        variant = S.variant_of(f)
        assert S.population_problems(f, linear(oracle, S.KERNEL_SIZE, variant, gab, epf), variant) == [], S.fmt_id(f)


@pytest.mark.parametrize("size,gab,epf", [((13, 200), 1, 1), ((65, 33), 0, 0), ((130, 66), 0, 0), ((16, 264), 1, 1)])
def test_small_frames_meet_the_population_conditions(oracle, size, gab, epf):
    for f in S.GENERAL_LIST + S.STORE_SHAPES:
        variant = S.variant_of(f)
        assert S.population_problems(f, linear(oracle, size, variant, gab, epf), variant) == [], S.fmt_id(f)


# ---- the comparator ---------------------------------------------------------------------------------------------------

def _yardstick(oracle, f):
    lin = linear(oracle, S.KERNEL_SIZE, S.variant_of(f), 0, 0)
    return lin, oracle.pack_output(f, lin)


def _rejects(f, got, want, lin, **kw):
    with pytest.raises(AssertionError):
        S.compare(f, got, want, lin, **kw)


@pytest.mark.parametrize("f", S.GENERAL_LIST + S.FIXED_LIST + S.STORE_SHAPES, ids=S.fmt_id)
def test_comparator_accepts_the_yardstick_itself(oracle, f):
    lin, want = _yardstick(oracle, f)
    f32 = oracle.pack_output(S.fmt(f["transfer"], abi.SAMPLE_F32, 3, par=f["tf_param"]), lin)
    res = S.compare(f, want.copy(), want, lin, got_f32=f32, want_f32=f32)
    assert res["share"] == 0.0


@pytest.mark.parametrize("f", [S.fmt(abi.TF_SRGB, abi.SAMPLE_U8, 3), S.fmt(abi.TF_PQ, abi.SAMPLE_U16, 4, swap=1, par=1000.0),
                               S.fmt(abi.TF_SRGB, abi.SAMPLE_U16, 3, bits=10)], ids=S.fmt_id)
def test_comparator_rejects_moved_integer_samples(oracle, f):
    lin, want = _yardstick(oracle, f)
    top = (1 << f["bits_per_sample"]) - 1
    rng = np.random.default_rng(1)
    n = S.native(f, want).astype(np.int64)

    def back(a):  # the stored layout again
        a = a.astype(want.dtype)
        return a.byteswap() if f["swap_endianness"] else a
    assert np.array_equal(back(n), want)
    # 1 % of the samples one code away (at 16 bits a float32 ulp is 1 / 256 of a code: there the share the bar allows
    # is 12 % for sRGB and 19 % for PQ, and the fault injected is twice that)
    bar = 2 * (2 * S.ULP_BAR[f["transfer"]] * 2.0 ** -24 * top)
    moved = n.copy()
    colour = moved[..., :3]
    hit = rng.random(colour.shape) < max(0.01, 2 * bar)
    colour[hit] += np.where(colour[hit] < top, 1, -1)
    _rejects(f, back(moved), want, lin)
    # one sample two codes away
    moved = n.copy()
    y, x = 70, 133
    moved[y, x, 1] += 2 if moved[y, x, 1] <= top - 2 else -2
    _rejects(f, back(moved), want, lin)
    # a wrong alpha
    if f["num_channels"] == 4:
        moved = n.copy()
        moved[5, 5, 3] -= 1
        _rejects(f, back(moved), want, lin)


def test_comparator_rejects_a_float_srgb_sample_32_ulps_off(oracle):
    f = S.fmt(abi.TF_SRGB, abi.SAMPLE_F32, 3)
    lin, want = _yardstick(oracle, f)
    y, x, c = [int(v[0]) for v in np.nonzero((lin > 0.2) & (lin < 0.9))]
    got = want.copy()
    got.view(np.uint32)[y, x, c] += 32
    _rejects(f, got, want, lin)
    got.view(np.uint32)[y, x, c] -= 28  # 4 ulps: inside the bar
    assert S.compare(f, got, want, lin)["ulp"] == 4.0
    # ... and one ulp on the 12.92 x branch, which is one multiply
    y, x, c = [int(v[0]) for v in np.nonzero((lin > 1e-4) & (lin < 0.003))]
    got = want.copy()
    got.view(np.uint32)[y, x, c] += 1
    _rejects(f, got, want, lin)


def test_comparator_rejects_a_half_float_step_the_float_samples_do_not_explain(oracle):
    f = S.fmt(abi.TF_PQ, abi.SAMPLE_F16, 3, par=1000.0)
    lin, want = _yardstick(oracle, f)
    f32 = oracle.pack_output(S.fmt(abi.TF_PQ, abi.SAMPLE_F32, 3, par=1000.0), lin)
    y, x, c = [int(v[0]) for v in np.nonzero((lin > 0.2) & (lin < 0.9))]
    got = want.copy()
    got[y, x, c] += 1
    _rejects(f, got, want, lin, got_f32=f32, want_f32=f32)
    g32 = f32.copy()
    g32.view(np.uint32)[y, x, c] += 1  # the float sample differs too: a rounding boundary may lie between the two
    assert S.compare(f, got, want, lin, got_f32=g32, want_f32=f32)["maxdiff"] == 1
    got[y, x, c] += 1
    _rejects(f, got, want, lin, got_f32=g32, want_f32=f32)


@pytest.mark.parametrize("f", [S.fmt(abi.TF_709, abi.SAMPLE_U16, 3), S.fmt(abi.TF_709, abi.SAMPLE_F32, 4, swap=1),
                               S.fmt(abi.TF_709, abi.SAMPLE_F16, 3)], ids=S.fmt_id)
def test_comparator_rejects_one_changed_byte_of_a_709_output(oracle, f):
    lin, want = _yardstick(oracle, f)
    for byte in range(want.dtype.itemsize):
        got = want.copy()
        got.view(np.uint8).reshape(want.shape + (-1,))[77, 201, 2, byte] ^= 1
        _rejects(f, got, want, lin)


@pytest.mark.parametrize("f", [S.fmt(abi.TF_SRGB, abi.SAMPLE_U8, 3), S.fmt(abi.TF_709, abi.SAMPLE_U8, 4),
                               S.fmt(abi.TF_PQ, abi.SAMPLE_U8, 3, bits=5, par=255.0)], ids=S.fmt_id)
def test_comparator_rejects_a_dither_phase_error(oracle, f):
    """The pattern one column off: the pixels are right, the dither added to them is the neighbour's."""
    lin, want = _yardstick(oracle, f)
    shifted = np.roll(oracle.pack_output(f, np.roll(lin, 1, axis=1)), -1, axis=1)
    assert (shifted != want).any()
    _rejects(f, shifted, want, lin)
    _rejects(f, np.roll(want, 1, axis=1), want, lin)  # (and the image itself rolled by a column)


def test_padding_check_rejects_a_touched_byte(oracle):
    f = S.fmt(abi.TF_SRGB, abi.SAMPLE_U8, 3)
    lin, want = _yardstick(oracle, f)
    h, w = want.shape[:2]
    raw = np.full((h, w * 3 + 1), 0xA5, np.uint8)
    raw[:, :w * 3] = want.reshape(h, -1)
    body, row_bytes = S.rows_of(f, raw, w)
    assert row_bytes == w * 3 and np.array_equal(body, want)
    S.check_padding(raw, row_bytes, 0xA5)
    raw[h - 1, w * 3] = 0
    with pytest.raises(AssertionError):
        S.check_padding(raw, row_bytes, 0xA5)
