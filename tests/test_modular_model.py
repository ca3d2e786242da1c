"""Known answers for tests/modular_model.py, the numpy model of the device stage of a lossless frame: the 42 reversible
colour transforms (lib/jxl/modular/transform/rct.cc:29-150) on hand-computed triples, inverse(forward(x)) == x in
wrapping int32 for every type, the group-then-global order, and the one-multiply conversion.  CPU only."""
import numpy as np
import pytest

import modular_model as mm


def inv(triple, rct_type):
    return [int(c[0]) for c in mm.inverse_rct([np.array([v], np.int32) for v in triple], rct_type)]


def test_ycocg_by_hand():
    """Type 6 (permutation 0, custom 6).  (Y, Co, Cg) = (100, 30, -20): tmp = 100 - (-20 >> 1) = 100 + 10 = 110;
    G = -20 + 110 = 90; B = 110 - (30 >> 1) = 95; R = 95 + 30 = 125."""
    assert inv((100, 30, -20), 6) == [125, 90, 95]
    # odd negative chroma: -7 >> 1 is -4 (arithmetic shift, not a division): tmp = 10 + 4 = 14; G = 7; B = 14 - (-3 >> 1) = 16; R = 13
    assert inv((10, -3, -7), 6) == [13, 7, 16]
    # the forward direction by hand: (R, G, B) = (125, 90, 95): Co = 30; tmp = 95 + 15 = 110; Cg = -20; Y = 110 + (-20 >> 1) = 100
    assert [int(c[0]) for c in mm.forward_rct([np.array([v], np.int32) for v in (125, 90, 95)], 6)] == [100, 30, -20]


def test_two_other_types_by_hand():
    """Type 5 = permutation 0, custom 5: Third += First; Second += (First + Third) >> 1.
    (10, 3, -4): Third = 6; Second = 3 + (16 >> 1) = 11 -> (10, 11, 6)."""
    assert inv((10, 3, -4), 5) == [10, 11, 6]
    """Type 10 = permutation 1, custom 3: Third += First; Second += First; the results go to channels 1, 2, 0.
    (10, 3, -4): First = 10, Second = 13, Third = 6 -> channel 0 = Third, 1 = First, 2 = Second."""
    assert inv((10, 3, -4), 10) == [6, 10, 13]
    """Type 21 = permutation 3, custom 0: a permutation alone: results to channels 0, 2, 1."""
    assert inv((1, 2, 3), 21) == [1, 3, 2]
    """Type 35 = permutation 5 (targets 2, 1, 0), custom 0."""
    assert inv((1, 2, 3), 35) == [3, 2, 1]
    assert inv((1, 2, 3), 0) == [1, 2, 3]


def test_permutation_targets_are_the_references():
    # rct.cc:106: 0 = RGB, 1 = GBR, 2 = BRG, 3 = RBG, 4 = GRB, 5 = BGR
    assert [mm._targets(p) for p in range(6)] == [(0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (1, 0, 2), (2, 1, 0)]


@pytest.mark.parametrize("rct_type", range(42))
def test_inverse_of_forward_is_the_identity_in_wrapping_int32(rct_type):
    rng = np.random.default_rng(rct_type)
    x = rng.integers(-2 ** 31, 2 ** 31, (3, 4096)).astype(np.int32)
    edge = np.array([-2 ** 31, -2 ** 31 + 1, 2 ** 31 - 1, 2 ** 31 - 2, -1, 0, 1], np.int32)
    x[:, :343] = np.stack(np.meshgrid(edge, edge, edge, indexing="ij")).reshape(3, -1)  # every triple of values near +-2^31
    with np.errstate(over="ignore"):
        back = mm.inverse_rct(mm.forward_rct(list(x), rct_type), rct_type)
    for c in range(3):
        assert back[c].dtype == np.int32 and np.array_equal(back[c], x[c]), c
    if rct_type % 7 == 0:  # a permutation alone moves samples and changes none
        assert sorted(map(bytes, mm.forward_rct(list(x), rct_type))) == sorted(map(bytes, x))


def test_group_programs_then_the_global_one_each_last_listed_first():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (3, 130, 257)).astype(np.int32)
    gd = 128
    group = np.array([6, 13 | (6 << 8), 7, 41, 21 | (30 << 8), 20], np.uint16)  # 3 x 2 groups; 7 and 21 only permute
    glob = 9 | (17 << 8)
    p = [c.copy() for c in img]
    for t in (glob & 0xFF, glob >> 8):  # the encoder: the global list first, in listed order ...
        p = mm.forward_rct(p, t)
    for g, prog in enumerate(group):  # ... then every group's
        ys, xs = slice((g // 3) * gd, (g // 3 + 1) * gd), slice((g % 3) * gd, (g % 3 + 1) * gd)
        q = [c[ys, xs].copy() for c in p]
        for t in (int(prog) & 0xFF, int(prog) >> 8):
            q = mm.forward_rct(q, t)
        for c in range(3):
            p[c][ys, xs] = q[c]
    back = mm.undo_programs(p, gd, group, glob)
    assert all(np.array_equal(back[c], img[c]) for c in range(3))
    # the order matters: the other one does not give the image back
    wrong = mm.undo_program([c.copy() for c in p], glob)
    assert not all(np.array_equal(wrong[c], img[c]) for c in range(3))
    # int16 planes are widened, not reinterpreted
    back16 = mm.undo_programs([c.astype(np.int16) for c in p], gd, group, glob)
    assert all(np.array_equal(back16[c], img[c]) for c in range(3))


@pytest.mark.parametrize("bits", [8, 10, 12, 16])
def test_conversion_is_one_float32_multiply(bits):
    top = (1 << bits) - 1
    v = np.arange(0, top + 1, max(1, top // 4099), dtype=np.int32)
    got = mm.to_float([v, v, v], bits)[..., 0]
    factor = np.float32(1.0 / top)
    assert got.dtype == np.float32 and np.array_equal(got, v.astype(np.float32) * factor)
    assert np.array_equal(np.rint(got.astype(np.float64) * top).astype(np.int64), v)  # (the integers come back)
    # ... which is not the correctly rounded quotient everywhere: the reference multiplies, and so does the model
    if bits == 8:
        assert (got != (v.astype(np.float64) / top).astype(np.float32)).any()
