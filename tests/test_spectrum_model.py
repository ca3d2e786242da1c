"""CPU tier of the whole-spectrum frames (spectrum.py): the frames meet their population conditions, the C oracle
equals the libjxl reference on them bit for bit, and a 1 % fault in ONE dequant-table entry moves the very "large"
impulse frames the GPU tier decodes (test_gpu_spectrum.py) by at least five times its bar at the four named
positions of every strategy, channel and coefficient type -- at every position for four strategies -- and a doubled
entry the flat frames, while the default-spectrum frame of test_blocks_each_strategy does not move at all."""
import ctypes as C

import numpy as np
import pytest

import frames
import spectrum as sp
from libjxl_amd import synth

TEETH = 5 * frames.TIGHT
MERGED_FLAT = list(range(21))
MERGED_IMPULSE = list(range(4, 12)) + [18, 19, 20]


@pytest.fixture(scope="module")
def ref(oracle):
    if not oracle.ref_available():
        pytest.fail("oracle/_ref not built and the reference tree absent: the yardstick tier cannot run")
    oracle.ref_lib()
    return oracle


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- population ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coeff_type", [0, 1])
@pytest.mark.parametrize("s", sp.STRATEGIES)
def test_population_alone(oracle, s, coeff_type):
    params, t = sp.flat_case(s, coeff_type)
    sp.check_flat_values(t, coeff_type)
    sp.check_flat_population(t, s)
    assert sp.used_set(params) <= {s, 0} and not sp.launch_of(params["used_acs"], 0)["merged"]
    for amplitude in sp.amplitudes(s):
        params, t = sp.impulse_case(s, coeff_type, amplitude)
        assert sp.check_impulse_population(params, t, s, coeff_type, amplitude, exact=True) == sp.impulse_blocks(s)
        assert params["xsize"] % (8 * synth.COVERED_X[s]) == 0 and params["ysize"] % (8 * synth.COVERED_Y[s]) == 0
        assert sp.used_set(params) == {s} and not sp.launch_of(params["used_acs"], 0)["merged"]


@pytest.mark.parametrize("coeff_type", [0, 1])
@pytest.mark.parametrize("s", MERGED_FLAT)
def test_population_merged(oracle, s, coeff_type):
    params, t = sp.flat_case(s, coeff_type, merged=True)
    sp.check_flat_values(t, coeff_type)
    sp.check_flat_population(t, s)
    assert {s, 6, 8} <= sp.used_set(params) and sp.launch_of(params["used_acs"], 0)["merged"]
    for amplitude in sp.amplitudes(s) if s in MERGED_IMPULSE else ():
        params, t = sp.impulse_case(s, coeff_type, amplitude, merged=True)
        sp.check_impulse_population(params, t, s, coeff_type, amplitude, exact=False)
        assert {s, 6, 8} <= sp.used_set(params) and sp.launch_of(params["used_acs"], 0)["merged"]


def test_blocks_of_follows_the_group_walk(oracle):
    """blocks_of against the scales synth laid down in stream order: a block's LLF slots are exactly the zero-scale
    slots at its offset, so on a flat frame of every strategy the first non-LLF slot of every block is where the walk
    says, and the slots behind a group's last block are empty."""
    params, t = sp.flat_case(0, 1, size=(533, 401), mix_all=True, seed=9)
    g, off, st = sp.blocks_of(t["ac_strategy"].numpy())
    assert len(set(st.tolist())) >= 12 and max(st) >= 18  # single blocks, both row-per-lane families, staged classes
    a = np.abs(t["coeffs"][1].numpy().astype(np.int64))
    for s in sorted(set(st.tolist())):
        b = sp.strategy_blocks(t, s)[1]
        assert not b[:, sp.llf_mask(s)].any() and (b[:, ~sp.llf_mask(s)] != 0).mean() > 0.99
    ng = a.size // sp.GROUP
    for gi in range(ng):
        last = np.flatnonzero(g == gi)[-1]
        assert not a[gi * sp.GROUP + off[last] + sp.slots(st[last]):(gi + 1) * sp.GROUP].any()


def test_launch_rule_restated():
    """sp.launch_of against the cases LaunchBlocksT distinguishes (kernels_blocks.hip: need_r16, need_r32, merged_r)."""
    bit = lambda *ss: sum(1 << s for s in ss)  # noqa: E731
    assert sp.launch_of(bit(0, 4), 0) == dict(need_r16=True, need_r32=False, merged=False)
    assert sp.launch_of(bit(0, 4), 1) == dict(need_r16=False, need_r32=False, merged=False)
    assert sp.launch_of(bit(5, 0), 0) == dict(need_r16=False, need_r32=True, merged=False)
    assert sp.launch_of(bit(4, 5), 0)["merged"] and not sp.launch_of(bit(4, 5), 1)["merged"]
    assert sp.launch_of(bit(4, 6, 8), 1)["merged"] and sp.launch_of(bit(7, 11), 1)["merged"]
    assert not sp.launch_of(bit(18, 0, 21), 0)["need_r16"] and not sp.launch_of(bit(6, 7, 4), 0)["merged"]


def test_handover_frame_has_dense_and_sparse_groups(ref):
    """From the arrays: the full group holds more non-zeros in X and in B than a chroma list of the sparse form takes,
    the clipped groups fewer.  And from the host decoder itself, on the reference encoder's streams, with the caps
    jxlhip_ac_group_decode_submit uses (kSparseCap, handover.hip): JXLHIP_ERR_RANGE for the one, 0 for the others."""
    from libjxl_amd import abi
    params, t = sp.handover_case()
    dense = sp.handover_group_kinds(t)
    assert dense.tolist() == [True, False, False, False]
    for c in range(3):
        assert np.abs(t["coeffs"][c].numpy().astype(np.int64)).max() <= 32767  # the sparse form's value range
    L = C.CDLL(abi.library_path())
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
    L.jxlhip_ac_pass_decode.argtypes = [vp, sz, C.POINTER(sz), u32, u32, vp, C.POINTER(vp)]
    L.jxlhip_ac_pass_destroy.argtypes = [vp]
    L.jxlhip_ac_pass_destroy.restype = None
    L.jxlhip_ac_group_decode_sparse.argtypes = [vp, u32, u32, u32, u32, vp, vp, vp, vp, sz, C.POINTER(sz), u32,
                                                vp * 3, u32 * 3, u32 * 3, C.POINTER(sz)]
    glob, groups, used_acs, _ = sp.reference_frame(ref, params, t).encode_ac_ref(histo_sets=2)
    g = np.frombuffer(glob, np.uint8)
    pos, h = sz(0), vp()
    assert L.jxlhip_ac_pass_decode(g.ctypes.data, len(g), C.byref(pos), used_acs, 2, None, C.byref(h)) == 0
    try:
        xs, ys = sp.HANDOVER_SIZE
        acs, rq = t["ac_strategy"].numpy(), t["raw_quant"].numpy()
        caps = (sp.SPARSE_CHROMA_CAP, sp.GROUP, sp.SPARSE_CHROMA_CAP)
        for gi, data in enumerate(groups):
            d = np.frombuffer(data, np.uint8)
            ent = [np.zeros(n + 1, np.uint32) for n in caps]
            cnt, gp, n = (u32 * 3)(), sz(0), sz(0)
            rc = L.jxlhip_ac_group_decode_sparse(h, (xs + 7) // 8, (ys + 7) // 8, gi % 2, gi // 2, acs.ctypes.data,
                                                 rq.ctypes.data, None, d.ctypes.data, len(d), C.byref(gp), 0,
                                                 (vp * 3)(*[e.ctypes.data for e in ent]), (u32 * 3)(*caps), cnt, C.byref(n))
            assert rc == (-8 if dense[gi] else 0), (gi, rc)  # JXLHIP_ERR_RANGE: the caller hands it over densely
    finally:
        L.jxlhip_ac_pass_destroy(h)


# ---- yardstick -------------------------------------------------------------------------------------------------------
def yardstick(ref, case, *args, **kw):
    for gab, epf, kind in ((False, 0, 0), (True, 1, 1)):
        params, t = case(*args, gab=gab, epf=epf, output_kind=kind, **kw)
        fr = sp.reference_frame(ref, params, t)
        o = fr.decode(threads=4)
        assert np.isfinite(o).all()
        assert np.array_equal(bits(o), bits(fr.decode_ref(threads=4))), (args, gab, epf)


ALONE_FRAMES = [(s, a) for s in sp.STRATEGIES for a in ("flat",) + sp.amplitudes(s)]
MERGED_FRAMES = [(s, a) for s in MERGED_FLAT for a in ("flat",) + (sp.amplitudes(s) if s in MERGED_IMPULSE else ())]


@pytest.mark.parametrize("coeff_type", [0, 1])
@pytest.mark.parametrize("s,frame", ALONE_FRAMES)
def test_oracle_bit_exact_with_reference_alone(ref, s, frame, coeff_type):
    if frame == "flat":
        yardstick(ref, sp.flat_case, s, coeff_type)
    else:
        yardstick(ref, sp.impulse_case, s, coeff_type, frame)


@pytest.mark.parametrize("coeff_type", [0, 1])
@pytest.mark.parametrize("s,frame", MERGED_FRAMES)
def test_oracle_bit_exact_with_reference_merged(ref, s, frame, coeff_type):
    if frame == "flat":
        yardstick(ref, sp.flat_case, s, coeff_type, merged=True)
    else:
        yardstick(ref, sp.impulse_case, s, coeff_type, frame, merged=True)


@pytest.mark.parametrize("coeff_type", [0, 1])
def test_oracle_bit_exact_with_reference_other_frames(ref, coeff_type):
    """The MIX_ALL frame of the fused tier, the all-DCT32X32 frame and the hand-over frame."""
    yardstick(ref, sp.flat_case, 0, coeff_type, size=sp.FUSED_MIX_SIZE, mix_all=True, seed=sp.FUSED_MIX_SEED)
    for amplitude in (None,) + sp.amplitudes(5):
        params, t = sp.dct32_only_impulse(coeff_type, amplitude) if amplitude else sp.dct32_only_flat(coeff_type)
        assert params["used_acs"] == 1 << 5
        (sp.check_impulse_population(params, t, 5, coeff_type, amplitude, exact=True) if amplitude else
         sp.check_flat_population(t, 5))
        fr = sp.reference_frame(ref, params, t)
        assert np.array_equal(bits(fr.decode(threads=4)), bits(fr.decode_ref(threads=4)))
    if coeff_type == 0:
        params, t = sp.handover_case()
        fr = sp.reference_frame(ref, params, t)
        assert np.array_equal(bits(fr.decode(threads=4)), bits(fr.decode_ref(threads=4)))


# ---- fault injection -------------------------------------------------------------------------------------------------
def fault_positions(s):
    rows, cols, _, _ = sp.block_shape(s)
    return {"last": (rows - 1, cols - 1), "last_row_first_col": (rows - 1, 0), "first_row_last_col": (0, cols - 1),
            "centre": (rows // 2, cols // 2)}


def faulty_tables(oracle, s, c, r, col, factor):
    t = oracle.default_dequant_tables().copy()
    t[oracle.lib().jxo_dequant_table_offset(s, c) + r * sp.block_shape(s)[1] + col] *= np.float32(factor)
    return t


def planes(oracle, params, t, table):
    return frames.oracle_frame(params, t, table).decode(threads=4)  # (3, ys, xs): XYB, no filters


def impulse_fault(oracle, s, coeff_type, probes):
    """The most a 1 % fault moves any of the "large" impulse frames of (s, coeff_type), exactly the frames the GPU tier
    decodes, for each (r, col, c) of `probes`."""
    per_frame = [impulse_fault_on(oracle, s, coeff_type, a, probes) for a in sp.amplitudes(s) if a != "small"]
    return np.max(per_frame, axis=0).tolist()


def impulse_fault_on(oracle, s, coeff_type, amplitude, probes):
    """One impulse frame with one table entry raised by 1 % for each (r, col, c) of `probes`: what the faulted channel
    moves by, as frames.per_channel_err measures it.  Only the group of the one block that carries the position can
    move, so only that group is decoded again."""
    good = oracle.default_dequant_tables()
    params, t = sp.impulse_case(s, coeff_type, amplitude)
    xs, ys = params["xsize"], params["ysize"]  # (multiples of the varblock: the planes have no padding)
    xsg, cols = (xs + 255) // 256, sp.block_shape(s)[1]
    g, off, st = sp.blocks_of(t["ac_strategy"].numpy())
    assert (st == s).all()
    here = []  # the probes whose position carries a large value in this frame
    for r, col, c in probes:
        at = t["coeffs"][c].numpy()[g * sp.GROUP + off + r * cols + col]
        assert np.count_nonzero(at) == 1
        here.append(sp.large_parts(s) == 1 or int(at[np.flatnonzero(at)[0]]) not in sp.SMALL_VALUES)
    if not any(here):
        return [0.0] * len(probes)
    want = planes(oracle, params, t, good)
    scale = [max(float(np.abs(want[k]).max()), 1e-3) for k in range(3)]
    out = []
    for (r, col, c), large in zip(probes, here):
        if not large:
            out.append(0.0)
            continue
        at = t["coeffs"][c].numpy()[g * sp.GROUP + off + r * cols + col]
        gi = int(g[np.flatnonzero(at)[0]])
        got = [np.zeros((ys, xs), np.float32) for _ in range(3)]
        fr = frames.oracle_frame(params, t, faulty_tables(oracle, s, c, r, col, 1.01))
        assert oracle.lib().jxo_decode_groups(C.byref(fr.c), (C.c_void_p * 3)(*[p.ctypes.data for p in got]), xs, gi,
                                              gi + 1) == 0
        y0, x0 = gi // xsg * 256, gi % xsg * 256
        moved = [float(np.abs(got[k][y0:y0 + 256, x0:x0 + 256].astype(np.float64) - want[k][y0:y0 + 256, x0:x0 + 256])
                       .max()) / scale[k] for k in range(3)]
        if c != 1:  # X and B tables feed their own channel only (Y reaches all three through CfL)
            assert moved[1] == 0.0
        out.append(moved[c])
    return out


@pytest.mark.parametrize("coeff_type", [0, 1])
@pytest.mark.parametrize("s", sp.STRATEGIES)
def test_one_percent_fault_shows_on_the_impulse_frame(oracle, s, coeff_type):
    """One table entry raised by 1 %, at the last position, the last row's first and the first row's last position and
    the centre, in each channel, on the very "large" impulse frames the GPU tier decodes (int16 and int32; where the
    class is split into several frames, the one that carries the position large): the faulted channel moves by >= 5x
    the bar (1e-4).  Measured over 27 strategies x 4 positions x 3 channels x 2 types: 2.2e-4 (the centre of 256x256
    and 256x128 in X, whose basis function peaks at 1/2 and whose block sums 64 impulses) to 1e-2 and more; the last
    position of Y, int16: strategy 0 1.0e-2, 5 1.0e-2, 18 5.6e-4, 24 4.7e-4."""
    named = fault_positions(s)
    probes = [(r, col, c) for (r, col) in named.values() for c in range(3)]
    moved = impulse_fault(oracle, s, coeff_type, probes)
    for (name, c), m in zip([(n, c) for n in named for c in range(3)], moved):
        print("MOVED impulse %d i%d %s c%d %.3e" % (s, 32 if coeff_type else 16, name, c, m))
    assert min(moved) >= TEETH, (s, list(zip(probes, moved)))


@pytest.mark.parametrize("coeff_type", [0, 1])
@pytest.mark.parametrize("s", [0, 2, 6, 13])
def test_one_percent_fault_shows_at_every_position(oracle, s, coeff_type):
    """The same at EVERY non-LLF position of every channel, for a strategy of each single-block kind (DCT8, DCT2X2,
    AFV) and the 16x8 transform: no position of the "large" frame is out of the bar's sight.  Measured minimum: 4.1e-3 (16x8), against the bar of 2e-5 that is asserted."""
    rows, cols, lo, hi = sp.block_shape(s)
    probes = [(r, col, c) for r in range(rows) for col in range(cols) if not (r < lo and col < hi) for c in range(3)]
    moved = impulse_fault(oracle, s, coeff_type, probes)
    worst = int(np.argmin(moved))
    print("MOVED everywhere %d i%d min %.3e at %s" % (s, 32 if coeff_type else 16, moved[worst], probes[worst]))
    assert moved[worst] >= frames.TIGHT, (s, probes[worst], moved[worst])


@pytest.mark.parametrize("s", sp.STRATEGIES)
def test_doubled_entry_shows_on_the_flat_frame(oracle, s):
    """The same places with the entry doubled, on the flat int16 frame: >= 5x the bar in that channel."""
    params, t = sp.flat_case(s, 0)
    want = planes(oracle, params, t, oracle.default_dequant_tables())
    for name, (r, col) in fault_positions(s).items():
        for c in range(3):
            moved = frames.per_channel_err(planes(oracle, params, t, faulty_tables(oracle, s, c, r, col, 2.0)), want, 0)
            print("MOVED flat %d %s c%d %.3e" % (s, name, c, moved[c]))
            assert moved[c] >= TEETH, (s, name, c, moved.tolist())


@pytest.mark.parametrize("s", sp.STRATEGIES)
def test_default_spectrum_frame_is_blind_to_the_last_entry(oracle, s):
    """The documented gap: on the frame of test_gpu_parity.py::test_blocks_each_strategy the last entry of the
    strategy's tables, doubled in all three channels, moves the decoded planes by exactly 0.0 -- every block holds 0
    there."""
    cx, cy = synth.COVERED_X[s], synth.COVERED_Y[s]
    xs, ys = max(272, 8 * cx + 24), max(264, 8 * cy + 8)
    if max(cx, cy) >= 16:
        xs, ys = 8 * cx + 256, 8 * cy
    params, t = synth.synth_frame(xs, ys, device="cpu", mix={s: 3.0 * cx * cy, 0: 1.0}, gab=False, epf_iters=0,
                                  seed=1000 + s, output_kind=0)
    table = oracle.default_dequant_tables().copy()
    for c in range(3):
        table[oracle.lib().jxo_dequant_table_offset(s, c) + sp.slots(s) - 1] *= np.float32(2.0)
    want = planes(oracle, params, t, oracle.default_dequant_tables())
    assert np.abs(want).max() > 0.1
    assert np.array_equal(bits(planes(oracle, params, t, table)), bits(want))
