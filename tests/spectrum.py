"""Frames that put energy on EVERY coefficient position of a transform, the conditions such a frame has to meet, and
the restated launch rule of phase 1.  Test infrastructure (test_spectrum_model.py, test_gpu_spectrum.py).

synth.synth_frame's default spectrum (Laplace scale 6 * exp(-6 f)) rounds to zero over the upper band: on the frames
of test_blocks_each_strategy between 45 % and 83 % of a strategy's positions are zero in every block, so the dequant
entry read there, the IDCT row / column it feeds and the transposes that carry it are multiplied by zero.

Flat frames: the same layouts with decay = 0 (every position draws from one Laplace scale): 0, +-1 (the quant-bias
branch of AdjustQuantBias) and larger values everywhere; as int32 with amp = 2e5, values beyond 16 bits.

Impulse frames: one strategy, DC 0, the coefficient arrays rewritten.  Up to 1024 slots the j-th varblock of the
strategy carries ONE non-zero per channel, at position j mod slots (nothing when that is an LLF slot: genuine streams
hold 0 there); raw_quant is 18 everywhere (synth's mean), the CfL maps stay as synth makes them.  Larger varblocks
carry d shifted diagonals (r, (r + shift) mod cols), shifts j + k cols / d (j mod cols / d): cols / d varblocks cover every position once, with d non-zeros per row and per column; d is the smallest of
1, 2, 4 whose frame stays within 4.2 Mpx (256x256: 4; 256x128, 128x256: 2; the others 1), because the sum of a block's
impulses sets the frame's range and the fewer there are the more one of them weighs.

The bar of the GPU tier is relative to the channel's magnitude over the FRAME, so a value is only held to it where it
is of the size of the largest value of its frame.  Hence one amplitude class per frame, and every frame runs on every
path.  "large": +-30000 at the position with the smallest dequantisation step of the strategy (int32: 2^24 + 3 and
-(2^24 + 1)) and that value times (smallest step / own step) everywhere else, so that EVERY impulse of the frame has
the same dequantised amplitude (large_scale); a block of 128x128 and more would sum hundreds of them, so its class is
split into frames "large0" .. that carry at most 64 large values per block and +1 .. +7 on the rest (large_parts).
"small": +1, -1, +2, -3, +7 and -300 (the quant-bias branch of AdjustQuantBias and its neighbourhood).  Which value of
its class a position gets is drawn from a seeded table per strategy (a regular pattern is a comb along a diagonal,
whose transform piles up in a few pixels and would set the range far above one impulse's amplitude); channel c takes
the next entry."""
import functools

import numpy as np
import torch

import frames
from libjxl_amd import synth
from phase1_plan import launch_of  # noqa: F401  (the restated launch rule of phase 1: need_r16 / need_r32 / merged)

LARGE_PER_BLOCK = 64           # at most this many range-setting impulses per varblock and channel
SMALL_VALUES = (1, -1, 2, -3, 7, -300)
LARGE_VALUES = {0: (30000, -30000), 1: ((1 << 24) + 3, -((1 << 24) + 1))}  # (odd: no float32 holds them)
IMPULSE_RAW_QUANT = 18      # synth's mean
MAX_IMPULSE_PIXELS = 4.2e6
SINGLE_IMPULSE_SLOTS = 1024   # up to DCT32X32: one non-zero per channel and varblock
GROUP = 65536                 # coefficient slots per group and channel (JXLHIP_GROUP_COEFFS)
STRATEGIES = list(range(27))


# ---- geometry -----------------------------------------------------------------------------------------------------
def block_shape(s):
    """(rows, cols, lo, hi) of a varblock's coefficient block: 8 lo rows of 8 hi slots, lo = min(cx, cy); its first lo
    rows x hi columns are the LLF slots (synth._layout_streams, ac_strategy.h)."""
    cx, cy = synth.COVERED_X[s], synth.COVERED_Y[s]
    lo, hi = min(cx, cy), max(cx, cy)
    return 8 * lo, 8 * hi, lo, hi


def slots(s):
    return 64 * synth.COVERED_X[s] * synth.COVERED_Y[s]


def llf_mask(s):
    """bool[slots(s)]: True at the LLF slots."""
    rows, cols, lo, hi = block_shape(s)
    m = np.zeros((rows, cols), bool)
    m[:lo, :hi] = True
    return m.reshape(-1)


def blocks_of(ac_strategy):
    """Every varblock as (group, stream offset, strategy), three int64 arrays in stream order: groups in index order,
    a group's first blocks in raster order, 64 cx cy slots each (oracle/group.c decode_group)."""
    acs = np.asarray(ac_strategy)
    ysb, xsb = acs.shape
    xsg = (xsb + 31) // 32
    covered = 64 * np.array(synth.COVERED_X, np.int64) * np.array(synth.COVERED_Y, np.int64)
    gs, offs, strs = [], [], []
    for g in range(xsg * ((ysb + 31) // 32)):
        gy, gx = divmod(g, xsg)
        a = acs[gy * 32:gy * 32 + 32, gx * 32:gx * 32 + 32].reshape(-1)  # (row-major = raster order)
        st = (a[(a & 1) == 1] >> 1).astype(np.int64)
        size = covered[st]
        off = np.cumsum(size) - size
        assert not len(st) or off[-1] + size[-1] <= GROUP
        gs.append(np.full(len(st), g, np.int64)), offs.append(off), strs.append(st)
    return np.concatenate(gs), np.concatenate(offs), np.concatenate(strs)


def strategy_blocks(t, s):
    """The coefficient blocks of strategy s: int64 [3, blocks of s, slots(s)], in stream order."""
    g, off, st = blocks_of(t["ac_strategy"].numpy())
    base = (g * GROUP + off)[st == s]
    idx = base[:, None] + np.arange(slots(s), dtype=np.int64)[None, :]
    return np.stack([t["coeffs"][c].numpy()[idx].astype(np.int64) for c in range(3)])


def used_set(params):
    return {s for s in range(27) if params["used_acs"] >> s & 1}


# ---- flat frames -----------------------------------------------------------------------------------------------------
def flat_kw(coeff_type):
    return dict(coeff_type=1, decay=0.0, amp=200000.0) if coeff_type else dict(coeff_type=0, decay=0.0, amp=6.0)


def flat_size(s):
    """The size of test_blocks_each_strategy (ragged: the last group clipped, no multiple of the block); where that
    holds too few blocks of s for every position to be drawn non-zero in some block (a chroma slot is zero in one block
    in six), a row or grid of more of them."""
    cx, cy = synth.COVERED_X[s], synth.COVERED_Y[s]
    if max(cx, cy) >= 16:      # 128x128 .. 256x256: 16 blocks or more (2 or 3 in test_blocks_each_strategy)
        return 8 * cx * 5 + 8, 8 * cy * 4
    if max(cx, cy) == 8:       # 64x64, 64x32, 32x64: about four groups' worth
        return 520, 512
    return max(272, 8 * cx + 24), max(264, 8 * cy + 8)


MERGE_FILLER = {6: 2.0, 8: 4.0}   # a small area share of 16x8 and 32x8: both row-per-lane families have work


def alone_mix(s):
    return {s: 3.0 * synth.COVERED_X[s] * synth.COVERED_Y[s], 0: 1.0}


def merged_mix(s):
    mix = {s: 16.0 * synth.COVERED_X[s] * synth.COVERED_Y[s], 0: 1.0}
    for k, v in MERGE_FILLER.items():
        mix[k] = mix.get(k, 0.0) + v
    return mix


@functools.lru_cache(maxsize=4)
def flat_case(s, coeff_type, merged=False, gab=False, epf=0, output_kind=0, size=None, mix_all=False, seed=None):
    """(params, tensors) of the flat frame of strategy s; shared between tests: read only."""
    xs, ys = size or flat_size(s)
    mix = synth.MIX_ALL if mix_all else (merged_mix(s) if merged else alone_mix(s))
    params, t = synth.synth_frame(xs, ys, device="cpu", mix=mix, gab=gab, epf_iters=epf, output_kind=output_kind,
                                  seed=(2000 + s + 100 * merged) if seed is None else seed, **flat_kw(coeff_type))
    return params, t


def check_flat_values(t, coeff_type):
    for c in range(3):
        a = t["coeffs"][c].numpy()
        assert a.dtype == (np.int32 if coeff_type else np.int16)
        if coeff_type:
            assert np.abs(a.astype(np.int64)).max() > 32767, c  # really needs 32 bits
        else:
            have = set(np.unique(a[:GROUP]).tolist())
            assert {0, 1, -1} <= have and max(have) > 2 and min(have) < -2, c


def check_flat_population(t, s):
    """Every non-LLF position of s is non-zero in some block of s, in each channel; the LLF slots hold 0."""
    b = strategy_blocks(t, s)
    assert b.shape[1] > 0, "no block of strategy %d" % s
    hit = (b != 0).any(axis=1)
    llf = llf_mask(s)
    assert not hit[:, llf].any()
    missing = np.argwhere(~hit[:, ~llf])
    assert len(missing) == 0, "strategy %d: %d (channel, position) pairs never non-zero in %d blocks, first %s" % (
        s, len(missing), b.shape[1], missing[:4].tolist())
    return b.shape[1]


# ---- impulse frames --------------------------------------------------------------------------------------------------
def impulse_diagonals(s):
    """Diagonals per varblock of more than 1024 slots: as few as the 4.2 Mpx of an impulse frame allow."""
    cols = block_shape(s)[1]
    return min(d for d in (1, 2, 4) if cols // d * slots(s) <= MAX_IMPULSE_PIXELS)


def impulse_blocks(s):
    """Varblocks that cover every position once."""
    n = slots(s)
    return n if n <= SINGLE_IMPULSE_SLOTS else block_shape(s)[1] // impulse_diagonals(s)


def impulse_size(s):
    """The most nearly square frame of impulse_blocks(s) varblocks."""
    w, h, nb = 8 * synth.COVERED_X[s], 8 * synth.COVERED_Y[s], impulse_blocks(s)
    bw = min((1 << k for k in range(nb.bit_length()) if nb % (1 << k) == 0),
             key=lambda bw: abs(bw * w - nb // bw * h))
    return bw * w, nb // bw * h


def large_parts(s):
    """Frames the "large" class of strategy s is split into.  The sum of a block's equal impulses sets the frame's
    range, about sqrt(their number) above one of them: with the 1024 of a 256x256 varblock one impulse in the block's
    centre, whose basis function peaks at 1/2, weighs 5e-3 of it.  So a frame holds at most LARGE_PER_BLOCK large
    values per block and channel: "large<k>" carries them on the k-th of `parts` runs of consecutive impulses (diagonal
    after diagonal, row after row) and small values on the rest.  256x256: 16; 256x128, 128x256: 4; 128x128: 2; every other: 1."""
    n = slots(s)
    return 1 if n <= SINGLE_IMPULSE_SLOTS else max(1, impulse_diagonals(s) * block_shape(s)[0] // LARGE_PER_BLOCK)


def amplitudes(s):
    """The impulse frames of strategy s: "large" (or "large0" .. ) and "small"."""
    k = large_parts(s)
    return tuple(["large"] if k == 1 else ["large%d" % i for i in range(k)]) + ("small",)


@functools.lru_cache(maxsize=None)
def value_index(s):
    """int64 [rows, cols], seeded per strategy: position (r, col) of channel c carries entry (value_index + c) mod n of
    its frame's n values."""
    rows, cols, _, _ = block_shape(s)
    return np.random.default_rng(5000 + s).integers(0, 1 << 16, size=(rows, cols)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def large_scale(s, c):
    """float64 [rows, cols] in (0, 1]: what the "large" frame multiplies its values by, so that every impulse of every
    channel has the same dequantised amplitude: (the smallest step of the strategy over the three channels) / (this
    position's step), a step being the default dequant-table entry times the channel's multiplier (x_dm_multiplier,
    1, b_dm_multiplier).  The entries of one transform span two orders of magnitude, and with equal coefficients the
    positions with small entries would sit far below the range the large entries set; and Y reaches X and B through
    CfL, so a louder Y would set their range."""
    import oracle
    rows, cols, _, _ = block_shape(s)
    p, _ = synth.synth_frame(8, 8, mix=synth.MIX_DCT8)
    mul = (p["x_dm_multiplier"], 1.0, p["b_dm_multiplier"])
    table = oracle.default_dequant_tables()
    step = [table[oracle.lib().jxo_dequant_table_offset(s, k):][:rows * cols].astype(np.float64) * mul[k] for k in range(3)]
    return (min(w[~llf_mask(s)].min() for w in step) / step[c]).reshape(rows, cols)


def write_impulses(t, s, coeff_type, amplitude):
    """DC planes 0; every coefficient 0 except the impulses in the blocks of s (see the module text)."""
    g, off, st = blocks_of(t["ac_strategy"].numpy())
    base = (g * GROUP + off)[st == s]
    rows, cols, lo, hi = block_shape(s)
    n, j = rows * cols, np.arange(len(base), dtype=np.int64)
    if n <= SINGLE_IMPULSE_SLOTS:
        r, col = np.divmod(j % n, cols)
        blk = j
    else:
        d = impulse_diagonals(s)
        q = cols // d
        shift = (j % q)[:, None] + q * np.arange(d, dtype=np.int64)[None, :]            # [blocks, d]
        r = np.broadcast_to(np.arange(rows, dtype=np.int64)[None, None, :], shift.shape + (rows,))
        col = (r + shift[:, :, None]) % cols
        blk = np.broadcast_to(j[:, None, None], r.shape)
        r, col, blk = r.reshape(-1), col.reshape(-1), blk.reshape(-1)
    keep = ~((r < lo) & (col < hi))  # the LLF slots stay 0
    r, col, blk = r[keep], col[keep], blk[keep]
    small, large = np.array(SMALL_VALUES, np.int64), np.array(LARGE_VALUES[coeff_type], np.int64)
    if amplitude == "small":
        is_large = np.zeros(len(r), bool)
    elif n <= SINGLE_IMPULSE_SLOTS:
        is_large = np.ones(len(r), bool)
    else:  # the run of the block's impulses this frame makes large (order: diagonal, then row)
        run = (np.arange(len(keep)) % (impulse_diagonals(s) * rows))[keep] * large_parts(s) // (impulse_diagonals(s) * rows)
        is_large = run == int(amplitude[5:] or 0)
    t["dc"] = [torch.zeros_like(d) for d in t["dc"]]
    # one quantisation step for every block: synth's field spans 1 .. 36 on these frames, and the one block with the
    # smallest step would set the frame's range an order of magnitude above every other block's impulses
    t["raw_quant"] = torch.full_like(t["raw_quant"], IMPULSE_RAW_QUANT)
    out = []
    for c in range(3):
        a = np.zeros(t["coeffs"][c].numel(), np.int32 if coeff_type else np.int16)
        k = value_index(s)[r, col] + c
        # (the rest of a split "large" frame leaves -300 out: an int16 large value is a few hundred where the step is big)
        rest = small[k % 6] if amplitude == "small" else small[k % 5]
        v = np.where(is_large, np.rint(large[k % 2] * large_scale(s, c)[r, col]).astype(np.int64), rest)
        a[base[blk] + r * cols + col] = v.astype(a.dtype)
        out.append(torch.from_numpy(a))
    t["coeffs"] = out


@functools.lru_cache(maxsize=4)
def impulse_case(s, coeff_type, amplitude="large", merged=False, gab=False, epf=0, output_kind=0):
    """(params, tensors) of the impulse frame of strategy s: tiled by s alone (mix = {s: 1}, a multiple of the
    varblock), or merged: s with the 16x8 / 32x8 filler, whose varblocks carry zeros, at a size that holds at least
    impulse_blocks(s) varblocks of s.  Shared between tests: read only."""
    if merged:
        w, h = 8 * synth.COVERED_X[s], 8 * synth.COVERED_Y[s]
        xs, ys = impulse_size(s)
        while True:  # the filler and the ragged placement cost blocks: grow until enough of s are placed
            params, t = synth.synth_frame(xs, ys, device="cpu", mix=merged_mix(s), gab=gab, epf_iters=epf,
                                          output_kind=output_kind, seed=3100 + s, coeff_type=coeff_type)
            if int((blocks_of(t["ac_strategy"].numpy())[2] == s).sum()) >= impulse_blocks(s):
                break
            xs, ys = (xs + max(w, 64), ys) if xs <= ys else (xs, ys + max(h, 64))
            assert xs * ys <= MAX_IMPULSE_PIXELS
    else:
        xs, ys = impulse_size(s)
        params, t = synth.synth_frame(xs, ys, device="cpu", mix={s: 1.0}, gab=gab, epf_iters=epf,
                                      output_kind=output_kind, seed=3000 + s, coeff_type=coeff_type)
        assert params["used_acs"] == 1 << s and int((blocks_of(t["ac_strategy"].numpy())[2] == s).sum()) == \
            impulse_blocks(s), "the frame is not tiled by strategy %d alone" % s
    write_impulses(t, s, coeff_type, amplitude)
    return params, t


def check_impulse_population(params, t, s, coeff_type, amplitude, exact):
    """Every non-LLF position of s carries a non-zero in some block of s (exact: in exactly one), in each channel; the
    LLF slots, every other varblock and the DC hold 0; no row or column of a block has more than four non-zeros; the
    frame has at most 4.2 Mpx; the values are those of the amplitude class (large ones: as large_scale scales them, at
    most LARGE_PER_BLOCK per block and channel)."""
    assert params["xsize"] * params["ysize"] <= MAX_IMPULSE_PIXELS
    assert all(not d.any() for d in t["dc"])
    b = strategy_blocks(t, s)
    nz = b != 0
    rows, cols, _, _ = block_shape(s)
    llf = llf_mask(s)
    count = nz.sum(axis=1)
    assert not count[:, llf].any()
    assert (count[:, ~llf] == 1).all() if exact else (count[:, ~llf] >= 1).all(), \
        (s, np.argwhere(count[:, ~llf] != 1)[:4].tolist())
    grid = nz.reshape(3, -1, rows, cols)
    assert grid.sum(axis=3).max() <= 4 and grid.sum(axis=2).max() <= 4
    for c in range(3):
        a = t["coeffs"][c].numpy()
        assert np.count_nonzero(a) == nz[c].sum(), "a non-zero outside the blocks of strategy %d" % s
        v = b[c][nz[c]]
        scale = np.broadcast_to(large_scale(s, c).reshape(-1), nz[c].shape)[nz[c]]
        large = (v == np.rint(LARGE_VALUES[coeff_type][0] * scale)) | (v == np.rint(LARGE_VALUES[coeff_type][1] * scale))
        small = np.isin(v, SMALL_VALUES)
        assert (large | small).all()
        if amplitude == "small":
            assert small.all() and set(np.unique(v).tolist()) == set(SMALL_VALUES)
        else:  # (a scaled large value may equal a small one: ~small counts the certain ones)
            assert 0 < (~small).sum() / b.shape[1] <= LARGE_PER_BLOCK and (large_parts(s) > 1 or large.all())
            assert np.abs(v).max() > (32767 if coeff_type else 300)  # (int32: the frame needs 32 bits)
    return b.shape[1]


# ---- other frames of the GPU tier --------------------------------------------------------------------------------------
FUSED_MIX_SIZE = (533, 404)   # every strategy, ragged (the classes k_fused_pc copies from the planes)
FUSED_MIX_SEED = 4000
DCT32_ONLY_SIZE = (1020, 508)  # 32 x 16 whole DCT32X32 varblocks, the last column / row clipped by the image


@functools.lru_cache(maxsize=2)
def dct32_only_flat(coeff_type):
    """All DCT32X32, no loop filter, linear RGB out: the frame whose matrix-core kernel writes the pixels itself."""
    params, t = synth.synth_frame(*DCT32_ONLY_SIZE, device="cpu", mix=synth.MIX_DCT32, gab=False, epf_iters=0,
                                  output_kind=1, seed=4032, **flat_kw(coeff_type))
    return params, t


def dct32_only_impulse(coeff_type, amplitude):
    return impulse_case(5, coeff_type, amplitude, output_kind=1)


# ---- the hand-over frame: dense fallback and sparse groups in one frame -----------------------------------------------
SPARSE_CHROMA_CAP = 16382     # kSparseCap of handover.hip: a group with more non-zeros in X or B goes up densely
HANDOVER_SIZE = (296, 280)    # one full group; the clipped ones hold 160, 96 and 15 blocks
HANDOVER_AMP = 1.3            # chroma scale 0.585: a slot is non-zero with p = exp(-0.5 / 0.585) = 0.43, 27 000 of the full
                              # group's 64 512 AC slots (cap: 16 382); a clipped group has 10 080 AC slots or fewer


@functools.lru_cache(maxsize=1)
def handover_case():
    params, t = synth.synth_frame(*HANDOVER_SIZE, device="cpu", mix=synth.MIX_ALL, gab=True, epf_iters=1, seed=4100,
                                  coeff_type=0, decay=0.0, amp=HANDOVER_AMP)
    return params, t


def handover_group_kinds(t):
    """Per group: True when the sparse form cannot hold it (it goes up densely)."""
    ng = t["coeffs"][0].numel() // GROUP
    nz = [np.count_nonzero(t["coeffs"][c].numpy().reshape(ng, GROUP), axis=1) for c in range(3)]
    return (nz[0] > SPARSE_CHROMA_CAP) | (nz[2] > SPARSE_CHROMA_CAP)


def reference_frame(ref, params, t):
    """The oracle.Frame of (params, tensors) over the REFERENCE's own dequant tables."""
    return frames.oracle_frame(params, t, ref.ref_default_dequant_tables())
