"""Planted frames for the render stages' kernel-against-model tests (test_gpu_noise.py, test_gpu_upsampling.py): zero or
fitted AC, no filters, planar XYB, values chosen so that every branch of the stage under test is taken -- and the
counts that say so, taken from planes the DEVICE produced with the stage off.  synth.synth_frame's tensors with
t["dc"] (and, for the one-block step frame, its AC coefficients) replaced, as output_sweep.sweep_frame plants its values.
Test infrastructure."""
import numpy as np
import torch

from libjxl_amd import synth

F32 = np.float32

# ---- noise: NoiseStrength's argument (y - x) / 2 and (y + x) / 2 in every place where its code decides --------------
KNOT_EPS = 5e-4  # how far from a knot k / 6 the planted values sit (asserted: within 1e-3, on the intended side)
NOISE_TARGETS = ([-0.05] + [k / 6 + s * KNOT_EPS for k in range(1, 8) for s in (-1, 1)] + [(k + 0.5) / 6 for k in range(7)] +
                 [1.3, 2.0])
# entries below 0 and above 1: both ends of NoiseStrength's final clamp decide (no stream can carry such a LUT)
NOISE_CLAMP_LUT = [-0.2, 0.3, 1.3, 0.0, 0.6, 1.2, -0.1, 0.8]


def noise_frame(xsize, ysize, device="cpu"):
    """Flat 8x8 blocks; block i has (y - x) / 2 = NOISE_TARGETS[i mod 24] and (y + x) / 2 = NOISE_TARGETS[(7 i + 3) mod 24]
    (7 is coprime to 24: any 24 consecutive blocks carry every target in both)."""
    params, t = synth.synth_frame(xsize, ysize, mix=synth.MIX_DCT8, device=device, gab=False, epf_iters=0, output_kind=0)
    for c in t["coeffs"]:
        c.zero_()
    xsb, ysb = (xsize + 7) // 8, (ysize + 7) // 8
    i = np.arange(xsb * ysb)
    tg = np.array(NOISE_TARGETS, np.float64)
    assert tg.size == 24 and xsb * ysb >= 24
    minus, plus = tg[i % 24], tg[(7 * i + 3) % 24]
    y, x = (plus + minus).astype(F32).reshape(ysb, xsb), (plus - minus).astype(F32).reshape(ysb, xsb)
    b = np.full((ysb, xsb), 0.3, F32)
    t["dc"] = [torch.from_numpy(p).to(device) for p in (x, y, b)]
    return params, t


def noise_population(planes):
    """name -> [pixels for (y - x) / 2, pixels for (y + x) / 2] of planar XYB [3, H, W]: below zero; within 1e-3 below
    and at-or-above each knot k / 6 (k = 1..7); the middle half of each interval 0..6; above 7 / 6 by more than 1e-3."""
    out = {}
    vs = [(planes[1] - planes[0]) * F32(0.5), (planes[1] + planes[0]) * F32(0.5)]
    out["below zero"] = [int((v < 0).sum()) for v in vs]
    for k in range(1, 8):
        out["under knot %d" % k] = [int(((v * F32(6) < k) & (v > k / 6 - 1e-3)).sum()) for v in vs]
        out["over knot %d" % k] = [int(((v * F32(6) >= k) & (v < k / 6 + 1e-3)).sum()) for v in vs]
    for k in range(7):
        out["middle of interval %d" % k] = [int(((v * F32(6) > k + 0.25) & (v * F32(6) < k + 0.75)).sum()) for v in vs]
    out["above 7/6"] = [int((v > 7 / 6 + 1e-3).sum()) for v in vs]
    return out


# ---- upsampling: step edges, so that the kernels' negative lobes overshoot and the clamp decides ---------------------
STEP_LEVELS = [(-0.02, 0.03), (0.2, 0.8), (0.1, 0.9)]  # X, Y, B: the two levels


def _block_steps(params, t):
    """A frame of one block has no block edges: its steps are made inside the block.  The quarters of the 8x8 block
    split at column 3 and row 2 alternate between the two levels (both orientations of a horizontal and of a vertical
    edge inside 7x5); the integer coefficients that give this come from the C oracle's response to each coefficient
    alone (the decode is linear apart from the quantisation bias of small values), least squares, rounded."""
    import frames
    import oracle
    dq = oracle.default_dequant_tables()
    p8 = dict(params, xsize=8, ysize=8)

    def decode():
        return np.asarray(frames.oracle_frame(p8, t, dq).decode(), np.float64)
    base = decode()
    K = 64
    resp = np.zeros((3, 63, 64))
    for j in range(1, 64):
        for c in t["coeffs"]:
            c[j] = K
        resp[:, j - 1] = ((decode() - base) / K).reshape(3, 64)
        for c in t["coeffs"]:
            c[j] = 0
    yy, xx = np.mgrid[0:8, 0:8]
    high = (xx >= 3) ^ (yy >= 2)
    for c, (lo, hi) in enumerate(STEP_LEVELS):
        want = (np.where(high, hi, lo) - base[c]).reshape(64)
        a = np.linalg.lstsq(resp[c].T, want, rcond=None)[0]
        t["coeffs"][c][1:64] = torch.from_numpy(np.clip(np.rint(a), -30000, 30000).astype(np.int16))


def step_frame(cw, ch, device="cpu"):
    """Coded cw x ch: flat 8x8 blocks that alternate between two levels -- by block row in the top third, by block
    column in the middle third, as a checkerboard below -- or, in a frame of a single block, the steps of _block_steps."""
    single = cw <= 8 and ch <= 8
    params, t = synth.synth_frame(cw, ch, mix=synth.MIX_DCT8, device="cpu" if single else device, gab=False, epf_iters=0,
                                  output_kind=0)
    for c in t["coeffs"]:
        c.zero_()
    xsb, ysb = (cw + 7) // 8, (ch + 7) // 8
    by, bx = np.mgrid[0:ysb, 0:xsb]
    third = np.minimum(3 * by // ysb, 2)
    high = np.where(third == 0, by % 2, np.where(third == 1, bx % 2, (bx + by) % 2)).astype(bool)
    t["dc"] = [torch.from_numpy(np.where(high, F32(hi), F32(lo)).astype(F32)).to(device) for lo, hi in STEP_LEVELS]
    if single:  # (chroma from luma off: the three channels are planted independently)
        params["cfl_base_b"] = 0.0
        t["ytox_map"].zero_()
        t["ytob_map"].zero_()
        t["dc"] = [torch.full((1, 1), (lo + hi) / 2, dtype=torch.float32) for lo, hi in STEP_LEVELS]
        _block_steps(params, t)
        t = {k: ([x.to(device) for x in v] if isinstance(v, list) else v.to(device)) for k, v in t.items()}
    return params, t
