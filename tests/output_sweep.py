"""A frame that sweeps the domain of the output encoder (libjxl_amd/csrc/emit.h), the format grid the encoder is held
to, the population conditions a run has to meet, and the comparison of a packed output with the yardstick
(oracle.pack_output = oracle/output.c's jxo_pack_output applied to LINEAR pixels).  Test infrastructure.

The frame: synth.synth_frame(mix=MIX_DCT8) with every coefficient zeroed, the identity for inverse_opsin_matrix and
opsin_biases 0.  A DCT8 block with no AC is its DC, and under the identity matrix linear channel c of the block is
the cube of (y + x, y - x, b): three chosen linear values per 8x8 block.  The values are kept in the CUBE-ROOT
domain (float32 `a`, the linear value is cube3(a) = fl(fl(a * a) * a) as XybToRgb evaluates it), so "the nearest
plantable float32 values around a branch point" are neighbouring floats a.  A block that carries a cluster value has
r == g (x = 0, so y + x is exact); everywhere else r and g are neighbours in magnitude, which keeps y +- x within an
ulp of the larger one.

Value list (planted_cbrt): +0 and -0 (a pixel of three tiny negative values: their cubes underflow to -0); both signs
log-spaced over [1e-8, 16], most of them in [1e-6, 1.2]; clusters on both sides of 1e-5, 1e-4, 0.0031308, 0.018, 1/12
and 1; 6e4 .. 7e4 and 1e-8 .. 1e-4 for half-float overflow and subnormals.  NONNEG has no negative value (HLG: the
OOTF raises the pixel's luminance to a power) and carries grey pixels whose OOTF output surrounds HLG's 1/12."""
import numpy as np
import torch

from libjxl_amd import abi, synth

F32 = np.float32
SIGNED, NONNEG = "signed", "nonneg"
MAIN_SIZE = (520, 264)    # 2145 blocks: the format grid
KERNEL_SIZE = (264, 136)  # 561 blocks: the per-kernel runs
SRGB_LUMINANCES = (0.2126, 0.7152, 0.0722)
HLG_NITS = (1000.0, 334.0, 255.0)  # (at 334 nits the system gamma is within 0.01 of 1: the reference skips the OOTF)

# the constants the transfer functions branch on, as the float32 code compares them (emit.h, oracle/output.c)
BRANCH = {abi.TF_LINEAR: None, abi.TF_SRGB: F32(0.0031308), abi.TF_PQ: F32(1e-4), abi.TF_709: F32(0.018),
          abi.TF_GAMMA: F32(1e-5), abi.TF_HLG: F32(1.0 / 12.0)}
ODD_SYMMETRIC = (abi.TF_SRGB, abi.TF_PQ, abi.TF_HLG)  # these look at |v|; 709 and gamma at v itself
CLUSTER_CENTRES = [F32(1e-5), F32(1e-4), F32(0.0031308), F32(0.018), F32(1.0 / 12.0), F32(1.0)]
NEAR = 1e-5  # "next to a branch point": within this, relative
TF_NAMES = {0: "linear", 1: "srgb", 2: "pq", 3: "709", 4: "gamma", 5: "hlg"}
ST_NAMES = {0: "f32", 1: "u8", 2: "u16", 3: "f16"}


def cube3(a):
    """XybToRgb's cube with a zero bias, in float32: fma(a * a, a, 0)."""
    a = np.asarray(a, F32)
    return ((a * a).astype(F32) * a).astype(F32)


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def _fast_powf(base, exponent):
    """FastPowf of the restatement (oracle/quant_tables.c), per distinct base."""
    import oracle
    L = oracle.lib()
    u, inv = np.unique(np.asarray(base, F32).ravel(), return_inverse=True)
    r = np.array([L.jxo_fast_powf(float(b), float(exponent)) for b in u], F32)
    return r[inv].reshape(np.shape(base))


def hlg_exponent(nits):
    """HlgOOTF's exponent gamma - 1 (0: the reference skips the OOTF), as context.hip and oracle/output.c compute it."""
    gamma = F32(F32(1 / F32(1.2)) * F32(np.power(F32(1.111), -np.log2(F32(nits) / F32(1000.0)), dtype=F32)))
    e = F32(gamma - F32(1))
    return float(e) if (e < F32(-0.01) or F32(0.01) < e) else 0.0


def tf_input(fmt, lin):
    """What the transfer function's branch sees: the linear sample, or for HLG the sample behind the OOTF
    (HlgOOTF::Apply: the pixel times min(luminance ^ exponent, 1e9)), restated here in float32."""
    lin = np.asarray(lin, F32)
    if fmt["transfer"] != abi.TF_HLG:
        return lin
    e = hlg_exponent(fmt["tf_param"])
    if e == 0.0:
        return lin
    lum_w = [F32(v) for v in fmt.get("luminances", SRGB_LUMINANCES)]
    lum = _fma(lum_w[0], lin[..., 0], _fma(lum_w[1], lin[..., 1], (lum_w[2] * lin[..., 2]).astype(F32)))
    with np.errstate(invalid="ignore"):
        pw = _fast_powf(lum, e)
        ratio = np.where(pw < F32(1e9), pw, F32(1e9)).astype(F32)
        return (lin * ratio[..., None]).astype(F32)


# ---- the value list ---------------------------------------------------------------------------------------------

def _neighbours(a0, reach=400):
    return (np.full(2 * reach + 1, a0, F32).view(np.int32) + np.arange(-reach, reach + 1, dtype=np.int32)).view(F32)


def _spread(a, value, t, offsets):
    """Of the candidates a (ascending, with `value` non-decreasing in them) the offsets-th nearest strictly below and
    strictly above t, as long as they stay within NEAR of it."""
    below, above = a[value < t][::-1], a[value > t]
    vb, va = value[value < t][::-1], value[value > t]
    pick = [below[o - 1] for o in offsets if o <= len(below) and abs(float(vb[o - 1]) / float(t) - 1) < 0.9 * NEAR]
    pick += [above[o - 1] for o in offsets if o <= len(above) and abs(float(va[o - 1]) / float(t) - 1) < 0.9 * NEAR]
    assert len(pick) >= 2 and min(value[np.isin(a, pick)]) < t < max(value[np.isin(a, pick)]), (t, pick)
    return np.array(pick, F32)


def _offsets(nblocks):
    # a large frame affords clusters dense next to the point and reaching out to ~NEAR (a filter or an upsampling
    # kernel in front of the encoder moves a constant block by a few 1e-7 relative); a small frame three or two per side
    return (1, 2, 3, 5, 8, 13, 21, 34) if nblocks >= 500 else (2, 8, 20) if nblocks >= 100 else (3, 15)


def _clusters(nblocks):
    out = []
    for t in CLUSTER_CENTRES:
        a = _neighbours(F32(np.cbrt(float(t))))
        out.append(_spread(a, cube3(a), t, _offsets(nblocks)))
    return np.concatenate(out)


def _hlg_grey(nits, nblocks):
    """Cube roots a of grey pixels (a, a, a) whose OOTF output surrounds HLG's branch point 1/12."""
    t = BRANCH[abi.TF_HLG]
    fmt = dict(transfer=abi.TF_HLG, tf_param=nits)
    e = hlg_exponent(nits)
    assert e != 0.0
    guess = F32(np.cbrt(float(t) ** (1.0 / (1.0 + e))))  # luminance of grey v is ~v: the output is ~v^(1 + e)
    for _ in range(4):  # FastPowf is a few 1e-5 off the power: walk the guess onto the point
        a = _neighbours(guess, 4000)
        v = cube3(a)
        out = tf_input(fmt, np.stack([v, v, v], axis=-1))[..., 0]
        if out[0] < t < out[-1]:
            break
        guess = F32(guess * F32(np.cbrt((float(t) / float(out[len(out) // 2])) ** (1.0 / (1.0 + e)))))
    keep = np.concatenate([[True], np.diff(out) > 0])  # (monotone up to FastPowf's ripple: keep an ascending subset)
    order = np.argsort(out[keep], kind="stable")
    return _spread(a[keep][order], out[keep][order], t, _offsets(nblocks))


def _log(lo, hi, n):
    return np.exp(np.linspace(np.log(lo), np.log(hi), n)) if n > 0 else np.zeros(0)


def planted_cbrt(xsb, ysb, variant, seed=0x5EED):
    """(ysb, xsb, 3) float32: the cube roots of the linear (r, g, b) each block carries."""
    assert variant in (SIGNED, NONNEG)
    nblocks = xsb * ysb
    rng = np.random.default_rng(seed)
    blocks = [np.zeros(3, F32), np.full(3, -1e-16, F32)]  # +0; -0 (cube3(-1e-16) underflows to -0 in all three)
    if variant == NONNEG:
        blocks[1] = np.zeros(3, F32)
    cl = _clusters(nblocks)
    if variant == SIGNED and nblocks >= 500:  # (the conditions look at |v|: a small frame plants the positive side only)
        cl = np.concatenate([cl, -cl])
    cl = cl[rng.permutation(len(cl))]
    if len(cl) % 2:
        cl = np.concatenate([cl, cl[:1]])
    for rg, b in zip(cl[0::2], cl[1::2]):
        blocks.append(np.array([rg, rg, b], F32))
    if variant == NONNEG:
        for nits in HLG_NITS:
            if hlg_exponent(nits) != 0.0:
                blocks += [np.full(3, a, F32) for a in _hlg_grey(nits, nblocks)]
    nfree = 3 * (nblocks - len(blocks))
    assert nfree >= 36, "frame too small for the value list: %d blocks, %d taken" % (nblocks, len(blocks))
    n_zero = 3
    n_hi = max(6, nfree // 30)    # 6e4 .. 7e4: around the largest half-float (65504; 65520 and up round to inf)
    n_sub = max(6, nfree // 12)   # 1e-8 .. 1e-4: half-float subnormals (below 6.1e-5) and what rounds to zero
    n_wide = max(8, nfree // 5)   # the thin ends of [1e-8, 16]
    n_main = nfree - n_zero - n_hi - n_sub - n_wide
    lin = np.concatenate([np.zeros(n_zero), np.linspace(6e4, 7e4, n_hi), _log(1e-8, 1e-4, n_sub),
                          _log(1e-8, 1e-6, n_wide // 2), _log(1.2, 16.0, n_wide - n_wide // 2),
                          _log(1e-6, 1.2, n_main)])
    if variant == SIGNED:  # every other value of each range negative
        lin = lin * np.where(np.arange(len(lin)) % 2 == 0, 1.0, -1.0)
    a = np.cbrt(lin).astype(F32)
    order = np.argsort(np.abs(a), kind="stable")
    a = a[order]
    third = np.arange(len(a)) % 3 == 2
    b_vals = a[third][rng.permutation(int(third.sum()))]
    rg_vals = a[~third].reshape(-1, 2)  # neighbours in magnitude
    flip = rng.random(len(rg_vals)) < 0.5
    rg_vals = np.where(flip[:, None], rg_vals[:, ::-1], rg_vals)
    blocks += [np.array([r, g, b], F32) for (r, g), b in zip(rg_vals, b_vals)]
    assert len(blocks) == nblocks
    arr = np.stack(blocks)[rng.permutation(nblocks)]
    return np.ascontiguousarray(arr.reshape(ysb, xsb, 3))


def sweep_frame(xsize, ysize, variant, *, device="cpu", **kw):
    """synth.synth_frame's (params, tensors) with the sweep planted; kw as synth_frame (gab, epf_iters, output_kind,
    out_format, undo_orientation)."""
    params, t = synth.synth_frame(xsize, ysize, mix=synth.MIX_DCT8, device=device, **kw)
    for c in t["coeffs"]:
        c.zero_()
    params["inverse_opsin_matrix"] = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    params["opsin_biases"] = [0.0, 0.0, 0.0]
    a = planted_cbrt((xsize + 7) // 8, (ysize + 7) // 8, variant)
    y = ((a[..., 0] + a[..., 1]) * F32(0.5)).astype(F32)
    x = ((a[..., 0] - a[..., 1]) * F32(0.5)).astype(F32)
    t["dc"] = [torch.from_numpy(np.ascontiguousarray(p)).to(device) for p in (x, y, a[..., 2])]
    return params, t


def sweep_case(xsize, ysize, variant, **kw):
    """(params, CPU tensors, oracle.Frame) as frames.make_case."""
    import frames
    import oracle
    params, t = sweep_frame(xsize, ysize, variant, **kw)
    return params, t, frames.oracle_frame(params, t, oracle.default_dequant_tables())


# ---- the format grid --------------------------------------------------------------------------------------------

TF_PARAMS = [(abi.TF_LINEAR, 0.0), (abi.TF_SRGB, 0.0), (abi.TF_PQ, 1000.0), (abi.TF_PQ, 255.0), (abi.TF_709, 0.0),
             (abi.TF_GAMMA, 1 / 2.6), (abi.TF_GAMMA, 0.45455)] + [(abi.TF_HLG, n) for n in HLG_NITS]
# the formats with a kernel of their own (JXLHIP_FIXED_FORMATS, filters_fast.h): (transfer, sample type, channels, swap)
FIXED_FORMATS = [(1, 1, 3, 0), (1, 1, 4, 0), (1, 2, 3, 0), (1, 2, 4, 0), (1, 2, 3, 1), (1, 2, 4, 1), (2, 2, 3, 1),
                 (2, 2, 4, 1), (1, 0, 3, 0), (1, 0, 4, 0), (0, 0, 4, 0), (1, 3, 4, 0), (0, 3, 4, 0)]


def fmt(tf, st, nc, bits=None, swap=0, par=0.0):
    if bits is None:
        bits = {abi.SAMPLE_U8: 8, abi.SAMPLE_U16: 16}.get(st, 0)
    return dict(transfer=tf, sample_type=st, num_channels=nc, bits_per_sample=bits, swap_endianness=swap,
                tf_param=float(par), luminances=SRGB_LUMINANCES)


def fmt_id(f):
    s = "%s%s-%sx%d" % (TF_NAMES[f["transfer"]], ("%g" % f["tf_param"]) if f["tf_param"] else "",
                        ST_NAMES[f["sample_type"]], f["num_channels"])
    if f["sample_type"] in (abi.SAMPLE_U8, abi.SAMPLE_U16):
        s += "-%db" % f["bits_per_sample"]
    return s + ("-be" if f["swap_endianness"] else "")


def is_fixed(f):
    return (f["transfer"], f["sample_type"], f["num_channels"], int(bool(f["swap_endianness"]))) in FIXED_FORMATS


def variant_of(f):
    return NONNEG if f["transfer"] == abi.TF_HLG else SIGNED


def format_grid():
    """Every transfer function (and parameter) x {F32, F16, U8, U16} x {3, 4} channels x both endiannesses where the
    type has one; and, with 3 channels, U8 at 1, 5, 7 bits and U16 at 1, 8, 9, 10, 12, 15 bits (8 and 16 are above)."""
    g = []
    for tf, par in TF_PARAMS:
        for nc in (3, 4):
            for st in (abi.SAMPLE_F32, abi.SAMPLE_F16, abi.SAMPLE_U8, abi.SAMPLE_U16):
                for sw in ((0,) if st == abi.SAMPLE_U8 else (0, 1)):
                    g.append(fmt(tf, st, nc, swap=sw, par=par))
        g += [fmt(tf, abi.SAMPLE_U8, 3, bits=b, par=par) for b in (1, 5, 7)]
        g += [fmt(tf, abi.SAMPLE_U16, 3, bits=b, par=par) for b in (1, 8, 9, 10, 12, 15)]
    return g


# the per-kernel runs: every store shape (U8x3, U8x4, 16-bit x3, 16-bit x4, F32x3, F32x4), every transfer function,
# none of them a fixed format -- the general kernels take these
GENERAL_LIST = [fmt(abi.TF_709, abi.SAMPLE_U8, 3, bits=7), fmt(abi.TF_HLG, abi.SAMPLE_U8, 4, par=1000.0),
                fmt(abi.TF_GAMMA, abi.SAMPLE_U16, 3, bits=10, par=0.45455),
                fmt(abi.TF_PQ, abi.SAMPLE_U16, 4, par=255.0), fmt(abi.TF_SRGB, abi.SAMPLE_F16, 3, swap=1),
                fmt(abi.TF_LINEAR, abi.SAMPLE_F32, 3), fmt(abi.TF_PQ, abi.SAMPLE_F32, 4, swap=1, par=1000.0)]
assert not any(is_fixed(f) for f in GENERAL_LIST)
FIXED_LIST = [fmt(tf, st, nc, swap=sw, par=1000.0 if tf == abi.TF_PQ else 0.0) for tf, st, nc, sw in FIXED_FORMATS]
# one format per store shape (the edge runs)
STORE_SHAPES = [fmt(abi.TF_SRGB, abi.SAMPLE_U8, 3), fmt(abi.TF_709, abi.SAMPLE_U8, 4),
                fmt(abi.TF_PQ, abi.SAMPLE_U16, 3, swap=1, par=1000.0), fmt(abi.TF_GAMMA, abi.SAMPLE_F16, 4, par=1 / 2.6),
                fmt(abi.TF_LINEAR, abi.SAMPLE_F32, 3), fmt(abi.TF_SRGB, abi.SAMPLE_F32, 4)]


# ---- population conditions --------------------------------------------------------------------------------------

def population_problems(f, lin, variant, want=None):
    """What a run with format f on the linear pixels `lin` (H, W, 3) fails to exercise; [] when all conditions hold."""
    import oracle
    lin = np.asarray(lin, F32)
    bad = []
    if not np.isfinite(lin).all():
        bad.append("%d non-finite linear samples" % int((~np.isfinite(lin)).sum()))
    t = BRANCH[f["transfer"]]
    if t is not None:
        v = tf_input(f, lin)
        v = np.abs(v) if f["transfer"] in ODD_SYMMETRIC else v
        with np.errstate(invalid="ignore"):
            if not ((v < t) & (v >= t * F32(1 - NEAR))).any():
                bad.append("no sample just below the branch point %r" % float(t))
            if not ((v > t) & (v <= t * F32(1 + NEAR))).any():
                bad.append("no sample just above the branch point %r" % float(t))
    if variant == SIGNED:
        if not (lin < 0).any():
            bad.append("no negative sample")
        if not ((lin == 0) & np.signbit(lin)).any():
            bad.append("no -0 sample")
    if not (lin == 0).any():
        bad.append("no zero sample")
    if not (lin > 1).any():
        bad.append("no sample above 1")
    st = f["sample_type"]
    if st in (abi.SAMPLE_U8, abi.SAMPLE_U16):
        want = oracle.pack_output(dict(f, swap_endianness=0), lin) if want is None else native(f, want)
        top = (1 << f["bits_per_sample"]) - 1
        if not (want[..., :3] == 0).any():
            bad.append("code 0 never occurs")
        if not (want[..., :3] == top).any():
            bad.append("code %d never occurs" % top)
    if st == abi.SAMPLE_F16 and f["transfer"] == abi.TF_LINEAR:
        mag = np.abs(lin)
        if not (mag >= 65520).any() or not ((mag > 6e4) & (mag < 65504)).any():
            bad.append("the half-float overflow point is not straddled")
        if not ((mag > 2.0 ** -24) & (mag < 2.0 ** -14)).any() or not ((mag > 0) & (mag < 2.0 ** -25)).any():
            bad.append("no half-float subnormal / no sample that rounds to a half-float zero")
    return bad


# ---- the comparison ---------------------------------------------------------------------------------------------

ULP_BAR = {abi.TF_SRGB: 8, abi.TF_PQ: 12}  # hardware v_sqrt_f32 / v_rcp_f32 in emit.h; every other function: 0
EXACT = (abi.TF_LINEAR, abi.TF_709, abi.TF_GAMMA, abi.TF_HLG)


def native(f, a):
    """The samples in host byte order and their natural dtype (uint8, uint16, float32; half-floats as uint16 bits)."""
    dt = {0: np.float32, 1: np.uint8, 2: np.uint16, 3: np.uint16}[f["sample_type"]]
    a = np.ascontiguousarray(a)
    a = a.view(dt) if a.dtype.itemsize == np.dtype(dt).itemsize else a.view(np.uint8).view(dt)
    if f["swap_endianness"] and a.dtype.itemsize > 1:
        a = a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))[..., ::-1].copy().view(dt).reshape(a.shape)
    return a


def _half_order(bits):
    """Half-float bit patterns on a line: neighbouring halfs are neighbouring integers (-0 and +0 coincide)."""
    b = bits.astype(np.int64)
    return np.where(b & 0x8000, -(b & 0x7FFF), b & 0x7FFF)


def _half_is_nan(bits):
    return ((bits & 0x7C00) == 0x7C00) & ((bits & 0x3FF) != 0)


def ulp_distance(got, want):
    """|got - want| in units of the float32 spacing at `want`; samples where want is NaN: 0 when got is NaN, else inf."""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    d = np.where(got == want, 0.0, d)  # (equal infinities)
    nan_w = np.isnan(want)
    d = np.where(nan_w, np.where(np.isnan(got), 0.0, np.inf), d)
    return np.where(~nan_w & np.isnan(d), np.inf, d)


def compare(f, got, want, lin, got_f32=None, want_f32=None):
    """Holds the packed output `got` to the yardstick `want` = oracle.pack_output(f, lin) under the bars of the format:

      linear, 709, gamma, HLG   every byte equal (where the expected float sample is NaN: NaN, whatever its bits);
      sRGB, PQ, float samples   <= 8 / <= 12 float32 ulps of the expected sample; sRGB at |linear| <= 0.0031308 (one
                                multiply) bit-equal; half-floats at most one half-float step from the expected one, and
                                only where the float32 samples of the same run differ (got_f32, want_f32: the F32 output
                                of the same transfer function on the same pixels, device and yardstick);
      sRGB, PQ, integers        max |got - want| <= 1, differing share <= 2 * (2 K 2^-24 (2^bits - 1)) + 4 / N;
      alpha (4 channels)        exactly the maximum code / 1.0.

    Returns dict(ulp=worst float32 ulp distance or None, maxdiff=worst integer / half-step distance or None,
    share=share of differing samples).  Raises AssertionError."""
    name = fmt_id(f)
    tf, st, nc = f["transfer"], f["sample_type"], f["num_channels"]
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert got.dtype.itemsize == want.dtype.itemsize, (name, got.dtype, want.dtype)
    g, w = native(f, got), native(f, want)
    res = dict(ulp=None, maxdiff=None, share=float((g[..., :3] != w[..., :3]).mean()))
    if nc == 4:  # the opaque alpha the reference substitutes
        one = {0: F32(1.0).view(np.uint32), 1: (1 << f["bits_per_sample"]) - 1, 2: (1 << f["bits_per_sample"]) - 1,
               3: 0x3C00}[st]
        ga = g[..., 3].view(np.uint32) if st == abi.SAMPLE_F32 else g[..., 3]
        assert (ga == one).all(), "%s: alpha is not the maximum code / 1.0 everywhere" % name
    g, w = g[..., :3], w[..., :3]
    if tf in EXACT:
        if st == abi.SAMPLE_F32:
            nan = np.isnan(w)
            assert np.isnan(g[nan]).all(), "%s: a sample is not NaN where NaN is expected" % name
            ne = (g.view(np.uint32) != w.view(np.uint32)) & ~nan
            res["ulp"] = float(ulp_distance(g, w).max())
        elif st == abi.SAMPLE_F16:
            nan = _half_is_nan(w)
            assert _half_is_nan(g[nan]).all(), "%s: a sample is not NaN where NaN is expected" % name
            ne = (g != w) & ~nan
        else:
            ne = g != w
        assert not ne.any(), "%s: %d samples differ, first at (y, x, c) = %s: got %r, want %r" % (
            name, int(ne.sum()), tuple(np.argwhere(ne)[0]), g[ne][0], w[ne][0])
        return res
    K = ULP_BAR[tf]
    low = np.abs(np.asarray(lin, F32)) <= BRANCH[abi.TF_SRGB] if tf == abi.TF_SRGB else np.zeros(g.shape, bool)
    if st == abi.SAMPLE_F32:
        d = ulp_distance(g, w)
        res["ulp"] = float(d.max())
        assert res["ulp"] <= K, "%s: %.1f float32 ulps from the yardstick at (y, x, c) = %s (bar %d)" % (
            name, res["ulp"], tuple(np.argwhere(d == d.max())[0]), K)
        ne = (g.view(np.uint32) != w.view(np.uint32)) & low
        assert not ne.any(), "%s: %d samples of the 12.92 x branch are not bit-equal" % (name, int(ne.sum()))
    elif st == abi.SAMPLE_F16:
        nan = _half_is_nan(w)
        assert _half_is_nan(g[nan]).all(), "%s: a sample is not NaN where NaN is expected" % name
        step = np.abs(_half_order(g) - _half_order(w))
        step[nan] = 0
        res["maxdiff"] = int(step.max())
        assert res["maxdiff"] <= 1, "%s: a half-float sample is %d steps from the yardstick" % (name, res["maxdiff"])
        assert got_f32 is not None and want_f32 is not None, "half-float sRGB / PQ needs the float32 samples of the run"
        same32 = np.asarray(got_f32, F32)[..., :3].view(np.uint32) == np.asarray(want_f32, F32)[..., :3].view(np.uint32)
        stray = (g != w) & ~nan & same32
        assert not stray.any(), "%s: %d half-float samples differ where the float32 samples agree" % (
            name, int(stray.sum()))
        assert not ((g != w) & low).any(), "%s: a half-float sample of the 12.92 x branch differs" % name
    else:
        d = np.abs(g.astype(np.int64) - w.astype(np.int64))
        res["maxdiff"] = int(d.max())
        assert res["maxdiff"] <= 1, "%s: a sample is %d codes from the yardstick" % (name, res["maxdiff"])
        bar = 2 * (2 * K * 2.0 ** -24 * ((1 << f["bits_per_sample"]) - 1)) + 4.0 / d.size
        assert res["share"] <= bar, "%s: %.3e of the samples differ (bar %.3e)" % (name, res["share"], bar)
    return res


def check_padding(raw, row_bytes, sentinel):
    """raw: (H, stride) uint8, the whole output buffer; every byte behind the row must still hold the sentinel."""
    pad = raw[:, row_bytes:]
    assert pad.size > 0
    touched = np.argwhere(pad != sentinel)
    assert len(touched) == 0, "%d padding bytes touched, first in row %d at byte %d of the row" % (
        len(touched), touched[0][0], row_bytes + touched[0][1])


def rows_of(f, raw, xsize):
    """The (H, W, channels) sample array inside a padded buffer raw (H, stride) uint8."""
    dt = {0: np.float32, 1: np.uint8, 2: np.uint16, 3: np.uint16}[f["sample_type"]]
    row_bytes = xsize * f["num_channels"] * np.dtype(dt).itemsize
    body = np.ascontiguousarray(raw[:, :row_bytes])
    return body.view(dt).reshape(raw.shape[0], xsize, f["num_channels"]), row_bytes
