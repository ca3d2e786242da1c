"""The reference's ToneMappingStage for a PQ original (render_pipeline/stage_tone_mapping.cc, cms/tone_mapping-inl.h,
cms/tone_mapping.h, TF_PQ of cms/transfer_functions-inl.h) restated as one numpy float32 function, the constants it
takes, and the JxlDecoder loop that asks the reference for tone-mapped pixels.  Test infrastructure.

Every operation is the one a single lane of the reference performs: float32 throughout, MulAdd as a single-rounding
fused multiply-add (fma below: exact through a float64 sum rounded to odd), IEEE square roots and divisions.

FAULTS: the four deliberate mistakes tests/test_tone_mapping_model.py puts into the model, one at a time, to show that
the GPU tier's bar would see them."""
import ctypes as C
import math

import numpy as np

F32 = np.float32
FAULTS = ("ks_moved", "no_gamut_map", "no_to_intensity_target", "identity_spline")
NUM_CONSTANTS = 18
(K_TO, K_FROM, K_SRC, K_DST, K_LR, K_LG, K_LB, K_PQMIN, K_PQRANGE, K_INVPQRANGE, K_MINLUM, K_MAXLUM, K_KS, K_INV1MKS,
 K_NORM, K_INVPEAK, K_1MKS, K_SAT) = range(NUM_CONSTANTS)


def fma(a, b, c):
    """fl32(a * b + c) with one rounding: the float64 product of two float32 values is exact; the float64 sum is
    rounded to odd (so that the final rounding to float32 sees on which side of a tie the exact value lies)."""
    a, b, c = (np.asarray(v, F32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)  # TwoSum: s + err == p + c exactly
    even = (np.asarray(s).view(np.int64) & 1) == 0
    with np.errstate(invalid="ignore"):
        nudge = (err != 0) & even & np.isfinite(s)
        s = np.where(nudge, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def _mul(a, b):
    return (np.asarray(a, F32) * np.asarray(b, F32)).astype(F32)


def _div(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.asarray(a, F32) / np.asarray(b, F32)).astype(F32)


def _min(a, b):  # hwy Min on one lane: (b < a) ? b : a
    return np.where(np.asarray(b) < np.asarray(a), b, a).astype(F32)


def _max(a, b):  # (a < b) ? b : a
    return np.where(np.asarray(a) < np.asarray(b), b, a).astype(F32)


def _rational44(x, p, q):
    yp, yq = np.full(np.shape(x), p[4], F32), np.full(np.shape(x), q[4], F32)
    for i in (3, 2, 1, 0):
        yp = fma(yp, x, F32(p[i]))
        yq = fma(yq, x, F32(q[i]))
    return _div(yp, yq)


_P_HI = (1.351392e-02, -1.095778e+00, 5.522776e+01, 1.492516e+02, 4.838434e+01)
_Q_HI = (1.012416e+00, 2.016708e+01, 9.263710e+01, 1.120607e+02, 2.590418e+01)
_P_LO = (9.863406e-06, 3.881234e-01, 1.352821e+02, 6.889862e+04, -2.864824e+05)
_Q_LO = (3.371868e+01, 1.477719e+03, 1.608477e+04, -4.389884e+04, -2.072546e+05)
_P_INV = (2.62975656e-04, -6.23553089e-03, 7.38602301e-01, 2.64553172e+00, 5.50034862e-01)
_Q_INV = (4.21350107e+02, -4.28736818e+02, 1.74364667e+02, -3.39078883e+01, 2.67718770e+00)


def pq_encoded_from_display_1(v):
    """TF_PQ(1.0)::EncodedFromDisplay (transfer_functions-inl.h:172-207)."""
    v = np.asarray(v, F32)
    x = np.abs(v)
    scale = F32(F32(1.0) * (F32(1.0) / F32(10000.0)))
    with np.errstate(invalid="ignore"):
        r = np.sqrt(np.sqrt(_mul(x, scale)).astype(F32)).astype(F32)
        mag = np.where(x < F32(1e-4), _rational44(r, _P_LO, _Q_LO), _rational44(r, _P_HI, _Q_HI)).astype(F32)
    return np.copysign(np.abs(mag), v).astype(F32)


def pq_display_from_encoded_1(v):
    """TF_PQ(1.0)::DisplayFromEncoded (transfer_functions-inl.h:145-168)."""
    v = np.asarray(v, F32)
    x = np.abs(v)
    mag = _mul(_rational44(fma(x, x, x), _P_INV, _Q_INV), F32(10000.0))
    return np.copysign(np.abs(mag), v).astype(F32)


def _inv_eotf_scalar(lum):
    """TF_PQ_Base::EncodedFromDisplay(1.0, lum) (cms/transfer_functions.h:107-119): double arithmetic, float result."""
    d = float(F32(lum))
    if d == 0.0:
        return F32(0.0)
    m1, m2 = 2610.0 / 16384, (2523.0 / 4096) * 128
    c1, c2, c3 = 3424.0 / 4096, (2413.0 / 4096) * 32, (2392.0 / 4096) * 32
    xp = math.pow(abs(d) * float(F32(F32(1.0) * (F32(1.0) / F32(10000.0)))), m1)
    e = math.pow((c1 + xp * c2) / (1.0 + xp * c3), m2)
    return F32(math.copysign(float(F32(e)), d))


def constants(orig, desired, luminances, dest_pq):
    """The constants of ToneMappingStage's constructor and Rec2408ToneMapperBase's member initialisers, in the order
    jxlhip_tone_mapping_constants reports them: float32[18]."""
    orig, desired = F32(orig), F32(desired)
    k = np.zeros(NUM_CONSTANTS, F32)
    k[K_TO] = F32(10000.0) / orig if dest_pq else F32(1.0)
    k[K_FROM] = desired / F32(10000.0) if dest_pq else F32(1.0)
    k[K_SRC], k[K_DST] = orig, desired
    k[K_LR:K_LB + 1] = np.asarray(luminances, F32)
    pq_min = _inv_eotf_scalar(0.0)
    pq_range = F32(_inv_eotf_scalar(orig) - pq_min)
    inv_range = F32(F32(1.0) / pq_range)
    k[K_PQMIN], k[K_PQRANGE], k[K_INVPQRANGE] = pq_min, pq_range, inv_range
    k[K_MINLUM] = F32(F32(_inv_eotf_scalar(0.0) - pq_min) * inv_range)
    k[K_MAXLUM] = F32(F32(_inv_eotf_scalar(desired) - pq_min) * inv_range)
    k[K_KS] = F32(F32(F32(1.5) * k[K_MAXLUM]) - F32(0.5))
    k[K_INV1MKS] = F32(1.0) / max(F32(1e-6), F32(F32(1.0) - k[K_KS]))
    k[K_NORM] = orig / desired
    k[K_INVPEAK] = F32(1.0) / desired
    k[K_1MKS] = F32(F32(1.0) - k[K_KS])
    k[K_SAT] = F32(0.1)
    return k


def normalized_pq(lin, k):
    """What the knee compares with ks, per pixel of LINEAR rgb (H, W, 3): for the population conditions."""
    rgb = _mul(np.asarray(lin, F32), k[K_TO])
    lum = _mul(k[K_SRC], fma(k[K_LR], rgb[..., 0], fma(k[K_LG], rgb[..., 1], _mul(k[K_LB], rgb[..., 2]))))
    return lum, _min(F32(1.0), _mul((pq_encoded_from_display_1(lum) - k[K_PQMIN]).astype(F32), k[K_INVPQRANGE]))


def tone_map(lin, k, fault=None, debug=None):
    """ToneMappingStage::ProcessRow on LINEAR rgb (H, W, 3) float32 with the constants k; returns float32.  debug: a
    dict that receives intermediates (population_problems reads them)."""
    assert fault is None or fault in FAULTS
    k = np.asarray(k, F32).copy()
    if fault == "ks_moved":  # the knee start 1 % off (and what the host derives from it)
        k[K_KS] = F32(k[K_KS] * F32(1.01))
        k[K_1MKS] = F32(F32(1.0) - k[K_KS])
        k[K_INV1MKS] = F32(1.0) / max(F32(1e-6), k[K_1MKS])
    if fault == "no_to_intensity_target":
        k[K_TO] = F32(1.0)
    rgb = _mul(np.asarray(lin, F32), k[K_TO])
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    # Rec2408ToneMapper::ToneMap (tone_mapping-inl.h:40-72)
    lum = _mul(k[K_SRC], fma(k[K_LR], r, fma(k[K_LG], g, _mul(k[K_LB], b))))
    npq_raw = _mul((pq_encoded_from_display_1(lum) - k[K_PQMIN]).astype(F32), k[K_INVPQRANGE])
    npq = _min(F32(1.0), npq_raw)
    t = _mul((npq - k[K_KS]).astype(F32), k[K_INV1MKS])
    t2 = _mul(t, t)
    t3 = _mul(t2, t)
    pa = fma(F32(2), t3, fma(F32(-3), t2, F32(1)))
    pb = (t3 + fma(F32(-2), t2, t)).astype(F32)
    pm = _mul(fma(F32(-2), t3, _mul(F32(3), t2)), k[K_MAXLUM])
    spline = fma(pa, k[K_KS], fma(pb, k[K_1MKS], pm))
    if fault == "identity_spline":
        spline = npq
    with np.errstate(invalid="ignore"):
        e2 = np.where(npq < k[K_KS], npq, spline).astype(F32)
    om = (F32(1) - e2).astype(F32)
    om2 = _mul(om, om)
    om4 = _mul(om2, om2)
    e3 = fma(k[K_MINLUM], om4, e2)
    e4 = fma(e3, k[K_PQRANGE], k[K_PQMIN])
    d4 = pq_display_from_encoded_1(e4)
    with np.errstate(invalid="ignore"):
        new_lum = _min(k[K_DST], np.where(d4 < 0, F32(0), d4).astype(F32))
        use_cap = lum <= F32(1e-6)
    ratio = _div(new_lum, _max(lum, F32(1e-6)))
    cap = _mul(new_lum, k[K_INVPEAK])
    mult = _mul(ratio, k[K_NORM])
    ch = [np.where(use_cap, cap, _mul(v, mult)).astype(F32) for v in (r, g, b)]
    if debug is not None:
        debug.update(lum=lum, npq=npq, npq_raw=npq_raw, use_cap=use_cap)
    if fault != "no_gamut_map":  # GamutMap (tone_mapping-inl.h:139-187)
        glum = fma(k[K_LR], ch[0], fma(k[K_LG], ch[1], _mul(k[K_LB], ch[2])))
        sat = np.zeros(glum.shape, F32)
        mixl = np.zeros(glum.shape, F32)
        vmgs = []
        for val in ch:
            vmg = (val - glum).astype(F32)
            vmgs.append(vmg)
            inv = _div(F32(1), np.where(vmg == 0, F32(1), vmg).astype(F32))
            vov = _mul(val, inv)
            with np.errstate(invalid="ignore"):
                sat = np.where(vmg >= 0, sat, _max(sat, vov)).astype(F32)
                mixl = _max(mixl, np.where(vmg <= 0, sat, (vov - inv).astype(F32)).astype(F32))
        mix = _min(_max(F32(0), fma(k[K_SAT], (sat - mixl).astype(F32), mixl)), F32(1))
        ch = [fma(mix, (glum - val).astype(F32), val) for val in ch]
        max_clr = _max(_max(F32(1), ch[0]), _max(ch[1], ch[2]))
        norm = _div(F32(1), max_clr)
        if debug is not None:
            debug.update(vmg=np.stack(vmgs, axis=-1), max_clr=max_clr)
        ch = [_mul(val, norm) for val in ch]
    return np.stack([_mul(val, k[K_FROM]) for val in ch], axis=-1).astype(F32)


# ---- the reference's public decoder with a display -----------------------------------------------------------------

JXL_DEC_COLOR_ENCODING = 0x100
# JxlColorEncoding's enums (lib/include/jxl/color_encoding.h)
PRIMARIES = {"srgb": 1, "rec2100": 9, "p3": 11}
TRANSFER = {"709": 1, "linear": 8, "srgb": 13, "pq": 16, "dci": 17, "hlg": 18}


class JxlColorEncoding(C.Structure):
    _fields_ = [("color_space", C.c_int), ("white_point", C.c_int), ("white_point_xy", C.c_double * 2),
                ("primaries", C.c_int), ("primaries_red_xy", C.c_double * 2), ("primaries_green_xy", C.c_double * 2),
                ("primaries_blue_xy", C.c_double * 2), ("transfer_function", C.c_int), ("gamma", C.c_double),
                ("rendering_intent", C.c_int)]


def color_encoding(primaries, transfer):
    """An enumerated RGB / D65 JxlColorEncoding, relative intent."""
    e = JxlColorEncoding()
    e.color_space, e.white_point, e.primaries = 0, 1, PRIMARIES[primaries]
    e.transfer_function, e.rendering_intent = TRANSFER[transfer], 1
    return e


def jxl_decode_display(RL, data, display_nits=None, encoding=None):
    """test_seam.jxl_decode's loop (float RGB) with JxlDecoderSetDesiredIntensityTarget(display_nits) and, at the
    colour-encoding event, JxlDecoderSetOutputColorProfile(encoding).  Returns ([H, W, 3] float32, the intensity target
    JxlDecoderGetBasicInfo reports)."""
    import test_seam as ts
    RL.JxlDecoderSetDesiredIntensityTarget.argtypes = [C.c_void_p, C.c_float]
    RL.JxlDecoderSetOutputColorProfile.argtypes = [C.c_void_p, C.POINTER(JxlColorEncoding), C.c_void_p, C.c_size_t]
    dec = RL.JxlDecoderCreate(None)
    assert dec
    try:
        events = ts.JXL_DEC_BASIC_INFO | JXL_DEC_COLOR_ENCODING | ts.JXL_DEC_FULL_IMAGE
        assert RL.JxlDecoderSubscribeEvents(dec, events) == ts.JXL_DEC_SUCCESS
        if display_nits is not None:
            assert RL.JxlDecoderSetDesiredIntensityTarget(dec, display_nits) == ts.JXL_DEC_SUCCESS
        assert RL.JxlDecoderSetInput(dec, data, len(data)) == ts.JXL_DEC_SUCCESS
        RL.JxlDecoderCloseInput(dec)
        fmt = ts.PixelFormat(3, 0, 0, 0)
        out, w, nits = None, 0, None
        while True:
            st = RL.JxlDecoderProcessInput(dec)
            if st == ts.JXL_DEC_BASIC_INFO:
                info = (C.c_uint8 * 1024)()
                assert RL.JxlDecoderGetBasicInfo(dec, info) == ts.JXL_DEC_SUCCESS
                w = int(np.frombuffer(bytes(info[4:8]), np.uint32)[0])
                nits = float(np.frombuffer(bytes(info[20:24]), np.float32)[0])  # JxlBasicInfo::intensity_target
            elif st == JXL_DEC_COLOR_ENCODING:
                if encoding is not None:
                    rc = RL.JxlDecoderSetOutputColorProfile(dec, C.byref(encoding), None, 0)
                    assert rc == ts.JXL_DEC_SUCCESS, "the reference refuses the output colour encoding"
            elif st == ts.JXL_DEC_NEED_IMAGE_OUT_BUFFER:
                n = C.c_size_t(0)
                assert RL.JxlDecoderImageOutBufferSize(dec, C.byref(fmt), C.byref(n)) == ts.JXL_DEC_SUCCESS
                out = np.zeros((n.value // (w * 12), w, 3), np.float32)
                assert RL.JxlDecoderSetImageOutBuffer(dec, C.byref(fmt), out.ctypes.data, n.value) == ts.JXL_DEC_SUCCESS
            elif st == ts.JXL_DEC_FULL_IMAGE:
                continue
            elif st == ts.JXL_DEC_SUCCESS:
                break
            else:
                raise AssertionError("JxlDecoderProcessInput -> %d" % st)
        return out, nits
    finally:
        RL.JxlDecoderDestroy(dec)


# ---- the planted-value frame ---------------------------------------------------------------------------------------

def planted_linear(nblocks, seed=0x70AE):
    """(nblocks, 3) float64: the linear (r, g, b) each 8x8 block of the planted frame carries, most telling first (a
    small frame takes the head of the list): black and near-black (use_cap), luminance above the source peak (the
    min(1, .)), greys (a component equal to the luminance: GamutMap's Eq guard), negative components, saturated
    colours that exceed 1 behind the tone mapper (max_clr); then log-spaced values on both sides of every knee."""
    head = [(0.9, 0.05, 0.0), (0.3, 0.3, 0.3), (0.0, 0.0, 0.0), (1.5, 1.5, 1.5), (0.5, -0.05, 0.2), (1.0, 0.0, 0.0),
            (0.02, 0.02, 0.02), (1e-12, 1e-12, 1e-12), (4.0, 0.2, 0.1), (0.0, 1.0, 0.0), (0.0, 0.0, 0.6), (-0.01, 0.3, 0.1),
            (0.2, 0.1, -0.3), (-0.1, -0.1, -0.1), (1.001, 1.001, 1.001), (0.0, 0.0, 1.0), (0.004, 0.001, 0.0)]
    head += [(v, v, v) for v in np.exp(np.linspace(np.log(1e-4), np.log(1.0), 24))]
    head += [(v, v, v) for v in (0.5, 0.25, 0.125, 0.0625)]
    rng = np.random.default_rng(seed)
    n = max(0, nblocks - len(head))
    base = np.exp(rng.uniform(np.log(1e-5), np.log(1.2), n))
    tail = np.stack([base * rng.uniform(0.5, 1.5, n), base * rng.uniform(0.5, 1.5, n), base * rng.uniform(0.2, 2.0, n)], axis=-1)
    return np.concatenate([np.array(head, np.float64), tail.reshape(-1, 3)])[:nblocks]


def planted_frame(xsize, ysize, *, device="cpu", **kw):
    """synth.synth_frame's (params, tensors) with planted_linear in the DC of a frame built the way
    output_sweep.sweep_frame builds its own: DCT8 blocks without AC, the identity for inverse_opsin_matrix, zero
    opsin_biases -- linear channel c of a block is the cube of (y + x, y - x, b)."""
    import torch
    from libjxl_amd import synth
    params, t = synth.synth_frame(xsize, ysize, mix=synth.MIX_DCT8, device=device, **kw)
    for c in t["coeffs"]:
        c.zero_()
    params["inverse_opsin_matrix"] = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    params["opsin_biases"] = [0.0, 0.0, 0.0]
    xsb, ysb = (xsize + 7) // 8, (ysize + 7) // 8
    a = np.cbrt(planted_linear(xsb * ysb)).astype(F32).reshape(ysb, xsb, 3)
    y = ((a[..., 0] + a[..., 1]) * F32(0.5)).astype(F32)
    x = ((a[..., 0] - a[..., 1]) * F32(0.5)).astype(F32)
    t["dc"] = [torch.from_numpy(np.ascontiguousarray(p)).to(device) for p in (x, y, a[..., 2])]
    return params, t


def population_problems(lin, k):
    """What the LINEAR pixels `lin` (H, W, 3) fail to exercise of the stage with constants k; [] when all hold."""
    dbg = {}
    tone_map(lin, k, debug=dbg)
    bad = []
    with np.errstate(invalid="ignore"):
        if not (dbg["npq"] < k[K_KS]).any() or not (dbg["npq"] >= k[K_KS]).any():
            bad.append("the knee start ks is not straddled")
        if not dbg["use_cap"].any():
            bad.append("no pixel of luminance <= 1e-6 (use_cap)")
        if not (dbg["npq_raw"] > 1).any():
            bad.append("no pixel above the source peak (the min(1, .))")
        if not (dbg["vmg"] == 0).any():
            bad.append("no component equal to the luminance (the Eq guard)")
        if not (np.asarray(lin) < 0).any():
            bad.append("no negative component")
        if not (dbg["max_clr"] > 1).any():
            bad.append("no component above 1 behind the mapping (max_clr)")
    return bad


# ---- comparisons and the GPU tier's bars ---------------------------------------------------------------------------

def compare_f32(got, want):
    """dict(ulp=worst float32 ulp distance, share=share of samples that differ at all)."""
    import output_sweep as S
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    d = S.ulp_distance(got, want)
    return dict(ulp=float(d.max()), maxdiff=None, share=float((got.view(np.uint32) != want.view(np.uint32)).mean()))


def compare_packed(f, got, want):
    """Colour samples of a packed output against the expected ones: dict(ulp, maxdiff = worst distance in codes or
    half-float steps, share of samples that differ)."""
    import output_sweep as S
    g, w = S.native(f, got)[..., :3], S.native(f, want)[..., :3]
    if f["sample_type"] == 0:
        return compare_f32(g, w)
    if f["sample_type"] == 3:
        d = np.abs(S._half_order(g) - S._half_order(w))
    else:
        d = np.abs(g.astype(np.int64) - w.astype(np.int64))
    return dict(ulp=None, maxdiff=int(d.max()), share=float((d != 0).mean()))


def check_bar(name, res):
    bar = GPU_BARS[name]
    if "ulp" in bar:
        assert res["ulp"] <= bar["ulp"], "%s: %.2f float32 ulps from the model (bar %d)" % (name, res["ulp"], bar["ulp"])
    else:
        assert res["maxdiff"] <= bar["maxdiff"], "%s: a sample is %d codes / steps from the model" % (name, res["maxdiff"])
        assert res["share"] <= bar["share"], "%s: %.3e of the samples differ (cap %.3e)" % (name, res["share"], bar["share"])


LUM_2100 = (0.2627002000808716, 0.6779980063438416, 0.0593017116189003)
ORIG_NITS = 1000.0


def gpu_cases():
    """The GPU tier's cases: (name, output kind, format or None, desired nits, luminances)."""
    import output_sweep as S
    from libjxl_amd import abi
    return [("linear-f32", 1, None, 250.0, S.SRGB_LUMINANCES),
            ("srgb-rgba8", 2, S.fmt(abi.TF_SRGB, abi.SAMPLE_U8, 4), 250.0, S.SRGB_LUMINANCES),  # (a fixed-format kernel)
            ("srgb-rgb8", 2, S.fmt(abi.TF_SRGB, abi.SAMPLE_U8, 3), 100.0, LUM_2100),  # (the other fixed-format kernel)
            ("709-u8x4-7b", 2, S.fmt(abi.TF_709, abi.SAMPLE_U8, 4, bits=7), 250.0, S.SRGB_LUMINANCES),  # (general tail, 8-bit stores)
            ("pq-u16", 2, S.fmt(abi.TF_PQ, abi.SAMPLE_U16, 3, par=ORIG_NITS), 100.0, LUM_2100),
            ("srgb-f16", 2, S.fmt(abi.TF_SRGB, abi.SAMPLE_F16, 3), 100.0, LUM_2100)]


# Kernel against model, per case of tests/test_gpu_tone_mapping.py.  Measured on an MI355X over the 72 runs of that
# file (3 sizes x 2 frames x 2 routings per case); the arithmetic is deterministic, the margin covers other seeds:
#   linear-f32   0 ulps, no sample differs in any run: k_tone_map restates the stage with IEEE division and square
#                root throughout and is bit-equal to the model.  Bar = 1.5 x 0 = 0 ulps.
#   srgb-rgba8   at most one code; worst share 1.85e-5 (263x137 d1 plain; 0 in the other eleven runs).  Cap 2x.
#   srgb-rgb8    at most one code; worst share 9.25e-6 (one sample of 263x137 d1 plain).  Cap 2x.
#   709-u8x4-7b  byte-equal in every run (an exact curve through the general tail).  Bar 0.
#   pq-u16       at most one code; worst share 6.94e-4 (263x137 planted plain).  Cap 2x.
#   srgb-f16     at most one half-float step; worst share 1.16e-4 (72x40 d1 plain: one sample).  Cap 2x.
# The integer and half-float differences are emit.h's hardware square root and reciprocal in the sRGB / PQ curve
# against oracle.pack_output (tests/test_gpu_output_encoding.py holds those on their own), not the tone mapper.
# The other form of the two PQ rationals (emit.h's Rational44 with v_rcp_f32, a -DJXLHIP_TONEMAP_RCP=1 build of
# kernels_tonemap.hip) measured on the same 72 runs: linear-f32 up to 3.1e9 float32 ulps from the model with half of
# the samples differing (GamutMap's differences of nearly equal values turn the rationals' last-place errors into whole
# values near zero), pq-u16 up to 5 codes, srgb-f16 up to 70 steps, 709-u8x4-7b one code.  A bar of 1.5 x 3.1e9 ulps
# would ask the faults to move the frames by 2.3e10 ulps; moving ks by 1 % moves the MIX_D1 frame by 4.3e5.  That form
# fails the fault-injection condition and is not in.
GPU_BARS = {
    "linear-f32": dict(ulp=0),
    "srgb-rgba8": dict(maxdiff=1, share=2 * 1.8502585736356655e-05),
    "srgb-rgb8": dict(maxdiff=1, share=2 * 9.251292868178327e-06),
    "709-u8x4-7b": dict(maxdiff=0, share=0.0),  # (an exact curve: bit-equal kernel, byte-equal output)
    "pq-u16": dict(maxdiff=1, share=2 * 0.0006938469651133746),
    "srgb-f16": dict(maxdiff=1, share=2 * 0.00011574074074074075),
}

# Whole files against JxlDecoder (tests/test_gpu_tone_mapping.py): max |difference| of float samples per destination
# and display peak = the maximum measured on an MI355X times 2 (263 x 137 Rec.2100 PQ stream of 1000 nits, 0 and 6
# workers alike).  Measured, with the same file's plain error (no tone mapping, same primaries and curve) beside it:
#   pq-rec2100    250 nits 5.364e-05 (plain 5.960e-07)    100 nits 2.682e-07 (plain 5.960e-07)
#   srgb-rec2100  250 nits 8.702e-06 (plain 1.371e-06)    100 nits 1.073e-05 (plain 1.371e-06)
#   srgb-srgb     250 nits 1.490e-05 (plain 3.159e-06)    100 nits 2.199e-05 (plain 3.159e-06)
#   linear-srgb   250 nits 2.921e-05 (plain 3.755e-06)    100 nits 4.452e-05 (plain 3.755e-06)
# The stage multiplies the pixel by (new luminance / luminance) * orig / desired, 4 and 10 here: the linear error of the
# pipeline in front of it comes out amplified by about that much.
_FILE_MEASURED = {("pq-rec2100", 250.0): 5.364e-05, ("pq-rec2100", 100.0): 2.682e-07,
                  ("srgb-rec2100", 250.0): 8.702e-06, ("srgb-rec2100", 100.0): 1.073e-05,
                  ("srgb-srgb", 250.0): 1.490e-05, ("srgb-srgb", 100.0): 2.199e-05,
                  ("linear-srgb", 250.0): 2.921e-05, ("linear-srgb", 100.0): 4.452e-05}
FILE_BARS = {k: 2 * v for k, v in _FILE_MEASURED.items()}


# ---- multi-frame files -----------------------------------------------------------------------------------------------

def with_animation(L, cs):
    """The image header (bytes up to the first frame) of bare codestream `cs`, rewritten to carry an AnimationHeader of
    100 ticks per second, no loops, no timecodes (image_metadata.cc:283-316, headers.cc AnimationHeader): extra_fields
    is switched on when the header has none.  The end of the coded header inside its last, zero-padded byte is found by
    trying: the rewritten header must read back through jxlhip_image_header_decode with have_animation set, every
    other field as before, and end exactly at its own last byte."""
    import layer_streams as ls
    from libjxl_amd import abi
    old, pos = abi.ImageHeader(), C.c_size_t(0)
    assert L.jxlhip_image_header_decode(cs, len(cs), C.byref(pos), None, 0, C.byref(old)) == 0
    assert not old.have_animation and not old.have_preview and not old.color_encoding.want_icc
    r = ls._Bits(cs, 16)  # behind the signature
    small = r.bits(1)  # SizeHeader
    r.bits(5) if small else r.u32(*ls._SIZE)
    if r.bits(3) == 0:
        r.bits(5) if small else r.u32(*ls._SIZE)
    assert r.bits(1) == 0, "ImageMetadata::all_default"
    at = r.pos
    extra = r.bits(1)
    if extra:
        r.bits(3)  # orientation
        assert r.bits(1) == 0 and r.bits(1) == 0, "have_intrinsic_size / have_preview"
        assert r.bits(1) == 0, "have_animation"
    resume = r.pos
    for end in range(pos.value - 7, pos.value + 1):
        if end < resume:
            continue
        w = ls._Writer()
        w.copy(cs, 0, at)
        w.bits(1, 1)  # extra_fields
        if extra:
            w.copy(cs, at + 1, resume - 1)  # orientation, have_intrinsic_size, have_preview
        else:
            w.bits(3, 0)  # orientation 1
            w.bits(1, 0)  # have_intrinsic_size
            w.bits(1, 0)  # have_preview
        w.bits(1, 1)  # have_animation
        w.bits(2, 0)  # tps_numerator = Val(100)
        w.bits(2, 0)  # tps_denominator = Val(1)
        w.bits(2, 0)  # num_loops = Val(0)
        w.bits(1, 0)  # have_timecodes
        w.copy(cs, resume, end)
        head = w.to_bytes()
        new, npos = abi.ImageHeader(), C.c_size_t(0)
        if L.jxlhip_image_header_decode(head, len(head), C.byref(npos), None, 0, C.byref(new)) != 0 or npos.value != len(head) * 8:
            continue
        same = all(getattr(new, f) == getattr(old, f) for f in ("xsize", "ysize", "orientation", "xyb_encoded", "intensity_target",
                                                                "num_extra_channels", "opsin_all_default"))
        same = same and bytes(new.color_encoding) == bytes(old.color_encoding)
        if same and new.have_animation and new.tps_numerator == 100 and new.tps_denominator == 1:
            return head
    raise AssertionError("no end of the image header reads back")


def splice_animation(L, header, streams, durations):
    """layer_streams.splice with `header` (the bytes of an image header alone, with_animation's) in front of full
    kReplace frames taken from `streams`, frame k shown for durations[k] ticks."""
    import layer_streams as ls
    from libjxl_amd import abi
    keep = ls.source_frame

    def source_frame(L_, cs, which=-1):
        if cs is header:  # (the header's own stream has no frame to walk)
            ih, pos = abi.ImageHeader(), C.c_size_t(0)
            assert L_.jxlhip_image_header_decode(cs, len(cs), C.byref(pos), None, 0, C.byref(ih)) == 0
            return cs, pos.value, ih
        return keep(L_, cs, which)

    ls.source_frame = source_frame
    try:
        return ls.splice(L, header, [dict(stream=s, duration=d) for s, d in zip(streams, durations)])
    finally:
        ls.source_frame = keep


def jxl_decode_frames_display(RL, data, display_nits=None, encoding=None):
    """layer_streams.jxl_decode_frames' loop (float RGB of every frame the coalescing JxlDecoder reports) with
    JxlDecoderSetDesiredIntensityTarget and, at the colour-encoding event, JxlDecoderSetOutputColorProfile."""
    import layer_streams as ls
    import test_seam as ts
    RL.JxlDecoderSetDesiredIntensityTarget.argtypes = [C.c_void_p, C.c_float]
    RL.JxlDecoderSetOutputColorProfile.argtypes = [C.c_void_p, C.POINTER(JxlColorEncoding), C.c_void_p, C.c_size_t]
    dec = RL.JxlDecoderCreate(None)
    assert dec
    frames = []
    try:
        events = ts.JXL_DEC_BASIC_INFO | JXL_DEC_COLOR_ENCODING | ls.JXL_DEC_FRAME | ts.JXL_DEC_FULL_IMAGE
        assert RL.JxlDecoderSubscribeEvents(dec, events) == ts.JXL_DEC_SUCCESS
        if display_nits is not None:
            assert RL.JxlDecoderSetDesiredIntensityTarget(dec, display_nits) == ts.JXL_DEC_SUCCESS
        assert RL.JxlDecoderSetInput(dec, data, len(data)) == ts.JXL_DEC_SUCCESS
        RL.JxlDecoderCloseInput(dec)
        fmt = ts.PixelFormat(3, 0, 0, 0)
        out, w = None, 0
        while True:
            st = RL.JxlDecoderProcessInput(dec)
            if st == ts.JXL_DEC_BASIC_INFO:
                info = (C.c_uint8 * 1024)()
                assert RL.JxlDecoderGetBasicInfo(dec, info) == ts.JXL_DEC_SUCCESS
                w = int(np.frombuffer(bytes(info[4:8]), np.uint32)[0])
            elif st == JXL_DEC_COLOR_ENCODING:
                if encoding is not None:
                    assert RL.JxlDecoderSetOutputColorProfile(dec, C.byref(encoding), None, 0) == ts.JXL_DEC_SUCCESS
            elif st == ls.JXL_DEC_FRAME:
                continue
            elif st == ts.JXL_DEC_NEED_IMAGE_OUT_BUFFER:
                n = C.c_size_t(0)
                assert RL.JxlDecoderImageOutBufferSize(dec, C.byref(fmt), C.byref(n)) == ts.JXL_DEC_SUCCESS
                out = np.zeros((n.value // (w * 12), w, 3), np.float32)
                assert RL.JxlDecoderSetImageOutBuffer(dec, C.byref(fmt), out.ctypes.data, n.value) == ts.JXL_DEC_SUCCESS
            elif st == ts.JXL_DEC_FULL_IMAGE:
                frames.append(out)
                out = None
            elif st == ts.JXL_DEC_SUCCESS:
                break
            else:
                raise AssertionError("JxlDecoderProcessInput -> %d" % st)
        return frames
    finally:
        RL.JxlDecoderDestroy(dec)
# The three-frame Rec.2100 PQ animation (seeds 12, 5, 9; 250 nits, linear sRGB primaries) through
# jxlhip_decode_codestream_next against JxlDecoder: the worst frame's measured maximum times 2
ANIMATION_BAR = 2 * 6.008e-05  # (measured 6.008e-05, 0 and 6 workers alike)
