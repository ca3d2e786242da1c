"""The output encoding stage ALONE (libjxl_amd/csrc/emit.h: transfer functions, scaling and 8-bit dither, clamp and
rounding, half-float conversion, byte swapping, the paired and DPP stores), in every kernel that carries it.

Principle: the same frame is decoded twice on the same path -- as JXLHIP_OUT_LINEAR_RGB_F32 (`lin`) and as
JXLHIP_OUT_PACKED -- and packed must be oracle.pack_output(format, lin) under the bars of output_sweep.compare:
every byte equal for linear / 709 / gamma / HLG; <= 8 (sRGB) and <= 12 (PQ) float32 ulps, at most one code or one
half-float step and a bounded share of differing samples for the two functions that use the hardware v_sqrt_f32 /
v_rcp_f32.  The input of the comparison is the device's own linear output, so what is measured is the encoder and its
stores and nothing in front of them; tests/test_reference_parity.py holds oracle.pack_output byte for byte to the
reference's FromLinearStage + WriteToOutputStage on the same frame and the same formats.  The frame
(tests/output_sweep.py) plants chosen linear values: both sides of every branch point, -0, negative values, values
above 1, 6e4 .. 7e4 and 1e-8 .. 1e-4; every test checks the population conditions on the device's linear output.

Every decoder here is created under JXLHIP_FUSE=0.  Left to itself a frame without loop filter takes the fused
kernel for the linear output at any size, and the fused kernels never emit packed samples: with the switch both
outputs come from the same kernel template (k_filters_fast<GAB, EPF, OUTK, FMT>, k_filters / k_xyb_only, and the
noise / spline / upsampling tails), which share XybToRgb.

Which kernel a row of the format grid takes: the 13 formats of JXLHIP_FIXED_FORMATS (output_sweep.FIXED_FORMATS:
sRGB u8 / u16 / u16-be RGB and RGBA, PQ u16-be RGB and RGBA, sRGB f32 RGB and RGBA, linear f32 RGBA, sRGB and linear
f16 RGBA -- at ANY bit depth, the depth is a launch parameter) take their own instantiation FmtSel<ID>; every other
row the general FmtSel<-1>.  The profile slots do not tell the two apart ("filters" either way), so the routing is
stated here, not asserted.

Seen on an MI355X ("WORST <kernel> <transfer> <format> ulp=.. maxdiff=.. share=..", one line per case: the worst
float32 ulp distance, the worst code / half-float step distance, the share of differing colour samples):

  linear, 709, gamma, HLG   every case byte-equal: all sample types, every kernel, the odd bit depths, both endiannesses.
  sRGB, float32             6 ulps on the 520x264 grid (general and fixed kernels alike); 4-5 at 264x136 on every stage
                            list, width and stride; 16 % of the samples differ by at least one ulp; bit-equal below 0.0031308.
  PQ, float32               7 ulps in the march, the generic kernel, the noise and spline tails and 2x / 4x upsampling,
                            8 behind 8x upsampling; 39-45 % of the samples differ.
  sRGB, integers            8 bits and fewer: no sample differs anywhere; 16 bits: one code, <= 4.7e-4 of the samples.
  PQ, integers              one code; 16 bits <= 5.9e-4 of the samples, 8 bits 2.4e-6.
  sRGB / PQ, half-float     one step, 1.9e-5 / 3.1e-4 of the samples, each where the float32 samples differ as well.
  padding                   untouched at +4 bytes in every store shape and at +1 byte for 8-bit RGB, widths 264 and 261.

Nothing here exceeded a bar, and the linear pixels of the two instantiations never had to be told apart: the exact
functions came out byte-equal, which they could not if `lin` were not what the packed kernel encoded."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import output_sweep as S
from libjxl_amd import abi

pytestmark = pytest.mark.gpu

STAGE_LISTS = [(0, 0), (1, 0), (0, 1), (1, 1), (0, 2), (1, 2)]
EPF3 = [(0, 3), (1, 3)]  # k_epf0 into row-major planes + the (0, 2) march in its row-major-source form
SWITCHES = ("JXLHIP_FUSE", "JXLHIP_FILTERS", "JXLHIP_MFMA", "JXLHIP_FUSED_PC_RH", "JXLHIP_FILTER_RH")
SENTINEL = 0xA5
# noise that is silent up to linear 8 and loud above (NoiseParams::lut over the intensity (y +- x) / 2 = cbrt / 2 in
# steps of 1 / 6): the planted clusters stay where they are, the blocks above 8 and at 6e4 carry real noise
NOISE = ([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0], 1, 0)


@functools.lru_cache(maxsize=None)
def inputs(size, variant):
    return S.sweep_frame(*size, variant, device="cuda")


@pytest.fixture(scope="module")
def decoder():
    """decoder(**env) -> the module's VarDctDecoder created under JXLHIP_FUSE=0 and `env` (a context copies its path
    switches when it is created); all of them closed behind the module."""
    from libjxl_amd import VarDctDecoder
    made = {}

    def get(**env):
        key = tuple(sorted(env.items()))
        if key not in made:
            saved = {k: os.environ.pop(k, None) for k in SWITCHES}
            os.environ.update(dict(env, JXLHIP_FUSE="0"))
            try:
                d = VarDctDecoder(0)
                d.dq = d.default_dequant_tables()
                d.generic = env.get("JXLHIP_FILTERS") == "generic"
            finally:
                for k in SWITCHES:
                    os.environ.pop(k, None)
                    if saved[k] is not None:
                        os.environ[k] = saved[k]
            made[key] = d
        return made[key]
    yield get
    for d in made.values():
        d.close()


def run(dec, size, variant, kind, f=None, gab=0, epf=0, orient=0, feature=None, pad=0):
    """One decode of the sweep frame.  feature: None | ("noise",) | ("splines",) | ("ups", n, (W, H)).  pad: bytes
    behind each output row (the buffer is prefilled with SENTINEL and comes back whole, as (H, stride) uint8)."""
    base, t = inputs(size, variant)
    params = dict(base, gab=int(gab), epf_iters=int(epf), output_kind=kind, out_format=f, undo_orientation=orient)
    dec.begin_frame(params)
    dec.set_inputs(t, dec.dq)
    if feature and feature[0] == "ups":
        dec.set_upsampling(feature[1], feature[2])
    if feature and feature[0] == "noise":
        dec.set_noise(*NOISE)
    if feature and feature[0] == "splines":
        from test_splines_front_end import built_sets
        sets = built_sets(*size)
        dec.set_splines(sets["edge"] + sets["tiny"])
    dec.profile(True)
    if pad:
        shape = dec.alloc_output().shape
        row_bytes = shape[1] * shape[2] * {0: 4, 1: 1, 2: 2, 3: 2}[f["sample_type"]]
        raw = torch.full((shape[0], row_bytes + pad), SENTINEL, dtype=torch.uint8, device="cuda")
        rc = dec.L.jxlhip_decode_frame(dec.ctx, C.c_void_p(raw.data_ptr()), row_bytes + pad, 0)
        assert rc == 0, dec.L.jxlhip_last_error(dec.ctx)
        dec.sync()
        return raw.cpu().numpy(), dec.profile_read()
    out = dec.decode_frame()
    dec.sync()
    return out.cpu().numpy(), dec.profile_read()


def f32_twin(f):
    return S.fmt(f["transfer"], abi.SAMPLE_F32, 3, par=f["tf_param"])


def check(oracle, kernel, dec, size, f, lin_cache, **how):
    """lin and packed from `dec` on the same path; conditions on lin; packed against the yardstick; the WORST line."""
    variant = S.variant_of(f)
    key = (size, variant, tuple(sorted(how.items())), id(dec))
    if key not in lin_cache:
        lin_cache[key], slots = run(dec, size, variant, 1, **how)
        assert "fused" not in slots, slots
    lin = lin_cache[key]
    got, slots = run(dec, size, variant, 2, f=f, **how)
    assert "fused" not in slots and "filters" in slots, slots
    if how.get("epf") == 3:  # k_epf0 in front of the march, unless the generic kernel takes all four stages
        assert ("epf0" in slots) == (not dec.generic), slots
    if how.get("feature"):
        assert {"noise": "noise", "splines": "splines", "ups": "upsample"}[how["feature"][0]] in slots, slots
    want = oracle.pack_output(f, lin)
    bad = S.population_problems(f, lin, variant, want=want)
    assert bad == [], (kernel, S.fmt_id(f), bad)
    extra = {}
    if f["sample_type"] == abi.SAMPLE_F16 and f["transfer"] in S.ULP_BAR:
        g32, _ = run(dec, size, variant, 2, f=f32_twin(f), **how)
        extra = dict(got_f32=g32, want_f32=oracle.pack_output(f32_twin(f), lin))
    report(kernel, f, S.compare(f, got, want, lin, **extra))
    return got, want, lin


def report(kernel, f, res):
    print("WORST %s %s %s ulp=%s maxdiff=%s share=%.3e" % (
        kernel, S.TF_NAMES[f["transfer"]], S.fmt_id(f), "-" if res["ulp"] is None else "%.1f" % res["ulp"],
        "-" if res["maxdiff"] is None else res["maxdiff"], res["share"]))


@pytest.fixture(scope="module")
def lin_cache():
    return {}


# ---- the format grid on the general march ------------------------------------------------------------------------------

@pytest.mark.parametrize("f", S.format_grid(), ids=S.fmt_id)
def test_format_grid_on_the_row_march(oracle, decoder, lin_cache, f):
    """Stage list (0, 0), 520x264: every transfer function and parameter x sample type x channel count x endianness,
    and the odd bit depths.  The 13 fixed formats among the rows take their own kernels (module docstring)."""
    dec = decoder()
    check(oracle, "march_fixed" if S.is_fixed(f) else "march_general", dec, S.MAIN_SIZE, f, lin_cache)


# ---- every kernel that carries the encoder -----------------------------------------------------------------------------

@pytest.mark.parametrize("gab,epf", STAGE_LISTS + EPF3)
@pytest.mark.parametrize("f", S.GENERAL_LIST, ids=S.fmt_id)
def test_general_march_every_stage_list(oracle, decoder, lin_cache, f, gab, epf):
    dec = decoder()
    check(oracle, "march_general_g%de%d" % (gab, epf), dec, S.KERNEL_SIZE, f, lin_cache, gab=gab, epf=epf)


@pytest.mark.parametrize("gab,epf", STAGE_LISTS + EPF3)
@pytest.mark.parametrize("f", S.FIXED_LIST, ids=S.fmt_id)
def test_fixed_formats_every_stage_list(oracle, decoder, lin_cache, f, gab, epf):
    dec = decoder()
    check(oracle, "march_fixed_g%de%d" % (gab, epf), dec, S.KERNEL_SIZE, f, lin_cache, gab=gab, epf=epf)


@pytest.mark.parametrize("gab,epf", [(0, 0), (1, 1), (0, 3)])
@pytest.mark.parametrize("f", S.GENERAL_LIST + S.STORE_SHAPES[:2], ids=S.fmt_id)
def test_generic_kernel_by_switch(oracle, decoder, lin_cache, f, gab, epf):
    """JXLHIP_FILTERS=generic: k_xyb_only without a loop filter, the LDS kernel k_filters with one; StorePackedPixel."""
    dec = decoder(JXLHIP_FILTERS="generic")
    check(oracle, "generic_g%de%d" % (gab, epf), dec, S.KERNEL_SIZE, f, lin_cache, gab=gab, epf=epf)


@pytest.mark.parametrize("f", S.GENERAL_LIST + S.STORE_SHAPES[:2], ids=S.fmt_id)
def test_generic_kernel_by_size(oracle, decoder, lin_cache, f):
    """13x200: narrower than the march's 16 columns."""
    dec = decoder()
    check(oracle, "generic_13x200", dec, (13, 200), f, lin_cache, gab=1, epf=1)


TAIL_LIST = S.GENERAL_LIST + S.STORE_SHAPES[:2]


@pytest.mark.parametrize("f", TAIL_LIST, ids=S.fmt_id)
def test_noise_tail(oracle, decoder, lin_cache, f):
    """k_noise_emit: the packed and the linear decode draw the same noise (the generators are seeded by position)."""
    dec = decoder()
    variant = S.variant_of(f)
    _, _, lin = check(oracle, "noise", dec, S.KERNEL_SIZE, f, lin_cache, gab=1, epf=1, feature=("noise",))
    key = ("plain", variant)
    if key not in lin_cache:
        lin_cache[key], _ = run(dec, S.KERNEL_SIZE, variant, 1, gab=1, epf=1)
    loud = np.abs(lin_cache[key][..., :2]).max(axis=2) > 8.5  # (the strength follows r and g)
    assert loud.any() and (lin[loud] != lin_cache[key][loud]).mean() > 0.5  # the noise is there


@pytest.mark.parametrize("f", TAIL_LIST, ids=S.fmt_id)
def test_spline_tail(oracle, decoder, lin_cache, f):
    dec = decoder()
    variant = S.variant_of(f)
    _, _, lin = check(oracle, "splines", dec, S.KERNEL_SIZE, f, lin_cache, gab=1, epf=1, feature=("splines",))
    key = ("plain", variant)
    if key not in lin_cache:
        lin_cache[key], _ = run(dec, S.KERNEL_SIZE, variant, 1, gab=1, epf=1)
    assert (lin != lin_cache[key]).mean() > 0.001  # the splines are there


# (coded size, factor, output size): 2x, 4x, 8x to 520x264 and below, and one cropped output
UPS = [((260, 132), 2, (520, 264)), ((130, 66), 4, (520, 264)), ((65, 33), 8, (520, 264)), ((260, 132), 2, (519, 263))]


@pytest.mark.parametrize("coded,n,out_size", UPS)
@pytest.mark.parametrize("f", TAIL_LIST, ids=S.fmt_id)
def test_upsampling_tail(oracle, decoder, lin_cache, f, coded, n, out_size):
    dec = decoder()
    got, _, lin = check(oracle, "upsample%d" % n, dec, coded, f, lin_cache, feature=("ups", n, out_size))
    assert lin.shape[:2] == out_size[::-1] and got.shape[:2] == out_size[::-1]


# ---- undo_orientation ----------------------------------------------------------------------------------------------------

def oriented(img, o):
    """An image in coded orientation -> display orientation (stage_write.cc: flips, then the transposed write)."""
    fx, fy, tr = o in (2, 3, 7, 8), o in (3, 4, 6, 7), o >= 5
    a = img[:, ::-1] if fx else img
    a = a[::-1] if fy else a
    return np.ascontiguousarray(a.swapaxes(0, 1) if tr else a)


@pytest.mark.parametrize("o", range(2, 9))
@pytest.mark.parametrize("f", [S.fmt(abi.TF_SRGB, abi.SAMPLE_U8, 3), S.fmt(abi.TF_SRGB, abi.SAMPLE_U16, 4),
                               S.fmt(abi.TF_709, abi.SAMPLE_U8, 3)], ids=S.fmt_id)
def test_orientation_staging(oracle, decoder, lin_cache, f, o):
    """The kernels write coded orientation into a staging frame and k_orient moves the pixels.  The yardstick is applied
    to the device's linear output in display orientation.  The reference dithers AFTER flipping and BEFORE its
    transposed write (stage_write.cc: OutputBuffers flips, StoreUnsignedRow dithers at the flipped (x, y),
    WriteToOutput transposes), so the dither coordinates are those of the flipped, not yet transposed frame: the
    yardstick packs the display frame with the transposition undone, and is transposed back."""
    def display(fm, lin_disp):
        flipped = np.ascontiguousarray(lin_disp.swapaxes(0, 1)) if o >= 5 else lin_disp
        want = oracle.pack_output(fm, flipped)
        return (np.ascontiguousarray(want.swapaxes(0, 1)) if o >= 5 else want), flipped
    dec = decoder()
    variant = S.variant_of(f)
    xs, ys = S.KERNEL_SIZE
    key = ("orient", o, variant)
    if key not in lin_cache:
        lin_cache[key], _ = run(dec, S.KERNEL_SIZE, variant, 1, gab=1, epf=1, orient=o)
        plain = ("orient", 0, variant)
        if plain not in lin_cache:
            lin_cache[plain], _ = run(dec, S.KERNEL_SIZE, variant, 1, gab=1, epf=1)
        assert np.array_equal(lin_cache[key], oriented(lin_cache[plain], o))
    lin_disp = lin_cache[key]
    assert lin_disp.shape == ((xs, ys, 3) if o >= 5 else (ys, xs, 3))
    got, _ = run(dec, S.KERNEL_SIZE, variant, 2, f=f, gab=1, epf=1, orient=o)
    want, flipped = display(f, lin_disp)
    assert S.population_problems(f, flipped, variant) == []
    report("orient%d" % o, f, S.compare(f, got, want, lin_disp))


# ---- edges ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width", [261, 262, 263, 264, 16])
@pytest.mark.parametrize("f", S.STORE_SHAPES, ids=S.fmt_id)
def test_widths(oracle, decoder, lin_cache, f, width):
    """Odd widths for the pair stores, width mod 4 for the DPP RGB8 store, and the narrowest march; stage list (1, 1)."""
    dec = decoder()
    check(oracle, "march_w%d" % width, dec, (width, 264 if width == 16 else 136), f, lin_cache, gab=1, epf=1)


PADS = [(f, 4) for f in S.STORE_SHAPES] + [(S.STORE_SHAPES[0], 1), (S.fmt(abi.TF_709, abi.SAMPLE_U8, 3, bits=7), 1)]


@pytest.mark.parametrize("width", [264, 261])
@pytest.mark.parametrize("f,pad", PADS, ids=lambda v: S.fmt_id(v) if isinstance(v, dict) else "pad%d" % v)
def test_padded_row_stride(oracle, decoder, lin_cache, f, pad, width):
    """A row stride larger than the row: every padding byte keeps the sentinel, every row is where the stride puts it."""
    dec = decoder()
    size, variant = (width, 136), S.variant_of(f)
    key = (size, variant, (("epf", 1), ("gab", 1)), id(dec))
    if key not in lin_cache:
        lin_cache[key], _ = run(dec, size, variant, 1, gab=1, epf=1)
    lin = lin_cache[key]
    raw, _ = run(dec, size, variant, 2, f=f, gab=1, epf=1, pad=pad)
    got, row_bytes = S.rows_of(f, raw, width)
    S.check_padding(raw, row_bytes, SENTINEL)
    report("march_pad%d_w%d" % (pad, width), f, S.compare(f, got, oracle.pack_output(f, lin), lin))
