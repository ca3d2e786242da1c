"""Shared by the CPU tiers that hold a render stage's numpy model to the reference (test_render_stage_streams.py): a
one-frame VarDCT file through the product's host parsers and entropy decoder into the C oracle, up to planar XYB behind
the loop filters at CODED size -- the chain of tests/test_patches_front_end.py's _filtered_xyb without the patch
dictionary, for files of one section (everything back to back, bit positions carried on) and of several -- and the
oracle's colour conversion and output packing for planes of any size.  No device.  Test infrastructure."""
import ctypes as C
import os

import numpy as np

from libjxl_amd import abi

FLAG_NOISE = 1
F32 = np.float32

# ---- the streams that take the upsampling and the noise stage beyond what the reference encoder chooses by itself
# (oracle.feature_stream's knobs).  name -> keyword arguments; every one is a "plain" frame, seed 5.
# Upsampling: N = 4 and 8 with the default and with custom tables, N = 2 custom, N = 4 custom cropped by 3 columns and
# 1 row; coded frames of two groups and more (several sections), and the two small ones of one section.
CUSTOM_SEED = 3
UPSAMPLING_STREAMS = {
    "n4": dict(xsize=1100, ysize=300, distance=2.0, resampling=4),
    "n8": dict(xsize=2200, ysize=300, distance=2.0, resampling=8),
    "n4_custom": dict(xsize=1100, ysize=300, distance=2.0, resampling=4, custom_weights_seed=CUSTOM_SEED),
    "n8_custom": dict(xsize=2195, ysize=297, distance=2.0, resampling=8, custom_weights_seed=CUSTOM_SEED),
    "n2_custom": dict(xsize=601, ysize=277, distance=2.0, resampling=2, custom_weights_seed=CUSTOM_SEED),
    "n4_custom_crop": dict(xsize=1097, ysize=299, distance=2.0, resampling=4, custom_weights_seed=CUSTOM_SEED),
    "n4_small": dict(xsize=333, ysize=277, distance=2.0, resampling=4),
    "n8_small": dict(xsize=333, ysize=277, distance=2.0, resampling=8),
}
# Noise: a LUT that is not monotone and has a zero entry (multiples of 1/1024 once coded); the in-gamut original keeps
# (y +- x) / 2 * 6 below 3, the original multiplied by 30 fills the intervals above and the branch at 7 and beyond.
# Its amplitude (0.7 times 0.45, 0.05, 0.4, 0, 0.5, 0.15, 0.35, 0.1) is the largest tried at which the CPU chain with
# XybToRgb in float64 stays within 1e-5 of JxlDecoder on the in-gamut streams, half their bar (8.9e-6 and 9.1e-6; at
# 0.8 times 1.14e-5, at 1.0 times 1.08e-5): strong noise makes dark, saturated samples whose conversion is badly
# conditioned (a cube, coefficients of 11 and -9.9 that cancel, the sRGB slope of 12.92), where one ulp of a plane is
# 1e-5 of the range in the output.
NOISE_LUT = [0.315, 0.035, 0.28, 0.0, 0.35, 0.105, 0.245, 0.07]
BRIGHT_GAIN = 30.0
NOISE_STREAMS = {
    "noise": dict(xsize=333, ysize=277, distance=1.0, noise_lut=NOISE_LUT),
    "noise_n4": dict(xsize=1100, ysize=300, distance=1.0, noise_lut=NOISE_LUT, resampling=4),
    "bright": dict(xsize=333, ysize=277, distance=1.0, noise_lut=NOISE_LUT, gain=BRIGHT_GAIN),
    "bright_n2": dict(xsize=601, ysize=277, distance=1.0, noise_lut=NOISE_LUT, gain=BRIGHT_GAIN, resampling=2),
}
BRIGHT_NO_NOISE = dict(xsize=333, ysize=277, distance=1.0, gain=BRIGHT_GAIN)  # (measured only: the bright bar)
TIGHT = 2e-5
# The bright streams' bar, as a fraction of their range of about 4.1: the float32 cube of XybToRgb on values that large
# dominates, with noise or without.  Twice the larger of the CPU chain's two errors against JxlDecoder with that
# conversion evaluated in float64, 2.473e-05 without noise and 4.302e-05 with it (test_render_stage_streams.py::
# test_bright_bar measures them again and holds this to them); the GPU tier uses it too.
BRIGHT_BAR = 8.7e-5


# a file that is NOT upsampled but carries the custom tables: its own 8x table draws the DC-only groups of a cut file
PARTIAL_CUSTOM = dict(xsize=600, ysize=400, distance=1.0, custom_weights_seed=CUSTOM_SEED)
ALL_STREAMS = dict(UPSAMPLING_STREAMS, **NOISE_STREAMS, bright_no_noise=BRIGHT_NO_NOISE, partial_custom=PARTIAL_CUSTOM)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_stage_streams")


def stream(oracle, kw):
    """The stream from the reference encoder (needs a reference library built with the knobs)."""
    return oracle.feature_stream("plain", seed=5, **kw)


def golden_stream(name):
    """The same stream as committed under tests/golden/render_stage_streams: what the GPU tier decodes, so that it
    needs the reference's decoder only.  test_render_stage_streams.py holds every file to what stream() writes."""
    with open(os.path.join(GOLDEN, name + ".jxl"), "rb") as f:
        return f.read()


class Chain:
    """ih, fh, dcg: the product's image header, frame header and DC-global fields; xyb: [3, ch, cw] float32 behind
    the loop filters; lut: the 8 noise points jxlhip_noise_lut_decode read (None without FrameHeader::kNoise);
    params: the oracle's frame parameters (opsin biases, inverse matrix)."""

    def upsampling_weights(self):
        """The coded table of the frame's factor as jxlhip_image_header_decode read it, or None for the defaults."""
        n = int(self.fh.upsampling)
        if n == 1 or not (self.ih.custom_weights_mask & {2: 1, 4: 2, 8: 4}[n]):
            return None
        return np.array(list({2: self.ih.upsampling2_weights, 4: self.ih.upsampling4_weights,
                              8: self.ih.upsampling8_weights}[n]), F32)


def filtered_xyb(L, cs):
    import oracle as O
    cs = np.frombuffer(cs, np.uint8)
    base, n = cs.ctypes.data, len(cs)
    ih, pos = abi.ImageHeader(), C.c_size_t(0)
    assert L.jxlhip_image_header_decode(base, n, C.byref(pos), None, 0, C.byref(ih)) == 0
    info = abi.ImageInfo(ih.xsize, ih.ysize, ih.xyb_encoded, 0, None, 0, 0, 0, ih.bit_depth.bits_per_sample)
    fh = abi.FrameHeader()
    assert L.jxlhip_frame_header_decode(base, n, C.byref(pos), C.byref(info), C.byref(fh)) == 0
    assert fh.is_last and not fh.is_modular
    nt = int(fh.num_toc_entries)
    off, sz, total = np.zeros(nt, np.uint64), np.zeros(nt, np.uint32), C.c_uint64(0)
    assert L.jxlhip_toc_decode(base, n, C.byref(pos), nt, off.ctypes.data, sz.ctypes.data, C.byref(total)) == 0
    start = pos.value // 8
    assert start + total.value == n  # the file ends with its frame
    sections = [cs[start + int(o): start + int(o) + int(s)].copy() for o, s in zip(off, sz)]
    xsb, ysb, ng, ndc, npass = fh.xsize_blocks, fh.ysize_blocks, int(fh.num_groups), int(fh.num_dc_groups), int(fh.num_passes)
    single = nt == 1
    assert single or nt == 2 + ndc + npass * ng
    assert ndc == 1  # (one DC group: its extra_precision is the frame's)
    s0 = sections[0]
    lut = None
    if fh.flags & FLAG_NOISE:
        lut, lpos = (C.c_float * 8)(), C.c_size_t(0)
        assert L.jxlhip_noise_lut_decode(s0.ctypes.data, len(s0), C.byref(lpos), lut) == 0 and lpos.value == 80
        lut = [float(v) for v in lut]
    dcg, spos = abi.DcGlobal(), C.c_size_t(0)
    assert L.jxlhip_dc_global_decode(s0.ctypes.data, len(s0), C.byref(spos), fh.flags, C.byref(dcg)) == 0
    tree = C.c_void_p()
    assert L.jxlhip_modular_global_decode(s0.ctypes.data, len(s0), C.byref(spos), C.byref(fh), C.byref(tree)) == 0
    qdc = [np.zeros(xsb * ysb, np.int32) for _ in range(3)]
    acs, rq, sharp = np.zeros(xsb * ysb, np.uint8), np.zeros(xsb * ysb, np.int32), np.zeros(xsb * ysb, np.uint8)
    cw, chh = (xsb + 7) // 8, (ysb + 7) // 8
    ytox, ytob = np.zeros(cw * chh, np.int8), np.zeros(cw * chh, np.int8)
    used, ep = C.c_uint32(0), C.c_uint32(0)
    try:
        d = s0 if single else sections[1]
        gp = spos if single else C.c_size_t(0)
        ptrs = (C.c_void_p * 3)(*[q.ctypes.data for q in qdc])
        assert L.jxlhip_dc_group_decode(tree, d.ctypes.data, len(d), C.byref(gp), C.byref(fh), 0, ptrs, C.byref(ep),
                                        acs.ctypes.data, rq.ctypes.data, sharp.ctypes.data, ytox.ctypes.data,
                                        ytob.ctypes.data, C.byref(used)) == 0
    finally:
        L.jxlhip_modular_tree_destroy(tree)
    qctx = np.zeros(xsb * ysb, np.uint8)
    qp = (C.c_void_p * 3)(*[q.ctypes.data for q in qdc])
    assert L.jxlhip_quant_dc_contexts(C.byref(dcg.block_ctx_map), xsb * ysb, qp, qctx.ctypes.data) == 0
    inv_quant_dc = (F32(65536.0) / F32(dcg.global_scale)) / F32(dcg.quant_dc)
    mul_dc = [F32(inv_quant_dc * F32(dcg.dc_quant[c])) for c in range(3)]
    scale = F32(1.0) / F32(dcg.cfl_color_factor)
    dc = O.ref_dequant_dc([q.reshape(ysb, xsb) for q in qdc], mul_dc,
                          float(F32(dcg.cfl_base_x) + F32(dcg.ytox_dc) * scale),
                          float(F32(dcg.cfl_base_b) + F32(dcg.ytob_dc) * scale),
                          not (fh.flags & 128), mul=float(F32(1.0) / F32(1 << ep.value)))
    encs, nh, bits, hs = abi.QuantEncodings(), C.c_uint32(0), C.c_size_t(0), (C.c_void_p * npass)()
    if single:
        assert L.jxlhip_ac_global_decode_at(s0.ctypes.data, len(s0), C.byref(spos), ng, npass, used.value,
                                            C.byref(dcg.block_ctx_map), C.byref(encs), C.byref(nh), hs) == 0
    else:
        glob = sections[1 + ndc]
        assert L.jxlhip_ac_global_decode(glob.ctypes.data, len(glob), ng, npass, used.value, C.byref(dcg.block_ctx_map),
                                         C.byref(encs), C.byref(nh), hs, C.byref(bits)) == 0
    coeffs = [np.zeros(ng * 65536, np.int32) for _ in range(3)]
    try:
        xsg = int(fh.xsize_groups)
        for g in range(ng):
            ptrs = (C.c_void_p * 3)(*[o[g * 65536:].ctypes.data for o in coeffs])
            for ps in range(npass):
                d = s0 if single else sections[2 + ndc + ps * ng + g]
                gp, cnt = (spos if single else C.c_size_t(0)), C.c_size_t(0)
                assert L.jxlhip_ac_group_decode(hs[ps], xsb, ysb, g % xsg, g // xsg, acs.ctypes.data, rq.ctypes.data,
                                                qctx.ctypes.data, d.ctypes.data, len(d), C.byref(gp), fh.shift[ps], 1,
                                                ptrs, C.byref(cnt)) == 0
    finally:
        for hh in hs:
            L.jxlhip_ac_pass_destroy(hh)
    p = O.FrameParams()
    p.xsize, p.ysize, p.coeff_type, p.output_kind = fh.xsize, fh.ysize, 1, 0  # planar XYB behind the loop filters
    p.global_scale, p.quant_dc = dcg.global_scale, dcg.quant_dc
    p.x_dm_multiplier, p.b_dm_multiplier = fh.x_dm_multiplier, fh.b_dm_multiplier
    p.quant_biases[:] = ih.quant_biases[:]
    p.cfl_base_x, p.cfl_base_b, p.cfl_color_factor = dcg.cfl_base_x, dcg.cfl_base_b, dcg.cfl_color_factor
    C.memmove(C.byref(p.lf), C.byref(fh.lf), C.sizeof(fh.lf))
    p.opsin_biases[:] = ih.opsin_biases[:]
    s = F32(255.0) / F32(ih.intensity_target)
    p.inverse_opsin_matrix[:] = [float(F32(v) * s) for v in ih.inverse_opsin_matrix]
    p.used_acs = used.value
    table = O.dequant_tables(encs)
    assert table is not None
    fr = O.Frame(p, coeffs, acs, rq, sharp, ytox, ytob, [np.ascontiguousarray(d) for d in dc], table)
    out = Chain()
    out.ih, out.fh, out.dcg, out.lut, out.params = ih, fh, dcg, lut, p
    out.xyb = np.asarray(fr.decode(threads=4))
    assert out.xyb.shape == (3, fh.ysize, fh.xsize)
    out.xyb.setflags(write=False)
    return out


def srgb_exact(chain, planes):
    """The same conversion with XybToRgb (dec_xyb-inl.h:38-86) evaluated in float64 on the float32 planes, rounded to
    float32 once: against JxlDecoder it measures the float32 rounding of the reference's own cube and dot product --
    the error any correct float32 implementation with another order of operations may show."""
    import oracle as O
    x, y, b = [np.asarray(planes[c], np.float64) for c in range(3)]
    bias = np.array(list(chain.params.opsin_biases)[:3], F32)
    cb = np.cbrt(bias).astype(F32).astype(np.float64)
    mixed = [(y + x - cb[0]) ** 3 + float(bias[0]), (y - x - cb[1]) ** 3 + float(bias[1]), (b - cb[2]) ** 3 + float(bias[2])]
    m = np.array(list(chain.params.inverse_opsin_matrix), F32).astype(np.float64).reshape(3, 3)
    lin = np.stack([m[r, 0] * mixed[0] + m[r, 1] * mixed[1] + m[r, 2] * mixed[2] for r in range(3)], axis=-1)
    return O.pack_output(dict(transfer=abi.TF_SRGB, sample_type=abi.SAMPLE_F32, num_channels=3, bits_per_sample=32),
                         np.ascontiguousarray(lin, F32))


def srgb(chain, planes):
    """The oracle's XybToRgb (oracle/filters.c) and its sRGB float output (oracle/output.c) of planar XYB [3, H, W] of
    any size under the chain's opsin parameters -> [H, W, 3] float32, what JxlDecoder gives for these files."""
    import oracle as O
    planes = [np.ascontiguousarray(planes[c], F32) for c in range(3)]
    h, w = planes[0].shape
    f = O.OracleFrame()
    f.p = chain.params
    f.p.xsize, f.p.ysize = w, h
    rgb = np.zeros((h, w, 3), F32)
    ptrs = (C.c_void_p * 3)(*[a.ctypes.data for a in planes])
    O.lib().jxo_xyb_to_linear_rgb(C.byref(f), ptrs, w, rgb.ctypes.data_as(C.c_void_p), w * 3, 0, h)
    return O.pack_output(dict(transfer=abi.TF_SRGB, sample_type=abi.SAMPLE_F32, num_channels=3, bits_per_sample=32), rgb)
