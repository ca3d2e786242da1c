"""Shared by the partial-file tests (test_partial_front_end.py, test_gpu_partial.py): the oracle streams they cut, their
sections as the product's own header parsers see them, and the reference's flushed picture for the first bytes of a
file -- JxlDecoderFlushImage on JXL_DEC_NEED_MORE_INPUT, the input left open (FrameDecoder::Flush, dec_frame.cc:737-797).
Test infrastructure."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from libjxl_amd import abi

import test_seam

# (feature, xsize, ysize): the multi-section streams, and the one-section stream that never flushes early
STREAMS = [("plain", 600, 400), ("progressive", 600, 400), ("plain", 2200, 520)]
ONE_SECTION = ("plain", 200, 13)
SENTINEL = np.float32(-7.0)  # what an untouched sample of a flushed picture would still hold


def load_reference():
    """(test_seam, libjxl_dec_ref.so with JxlDecoderFlushImage declared); skips only where the reference libraries are
    neither present nor buildable."""
    sys.path.insert(0, os.path.join(test_seam.ROOT, "integration"))
    import build_seam
    prebuilt = [os.path.join(build_seam.B.OUT, n) for n in ("libjxl_dec_ref.so", "libjxl_dec_hip.so")]
    if not build_seam.available() and not all(os.path.exists(p) for p in prebuilt):
        pytest.skip("reference tree not present and no prebuilt seam libraries")
    ref_so, _ = build_seam.build()  # (a compile or link failure fails the tests: it must not skip them)
    RL = test_seam.load(ref_so)
    RL.JxlDecoderFlushImage.argtypes = [C.c_void_p]
    RL.JxlDecoderFlushImage.restype = C.c_int
    return test_seam, RL


def stream(oracle, key):
    feature, xs, ys = key
    return oracle.feature_stream(feature, xsize=xs, ysize=ys, seed=5, distance=1.0)


class Sections:
    """The one frame of a plain file as the product's parsers see it: base = the first byte behind the TOC, off / size =
    every section in TOC order (DC global, the DC groups, AC global, then pass by pass the AC groups)."""

    def __init__(self, L, cs):
        a = np.frombuffer(cs, np.uint8)
        base, n = a.ctypes.data, len(a)
        ih, pos = abi.ImageHeader(), C.c_size_t(0)
        assert L.jxlhip_image_header_decode(base, n, C.byref(pos), None, 0, C.byref(ih)) == 0
        info = abi.ImageInfo(ih.xsize, ih.ysize, ih.xyb_encoded, 0, None, 0, 0, 0, ih.bit_depth.bits_per_sample)
        self.fh = fh = abi.FrameHeader()
        assert L.jxlhip_frame_header_decode(base, n, C.byref(pos), C.byref(info), C.byref(fh)) == 0
        assert fh.is_last
        nt = int(fh.num_toc_entries)
        off, sz, total = np.zeros(nt, np.uint64), np.zeros(nt, np.uint32), C.c_uint64(0)
        assert L.jxlhip_toc_decode(base, n, C.byref(pos), nt, off.ctypes.data, sz.ctypes.data, C.byref(total)) == 0
        self.base = pos.value // 8
        assert self.base + total.value == n  # the file ends with its frame
        self.off, self.size = [int(o) for o in off], [int(s) for s in sz]
        self.ng, self.ndc, self.np = int(fh.num_groups), int(fh.num_dc_groups), int(fh.num_passes)
        assert nt == 1 or nt == 2 + self.ndc + self.np * self.ng

    def end(self, i):
        return self.base + self.off[i] + self.size[i]

    def boundaries(self):
        return sorted({self.end(i) for i in range(len(self.off))})

    def ac(self, p, g):
        return 2 + self.ndc + p * self.ng + g

    def expect(self, n):
        """None where nothing can be drawn from the first n bytes, else (complete, groups_complete, groups_partial,
        groups_dc_only, have_ac_global, bytes_used): the rules of the reference, from the TOC alone."""
        last = max(self.end(i) for i in range(len(self.off)))
        if n >= last:
            return (1, self.ng, 0, 0, 1, last)
        if len(self.off) == 1 or any(self.end(i) > n for i in range(1 + self.ndc)):
            return None
        used = max(self.end(i) for i in range(1 + self.ndc))
        ag = self.end(1 + self.ndc) <= n
        if ag:
            used = max(used, self.end(1 + self.ndc))
        counts = [0, 0, 0]
        for g in range(self.ng):
            k = 0
            while ag and k < self.np and self.end(self.ac(k, g)) <= n:
                used = max(used, self.end(self.ac(k, g)))
                k += 1
            counts[0 if k == self.np else 1 if k else 2] += 1
        return (0, counts[0], counts[1], counts[2], int(ag), used)


def partial_info(L, cs, n):
    """(rc, the fields Sections.expect returns) of jxlhip_codestream_partial_info on the first n bytes."""
    pi = abi.PartialInfo()
    rc = L.jxlhip_codestream_partial_info(cs, n, None, C.byref(pi))
    return rc, (pi.complete, pi.groups_complete, pi.groups_partial, pi.groups_dc_only, pi.have_ac_global, pi.bytes_used)


def flush(ts, RL, data, want_pixels=True):
    """The reference on the first bytes of a file, the input left open.  Returns (flushed, picture): flushed = False
    where JxlDecoderFlushImage answers JXL_DEC_ERROR (or no output buffer was asked for yet); picture = float32
    [H, W, 3], samples nothing wrote still SENTINEL."""
    dec = RL.JxlDecoderCreate(None)
    assert dec
    try:
        assert RL.JxlDecoderSubscribeEvents(dec, ts.JXL_DEC_BASIC_INFO | ts.JXL_DEC_FULL_IMAGE) == ts.JXL_DEC_SUCCESS
        assert RL.JxlDecoderSetInput(dec, data, len(data)) == ts.JXL_DEC_SUCCESS
        fmt = ts.PixelFormat(3, 0, 0, 0)  # JXL_TYPE_FLOAT, JXL_NATIVE_ENDIAN
        out, w = None, 0
        while True:
            st = RL.JxlDecoderProcessInput(dec)
            if st == ts.JXL_DEC_BASIC_INFO:
                info = (C.c_uint8 * 1024)()
                assert RL.JxlDecoderGetBasicInfo(dec, info) == ts.JXL_DEC_SUCCESS
                w = int(np.frombuffer(bytes(info[4:12]), np.uint32)[0])
            elif st == ts.JXL_DEC_NEED_IMAGE_OUT_BUFFER:
                n = C.c_size_t(0)
                assert RL.JxlDecoderImageOutBufferSize(dec, C.byref(fmt), C.byref(n)) == ts.JXL_DEC_SUCCESS
                out = np.full((n.value // (w * 12), w, 3), SENTINEL, np.float32)
                assert RL.JxlDecoderSetImageOutBuffer(dec, C.byref(fmt), out.ctypes.data, n.value) == ts.JXL_DEC_SUCCESS
            elif st == ts.JXL_DEC_FULL_IMAGE:
                continue
            elif st == ts.JXL_DEC_SUCCESS:
                return True, out
            elif st == ts.JXL_DEC_NEED_MORE_INPUT:
                if out is None:
                    return False, None
                return RL.JxlDecoderFlushImage(dec) == ts.JXL_DEC_SUCCESS, out
            else:
                raise AssertionError(f"JxlDecoderProcessInput -> {st}")
    finally:
        RL.JxlDecoderDestroy(dec)
