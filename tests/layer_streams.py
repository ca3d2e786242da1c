"""Frame sequences for the tests of jxlhip_codestream_sequence_info / jxlhip_decode_codestream_next, and the truth for
them: the reference's public JxlDecoder on the same bytes.

  jxl_decode_frames   the event loop of tests/test_seam.jxl_decode that keeps EVERY JXL_DEC_FULL_IMAGE (the coalesced
                      frames, as float in the original's encoding) and reads JxlDecoderGetFrameHeader for each
  splice              frames of oracle streams behind the image header of another oracle stream, each with a rewritten
                      frame header (crop, blending info, duration, is_last, save_as_reference): the blended, cropped and
                      layered files no encoder entry point of the oracle writes
"""
import ctypes as C

import numpy as np

import test_seam as ts

JXL_DEC_FRAME = 0x400


class BlendInfo(C.Structure):
    _fields_ = [("blendmode", C.c_int), ("source", C.c_uint32), ("alpha", C.c_uint32), ("clamp", C.c_int)]


class LayerInfo(C.Structure):
    _fields_ = [("have_crop", C.c_int), ("crop_x0", C.c_int32), ("crop_y0", C.c_int32), ("xsize", C.c_uint32),
                ("ysize", C.c_uint32), ("blend_info", BlendInfo), ("save_as_reference", C.c_uint32)]


class FrameHeader(C.Structure):
    """JxlFrameHeader (include/jxl/codestream_header.h)"""
    _fields_ = [("duration", C.c_uint32), ("timecode", C.c_uint32), ("name_length", C.c_uint32), ("is_last", C.c_int),
                ("layer_info", LayerInfo)]


def jxl_decode_frames(L, data, channels=3):
    """[(pixels [H, W, channels] float32, dict of JxlFrameHeader's fields)] for every frame the coalescing JxlDecoder
    reports.  Raises AssertionError when the decoder fails: the reference does not accept the bytes."""
    L.JxlDecoderGetFrameHeader.argtypes = [C.c_void_p, C.POINTER(FrameHeader)]
    dec = L.JxlDecoderCreate(None)
    assert dec
    frames = []
    try:
        assert L.JxlDecoderSubscribeEvents(dec, ts.JXL_DEC_BASIC_INFO | JXL_DEC_FRAME | ts.JXL_DEC_FULL_IMAGE) == ts.JXL_DEC_SUCCESS
        assert L.JxlDecoderSetInput(dec, data, len(data)) == ts.JXL_DEC_SUCCESS
        L.JxlDecoderCloseInput(dec)
        fmt = ts.PixelFormat(channels, 0, 0, 0)  # JXL_TYPE_FLOAT, JXL_NATIVE_ENDIAN
        out, head, w = None, None, 0
        while True:
            st = L.JxlDecoderProcessInput(dec)
            if st == ts.JXL_DEC_BASIC_INFO:
                info = (C.c_uint8 * 1024)()
                assert L.JxlDecoderGetBasicInfo(dec, info) == ts.JXL_DEC_SUCCESS
                w = int(np.frombuffer(bytes(info[4:12]), np.uint32)[0])
            elif st == JXL_DEC_FRAME:
                fh = FrameHeader()
                assert L.JxlDecoderGetFrameHeader(dec, C.byref(fh)) == ts.JXL_DEC_SUCCESS
                head = dict(duration=fh.duration, timecode=fh.timecode, name_length=fh.name_length, is_last=int(fh.is_last != 0),
                            xsize=fh.layer_info.xsize, ysize=fh.layer_info.ysize)
            elif st == ts.JXL_DEC_NEED_IMAGE_OUT_BUFFER:
                n = C.c_size_t(0)
                assert L.JxlDecoderImageOutBufferSize(dec, C.byref(fmt), C.byref(n)) == ts.JXL_DEC_SUCCESS
                out = np.zeros((n.value // (w * channels * 4), w, channels), np.float32)
                assert L.JxlDecoderSetImageOutBuffer(dec, C.byref(fmt), out.ctypes.data, n.value) == ts.JXL_DEC_SUCCESS
            elif st == ts.JXL_DEC_FULL_IMAGE:
                frames.append((out, head))
                out = None
            elif st == ts.JXL_DEC_SUCCESS:
                break
            else:
                raise AssertionError(f"JxlDecoderProcessInput -> {st}")
        return frames
    finally:
        L.JxlDecoderDestroy(dec)


# ---- splicing ---------------------------------------------------------------------------------------------------------

class _Bits:
    """LSB-first bit reader over bytes (BitReader)."""

    def __init__(self, data, pos):
        self.d, self.pos = data, pos

    def bits(self, n):
        v = 0
        for i in range(n):
            v |= ((self.d[self.pos >> 3] >> (self.pos & 7)) & 1) << i
            self.pos += 1
        return v

    def u32(self, *enc):
        """enc: four (bits, offset) pairs; Val(v) = (0, v)."""
        b, o = enc[self.bits(2)]
        return o + self.bits(b)

    def u64(self):
        sel = self.bits(2)
        if sel == 0:
            return 0
        if sel == 1:
            return 1 + self.bits(4)
        if sel == 2:
            return 17 + self.bits(8)
        v, shift = self.bits(12), 12
        while self.bits(1):
            if shift == 60:
                v |= self.bits(4) << shift
                break
            v |= self.bits(8) << shift
            shift += 8
        return v


class _Writer:
    def __init__(self):
        self.b = []

    def bits(self, n, v):
        assert 0 <= v < (1 << n) or n == 0, (n, v)
        self.b += [(v >> i) & 1 for i in range(n)]

    def u32(self, v, *enc):
        for sel, (b, o) in enumerate(enc):
            if o <= v < o + (1 << b):
                self.bits(2, sel)
                self.bits(b, v - o)
                return
        raise ValueError(v)

    def copy(self, data, a, b):
        self.b += [(data[i >> 3] >> (i & 7)) & 1 for i in range(a, b)]

    def to_bytes(self):
        bits = self.b + [0] * (-len(self.b) % 8)
        return bytes(sum(bits[i + k] << k for k in range(8)) for i in range(0, len(bits), 8))


def _val(*vs):
    return tuple((0, v) for v in vs)


_ORIGIN = ((8, 0), (11, 256), (14, 2304), (30, 18688))
_MODE = ((0, 0), (0, 1), (0, 2), (2, 3))
_DURATION = ((0, 0), (0, 1), (8, 0), (32, 0))
_TOC = ((10, 0), (14, 1024), (22, 17408), (30, 4211712))
REPLACE, ADD, BLEND, ALPHA_WEIGHTED_ADD, MUL = range(5)


def _pack_signed(v):
    return 2 * v if v >= 0 else -2 * v - 1


def _unpack_signed(u):
    return (u >> 1) if not u & 1 else -((u + 1) >> 1)


_ALPHA = ((0, 0), (0, 1), (0, 2), (3, 3))


def _read_blending(r, num_ec, partial):
    """BlendingInfo (frame_header.cc:65-93)"""
    b = dict(mode=r.u32(*_MODE), alpha_channel=0, clamp=0, source=0)
    if num_ec > 0 and b["mode"] in (BLEND, ALPHA_WEIGHTED_ADD):
        b["alpha_channel"] = r.u32(*_ALPHA)
        b["clamp"] = r.bits(1)
    elif b["mode"] == MUL:
        b["clamp"] = r.bits(1)
    if b["mode"] != REPLACE or partial:
        b["source"] = r.u32(*_val(0, 1, 2, 3))
    return b


def _write_blending(w, num_ec, partial, mode, clamp=0, source=0, alpha_channel=0):
    w.u32(mode, *_MODE)
    if num_ec > 0 and mode in (BLEND, ALPHA_WEIGHTED_ADD):
        w.u32(alpha_channel, *_ALPHA)
        w.bits(1, int(clamp))
    elif mode == MUL:
        w.bits(1, int(clamp))
    if mode != REPLACE or partial:
        w.u32(source, *_val(0, 1, 2, 3))


def _tail_fields(r, image_size, have_animation, num_ec=0):
    """Reads custom_size_or_origin .. save_before_color_transform of a regular frame (frame_header.cc:320-425): the
    reader ends on the first bit of the name."""
    out = dict(crop=None, size=image_size, mode=0, clamp=0, source=0, duration=0, is_last=1, save_as_reference=0)
    partial = False
    if r.bits(1):
        x0, y0 = _unpack_signed(r.u32(*_ORIGIN)), _unpack_signed(r.u32(*_ORIGIN))
        xs, ys = r.u32(*_ORIGIN), r.u32(*_ORIGIN)
        out.update(crop=(x0, y0), size=(xs, ys))
        partial = x0 > 0 or y0 > 0 or xs + x0 < image_size[0] or ys + y0 < image_size[1]
    b = _read_blending(r, num_ec, partial)
    out.update(mode=b["mode"], clamp=b["clamp"], source=b["source"])
    out["ec"] = [_read_blending(r, num_ec, partial) for _ in range(num_ec)]
    if have_animation:
        out["duration"] = r.u32(*_DURATION)
    out["is_last"] = r.bits(1)
    if not out["is_last"]:
        out["save_as_reference"] = r.u32(*_val(0, 1, 2, 3))
    can = not out["is_last"] and (out["duration"] == 0 or out["save_as_reference"] != 0)
    if can and out["mode"] == REPLACE and not partial:
        out["save_before_color_transform"] = r.bits(1)
    return out


def read_fields(L, cs):
    """The rewritable fields of every frame of a file whose frames are regular VarDCT frames, through this module's own
    reader: what splice() wrote must read back."""
    from libjxl_amd import abi
    ih, pos = abi.ImageHeader(), C.c_size_t(0)
    assert L.jxlhip_image_header_decode(cs, len(cs), C.byref(pos), None, 0, C.byref(ih)) == 0
    out = []
    while True:
        r = _Bits(cs, pos.value)
        _head(r, ih.num_extra_channels)
        out.append(_tail_fields(r, (ih.xsize, ih.ysize), ih.have_animation, ih.num_extra_channels))
        pos = C.c_size_t(_frame_end(L, cs, pos.value, ih)[2])
        if out[-1]["is_last"]:
            return out


def _head(r, num_ec=0):
    """all_default .. passes of a regular VarDCT XYB frame (frame_header.cc:216-308); returns the bit positions the
    rewriter cuts at and the flags."""
    assert r.bits(1) == 0, "all_default frame header"
    assert r.bits(2) == 0 and r.bits(1) == 0, "not a regular VarDCT frame"
    p = dict(flags_at=r.pos)
    p["flags"] = r.u64()
    assert not p["flags"] & 32, "kUseDcFrame"
    p["upsampling_at"] = r.pos
    for _ in range(1 + num_ec):
        r.u32(*_val(1, 2, 4, 8))  # upsampling, extra_channel_upsampling
    p["qm_at"] = r.pos
    r.bits(6)  # x_qm_scale, b_qm_scale
    p["passes_at"] = r.pos
    num_passes = r.u32((0, 1), (0, 2), (0, 3), (3, 4))
    if num_passes != 1:
        nds = r.u32((0, 0), (0, 1), (0, 2), (1, 3))
        r.bits(2 * (num_passes - 1))
        for _ in range(nds):
            r.u32(*_val(1, 2, 4, 8))
        for _ in range(nds):
            r.u32((0, 0), (0, 1), (0, 2), (3, 0))
    return p


def _frame_end(L, cs, frame_bit, ih):
    """(first bit of the TOC, first byte of the sections, first bit behind the frame) of the frame at frame_bit."""
    from libjxl_amd import abi
    info = abi.ImageInfo(ih.xsize, ih.ysize, ih.xyb_encoded, ih.num_extra_channels, None, ih.have_animation, ih.have_timecodes,
                         0, ih.bit_depth.bits_per_sample)
    fh, pos = abi.FrameHeader(), C.c_size_t(frame_bit)
    assert L.jxlhip_frame_header_decode(cs, len(cs), C.byref(pos), C.byref(info), C.byref(fh)) == 0
    toc = pos.value
    nt = int(fh.num_toc_entries)
    off, sz, total = np.zeros(nt, np.uint64), np.zeros(nt, np.uint32), C.c_uint64(0)
    assert L.jxlhip_toc_decode(cs, len(cs), C.byref(pos), nt, off.ctypes.data, sz.ctypes.data, C.byref(total)) == 0
    assert pos.value % 8 == 0
    return toc, pos.value // 8, (pos.value // 8 + total.value) * 8, nt


def source_frame(L, cs, which=-1):
    """(cs, first bit of frame `which` of the file -- -1: its last --, its image header)."""
    from libjxl_amd import abi
    ih, pos = abi.ImageHeader(), C.c_size_t(0)
    assert L.jxlhip_image_header_decode(cs, len(cs), C.byref(pos), None, 0, C.byref(ih)) == 0
    assert pos.value % 8 == 0 and not ih.color_encoding.want_icc
    starts = []
    at = pos.value
    while at < len(cs) * 8:
        starts.append(at)
        at = _frame_end(L, cs, at, ih)[2]
    return cs, starts[which], ih


def splice(L, header_stream, frames):
    """The image header of header_stream, then one frame per entry of `frames`: dict(stream=bytes of an oracle stream
    whose last frame is taken (which=k: its frame k), crop=(x0, y0) or None = a full frame at the origin, mode, clamp,
    source, duration, is_last, save_as_reference; frame_type / modular / flags_or / ec_mode for the files the walk refuses).  Everything in front of the rewritten fields (up to and including the
    passes) and behind them (name, loop filter, extensions) is copied bit for bit, then the TOC's flag, padded to a byte,
    then the TOC's entries and the sections as bytes."""
    _, first, ih = source_frame(L, header_stream, 0)
    out = bytearray(header_stream[:first // 8])
    W, H, nec = ih.xsize, ih.ysize, ih.num_extra_channels
    for k, f in enumerate(frames):
        cs, at, sih = source_frame(L, f["stream"], f.get("which", -1))
        assert sih.num_extra_channels == nec, "the frame's stream and the image header disagree on the extra channels"
        toc, sec, end, nt = _frame_end(L, cs, at, sih)
        r = _Bits(cs, at)
        hp = _head(r, nec)
        p1 = r.pos
        old = _tail_fields(r, (sih.xsize, sih.ysize), sih.have_animation, nec)
        assert old["crop"] is None and not old.get("save_before_color_transform"), "the source frame is cropped / saved in XYB"
        p2 = r.pos
        w = _Writer()
        ftype, flags = f.get("frame_type", 0), hp["flags"] | f.get("flags_or", 0)
        w.bits(1, 0)          # all_default
        w.bits(2, ftype)      # FrameType: regular 0, DC 1, reference-only 2, skip-progressive 3
        w.bits(1, int(f.get("modular", 0)))  # FrameEncoding: VarDCT, or -- for the walk's refusal -- Modular
        if flags == hp["flags"]:
            w.copy(cs, hp["flags_at"], hp["upsampling_at"])
        else:                 # U64 (fields.cc): 0 | 1 + Bits(4) | 17 + Bits(8)
            assert 1 <= flags < 273
            if flags < 17:
                w.bits(2, 1)
                w.bits(4, flags - 1)
            else:
                w.bits(2, 2)
                w.bits(8, flags - 17)
        if not flags & 32:    # (kUseDcFrame: no upsampling fields)
            w.copy(cs, hp["upsampling_at"], hp["qm_at"])
        if f.get("modular", 0):
            w.bits(2, 1)      # group_size_shift where a VarDCT frame has its x_qm_scale / b_qm_scale
        else:
            w.copy(cs, hp["qm_at"], hp["passes_at"])
        if ftype != 2:        # (a reference-only frame has no passes)
            w.copy(cs, hp["passes_at"], p1)
        fw, fh = sih.xsize, sih.ysize
        if ftype == 1:        # a DC frame: its level, and nothing of what follows up to the name
            w.bits(2, 0)      # dc_level 1
        elif ftype == 2:      # a reference-only frame: full size, slot, saved before the colour transform
            w.bits(1, 0)
            w.u32(f.get("save_as_reference", 0), *_val(0, 1, 2, 3))
            w.bits(1, 1)
        else:
            crop = f.get("crop")
            if crop is None:
                assert (fw, fh) == (W, H), "a frame of another size than the image needs an origin"
            custom = crop is not None
            w.bits(1, int(custom))
            partial = False
            if custom:
                x0, y0 = crop
                w.u32(_pack_signed(x0), *_ORIGIN)
                w.u32(_pack_signed(y0), *_ORIGIN)
                w.u32(fw, *_ORIGIN)
                w.u32(fh, *_ORIGIN)
                partial = x0 > 0 or y0 > 0 or fw + x0 < W or fh + y0 < H
            mode, last = f.get("mode", REPLACE), int(f.get("is_last", k + 1 == len(frames)))
            _write_blending(w, nec, partial, mode, f.get("clamp", 0), f.get("source", 0))
            for _ in range(nec):  # every extra channel with ec_mode (default kReplace) from the same source
                _write_blending(w, nec, partial, f.get("ec_mode", REPLACE), 0, f.get("source", 0))
            duration = f.get("duration", 0)
            if ih.have_animation:
                w.u32(duration, *_DURATION)
            else:
                assert duration == 0
            w.bits(1, last)
            save = f.get("save_as_reference", 0)
            if not last:
                w.u32(save, *_val(0, 1, 2, 3))
            else:
                assert save == 0
            if not last and (duration == 0 or save != 0) and mode == REPLACE and not partial:
                w.bits(1, int(f.get("save_before_color_transform", 0)))  # (default: saved after it)
        if f.get("modular", 0):  # (a Modular frame's loop filter has other fields: no name, the default filter, no extensions)
            w.bits(2, 0)
            w.bits(1, 1)
            w.bits(2, 0)
        else:
            w.copy(cs, p2, toc)
        # the TOC: the permutation flag, padding to a byte, the entries from a byte boundary on, padding (toc.cc ReadToc)
        t = _Bits(cs, toc)
        assert t.bits(1) == 0, "permuted TOC"
        w.bits(1, 0)
        entries = (t.pos + 7) // 8
        t.pos = entries * 8
        for _ in range(nt):
            t.u32(*_TOC)
        assert (t.pos + 7) // 8 == sec
        out += w.to_bytes() + cs[entries:end // 8]
    return bytes(out)


_SIZE = ((9, 1), (13, 1), (18, 1), (30, 1))


def with_preview(cs):
    """The bytes of a bare codestream whose image header already has extra_fields (an animation) with have_preview set
    and a 128 x 128 PreviewHeader inserted (headers.cc:129-181, image_metadata.cc:283-316).  No preview frame follows and
    the frames are no longer byte-aligned: for the walk's refusal, which looks at the image header only."""
    r = _Bits(cs, 16)  # behind the signature
    small = r.bits(1)  # SizeHeader
    if small:
        r.bits(5)
    else:
        r.u32(*_SIZE)
    if r.bits(3) == 0:
        if small:
            r.bits(5)
        else:
            r.u32(*_SIZE)
    assert r.bits(1) == 0 and r.bits(1) == 1, "ImageMetadata: all_default, or without extra_fields"
    r.bits(3)  # orientation
    assert r.bits(1) == 0, "have_intrinsic_size"
    at = r.pos
    assert r.bits(1) == 0, "the stream has a preview already"
    w = _Writer()
    w.copy(cs, 0, at)
    w.bits(1, 1)   # have_preview
    w.bits(1, 1)   # PreviewHeader: div8
    w.bits(2, 0)   #   ysize_div8 = Val(16)
    w.bits(3, 1)   #   ratio 1: xsize = ysize
    w.copy(cs, at + 1, len(cs) * 8)
    return w.to_bytes()
