"""Frame sequences of images with extra channels, for the tests of alpha blending: what tests/layer_streams.py does, with
the blending info of every extra channel and the colour's alpha channel under the caller's control, and the image
header's alpha_associated bit.

  splice_ec             frames of oracle streams behind the image header of another one, each with a rewritten frame
                        header: layer_streams.splice's fields for the colour plus alpha_channel, and ec = one dict(mode,
                        clamp, source, alpha_channel) per extra channel (default: kReplace from the colour's source)
  set_alpha_associated  the bytes of a codestream with ExtraChannelInfo::alpha_associated of its first alpha channel set
"""
import layer_streams as ls
from layer_streams import ADD, ALPHA_WEIGHTED_ADD, BLEND, MUL, REPLACE  # noqa: F401


def splice_ec(L, header_stream, frames):
    """The image header of header_stream, then one regular VarDCT frame per entry of `frames` (see the module's
    docstring; stream, which, crop, mode, clamp, source, duration, is_last, save_as_reference as layer_streams.splice;
    upsampling = 2 | 4 | 8 rewrites the upsampling factors of the colour and the extra channels and nothing else, for the
    file the walk refuses)."""
    _, first, ih = ls.source_frame(L, header_stream, 0)
    out = bytearray(header_stream[:first // 8])
    W, H, nec = ih.xsize, ih.ysize, ih.num_extra_channels
    for k, f in enumerate(frames):
        cs, at, sih = ls.source_frame(L, f["stream"], f.get("which", -1))
        assert sih.num_extra_channels == nec, "the frame's stream and the image header disagree on the extra channels"
        toc, sec, end, nt = ls._frame_end(L, cs, at, sih)
        r = ls._Bits(cs, at)
        hp = ls._head(r, nec)
        p1 = r.pos
        old = ls._tail_fields(r, (sih.xsize, sih.ysize), sih.have_animation, nec)
        assert old["crop"] is None and not old.get("save_before_color_transform"), "the source frame is cropped / saved in XYB"
        p2 = r.pos
        w = ls._Writer()
        w.copy(cs, at, p1)  # all_default .. passes, bit for bit
        if f.get("upsampling"):  # (for the walk's refusal: U32(Val(1), Val(2), Val(4), Val(8)) is its two selector bits;
            # the extra channels' factors follow and must not be below the colour's)
            sel = {1: 0, 2: 1, 4: 2, 8: 3}[f["upsampling"]]
            u = hp["upsampling_at"] - at
            assert hp["qm_at"] - hp["upsampling_at"] == 2 * (1 + nec)
            w.b[u:u + 2 * (1 + nec)] = [sel & 1, sel >> 1] * (1 + nec)
        fw, fh = sih.xsize, sih.ysize
        crop = f.get("crop")
        if crop is None:
            assert (fw, fh) == (W, H), "a frame of another size than the image needs an origin"
        w.bits(1, int(crop is not None))
        partial = False
        if crop is not None:
            x0, y0 = crop
            w.u32(ls._pack_signed(x0), *ls._ORIGIN)
            w.u32(ls._pack_signed(y0), *ls._ORIGIN)
            w.u32(fw, *ls._ORIGIN)
            w.u32(fh, *ls._ORIGIN)
            partial = x0 > 0 or y0 > 0 or fw + x0 < W or fh + y0 < H
        mode, last = f.get("mode", REPLACE), int(f.get("is_last", k + 1 == len(frames)))
        ls._write_blending(w, nec, partial, mode, f.get("clamp", 0), f.get("source", 0), f.get("alpha_channel", 0))
        ec = f.get("ec") or [{}] * nec
        assert len(ec) == nec
        for e in ec:
            ls._write_blending(w, nec, partial, e.get("mode", REPLACE), e.get("clamp", 0), e.get("source", f.get("source", 0)),
                               e.get("alpha_channel", 0))
        duration = f.get("duration", 0)
        if ih.have_animation:
            w.u32(duration, *ls._DURATION)
        else:
            assert duration == 0
        w.bits(1, last)
        save = f.get("save_as_reference", 0)
        if not last:
            w.u32(save, *ls._val(0, 1, 2, 3))
        else:
            assert save == 0
        if not last and (duration == 0 or save != 0) and mode == REPLACE and not partial:
            w.bits(1, 0)  # saved after the colour transform
        w.copy(cs, p2, toc)
        t = ls._Bits(cs, toc)
        assert t.bits(1) == 0, "permuted TOC"
        w.bits(1, 0)
        entries = (t.pos + 7) // 8
        t.pos = entries * 8
        for _ in range(nt):
            t.u32(*ls._TOC)
        assert (t.pos + 7) // 8 == sec
        out += w.to_bytes() + cs[entries:end // 8]
    return bytes(out)


def _bit_depth(r):
    """BitDepth (image_metadata.cc:26-46)"""
    if r.bits(1):  # floating_point_sample
        r.u32((0, 32), (0, 16), (0, 24), (6, 1))
        r.bits(4)  # exponent_bits_per_sample - 1
    else:
        r.u32((0, 8), (0, 10), (0, 12), (6, 1))


def set_alpha_associated(cs):
    """The bytes of a bare codestream with ExtraChannelInfo::alpha_associated of its first alpha channel set to 1
    (image_metadata.cc:221-262; the fields in front of it: headers.cc SizeHeader / AnimationHeader,
    image_metadata.cc:283-340).  The channel's info must not be all_default -- an 8-bit alpha channel's is, and then the
    bit is not in the stream: use a 16-bit one."""
    r = ls._Bits(cs, 16)  # behind the signature
    small = r.bits(1)  # SizeHeader
    if small:
        r.bits(5)
    else:
        r.u32(*ls._SIZE)
    if r.bits(3) == 0:
        if small:
            r.bits(5)
        else:
            r.u32(*ls._SIZE)
    assert r.bits(1) == 0, "ImageMetadata: all_default"
    if r.bits(1):  # extra_fields
        r.bits(3)  # orientation
        assert r.bits(1) == 0, "have_intrinsic_size"
        assert r.bits(1) == 0, "have_preview"
        if r.bits(1):  # AnimationHeader
            r.u32((0, 100), (0, 1000), (10, 1), (30, 1))
            r.u32((0, 1), (0, 1001), (8, 1), (10, 1))
            r.u32((0, 0), (3, 0), (16, 0), (32, 0))
            r.bits(1)
    _bit_depth(r)
    r.bits(1)  # modular_16_bit_buffer_sufficient
    n = r.u32((0, 0), (0, 1), (4, 2), (12, 1))
    for _ in range(n):
        assert r.bits(1) == 0, "ExtraChannelInfo: all_default (the bit is not coded)"
        kind = r.u32((0, 0), (0, 1), (4, 2), (6, 18))  # Enum
        _bit_depth(r)
        r.u32((0, 0), (0, 3), (0, 4), (3, 1))  # dim_shift
        r.bits(8 * r.u32((0, 0), (4, 0), (5, 16), (10, 48)))  # name
        if kind == 0:  # kAlpha
            out = bytearray(cs)
            out[r.pos >> 3] |= 1 << (r.pos & 7)
            return bytes(out)
        if kind == 2:  # kSpotColor
            r.bits(64)
        if kind == 5:  # kCFA
            r.u32((0, 1), (2, 0), (4, 3), (8, 19))
    raise AssertionError("no alpha channel")
