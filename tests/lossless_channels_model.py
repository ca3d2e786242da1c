"""A numpy model of the device stage of a lossless frame WITH an alpha plane and / or of a GREY image --
jxlhip_decode_modular_channels / k_modular_planes (libjxl_amd/csrc/kernels_modular.hip) -- which is tests/modular_model.py
plus two things, both written from the reference's text:

  * a grey image has ONE colour channel and no RCT (dec_modular.cc:215-219); its sample goes to R, G and B -- the
    reference's pipeline carries a grey image as three equal channels;
  * alpha is converted with the factor of ITS bit depth, float32(1.0 / (2^alpha_bits - 1)), one IEEE multiply
    (dec_modular.cc:697-734), and written like a colour channel; without an alpha plane the fourth channel is the opaque 1.0
    (stage_write.cc:355-360).  Nothing un-premultiplies.

Also: the fixtures of tests/golden/lossless_channels/ and the host front-end through jxlhip_modular_image_decode_channels.
Shared by tests/test_lossless_channels_front_end.py (CPU) and tests/test_gpu_lossless_channels.py."""
import ctypes as C
import json
import os

import numpy as np

import modular_model as mm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lossless_channels")
CS_GRAY = 1  # JXLHIP_CS_GRAY
EC_ALPHA = 0  # JXLHIP_EC_ALPHA


def manifest():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)["files"]


def fixture(name):
    with open(os.path.join(GOLDEN, name + ".jxl"), "rb") as f:
        return f.read()


def samples(planes, group_dim=256, group_rct=None, global_rct=0):
    """The image's colour samples from the planes the front-end leaves: three planes through their programs, one (grey)
    as it is -- a non-zero program on one plane is an error.  Returns a list of int32 [H, W] arrays."""
    if len(planes) == 3:
        return mm.undo_programs(planes, group_dim, group_rct, global_rct)
    assert len(planes) == 1 and global_rct == 0 and (group_rct is None or not np.asarray(group_rct).any())
    return [np.array(planes[0], dtype=np.int64).astype(np.uint32).astype(np.int32)]


def emit_rgba_f32(planes, bits, alpha=None, alpha_bits=0, group_dim=256, group_rct=None, global_rct=0):
    """What k_modular_planes writes as 4-channel float: [H, W, 4] float32."""
    s = samples(planes, group_dim, group_rct, global_rct)
    if len(s) == 1:
        s = [s[0], s[0], s[0]]
    rgb = mm.to_float(s, bits)
    if alpha is None:
        a = np.ones(rgb.shape[:2], np.float32)
    else:
        a = np.asarray(alpha).astype(np.int32).astype(np.float32) * np.float32(1.0 / ((1 << alpha_bits) - 1))
    return np.concatenate([rgb, a[..., None]], axis=-1)


def headers(L, abi, cs):
    """(rc, image header, its first four extra channels, frame header, the TOC's bit position)"""
    ih, extra = abi.ImageHeader(), (abi.ExtraChannel * 4)()
    pos = C.c_size_t(0)
    rc = L.jxlhip_image_header_decode(cs, len(cs), C.byref(pos), extra, 4, C.byref(ih))
    if rc:
        return rc, None, None, None, 0
    info = abi.ImageInfo(ih.xsize, ih.ysize, ih.xyb_encoded, ih.num_extra_channels, None, ih.have_animation, ih.have_timecodes, 0,
                         ih.bit_depth.bits_per_sample)
    fh = abi.FrameHeader()
    rc = L.jxlhip_frame_header_decode(cs, len(cs), C.byref(pos), C.byref(info), C.byref(fh))
    return rc, ih, extra, fh, pos.value


def is_grey(ih):
    return bool(not ih.color_encoding.all_default and ih.color_encoding.color_space == CS_GRAY)


def host_decode(L, abi, cs, sample_type=None, runner=None, runner_opaque=None, fh_edit=None, num_extra=None):
    """The headers of a bare codestream, then jxlhip_modular_image_decode_channels on its frame.  fh_edit(fh) may change
    the parsed frame header first.  Returns (rc, why, dict)."""
    cs = bytes(cs)
    rc, ih, extra, fh, pos = headers(L, abi, cs)
    if rc:
        return rc, "", None
    if fh_edit:
        fh_edit(fh)
    if sample_type is None:
        sample_type = abi.MODULAR_I16 if ih.modular_16_bit_buffer_sufficient else abi.MODULAR_I32
    h, w = fh.ysize, fh.xsize
    nc, ne = (1 if is_grey(ih) else 3), (min(4, ih.num_extra_channels) if num_extra is None else num_extra)
    stride = w + 5  # (rows with padding: the entry must leave it alone)
    dtype = np.int16 if sample_type == abi.MODULAR_I16 else np.int32
    planes = np.full((nc + ne, h, stride), -12345, dtype)
    group_rct = np.full(int(fh.num_groups), 0xFFFF, np.uint16)
    ch = abi.ModularImageChannels()
    ch.num_color, ch.num_extra = nc, ne
    for c in range(nc):
        ch.planes[c] = planes[c].ctypes.data
    for e in range(ne):
        ch.extra_planes[e] = planes[nc + e].ctypes.data
        ch.extra_bits[e] = extra[e].bit_depth.bits_per_sample if e < ih.num_extra_channels else 8
    ch.stride_samples, ch.sample_type, ch.group_rct = stride, sample_type, group_rct.ctypes.data
    why, p = C.c_char_p(), C.c_size_t(pos)
    rc = L.jxlhip_modular_image_decode_channels(cs, len(cs), C.byref(p), C.byref(fh), runner, runner_opaque, C.byref(ch), C.byref(why))
    out = dict(ih=ih, fh=fh, extra=extra, num_color=nc, planes=planes[:nc, :, :w], extras=planes[nc:, :, :w], padding=planes[:, :, w:],
               extra_bits=[int(ch.extra_bits[e]) for e in range(ne)], group_rct=group_rct, global_rct=ch.global_rct,
               global_tree=ch.global_tree, global_on_host=ch.global_on_host, groups_on_device=ch.groups_on_device,
               groups_on_host=ch.groups_on_host, end_bit=p.value, int16=dtype == np.int16)
    return rc, (why.value or b"").decode(), out


def alpha_index(o):
    """The first extra channel of type alpha, or None."""
    for e in range(len(o["extra_bits"])):
        if o["extra"][e].type == EC_ALPHA:
            return e
    return None
