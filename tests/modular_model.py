"""A numpy model of the device stage of a lossless (regular Modular) frame -- jxlhip_decode_modular_frame / k_modular_emit
(libjxl_amd/csrc/kernels_modular.hip) -- written from the reference's text, not from the kernel:

  * the 42 reversible colour transforms and their inverses (lib/jxl/modular/transform/rct.cc:29-150 for the inverse,
    lib/jxl/modular/transform/enc_rct.cc for the forward direction), type = 7 * permutation + custom, in int32
    arithmetic that wraps like the reference's Add / PixelAdd, with its arithmetic >> 1;
  * the order: a pixel's GROUP program first, then the GLOBAL one, each undone last-listed first (a program is the
    first-listed type | the second-listed type << 8; type 0 is the identity);
  * the conversion: (float32) v * float32(1.0 / (2^bits - 1)), one IEEE multiply (dec_modular.cc:75-104,584-586).

Shared by tests/test_modular_model.py, tests/test_modular_front_end.py (CPU) and tests/test_gpu_modular.py."""
import ctypes as C

import numpy as np

MAX_RCTS = 2



def _add(a, b):  # PixelAdd: the sum in uint32, back to int32
    return (a.astype(np.uint32) + b.astype(np.uint32)).astype(np.int32)


def _sub(a, b):
    return (a.astype(np.uint32) - b.astype(np.uint32)).astype(np.int32)


def _targets(permutation):
    """rct.cc:121-125: where the first / second / third result goes."""
    return permutation % 3, (permutation + 1 + permutation // 3) % 3, (permutation + 2 - permutation // 3) % 3


def inverse_rct(planes, rct_type):
    """InvRCT (rct.cc:29-148) on three int32 arrays (any equal shape); returns the three output channels."""
    c0, c1, c2 = (np.asarray(p, np.int32) for p in planes)
    assert 0 <= rct_type < 42
    if rct_type == 0:
        return [c0, c1, c2]
    permutation, custom = divmod(rct_type, 7)
    if custom == 6:  # YCoCg
        tmp = _sub(c0, c2 >> 1)
        g = _add(c2, tmp)
        b = _sub(tmp, c1 >> 1)
        r = _add(b, c1)
        first, second, third = r, g, b
    else:
        first, second, third = c0, c1, c2
        if custom & 1:
            third = _add(third, first)
        if custom >> 1 == 1:
            second = _add(second, first)
        elif custom >> 1 == 2:
            second = _add(second, _add(first, third) >> 1)
    out = [None, None, None]
    t = _targets(permutation)
    out[t[0]], out[t[1]], out[t[2]] = first, second, third
    return out


def forward_rct(planes, rct_type):
    """FwdRCT (enc_rct.cc): the encoder's direction, so that inverse_rct(forward_rct(x)) == x for every int32 x."""
    assert 0 <= rct_type < 42
    p = [np.asarray(q, np.int32) for q in planes]
    if rct_type == 0:
        return p
    permutation, custom = divmod(rct_type, 7)
    t = _targets(permutation)
    first, second, third = p[t[0]], p[t[1]], p[t[2]]
    if custom == 6:
        r, g, b = first, second, third
        co = _sub(r, b)
        tmp = _add(b, co >> 1)
        cg = _sub(g, tmp)
        y = _add(tmp, cg >> 1)
        return [y, co, cg]
    if custom >> 1 == 1:
        second = _sub(second, first)
    elif custom >> 1 == 2:
        second = _sub(second, _add(first, third) >> 1)
    if custom & 1:
        third = _sub(third, first)
    return [first, second, third]


def undo_program(planes, program):
    """A program's RCTs undone, the last-listed (high byte) first."""
    for rct_type in (program >> 8, program & 0xFF):
        planes = inverse_rct(planes, rct_type)
    return planes


def undo_programs(planes, group_dim, group_rct, global_rct):
    """planes: three [H, W] integer arrays as the host front-end leaves them; group_rct: one program per group of
    group_dim x group_dim pixels, raster order (None = all 0).  Returns three int32 [H, W] arrays: the image's samples."""
    planes = [np.array(p, dtype=np.int64).astype(np.uint32).astype(np.int32) for p in planes]
    h, w = planes[0].shape
    xsg, ysg = -(-w // group_dim), -(-h // group_dim)
    if group_rct is not None:
        group_rct = np.asarray(group_rct).reshape(-1)
        assert group_rct.size == xsg * ysg
        for g in range(xsg * ysg):
            if group_rct[g] == 0:
                continue
            ys = slice((g // xsg) * group_dim, min(h, (g // xsg + 1) * group_dim))
            xs = slice((g % xsg) * group_dim, min(w, (g % xsg + 1) * group_dim))
            got = undo_program([p[ys, xs].copy() for p in planes], int(group_rct[g]))  # (copies: a permutation returns its inputs)
            for c in range(3):
                planes[c][ys, xs] = got[c]
    return undo_program(planes, int(global_rct))


def to_float(samples, bits):
    """ModularImageToDecodedRect for integer samples: one float32 multiply by float32(1 / (2^bits - 1))."""
    factor = np.float32(1.0 / ((1 << bits) - 1))
    return np.stack([s.astype(np.float32) * factor for s in samples], axis=-1)


def emit_f32(planes, bits, group_dim, group_rct=None, global_rct=0):
    """What k_modular_emit writes as float RGB: [H, W, 3] float32."""
    return to_float(undo_programs(planes, group_dim, group_rct, global_rct), bits)


# ---- the host front-end through its one entry (no device): jxlhip_modular_image_decode

def host_decode(L, abi, cs, sample_type=None, runner=None, runner_opaque=None):
    """The headers of a bare codestream, then jxlhip_modular_image_decode on its frame.  Returns (rc, why, dict) with the
    planes ([3, H, W] of int16 / int32), group_rct, global_rct, the struct's out fields, and the headers."""
    cs = bytes(cs)
    ih = abi.ImageHeader()
    pos = C.c_size_t(0)
    rc = L.jxlhip_image_header_decode(cs, len(cs), C.byref(pos), None, 0, C.byref(ih))
    if rc:
        return rc, "", None
    info = abi.ImageInfo(ih.xsize, ih.ysize, ih.xyb_encoded, ih.num_extra_channels, None, ih.have_animation, ih.have_timecodes, 0,
                         ih.bit_depth.bits_per_sample)
    fh = abi.FrameHeader()
    rc = L.jxlhip_frame_header_decode(cs, len(cs), C.byref(pos), C.byref(info), C.byref(fh))
    if rc:
        return rc, "", None
    if sample_type is None:
        sample_type = abi.MODULAR_I16 if ih.modular_16_bit_buffer_sufficient else abi.MODULAR_I32
    h, w = fh.ysize, fh.xsize
    stride = w + 5  # (rows with padding: the entry must leave it alone)
    dtype = np.int16 if sample_type == abi.MODULAR_I16 else np.int32
    planes = np.full((3, h, stride), -12345, dtype)
    group_rct = np.full(int(fh.num_groups), 0xFFFF, np.uint16)
    pl = abi.ModularImagePlanes()
    for c in range(3):
        pl.planes[c] = planes[c].ctypes.data
    pl.stride_samples = stride
    pl.sample_type = sample_type
    pl.group_rct = group_rct.ctypes.data
    why = C.c_char_p()
    rc = L.jxlhip_modular_image_decode(cs, len(cs), C.byref(pos), C.byref(fh), runner, runner_opaque, C.byref(pl), C.byref(why))
    out = dict(ih=ih, fh=fh, planes=planes[:, :, :w], padding=planes[:, :, w:], group_rct=group_rct, global_rct=pl.global_rct,
               global_tree=pl.global_tree, global_on_host=pl.global_on_host, groups_on_device=pl.groups_on_device,
               groups_on_host=pl.groups_on_host, end_bit=pos.value)
    return rc, (why.value or b"").decode(), out
