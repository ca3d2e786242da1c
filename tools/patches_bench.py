"""GPU box: ms/frame of an 8K d1.0 synthetic frame (Gaborish + EPF1) with patches off and on (jxlhip_set_reference_frame,
jxlhip_set_patches), as linear float RGB and as sRGB RGBA8, one frame in flight: the median of N synchronised decodes
each, then one profiled decode per mode (per-kernel-slot times from jxlhip_profile_read_ex).  Two dictionaries:
  a  the glyph sheet and the placements of the reference encoder's 600 x 400 patches stream
     (oracle.feature_stream("patches")), tiled across the frame at that stream's density;
  b  about a million patches of 3 x 3 .. 8 x 8 from a random 64 x 64 sheet at random places, kAdd / kReplace / kMul.
Beside them, in the same run: k_splines' emit-only launch on the same frame (one short spline), the launch that moves
the same bytes as k_patches without the reference reads.
Usage: python tools/patches_bench.py [N=30] [xsize ysize]"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from libjxl_amd import VarDctDecoder, abi, synth  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 30
XS, YS = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (7680, 4320)
FIELDS = [n for n, _ in abi.Patch._fields_]


def genuine(L):
    """(sheet [3, h, w], slot, placements [n, 10], stream size) of the 600 x 400 d1 patches stream."""
    import oracle
    cs = np.frombuffer(oracle.feature_stream("patches", xsize=600, ysize=400, seed=5, distance=1.0), np.uint8)
    base, n = cs.ctypes.data, len(cs)
    ih, pos = abi.ImageHeader(), C.c_size_t(0)
    assert L.jxlhip_image_header_decode(base, n, C.byref(pos), None, 0, C.byref(ih)) == 0
    info = abi.ImageInfo(ih.xsize, ih.ysize, ih.xyb_encoded, 0, None, 0, 0, 0, ih.bit_depth.bits_per_sample)
    fh0 = abi.FrameHeader()
    assert L.jxlhip_frame_header_decode(base, n, C.byref(pos), C.byref(info), C.byref(fh0)) == 0
    off, sz, total = np.zeros(1, np.uint64), np.zeros(1, np.uint32), C.c_uint64(0)
    assert L.jxlhip_toc_decode(base, n, C.byref(pos), 1, off.ctypes.data, sz.ctypes.data, C.byref(total)) == 0
    start = pos.value // 8
    s0 = cs[start:start + int(sz[0])].copy()
    sheet = np.zeros((3, fh0.ysize, fh0.xsize), np.float32)
    ptrs = (C.c_void_p * 3)(*[sheet[k].ctypes.data for k in range(3)])
    assert L.jxlhip_modular_frame_decode(s0.ctypes.data, len(s0), C.byref(C.c_size_t(0)), C.byref(fh0), ptrs, fh0.xsize, None) == 0
    pos = C.c_size_t((start + total.value) * 8)
    fh1 = abi.FrameHeader()
    assert L.jxlhip_frame_header_decode(base, n, C.byref(pos), C.byref(info), C.byref(fh1)) == 0
    nt = int(fh1.num_toc_entries)
    off, sz, total = np.zeros(nt, np.uint64), np.zeros(nt, np.uint32), C.c_uint64(0)
    assert L.jxlhip_toc_decode(base, n, C.byref(pos), nt, off.ctypes.data, sz.ctypes.data, C.byref(total)) == 0
    d0 = cs[pos.value // 8 + int(off[0]):][:int(sz[0])].tobytes()
    slot = int(fh0.save_as_reference)
    rc, h, _ = abi.patches_decode(d0, 0, fh1.xsize_blocks * 8, fh1.ysize_blocks * 8, {slot: (fh0.xsize, fh0.ysize)}, L=L)
    assert rc == 0
    lst = abi.patches_list(h, L)[0]
    abi.patches_destroy(h, L)
    return sheet, slot, np.array([[p[f] for f in FIELDS] for p in lst], np.uint32), (600, 400)


def set_a(placements, size, xs, ys):
    ix, iy = FIELDS.index("x"), FIELDS.index("y")
    iw, ih = FIELDS.index("xsize"), FIELDS.index("ysize")
    parts = []
    for oy in range(0, ys, size[1]):
        for ox in range(0, xs, size[0]):
            p = placements.copy()
            p[:, ix] += ox
            p[:, iy] += oy
            parts.append(p[(p[:, ix] + p[:, iw] <= xs) & (p[:, iy] + p[:, ih] <= ys)])
    return np.concatenate(parts)


def set_b(xs, ys, slot, n=1000000):
    rng = np.random.default_rng(9)
    p = np.zeros((n, len(FIELDS)), np.uint32)
    w, h = rng.integers(3, 9, n), rng.integers(3, 9, n)
    p[:, FIELDS.index("ref")] = slot
    p[:, FIELDS.index("xsize")], p[:, FIELDS.index("ysize")] = w, h
    p[:, FIELDS.index("ref_x0")], p[:, FIELDS.index("ref_y0")] = rng.integers(0, 64 - w + 1), rng.integers(0, 64 - h + 1)
    p[:, FIELDS.index("x")], p[:, FIELDS.index("y")] = rng.integers(0, xs - w + 1), rng.integers(0, ys - h + 1)
    p[:, FIELDS.index("mode")] = rng.choice([1, 2, 2, 2, 3], n)
    return p


L = abi.load_library()
sheet, slot_a, placements, size = genuine(L)
slot_b = (slot_a + 1) % 4
sheet_b = (np.random.default_rng(3).standard_normal((3, 64, 64)) * 0.01).astype(np.float32)
sets = {"a": set_a(placements, size, XS, YS), "b": set_b(XS, YS, slot_b)}
print("set a: %d patches (%.0f per Mpx, the stream's %d on %dx%d), sheet %dx%d; set b: %d patches, sheet 64x64" % (
    len(sets["a"]), len(sets["a"]) / (XS * YS / 1e6), len(placements), size[0], size[1], sheet.shape[2], sheet.shape[1],
    len(sets["b"])), flush=True)
for name, p in sets.items():
    covered = int((p[:, FIELDS.index("xsize")].astype(np.int64) * p[:, FIELDS.index("ysize")]).sum())
    print("set %s: %.1f Mpx of reference samples read per frame (%.2f of the frame)" % (name, covered / 1e6, covered / (XS * YS)))
fmt8 = dict(transfer=abi.TF_SRGB, sample_type=abi.SAMPLE_U8, num_channels=4, bits_per_sample=8)
short_spline = [dict(start=(100, 100), deltas=[(8, 0), (0, 0)], color=np.zeros((3, 32), int).tolist(), sigma=[4] + [0] * 31)]
short_spline[0]["color"][1][0] = 3
dec = VarDctDecoder(0)
dq = dec.default_dequant_tables()
dec.set_reference_frame(slot_a, sheet)
dec.set_reference_frame(slot_b, sheet_b)
ref_sizes = {slot_a: (sheet.shape[2], sheet.shape[1]), slot_b: (64, 64)}
res = {}
for out_name, kw in (("f32", dict(output_kind=1)), ("rgba8", dict(output_kind=2, out_format=fmt8))):
    params, t = synth.synth_frame(XS, YS, device="cuda", gab=True, epf_iters=1, **kw)
    out = None
    for mode in ("off", "a", "b", "spline"):
        dec.begin_frame(params)
        dec.set_inputs(t, dq)
        host_ms = 0.0
        if mode in sets:
            rc, h = abi.patches_from_list(sets[mode], (XS + 7) & ~7, (YS + 7) & ~7, ref_sizes, L=L)
            assert rc == 0
            t0 = time.perf_counter()
            dec.set_patches(h)
            host_ms = (time.perf_counter() - t0) * 1e3
            abi.patches_destroy(h, L)
        elif mode == "spline":
            dec.set_splines(short_spline)
        out = dec.alloc_output() if out is None else out
        for _ in range(3):
            dec.decode_frame(out)
        dec.sync()
        times = []
        for _ in range(N):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dec.decode_frame(out)
            dec.sync()
            times.append(time.perf_counter() - t0)
        dec.profile(True)
        dec.decode_frame(out)
        prof = dec.profile_read()
        dec.profile(False)
        res[(out_name, mode)] = (statistics.median(times) * 1e3, prof)
        print("%dx%d d1.0 gab+epf1 %-5s, %-7s: median %.3f ms/frame (min %.3f, %d runs) = %.1f Gpx/s; set_patches %.1f ms "
              "(host); kernel slots: %s" % (XS, YS, out_name, "patches " + mode if mode in sets else mode,
                                            res[(out_name, mode)][0], min(times) * 1e3, N,
                                            XS * YS / (res[(out_name, mode)][0] * 1e6), host_ms,
                                            ", ".join("%s %.3f ms" % (k, v[0]) for k, v in prof.items())), flush=True)
    spl = res[(out_name, "spline")][1]["splines"][0]
    for mode in ("a", "b"):
        pat = res[(out_name, mode)][1]["patches"][0]
        print("%s: patches %s / off = %.2fx; k_patches %.3f ms / k_splines emit-only %.3f ms = %.2f" % (
            out_name, mode, res[(out_name, mode)][0] / res[(out_name, "off")][0], pat, spl, pat / spl))
dec.close()
