"""GPU box: ms/frame of an 8K d1.0 synthetic frame (Gaborish + EPF1) with tone mapping off and on
(jxlhip_set_tone_mapping, 1000 -> 250 nits), as float RGB (linear) and as sRGB RGBA8, one frame in flight: the median of N
synchronised decodes each, then one profiled decode per case (per-kernel-slot times from jxlhip_profile_read_ex).
Cases:
  off        no tone mapping: the frame's plain path writes the output
  tone       the plain path writes planar XYB into context memory, k_tone_map writes the output
  spline     k_splines' emit-only launch on the same frame (one short spline): the yardstick, a launch that moves the
             same bytes (three planes in, the output out) with ~25 VALU operations per pixel
Usage: python tools/tone_map_bench.py [N=30] [xsize ysize]"""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from libjxl_amd import VarDctDecoder, abi, synth  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 30
XS, YS = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (7680, 4320)

fmt8 = dict(transfer=abi.TF_SRGB, sample_type=abi.SAMPLE_U8, num_channels=4, bits_per_sample=8)
short_spline = [dict(start=(100, 100), deltas=[(8, 0), (0, 0)], color=[[0] * 32 for _ in range(3)], sigma=[4] + [0] * 31)]
short_spline[0]["color"][1][0] = 3
dec = VarDctDecoder(0)
dq = dec.default_dequant_tables()
for out_name, kw, bpp in (("f32", dict(output_kind=1), 12), ("rgba8", dict(output_kind=2, out_format=fmt8), 4)):
    params, t = synth.synth_frame(XS, YS, device="cuda", gab=True, epf_iters=1, **kw)
    out = torch.empty((YS, XS, 3 if bpp == 12 else 4), dtype=torch.float32 if bpp == 12 else torch.uint8, device="cuda")
    res = {}
    for case in ("off", "tone", "spline"):
        dec.begin_frame(params)
        dec.set_inputs(t, dq)
        if case == "tone":
            dec.set_tone_mapping(1000.0, 250.0)
        elif case == "spline":
            dec.set_splines(short_spline)
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
        med = statistics.median(times) * 1e3
        res[case] = (med, prof)
        print("%dx%d d1.0 gab+epf1 %-5s %-6s: median %.3f ms/frame (min %.3f, %d runs); kernel slots: %s" % (
            XS, YS, out_name, case, med, min(times) * 1e3, N, ", ".join("%s %.3f ms" % (k, v[0]) for k, v in prof.items())),
            flush=True)
    moved = XS * YS * (12 + bpp)
    tm, spl = res["tone"][1]["tone_map"][0], res["spline"][1]["splines"][0]
    print("%s: k_tone_map %.3f ms for %.0f MB = %.2f TB/s; k_splines emit-only %.3f ms = %.2f TB/s; k_tone_map / emit-only = %.2fx; "
          "tone / off = %.2fx" % (out_name, tm, moved / 1e6, moved / (tm * 1e9), spl, moved / (spl * 1e9), tm / spl,
                                  res["tone"][0] / res["off"][0]))
dec.close()
