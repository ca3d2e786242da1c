"""GPU box: ms/frame of an 8K d1.0 synthetic frame (Gaborish + EPF1) with blending off and on (jxlhip_set_blending), as
float RGB (linear) and as sRGB RGBA8, one frame in flight: the median of N synchronised decodes each, then one profiled
decode per case (per-kernel-slot times from jxlhip_profile_read_ex).  Cases:
  off        no blending
  save       full-frame kReplace saved into a slot (an animation frame a later frame blends over)
  add        full-frame kAdd over a canvas, saved into its own source slot
  crop       a 1920 x 1080 frame at (2880, 1620) with kAdd over the 8K canvas, saved into its own source slot
  crop-nosave  the same crop, not saved
Beside them, in the same run: k_splines' emit-only launch on the same frame (one short spline), the yardstick for a
launch that reads a frame's worth of floats and writes the output.  For every case the bytes k_blend has to move (the
canvas vectors it reads, the staged frame under the rectangle, the slot it writes, the caller's output) are set against
its time.
Usage: python tools/blend_bench.py [N=30] [xsize ysize]"""
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
CW, CH = min(1920, XS), min(1080, YS)
CX, CY = (XS - CW) // 2, (YS - CH) // 2
# case -> (frame, origin, mode, source, save slot)
CASES = {"save": ("full", (0, 0), abi.BLEND_REPLACE, 0, 0), "add": ("full", (0, 0), abi.BLEND_ADD, 0, 0),
         "crop": ("crop", (CX, CY), abi.BLEND_ADD, 0, 0), "crop-nosave": ("crop", (CX, CY), abi.BLEND_ADD, 0, None)}


def traffic(case, out_bpp):
    """Bytes k_blend must move: (canvas read, staged frame read, slot written, output written).  The caller's output
    is written in every case, so every launch visits the whole canvas."""
    frame, _, mode, _, save = CASES[case]
    px = XS * YS
    rect = px if frame == "full" else CW * CH
    bg = 0 if (mode == abi.BLEND_REPLACE and frame == "full") else px * 12  # dead under a full-frame kReplace
    slot = 0 if save is None else rect * 12  # saved into its own source slot: only under the rectangle
    return bg, rect * 12, slot, px * out_bpp


fmt8 = dict(transfer=abi.TF_SRGB, sample_type=abi.SAMPLE_U8, num_channels=4, bits_per_sample=8)
short_spline = [dict(start=(100, 100), deltas=[(8, 0), (0, 0)], color=[[0] * 32 for _ in range(3)], sigma=[4] + [0] * 31)]
short_spline[0]["color"][1][0] = 3
dec = VarDctDecoder(0)
dq = dec.default_dequant_tables()
res = {}
for out_name, kw, bpp in (("f32", dict(output_kind=1), 12), ("rgba8", dict(output_kind=2, out_format=fmt8), 4)):
    frames = {"full": synth.synth_frame(XS, YS, device="cuda", gab=True, epf_iters=1, **kw),
              "crop": synth.synth_frame(CW, CH, device="cuda", gab=True, epf_iters=1, seed=7, **kw)}
    out = torch.empty((YS, XS, 3 if bpp == 12 else 4), dtype=torch.float32 if bpp == 12 else torch.uint8, device="cuda")

    def begin(case):
        frame = CASES[case][0] if case in CASES else "full"
        dec.begin_frame(frames[frame][0])
        dec.set_inputs(frames[frame][1], dq)
        if case in CASES:
            _, origin, mode, source, save = CASES[case]
            dec.set_blending((XS, YS), origin, mode, False, source, save)
        elif case == "spline":
            dec.set_splines(short_spline)

    # the canvas the blends read: one full frame saved into slot 0
    begin("save")
    dec.decode_frame(out)
    dec.sync()
    for case in ("off", "save", "add", "crop", "crop-nosave", "spline"):
        begin(case)
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
        res[(out_name, case)] = (med, prof)
        line = "%dx%d d1.0 gab+epf1 %-5s %-11s: median %.3f ms/frame (min %.3f, %d runs); kernel slots: %s" % (
            XS, YS, out_name, case, med, min(times) * 1e3, N, ", ".join("%s %.3f ms" % (k, v[0]) for k, v in prof.items()))
        if case in CASES:
            b = traffic(case, bpp)
            ms = prof["blend"][0]
            line += "; k_blend moves %.0f MB (canvas %.0f + frame %.0f read, slot %.0f + output %.0f written) = %.2f TB/s" % (
                sum(b) / 1e6, b[0] / 1e6, b[1] / 1e6, b[2] / 1e6, b[3] / 1e6, sum(b) / (ms * 1e9))
        print(line, flush=True)
    spl = res[(out_name, "spline")][1]["splines"][0]
    emit_bytes = XS * YS * (12 + bpp)
    print("%s: k_splines emit-only %.3f ms for %.0f MB = %.2f TB/s" % (out_name, spl, emit_bytes / 1e6, emit_bytes / (spl * 1e9)))
    for case in CASES:
        med, prof = res[(out_name, case)]
        print("%s: %s / off = %.2fx; k_blend %.3f ms" % (out_name, case, med / res[(out_name, "off")][0], prof["blend"][0]))
dec.close()
