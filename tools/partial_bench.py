"""GPU box: ms/frame of an 8K d1.0 synthetic frame (Gaborish + EPF1, float RGB) with no, half (a checkerboard) and all
of its AC groups drawn from their DC (jxlhip_set_dc_only_groups), one frame in flight: the median of N synchronised
decodes each, then one profiled decode per case (per-kernel-slot times from jxlhip_profile_read_ex).  For k_dc_upsample8
the bytes it has to move (64 floats written per masked DC sample and plane, the three DC planes read once) are set
against its time; beside it, in the same run, the two-phase k_upsample<8> of a frame whose output has the same size: the
same 25-tap arithmetic from planes at coded size, with the colour stages and the output behind it.
Usage: python tools/partial_bench.py [N=30] [xsize ysize]"""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from libjxl_amd import VarDctDecoder, synth  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 30
XS, YS = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (7680, 4320)
XSG, YSG = (XS + 255) // 256, (YS + 255) // 256
gy, gx = np.mgrid[0:YSG, 0:XSG]
MASKS = {"none": None, "half": (gx + gy) % 2 == 0, "all": np.ones((YSG, XSG), bool)}


def run(dec, begin, out):
    begin()
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
    return statistics.median(times) * 1e3, min(times) * 1e3, prof


dec = VarDctDecoder(0)
dq = dec.default_dequant_tables()
params, t = synth.synth_frame(XS, YS, device="cuda", gab=True, epf_iters=1, output_kind=1)
out = torch.empty((YS, XS, 3), dtype=torch.float32, device="cuda")
for name, mask in MASKS.items():
    def begin():
        dec.begin_frame(params)
        dec.set_inputs(t, dq)
        dec.set_dc_only_groups(mask)
    med, best, prof = run(dec, begin, out)
    line = "%dx%d d1.0 gab+epf1 f32 mask %-4s: median %.3f ms/frame (min %.3f, %d runs); kernel slots: %s" % (
        XS, YS, name, med, best, N, ", ".join("%s %.3f ms" % (k, v[0]) for k, v in prof.items()))
    if mask is not None:
        # the masked groups' DC samples (clipped at the frame's edges), 256 bytes per sample and plane
        xsb, ysb = (XS + 7) // 8, (YS + 7) // 8
        by, bx = np.mgrid[0:ysb, 0:xsb]
        samples = int(mask[by // 32, bx // 32].sum())
        wr, rd = 3 * samples * 256, 3 * xsb * ysb * 4
        ms = prof["dc_upsample"][0]
        line += "; k_dc_upsample8 moves %.0f MB (%.0f written, %.1f DC read) = %.2f TB/s" % ((wr + rd) / 1e6, wr / 1e6, rd / 1e6,
                                                                                         (wr + rd) / (ms * 1e9))
    print(line, flush=True)
# for scale: k_upsample<8> to the same output size (planes at 1/64 of the pixels in, float RGB out)
cw, ch = (XS + 7) // 8, (YS + 7) // 8
p8, t8 = synth.synth_frame(cw, ch, device="cuda", gab=True, epf_iters=1, output_kind=1)


def begin8():
    dec.begin_frame(p8)
    dec.set_inputs(t8, dq)
    dec.set_upsampling(8, (XS, YS))


med, best, prof = run(dec, begin8, out)
ms = prof["upsample"][0]
moved = XS * YS * 12 + 3 * cw * ch * 4
print("%dx%d coded, upsampled 8x to %dx%d f32: median %.3f ms/frame; k_upsample<8> %.3f ms for %.0f MB = %.2f TB/s" % (
    cw, ch, XS, YS, med, ms, moved / 1e6, moved / (ms * 1e9)), flush=True)
dec.close()
