"""GPU box: ms/frame of an 8K d1.0 synthetic frame (Gaborish + EPF1, linear float RGB out) with photon noise on and off
(jxlhip_set_noise), one frame in flight: the median of N synchronised decodes each, then one profiled decode per mode
(per-kernel-slot times from jxlhip_profile_read).  Usage: python tools/noise_bench.py [N=30] [xsize ysize]"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libjxl_amd import VarDctDecoder, synth  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 30
XS, YS = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (7680, 4320)
LUT = [0.05, 0.12, 0.3, 0.45, 0.6, 0.75, 0.9, 1.0]  # every pixel gets noise

params, t = synth.synth_frame(XS, YS, device="cuda", output_kind=1, gab=True, epf_iters=1)
dec = VarDctDecoder(0)
dq = dec.default_dequant_tables()
out = None
res = {}
for mode in ("off", "on"):
    dec.begin_frame(params)
    dec.set_inputs(t, dq)
    if mode == "on":
        dec.set_noise(LUT, 1, 0)
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
    res[mode] = statistics.median(times) * 1e3
    print("%dx%d d1.0 gab+epf1 f32, noise %-3s: median %.3f ms/frame (min %.3f, %d runs) = %.1f Gpx/s; kernel slots: %s" % (
        XS, YS, mode, res[mode], min(times) * 1e3, N, XS * YS / (res[mode] * 1e6),
        ", ".join("%s %.3f ms" % (k, v[0]) for k, v in prof.items())), flush=True)
print("noise on / off = %.2fx" % (res["on"] / res["off"]))
dec.close()
