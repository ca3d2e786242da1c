"""GPU box: the JXLHIP_KERNEL_UPSAMPLE slot (k_upsample, jxlhip_set_upsampling) for an 8K output -- a synthetic frame
coded at 3840x2160 (Gaborish + EPF1) upsampled 2x -- as linear float RGB and as sRGB RGBA8, and beside it the two
in-tree launches that write the same output from full-size planar XYB: k_splines' draw-and-emit launch with one short
spline (every other tile only emits) and the noise launches (k_noise_rng + k_noise_emit) on a 7680x4320 frame.  Per
mode: warm-up, then N frames each profiled on its own (jxlhip_profile_read: one event pair per launch group), the
median per kernel slot; and the bytes the launch must move against the HBM peak.
Usage: python tools/upsample_bench.py [N=30] [factor=2]"""
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libjxl_amd import VarDctDecoder, abi, synth  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 30
F = int(sys.argv[2]) if len(sys.argv) > 2 else 2
W, H = 7680, 4320
CW, CH = W // F, H // F
PEAK = 8.0e12  # bytes/s, MI355X HBM3E
LUT = [0.05, 0.12, 0.3, 0.45, 0.6, 0.75, 0.9, 1.0]
RGBA8 = dict(transfer=abi.TF_SRGB, sample_type=abi.SAMPLE_U8, num_channels=4, bits_per_sample=8)


def short_spline():
    color = np.zeros((3, 32), np.int64)
    color[0][0], color[1][0], color[2][0] = 2, 40, 10
    sigma = np.zeros(32, np.int64)
    sigma[0] = 12
    return [dict(start=(10, 10), deltas=[(30, 20)], color=color.tolist(), sigma=sigma.tolist())]


def run(name, slot, xs, ys, kind, fmt, setup, moved):
    params, t = synth.synth_frame(xs, ys, device="cuda", output_kind=kind, gab=True, epf_iters=1, out_format=fmt)
    dec = VarDctDecoder(0)
    dq = dec.default_dequant_tables()
    dec.begin_frame(params)
    dec.set_inputs(t, dq)
    setup(dec)
    out = dec.alloc_output()
    for _ in range(5):
        dec.decode_frame(out)
    dec.sync()
    dec.profile(True)
    per = {}
    for _ in range(N):
        dec.decode_frame(out)
        for k, v in dec.profile_read().items():
            per.setdefault(k, []).append(v[0])
    dec.close()
    med = {k: statistics.median(v) for k, v in per.items()}
    ms = med[slot]
    print("%-34s %s slot: median %.3f ms (min %.3f, %d frames); must move %.1f MB = %.2f of the %.0f TB/s peak; "
          "all slots: %s" % (name, slot, ms, min(per[slot]), N, moved / 1e6, moved / (ms * 1e-3) / PEAK, PEAK / 1e12,
                             ", ".join("%s %.3f" % kv for kv in sorted(med.items()))), flush=True)


planes_in = 3 * 4 * CW * CH
full_in = 3 * 4 * W * H
for label, kind, fmt, bpp in (("f32 RGB", 1, None, 12), ("sRGB RGBA8", 2, RGBA8, 4)):
    run("upsample %dx %dx%d -> 8K, %s" % (F, CW, CH, label), "upsample", CW, CH, kind, fmt,
        lambda d: d.set_upsampling(F, (W, H)), planes_in + bpp * W * H)
    run("splines (one short spline) 8K, %s" % label, "splines", W, H, kind, fmt,
        lambda d: d.set_splines(short_spline()), full_in + bpp * W * H)
    # the noise launches also write and read back the three random planes
    run("noise 8K, %s" % label, "noise", W, H, kind, fmt, lambda d: d.set_noise(LUT, 1, 0),
        3 * full_in + bpp * W * H)
