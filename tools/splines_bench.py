"""GPU box: ms/frame of an 8K d1.0 synthetic frame (Gaborish + EPF1, linear float RGB out) with splines off, on, and on
with photon noise (jxlhip_set_splines, jxlhip_set_noise), one frame in flight: the median of N synchronised decodes
each, then one profiled decode per mode (per-kernel-slot times from jxlhip_profile_read).  Two spline sets:
  a  the two splines of the reference encoder's feature stream (oracle/ref_real_stream.cc FeatureStream), scaled to
     the frame and quantized as QuantizedSpline::Create does (y_to_x = 0, y_to_b = 1);
  b  256 random splines of 32 control points, sigma 2-8, across the frame.
Usage: python tools/splines_bench.py [N=30] [xsize ysize]"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libjxl_amd import VarDctDecoder, abi, synth  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 30
XS, YS = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (7680, 4320)
LUT = [0.05, 0.12, 0.3, 0.45, 0.6, 0.75, 0.9, 1.0]
WEIGHT = [0.0042, 0.075, 0.07, 0.3333]


def _round(v):
    return int(np.sign(v) * np.floor(abs(v) + 0.5))


def quantize(points, color, sigma):
    """QuantizedSpline::Create with quantization_adjustment 0, y_to_x 0, y_to_b 1 (splines.cc:385-437)."""
    pts = [(_round(x), _round(y)) for x, y in points]
    deltas, pdx, pdy = [], 0, 0
    for (x0, y0), (x1, y1) in zip(pts, pts[1:]):
        deltas.append((x1 - x0 - pdx, y1 - y0 - pdy))
        pdx, pdy = x1 - x0, y1 - y0
    q = np.zeros((3, 32), np.int64)
    for i in range(32):
        f = 1.41421356237 if i == 0 else 1.0
        q[1][i] = _round(color[1][i] * f / WEIGHT[1])
        ry = q[1][i] / f * WEIGHT[1]
        q[0][i] = _round(color[0][i] * f / WEIGHT[0])
        q[2][i] = _round((color[2][i] - ry) * f / WEIGHT[2])
    s = [_round(sigma[i] * (1.41421356237 if i == 0 else 1.0) / WEIGHT[3]) for i in range(32)]
    return dict(start=pts[0], deltas=deltas, color=q.tolist(), sigma=s)


def set_a(xs, ys):
    out = []
    for k in range(2):
        pts = [(xs * (0.1 + 0.2 * i), ys * ((0.25 + 0.1 * ((i * 3) % 4)) if k else (0.8 - 0.12 * ((i * 2) % 5))))
               for i in range(5)]
        color = np.zeros((3, 32))
        sigma = np.zeros(32)
        color[1][0], color[0][0], color[2][0] = (0.35, 0.01, 0.1) if k else (0.2, -0.02, 0.25)
        color[1][1] = 0.05
        sigma[0], sigma[1] = (4.5 if k else 3.0), 0.5
        out.append(quantize(pts, color, sigma))
    return out


def set_b(xs, ys, n=256, points=32):
    rng = np.random.default_rng(7)
    out = []
    for _ in range(n):
        x, y = rng.uniform(0, xs), rng.uniform(0, ys)
        pts = [(x, y)]
        for _ in range(points - 1):
            a = rng.uniform(0, 2 * np.pi)
            r = rng.uniform(40, 200)
            x = float(np.clip(x + r * np.cos(a), 0, xs - 1))
            y = float(np.clip(y + r * np.sin(a), 0, ys - 1))
            if (_round(x), _round(y)) == (_round(pts[-1][0]), _round(pts[-1][1])):
                x = x + 1.0 if x < xs - 2 else x - 1.0
            pts.append((x, y))
        color = np.zeros((3, 32))
        color[1][0], color[0][0], color[2][0] = rng.uniform(0.05, 0.3), rng.uniform(-0.02, 0.02), rng.uniform(0, 0.2)
        sigma = np.zeros(32)
        sigma[0] = rng.uniform(2, 8) * 1.41421356237  # ContinuousIDCT of {s * sqrt2 / sqrt2, 0, ...} = s
        out.append(quantize(pts, color, sigma / 1.41421356237))
    return out


params, t = synth.synth_frame(XS, YS, device="cuda", output_kind=1, gab=True, epf_iters=1)
dec = VarDctDecoder(0)
dq = dec.default_dequant_tables()
sets = {"a": set_a(XS, YS), "b": set_b(XS, YS)}
for name, s in sets.items():
    rc, h = abi.splines_from_quantized(s)
    assert rc == 0
    rc, segs = abi.splines_segments(h, XS, YS, params.get("cfl_base_x", 0.0), params.get("cfl_base_b", 1.0))
    abi.splines_destroy(h)
    assert rc == 0, rc
    print("set %s: %d splines, %d segments" % (name, len(s), len(segs)), flush=True)
out = None
res = {}
for mode in ("off", "a", "b", "a+noise", "b+noise"):
    dec.begin_frame(params)
    dec.set_inputs(t, dq)
    if mode.endswith("+noise"):
        dec.set_noise(LUT, 1, 0)
    t0 = time.perf_counter()
    if mode != "off":
        dec.set_splines(sets[mode[0]])
    host_ms = (time.perf_counter() - t0) * 1e3
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
    print("%dx%d d1.0 gab+epf1 f32, splines %-7s: median %.3f ms/frame (min %.3f, %d runs) = %.1f Gpx/s; "
          "set_splines %.1f ms (host); kernel slots: %s" % (
              XS, YS, mode, res[mode], min(times) * 1e3, N, XS * YS / (res[mode] * 1e6), host_ms,
              ", ".join("%s %.3f ms" % (k, v[0]) for k, v in prof.items())), flush=True)
for mode in ("a", "b", "a+noise", "b+noise"):
    print("splines %s / off = %.2fx" % (mode, res[mode] / res["off"]))
dec.close()
