#!/usr/bin/env python3
"""GPU box: the c3 step (8K d1.0, Gaborish + EPF1, int16 -> f32) when the caller hands new side info over for EVERY
frame -- the case that must not get slower by preparing once per hand-over (context.hip: LaunchPhase1): k_prepare
still runs once per frame there, only from another place.

  set_inputs : every step is jxlhip_frame_set_inputs + jxlhip_decode_frame (zero-copy; the prepare stays in the decode)
  upload     : every step is jxlhip_upload_side_info from pinned host arrays + jxlhip_decode_frame, the coefficients
               already resident in the upload buffers (submitted once; the prepare rides behind the side-info copies)
  repeat     : jxlhip_decode_frame alone (bench.py's `value` step), for scale

Per mode: R repetitions of K steps after W warm-up steps, ms per step of each repetition, their median and range.
Prints one JSON line.  Run it on the build before and the build after; JXLHIP_PREPARE_ONCE=0 / 1 is the A/B inside one.

usage: python tools/prepare_once_bench.py [--steps K] [--warmup W] [--reps R] [--width X --height Y]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--width", type=int, default=7680)
    ap.add_argument("--height", type=int, default=4320)
    args = ap.parse_args()
    import torch
    from libjxl_amd import VarDctDecoder, synth
    xs, ys = args.width, args.height
    params, t = synth.synth_frame(xs, ys, mix=synth.MIX_D1, gab=True, epf_iters=1, device="cuda:0")
    dec = VarDctDecoder(0)
    dec.begin_frame(params)
    dq = dec.default_dequant_tables()
    dec.set_inputs(t, dq)
    out = dec.alloc_output()
    dec.decode_frame(out)
    dec.sync()
    want = out.clone()

    def measure(step):
        per = []
        for _ in range(args.warmup):
            step()
        dec.sync()
        for _ in range(args.reps):
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            dec.sync()
            per.append((time.perf_counter() - t0) / args.steps * 1e3)
        return dict(ms_per_step=[round(v, 4) for v in per], median=round(statistics.median(per), 4),
                    min=round(min(per), 4), max=round(max(per), 4))

    res = {}

    def step_repeat():
        dec.decode_frame(out)
    res["repeat"] = measure(step_repeat)

    def step_set_inputs():
        dec.set_inputs(t, dq)
        dec.decode_frame(out)
    res["set_inputs"] = measure(step_set_inputs)
    assert torch.equal(out, want)

    # the host-upload path: side info from pinned host arrays every step, the coefficients submitted once
    up = VarDctDecoder(0)
    up.begin_frame(params)
    L = up.L
    host = {k: t[k].cpu().pin_memory() for k in ("ac_strategy", "raw_quant", "epf_sharpness", "ytox_map", "ytob_map")}
    dc = [d.cpu().pin_memory() for d in t["dc"]]
    dqh = dq.cpu().pin_memory()
    dc3 = (C.c_void_p * 3)(*[d.data_ptr() for d in dc])

    def side_info():
        rc = L.jxlhip_upload_side_info(up.ctx, host["ac_strategy"].data_ptr(), host["raw_quant"].data_ptr(),
                                       host["epf_sharpness"].data_ptr(), host["ytox_map"].data_ptr(),
                                       host["ytob_map"].data_ptr(), dc3, dqh.data_ptr())
        assert rc == 0, L.jxlhip_last_error(up.ctx)
    side_info()
    coeffs = [c.cpu() for c in t["coeffs"]]
    ngroups = ((xs + 255) // 256) * ((ys + 255) // 256)
    esz = coeffs[0].element_size()
    for g in range(ngroups):
        ptrs = (C.c_void_p * 3)(*[c.data_ptr() + g * 65536 * esz for c in coeffs])
        assert L.jxlhip_submit_group(up.ctx, g, ptrs, 65536) == 0
    up.decode_frame(out)
    up.sync()
    assert torch.equal(out, want), "the upload path decoded another frame"
    dec_saved = dec
    dec = up  # (measure() synchronises through `dec`)

    def step_upload():
        side_info()
        up.decode_frame(out)
    res["upload"] = measure(step_upload)
    assert torch.equal(out, want)
    dec = dec_saved
    line = dict(tool="prepare_once_bench", width=xs, height=ys, steps=args.steps, warmup=args.warmup, reps=args.reps,
                prepare_once_env=os.environ.get("JXLHIP_PREPARE_ONCE"), modes=res)
    for name, d in (("repeat_ctx", dec), ("upload_ctx", up)):
        if hasattr(d, "prepare_launches"):
            line[name + "_prepares"] = list(d.prepare_launches())
    print(json.dumps(line))


if __name__ == "__main__":
    main()
