#!/usr/bin/env python3
"""djxl_hip.py IN.jxl OUT.{pfm,npy,ppm,pam} [--threads N] [--reps K] [--frames] [--display_nits N]
                                            [--output_primaries {srgb,p3,rec2100}] [--allow_partial_files]

Decodes a .jxl file (container or bare codestream, one VarDCT still frame) on an MI355X through
jxlhip_decode_codestream (include/jxl_hip_codestream.h) and writes the pixels the way djxl does for these
extensions (tools/djxl_main.cc, lib/extras/enc/pnm.cc):
  .pfm  linear-light float RGB, bottom-up rows, little endian (scale -1.0)
  .npy  float32 [H, W, 3] linear RGB (what tools/conformance/conformance.py reads, conformance.py:34-66)
  .ppm  8-bit RGB               .pam  8-bit RGBA (the image's alpha channel, opaque without one)
        -- both in the image's original colour encoding (its transfer function over its primaries; an ICC
           original: linear sRGB, like djxl without a CMS)
Photon noise (kNoise frames), splines (kSplines) and patches (kPatches behind their kReferenceOnly frames: what cjxl
writes for screenshots and text) are rendered on the device.  Streams outside the back-end (Modular frames, animation
...) exit with status 3 and the error text so that a
wrapper can fall back to libjxl's djxl.  Prints Mpx/s of the decode call like djxl's SpeedStats.
--frames: animations, layers, cropped and blended frames through jxlhip_decode_codestream_next: one file per DISPLAYED
frame, OUT-000.ext, OUT-001.ext ... (coalesced, like djxl); the frames are blended on the device in the encoding of the
output: the original's for .ppm / .pam (what the reference blends in), linear light for .pfm / .npy.  .pam writes every
displayed frame of an image with alpha as RGBA, its alpha blended with the colour (opaque without an alpha channel).
--display_nits N: the display's peak luminance, djxl's flag of that name (JxlDecoderSetDesiredIntensityTarget): a PQ
original mastered brighter is tone-mapped to it on the device (jxlhip_codestream_set_display).
--output_primaries: the pixels in these primaries (D65) instead of the original's, as JxlDecoderSetOutputColorProfile
with an enumerated encoding gives them; the transfer function stays the original's (its PQ curve keeps the
original's intensity target, as the reference's does).
--allow_partial_files: djxl's flag of that name: a file that ends early is rendered from what has arrived
(jxlhip_decode_codestream_partial: groups without AC from their DC, upsampled 8x on the device) and the three group
counts are printed; a file that ends before its DC groups exits with status 4.  Not with --frames."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def write(path, ext, px, w, h):
    if ext == ".npy":
        np.save(path, px)
    elif ext == ".pfm":
        with open(path, "wb") as f:
            f.write(b"PF\n%d %d\n-1.0\n" % (w, h))
            f.write(np.ascontiguousarray(px[::-1]).astype("<f4").tobytes())
    elif ext == ".ppm":
        with open(path, "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (w, h))
            f.write(px.tobytes())
    elif ext == ".pam":
        with open(path, "wb") as f:
            f.write(b"P7\nWIDTH %d\nHEIGHT %d\nDEPTH 4\nMAXVAL 255\nTUPLTYPE RGB_ALPHA\nENDHDR\n" % (w, h))
            f.write(px.tobytes())
    else:
        sys.exit("output must be .pfm, .npy, .ppm or .pam")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--frames", action="store_true")
    ap.add_argument("--display_nits", type=float, default=0.0)
    ap.add_argument("--output_primaries", choices=["srgb", "p3", "rec2100"])
    ap.add_argument("--allow_partial_files", action="store_true")
    a = ap.parse_args()
    if a.allow_partial_files and a.frames:
        sys.exit("--allow_partial_files renders single-frame files: not with --frames")
    import torch
    from libjxl_amd import VarDctDecoder, abi
    L = abi.load_library()
    blob = open(a.input, "rb").read()
    info = abi.CodestreamInfo()
    seq = abi.SequenceInfo()
    part = abi.PartialInfo()
    if a.frames:
        rc = L.jxlhip_codestream_sequence_info_ex(blob, len(blob), abi.SEQUENCE_EXTRA_CHANNELS, C.byref(info), C.byref(seq))
    elif a.allow_partial_files:
        rc = L.jxlhip_codestream_partial_info(blob, len(blob), C.byref(info), C.byref(part))
        if rc == abi.ERR_NEED_MORE_INPUT:
            sys.stderr.write(f"djxl_hip: {a.input}: {L.jxlhip_status_string(rc).decode()}\n")
            sys.exit(4)
    else:
        rc = L.jxlhip_codestream_basic_info(blob, len(blob), C.byref(info))
    if rc:
        sys.stderr.write(f"djxl_hip: {a.input}: {L.jxlhip_status_string(rc).decode()}\n")
        sys.exit(3 if rc == -7 else 1)
    orig_nits = info.intensity_target  # (the PQ curve of the output keeps it, whatever the display's peak)
    display = None
    if (a.display_nits or a.output_primaries) and a.allow_partial_files and not part.complete:
        sys.exit("--display_nits / --output_primaries need the whole file")  # (jxlhip_codestream_display_info reads it all)
    if a.display_nits or a.output_primaries:
        display = abi.Display(a.display_nits, {None: 0, "srgb": 1, "rec2100": 9, "p3": 11}[a.output_primaries],
                              1 if a.output_primaries else 0)
        why = C.c_char_p()
        rc = L.jxlhip_codestream_display_info(blob, len(blob), C.byref(display), C.byref(info), C.byref(why))
        if rc:
            sys.stderr.write(f"djxl_hip: {a.input}: {L.jxlhip_status_string(rc).decode()}: {(why.value or b'').decode()}\n")
            sys.exit(3 if rc == -7 else 1)
    ext = os.path.splitext(a.output)[1].lower()
    packed = ext in (".ppm", ".pam")
    R = C.CDLL(abi.runner_library_path())
    R.JxlThreadParallelRunnerCreate.restype = C.c_void_p
    R.JxlThreadParallelRunnerCreate.argtypes = [C.c_void_p, C.c_size_t]
    R.JxlThreadParallelRunnerDestroy.argtypes = [C.c_void_p]
    pool = R.JxlThreadParallelRunnerCreate(None, a.threads) if a.threads else None
    runner = C.cast(R.JxlThreadParallelRunner, C.c_void_p) if a.threads else None
    dec = VarDctDecoder(0)
    if display is not None:
        dec.set_display(a.display_nits, a.output_primaries)
    w, h = info.xsize, info.ysize
    if info.orientation >= 5:  # display orientation like djxl (JXLHIP_OUT_UNDO_ORIENTATION): transposed frame
        w, h = h, w
    UNDO = 0x100
    if packed:
        nc = 4 if ext == ".pam" else 3
        # 8-bit samples in the ORIGINAL colour encoding, like djxl: the original's transfer function over pixels in the
        # original's primaries (jxlhip_decode_codestream adapts the opsin inverse; the info struct names the rest)
        if info.gamma > 0:
            tf, par = 4, info.gamma
        else:
            tf, par = {8: (0, 0.0), 13: (1, 0.0), 16: (2, orig_nits), 1: (3, 0.0), 17: (4, 1 / 2.6),
                       18: (5, orig_nits)}.get(info.transfer_function, (1, 0.0))
        fmt = abi.OutputFormat(tf, 1, nc, 8, 0, par, info.luminances)
        out = torch.empty((h, w, nc), dtype=torch.uint8, device="cuda")
        args = (2 | UNDO, C.byref(fmt), out.data_ptr(), w * nc, 0)
    else:
        out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        args = (1 | UNDO, None, out.data_ptr(), w * 12, 0)
    if a.frames:
        args = (args[0] | abi.OUT_BLEND_EXTRA_CHANNELS,) + args[1:]  # (layers of an image with alpha are composited with it)
        stem, cursor, t0 = os.path.splitext(a.output)[0], C.c_uint64(0), time.perf_counter()
        for k in range(seq.num_displayed_frames):
            fr = abi.SequenceFrame()
            rc = L.jxlhip_decode_codestream_next(dec.ctx, runner, pool, blob, len(blob), C.byref(cursor), *args, C.byref(info),
                                                 C.byref(fr))
            if rc:
                sys.stderr.write(f"djxl_hip: {a.input}: frame {k}: {L.jxlhip_status_string(rc).decode()}: "
                                 f"{L.jxlhip_last_error(dec.ctx).decode()}\n")
                sys.exit(3 if rc == -7 else 1)
            write(f"{stem}-{k:03d}{ext}", ext, out.cpu().numpy(), w, h)
            print(f"frame {k}: duration {fr.duration} tick(s), {fr.coded_frames} coded frame(s)" + (" (last)" if fr.is_last else ""))
        dt = time.perf_counter() - t0
        print(f"{w} x {h}, {seq.num_displayed_frames} frame(s) of {seq.num_coded_frames} coded, "
              f"{w * h * seq.num_displayed_frames / dt / 1e6:.1f} MP/s [{a.threads} threads]")
        dec.close()
        if pool:
            R.JxlThreadParallelRunnerDestroy(pool)
        return
    best = None
    for _ in range(max(1, a.reps)):
        t0 = time.perf_counter()
        if a.allow_partial_files:
            if ext == ".pam" and info.num_extra_channels and not part.complete:
                sys.exit("a partial file of an image with extra channels: write .ppm, .pfm or .npy")
            rc = L.jxlhip_decode_codestream_partial(dec.ctx, runner, pool, blob, len(blob), *args, C.byref(info), C.byref(part))
        else:
            rc = L.jxlhip_decode_codestream(dec.ctx, runner, pool, blob, len(blob), *args, C.byref(info))
        dt = time.perf_counter() - t0
        if rc:
            sys.stderr.write(f"djxl_hip: {a.input}: {L.jxlhip_status_string(rc).decode()}: "
                             f"{L.jxlhip_last_error(dec.ctx).decode()}\n")
            sys.exit(3 if rc == -7 else 1)
        best = dt if best is None else min(best, dt)
    write(a.output, ext, out.cpu().numpy(), w, h)
    print(f"{w} x {h}, {w * h / best / 1e6:.1f} MP/s [{a.reps} reps, {a.threads} threads], "
          f"{info.num_groups} groups, {info.num_passes} pass(es), coefficients "
          f"{'int16' if info.coeff_type == 0 else 'int32'}, epf_iters {info.epf_iters} gab {info.gab}")
    if a.allow_partial_files:
        print(f"{'complete' if part.complete else 'partial'} file: {part.groups_complete} group(s) complete, "
              f"{part.groups_partial} partial, {part.groups_dc_only} DC only; {part.bytes_used} of {len(blob)} bytes drawn")
    dec.close()
    if pool:
        R.JxlThreadParallelRunnerDestroy(pool)


if __name__ == "__main__":
    main()
