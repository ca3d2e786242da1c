"""The two figures DESIGN.md section 3 "Modular frames" quotes.

(a) k_modular_emit on a synthetic 7680x4320 frame, int16 planes -> 8-bit RGB and int32 planes -> float RGB, and its
    sibling k_modular_planes, int16 planes + an int16 alpha plane -> 8-bit RGBA, every group with one RCT (YCoCg): run this under `rocprofv3 --kernel-trace --stats -- python tools/modular_bench.py --kernel`
    and read the kernel's time there (the call also uploads the planes, which is not the kernel's time); the script
    prints the bytes each launch must move.
(b) the jxlhip_codestream_phase_ms split of a lossless file (`--file`: oracle.feature_stream("modular", 2100, 300) by
    default), with 0 and 6 workers: what share of a file's decode is the host's entropy decode."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel(reps):
    import torch
    from libjxl_amd import VarDctDecoder, abi
    w, h, gd = 7680, 4320, 256
    dec = VarDctDecoder(0)
    L = dec.L
    rng = np.random.default_rng(1)
    ng = -(-w // gd) * -(-h // gd)
    rct = np.full(ng, 6, np.uint16)
    for dtype, kind, fmt, name, out_bytes in ((np.int16, 2, abi.OutputFormat(1, 1, 3, 8, 0, 0.0, (0.2126, 0.7152, 0.0722)), "int16 -> u8 RGB", 3),
                                             (np.int32, 1, None, "int32 -> f32 RGB", 12)):
        planes = rng.integers(0, 256, (3, h, w)).astype(dtype)
        m = abi.ModularFrame()
        m.xsize, m.ysize, m.stride_samples = w, h, w
        for c in range(3):
            m.planes[c] = planes[c].ctypes.data
        m.sample_type = abi.MODULAR_I16 if dtype == np.int16 else abi.MODULAR_I32
        m.bits_per_sample, m.group_dim, m.group_rct, m.global_rct = 8, gd, rct.ctypes.data, 0
        out = torch.empty(h * w * out_bytes, dtype=torch.uint8, device="cuda")
        for _ in range(reps):
            rc = L.jxlhip_decode_modular_frame(dec.ctx, C.byref(m), kind, C.byref(fmt) if fmt else None, out.data_ptr(), w * out_bytes, 0)
            assert rc == 0, L.jxlhip_last_error(dec.ctx)
            assert L.jxlhip_sync(dec.ctx) == 0
        moved = w * h * (3 * planes.itemsize + out_bytes) + ng * 2
        print("%s: %d launches of k_modular_emit, %.1f MB moved per launch (planes read + pixels written)" % (name, reps, moved / 1e6))
    # the sibling: the same int16 planes and an alpha plane of 8-bit values -> RGBA8 (12 bytes per pixel against 9)
    planes = rng.integers(0, 256, (4, h, w)).astype(np.int16)
    m = abi.ModularChannels()
    m.xsize, m.ysize, m.stride_samples, m.num_color = w, h, w, 3
    for c in range(3):
        m.planes[c] = planes[c].ctypes.data
    m.alpha_plane, m.alpha_bits = planes[3].ctypes.data, 8
    m.sample_type, m.bits_per_sample, m.group_dim, m.group_rct, m.global_rct = abi.MODULAR_I16, 8, gd, rct.ctypes.data, 0
    fmt = abi.OutputFormat(1, 1, 4, 8, 0, 0.0, (0.2126, 0.7152, 0.0722))
    out = torch.empty(h * w * 4, dtype=torch.uint8, device="cuda")
    for _ in range(reps):
        rc = L.jxlhip_decode_modular_channels(dec.ctx, C.byref(m), 2, C.byref(fmt), out.data_ptr(), w * 4, 0)
        assert rc == 0, L.jxlhip_last_error(dec.ctx)
        assert L.jxlhip_sync(dec.ctx) == 0
    moved = w * h * (4 * 2 + 4) + ng * 2
    print("int16 + alpha -> u8 RGBA: %d launches of k_modular_planes, %.1f MB moved per launch (planes read + pixels written)" % (reps, moved / 1e6))
    dec.close()


def file_phases(path, reps):
    from libjxl_amd import VarDctDecoder, abi
    import torch
    if path:
        cs = open(path, "rb").read()
    else:
        import oracle
        oracle.build()
        cs = oracle.feature_stream("modular", xsize=2100, ysize=300, seed=5, distance=1.0)
    dec = VarDctDecoder(0)
    L = dec.L
    info = abi.CodestreamInfo()
    assert L.jxlhip_codestream_basic_info(cs, len(cs), C.byref(info)) == 0 and info.modular == 1
    w, h = info.xsize, info.ysize
    fmt = abi.OutputFormat(1, 1, 3, 8, 0, 0.0, (0.2126, 0.7152, 0.0722))
    out = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    R = C.CDLL(abi.runner_library_path())
    R.JxlThreadParallelRunnerCreate.restype = C.c_void_p
    R.JxlThreadParallelRunnerCreate.argtypes = [C.c_void_p, C.c_size_t]
    R.JxlThreadParallelRunnerDestroy.argtypes = [C.c_void_p]
    names = ["headers", "dc_groups", "ac_global", "side_info", "groups (host entropy decode)", "extra_channels", "upload + kernel + sync"]
    for workers in (0, 6):
        pool = R.JxlThreadParallelRunnerCreate(None, workers) if workers else None
        runner = C.cast(R.JxlThreadParallelRunner, C.c_void_p) if workers else None
        best = None
        for _ in range(reps):
            t0 = time.perf_counter()
            rc = L.jxlhip_decode_codestream(dec.ctx, runner, pool, cs, len(cs), 2, C.byref(fmt), out.data_ptr(), w * 3, 0, C.byref(info))
            dt = (time.perf_counter() - t0) * 1e3
            assert rc == 0, L.jxlhip_last_error(dec.ctx)
            ms = (C.c_double * 7)()
            L.jxlhip_codestream_phase_ms(dec.ctx, ms)
            if best is None or dt < best[0]:
                best = (dt, list(ms))
        print("%dx%d, %d bytes, %d groups, %d workers: %.2f ms whole call (best of %d)" % (w, h, len(cs), info.num_groups, workers, best[0], reps))
        for n, v in zip(names, best[1]):
            if v:
                print("    %-30s %7.3f ms  %5.1f %%" % (n, v, 100 * v / sum(best[1])))
        if pool:
            R.JxlThreadParallelRunnerDestroy(pool)
    dec.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--file", nargs="?", const="", default=None)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.kernel:
        kernel(a.reps)
    if a.file is not None:
        file_phases(a.file, a.reps)
