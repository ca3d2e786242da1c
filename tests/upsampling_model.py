"""The upsampling stage (FrameHeader::upsampling = 2, 4, 8; lib/jxl/render_pipeline/stage_upsampling.cc) restated in
numpy, as a checker of kernels_upsample.hip: the expansion of the 15 / 55 / 210 coded weights to N x N kernels of
5 x 5 taps, the 2-pixel border mirrored at the edge of the CODED frame (lib/jxl/image_ops.h:184-196, applied repeatedly
when the frame is narrower than the border), the 25-tap sum in the reference's order -- three accumulators over taps
i, i + 1, i + 2 with fused multiply-adds, (acc1 + acc2) + acc0 -- and the clamp to the neighbourhood's range.  One
function for every N.  Test infrastructure."""
import os
import re

import numpy as np

F32 = np.float32
NUM_WEIGHTS = {2: 15, 4: 55, 8: 210}


def default_weights(n):
    """The format's default weights of factor n (libjxl_amd/csrc/upsampling_constants.inc: data)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "libjxl_amd", "csrc", "upsampling_constants.inc")).read()
    m = re.search(r"kUpsampling%dWeights\[%d\]\s*=\s*\{(.*?)\};" % (n, NUM_WEIGHTS[n]), text, flags=re.S)
    w = np.array([float(t.rstrip("f")) for t in re.findall(r"-?\d+\.\d*(?:e[-+]?\d+)?f", m.group(1))], F32)
    assert w.size == NUM_WEIGHTS[n]
    return w


def kernels(n, weights):
    """[n * n, 25]: kernel (oy * n + ox) of output pixel (ox, oy) inside a coded pixel, taps row-major over the 5 x 5
    neighbourhood.  The coded weights are the upper triangle of a symmetric matrix of 5n/2 x 5n/2 entries that holds
    the top-left quarter of the kernels; the other quarters are its mirror images."""
    w = np.asarray(weights, F32)
    assert w.size == NUM_WEIGHTS[n], w.size
    h = n // 2
    k = np.zeros((n * n, 25), F32)
    for ky in range(h):
        for kx in range(h):
            for py in range(5):
                for px in range(5):
                    j, i = 5 * ky + py, 5 * kx + px
                    my, mx = min(i, j), max(i, j)
                    v = w[5 * h * my - my * (my - 1) // 2 + mx - my]
                    k[ky * n + kx, py * 5 + px] = v
                    k[ky * n + (n - 1 - kx), py * 5 + (4 - px)] = v
                    k[(n - 1 - ky) * n + kx, (4 - py) * 5 + px] = v
                    k[(n - 1 - ky) * n + (n - 1 - kx), (4 - py) * 5 + (4 - px)] = v
    return k


def _mirror(i, n):
    while i < 0 or i >= n:
        i = -i - 1 if i < 0 else 2 * n - 1 - i
    return i


def _fma(a, b, c):
    # (a float32 product is exact in float64, the sum is rounded once more to float32: double rounding can differ from
    # a true fused multiply-add by one ulp in rare ties -- far inside the 1e-5 these planes are compared with)
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def upsample(planes, n, weights=None, out_size=None, kernel_table=None, clamp=True):
    """planes: [C, ch, cw] float32 at coded size -> [C, H, W] at out_size = (W, H) (default n * cw, n * ch), where
    ceil(W / n) == cw and ceil(H / n) == ch: upsampled, then cropped.  kernel_table ([n * n, 25], in place of
    kernels(n, weights)) and clamp=False are for tests that damage the model on purpose."""
    planes = np.asarray(planes, F32)
    nc, ch, cw = planes.shape
    W, H = out_size if out_size is not None else (n * cw, n * ch)
    assert -(-W // n) == cw and -(-H // n) == ch, (W, H, n, cw, ch)
    k = kernels(n, default_weights(n) if weights is None else weights) if kernel_table is None else kernel_table
    assert k.shape == (n * n, 25) and k.dtype == F32
    ys = np.array([_mirror(i, ch) for i in range(-2, ch + 2)])
    xs = np.array([_mirror(i, cw) for i in range(-2, cw + 2)])
    p = planes[:, ys][:, :, xs]
    taps = [p[:, i // 5:i // 5 + ch, i % 5:i % 5 + cw] for i in range(25)]
    lo = np.minimum.reduce(taps)
    hi = np.maximum.reduce(taps)
    out = np.zeros((nc, n * ch, n * cw), F32)
    for oy in range(n):
        for ox in range(n):
            kk = k[oy * n + ox]
            acc = [taps[i] * kk[i] for i in range(3)]
            for i in range(3, 24, 3):
                for a in range(3):
                    acc[a] = _fma(taps[i + a], kk[i + a], acc[a])
            acc[0] = _fma(taps[24], kk[24], acc[0])
            r = (acc[1] + acc[2]) + acc[0]
            out[:, oy::n, ox::n] = np.minimum(np.maximum(r, lo), hi) if clamp else r
    return out[:, :H, :W]
