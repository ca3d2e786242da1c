"""A numpy restatement of libjxl's photon-noise rendering, independent of the product's kernels: the random planes of
PrepareNoiseInput (lib/jxl/dec_noise.cc:58-151) from a step-by-step Xorshift128+ seeded through SplitMix64
(lib/jxl/xorshift128plus-inl.h:28-86), ConvolveNoiseStage and AddNoiseStage (lib/jxl/render_pipeline/stage_noise.cc).
Test infrastructure."""
import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
F32 = np.float32


def splitmix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def seed(s1, s2, s3, s4):
    """Xorshift128Plus(seed1..seed4): the 8 lanes' (s0, s1) as python ints."""
    a = [splitmix64((((s1 << 32) + s2) + GOLDEN) & M64)]
    b = [splitmix64((((s3 << 32) + s4) + GOLDEN) & M64)]
    for _ in range(7):
        a.append(splitmix64(a[-1]))
        b.append(splitmix64(b[-1]))
    return a, b


def step(a, b):
    """One Fill on python ints: returns the 8 lanes' bits, advances the state in place."""
    bits = []
    for i in range(8):
        s1, s0 = a[i], b[i]
        bits.append((s1 + s0) & M64)
        a[i] = s0
        s1 ^= (s1 << 23) & M64
        b[i] = s1 ^ s0 ^ (s1 >> 18) ^ (s0 >> 5)
    return bits


def random_planes(xsize, ysize, visible=1, nonvisible=0):
    """The three random planes [3, ysize, xsize] float32 in [1, 2), generated group by group in the reference's
    serial order (all groups' generators step together, one numpy array lane per group and generator lane)."""
    xsg, ysg = (xsize + 255) // 256, (ysize + 255) // 256
    groups = [(gx, gy) for gy in range(ysg) for gx in range(xsg)]
    a = np.zeros((len(groups), 8), np.uint64)
    b = np.zeros((len(groups), 8), np.uint64)
    dims = []
    for i, (gx, gy) in enumerate(groups):
        sa, sb = seed(visible, nonvisible, gx * 256, gy * 256)
        a[i], b[i] = sa, sb
        w, h = min(256, xsize - 256 * gx), min(256, ysize - 256 * gy)
        dims.append((w, h, (w + 15) // 16))
    nsteps = max(3 * h * f for w, h, f in dims)
    bits = np.empty((nsteps, len(groups), 8), np.uint64)
    with np.errstate(over="ignore"):
        for s in range(nsteps):
            s1, s0 = a, b
            bits[s] = s1 + s0
            t = s1 ^ (s1 << np.uint64(23))
            a = s0
            b = t ^ s0 ^ (t >> np.uint64(18)) ^ (s0 >> np.uint64(5))
    out = np.zeros((3, ysize, xsize), np.float32)
    for i, (gx, gy) in enumerate(groups):
        w, h, f = dims[i]
        g = np.ascontiguousarray(bits[:3 * h * f, i, :])  # [fill][lane]
        u32 = g.view(np.uint32).reshape(3, h, f * 16)   # little endian: lane i = floats 2i (low), 2i + 1 (high)
        fl = ((u32 >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32)
        out[:, gy * 256:gy * 256 + h, gx * 256:gx * 256 + w] = fl[:, :, :w]
    return out


def _mirror(n, i):
    while i < 0 or i >= n:
        i = -i - 1 if i < 0 else 2 * n - 1 - i
    return i


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def convolve(plane):
    """ConvolveNoiseStage on one plane, mirrored at the image edge, its order of additions."""
    h, w = plane.shape
    ys = np.array([_mirror(h, i) for i in range(-2, h + 2)])
    xs = np.array([_mirror(w, i) for i in range(-2, w + 2)])
    p = plane[ys][:, xs]

    def at(dy, dx):
        return p[2 + dy:2 + dy + h, 2 + dx:2 + dx + w]
    others = np.zeros((h, w), np.float32)
    for i in range(-2, 3):
        for dy in (-2, -1, 1, 2):
            others = others + at(dy, i)
    for dx in (-2, -1, 1, 2):
        others = others + at(0, dx)
    return _fma(others, F32(0.16), at(0, 0) * F32(-3.84))


def strength(lut, x, clamp=True):
    """NoiseStrength; clamp=False leaves out its final clamp to [0, 1] (for tests that count where it decides)."""
    lut = np.asarray(lut, np.float32)
    scaled = np.maximum(F32(0), x * F32(6))
    fl = np.floor(scaled)
    fr = scaled - fl
    big = scaled >= 7
    fl = np.where(big, F32(6), fl)
    fr = np.where(big, F32(1), fr).astype(np.float32)
    i = fl.astype(np.int64)
    lo, hi = lut[i], lut[i + 1]
    v = _fma(hi - lo, fr, lo)
    return np.clip(v, 0, 1).astype(np.float32) if clamp else v


def add_noise(xyb, lut, ytox, ytob, visible=1, nonvisible=0):
    """The XYB planes [3, H, W] after ConvolveNoise + AddNoise."""
    _, h, w = xyb.shape
    rnd = random_planes(w, h, visible, nonvisible)
    nr, ng, nc = [convolve(rnd[c]) * F32(0.22) for c in range(3)]
    vx, vy, vb = [xyb[c].astype(np.float32) for c in range(3)]
    sg = strength(lut, (vy - vx) * F32(0.5))
    sr = strength(lut, (vy + vx) * F32(0.5))
    red = sr * _fma(F32(0.0078125), nr, F32(0.9921875) * nc)
    green = sg * _fma(F32(0.0078125), ng, F32(0.9921875) * nc)
    rg = red + green
    return np.stack([_fma(F32(ytox), rg, red - green) + vx, vy + rg, _fma(F32(ytob), rg, vb)])
