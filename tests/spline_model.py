"""A numpy / python restatement of libjxl's spline rendering, independent of the product's code: QuantizedSpline::
Dequantize, Splines::InitializeDrawCache with the centripetal Catmull-Rom curve, the equally spaced points,
ContinuousIDCT / FastCosf and ComputeSegments (lib/jxl/splines.cc:55-758), and DrawSegment with FastErff
(:82-127; lib/jxl/base/fast_math-inl.h:97-157).  Float32 throughout, fmaf emulated through float64.
Quantized splines are dicts: start (x, y), deltas [(ddx, ddy), ...], color (3 x 32 ints), sigma (32 ints).
Test infrastructure."""
import math

import numpy as np

F32 = np.float32
F64 = np.float64
PI = math.pi
SQRT2 = F32(1.41421356237)
SQRT0_5 = F32(0.70710678118)
WEIGHT = [F32(0.0042), F32(0.075), F32(0.07), F32(0.3333)]
POS_LIMIT = 1 << 23


class SplineError(ValueError):
    """Where the reference's draw cache fails."""


def fma(a, b, c):
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def llround(v):
    """std::llround of a float as x86-64 evaluates it (out of range / NaN: INT64_MIN)."""
    v = float(v)
    if not abs(v) < 9.0e18:
        return -(1 << 63)
    return int(math.copysign(math.floor(abs(v) + 0.5), v))


def inv_adjusted_quant(adj):
    return F32(1) / (F32(1) + F32(0.125) * F32(adj)) if adj >= 0 else F32(1) - F32(0.125) * F32(adj)


def dequantize(q, adj, y_to_x, y_to_b, image_size, total):
    """-> (points [(x, y)], color (3, 32) f32, sigma (32,) f32, new total area); SplineError on the reference's
    failures."""
    area_limit = min(1024 * image_size + (1 << 32), 1 << 42)
    px, py = q["start"]
    if not (-POS_LIMIT < px < POS_LIMIT and -POS_LIMIT < py < POS_LIMIT):
        raise SplineError("start")
    pts = [(F32(px), F32(py))]
    cx, cy, dx, dy, manhattan = px, py, 0, 0, 0
    for ddx, ddy in q["deltas"]:
        dx += ddx
        dy += ddy
        manhattan += abs(dx) + abs(dy)
        if manhattan > area_limit:
            raise SplineError("manhattan")
        if not (-POS_LIMIT < dx < POS_LIMIT and -POS_LIMIT < dy < POS_LIMIT):
            raise SplineError("delta")
        cx += dx
        cy += dy
        if not (-POS_LIMIT < cx < POS_LIMIT and -POS_LIMIT < cy < POS_LIMIT):
            raise SplineError("position")
        pts.append((F32(cx), F32(cy)))
    iq = inv_adjusted_quant(adj)
    qc = np.asarray(q["color"], np.int64).reshape(3, 32)
    qs = np.asarray(q["sigma"], np.int64).reshape(32)
    f = np.ones(32, F32)
    f[0] = SQRT0_5
    color = np.stack([qc[c].astype(F32) * f * WEIGHT[c] * iq for c in range(3)])
    color[0] = color[0] + F32(y_to_x) * color[1]
    color[2] = color[2] + F32(y_to_b) * color[1]
    csum = [sum(int(math.ceil(F32(iq * F32(abs(int(v)))))) for v in qc[c]) for c in range(3)]
    csum[0] += int(math.ceil(abs(F32(y_to_x)))) * csum[1]
    csum[2] += int(math.ceil(abs(F32(y_to_b)))) * csum[1]
    logcolor = max(1, max(csum).bit_length())
    wl = F32(math.ceil(np.sqrt(F32(F32(area_limit) / F32(logcolor)) / F32(max(1, manhattan)))))
    sigma = qs.astype(F32) * f * WEIGHT[3] * iq
    width = 0
    for v in qs:
        wf = F32(math.ceil(F32(iq * F32(abs(int(v))))))
        w = int(min(wl, max(F32(1), wf)))
        width += w * w * logcolor
    total += width * manhattan
    if total > area_limit:
        raise SplineError("area")
    return pts, color, sigma, total


def catmull_rom(p):
    p = list(p)
    if len(p) == 1:
        return [p[0]]

    def add(a, b):
        return (F32(a[0] + b[0]), F32(a[1] + b[1]))

    def sub(a, b):
        return (F32(a[0] - b[0]), F32(a[1] - b[1]))

    def mul(k, v):
        return (F32(k * v[0]), F32(k * v[1]))
    p = [add(p[0], sub(p[0], p[1]))] + p + [add(p[-1], sub(p[-1], p[-2]))]
    out = []
    for s in range(len(p) - 3):
        q = p[s:s + 4]
        out.append(q[1])
        d, t = [], [F32(0)]
        for k in range(3):
            v = sub(q[k + 1], q[k])
            d.append(F32(np.sqrt(F32(math.hypot(float(v[0]), float(v[1]))))))
            t.append(F32(t[k] + d[k]))
        for i in range(1, 16):
            tt = F32(d[0] + F32(F32(i) / F32(16)) * d[1])
            a = [add(q[k], mul(F32((tt - t[k]) / d[k]), sub(q[k + 1], q[k]))) for k in range(3)]
            b = [add(a[k], mul(F32((tt - t[k]) / F32(d[k] + d[k + 1])), sub(a[k + 1], a[k]))) for k in range(2)]
            out.append(add(b[0], mul(F32((tt - t[1]) / d[1]), sub(b[1], b[0]))))
    out.append(p[-2])
    return out


def equally_spaced(pts):
    cur = pts[0]
    out = [(cur, F32(1))]
    nxt = 0
    while nxt != len(pts):
        prev, acc = cur, F32(0)
        while True:
            if nxt == len(pts):
                out.append((prev, acc))
                return out
            vx, vy = F32(pts[nxt][0] - prev[0]), F32(pts[nxt][1] - prev[1])
            to_next = F32(np.sqrt(F32(F32(vx * vx) + F32(vy * vy))))
            if F32(acc + to_next) >= F32(1):
                f = F32(F32(F32(1) - acc) / to_next)
                cur = (F32(prev[0] + F32(f * vx)), F32(prev[1] + F32(f * vy)))
                out.append((cur, F32(1)))
                break
            acc = F32(acc + to_next)
            prev = pts[nxt]
            nxt += 1
    return out


def fast_cos(x):
    x = np.asarray(x, F32)
    pi2, pi2_inv = F32(PI * 2.0), F32(0.5 / PI)
    xm = (x - np.floor(x * pi2_inv) * pi2).astype(F32)
    x_pi = np.minimum(xm, (pi2 - xm).astype(F32))
    above = x_pi >= F32(PI / 2.0)
    xh = np.where(above, (F32(PI) - x_pi).astype(F32), x_pi)
    xs = (xh * F32(0.25)).astype(F32)
    x2 = (xs * xs).astype(F32)
    x4 = (x2 * x2).astype(F32)
    pre = fma(x4, F32(0.06960438), fma(x2, F32(-0.84087373), F32(1.68179268)))
    s1 = fma(pre, pre, F32(-1.414213562))
    s2 = fma(s1, s1, F32(-1))
    return np.where(above, -s2, s2).astype(F32)


def idct(dct, t):
    """ContinuousIDCT at every t (an array)."""
    th = (np.asarray(t, F32) + F32(0.5)).astype(F32)
    r = np.zeros_like(th)
    for i in range(32):
        local = (F32(dct[i]) * fast_cos((F32(PI / 32 * i) * th).astype(F32))).astype(F32)
        r = fma(SQRT2, local, r)
    return r


def segments(splines, adj, xsize, ysize, y_to_x=0.0, y_to_b=1.0):
    """The draw list: a list of dicts (center_x, center_y, inv_sigma, sigma_over_4_times_intensity, color,
    maximum_distance, y0, y1) in DrawSegments order."""
    total, deq = 0, []
    for q in splines:
        pts, color, sigma, total = dequantize(q, adj, y_to_x, y_to_b, xsize * ysize, total)
        if any(pts[i] == pts[i + 1] for i in range(len(pts) - 1)):
            raise SplineError("identical successive points")
        deq.append((pts, color, sigma))
    out = []
    log01 = F32(F32(math.log(F32(0.1))) * F32(5))  # kDistanceExp = 5: JXL_HIGH_PRECISION, the default build
    for pts, color, sigma in deq:
        draw = equally_spaced(catmull_rom(pts))
        arc = F32(F32(len(draw) - 2) + draw[-1][1])
        if arc <= 0:
            continue
        inv_arc = F32(F32(1) / arc)
        prog = np.minimum(F32(1), (np.arange(len(draw)).astype(F32) * inv_arc).astype(F32))
        t = (F32(31) * prog).astype(F32)
        cols = [idct(color[c], t) for c in range(3)]
        sig = idct(sigma, t)
        for k, (pt, mult) in enumerate(draw):
            s, col = sig[k], [cols[c][k] for c in range(3)]
            with np.errstate(all="ignore"):
                if not (np.isfinite(s) and s != 0 and np.isfinite(F32(1) / s) and np.isfinite(mult)):
                    continue
                mc = F32(0.01)
                for c in range(3):
                    mc = max(mc, abs(F32(col[c] * mult)))
                md = F32(np.sqrt(F32(F32(F32(F32(-2) * s) * s) * F32(log01 - F32(math.log(mc))))))
            y0 = max(llround(F32(pt[1] - md)), 0)
            y1 = llround(F32(pt[1] + md)) + 1
            y1 = min(y1, ysize)
            if y1 <= y0:
                continue
            out.append(dict(center_x=pt[0], center_y=pt[1], inv_sigma=F32(F32(1) / s),
                            sigma_over_4_times_intensity=F32(F32(F32(0.25) * s) * mult), color=col,
                            maximum_distance=md, y0=y0, y1=y1))
    return out


def fast_erf(x):
    x = np.asarray(x, F32)
    ax = np.abs(x)
    d1 = fma(ax, F32(7.77394369e-02), F32(2.05260015e-04))
    d2 = fma(d1, ax, F32(2.32120216e-01))
    d3 = fma(d2, ax, F32(2.77820801e-01))
    d4 = fma(d3, ax, F32(1))
    d5 = (d4 * d4).astype(F32)
    inv = (F32(1) / d5).astype(F32)
    r = fma(-inv, inv, F32(1))
    return np.where(x <= 0, -r, r).astype(F32)


def draw(planes, segs):
    """planes (3, ysize, xsize) float32 with every segment added, segment after segment (DrawSegment)."""
    out = np.array(planes, F32, copy=True)
    _, ys, xs = out.shape
    for g in segs:
        start = llround(F32(g["center_x"] - g["maximum_distance"]))
        end = llround(F32(g["center_x"] + g["maximum_distance"]))
        if end < 0 or start >= xs:
            continue
        x0, x1 = max(start, 0), min(end + 1, xs)
        xx = np.arange(x0, x1).astype(F32)[None, :]
        yy = np.arange(g["y0"], g["y1"]).astype(F32)[:, None]
        dx = (xx - F32(g["center_x"])).astype(F32)
        dy = (yy - F32(g["center_y"])).astype(F32)
        d = np.sqrt(fma(dx, dx, (dy * dy).astype(F32))).astype(F32)
        inv = F32(g["inv_sigma"])
        f = (fast_erf((fma(d, F32(0.5), F32(0.353553391)) * inv).astype(F32)) -
             fast_erf((fma(d, F32(0.5), F32(-0.353553391)) * inv).astype(F32))).astype(F32)
        li = (F32(g["sigma_over_4_times_intensity"]) * (f * f).astype(F32)).astype(F32)
        for c in range(3):
            sl = out[c, g["y0"]:g["y1"], x0:x1]
            out[c, g["y0"]:g["y1"], x0:x1] = fma(F32(g["color"][c]), li, sl)
    return out
