"""Splines in the host front-end (CPU): spline frames written by the reference encoder (oracle.feature_stream("splines"),
its custom_splines) through jxlhip_splines_decode -- the bundle at the head of the DC-global section
(Splines::Decode, lib/jxl/splines.cc:600-642) -- and on through the DC-global fields, the DC groups, the AC global
section and every AC group; the draw list (jxlhip_splines_segments) against tests/spline_model.py on the streams'
splines and on built sets; and the failures the reference reports.

At distance 1.0 the reference encoder writes no splines into frames above about a megapixel (its streaming path skips
them), so the 2200 x 520 stream is written at distance 3.0."""
import ctypes as C

import numpy as np
import pytest

from libjxl_amd import abi

import spline_model as sm

FLAG_NOISE, FLAG_PATCHES, FLAG_SPLINES = 1, 2, 16
BAD = -5
SIZES = [((600, 400), 1.0), ((777, 333), 1.0), ((2200, 520), 3.0)]


@pytest.fixture(scope="module")
def ref(oracle):
    if not oracle.ref_available():
        pytest.skip("oracle/_ref not available")
    oracle.ref_lib()
    return oracle


@pytest.fixture(scope="module")
def L():
    return abi.load_library()


class _Stream:
    def __init__(self, cs):
        self.codestream = np.frombuffer(cs, np.uint8)


def encoder_splines(xs, ys):
    """The splines FeatureStream hands the encoder (oracle/ref_real_stream.cc), float32 as there: control points and
    the colour / sigma DCT inputs."""
    f = np.float32
    out = []
    for k in range(2):
        pts = [(f(xs) * (f(0.1) + f(0.2) * f(i)),
                f(ys) * ((f(0.25) + f(0.1) * f((i * 3) % 4)) if k else (f(0.8) - f(0.12) * f((i * 2) % 5))))
               for i in range(5)]
        color = np.zeros((3, 32), np.float32)
        sigma = np.zeros(32, np.float32)
        color[1][0] = 0.35 if k else 0.2
        color[0][0] = 0.01 if k else -0.02
        color[2][0] = 0.1 if k else 0.25
        color[1][1] = 0.05
        sigma[0] = 4.5 if k else 3.0
        sigma[1] = 0.5
        out.append((pts, color, sigma))
    return out


def control_points(q):
    x, y = q["start"]
    pts, dx, dy = [(x, y)], 0, 0
    for ddx, ddy in q["deltas"]:
        dx, dy = dx + ddx, dy + ddy
        x, y = x + dx, y + dy
        pts.append((x, y))
    return pts


def decode_bundle(L, ref, xs, ys, distance):
    from test_dc_groups import parse_to_sections
    cs = ref.feature_stream("splines", xsize=xs, ysize=ys, seed=5, distance=distance)
    _, _, fh, sections = parse_to_sections(L, _Stream(cs))
    assert fh.flags & FLAG_SPLINES
    s0 = sections[0]
    h, pos = C.c_void_p(), C.c_size_t(0)
    assert L.jxlhip_splines_decode(s0.ctypes.data, len(s0), C.byref(pos), xs * ys, C.byref(h)) == 0
    return cs, fh, sections, h, pos.value


def side_info_from(L, fh, sections, start):
    """decode_side_info (tests/test_dc_groups.py) with the DC-global fields read from behind the splines bundle."""
    s0 = sections[0]
    dcg, dpos = abi.DcGlobal(), C.c_size_t(start)
    assert L.jxlhip_dc_global_decode(s0.ctypes.data, len(s0), C.byref(dpos), fh.flags & ~FLAG_SPLINES,
                                     C.byref(dcg)) == 0
    tree = C.c_void_p()
    assert L.jxlhip_modular_global_decode(s0.ctypes.data, len(s0), C.byref(dpos), C.byref(fh), C.byref(tree)) == 0
    assert (dpos.value + 7) // 8 == len(s0)
    xsb, ysb = fh.xsize_blocks, fh.ysize_blocks
    qdc = [np.zeros(xsb * ysb, np.int32) for _ in range(3)]
    acs = np.zeros(xsb * ysb, np.uint8)
    rq = np.zeros(xsb * ysb, np.int32)
    sharp = np.zeros(xsb * ysb, np.uint8)
    cw, chh = (xsb + 7) // 8, (ysb + 7) // 8
    ytox, ytob = np.zeros(cw * chh, np.int8), np.zeros(cw * chh, np.int8)
    used = C.c_uint32(0)
    try:
        for g in range(int(fh.num_dc_groups)):
            d = sections[1 + g]
            gp, ep = C.c_size_t(0), C.c_uint32(0)
            ptrs = (C.c_void_p * 3)(*[q.ctypes.data for q in qdc])
            assert L.jxlhip_dc_group_decode(tree, d.ctypes.data, len(d), C.byref(gp), C.byref(fh), g, ptrs,
                                            C.byref(ep), acs.ctypes.data, rq.ctypes.data, sharp.ctypes.data,
                                            ytox.ctypes.data, ytob.ctypes.data, C.byref(used)) == 0, g
            assert (gp.value + 7) // 8 == len(d)
    finally:
        L.jxlhip_modular_tree_destroy(tree)
    return qdc, acs, rq, used.value


def compare_segments(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert (a.y0, a.y1) == (b["y0"], b["y1"])
        for name in ("center_x", "center_y", "inv_sigma", "sigma_over_4_times_intensity", "maximum_distance"):
            assert abs(getattr(a, name) - b[name]) <= 1e-6 * abs(b[name]), name
        for c in range(3):
            assert abs(a.color[c] - b["color"][c]) <= 1e-6 * abs(b["color"][c]) + 1e-12


@pytest.mark.parametrize("size,distance", SIZES)
def test_spline_stream_through_the_front_end(L, ref, size, distance):
    xs, ys = size
    _, fh, sections, h, end = decode_bundle(L, ref, xs, ys, distance)
    s0 = sections[0]
    try:
        # the DC-global fields from behind the bundle: the same struct as a spline-free read of the same section
        dcg, pos = abi.DcGlobal(), C.c_size_t(end)
        assert L.jxlhip_dc_global_decode(s0.ctypes.data, len(s0), C.byref(pos), fh.flags & ~FLAG_SPLINES,
                                         C.byref(dcg)) == 0
        assert dcg.global_scale > 0 and dcg.quant_dc > 0
        # the spline flag itself is still refused by the DC-global decode
        p2 = C.c_size_t(end)
        assert L.jxlhip_dc_global_decode(s0.ctypes.data, len(s0), C.byref(p2), fh.flags, C.byref(abi.DcGlobal())) == -7
        adj, q = abi.splines_quantized(h)
        assert adj == 0 and len(q) == 2
        for sp, (pts, color, sigma) in zip(q, encoder_splines(xs, ys)):
            assert control_points(sp) == [(sm.llround(x), sm.llround(y)) for x, y in pts]  # std::round: half away
            _, dc, ds, _ = sm.dequantize(sp, adj, dcg.cfl_base_x, dcg.cfl_base_b, xs * ys, 0)
            steps = np.array([sm.WEIGHT[c] for c in range(3)], np.float32)[:, None]
            assert np.all(np.abs(dc - color) <= steps * 1.0001)
            assert np.all(np.abs(ds - sigma) <= sm.WEIGHT[3] * 1.0001)
        rc, segs = abi.splines_segments(h, xs, ys, dcg.cfl_base_x, dcg.cfl_base_b)
        assert rc == 0 and len(segs) > 100
        compare_segments(segs, sm.segments(q, adj, xs, ys, dcg.cfl_base_x, dcg.cfl_base_b))
    finally:
        abi.splines_destroy(h)
    # from the returned bit position on: the modular global info consumes the section exactly, then the DC groups, the
    # AC global section and every AC group decode
    qdc, acs, rq, used = side_info_from(L, fh, sections, end)
    xsb, ysb, ng, ndc = fh.xsize_blocks, fh.ysize_blocks, int(fh.num_groups), int(fh.num_dc_groups)
    qctx = np.zeros(xsb * ysb, np.uint8)
    qp = (C.c_void_p * 3)(*[q.ctypes.data for q in qdc])
    assert L.jxlhip_quant_dc_contexts(C.byref(dcg.block_ctx_map), xsb * ysb, qp, qctx.ctypes.data) == 0
    glob = sections[1 + ndc]
    encs = abi.QuantEncodings()
    nh, bits, hs = C.c_uint32(0), C.c_size_t(0), (C.c_void_p * fh.num_passes)()
    assert L.jxlhip_ac_global_decode(glob.ctypes.data, len(glob), ng, fh.num_passes, used,
                                     C.byref(dcg.block_ctx_map), C.byref(encs), C.byref(nh), hs, C.byref(bits)) == 0
    coeffs = [np.zeros(ng * 65536, np.int32) for _ in range(3)]
    try:
        xsg = int(fh.xsize_groups)
        for g in range(ng):
            ptrs = (C.c_void_p * 3)(*[o[g * 65536:].ctypes.data for o in coeffs])
            for ps in range(fh.num_passes):
                d = sections[2 + ndc + ps * ng + g]
                gp, cnt = C.c_size_t(0), C.c_size_t(0)
                assert L.jxlhip_ac_group_decode(hs[ps], xsb, ysb, g % xsg, g // xsg, acs.ctypes.data, rq.ctypes.data,
                                                qctx.ctypes.data, d.ctypes.data, len(d), C.byref(gp), fh.shift[ps], 1,
                                                ptrs, C.byref(cnt)) == 0, (g, ps)
    finally:
        for hh in hs:
            L.jxlhip_ac_pass_destroy(hh)
    assert any(np.count_nonzero(c) for c in coeffs)


def test_codestream_basic_info_accepts_a_spline_stream(L, ref):
    cs = ref.feature_stream("splines")
    info = abi.CodestreamInfo()
    assert L.jxlhip_codestream_basic_info(cs, len(cs), C.byref(info)) == 0


def test_truncated_bundle_is_bad(L, ref):
    from test_dc_groups import parse_to_sections
    _, _, fh, sections = parse_to_sections(L, _Stream(ref.feature_stream("splines")))
    s0 = sections[0]
    h, pos = C.c_void_p(), C.c_size_t(0)
    assert L.jxlhip_splines_decode(s0.ctypes.data, len(s0), C.byref(pos), 600 * 400, C.byref(h)) == 0
    end = pos.value
    abi.splines_destroy(h)
    for nbytes in (1, 4, end // 16, end // 8 - 1):
        p = C.c_size_t(0)
        assert L.jxlhip_splines_decode(s0.ctypes.data, nbytes, C.byref(p), 600 * 400, C.byref(h)) == BAD, nbytes
        assert p.value == 0 and not h.value
    # the control-point cap: min(2^20, pixels / 2) -- two splines of 5 points do not fit into 8 pixels
    p = C.c_size_t(0)
    assert L.jxlhip_splines_decode(s0.ctypes.data, len(s0), C.byref(p), 8, C.byref(h)) == BAD


def spline(start, deltas, y=40, x=2, b=10, sigma=12, sigma1=0):
    color = np.zeros((3, 32), np.int64)
    color[0][0], color[1][0], color[2][0] = x, y, b
    color[1][1] = 3
    s = np.zeros(32, np.int64)
    s[0], s[1] = sigma, sigma1
    return dict(start=start, deltas=deltas, color=color.tolist(), sigma=s.tolist())


def path(points):
    """Delta-deltas of a list of integer control points."""
    out, pdx, pdy = [], 0, 0
    for (x0, y0), (x1, y1) in zip(points, points[1:]):
        dx, dy = x1 - x0, y1 - y0
        out.append((dx - pdx, dy - pdy))
        pdx, pdy = dx, dy
    return points[0], out


def built_sets(xs, ys):
    edge = [spline(*path([(-30, 20), (xs // 2, -25), (xs + 30, ys // 3)])),
            spline(*path([(xs + 20, ys - 10), (xs // 3, ys + 25), (-40, ys // 2)]), y=-30, b=-20),
            spline(*path([(5, -50), (8, ys // 2), (3, ys + 50)]), sigma=20)]
    tiny = [spline(*path([(10, 10), (xs - 10, ys - 10)]), sigma=1),
            spline(*path([(xs - 12, 7), (15, ys - 3), (xs // 2, ys // 2)]), sigma=2, sigma1=-1)]
    large = [spline(*path([(xs // 4, ys // 4), (3 * xs // 4, ys // 2), (xs // 2, 3 * ys // 4)]), sigma=400, y=12)]
    single = [spline((xs // 2, ys // 2), [])]
    return dict(edge=edge, tiny=tiny, large=large, single=single)


@pytest.mark.parametrize("name", ["edge", "tiny", "large", "single"])
@pytest.mark.parametrize("size", [(61, 70), (300, 520)])
@pytest.mark.parametrize("adj", [0, 3, -2])
def test_built_sets_match_the_model(L, name, size, adj):
    xs, ys = size
    sets = built_sets(xs, ys)
    rc, h = abi.splines_from_quantized(sets[name], adj)
    assert rc == 0
    try:
        rc, segs = abi.splines_segments(h, xs, ys, 0.1, 0.9)
        assert rc == 0
        want = sm.segments(sets[name], adj, xs, ys, 0.1, 0.9)
        compare_segments(segs, want)
        if name == "single":
            assert len(segs) == 0  # one control point draws nothing
        else:
            assert len(segs) > 0
        if name == "tiny":
            assert all(s.maximum_distance < 8 for s in segs)
        if name == "large":
            assert max(s.maximum_distance for s in segs) > 200
        # the round trip through the read-out
        adj2, q = abi.splines_quantized(h)
        assert adj2 == adj and [c["start"] for c in q] == [tuple(s["start"]) for s in sets[name]]
    finally:
        abi.splines_destroy(h)


def _segments_rc(L, splines, xs=300, ys=200, adj=0):
    rc, h = abi.splines_from_quantized(splines, adj)
    if rc:
        return rc
    try:
        rc, _ = abi.splines_segments(h, xs, ys, 0.0, 1.0)
        return rc
    finally:
        abi.splines_destroy(h)


def test_failures_are_bad_stream(L):
    ok = spline(*path([(10, 10), (100, 50), (200, 20)]))
    assert _segments_rc(L, [ok]) == 0
    # identical successive control points
    assert _segments_rc(L, [spline(*path([(10, 10), (100, 50), (100, 50), (200, 20)]))]) == BAD
    with pytest.raises(sm.SplineError):
        sm.segments([spline(*path([(10, 10), (100, 50), (100, 50)]))], 0, 300, 200)
    # coordinates at or beyond +-2^23: a starting point, and a point reached through the deltas
    assert _segments_rc(L, [spline((1 << 23, 5), [(1, 1)])]) == BAD
    assert _segments_rc(L, [spline((5, -(1 << 23)), [(1, 1)])]) == BAD
    assert _segments_rc(L, [spline((5, 5), [((1 << 23) - 6, 0)])]) == BAD
    # delta-deltas at 2^30 and INT_MIN in a DCT value are refused when the object is built
    assert _segments_rc(L, [spline((5, 5), [(1 << 30, 0)])]) == BAD
    bad = spline((5, 5), [(1, 1)])
    bad["sigma"][3] = -(1 << 31)
    assert _segments_rc(L, [bad]) == BAD
    # the manhattan-distance limit min(1024 * pixels + 2^32, 2^42): a long zig-zag in a 4 x 4 frame
    zig = [(0, 0)] + [((i % 2) * 4000000, 0) for i in range(1, 1200)]
    start, dd = path([(x + 1, y) for x, y in zig])
    assert _segments_rc(L, [spline(start, dd)], 4, 4) == BAD
    with pytest.raises(sm.SplineError):
        sm.segments([spline(start, dd)], 0, 4, 4)
    # the estimated-area limit: wide sigma DCTs along a long path in a small frame
    wide = spline(*path([(0, 0), (4000000, 0), (4000000, 4000000)]), y=100000)
    wide["sigma"] = [1000000] * 32
    assert _segments_rc(L, [wide], 16, 16) == BAD
    with pytest.raises(sm.SplineError):
        sm.segments([wide], 0, 16, 16)
    # no splines at all
    h = C.c_void_p()
    assert L.jxlhip_splines_from_quantized(0, None, None, None, None, 0, C.byref(h)) == BAD


def test_a_spline_just_inside_the_position_limit(L):
    """Just inside +-2^23 the draw list is computed: its segments lie far right of the frame (they are still listed,
    as in the reference; the draw skips them by column)."""
    far = spline(((1 << 23) - 100, 5), [(50, 3)])
    rc, h = abi.splines_from_quantized([far])
    assert rc == 0
    try:
        rc, segs = abi.splines_segments(h, 300, 200, 0.0, 1.0)
        assert rc == 0 and len(segs) > 0 and min(s.center_x for s in segs) > 8e6
        compare_segments(segs, sm.segments([far], 0, 300, 200))
    finally:
        abi.splines_destroy(h)
