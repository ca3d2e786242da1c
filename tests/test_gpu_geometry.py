"""Every phase-2 row march against the libjxl reference over GEOMETRY: the frame sizes of geometry.py, which put a
frame edge, a strip seam, a chunk seam or a height residue on every branch the launch geometry selects
(test_geometry_model.py shows on the CPU that the lists reach those branches, and that a stale sigma at a seam row or
padding read for the mirror would move the picture by many times the bar).

One test is one path x one stage list (gab, epf_iters).  It loops over that list's frames with one VarDctDecoder per
environment setting, decoders one after the other: the switches are sampled when a context is created.  The reference
is the libjxl decoder with its own dequant tables; the bar is the per-channel one of test_gpu_frame_params.py
(frames.TIGHT = 2e-5 of the channel's magnitude), held on EVERY frame.  Each test prints the worst error it saw:
"WORST <path> <stage list> <c0> <c1> <c2> over <n> decodes"."""
import numpy as np
import pytest

import frames
import geometry as G

pytestmark = pytest.mark.gpu

TIGHT = frames.TIGHT
SWITCHES = ("JXLHIP_FUSE", "JXLHIP_FILTERS", "JXLHIP_MFMA", "JXLHIP_FUSED_PC_RH", "JXLHIP_FILTER_RH")
RGB, XYB = 1, 0  # JXLHIP_OUT_LINEAR_RGB_F32, JXLHIP_OUT_XYB_PLANAR


@pytest.fixture(scope="module")
def ref(oracle):
    if not oracle.ref_available():
        pytest.fail("oracle/_ref/libjxl_ref.so missing: run __graft_entry__.build() in the build container")
    oracle.ref_lib()
    return oracle


class Case:
    """One frame: the product's inputs on the device and the reference's picture."""

    def __init__(self, ref, W, H, gab, epf, kind=RGB, seams=()):
        self.W, self.H, self.kind = W, H, kind
        self.params, t = G.make_frame(W, H, gab, epf, output_kind=kind, seams=seams)
        self.want = frames.oracle_frame(self.params, t, ref.ref_default_dequant_tables()).decode_ref(threads=1)
        self.dev = {k: ([x.cuda() for x in v] if isinstance(v, list) else v.cuda()) for k, v in t.items()}
        self.name = "%dx%d%s" % (W, H, "" if kind == RGB else " xyb")


def decode_all(env, cases, monkeypatch):
    """One decoder created under `env` decodes every case: [(output as numpy, profile slots)]."""
    from libjxl_amd import VarDctDecoder
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    d = VarDctDecoder(0)
    out = []
    try:
        d.profile(True)
        dq = None
        for c in cases:
            d.begin_frame(c.params)
            if dq is None:
                dq = d.default_dequant_tables()
            d.set_inputs(c.dev, dq)
            o = d.decode_frame().cpu().numpy()
            d.sync()
            out.append((o, d.profile_read()))
    finally:
        d.close()
    return out


class Worst:
    """The bar on every decode, the worst error for the test's WORST line, every miss in the final assert."""

    def __init__(self, path, gab, epf):
        self.label = "%s (%d, %d)" % (path, gab, epf)
        self.err, self.n, self.missed = np.zeros(3), 0, []

    def check(self, what, case, got):
        assert got.shape == case.want.shape, (what, case.name)
        err = frames.per_channel_err(got, case.want, 2 if case.kind == RGB else 0)
        self.err, self.n = np.maximum(self.err, err), self.n + 1
        if not (err <= TIGHT).all():  # (NaN misses too)
            self.missed.append((what, case.name, err.tolist()))

    def done(self):
        print("WORST %s %.3e %.3e %.3e over %d decodes" % (self.label, *self.err, self.n))
        assert not self.missed, (self.label, len(self.missed), self.missed[:12])


def same(a, b, what, cases):
    for c, (x, _), (y, _) in zip(cases, a, b):
        assert np.array_equal(x, y), (what, c.name, np.argwhere(x != y)[:5].tolist())


def check_slots(path, epf, case, slots):
    if path == "two_phase":
        assert "fused" not in slots and "filters" in slots, (case.name, slots)
    elif path == "epf3":
        assert "fused" not in slots and "epf0" in slots and "filters" in slots, (case.name, slots)
    elif path == "fused":
        if G.fused_supported(case.W, case.H, epf):  # an accepted tail: the fused kernel and nothing behind it
            assert "fused" in slots and "filters" not in slots, (case.name, slots)
        else:  # a refused tail or a frame under 16: the two-phase march / the generic kernel
            assert "fused" not in slots and "filters" in slots, (case.name, slots)
    else:  # fused_epf3: k_fused_pc0 and k_epf0 mark the same slot; the march behind either marks "filters"
        assert "fused" not in slots and "filters" in slots, (case.name, slots)
        assert ("epf0" in slots) == G.march_takes(case.W, case.H), (case.name, slots)


def run_path(ref, monkeypatch, path, gab, epf):
    fused = path in ("fused", "fused_epf3")
    base = {"JXLHIP_FUSE": "1" if fused else "0"}
    rh_switch = "JXLHIP_FUSED_PC_RH" if fused else "JXLHIP_FILTER_RH"
    one_chunk = G.ONE_CHUNK_FUSED_PC_RH if fused else G.ONE_CHUNK_FILTER_RH
    forced = G.FUSED_PC_RH if fused else G.FILTER_RH
    worst = Worst(path, gab, epf)
    sizes = G.path_frames(path, gab, epf)

    # 1. every frame at the product's own chunk height (16 rows here) and as one chunk; float RGB
    cases = [Case(ref, W, H, gab, epf) for W, H in sizes]
    own = decode_all(base, cases, monkeypatch)
    one = decode_all(dict(base, **{rh_switch: str(one_chunk)}), cases, monkeypatch)
    for what, outs in (("own", own), ("one chunk", one)):
        for c, (got, slots) in zip(cases, outs):
            worst.check(what, c, got)
            check_slots(path, epf, c, slots)
    same(own, one, "own chunk height / one chunk", cases)
    if path == "fused_epf3":  # which EPF0 march ran the slots cannot tell: the fused path equals the two-phase one
        same(own, decode_all({"JXLHIP_FUSE": "0"}, cases, monkeypatch), "JXLHIP_FUSE=1 / 0", cases)

    # 2. the tall frames with their seams moved: the bar at every chunk height, and the same bits at all of them
    g = G.path_geom(path, gab, epf)
    tall = [Case(ref, W, H, gab, epf, seams=G.tall_seams(H)) for W, H in G.tall_frames(g)]
    runs = [("own", decode_all(base, tall, monkeypatch))]
    for rh in forced:
        runs.append(("%s=%d" % (rh_switch, rh), decode_all(dict(base, **{rh_switch: str(rh)}), tall, monkeypatch)))
    for what, outs in runs:
        for c, (got, slots) in zip(tall, outs):
            worst.check(what, c, got)
            check_slots(path, epf, c, slots)
        same(runs[0][1], outs, "own chunk height / " + what, tall)
    if path == "fused_epf3":
        same(runs[0][1], decode_all({"JXLHIP_FUSE": "0"}, tall, monkeypatch), "JXLHIP_FUSE=1 / 0", tall)

    # 3. planar XYB: one frame per predicate value, and one tall frame at the first forced height
    reduced = G.cover(sizes, lambda f: G.features(path, gab, epf, f[0], f[1], 16))
    xyb = [Case(ref, W, H, gab, epf, kind=XYB) for W, H in reduced]
    for c, (got, slots) in zip(xyb, decode_all(base, xyb, monkeypatch)):
        worst.check("own", c, got)
        check_slots(path, epf, c, slots)
    W, H = G.tall_frames(g)[-1]
    xyb_tall = [Case(ref, W, H, gab, epf, kind=XYB, seams=G.tall_seams(H))]
    for c, (got, _) in zip(xyb_tall, decode_all(dict(base, **{rh_switch: str(forced[0])}), xyb_tall, monkeypatch)):
        worst.check("%s=%d" % (rh_switch, forced[0]), c, got)
    worst.done()


@pytest.mark.parametrize("gab,epf", G.STAGE_LISTS)
def test_two_phase(ref, gab, epf, monkeypatch):
    """JXLHIP_FUSE=0: k_filters_fast<gab, epf> from the block-major planes.  JXLHIP_FILTER_RH = 17 and 23 start chunks
    on every row of a block row (the reloads of inv_sigma_blk / inv_sigma_blk2 at o == y_begin - (EPF == 2) and
    o2 == y_begin in Step, filters_march.h)."""
    run_path(ref, monkeypatch, "two_phase", gab, epf)


@pytest.mark.parametrize("gab,epf", G.EPF3_LISTS)
def test_epf3(ref, gab, epf, monkeypatch):
    """JXLHIP_FUSE=0, three EPF iterations: k_epf0<gab> and the row-major k_filters_fast<0, 2, SRC_LINEAR> behind it;
    JXLHIP_FILTER_RH cuts both (Step0's reload at o == y_begin, epf0_march.h)."""
    run_path(ref, monkeypatch, "epf3", gab, epf)


@pytest.mark.parametrize("gab,epf", G.STAGE_LISTS)
def test_fused(ref, gab, epf, monkeypatch):
    """JXLHIP_FUSE=1: k_fused_pc on the heights FusedSupported accepts (tails 0 and 4..7: the producer's mirror rows,
    the interior / generic chunk forms, launches of 1, 7, 8 and 9 windows), the two-phase march on those it refuses
    (tails 1..3) and the generic kernel under 16 pixels -- within the bar either way."""
    run_path(ref, monkeypatch, "fused", gab, epf)


@pytest.mark.parametrize("gab,epf", G.EPF3_LISTS)
def test_fused_epf3(ref, gab, epf, monkeypatch):
    """JXLHIP_FUSE=1, three EPF iterations: k_fused_pc0<gab> from the producer's slab, then the row-major march;
    bit-equal to the JXLHIP_FUSE=0 decode of the same frame (k_epf0), as test_fused_kernels of
    test_gpu_frame_params.py holds it at one size."""
    run_path(ref, monkeypatch, "fused_epf3", gab, epf)


@pytest.mark.parametrize("gab,epf", G.ALL_LISTS)
def test_tiny(ref, gab, epf, monkeypatch):
    """Frames under 16 pixels in a dimension: the generic LDS kernel, whatever JXLHIP_FUSE says; widths and heights of
    1 and 2 mirror twice and more in every stage.  15x16, 16x15 and 16x16 cross to the march."""
    worst = Worst("tiny", gab, epf)
    cases = [Case(ref, W, H, gab, epf) for W, H in G.tiny_frames()]
    for env in ({}, {"JXLHIP_FUSE": "1"}):
        for c, (got, slots) in zip(cases, decode_all(env, cases, monkeypatch)):
            worst.check("JXLHIP_FUSE=" + env.get("JXLHIP_FUSE", "unset"), c, got)
            if not G.march_takes(c.W, c.H):
                assert "fused" not in slots and "epf0" not in slots and "filters" in slots, (c.name, slots)
    worst.done()
