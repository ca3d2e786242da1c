"""k_prepare once per hand-over of side info (context.hip: LaunchPhase1, PrepareAhead).

k_prepare reads side info and frame constants only, so a context remembers the prepare it has enqueued -- keyed by the
`fused` mode and a hand-over generation -- and a later direct decode of the same hand-over launches the transform
kernels on the remembered work lists.  What these tests hold: the reuse changes no sample (against a
JXLHIP_PREPARE_ONCE=0 context, which prepares in front of every phase 1, and against the oracle); everything that may
change what k_prepare reads or wrote ends it (new inputs, a new frame, another stream, a reported error, another
`fused` mode, a capture); jxlhip_debug_prepare_launches says what happened.

Frames: frames.make_case, 520x264 (3 x 2 groups, ragged on both edges), synth.MIX_D1; the bar against the oracle is
test_gpu_parity.py's TIGHT; "equal" is torch.equal.  The list-length hand-off to the host (exact special_wgs) was
not kept, so there is no case for it.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import frames
from libjxl_amd import VarDctDecoder, abi, synth

pytestmark = pytest.mark.gpu

TIGHT = 2e-5
XS, YS = 520, 264


def to_dev(t):
    return {k: ([x.cuda() for x in v] if isinstance(v, list) else v.cuda()) for k, v in t.items()}


def rel_err(got, ref):
    scale = max(1.0, float(np.abs(ref).max()))
    return float(np.abs(got.astype(np.float64) - ref).max()) / scale


@functools.lru_cache(maxsize=None)
def case(xs=XS, ys=YS, seed=41, gab=True, epf=1):
    """(params, device tensors, oracle frame decoded once): shared by the tests, never written to."""
    params, t, fr = frames.make_case(xs, ys, mix=synth.MIX_D1, gab=gab, epf_iters=epf, seed=seed)
    return params, to_dev(t), t, fr.decode(threads=4)


def make_dec(monkeypatch, fuse, once=True):
    monkeypatch.setenv("JXLHIP_FUSE", fuse)
    if once:
        monkeypatch.delenv("JXLHIP_PREPARE_ONCE", raising=False)
    else:
        monkeypatch.setenv("JXLHIP_PREPARE_ONCE", "0")
    return VarDctDecoder(0)  # (the path switches are copied when the context is created)


@pytest.fixture(scope="module")
def dq(oracle):
    d = VarDctDecoder(0)
    p, _ = synth.synth_frame(8, 8, mix=synth.MIX_DCT8)
    d.begin_frame(p)
    t = d.default_dequant_tables()
    d.sync()
    d.close()
    return t


def fresh(monkeypatch, fuse, params, devt, dq, once=False):
    d = make_dec(monkeypatch, fuse, once=once)
    d.begin_frame(params)
    d.set_inputs(devt, dq)
    out = d.decode_frame()
    d.sync()
    d.close()
    return out


@pytest.mark.parametrize("epf", [0, 1, 2, 3])
@pytest.mark.parametrize("fuse", ["1", "0"])
def test_reuse_is_invisible(dq, fuse, epf, monkeypatch):
    params, devt, _, ref = case(epf=epf)
    outs = {}
    for once in (True, False):
        d = make_dec(monkeypatch, fuse, once=once)
        d.begin_frame(params)
        d.set_inputs(devt, dq)
        outs[once] = [d.decode_frame().clone() for _ in range(3)]
        d.sync()
        assert d.prepare_launches() == ((1, 2) if once else (3, 0))
        d.close()
    for o in outs[True] + outs[False]:
        assert torch.equal(o, outs[False][0])
    assert rel_err(outs[True][2].cpu().numpy(), ref) <= TIGHT


def upload(d, params, t, dq):
    """jxlhip_upload_side_info + jxlhip_submit_group per group, from host arrays (test_upload_path_equals_device_path)."""
    L = d.L
    npy = {k: ([x.numpy() for x in v] if isinstance(v, list) else v.numpy()) for k, v in t.items()}
    dqh = dq.cpu().numpy()
    dc3 = (C.c_void_p * 3)(*[x.ctypes.data for x in npy["dc"]])
    assert L.jxlhip_upload_side_info(d.ctx, npy["ac_strategy"].ctypes.data, npy["raw_quant"].ctypes.data,
                                     npy["epf_sharpness"].ctypes.data, npy["ytox_map"].ctypes.data,
                                     npy["ytob_map"].ctypes.data, dc3, dqh.ctypes.data) == 0
    ngroups = ((params["xsize"] + 255) // 256) * ((params["ysize"] + 255) // 256)
    for g in range(ngroups):
        ptrs = (C.c_void_p * 3)(*[npy["coeffs"][c][g * 65536:].ctypes.data for c in range(3)])
        assert L.jxlhip_submit_group(d.ctx, g, ptrs, 65536) == 0
    d.sync()  # (the host arrays are temporaries)


@pytest.mark.parametrize("fuse", ["1", "0"])
def test_new_side_info_is_seen(dq, fuse, monkeypatch):
    """Two seeds of one geometry: another strategy map, quant field and sharpness.  used_acs = 0 ("not known") so that
    one frame_begin serves both."""
    pa, da, ta, ref_a = case(seed=41)
    _, db, tb, ref_b = case(seed=42)
    assert not torch.equal(ta["ac_strategy"], tb["ac_strategy"]) and not torch.equal(ta["raw_quant"], tb["raw_quant"])
    assert not torch.equal(ta["epf_sharpness"], tb["epf_sharpness"])
    params = dict(pa, used_acs=0)
    want = {"a": fresh(monkeypatch, fuse, params, da, dq), "b": fresh(monkeypatch, fuse, params, db, dq)}
    assert not torch.equal(want["a"], want["b"])
    assert rel_err(want["a"].cpu().numpy(), ref_a) <= TIGHT and rel_err(want["b"].cpu().numpy(), ref_b) <= TIGHT
    # the zero-copy hand-over
    d = make_dec(monkeypatch, fuse)
    d.begin_frame(params)
    for i, (k, devt) in enumerate([("a", da), ("b", db), ("a", da)]):
        d.set_inputs(devt, dq)
        out = d.decode_frame()
        d.sync()
        assert torch.equal(out, want[k]), (i, k)
    assert d.prepare_launches() == (3, 0)
    # host arrays: the second and third upload have no frame_begin in front; the prepare rides behind the copies
    d.begin_frame(params)
    for i, (k, t) in enumerate([("a", ta), ("b", tb), ("a", ta)]):
        upload(d, params, t, dq)
        assert d.prepare_launches() == (4 + i, 0)
        out = d.decode_frame()
        d.sync()
        assert torch.equal(out, want[k]), ("upload", i, k)
        assert d.prepare_launches() == (4 + i, 0)  # (the decode took up the hand-over's launch: nothing saved, nothing added)
    assert torch.equal(d.decode_frame(), want["a"])
    assert d.prepare_launches() == (6, 1)
    # across a frame_begin to another geometry and back
    ps, ds, _, ref_s = case(xs=264, ys=200, seed=43)
    small = fresh(monkeypatch, fuse, ps, ds, dq)
    assert rel_err(small.cpu().numpy(), ref_s) <= TIGHT
    for p, devt, w in [(params, da, want["a"]), (ps, ds, small), (params, da, want["a"])]:
        d.begin_frame(p)
        d.set_inputs(devt, dq)
        for _ in range(2):
            out = d.decode_frame()
            d.sync()
            assert torch.equal(out, w)
    assert d.prepare_launches() == (9, 4)
    d.close()


def test_key_follows_the_fused_mode(dq, monkeypatch):
    """One context: decode_frame (fused = 1 under JXLHIP_FUSE=1), the split calls (0), decode_frame with a concurrency
    hint and without (1: the hint moves nothing when the switch forces the path) -- a new prepare exactly where `fused`
    changes, the same pixels everywhere, and the taps behind the split calls as a context without the reuse has them."""
    params, devt, _, ref = case()
    d = make_dec(monkeypatch, "1")
    d.begin_frame(params)
    d.set_inputs(devt, dq)
    first = d.decode_frame().clone()
    assert d.prepare_launches() == (1, 0)
    out = d.alloc_output()
    d.decode_blocks()
    d.decode_filters(out)
    assert d.prepare_launches() == (2, 0)
    assert torch.equal(out, first)
    xyb = d.export_xyb()
    sigma = d.sigma()
    d.decode_blocks()
    d.decode_filters(out)
    assert d.prepare_launches() == (2, 1)
    assert torch.equal(out, first)
    for x, y in zip(d.export_xyb(), xyb):
        assert np.array_equal(x, y)
    d.set_concurrency_hint(3)
    assert torch.equal(d.decode_frame(), first)
    assert d.prepare_launches() == (3, 1)
    d.set_concurrency_hint(1)
    assert torch.equal(d.decode_frame(), first)
    assert d.prepare_launches() == (3, 2)
    d.sync()
    d.close()
    off = make_dec(monkeypatch, "1", once=False)
    off.begin_frame(params)
    off.set_inputs(devt, dq)
    off.decode_blocks()
    off.decode_filters(out)
    assert torch.equal(out, first)
    for x, y in zip(off.export_xyb(), xyb):
        assert np.array_equal(x, y)
    assert torch.equal(off.sigma(), sigma)
    off.close()
    assert rel_err(first.cpu().numpy(), ref) <= TIGHT


def test_key_follows_the_concurrency_hint(dq, oracle, monkeypatch):
    """Without a forced path the hint moves the fused threshold (12 -> 6 Mpx): on a 3328x2048 frame it changes `fused`,
    and with it the key."""
    monkeypatch.delenv("JXLHIP_FUSE", raising=False)
    monkeypatch.delenv("JXLHIP_PREPARE_ONCE", raising=False)
    params, t = synth.synth_frame(3328, 2048, mix=synth.MIX_D1, gab=True, epf_iters=1, seed=3, device="cuda")
    d = VarDctDecoder(0)
    d.begin_frame(params)
    d.set_inputs(t, dq)
    outs = []
    want = [(1, 0), (1, 1), (2, 1), (2, 2), (3, 2)]
    for hint, n in zip([1, 1, 3, 3, 1], want):
        d.set_concurrency_hint(hint)
        outs.append(d.decode_frame().clone())
        assert d.prepare_launches() == n
    d.sync()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[2], outs[3]) and torch.equal(outs[0], outs[4])
    assert rel_err(outs[2].cpu().numpy(), outs[0].cpu().numpy().astype(np.float64)) <= 2 * TIGHT  # (both paths within TIGHT of the oracle)
    d.close()


@pytest.mark.parametrize("fuse", ["1", "0"])
def test_stripes_reuse(dq, fuse, monkeypatch):
    """Three group rows as three stripe contexts (the pattern of test_stripe_step_in_three_calls_equals_whole_frame),
    decoded twice per context: both rounds are the whole frame's rows, the second round launches no k_prepare."""
    params, devt, _, ref = case(xs=520, ys=600, seed=44)
    whole = fresh(monkeypatch, fuse, params, devt, dq)
    assert rel_err(whole.cpu().numpy(), ref) <= TIGHT
    parts = [(0, 1), (1, 1), (2, 1)]
    decs = []
    for (g0, gr) in parts:
        d = make_dec(monkeypatch, fuse)
        d.begin_frame(dict(params, stripe_group_y0=g0, stripe_group_rows=gr))
        d.set_inputs(devt, dq)
        decs.append(d)
    h = decs[0].halo_rows()
    for round_ in range(2):
        bufs, outs = [], []
        for d, (g0, gr) in zip(decs, parts):
            mk = lambda: torch.full((3, h, 520), float("nan"), dtype=torch.float32, device="cuda")  # noqa: E731
            up, dn = g0 > 0, g0 + gr < 3
            b = dict(up=mk() if up else None, dn=mk() if dn else None)
            d.stripe_begin(b["up"], b["dn"])
            out = d.alloc_output()
            y0, y1 = d.stripe_rows()
            rows = (y0 + 8 if up else y0, y1 - 8 if dn else y1)
            d.decode_filters(out, rows=rows)
            bufs.append(b), outs.append((out, rows))
        torch.cuda.synchronize()
        for i, d in enumerate(decs):
            d.stripe_finish(outs[i][0], bufs[i - 1]["dn"] if i > 0 else None, bufs[i + 1]["up"] if i + 1 < len(decs) else None,
                            outs[i][1])
            d.sync()
        assert torch.equal(torch.cat([o for o, _ in outs], dim=0), whole), round_
        for d in decs:
            assert d.prepare_launches() == (1, round_)
    for d in decs:
        d.close()


def bad_map_case():
    params, t = synth.synth_frame(256, 256, mix=synth.MIX_DCT8, gab=False, epf_iters=0)
    bad = dict(t)
    acs = t["ac_strategy"].clone()
    acs[31, 31] = (5 << 1) | 1   # a 32x32 block starting in the last cell: overflows the group (test_bad_strategy_map_is_reported)
    bad["ac_strategy"] = acs
    return params, t, bad


@pytest.mark.parametrize("fuse", ["1", "0"])
def test_errors_are_reported_on_every_decode(dq, oracle, fuse, monkeypatch):
    params, good, bad = bad_map_case()
    want = fresh(monkeypatch, fuse, params, to_dev(good), dq)
    fr = frames.oracle_frame(params, good, oracle.default_dequant_tables())
    assert rel_err(want.cpu().numpy(), fr.decode(threads=4)) <= TIGHT
    d = make_dec(monkeypatch, fuse)
    d.begin_frame(params)
    d.set_inputs(to_dev(bad), dq)
    for _ in range(2):
        d.decode_frame()
        with pytest.raises(abi.JxlHipError, match="format constraint"):
            d.sync()
        d.sync()  # the flag is cleared
    d.decode_frame()
    d.decode_frame()  # (reused: the flag of the first one is still up)
    with pytest.raises(abi.JxlHipError, match="format constraint"):
        d.sync()
    d.set_inputs(to_dev(good), dq)
    out = d.decode_frame()
    d.sync()
    assert torch.equal(out, want)
    # a used_acs mask that rules out a strategy the frame uses: k_prepare reports it, again on every decode
    pm, devm, _, _ = case()
    assert pm["used_acs"] & (1 << 4)
    d.begin_frame(dict(pm, used_acs=pm["used_acs"] & ~(1 << 4)))
    d.set_inputs(devm, dq)
    for _ in range(2):
        d.decode_frame()
        with pytest.raises(abi.JxlHipError):
            d.sync()
        d.sync()
    d.begin_frame(pm)
    d.set_inputs(devm, dq)
    out = d.decode_frame()
    d.sync()
    assert torch.equal(out, fresh(monkeypatch, fuse, pm, devm, dq))
    d.close()


@pytest.mark.parametrize("fuse", ["1", "0"])
def test_streams(dq, fuse, monkeypatch):
    """jxlhip_set_stream to another stream ends the prepared state: the old stream's k_prepare is ordered on that stream
    only.  Each stream is synchronised by d.sync() alone."""
    params, devt, _, _ = case()
    want = fresh(monkeypatch, fuse, params, devt, dq)
    torch.cuda.synchronize()
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    d = make_dec(monkeypatch, fuse)
    d.set_stream(a)
    d.begin_frame(params)
    d.set_inputs(devt, dq)
    n = 0
    for st in (a, b, a):
        d.set_stream(st)
        outs = [d.decode_frame(), d.decode_frame()]
        d.sync()
        n += 1
        assert d.prepare_launches() == (n, n)
        assert torch.equal(outs[0], want) and torch.equal(outs[1], want)
    d.close()


@pytest.mark.parametrize("fuse", ["1", "0"])
def test_capture_turns_the_reuse_off_until_the_next_frame(dq, fuse, monkeypatch):
    params, devt, _, _ = case(xs=1000, ys=520, seed=45)
    want = fresh(monkeypatch, fuse, params, devt, dq)
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(cs):
        d = make_dec(monkeypatch, fuse)  # bound to cs for its whole life
        d.begin_frame(params)
        d.set_inputs(devt, dq)
        out = d.alloc_output()
        d.decode_frame(out)
        d.decode_frame(out)
    cs.synchronize()
    assert d.prepare_launches() == (1, 1) and torch.equal(out, want)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        d.decode_frame(out)
    assert d.prepare_launches() == (1, 1)  # (captured launches count in neither)
    with torch.cuda.stream(cs):
        for i in range(3):
            out.zero_()
            d.decode_frame(out)
            cs.synchronize()
            assert torch.equal(out, want), ("direct", i)
            out.zero_()
            g.replay()
            cs.synchronize()
            assert torch.equal(out, want), ("replay", i)
        assert d.prepare_launches() == (4, 1)
        d.begin_frame(params)
        d.set_inputs(devt, dq)
        for i in range(3):
            out.zero_()
            d.decode_frame(out)
            d.sync()
            assert torch.equal(out, want), ("after frame_begin", i)
        assert d.prepare_launches() == (5, 3)
    d.close()


def test_whole_file_prepares_once_per_file(dq, oracle, monkeypatch):
    """jxlhip_decode_codestream enqueues the prepare behind its side-info copies and the frame's decode takes it up: one
    k_prepare per file, none saved.  The stream and the bar are tests/test_codestream.py's first case."""
    import test_codestream as tc
    if not oracle.ref_available():
        pytest.skip("oracle/_ref not available")
    oracle.ref_lib()
    monkeypatch.delenv("JXLHIP_FUSE", raising=False)
    monkeypatch.delenv("JXLHIP_PREPARE_ONCE", raising=False)
    rs = oracle.RealStream(seed=23, **tc.CASES[0])
    cs = rs.codestream.tobytes()
    L = abi.load_library()
    d = VarDctDecoder(0)
    info = abi.CodestreamInfo()
    assert L.jxlhip_codestream_basic_info(cs, len(cs), C.byref(info)) == 0
    out = torch.empty((info.ysize, info.xsize, 3), dtype=torch.float32, device="cuda")
    scale = max(1.0, float(np.abs(rs.rgb).max()))
    for n in (1, 2):
        out.zero_()
        rc = L.jxlhip_decode_codestream(d.ctx, None, None, cs, len(cs), 1, None, out.data_ptr(), info.xsize * 12, 0,
                                        C.byref(info))
        assert rc == 0, L.jxlhip_last_error(d.ctx)
        assert float(np.abs(out.cpu().numpy() - rs.rgb).max()) / scale <= tc.TIGHT
        assert d.prepare_launches() == (n, 0)  # launched behind the side info, taken up by the frame's one decode
    d.close()


# (launched, reused) of jxlhip_debug_prepare_launches after one hand-over and two decodes of a staged frame.  Taken from
# the commit before the render stages moved into render_stages.hip, on the same machine: the explicit output target
# must route every staged decode, and PrepareAhead's guess for it, exactly as the temporary rewrite of c->p did.
STAGED_PAIRS = {"plain": (1, 1), "noise": (1, 1), "tone-mapped": (1, 1), "blended": (1, 1), "blended-srgb8-rgba": (1, 1)}


@pytest.mark.parametrize("stage", sorted(STAGED_PAIRS))
def test_staged_frames_prepare_as_before(dq, stage, monkeypatch):
    """A one-group frame without Gaborish or EPF (the automatic rule fuses it at any size), handed over once through
    jxlhip_upload_side_info (which prepares ahead, in the mode PrepareAhead assumes for the stage) and decoded twice."""
    from output_sweep import fmt
    monkeypatch.delenv("JXLHIP_FUSE", raising=False)
    monkeypatch.delenv("JXLHIP_PREPARE_ONCE", raising=False)
    rgba8 = stage == "blended-srgb8-rgba"
    params, t = synth.synth_frame(200, 56, mix=synth.MIX_D1, gab=False, epf_iters=0, seed=46, output_kind=2 if rgba8 else 1,
                                  out_format=fmt(abi.TF_SRGB, abi.SAMPLE_U8, 4) if rgba8 else None)
    d = VarDctDecoder(0)
    d.begin_frame(params)
    if stage == "noise":
        d.set_noise([0.02, 0.03, 0.05, 0.05, 0.04, 0.03, 0.02, 0.02])
    elif stage == "tone-mapped":
        d.set_tone_mapping(1000.0, 100.0)
    elif stage.startswith("blended"):  # over an empty slot, off the origin, into a larger image: k_blend runs
        d.set_blending((208, 60), (3, 2), abi.BLEND_ADD)
    upload(d, params, t, dq)
    outs = [d.decode_frame().clone() for _ in range(2)]
    d.sync()
    pair = d.prepare_launches()
    print("prepare launches", stage, pair)
    assert torch.equal(outs[0], outs[1])
    assert pair == STAGED_PAIRS[stage]
    d.close()
