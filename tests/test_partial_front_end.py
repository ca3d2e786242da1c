"""Which sections of a file that ends early count (jxlhip_codestream_partial_info, host only): against the counts the
test derives from the TOC by itself at every section boundary and one byte either side of it, and against the
reference -- JxlDecoderFlushImage on the same bytes fails exactly where the call answers JXLHIP_ERR_NEED_MORE_INPUT --
over a grid of 200 lengths per stream."""
import ctypes as C

import numpy as np
import pytest

from libjxl_amd import abi

import partial_ref as pr

NEED_MORE_INPUT = -9
GRID = 200


@pytest.fixture(scope="module")
def L():
    return abi.load_library()


@pytest.fixture(scope="module")
def ref(oracle):
    if not oracle.ref_available():
        pytest.skip("oracle/_ref not available")
    oracle.ref_lib()
    return oracle


@pytest.fixture(scope="module")
def jxl_ref():
    return pr.load_reference()


@pytest.fixture(scope="module")
def files(L, ref):
    return {key: (pr.stream(ref, key), pr.Sections(L, pr.stream(ref, key))) for key in pr.STREAMS + [pr.ONE_SECTION]}


def test_the_abi_has_the_new_code_and_struct(L):
    assert abi.ERR_NEED_MORE_INPUT == NEED_MORE_INPUT and L.jxlhip_status_string(NEED_MORE_INPUT) != L.jxlhip_status_string(-100)
    assert C.sizeof(abi.PartialInfo) == 40
    pi = abi.PartialInfo()
    assert L.jxlhip_codestream_partial_info(None, 0, None, C.byref(pi)) == -1
    assert L.jxlhip_codestream_partial_info(b"", 0, None, C.byref(pi)) == NEED_MORE_INPUT
    assert L.jxlhip_codestream_partial_info(b"\xff", 1, None, C.byref(pi)) == NEED_MORE_INPUT
    assert L.jxlhip_codestream_partial_info(b"\x00\x00\x00\x0cJX", 6, None, C.byref(pi)) == NEED_MORE_INPUT
    assert L.jxlhip_codestream_partial_info(b"GIF89a", 6, None, C.byref(pi)) == -5


@pytest.mark.parametrize("key", pr.STREAMS)
def test_the_streams_have_the_sections_the_cases_need(files, key):
    cs, s = files[key]
    assert len(s.off) > 1 and s.ng > 1
    assert s.np == (1 if key[0] == "plain" else 3) or s.np > 1


@pytest.mark.parametrize("key", pr.STREAMS)
def test_counts_at_every_section_boundary(L, files, key):
    cs, s = files[key]
    seen = set()
    for b in s.boundaries():
        for n in (b - 1, b, b + 1):
            if n > len(cs):
                continue
            want = s.expect(n)
            rc, got = pr.partial_info(L, cs, n)
            assert rc == (NEED_MORE_INPUT if want is None else 0), (n, rc)
            if want is not None:
                assert got == want, (n, got, want)
                seen.add(want[1:4])
    # the boundaries walk through DC-only, mixed and complete states
    assert any(c[2] == s.ng for c in seen) and any(c[0] == s.ng for c in seen) and len(seen) > 3
    if s.np > 1:
        assert any(c[1] > 0 for c in seen)


@pytest.mark.parametrize("key", pr.STREAMS)
def test_need_more_input_exactly_where_the_reference_flush_fails(L, files, jxl_ref, key):
    ts, RL = jxl_ref
    cs, s = files[key]
    lengths = sorted(set(np.linspace(1, len(cs), GRID).astype(int).tolist()))
    assert len(lengths) >= GRID
    prev = (0, 0, -s.ng)
    flushed_any = failed_any = False
    for n in lengths:
        rc, got = pr.partial_info(L, cs, n)
        flushed, pic = pr.flush(ts, RL, cs[:n])
        assert rc == (0 if flushed else NEED_MORE_INPUT), (n, rc, flushed)
        flushed_any |= flushed
        failed_any |= not flushed
        if not flushed:
            continue
        assert not (pic == pr.SENTINEL).any()  # the picture is written in full
        want = s.expect(n)
        assert want is not None and got == want, (n, got, want)
        # complete and complete + partial never shrink, DC-only never grows
        state = (got[1], got[1] + got[2], -got[3])
        assert all(a >= b for a, b in zip(state, prev)), (n, state, prev)
        prev = state
    assert flushed_any and failed_any


def test_a_one_section_frame_is_all_or_nothing(L, files, jxl_ref):
    ts, RL = jxl_ref
    cs, s = files[pr.ONE_SECTION]
    assert len(s.off) == 1
    for n in range(1, len(cs)):
        rc, _ = pr.partial_info(L, cs, n)
        assert rc == NEED_MORE_INPUT, (n, rc)
    for n in (len(cs) // 3, len(cs) - 1):
        assert not pr.flush(ts, RL, cs[:n])[0]
    rc, got = pr.partial_info(L, cs, len(cs))
    assert rc == 0 and got == (1, 1, 0, 0, 1, len(cs))
    assert pr.flush(ts, RL, cs)[0]


def test_a_container_that_ends_early(L, files):
    """The same file in a jxlc box behind ftyp: a box cut short gives the codestream bytes that are there (the counts of
    the bare codestream at that length, bytes_used an offset into the codestream); a file that ends inside the box
    headers has nothing to draw yet."""
    key = pr.STREAMS[0]
    cs, s = files[key]
    head = (b"\x00\x00\x00\x0cJXL \x0d\x0a\x87\x0a" + b"\x00\x00\x00\x14ftypjxl \x00\x00\x00\x00jxl " +
            (8 + len(cs)).to_bytes(4, "big") + b"jxlc")
    box = head + cs
    info, pi = abi.CodestreamInfo(), abi.PartialInfo()
    for m in range(1, len(head) + 2):
        assert L.jxlhip_codestream_partial_info(box, m, None, C.byref(pi)) == NEED_MORE_INPUT, m
    bounds = s.boundaries()
    for n in (bounds[0] - 1, bounds[len(bounds) // 4], bounds[len(bounds) // 2] + 1, bounds[-1] - 1, bounds[-1]):
        want = s.expect(n)
        rc, got = pr.partial_info(L, box, len(head) + n)
        assert rc == (NEED_MORE_INPUT if want is None else 0), (n, rc)
        if want is not None:
            assert got == want, (n, got, want)
    assert L.jxlhip_codestream_partial_info(box, len(box), C.byref(info), C.byref(pi)) == 0
    assert (info.container, info.xsize, info.ysize, pi.complete) == (1, key[1], key[2], 1)
    # the calls that take whole files still refuse the cut container
    assert L.jxlhip_codestream_basic_info(box, len(box) - 1, C.byref(info)) == -5
