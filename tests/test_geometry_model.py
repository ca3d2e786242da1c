"""CPU tier of the geometry sweep (geometry.py, test_gpu_geometry.py).

The lists reach what they claim: the restated predicates of the launchers, evaluated over the frame lists, take every
value they can take.  And the inputs have teeth: the oracle's staged calls equal its whole decode, a stale inv_sigma
in ONE row at a chunk seam moves that row of the picture by at least ten times the bar of the GPU tier, and the
padding below and beside a frame is nothing like its mirror image."""
import os
import re

import numpy as np
import pytest

import frames
import geometry as G

TIGHT = frames.TIGHT
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "libjxl_amd", "csrc")
EPF_LISTS = [(g, e) for g, e in G.ALL_LISTS if e]
TWO_PHASE = [("two_phase", g, e) for g, e in G.STAGE_LISTS] + [("epf3", g, e) for g, e in G.EPF3_LISTS]
FUSED = [("fused", g, e) for g, e in G.STAGE_LISTS] + [("fused_epf3", g, e) for g, e in G.EPF3_LISTS]


def source(name):
    return open(os.path.join(CSRC, name)).read()


# ---- the restatement follows the sources ----------------------------------------------------------------------------------
def test_restated_constants_are_the_sources():
    ff, e0, fp, fm = source("filters_fast.h"), source("kernels_epf0.hip"), source("fused_pc.h"), source("filters_march.h")
    assert "HX = GAB + (EPF >= 1 ? 2 : 0) + (EPF == 2 ? 1 : 0)" in ff and "HXP = (HX + 1) & ~1" in ff
    assert "USE = 128 - 2 * HXP" in ff and "USE = 128 - 2 * HXP" in e0
    assert "HX = GAB + 3;" in e0 and re.search(r"HXP = 4;", e0)
    assert "kFusedHalo = 8;" in fp and "kFusedUse = kSlabCols - 2 * kFusedHalo;" in fp and "kPcPerCu = 6;" in fp
    assert "kSlabCols = 128;" in fm
    assert "return ChunkRows(strips, rows, DeviceCus() * per_cu, 16, 1024, 8, 6 + 16);" in fp
    assert "if (forced > 0) return (forced + 7) & ~7;" in fp
    assert "DeviceCus() * 2u, 16, 512, 1, 2 * G::HX + 6)" in ff and "DeviceCus() * 2u, 16, 512, 1, 2 * (3 + gab) + 6)" in e0
    assert "filter_rh" in e0  # LaunchEpf0 takes JXLHIP_FILTER_RH: the forced seams below are k_epf0's too
    for text in (ff, e0):
        assert "const bool edge = x_first - HXP < 0 || x_first - HXP + 128 > W;" in text
    for name in ("kernels_fused.hip", "kernels_fused_epf0.hip"):
        text = source(name)
        assert "const bool edge = x0 < 0 || x0 + kSlabCols > W;" in text and "const int x0 = x_first - kFusedHalo;" in text
        assert "if (f.xsize < 16 || f.ysize < 16) return false;" in text
        assert "if (tail >= 1 && tail <= 3) return false;" in text
    assert re.search(r"interior = \(y_begin & 7\) == 0 && \(\(y_end - y_begin\) & 7\) == 0 && y_begin >= 8 &&\s+"
                     r"y_end \+ 8 <= \(int\)f\.ysize;", source("kernels_fused.hip"))
    assert [G.fast_geom(g, e).use for g, e in G.STAGE_LISTS] == [128, 124, 124, 120, 120, 120]
    assert G.geom0(0).use == G.geom0(1).use == 120 and G.K_FUSED_USE == 112


def all_frames(path, gab, epf):
    return G.path_frames(path, gab, epf) + G.tall_frames(G.path_geom(path, gab, epf))


@pytest.mark.parametrize("path,gab,epf", TWO_PHASE + FUSED)
def test_frames_are_small_and_cut_at_16_rows_on_every_device(path, gab, epf):
    """ChunkRows returns 16 for every frame here whatever the compute-unit count: one generation of workgroups is
    enough, so the lowest height wins.  The seams of the unforced decodes therefore do not move with the device."""
    for W, H in all_frames(path, gab, epf):
        assert W <= 520 and H <= 160
        if G.march_takes(W, H):
            for cus in G.CU_COUNTS:
                assert G.path_rh(path, gab, epf, W, H, cus) == 16, (W, H, cus)
    for W, H in G.tiny_frames():
        assert not G.march_takes(W, H) or (W, H) == (16, 16)


@pytest.mark.parametrize("path,gab,epf", TWO_PHASE + FUSED)
def test_pairing(path, gab, epf):
    fr = G.pair(G.widths(G.path_geom(path, gab, epf)), G.HEIGHTS)
    assert len(fr) < len(set(w for w, _ in fr)) * len(G.HEIGHTS) // 4  # no cross product
    for w in {w for w, _ in fr}:
        assert len({h & 7 for ww, h in fr if ww == w}) >= 2, w
    for h in G.HEIGHTS:
        assert len({w for w, hh in fr if hh == h}) >= 2, h
    assert sorted(h & 7 for h in range(16, 32)) == sorted(list(range(8)) * 2) and min(G.HEIGHTS) == 16


# ---- what the lists reach ------------------------------------------------------------------------------------------------
def reachable_edges(g):
    return {("edge", G.strip_position(s, G.num_strips(g, W)), G.edge(g, s, W))
            for W in range(16, 1200) for s in range(G.num_strips(g, W))}


@pytest.mark.parametrize("path,gab,epf", TWO_PHASE + FUSED)
def test_strip_seams_and_both_values_of_edge(path, gab, epf):
    g = G.path_geom(path, gab, epf)
    ws = G.widths(g)
    for k in (1, 2, 4):
        assert {k * g.use - 1, k * g.use, k * g.use + 1, k * g.use + 2} <= set(ws)
    assert (4 * g.use + 1 + g.use - 1) // g.use == 5  # a fifth wave: the second workgroup of the two-phase kernels
    # the edge / non-edge flip of the window that ends on W
    W0 = G.window_end_width(g)
    assert not G.edge(g, 1, W0) and {W0 - 1, W0, W0 + 1} <= set(ws)
    assert G.edge(g, 1, W0 - 1) and 1 * g.use - g.hxp + G.WINDOW == W0
    if g.hxp:  # the last wave's window always overshoots: non-edge first / last strips do not exist
        assert all(G.edge(g, G.num_strips(g, W) - 1, W) and G.edge(g, 0, W) for W in range(16, 1200))
    # the EPF2 fix lanes (Lane::fix_right_even / fix_right_odd): W of both parities right of a strip seam
    assert {w & 1 for w in ws if w > g.use} == {0, 1}
    got = set()
    for W, H in G.path_frames(path, gab, epf):
        if G.march_takes(W, H):
            got |= {f for f in G.features("two_phase" if path == "epf3" else path, gab, epf, W, H, 16) if f[0] == "edge"}
    want = reachable_edges(g)
    if path in ("fused", "fused_epf3"):  # (their fallback frames report the two-phase windows)
        got = {("edge", G.strip_position(s, G.num_strips(g, W)), G.edge(g, s, W))
               for W, H in G.path_frames(path, gab, epf) if G.path_fuses(path, W, H, epf) for s in range(G.num_strips(g, W))}
    assert got == want, want - got
    if g.hxp:
        assert want == {("edge", "middle", False), ("edge", "middle", True), ("edge", "first", True), ("edge", "last", True)}
    else:  # (0, 0), no halo: a window leaves the frame only on the right, and only the last one can
        assert want == {("edge", "middle", False)} | {("edge", p, v) for p in ("first", "last") for v in (False, True)}


@pytest.mark.parametrize("path,gab,epf", TWO_PHASE)
def test_forced_chunk_heights_put_a_seam_on_every_row_of_a_block(path, gab, epf):
    g = G.path_geom(path, gab, epf)
    seen = set()
    for W, H in G.tall_frames(g):
        assert G.march_takes(W, H) and G.num_strips(g, W) >= 2
        for rh in G.FILTER_RH:
            ch = G.chunks(H, rh)
            if rh > H:
                assert len(ch) == 1
                continue
            assert np.gcd(rh, 8) == 1 and ch[-1][1] - ch[-1][0] < rh  # the last chunk is partial
            seen |= {y & 7 for y, _ in ch}
        assert G.tall_seams(H) == sorted(y for rh in G.FILTER_RH for y in G.seam_rows(H, rh))
        assert all(y & 7 for y in G.tall_seams(H)) and len(G.tall_seams(H)) >= 12
    assert seen == set(range(8))
    # ... while the unforced frames never start a chunk inside a block row: their seams test nothing of the reloads
    assert {y & 7 for W, H in all_frames(path, gab, epf) for y, _ in G.chunks(H, 16)} == {0}


@pytest.mark.parametrize("path,gab,epf", TWO_PHASE + FUSED)
def test_every_tail_under_one_chunk_and_under_many(path, gab, epf):
    fused = path in ("fused", "fused_epf3")
    fr = [(W, H) for W, H in G.path_frames(path, gab, epf) if G.march_takes(W, H)]
    one_rh = G.ONE_CHUNK_FUSED_PC_RH if fused else G.ONE_CHUNK_FILTER_RH
    assert {H & 7 for _, H in fr} == set(range(8))
    tails = (0, 4, 5, 6, 7) if fused else range(8)
    many = {H & 7 for _, H in fr if len(G.chunks(H, 16)) > 1}
    one = {H & 7 for _, H in fr if len(G.chunks(H, one_rh)) == 1}
    non_first = {H & 7 for _, H in fr if len(G.chunks(H, 16)) > 2}  # 36..47: the tail sits under a third chunk
    assert set(tails) <= many and set(tails) <= one and set(tails) <= non_first
    assert all(H <= one_rh for H in G.HEIGHTS)
    if fused:
        refused = {H & 7 for W, H in fr if not G.path_fuses(path, W, H, epf)}
        assert refused == {1, 2, 3}
        assert {H & 7 for W, H in fr if G.path_fuses(path, W, H, epf)} == set(tails)
        for W, H in G.tall_frames(G.path_geom(path, gab, epf)):
            assert G.path_fuses(path, W, H, epf)
        assert {H & 7 for H in G.TALL_HEIGHTS} == {5, 6, 7}
        assert not G.fused_supported(15, 16, epf if epf < 3 else 2) and not G.fused_supported(16, 15, epf if epf < 3 else 2)
        assert {(15, 16), (16, 15), (16, 16)} <= set(G.path_frames(path, gab, epf))


@pytest.mark.parametrize("gab,epf", G.STAGE_LISTS)
def test_both_values_of_interior(gab, epf):
    """k_fused_pc: the first chunk (y_begin < 8) and the last (no 8 rows below it) are never interior; a middle chunk
    of RH = 16 is from H = 40 on, and 36..47 bracket that flip."""
    assert not G.interior(16, 32, 39) and G.interior(16, 32, 40) and {39, 40} <= set(G.HEIGHTS)
    want = {("interior", G.chunk_position(i, len(G.chunks(H, rh))), G.interior(y0, y1, H))
            for H in range(16, 400) for rh in (16, 24, 40) for i, (y0, y1) in enumerate(G.chunks(H, rh))}
    got = set()
    for W, H in G.path_frames("fused", gab, epf):
        if G.fused_supported(W, H, epf):
            got |= {f for f in G.features("fused", gab, epf, W, H, 16) if f[0] == "interior"}
    assert got == want, want - got
    assert ("interior", "middle", True) in want and ("interior", "middle", False) in want
    for W, H in G.tall_frames(G.fused_geom(gab, epf)):  # the forced heights: interior and generic chunks in one launch
        for rh in G.FUSED_PC_RH:
            assert len({G.interior(y0, y1, H) for y0, y1 in G.chunks(H, G.fused_rows_pc(0, H, 256, rh))}) == 2


def test_fused_launch_sizes():
    """nwg = strips x chunks at 1, 7, 8, 9: the grid is nwg rounded up to 8 and the windows are dealt XCD-first, so 7
    leaves one idle workgroup, 8 none and 9 seven (logical >= nwg)."""
    for nwg, (W, H) in G.nwg_frames().items():
        for gab, epf in G.ALL_LISTS:
            path = "fused_epf3" if epf == 3 else "fused"
            assert G.path_fuses(path, W, H, epf)
            assert G.fused_nwg(G.fused_geom(gab, epf), W, H, 16) == nwg
            assert (W, H) in G.path_frames(path, gab, epf)
    assert sorted(G.nwg_frames()) == [1, 7, 8, 9]


def test_tiny_frames():
    fr = set(G.tiny_frames())
    for a in G.TINY_A:
        for b in G.TINY_B:
            assert (a, b) in fr and (b, a) in fr
    assert {(15, 16), (16, 15), (16, 16)} <= fr
    assert {(1, 1), (2, 1), (1, 2), (2, 2)} <= fr  # two and more reflections in every stage
    assert all(not G.march_takes(W, H) for W, H in fr if (W, H) != (16, 16)) and G.march_takes(16, 16)


def test_reduced_lists_keep_every_predicate_value():
    for path, gab, epf in TWO_PHASE + FUSED:
        fr = G.path_frames(path, gab, epf)

        def feats(f):
            return G.features(path, gab, epf, f[0], f[1], 16)
        sub = G.cover(fr, feats)
        assert len(sub) <= 16 and set().union(*map(feats, sub)) == set().union(*map(feats, fr))


# ---- teeth ----------------------------------------------------------------------------------------------------------------
def staged(fr, gab, epf, sigma, planes, splice=None):
    """The oracle's stages one by one; splice = (which, row, sigma): that stage's output row computed with another map."""
    p = fr.gaborish(planes) if gab else planes
    for which in G.epf_stages(epf):
        q = fr.epf(which, sigma, p)
        if splice is not None and splice[0] == which:
            bad = fr.epf(which, splice[2], p)
            for c in range(3):
                q[c][splice[1]] = bad[c][splice[1]]
        p = q
    return fr.xyb_to_rgb(p)


@pytest.mark.parametrize("gab,epf", G.ALL_LISTS)
def test_staged_calls_equal_the_whole_decode(oracle, gab, epf):
    params, t = G.make_frame(130, 150, gab, epf)
    fr = frames.oracle_frame(params, t, oracle.default_dequant_tables())
    got = staged(fr, gab, epf, fr.compute_sigma() if epf else None, fr.decode_groups())
    assert np.array_equal(got, fr.decode())


@pytest.mark.parametrize("gab,epf", EPF_LISTS)
def test_a_stale_sigma_in_one_seam_row_shows(oracle, gab, epf):
    """For every tall frame of the GPU tier, every seam row y its forced chunk heights put inside a block row, and every
    EPF stage of the list: row y of that stage computed with the sigma of the block row above (np.roll: what a missed
    reload leaves in inv_sigma_blk / inv_sigma_blk2 when the wave marched down from there), the remaining stages run
    on the result.  Row y of the picture moves by at least 10x the bar in some channel -- for EVERY such row, stage and
    frame; the smallest movement over all lists was 110x the bar when this was written.  Reverting a reload in Step /
    Step0 leaves the wave's INITIAL inv_sigma (-1.0) in a chunk's first rows instead, which is further off still (the
    second model: 450x the bar at least), so either revert fails test_gpu_geometry.py at every listed seam."""
    path = "epf3" if epf == 3 else "two_phase"
    worst = {}
    for W, H in G.tall_frames(G.path_geom(path, gab, epf)):
        seams = G.tall_seams(H)
        params, t = G.make_frame(W, H, gab, epf, seams=seams)
        fr = frames.oracle_frame(params, t, oracle.default_dequant_tables())
        planes, sigma = fr.decode_groups(), fr.compute_sigma()
        base = staged(fr, gab, epf, sigma, planes)
        mag = np.maximum(np.abs(base).reshape(-1, 3).max(axis=0), 1e-3)
        models = {"block row above": np.roll(sigma, 1, axis=0), "initial -1.0": np.full_like(sigma, -1.0)}
        stages = G.epf_stages(epf)
        ins = [fr.gaborish(planes) if gab else planes]  # ins[i]: what stage i reads; ins[-1]: what XybToRgb reads
        for which in stages:
            ins.append(fr.epf(which, sigma, ins[-1]))
        assert np.array_equal(fr.xyb_to_rgb(ins[-1]), base)
        for model, bad_sigma in models.items():
            for i, which in enumerate(stages):
                bad = fr.epf(which, bad_sigma, ins[i])
                for y in seams:
                    if model == "initial -1.0" and y != seams[0]:
                        continue  # (one row per frame and stage: the model the issue sets is the other one)
                    p = [a.copy() for a in ins[i + 1]]
                    for c in range(3):
                        p[c][y] = bad[c][y]
                    for rest in stages[i + 1:]:
                        p = fr.epf(rest, sigma, p)
                    out = fr.xyb_to_rgb(p)
                    moved = float((np.abs(out[y].astype(np.float64) - base[y]).max(axis=0) / mag).max())
                    worst[model] = min(worst.get(model, np.inf), moved / TIGHT)
                    assert moved >= 10 * TIGHT, (model, W, H, which, y, moved / TIGHT)
                    far = np.delete(np.arange(H), np.arange(max(0, y - 4), min(H, y + 5)))
                    assert np.array_equal(out[far], base[far])  # (the splice is local: nothing else moved)
    print("TEETH seam rows (%d, %d): least movement / bar: %s" % (gab, epf, {k: round(v, 1) for k, v in worst.items()}))


@pytest.mark.parametrize("gab,epf", [(1, 2)])
def test_padding_is_not_the_mirror(oracle, gab, epf):
    """Rows H .. H + 2 and column W of the block-padded planes hold what the inverse transforms left there; the stages
    must read the MIRROR of the frame instead.  In every frame with such rows / such a column the two differ by at
    least 50x the bar in every channel."""
    sizes = set()
    for path, g_, e_ in TWO_PHASE + FUSED:
        sizes |= set(G.path_frames(path, g_, e_)) | set(G.tall_frames(G.path_geom(path, g_, e_)))
    rows_checked = cols_checked = 0
    for W, H in sorted(sizes):
        if not G.march_takes(W, H) or (H % 8 == 0 and W % 8 == 0):
            continue
        params, t = G.make_frame(W, H, gab, epf)
        planes = frames.oracle_frame(params, t, oracle.default_dequant_tables()).decode_groups()
        for c in range(3):
            p = planes[c].astype(np.float64)
            mag = max(np.abs(p[:H, :W]).max(), 1e-3)
            for k in range(3):
                if H + k < p.shape[0]:
                    assert np.abs(p[H + k, :W] - p[H - 1 - k, :W]).max() >= 50 * TIGHT * mag, (W, H, c, k)
                    rows_checked += 1
            if W < p.shape[1]:
                assert np.abs(p[:H, W] - p[:H, W - 1]).max() >= 50 * TIGHT * mag, (W, H, c)
                cols_checked += 1
    assert rows_checked > 300 and cols_checked > 300
