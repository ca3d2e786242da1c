"""The launch geometry of the phase-2 row marches, restated in plain Python, and the frame sizes derived from it
(test_geometry_model.py checks what the lists reach on the CPU, test_gpu_geometry.py decodes them).

Every function names the host code it restates.  None of the 32-bit offset limits of the launchers matter here: no
frame of these lists exceeds 520 x 160 pixels."""
import numpy as np

WINDOW = 128           # columns a wave holds: 64 lanes x a pair of columns (filters_fast.h, kSlabCols in filters_march.h)
STAGE_LISTS = [(0, 0), (1, 0), (0, 1), (1, 1), (0, 2), (1, 2)]  # JXLHIP_STAGE_LISTS (filters_fast.h): (gab, epf_iters)
EPF3_LISTS = [(0, 3), (1, 3)]                                   # k_epf0 / k_fused_pc0 + the (0, 2) march behind them
ALL_LISTS = STAGE_LISTS + EPF3_LISTS
CU_COUNTS = (32, 64, 128, 256)  # DeviceCus(): a CPX / QPX / DPX partition and a whole card


class Geom:
    """HX halo rows / columns a side, HXP the columns in whole pairs, USE the output columns of a wave."""

    def __init__(self, hx, hxp, use):
        self.hx, self.hxp, self.use = hx, hxp, use
        assert use == WINDOW - 2 * hxp


def march_hx(gab, epf):
    """FastGeom::HX (filters_fast.h) = MarchGeom::HX (filters_march.h)."""
    return gab + (2 if epf >= 1 else 0) + (1 if epf == 2 else 0)


def fast_geom(gab, epf):
    """FastGeom (filters_fast.h): k_filters_fast."""
    hx = march_hx(gab, epf)
    hxp = (hx + 1) & ~1
    return Geom(hx, hxp, WINDOW - 2 * hxp)


def geom0(gab):
    """Geom0 (kernels_epf0.hip): k_epf0."""
    return Geom(gab + 3, 4, WINDOW - 8)


K_FUSED_HALO = 8                            # kFusedHalo (fused_pc.h)
K_SLAB_COLS = WINDOW                        # kSlabCols (filters_march.h)
K_FUSED_USE = K_SLAB_COLS - 2 * K_FUSED_HALO  # kFusedUse (fused_pc.h): 112
K_PC_PER_CU = 6                             # kPcPerCu (fused_pc.h)


def fused_geom(gab, epf):
    """The window of k_fused_pc / k_fused_pc0 (kernels_fused.hip, kernels_fused_epf0.hip): the halo is 8 columns
    whatever the stage list needs."""
    return Geom(gab + 3 if epf == 3 else march_hx(gab, epf), K_FUSED_HALO, K_FUSED_USE)


def path_geom(path, gab, epf):
    if path in ("fused", "fused_epf3"):
        return fused_geom(gab, epf)
    return geom0(gab) if epf == 3 else fast_geom(gab, epf)


def num_strips(g, W):
    return (W + g.use - 1) // g.use


def edge(g, strip, W):
    """`edge` of k_filters_fast, k_epf0 (x_first - HXP), k_fused_pc, k_fused_pc0 (x0 = x_first - kFusedHalo): the
    wave's 128-column window leaves [0, W)."""
    x0 = strip * g.use - g.hxp
    return x0 < 0 or x0 + WINDOW > W


def strip_position(strip, strips):
    return "first" if strip == 0 else ("last" if strip == strips - 1 else "middle")


def chunk_rows(wgx, rows, resident, first, last, step, overhead):
    """ChunkRows (kernels.h)."""
    best, best_cost = 64, 1e30
    for rh in range(first, last + 1, step):
        wgs = wgx * ((rows + rh - 1) // rh)
        gens = (wgs + resident - 1) // resident
        cost = float(gens) * (rh + overhead)
        if cost < best_cost:
            best_cost, best = cost, rh
    return best


def fast_rh(g, W, rows, cus, forced=0):
    """LaunchFastT (filters_fast.h); JXLHIP_FILTER_RH = forced."""
    wgx = (num_strips(g, W) + 3) // 4
    return forced if forced > 0 else chunk_rows(wgx, rows, cus * 2, 16, 512, 1, 2 * g.hx + 6)


def epf0_rh(gab, W, rows, cus, forced=0):
    """LaunchEpf0 (kernels_epf0.hip); JXLHIP_FILTER_RH = forced."""
    wgx = (num_strips(geom0(gab), W) + 3) // 4
    return forced if forced > 0 else chunk_rows(wgx, rows, cus * 2, 16, 512, 1, 2 * (3 + gab) + 6)


def fused_rows_pc(strips, rows, cus, forced=0, per_cu=K_PC_PER_CU):
    """FusedRowsPC (fused_pc.h); JXLHIP_FUSED_PC_RH = forced, rounded up to whole block rows."""
    if forced > 0:
        return (forced + 7) & ~7
    return chunk_rows(strips, rows, cus * per_cu, 16, 1024, 8, 6 + 16)


def path_rh(path, gab, epf, W, H, cus, forced=0):
    """Rows per chunk of the path's first march over a whole frame (rows 0 .. H)."""
    if path in ("fused", "fused_epf3"):
        per_cu = 4 if (epf == 3 and gab) else K_PC_PER_CU  # LaunchFusedEpf0: four windows per CU with Gaborish
        return fused_rows_pc(num_strips(fused_geom(gab, epf), W), H, cus, forced, per_cu)
    if epf == 3:
        return epf0_rh(gab, W, H, cus, forced)
    return fast_rh(fast_geom(gab, epf), W, H, cus, forced)


def chunks(H, rh):
    """[(y_begin, y_end)] of a whole frame: y_begin = blockIdx.y * RH, y_end = min(y_begin + RH, H)."""
    return [(y, min(y + rh, H)) for y in range(0, H, rh)]


def chunk_position(i, n):
    return "first" if i == 0 else ("last" if i == n - 1 else "middle")


def interior(y_begin, y_end, H):
    """`interior` of k_fused_pc (kernels_fused.hip)."""
    return (y_begin & 7) == 0 and ((y_end - y_begin) & 7) == 0 and y_begin >= 8 and y_end + 8 <= H


def march_takes(W, H):
    """LaunchFiltersFast (kernels_filters_fast.hip), LaunchEpf0 (kernels_epf0.hip): smaller frames go to the generic
    kernel (multiply mirrored rows / columns)."""
    return W >= 16 and H >= 16


def fused_supported(W, H, epf):
    """FusedSupported (kernels_fused.hip) for a whole frame with float RGB / planar XYB output."""
    return epf <= 2 and march_takes(W, H) and not 1 <= (H & 7) <= 3


def fused_epf0_supported(W, H):
    """FusedEpf0Supported (kernels_fused_epf0.hip) for a whole frame."""
    return march_takes(W, H) and not 1 <= (H & 7) <= 3


def path_fuses(path, W, H, epf):
    if path == "fused":
        return fused_supported(W, H, epf)
    if path == "fused_epf3":
        return fused_epf0_supported(W, H)
    return False


def fused_nwg(g, W, H, rh):
    """nwg of LaunchFusedPcT / LaunchFusedEpf0: strips x chunks (the grid is nwg rounded up to 8)."""
    return num_strips(g, W) * ((H + rh - 1) // rh)


# ---- the size lists ----------------------------------------------------------------------------------------------------
BASE_WIDTHS = [16, 17, 18, 23, 24, 25, 31]
HEIGHTS = list(range(16, 32)) + list(range(36, 48))  # every residue twice from the minimum on; 36..47: see the model test
TALL_HEIGHTS = [150, 151, 157]                       # tails 6, 7, 5
FILTER_RH = [17, 23, 200]                            # JXLHIP_FILTER_RH: coprime to 8 twice, and one chunk
FUSED_PC_RH = [16, 24, 40]                           # JXLHIP_FUSED_PC_RH
ONE_CHUNK_FILTER_RH = 200                            # above every height here: the whole frame in one chunk
ONE_CHUNK_FUSED_PC_RH = 48                           # ... above every height of HEIGHTS (a multiple of 8)
TINY_A = [1, 2, 3, 7, 8, 9, 15]
TINY_B = [1, 2, 8, 15, 16, 40]
BOUNDARY_15_16 = [(15, 16), (16, 15), (16, 16)]


def window_end_width(g):
    """The W at which the window of strip 1 ends exactly on W.  With a halo (HXP > 0) the LAST wave's window always
    overshoots (it ends at strips * USE + HXP > W), so the last window that can end on W is the one before it."""
    return 2 * g.use + g.hxp


def widths(g):
    w = set(BASE_WIDTHS)
    w |= {k * g.use + d for k in (1, 2, 4) for d in (-1, 0, 1, 2)}  # strip seams; 4 * USE + 1: a second workgroup
    w |= {window_end_width(g) + d for d in (-1, 0, 1)}
    return sorted(w)


def pair(ws, hs, per=3):
    """Every width with `per` consecutive heights of the list (consecutive heights differ in residue), walking the
    height list cyclically: no cross product, yet every height meets at least two widths once
    per * len(ws) >= 2 * len(hs)."""
    out = []
    for i, w in enumerate(ws):
        for j in range(per):
            out.append((w, hs[(per * i + j) % len(hs)]))
    return out


def tall_frames(g):
    """Two strips with a one-column last strip, and the width whose middle window ends on W."""
    return [(w, h) for w in (g.use + 1, window_end_width(g)) for h in TALL_HEIGHTS]


def nwg_frames():
    """(W, H) whose fused launch at the product's own chunk height (16) has 1, 7, 8 and 9 workgroups."""
    return {1: (100, 16), 7: (100, 100), 8: (130, 60), 9: (230, 47)}


def path_frames(path, gab, epf):
    """The frames one GPU test of (path, stage list) decodes at the product's own chunk height."""
    g = path_geom(path, gab, epf)
    fr = pair(widths(g), HEIGHTS)
    if path in ("fused", "fused_epf3"):
        fr += list(nwg_frames().values()) + BOUNDARY_15_16
    return fr


def tiny_frames():
    fr = [(a, b) for a in TINY_A for b in TINY_B] + [(b, a) for a in TINY_A for b in TINY_B] + BOUNDARY_15_16
    return sorted(set(fr))


def features(path, gab, epf, W, H, rh):
    """The predicate values frame (W, H) reaches on `path` with chunks of `rh` rows."""
    if not march_takes(W, H):
        return {("march", False)}
    fuses = path_fuses(path, W, H, epf)
    if path in ("fused", "fused_epf3") and not fuses:  # the two-phase fallback of the same stage list
        return {("fuses", False), ("tail", H & 7)} | {f for f in features("two_phase", gab, epf, W, H, rh) if f[0] == "edge"}
    g = path_geom(path, gab, epf)
    n = num_strips(g, W)
    out = {("edge", strip_position(s, n), edge(g, s, W)) for s in range(n)}
    out.add(("tail", H & 7))
    ch = chunks(H, rh)
    out.add(("chunks", "one" if len(ch) == 1 else "many", H & 7))
    for i, (y0, y1) in enumerate(ch):
        out.add(("y_begin", y0 & 7))
        if path == "fused":
            out.add(("interior", chunk_position(i, len(ch)), interior(y0, y1, H)))
    if fuses:
        out.add(("fuses", True))
    return out


def cover(frames, feats):
    """A small sublist of `frames` that reaches every feature the whole list reaches (greedy set cover; feats(frame)
    -> set)."""
    todo = set().union(*[feats(f) for f in frames])
    out = []
    while todo:
        best = max(frames, key=lambda f: len(feats(f) & todo))
        out.append(best)
        todo -= feats(best)
    return out


def seam_rows(H, rh):
    """y_begin of every chunk but the first that starts inside a block row: where the march reloads inv_sigma because
    its chunk begins (Step in filters_march.h: o == y_begin - (EPF == 2), o2 == y_begin; Step0 in epf0_march.h:
    o == y_begin), not because a block row does."""
    return [y for y, _ in chunks(H, rh)[1:] if y & 7]


def epf_stages(epf):
    """`which` of the oracle's epf() for the EPF stages of a stage list, in order (dec_cache.cc:156-170)."""
    return {0: [], 1: [1], 2: [1, 2], 3: [0, 1, 2]}[epf]


# ---- the frames themselves ---------------------------------------------------------------------------------------------
# roughly half DCT8 by area, the rest the strategies of one block and of 2 x 1 / 1 x 2 / 2 x 2 blocks: the fused
# producer then both decodes cells (DCT8) and copies them from the planes (everything else)
GEOM_MIX = {0: 50, 1: 4, 2: 4, 3: 4, 12: 4, 13: 4, 14: 3, 15: 3, 16: 3, 17: 3, 6: 6, 7: 6, 4: 6}
SEAM_SHARPNESS = ((4, 5), (6, 7))
# synth's quant field at its default scale puts 1 / sigma of most cells below kMinSigma (-3.9: inv_sigma is about
# -0.2 * raw_quant / LUT value at the default global_scale), where an EPF stage copies its input -- a wrong sigma would
# then show in few cells.  At half the scale the cells of sharpness 4..7, about nine in ten, filter.
QUANT_MUL = 0.5


def make_frame(W, H, gab, epf, output_kind=1, seams=()):
    """frames.make_case for one geometry frame: (params, CPU tensors).  The seed depends on the size alone, so the
    stage lists share their inputs.  seams: rows whose block row and the block row above get sharpness values from
    two disjoint sets (random inside each), so that the sigma of the one is never the sigma of the other."""
    import torch
    from libjxl_amd import synth
    params, t = synth.synth_frame(W, H, device="cpu", mix=GEOM_MIX, gab=bool(gab), epf_iters=epf, seed=7000 + 1000 * W + H,
                                  quant_mul=QUANT_MUL, output_kind=output_kind)
    if seams:
        sh = t["epf_sharpness"].numpy().copy()
        rng = np.random.default_rng(W * 4099 + H)
        by_rows = sorted({y >> 3 for y in seams} | {(y >> 3) - 1 for y in seams})
        for by in by_rows:
            sh[by] = rng.choice(SEAM_SHARPNESS[by & 1], size=sh.shape[1]).astype(np.uint8)
        t["epf_sharpness"] = torch.from_numpy(sh)
    return params, t


def tall_seams(H):
    return sorted({y for rh in FILTER_RH for y in seam_rows(H, rh)})
