"""Patches as the reference renders them, restated in numpy: PatchDictionary::AddOneRow (lib/jxl/dec_patch_dictionary.cc:
319-357) with PerformBlending's colour channels on an image without an alpha channel (lib/jxl/blending.cc:150-184) and
PerformMulBlending (lib/jxl/alpha.cc:82-93).  Patch after patch in dictionary order -- the order GetPatchesForRow
restores for every row -- one float32 operation per sample.  Test infrastructure, not part of the product."""
import numpy as np

NONE, REPLACE, ADD, MUL, BLEND_ABOVE, BLEND_BELOW, ALPHA_ADD_ABOVE, ALPHA_ADD_BELOW = range(8)


def blend(mode, clamp, bg, fg):
    """One colour plane's rectangle: float32 in, float32 out."""
    bg, fg = bg.astype(np.float32), fg.astype(np.float32)
    if mode == NONE:
        return bg
    if mode in (REPLACE, BLEND_ABOVE, BLEND_BELOW):  # without alpha the blend modes copy the foreground
        return fg
    if mode in (ADD, ALPHA_ADD_ABOVE, ALPHA_ADD_BELOW):  # ... and the weighted adds add
        return (bg + fg).astype(np.float32)
    assert mode == MUL, mode
    if clamp:  # Clamp1(fg, 0, 1): a NaN passes
        fg = np.where(fg < 0, np.float32(0), np.where(fg > 1, np.float32(1), fg)).astype(np.float32)
    return (bg * fg).astype(np.float32)


def apply(planes, patches, refs):
    """planes: float32 [3, ysize, xsize] (X, Y, B) behind the loop filters; patches: dicts with the fields of jxlhip_patch
    (abi.patches_list); refs: {slot: float32 [3, h, w]}.  Returns the blended planes; rectangles are clipped to the frame
    as the row loops of the render pipeline clip them."""
    out = np.array(planes, dtype=np.float32, copy=True)
    _, H, W = out.shape
    for p in patches:
        x0, y0 = p["x"], p["y"]
        x1, y1 = min(x0 + p["xsize"], W), min(y0 + p["ysize"], H)
        if x0 >= x1 or y0 >= y1:
            continue
        ref = refs[p.get("ref", 0)]
        rx, ry = p.get("ref_x0", 0), p.get("ref_y0", 0)
        assert rx + p["xsize"] <= ref.shape[2] and ry + p["ysize"] <= ref.shape[1]
        fg = ref[:, ry:ry + (y1 - y0), rx:rx + (x1 - x0)]
        for c in range(3):
            out[c, y0:y1, x0:x1] = blend(p["mode"], p.get("clamp", 0), out[c, y0:y1, x0:x1], fg[c])
    return out
