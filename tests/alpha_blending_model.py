"""numpy float32 restatement of frame blending on an image WITH extra channels: the reference's BlendingStage
(render_pipeline/stage_blending.cc: ProcessRow inside the frame's rectangle, ProcessPaddingRow outside, every extra
channel with a source slot of its own) over all of PerformBlending (blending.cc:42-190) and the row loops of alpha.cc:18-93.
Every intermediate is held in float32 and every expression is evaluated in the reference's operation order, so a kernel
that does the same is bit-equal to this.  (blending_model.py is the image without extra channels.)"""
import numpy as np

from blending_model import ADD, ALPHA_WEIGHTED_ADD, BLEND, MODES, MUL, REPLACE, rect  # noqa: F401  (BlendMode)

ONE, ZERO = np.float32(1), np.float32(0)


def clamp01(v):
    """Clamp1(x, 0, 1) (base/common.h): a NaN passes (np.clip does the same)."""
    return np.clip(v, ZERO, ONE)


def new_alpha(fa, bga):
    return (ONE - (ONE - fa) * (ONE - bga)).astype(np.float32)


def reciprocal(new_a):
    """rnew_a = new_a > 0 ? 1.f / new_a : 0.f"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(new_a > 0, ONE / new_a, ZERO).astype(np.float32)


def alpha_blend_channel(bg, bga, fg, fga, premultiplied, clamp, same):
    """PerformAlphaBlending, single-channel form (alpha.cc:42-65); same = the channel is its own alpha channel (the
    reference compares the row pointers)."""
    fa = clamp01(fga) if clamp else fga
    if same:
        return new_alpha(fa, bga)
    if premultiplied:
        return (fg + bg * (ONE - fa)).astype(np.float32)
    na = new_alpha(fa, bga)
    return ((fg * fa + bg * bga * (ONE - fa)) * reciprocal(na)).astype(np.float32)


def alpha_weighted_add(bg, fg, fga, clamp, same):
    """PerformAlphaWeightedAdd (alpha.cc:67-80)"""
    if same:
        return bg.copy()
    return (bg + fg * (clamp01(fga) if clamp else fga)).astype(np.float32)


def mul_blend(bg, fg, clamp):
    """PerformMulBlending (alpha.cc:82-93)"""
    return (bg * (clamp01(fg) if clamp else fg)).astype(np.float32)


def perform_blending(bg, fg, color, ec, info):
    """PerformBlending on arrays that cover the frame's clipped rectangle: bg, fg = lists of 3 + n planes (each a
    float32 array of one shape), color = dict(mode, clamp, alpha_channel), ec = n such dicts, info = n dicts with
    is_alpha and alpha_associated.  Returns the 3 + n blended planes."""
    n = len(ec)
    has_alpha = any(i["is_alpha"] for i in info)
    out = [None] * (3 + n)
    # the extra channels first, so that every blend uses the pre-blend alpha
    for i, e in enumerate(ec):
        a = e.get("alpha_channel", 0)
        b, f = bg[3 + i], fg[3 + i]
        if e["mode"] == ADD:
            r = (b + f).astype(np.float32)
        elif e["mode"] == BLEND:
            r = alpha_blend_channel(b, bg[3 + a], f, fg[3 + a], bool(info[a]["alpha_associated"]), bool(e.get("clamp")), a == i)
        elif e["mode"] == ALPHA_WEIGHTED_ADD:
            r = alpha_weighted_add(b, f, fg[3 + a], bool(e.get("clamp")), a == i)
        elif e["mode"] == MUL:
            r = mul_blend(b, f, bool(e.get("clamp")))
        elif e["mode"] == REPLACE:
            r = f.copy()
        else:
            raise ValueError(e["mode"])
        out[3 + i] = r
    a = color.get("alpha_channel", 0)
    clamp = bool(color.get("clamp"))
    mode = color["mode"]
    if mode == ADD or (mode == ALPHA_WEIGHTED_ADD and not has_alpha):
        for c in range(3):
            out[c] = (bg[c] + fg[c]).astype(np.float32)
    elif mode == ALPHA_WEIGHTED_ADD:
        for c in range(3):
            out[c] = alpha_weighted_add(bg[c], fg[c], fg[3 + a], clamp, False)
    elif mode == REPLACE or (mode == BLEND and not has_alpha):
        for c in range(3):
            out[c] = fg[c].copy()
    elif mode == BLEND:
        # PerformAlphaBlending, four-channel form (alpha.cc:18-41): writes the alpha channel's row as well
        premultiplied = bool(info[a]["alpha_associated"])
        fa = clamp01(fg[3 + a]) if clamp else fg[3 + a]
        na = new_alpha(fa, bg[3 + a])
        for c in range(3):
            if premultiplied:
                out[c] = (fg[c] + bg[c] * (ONE - fa)).astype(np.float32)
            else:
                out[c] = ((fg[c] * fa + bg[c] * bg[3 + a] * (ONE - fa)) * reciprocal(na)).astype(np.float32)
        out[3 + a] = na
    elif mode == MUL:
        for c in range(3):
            out[c] = mul_blend(bg[c], fg[c], clamp)
    else:
        raise ValueError(mode)
    return out


def blend(bg_color, bg_ec, fg_color, fg_ec, origin, color, ec, info, size=None):
    """bg_color: the colour's source canvas [H', W', 3] float32 (H' >= H, W' >= W) or None (an empty slot: zeroes);
    bg_ec: per extra channel the plane [H', W'] of ITS source slot or None; fg_color [fh, fw, 3], fg_ec [n, fh, fw]: the
    frame, placed with its first pixel at origin = (x0, y0), which may be negative or outside; size = (W, H) of the
    image (default: bg_color's).  Returns (colour [H, W, 3], planes [n, H, W]): inside the frame's rectangle
    PerformBlending, outside every channel's own background."""
    fg_color = np.asarray(fg_color, np.float32)
    fg_ec = np.asarray(fg_ec, np.float32)
    n = len(ec)
    assert fg_ec.shape == (n,) + fg_color.shape[:2] and len(bg_ec) == n and len(info) == n
    if size is None:
        size = (bg_color.shape[1], bg_color.shape[0])
    W, H = size
    out = np.zeros((H, W, 3), np.float32) if bg_color is None else np.array(bg_color[:H, :W], np.float32)
    planes = np.zeros((n, H, W), np.float32)
    for i in range(n):
        if bg_ec[i] is not None:
            planes[i] = bg_ec[i][:H, :W]
    assert out.shape == (H, W, 3), out.shape
    x0, y0, x1, y1 = rect(size, (fg_color.shape[1], fg_color.shape[0]), origin)
    if x1 <= x0 or y1 <= y0:
        return out, planes
    fs = (slice(y0 - origin[1], y1 - origin[1]), slice(x0 - origin[0], x1 - origin[0]))
    cs = (slice(y0, y1), slice(x0, x1))
    bg = [out[cs + (c,)].copy() for c in range(3)] + [planes[i][cs].copy() for i in range(n)]
    fg = [fg_color[fs + (c,)] for c in range(3)] + [fg_ec[i][fs] for i in range(n)]
    r = perform_blending(bg, fg, color, ec, info)
    for c in range(3):
        out[cs + (c,)] = r[c]
    for i in range(n):
        planes[i][cs] = r[3 + i]
    return out, planes


def blend_sequence(frames, size, info):
    """A still's coded frames through the reference's slots (dec_frame.cc:870-885: every frame but the last is saved
    into its save_as_reference slot, extra channels with the colour): frames = dicts with pixels = (colour [fh, fw, 3],
    planes [n, fh, fw]) and the header fields tests/alpha_layer_streams.splice_ec takes (crop, mode, clamp, source,
    alpha_channel, ec, save_as_reference).  Returns the last frame's (colour, planes) at image size."""
    n = len(info)
    slots = {}
    out = None
    for k, f in enumerate(frames):
        src = f.get("source", 0)
        ec = [dict(mode=e.get("mode", REPLACE), clamp=e.get("clamp", 0), alpha_channel=e.get("alpha_channel", 0),
                   source=e.get("source", src)) for e in (f.get("ec") or [{}] * n)]
        bg_color = slots[src][0] if src in slots else None
        bg_ec = [slots[e["source"]][1][i] if e["source"] in slots else None for i, e in enumerate(ec)]
        color = dict(mode=f.get("mode", REPLACE), clamp=f.get("clamp", 0), alpha_channel=f.get("alpha_channel", 0))
        out = blend(bg_color, bg_ec, f["pixels"][0], f["pixels"][1], f.get("crop") or (0, 0), color, ec, info, size=size)
        if k + 1 < len(frames):
            slots[f.get("save_as_reference", 0)] = out
    return out
