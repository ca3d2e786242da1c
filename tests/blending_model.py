"""numpy restatement of frame blending on an image without an alpha channel: the reference's BlendingStage
(render_pipeline/stage_blending.cc: ProcessRow inside the frame's rectangle, ProcessPaddingRow outside) over
PerformBlending's colour modes (blending.cc:150-184) and PerformMulBlending (alpha.cc:82-93).  Every sample is ONE float32
operation on (bg, fg), so a kernel that does the same is bit-equal to this."""
import numpy as np

REPLACE, ADD, BLEND, ALPHA_WEIGHTED_ADD, MUL = range(5)  # BlendMode (frame_header.h)
MODES = (REPLACE, ADD, BLEND, ALPHA_WEIGHTED_ADD, MUL)


def rect(size, fsize, origin):
    """The frame's rectangle clipped to the image: (x0, y0, x1, y1), empty when x1 <= x0 or y1 <= y0."""
    (W, H), (fw, fh), (ox, oy) = size, fsize, origin
    return max(ox, 0), max(oy, 0), min(ox + fw, W), min(oy + fh, H)


def blend(bg, fg, origin, mode, clamp=False, size=None):
    """bg: the source canvas [H', W', 3] float32 with H' >= H, W' >= W, or None (an empty slot: zeroes); fg: the frame
    [fh, fw, 3] float32 placed with its first pixel at origin = (x0, y0), which may be negative or outside; size =
    (W, H) of the image (default: bg's).  Returns the blended image [H, W, 3] float32."""
    fg = np.asarray(fg, np.float32)
    if size is None:
        size = (bg.shape[1], bg.shape[0])
    W, H = size
    out = np.zeros((H, W, 3), np.float32) if bg is None else np.array(bg[:H, :W], np.float32)
    assert out.shape == (H, W, 3), out.shape
    x0, y0, x1, y1 = rect(size, (fg.shape[1], fg.shape[0]), origin)
    if x1 <= x0 or y1 <= y0:
        return out
    f = fg[y0 - origin[1]:y1 - origin[1], x0 - origin[0]:x1 - origin[0]]
    b = out[y0:y1, x0:x1]
    if mode in (REPLACE, BLEND):
        r = f
    elif mode in (ADD, ALPHA_WEIGHTED_ADD):
        r = b + f
    elif mode == MUL:
        # Clamp(fg) = Clamp1(fg, 0, 1): a NaN passes (np.clip does the same)
        r = b * (np.clip(f, np.float32(0), np.float32(1)) if clamp else f)
    else:
        raise ValueError(mode)
    out[y0:y1, x0:x1] = r.astype(np.float32)
    return out
