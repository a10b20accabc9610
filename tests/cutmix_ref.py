"""Host reference of CutMix / VideoMix (vl_cutmix_pairs, vl_cutmix_pairs_s2d, NetConfig.cutmix_alpha): the swap of one half-open
(t, y, x) box between clip i and clip clips - 1 - i on frames in their logical order, and the label weight.  The swap moves values and
computes nothing, so it is exact for any dtype; the device result is compared bit for bit with the feed of the swapped frames."""
import numpy as np


def clamp(box, fpc, h, w):
    """The box a device launch works on: every bound clamped to its axis; an axis that is then empty or reversed empties the box."""
    b = [min(max(int(v), 0), n) for v, n in zip(box, (fpc, fpc, h, h, w, w))]
    if b[0] >= b[1] or b[2] >= b[3] or b[4] >= b[5]:
        return (0, 0, 0, 0, 0, 0)
    return tuple(b)


def swap(x, box):
    """x [clips, fpc, h, w, c] -> a copy with the box (t0, t1, y0, y1, x0, x1) of clip i and clip clips - 1 - i exchanged, all channels.
    The middle clip of an odd count is its own partner and keeps its values."""
    x = np.asarray(x)
    assert x.ndim == 5
    t0, t1, y0, y1, x0, x1 = clamp(box, *x.shape[1:4])
    out = x.copy()
    out[:, t0:t1, y0:y1, x0:x1] = x[::-1, t0:t1, y0:y1, x0:x1]
    return out


def swap_frames(frames, clips, box):
    """swap on frames [clips * fpc, h, w, c], the layout the feeds take."""
    f = np.asarray(frames)
    return swap(f.reshape((clips, f.shape[0] // clips) + f.shape[1:]), box).reshape(f.shape)


def lam(box, fpc, h, w):
    """1 - volume / (fpc h w) from the integers in float64, rounded to the float32 the device word holds."""
    t0, t1, y0, y1, x0, x1 = (int(v) for v in box)
    vol = max(t1 - t0, 0) * max(y1 - y0, 0) * max(x1 - x0, 0)
    return float(np.float32(1.0 - vol / float(fpc * h * w)))
