"""Host reference of the random resized crop, in numpy fp64: the sampling rule of vl_input_prep_u8_box restated
(`sample_box`, `feed`), the kernel's documented clamp (`clamp_box`) and the draws of dataset_.resized_crop_boxes restated
(`draw_boxes`).  Imported by the CPU and GPU tests; nothing here touches the package's own implementation."""
import math

import numpy as np

SCALE, RATIO = (0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0)


def axis_taps(b, out):
    """Per output index of one axis: (i0, i1, f) from integers -- num = max((2 o + 1) b - out, 0) is 2 out times the source coordinate."""
    o = np.arange(out, dtype=np.int64)
    num = np.maximum((2 * o + 1) * b - out, 0)
    q, r = num // (2 * out), num % (2 * out)
    return np.minimum(q, b - 1), np.minimum(q + 1, b - 1), r.astype(np.float64) / float(2 * out)


def sample_box(frame, box, out_hw):
    """frame [H, W, C] (any real dtype), box (y0, x0, bh, bw) inside it -> fp64 [out_h, out_w, C]: bilinear, half-pixel centres,
    clamped to the box's edge, the horizontal lerp first."""
    y0, x0, bh, bw = (int(v) for v in box)
    p = np.asarray(frame, np.float64)[y0:y0 + bh, x0:x0 + bw]
    assert p.shape[:2] == (bh, bw) and bh >= 1 and bw >= 1, (box, np.shape(frame))
    i0, i1, fy = axis_taps(bh, out_hw[0])
    j0, j1, fx = axis_taps(bw, out_hw[1])
    fx, fy = fx[None, :, None], fy[:, None, None]
    lerp = lambda a, b, f: a * (1.0 - f) + b * f
    top = lerp(p[i0][:, j0], p[i0][:, j1], fx)
    bot = lerp(p[i1][:, j0], p[i1][:, j1], fx)
    return lerp(top, bot, fy)


def clamp_box(box, raw_h, raw_w):
    """The kernel's clamp: sizes into [1, raw] first, then the corner into [0, raw - size]."""
    y0, x0, bh, bw = (int(v) for v in box)
    bh, bw = min(max(bh, 1), raw_h), min(max(bw, 1), raw_w)
    return (min(max(y0, 0), raw_h - bh), min(max(x0, 0), raw_w - bw), bh, bw)


def feed(frames, boxes, out_hw, mirror=None, mean=None):
    """frames uint8 [n, H, W, C], boxes [n, 4] -> fp64 NHWC [n, out_h, out_w, C]: sample, mirror the output W axis, subtract the mean."""
    out = np.empty((len(frames),) + tuple(out_hw) + (frames.shape[3],), np.float64)
    for i, f in enumerate(frames):
        v = sample_box(f, boxes[i], out_hw)
        if mirror is not None and mirror[i]:
            v = v[:, ::-1]
        out[i] = v - (0.0 if mean is None else np.asarray(mean, np.float64))
    return out


def draw_boxes(seed, counter, clips, raw_h, raw_w, scale=SCALE, ratio=RATIO, mirror_on=True):
    """The draw rule restated: one Philox generator per (seed, counter), clip by clip; torchvision's get_params with up to 10 attempts,
    then the centred fallback; then the clip's mirror draw.  -> (boxes int32 [clips, 4], mirror uint8 [clips], fallback bool [clips])."""
    g = np.random.Generator(np.random.Philox(key=[seed, counter]))
    boxes, mirror, fell = np.zeros((clips, 4), np.int32), np.zeros(clips, np.uint8), np.zeros(clips, bool)
    for i in range(clips):
        done = False
        for _ in range(10):
            area = raw_h * raw_w * g.uniform(scale[0], scale[1])
            ar = math.exp(g.uniform(math.log(ratio[0]), math.log(ratio[1])))
            bw, bh = int(round(math.sqrt(area * ar))), int(round(math.sqrt(area / ar)))
            if 0 < bw <= raw_w and 0 < bh <= raw_h:
                y0 = int(g.integers(0, raw_h - bh + 1))
                x0 = int(g.integers(0, raw_w - bw + 1))
                done = True
                break
        if not done:
            fell[i] = True
            bh, bw = raw_h, raw_w
            if raw_w / raw_h < ratio[0]:
                bh = min(raw_h, max(1, int(round(raw_w / ratio[0]))))
            elif raw_w / raw_h > ratio[1]:
                bw = min(raw_w, max(1, int(round(raw_h * ratio[1]))))
            y0, x0 = (raw_h - bh) // 2, (raw_w - bw) // 2
        boxes[i] = (y0, x0, bh, bw)
        m = int(g.integers(2))
        mirror[i] = m if mirror_on else 0
    return boxes, mirror, fell
