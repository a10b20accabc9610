"""Host reference of random erasing (vl_erase_boxes, vl_erase_boxes_s2d, NetConfig.erase_prob), written from the specification in
include/vltf.h and independently of vltf_amd.engine: splitmix64 and the four-field noise in uint64 / fp32 numpy (every bit of the
device's value), the clamp of a table row, the fill of a clip's box on frames in their logical order, the two layout maps, the
round-to-nearest-even bf16 packing, and the draw of a clip's row from its Philox stream."""
import math

import numpy as np

MODES = ("zero", "clip", "pixel")
SUM_STD = 37837.22723720648                      # sqrt(4 (65536^2 - 1) / 12): the deviation of a sum of four uniform 16-bit fields
CLIP_ELEMENT = 1 << 40


def splitmix64(z):
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def scale_of(std):
    """The fp32 factor the host passes: (float)(std / 37837.22723720648)."""
    return np.float32(float(std) / SUM_STD)


def noise(key, e, scale):
    """fp32 noise(key, e) for an array of element indices e: the centred four-field sum, an exact integer, times the fp32 scale."""
    h = splitmix64(np.uint64(int(key) & (2 ** 64 - 1)) ^ splitmix64(e))
    m = np.uint64(0xFFFF)
    s = (h & m) + ((h >> np.uint64(16)) & m) + ((h >> np.uint64(32)) & m) + (h >> np.uint64(48))
    return (s.astype(np.int64) - 131070).astype(np.float32) * np.float32(scale)


def key_of(row):
    """key_hi << 32 | key_lo of a table row, both words read as unsigned."""
    return ((int(row[7]) & 0xFFFFFFFF) << 32) | (int(row[6]) & 0xFFFFFFFF)


def key_words(key):
    """(key_lo, key_hi) as the int32 values that hold the halves' bits."""
    return tuple(int(np.array([v], np.uint32).view(np.int32)[0]) for v in (key & 0xFFFFFFFF, key >> 32))


def clamp(box, fpc, h, w):
    """The box a launch works on: every bound clamped to its axis; an axis that is then empty or reversed empties the box."""
    b = [min(max(int(v), 0), n) for v, n in zip(box[:6], (fpc, fpc, h, h, w, w))]
    if b[0] >= b[1] or b[2] >= b[3] or b[4] >= b[5]:
        return (0, 0, 0, 0, 0, 0)
    return tuple(b)


def fill(shape, key, mode, scale):
    """fp32 [fpc, h, w, c]: what a clip with this key holds wherever it is erased; the element index is the logical one."""
    fpc, h, w, c = shape
    if mode == 0:
        return np.zeros(shape, np.float32)
    if mode == 1:
        return np.broadcast_to(noise(key, np.uint64(CLIP_ELEMENT) + np.arange(c, dtype=np.uint64), scale), shape).copy()
    t, y, x, ch = np.meshgrid(np.arange(fpc), np.arange(h), np.arange(w), np.arange(c), indexing="ij")
    return noise(key, (((t * c + ch) * h + y) * w + x).astype(np.uint64), scale)


def mask(clips, fpc, h, w, table):
    """bool [clips, fpc, h, w]: the erased positions of every clip, from the clamped rows of the table."""
    m = np.zeros((clips, fpc, h, w), bool)
    for i in range(clips):
        t0, t1, y0, y1, x0, x1 = clamp(table[i], fpc, h, w)
        m[i, t0:t1, y0:y1, x0:x1] = True
    return m


def erase(x, table, mode, scale):
    """x fp32 [clips, fpc, h, w, c] -> a copy with every clip's box overwritten, all channels."""
    x = np.asarray(x, np.float32)
    clips, fpc, h, w, c = x.shape
    out = x.copy()
    m = mask(clips, fpc, h, w, table)
    for i in range(clips):
        if m[i].any():
            out[i][m[i]] = fill((fpc, h, w, c), key_of(table[i]), mode, scale)[m[i]]
    return out


def erase_frames(frames, clips, table, mode, scale):
    """erase on fp32 frames [clips * fpc, h, w, c], the layout the feeds take."""
    f = np.asarray(frames, np.float32)
    return erase(f.reshape((clips, f.shape[0] // clips) + f.shape[1:]), table, mode, scale).reshape(f.shape)


def bf16_bits(v):
    """uint16 bits of fp32 values rounded to bf16 to nearest even (finite values)."""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def x0_index(clips, fpc, h, w, halo, phase, c=3):
    """flat index into x0 of logical element [frame, y, x, c]: plane c * phase + (x + halo) % phase, row y + halo, column
    (x + halo) // phase (x0_index of tests/test_cutmix_gpu.py)."""
    hp, wq = h + 2 * halo, -(-(w + 2 * halo) // phase)
    f, y, x, ch = np.meshgrid(np.arange(clips * fpc), np.arange(h), np.arange(w), np.arange(c), indexing="ij")
    return ((f * c * phase + ch * phase + (x + halo) % phase) * hp + y + halo) * wq + (x + halo) // phase


def s2d_index(clips, fpc, cin, h, w, k, s, oh, ow):
    """flat 16-bit index into the packed space-to-depth input of logical element [frame, y, x, c] (s2d_index of
    tests/test_cutmix_gpu.py): chunk cb = cp // 8, element cp % 8 with cp = (c s + py) s + px, chunk row R = (y + pt) // s,
    py = (y + pt) % s, likewise S, px; TF SAME padding puts the smaller half in front."""
    ka = (k - 1) // s + 1
    ohp, owp, cb_n = oh + ka - 1, ow + ka - 1, -(-(cin * s * s) // 8)
    pt, pl = max((oh - 1) * s + k - h, 0) // 2, max((ow - 1) * s + k - w, 0) // 2
    f, y, x, c = np.meshgrid(np.arange(clips * fpc), np.arange(h), np.arange(w), np.arange(cin), indexing="ij")
    cp = (c * s + (y + pt) % s) * s + (x + pl) % s
    return ((((f * cb_n + cp // 8) * ohp + (y + pt) // s) * owp + (x + pl) // s) * 8 + cp % 8)


def erase_row(prob, scale, ratio, frames, seed, draw_index, global_clip, fpc, h, w):
    """The eight ints of one clip's row.  Philox keyed (seed, draw_index) with the counter (global_clip, 0, 0, 0); in this order: the
    64-bit key (always); u (erased iff u < prob); up to 10 attempts of torchvision's get_params, the accepted one followed by its
    corner; the frame run.  No accepted attempt, or not erased: six zeros and the key."""
    bg = np.random.Philox(key=np.array([seed, draw_index], dtype=np.uint64), counter=np.array([global_clip, 0, 0, 0], dtype=np.uint64))
    g = np.random.Generator(bg)
    key = int(g.integers(0, 2 ** 64, dtype=np.uint64))
    box = [0] * 6
    u = g.random()
    if u < prob:
        for _attempt in range(10):
            area = h * w * g.uniform(scale[0], scale[1])
            r = math.exp(g.uniform(math.log(ratio[0]), math.log(ratio[1])))
            bh = int(round(math.sqrt(area * r)))
            bw = int(round(math.sqrt(area / r)))
            if not (0 < bh < h and 0 < bw < w):
                continue
            y0 = int(g.integers(h - bh + 1))
            x0 = int(g.integers(w - bw + 1))
            length = max(1, int(round(fpc * g.uniform(frames[0], frames[1]))))
            t0 = int(g.integers(fpc - length + 1))
            box = [t0, t0 + length, y0, y0 + bh, x0, x0 + bw]
            break
    return tuple(box) + key_words(key)
