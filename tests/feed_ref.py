"""Restatements for the feed, layout and LSTM-dropout tests (no tests here), in numpy, from the layout formulas of include/vltf.h and
from no kernel:

crop_feed     vl_input_prep_u8's whole destination: pixel (y, x) of channel c in plane c * phase + (x + halo) % phase, row y + halo,
              column (x + halo) // phase; the other columns of the interior rows written 0.0; the halo rows not written at all.
packed_feed   vl_input_prep_u8_s2d's whole destination as int16 bits: element j of chunk (cb, R, S) is channel cp = 8 cb + j with
              px = cp % s, py = (cp // s) % s, c = cp // s^2 at pixel (s R + py - pt, s S + px - pl); +0 where c >= cin or the pixel is
              outside the frame; float32(u8) - float32(mean[c]) rounded to bf16, ties to even.
dropout_mask  vl_dropout_fwd's draw: h = splitmix64(seed ^ splitmix64(e)), kept iff (h >> 40) * 2^-24 < keep in float32.

`wrong` selects ONE deliberate defect (WRONG_CROP, WRONG_PACKED); tests/test_feed_geometry.py shows that the case lists of the GPU tests
tell every one of them from the reference, so a kernel with that defect could not pass."""
import numpy as np

from oracle import lrcn_oracle as O
from tests.fc_dropout_ref import splitmix64

MEAN = np.array([99.197148, 105.293620, 109.503945], np.float32)
TIE_MEAN = np.array([0.5, 0.25, 100.5], np.float32)          # u8 - 0.5 >= 128.5 and u8 - 100.5 >= 128.5 lie between two bf16 values
_M64 = (1 << 64) - 1

WRONG_CROP = ("mirror about the raw frame", "cy and cx swapped", "mean reversed", "phase plane x % phase")
WRONG_PACKED = ("mirror about the raw frame", "cy and cx swapped", "mean reversed", "py and px swapped", "pt and pl swapped", "truncation")


# ---- geometry -------------------------------------------------------------------------------------------------------------------------
def same_geometry(h, w, k, s):
    """TF 'SAME' for a k x k kernel at stride s: (oh, ow, pt, pl), the smaller half of the padding in front."""
    oh, ow = -(-h // s), -(-w // s)
    return oh, ow, max((oh - 1) * s + k - h, 0) // 2, max((ow - 1) * s + k - w, 0) // 2


def packed_dims(cin, k, s, oh, ow):
    """(chunks per pixel, rows, columns) of the packed space-to-depth input: ka = ceil(k / s)."""
    ka = -(-k // s)
    return -(-(cin * s * s) // 8), oh + ka - 1, ow + ka - 1


def c3s4_classes(w, pl, owp):
    """What the column quads S = 0 .. owp - 1 of the three-channel stride-4 kernel are to its `interior` test (4 S - pl >= 0 and
    4 S - pl + 3 < w): inside, cut by the left / right edge of the frame (the per-pixel path with some pixels valid), or wholly out."""
    out = set()
    for S in range(owp):
        a = 4 * S - pl
        if a >= 0 and a + 3 < w:
            out.add("interior")
        elif a < 0:
            out.add("left, cut" if a + 3 >= 0 else "left, outside")
        else:
            out.add("right, cut" if a < w else "right, outside")
    return out


# ---- pixel values -----------------------------------------------------------------------------------------------------------------------
def crops(rng, n, rh, rw, oh, ow):
    """Per-frame crop of the GPU tests: corners (all four from n = 6 on), then random offsets; mirror alternating, frame 0 unmirrored."""
    my, mx = rh - oh, rw - ow
    corners = [(0, 0), (my, 0), (0, mx), (my, mx)] if n >= 6 else [(0, 0), (my, mx)][:max(n - 1, 0)]
    yx = corners + [(int(rng.integers(0, my + 1)), int(rng.integers(0, mx + 1))) for _ in range(n - len(corners))]
    return np.array([p[0] for p in yx], np.int32), np.array([p[1] for p in yx], np.int32), (np.arange(n) % 2).astype(np.uint8)


def _frame(img, oh, ow, cy, cx, mir, mean, wrong):
    """float32 [oh, ow, c]: what conv1 sees of one raw frame -- Dataset.process_image -- or that with one defect."""
    rh, rw, c = img.shape
    mean = None if mean is None else np.asarray(mean, np.float32)
    if wrong == "cy and cx swapped":
        cy, cx = min(cx, rh - oh), min(cy, rw - ow)
    if wrong == "mean reversed" and mean is not None:
        mean = mean[::-1]
    if wrong == "mirror about the raw frame":
        v = (img[:, ::-1] if mir else img)[cy:cy + oh, cx:cx + ow].astype(np.float32)
        return v if mean is None else v - mean.reshape(1, 1, c)
    if c == 3:
        return O.process_image(img, (oh, ow, 3), (cy, cx), mean, bool(mir))
    v = img[cy:cy + oh, cx:cx + ow].astype(np.float32)                  # the same steps for another channel count
    if mean is not None:
        v = v - mean.reshape(1, 1, c)
    return v[:, ::-1] if mir else v


def _args(n, cy, cx, mir):
    z = np.zeros(n, np.int64)
    return (z if cy is None else np.asarray(cy)), (z if cx is None else np.asarray(cx)), (z if mir is None else np.asarray(mir))


# ---- vl_input_prep_u8 ------------------------------------------------------------------------------------------------------------------
def crop_feed(src, cy, cx, mir, mean, oh, ow, halo, phase, wrong=None):
    """-> (values float32 [n, 3 * phase, oh + 2 halo, ceil((ow + 2 halo) / phase)], written bool of that shape).  Where `written`
    is false the call leaves the destination as it was."""
    n = src.shape[0]
    hp, wq = oh + 2 * halo, -(-(ow + 2 * halo) // phase)
    val = np.zeros((n, 3 * phase, hp, wq), np.float32)
    written = np.zeros(val.shape, bool)
    written[:, :, halo:halo + oh, :] = True
    c, y, x = np.meshgrid(np.arange(3), np.arange(oh), np.arange(ow), indexing="ij")
    plane = x % phase if wrong == "phase plane x % phase" else (x + halo) % phase
    val[:, c * phase + plane, y + halo, (x + halo) // phase] = feed_frames(src, cy, cx, mir, mean, oh, ow, wrong).transpose(0, 3, 1, 2)
    return val, written


def expected_bits(val, written, sentinel):
    """uint32 image of the destination after the call into a sentinel-filled buffer."""
    return np.where(written, val.view(np.uint32), np.float32(sentinel).view(np.uint32)).reshape(-1)


# ---- bf16 ------------------------------------------------------------------------------------------------------------------------------
def bf16_bits(v, truncate=False):
    """int16 bit patterns of finite float32 values rounded to bf16, ties to even (truncate: the defect)."""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    if not truncate:
        u = u + np.uint64(0x7fff) + ((u >> np.uint64(16)) & np.uint64(1))
    return (u >> np.uint64(16)).astype(np.uint16).view(np.int16)


def is_bf16_tie(v):
    """Exactly between two bf16 values."""
    return (np.ascontiguousarray(v, np.float32).view(np.uint32) & 0xffff) == 0x8000


# ---- vl_input_prep_u8_s2d / vl_s2d_c8_from_x0 ----------------------------------------------------------------------------------------------
def pack_s2d(img, cin, h, w, k, s, pt, pl, oh, ow, wrong=None):
    """float32 frames [n, h, w, cin] as conv1 sees them -> int16 [n, chunks, oh + ka - 1, ow + ka - 1, 8]: every slot of the buffer."""
    n = img.shape[0]
    cb, ohp, owp = packed_dims(cin, k, s, oh, ow)
    if wrong == "pt and pl swapped":
        pt, pl = pl, pt
    cp = np.arange(cb * 8)
    px, py, c = cp % s, (cp // s) % s, cp // (s * s)
    if wrong == "py and px swapped":
        px, py = py, px
    ih = s * np.arange(ohp)[None, :] + py[:, None] - pt                   # [cp, R]
    iw = s * np.arange(owp)[None, :] + px[:, None] - pl                   # [cp, S]
    ok = (c < cin)[:, None, None] & ((ih >= 0) & (ih < h))[:, :, None] & ((iw >= 0) & (iw < w))[:, None, :]
    v = img[:, np.clip(ih, 0, h - 1)[:, :, None], np.clip(iw, 0, w - 1)[:, None, :], np.minimum(c, cin - 1)[:, None, None]]
    v = np.where(ok[None], v, np.float32(0)).astype(np.float32)            # [n, cp, R, S]
    bits = bf16_bits(v, truncate=wrong == "truncation")
    return np.ascontiguousarray(bits.reshape(n, cb, 8, ohp, owp).transpose(0, 1, 3, 4, 2))


def feed_frames(src, cy, cx, mir, mean, h, w, wrong=None):
    """float32 [n, h, w, cin]: the frames behind crop, mirror and mean."""
    n = src.shape[0]
    cy, cx, mir = _args(n, cy, cx, mir)
    return np.stack([_frame(src[i], h, w, int(cy[i]), int(cx[i]), bool(mir[i]), mean, wrong) for i in range(n)])


def packed_feed(src, cy, cx, mir, mean, cin, h, w, k, s, pt, pl, oh, ow, wrong=None):
    return pack_s2d(feed_frames(src, cy, cx, mir, mean, h, w, wrong), cin, h, w, k, s, pt, pl, oh, ow, wrong)


def x0_layout(img, halo, phase):
    """float32 frames [n, h, w, c] -> x0 as a strided conv takes it: zero halo, plain (phase 1) or column-phase-split."""
    n, h, w, c = img.shape
    hp, wq = h + 2 * halo, -(-(w + 2 * halo) // phase)
    x0 = np.zeros((n, c * phase, hp, wq), np.float32)
    x = np.arange(w)
    for ch in range(c):
        x0[:, (ch * phase + (x + halo) % phase)[None, :], (np.arange(h) + halo)[:, None], ((x + halo) // phase)[None, :]] = img[:, :, :, ch]
    return x0


# ---- vl_dropout_fwd ---------------------------------------------------------------------------------------------------------------------
def dropout_mask(seed, count, keep):
    """bool[count]: element e, counted from the pointer the launch gets, is kept."""
    h = splitmix64(np.uint64(int(seed) & _M64) ^ splitmix64(np.arange(count, dtype=np.uint64)))
    uni = (h >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)       # 24 bits: exact in float32
    return uni < np.float32(keep)


def st_seed(step):
    """The seed vl_dropout_fwd_st forms from the step state's count."""
    return ((int(step) << 20) ^ 0x5DEECE66D) & _M64


# ---- the case lists of tests/test_feed_geometry_gpu.py (tests/test_feed_geometry.py shows that they discriminate) -----------------------------
CROP_LAYOUTS = [(0, 1), (2, 1), (5, 4), (2, 4), (1, 3), (3, 4)]            # (halo, phase)
CROP_SIZES = [(17, 19), (1, 1), (9, 14), (8, 13)]                          # (oh, ow): ow + 2 halo a multiple of the phase and not
GENERIC = [(2, 9, 10, 5, 2), (3, 9, 10, 5, 2), (4, 11, 8, 9, 3)]           # (cin, h, w, k, s); (3, ...): the last chunk half used
REFUSED = (1, 7, 7, 3, 2)                                                  # ceil(3 / 2) = 2 is even: s2d_check refuses it, so it is not in GENERIC
C3S4_SWEEP = [(3, h, w, 11, 4) for h in (17, 18, 19, 20) for w in (20, 21, 22, 23)]
C3S4_FULL = (3, 227, 227, 11, 4)                                           # from 240 x 320 frames
S2D_ALONE = [(3, 19, 23, 11, 4), (2, 9, 10, 5, 2)]


def u8_frames(seed, n, rh, rw, c=3):
    return np.random.default_rng(seed).integers(0, 256, (n, rh, rw, c), dtype=np.uint8)


def crop_case(oh, ow, halo, phase, kind="crop"):
    """One vl_input_prep_u8 call as a dict.  kind: "crop" (6 frames of (oh + 3) x (ow + 5): four corners, two random offsets, mirror
    alternating), "no mean", "no offsets" (crop_y = crop_x = None, mirror given), "no room" (the raw frame is the output frame)."""
    rh, rw = (oh, ow) if kind == "no room" else (oh + 3, ow + 5)
    rng = np.random.default_rng(1000 * oh + 10 * ow + halo + phase)
    cy, cx, mir = crops(rng, 6, rh, rw, oh, ow)
    if kind == "no offsets":
        cy = cx = None
    return dict(name="%s %dx%d halo %d phase %d" % (kind, oh, ow, halo, phase), src=u8_frames(oh * 100 + ow, 6, rh, rw), cy=cy, cx=cx, mir=mir,
                mean=None if kind == "no mean" else MEAN, oh=oh, ow=ow, halo=halo, phase=phase)


def crop_cases(halo, phase):
    cases = [crop_case(oh, ow, halo, phase) for oh, ow in CROP_SIZES]
    if (halo, phase) in ((0, 1), (2, 4)):
        cases += [crop_case(17, 19, halo, phase, kind) for kind in ("no mean", "no offsets", "no room")]
    return cases


def crop_want(case, wrong=None):
    return crop_feed(case["src"], case["cy"], case["cx"], case["mir"], case["mean"], case["oh"], case["ow"], case["halo"], case["phase"], wrong)


def mean_of(cin, tie=False):
    return np.append(TIE_MEAN if tie else MEAN, np.float32(97.75))[:cin].astype(np.float32)


def packed_case(desc, tie=False):
    """One vl_input_prep_u8_s2d call as a dict.  Generic descriptors: 4 frames of (h + 3) x (w + 5), two corners and two random crops,
    mirror alternating.  Three channels at stride 4: 3 frames -- uncropped and unmirrored; the bottom-right corner, mirrored; a random
    crop, mirrored -- of (h + 3) x (w + 5), or 2 frames of 240 x 320 for the 227 x 227 layer."""
    cin, h, w, k, s = desc
    rng = np.random.default_rng(h * 1000 + w * 10 + cin + (5 if tie else 0))
    if cin == 3 and s == 4:
        rh, rw, n = (240, 320, 2) if desc == C3S4_FULL else (h + 3, w + 5, 3)
        cy = np.array([0, rh - h, rng.integers(0, rh - h + 1)], np.int32)[:n]
        cx = np.array([0, rw - w, rng.integers(0, rw - w + 1)], np.int32)[:n]
        mir = np.array([0, 1, 1], np.uint8)[:n]
    else:
        rh, rw, n = h + 3, w + 5, 4
        cy, cx, mir = crops(rng, n, rh, rw, h, w)
    return dict(name="%s%s" % (desc, " ties" if tie else ""), desc=desc, src=u8_frames(h * 100 + w + cin, n, rh, rw, cin), cy=cy, cx=cx, mir=mir,
                mean=mean_of(cin, tie))


def packed_cases():
    return ([packed_case(d) for d in GENERIC] + [packed_case(GENERIC[1], tie=True)] + [packed_case(d) for d in C3S4_SWEEP]
            + [packed_case(S2D_ALONE[0], tie=True)])


def packed_want(case, wrong=None):
    cin, h, w, k, s = case["desc"]
    oh, ow, pt, pl = same_geometry(h, w, k, s)
    return packed_feed(case["src"], case["cy"], case["cx"], case["mir"], case["mean"], cin, h, w, k, s, pt, pl, oh, ow, wrong)


def s2d_alone_frames(desc):
    """float32 [2, h, w, cin]: random normals scaled over a few binades, a quarter of them exactly between two bf16 values (both
    signs), some zeros of both signs."""
    cin, h, w, k, s = desc
    rng = np.random.default_rng(cin * 97 + h)
    v = (rng.standard_normal((2, h, w, cin)) * np.exp2(rng.integers(-3, 8, (2, h, w, cin)))).astype(np.float32)
    u = v.view(np.uint32)
    tie = rng.random(v.shape) < 0.25
    u[tie] = (u[tie] & np.uint32(0xffff0000)) | np.uint32(0x8000)
    zero = rng.random(v.shape) < 0.02
    u[zero] &= np.uint32(0x80000000)
    return v
