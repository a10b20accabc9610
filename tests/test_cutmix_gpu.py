"""CutMix / VideoMix on the device (vl_cutmix_pairs, vl_cutmix_pairs_s2d, NetConfig.cutmix_alpha): the in-place box swap in both
layouts conv1 reads against the feed of host-swapped frames (tests/cutmix_ref.py), bit for bit over the whole buffer; special values
and untouched bytes against a host map written from the layout formulas; refusals that launch nothing and device boxes that are
clamped; whole steps of LRCNEngine (override, odd clip count with label smoothing, per-frame head, a drawn temporal box, captured,
replayed with another box, accumulated, the bf16 conv path, mixup and CutMix together) against the fp64 oracle fed the host-swapped
frames and the mixed labels, and run_task on the example.

Tolerances.  The swap computes nothing: every comparison of buffers is of bits.  Whole steps against the fp64 oracle hold the bounds
of tests/test_mixup_gpu.py::check_step, which are those of tests/test_engine_gpu.py::test_train_step_small (loss 1e-4 * max(1, |loss|),
gradient norm 1e-3 relative, parameters rtol 1e-4 and atol 1e-5, logits rtol 1e-3 and atol 1e-3)."""
import glob
import os
import re

import numpy as np
import pytest
import torch
import yaml

from oracle import lrcn_oracle as O
from tests import cutmix_ref as CM
from tests import label_smoothing_ref as LS
from tests import mixup_ref as MX
from tests.test_label_smoothing_gpu import B, CLIP, FPC, LR, MEAN, SHAPE, bits, data, dev_batch, small_cfg
from tests.test_mixup_gpu import check_step, same_bits, step_keys_equal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = SHAPE[:2]
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def ops():
    import vltf_amd.ops as ops_
    return ops_


def dbox(box):
    return torch.tensor(list(box), dtype=torch.int32, device=DEV)


# ---- 1. the fp32 launch against the feed of the host-swapped frames ------------------------------------------------------------------------
FH, FW, FFPC = 9, 11, 3
BOXES = [(0, 0, 0, 0, 0, 0), (0, 3, 4, 4, 0, 11), (0, FFPC, 0, FH, 0, FW), (0, 1, 0, 1, 0, 1), (2, 3, 0, 1, 10, 11), (0, 1, 8, 9, 0, 1),
         (2, 3, 8, 9, 10, 11), (0, 3, 1, 6, 3, 10), (1, 2, 0, 9, 0, 11)]
_FRAMES = {}


def frames_u8(clips, fpc, h, w, c=3):
    """[clips * fpc, h, w, c] uint8, made once per shape and never written."""
    key = (clips, fpc, h, w, c)
    if key not in _FRAMES:
        _FRAMES[key] = np.random.default_rng(clips * 1009 + h * 31 + w + c).integers(0, 256, (clips * fpc, h, w, c), dtype=np.uint8)
    return _FRAMES[key]


def feed_x0(ops, frames, h, w, halo, phase, crop=None):
    """vl_input_prep_u8 into a sentinel-filled x0: the halo rows, which the feed does not write, keep the sentinel."""
    n = frames.shape[0]
    x0 = torch.full(ops.phase_split_shape(n, 3, h, w, halo, phase), SENTINEL, device=DEV)
    cy, cx, mir = crop if crop is not None else (None, None, None)
    ops.input_prep_u8(torch.from_numpy(frames).to(DEV), x0, cy, cx, mir, torch.from_numpy(MEAN).to(DEV), halo=halo, phase=phase,
                      out_hw=(h, w))
    return x0


@pytest.mark.parametrize("halo,phase", [(0, 1), (2, 1), (2, 4)])
@pytest.mark.parametrize("clips", [1, 2, 3, 4])
def test_cutmix_pairs_f32(ops, clips, halo, phase):
    f = frames_u8(clips, FFPC, FH, FW)
    for box in BOXES:
        want = feed_x0(ops, CM.swap_frames(f, clips, box), FH, FW, halo, phase)
        got = feed_x0(ops, f, FH, FW, halo, phase)
        ops.cutmix_pairs(got, clips, FFPC, (FH, FW), halo, phase, box)
        assert torch.equal(bits(got), bits(want)), (box, "host box")                      # the WHOLE buffer: halo and phase padding too
        got2 = feed_x0(ops, f, FH, FW, halo, phase)
        ops.cutmix_pairs(got2, clips, FFPC, (FH, FW), halo, phase, dbox(box))
        assert torch.equal(bits(got2), bits(want)), (box, "device box")
        vol = (box[1] - box[0]) * (box[3] - box[2]) * (box[5] - box[4])
        if vol > 0 and clips > 1:
            assert not torch.equal(bits(got), bits(feed_x0(ops, f, FH, FW, halo, phase)))   # and something moved


def test_cutmix_pairs_f32_after_crop_and_mirror(ops):
    """The box is in the coordinates of the frame conv1 sees: the reference crops and mirrors on the host, swaps, and feeds without."""
    clips, rh, rw = 4, 13, 15
    rng = np.random.default_rng(17)
    raw = rng.integers(0, 256, (clips * FFPC, rh, rw, 3), dtype=np.uint8)
    cy, cx = rng.integers(0, rh - FH + 1, clips * FFPC).astype(np.int32), rng.integers(0, rw - FW + 1, clips * FFPC).astype(np.int32)
    mir = rng.integers(0, 2, clips * FFPC).astype(np.uint8)
    assert mir.any() and not mir.all()
    seen = np.stack([raw[i, cy[i]:cy[i] + FH, cx[i]:cx[i] + FW][:, ::-1 if mir[i] else 1] for i in range(clips * FFPC)])
    crop = tuple(torch.from_numpy(a).to(DEV) for a in (cy, cx, mir))
    for box in ((0, 3, 1, 6, 3, 10), (1, 3, 2, 9, 0, 5)):
        got = feed_x0(ops, raw, FH, FW, 2, 4, crop)
        ops.cutmix_pairs(got, clips, FFPC, (FH, FW), 2, 4, box)
        want = feed_x0(ops, CM.swap_frames(np.ascontiguousarray(seen), clips, box), FH, FW, 2, 4)
        assert torch.equal(bits(got), bits(want)), box


# ---- 2. the packed launch against the packed feed of the host-swapped frames ----------------------------------------------------------------
DESCS = {"conv1-like": (3, 19, 23, 11, 4), "generic": (2, 9, 10, 5, 2), "half-used last chunk": (3, 9, 10, 5, 2)}   # cin, h, w, k, stride
S2D_BOXES = {"conv1-like": [(0, 0, 0, 0, 0, 0), (0, 3, 0, 19, 0, 23), (0, 3, 1, 6, 3, 10), (1, 3, 5, 18, 2, 21), (0, 2, 7, 8, 9, 10),
                            (0, 1, 0, 1, 0, 1), (2, 3, 18, 19, 22, 23), (1, 2, 0, 19, 0, 23), (0, 3, 4, 12, 8, 16)],
             "generic": [(0, 0, 0, 0, 0, 0), (0, 3, 0, 9, 0, 10), (0, 3, 1, 6, 3, 10), (1, 2, 3, 4, 5, 6), (0, 1, 0, 1, 0, 1),
                         (2, 3, 8, 9, 9, 10), (0, 3, 2, 8, 2, 8)],
             "half-used last chunk": [(0, 0, 0, 0, 0, 0), (0, 3, 0, 9, 0, 10), (0, 3, 1, 6, 3, 10), (1, 2, 3, 4, 5, 6)]}


def s2d_desc(ops, name):
    cin, h, w, k, s = DESCS[name]
    conv = ops.Conv(cin, h, w, 8, k, k, s, 1)
    conv.set_halo(conv.same_pad(), 0, 0, 0)
    ka = (k - 1) // s + 1
    return conv, (cin * s * s, conv.oh, conv.ow, (ka - 1) // 2)


def feed_xb(ops, conv, geom, frames):
    """vl_input_prep_u8_s2d into a fresh packed buffer (the feed writes every chunk)."""
    n = frames.shape[0]
    xb = torch.zeros(ops.c8_shape(n, *geom), dtype=torch.bfloat16, device=DEV)
    mean = torch.tensor([99.2, 105.3, 109.5][:conv.cin], device=DEV)
    conv.input_prep_u8_s2d(torch.from_numpy(frames).to(DEV), xb, None, None, None, mean)
    return xb


def bits16(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("name", list(DESCS))
@pytest.mark.parametrize("clips", [1, 2, 3, 4])
def test_cutmix_pairs_s2d(ops, name, clips):
    conv, geom = s2d_desc(ops, name)
    cin, h, w, k, s = DESCS[name]
    f = frames_u8(clips, FFPC, h, w, cin)
    plain = feed_xb(ops, conv, geom, f)
    for box in S2D_BOXES[name]:
        want = feed_xb(ops, conv, geom, CM.swap_frames(f, clips, box))
        got = plain.clone()
        conv.cutmix_pairs_s2d(got, clips, FFPC, box)
        assert torch.equal(bits16(got), bits16(want)), (box, "host box")
        got2 = plain.clone()
        conv.cutmix_pairs_s2d(got2, clips, FFPC, dbox(box))
        assert torch.equal(bits16(got2), bits16(want)), (box, "device box")
        vol = (box[1] - box[0]) * (box[3] - box[2]) * (box[5] - box[4])
        if vol > 0 and clips > 1:
            assert not torch.equal(bits16(got), bits16(plain))
    assert any(b[2] % s or b[3] % s or b[4] % s or b[5] % s for b in S2D_BOXES[name])      # edges that cut through a chunk


# ---- 3. special values and untouched bytes, against a host map written from the layout formulas ---------------------------------------------
def x0_index(clips, fpc, h, w, halo, phase):
    """flat index into x0 of logical element [frame, y, x, c]: plane c * phase + (x + halo) % phase, row y + halo, column (x + halo) // phase."""
    hp, wq = h + 2 * halo, -(-(w + 2 * halo) // phase)
    f, y, x, c = np.meshgrid(np.arange(clips * fpc), np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    return ((f * 3 * phase + c * phase + (x + halo) % phase) * hp + y + halo) * wq + (x + halo) // phase


def special_words(n, seed):
    """n 32-bit patterns: random bits (NaN payloads among them), with -0.0, both infinities and two quiet / signalling NaNs sprinkled in."""
    rng = np.random.default_rng(seed)
    u = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x80000000, 0x7f800000, 0xff800000, 0x7fc00001, 0x7f800123, 0xffc0beef, 0x00000001], np.uint32)
    u[rng.integers(0, n, n // 3)] = special[rng.integers(0, len(special), n // 3)]
    return u


@pytest.mark.parametrize("halo,phase", [(0, 1), (2, 4), (1, 3)])
def test_cutmix_pairs_f32_special_values_and_untouched_bytes(ops, halo, phase):
    clips = 3
    shape = ops.phase_split_shape(clips * FFPC, 3, FH, FW, halo, phase)
    u = special_words(int(np.prod(shape)), 5 + phase)
    idx = x0_index(clips, FFPC, FH, FW, halo, phase).reshape(clips, FFPC, FH, FW, 3)
    assert len(np.unique(idx)) == idx.size and idx.max() < u.size
    for box in ((0, 3, 1, 6, 3, 10), (1, 2, 0, 9, 0, 11), (0, FFPC, 0, FH, 0, FW)):
        want = u.copy()
        logical = u[idx]
        want[idx] = CM.swap(logical, box)                                                  # everything outside idx, and outside the box: as it was
        for b in (box, dbox(box)):
            got = torch.from_numpy(u.view(np.int32).copy()).to(DEV).view(torch.float32).view(shape)
            ops.cutmix_pairs(got, clips, FFPC, (FH, FW), halo, phase, b)
            assert np.array_equal(got.view(torch.int32).cpu().numpy().reshape(-1).view(np.uint32), want), box
        assert not np.array_equal(want, u)


def s2d_index(clips, fpc, cin, h, w, k, s, conv):
    """(flat 16-bit index into the packed input, validity) of logical element [frame, y, x, c]: chunk cb = cp // 8, element cp % 8 with
    cp = (c s + py) s + px, chunk row R = (y + pt) // s, py = (y + pt) % s, likewise S, px."""
    ka = (k - 1) // s + 1
    ohp, owp, cb_n = conv.oh + ka - 1, conv.ow + ka - 1, -(-(cin * s * s) // 8)

    def before(n, out):                                                                   # TF SAME: the smaller half goes in front
        return max((out - 1) * s + k - n, 0) // 2
    pt, pl = before(h, conv.oh), before(w, conv.ow)
    f, y, x, c = np.meshgrid(np.arange(clips * fpc), np.arange(h), np.arange(w), np.arange(cin), indexing="ij")
    cp = (c * s + (y + pt) % s) * s + (x + pl) % s
    return ((((f * cb_n + cp // 8) * ohp + (y + pt) // s) * owp + (x + pl) // s) * 8 + cp % 8)


@pytest.mark.parametrize("name", list(DESCS))
def test_cutmix_pairs_s2d_special_patterns_and_untouched_bytes(ops, name):
    """Random 16-bit patterns (bf16 NaNs, infinities and -0 among them) in EVERY slot of the buffer, the slots no pixel maps to
    included; the box comes back exchanged and every other slot as it was."""
    conv, geom = s2d_desc(ops, name)
    cin, h, w, k, s = DESCS[name]
    clips = 3
    shape = ops.c8_shape(clips * FFPC, *geom)
    rng = np.random.default_rng(23)
    u = rng.integers(0, 2 ** 16, int(np.prod(shape)), dtype=np.uint64).astype(np.uint16)
    u[rng.integers(0, u.size, u.size // 4)] = np.array([0x8000, 0x7f80, 0xff80, 0x7fc1, 0x7f81], np.uint16)[rng.integers(0, 5, u.size // 4)]
    idx = s2d_index(clips, FFPC, cin, h, w, k, s, conv).reshape(clips, FFPC, h, w, cin)
    assert len(np.unique(idx)) == idx.size and idx.max() < u.size
    # the map is the feed's: a feed of frames with one marked pixel puts it where the map says
    f = np.zeros((clips * FFPC, h, w, cin), np.uint8)
    f[4, h - 2, w - 3, cin - 1] = 200
    fed = feed_xb(ops, conv, (geom[0], geom[1], geom[2], geom[3]), f).view(-1).float().cpu().numpy()
    assert fed[idx[1, 1, h - 2, w - 3, cin - 1]] > 0 and np.count_nonzero(fed > 0) == 1
    for box in S2D_BOXES[name][1:4]:
        want = u.copy()
        want[idx] = CM.swap(u[idx], box)
        for b in (box, dbox(box)):
            got = torch.from_numpy(u.view(np.int16).copy()).to(DEV).view(torch.bfloat16).view(shape)
            conv.cutmix_pairs_s2d(got, clips, FFPC, b)
            assert np.array_equal(got.view(torch.int16).cpu().numpy().reshape(-1).view(np.uint16), want), box
        assert not np.array_equal(want, u)


# ---- 4. refusals launch nothing; a device box is clamped -----------------------------------------------------------------------------------
def test_refusals_launch_nothing(ops):
    from vltf_amd import _ffi
    from vltf_amd._ffi import VltfError
    import ctypes
    clips, halo, phase = 2, 2, 4
    x0 = torch.full(ops.phase_split_shape(clips * FFPC, 3, FH, FW, halo, phase), SENTINEL, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def hb(*v):
        return (ctypes.c_int32 * 6)(*v)
    ok = dict(x=x0.data_ptr(), clips=clips, fpc=FFPC, h=FH, w=FW, halo=halo, phase=phase, box=hb(0, 3, 1, 6, 3, 10))
    for change, msg in ((dict(x=None), "x0 is null"), (dict(box=None), "both box pointers are null"), (dict(clips=-1), "clips must be >= 0"),
                        (dict(fpc=0), "fpc must lie in"), (dict(h=0), "bad frame size"), (dict(halo=-1), "halo must be >= 0"),
                        (dict(phase=0), "phase must be >= 1"), (dict(box=hb(0, 4, 1, 6, 3, 10)), "t range .* leaves"),
                        (dict(box=hb(0, 3, -1, 6, 3, 10)), "y range .* leaves"), (dict(box=hb(0, 3, 1, 6, 3, 12)), "x range .* leaves"),
                        (dict(box=hb(0, 3, 6, 1, 3, 10)), "y range .* is reversed")):
        a = dict(ok, **change)
        with pytest.raises(VltfError, match=msg):
            _ffi.call("vl_cutmix_pairs", a["x"], a["clips"], a["fpc"], a["h"], a["w"], a["halo"], a["phase"], a["box"], None, st)
    with pytest.raises(VltfError, match="is not 2 clips of 3 frames"):
        ops.cutmix_pairs(x0[:3], clips, FFPC, (FH, FW), halo, phase, (0, 3, 1, 6, 3, 10))
    with pytest.raises(VltfError, match="float32"):
        ops.cutmix_pairs(x0.double(), clips, FFPC, (FH, FW), halo, phase, (0, 3, 1, 6, 3, 10))
    for bad in (torch.zeros(5, dtype=torch.int32, device=DEV), torch.zeros(6, device=DEV), torch.zeros(6, dtype=torch.int32)):
        with pytest.raises(VltfError, match="six contiguous int32 words"):
            ops.cutmix_pairs(x0, clips, FFPC, (FH, FW), halo, phase, bad)
    conv, geom = s2d_desc(ops, "generic")
    xb = torch.full(ops.c8_shape(clips * FFPC, *geom), 3.0, dtype=torch.bfloat16, device=DEV)
    for args, msg in (((conv._d, None, clips, FFPC, hb(0, 1, 0, 1, 0, 1), None), "xb is null"),
                      ((conv._d, xb.data_ptr(), clips, FFPC, None, None), "both box pointers are null"),
                      ((conv._d, xb.data_ptr(), -2, FFPC, hb(0, 1, 0, 1, 0, 1), None), "clips must be >= 0"),
                      ((conv._d, xb.data_ptr(), clips, -1, hb(0, 1, 0, 1, 0, 1), None), "fpc must lie in"),
                      ((None, xb.data_ptr(), clips, FFPC, hb(0, 1, 0, 1, 0, 1), None), "a strided, ungrouped, square layer"),
                      ((conv._d, xb.data_ptr(), clips, FFPC, hb(0, 1, 0, 10, 0, 1), None), "y range .* leaves"),
                      ((conv._d, xb.data_ptr(), clips, FFPC, hb(0, 1, 0, 1, 0, 11), None), "x range .* leaves"),
                      ((conv._d, xb.data_ptr(), clips, FFPC, hb(2, 1, 0, 1, 0, 1), None), "t range .* is reversed")):
        with pytest.raises(VltfError, match=msg):
            _ffi.call("vl_cutmix_pairs_s2d", *args, st)
    plain = ops.Conv(3, 9, 9, 8, 3, 3, 1, 1)                                              # unit stride: no space-to-depth input
    with pytest.raises(VltfError, match="a strided, ungrouped, square layer"):
        _ffi.call("vl_cutmix_pairs_s2d", plain._d, xb.data_ptr(), clips, FFPC, hb(0, 1, 0, 1, 0, 1), None, st)
    with pytest.raises(VltfError, match="packed input of 2 clips of 3 frames"):
        conv.cutmix_pairs_s2d(xb[:4], clips, FFPC, (0, 1, 0, 1, 0, 1))
    # nothing to pair: accepted, nothing launched
    ops.cutmix_pairs(x0[:FFPC], 1, FFPC, (FH, FW), halo, phase, (0, 3, 1, 6, 3, 10))
    conv.cutmix_pairs_s2d(xb[:FFPC], 1, FFPC, (0, 3, 1, 6, 3, 10))
    torch.cuda.synchronize()
    assert bool((x0 == SENTINEL).all()) and bool((xb == 3.0).all())


@pytest.mark.parametrize("words", [(-5, 99, -1, 6, 3, 400), (2, 1, 0, 9, 0, 11), (0, 3, 7, 2, 0, 11), (0, 3, 0, 9, 11, 11),
                                   (-2 ** 31, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1), (2 ** 31 - 1, -2 ** 31, 0, 9, 0, 11),
                                   (5, 9, 0, 9, 0, 11), (0, 3, 2 ** 30, 2 ** 31 - 1, 0, 11), (0, 3, -2 ** 31, -2 ** 30, 0, 11)])
def test_a_device_box_is_clamped_to_the_frame(ops, words):
    """Defined behaviour: whatever the six device words hold, the launch swaps the clamped box and touches nothing else."""
    clips = 4
    f = frames_u8(clips, FFPC, FH, FW)
    want = feed_x0(ops, CM.swap_frames(f, clips, CM.clamp(words, FFPC, FH, FW)), FH, FW, 2, 4)
    got = feed_x0(ops, f, FH, FW, 2, 4)
    ops.cutmix_pairs(got, clips, FFPC, (FH, FW), 2, 4, dbox(words))
    assert torch.equal(bits(got), bits(want))
    conv, geom = s2d_desc(ops, "generic")
    cin, h, w, k, s = DESCS["generic"]
    f2 = frames_u8(clips, FFPC, h, w, cin)
    want2 = feed_xb(ops, conv, geom, CM.swap_frames(f2, clips, CM.clamp(words, FFPC, h, w)))
    got2 = feed_xb(ops, conv, geom, f2)
    conv.cutmix_pairs_s2d(got2, clips, FFPC, dbox(words))
    assert torch.equal(bits16(got2), bits16(want2))


# ---- 5. engine steps against the fp64 oracle (the geometry of tests/test_mixup_gpu.py) ------------------------------------------------------
BOX = (0, 3, 10, 40, 20, 63)                     # 3 x 30 x 43 of 3 x 67 x 67: lam = 1 - 3870 / 13467
_ORACLE = {}


def oracle_step(clips, box, eps=0.0):
    """O.lrcn_train_step fed the frames of the first `clips` clips swapped on the host and their mixed labels; once per case."""
    p, frames, onehot = data()
    if (clips, box, eps) not in _ORACLE:
        x = (frames[:clips * FPC].astype(np.float32) - MEAN).reshape((clips, FPC) + SHAPE)
        lam = CM.lam(box, FPC, H, W)
        _ORACLE[(clips, box, eps)] = O.lrcn_train_step(p, CM.swap(x, box).reshape((clips * FPC,) + SHAPE), MX.targets(onehot[:clips], lam, eps),
                                                       FPC, lr=LR, clip_norm=CLIP)
    return _ORACLE[(clips, box, eps)]


def test_engine_step_with_a_box_override():
    from vltf_amd._ffi import VltfError
    from vltf_amd.engine import LRCNEngine
    p, _, onehot = data()
    assert not np.array_equal(onehot[0], onehot[1])
    eng = LRCNEngine(small_cfg(cutmix_alpha=1.0, cutmix_seed=7), max_clips=B, device=DEV)
    eng.load_params(p)
    assert eng.cut_box is not None and eng.cut_box.dtype == torch.int32 and eng.cut_box.numel() == 6 and eng.blend_lam is None
    assert eng.mix_lam.numel() == 1 and eng.stats.numel() == 3 and eng.loss_rows.numel() == 3 * B
    for bad, msg in (((0, 4, 0, 1, 0, 1), "leaves the frame"), ((0, 3, 5, 4, 0, 1), "is reversed"), ((0, 3, 0, 67, 0, 34), "above half the clip"),
                     ((0, 3, 0, 1, 0), "six whole numbers")):
        with pytest.raises(VltfError, match=msg):
            eng.train_step_u8(*dev_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, cut_box=bad)
    with pytest.raises(VltfError, match="mix_lambda is given, but mixup is off"):
        eng.train_step_u8(*dev_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, mix_lambda=0.7)
    assert eng.step_count == 0
    out = eng.train_step_u8(*dev_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, cut_box=BOX)
    lam = CM.lam(BOX, FPC, H, W)
    assert eng.cut_box_last == BOX and eng.mix_lambda_last == lam and float(eng.mix_lam) == np.float32(lam)
    assert eng.cut_box.cpu().tolist() == list(BOX)
    check_step(out, eng, oracle_step(B, BOX), onehot[:B])
    from tests.test_mixup_gpu import oracle_step as mixup_oracle
    uncut = mixup_oracle(B, 1.0)
    assert abs(out["loss"] - uncut[1]) > 1e-3 * abs(uncut[1])                          # and it is not the uncut step
    # the same step from fp32 frames: cut in x0
    again = LRCNEngine(small_cfg(cutmix_alpha=1.0, cutmix_seed=7), max_clips=B, device=DEV)
    again.load_params(p)
    frames, labels = dev_batch(0, B)
    x = frames.float() - torch.from_numpy(MEAN).to(DEV)
    out2 = again.train_step_f32(x, labels, lr=LR, clip_norm=CLIP, cut_box=BOX)
    check_step(out2, again, oracle_step(B, BOX), onehot[:B])
    # a forward-only engine ignores the option
    infer = LRCNEngine(small_cfg(cutmix_alpha=1.0, cutmix_seed=7), max_clips=B, device=DEV, training=False)
    assert infer.mix_lam is None and infer.cut_box is None and infer.cutmix_alpha == 0.0 and infer.stats.numel() == 2
    with pytest.raises(VltfError, match="cut_box and mix_lambda are given together"):
        both = LRCNEngine(small_cfg(cutmix_alpha=1.0, mixup_alpha=0.2), max_clips=B, device=DEV)
        both.train_step_u8(*dev_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, cut_box=BOX, mix_lambda=0.7)


def test_engine_with_label_smoothing_top_k_and_an_odd_clip_count():
    from vltf_amd.engine import LRCNEngine
    p, _, onehot = data()
    eng = LRCNEngine(small_cfg(cutmix_alpha=1.0, label_smoothing=0.1, top_k=2), max_clips=3, device=DEV)
    eng.load_params(p)
    out = eng.train_step_u8(*dev_batch(0, 3), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, cut_box=BOX)
    check_step(out, eng, oracle_step(3, BOX, 0.1), onehot[:3])
    assert out["topk_correct"] == float(LS.topk_hits(eng.logits_host(), onehot[:3], 2).sum())


def test_engine_per_frame_fc_head():
    """classifier fc without frame fusion: one logits row per FRAME, every row of a clip under the clip's weight (VideoMix's rule)."""
    from vltf_amd.engine import LRCNEngine
    ncls = 11
    rng = np.random.default_rng(12)
    cfg = small_cfg(num_classes=ncls, classifier="fc", frame_fusion=None, cutmix_alpha=1.0, cutmix_mode="cuboid")
    p = O.init_params(rng, ncls, "fc6", cfg.lstm_hidden, 1, SHAPE, classifier="fc", well_scaled=True)
    frames = rng.integers(0, 256, (B * FPC,) + SHAPE, dtype=np.uint8)
    onehot = O.labels_to_one_hot([[l] for l in rng.integers(0, ncls, B * FPC)], ncls)
    box = (1, 3, 5, 50, 8, 30)
    lam = CM.lam(box, FPC, H, W)
    x = (frames.astype(np.float32) - MEAN).reshape((B, FPC) + SHAPE)
    want = O.lrcn_train_step(p, CM.swap(x, box).reshape((B * FPC,) + SHAPE), MX.targets(onehot, lam, 0.0, FPC), FPC, lr=LR, clip_norm=CLIP,
                             classifier="fc", frame_fusion=None)
    eng = LRCNEngine(cfg, max_clips=B, device=DEV)
    eng.load_params(p)
    out = eng.train_step_u8(torch.tensor(frames, device=DEV), torch.tensor(onehot, device=DEV), lr=LR, clip_norm=CLIP, mean_bgr=MEAN,
                            cut_box=box)
    assert out["rows"] == B * FPC
    check_step(out, eng, want, onehot)


def test_engine_draws_a_temporal_box():
    """No override: the step cuts the box cutmix_box gives for (alpha, seed, mode, draw index 0)."""
    from vltf_amd.engine import LRCNEngine, cutmix_box
    p, _, onehot = data()
    seed = next(s for s in range(1000) if cutmix_box(1.0, s, "temporal", 0, FPC, H, W)[0][1] > cutmix_box(1.0, s, "temporal", 0, FPC, H, W)[0][0])
    box, _ = cutmix_box(1.0, seed, "temporal", 0, FPC, H, W)
    assert box[1] - box[0] == 1 and box[2:] == (0, H, 0, W)
    eng = LRCNEngine(small_cfg(cutmix_alpha=1.0, cutmix_seed=seed, cutmix_mode="temporal"), max_clips=B, device=DEV)
    eng.load_params(p)
    out = eng.train_step_u8(*dev_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN)
    assert eng.cut_box_last == box and eng.mix_lambda_last == CM.lam(box, FPC, H, W) == float(np.float32(2.0 / 3.0))
    check_step(out, eng, oracle_step(B, box), onehot[:B])


# ---- 6. off is the engine of before -----------------------------------------------------------------------------------------------------------
def test_cutmix_off_is_the_engine_of_before(monkeypatch):
    import vltf_amd.ops as ops_
    from vltf_amd._ffi import VltfError
    from vltf_amd.engine import LRCNEngine
    monkeypatch.setattr(ops_, "cutmix_pairs", lambda *a, **k: pytest.fail("cutmix_pairs was launched"))
    monkeypatch.setattr(ops_.Conv, "cutmix_pairs_s2d", lambda *a, **k: pytest.fail("cutmix_pairs_s2d was launched"))
    p, _, _ = data()
    for base in (dict(), dict(mixup_alpha=0.2, mixup_seed=7)):                             # a plain engine, and a mixup-only one
        res = []
        for kw in (dict(cutmix_alpha=0.0, cutmix_seed=0), dict(cutmix_alpha=None, cutmix_seed=None, cutmix_mode=None, cutmix_prob=None), dict()):
            eng = LRCNEngine(small_cfg(**dict(base, **kw)), max_clips=B, device=DEV)
            eng.load_params(p)
            assert eng.cut_box is None and eng.cutmix_alpha == 0.0
            if base:
                assert eng.blend_lam is eng.mix_lam and eng.mix_lam is not None
            else:
                assert eng.mix_lam is None and eng.blend_lam is None and eng.stats.numel() == 2 and eng.loss_rows.numel() == 2 * B
            outs = [eng.train_step_u8(*dev_batch(c0, c0 + B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN) for c0 in (0, 2)]
            res.append((outs, eng.logits_host().copy(), eng.get_params()))
            with pytest.raises(VltfError, match="cut_box is given, but CutMix is off"):
                eng.train_step_u8(*dev_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, cut_box=BOX)
            with pytest.raises(VltfError, match="cut_box is given, but CutMix is off"):
                eng.train_step_f32(torch.zeros((B * FPC,) + SHAPE, device=DEV), dev_batch(0, B)[1], lr=LR, cut_box=BOX)
            assert eng.step_count == 2
        for outs, logits, params in res[:2]:
            assert outs == res[2][0] and np.array_equal(logits.view(np.int32), res[2][1].view(np.int32))
            for k in params:
                assert np.array_equal(params[k].view(np.int32), res[2][2][k].view(np.int32)), k


# ---- 7. captured steps ------------------------------------------------------------------------------------------------------------------------
BOXES3 = (BOX, (1, 2, 0, 67, 0, 67), (0, 2, 33, 67, 0, 50))


def test_captured_step_equals_eager():
    """Step 1 is the warm-up, step 2 is captured and replayed, step 3 is a replay, each with a box of its own: the replays pick up the
    box and the weight the host wrote before them and are bit-equal to the eager engine."""
    from vltf_amd.engine import LRCNEngine
    p, _, onehot = data()
    eager = LRCNEngine(small_cfg(cutmix_alpha=1.0), max_clips=B, device=DEV)
    graph = LRCNEngine(small_cfg(cutmix_alpha=1.0, step_graph=True), max_clips=B, device=DEV)
    eager.load_params(p)
    graph.load_params(p)
    for step, (c0, box) in enumerate(zip((0, 2, 0), BOXES3)):
        outs = [e.train_step_u8(*dev_batch(c0, c0 + B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, cut_box=box) for e in (eager, graph)]
        assert step_keys_equal(*outs), (step, outs)
        assert same_bits(eager, graph), step
        assert np.array_equal(eager.logits_host().view(np.int32), graph.logits_host().view(np.int32))
        if step == 0:
            check_step(outs[1], graph, oracle_step(B, BOX), onehot[:B])
    assert len(graph._graphs) == 1                                                    # one graph: the box is no part of the key


def test_a_replay_reads_the_box_written_before_it():
    from vltf_amd.engine import LRCNEngine
    p, _, _ = data()
    box1, box2 = BOXES3[0], BOXES3[2]
    graph = LRCNEngine(small_cfg(cutmix_alpha=1.0, step_graph=True), max_clips=B, device=DEV)
    eager1, eager2 = (LRCNEngine(small_cfg(cutmix_alpha=1.0), max_clips=B, device=DEV) for _ in range(2))
    for e in (graph, eager1, eager2):
        e.load_params(p)
        for c0 in (0, 2):
            e.train_step_u8(*dev_batch(c0, c0 + B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, cut_box=box1)
    assert len(graph._graphs) == 1 and same_bits(graph, eager1) and same_bits(graph, eager2)
    og = graph.train_step_u8(*dev_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, cut_box=box2)
    o1 = eager1.train_step_u8(*dev_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, cut_box=box1)
    o2 = eager2.train_step_u8(*dev_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, cut_box=box2)
    assert len(graph._graphs) == 1
    assert step_keys_equal(og, o2) and same_bits(graph, eager2)
    assert og["loss_sum"] != o1["loss_sum"] and not same_bits(graph, eager1)


# ---- 8. the bf16 conv path cuts the packed input ------------------------------------------------------------------------------------------------
def test_bf16_conv_path_cuts_the_packed_input():
    from vltf_amd.engine import LRCNEngine
    p, frames_np, _ = data()
    eng = LRCNEngine(small_cfg(cutmix_alpha=1.0, conv_math="bf16"), max_clips=B, device=DEV)
    eng.load_params(p)
    frames, onehot = dev_batch(0, B)
    box = (0, 2, 9, 42, 21, 62)                                                           # no edge a multiple of conv1's stride
    n, b = eng.feed_u8(torch.from_numpy(CM.swap_frames(frames_np[:B * FPC], B, box)).to(DEV), MEAN)
    assert eng.c8 and eng._xb_fed and (n, b) == (B * FPC, B)
    want = eng.layers[0]["xb"][:n].clone()
    eng.feed_u8(frames, MEAN)
    plain = eng.layers[0]["xb"][:n].clone()
    eng._mix_write(None, None, box)
    eng._mix_launch(n, b)
    got = eng.layers[0]["xb"][:n]
    assert torch.equal(bits16(got), bits16(want)) and not torch.equal(bits16(got), bits16(plain))
    out = eng.train_step_u8(frames, onehot, lr=LR, clip_norm=CLIP, mean_bgr=MEAN, cut_box=box)
    assert torch.equal(bits16(eng.layers[0]["xb"][:n]), bits16(want))                    # the step's own launch: the same packed input
    assert np.isfinite(out["loss"]) and np.isfinite(out["grad_norm"]) and out["grad_norm"] > 0 and np.isfinite(eng.logits_host()).all()
    assert all(np.isfinite(v).all() for v in eng.get_params().values())


# ---- 9. mixup and CutMix together ---------------------------------------------------------------------------------------------------------------
def test_both_on_follow_the_switch():
    from vltf_amd.engine import LRCNEngine, cutmix_box, cutmix_lambda, mixup_lambda
    p, _, _ = data()
    mx, cm = dict(mixup_alpha=0.4, mixup_seed=11), dict(cutmix_alpha=1.0, cutmix_seed=5, cutmix_mode="cuboid")
    prob = 0.5
    both = LRCNEngine(small_cfg(cutmix_prob=prob, **mx, **cm), max_clips=B, device=DEV)
    assert both.blend_lam is not None and both.blend_lam is not both.mix_lam and both.cut_box is not None
    chosen = {}
    for i in range(12):
        both.step_count = i
        both._mix_write(None, None)
        box, u = cutmix_box(1.0, 5, "cuboid", i, FPC, H, W)
        if u < prob:
            want = (cutmix_lambda(box, FPC, H, W), box, 1.0)
            if box[1] > box[0] and box[3] > box[2] and box[5] > box[4]:
                chosen.setdefault("cut", i)
        else:
            lam = mixup_lambda(0.4, 11, i)
            want = (lam, (0, 0, 0, 0, 0, 0), lam)
            chosen.setdefault("mix", i)
        assert (both.mix_lambda_last, both.cut_box_last) == want[:2], i
        assert float(both.mix_lam) == np.float32(want[0]) and float(both.blend_lam) == np.float32(want[2])
        assert both.cut_box.cpu().tolist() == list(want[1])
    assert set(chosen) == {"cut", "mix"}
    for kind, only_kw in (("mix", mx), ("cut", cm)):
        engines = [LRCNEngine(small_cfg(cutmix_prob=prob, **mx, **cm), max_clips=B, device=DEV), LRCNEngine(small_cfg(**only_kw), max_clips=B, device=DEV)]
        outs = []
        for e in engines:
            e.load_params(p)
            e.step_count = chosen[kind]
            outs.append(e.train_step_u8(*dev_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN))
        assert engines[0].mix_lambda_last == engines[1].mix_lambda_last
        assert step_keys_equal(*outs) and same_bits(*engines), kind
        assert np.array_equal(engines[0].logits_host().view(np.int32), engines[1].logits_host().view(np.int32))
    # an override decides for its method
    both.load_params(p)
    both.step_count = chosen["mix"]
    both._mix_write(None, None, BOX)
    assert both.cut_box_last == BOX and float(both.blend_lam) == 1.0
    both.step_count = chosen["cut"]
    both._mix_write(0.7, None)
    assert both.cut_box_last == (0, 0, 0, 0, 0, 0) and both.mix_lambda_last == 0.7 and float(both.blend_lam) == np.float32(0.7)


# ---- 10. accumulation -----------------------------------------------------------------------------------------------------------------------------
def test_accumulated_update_draws_a_box_per_micro_step():
    """accumulate 2, three updates, captured: every micro-step draws cutmix_box(.., step_count * 2 + i).  Bit for bit the eager engine
    given those boxes through cut_box."""
    from vltf_amd.engine import LRCNEngine, cutmix_box
    p, _, _ = data()
    kw = dict(cutmix_alpha=1.0, cutmix_seed=3, cutmix_mode="spatial", accumulate=2)
    drawn = LRCNEngine(small_cfg(step_graph=True, **kw), max_clips=B, device=DEV)
    given = LRCNEngine(small_cfg(**kw), max_clips=B, device=DEV)
    drawn.load_params(p)
    given.load_params(p)
    seen = []
    for update in range(3):
        for i, c0 in enumerate((0, 2)):
            box, _ = cutmix_box(1.0, 3, "spatial", update * 2 + i, FPC, H, W)
            a = drawn.train_step_u8(*dev_batch(c0, c0 + B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, micro=(i, 2))
            b = given.train_step_u8(*dev_batch(c0, c0 + B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, micro=(i, 2), cut_box=box)
            assert drawn.cut_box_last == box == given.cut_box_last and drawn.mix_lambda_last == given.mix_lambda_last
            assert a["loss_sum"] == b["loss_sum"] and a["correct"] == b["correct"] and a["rows"] == b["rows"], (update, i)
            seen.append(box)
        assert a["grad_norm"] == b["grad_norm"] and same_bits(drawn, given), update
    assert len(set(seen)) == 6 and drawn.step_count == 3


# ---- 11. run_task on the example ----------------------------------------------------------------------------------------------------------------
def test_run_task_on_the_example(tmp_path, monkeypatch):
    """examples/lrcn_cutmix.yml shrunk: the synthetic dataset and the small network of tests/test_run_task_gpu.py, one epoch, with the
    example's own mixup and cutmix keys.  The info line is there, the losses are finite, and a second run logs the same losses."""
    from tests.test_host_workflow import make_dataset
    from tests.test_run_task_gpu import RAW, write_cfg
    from vltf_amd import run_task
    monkeypatch.setenv("VLTF_PREFETCH", "0")
    monkeypatch.setenv("VLTF_CONV_MATH", "f32")
    monkeypatch.delenv("VLTF_STEP_GRAPH", raising=False)
    with open(os.path.join(ROOT, "examples", "lrcn_cutmix.yml")) as f:
        example = yaml.safe_load(f)["run"]
    keys = ("mixup_alpha", "mixup_seed", "cutmix_alpha", "cutmix_seed", "cutmix_mode", "cutmix_prob")
    assert [example["train"][k] for k in keys] == [0.2, 7, 1.0, 7, "cuboid", 0.5]
    folder = str(tmp_path)
    train_path, _, _ = make_dataset(folder, "train.txt", nvid=4, cpv=(1, 2, 1, 1), shape=RAW, seed=1)
    losses = []
    for run in ("run_a", "run_b"):
        out = write_cfg(folder, run + ".yml", train_path, "train", epochs=1, det=True, run=run)
        with open(out) as f:
            c = yaml.safe_load(f)
        c["run"]["train"].update({k: example["train"][k] for k in keys})
        with open(out, "w") as f:
            yaml.safe_dump(c, f)
        run_task.main(out, seed=3)
        log = open(glob.glob(os.path.join(folder, run, "log_e2e_train_scratch_*.log"))[0]).read()
        assert "CutMix: alpha 1.0, seed 7, mode cuboid" in log and "exchange the box" in log and "cut with probability 0.5" in log
        assert "Mixup: alpha 0.2, seed 7" in log
        found = [float(v) for v in re.findall(r"batch loss/nats : ([-+0-9.eE]+|nan|inf) /", log)]
        assert len(found) >= 2 and np.isfinite(found).all(), found
        losses.append(found)
    assert losses[0] == losses[1]
