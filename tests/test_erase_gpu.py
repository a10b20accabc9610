"""Random erasing on the device (vl_erase_boxes, vl_erase_boxes_s2d, NetConfig.erase_prob): the in-place, write-only box fill in both
layouts conv1 reads against a host map written from the layout formulas and the numpy restatement of the noise (tests/erase_ref.py),
bit for bit over the whole allocation, guard words on both sides included; special bit patterns outside the boxes; device rows that
are clamped; the chain contract between the two layouts; refusals that launch nothing; whole steps of LRCNEngine (box override against
the fp64 oracle, captured and replayed with another table, the bf16 conv path, the order with mixup and CutMix, accumulation, off) and
run_task on the example.

Tolerances.  The fill is an integer times one fp32 factor, restated on the host with the same two operations, and the packed form
rounds it to nearest even as the host does: every comparison of buffers is of bits.  The whole step against the fp64 oracle holds the
bounds of tests/test_cutmix_gpu.py::test_engine_step_with_a_box_override, which are tests/test_mixup_gpu.py::check_step's (loss
1e-4 * max(1, |loss|), gradient norm 1e-3 relative, parameters rtol 1e-4 and atol 1e-5, logits rtol 1e-3 and atol 1e-3).  The blend
that follows an erase is compared with tests/test_mixup_gpu.py's bound of the blend launch, 8 eps32 times the pair's magnitude."""
import glob
import os
import re

import numpy as np
import pytest
import torch
import yaml

from oracle import lrcn_oracle as O
from tests import cutmix_ref as CM
from tests import erase_ref as ER
from tests import mixup_ref as MX
from tests.test_cutmix_gpu import BOX, DESCS, FFPC, FH, FW, bits16, feed_x0, feed_xb, frames_u8, s2d_desc, special_words
from tests.test_label_smoothing_gpu import B, CLIP, FPC, LR, MEAN, SHAPE, bits, data, dev_batch, small_cfg
from tests.test_mixup_gpu import EPS32, check_step, pair_scale, same_bits, step_keys_equal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = SHAPE[:2]
GUARD = 64                                       # words in front of and behind every buffer a launch is given
STD = 57.63
SCALE = ER.scale_of(STD)
MODES = (0, 1, 2)
GEOMS = [(0, 1), (2, 1), (2, 4), (1, 3)]         # (halo, phase) of x0


@pytest.fixture(scope="module")
def ops():
    import vltf_amd.ops as ops_
    return ops_


def box_set(fpc, h, w):
    """The boxes every kernel test cycles through, a different one per clip: empty, the full clip, a 1 x 1 x 1 box at each of the
    eight corners, one frame only, x edges in every phase (x0 = 0 .. 3, with x1 in every phase too), and boxes whose edges cut a
    space-to-depth chunk on both axes (odd bounds: no multiple of a stride 2 or 4)."""
    corners = [(t, t + 1, y, y + 1, x, x + 1) for t in (0, fpc - 1) for y in (0, h - 1) for x in (0, w - 1)]
    phases = [(0, fpc, 2, h - 2, x0, x0 + 4 + x0) for x0 in range(4)]
    return [(0, 0, 0, 0, 0, 0), (0, fpc, 0, h, 0, w)] + corners + [(1, 2, 0, h, 0, w)] + phases + [(0, fpc, 1, 6, 3, w - 1), (1, fpc, 3, h - 2, 1, w - 3)]


def tables(clips, boxes, seed):
    """int32 [rounds][clips][8]: the boxes dealt out in order, a different one per clip, until each was used; random 64-bit keys (both
    signs in both words)."""
    rng = np.random.default_rng(seed)
    rounds = -(-len(boxes) // clips)
    out = np.zeros((rounds, clips, 8), np.int32)
    for r in range(rounds):
        for i in range(clips):
            out[r, i, :6] = boxes[(r * clips + i) % len(boxes)]
    out[:, :, 6:] = rng.integers(-2 ** 31, 2 ** 31, (rounds, clips, 2))
    assert (out[:, :, 6:] < 0).any() and (out[:, :, 6:] > 0).any()
    return out


def dtab(table):
    return torch.from_numpy(np.ascontiguousarray(table, np.int32)).to(DEV)


def guarded(words, dtype, shape):
    """(the whole allocation as integers, the tensor a launch is given): `words` with GUARD patterned words on both sides."""
    kind = np.uint32 if dtype == torch.float32 else np.uint16
    guard = (np.arange(GUARD, dtype=np.uint64) * 2654435761 % (1 << (8 * kind().itemsize))).astype(kind)
    host = np.concatenate([guard, np.asarray(words, kind).reshape(-1), guard[::-1]])
    itype = torch.int32 if dtype == torch.float32 else torch.int16
    whole = torch.from_numpy(host.view(np.int32 if kind is np.uint32 else np.int16).copy()).to(DEV)
    assert whole.dtype == itype
    return host, whole, whole[GUARD:GUARD + host.size - 2 * GUARD].view(dtype).view(shape)


def want_words(host, idx, table, fpc, h, w, c, mode, packed):
    """The allocation after the launch: the words of the erased positions (through the layout map idx, [clips, fpc, h, w, c]) replaced
    by the reference fill of their clip, everything else as it was."""
    want = host.copy()
    clips = len(table)
    m = ER.mask(clips, fpc, h, w, table)
    for i in range(clips):
        if not m[i].any():
            continue
        v = ER.fill((fpc, h, w, c), ER.key_of(table[i]), mode, SCALE)
        words = ER.bf16_bits(v) if packed else v.view(np.uint32)
        want[GUARD + idx[i][m[i]]] = words[m[i]]
    return want


def back(whole):
    a = whole.cpu().numpy()
    return a.view(np.uint32 if a.dtype == np.int32 else np.uint16)


# ---- 1. the fp32 launch, bit for bit, on fed frames -------------------------------------------------------------------------------------
@pytest.mark.parametrize("halo,phase", GEOMS)
@pytest.mark.parametrize("clips", [1, 2, 3, 4])
def test_erase_boxes_f32(ops, clips, halo, phase):
    f = frames_u8(clips, FFPC, FH, FW)
    fed = feed_x0(ops, f, FH, FW, halo, phase)
    shape = tuple(fed.shape)
    idx = ER.x0_index(clips, FFPC, FH, FW, halo, phase).reshape(clips, FFPC, FH, FW, 3)
    assert len(np.unique(idx)) == idx.size and idx.max() < fed.numel()
    words = fed.view(torch.int32).cpu().numpy().reshape(-1).view(np.uint32)
    for mode in MODES:
        for table in tables(clips, box_set(FFPC, FH, FW), 11 * clips + mode):
            host, whole, x0 = guarded(words, torch.float32, shape)
            ops.erase_boxes(x0, clips, FFPC, (FH, FW), halo, phase, dtab(table), mode, float(SCALE))
            want = want_words(host, idx, table, FFPC, FH, FW, 3, mode, False)
            assert np.array_equal(back(whole), want), (mode, table[:, :6].tolist())      # the WHOLE allocation: halo, padding, guards
            if ER.mask(clips, FFPC, FH, FW, table).any():
                assert not np.array_equal(want, host)
    if clips == 4 and phase == 4:                # mode 0 is +0.0, and mode 1 is one value per (clip, channel), different between clips
        table = np.array([[0, FFPC, 0, FH, 0, FW, 5 + i, -i] for i in range(clips)], np.int32)
        for mode in (0, 1):
            host, whole, x0 = guarded(words, torch.float32, shape)
            ops.erase_boxes(x0, clips, FFPC, (FH, FW), halo, phase, dtab(table), mode, float(SCALE))
            got = back(whole)[GUARD + idx]
            if mode == 0:
                assert not got.any()
            else:
                per = got.reshape(clips, -1, 3)
                assert (per == per[:, :1]).all() and len(np.unique(per[:, 0])) == 3 * clips


# ---- 2. the packed launch, bit for bit, on fed frames -----------------------------------------------------------------------------------
def packed_index(conv, name, clips):
    cin, h, w, k, s = DESCS[name]
    return ER.s2d_index(clips, FFPC, cin, h, w, k, s, conv.oh, conv.ow).reshape(clips, FFPC, h, w, cin)


@pytest.mark.parametrize("name", list(DESCS))
@pytest.mark.parametrize("clips", [1, 2, 3, 4])
def test_erase_boxes_s2d(ops, name, clips):
    conv, geom = s2d_desc(ops, name)
    cin, h, w, k, s = DESCS[name]
    fed = feed_xb(ops, conv, geom, frames_u8(clips, FFPC, h, w, cin))
    shape = tuple(fed.shape)
    idx = packed_index(conv, name, clips)
    assert len(np.unique(idx)) == idx.size and idx.max() < fed.numel()
    words = fed.view(torch.int16).cpu().numpy().reshape(-1).view(np.uint16)
    boxes = box_set(FFPC, h, w)
    assert any(b[2] % s and b[3] % s and b[4] % s and b[5] % s for b in boxes)           # edges that cut through a chunk on both axes
    for mode in MODES:
        for table in tables(clips, boxes, 13 * clips + mode):
            host, whole, xb = guarded(words, torch.bfloat16, shape)
            conv.erase_boxes_s2d(xb, clips, FFPC, dtab(table), mode, float(SCALE))
            want = want_words(host, idx, table, FFPC, h, w, cin, mode, True)
            assert np.array_equal(back(whole), want), (mode, table[:, :6].tolist())
            if ER.mask(clips, FFPC, h, w, table).any():
                assert not np.array_equal(want, host)


# ---- 3. special bit patterns and untouched bytes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("halo,phase", GEOMS)
def test_f32_untouched_bytes_among_special_patterns(ops, halo, phase):
    """Random 32-bit patterns (-0, infinities, NaN payloads) in EVERY word of the buffer; every word outside the boxes compares equal as
    an integer, the guards included, and a clip with an empty box is untouched whatever its key."""
    clips = 3
    shape = ops.phase_split_shape(clips * FFPC, 3, FH, FW, halo, phase)
    u = special_words(int(np.prod(shape)), 7 + phase)
    idx = ER.x0_index(clips, FFPC, FH, FW, halo, phase).reshape(clips, FFPC, FH, FW, 3)
    for mode in MODES:
        table = np.array([[0, 3, 1, 6, 3, 10, 77, -5], [0, 0, 0, 0, 0, 0, -123456789, 987654321], [1, 2, 0, FH, 0, FW, 1, 1 << 30]], np.int32)
        host, whole, x0 = guarded(u, torch.float32, shape)
        ops.erase_boxes(x0, clips, FFPC, (FH, FW), halo, phase, dtab(table), mode, float(SCALE))
        got = back(whole)
        assert np.array_equal(got, want_words(host, idx, table, FFPC, FH, FW, 3, mode, False)), mode
        m = ER.mask(clips, FFPC, FH, FW, table)
        outside = np.ones(host.size, bool)
        outside[GUARD + idx[m]] = False
        assert np.array_equal(got[outside], host[outside]) and not np.array_equal(got[~outside], host[~outside])
        assert np.array_equal(got[GUARD + idx[1]], host[GUARD + idx[1]])                  # the clip with the empty box


@pytest.mark.parametrize("name", list(DESCS))
def test_s2d_untouched_bytes_among_special_patterns(ops, name):
    """Random 16-bit patterns in every slot of the packed buffer, the slots no pixel maps to (padding, the unused channels of a last
    chunk) included."""
    conv, geom = s2d_desc(ops, name)
    cin, h, w, k, s = DESCS[name]
    clips = 3
    shape = ops.c8_shape(clips * FFPC, *geom)
    rng = np.random.default_rng(29)
    u = rng.integers(0, 2 ** 16, int(np.prod(shape)), dtype=np.uint64).astype(np.uint16)
    u[rng.integers(0, u.size, u.size // 4)] = np.array([0x8000, 0x7f80, 0xff80, 0x7fc1, 0x7f81], np.uint16)[rng.integers(0, 5, u.size // 4)]
    idx = packed_index(conv, name, clips)
    assert idx.size < u.size                                                              # there ARE slots no pixel maps to
    for mode in MODES:
        table = np.array([[0, 3, 1, 6, 3, w - 1, 77, -5], [0, 0, 0, 0, 0, 0, -123456789, 987654321], [1, 2, 0, h, 0, w, 1, 1 << 30]], np.int32)
        host, whole, xb = guarded(u, torch.bfloat16, shape)
        conv.erase_boxes_s2d(xb, clips, FFPC, dtab(table), mode, float(SCALE))
        got = back(whole)
        assert np.array_equal(got, want_words(host, idx, table, FFPC, h, w, cin, mode, True)), mode
        m = ER.mask(clips, FFPC, h, w, table)
        outside = np.ones(host.size, bool)
        outside[GUARD + idx[m]] = False
        assert np.array_equal(got[outside], host[outside]) and not np.array_equal(got[~outside], host[~outside])


# ---- 4. device rows are clamped ------------------------------------------------------------------------------------------------------------
WORDS = [(-5, 99, -1, 6, 3, 400), (2, 1, 0, 9, 0, 11), (0, 3, 7, 2, 0, 11), (0, 3, 0, 9, 11, 11),
         (-2 ** 31, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1), (2 ** 31 - 1, -2 ** 31, 0, 9, 0, 11),
         (5, 9, 0, 9, 0, 11), (0, 3, 2 ** 30, 2 ** 31 - 1, 0, 11), (0, 3, -2 ** 31, -2 ** 30, 0, 11)]   # those of the CutMix clamp test


@pytest.mark.parametrize("mode", MODES)
def test_device_rows_are_clamped_to_the_frame(ops, mode):
    """Defined behaviour: whatever a row holds, the launch fills the clamped box, ignores a reversed or empty range, and writes nothing
    outside the buffer (the guards on both sides are compared too)."""
    clips = 3
    assert sum(1 for wd in WORDS if ER.clamp(wd, FFPC, FH, FW) != (0,) * 6) >= 2 and len(WORDS) % clips == 0
    fed = feed_x0(ops, frames_u8(clips, FFPC, FH, FW), FH, FW, 2, 4)
    idx = ER.x0_index(clips, FFPC, FH, FW, 2, 4).reshape(clips, FFPC, FH, FW, 3)
    words = fed.view(torch.int32).cpu().numpy().reshape(-1).view(np.uint32)
    conv, geom = s2d_desc(ops, "generic")
    cin, h, w, k, s = DESCS["generic"]
    fedb = feed_xb(ops, conv, geom, frames_u8(clips, FFPC, h, w, cin))
    idxb = packed_index(conv, "generic", clips)
    wordsb = fedb.view(torch.int16).cpu().numpy().reshape(-1).view(np.uint16)
    for table in tables(clips, WORDS, 3 + mode):
        host, whole, x0 = guarded(words, torch.float32, tuple(fed.shape))
        ops.erase_boxes(x0, clips, FFPC, (FH, FW), 2, 4, dtab(table), mode, float(SCALE))
        assert np.array_equal(back(whole), want_words(host, idx, table, FFPC, FH, FW, 3, mode, False)), table[:, :6].tolist()
        host, whole, xb = guarded(wordsb, torch.bfloat16, tuple(fedb.shape))
        conv.erase_boxes_s2d(xb, clips, FFPC, dtab(table), mode, float(SCALE))
        assert np.array_equal(back(whole), want_words(host, idxb, table, FFPC, h, w, cin, mode, True)), table[:, :6].tolist()


# ---- 5. the chain contract -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(DESCS))
def test_erase_then_pack_equals_packed_feed_then_erase(ops, name, mode):
    """vl_erase_boxes followed by vl_s2d_c8_from_x0 == vl_input_prep_u8_s2d followed by vl_erase_boxes_s2d, bit for bit.  The fp32 feed
    and vl_erase_boxes work on three channels: a two-channel descriptor rides in the first two planes (as in
    tests/test_scale_jitter_gpu.py), which holds for modes 0 and 1; the element index of mode 2 contains the channel count, 3 in x0
    and 2 in that descriptor's packed input, so that one combination has no contract to check and checks the packed side alone."""
    conv, geom = s2d_desc(ops, name)
    cin, h, w, k, s = DESCS[name]
    clips = 3
    f = frames_u8(clips, FFPC, h, w, cin)
    f3 = f if cin == 3 else np.ascontiguousarray(np.concatenate([f, frames_u8(clips, FFPC, h, w, 3)[..., :3 - cin]], axis=3))
    table = dtab(np.array([[0, 3, 1, 6, 3, w - 1, 77, -5], [1, 3, 3, h - 1, 1, 6, -9, 4], [0, 1, 0, h, 0, w, 1, 1 << 30]], np.int32))
    mean3 = torch.tensor([99.2, 105.3, 109.5], device=DEV)                                # feed_xb's mean
    packed = feed_xb(ops, conv, geom, f)
    plain = packed.clone()
    conv.erase_boxes_s2d(packed, clips, FFPC, table, mode, float(SCALE))
    assert not torch.equal(bits16(packed), bits16(plain))
    if cin != 3 and mode == 2:
        idx = packed_index(conv, name, clips)
        host = np.concatenate([np.zeros(GUARD, np.uint16), plain.view(torch.int16).cpu().numpy().reshape(-1).view(np.uint16), np.zeros(GUARD, np.uint16)])
        want = want_words(host, idx, table.cpu().numpy(), FFPC, h, w, cin, mode, True)[GUARD:-GUARD]
        assert np.array_equal(packed.view(torch.int16).cpu().numpy().reshape(-1).view(np.uint16), want)
        return
    phase = max(conv.x_phase, 1)
    x3 = torch.zeros(ops.phase_split_shape(clips * FFPC, 3, h, w, conv.x_halo, phase), device=DEV)
    ops.input_prep_u8(torch.from_numpy(f3).to(DEV), x3, None, None, None, mean3, halo=conv.x_halo, phase=phase, out_hw=(h, w))
    ops.erase_boxes(x3, clips, FFPC, (h, w), conv.x_halo, phase, table, mode, float(SCALE))
    x0 = x3[:, :cin * phase].contiguous()
    assert tuple(x0.shape) == tuple(conv.x_shape(clips * FFPC))
    chained = torch.full_like(packed, 7.0)
    conv.s2d_c8_from_x0(x0, chained)
    assert torch.equal(bits16(chained), bits16(packed))


# ---- 6. refusals launch nothing ------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ops):
    from vltf_amd import _ffi
    from vltf_amd._ffi import VltfError
    clips, halo, phase = 2, 2, 4
    x0 = torch.full(ops.phase_split_shape(clips * FFPC, 3, FH, FW, halo, phase), 12345.0, device=DEV)
    table = dtab(np.array([[0, 3, 1, 6, 3, 10, 7, 0]] * clips, np.int32))
    st = torch.cuda.current_stream().cuda_stream
    ok = dict(x=x0.data_ptr(), clips=clips, fpc=FFPC, h=FH, w=FW, halo=halo, phase=phase, table=table.data_ptr(), mode=2, scale=float(SCALE))
    for change, msg in ((dict(x=None), "x0 is null"), (dict(table=None), "table_dev is null"), (dict(clips=-1), "clips must be >= 0"),
                        (dict(fpc=0), "fpc must lie in"), (dict(fpc=65536), "fpc must lie in"), (dict(h=0), "bad frame size"),
                        (dict(halo=-1), "halo must be >= 0"), (dict(phase=0), "phase must be >= 1"), (dict(mode=3), "mode must be 0"),
                        (dict(mode=-1), "mode must be 0"), (dict(scale=float("nan")), "scale must be finite"),
                        (dict(scale=float("inf")), "scale must be finite")):
        a = dict(ok, **change)
        with pytest.raises(VltfError, match=msg):
            _ffi.call("vl_erase_boxes", a["x"], a["clips"], a["fpc"], a["h"], a["w"], a["halo"], a["phase"], a["table"], a["mode"], a["scale"], st)
        assert msg.encode() in _ffi.lib().vl_last_error()
    with pytest.raises(VltfError, match="is not 2 clips of 3 frames"):
        ops.erase_boxes(x0[:3], clips, FFPC, (FH, FW), halo, phase, table, 0, 1.0)
    with pytest.raises(VltfError, match="float32"):
        ops.erase_boxes(x0.double(), clips, FFPC, (FH, FW), halo, phase, table, 0, 1.0)
    for bad in (table[:1], table.float(), table.cpu(), torch.zeros((clips, 6), dtype=torch.int32, device=DEV), table.t().contiguous().t(), None):
        with pytest.raises(VltfError, match=r"contiguous device int32 \[2\]\[8\] tensor"):
            ops.erase_boxes(x0, clips, FFPC, (FH, FW), halo, phase, bad, 0, 1.0)
    conv, geom = s2d_desc(ops, "generic")
    xb = torch.full(ops.c8_shape(clips * FFPC, *geom), 3.0, dtype=torch.bfloat16, device=DEV)
    for args, msg in (((conv._d, None, clips, FFPC, table.data_ptr(), 0, 1.0), "xb is null"),
                      ((conv._d, xb.data_ptr(), clips, FFPC, None, 0, 1.0), "table_dev is null"),
                      ((conv._d, xb.data_ptr(), -2, FFPC, table.data_ptr(), 0, 1.0), "clips must be >= 0"),
                      ((conv._d, xb.data_ptr(), clips, 0, table.data_ptr(), 0, 1.0), "fpc must lie in"),
                      ((None, xb.data_ptr(), clips, FFPC, table.data_ptr(), 0, 1.0), "a strided, ungrouped, square layer"),
                      ((conv._d, xb.data_ptr(), clips, FFPC, table.data_ptr(), 5, 1.0), "mode must be 0"),
                      ((conv._d, xb.data_ptr(), clips, FFPC, table.data_ptr(), 1, float("nan")), "scale must be finite")):
        with pytest.raises(VltfError, match=msg):
            _ffi.call("vl_erase_boxes_s2d", *args, st)
        assert msg.encode() in _ffi.lib().vl_last_error()
    plain = ops.Conv(3, 9, 9, 8, 3, 3, 1, 1)                                              # unit stride: no space-to-depth input
    with pytest.raises(VltfError, match="a strided, ungrouped, square layer"):
        _ffi.call("vl_erase_boxes_s2d", plain._d, xb.data_ptr(), clips, FFPC, table.data_ptr(), 0, 1.0, st)
    with pytest.raises(VltfError, match="packed input of 2 clips of 3 frames"):
        conv.erase_boxes_s2d(xb[:4], clips, FFPC, table, 0, 1.0)
    with pytest.raises(VltfError, match=r"contiguous device int32 \[2\]\[8\] tensor"):
        conv.erase_boxes_s2d(xb, clips, FFPC, table[:1], 0, 1.0)
    # no clips: accepted, nothing launched
    _ffi.call("vl_erase_boxes", x0.data_ptr(), 0, FFPC, FH, FW, halo, phase, table.data_ptr(), 2, 1.0, st)
    _ffi.call("vl_erase_boxes_s2d", conv._d, xb.data_ptr(), 0, FFPC, table.data_ptr(), 2, 1.0, st)
    torch.cuda.synchronize()
    assert bool((x0 == 12345.0).all()) and bool((xb == 3.0).all())


# ---- 7. engine steps (the geometry of tests/test_cutmix_gpu.py) -----------------------------------------------------------------------------
EBOXES = [(0, 3, 10, 40, 20, 63), (1, 2, 5, 60, 0, 31)]                                    # one per clip of a batch of B = 2
EBOXES2 = [(0, 2, 33, 67, 0, 50), (0, 0, 0, 0, 0, 0)]
_ORACLE = {}


def host_inputs(c0, clips):
    _, frames, _ = data()
    return (frames[c0 * FPC:(c0 + clips) * FPC].astype(np.float32) - MEAN).reshape((clips, FPC) + SHAPE)


def rows_of(boxes, keys=None):
    return np.array([tuple(b) + (tuple(keys[i]) if keys is not None else (0, 0)) for i, b in enumerate(boxes)], np.int32)


def oracle_step(boxes):
    """O.lrcn_train_step fed the first B clips erased on the host in zero mode; once per set of boxes."""
    p, _, onehot = data()
    key = tuple(boxes)
    if key not in _ORACLE:
        x = ER.erase(host_inputs(0, B), rows_of(boxes), 0, SCALE)
        _ORACLE[key] = O.lrcn_train_step(p, x.reshape((B * FPC,) + SHAPE), onehot[:B].astype(np.float64), FPC, lr=LR, clip_norm=CLIP)
    return _ORACLE[key]


def logical_x0(eng, n):
    """x0 of the engine's first n frames in logical order [n, h, w, 3], as bits."""
    idx = ER.x0_index(n // FPC, FPC, H, W, eng.x0_halo, eng.x0_phase)
    return eng.x0[:n].view(torch.int32).cpu().numpy().reshape(-1)[idx].view(np.uint32)


def fed_inputs(eng, frames):
    """The engine's own feed of these frames in logical order, fp32 [clips, fpc, h, w, 3] (what the erase launch finds)."""
    n = frames.shape[0]
    eng.feed_u8(frames, MEAN)
    return logical_x0(eng, n).view(np.float32).reshape((n // FPC, FPC) + SHAPE).copy()


def test_engine_step_with_a_box_override():
    from vltf_amd._ffi import VltfError
    from vltf_amd.engine import LRCNEngine, erase_row, erase_config
    p, _, onehot = data()
    assert len(EBOXES) == B
    cfg = small_cfg(erase_prob=0.5, erase_seed=7)
    eng = LRCNEngine(cfg, max_clips=B, device=DEV)
    eng.load_params(p)
    assert eng.erase_table is not None and eng.erase_table.dtype == torch.int32 and tuple(eng.erase_table.shape) == (B, 8)
    assert eng.erase.mode == "zero" and eng.mix_lam is None and eng.stats.numel() == 2
    for bad, msg in (([(0, 4, 0, 1, 0, 1), (0,) * 6], "leaves the frame"), ([(0, 3, 5, 4, 0, 1), (0,) * 6], "is reversed"),
                     ([(0, 3, 0, 1, 0)] * 2, "six whole numbers"), ([(0,) * 6], "must be 2 boxes")):
        with pytest.raises(VltfError, match=msg):
            eng.train_step_u8(*dev_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, erase_boxes=bad)
    assert eng.step_count == 0
    plain = fed_inputs(eng, dev_batch(0, B)[0])
    out = eng.train_step_u8(*dev_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, erase_boxes=EBOXES)
    keys = [erase_row(erase_config(cfg), 0, i, FPC, H, W)[6:] for i in range(B)]          # the keys are still the drawn ones
    assert np.array_equal(eng.erase_table_last, rows_of(EBOXES, keys)) and np.array_equal(eng.erase_table.cpu().numpy(), eng.erase_table_last)
    assert np.array_equal(logical_x0(eng, B * FPC), ER.erase(plain, rows_of(EBOXES), 0, SCALE).reshape((-1,) + SHAPE).view(np.uint32))
    check_step(out, eng, oracle_step(EBOXES), onehot[:B])
    unerased = oracle_step([(0,) * 6] * B)
    assert abs(out["loss"] - unerased[1]) > 1e-4 * abs(unerased[1])                       # and it is not the unerased step
    # more than half the clip is fine (the labels do not change), and the full clip leaves nothing
    eng.train_step_u8(*dev_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, erase_boxes=[(0, FPC, 0, H, 0, W)] * B)
    assert not logical_x0(eng, B * FPC).any()
    # the same step from fp32 frames: erased in x0
    again = LRCNEngine(cfg, max_clips=B, device=DEV)
    again.load_params(p)
    frames, labels = dev_batch(0, B)
    out2 = again.train_step_f32(frames.float() - torch.from_numpy(MEAN).to(DEV), labels, lr=LR, clip_norm=CLIP, erase_boxes=EBOXES)
    check_step(out2, again, oracle_step(EBOXES), onehot[:B])
    # a forward-only engine ignores the option, and forward never erases
    infer = LRCNEngine(cfg, max_clips=B, device=DEV, training=False)
    assert infer.erase is None and infer.erase_table is None
    eng.forward_u8(dev_batch(0, B)[0], MEAN)
    assert np.array_equal(logical_x0(eng, B * FPC), plain.view(np.uint32).reshape((-1,) + SHAPE))


def test_engine_draws_its_table():
    """No override: the step erases the rows erase_row gives for (config, draw index 0, clip i), in pixel mode, bit for bit."""
    from vltf_amd.engine import LRCNEngine, erase_table
    p, _, _ = data()
    cfg = small_cfg(erase_prob=1.0, erase_mode="pixel", erase_seed=3, erase_frames=(0.4, 1.0))
    eng = LRCNEngine(cfg, max_clips=B, device=DEV)
    eng.load_params(p)
    plain = fed_inputs(eng, dev_batch(0, B)[0])
    for step in range(2):
        out = eng.train_step_u8(*dev_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN)
        table = erase_table(cfg, step, 0, B, FPC, H, W)
        assert np.array_equal(eng.erase_table_last, table) and ER.mask(B, FPC, H, W, table).any(axis=(1, 2, 3)).all()
        assert [tuple(r) for r in table] == [ER.erase_row(1.0, (0.02, 0.33), (0.3, 3.3), (0.4, 1.0), 3, step, i, FPC, H, W) for i in range(B)]
        want = ER.erase(plain, table, 2, ER.scale_of(57.63))
        assert np.array_equal(logical_x0(eng, B * FPC), want.reshape((-1,) + SHAPE).view(np.uint32)), step
        assert np.isfinite(out["loss"]) and out["grad_norm"] > 0


# ---- 8. captured steps ---------------------------------------------------------------------------------------------------------------------
def test_captured_step_equals_eager_and_a_replay_reads_the_table_written_before_it():
    """Step 1 is the warm-up, step 2 is captured and replayed, step 3 is a replay with ANOTHER table: each is bit-equal to the eager
    engine given the same table, in the sums, the parameters and the contents of x0; the two replays leave different x0 contents."""
    from vltf_amd.engine import LRCNEngine
    p, _, _ = data()
    kw = dict(erase_prob=0.5, erase_mode="pixel")
    eager = LRCNEngine(small_cfg(**kw), max_clips=B, device=DEV)
    graph = LRCNEngine(small_cfg(step_graph=True, **kw), max_clips=B, device=DEV)
    eager.load_params(p)
    graph.load_params(p)
    table = graph.erase_table
    seen = []
    for step, boxes in enumerate((EBOXES, EBOXES, EBOXES2)):
        outs = [e.train_step_u8(*dev_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, erase_boxes=boxes) for e in (eager, graph)]
        assert step_keys_equal(*outs), (step, outs)
        assert same_bits(eager, graph), step
        assert np.array_equal(eager.logits_host().view(np.int32), graph.logits_host().view(np.int32))
        assert np.array_equal(eager.erase_table_last, graph.erase_table_last)
        x0 = logical_x0(graph, B * FPC)
        assert np.array_equal(x0, logical_x0(eager, B * FPC)), step
        seen.append(x0)
    assert len(graph._graphs) == 1 and graph.erase_table is table                         # one graph, one table: allocated at setup
    assert not np.array_equal(seen[1], seen[2])
    m1, m2 = (ER.mask(B, FPC, H, W, rows_of(b)).reshape((-1,) + SHAPE[:2]) for b in (EBOXES, EBOXES2))
    only2 = m2 & ~m1
    assert only2.any() and not np.array_equal(seen[1][only2], seen[2][only2])


# ---- 9. the bf16 conv path erases the packed input ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["zero", "pixel"])
def test_bf16_conv_path_erases_the_packed_input(mode):
    from vltf_amd.engine import LRCNEngine
    p, _, _ = data()
    eng = LRCNEngine(small_cfg(erase_prob=0.5, erase_mode=mode, conv_math="bf16"), max_clips=B, device=DEV)
    eng.load_params(p)
    frames, onehot = dev_batch(0, B)
    boxes = [(0, 2, 9, 42, 21, 62), (1, 3, 3, 66, 1, 30)]                                  # no edge a multiple of conv1's stride
    n, b = eng.feed_u8(frames, MEAN)
    assert eng.c8 and eng._xb_fed and (n, b) == (B * FPC, B)
    plain = eng.layers[0]["xb"][:n].view(torch.int16).cpu().numpy().reshape(-1).view(np.uint16).copy()
    out = eng.train_step_u8(frames, onehot, lr=LR, clip_norm=CLIP, mean_bgr=MEAN, erase_boxes=boxes)
    conv = eng.layers[0]["conv"]
    idx = ER.s2d_index(B, FPC, 3, H, W, conv.kh, conv.stride, conv.oh, conv.ow).reshape((B, FPC) + SHAPE)
    host = np.concatenate([np.zeros(GUARD, np.uint16), plain, np.zeros(GUARD, np.uint16)])
    want = want_words(host, idx, eng.erase_table_last, FPC, H, W, 3, ("zero", "clip", "pixel").index(mode), True)[GUARD:-GUARD]
    got = eng.layers[0]["xb"][:n].view(torch.int16).cpu().numpy().reshape(-1).view(np.uint16)
    assert np.array_equal(got, want) and not np.array_equal(got, plain)
    assert np.isfinite(out["loss"]) and np.isfinite(out["grad_norm"]) and out["grad_norm"] > 0 and np.isfinite(eng.logits_host()).all()
    # frames fed as fp32 on the bf16 path are erased in x0, ahead of the pack
    x = frames.float() - torch.from_numpy(MEAN).to(DEV)
    eng.train_step_f32(x, onehot, lr=LR, clip_norm=CLIP, erase_boxes=boxes)
    assert not eng._xb_fed
    table = eng.erase_table_last
    erased = ER.erase(host_inputs(0, B), table, ("zero", "clip", "pixel").index(mode), SCALE)
    assert np.array_equal(logical_x0(eng, n), erased.reshape((-1,) + SHAPE).view(np.uint32))


# ---- 10. the order with mixup and CutMix ----------------------------------------------------------------------------------------------------
def test_erase_comes_before_the_blend_and_the_cut():
    """Both on: a batch that is cut holds CutMix's swap of the ERASED frames (bit for bit), a batch that is blended mixup's blend of them
    (to the blend launch's bound) -- and neither is what the other order would have left."""
    from vltf_amd.engine import LRCNEngine
    p, _, _ = data()
    eng = LRCNEngine(small_cfg(erase_prob=0.5, erase_mode="pixel", mixup_alpha=0.4, cutmix_alpha=1.0), max_clips=B, device=DEV)
    eng.load_params(p)
    plain = fed_inputs(eng, dev_batch(0, B)[0])
    eng.train_step_u8(*dev_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, erase_boxes=EBOXES, cut_box=BOX)
    erased = ER.erase(plain, eng.erase_table_last, 2, SCALE)
    got = logical_x0(eng, B * FPC).reshape((B, FPC) + SHAPE)
    assert np.array_equal(got, CM.swap(erased, BOX).view(np.uint32))
    other = ER.erase(CM.swap(plain, BOX), eng.erase_table_last, 2, SCALE)
    assert not np.array_equal(got, other.view(np.uint32))
    lam = 0.7
    eng.train_step_u8(*dev_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, erase_boxes=EBOXES, mix_lambda=lam)
    erased = ER.erase(plain, eng.erase_table_last, 2, SCALE)
    got = logical_x0(eng, B * FPC).view(np.float32).reshape((B, -1)).astype(np.float64)
    want = MX.blend(erased.reshape(B, -1), lam)
    bound = 8 * EPS32 * pair_scale(erased.reshape(B, -1))
    assert (np.abs(got - want) <= bound).all()
    other = ER.erase(MX.blend(plain.reshape(B, -1), lam).astype(np.float32).reshape(plain.shape), eng.erase_table_last, 2, SCALE)
    assert (np.abs(got - other.reshape(B, -1)) > bound).any()


# ---- 11. accumulation ------------------------------------------------------------------------------------------------------------------------
def test_accumulated_update_draws_a_table_per_micro_step():
    """accumulate 2, three updates, captured: every micro-step draws erase_table(.., step_count * 2 + i, ..).  Bit for bit the eager
    engine given those boxes through erase_boxes (its keys are the same draws)."""
    from vltf_amd.engine import LRCNEngine, erase_table
    p, _, _ = data()
    kw = dict(erase_prob=1.0, erase_seed=3, erase_mode="clip", accumulate=2)
    drawn = LRCNEngine(small_cfg(step_graph=True, **kw), max_clips=B, device=DEV)
    given = LRCNEngine(small_cfg(**kw), max_clips=B, device=DEV)
    drawn.load_params(p)
    given.load_params(p)
    seen = []
    for update in range(3):
        for i, c0 in enumerate((0, 2)):
            table = erase_table(small_cfg(**kw), update * 2 + i, 0, B, FPC, H, W)
            a = drawn.train_step_u8(*dev_batch(c0, c0 + B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, micro=(i, 2))
            b = given.train_step_u8(*dev_batch(c0, c0 + B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, micro=(i, 2),
                                    erase_boxes=[tuple(r[:6]) for r in table.tolist()])
            assert np.array_equal(drawn.erase_table_last, table) and np.array_equal(given.erase_table_last, table)
            assert a["loss_sum"] == b["loss_sum"] and a["correct"] == b["correct"] and a["rows"] == b["rows"], (update, i)
            seen.append(table.tobytes())
        assert a["grad_norm"] == b["grad_norm"] and same_bits(drawn, given), update
    assert len(set(seen)) == 6 and drawn.step_count == 3


# ---- 12. off is the engine of before -------------------------------------------------------------------------------------------------------
def test_erase_off_is_the_engine_of_before(monkeypatch):
    import vltf_amd.ops as ops_
    from vltf_amd._ffi import VltfError
    from vltf_amd.engine import LRCNEngine
    monkeypatch.setattr(ops_, "erase_boxes", lambda *a, **k: pytest.fail("erase_boxes was launched"))
    monkeypatch.setattr(ops_.Conv, "erase_boxes_s2d", lambda *a, **k: pytest.fail("erase_boxes_s2d was launched"))
    p, _, _ = data()
    none = dict.fromkeys(("erase_prob", "erase_scale", "erase_ratio", "erase_frames", "erase_mode", "erase_std", "erase_seed"))
    for base in (dict(), dict(conv_math="bf16"), dict(mixup_alpha=0.2, cutmix_alpha=1.0, cutmix_seed=7)):
        res = []
        for kw in (dict(erase_prob=0.0, erase_seed=0), none, dict()):
            eng = LRCNEngine(small_cfg(**dict(base, **kw)), max_clips=B, device=DEV)
            eng.load_params(p)
            assert eng.erase is None and eng.erase_table is None and eng.erase_table_last is None
            outs = [eng.train_step_u8(*dev_batch(c0, c0 + B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN) for c0 in (0, 2)]
            res.append((outs, eng.logits_host().copy(), eng.get_params()))
            with pytest.raises(VltfError, match="erase_boxes is given, but random erasing is off"):
                eng.train_step_u8(*dev_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, erase_boxes=EBOXES)
            with pytest.raises(VltfError, match="erase_boxes is given, but random erasing is off"):
                eng.train_step_f32(torch.zeros((B * FPC,) + SHAPE, device=DEV), dev_batch(0, B)[1], lr=LR, erase_boxes=EBOXES)
            assert eng.step_count == 2 and eng.erase_table is None
        for outs, logits, params in res[:2]:
            assert outs == res[2][0] and np.array_equal(logits.view(np.int32), res[2][1].view(np.int32))
            for k in params:
                assert np.array_equal(params[k].view(np.int32), res[2][2][k].view(np.int32)), k


# ---- 13. run_task on the example -------------------------------------------------------------------------------------------------------------
def test_run_task_on_the_example(tmp_path, monkeypatch):
    """examples/lrcn_erase.yml shrunk: the synthetic dataset and the small network of tests/test_run_task_gpu.py, one epoch, with the
    example's own mixup, cutmix and erase keys.  The info line is there, at least two steps ran with finite losses, and a second run logs
    the same losses."""
    from tests.test_host_workflow import make_dataset
    from tests.test_run_task_gpu import RAW, write_cfg
    from vltf_amd import run_task
    monkeypatch.setenv("VLTF_PREFETCH", "0")
    monkeypatch.setenv("VLTF_CONV_MATH", "f32")
    monkeypatch.delenv("VLTF_STEP_GRAPH", raising=False)
    with open(os.path.join(ROOT, "examples", "lrcn_erase.yml")) as f:
        example = yaml.safe_load(f)["run"]
    keys = ("mixup_alpha", "mixup_seed", "cutmix_alpha", "cutmix_seed", "cutmix_mode", "cutmix_prob", "erase_prob", "erase_scale",
            "erase_ratio", "erase_frames", "erase_mode", "erase_std", "erase_seed")
    assert [example["train"][k] for k in keys[6:]] == [0.25, [0.02, 0.33], [0.3, 3.3], [1.0, 1.0], "pixel", 57.63, 7]
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
        assert "Random erasing: prob 0.25, scale (0.02, 0.33), ratio (0.3, 3.3), frames (1.0, 1.0), mode pixel (std 57.63), seed 7" in log
        assert "CutMix: alpha 1.0" in log and "Mixup: alpha 0.2" in log
        found = [float(v) for v in re.findall(r"batch loss/nats : ([-+0-9.eE]+|nan|inf) /", log)]
        assert len(found) >= 2 and np.isfinite(found).all(), found
        losses.append(found)
    assert losses[0] == losses[1]
