"""Random resized crop on the device (vl_input_prep_u8_box, vl_input_prep_u8_box_s2d, the engines' crop_box): both feed kernels
against the fp64 reference of tests/scale_jitter_ref.py and against each other, the identity box against the crop kernels bit for bit,
the kernels' clamp, whole steps of LRCNEngine (drawn boxes against the fp64 oracle, identity boxes against the crop_y / crop_x step in
fp32 and on the bf16 conv path, captured and replayed with other boxes, with CutMix on), a two-tower GraphEngine, and run_task on the
example.

Tolerances.  The fp32 kernel against the fp64 rule: atol 3e-4 and no rtol -- at most 12 fp32 roundings (two weights, three lerps of
three roundings each, the mean) of values no larger than 255 + 109.5: 12 x 364.5 x 2^-24 = 2.6e-4.  Everything between the two
kernels, against the crop kernels and between captured and eager steps is compared in bits.  Whole steps against the fp64 oracle hold
the bounds of tests/test_mixup_gpu.py::check_step, which are those of tests/test_engine_gpu.py::test_train_step_small."""
import glob
import os
import re

import numpy as np
import pytest
import torch
import yaml

from oracle import lrcn_oracle as O
from tests import cutmix_ref as CM
from tests import mixup_ref as MX
from tests import scale_jitter_ref as SJ
from tests.test_label_smoothing_gpu import B, CLIP, FPC, LR, MEAN, SHAPE, bits, data, small_cfg
from tests.test_mixup_gpu import check_step, same_bits, step_keys_equal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = SHAPE[:2]
SENTINEL = 12345.0
ATOL = 3e-4

RH, RW, OH, OW, CLIPS, FFPC = 13, 15, 9, 11, 2, 3
# identity | full frame | upscale | one pixel | one row | one column | lower half: a different box per frame within one launch
BOXES = [(2, 3, 9, 11), (0, 0, 13, 15), (4, 5, 3, 4), (12, 14, 1, 1), (0, 0, 1, 15), (0, 0, 13, 1), (6, 0, 7, 15)]
_RAW = {}


@pytest.fixture(scope="module")
def ops():
    import vltf_amd.ops as ops_
    return ops_


def raw_frames(n, h, w, c=3):
    """[n, h, w, c] uint8, made once per shape and never written."""
    if (n, h, w, c) not in _RAW:
        _RAW[(n, h, w, c)] = np.random.default_rng(n * 1009 + h * 31 + w + c).integers(0, 256, (n, h, w, c), dtype=np.uint8)
    return _RAW[(n, h, w, c)]


def box_sets(n, boxes):
    """Three assignments of the box family to n frames, so that every box meets a mirrored and an unmirrored frame."""
    return [np.array([boxes[(i + s) % len(boxes)] for i in range(n)], np.int32) for s in (0, 3, 5)]


def idev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def feed_box(ops, frames, box, mirror, mean, halo, phase, oh=OH, ow=OW):
    """vl_input_prep_u8_box into a sentinel-filled x0: the halo rows, which the feed does not write, keep the sentinel."""
    x0 = torch.full(ops.phase_split_shape(len(frames), 3, oh, ow, halo, phase), SENTINEL, device=DEV)
    ops.input_prep_u8_box(idev(frames), x0, idev(np.asarray(box, np.int32)), None if mirror is None else idev(mirror),
                          None if mean is None else idev(mean), halo=halo, phase=phase, out_hw=(oh, ow))
    return x0


def unsplit(x0, n, oh, ow, halo, phase):
    """x0 (plain or column-phase-split) -> the padded NCHW array [n, 3, oh + 2 halo, wq * phase] of physical columns."""
    a = x0.cpu().numpy()
    if phase == 1:
        return a
    wq = a.shape[3]
    a = a.reshape(n, 3, phase, oh + 2 * halo, wq)
    return a.transpose(0, 1, 3, 4, 2).reshape(n, 3, oh + 2 * halo, wq * phase)              # column q * phase + ph


# ---- 1. the fp32 kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("halo,phase", [(0, 1), (2, 1), (2, 4)])
@pytest.mark.parametrize("with_mean", [True, False])
def test_box_kernel_against_fp64(ops, halo, phase, with_mean):
    n = CLIPS * FFPC
    frames = raw_frames(n, RH, RW)
    mirror = np.array([0, 1, 1, 0, 1, 0], np.uint8)
    mean = MEAN if with_mean else None
    for box in box_sets(n, BOXES):
        want = SJ.feed(frames, box, (OH, OW), mirror, mean).transpose(0, 3, 1, 2)
        x0 = feed_box(ops, frames, box, mirror, mean, halo, phase)
        got = unsplit(x0, n, OH, OW, halo, phase)
        inner = got[:, :, halo:halo + OH, halo:halo + OW]
        err = np.abs(inner.astype(np.float64) - want).max()
        print("halo %d phase %d mean %s: max |kernel - fp64| %.3e" % (halo, phase, with_mean, err))
        assert err <= ATOL
        # halo and padding columns of the interior rows are 0.0; the halo rows still hold the sentinel
        assert (got[:, :, halo:halo + OH, :halo] == 0.0).all() and (got[:, :, halo:halo + OH, halo + OW:] == 0.0).all()
        assert (got[:, :, :halo] == SENTINEL).all() and (got[:, :, halo + OH:] == SENTINEL).all()
        # a 1 x 1 box is the pixel minus the mean, exactly
        for i in np.nonzero((box[:, 2] == 1) & (box[:, 3] == 1))[0]:
            px = frames[i, box[i, 0], box[i, 1]].astype(np.float32) - (MEAN if with_mean else np.zeros(3, np.float32))
            assert (inner[i] == px[:, None, None]).all(), i


@pytest.mark.parametrize("halo,phase", [(0, 1), (2, 1), (2, 4)])
def test_identity_boxes_equal_the_crop_kernel_bit_for_bit(ops, halo, phase):
    n = CLIPS * FFPC
    frames = raw_frames(n, RH, RW)
    mirror = np.array([0, 1, 1, 0, 1, 0], np.uint8)
    cy, cx = np.array([2, 0, 4, 1, 3, 2], np.int32), np.array([3, 4, 0, 2, 1, 3], np.int32)
    box = np.stack([cy, cx, np.full(n, OH, np.int32), np.full(n, OW, np.int32)], 1)
    got = feed_box(ops, frames, box, mirror, MEAN, halo, phase)
    want = torch.full_like(got, SENTINEL)
    ops.input_prep_u8(idev(frames), want, idev(cy), idev(cx), idev(mirror), idev(MEAN), halo=halo, phase=phase, out_hw=(OH, OW))
    assert torch.equal(bits(got), bits(want))                                                # the WHOLE buffer
    same = feed_box(ops, frames, np.array([(2, 3, 9, 11)] * n, np.int32), None, None, halo, phase)
    want2 = torch.full_like(same, SENTINEL)
    ops.input_prep_u8(idev(frames), want2, idev(np.full(n, 2, np.int32)), idev(np.full(n, 3, np.int32)), None, None, halo=halo, phase=phase,
                      out_hw=(OH, OW))
    assert torch.equal(bits(same), bits(want2))


def test_many_blocks_and_an_upsampled_frame(ops):
    """More than one workgroup per image and per launch, out larger than raw in both axes, a size that is no multiple of anything."""
    n, rh, rw, oh, ow = 3, 21, 17, 67, 67
    frames = raw_frames(n, rh, rw)
    box = np.array([(0, 0, 21, 17), (5, 3, 9, 13), (20, 16, 1, 1)], np.int32)
    mirror = np.array([1, 0, 1], np.uint8)
    want = SJ.feed(frames, box, (oh, ow), mirror, MEAN).transpose(0, 3, 1, 2)
    for halo, phase in ((0, 1), (2, 4)):
        got = unsplit(feed_box(ops, frames, box, mirror, MEAN, halo, phase, oh, ow), n, oh, ow, halo, phase)
        assert np.abs(got[:, :, halo:halo + oh, halo:halo + ow].astype(np.float64) - want).max() <= ATOL


# ---- 2. the clamp ------------------------------------------------------------------------------------------------------------------------
def test_boxes_outside_the_frame_are_clamped(ops):
    """Defined behaviour: whatever the words hold, the launch samples SJ.clamp_box of them -- sizes into [1, raw], then the corner."""
    bad = [(2, 3, 0, 11), (2, 3, 99, 11), (-4, 3, 9, 11), (2, 9, 9, 11), (2 ** 31 - 1, -2 ** 31, -2 ** 31, 2 ** 31 - 1), (-1, -1, -1, -1)]
    n = len(bad)
    frames = raw_frames(CLIPS * FFPC, RH, RW)[:n]
    mirror = np.array([0, 1, 0, 1, 1, 0], np.uint8)
    clamped = np.array([SJ.clamp_box(b, RH, RW) for b in bad], np.int32)
    assert clamped.tolist() == [[2, 3, 1, 11], [0, 3, 13, 11], [0, 3, 9, 11], [2, 4, 9, 11], [12, 0, 1, 15], [0, 0, 1, 1]]
    got = feed_box(ops, frames, np.array(bad, np.int64).astype(np.int32), mirror, MEAN, 2, 4)
    want = feed_box(ops, frames, clamped, mirror, MEAN, 2, 4)
    assert torch.equal(bits(got), bits(want))
    conv, geom = s2d_desc(ops, "generic")
    cin, h, w, k, s = DESCS["generic"]
    f2 = raw_frames(n, RH, RW, cin)
    assert torch.equal(bits16(feed_box_s2d(ops, conv, geom, f2, np.array(bad, np.int64).astype(np.int32), mirror)),
                       bits16(feed_box_s2d(ops, conv, geom, f2, clamped, mirror)))


# ---- 3. the packed kernel ----------------------------------------------------------------------------------------------------------------
DESCS = {"conv1-like": (3, 19, 23, 11, 4), "generic": (2, 9, 10, 5, 2), "half-used last chunk": (3, 9, 10, 5, 2)}   # cin, h, w, k, stride
RAWS = {"conv1-like": (25, 31), "generic": (13, 15), "half-used last chunk": (13, 15)}


def s2d_desc(ops, name):
    cin, h, w, k, s = DESCS[name]
    conv = ops.Conv(cin, h, w, 8, k, k, s, 1)
    conv.set_halo(conv.same_pad(), 0, 0, 0)
    ka = (k - 1) // s + 1
    return conv, (cin * s * s, conv.oh, conv.ow, (ka - 1) // 2)


def bits16(t):
    return t.view(torch.int16)


def feed_box_s2d(ops, conv, geom, frames, box, mirror, mean=True):
    xb = torch.full(ops.c8_shape(len(frames), *geom), 7.0, dtype=torch.bfloat16, device=DEV)       # the feed writes every chunk
    m = torch.tensor([99.2, 105.3, 109.5][:conv.cin], device=DEV) if mean else None
    conv.input_prep_u8_box_s2d(idev(frames), xb, idev(np.asarray(box, np.int32)), None if mirror is None else idev(mirror), m)
    return xb


@pytest.mark.parametrize("name", list(DESCS))
def test_packed_kernel_equals_the_fp32_kernel_then_s2d(ops, name):
    conv, geom = s2d_desc(ops, name)
    cin, h, w, k, s = DESCS[name]
    rh, rw = RAWS[name]
    n = CLIPS * FFPC
    frames = raw_frames(n, rh, rw, cin)
    mirror = np.array([0, 1, 1, 0, 1, 0], np.uint8)
    family = [(2, 3, h, w), (0, 0, rh, rw), (4, 5, 3, 4), (rh - 1, rw - 1, 1, 1), (0, 0, 1, rw), (0, 0, rh, 1), (6, 0, 7, rw)]
    mean3 = torch.tensor([99.2, 105.3, 109.5], device=DEV)
    frames3 = frames if cin == 3 else np.ascontiguousarray(np.concatenate([frames, raw_frames(n, rh, rw, 3)[..., :3 - cin]], axis=3))
    from tests.test_cutmix_gpu import s2d_index
    for box in box_sets(n, family):
        for mir, mean in ((mirror, True), (None, False)):
            got = feed_box_s2d(ops, conv, geom, frames, box, mir, mean)
            # the fp32 kernel feeds three channels: a two-channel source rides in the first two, and their planes are conv's x0
            phase = max(conv.x_phase, 1)
            x3 = torch.zeros(ops.phase_split_shape(n, 3, h, w, conv.x_halo, phase), device=DEV)
            ops.input_prep_u8_box(idev(frames3), x3, idev(box), None if mir is None else idev(mir), mean3 if mean else None,
                                  halo=conv.x_halo, phase=phase, out_hw=(h, w))
            x0 = x3[:, :cin * phase].contiguous()
            assert tuple(x0.shape) == tuple(conv.x_shape(n))
            want = torch.full_like(got, 7.0)
            conv.s2d_c8_from_x0(x0, want)
            assert torch.equal(bits16(got), bits16(want)), (name, "against the fp32 kernel + s2d_c8_from_x0")     # the WHOLE packed buffer
            # and against the fp64 rule rounded to bf16 through fp32: the pixel map of tests/test_cutmix_gpu.py::s2d_index
            idx = s2d_index(CLIPS, FFPC, cin, h, w, k, s, conv).reshape(n, h, w, cin)
            ref = SJ.feed(frames, box, (h, w), mir, [99.2, 105.3, 109.5][:cin] if mean else None)
            flat = got.view(-1).float().cpu().numpy()
            # and one rounding to bf16 (8 significant bits: spacing 2^(e - 7), so half a spacing is at most |v| 2^-8)
            tol = ATOL + (np.abs(ref) + ATOL) * 2.0 ** -8
            assert (np.abs(flat[idx] - ref) <= tol).all(), name
            rest = np.ones(flat.size, bool)
            rest[idx.reshape(-1)] = False
            assert (flat[rest] == 0.0).all()                                              # padding and unused channel slots: zeros


# ---- 4. engine steps (the geometry of tests/test_mixup_gpu.py; raw frames larger than the input) ------------------------------------------
ERH, ERW = 73, 79
_E = {}


def edata():
    """4 clips of raw ERH x ERW frames with the parameters and labels of tests/test_label_smoothing_gpu.py::data; two drawn box sets."""
    if not _E:
        from vltf_amd.dataset_ import CROP_RATIO, resized_crop_boxes
        p, _, onehot = data()
        _E["raw"] = np.random.default_rng(31).integers(0, 256, (4 * FPC, ERH, ERW, 3), dtype=np.uint8)
        for k, counter in (("a", 0), ("b", 1)):
            boxes, flips = resized_crop_boxes(7, counter, 4, ERH, ERW, (0.3, 1.0), CROP_RATIO, True)
            _E[k] = (np.repeat(boxes, FPC, axis=0), np.repeat(flips, FPC))
        assert not np.array_equal(_E["a"][0], _E["b"][0]) and _E["a"][1].any()
        _E["oracle"] = {}
    return _E


def ebatch(c0, c1, which):
    e = edata()
    _, _, onehot = data()
    box, mir = e[which]
    s = slice(c0 * FPC, c1 * FPC)
    return (idev(e["raw"][s]), torch.tensor(onehot[c0:c1], device=DEV)), dict(crop_box=idev(box[s]), mirror=idev(mir[s]))


def resampled(c0, c1, which):
    """The reference feed of clips c0 .. c1: fp64 NHWC, box-sampled, mirrored, mean-subtracted."""
    e = edata()
    box, mir = e[which]
    s = slice(c0 * FPC, c1 * FPC)
    return SJ.feed(e["raw"][s], box[s], (H, W), mir[s], MEAN)


def test_engine_step_with_drawn_boxes_against_the_oracle():
    from vltf_amd._ffi import VltfError
    from vltf_amd.engine import LRCNEngine
    p, _, onehot = data()
    eng = LRCNEngine(small_cfg(), max_clips=B, device=DEV)
    eng.load_params(p)
    (frames, labels), kw = ebatch(0, B, "a")
    with pytest.raises(VltfError, match="crop_box .* refused together with crop_y / crop_x"):
        eng.train_step_u8(frames, labels, lr=LR, clip_norm=CLIP, mean_bgr=MEAN, crop_y=torch.zeros(B * FPC, dtype=torch.int32, device=DEV),
                          **kw)
    with pytest.raises(VltfError, match="crop_box"):
        eng.forward_u8(frames, MEAN, None, torch.zeros(B * FPC, dtype=torch.int32, device=DEV), crop_box=kw["crop_box"])
    assert eng.step_count == 0
    out = eng.train_step_u8(frames, labels, lr=LR, clip_norm=CLIP, mean_bgr=MEAN, **kw)
    want = O.lrcn_train_step(p, resampled(0, B, "a").astype(np.float32), onehot[:B], FPC, lr=LR, clip_norm=CLIP)
    check_step(out, eng, want, onehot[:B])
    # and forward_u8 gives the logits of the same feed
    fwd = LRCNEngine(small_cfg(), max_clips=B, device=DEV, training=False)
    fwd.load_params(p)
    z = fwd.forward_u8(frames, MEAN, crop_box=kw["crop_box"], mirror=kw["mirror"]).cpu().numpy()
    np.testing.assert_allclose(z, want[4], rtol=1e-3, atol=1e-3)


@pytest.mark.parametrize("conv_math", ["f32", "bf16"])
def test_identity_boxes_are_the_crop_step_bit_for_bit(conv_math):
    from vltf_amd.engine import LRCNEngine
    p, _, onehot = data()
    e = edata()
    n = B * FPC
    rng = np.random.default_rng(3)
    cy, cx = rng.integers(0, ERH - H + 1, n).astype(np.int32), rng.integers(0, ERW - W + 1, n).astype(np.int32)
    mir = rng.integers(0, 2, n).astype(np.uint8)
    box = np.stack([cy, cx, np.full(n, H, np.int32), np.full(n, W, np.int32)], 1)
    frames, labels = idev(e["raw"][:n]), torch.tensor(onehot[:B], device=DEV)
    engines = [LRCNEngine(small_cfg(conv_math=conv_math), max_clips=B, device=DEV) for _ in range(2)]
    for eng in engines:
        eng.load_params(p)
    a = engines[0].train_step_u8(frames, labels, lr=LR, clip_norm=CLIP, mean_bgr=MEAN, crop_y=idev(cy), crop_x=idev(cx), mirror=idev(mir))
    b = engines[1].train_step_u8(frames, labels, lr=LR, clip_norm=CLIP, mean_bgr=MEAN, mirror=idev(mir), crop_box=idev(box))
    assert engines[0].c8 == (conv_math == "bf16")
    assert step_keys_equal(a, b) and a == b and same_bits(*engines)
    assert np.array_equal(engines[0].logits_host().view(np.int32), engines[1].logits_host().view(np.int32))
    if conv_math == "bf16":
        assert torch.equal(bits16(engines[0].layers[0]["xb"][:n]), bits16(engines[1].layers[0]["xb"][:n]))
    else:
        assert torch.equal(bits(engines[0].x0[:n]), bits(engines[1].x0[:n]))


def test_captured_step_replayed_with_other_boxes_equals_eager():
    """Step 1 is the warm-up, step 2 is captured and replayed, step 3 is a replay with the second box set."""
    from vltf_amd.engine import LRCNEngine
    p, _, _ = data()
    eager = LRCNEngine(small_cfg(), max_clips=B, device=DEV)
    graph = LRCNEngine(small_cfg(step_graph=True), max_clips=B, device=DEV)
    eager.load_params(p)
    graph.load_params(p)
    outs_by_step = []
    for step, (c0, which) in enumerate(((0, "a"), (2, "a"), (0, "b"))):
        outs = []
        for eng in (eager, graph):
            args, kw = ebatch(c0, c0 + B, which)
            outs.append(eng.train_step_u8(*args, lr=LR, clip_norm=CLIP, mean_bgr=MEAN, **kw))
        assert step_keys_equal(*outs), (step, outs)
        assert same_bits(eager, graph), step
        assert np.array_equal(eager.logits_host().view(np.int32), graph.logits_host().view(np.int32))
        outs_by_step.append(outs[1])
    assert len(graph._graphs) == 1 and "crop_box" in next(iter(graph._graphs.values()))["inputs"]
    # the boxes are a graph input, their presence is part of the key: a crop_y / crop_x step is another graph
    args, _ = ebatch(0, B, "a")
    zero = torch.zeros(B * FPC, dtype=torch.int32, device=DEV)
    for _ in range(2):
        graph.train_step_u8(*args, lr=LR, clip_norm=CLIP, mean_bgr=MEAN, crop_y=zero, crop_x=zero)
    assert len(graph._graphs) == 2
    assert outs_by_step[0]["loss_sum"] != outs_by_step[2]["loss_sum"]


def test_step_with_cutmix_on_and_boxes_given():
    from vltf_amd.engine import LRCNEngine
    p, _, onehot = data()
    cut = (0, 3, 10, 40, 20, 63)
    eng = LRCNEngine(small_cfg(cutmix_alpha=1.0, cutmix_seed=7), max_clips=B, device=DEV)
    eng.load_params(p)
    args, kw = ebatch(0, B, "a")
    out = eng.train_step_u8(*args, lr=LR, clip_norm=CLIP, mean_bgr=MEAN, cut_box=cut, **kw)
    x = resampled(0, B, "a").astype(np.float32).reshape((B, FPC) + SHAPE)               # resampled, then swapped
    lam = CM.lam(cut, FPC, H, W)
    want = O.lrcn_train_step(p, CM.swap(x, cut).reshape((B * FPC,) + SHAPE), MX.targets(onehot[:B], lam, 0.0), FPC, lr=LR, clip_norm=CLIP)
    check_step(out, eng, want, onehot[:B])


def test_two_tower_graph_engine_forward_with_boxes_in_one_feed():
    from tests import graph_cases as GC
    from vltf_amd.graph import GraphEngine
    case = GC.two_stream("avg")
    pipes, ds = GC.specs_and_datasets(case)
    eng = GraphEngine(pipes, ds, case["V"], device=DEV)
    eng.load_params(eng.init_params(seed=case["seed"], well_scaled=True))
    e = edata()
    n = case["items"] * 3
    raw, _ = GC.inputs(case)
    box, mir = e["a"][0][:n], e["a"][1][:n]
    rgb = idev(e["raw"][:n])
    feeds = {"main": dict(frames_u8=rgb, mean_bgr=GC.MEAN, mirror=idev(mir), crop_box=idev(box)),
             "aux": dict(frames_u8=idev(raw["aux"]), mean_bgr=GC.MEAN)}
    z = eng.forward(feeds).clone()
    tw, other = eng.by_name["rgb"].tower, eng.by_name["flow"].tower
    feat, x0, flow_feat = tw.logits[:n].clone(), tw.x0[:n].clone(), other.logits[:n].clone()
    # the tower fed alone: the same x0 and the same features, bit for bit
    tw.feed_u8(rgb, GC.MEAN, mirror=idev(mir), crop_box=idev(box))
    tw._forward(n, n // 3, False)
    assert torch.equal(bits(tw.x0[:n]), bits(x0)) and torch.equal(bits(tw.logits[:n]), bits(feat))
    want = SJ.feed(e["raw"][:n], box, (H, W), mir, GC.MEAN).transpose(0, 3, 1, 2)
    hl, ph = tw.x0_halo, tw.x0_phase
    got = unsplit(x0, n, H, W, hl, ph)[:, :, hl:hl + H, hl:hl + W]
    assert np.abs(got.astype(np.float64) - want).max() <= ATOL
    # other boxes in that feed move the logits and leave the other tower's features alone
    feeds["main"]["crop_box"] = idev(e["b"][0][:n])
    z2 = eng.forward(feeds)
    assert not torch.equal(z2, z) and torch.equal(bits(other.logits[:n]), bits(flow_feat))


# ---- 5. run_task on the example -----------------------------------------------------------------------------------------------------------
def test_run_task_on_the_example(tmp_path, monkeypatch):
    """examples/lrcn_scale_jitter.yml shrunk: the synthetic dataset and the small network of tests/test_run_task_gpu.py, one epoch of two
    steps with the example's own imgproc list and crop keys, fed synchronously and through the read-ahead: the same finite losses."""
    from tests.test_host_workflow import make_dataset
    from tests.test_run_task_gpu import RAW, write_cfg
    from vltf_amd import run_task
    monkeypatch.setenv("VLTF_CONV_MATH", "f32")
    monkeypatch.delenv("VLTF_STEP_GRAPH", raising=False)
    with open(os.path.join(ROOT, "examples", "lrcn_scale_jitter.yml")) as f:
        entry = yaml.safe_load(f)["run"]["data"]["train_set"]
    keys = ("imgproc", "crop_scale", "crop_ratio", "crop_seed")
    assert entry["imgproc"][0] == "defs.imgproc.rand_resized_crop"
    folder = str(tmp_path)
    train_path, _, _ = make_dataset(folder, "train.txt", nvid=4, cpv=(1, 2, 1, 1), shape=RAW, seed=1)
    losses = []
    for run, prefetch in (("run_a", "0"), ("run_b", "2")):
        monkeypatch.setenv("VLTF_PREFETCH", prefetch)
        out = write_cfg(folder, run + ".yml", train_path, "train", epochs=1, det=True, run=run)
        with open(out) as f:
            c = yaml.safe_load(f)
        c["run"]["data"]["d"].update({k: entry[k] for k in keys})
        with open(out, "w") as f:
            yaml.safe_dump(c, f)
        run_task.main(out, seed=3)
        log = open(glob.glob(os.path.join(folder, run, "log_e2e_train_scratch_*.log"))[0]).read()
        assert "Random resized crop: scale (0.08, 1.0), ratio (0.75, 1.3333), seed 7" in log
        found = [float(v) for v in re.findall(r"batch loss/nats : ([-+0-9.eE]+|nan|inf) /", log)]
        assert len(found) == 2 and np.isfinite(found).all(), found
        losses.append(found)
    assert losses[0] == losses[1]
