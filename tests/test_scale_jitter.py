"""Random resized crop on the host: the fp64 reference against torch's F.interpolate, the draws of
dataset_.resized_crop_boxes and their properties, the Dataset over the committed config1 TFRecord (tuple shape, clip consistency,
shards, resume), the YAML keys with their refusals, the example, the C-ABI rows and the entry points' argument checks.  No GPU:
nothing is launched."""
import os
import random

import numpy as np
import pytest
import torch
import yaml

from tests import scale_jitter_ref as SJ
from tests.test_host_workflow import config, make_dataset
from vltf_amd import settings_
from vltf_amd.dataset_ import CROP_RATIO, CROP_SCALE, Dataset, check_crop_jitter, resized_crop_boxes
from vltf_amd.defs_ import defs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "config1")
MEAN = [99.197148, 105.293620, 109.503945]
RRC = [defs.imgproc.rand_resized_crop, defs.imgproc.rand_mirror, defs.imgproc.sub_mean]


# ---- the reference against torch ----------------------------------------------------------------------------------------------------
def _cases():
    rng = np.random.default_rng(11)
    cases = [((13, 15), (12, 14, 1, 1), (9, 11)), ((13, 15), (0, 0, 1, 15), (9, 11)), ((13, 15), (0, 0, 13, 1), (9, 11)),
             ((13, 15), (4, 5, 3, 4), (9, 11)), ((13, 15), (0, 0, 13, 15), (9, 11)), ((13, 15), (2, 3, 9, 11), (9, 11)),
             ((5, 7), (1, 2, 3, 3), (31, 29)), ((40, 50), (3, 4, 33, 41), (7, 5)), ((1, 1), (0, 0, 1, 1), (4, 3))]
    for _ in range(60):
        h, w = (int(v) for v in rng.integers(1, 41, 2))
        bh, bw = int(rng.integers(1, h + 1)), int(rng.integers(1, w + 1))
        box = (int(rng.integers(0, h - bh + 1)), int(rng.integers(0, w - bw + 1)), bh, bw)
        cases.append(((h, w), box, tuple(int(v) for v in rng.integers(1, 45, 2))))
    return cases


def test_reference_agrees_with_torch_interpolate():
    rng = np.random.default_rng(5)
    up = down = 0
    for (h, w), box, out_hw in _cases():
        frame = rng.integers(0, 256, (h, w, 3)).astype(np.float64)
        y0, x0, bh, bw = box
        crop = torch.from_numpy(frame[y0:y0 + bh, x0:x0 + bw].transpose(2, 0, 1)[None].copy())
        want = torch.nn.functional.interpolate(crop, size=out_hw, mode="bilinear", align_corners=False)[0].numpy().transpose(1, 2, 0)
        got = SJ.sample_box(frame, box, out_hw)
        assert np.abs(got - want).max() <= 1e-9, ((h, w), box, out_hw, np.abs(got - want).max())
        up += out_hw[0] > bh or out_hw[1] > bw
        down += out_hw[0] < bh or out_hw[1] < bw
    assert up > 10 and down > 10


def test_reference_identity_box_is_the_plain_crop():
    rng = np.random.default_rng(6)
    frame = rng.integers(0, 256, (13, 15, 3), dtype=np.uint8)
    got = SJ.sample_box(frame, (2, 3, 9, 11), (9, 11))
    assert np.array_equal(got, frame[2:11, 3:14].astype(np.float64))
    frames = frame[None]
    fed = SJ.feed(frames, [(2, 3, 9, 11)], (9, 11), mirror=[1], mean=MEAN)
    assert np.array_equal(fed[0], frame[2:11, 3:14][:, ::-1].astype(np.float64) - np.asarray(MEAN, np.float64))
    assert SJ.clamp_box((-3, 9, 0, 40), 13, 15) == (0, 0, 1, 15) and SJ.clamp_box((12, 14, 5, 5), 13, 15) == (8, 10, 5, 5)


# ---- resized_crop_boxes ---------------------------------------------------------------------------------------------------------------
def test_boxes_are_a_pure_function_inside_the_frame_and_the_ranges():
    state = np.random.get_state()[1].copy()
    pystate = random.getstate()
    a = resized_crop_boxes(7, 3, 200, 240, 320, CROP_SCALE, CROP_RATIO, True)
    b = resized_crop_boxes(7, 3, 200, 240, 320, CROP_SCALE, CROP_RATIO, True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(np.random.get_state()[1], state) and random.getstate() == pystate      # no global generator is consumed
    boxes, mirror = a
    assert boxes.dtype == np.int32 and boxes.shape == (200, 4) and mirror.dtype == np.uint8 and mirror.shape == (200,)
    assert set(np.unique(mirror)) == {0, 1}
    ref_boxes, ref_mirror, fell = SJ.draw_boxes(7, 3, 200, 240, 320)
    assert np.array_equal(boxes, ref_boxes) and np.array_equal(mirror, ref_mirror)
    y0, x0, bh, bw = boxes.T.astype(np.int64)
    assert (bh >= 1).all() and (bw >= 1).all() and (y0 >= 0).all() and (x0 >= 0).all()
    assert (y0 + bh <= 240).all() and (x0 + bw <= 320).all()
    # area and ratio inside the ranges up to the round of the two sides (each side moves by at most 1 / 2)
    ok = ~fell
    assert ok.sum() > 150
    for h, w in zip(bh[ok], bw[ok]):
        lo_a, hi_a = (h - 0.5) * (w - 0.5), (h + 0.5) * (w + 0.5)
        assert hi_a >= CROP_SCALE[0] * 240 * 320 and lo_a <= CROP_SCALE[1] * 240 * 320, (h, w)
        assert (w + 0.5) / (h - 0.5) >= CROP_RATIO[0] and (w - 0.5) / (h + 0.5) <= CROP_RATIO[1], (h, w)
    # other keys, other draws
    assert not np.array_equal(boxes, resized_crop_boxes(7, 4, 200, 240, 320, CROP_SCALE, CROP_RATIO, True)[0])
    assert not np.array_equal(boxes, resized_crop_boxes(8, 3, 200, 240, 320, CROP_SCALE, CROP_RATIO, True)[0])
    # a prefix of the clips draws a prefix of the boxes (clip by clip, in order)
    assert np.array_equal(resized_crop_boxes(7, 3, 50, 240, 320, CROP_SCALE, CROP_RATIO, True)[0], boxes[:50])


def test_mirror_off_leaves_the_boxes_unchanged():
    on = resized_crop_boxes(2, 9, 64, 240, 320, (0.3, 0.9), (0.5, 2.0), True)
    off = resized_crop_boxes(2, 9, 64, 240, 320, (0.3, 0.9), (0.5, 2.0), False)
    assert np.array_equal(on[0], off[0]) and on[1].any() and not off[1].any()


def test_fallback_box_for_a_ratio_the_frame_cannot_satisfy():
    # the whole frame's area at ratio >= 3 over a 240 x 320 frame: bw = sqrt(240 * 320 * 3) = 480 > 320 on every attempt
    boxes, _ = resized_crop_boxes(0, 0, 5, 240, 320, (1.0, 1.0), (3.0, 4.0), True)
    assert (boxes == np.array([66, 0, 107, 320])).all()              # ratio 4 / 3 < 3: bw = 320, bh = round(320 / 3) = 107, centred
    boxes, _ = resized_crop_boxes(0, 0, 5, 240, 320, (1.0, 1.0), (0.2, 0.25), True)
    assert (boxes == np.array([0, 130, 240, 60])).all()              # ratio 4 / 3 > 1 / 4: bh = 240, bw = round(240 / 4) = 60
    assert SJ.draw_boxes(0, 0, 5, 240, 320, (1.0, 1.0), (3.0, 4.0))[2].all()
    # the full frame at its own ratio is an ordinary accepted draw
    boxes, _ = resized_crop_boxes(0, 0, 3, 240, 320, (1.0, 1.0), (4.0 / 3.0, 4.0 / 3.0), True)
    assert (boxes == np.array([0, 0, 240, 320])).all()


def test_check_crop_jitter():
    assert check_crop_jitter() == (CROP_SCALE, CROP_RATIO, 0) == ((0.08, 1.0), (0.75, 4.0 / 3.0), 0)
    assert check_crop_jitter([0.5, 1], (1, 2), 2 ** 64 - 1) == ((0.5, 1.0), (1.0, 2.0), 2 ** 64 - 1)
    for bad in ([0.0, 1.0], [0.5, 0.4], [0.5, 1.5], [0.5], [0.1, 0.2, 0.3], 0.5, "0.5", [float("nan"), 1.0], [0.1, float("inf")],
                [True, 1.0], ["a", "b"]):
        with pytest.raises(ValueError, match="crop_scale"):
            check_crop_jitter(bad)
    for bad in ([0.0, 1.0], [-1.0, 1.0], [2.0, 1.0], [1.0], 1.0, [1.0, float("inf")], [float("nan"), 2.0]):
        with pytest.raises(ValueError, match="crop_ratio"):
            check_crop_jitter(None, bad)
    assert check_crop_jitter(None, [0.5, 3.0])[1] == (0.5, 3.0)           # no upper limit on the ratio
    for bad in (-1, 2 ** 64, 1.5, "7", True, [7]):
        with pytest.raises(ValueError, match="crop_seed"):
            check_crop_jitter(None, None, bad)


# ---- Dataset over the committed TFRecord (2 videos of one clip, 4 frames of 240 x 320 each) ----------------------------------------
def _dataset(imgproc, jitter=None, batch=2):
    d = Dataset()
    d.initialize("c1", os.path.join(FIX, "frames.txt"), MEAN, None, (227, 227, 3), imgproc, (240, 320, 3), defs.data_format.tfrecord, "jpg",
                 defs.batch_item.default, 101, defs.dataset_tag.main, 1, crop_jitter=jitter)
    d.calculate_batches(batch, defs.input_mode.video)
    return d


def test_dataset_option_off_keeps_its_draws_and_has_no_box():
    d = _dataset([defs.imgproc.rand_crop, defs.imgproc.rand_mirror, defs.imgproc.sub_mean])
    d.seed(3)
    out = d.get_next_batch()
    assert len(out) == 5 and d.crop_box is None
    frames, cy, cx, mirror, onehot = out
    assert frames.shape == (8, 240, 320, 3) and cy.shape == cx.shape == mirror.shape == (8,) and onehot.shape == (2, 101)


def test_dataset_one_box_and_one_flag_per_clip():
    jitter = check_crop_jitter([0.2, 0.9], None, 7)
    d = _dataset(RRC, jitter)
    d.seed(3)
    before = d.rng.getstate()
    out = d.get_next_batch()
    assert len(out) == 5                                                   # the 5-tuple is kept
    frames, cy, cx, mirror, onehot = out
    assert cy is None and cx is None and frames.shape == (8, 240, 320, 3) and onehot.shape == (2, 101)
    assert d.rng.getstate() == before                                      # the reference's `random` draws are not consumed
    box = d.crop_box
    assert box.dtype == np.int32 and box.shape == (8, 4) and mirror.dtype == np.uint8 and mirror.shape == (8,)
    want_box, want_mirror = resized_crop_boxes(7, 0, 2, 240, 320, (0.2, 0.9), CROP_RATIO, True)
    for c in range(2):                                                      # a clip's four frames share one row and one flag
        assert (box[4 * c:4 * c + 4] == want_box[c]).all() and (mirror[4 * c:4 * c + 4] == want_mirror[c]).all()
    assert len({tuple(r) for r in box}) == 2
    # without rand_mirror the boxes are the same and nothing is flipped
    d2 = _dataset([defs.imgproc.rand_resized_crop, defs.imgproc.sub_mean], jitter)
    _, _, _, mirror2, _ = d2.get_next_batch()
    assert np.array_equal(d2.crop_box, box) and not mirror2.any()


def test_dataset_two_shards_equal_the_one_process_draw():
    jitter = check_crop_jitter(None, None, 5)
    whole = _dataset(RRC, jitter)
    frames, _, _, mirror, onehot = whole.get_next_batch()
    parts = []
    for rank in range(2):
        d = _dataset(RRC, jitter)
        d.set_shard(rank, 2)
        f, cy, cx, m, oh = d.get_next_batch()
        assert cy is None and cx is None and d.global_clips == 2
        parts.append((f, d.crop_box, m, oh))
    assert [len(p[0]) for p in parts] == [4, 4]                             # a video of one clip each
    assert np.array_equal(np.concatenate([p[0] for p in parts]), frames)
    assert np.array_equal(np.concatenate([p[1] for p in parts]), whole.crop_box)
    assert np.array_equal(np.concatenate([p[2] for p in parts]), mirror)
    assert np.array_equal(np.concatenate([p[3] for p in parts]), onehot)


def test_dataset_restore_continues_the_sequence():
    jitter = check_crop_jitter(None, None, 9)
    a = _dataset(RRC, jitter, batch=1)                                      # two batches of one clip an epoch
    seq = []
    for epoch in range(2):
        while a.loop():
            _, _, _, m, _ = a.get_next_batch()
            seq.append((a.crop_box.copy(), m.copy()))
        a.rewind()
    assert len(seq) == 4 and [len(s[0]) for s in seq] == [4, 4, 4, 4]
    assert not np.array_equal(seq[0][0], seq[2][0])                         # the second epoch draws anew
    for batch_index, epoch_index, k in ((1, 0, 1), (0, 1, 2), (1, 1, 3)):
        b = _dataset(RRC, jitter, batch=1)
        b.restore(batch_index, epoch_index)
        _, _, _, m, _ = b.get_next_batch()
        assert np.array_equal(b.crop_box, seq[k][0]) and np.array_equal(m, seq[k][1]), (batch_index, epoch_index)


# ---- settings -------------------------------------------------------------------------------------------------------------------------
def _settings(tmp_path, data=None, imgproc=None, phase="train"):
    folder = str(tmp_path)
    data_path, _, _ = make_dataset(folder, "%s.txt" % phase)
    path = config(folder, data_path, phase=phase)
    with open(path) as f:
        cfg = yaml.safe_load(f)
    entry = cfg["run"]["data"]["d1"]
    if imgproc is not None:
        entry["imgproc"] = ["defs.imgproc.%s" % o for o in imgproc]
    entry.update(data or {})
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    s = settings_.Settings()
    return s, s.initialize(path)


def test_settings_parse_the_keys_and_the_defaults(tmp_path):
    s, feeder = _settings(tmp_path, {"crop_scale": [0.25, 0.75], "crop_ratio": "(0.5, 2.0)", "crop_seed": 7},
                          ("rand_resized_crop", "rand_mirror", "sub_mean"))
    d = feeder.get_dataset_by_tag("main")[0]
    assert (d.crop_scale, d.crop_ratio, d.crop_seed) == ((0.25, 0.75), (0.5, 2.0), 7)
    assert d.crop_mode == defs.imgproc.rand_resized_crop and d.resize_chain == []
    fdict, num_data, num_labels, _ = feeder.get_feed_dict()
    assert fdict["crop_y"] is None and fdict["crop_x"] is None and fdict["crop_box"].shape == (num_data[0], 4)
    assert fdict["mirror"].shape == (num_data[0],)
    want, _ = resized_crop_boxes(7, 0, num_labels, 20, 24, (0.25, 0.75), (0.5, 2.0), True)
    assert np.array_equal(fdict["crop_box"], np.repeat(want, 3, axis=0))
    s, feeder = _settings(tmp_path, {"crop_scale": "None"}, ("rand_resized_crop", "sub_mean"))
    d = feeder.get_dataset_by_tag("main")[0]
    assert (d.crop_scale, d.crop_ratio, d.crop_seed) == (CROP_SCALE, CROP_RATIO, 0)
    # the option off: the feed dict has the key, and it is None
    s, feeder = _settings(tmp_path)
    assert feeder.get_feed_dict()[0]["crop_box"] is None


@pytest.mark.parametrize("imgproc,data,phase,msg", [
    (("rand_resized_crop", "rand_crop", "sub_mean"), {}, "train", "refused together with"),
    (("rand_resized_crop", "center_crop", "sub_mean"), {}, "train", "refused together with"),
    (("rand_resized_crop", "resize", "sub_mean"), {}, "train", "refused together with"),
    (("rand_resized_crop", "sub_mean"), {}, "val", "validation"),
    (("rand_resized_crop", "sub_mean"), {"crop_scale": [0.0, 1.0]}, "train", "crop_scale"),
    (("rand_resized_crop", "sub_mean"), {"crop_scale": [0.5, 1.5]}, "train", "crop_scale"),
    (("rand_resized_crop", "sub_mean"), {"crop_scale": [0.6, 0.5]}, "train", "crop_scale"),
    (("rand_resized_crop", "sub_mean"), {"crop_scale": 0.5}, "train", "crop_scale"),
    (("rand_resized_crop", "sub_mean"), {"crop_scale": [0.1, float("inf")]}, "train", "crop_scale"),
    (("rand_resized_crop", "sub_mean"), {"crop_ratio": [2.0, 1.0]}, "train", "crop_ratio"),
    (("rand_resized_crop", "sub_mean"), {"crop_ratio": [0.0, 1.0]}, "train", "crop_ratio"),
    (("rand_resized_crop", "sub_mean"), {"crop_ratio": [1.0, float("nan")]}, "train", "crop_ratio"),
    (("rand_resized_crop", "sub_mean"), {"crop_seed": -1}, "train", "crop_seed"),
    (("rand_resized_crop", "sub_mean"), {"crop_seed": 1.5}, "train", "crop_seed"),
    (("rand_resized_crop", "sub_mean"), {"crop_seed": 2 ** 64}, "train", "crop_seed"),
    (("rand_crop", "sub_mean"), {"crop_scale": [0.5, 1.0]}, "train", "need imgproc"),
    (("rand_crop", "sub_mean"), {"crop_ratio": [0.5, 1.0]}, "train", "need imgproc"),
    (("center_crop", "sub_mean"), {"crop_seed": 3}, "train", "need imgproc"),
])
def test_settings_refusals(tmp_path, imgproc, data, phase, msg):
    with pytest.raises(Exception, match=msg):
        _settings(tmp_path, data, imgproc, phase)


def test_vectors_dataset_refuses_the_entry():
    d = Dataset()
    d.initialize("v", "unused", None, None, None, [defs.imgproc.rand_resized_crop], None, defs.data_format.tfrecord, None,
                 defs.batch_item.default, 4, defs.dataset_tag.aux, 1)
    d.input_mode = defs.input_mode.vectors
    with pytest.raises(Exception, match="no frames to crop"):
        d.initialize_imgproc()


def test_example_yaml_parses(tmp_path):
    with open(os.path.join(ROOT, "examples", "lrcn_scale_jitter.yml")) as f:
        cfg = yaml.safe_load(f)["run"]
    entry = cfg["data"]["train_set"]
    assert entry["imgproc"] == ["defs.imgproc.rand_resized_crop", "defs.imgproc.rand_mirror", "defs.imgproc.sub_mean"]
    assert (entry["crop_scale"], entry["crop_ratio"], entry["crop_seed"]) == ([0.08, 1.0], [0.75, 1.3333], 7)
    s, feeder = _settings(tmp_path, {k: entry[k] for k in ("crop_scale", "crop_ratio", "crop_seed")},
                          [o.split(".")[-1] for o in entry["imgproc"]])
    d = feeder.get_dataset_by_tag("main")[0]
    assert (d.crop_scale, d.crop_ratio, d.crop_seed) == ((0.08, 1.0), (0.75, 1.3333), 7)


# ---- C-ABI ------------------------------------------------------------------------------------------------------------------------------
def test_ffi_rows_and_ops_names():
    from tests.test_mixup import _header_arg_count
    from vltf_amd import _ffi
    import vltf_amd.ops as ops
    p, i32 = _ffi.p, _ffi.i32
    assert _ffi.SIGNATURES["vl_input_prep_u8_box"] == (i32, [p, p, i32, i32, i32, i32, i32, p, p, p, i32, i32, p])
    assert _ffi.SIGNATURES["vl_input_prep_u8_box_s2d"] == (i32, [p, p, p, i32, i32, i32, p, p, p, p])
    for name in ("vl_input_prep_u8_box", "vl_input_prep_u8_box_s2d"):
        assert len(_ffi.SIGNATURES[name][1]) == _header_arg_count(name), name
    assert _ffi.SIGNATURES["vl_input_prep_u8"] == (i32, [p, p, i32, i32, i32, i32, i32, p, p, p, p, i32, i32, p])      # as it was
    assert callable(ops.input_prep_u8_box) and callable(ops.Conv.input_prep_u8_box_s2d)


def test_host_refusals_need_no_device():
    """Both entry points validate before they launch.  The addresses are never touched: nothing runs."""
    from vltf_amd import _ffi
    lib = _ffi.lib()
    fake = 4096
    ok = dict(src=fake, dst=fake, n=6, rh=13, rw=15, oh=9, ow=11, box=fake, halo=2, phase=4)
    for change, msg in ((dict(src=None), b"bad argument"), (dict(dst=None), b"bad argument"), (dict(box=None), b"bad argument"),
                        (dict(halo=-1), b"bad argument"), (dict(phase=0), b"bad argument"), (dict(n=0), b"bad shape"),
                        (dict(oh=0), b"bad shape"), (dict(ow=-11), b"bad shape"), (dict(rh=0), b"bad shape"), (dict(rw=-1), b"bad shape"),
                        (dict(n=65536), b"exceeds the grid limit"), (dict(rh=1 << 20, oh=1 << 20), b"image too large")):
        a = dict(ok, **change)
        rc = lib.vl_input_prep_u8_box(a["src"], a["dst"], a["n"], a["rh"], a["rw"], a["oh"], a["ow"], a["box"], None, None, a["halo"],
                                      a["phase"], None)
        err = lib.vl_last_error()
        assert rc != 0 and b"vl_input_prep_u8_box" in err and msg in err, (change, err)
    s2d = lib.vl_input_prep_u8_box_s2d
    assert s2d(None, None, fake, 6, 13, 15, fake, None, None, None) != 0 and b"vl_input_prep_u8_box_s2d: bad argument" in lib.vl_last_error()
    assert s2d(None, fake, None, 6, 13, 15, fake, None, None, None) != 0 and b"vl_input_prep_u8_box_s2d: bad argument" in lib.vl_last_error()
    assert s2d(None, fake, fake, 6, 13, 15, None, None, None, None) != 0 and b"vl_input_prep_u8_box_s2d: bad argument" in lib.vl_last_error()
    assert s2d(None, fake, fake, 6, 0, 15, fake, None, None, None) != 0 and b"vl_input_prep_u8_box_s2d: bad shape" in lib.vl_last_error()
    assert s2d(None, fake, fake, 65536, 13, 15, fake, None, None, None) != 0 and b"vl_input_prep_u8_box_s2d: bad shape" in lib.vl_last_error()
    assert s2d(None, fake, fake, 6, 13, 15, fake, None, None, None) != 0                  # a null descriptor: s2d_check's refusal
    assert b"vl_input_prep_u8_box_s2d: a strided, ungrouped, square layer" in lib.vl_last_error()


def test_engine_refuses_a_box_beside_crop_offsets_before_any_launch():
    from vltf_amd._ffi import VltfError
    from vltf_amd.engine import LRCNEngine
    box = object()                                       # never looked at: the refusal comes first
    with pytest.raises(VltfError, match="crop_box .* refused together with crop_y / crop_x"):
        LRCNEngine._check_crop_box(box, object(), None)
    with pytest.raises(VltfError, match="crop_box"):
        LRCNEngine._check_crop_box(box, None, object())
    LRCNEngine._check_crop_box(box, None, None)
    LRCNEngine._check_crop_box(None, object(), object())
