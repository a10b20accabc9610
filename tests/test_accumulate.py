"""Gradient accumulation on the host: the `accumulate` key of the `train:` section and its refusals, engine.check_accumulate, the
micro-step sequence both engines keep, train.accumulate_groups, and what Train.run_step / run_task.do_train hand an engine -- on a fake
engine that records its calls.  No GPU: no engine is constructed."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import yaml

from tests.test_finetune import _settings
from vltf_amd import _ffi
from vltf_amd._ffi import VltfError
from vltf_amd.defs_ import defs
from vltf_amd.engine import MicroSequence, NetConfig, check_accumulate
from vltf_amd.train import Train, accumulate_groups

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- settings ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train,want", [({}, 1), ({"accumulate": None}, 1), ({"accumulate": "None"}, 1), ({"accumulate": 1}, 1),
                                        ({"accumulate": 4}, 4)], ids=["absent", "null", "None-string", "one", "four"])
def test_settings_accumulate_parses(tmp_path, train, want):
    s = _settings(tmp_path, train=train)
    assert s.train.accumulate == want and type(s.train.accumulate) is int
    assert NetConfig().accumulate == 1


@pytest.mark.parametrize("bad", [0, -2, 1.5, "x", True], ids=["zero", "negative", "fraction", "string", "bool"])
def test_settings_refusals(tmp_path, bad):
    with pytest.raises(Exception, match=r"train\.accumulate"):
        _settings(tmp_path, train={"accumulate": bad})


def test_check_accumulate():
    assert check_accumulate(None) == 1 and check_accumulate(1) == 1 and check_accumulate(4) == 4 and check_accumulate(np.int64(3)) == 3
    assert check_accumulate(2.0) == 2 and type(check_accumulate(2.0)) is int             # a whole float is a count
    for bad in (0, -2, 1.5, "x", "4", True, False, float("nan"), float("inf"), [2], b"2"):
        with pytest.raises(VltfError, match="accumulate must be a whole number >= 1"):
            check_accumulate(bad)


# ---- the groups of an epoch ------------------------------------------------------------------------------------------------------
def test_accumulate_groups():
    assert accumulate_groups(10, 4, 0) == [(0, 3), (4, 7), (8, 9)]
    assert accumulate_groups(10, 4, 8) == [(8, 9)]
    assert accumulate_groups(10, 4, 4) == [(4, 7), (8, 9)]
    assert accumulate_groups(5, 1, 0) == [(i, i) for i in range(5)]
    assert accumulate_groups(5, 1, 3) == [(3, 3), (4, 4)]
    assert accumulate_groups(3, 8, 0) == [(0, 2)]                                         # k > num_batches: one group
    assert accumulate_groups(10, 4, 10) == []                                             # a finished epoch
    for start in (1, 2, 3, 5, 9):
        with pytest.raises(ValueError, match="does not begin a group"):
            accumulate_groups(10, 4, start)
    for args in ((10, 0, 0), (10, 4, -1), (10, 4, 11)):
        with pytest.raises(ValueError):
            accumulate_groups(*args)


# ---- the micro-step sequence of the engines --------------------------------------------------------------------------------------
def test_micro_sequence():
    m = MicroSequence(3)
    assert m.enter(None) is None and not m.open()
    assert m.enter((0, 3)) == (0, 3) and m.open() and m.enter((1, 3)) == (1, 3) and m.enter((2, 3)) == (2, 3) and not m.open()
    assert m.enter((0, 1)) == (0, 1) and not m.open()                                     # a group of one closes at once
    for first, bad in ((None, (1, 2)), ((0, 2), (0, 2)), ((0, 2), (1, 3)), (None, (0, 4)), ((0, 2), None), (None, (0, 0)),
                       (None, (-1, 2)), (None, (0.0, 2)), (None, (True, 2)), (None, 3), (None, (0, 2, 1))):
        if first is not None:
            m.enter(first)
        with pytest.raises(VltfError):
            m.enter(bad)
        assert not m.open()                                                               # a refusal abandons the group
        assert m.enter((0, 2)) == (0, 2) and m.enter((1, 2)) == (1, 2)                    # and the next (0, k) works
    assert m.add_rows(None, 7) == 7
    assert m.add_rows((0, 3), 4) == 4 and m.add_rows((1, 3), 4) == 8 and m.add_rows((2, 3), 1) == 9 and m.add_rows((0, 2), 2) == 2
    assert [MicroSequence.role(mi) for mi in (None, (0, 1), (0, 3), (1, 3), (2, 3), (1, 2))] == \
        [("single", 1), ("single", 1), ("first", 3), ("middle", 3), ("last", 3), ("last", 2)]


# ---- Train.run_step / do_train on a fake engine ------------------------------------------------------------------------------------
class FakeEngine:
    """Records every train call; returns what the engines return (no grad_norm before an update's last micro-step)."""
    dev, dp = torch.device("cpu"), None
    cfg = SimpleNamespace(classifier="lstm", fpc=3)
    early = late = False

    def __init__(self):
        self.calls, self.step_count = [], 0

    def train_step_u8(self, frames, onehot, lr, clip_norm, mean_bgr, crop_y, crop_x, mirror, global_rows=None, resize=None, micro=None):
        self.calls.append(dict(rows=int(onehot.shape[0]), lr=lr, global_rows=global_rows, micro=micro))
        out = dict(loss=1.0, accuracy=0.0, rows=int(onehot.shape[0]), loss_sum=1.0, correct=0.0)
        if micro is None or micro[0] == micro[1] - 1:
            self.step_count += 1
            out["grad_norm"] = 2.0
        return out


CPV = [1, 2, 1, 1, 2]            # clips per video; batch_size 2 -> batches of 3, 2 and 2 clips (the last one a single video)


class FakeFeeder:
    def __init__(self, save_interval):
        self.d = SimpleNamespace(batches=[2, 2, 1], clips_per_video=CPV, batch_size=2, batch_index=0)
        self.datasets = {defs.phase.train: [self.d]}
        self.save_interval, self.saved = save_interval, []

    def get_num_batches(self):
        return len(self.d.batches)

    def loop(self):
        return self.d.batch_index < len(self.d.batches)

    def get_batch_index(self):
        return self.d.batch_index

    def get_batch_sizes(self):
        return [self.d.batch_size]

    def rewind_datasets(self):
        self.d.batch_index = 0

    def get_feed_dict(self):
        v0 = self.d.batch_index * self.d.batch_size
        clips = sum(CPV[v0:v0 + self.d.batch_size])
        self.d.batch_index += 1
        n = clips * 3
        fd = dict(frames_u8=np.zeros((n, 4, 4, 3), np.uint8), crop_y=np.zeros(n, np.int32), crop_x=np.zeros(n, np.int32),
                  mirror=np.zeros(n, np.uint8), labels=np.zeros((clips, 4), np.int32), mean_bgr=None, resize=None, dataset=self.d,
                  batch_index=self.d.batch_index, global_clips=clips)
        return fd, [n], clips, 0

    def should_save(self, step):
        return step % self.save_interval == 0

    def save(self, engine, progress, global_step):
        self.saved.append((progress, global_step, engine.step_count))


def fake_settings(tmp_path, accumulate):
    train = SimpleNamespace(base_lr=0.1, lr_decay=[defs.decay.exp, defs.periodicity.interval, 1, 0.5], epochs=2, epoch_index=0,
                            clip_norm=0, accumulate=accumulate, batch_size=2)
    return SimpleNamespace(train=train, val=None, run_folder=str(tmp_path), run_id="fake", global_step=0, phase=defs.phase.train,
                           num_classes=4, graph_tags=None)


def test_group_plumbing(tmp_path):
    """accumulate 2 over batches of 3, 2 and 2 clips: groups (0, 1) and the short (2, 2).  Every call of a group carries the group's
    clips as global_rows; the update's lr is its last batch's; global_step counts batches; a save that falls inside a group waits."""
    from vltf_amd import run_task
    settings, feeder, eng = fake_settings(tmp_path, 2), FakeFeeder(save_interval=2), FakeEngine()
    train = Train(settings, feeder, eng)
    lrs = train.learning_rates
    assert len(lrs) == 6 and len(set(lrs)) == 6                                           # a table entry per BATCH, all different
    run_task.do_train(settings, train, feeder, eng)
    assert [c["micro"] for c in eng.calls] == [(0, 2), (1, 2), (0, 1)] * 2
    assert [c["global_rows"] for c in eng.calls] == [5, 5, 2] * 2                         # 3 + 2 clips, then the short group's 2
    assert [c["rows"] for c in eng.calls] == [3, 2, 2] * 2
    assert [c["lr"] for c in eng.calls] == [float(v) for v in lrs]                        # each call gets its batch's lr:
    assert [c["lr"] for c in eng.calls if c["micro"][0] == c["micro"][1] - 1] == [lrs[1], lrs[2], lrs[4], lrs[5]]   # the update's = the last's
    assert settings.global_step == train.global_step == 6 and eng.step_count == 4
    # should_save fires at batches 2, 4 and 6; batch 4 opens a group, so its save waits for batch 5; nothing is saved out of turn
    assert [(gs, upd) for _, gs, upd in feeder.saved] == [(2, 1), (5, 3), (6, 4)]
    assert [p for p, _, _ in feeder.saved] == ["ep_1_btch_2_gs_2", "ep_2_btch_2_gs_5", "ep_2_btch_3_gs_6"]


def test_accumulate_one_is_the_plain_loop(tmp_path):
    from vltf_amd import run_task
    settings, feeder, eng = fake_settings(tmp_path, 1), FakeFeeder(save_interval=2), FakeEngine()
    train = Train(settings, feeder, eng)
    run_task.do_train(settings, train, feeder, eng)
    assert all(c["micro"] is None and c["global_rows"] is None for c in eng.calls) and len(eng.calls) == 6
    assert [gs for _, gs, _ in feeder.saved] == [2, 4, 6] and eng.step_count == 6


def test_resume_inside_a_group_is_refused(tmp_path):
    settings, feeder, eng = fake_settings(tmp_path, 2), FakeFeeder(save_interval=2), FakeEngine()
    train = Train(settings, feeder, eng)
    feeder.d.batch_index = 1                                                              # a position no checkpoint of this run has
    with pytest.raises(Exception, match=r"train\.accumulate"):
        train.run_step(feeder.get_feed_dict()[0])


# ---- C ABI and example --------------------------------------------------------------------------------------------------------------
def test_abi_entries_are_declared():
    hdr = open(os.path.join(HERE, "..", "include", "vltf.h")).read()
    assert re.search(r"int vl_grad_accumulate\(float\* acc, float\* g, int64_t count, int mode,\s*const vl_lr_tier\* ranges, "
                     r"int n_ranges, vl_stream_t stream\);", hdr)
    assert re.search(r"int vl_step_state_set_micro\(vl_step_state\* state, int64_t update_step, int64_t draw_step, float lr, "
                     r"uint32_t tag_origin,\s*vl_stream_t stream\);", hdr)
    assert len(_ffi.SIGNATURES["vl_grad_accumulate"][1]) == 7 and len(_ffi.SIGNATURES["vl_step_state_set_micro"][1]) == 6


def test_example_config():
    with open(os.path.join(HERE, "..", "examples", "lrcn_accumulate.yml")) as f:
        t = yaml.safe_load(f)["run"]["train"]
    assert t["batch_size"] == 16 and t["accumulate"] == 4 and t["momentum"] == 0.9 and t["weight_decay"] == 0.0005
    assert check_accumulate(t["accumulate"]) == 4
