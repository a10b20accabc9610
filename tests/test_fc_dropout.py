"""Dropout on relu(fc6) / relu(fc7) of the AlexNet tower (train.fc_dropout_keep_prob), host side: the YAML key, its check, the
example, the statistics of the mask definition (on the numpy restatement tests/fc_dropout_ref.py -- the device only has to equal it,
tests/test_fc_dropout_gpu.py), and the graph engine's host logic with the option off."""
import math
import os

import numpy as np
import pytest
import torch
import yaml

from tests import fc_dropout_ref as R
from tests import graph_cases as GC
from tests.test_finetune import _settings
from vltf_amd.defs_ import defs
from vltf_amd._ffi import VltfError
from vltf_amd.engine import NetConfig, check_fc_dropout, dropout_seed, fc_dropout_salt

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- settings ------------------------------------------------------------------------------------------------------------------
def test_settings_key_parses(tmp_path):
    s = _settings(tmp_path, train={"fc_dropout_keep_prob": 0.5})
    assert s.train.fc_dropout_keep_prob == 0.5 and isinstance(s.train.fc_dropout_keep_prob, float)
    assert s.get_fc_dropout() == 0.5
    assert _settings(tmp_path, train={"fc_dropout_keep_prob": "0.25"}).train.fc_dropout_keep_prob == 0.25
    assert _settings(tmp_path, train={"fc_dropout_keep_prob": 1}).train.fc_dropout_keep_prob == 1.0
    assert _settings(tmp_path, train={"fc_dropout_keep_prob": 0}).get_fc_dropout() == 0.0


@pytest.mark.parametrize("train", [{}, {"fc_dropout_keep_prob": None}, {"fc_dropout_keep_prob": "None"}], ids=["absent", "null", "None-string"])
def test_settings_absent_key_changes_nothing(tmp_path, train):
    s, base = _settings(tmp_path, train=train), _settings(tmp_path)
    assert s.train.fc_dropout_keep_prob == 0.0 and s.get_fc_dropout() == 0.0
    assert vars(s.train) == vars(base.train)
    assert NetConfig().fc_dropout_keep_prob == 0.0


@pytest.mark.parametrize("bad", [-0.1, 1.5, "nan", "much", float("inf"), True], ids=["negative", "above-1", "nan-string", "string", "inf", "bool"])
def test_settings_refusals(tmp_path, bad):
    with pytest.raises(Exception, match=r"train\.fc_dropout_keep_prob: fc_dropout_keep_prob must be a number in \[0, 1\]"):
        _settings(tmp_path, train={"fc_dropout_keep_prob": bad})


def test_get_fc_dropout_is_zero_outside_the_train_phase(tmp_path):
    s = _settings(tmp_path, train={"fc_dropout_keep_prob": 0.5})
    assert s.get_fc_dropout() == 0.5
    s.phase = defs.phase.val                              # a val run of the same file: nothing is dropped
    assert s.get_fc_dropout() == 0.0 and s.get_dropout() == 0.0


def test_check_fc_dropout():
    assert check_fc_dropout(None) == 0.0 and check_fc_dropout(0) == 0.0 and check_fc_dropout(0.5) == 0.5 and check_fc_dropout(1) == 1.0
    assert check_fc_dropout(np.float32(0.25)) == 0.25 and isinstance(check_fc_dropout(1), float)
    for bad in (-0.1, -1e-9, 1.0000001, 1.5, float("nan"), float("inf"), -float("inf"), "0.5", "much", b"1", True, [0.5], {}):
        with pytest.raises(VltfError, match=r"fc_dropout_keep_prob must be a number in \[0, 1\]"):
            check_fc_dropout(bad)


def test_seed_and_salts():
    """The seed is the head dropout's; fc6 / fc7 of a tower and the towers of a graph all get different salts."""
    assert dropout_seed(0) == 0x5DEECE66D and dropout_seed(3) == (3 << 20) ^ 0x5DEECE66D
    salts = [fc_dropout_salt(NetConfig(fc_dropout_salt=t), l) for t in range(4) for l in ("fc6", "fc7")]
    assert len(set(salts)) == len(salts) and all(0 <= s < 2 ** 32 for s in salts)


def test_example_yaml_is_the_finetune_one_plus_the_key():
    here = os.path.join(HERE, "..", "examples")
    with open(os.path.join(here, "lrcn_fc_dropout.yml")) as f:
        drop = yaml.safe_load(f)
    with open(os.path.join(here, "lrcn_finetune.yml")) as f:
        fin = yaml.safe_load(f)
    assert drop["run"]["train"].pop("fc_dropout_keep_prob") == 0.5
    assert drop["run"]["run_folder"] != fin["run"]["run_folder"] and drop["run"]["run_id"] != fin["run"]["run_id"]
    for cfg in (drop, fin):                                   # each run keeps its own folder and id
        cfg["run"].pop("run_folder"), cfg["run"].pop("run_id")
    assert drop == fin


# ---- statistics of the mask definition (fixed seeds and salts: the outcome is a constant of the definition) -----------------------
N = 1 << 20
SEED_A, SEED_B = dropout_seed(0), dropout_seed(1)            # two consecutive steps of a run
SALT_A, SALT_B = 0, 1                                         # fc6 and fc7 of one tower


@pytest.mark.parametrize("keep", [0.25, 0.5, 0.9])
def test_kept_fraction(keep):
    frac = R.keep_mask(SEED_A, SALT_A, N, keep).mean()
    assert abs(frac - keep) <= 4 * math.sqrt(keep * (1 - keep) / N), frac


@pytest.mark.parametrize("keep", [0.25, 0.5, 0.9])
@pytest.mark.parametrize("other", [(SEED_A, SALT_B), (SEED_B, SALT_A)], ids=["two-salts", "two-seeds"])
def test_streams_are_independent(keep, other):
    """Two salts (or two seeds) agree on an element with probability keep^2 + (1 - keep)^2 when their draws are independent."""
    a, b = R.keep_mask(SEED_A, SALT_A, N, keep), R.keep_mask(other[0], other[1], N, keep)
    q = keep ** 2 + (1 - keep) ** 2
    agree = (a == b).mean()
    assert abs(agree - q) <= 4 * math.sqrt(q * (1 - q) / N), agree


def test_mask_is_a_function_of_the_element_index_alone():
    """A longer range begins with the shorter one's mask, and keep only moves the threshold: every element kept at 0.25 is kept at 0.5."""
    a, b = R.keep_mask(SEED_A, 5, 1000, 0.5), R.keep_mask(SEED_A, 5, 4099, 0.5)
    assert np.array_equal(a, b[:1000])
    assert not (R.keep_mask(SEED_A, 5, 4099, 0.25) & ~b).any()


# ---- GraphEngine host logic with the option off: the CPU double has none of the new ops ---------------------------------------------
def test_cpu_graph_engine_plans_and_steps_with_the_option_off(monkeypatch):
    from tests.cpu_double import install
    Engine = install(monkeypatch)
    case = GC.CASES["two_stream_avg"]()
    pipes, ds = GC.specs_and_datasets(case)
    eng = Engine(pipes, ds, case["V"], device="cpu", fc_dropout_keep_prob=0.0)
    assert eng.fc_dropout_keep_prob == 0.0
    towers = [nd.tower_cfg for nd in eng.nodes if nd.tower is not None]
    assert [c.fc_dropout_keep_prob for c in towers] == [0.0, 0.0] and len({c.fc_dropout_salt for c in towers}) == 2
    p = eng.init_params(seed=case["seed"], well_scaled=True)
    eng.load_params(p)
    raw, feeds = GC.inputs(case)
    logits, onehot, loss, _, _ = GC.expect(case, p, feeds)
    dev_feeds = {t: dict(frames_u8=torch.from_numpy(v), mean_bgr=GC.MEAN) for t, v in raw.items()}
    out = eng.train_step(dev_feeds, torch.from_numpy(onehot), lr=0.01, clip_norm=0.5)
    assert abs(out["loss"] - loss) < 1e-4 * max(1, abs(loss))
    with pytest.raises(VltfError, match="fc_dropout_keep_prob"):
        Engine(pipes, ds, case["V"], device="cpu", fc_dropout_keep_prob=1.5)
