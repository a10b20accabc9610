"""SGD with momentum on the host: the `momentum` / `nesterov` keys of the `train:` section, their refusals, and the refusal of an
optimizer name that has no update (rmsprop).  No GPU: no engine is constructed."""
import pytest

from tests.test_finetune import _settings
from vltf_amd._ffi import VltfError
from vltf_amd.engine import NetConfig, check_momentum

TODAY = ("batch_size", "epochs", "epoch_index", "optimizer", "base_lr", "lr_mult", "lr_decay", "clip_norm", "dropout_keep_prob")


def test_settings_momentum_parses(tmp_path):
    s = _settings(tmp_path, train={"momentum": 0.9})
    assert s.train.momentum == 0.9 and isinstance(s.train.momentum, float) and s.train.nesterov is False
    s = _settings(tmp_path, train={"momentum": "0.5", "nesterov": True})
    assert s.train.momentum == 0.5 and s.train.nesterov is True
    s = _settings(tmp_path, train={"momentum": 0, "nesterov": False})
    assert s.train.momentum == 0.0 and s.train.nesterov is False


@pytest.mark.parametrize("train", [{}, {"momentum": None}, {"momentum": "None", "nesterov": "None"}, {"nesterov": None}],
                         ids=["absent", "null", "None-strings", "nesterov-null"])
def test_settings_absent_keys_change_nothing(tmp_path, train):
    """Without the keys the train settings are the ones read before there was momentum, and the engine gets plain SGD."""
    s = _settings(tmp_path, train=train)
    assert s.train.momentum == 0.0 and s.train.nesterov is False
    base = _settings(tmp_path)
    assert {k: getattr(s.train, k) for k in TODAY} == {k: getattr(base.train, k) for k in TODAY}
    assert sorted(k for k in vars(s.train)) == sorted(k for k in vars(base.train))
    assert NetConfig().momentum == 0.0 and NetConfig().nesterov is False


@pytest.mark.parametrize("train,msg", [
    ({"momentum": 1.0}, r"\[0, 1\)"), ({"momentum": -0.1}, r"\[0, 1\)"), ({"momentum": 1.5}, r"\[0, 1\)"), ({"momentum": "nan"}, r"\[0, 1\)"),
    ({"momentum": "much"}, "momentum"),
    ({"nesterov": True}, "nesterov needs momentum"), ({"momentum": 0.0, "nesterov": True}, "nesterov needs momentum"),
    ({"nesterov": "yes"}, "boolean"),
    ({"optimizer": "defs.optim.adam", "momentum": 0.9}, "adam"), ({"optimizer": "defs.optim.adam", "nesterov": True}, "nesterov|adam"),
    ({"optimizer": "defs.optim.adam", "momentum": 0.9, "nesterov": True}, "adam"),
    ({"optimizer": "defs.optim.rmsprop"}, "Undefined optimizer rmsprop"),
])
def test_settings_refusals(tmp_path, train, msg):
    with pytest.raises(Exception, match=msg):
        _settings(tmp_path, train=train)


def test_settings_adam_without_momentum_still_parses(tmp_path):
    s = _settings(tmp_path, train={"optimizer": "defs.optim.adam"})
    assert s.train.optimizer == "adam" and s.train.momentum == 0.0 and s.train.nesterov is False


def test_check_momentum():
    assert check_momentum("sgd", None, None) == (0.0, False) and check_momentum("adam", 0.0, False) == (0.0, False)
    assert check_momentum("sgd", 0.9, True) == (0.9, True)
    for opt, m, n in (("sgd", 1.0, False), ("sgd", -0.5, False), ("sgd", float("nan"), False), ("sgd", 0.0, True), ("adam", 0.9, False),
                      ("adam", 0.0, True)):
        with pytest.raises(VltfError):
            check_momentum(opt, m, n)


def test_example_yaml_is_the_finetune_one_with_momentum():
    import os
    import yaml
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples")
    with open(os.path.join(here, "lrcn_momentum.yml")) as f:
        mom = yaml.safe_load(f)
    with open(os.path.join(here, "lrcn_finetune.yml")) as f:
        fin = yaml.safe_load(f)
    assert mom["run"]["train"].pop("momentum") == 0.9
    mom["run"]["train"].pop("nesterov", None)
    for cfg in (mom, fin):                                    # each run keeps its own folder and id
        cfg["run"].pop("run_folder", None), cfg["run"].pop("run_id", None)
    assert mom == fin
