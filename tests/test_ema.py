"""Exponential moving average of the weights on the host: check_ema, the rate function every launch takes its rate from, the
`train: ema_decay / ema_warmup` and `val: use_ema` keys with their refusals, the example, and the layout of vl_step_state (header, ctypes
record and library agree; the fields of before keep their offsets).  No GPU: no engine is constructed."""
import ctypes
import os
import re

import numpy as np
import pytest
import yaml

from tests.test_finetune import _settings
from tests.test_host_workflow import config, make_dataset
from vltf_amd import settings_
from vltf_amd._ffi import VltfError
from vltf_amd.engine import NetConfig, check_ema, ema_rate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- check_ema -------------------------------------------------------------------------------------------------------------------------
def test_check_ema_accepts():
    assert check_ema(None, None) == (0.0, False) and check_ema(0, False) == (0.0, False) and check_ema(0.0, None) == (0.0, False)
    assert check_ema(0.999, True) == (0.999, True) and check_ema(0.9, False) == (0.9, False) and check_ema(0.5, None) == (0.5, False)
    assert check_ema(np.float32(0.5), np.bool_(True)) == (0.5, True)
    assert NetConfig().ema_decay == 0.0 and NetConfig().ema_warmup is False


@pytest.mark.parametrize("decay,warmup", [(1.0, False), (-0.1, False), (1.5, False), (float("nan"), False), (float("inf"), False),
                                          (0.0, True), (None, True), ("0.9", False), (True, False), (0.9, "yes"), (0.9, 1)])
def test_check_ema_refuses(decay, warmup):
    with pytest.raises(VltfError, match="ema"):
        check_ema(decay, warmup)


# ---- the rate function -------------------------------------------------------------------------------------------------------------------
def test_rate_without_warmup_is_one_minus_decay():
    for decay in (0.9, 0.99, 0.999, 0.9999, 0.5):
        for n in (0, 1, 10, 10 ** 6):
            r = ema_rate(decay, False, n)
            assert isinstance(r, float) and r == float(np.float32(1.0 - decay))


def test_rate_with_warmup():
    assert ema_rate(0.999, True, 0) == float(np.float32(0.9))                     # TF: min(decay, 1 / 10) at the first update
    assert ema_rate(0.999, True, 5) == float(np.float32(9.0 / 15.0))
    # 9 / (10 + n) = 1 - decay at n = 9 / (1 - decay) - 10: the warm-up branch before it, the constant from it on
    for decay, cross in ((0.9, 80), (0.99, 890), (0.999, 8990)):
        floor = float(np.float32(1.0 - decay))
        assert ema_rate(decay, True, cross - 1) == float(np.float32(9.0 / (9.0 + cross))) > floor
        for n in (cross, cross + 1, 10 * cross, 10 ** 9):
            assert ema_rate(decay, True, n) == floor
        rates = [ema_rate(decay, True, n) for n in range(0, cross + 50)]
        assert min(rates) == floor and all(a >= b for a, b in zip(rates, rates[1:]))      # never below 1 - decay, never rising
        assert all(0.0 < r <= 1.0 for r in rates)


def test_rate_equals_tf_decay_rule():
    """TF: decay_n = min(decay, (1 + n) / (10 + n)); the rate is 1 - decay_n, computed without the cancellation."""
    for decay in (0.9, 0.999, 0.9999):
        for n in (0, 1, 7, 100, 5000, 10 ** 5):
            want = 1.0 - min(decay, (1.0 + n) / (10.0 + n))
            assert abs(ema_rate(decay, True, n) - want) <= 2.0 ** -23 * want


# ---- YAML ----------------------------------------------------------------------------------------------------------------------------
def test_settings_train_keys_parse(tmp_path):
    s = _settings(tmp_path, train={"ema_decay": 0.999, "ema_warmup": True})
    assert s.train.ema_decay == 0.999 and isinstance(s.train.ema_decay, float) and s.train.ema_warmup is True
    assert s.get_ema() == (0.999, True)
    s = _settings(tmp_path, train={"ema_decay": "0.9"})
    assert s.train.ema_decay == 0.9 and s.train.ema_warmup is False
    s = _settings(tmp_path, train={"ema_decay": 0, "ema_warmup": False})
    assert s.get_ema() == (0.0, False)


@pytest.mark.parametrize("train", [{}, {"ema_decay": None}, {"ema_decay": "None", "ema_warmup": "None"}, {"ema_warmup": None}],
                         ids=["absent", "null", "None-strings", "warmup-null"])
def test_settings_absent_keys_mean_off(tmp_path, train):
    s = _settings(tmp_path, train=train)
    assert s.train.ema_decay == 0.0 and s.train.ema_warmup is False and s.get_ema() == (0.0, False)


@pytest.mark.parametrize("train", [{"ema_decay": 1.0}, {"ema_decay": -0.1}, {"ema_decay": "nan"}, {"ema_decay": "much"},
                                   {"ema_decay": True}, {"ema_warmup": True}, {"ema_decay": 0.0, "ema_warmup": True},
                                   {"ema_decay": 0.9, "ema_warmup": "yes"}])
def test_settings_train_refusals(tmp_path, train):
    with pytest.raises(Exception, match="ema"):
        _settings(tmp_path, train=train)


def _val_settings(tmp_path, val=None, train=None):
    folder = str(tmp_path)
    data_path, _, _ = make_dataset(folder, "val.txt")
    path = config(folder, data_path, phase="val")
    with open(path) as f:
        cfg = yaml.safe_load(f)
    cfg["run"]["val"].update(val or {})
    cfg["run"]["train"].update(train or {})
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    s = settings_.Settings()
    s.initialize(path)
    return s


def test_settings_val_use_ema(tmp_path):
    assert _val_settings(tmp_path, {"use_ema": True}).val.use_ema is True
    for val in ({}, {"use_ema": False}, {"use_ema": None}, {"use_ema": "None"}):
        assert _val_settings(tmp_path, val).val.use_ema is False
    # a validation run keeps no shadow of its own, whatever the train section says
    assert _val_settings(tmp_path, {"use_ema": True}, train={"ema_decay": 0.9}).get_ema() == (0.0, False)
    for bad in ("yes", 1, 0.5):
        with pytest.raises(Exception, match="use_ema"):
            _val_settings(tmp_path, {"use_ema": bad})


def test_example_yaml_is_the_finetune_one_with_the_two_keys(tmp_path):
    here = os.path.join(ROOT, "examples")
    with open(os.path.join(here, "lrcn_ema.yml")) as f:
        ema = yaml.safe_load(f)
    with open(os.path.join(here, "lrcn_finetune.yml")) as f:
        fin = yaml.safe_load(f)
    assert ema["run"]["train"].pop("ema_decay") == 0.999 and ema["run"]["train"].pop("ema_warmup") is True
    for cfg in (ema, fin):                                    # each run keeps its own folder and id
        cfg["run"].pop("run_folder", None), cfg["run"].pop("run_id", None)
    assert ema == fin
    # and its train section loads through the settings
    with open(os.path.join(here, "lrcn_ema.yml")) as f:
        keys = yaml.safe_load(f)["run"]["train"]
    s = _settings(tmp_path, train={k: keys[k] for k in ("ema_decay", "ema_warmup", "lr_mult")}, pipeline={"train_from": "fc6"})
    assert s.get_ema() == (0.999, True)


# ---- vl_step_state: header, ctypes record, library -----------------------------------------------------------------------------------------
def header_step_state():
    """[(type, name, array length or None)] of the struct's fields, from the header text."""
    src = open(os.path.join(ROOT, "include", "vltf.h")).read()
    body = re.search(r"typedef struct vl_step_state \{(.*?)\} vl_step_state;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            m = re.fullmatch(r"(\w+)\s+(\w+)(?:\[(\d+)\])?", decl)
            assert m, decl
            out.append((m.group(1), m.group(2), int(m.group(3)) if m.group(3) else None))
    return out


def test_step_state_layout():
    from vltf_amd import _ffi
    ctype = {"int64_t": ctypes.c_int64, "float": ctypes.c_float, "uint32_t": ctypes.c_uint32}
    fields = header_step_state()
    assert [f[1] for f in fields] == ["step", "lr", "tag_origin", "adam_lr", "ema_rate", "reserved"]

    class FromHeader(ctypes.Structure):
        _fields_ = [(name, ctype[t] * n if n else ctype[t]) for t, name, n in fields]

    S = _ffi.StepState
    assert [(n, ctypes.sizeof(t)) for n, t in FromHeader._fields_] == [(n, ctypes.sizeof(t)) for n, t in S._fields_]
    assert ctypes.sizeof(FromHeader) == ctypes.sizeof(S) == 32
    # the fields of before the average keep their places; the rate took the first reserved word
    assert (S.step.offset, S.lr.offset, S.tag_origin.offset, S.adam_lr.offset) == (0, 8, 12, 16)
    assert S.ema_rate.offset == 20 and S.reserved.offset == 24 and S.reserved.size == 8
    for name in ("step", "lr", "tag_origin", "adam_lr", "ema_rate", "reserved"):
        assert getattr(FromHeader, name).offset == getattr(S, name).offset, name
    assert int(_ffi.lib().vl_step_state_bytes()) == 32


def test_ffi_table_has_the_entry_points():
    from vltf_amd import _ffi
    p, i32, i64, f32 = _ffi.p, _ffi.i32, _ffi.i64, _ffi.f32
    assert _ffi.SIGNATURES["vl_ema_update"] == (i32, [p, p, i64, f32, p, p, i32, p])
    assert _ffi.SIGNATURES["vl_ema_update_st"] == (i32, [p, p, i64, p, p, p, i32, p])
    assert _ffi.SIGNATURES["vl_step_state_set_ema"] == (i32, [p, f32, p])
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vltf.h")).read(), flags=re.S)
    for name in ("vl_ema_update", "vl_ema_update_st", "vl_step_state_set_ema"):
        m = re.search(r"\bint %s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
        assert m and m.group(1).count(",") + 1 == len(_ffi.SIGNATURES[name][1]), name
        assert hasattr(_ffi.lib(), name)
    # the setters of before are declared as they were
    assert "int vl_step_state_set(vl_step_state* state, int64_t step, float lr, uint32_t tag_origin, vl_stream_t stream);" in src
    assert _ffi.SIGNATURES["vl_step_state_set"] == (i32, [p, i64, f32, _ffi.u32, p])
    assert _ffi.SIGNATURES["vl_step_state_set_micro"] == (i32, [p, i64, i64, f32, _ffi.u32, p])
