"""LARS on the host: check_lars, the `train: lars_eeta / lars_epsilon` keys with their refusals, the range table of the update against
tests/lars_ref.py, the trust formula's corner cases, the example, and the C-ABI table (header, ctypes record and library agree).  No
GPU: no engine is constructed."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import yaml

from tests import lars_ref
from tests.test_finetune import _settings
from vltf_amd._ffi import VltfError
from vltf_amd.engine import NetConfig, check_lars, finetune_plan, lars_ranges, param_specs, stat_segments, tier_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- check_lars ------------------------------------------------------------------------------------------------------------------------
def test_check_lars_accepts():
    for eeta, eps in ((None, None), (0, 0), (0.0, None), (None, 0.0)):
        assert check_lars("sgd", 0.0, eeta, eps) == (0.0, 0.0)
        assert check_lars("adam", 0.0, eeta, eps) == (0.0, 0.0)           # off: no demand on the optimizer
    assert check_lars("sgd", 0.9, 0.001, None) == (0.001, 0.0)
    assert check_lars("sgd", 0.9, 0.001, 1e-9) == (0.001, 1e-9)
    assert check_lars("sgd", 0.5, np.float32(0.5), np.float64(0.25)) == (0.5, 0.25)
    assert check_lars("sgd", 0.9, 1, 0) == (1.0, 0.0)
    assert NetConfig().lars_eeta == 0.0 and NetConfig().lars_epsilon == 0.0


@pytest.mark.parametrize("eeta,eps", [(-0.001, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), ("0.001", 0.0), (True, 0.0),
                                      (0.001, -1e-9), (0.001, float("nan")), (0.001, float("inf")), (0.001, "0"), (0.001, False),
                                      (0.0, 1e-9), (None, 1e-9)])
def test_check_lars_refuses_values(eeta, eps):
    with pytest.raises(VltfError, match="lars"):
        check_lars("sgd", 0.9, eeta, eps)


def test_check_lars_refuses_adam_and_no_momentum():
    with pytest.raises(VltfError, match="adam"):
        check_lars("adam", 0.0, 0.001, 0.0)
    for m in (0.0, None):
        with pytest.raises(VltfError, match="momentum"):
            check_lars("sgd", m, 0.001, 0.0)


# ---- YAML ------------------------------------------------------------------------------------------------------------------------------
def test_settings_keys_parse(tmp_path):
    s = _settings(tmp_path, train={"momentum": 0.9, "lars_eeta": 0.001, "lars_epsilon": 1e-9})
    assert s.train.lars_eeta == 0.001 and s.train.lars_epsilon == 1e-9 and s.get_lars() == (0.001, 1e-9)
    assert isinstance(s.train.lars_eeta, float) and isinstance(s.train.lars_epsilon, float)
    s = _settings(tmp_path, train={"momentum": 0.9, "lars_eeta": "1e-3"})       # YAML reads 1e-3 as a string
    assert s.get_lars() == (0.001, 0.0)
    s = _settings(tmp_path, train={"momentum": 0.9, "nesterov": True, "lars_eeta": 0.02, "lars_epsilon": 0})
    assert s.get_lars() == (0.02, 0.0) and s.train.nesterov is True


@pytest.mark.parametrize("train", [{}, {"lars_eeta": None}, {"lars_eeta": "None", "lars_epsilon": "None"}, {"lars_epsilon": None},
                                   {"lars_eeta": 0, "lars_epsilon": 0.0}, {"momentum": 0.9}],
                         ids=["absent", "null", "None-strings", "epsilon-null", "zeros", "momentum-only"])
def test_settings_absent_keys_mean_off(tmp_path, train):
    s = _settings(tmp_path, train=train)
    assert s.train.lars_eeta == 0.0 and s.train.lars_epsilon == 0.0 and s.get_lars() == (0.0, 0.0)


@pytest.mark.parametrize("train", [{"momentum": 0.9, "lars_eeta": -0.001}, {"momentum": 0.9, "lars_eeta": "nan"},
                                   {"momentum": 0.9, "lars_eeta": "inf"}, {"momentum": 0.9, "lars_eeta": "much"},
                                   {"momentum": 0.9, "lars_eeta": True}, {"momentum": 0.9, "lars_eeta": 0.001, "lars_epsilon": -1.0},
                                   {"momentum": 0.9, "lars_eeta": 0.001, "lars_epsilon": "nan"}, {"momentum": 0.9, "lars_epsilon": 1e-9},
                                   {"lars_eeta": 0.001}, {"momentum": 0, "lars_eeta": 0.001},
                                   {"optimizer": "defs.optim.adam", "lars_eeta": 0.001}])
def test_settings_refusals(tmp_path, train):
    with pytest.raises(Exception, match="lars"):
        _settings(tmp_path, train=train)


def test_settings_outside_the_train_phase_is_off(tmp_path):
    from tests.test_ema import _val_settings
    assert _val_settings(tmp_path, train={"momentum": 0.9, "lars_eeta": 0.001}).get_lars() == (0.0, 0.0)


def test_example_yaml_is_the_momentum_one_with_the_two_keys(tmp_path):
    here = os.path.join(ROOT, "examples")
    with open(os.path.join(here, "lrcn_lars.yml")) as f:
        lars = yaml.safe_load(f)
    with open(os.path.join(here, "lrcn_momentum.yml")) as f:
        mom = yaml.safe_load(f)
    assert lars["run"]["train"].pop("lars_eeta") == 0.001 and lars["run"]["train"].pop("lars_epsilon") == 0.0
    for cfg in (lars, mom):
        cfg["run"].pop("run_folder", None), cfg["run"].pop("run_id", None)
    assert lars == mom
    with open(os.path.join(here, "lrcn_lars.yml")) as f:
        keys = yaml.safe_load(f)["run"]["train"]
    s = _settings(tmp_path, train={k: keys[k] for k in ("momentum", "lars_eeta", "lars_epsilon", "lr_mult")}, pipeline={"train_from": "fc6"})
    assert s.get_lars() == (0.001, 0.0)


# ---- the range table -----------------------------------------------------------------------------------------------------------------
SPECS = [("head/W", (6, 4)), ("head/b", (4,)), ("dcnn/fc7W", (5, 3)), ("dcnn/fc7b", (3,)), ("dcnn/fc6W", (7, 5)), ("dcnn/fc6b", (5,)),
         ("dcnn/conv5W", (3, 3, 2, 2)), ("dcnn/conv5b", (2,)), ("dcnn/conv4W", (3, 3, 2, 2)), ("dcnn/conv4b", (2,))]


def test_range_table_small_spec_list_with_a_frozen_layer():
    """conv5 frozen, lr_mult 4 on the head: biases carry -1, the frozen layer is absent from ranges and segments, the trust indices of
    the weight tensors count from 0 without a hole, and the table equals the reference's restatement."""
    total = sum(int(np.prod(s)) for _, s in SPECS)
    plan = tier_plan(SPECS, {"dcnn/conv5W", "dcnn/conv5b"}, 4.0, [(0, total)])
    ranges, segs, decays = lars_ranges(SPECS, plan, 0.0005)
    assert (ranges, segs, decays) == lars_ref.ranges(SPECS, plan.tiers, 0.0005)
    assert ranges == [(0, 24, 4.0, 0), (24, 28, 4.0, -1), (28, 43, 1.0, 1), (43, 46, 1.0, -1), (46, 81, 1.0, 2), (81, 86, 1.0, -1),
                      (124, 160, 1.0, 3), (160, 162, 1.0, -1)]
    assert [s[0] for s in segs] == ["head/W", "dcnn/fc7W", "dcnn/fc6W", "dcnn/conv4W"] and decays == [0.0005] * 4
    assert [r[3] for r in ranges if r[3] >= 0] == list(range(len(segs)))
    assert [(r[0], r[1]) for r in ranges if r[3] >= 0] == [(s[1], s[2]) for s in segs]
    assert not any(lo < 124 and hi > 86 for lo, hi, _, _ in ranges)                   # nothing touches the frozen extent [86, 124)
    assert lars_ranges(SPECS, plan, 0.0)[2] == [0.0] * 4                              # weight decay off: the coefficient is 0


def test_adjacent_biases_of_one_factor_merge_and_of_two_do_not():
    specs = [("a/W", (2, 2)), ("a/b", (2,)), ("a/c", (3,)), ("dcnn/fc6b", (4,)), ("dcnn/fc6W", (2, 3))]
    plan = tier_plan(specs, (), 2.0, [(0, 19)])
    ranges, segs, _ = lars_ranges(specs, plan, 0.0)
    assert ranges == [(0, 4, 2.0, 0), (4, 9, 2.0, -1), (9, 13, 1.0, -1), (13, 19, 1.0, 1)] == lars_ref.ranges(specs, plan.tiers)[0]
    assert [s[0] for s in segs] == ["a/W", "dcnn/fc6W"]


@pytest.mark.parametrize("train_from", [None, "fc6"])
def test_range_table_of_the_lrcn(train_from):
    cfg = NetConfig(image_shape=(67, 67, 3), num_classes=7, fpc=3, lstm_hidden=8, train_from=train_from, lr_mult=10.0)
    specs, plan = param_specs(cfg), finetune_plan(cfg)
    ranges, segs, decays = lars_ranges(specs, plan, 0.001)
    assert (ranges, segs, decays) == lars_ref.ranges(specs, plan.tiers, 0.001)
    shapes = dict(specs)
    trained = [n for n, _, _ in stat_segments(specs, plan)]
    assert [s[0] for s in segs] == [n for n in trained if len(shapes[n]) >= 2] and len(segs) < len(trained)
    assert sum(hi - lo for lo, hi, _, _ in ranges) == sum(hi - lo for lo, hi, _ in plan.tiers)      # every trained element, once
    assert all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:]))
    assert not any(n in plan.frozen for n, _, _ in segs)
    if train_from:
        assert plan.frozen and {m for _, _, m, _ in ranges} == {1.0, 10.0}


# ---- the trust formula of the reference ---------------------------------------------------------------------------------------------------
def test_reference_trust_formula():
    w, g = np.array([3.0, 4.0]), np.array([0.6, 0.8])
    assert lars_ref.trust(w, g, 0.001) == pytest.approx(0.005, rel=1e-15)
    assert lars_ref.trust(w, g, 0.001, eps=1.0) == pytest.approx(0.001 * 5 / 2.0, rel=1e-15)
    assert lars_ref.trust(w, g, 0.001, decay=0.5, sc=0.5) == pytest.approx(0.001 * 5 / (0.5 + 2.5), rel=1e-15)
    assert lars_ref.trust(np.zeros(2), g, 0.001) == 1.0 and lars_ref.trust(w, np.zeros(2), 0.001) == 1.0
    assert lars_ref.trust(w, np.array([np.nan, 1.0]), 0.001) == 1.0 and lars_ref.trust(np.array([np.inf, 1.0]), g, 0.001) == 1.0
    assert lars_ref.clip_scale_f32(0.0, 4.0) == 1.0 and lars_ref.clip_scale_f32(0.0, 4.0, 0.125) == 0.125
    assert lars_ref.clip_scale_f32(1.0, 16.0) == 0.25 and lars_ref.clip_scale_f32(8.0, 16.0) == 1.0
    assert lars_ref.clip_scale_f32(0.25, 16.0, 0.125) == np.float32(0.125 * 0.25 / 0.5)
    assert lars_ref.lr_k(0.01, 4.0, 1.0) == np.float32(np.float32(0.01) * np.float32(4.0))


# ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------
def test_ffi_table_and_range_record():
    from vltf_amd import _ffi
    p, i32, i64, f32, f64 = _ffi.p, _ffi.i32, _ffi.i64, _ffi.f32, ctypes.c_double
    assert _ffi.SIGNATURES["vl_lars_trust"] == (i32, [p, i32, f64, f64, p, f32, p, f32, p, p])
    assert _ffi.SIGNATURES["vl_lars_apply"] == (i32, [p, p, p, i64, f32, f32, i32, f32, p, f32, p, p, i32, p, i32, p])
    assert _ffi.SIGNATURES["vl_lars_apply_st"] == (i32, [p, p, p, i64, p, f32, i32, f32, p, f32, p, p, i32, p, i32, p])
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vltf.h")).read(), flags=re.S)
    for name in ("vl_lars_trust", "vl_lars_apply", "vl_lars_apply_st"):
        m = re.search(r"\bint %s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
        assert m and m.group(1).count(",") + 1 == len(_ffi.SIGNATURES[name][1]), name
        assert hasattr(_ffi.lib(), name)
    body = re.search(r"typedef struct vl_lars_range \{(.*?)\} vl_lars_range;", src, flags=re.S).group(1)
    assert [d.strip() for d in body.split(";") if d.strip()] == ["int64_t begin, end", "float lr_mult", "int32_t trust_index"]
    R = _ffi.LarsRange
    assert [n for n, _ in R._fields_] == ["begin", "end", "lr_mult", "trust_index"] and ctypes.sizeof(R) == 24
    assert (R.begin.offset, R.end.offset, R.lr_mult.offset, R.trust_index.offset) == (0, 8, 16, 20)
    # the momentum entry points LARS stands beside are declared as they were
    assert _ffi.SIGNATURES["vl_momentum_apply"] == (i32, [p, p, p, i64, f32, f32, i32, f32, p, f32, p, p, i32, p])


def test_host_refusals_need_no_device():
    """The C entry points validate before they launch: null pointers, counts, eeta / eps / decay, the table.  Nothing runs."""
    from vltf_amd import _ffi
    lib = _ffi.lib()
    one = (_ffi.f32 * 1)(0.0)
    fake = 4096                                  # a non-null, aligned address: validation fails before anything dereferences it
    bad = [(None, 1, 0.001, 0.0, one, fake), (fake, 1, 0.001, 0.0, None, fake), (fake, 1, 0.001, 0.0, one, None),
           (fake, 0, 0.001, 0.0, one, fake), (fake, 65, 0.001, 0.0, (_ffi.f32 * 65)(), fake),
           (fake, 1, 0.0, 0.0, one, fake), (fake, 1, -1.0, 0.0, one, fake), (fake, 1, math.nan, 0.0, one, fake),
           (fake, 1, math.inf, 0.0, one, fake), (fake, 1, 0.001, -1.0, one, fake), (fake, 1, 0.001, math.nan, one, fake),
           (fake, 1, 0.001, math.inf, one, fake), (fake, 1, 0.001, 0.0, (_ffi.f32 * 1)(-0.5), fake),
           (fake, 1, 0.001, 0.0, (_ffi.f32 * 1)(math.nan), fake), (fake, 1, 0.001, 0.0, (_ffi.f32 * 1)(math.inf), fake)]
    for rows, n, eeta, eps, decay, trust in bad:
        assert lib.vl_lars_trust(rows, n, eeta, eps, decay, 0.0, None, 1.0, trust, None) != 0, (rows, n, eeta, eps, trust)
        assert b"vl_lars_trust" in lib.vl_last_error()

    def table(entries):
        arr = (_ffi.LarsRange * max(len(entries), 1))()
        for k, (a, b, m, t) in enumerate(entries):
            arr[k].begin, arr[k].end, arr[k].lr_mult, arr[k].trust_index = a, b, m, t
        return arr, len(entries)

    count, n_trust = 1000, 3
    tables = [[], [(i, i + 1, 1.0, -1) for i in range(65)], [(0, 10, 1.0, 3)], [(0, 10, 1.0, -2)], [(0, 10, 0.0, 0)], [(0, 10, math.nan, 0)],
              [(0, 10, 1.0, 0), (9, 20, 1.0, 1)], [(10, 20, 1.0, 0), (5, 8, 1.0, 1)], [(0, count + 1, 1.0, 0)], [(5, 5, 1.0, 0)]]
    for entries in tables:
        arr, n = table(entries)
        for name, lr in (("vl_lars_apply", 0.01), ("vl_lars_apply_st", fake)):
            assert getattr(lib, name)(fake, fake, fake, count, lr, 0.9, 0, 0.0, None, 1.0, None, arr, n, fake, n_trust, None) != 0, entries
            assert name.encode() in lib.vl_last_error()
    arr, n = table([(0, 10, 1.0, 0)])
    assert lib.vl_lars_apply(fake, fake, fake, count, 0.01, 0.9, 0, 0.0, None, 1.0, None, arr, n, None, 1, None) != 0      # a null trust array
    assert lib.vl_lars_apply(fake, fake, fake, count, 0.01, 0.9, 0, 0.0, None, 1.0, None, arr, n, None, 0, None) != 0      # index 0 of 0
    assert lib.vl_lars_apply(fake, fake, None, count, 0.01, 0.9, 0, 0.0, None, 1.0, None, arr, n, fake, 1, None) != 0      # no accumulator
    assert lib.vl_lars_apply_st(fake, fake, fake, count, None, 0.9, 0, 0.0, None, 1.0, None, arr, n, fake, 1, None) != 0   # no step state
    for m in (0.0, 1.0, -0.5, math.nan):
        assert lib.vl_lars_apply(fake, fake, fake, count, 0.01, m, 0, 0.0, None, 1.0, None, arr, n, fake, 1, None) != 0
        assert b"momentum" in lib.vl_last_error()
