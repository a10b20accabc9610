"""LAMB on the host: check_lamb, the `train: lamb / lamb_epsilon` keys with their refusals, the range table of the update against
tests/lamb_ref.py, lamb_corrections against double arithmetic, the example, and the C-ABI table (header, ctypes records and library
agree, the step state keeps its size and offsets).  No GPU: no engine is constructed."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import yaml

from tests import lamb_ref
from tests.test_finetune import _settings
from vltf_amd._ffi import VltfError
from vltf_amd.engine import (NetConfig, check_lamb, check_lars, finetune_plan, lamb_corrections, lamb_ranges, param_specs, stat_segments,
                             tier_plan)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADAM = "defs.optim.adam"


# ---- check_lamb ------------------------------------------------------------------------------------------------------------------------
def test_check_lamb_accepts():
    for opt in ("sgd", "adam"):
        for lamb in (None, False, np.bool_(False)):
            assert check_lamb(opt, lamb, None) == (False, 0.0)                  # off: no demand on the optimizer
    assert check_lamb("adam", True, None) == (True, 1e-6)                       # TFA's default
    assert check_lamb("adam", np.bool_(True), 1e-8) == (True, 1e-8)
    assert check_lamb("adam", True, np.float32(0.5)) == (True, 0.5)
    assert check_lamb("adam", True, 1) == (True, 1.0)
    assert NetConfig().lamb is False and NetConfig().lamb_epsilon is None


@pytest.mark.parametrize("lamb,eps", [(1, None), ("True", None), (0.5, None), (True, 0.0), (True, -1e-6), (True, float("nan")),
                                      (True, float("inf")), (True, "1e-6"), (True, True), (True, 1e-60), (False, 1e-6), (None, 1e-6)])
def test_check_lamb_refuses_values(lamb, eps):
    with pytest.raises(VltfError, match="lamb"):
        check_lamb("adam", lamb, eps)


def test_check_lamb_refuses_any_optimizer_but_adam_and_lars_stays_refused():
    for opt in ("sgd", "rmsprop", None):
        with pytest.raises(VltfError, match="adam"):
            check_lamb(opt, True, None)
    with pytest.raises(VltfError, match="adam"):
        check_lars("adam", 0.0, 0.001, 0.0)


# ---- YAML ------------------------------------------------------------------------------------------------------------------------------
def test_settings_keys_parse(tmp_path):
    s = _settings(tmp_path, train={"optimizer": ADAM, "lamb": True, "lamb_epsilon": 1e-7})
    assert s.train.lamb is True and s.train.lamb_epsilon == 1e-7 and s.get_lamb() == (True, 1e-7)
    s = _settings(tmp_path, train={"optimizer": ADAM, "lamb": True})
    assert s.get_lamb() == (True, 1e-6)
    s = _settings(tmp_path, train={"optimizer": ADAM, "lamb": True, "lamb_epsilon": "1e-5"})     # YAML reads 1e-5 as a string
    assert s.get_lamb() == (True, 1e-5)
    s = _settings(tmp_path, train={"optimizer": ADAM, "lamb": True, "weight_decay": 0.01})
    assert s.get_lamb() == (True, 1e-6) and s.train.weight_decay == 0.01


@pytest.mark.parametrize("train", [{}, {"lamb": None}, {"lamb": "None", "lamb_epsilon": "None"}, {"lamb": False}, {"lamb_epsilon": None},
                                   {"optimizer": ADAM}, {"optimizer": ADAM, "lamb": False}],
                         ids=["absent", "null", "None-strings", "false", "epsilon-null", "adam-only", "adam-false"])
def test_settings_absent_keys_mean_off(tmp_path, train):
    s = _settings(tmp_path, train=train)
    assert s.train.lamb is False and s.train.lamb_epsilon is None and s.get_lamb() == (False, None)


@pytest.mark.parametrize("train", [{"lamb": True}, {"optimizer": "defs.optim.sgd", "momentum": 0.9, "lamb": True},
                                   {"optimizer": ADAM, "lamb": 1}, {"optimizer": ADAM, "lamb": "yes"},
                                   {"optimizer": ADAM, "lamb": True, "lamb_epsilon": 0}, {"optimizer": ADAM, "lamb": True, "lamb_epsilon": -1e-6},
                                   {"optimizer": ADAM, "lamb": True, "lamb_epsilon": "nan"}, {"optimizer": ADAM, "lamb": True, "lamb_epsilon": "inf"},
                                   {"optimizer": ADAM, "lamb": True, "lamb_epsilon": "small"}, {"optimizer": ADAM, "lamb_epsilon": 1e-6},
                                   {"optimizer": ADAM, "lamb": False, "lamb_epsilon": 1e-6}])
def test_settings_refusals(tmp_path, train):
    with pytest.raises(Exception, match="lamb"):
        _settings(tmp_path, train=train)


def test_settings_lars_with_adam_stays_refused(tmp_path):
    with pytest.raises(Exception, match="lars"):
        _settings(tmp_path, train={"optimizer": ADAM, "lamb": True, "lars_eeta": 0.001})


def test_settings_outside_the_train_phase_is_off(tmp_path):
    from tests.test_ema import _val_settings
    s = _val_settings(tmp_path, train={"optimizer": ADAM, "lamb": True, "lamb_epsilon": 1e-7})
    assert s.get_lamb() == (False, None)


def test_example_yaml_is_the_adam_configuration_with_the_two_keys(tmp_path):
    """examples/lrcn_lamb.yml without `lamb` and `lamb_epsilon` is an Adam configuration -- that of lrcn_weight_decay.yml with the
    optimizer exchanged (no momentum, Adam's own decay value) -- and parses as plain Adam; with them it parses as LAMB."""
    here = os.path.join(ROOT, "examples")
    with open(os.path.join(here, "lrcn_lamb.yml")) as f:
        lamb = yaml.safe_load(f)
    with open(os.path.join(here, "lrcn_weight_decay.yml")) as f:
        base = yaml.safe_load(f)
    keys = dict(lamb["run"]["train"])
    assert lamb["run"]["train"].pop("lamb") is True and lamb["run"]["train"].pop("lamb_epsilon") == 1e-6
    assert base["run"]["train"].pop("momentum") == 0.9
    base["run"]["train"].update(optimizer=ADAM, weight_decay=lamb["run"]["train"]["weight_decay"])
    for cfg in (lamb, base):
        cfg["run"].pop("run_folder", None), cfg["run"].pop("run_id", None)
    assert lamb == base and lamb["run"]["train"]["optimizer"] == ADAM
    plain = {k: keys[k] for k in ("optimizer", "weight_decay", "lr_mult")}
    s = _settings(tmp_path, train=plain, pipeline={"train_from": "fc6"})
    assert s.get_lamb() == (False, None) and s.train.optimizer == "adam"
    s = _settings(tmp_path, train=dict(plain, lamb=keys["lamb"], lamb_epsilon=keys["lamb_epsilon"]), pipeline={"train_from": "fc6"})
    assert s.get_lamb() == (True, 1e-6) and s.train.weight_decay == keys["weight_decay"]


# ---- the range table -----------------------------------------------------------------------------------------------------------------
SPECS = [("head/W", (6, 4)), ("head/b", (4,)), ("dcnn/fc7W", (5, 3)), ("dcnn/fc7b", (3,)), ("dcnn/fc6W", (7, 5)), ("dcnn/fc6b", (5,)),
         ("dcnn/conv5W", (3, 3, 2, 2)), ("dcnn/conv5b", (2,)), ("dcnn/conv4W", (3, 3, 2, 2)), ("dcnn/conv4b", (2,))]


def test_range_table_small_spec_list_with_a_frozen_layer():
    """conv5 frozen, lr_mult 4 on the head: biases carry decay 0 and index -1, the frozen layer is absent from ranges and segments, the
    trust indices of the weight tensors count from 0 without a hole, and the table equals the reference's restatement."""
    total = sum(int(np.prod(s)) for _, s in SPECS)
    plan = tier_plan(SPECS, {"dcnn/conv5W", "dcnn/conv5b"}, 4.0, [(0, total)])
    ranges, segs = lamb_ranges(SPECS, plan, 0.0005)
    assert (ranges, segs) == lamb_ref.ranges(SPECS, plan.tiers, 0.0005)
    assert ranges == [(0, 24, 4.0, 0.0005, 0), (24, 28, 4.0, 0.0, -1), (28, 43, 1.0, 0.0005, 1), (43, 46, 1.0, 0.0, -1),
                      (46, 81, 1.0, 0.0005, 2), (81, 86, 1.0, 0.0, -1), (124, 160, 1.0, 0.0005, 3), (160, 162, 1.0, 0.0, -1)]
    assert [s[0] for s in segs] == ["head/W", "dcnn/fc7W", "dcnn/fc6W", "dcnn/conv4W"]
    assert [r[4] for r in ranges if r[4] >= 0] == list(range(len(segs)))
    assert [(r[0], r[1]) for r in ranges if r[4] >= 0] == [(s[1], s[2]) for s in segs]
    assert not any(r[0] < 124 and r[1] > 86 for r in ranges)                          # nothing touches the frozen extent [86, 124)
    assert [r[3] for r in lamb_ranges(SPECS, plan, 0.0)[0]] == [0.0] * 8              # weight decay off: the coefficient is 0
    assert [r[3] for r in lamb_ranges(SPECS, plan, None)[0]] == [0.0] * 8


def test_adjacent_biases_of_one_factor_merge_and_of_two_do_not():
    specs = [("a/W", (2, 2)), ("a/b", (2,)), ("a/c", (3,)), ("dcnn/fc6b", (4,)), ("dcnn/fc6W", (2, 3))]
    plan = tier_plan(specs, (), 2.0, [(0, 19)])
    ranges, segs = lamb_ranges(specs, plan, 0.25)
    assert ranges == [(0, 4, 2.0, 0.25, 0), (4, 9, 2.0, 0.0, -1), (9, 13, 1.0, 0.0, -1), (13, 19, 1.0, 0.25, 1)]
    assert ranges == lamb_ref.ranges(specs, plan.tiers, 0.25)[0]
    assert [s[0] for s in segs] == ["a/W", "dcnn/fc6W"]


@pytest.mark.parametrize("train_from", [None, "conv3", "fc6"])
def test_range_table_of_the_lrcn(train_from):
    cfg = NetConfig(image_shape=(67, 67, 3), num_classes=7, fpc=3, lstm_hidden=8, train_from=train_from, lr_mult=10.0, optimizer="adam")
    specs, plan = param_specs(cfg), finetune_plan(cfg)
    ranges, segs = lamb_ranges(specs, plan, 0.001)
    assert (ranges, segs) == lamb_ref.ranges(specs, plan.tiers, 0.001)
    shapes = dict(specs)
    trained = [n for n, _, _ in stat_segments(specs, plan)]
    assert [s[0] for s in segs] == [n for n in trained if len(shapes[n]) >= 2] and len(segs) < len(trained)
    assert sum(r[1] - r[0] for r in ranges) == sum(hi - lo for lo, hi, _ in plan.tiers)          # every trained element, once
    assert all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:]))
    assert not any(n in plan.frozen for n, _, _ in segs)
    assert all((r[3] == 0.001) == (r[4] >= 0) for r in ranges)                                     # decay exactly where there is an index
    if train_from:
        assert plan.frozen and {r[2] for r in ranges} == {1.0, 10.0}


# ---- the bias corrections ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1, 2, 1000])
def test_lamb_corrections_against_double_arithmetic(t):
    c1, c2 = lamb_corrections(t - 1)                      # n earlier updates, t = n + 1
    want1, want2 = 1.0 / (1.0 - math.pow(0.9, t)), 1.0 / (1.0 - math.pow(0.999, t))
    assert c1 == float(np.float32(want1)) and c2 == float(np.float32(want2))
    assert (np.float32(c1), np.float32(c2)) == lamb_ref.corrections(t)
    assert isinstance(c1, float) and isinstance(c2, float) and c1 >= 1.0 and c2 >= 1.0
    if t == 1:
        assert (c1, c2) == (10.0, 1000.0)
    if t == 1000:
        assert c1 == 1.0 and 1.5 < c2 < 1.6
    with pytest.raises(VltfError):
        lamb_corrections(-1)


def test_reference_rule():
    """The reference itself at hand-checked values."""
    w, u = np.array([3.0, 4.0], np.float32), np.array([0.6, 0.8], np.float32)
    assert lamb_ref.trust(w, u) == pytest.approx(5.0, rel=1e-7)
    assert lamb_ref.trust(np.zeros(2), u) == 1.0 and lamb_ref.trust(w, np.zeros(2)) == 1.0
    assert lamb_ref.trust(w, np.array([np.nan, 1.0])) == 1.0 and lamb_ref.trust(np.array([np.inf, 1.0]), u) == 1.0
    m1, v1 = lamb_ref.moments(np.array([2.0], np.float32), np.zeros(1, np.float32), np.zeros(1, np.float32), 0.5)
    assert m1[0] == np.float32(np.float32(0.1) * np.float32(1.0)) and v1[0] == np.float32(0.001)
    u0 = lamb_ref.direction(np.array([7.0], np.float32), m1, v1, 10.0, 1000.0, 1e-6, 0.0)
    assert u0[0] == pytest.approx(1.0, rel=1e-5)
    u1 = lamb_ref.direction(np.array([7.0], np.float32), m1, v1, 10.0, 1000.0, 1e-6, 0.5)
    assert u1[0] == pytest.approx(4.5, rel=1e-5)
    assert lamb_ref.rate(0.01, 4.0, 1.0) == np.float32(np.float32(0.01) * np.float32(4.0))
    assert lamb_ref.trust_tol(10, 0.0) < lamb_ref.trust_tol(10, 0.1) < 2.0 ** -22


# ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------
NAMES = ("vl_lamb_moments", "vl_lamb_moments_st", "vl_lamb_apply", "vl_lamb_apply_st", "vl_step_state_set_lamb")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vltf.h")).read(), flags=re.S)


def test_ffi_table_records_and_step_state():
    from vltf_amd import _ffi
    p, i32, i64, f32, sz = _ffi.p, _ffi.i32, _ffi.i64, _ffi.f32, _ffi.sz
    S = _ffi.SIGNATURES
    assert S["vl_lamb_moments_ws_bytes"] == (sz, [p, i32])
    assert S["vl_lamb_moments"] == (i32, [p, p, p, p, i64, f32, f32, f32, f32, p, f32, p, p, i32, p, p, i32, p, sz, p])
    assert S["vl_lamb_moments_st"] == (i32, [p, p, p, p, i64, p, f32, f32, p, f32, p, p, i32, p, p, i32, p, sz, p])
    assert S["vl_lamb_apply"] == (i32, [p, p, p, i64, f32, f32, f32, f32, p, p, i32, p, i32, p])
    assert S["vl_lamb_apply_st"] == (i32, [p, p, p, i64, p, f32, p, p, i32, p, i32, p])
    assert S["vl_step_state_set_lamb"] == (i32, [p, f32, f32, p])
    src = _header()
    for name in NAMES:
        m = re.search(r"\bint %s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
        assert m and m.group(1).count(",") + 1 == len(S[name][1]), name
        assert hasattr(_ffi.lib(), name)
    assert hasattr(_ffi.lib(), "vl_lamb_moments_ws_bytes")
    body = re.search(r"typedef struct vl_lamb_range \{(.*?)\} vl_lamb_range;", src, flags=re.S).group(1)
    assert [d.strip() for d in body.split(";") if d.strip()] == ["int64_t begin, end", "float lr_mult", "float decay",
                                                                  "int32_t trust_index", "int32_t reserved"]
    R = _ffi.LambRange
    assert [n for n, _ in R._fields_] == ["begin", "end", "lr_mult", "decay", "trust_index", "reserved"] and ctypes.sizeof(R) == 32
    assert (R.begin.offset, R.end.offset, R.lr_mult.offset, R.decay.offset, R.trust_index.offset, R.reserved.offset) == (0, 8, 16, 20, 24, 28)
    body = re.search(r"typedef struct vl_lamb_row \{(.*?)\} vl_lamb_row;", src, flags=re.S).group(1)
    assert [d.strip() for d in body.split(";") if d.strip()] == ["double w_sumsq, u_sumsq", "uint32_t nonfinite, reserved"]
    W = _ffi.LambRow
    assert ctypes.sizeof(W) == 24 and (W.w_sumsq.offset, W.u_sumsq.offset, W.nonfinite.offset, W.reserved.offset) == (0, 8, 16, 20)
    from vltf_amd import ops
    assert ops.LAMB_ROW_BYTES == 24 and ops.LAMB_ROW_DTYPE.itemsize == 24
    assert [ops.LAMB_ROW_DTYPE.fields[k][1] for k in ("w_sumsq", "u_sumsq", "nonfinite", "reserved")] == [0, 8, 16, 20]
    # the step state: its size and every earlier field offset stay; LAMB's two words are the block's last two, bytes 24 and 28
    St = _ffi.StepState
    assert ctypes.sizeof(St) == 32 and int(_ffi.lib().vl_step_state_bytes()) == 32
    assert (St.step.offset, St.lr.offset, St.tag_origin.offset, St.adam_lr.offset, St.ema_rate.offset) == (0, 8, 12, 16, 20)
    assert (_ffi.STEP_STATE_LAMB_C1_OFFSET, _ffi.STEP_STATE_LAMB_C2_OFFSET) == (24, 28)
    assert St.reserved.offset == 24 and St.reserved.size == 8
    c1 = int(re.search(r"#define VL_STEP_STATE_LAMB_C1 (\d+)", src).group(1))
    c2 = int(re.search(r"#define VL_STEP_STATE_LAMB_C2 (\d+)", src).group(1))
    assert (St.reserved.offset + 4 * c1, St.reserved.offset + 4 * c2) == (24, 28)
    # the Adam entry points LAMB stands beside are declared as they were
    assert S["vl_adam_apply"] == (i32, [p, p, p, p, i64, f32, f32, p, f32, i32, p, p])
    assert S["vl_step_state_set"] == (i32, [p, i64, f32, _ffi.u32, p])


def _table(entries):
    from vltf_amd import _ffi
    arr = (_ffi.LambRange * max(len(entries), 1))()
    for k, (a, b, m, d, t) in enumerate(entries):
        arr[k].begin, arr[k].end, arr[k].lr_mult, arr[k].decay, arr[k].trust_index = a, b, m, d, t
    return arr, len(entries)


BAD_TABLES = [[], [(i, i + 1, 1.0, 0.0, -1) for i in range(65)], [(0, 10, 1.0, 0.0, 3)], [(0, 10, 1.0, 0.0, -2)], [(0, 10, 0.0, 0.0, 0)],
              [(0, 10, math.nan, 0.0, 0)], [(0, 10, math.inf, 0.0, 0)], [(0, 10, 1.0, -0.5, 0)], [(0, 10, 1.0, math.nan, 0)],
              [(0, 10, 1.0, math.inf, 0)], [(0, 10, 1.0, 0.0, 0), (9, 20, 1.0, 0.0, 1)], [(10, 20, 1.0, 0.0, 0), (5, 8, 1.0, 0.0, 1)],
              [(0, 1001, 1.0, 0.0, 0)], [(5, 5, 1.0, 0.0, 0)]]


def test_host_refusals_need_no_device():
    """The C entry points validate before they launch: null pointers, count, the scalars, the table, the workspace.  Nothing runs, and
    every message names the entry point and the argument."""
    from vltf_amd import _ffi
    lib = _ffi.lib()
    fake = 4096                                  # a non-null, aligned address: validation fails before anything dereferences it
    count, n_trust = 1000, 3
    good, n = _table([(0, 10, 1.0, 0.0, 0), (10, 20, 2.0, 0.01, -1)])
    big = 1 << 20

    def moments(w=fake, g=fake, m=fake, v=fake, cnt=count, c1=10.0, c2=1000.0, eps=1e-6, arr=good, na=n, rows=fake, trust=fake,
                nt=n_trust, ws=fake, wsb=big):
        return lib.vl_lamb_moments(w, g, m, v, cnt, c1, c2, eps, 0.0, None, 1.0, None, arr, na, rows, trust, nt, ws, wsb, None)

    def moments_st(state=fake, eps=1e-6, arr=good, na=n, w=fake, wsb=big):
        return lib.vl_lamb_moments_st(w, fake, fake, fake, count, state, eps, 0.0, None, 1.0, None, arr, na, fake, fake, n_trust, fake, wsb, None)

    def apply(w=fake, m=fake, v=fake, cnt=count, lr=0.01, c1=10.0, c2=1000.0, eps=1e-6, arr=good, na=n, trust=fake, nt=n_trust):
        return lib.vl_lamb_apply(w, m, v, cnt, lr, c1, c2, eps, None, arr, na, trust, nt, None)

    def apply_st(state=fake, eps=1e-6, arr=good, na=n, w=fake):
        return lib.vl_lamb_apply_st(w, fake, fake, count, state, eps, None, arr, na, fake, n_trust, None)

    def refused(rc, who, word):
        err = lib.vl_last_error()
        assert rc != 0 and who.encode() in err and word.encode() in err, (rc, who, word, err)

    for arg in ("w", "g", "m", "v", "ws"):
        refused(moments(**{arg: None}), "vl_lamb_moments", arg)
    refused(moments(rows=None), "vl_lamb_moments", "rows")
    refused(moments(trust=None), "vl_lamb_moments", "trust")
    refused(moments(nt=-1), "vl_lamb_moments", "trust")
    for cnt in (0, -5):
        refused(moments(cnt=cnt), "vl_lamb_moments", "count")
        refused(apply(cnt=cnt), "vl_lamb_apply", "count")
    for arg in ("w", "m", "v"):
        refused(apply(**{arg: None}), "vl_lamb_apply", arg)
    refused(apply(trust=None), "vl_lamb_apply", "trust")
    refused(moments_st(state=None), "vl_lamb_moments_st", "state")
    refused(apply_st(state=None), "vl_lamb_apply_st", "state")
    refused(moments_st(w=None), "vl_lamb_moments_st", "w")
    refused(apply_st(w=None), "vl_lamb_apply_st", "w")
    for eps in (0.0, -1e-6, math.nan, math.inf):
        refused(moments(eps=eps), "vl_lamb_moments", "eps")
        refused(moments_st(eps=eps), "vl_lamb_moments_st", "eps")
        refused(apply(eps=eps), "vl_lamb_apply", "eps")
        refused(apply_st(eps=eps), "vl_lamb_apply_st", "eps")
    for c in (0.5, 0.0, -2.0, math.nan, math.inf):
        refused(moments(c1=c), "vl_lamb_moments", "c1")
        refused(moments(c2=c), "vl_lamb_moments", "c2")
        refused(apply(c1=c), "vl_lamb_apply", "c1")
        refused(apply(c2=c), "vl_lamb_apply", "c2")
        refused(lib.vl_step_state_set_lamb(fake, c, 1.0, None), "vl_step_state_set_lamb", "c1")
        refused(lib.vl_step_state_set_lamb(fake, 1.0, c, None), "vl_step_state_set_lamb", "c2")
    refused(lib.vl_step_state_set_lamb(None, 10.0, 1000.0, None), "vl_step_state_set_lamb", "state")
    for entries in BAD_TABLES:
        arr, na = _table(entries)
        refused(moments(arr=arr, na=na), "vl_lamb_moments", "ranges")
        refused(moments_st(arr=arr, na=na), "vl_lamb_moments_st", "ranges")
        refused(apply(arr=arr, na=na), "vl_lamb_apply", "ranges")
        refused(apply_st(arr=arr, na=na), "vl_lamb_apply_st", "ranges")
    refused(moments(arr=None), "vl_lamb_moments", "ranges")
    arr, na = _table([(0, 10, 1.0, 0.0, 0)])
    refused(moments(arr=arr, na=na, nt=0, rows=None, trust=None), "vl_lamb_moments", "ranges")     # index 0 of 0
    refused(apply(arr=arr, na=na, nt=0, trust=None), "vl_lamb_apply", "ranges")
    # the workspace: one 24-byte row per chunk of every range
    assert lib.vl_lamb_moments_ws_bytes(good, n) == 2 * 24
    two, nn = _table([(0, _ffi.STAT_CHUNK + 5, 1.0, 0.0, 0), (_ffi.STAT_CHUNK + 9, _ffi.STAT_CHUNK + 10, 1.0, 0.0, -1)])
    assert lib.vl_lamb_moments_ws_bytes(two, nn) == 3 * 24
    assert lib.vl_lamb_moments_ws_bytes(None, 1) == 0 and lib.vl_lamb_moments_ws_bytes(*_table([(5, 5, 1.0, 0.0, 0)])) == 0
    refused(moments(wsb=2 * 24 - 1), "vl_lamb_moments", "ws")
    refused(moments_st(wsb=0), "vl_lamb_moments_st", "ws")
    refused(moments(w=fake + 2), "vl_lamb_moments", "misaligned")
    refused(moments(ws=fake + 4), "vl_lamb_moments", "misaligned")
