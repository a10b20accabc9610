"""L2 weight decay on the host: the `weight_decay` key of the `train:` section and its refusals, engine.check_weight_decay, the range
table engine.decay_ranges hands the kernel (weights decayed, biases and frozen variables exempt), the C-ABI symbol and its struct, and
the example YAML.  No GPU: no engine is constructed."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import yaml

from tests.test_finetune import _settings
from vltf_amd import _ffi
from vltf_amd._ffi import VltfError
from vltf_amd.engine import NetConfig, check_weight_decay, decay_ranges, finetune_plan, param_specs, tier_plan

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPE, NCLS, FPC, HID = (67, 67, 3), 7, 3, 8
WD = 0.05


def small_cfg(**kw):
    return NetConfig(image_shape=SHAPE, num_classes=NCLS, fpc=FPC, frame_encoding_layer="fc6", lstm_hidden=HID, **kw)


# ---- settings ------------------------------------------------------------------------------------------------------------------
def test_settings_weight_decay_parses(tmp_path):
    s = _settings(tmp_path, train={"weight_decay": 0.0005})
    assert s.train.weight_decay == 0.0005 and isinstance(s.train.weight_decay, float)
    assert _settings(tmp_path, train={"weight_decay": "5e-4"}).train.weight_decay == 0.0005      # (YAML 1.1 reads 5e-4 as a string)
    assert _settings(tmp_path, train={"weight_decay": 0}).train.weight_decay == 0.0


@pytest.mark.parametrize("train", [{}, {"weight_decay": None}, {"weight_decay": "None"}], ids=["absent", "null", "None-string"])
def test_settings_absent_key_changes_nothing(tmp_path, train):
    s, base = _settings(tmp_path, train=train), _settings(tmp_path)
    assert s.train.weight_decay == 0.0 and NetConfig().weight_decay == 0.0
    assert vars(s.train) == vars(base.train)


@pytest.mark.parametrize("bad", [-0.001, float("nan"), float("inf"), "nan", "inf", "-inf", "much", True, [0.1]],
                         ids=["negative", "nan", "inf", "nan-string", "inf-string", "neg-inf-string", "string", "bool", "list"])
def test_settings_refusals(tmp_path, bad):
    with pytest.raises(Exception, match="weight_decay must be a finite number >= 0"):
        _settings(tmp_path, train={"weight_decay": bad})


def test_check_weight_decay():
    assert check_weight_decay(None) == 0.0 and check_weight_decay(0) == 0.0 and check_weight_decay(0.0005) == 0.0005
    assert check_weight_decay(np.float32(0.5)) == 0.5 and isinstance(check_weight_decay(1), float)
    for bad in (-1, -1e-9, float("nan"), float("inf"), -float("inf"), "0.1", "much", b"1", True, [1.0], {}):
        with pytest.raises(VltfError, match="weight_decay must be a finite number >= 0"):
            check_weight_decay(bad)


# ---- the range table -------------------------------------------------------------------------------------------------------------
def extents(specs):
    out, off = [], 0
    for name, shp in specs:
        out.append((name, off, off + int(np.prod(shp)), len(shp)))
        off += int(np.prod(shp))
    return out


def test_decay_ranges_full_model():
    """Weights and biases alternate in the flat buffer, so nothing merges: one entry per variable, lambda on rank >= 2, 0 on rank 1."""
    cfg = small_cfg()
    specs, plan = param_specs(cfg), finetune_plan(cfg)
    table = decay_ranges(specs, plan, WD)
    ext = extents(specs)
    assert len(table) == len(specs) == 16
    assert table == [(lo, hi, WD if rank >= 2 else 0.0) for _, lo, hi, rank in ext]
    assert [c for _, _, c in table] == [WD, 0.0] * 8
    decayed = {n for n, _, _, rank in ext if rank >= 2}
    assert decayed == {"output_fc_w", "rnn/multi_rnn_cell/cell_0/basic_lstm_cell/kernel", "dcnn/fc6W"} | {"dcnn/conv%dW" % i for i in range(1, 6)}
    # lr_mult changes the tiers (two of them), not the table
    assert decay_ranges(specs, finetune_plan(small_cfg(lr_mult=10.0)), WD) == table
    assert decay_ranges(specs, plan, 0.0) == [(0, plan.total, 0.0)]               # everything one coefficient: one merged entry


def test_decay_ranges_train_from_fc6():
    cfg = small_cfg(train_from="fc6", lr_mult=4.0)
    specs, plan = param_specs(cfg), finetune_plan(cfg)
    table = decay_ranges(specs, plan, WD)
    kept = [(lo, hi, WD if rank >= 2 else 0.0) for n, lo, hi, rank in extents(specs) if "conv" not in n]
    assert table == kept and len(table) == 6                                      # output_fc w/b, LSTM kernel/bias, fc6 W/b
    assert table[-1][1] == plan.tiers[-1][1] < plan.total                         # nothing reaches into the frozen conv stack
    for name in plan.frozen:
        assert "conv" in name


def test_decay_ranges_merges_adjacent_equal_coefficients():
    specs = [("aW", (3, 4)), ("ab", (4,)), ("bb", (5,)), ("cW", (2, 2)), ("dW", (2, 3)), ("db", (3,))]
    plan = tier_plan(specs, [], None, [(0, 34)])
    assert decay_ranges(specs, plan, 0.1) == [(0, 12, 0.1), (12, 21, 0.0), (21, 31, 0.1), (31, 34, 0.0)]
    # a frozen variable between two biases keeps them apart (the gap is in no entry)
    plan = tier_plan(specs, ["bb"], None, [(0, 34)])
    assert decay_ranges(specs, plan, 0.1) == [(0, 12, 0.1), (12, 16, 0.0), (21, 31, 0.1), (31, 34, 0.0)]


def test_decay_ranges_refuses_65_entries():
    specs = []
    for i in range(33):
        specs += [("l%dW" % i, (2, 2)), ("l%db" % i, (2,))]
    plan = tier_plan(specs, [], None, [(0, 33 * 6)])
    with pytest.raises(VltfError, match="65"):
        decay_ranges(specs[:65], tier_plan(specs[:65], [], None, [(0, 1)]), 0.1)
    assert len(decay_ranges(specs[:64], tier_plan(specs[:64], [], None, [(0, 1)]), 0.1)) == 64
    with pytest.raises(VltfError, match="66"):
        decay_ranges(specs, plan, 0.1)
    with pytest.raises(VltfError, match="finite number >= 0"):
        decay_ranges(specs[:4], tier_plan(specs[:4], [], None, [(0, 1)]), -0.1)


# ---- symbols -----------------------------------------------------------------------------------------------------------------------
def header():
    with open(os.path.join(HERE, "..", "include", "vltf.h")) as f:
        return f.read()


def test_symbol_in_table_header_and_library():
    assert "vl_l2_regularize" in _ffi.SIGNATURES
    res, args = _ffi.SIGNATURES["vl_l2_regularize"]
    assert len(args) == 8
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    m = re.search(r"\bint\s+vl_l2_regularize\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert m and len(m.group(1).split(",")) == 8
    assert hasattr(_ffi.lib(), "vl_l2_regularize")


def test_decay_range_layout_matches_header():
    src = header()
    assert re.search(r"#define\s+VL_MAX_DECAY_RANGES\s+64\b", src) and _ffi.MAX_DECAY_RANGES == 64
    m = re.search(r"typedef\s+struct\s+vl_decay_range\s*\{(.*?)\}\s*vl_decay_range\s*;", src, flags=re.S)
    assert m and [s.strip() for s in m.group(1).split(";") if s.strip()] == ["int64_t begin, end", "float decay"]
    R = _ffi.DecayRange
    assert [(n, t) for n, t in R._fields_] == [("begin", ctypes.c_int64), ("end", ctypes.c_int64), ("decay", ctypes.c_float)]
    assert (R.begin.offset, R.end.offset, R.decay.offset, ctypes.sizeof(R)) == (0, 8, 16, 24)


# ---- example -----------------------------------------------------------------------------------------------------------------------
def test_example_yaml_is_the_momentum_one_plus_the_key():
    ex = os.path.join(HERE, "..", "examples")
    with open(os.path.join(ex, "lrcn_weight_decay.yml")) as f:
        wd = yaml.safe_load(f)
    with open(os.path.join(ex, "lrcn_momentum.yml")) as f:
        mom = yaml.safe_load(f)
    assert wd["run"]["train"].pop("weight_decay") == 0.0005
    assert wd["run"].pop("run_id") != mom["run"].pop("run_id")                    # each run keeps its own id
    assert wd == mom
    assert math.isclose(check_weight_decay(0.0005), 5e-4)
