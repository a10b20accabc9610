"""Per-variable gradient and weight statistics (logging.tensor_stats_interval), host side: the interval's check, the YAML key, the
segment table of the default model / frozen models / a two-pipeline graph, the chunk plan of the segmented launch, the derived keys
against hand-computed rows, the JSONL writer and the example.  No engine is constructed and no device is used; the launch itself is
tests/test_tensor_stats_gpu.py's."""
import collections
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import yaml

from tests import tensor_stats_ref as R
from tests.test_finetune import _settings, graph_plan
from vltf_amd import _ffi, ops
from vltf_amd._ffi import VltfError
from vltf_amd.defs_ import defs
from vltf_amd.engine import (NetConfig, check_tensor_stats_interval, clip_scale_of, finetune_plan, param_specs, stat_segments,
                             tensor_stats_report)

HERE = os.path.dirname(os.path.abspath(__file__))
CHUNK = ops.STAT_CHUNK


# ---- the interval ------------------------------------------------------------------------------------------------------------------
def test_check_tensor_stats_interval():
    assert check_tensor_stats_interval(None) == 0 and check_tensor_stats_interval(0) == 0
    assert check_tensor_stats_interval(1) == 1 and check_tensor_stats_interval(10) == 10 and check_tensor_stats_interval(np.int64(3)) == 3
    assert isinstance(check_tensor_stats_interval(np.int32(7)), int)
    for bad in (-1, 1.0, 2.5, float("nan"), "10", b"1", True, False, [1], {}):
        with pytest.raises(VltfError, match="tensor_stats_interval must be an integer >= 1"):
            check_tensor_stats_interval(bad)
    assert NetConfig().tensor_stats_interval == 0


# ---- settings ----------------------------------------------------------------------------------------------------------------------
def _with_logging(tmp_path, **logging_keys):
    """The settings of tests.test_finetune's config with keys added to its logging block."""
    from tests.test_host_workflow import config, make_dataset
    from vltf_amd import settings_
    folder = str(tmp_path)
    data_path, _, _ = make_dataset(folder, "train.txt")
    path = config(folder, data_path)
    with open(path) as f:
        cfg = yaml.safe_load(f)
    cfg["run"]["logging"].update(logging_keys)
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    s = settings_.Settings()
    s.initialize(path)
    return s


@pytest.mark.parametrize("keys", [{}, {"tensor_stats_interval": None}, {"tensor_stats_interval": "None"}, {"tensor_stats_interval": 0}],
                         ids=["absent", "null", "None-string", "zero"])
def test_settings_off_forms(tmp_path, keys):
    s, base = _with_logging(tmp_path, **keys), _settings(tmp_path)
    assert s.tensor_stats_interval == 0 and s.get_tensor_stats_interval() == 0
    assert vars(s.train) == vars(base.train)


def test_settings_key_parses_and_holds_in_the_train_phase_only(tmp_path):
    s = _with_logging(tmp_path, tensor_stats_interval=10)
    assert s.tensor_stats_interval == 10 and s.get_tensor_stats_interval() == 10
    assert _with_logging(tmp_path, tensor_stats_interval="5").get_tensor_stats_interval() == 5       # a quoted number
    s.phase = defs.phase.val                              # a val run of the same file: no statistics
    assert s.get_tensor_stats_interval() == 0


@pytest.mark.parametrize("bad", [-1, 2.5, "much", "1.5", True, [3]], ids=["negative", "float", "string", "float-string", "bool", "list"])
def test_settings_refusals_name_the_key(tmp_path, bad):
    with pytest.raises(Exception, match=r"logging\.tensor_stats_interval: tensor_stats_interval must be an integer >= 1"):
        _with_logging(tmp_path, tensor_stats_interval=bad)


def test_run_task_passes_the_key_to_the_single_pipeline_config(tmp_path):
    from vltf_amd import run_task
    s = _with_logging(tmp_path, tensor_stats_interval=3)
    dataset = s.feeder.get_dataset_by_tag(defs.dataset_tag.main)[0]
    assert run_task.net_config(s, dataset)[0].tensor_stats_interval == 3
    s.phase = defs.phase.val
    assert run_task.net_config(s, dataset)[0].tensor_stats_interval == 0


def test_example_yaml_is_the_finetune_one_plus_the_key():
    here = os.path.join(HERE, "..", "examples")
    with open(os.path.join(here, "lrcn_tensor_stats.yml")) as f:
        st = yaml.safe_load(f)
    with open(os.path.join(here, "lrcn_finetune.yml")) as f:
        fin = yaml.safe_load(f)
    assert st["run"]["logging"].pop("tensor_stats_interval") == 10
    assert st["run"]["run_folder"] != fin["run"]["run_folder"] and st["run"]["run_id"] != fin["run"]["run_id"]
    for c in (st, fin):
        del c["run"]["run_folder"], c["run"]["run_id"]
    assert st == fin


# ---- segments ----------------------------------------------------------------------------------------------------------------------
def extents(specs):
    off, out = 0, collections.OrderedDict()
    for name, shp in specs:
        n = int(np.prod(shp))
        out[name] = (off, off + n)
        off += n
    return out, off


def test_stat_segments_default_model_tiles_the_buffer():
    cfg = NetConfig()
    specs, plan = param_specs(cfg), finetune_plan(cfg)
    segs = stat_segments(specs, plan)
    ext, total = extents(specs)
    assert [s[0] for s in segs] == [n for n, _ in specs] and len({s[0] for s in segs}) == len(segs) == 16
    assert all((lo, hi) == ext[n] for n, lo, hi in segs)
    assert segs[0][1] == 0 and segs[-1][2] == total == plan.total and all(a[2] == b[1] for a, b in zip(segs, segs[1:]))
    assert dict((n, hi - lo) for n, lo, hi in segs)["dcnn/fc6W"] == 9216 * 4096


@pytest.mark.parametrize("train_from,frozen_layers", [("fc6", ["conv1", "conv2", "conv3", "conv4", "conv5"]),
                                                      ("classifier", ["conv1", "conv2", "conv3", "conv4", "conv5", "fc6"])])
def test_stat_segments_leave_frozen_variables_out(train_from, frozen_layers):
    full = NetConfig()
    cfg = NetConfig(train_from=train_from, lr_mult=10.0)
    specs = param_specs(cfg)
    segs, all_segs = stat_segments(specs, finetune_plan(cfg)), stat_segments(param_specs(full), finetune_plan(full))
    frozen = {"dcnn/%s%s" % (l, k) for l in frozen_layers for k in "Wb"}
    assert segs == [s for s in all_segs if s[0] not in frozen] and len(segs) == 16 - len(frozen)
    assert not frozen & {s[0] for s in segs}


def test_stat_segments_two_pipeline_plan():
    """A graph's variable list (the host path graph.model_specs uses): scoped names, one tower frozen whole, one from conv3 on."""
    pipes = [("rgb", dict(input=["main"], representation="dcnn", frame_encoding_layer="fc6", train_from="classifier")),
             ("flow", dict(input=["aux"], representation="dcnn", frame_encoding_layer="fc7", train_from="conv3")),
             ("fuse", dict(input=["rgb", "flow"], input_fusion="avg", representation="nop", classifier="lstm", lstm_params=(6, 1, "avg")))]
    eng = graph_plan(pipes, ["main", "aux"], 7, lr_mult=2.0)
    segs = stat_segments(eng.specs, eng.plan)
    ext, _ = extents(eng.specs)
    frozen = set(eng.plan.frozen)
    assert [s[0] for s in segs] == [n for n, _ in eng.specs if n not in frozen]
    assert all((lo, hi) == ext[n] for n, lo, hi in segs)
    assert not any(n.startswith("rgb/") for n, _, _ in segs) and "flow/dcnn/conv2W" not in {s[0] for s in segs}
    assert {"flow/dcnn/fc7W", "flow/dcnn/conv3b"} <= {s[0] for s in segs}
    assert sum(hi - lo for _, lo, hi in segs) == sum(hi - lo for lo, hi, _ in eng.plan.tiers)


# ---- the chunk plan ----------------------------------------------------------------------------------------------------------------
def test_abi_constants_and_layout():
    src = open(os.path.join(HERE, "..", "include", "vltf.h")).read()
    assert int(re.search(r"#define VL_MAX_STAT_SEGMENTS (\d+)", src).group(1)) == _ffi.MAX_STAT_SEGMENTS == ops.MAX_STAT_SEGMENTS == 64
    assert int(re.search(r"#define VL_STAT_CHUNK (\d+)", src).group(1)) == _ffi.STAT_CHUNK == CHUNK
    assert CHUNK > 0 and CHUNK & (CHUNK - 1) == 0
    assert ctypes.sizeof(_ffi.TensorStat) == 64 == ops.STAT_ROW_BYTES == ops.STAT_DTYPE.itemsize and ctypes.sizeof(_ffi.StatSegment) == 16
    for f in ops.STAT_DTYPE.names:
        assert getattr(_ffi.TensorStat, f).offset == ops.STAT_DTYPE.fields[f][1], f


def test_chunk_plan_and_ws_bytes():
    lengths = [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5]
    segs, off = [], 3
    for n in lengths:
        segs.append((off, off + n))
        off += n + 1
    first, chunks = ops.stat_chunk_plan(segs)
    assert first == [0, 1, 2, 3, 5] and chunks == 8
    assert ops.tensor_stats_ws_bytes(segs) == 8 * 64
    for n, c in zip(lengths, [1, 1, 1, 2, 3]):
        assert ops.stat_chunk_plan([(7, 7 + n)]) == ([0], c) and ops.tensor_stats_ws_bytes([("x", 7, 7 + n)]) == 64 * c
    # more than one launch: the requirement is the largest over the slices of 64 entries, not their sum
    many = [(2 * k, 2 * k + 1) for k in range(64)] + [(1000, 1000 + 3 * CHUNK)]
    assert ops.stat_chunk_plan(many)[1] == 67 and ops.tensor_stats_ws_bytes(many) == 64 * 64
    assert ops.tensor_stats_ws_bytes(many[1:]) == 64 * 66
    for bad, what in (([(5, 5)], "segment 0"), ([(0, 4), (3, 8)], "segment 1"), ([(8, 9), (0, 4)], "segment 1"),
                      ([(0, 2 ** 32)], "2\\^32 - 1")):
        with pytest.raises(VltfError, match=what):
            ops.tensor_stats_ws_bytes(bad)
    with pytest.raises(VltfError, match="empty"):
        ops.tensor_stats_ws_bytes([])
    assert ops.tensor_stats_ws_bytes([(0, 2 ** 32 - 1)]) == 64 * (2 ** 32 // CHUNK)


# ---- derived keys ------------------------------------------------------------------------------------------------------------------
def row(g, w, g_nonfinite=0, w_nonfinite=0):
    """A vl_tensor_stat row computed by hand from short lists of finite values."""
    return dict(g_sum=sum(g), g_sumsq=sum(x * x for x in g), w_sum=sum(w), w_sumsq=sum(x * x for x in w),
                g_min=min(g, default=math.inf), g_max=max(g, default=-math.inf), w_min=min(w, default=math.inf),
                w_max=max(w, default=-math.inf), g_nonfinite=g_nonfinite, w_nonfinite=w_nonfinite, g_zero=sum(1 for x in g if x == 0))


def test_derived_keys_by_hand():
    segs = [("head_w", 0, 4), ("dcnn/fc6b", 4, 6), ("dead", 6, 9), ("allnan", 9, 11)]
    tiers = [(0, 4, 10.0), (4, 11, 1.0)]
    rows = [row([3.0, -4.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0]),         # |g| = 5, |w| = 2, two zeros of four
            row([0.5], [2.0, -2.0], g_nonfinite=1),                     # one NaN left out of a two-element gradient
            row([0.0, 0.0, 0.0], [0.0, 0.0, 0.0]),                      # weight_norm 0
            row([], [], g_nonfinite=2, w_nonfinite=2)]                  # no finite element at all
    ss = 25.0 + 0.25
    stats, mean = tensor_stats_report(segs, rows, tiers, lr=0.1, clip_norm=0.0, sumsq=ss)
    assert list(stats) == [s[0] for s in segs]
    a = stats["head_w"]
    assert a["grad_norm"] == 5.0 and a["weight_norm"] == 2.0 and a["grad_mean"] == -0.25 and a["weight_mean"] == 1.0
    assert a["grad_std"] == math.sqrt(25.0 / 4 - 0.0625) and a["weight_std"] == 0.0
    assert (a["grad_min"], a["grad_max"], a["weight_min"], a["weight_max"]) == (-4.0, 3.0, 1.0, 1.0)
    assert a["grad_zero_fraction"] == 0.5 and a["lr_mult"] == 10.0 and a["grad_nonfinite"] == 0 == a["weight_nonfinite"]
    assert a["sgd_update_ratio"] == pytest.approx(0.1 * 10.0 * 5.0 / 2.0, rel=1e-15)
    b = stats["dcnn/fc6b"]
    assert b["grad_nonfinite"] == 1 and b["grad_mean"] == 0.5 and b["grad_std"] == 0.0 and b["lr_mult"] == 1.0      # n = the finite count
    assert b["sgd_update_ratio"] == pytest.approx(0.1 * 0.5 / math.sqrt(8.0), rel=1e-15)
    c = stats["dead"]
    assert c["weight_norm"] == 0.0 and c["sgd_update_ratio"] is None and c["grad_zero_fraction"] == 1.0
    d = stats["allnan"]
    assert math.isnan(d["grad_mean"]) and math.isnan(d["weight_std"]) and d["grad_min"] == math.inf and d["grad_max"] == -math.inf
    assert d["grad_norm"] == 0.0 and d["sgd_update_ratio"] is None and d["grad_nonfinite"] == 2
    assert mean == pytest.approx((5.0 + 0.5 + 0.0 + 0.0) / 4, rel=1e-15)            # no clip: the plain mean of the norms
    # a clip that bites: every update and grads_norm_mean shrink by clip_norm / norm
    clipped, cmean = tensor_stats_report(segs, rows, tiers, lr=0.1, clip_norm=1.0, sumsq=ss)
    sc = 1.0 / math.sqrt(ss)
    assert clip_scale_of(ss, 1.0) == sc and clip_scale_of(ss, 0.0) == 1.0 and clip_scale_of(ss, 100.0) == 1.0
    assert cmean == pytest.approx(sc * mean, rel=1e-15)
    assert clipped["head_w"]["sgd_update_ratio"] == pytest.approx(sc * a["sgd_update_ratio"], rel=1e-15)
    assert clipped["head_w"]["grad_norm"] == 5.0                                     # the statistics see the gradient before the clip
    # a clip that does not bite changes nothing
    assert tensor_stats_report(segs, rows, tiers, lr=0.1, clip_norm=100.0, sumsq=ss)[1] == mean
    # the restatement the device tests use derives the same dict
    names = [s[0] for s in segs]
    wr = [dict(sum=r["w_sum"], sumsq=r["w_sumsq"], min=r["w_min"], max=r["w_max"], nonfinite=r["w_nonfinite"], n=hi - lo)
          for r, (_, lo, hi) in zip(rows, segs)]
    gr = [dict(sum=r["g_sum"], sumsq=r["g_sumsq"], min=r["g_min"], max=r["g_max"], nonfinite=r["g_nonfinite"], zero=r["g_zero"], n=hi - lo)
          for r, (_, lo, hi) in zip(rows, segs)]
    want, wmean = R.derived(names, list(zip(wr, gr)), [10.0, 1.0, 1.0, 1.0], 0.1, 1.0, ss)
    R.close_reports(clipped, want, {n: hi - lo for n, lo, hi in segs})
    assert wmean == pytest.approx(cmean, rel=1e-15)


def test_restatement_of_a_segment():
    """The numpy restatement itself on values whose answers are known: non-finite elements are counted and left out, a denormal is
    finite and not zero, -0 is zero, FLT_MAX squares to a finite float64."""
    flt_max, den = float(np.finfo(np.float32).max), float(np.float32(1e-42))
    x = np.array([1.0, np.nan, -2.0, np.inf, -np.inf, -0.0, 0.0, den, flt_max], np.float32)
    s = R.one_side(x)
    assert s["n"] == 9 and s["nonfinite"] == 3 and s["zero"] == 2 and s["min"] == -2.0 and s["max"] == flt_max
    assert s["sum"] == math.fsum([1.0, -2.0, den, flt_max]) and s["sumsq"] == math.fsum([1.0, 4.0, den * den, flt_max * flt_max])
    assert math.isfinite(s["sumsq"]) and s["sumsq"] > 1e76
    e = R.one_side(np.array([np.nan, np.inf], np.float32))
    assert (e["sum"], e["sumsq"], e["min"], e["max"], e["nonfinite"], e["zero"]) == (0.0, 0.0, math.inf, -math.inf, 2, 0)


# ---- the JSONL writer and the log lines --------------------------------------------------------------------------------------------
def result(nan_in=None):
    segs = [("a", 0, 2), ("b", 2, 4)]
    rows = [row([1.0, 2.0], [1.0, 1.0]), row([3.0], [0.0, 0.0], g_nonfinite=1) if nan_in else row([3.0, 0.0], [0.0, 0.0])]
    ss = float("nan") if nan_in else 14.0
    stats, mean = tensor_stats_report(segs, rows, [(0, 4, 1.0)], lr=0.01, clip_norm=0.0, sumsq=14.0)
    return dict(loss=1.0, grad_norm=math.sqrt(ss) if not nan_in else float("nan"), tensor_stats=stats, grads_norm_mean=mean)


def test_jsonl_writer_strict_json_append_and_rank(tmp_path):
    from vltf_amd.train import TensorStatsLog, json_safe
    log = TensorStatsLog(str(tmp_path), "run7", rank=0)
    assert log.path == os.path.join(str(tmp_path), "run7_tensor_stats.jsonl") and not os.path.exists(log.path)
    out = result()
    out["tensor_stats"]["b"]["grad_max"] = float("inf")
    out["tensor_stats"]["b"]["grad_min"] = float("-inf")
    out["tensor_stats"]["b"]["grad_mean"] = float("nan")
    log.write(3, 2, 0.01, 0.0, out)
    TensorStatsLog(str(tmp_path), "run7", rank=0).write(5, 4, 0.005, 0.0, result())       # a resumed run appends
    lines = open(log.path).read().splitlines()
    assert len(lines) == 2

    def strict(text):
        return json.loads(text, parse_constant=lambda c: pytest.fail("non-strict JSON constant %s" % c))
    first, second = strict(lines[0]), strict(lines[1])
    assert sorted(first) == ["clip_scale", "global_step", "grad_norm", "grads_norm_mean", "lr", "update", "vars"]
    assert (first["global_step"], first["update"], first["lr"], first["clip_scale"]) == (3, 2, 0.01, 1.0)
    assert (second["global_step"], second["update"]) == (5, 4)
    assert list(first["vars"]) == ["a", "b"] and first["vars"]["a"]["grad_norm"] == math.sqrt(5.0)
    b = first["vars"]["b"]
    assert (b["grad_max"], b["grad_min"], b["grad_mean"]) == ("inf", "-inf", "nan") and b["sgd_update_ratio"] is None
    assert first["grad_norm"] == pytest.approx(math.sqrt(14.0)) and second["vars"]["b"]["grad_max"] == 3.0
    # rank > 0 writes nothing
    other = TensorStatsLog(str(tmp_path / "r1"), "run7", rank=1)
    assert other.path is None and other.write(3, 2, 0.01, 0.0, result()) is None and not os.path.exists(str(tmp_path / "r1"))
    assert json_safe({"x": [np.float32("nan"), np.int64(3), 1.5, None, "s"]}) == {"x": ["nan", 3, 1.5, None, "s"]}


def test_log_lines_name_the_extremes_and_the_non_finite():
    from vltf_amd.train import tensor_stats_lines
    line, bad = tensor_stats_lines(result()["tensor_stats"])
    assert "largest" in line and "[a]" in line and bad is None          # b has weight_norm 0: no ratio, a is both extremes
    stats = result(nan_in=True)["tensor_stats"]
    stats["a"]["sgd_update_ratio"], stats["b"]["sgd_update_ratio"] = 0.5, 0.001
    line, bad = tensor_stats_lines(stats)
    assert re.search(r"largest 5\.000e-01 \[a\], smallest 1\.000e-03 \[b\]", line)
    assert bad is not None and "b (gradient 1, weights 0)" in bad and "a (" not in bad
