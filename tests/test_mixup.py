"""Mixup on the host: check_mixup, the YAML keys with their refusals and the getter outside the train phase, the draws of
mixup_lambda, the identities of the float64 reference (tests/mixup_ref.py), the C-ABI rows and the entry points' argument checks, the
example, and the refusals of GraphEngine and run_task ahead of any device call.  No GPU: nothing is launched."""
import math
import os
import re

import numpy as np
import pytest
import yaml

from oracle import lrcn_oracle as O
from tests import label_smoothing_ref as LS
from tests import mixup_ref as MX
from tests.test_ema import _val_settings
from tests.test_finetune import _settings
from vltf_amd._ffi import VltfError
from vltf_amd.engine import NetConfig, check_mixup, fold_lambda, mixup_lambda

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- check_mixup ------------------------------------------------------------------------------------------------------------------------
def test_check_mixup_accepts():
    assert check_mixup(None, None) == (0.0, 0) and check_mixup(None) == (0.0, 0) and check_mixup(0, 0) == (0.0, 0)
    assert check_mixup(0.2, 7) == (0.2, 7) and check_mixup(1, None) == (1.0, 0) and check_mixup(np.float32(0.5), np.int64(3)) == (0.5, 3)
    assert check_mixup(2.0, 5.0) == (2.0, 5) and check_mixup(0.2, 2 ** 64 - 1) == (0.2, 2 ** 64 - 1)
    a, s = check_mixup(1, 2.0)
    assert isinstance(a, float) and isinstance(s, int)
    assert NetConfig().mixup_alpha == 0.0 and NetConfig().mixup_seed == 0


@pytest.mark.parametrize("bad", [-0.1, float("nan"), float("inf"), -float("inf"), True, False, "0.2", b"0.2", [0.2], np.bool_(True)])
def test_check_mixup_refuses_alpha(bad):
    with pytest.raises(VltfError, match="mixup_alpha") as ex:
        check_mixup(bad, 0)
    assert repr(bad) in str(ex.value)


@pytest.mark.parametrize("bad", [-1, 2.5, float("nan"), float("inf"), True, False, "7", b"7", [7], np.bool_(True), 2 ** 64])
def test_check_mixup_refuses_seed(bad):
    with pytest.raises(VltfError, match="mixup_seed") as ex:
        check_mixup(0.2, bad)
    assert repr(bad) in str(ex.value)


@pytest.mark.parametrize("alpha", [None, 0, 0.0])
def test_check_mixup_refuses_a_seed_without_alpha(alpha):
    with pytest.raises(VltfError, match="mixup_seed 7 is given without mixup_alpha"):
        check_mixup(alpha, 7)


# ---- YAML -------------------------------------------------------------------------------------------------------------------------------
def test_settings_keys_parse(tmp_path):
    s = _settings(tmp_path, train={"mixup_alpha": 0.2, "mixup_seed": 7})
    assert (s.train.mixup_alpha, s.train.mixup_seed) == (0.2, 7) and s.get_mixup() == (0.2, 7)
    assert isinstance(s.train.mixup_alpha, float) and isinstance(s.train.mixup_seed, int)
    s = _settings(tmp_path, train={"mixup_alpha": "2e-1", "mixup_seed": "7"})           # quoted numbers (YAML reads 2e-1 as a string)
    assert s.get_mixup() == (0.2, 7)
    assert _settings(tmp_path, train={"mixup_alpha": 1}).get_mixup() == (1.0, 0)


@pytest.mark.parametrize("train", [{}, {"mixup_alpha": None, "mixup_seed": None}, {"mixup_alpha": "None", "mixup_seed": "None"},
                                   {"mixup_alpha": 0, "mixup_seed": 0}, {"mixup_alpha": "None"}], ids=["absent", "null", "None-strings", "zeros", "None-alpha"])
def test_settings_absent_keys_mean_off(tmp_path, train):
    s = _settings(tmp_path, train=train)
    assert (s.train.mixup_alpha, s.train.mixup_seed) == (0.0, 0) and s.get_mixup() == (0.0, 0)


@pytest.mark.parametrize("train", [{"mixup_alpha": -0.2}, {"mixup_alpha": "nan"}, {"mixup_alpha": "inf"}, {"mixup_alpha": "much"},
                                   {"mixup_alpha": True}, {"mixup_seed": 7}, {"mixup_alpha": "None", "mixup_seed": 7},
                                   {"mixup_alpha": 0.2, "mixup_seed": -1}, {"mixup_alpha": 0.2, "mixup_seed": 1.5},
                                   {"mixup_alpha": 0.2, "mixup_seed": "seven"}, {"mixup_alpha": 0.2, "mixup_seed": True}])
def test_settings_refusals(tmp_path, train):
    with pytest.raises(Exception, match="train.mixup_alpha / train.mixup_seed"):
        _settings(tmp_path, train=train)


def test_settings_outside_the_train_phase_is_off(tmp_path):
    s = _val_settings(tmp_path, train={"mixup_alpha": 0.2, "mixup_seed": 7})
    assert s.get_mixup() == (0.0, 0)


def test_example_yaml_is_the_label_smoothing_one_with_the_two_keys(tmp_path):
    here = os.path.join(ROOT, "examples")
    with open(os.path.join(here, "lrcn_mixup.yml")) as f:
        mix = yaml.safe_load(f)
    with open(os.path.join(here, "lrcn_label_smoothing.yml")) as f:
        base = yaml.safe_load(f)
    assert mix["run"]["train"].pop("mixup_alpha") == 0.2 and mix["run"]["train"].pop("mixup_seed") == 7
    for cfg in (mix, base):
        cfg["run"].pop("run_folder", None), cfg["run"].pop("run_id", None)
    assert mix == base
    assert _settings(tmp_path, train={"mixup_alpha": 0.2, "mixup_seed": 7, "label_smoothing": 0.1, "top_k": 5}).get_mixup() == (0.2, 7)


# ---- the draws --------------------------------------------------------------------------------------------------------------------------
def test_fold_lambda():
    assert fold_lambda(0.3) == 0.7 and fold_lambda(0.7) == 0.7 and fold_lambda(0) == 1.0 and fold_lambda(1) == 1.0 and fold_lambda(0.5) == 0.5
    for bad in (-0.1, 1.1, float("nan"), float("inf"), True, "0.5", None):
        with pytest.raises(VltfError, match="mix_lambda"):
            fold_lambda(bad)


def test_mixup_lambda_is_a_pure_function_of_its_arguments():
    draws = [mixup_lambda(0.2, 7, i) for i in range(64)]
    assert all(0.5 <= l <= 1.0 for l in draws)
    assert draws == [mixup_lambda(0.2, 7, i) for i in range(64)]                         # equal for equal (alpha, seed, index)
    assert len(set(draws)) == 64                                                         # differs across indices
    other = [mixup_lambda(0.2, 8, i) for i in range(64)]
    assert all(a != b for a, b in zip(draws, other))                                     # and across seeds
    assert mixup_lambda(0.2, 7, 5) != mixup_lambda(0.4, 7, 5)
    assert mixup_lambda(0.0, 0, 3) == 1.0 and mixup_lambda(None, None, 3) == 1.0         # off: nothing is mixed
    assert mixup_lambda(0.2, 7, 2 ** 40) == mixup_lambda(0.2, 7, 2 ** 40)                # a draw index past 32 bits is a key like any other
    with pytest.raises(VltfError, match="mixup_alpha"):
        mixup_lambda(-1.0, 0, 0)


def test_mixup_lambda_distribution():
    """alpha = 1: Beta(1, 1) is uniform, the folded uniform on [0.5, 1] has mean 0.75 and sigma 0.25 / sqrt(3) = 0.1443; the mean of 4096
    draws lies within 5 sigma / sqrt(4096) = 0.0113 of it.  The draws are a function of (alpha, seed, index): this cannot flake.
    alpha = 0.2 is U-shaped: its folded mean is higher."""
    one = np.array([mixup_lambda(1.0, 7, i) for i in range(4096)])
    small = np.array([mixup_lambda(0.2, 7, i) for i in range(4096)])
    print("alpha 1: mean %.5f sigma %.5f; alpha 0.2: mean %.5f" % (one.mean(), one.std(), small.mean()))
    assert abs(one.mean() - 0.75) <= 0.0113
    assert abs(one.std() - 0.1443) < 0.01
    assert small.mean() > one.mean()
    assert one.min() >= 0.5 and one.max() <= 1.0 and small.min() >= 0.5 and small.max() <= 1.0


# ---- the reference's identities, float64 to 1e-12 -----------------------------------------------------------------------------------------
def _case(b, c, seed=0):
    rng = np.random.default_rng(b * c + seed)
    z = (rng.standard_normal((b, c)) * 2).astype(np.float32)
    return z, O.labels_to_one_hot([[l] for l in rng.integers(0, c, b)], c)


@pytest.mark.parametrize("b,c,rpc", [(5, 7, 1), (4, 64, 2), (6, 101, 2), (9, 101, 3)])
@pytest.mark.parametrize("lam", [0.5, 0.8, 1.0])
def test_reference_loss_is_the_weighted_sum_of_the_two_hard_losses(b, c, rpc, lam):
    z, onehot = _case(b, c)
    l = MX.lam32(lam)
    pr = MX.partner_rows(b, rpc)
    assert np.array_equal(pr[pr], np.arange(b))                                          # an involution
    for eps in (0.0, 0.1):
        own = MX.row_losses(z, LS.smooth(onehot, eps))
        partner = MX.row_losses(z, LS.smooth(onehot[pr], eps))
        mixed = MX.row_losses(z, MX.targets(onehot, lam, eps, rpc))
        assert np.abs(mixed - (l * own + (1.0 - l) * partner)).max() < 1e-12
        want = MX.xent(z, onehot, lam, eps, 2, rpc)
        assert abs(want["loss"] - mixed.mean()) < 1e-12 and abs(want["loss_sum"] - mixed.sum()) < 1e-12
        assert np.abs(MX.targets(onehot, lam, eps, rpc).sum(axis=1) - 1.0).max() < 1e-12
        # hits are those of the row's own label, whatever lam
        ls = LS.xent(z, onehot, eps, 2)
        assert want["hits"] == ls["hits"] and want["topk"] == ls["topk"]


@pytest.mark.parametrize("b,c,rpc", [(5, 7, 1), (4, 64, 2), (9, 101, 3)])
def test_reference_at_lambda_one_is_the_label_smoothing_reference(b, c, rpc):
    z, onehot = _case(b, c, 1)
    for eps in (0.0, 0.1):
        got, want = MX.xent(z, onehot, 1.0, eps, 5, rpc), LS.xent(z, onehot, eps, 5)
        assert abs(got["loss"] - want["loss"]) < 1e-12 and np.abs(got["dlogits"] - want["dlogits"]).max() < 1e-12
        assert (got["hits"], got["topk"]) == (want["hits"], want["topk"])
        assert np.array_equal(MX.targets(onehot, 1.0, eps, rpc), LS.smooth(onehot, eps))


@pytest.mark.parametrize("clips", [1, 2, 3, 4, 5])
def test_reference_blend_is_a_symmetric_pair(clips):
    rng = np.random.default_rng(clips)
    x = rng.standard_normal((clips, 11)) * 64
    for lam in (0.5, 0.7310586, 1.0):
        l = MX.lam32(lam)
        y = MX.blend(x, lam)
        assert np.abs(y[::-1] - MX.blend(x[::-1], lam)).max() < 1e-12                     # blending the mirrored batch mirrors the result
        assert np.abs((y + y[::-1]) - (x + x[::-1])).max() < 1e-12                        # a pair's sum is kept
        assert np.abs((y - y[::-1]) - (2 * l - 1) * (x - x[::-1])).max() < 1e-12          # its difference shrinks by 2 lam - 1
        if clips % 2:
            assert np.array_equal(y[clips // 2], x[clips // 2])                           # the middle clip: bit for bit
    assert np.array_equal(MX.blend(x, 1.0), x)
    assert np.abs(MX.blend(x, 0.5) - MX.blend(x, 0.5)[::-1]).max() < 1e-12                # lam = 0.5: both partners become the mean


def test_reference_bf16_rounding_is_to_nearest_even():
    import torch
    rng = np.random.default_rng(3)
    x = np.concatenate([(rng.standard_normal(4096) * 64).astype(np.float32),
                        np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 0.0, 255.5, 3.0e38], np.float32)])   # ties: up to even, down to even
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(MX.bf16_bits(x), want)
    assert np.array_equal(MX.bf16_value(want), torch.from_numpy(x).to(torch.bfloat16).to(torch.float64).numpy())
    assert MX.bf16_ulp(1.0) == 2.0 ** -7 and MX.bf16_ulp(1.99) == 2.0 ** -7 and MX.bf16_ulp(-64.0) == 0.5
    assert np.abs(MX.bf16_round(x[:4096]) - x[:4096].astype(np.float64)).max() <= 0.5 * MX.bf16_ulp(np.abs(x[:4096]).max())


# ---- C-ABI ------------------------------------------------------------------------------------------------------------------------------
def _header_arg_count(name):
    with open(os.path.join(ROOT, "include", "vltf.h")) as f:
        text = f.read()
    m = re.search(r"\bint %s\(([^;]*?)\);" % name, text, re.S)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_ffi_rows_have_the_headers_argument_counts():
    """The two new entry points, and vl_fill, which writes the blend weight to the device word both of them read."""
    from vltf_amd import _ffi
    p, i32, i64, f32 = _ffi.p, _ffi.i32, _ffi.i64, _ffi.f32
    assert _ffi.SIGNATURES["vl_mixup_pairs"] == (i32, [p, i32, i32, i64, f32, p, p])
    assert _ffi.SIGNATURES["vl_softmax_xent_mix"] == (i32, [p, p, p, p, p, i32, i32, f32, i32, f32, i32, f32, p, p])
    for name in ("vl_mixup_pairs", "vl_softmax_xent_mix", "vl_fill"):
        assert len(_ffi.SIGNATURES[name][1]) == _header_arg_count(name), name
    assert _ffi.SIGNATURES["vl_softmax_xent_ls"] == (i32, [p, p, p, p, p, i32, i32, f32, p, i32, f32, i32, p])     # as it was
    import vltf_amd.ops as ops
    assert callable(ops.mixup_pairs) and callable(ops.softmax_xent_mix)


def test_host_refusals_need_no_device():
    """Both entry points validate before they launch, each refusal with a message of its own.  Nothing runs."""
    from vltf_amd import _ffi
    lib = _ffi.lib()
    fake = 4096                                  # a non-null, aligned address: validation fails before anything dereferences it
    for args, msg in (((None, 0, 2, 8, 0.5, None), b"x is null"), ((fake, 0, -1, 8, 0.5, None), b"clips must be >= 0"),
                      ((fake, 0, 2, 0, 0.5, None), b"clip_elems must be > 0"), ((fake, 0, 2, -8, 0.5, None), b"clip_elems must be > 0"),
                      ((fake, 2, 2, 8, 0.5, None), b"dtype must be 0"), ((fake, -1, 2, 8, 0.5, None), b"dtype must be 0"),
                      ((fake, 1, 2, 12, 0.5, None), b"no multiple of 8"), ((fake, 0, 2, 8, -0.1, None), b"lam must lie in [0, 1]"),
                      ((fake, 0, 2, 8, 1.5, None), b"lam must lie in [0, 1]"), ((fake, 0, 2, 8, math.nan, None), b"lam must lie in [0, 1]"),
                      ((fake, 0, 2, 8, math.inf, None), b"lam must lie in [0, 1]")):
        assert lib.vl_mixup_pairs(*args, None) != 0, args
        err = lib.vl_last_error()
        assert b"vl_mixup_pairs" in err and msg in err, (args, err)
    assert lib.vl_mixup_pairs(fake, 0, 1, 8, 0.5, None, None) == 0 and lib.vl_mixup_pairs(fake, 0, 0, 8, 0.5, None, None) == 0   # nothing to pair
    ok = dict(logits=fake, labels=fake, stats=fake, batch=4, classes=7, rpc=1, eps=0.1, k=2, lam=0.5)
    for change, msg in ((dict(logits=None), b"bad argument"), (dict(labels=None), b"bad argument"), (dict(stats=None), b"bad argument"),
                        (dict(batch=0), b"bad argument"), (dict(classes=0), b"bad argument"), (dict(rpc=0), b"whole clips"),
                        (dict(rpc=3), b"whole clips"), (dict(eps=-0.1), b"smoothing"), (dict(eps=1.0), b"smoothing"),
                        (dict(eps=math.nan), b"smoothing"), (dict(k=-1), b"top_k"), (dict(lam=-0.1), b"lam must lie in [0, 1]"),
                        (dict(lam=1.5), b"lam must lie in [0, 1]"), (dict(lam=math.nan), b"lam must lie in [0, 1]")):
        a = dict(ok, **change)
        assert lib.vl_softmax_xent_mix(a["logits"], a["labels"], None, a["stats"], None, a["batch"], a["classes"], 1.0, a["rpc"], a["eps"],
                                       a["k"], a["lam"], None, None) != 0, change
        err = lib.vl_last_error()
        assert b"vl_softmax_xent_mix" in err and msg in err, (change, err)


# ---- GraphEngine / run_task: refused before any device call ---------------------------------------------------------------------------------
class _NoOps:
    def __getattr__(self, name):
        raise AssertionError("ops.%s was reached before mixup was refused" % name)


def test_graph_engine_refuses_mixup(monkeypatch):
    from tests import graph_cases as GC
    from vltf_amd import graph
    case = GC.encdec()
    pipes, ds = GC.specs_and_datasets(case, None)
    monkeypatch.setattr(graph, "ops", _NoOps())
    monkeypatch.setattr(graph.torch, "zeros", lambda *a, **k: pytest.fail("a buffer was allocated"))
    with pytest.raises(VltfError, match="mixup_alpha = 0.2 is refused by GraphEngine.*single-pipeline"):
        graph.GraphEngine(pipes, ds, case["V"], device="cuda:0", mixup_alpha=0.2)
    with pytest.raises(VltfError, match="mixup_alpha"):
        graph.GraphEngine(pipes, ds, case["V"], device="cuda:0", mixup_alpha=-1.0)


def test_run_task_refuses_mixup_on_a_multi_pipeline_model(tmp_path, monkeypatch):
    from tests import test_run_task_graph_gpu as TS
    from vltf_amd import graph, run_task
    folder = str(tmp_path)
    rpath, _, _ = TS.make_dataset(folder, "rgb.txt", nvid=5, cpv=TS.CPV, shape=TS.RAW, classes=TS.V, seed=7)
    fpath, _, _ = TS.make_dataset(folder, "flow.txt", nvid=5, cpv=TS.CPV, shape=TS.RAW, classes=TS.V, seed=8)
    path = TS.write_two_stream_cfg(folder, "ts.yml", rpath, fpath, "train")
    with open(path) as f:
        cfg = yaml.safe_load(f)
    cfg["run"]["train"].update(mixup_alpha=0.2, mixup_seed=7)
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    monkeypatch.setattr(graph, "GraphEngine", lambda *a, **k: pytest.fail("an engine was built"))
    monkeypatch.setattr(run_task, "LRCNEngine", lambda *a, **k: pytest.fail("an engine was built"))
    monkeypatch.setattr(run_task, "graph_config", lambda *a, **k: pytest.fail("the graph was configured"))
    with pytest.raises(Exception, match="train.mixup_alpha is refused for this model.*single-pipeline"):
        run_task.main(path, seed=3)
