"""The multi-label mode on the host (network.label_type multiple): the float64 closed form of tests/multilabel_ref.py against
torch's binary_cross_entropy_with_logits, a central finite difference of its own loss and Lin et al.'s focal line; val.multilabel_metrics
against the brute-force AP (and sklearn where it is installed), the F1 corner cases and the chunked Validation path; balanced_pos_weights,
the YAML key, every refusal, the dp_scalars round trip and the C-ABI argument checks.  No GPU: no engine is constructed and nothing is
launched."""
import math
import os
import types

import numpy as np
import pytest
import torch
import yaml

from tests import multilabel_ref as ML
from tests.test_host_workflow import config, make_dataset
from vltf_amd import settings_
from vltf_amd._ffi import VltfError
from vltf_amd.engine import NetConfig, check_label_type

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def multi_hot(rng, b, c, density=0.2):
    y = (rng.random((b, c)) < density).astype(np.int32)
    y[0] = 0                                              # a row without labels is legal
    return y


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,c", [(5, 3), (7, 130), (8, 1000)])
@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "weights"])
def test_reference_is_torch_bce_with_logits_at_gamma_zero(b, c, weighted):
    rng = np.random.default_rng(b * c)
    z = (rng.standard_normal((b, c)) * 2).astype(np.float32)
    y = multi_hot(rng, b, c)
    q = rng.uniform(0.25, 4.0, c).astype(np.float32) if weighted else None
    for lam, eps in ((1.0, 0.0), (0.7, 0.1)):
        t = ML.targets(y, lam, eps)
        zt = torch.tensor(z.astype(np.float64), requires_grad=True)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(zt, torch.tensor(t), pos_weight=None if q is None else
                                                                    torch.tensor(q.astype(np.float64)), reduction="mean")
        loss.backward()
        got = ML.xent(z, y, q, 0.0, eps, lam)
        assert got["loss"] == pytest.approx(float(loss.detach()), rel=1e-12)
        np.testing.assert_allclose(got["dlogits"], zt.grad.numpy(), rtol=1e-12, atol=1e-12 * np.abs(zt.grad.numpy()).max())
        mean, d = ML.xent_mean(z, t, q, 0.0)
        assert mean == pytest.approx(float(loss.detach()), rel=1e-12) and np.array_equal(d, got["dlogits"])


@pytest.mark.parametrize("gamma", [0.5, 2.0])
def test_reference_gradient_is_the_finite_difference_of_its_loss(gamma):
    rng = np.random.default_rng(17)
    b, c, h = 6, 11, 1e-6
    z = rng.standard_normal((b, c)) * 2
    y = multi_hot(rng, b, c, 0.3)
    q = rng.uniform(0.25, 4.0, c).astype(np.float32)
    t = ML.targets(y, 0.7, 0.1)
    _, d = ML.elem_terms(z, t, q, gamma)
    lp, _ = ML.elem_terms(z + h, t, q, gamma)             # the elements do not couple: one shifted evaluation serves every element
    lm, _ = ML.elem_terms(z - h, t, q, gamma)
    np.testing.assert_allclose(d, (lp - lm) / (2 * h), rtol=1e-6, atol=1e-6 * np.abs(d).max())


def test_reference_on_one_hot_rows_is_lin_et_al():
    """gamma 2, q 1, hard labels: -(1 - p_t)^g log p_t summed over the classes, p_t = p where y = 1 and 1 - p where y = 0."""
    rng = np.random.default_rng(5)
    z = rng.standard_normal((9, 13)) * 2
    y = np.eye(13, dtype=np.int32)[rng.integers(0, 13, 9)]
    p = 1.0 / (1.0 + np.exp(-z))
    pt = np.where(y > 0, p, 1.0 - p)
    want = (-(1.0 - pt) ** 2.0 * np.log(pt)).sum(axis=1)
    l, _ = ML.elem_terms(z, y.astype(np.float64), None, 2.0)
    np.testing.assert_allclose(l.sum(axis=1), want, rtol=1e-12)


def test_reference_is_finite_at_the_ends_and_counts_hits():
    z = np.array([[120.0, -120.0, 0.0], [-120.0, 120.0, 0.0]])
    y = np.array([[1, 1, 0], [1, 1, 1]], np.int32)
    for gamma in (0.0, 0.5, 1.0, 2.0, 5.0):
        got = ML.xent(z, y, [1.0, 0.0, 2.0], gamma, 0.1)
        assert np.isfinite(got["row_losses"]).all() and np.isfinite(got["dlogits"]).all()
    got = ML.xent(np.array([[1.0, -1.0, 0.0], [1.0, 1.0, -1.0], [-1.0, -2.0, 0.0]]), np.array([[1, 0, 0], [0, 1, 0], [0, 0, 0]]))
    assert got["hit_rows"].tolist() == [True, False, False] and got["exact_rows"].tolist() == [True, False, True]


def test_reference_lengths_leave_dead_rows_out():
    rng = np.random.default_rng(4)
    z = (rng.standard_normal((6, 5)) * 2).astype(np.float32)
    y = multi_hot(rng, 6, 5, 0.4)
    live = np.array([1, 0, 1, 1, 0, 1], bool)
    zz = z.copy()
    zz[~live] = np.nan
    got, want = ML.xent(zz, y, None, 2.0, 0.1, live=live), ML.xent(z[live], y[live], None, 2.0, 0.1)
    assert got["rows"] == 4 and got["loss_sum"] == want["loss_sum"] and not got["dlogits"][~live].any()
    assert np.array_equal(got["dlogits"][live], want["dlogits"]) and got["hits"] == want["hits"] and got["exact"] == want["exact"]


# ---- metrics ---------------------------------------------------------------------------------------------------------------------------
def metric_case():
    """12 items, 5 classes: tied scores in every class (logits rounded to halves), class 3 without a positive, class 4 all positives."""
    rng = np.random.default_rng(8)
    z = np.round(rng.standard_normal((12, 5)) * 2) / 2
    y = (rng.random((12, 5)) < 0.4).astype(np.float32)
    y[:, 3], y[:, 4] = 0, 1
    y[0, :3] = 0
    assert any(len(set(z[:, c])) < 12 for c in range(5))
    return z.astype(np.float32), y


def test_metrics_agree_with_the_brute_force_reference():
    from vltf_amd.val import average_precision, multilabel_metrics
    z, y = metric_case()
    got, want = multilabel_metrics(z, y), ML.metrics_brute(z, y)
    assert math.isnan(got["ap"][3]) and math.isnan(want["ap"][3]) and got["ap"][4] == 1.0
    np.testing.assert_allclose(got["ap"][[0, 1, 2, 4]], want["ap"][[0, 1, 2, 4]], rtol=1e-12)
    for k in ("map", "f1_micro", "f1_macro", "hit1", "subset_accuracy"):
        assert got[k] == pytest.approx(want[k], rel=1e-12), k
    assert got["map"] == pytest.approx(np.mean(want["ap"][[0, 1, 2, 4]]), rel=1e-12) and got["positives"].tolist() == y.sum(axis=0).tolist()
    # a hand-made class: scores 1, 1, 0.5, -1 with positives 1, 0, 1, 0 -- thresholds 1 (P 1/2, R 1/2) and 0.5 (P 2/3, R 1)
    assert average_precision([1, 1, 0.5, -1], [1, 0, 1, 0]) == pytest.approx(0.5 * 0.5 + 0.5 * 2 / 3)
    assert ML.average_precision_brute([1, 1, 0.5, -1], [1, 0, 1, 0]) == pytest.approx(0.5 * 0.5 + 0.5 * 2 / 3)


def test_metrics_agree_with_sklearn_where_it_is_installed():
    skm = pytest.importorskip("sklearn.metrics")
    from vltf_amd.val import multilabel_metrics
    z, y = metric_case()
    got = multilabel_metrics(z, y)
    for c in (0, 1, 2, 4):
        assert got["ap"][c] == pytest.approx(skm.average_precision_score(y[:, c], z[:, c]), rel=1e-12)
    assert got["f1_micro"] == pytest.approx(skm.f1_score(y, z > 0, average="micro", zero_division=0), rel=1e-12)


def test_f1_with_an_empty_denominator_counts_as_zero():
    from vltf_amd.val import multilabel_metrics
    # class 0: no positive and no prediction (left out of macro); class 1: a positive never predicted (F1 0); class 2: perfect
    z = np.array([[-1.0, -1.0, 1.0], [-1.0, -2.0, -1.0]], np.float32)
    y = np.array([[0, 1, 1], [0, 0, 0]], np.float32)
    m = multilabel_metrics(z, y)
    assert m["f1_macro"] == pytest.approx(0.5) and m["f1_micro"] == pytest.approx(2 / 3) and m["subset_accuracy"] == 0.5 and m["hit1"] == 0.5
    m = multilabel_metrics(-np.ones((2, 3), np.float32), np.zeros((2, 3), np.float32))      # nothing positive, nothing predicted
    assert m["f1_micro"] == 0.0 and m["f1_macro"] == 0.0 and math.isnan(m["map"]) and m["subset_accuracy"] == 1.0 and m["hit1"] == 0.0
    assert multilabel_metrics(np.zeros((1, 2), np.float32), np.zeros((1, 2), np.float32))["subset_accuracy"] == 1.0   # z == 0: negative


def test_chunked_validation_equals_the_one_shot_call(tmp_path):
    from vltf_amd.defs_ import defs
    from vltf_amd.val import Validation, multilabel_metrics
    z, y = metric_case()
    settings = types.SimpleNamespace(num_classes=5, val=types.SimpleNamespace(logits_save_interval=5), run_folder=str(tmp_path),
                                     run_id="r", timestamp="t", label_type="multiple")
    val = Validation(settings)
    assert val.multilabel
    for i in range(12):
        val.apply_clip_fusion(z[i:i + 1], 1, y[i:i + 1], defs.fusion_method.avg)
        val.save_validation_logits_chunk()
    assert val.save_counter == 2 and len(val.item_logits) == 2
    want = multilabel_metrics(z, y)
    for step in range(2):                                  # two chunks on disk and two rows in memory, then all three on disk
        got = val.get_multilabel()
        for k in ("map", "f1_micro", "f1_macro", "hit1", "subset_accuracy"):
            assert got[k] == want[k], k
        assert np.array_equal(got["ap"], want["ap"], equal_nan=True)
        val.save_validation_logits_chunk(save_all=True)
    assert val.get_chunk_accuracy(z, y) == want["hit1"]    # the incremental line and accuracy_<run_id> report hit@1
    m = val.report_multilabel()
    for name in ("map", "f1_micro", "f1_macro", "subset_accuracy"):
        assert float(open(os.path.join(str(tmp_path), "%s_r" % name)).read()) == m[name] == want[name]
    lines = [l.split() for l in open(os.path.join(str(tmp_path), "ap_per_class_r")).read().splitlines()]
    assert [[int(l[0]), int(l[1])] for l in lines] == [[c, int(y[:, c].sum())] for c in range(5)]
    assert math.isnan(float(lines[3][2])) and [float(l[2]) for l in lines[:3]] == want["ap"][:3].tolist()
    single = Validation(types.SimpleNamespace(num_classes=5, val=settings.val, run_folder=str(tmp_path), run_id="r", timestamp="t"))
    assert not single.multilabel and single.get_chunk_accuracy(z, y) == np.mean(np.argmax(z, 1) == np.argmax(y, 1))


# ---- settings and refusals -------------------------------------------------------------------------------------------------------------
def test_balanced_pos_weights_on_a_hand_made_item_list():
    """q_c = (N - n_c) / n_c over ITEMS: a label repeated inside an item counts once, an absent class gets 1.0."""
    from vltf_amd.settings_ import balanced_class_weights, balanced_pos_weights
    items = [["0", "1"], ["0"], ["0", "2", "2"], ["1"], ["0"]]                  # n = 4, 2, 1, 0 of N = 5 items
    q, absent = balanced_pos_weights(items, 4)
    assert q == [1 / 4, 3 / 2, 4.0, 1.0] and absent == [3]
    assert balanced_pos_weights([[0], [0, 1]], 2) == ([0.0, 1.0], [])
    assert balanced_class_weights(items, 4)[0] == [8 / 16, 8 / 8, 8 / 8, 1.0]   # the single-label rule is what it was
    with pytest.raises(Exception, match="class_weights"):
        balanced_pos_weights([["4"]], 4)
    with pytest.raises(Exception, match="class_weights"):
        balanced_pos_weights([], 4)


def _settings(tmp_path, network=None, train=None, val=None, phase="train"):
    folder = str(tmp_path)
    data_path, _, _ = make_dataset(folder, "%s.txt" % phase)
    path = config(folder, data_path, phase=phase)
    with open(path) as f:
        cfg = yaml.safe_load(f)
    cfg["run"]["network"].update(network or {})
    cfg["run"]["train"].update(train or {})
    cfg["run"]["val"].update(val or {})
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    s = settings_.Settings()
    s.initialize(path)
    return s


@pytest.mark.parametrize("network,want", [({"label_type": "defs.label_type.multiple"}, "multiple"), ({"label_type": "multiple"}, "multiple"),
                                          ({"label_type": "defs.label_type.single"}, "single"), ({"label_type": "single"}, "single"),
                                          ({}, "single"), ({"label_type": None}, "single"), ({"label_type": "None"}, "single")])
def test_yaml_label_type_parses(tmp_path, network, want):
    assert _settings(tmp_path, network).label_type == want


@pytest.mark.parametrize("bad", ["many", "defs.label_type.many", "defs.phase.train", "Multiple", 2, True])
def test_yaml_label_type_refuses(tmp_path, bad):
    with pytest.raises(Exception, match="label_type|not defined|should be a child"):
        _settings(tmp_path, {"label_type": bad})


def test_yaml_balanced_weights_follow_the_label_type(tmp_path):
    s = _settings(tmp_path, {"label_type": "multiple"}, train={"class_weights": "balanced"})
    labels = s.feeder.get_dataset_by_tag("main")[0].labels
    want = settings_.balanced_pos_weights(labels, 4)[0]
    assert s.get_class_weights() == want and len(labels) == 5
    assert _settings(tmp_path, train={"class_weights": "balanced"}).get_class_weights() == settings_.balanced_class_weights(labels, 4)[0]


def test_yaml_refusals_with_multiple(tmp_path):
    multiple = {"label_type": "defs.label_type.multiple"}
    with pytest.raises(Exception, match="train.top_k"):
        _settings(tmp_path, multiple, train={"top_k": 3})
    with pytest.raises(Exception, match="val.top_k"):
        _settings(tmp_path, multiple, val={"top_k": 3}, phase="val")
    with pytest.raises(Exception, match="val.per_class"):
        _settings(tmp_path, multiple, val={"per_class": True}, phase="val")
    s = _settings(tmp_path, val={"per_class": True, "top_k": 3}, phase="val")      # single: both stay available
    assert s.val.per_class is True and s.val.top_k == 3 and s.label_type == "single"


def test_check_label_type():
    assert check_label_type(None) == "single" and check_label_type("single") == "single" and check_label_type("multiple") == "multiple"
    assert NetConfig().label_type == "single"
    for bad in ("many", "Multiple", "", 1, True, ["multiple"], b"multiple"):
        with pytest.raises(VltfError, match="label_type"):
            check_label_type(bad)


def test_composed_engine_refuses_multiple():
    """The check comes before anything touches a device."""
    from vltf_amd.composed import ComposedEngine, HeadConfig
    head = HeadConfig(in_dim=6, fpc=4, num_classes=9)
    with pytest.raises(VltfError, match="label_type multiple"):
        ComposedEngine(NetConfig(classifier="lstm", label_type="multiple"), head, max_clips=2, device="cpu")
    with pytest.raises(VltfError, match="label_type must be"):
        ComposedEngine(NetConfig(classifier="lstm", label_type="many"), head, max_clips=2, device="cpu")


def test_engine_loss_setup_refuses_top_k_and_a_bad_label_type():
    """LRCNEngine._loss_setup on a stand-in: the checks run before any allocation."""
    from vltf_amd.engine import LRCNEngine
    stub = types.SimpleNamespace(cfg=NetConfig(num_classes=4), training=True, dev="cpu")
    with pytest.raises(VltfError, match="top_k = 3 is refused with label_type multiple"):
        LRCNEngine._loss_setup(stub, 0.0, 3, 8, label_type="multiple")
    with pytest.raises(VltfError, match="label_type must be"):
        LRCNEngine._loss_setup(stub, 0.0, 0, 8, label_type="several")
    LRCNEngine._loss_setup(stub, 0.1, 0, 8, [1.0, 2.0, 0.5, 1.0], 2.0, label_type="multiple")        # (host tensors: dev is the CPU)
    assert stub.multilabel and stub.stats.numel() == 3 and stub.loss_rows.numel() == 24 and stub.class_weights_dev.dtype == torch.float32
    out = LRCNEngine._fetch_topk(stub, {}, np.array([1.0, 2.0, 3.0]), 4)
    assert out == {"subset_accuracy": 0.75, "subset_correct": 3.0}
    LRCNEngine._loss_setup(stub, 0.0, 0, 8)
    assert not stub.multilabel and stub.stats.numel() == 2 and LRCNEngine._fetch_topk(stub, {}, np.array([1.0, 2.0]), 4) == {}


def test_dp_scalars_round_trip_with_the_subset_count():
    from vltf_amd.train import dp_global, dp_scalars
    a = dict(loss_sum=3.0, correct=2.0, rows=4, subset_correct=1.0, loss=0.75, accuracy=0.5, subset_accuracy=0.25)
    b = dict(loss_sum=1.0, correct=1.0, rows=2, subset_correct=2.0, loss=0.5, accuracy=0.5, subset_accuracy=1.0)
    assert dp_scalars(a) == [3.0, 2.0, 4.0, 1.0]
    g = dp_global(a, np.add(dp_scalars(a), dp_scalars(b)))
    assert g["loss"] == 4 / 6 and g["accuracy"] == 3 / 6 and g["subset_accuracy"] == 3 / 6 and "topk_accuracy" not in g
    plain = dict(loss_sum=3.0, correct=2.0, rows=4)
    assert dp_scalars(plain) == [3.0, 2.0, 4.0] and set(dp_global(plain, [3.0, 2.0, 4.0])) == {"loss_sum", "correct", "rows", "loss", "accuracy"}
    k = dict(plain, topk_correct=3.0)
    assert dp_scalars(k) == [3.0, 2.0, 4.0, 3.0] and dp_global(k, dp_scalars(k))["topk_accuracy"] == 0.75


def test_example_yaml_is_the_lrcn_one_with_the_two_keys():
    here = os.path.join(ROOT, "examples")
    with open(os.path.join(here, "lrcn_multilabel.yml")) as f:
        multi = yaml.safe_load(f)
    with open(os.path.join(here, "lrcn_ucf101_shaped.yml")) as f:
        base = yaml.safe_load(f)
    assert multi["run"]["network"].pop("label_type") == "defs.label_type.multiple" and multi["run"]["train"].pop("class_weights") == "balanced"
    for cfg in (multi, base):
        cfg["run"].pop("run_folder", None), cfg["run"].pop("run_id", None)
    assert multi == base


# ---- C-ABI -----------------------------------------------------------------------------------------------------------------------------
def test_ffi_refusals_need_no_device():
    """The entry point validates before it launches: null pointers, sizes, smoothing, lam, gamma, the T rule, partial clips, lengths with
    mixed labels.  Nothing runs."""
    from vltf_amd import _ffi
    p, i32, f32 = _ffi.p, _ffi.i32, _ffi.f32
    assert _ffi.SIGNATURES["vl_sigmoid_xent"] == (i32, [p, p, p, p, p, i32, i32, f32, p, i32, i32, f32, f32, p, p, f32, p])
    lib = _ffi.lib()
    fake = 4096                                  # a non-null, aligned address: validation fails before anything dereferences it
    ok = dict(logits=fake, labels=fake, stats=fake, batch=4, classes=7, seq_len=None, T=1, rpc=1, eps=0.1, lam=1.0, lam_dev=None, gamma=2.0)
    bad = [dict(logits=None), dict(labels=None), dict(stats=None), dict(batch=0), dict(classes=0), dict(eps=-0.1), dict(eps=1.0),
           dict(eps=math.nan), dict(lam=1.5), dict(lam=-0.1), dict(lam=math.nan), dict(gamma=-1.0), dict(gamma=math.nan),
           dict(gamma=math.inf), dict(rpc=0), dict(rpc=3), dict(seq_len=fake, T=3), dict(seq_len=fake, T=0),
           dict(seq_len=fake, T=2, rpc=2), dict(seq_len=fake, T=2, lam=0.7), dict(seq_len=fake, T=2, lam_dev=fake)]
    for over in bad:
        a = dict(ok, **over)
        rc = lib.vl_sigmoid_xent(a["logits"], a["labels"], None, a["stats"], None, a["batch"], a["classes"], 1.0, a["seq_len"], a["T"],
                                 a["rpc"], a["eps"], a["lam"], a["lam_dev"], None, a["gamma"], None)
        assert rc != 0, over
        assert b"vl_sigmoid_xent" in lib.vl_last_error()
