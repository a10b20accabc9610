"""Class weights and the focal loss on the host: the float64 closed form of tests/focal_ref.py against torch's fp64 autograd
of the loss line, the saturated limit, a zero-weight label, check_class_weights / check_focal_gamma, the YAML keys (a list, `balanced`
with the numbers it yields on a hand-made item list, off when absent and outside the train phase), and val.per_class on hand-made
logits over two chunks.  No GPU: no engine is constructed and nothing is launched."""
import math
import os
import types

import numpy as np
import pytest
import torch
import yaml

from oracle import lrcn_oracle as O
from tests import focal_ref as FR
from tests import mixup_ref as MX
from tests.test_ema import _val_settings
from tests.test_finetune import _settings
from vltf_amd._ffi import VltfError
from vltf_amd.engine import NetConfig, check_class_weights, check_focal_gamma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMAS = [0.0, 0.5, 1.0, 2.0, 5.0]


def labels_of(kind, rng, b, c):
    """-> (int label matrix, lam, eps): hard one-hot | smoothed | mixed with the mirrored row and smoothed | multi-hot (two labels a row)"""
    onehot = O.labels_to_one_hot([[l] for l in rng.integers(0, c, b)], c)
    if kind == "multi-hot":
        onehot = O.labels_to_one_hot([list(rng.choice(c, 2, replace=False)) for _ in range(b)], c)
    return onehot, (0.7 if kind == "mixed" else 1.0), (0.1 if kind in ("smoothed", "mixed") else 0.0)


def autograd(z, y, w, gamma):
    """The loss line in torch float64 and its gradient: sum_r sum_c w_c y'_c (1 - p_c)^gamma (-log p_c)."""
    zt = torch.tensor(np.asarray(z, np.float64), requires_grad=True)
    lp = torch.log_softmax(zt, dim=1)
    m = (1.0 - lp.exp()) ** gamma if gamma != 0.0 else torch.ones_like(lp)
    rows = (torch.tensor(w)[None, :] * torch.tensor(y) * m * -lp).sum(dim=1)
    rows.sum().backward()
    return rows.detach().numpy(), zt.grad.numpy()


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,c", [(5, 3), (7, 130), (64, 101), (8, 1000)])
@pytest.mark.parametrize("kind", ["hard", "smoothed", "mixed", "multi-hot"])
@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "weights"])
def test_reference_is_autograd_of_the_loss_line(b, c, kind, weighted):
    rng = np.random.default_rng(b * c + len(kind))
    z = (rng.standard_normal((b, c)) * 2).astype(np.float32)
    onehot, lam, eps = labels_of(kind, rng, b, c)
    w = rng.uniform(0.25, 4.0, c).astype(np.float32) if weighted else None
    y = MX.targets(onehot, lam, eps)
    for gamma in GAMMAS:
        rl, d, p = FR.row_terms(z, y, w, gamma)
        keep = ~(p == 1.0).any(axis=1)                    # a saturated row: autograd gives NaN for 0 < gamma < 1 (none at these logits)
        assert keep.all()
        want_rl, want_d = autograd(z, y, FR.weights32(w, c), gamma)
        np.testing.assert_allclose(rl[keep], want_rl[keep], rtol=1e-10, atol=0)
        np.testing.assert_allclose(d[keep], want_d[keep], rtol=1e-10, atol=1e-10 * np.abs(want_d).max())
        full = FR.xent(z, onehot, w, gamma, eps, 3, lam)
        assert full["rows"] == b and np.allclose(full["dlogits"] * b, d, rtol=1e-15, atol=0)
        assert full["loss"] == pytest.approx(rl.sum() / b, rel=1e-15)
        # ones and gamma 0: the project's plain loss on the same labels -- where a label row sums to 1.  (TF's registered backprop
        # softmax - labels, which the plain launches keep, is the gradient only then; p A - a is the gradient of a multi-hot row too.)
        if gamma == 0.0 and not weighted and kind != "multi-hot":
            loss, dl = O.softmax_xent_mean(z, y)
            assert full["loss"] == pytest.approx(loss, rel=1e-12) and np.abs(full["dlogits"] - dl).max() < 1e-14


def test_saturated_rows_are_left_out_of_the_autograd_comparison_only():
    """One logit 120 above the rest: p_t == 1 in float64.  Autograd is NaN for 0 < gamma < 1; the closed form is finite and about 0."""
    z = np.zeros((3, 9), np.float32)
    z[0, 4] = z[1, 0] = z[2, 8] = 120.0
    onehot = O.labels_to_one_hot([[4], [0], [8]], 9)
    w = np.linspace(0.5, 2.0, 9).astype(np.float32)
    _, want_d = autograd(z, onehot.astype(np.float64), FR.weights32(w, 9), 0.5)
    assert np.isnan(want_d).any()
    for gamma in GAMMAS:
        for eps in (0.0, 0.1):
            got = FR.xent(z, onehot, w, gamma, eps)
            assert np.isfinite(got["row_losses"]).all() and np.isfinite(got["dlogits"]).all()
            if eps == 0.0:                                # the label is the saturated class: loss and gradient vanish
                assert np.abs(got["row_losses"]).max() < 1e-40 and np.abs(got["dlogits"]).max() < 1e-40


def test_zero_weight_label_gives_no_loss_and_no_gradient():
    rng = np.random.default_rng(3)
    z = (rng.standard_normal((4, 7)) * 2).astype(np.float32)
    onehot = O.labels_to_one_hot([[2], [5], [2], [0]], 7)
    w = np.ones(7, np.float32)
    w[2] = 0.0
    for gamma in GAMMAS:
        got = FR.xent(z, onehot, w, gamma)
        assert not got["row_losses"][[0, 2]].any() and not got["dlogits"][[0, 2]].any()
        assert (got["row_losses"][[1, 3]] > 0).all() and got["dlogits"][[1, 3]].any(axis=1).all()


def test_lengths_leave_dead_rows_out():
    rng = np.random.default_rng(4)
    z = (rng.standard_normal((6, 5)) * 2).astype(np.float32)
    onehot = O.labels_to_one_hot([[l] for l in rng.integers(0, 5, 6)], 5)
    live = np.array([1, 0, 1, 1, 0, 1], bool)
    zz = z.copy()
    zz[~live] = np.nan
    got, want = FR.xent(zz, onehot, None, 2.0, 0.1, 2, live=live), FR.xent(z[live], onehot[live], None, 2.0, 0.1, 2)
    assert got["rows"] == 4 and got["loss_sum"] == want["loss_sum"] and not got["dlogits"][~live].any()
    assert np.array_equal(got["dlogits"][live], want["dlogits"]) and got["topk"] == want["topk"] and got["hits"] == want["hits"]


# ---- check_class_weights / check_focal_gamma ---------------------------------------------------------------------------------------------
def test_checks_accept():
    assert check_class_weights(None, 3) is None and check_focal_gamma(None) == 0.0 and check_focal_gamma(0) == 0.0
    w = check_class_weights([1, 2.5, 0], 3)
    assert w.dtype == np.float32 and w.tolist() == [1.0, 2.5, 0.0]
    assert check_class_weights(np.array([0.5, 0.5], np.float64), 2).tolist() == [0.5, 0.5]
    assert check_class_weights((np.float32(2), np.int64(1)), 2).tolist() == [2.0, 1.0]
    assert check_focal_gamma(2) == 2.0 and isinstance(check_focal_gamma(2), float) and check_focal_gamma(np.float32(0.5)) == 0.5
    assert NetConfig().class_weights is None and NetConfig().focal_gamma == 0.0


@pytest.mark.parametrize("bad", [[1, 2], [1, 2, 3, 4], [1, -1, 1], [1, float("nan"), 1], [1, float("inf"), 1], [0, 0, 0], [1, "2", 1],
                                 [1, True, 1], "balanced", 1.0, [1, 1e39, 1], [1, None, 1]])
def test_check_class_weights_refuses(bad):
    with pytest.raises(VltfError, match="class_weights"):
        check_class_weights(bad, 3)


@pytest.mark.parametrize("bad", [-0.1, float("nan"), float("inf"), -float("inf"), True, "2", [2], np.bool_(False), 1e39])
def test_check_focal_gamma_refuses(bad):
    with pytest.raises(VltfError, match="focal_gamma") as ex:
        check_focal_gamma(bad)
    assert repr(bad) in str(ex.value)


# ---- YAML ------------------------------------------------------------------------------------------------------------------------------
def test_settings_keys_parse(tmp_path):
    s = _settings(tmp_path, train={"class_weights": [1, 2.5, 1, 0.5], "focal_gamma": 2.0})
    assert s.get_class_weights() == [1.0, 2.5, 1.0, 0.5] and s.get_focal_gamma() == 2.0 and isinstance(s.get_focal_gamma(), float)
    s = _settings(tmp_path, train={"class_weights": ["1", "2.5", 1, "5e-1"], "focal_gamma": "2"})        # quoted numbers
    assert s.get_class_weights() == [1.0, 2.5, 1.0, 0.5] and s.get_focal_gamma() == 2.0
    s = _settings(tmp_path, train={"class_weights": "[1, 2.5, 1, 0.5]"})
    assert s.get_class_weights() == [1.0, 2.5, 1.0, 0.5] and s.get_focal_gamma() == 0.0
    s = _settings(tmp_path, train={"focal_gamma": 0.5})
    assert s.get_class_weights() is None and s.get_focal_gamma() == 0.5


def test_balanced_weights_on_a_hand_made_item_list(tmp_path):
    """sklearn's rule, w_c = N / (C n_c), with an absent class at 1.0."""
    from vltf_amd.settings_ import balanced_class_weights
    items = [["0"], ["0"], ["0"], ["2"], ["1"], ["0"], ["2", "1"]]          # counts 4, 2, 2, 0 of N = 8 labels, C = 4
    w, absent = balanced_class_weights(items, 4)
    assert w == [8 / 16, 8 / 8, 8 / 8, 1.0] and absent == [3]
    w, absent = balanced_class_weights([[0], [1], [1]], 2)
    assert w == [3 / 2, 3 / 4] and absent == []
    with pytest.raises(Exception, match="class_weights"):
        balanced_class_weights([["4"]], 4)
    with pytest.raises(Exception, match="class_weights"):
        balanced_class_weights([], 4)
    # through the YAML: the labels of the synthetic training list (tests/test_host_workflow.py::make_dataset)
    s = _settings(tmp_path, train={"class_weights": "balanced", "focal_gamma": 2})
    labels = s.feeder.get_dataset_by_tag("main")[0].labels
    counts = np.bincount([int(l[0]) for l in labels], minlength=4)
    want = [len(labels) / (4 * n) if n else 1.0 for n in counts]
    assert s.get_class_weights() == want and len(labels) == 5 and s.get_focal_gamma() == 2.0
    check_class_weights(s.get_class_weights(), 4)


@pytest.mark.parametrize("train", [{}, {"class_weights": None, "focal_gamma": None}, {"class_weights": "None", "focal_gamma": "None"},
                                   {"focal_gamma": 0}], ids=["absent", "null", "None-strings", "zero"])
def test_settings_absent_keys_mean_off(tmp_path, train):
    s = _settings(tmp_path, train=train)
    assert s.train.class_weights is None and s.train.focal_gamma == 0.0 and s.get_class_weights() is None and s.get_focal_gamma() == 0.0


@pytest.mark.parametrize("train,msg", [({"class_weights": [1, 2, 3]}, "train.class_weights"), ({"class_weights": [1, -2, 3, 4]}, "train.class_weights"),
                                       ({"class_weights": [0, 0, 0, 0]}, "train.class_weights"), ({"class_weights": "heavy"}, "train.class_weights"),
                                       ({"class_weights": [1, "nan", 1, 1]}, "train.class_weights"), ({"class_weights": 2.0}, "train.class_weights"),
                                       ({"class_weights": [1, True, 1, 1]}, "train.class_weights"),
                                       ({"focal_gamma": -1}, "train.focal_gamma"), ({"focal_gamma": "nan"}, "train.focal_gamma"),
                                       ({"focal_gamma": "inf"}, "train.focal_gamma"), ({"focal_gamma": "much"}, "train.focal_gamma"),
                                       ({"focal_gamma": True}, "train.focal_gamma")])
def test_settings_refusals(tmp_path, train, msg):
    with pytest.raises(Exception, match=msg):
        _settings(tmp_path, train=train)


def test_settings_outside_the_train_phase_is_off(tmp_path):
    s = _val_settings(tmp_path, train={"class_weights": "balanced", "focal_gamma": 2.0})
    assert s.get_class_weights() is None and s.get_focal_gamma() == 0.0 and s.val.per_class is False


def test_settings_val_per_class(tmp_path):
    assert _val_settings(tmp_path, {"per_class": True}).val.per_class is True
    for val in ({}, {"per_class": False}, {"per_class": None}, {"per_class": "None"}):
        assert _val_settings(tmp_path, val).val.per_class is False
    for bad in ("yes", 1, 0.5):
        with pytest.raises(Exception, match="per_class"):
            _val_settings(tmp_path, {"per_class": bad})


def test_example_yaml_is_the_lrcn_one_with_the_three_keys(tmp_path):
    here = os.path.join(ROOT, "examples")
    with open(os.path.join(here, "lrcn_focal.yml")) as f:
        focal = yaml.safe_load(f)
    with open(os.path.join(here, "lrcn_ucf101_shaped.yml")) as f:
        base = yaml.safe_load(f)
    assert focal["run"]["train"].pop("class_weights") == "balanced" and focal["run"]["train"].pop("focal_gamma") == 2.0
    assert focal["run"]["val"].pop("per_class") is True
    for cfg in (focal, base):
        cfg["run"].pop("run_folder", None), cfg["run"].pop("run_id", None)
    assert focal == base


# ---- validation ------------------------------------------------------------------------------------------------------------------------
def test_per_class_over_two_chunks_one_of_which_lacks_a_class(tmp_path):
    """Seven videos, four classes, chunks of four: class 2 occurs in the second chunk only, class 3 never.  Hits and items are summed
    over the chunks, and the mean is over the three classes that have items."""
    from vltf_amd.defs_ import defs
    from vltf_amd.val import Validation
    settings = types.SimpleNamespace(num_classes=4, val=types.SimpleNamespace(logits_save_interval=4), run_folder=str(tmp_path),
                                     run_id="r", timestamp="t")
    truth = [0, 0, 1, 0, 2, 1, 2]
    guess = [0, 1, 1, 0, 2, 3, 0]                          # class 0: 2 / 3, class 1: 1 / 2, class 2: 1 / 2
    logits = np.eye(4, dtype=np.float32)[guess] * 3
    labels = np.eye(4, dtype=np.float32)[truth]
    labels[4, 3] = 1.0                                     # multi-hot: counted under its first arg-max label, class 2
    val = Validation(settings)
    for i in range(7):
        val.apply_clip_fusion(logits[i:i + 1], 1, labels[i:i + 1], defs.fusion_method.avg)
        val.save_validation_logits_chunk()
    assert val.save_counter == 1 and len(val.item_logits) == 3
    mean_class, hits, items = val.get_per_class()
    assert hits.tolist() == [2, 1, 1, 0] and items.tolist() == [3, 2, 2, 0]
    assert mean_class == pytest.approx((2 / 3 + 1 / 2 + 1 / 2) / 3)
    assert val.get_accuracy() == pytest.approx(np.mean([3 / 4, 1 / 3]))           # the global number is another one
    val.save_validation_logits_chunk(save_all=True)                                # both chunks on disk: the same numbers
    assert val.save_counter == 2 and val.get_per_class()[0] == mean_class
    assert val.report_per_class() == mean_class
    assert float(open(os.path.join(str(tmp_path), "accuracy_mean_class_r")).read()) == mean_class
    lines = [l.split() for l in open(os.path.join(str(tmp_path), "accuracy_per_class_r")).read().splitlines()]
    assert [l[:3] for l in lines] == [["0", "2", "3"], ["1", "1", "2"], ["2", "1", "2"], ["3", "0", "0"]]
    assert [float(l[3]) for l in lines[:3]] == [2 / 3, 0.5, 0.5] and math.isnan(float(lines[3][3]))


# ---- C-ABI -----------------------------------------------------------------------------------------------------------------------------
def test_ffi_refusals_need_no_device():
    """The entry point validates before it launches: null pointers, sizes, smoothing, top_k, lam, gamma, the T rule, lengths with mixed
    labels.  Nothing runs."""
    from vltf_amd import _ffi
    p, i32, f32 = _ffi.p, _ffi.i32, _ffi.f32
    assert _ffi.SIGNATURES["vl_softmax_xent_wf"] == (i32, [p, p, p, p, p, i32, i32, f32, p, i32, i32, f32, i32, f32, p, p, f32, p])
    lib = _ffi.lib()
    fake = 4096                                  # a non-null, aligned address: validation fails before anything dereferences it
    ok = dict(logits=fake, labels=fake, stats=fake, batch=4, classes=7, seq_len=None, T=1, rpc=1, eps=0.1, k=2, lam=1.0, lam_dev=None, gamma=2.0)
    bad = [dict(logits=None), dict(labels=None), dict(stats=None), dict(batch=0), dict(classes=0), dict(eps=-0.1), dict(eps=1.0),
           dict(eps=math.nan), dict(k=-1), dict(lam=1.5), dict(lam=-0.1), dict(lam=math.nan), dict(gamma=-1.0), dict(gamma=math.nan),
           dict(gamma=math.inf), dict(rpc=0), dict(rpc=3), dict(seq_len=fake, T=3), dict(seq_len=fake, T=0),
           dict(seq_len=fake, T=2, rpc=2), dict(seq_len=fake, T=2, lam=0.7), dict(seq_len=fake, T=2, lam_dev=fake)]
    for over in bad:
        a = dict(ok, **over)
        rc = lib.vl_softmax_xent_wf(a["logits"], a["labels"], None, a["stats"], None, a["batch"], a["classes"], 1.0, a["seq_len"], a["T"],
                                    a["rpc"], a["eps"], a["k"], a["lam"], a["lam_dev"], None, a["gamma"], None)
        assert rc != 0, over
        assert b"vl_softmax_xent_wf" in lib.vl_last_error()
