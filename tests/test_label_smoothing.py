"""Label smoothing and top-k accuracy on the host: the float64 reference of tests/label_smoothing_ref.py against torch's own
cross_entropy(label_smoothing=), the rank rule against the stable argsort, check_label_smoothing / check_top_k, the YAML keys with
their refusals, the getters outside the train phase, Validation.get_topk_accuracy, the data-parallel scalar vector, the example, and
the C entry point's argument checks.  No GPU: no engine is constructed and nothing is launched."""
import math
import os
import types

import numpy as np
import pytest
import torch
import yaml

from oracle import lrcn_oracle as O
from tests import label_smoothing_ref as LS
from tests.test_ema import _val_settings
from tests.test_finetune import _settings
from vltf_amd._ffi import VltfError
from vltf_amd.engine import NetConfig, check_label_smoothing, check_top_k

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,c", [(5, 7), (3, 65), (9, 101)])
@pytest.mark.parametrize("eps", [0.1, 0.3])
def test_reference_is_torch_cross_entropy_with_label_smoothing(b, c, eps):
    """Loss and gradient in float64, to 1e-12 (they agree to a few 1e-15: both are the same sums in another order)."""
    rng = np.random.default_rng(b * c)
    z = (rng.standard_normal((b, c)) * 2).astype(np.float32)
    labels = rng.integers(0, c, b)
    onehot = O.labels_to_one_hot([[l] for l in labels], c)
    e = float(np.float32(eps))
    loss, dl = O.softmax_xent_mean(z, LS.smooth(onehot, eps))
    zt = torch.tensor(z.astype(np.float64), requires_grad=True)
    want = torch.nn.functional.cross_entropy(zt, torch.tensor(labels), label_smoothing=e)
    want.backward()
    assert abs(loss - float(want.detach())) < 1e-12
    assert np.abs(dl - zt.grad.numpy()).max() < 1e-12
    y = LS.smooth(onehot, eps)
    assert np.allclose(y.sum(axis=1), 1.0, rtol=0, atol=1e-15) and y.min() == e / c
    assert np.array_equal(LS.smooth(onehot, 0.0), onehot.astype(np.float64))


def tie_logits(rows, c, seed):
    """Integer-valued logits in [-3, 3]: exactly representable, with many exact ties."""
    rng = np.random.default_rng(seed)
    z = rng.integers(-3, 4, (rows, c)).astype(np.float32)
    onehot = O.labels_to_one_hot([[l] for l in rng.integers(0, c, rows)], c)
    return z, onehot


@pytest.mark.parametrize("k", [1, 2, 5, 9])
def test_rank_rule_is_the_stable_argsort(k):
    from vltf_amd.val import topk_hits
    z, onehot = tie_logits(200, 9, 7)
    want = LS.topk_hits(z, onehot, k)
    assert np.array_equal(LS.rank(z, onehot) < k, want)
    assert np.array_equal(topk_hits(z, onehot.astype(np.float32), k), want)
    assert 0 < want.sum() and (k >= 9 or want.sum() < 200)
    if k == 1:                                            # the top-1 hit of today: first arg-max of the logits == first arg-max of the labels
        assert np.array_equal(want, np.argmax(z, 1) == np.argmax(onehot, 1))
    if k >= 9:
        assert want.all()


# ---- check_label_smoothing / check_top_k ------------------------------------------------------------------------------------------------
def test_checks_accept():
    assert check_label_smoothing(None) == 0.0 and check_label_smoothing(0) == 0.0 and check_label_smoothing(0.0) == 0.0
    assert check_label_smoothing(0.1) == 0.1 and check_label_smoothing(np.float32(0.5)) == 0.5 and check_label_smoothing(np.float64(0.25)) == 0.25
    assert isinstance(check_label_smoothing(0), float)
    assert check_top_k(None) == 0 and check_top_k(0) == 0 and check_top_k(5) == 5 and check_top_k(np.int64(3)) == 3 and check_top_k(2.0) == 2
    assert check_top_k(100000) == 100000                  # above any row width: every live row is a hit
    assert isinstance(check_top_k(2.0), int)
    assert NetConfig().label_smoothing == 0.0 and NetConfig().top_k == 0


@pytest.mark.parametrize("bad", [-0.1, 1.0, 1.5, float("nan"), float("inf"), -float("inf"), True, False, "0.1", b"0.1", [0.1], np.bool_(True)])
def test_check_label_smoothing_refuses(bad):
    with pytest.raises(VltfError, match="label_smoothing") as ex:
        check_label_smoothing(bad)
    assert repr(bad) in str(ex.value)


@pytest.mark.parametrize("bad", [-1, 2.5, float("nan"), float("inf"), True, False, "5", b"5", [5], np.bool_(True), 2 ** 31])
def test_check_top_k_refuses(bad):
    with pytest.raises(VltfError, match="top_k") as ex:
        check_top_k(bad)
    assert repr(bad) in str(ex.value)


# ---- YAML ------------------------------------------------------------------------------------------------------------------------------
def test_settings_keys_parse(tmp_path):
    s = _settings(tmp_path, train={"label_smoothing": 0.1, "top_k": 5})
    assert s.train.label_smoothing == 0.1 and s.train.top_k == 5 and s.get_label_smoothing() == 0.1 and s.get_top_k() == 5
    assert isinstance(s.train.label_smoothing, float) and isinstance(s.train.top_k, int)
    s = _settings(tmp_path, train={"label_smoothing": "1e-1", "top_k": "5"})         # quoted numbers (YAML reads 1e-1 as a string)
    assert s.get_label_smoothing() == 0.1 and s.get_top_k() == 5
    s = _settings(tmp_path, train={"label_smoothing": 0.3})
    assert s.get_label_smoothing() == 0.3 and s.get_top_k() == 0
    s = _settings(tmp_path, train={"top_k": 2})
    assert s.get_label_smoothing() == 0.0 and s.get_top_k() == 2


@pytest.mark.parametrize("train", [{}, {"label_smoothing": None, "top_k": None}, {"label_smoothing": "None", "top_k": "None"},
                                   {"label_smoothing": 0, "top_k": 0}], ids=["absent", "null", "None-strings", "zeros"])
def test_settings_absent_keys_mean_off(tmp_path, train):
    s = _settings(tmp_path, train=train)
    assert s.train.label_smoothing == 0.0 and s.train.top_k == 0 and s.get_label_smoothing() == 0.0 and s.get_top_k() == 0


@pytest.mark.parametrize("train,msg", [({"label_smoothing": -0.1}, "train.label_smoothing"), ({"label_smoothing": 1.0}, "train.label_smoothing"),
                                       ({"label_smoothing": "nan"}, "train.label_smoothing"), ({"label_smoothing": "inf"}, "train.label_smoothing"),
                                       ({"label_smoothing": "much"}, "train.label_smoothing"), ({"label_smoothing": True}, "train.label_smoothing"),
                                       ({"top_k": -1}, "train.top_k"), ({"top_k": 2.5}, "train.top_k"), ({"top_k": "five"}, "train.top_k"),
                                       ({"top_k": True}, "train.top_k"), ({"top_k": "2.5"}, "train.top_k")])
def test_settings_refusals(tmp_path, train, msg):
    with pytest.raises(Exception, match=msg):
        _settings(tmp_path, train=train)


def test_settings_outside_the_train_phase_is_off(tmp_path):
    s = _val_settings(tmp_path, train={"label_smoothing": 0.1, "top_k": 5})
    assert s.get_label_smoothing() == 0.0 and s.get_top_k() == 0 and s.val.top_k == 0


def test_settings_val_top_k(tmp_path):
    assert _val_settings(tmp_path, {"top_k": 5}).val.top_k == 5
    assert _val_settings(tmp_path, {"top_k": "2"}).val.top_k == 2
    for val in ({}, {"top_k": None}, {"top_k": "None"}, {"top_k": 0}):
        assert _val_settings(tmp_path, val).val.top_k == 0
    for bad in (-1, 1.5, True, "many"):
        with pytest.raises(Exception, match="val.top_k"):
            _val_settings(tmp_path, {"top_k": bad})


def test_example_yaml_is_the_lrcn_one_with_the_three_keys(tmp_path):
    here = os.path.join(ROOT, "examples")
    with open(os.path.join(here, "lrcn_label_smoothing.yml")) as f:
        ls = yaml.safe_load(f)
    with open(os.path.join(here, "lrcn_ucf101_shaped.yml")) as f:
        base = yaml.safe_load(f)
    assert ls["run"]["train"].pop("label_smoothing") == 0.1 and ls["run"]["train"].pop("top_k") == 5 and ls["run"]["val"].pop("top_k") == 5
    for cfg in (ls, base):
        cfg["run"].pop("run_folder", None), cfg["run"].pop("run_id", None)
    assert ls == base
    s = _settings(tmp_path, train={"label_smoothing": 0.1, "top_k": 5})
    assert (s.get_label_smoothing(), s.get_top_k()) == (0.1, 5)


# ---- validation ------------------------------------------------------------------------------------------------------------------------
def test_get_topk_accuracy_with_a_tie_at_the_boundary(tmp_path):
    """Five videos, four classes.  Row 2: the label's logit ties with a lower class for second place -> rank 2, outside the top 2, inside
    the top 3.  Row 3: the same tie with the label at the LOWER index -> rank 1, inside the top 2."""
    from vltf_amd.defs_ import defs
    from vltf_amd.val import Validation, topk_hits
    settings = types.SimpleNamespace(num_classes=4, val=types.SimpleNamespace(logits_save_interval=-1), run_folder=str(tmp_path),
                                     run_id="r", timestamp="t")
    logits = np.array([[4.0, 1.0, 0.0, -1.0],             # label 0: rank 0
                       [4.0, 1.0, 0.0, -1.0],             # label 3: rank 3
                       [5.0, 2.0, 2.0, 0.0],              # label 2: ties with class 1 below it -> rank 2
                       [5.0, 2.0, 2.0, 0.0],              # label 1: the tie goes to the lower index -> rank 1
                       [0.0, 0.0, 0.0, 0.0]], np.float32)  # label 2: all equal -> rank 2
    labels = np.eye(4, dtype=np.float32)[[0, 3, 2, 1, 2]]
    val = Validation(settings)
    val.add_items(logits, labels)
    assert val.get_accuracy() == pytest.approx(1 / 5)
    assert val.get_topk_accuracy(1) == val.get_accuracy()
    assert val.get_topk_accuracy(2) == pytest.approx(2 / 5)
    assert val.get_topk_accuracy(3) == pytest.approx(4 / 5)
    assert val.get_topk_accuracy(4) == 1.0 and val.get_topk_accuracy(9) == 1.0
    for k in (1, 2, 3, 4):
        assert np.array_equal(topk_hits(logits, labels, k), LS.topk_hits(logits, labels, k))
    # chunked: the mean of the per-chunk means, as get_accuracy
    settings.val.logits_save_interval = 2
    val = Validation(settings)
    for i in range(5):
        val.apply_clip_fusion(logits[i:i + 1], 1, labels[i:i + 1], defs.fusion_method.avg)       # one clip per video
        val.save_validation_logits_chunk()
    assert val.save_counter == 2 and len(val.item_logits) == 1
    assert val.get_topk_accuracy(2) == pytest.approx(np.mean([1 / 2, 1 / 2, 0.0]))
    assert val.get_topk_accuracy(1) == val.get_accuracy()


# ---- data parallelism ------------------------------------------------------------------------------------------------------------------
def test_topk_joins_the_exchanged_scalars_only_when_on():
    from vltf_amd.train import dp_global, dp_scalars
    off = {"loss": 1.0, "accuracy": 0.5, "loss_sum": 4.0, "correct": 2.0, "rows": 4, "grad_norm": 1.5}
    on = dict(off, topk_accuracy=0.75, topk_correct=3.0)
    assert dp_scalars(off) == [4.0, 2.0, 4.0]             # the 3-element vector of before
    assert dp_scalars(on) == [4.0, 2.0, 4.0, 3.0]
    g = dp_global(off, np.array([10.0, 6.0, 8.0]))
    assert g == dict(off, loss=1.25, accuracy=0.75) and "topk_accuracy" not in g
    g = dp_global(on, np.array([10.0, 6.0, 8.0, 7.0]))
    assert g == dict(on, loss=1.25, accuracy=0.75, topk_accuracy=0.875)
    assert dp_global(on, np.zeros(4))["topk_accuracy"] == 0.0                  # an empty global batch divides by 1


# ---- C-ABI -----------------------------------------------------------------------------------------------------------------------------
def test_ffi_row_and_host_refusals_need_no_device():
    """The entry point validates before it launches: null pointers, sizes, smoothing, top_k, the T rule.  Nothing runs."""
    from vltf_amd import _ffi
    p, i32, f32 = _ffi.p, _ffi.i32, _ffi.f32
    assert _ffi.SIGNATURES["vl_softmax_xent_ls"] == (i32, [p, p, p, p, p, i32, i32, f32, p, i32, f32, i32, p])
    assert _ffi.SIGNATURES["vl_softmax_xent"] == (i32, [p, p, p, p, p, i32, i32, f32, p])                 # as they were
    assert _ffi.SIGNATURES["vl_softmax_xent_len"] == (i32, [p, p, p, p, p, i32, i32, f32, p, i32, p])
    lib = _ffi.lib()
    fake = 4096                                  # a non-null, aligned address: validation fails before anything dereferences it
    bad = [(None, fake, fake, 4, 7, None, 1, 0.1, 2), (fake, None, fake, 4, 7, None, 1, 0.1, 2), (fake, fake, None, 4, 7, None, 1, 0.1, 2),
           (fake, fake, fake, 0, 7, None, 1, 0.1, 2), (fake, fake, fake, 4, 0, None, 1, 0.1, 2),
           (fake, fake, fake, 4, 7, None, 1, -0.1, 2), (fake, fake, fake, 4, 7, None, 1, 1.0, 2), (fake, fake, fake, 4, 7, None, 1, math.nan, 2),
           (fake, fake, fake, 4, 7, None, 1, math.inf, 2), (fake, fake, fake, 4, 7, None, 1, 0.1, -1),
           (fake, fake, fake, 4, 7, fake, 3, 0.1, 2), (fake, fake, fake, 4, 7, fake, 0, 0.1, 2)]
    for logits, labels, stats, batch, classes, seq_len, T, eps, k in bad:
        assert lib.vl_softmax_xent_ls(logits, labels, None, stats, None, batch, classes, 1.0, seq_len, T, eps, k, None) != 0, (batch, classes, eps, k)
        assert b"vl_softmax_xent_ls" in lib.vl_last_error()
