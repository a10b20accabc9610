"""Class weights and the focal loss on the device (vl_softmax_xent_wf, NetConfig.class_weights / focal_gamma): the launch
against the float64 closed form of tests/focal_ref.py in both launch forms, mixed labels, per-clip lengths, a saturated and a zero-weight
row, the identity with vl_softmax_xent_ls at weights 1 and gamma 0, whole steps of LRCNEngine (eager, with mixup, captured, accumulated,
a per-frame fc head) and of GraphEngine with a word-level loss against the fp64 oracles run on the reference's dlogits, the engines with
the options off, and run_task on the example.

Tolerances are the project's for the loss launch and for whole steps, as tests/test_label_smoothing_gpu.py states them: the launch --
loss 1e-5 * max(1, |loss|), dlogits rtol 1e-4 with atol 1e-6 of the largest element, hit counts exact; whole steps -- loss 1e-4 *
max(1, |loss|), gradient norm 1e-3 relative, parameters rtol 1e-4 and atol 1e-5.  The identity with vl_softmax_xent_ls: rtol 1e-6 (p A and
p round differently, so not bit for bit), with an atol of 1e-6 of the largest element for the near-cancelled label entries."""
import glob
import os
import pickle

import numpy as np
import pytest
import torch
import yaml

from oracle import lrcn_oracle as O
from tests import focal_ref as FR
from tests import graph_cases as GC
from tests import label_smoothing_ref as LS
from tests import mixup_ref as MX
from tests import seq_len_ref as R
from tests.test_graph_gpu import device_feeds
from tests.test_label_smoothing_gpu import B, CLIP, FPC, HID, LR, MEAN, NCLS, SHAPE, bits, data, dev_batch, idev, small_cfg
from tests.test_ops_gpu import close, dev, host

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# fewer classes than lanes | two passes and a remainder, a batch that is no multiple of 4 | the sum kernel's stride loop | 16 passes
SHAPES = [(5, 3), (7, 130), (261, 9), (8, 1000)]
# (weights, gamma, smoothing, top_k)
CASES = [(True, 0.0, 0.0, 0), (False, 2.0, 0.0, 0), (True, 0.5, 0.0, 0), (True, 2.0, 0.1, 3)]
CASE_IDS = ["weights", "gamma2", "gamma0.5-weights", "gamma2-weights-eps0.1-top3"]
LAM = 0.7


@pytest.fixture(scope="module")
def ops():
    import vltf_amd.ops as ops_
    return ops_


_CASES = {}


def case(b, c):
    """Logits 2 N(0, 1), one-hot labels with every third row a hit (its label moved to the arg-max), weights in [0.25, 4); made once per
    shape, never written."""
    if (b, c) not in _CASES:
        rng = np.random.default_rng(b * c + 1)
        z = (rng.standard_normal((b, c)) * 2).astype(np.float32)
        onehot = O.labels_to_one_hot([[l] for l in rng.integers(0, c, b)], c)
        for r in range(0, b, 3):
            onehot[r] = 0
            onehot[r, np.argmax(z[r])] = 1
        _CASES[(b, c)] = (z, onehot, rng.uniform(0.25, 4.0, c).astype(np.float32))
    return _CASES[(b, c)]


def launch(ops, z, onehot, rows_ws, w=None, gamma=0.0, eps=0.0, k=0, lam=1.0, rpc=1, lens=None, T=None, scale=None, live=None, stats=None):
    """-> (stats[3], dlogits, rows workspace or None) of one ops.softmax_xent_wf; every output buffer holds NaN beforehand but stats."""
    n, c = z.shape
    zd = dev(z)
    if live is not None:
        zd[torch.from_numpy(~live).to(DEV)] = NAN
    dl = torch.full((n, c), NAN, device=DEV)
    stats = torch.zeros(3, device=DEV) if stats is None else stats
    rows = torch.full((3 * n,), NAN, device=DEV) if rows_ws else None
    ops.softmax_xent_wf(zd, dev(onehot, torch.int32), dl, stats, scale if scale is not None else 1.0 / n, rows, eps, k,
                        None if w is None else dev(w), gamma, seq_len=None if lens is None else idev(lens), T=T, rows_per_clip=rpc, lam=lam)
    return stats, dl, rows


def check_launch(got, want, n_live, k, what):
    stats, dl, rows = got
    st = host(stats)
    print("%s: loss %.8f want %.8f, hits %g / %g, top-k %g / %g" % (what, st[0] / n_live, want["loss"], st[1], want["hits"], st[2], want["topk"]))
    assert abs(st[0] / n_live - want["loss"]) < 1e-5 * max(1.0, abs(want["loss"]))
    assert st[1] == want["hits"] and st[2] == (want["topk"] if k > 0 else 0.0)
    close(host(dl), want["dlogits"], rtol=1e-4, atol_rel=1e-6, msg="dlogits " + what)
    if rows is not None:
        rw = host(rows).reshape(3, -1)
        assert np.isfinite(rw).all()
        np.testing.assert_allclose(rw[0], want["row_losses"], rtol=1e-5, atol=1e-5)


# ---- 1. the launch against float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_ws", [False, True], ids=["one-workgroup", "rows"])
@pytest.mark.parametrize("use_w,gamma,eps,k", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("b,c", SHAPES)
def test_launch_against_fp64(ops, b, c, use_w, gamma, eps, k, rows_ws):
    z, onehot, w = case(b, c)
    w = w if use_w else None
    want = FR.xent(z, onehot, w, gamma, eps, k)
    assert want["hits"] > 0
    got = launch(ops, z, onehot, rows_ws, w, gamma, eps, k)
    check_launch(got, want, b, k, "b %d c %d gamma %g eps %g k %d" % (b, c, gamma, eps, k))
    if rows_ws:
        rw = host(got[2]).reshape(3, b)
        assert np.array_equal(rw[1], (np.argmax(z, 1) == np.argmax(onehot, 1)).astype(np.float32))
        if k > 0:
            assert np.array_equal(rw[2], LS.topk_hits(z, onehot, k).astype(np.float32))
    again = launch(ops, z, onehot, rows_ws, w, gamma, eps, k)                  # a second call: the same bytes
    assert torch.equal(bits(again[0]), bits(got[0])) and torch.equal(bits(again[1]), bits(got[1]))


# ---- 2. mixed labels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_ws", [False, True], ids=["one-workgroup", "rows"])
@pytest.mark.parametrize("on_device", [False, True], ids=["argument", "device-word"])
@pytest.mark.parametrize("clips,rpc,c", [(5, 1, 130), (3, 3, 9)])
def test_mixed_labels(ops, clips, rpc, c, on_device, rows_ws):
    """An odd clip count: the middle clip is its own partner and reads no other label row."""
    n = clips * rpc
    rng = np.random.default_rng(n * c)
    z = (rng.standard_normal((n, c)) * 2).astype(np.float32)
    onehot = O.labels_to_one_hot([[l] for l in rng.integers(0, c, n)], c)
    onehot[0] = 0
    onehot[0, np.argmax(z[0])] = 1
    w = rng.uniform(0.25, 4.0, c).astype(np.float32)
    assert not np.array_equal(onehot, onehot[MX.partner_rows(n, rpc)])
    for gamma, eps, k in ((0.0, 0.0, 0), (2.0, 0.1, 3)):
        want = FR.xent(z, onehot, w, gamma, eps, k, LAM, rpc)
        lam = torch.tensor([LAM], device=DEV) if on_device else LAM
        got = launch(ops, z, onehot, rows_ws, w, gamma, eps, k, lam=lam, rpc=rpc)
        check_launch(got, want, n, k, "clips %d rpc %d gamma %g" % (clips, rpc, gamma))
        mid = slice((clips // 2) * rpc, (clips // 2 + 1) * rpc)               # the middle clip alone: its own labels, unmixed
        alone = FR.xent(z, onehot, w, gamma, eps, k)
        close(host(got[1])[mid], alone["dlogits"][mid], rtol=1e-4, atol_rel=1e-6, msg="the middle clip")


# ---- 3. lengths -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_ws", [False, True], ids=["one-workgroup", "rows"])
@pytest.mark.parametrize("clips,T,C", [(3, 4, 7), (8, 21, 1000)])
def test_lengths(ops, clips, T, C, rows_ws):
    rng = np.random.default_rng(clips * C + 2)
    n = clips * T
    z = (rng.standard_normal((n, C)) * 2).astype(np.float32)
    onehot = O.labels_to_one_hot([[l] for l in rng.integers(0, C, n)], C)
    w = rng.uniform(0.25, 4.0, C).astype(np.float32)
    lens = rng.integers(1, T + 1, clips)
    lens[0], lens[1] = 1, T
    live = R.live_rows(lens, T)
    for r in np.flatnonzero(live)[::3]:
        onehot[r] = 0
        onehot[r, np.argmax(z[r])] = 1
    n_live = int(live.sum())
    for gamma, eps, k in ((0.0, 0.0, 0), (2.0, 0.1, 2)):
        want = FR.xent(z, onehot, w, gamma, eps, k, live=live)
        got = launch(ops, z, onehot, rows_ws, w, gamma, eps, k, lens=lens, T=T, scale=1.0 / n_live, live=live)   # NaN logits in the dead rows
        check_launch(got, want, n_live, k, "clips %d T %d C %d gamma %g" % (clips, T, C, gamma))
        assert want["hits"] > 0 and not host(got[1])[~live].any(), "dlogits of a dead row is not exactly zero"
        if rows_ws:
            assert not host(got[2]).reshape(3, n)[:, ~live].any()


# ---- 4. edge rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_ws", [False, True], ids=["one-workgroup", "rows"])
def test_saturated_and_zero_weight_rows(ops, rows_ws):
    """Row 0: the label's logit 120 above the rest (p_t == 1).  Row 1: the same logits, another label.  Row 2: a label of weight 0.
    Rows 3..5: ordinary.  Finite everywhere and the reference's numbers, at every gamma."""
    rng = np.random.default_rng(11)
    c = 70
    z = (rng.standard_normal((6, c)) * 2).astype(np.float32)
    z[0] = z[1] = 0.0
    z[0, 65] = z[1, 65] = 120.0
    labels = [65, 3, 9, 1, 2, 5]
    onehot = O.labels_to_one_hot([[l] for l in labels], c)
    w = rng.uniform(0.25, 4.0, c).astype(np.float32)
    w[9] = 0.0
    for gamma in (0.0, 0.5, 1.0, 2.0, 5.0):
        for eps in (0.0, 0.1):
            want = FR.xent(z, onehot, w, gamma, eps, 2)
            got = launch(ops, z, onehot, rows_ws, w, gamma, eps, 2)
            assert bool(torch.isfinite(got[1]).all()) and bool(torch.isfinite(got[0]).all())
            check_launch(got, want, 6, 2, "gamma %g eps %g" % (gamma, eps))
            if eps == 0.0:
                dl = host(got[1])
                assert not dl[2].any() and (gamma == 0.0 or not dl[0].any())       # zero weight: no gradient; saturated and focal: none
                if rows_ws:
                    assert host(got[2])[2] == 0.0


# ---- 5. weights 1 and gamma 0 is vl_softmax_xent_ls ------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_ws", [False, True], ids=["one-workgroup", "rows"])
@pytest.mark.parametrize("b,c", SHAPES)
def test_ones_and_gamma_zero_is_the_ls_launch(ops, b, c, rows_ws):
    z, onehot, _ = case(b, c)
    zd, yd = dev(z), dev(onehot, torch.int32)
    for eps, k in ((0.0, 1), (0.1, 3)):
        dl0, st0 = torch.full((b, c), NAN, device=DEV), torch.zeros(3, device=DEV)
        ops.softmax_xent_ls(zd, yd, dl0, st0, 1.0 / b, torch.full((3 * b,), NAN, device=DEV) if rows_ws else None, eps, k)
        for w in (None, np.ones(c, np.float32)):
            st1, dl1, _ = launch(ops, z, onehot, rows_ws, w, 0.0, eps, k)
            a, d = host(st0), host(st1)
            assert d[1] == a[1] and d[2] == a[2] and abs(d[0] - a[0]) <= 1e-6 * abs(a[0])
            close(host(dl1), host(dl0), rtol=1e-6, atol_rel=1e-6, msg="dlogits")


# ---- 6. other launch checks -------------------------------------------------------------------------------------------------------------
def test_top_k_zero_leaves_the_third_sum_alone_and_sums_accumulate(ops):
    z, onehot, w = case(7, 130)
    for rows_ws in (False, True):
        stats = torch.tensor([0.0, 0.0, -7.0], device=DEV)
        launch(ops, z, onehot, rows_ws, w, 2.0, 0.1, 0, stats=stats)
        first = host(stats).copy()
        assert first[2] == -7.0 and first[0] > 0
        launch(ops, z, onehot, rows_ws, w, 2.0, 0.1, 2, stats=stats)
        second = host(stats)
        want = FR.xent(z, onehot, w, 2.0, 0.1, 2)
        assert second[2] == -7.0 + want["topk"] and second[1] == 2 * first[1] and second[0] == np.float32(first[0] + first[0])


def test_host_and_c_side_refusals(ops):
    from vltf_amd._ffi import VltfError
    z, onehot, w = case(8, 1000)
    zd, yd, wd = dev(z), dev(onehot, torch.int32), dev(w)
    dl, stats, rows = torch.empty_like(zd), torch.zeros(3, device=DEV), torch.zeros(24, device=DEV)
    with pytest.raises(VltfError, match="3\\*batch"):
        ops.softmax_xent_wf(zd, yd, dl, stats, 0.125, rows[:16], 0.1, 2, wd, 2.0)
    with pytest.raises(VltfError, match="3 floats"):
        ops.softmax_xent_wf(zd, yd, dl, stats[:2], 0.125, rows, 0.1, 2, wd, 2.0)
    with pytest.raises(VltfError, match="class_weights holds 999"):
        ops.softmax_xent_wf(zd, yd, dl, stats, 0.125, rows, 0.1, 2, wd[:999], 2.0)
    with pytest.raises(VltfError, match="float32"):
        ops.softmax_xent_wf(zd, yd, dl, stats, 0.125, rows, 0.1, 2, wd.double(), 2.0)
    with pytest.raises(VltfError, match="T"):
        ops.softmax_xent_wf(zd, yd, dl, stats, 0.125, rows, 0.1, 2, wd, 2.0, seq_len=idev([1, 1, 1]), T=3)
    for kw in (dict(lam=0.7), dict(rows_per_clip=2), dict(lam=torch.tensor([0.7], device=DEV))):
        with pytest.raises(VltfError, match="seq_len cannot be combined"):
            ops.softmax_xent_wf(zd, yd, dl, stats, 0.125, rows, 0.1, 2, wd, 2.0, seq_len=idev([1, 2, 1, 2]), T=2, **kw)
    for eps, k, lam, gamma in ((-0.1, 2, 1.0, 2.0), (1.0, 2, 1.0, 2.0), (NAN, 2, 1.0, 2.0), (0.1, -1, 1.0, 2.0), (0.1, 2, 1.5, 2.0),
                               (0.1, 2, 1.0, -0.5), (0.1, 2, 1.0, NAN), (0.1, 2, 1.0, float("inf"))):
        with pytest.raises(VltfError, match="smoothing|top_k|lam|gamma"):
            ops.softmax_xent_wf(zd, yd, dl, stats, 0.125, rows, eps, k, wd, gamma, lam=lam)
    with pytest.raises(VltfError, match="whole clips"):
        ops.softmax_xent_wf(zd, yd, dl, stats, 0.125, rows, 0.1, 2, wd, 2.0, rows_per_clip=3)
    torch.cuda.synchronize()
    assert not bool(stats.any())                                               # nothing was launched


# ---- 7. engine steps ------------------------------------------------------------------------------------------------------------------
W = [0.5, 2.0, 1.0, 0.25, 3.0, 1.5, 0.75]               # NCLS weights
GAMMA, EPS, TOPK = 2.0, 0.1, 2
ON = dict(class_weights=W, focal_gamma=GAMMA, label_smoothing=EPS, top_k=TOPK)
_ORACLE = {}


def oracle_step(clips, lam=1.0):
    """O.lrcn_train_step on the first `clips` clips (blended on the host when lam < 1) with its backward run on focal_ref's dlogits of
    the mixed and smoothed labels; computed once per case."""
    p, frames, onehot = data()
    if (clips, lam) not in _ORACLE:
        x = (frames[:clips * FPC].astype(np.float32) - MEAN).reshape((clips, FPC) + SHAPE)
        with FR.oracle_loss(W, GAMMA):
            _ORACLE[(clips, lam)] = O.lrcn_train_step(p, MX.blend(x, lam).reshape((clips * FPC,) + SHAPE), MX.targets(onehot[:clips], lam, EPS),
                                                      FPC, lr=LR, clip_norm=CLIP)
    return _ORACLE[(clips, lam)]


def check_step(out, eng, want, onehot, logits=None):
    """out / eng after one update against want = O.lrcn_train_step(..); accuracies on the device's own logits, unweighted."""
    newp, loss, gn = want[0], want[1], want[2]
    print("loss %.8f want %.8f, grad norm %.8f want %.8f, accuracy %g, top-k accuracy %g" %
          (out["loss"], loss, out["grad_norm"], gn, out["accuracy"], out["topk_accuracy"]))
    assert abs(out["loss"] - loss) < 1e-4 * max(1, abs(loss)) and abs(out["grad_norm"] - gn) < 1e-3 * gn
    z = eng.logits_host() if logits is None else logits
    assert out["accuracy"] == O.accuracy(z, onehot)
    assert out["topk_correct"] == float(LS.topk_hits(z, onehot, TOPK).sum()) and out["topk_accuracy"] == out["topk_correct"] / len(z)
    got = eng.get_params()
    for k in newp:
        np.testing.assert_allclose(got[k], newp[k], rtol=1e-4, atol=1e-5, err_msg="param " + k)


def test_engine_eager_step():
    from vltf_amd.engine import LRCNEngine
    p, _, onehot = data()
    eng = LRCNEngine(small_cfg(**ON), max_clips=B, device=DEV)
    eng.load_params(p)
    assert eng.stats.numel() == 3 and eng.loss_rows.numel() == 3 * B and eng.xent_wf and eng.class_weights_dev.dtype == torch.float32
    out = eng.train_step_u8(*dev_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN)
    want = oracle_step(B)
    check_step(out, eng, want, onehot[:B])
    plain = O.softmax_xent_mean(want[4], LS.smooth(onehot[:B], EPS))[0]          # and it is not the unweighted, unfocused loss
    assert abs(out["loss"] - plain) > 1e-2 * abs(plain)
    # each option alone allocates the three columns; a forward-only engine ignores both
    for kw in (dict(class_weights=W), dict(focal_gamma=GAMMA)):
        one = LRCNEngine(small_cfg(**kw), max_clips=B, device=DEV)
        assert one.xent_wf and not one.xent_ls and one.stats.numel() == 3 and one.loss_rows.numel() == 3 * B
    infer = LRCNEngine(small_cfg(**ON), max_clips=B, device=DEV, training=False)
    assert infer.stats.numel() == 2 and not infer.xent_wf and infer.class_weights is None and infer.focal_gamma == 0.0


def test_engine_step_with_mixup():
    """Three clips: the middle one is its own partner.  The launch carries the engine's lambda word."""
    from vltf_amd.engine import LRCNEngine
    p, _, onehot = data()
    eng = LRCNEngine(small_cfg(mixup_alpha=0.2, mixup_seed=7, **ON), max_clips=3, device=DEV)
    eng.load_params(p)
    out = eng.train_step_u8(*dev_batch(0, 3), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, mix_lambda=LAM)
    assert eng.mix_lambda_last == LAM
    check_step(out, eng, oracle_step(3, LAM), onehot[:3])


def test_engine_refusals():
    from vltf_amd._ffi import VltfError
    from vltf_amd.engine import LRCNEngine
    from vltf_amd.graph import GraphEngine
    for kw in (dict(class_weights=W[:6]), dict(class_weights=W + [1.0]), dict(class_weights=[-1.0] + W[1:]), dict(class_weights=[NAN] + W[1:]),
               dict(class_weights=[0.0] * NCLS), dict(class_weights="balanced"), dict(focal_gamma=-1.0), dict(focal_gamma=NAN),
               dict(focal_gamma=float("inf")), dict(focal_gamma=True)):
        with pytest.raises(VltfError, match="class_weights|focal_gamma"):
            LRCNEngine(small_cfg(**kw), max_clips=B, device=DEV)
    case = GC.encdec()
    pipes, ds = GC.specs_and_datasets(case, 5)
    for kw in (dict(class_weights=[1.0] * (case["V"] - 1)), dict(focal_gamma=-2.0)):
        with pytest.raises(VltfError, match="class_weights|focal_gamma"):
            GraphEngine(pipes, ds, case["V"], device=DEV, **kw)


def test_captured_step_equals_eager():
    """Step 1 is the warm-up, step 2 is captured and replayed, step 3 is a replay: each bit-equal to the eager engine in the three sums,
    the norm and every parameter; the first step is also the oracle's.  The weights are a device pointer the replay reads."""
    from vltf_amd.engine import LRCNEngine
    p, _, onehot = data()
    eager = LRCNEngine(small_cfg(**ON), max_clips=B, device=DEV)
    graph = LRCNEngine(small_cfg(step_graph=True, **ON), max_clips=B, device=DEV)
    eager.load_params(p)
    graph.load_params(p)
    for step, (c0, lr) in enumerate(((0, LR), (2, 0.02), (0, 0.005))):
        outs = [e.train_step_u8(*dev_batch(c0, c0 + B), lr=lr, clip_norm=CLIP, mean_bgr=MEAN) for e in (eager, graph)]
        assert set(outs[0]) == set(outs[1]) and "topk_correct" in outs[1]
        for k in ("loss_sum", "correct", "topk_correct", "grad_norm", "rows", "loss", "topk_accuracy"):
            assert outs[0][k] == outs[1][k], (step, k, outs[0][k], outs[1][k])
        pa, pb = eager.get_params(), graph.get_params()
        for k in pa:
            assert np.array_equal(pa[k].view(np.int32), pb[k].view(np.int32)), (step, k)
        if step == 0:
            check_step(outs[1], graph, oracle_step(B), onehot[:B])
    assert len(graph._graphs) == 1


def test_accumulated_update_is_the_step_on_the_concatenated_batch():
    from vltf_amd.engine import LRCNEngine
    p, _, onehot = data()
    eng = LRCNEngine(small_cfg(accumulate=2, **ON), max_clips=B, device=DEV)
    eng.load_params(p)
    first = eng.train_step_u8(*dev_batch(0, 2), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, micro=(0, 2))
    z0 = eng.logits_host().copy()
    assert "grad_norm" not in first and first["rows"] == 2
    out = eng.train_step_u8(*dev_batch(2, 4), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, micro=(1, 2))
    z = np.concatenate([z0, eng.logits_host()])
    assert out["rows"] == 4 and eng.step_count == 1
    check_step(out, eng, oracle_step(4), onehot[:4], logits=z)


def test_empty_step_with_the_options_on():
    """train_step_empty (a rank whose shard of the batch is empty) launches no loss: three zero sums and no change of the weights.
    The exchange is a stand-in that leaves the zero gradients as they are."""
    from vltf_amd.engine import LRCNEngine

    class OneRank:
        world = 1

        def reduce_async(self, flat, off, cnt):
            pass

        def wait(self):
            pass

    p, _, _ = data()
    eng = LRCNEngine(small_cfg(**ON), max_clips=B, device=DEV, dp=OneRank())
    eng.load_params(p)
    out = eng.train_step_empty(lr=LR, clip_norm=CLIP)
    assert out["rows"] == 0 and out["loss_sum"] == 0.0 and out["correct"] == 0.0 and out["topk_correct"] == 0.0 and out["grad_norm"] == 0.0
    got = eng.get_params()
    assert all(np.array_equal(got[k], p[k]) for k in p)


def test_per_frame_fc_head():
    """classifier fc without frame fusion: one logits row per FRAME (6 rows) of 11 classes."""
    from vltf_amd.engine import LRCNEngine
    ncls = 11
    rng = np.random.default_rng(12)
    w = rng.uniform(0.25, 4.0, ncls).astype(np.float32)
    cfg = small_cfg(num_classes=ncls, classifier="fc", frame_fusion=None, **dict(ON, class_weights=w.tolist()))
    p = O.init_params(rng, ncls, "fc6", cfg.lstm_hidden, 1, SHAPE, classifier="fc", well_scaled=True)
    frames = rng.integers(0, 256, (B * FPC,) + SHAPE, dtype=np.uint8)
    onehot = O.labels_to_one_hot([[l] for l in rng.integers(0, ncls, B * FPC)], ncls)
    with FR.oracle_loss(w, GAMMA):
        want = O.lrcn_train_step(p, frames.astype(np.float32) - MEAN, LS.smooth(onehot, EPS), FPC, lr=LR, clip_norm=CLIP, classifier="fc",
                                 frame_fusion=None)
    eng = LRCNEngine(cfg, max_clips=B, device=DEV)
    eng.load_params(p)
    assert eng.loss_rows.numel() == 3 * B * FPC
    out = eng.train_step_u8(torch.tensor(frames, device=DEV), torch.tensor(onehot, device=DEV), lr=LR, clip_norm=CLIP, mean_bgr=MEAN)
    assert out["rows"] == B * FPC and eng.logits_host().shape == (B * FPC, ncls)
    check_step(out, eng, want, onehot)


def test_graph_engine_word_level_loss_with_lengths():
    """encdec_reshape of tests/graph_cases.py with per-clip lengths on both pipelines: the loss is a mean over the live words, weighted
    over the vocabulary and focused; against the graph oracle of tests/seq_len_ref.py run on focal_ref's dlogits."""
    from vltf_amd.graph import GraphEngine
    items = 5
    case, lens = GC.encdec(), {"enc": [1, 2, 2, 1, 2], "dec": [1, 4, 2, 3, 4]}
    w = np.random.default_rng(case["V"]).uniform(0.25, 4.0, case["V"]).astype(np.float32)
    pipes, ds = GC.specs_and_datasets(case, items)
    eng = GraphEngine(pipes, ds, case["V"], device=DEV, label_smoothing=EPS, top_k=TOPK, class_weights=w.tolist(), focal_gamma=GAMMA)
    p = eng.init_params(seed=case["seed"], well_scaled=True)
    eng.load_params(p)
    raw, feeds = GC.inputs(case, items)
    fd = device_feeds(raw)
    got = eng.forward(fd, seq_len=lens).cpu().numpy()
    onehot = O.labels_to_one_hot([[l] for l in np.random.default_rng(0).integers(0, case["V"], got.shape[0])], case["V"])
    with FR.oracle_loss(w, GAMMA):
        logits, mask, loss, grads, n_valid = R.model_with_lengths(p, case, feeds, lens, LS.smooth(onehot, EPS), items)
    assert eng.xent_wf and eng.stats.numel() == 3 and eng.loss_rows.numel() == 3 * got.shape[0]
    out = eng.train_step(fd, torch.from_numpy(onehot).to(DEV), lr=LR, clip_norm=CLIP, seq_len=lens)
    clipped, gn = O.clip_by_global_norm(grads, CLIP)
    print("loss %.8f want %.8f, grad norm %.8f want %.8f, top-k %g of %d" % (out["loss"], loss, out["grad_norm"], gn, out["topk_correct"], n_valid))
    assert out["rows"] == n_valid == sum(lens["dec"])
    assert abs(out["loss"] - loss) < 1e-4 * max(1, abs(loss)) and abs(out["grad_norm"] - gn) < 1e-3 * gn
    assert out["accuracy"] == O.accuracy(got[mask], onehot[mask])
    assert out["topk_correct"] == float(LS.topk_hits(got[mask], onehot[mask], TOPK).sum())
    newp = eng.get_params()
    for k in p:
        np.testing.assert_allclose(newp[k], p[k].astype(np.float64) - LR * clipped[k], rtol=1e-4, atol=1e-5, err_msg="param " + k)


# ---- 8. the options off ---------------------------------------------------------------------------------------------------------------
def test_options_off_is_the_engine_of_before(monkeypatch):
    """class_weights None and focal_gamma 0, given or not: the workspace, the ops calls, the keys and the bytes of an engine without them,
    plain, with label smoothing and with mixup; ops.softmax_xent_wf is never called."""
    import vltf_amd.ops as ops_
    from vltf_amd.engine import LRCNEngine
    calls = []

    def record(name):
        real = getattr(ops_, name)
        monkeypatch.setattr(ops_, name, lambda *a, **k: (calls.append(name), real(*a, **k))[1])

    for name in ("softmax_xent", "softmax_xent_ls", "softmax_xent_mix", "softmax_xent_wf"):
        record(name)
    p, _, _ = data()
    for base, name, cols in ((dict(), "softmax_xent", 2), (dict(label_smoothing=EPS, top_k=TOPK), "softmax_xent_ls", 3),
                             (dict(mixup_alpha=0.2, mixup_seed=7), "softmax_xent_mix", 3)):
        res = []
        del calls[:]
        for kw in (dict(class_weights=None, focal_gamma=0.0), dict(focal_gamma=None), dict(focal_gamma=0), dict()):
            eng = LRCNEngine(small_cfg(**dict(base, **kw)), max_clips=B, device=DEV)
            eng.load_params(p)
            assert eng.stats.numel() == cols and eng.loss_rows.numel() == cols * B and not eng.xent_wf and eng.class_weights_dev is None
            out = eng.train_step_u8(*dev_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN)
            res.append((out, eng.get_params()))
        assert calls == [name] * 4
        for out, params in res[:3]:
            assert out == res[3][0]
            for k in params:
                assert np.array_equal(params[k].view(np.int32), res[3][1][k].view(np.int32)), k
    eng = LRCNEngine(small_cfg(**ON), max_clips=B, device=DEV)                   # and on: the new launch alone
    eng.load_params(p)
    del calls[:]
    eng.train_step_u8(*dev_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN)
    assert calls == ["softmax_xent_wf"]


# ---- 9. run_task on the example -------------------------------------------------------------------------------------------------------
def test_run_task_on_the_example(tmp_path, monkeypatch):
    """examples/lrcn_focal.yml shrunk: the synthetic dataset and the small network of tests/test_run_task_gpu.py, two batches, one epoch,
    with the example's own class_weights: balanced and focal_gamma; the validation run writes the per-class files."""
    from tests.test_host_workflow import make_dataset
    from tests.test_run_task_gpu import RAW, write_cfg
    from vltf_amd import run_task
    from vltf_amd.settings_ import balanced_class_weights
    monkeypatch.setenv("VLTF_PREFETCH", "0")
    monkeypatch.setenv("VLTF_CONV_MATH", "f32")
    monkeypatch.delenv("VLTF_STEP_GRAPH", raising=False)
    with open(os.path.join(ROOT, "examples", "lrcn_focal.yml")) as f:
        example = yaml.safe_load(f)["run"]
    assert example["train"]["class_weights"] == "balanced" and example["train"]["focal_gamma"] == 2.0 and example["val"]["per_class"] is True
    folder = str(tmp_path)
    train_path, _, tlabels = make_dataset(folder, "train.txt", nvid=4, cpv=(1, 2, 1, 1), shape=RAW, seed=1)
    val_path, _, vlabels = make_dataset(folder, "val.txt", nvid=3, cpv=(2, 1, 2), shape=RAW, seed=2)

    def cfg(name, path, phase, resume=None):
        out = write_cfg(folder, name, path, phase, resume=resume, epochs=1, det=True)
        with open(out) as f:
            c = yaml.safe_load(f)
        c["run"]["train"].update(class_weights=example["train"]["class_weights"], focal_gamma=example["train"]["focal_gamma"])
        c["run"]["val"].update(per_class=example["val"]["per_class"])
        with open(out, "w") as f:
            yaml.safe_dump(c, f)
        return out

    run = os.path.join(folder, "run")
    run_task.main(cfg("train.yml", train_path, "train"), seed=3)
    log = open(glob.glob(os.path.join(run, "log_e2e_train_scratch_*.log"))[0]).read()
    w = np.asarray(balanced_class_weights([[l] for l in tlabels], 4)[0], np.float32)
    assert ("Loss: focal gamma 2.0, class weights min %g (class %d), max %g (class %d)" % (w.min(), w.argmin(), w.max(), w.argmax())) in log
    assert "global step: 2" in log
    acc = run_task.main(cfg("val.yml", val_path, "val", resume="latest"))
    assert float(open(os.path.join(run, "accuracy_e2e_val_resume")).read()) == acc
    tot = glob.glob(os.path.join(run, "validation_logits_e2e_val_resume_*.total"))
    assert len(tot) == 1
    with open(tot[0], "rb") as f:
        logits = pickle.load(f)                                                   # written by this run
    guess, truth = np.argmax(logits, axis=1), np.asarray(vlabels)
    items = np.bincount(truth, minlength=4)
    hits = np.bincount(truth[guess == truth], minlength=4)
    want = float(np.mean(hits[items > 0] / items[items > 0]))
    assert float(open(os.path.join(run, "accuracy_mean_class_e2e_val_resume")).read()) == want
    lines = [l.split() for l in open(os.path.join(run, "accuracy_per_class_e2e_val_resume")).read().splitlines()]
    assert [[int(v) for v in l[:3]] for l in lines] == [[c, hits[c], items[c]] for c in range(4)]
    assert "Validation mean-class accuracy: %2.5f" % want in open(glob.glob(os.path.join(run, "log_e2e_val_resume_*.log"))[0]).read()
