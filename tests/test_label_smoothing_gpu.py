"""Label smoothing and top-k accuracy on the device (vl_softmax_xent_ls, NetConfig.label_smoothing / top_k): the launch against the
float64 reference of tests/label_smoothing_ref.py in both launch forms, exact ties, smoothing 0 bit for bit against vl_softmax_xent
and vl_softmax_xent_len, per-clip lengths, whole steps of LRCNEngine (eager, captured, accumulated, a per-frame fc head) and of
GraphEngine with a word-level loss against the oracles fed the smoothed labels, and run_task on the example.

Tolerances.  The launch: those tests/test_ops_gpu.py and tests/test_seq_len_gpu.py hold vl_softmax_xent to -- loss 1e-5 * max(1, |loss|),
dlogits rtol 1e-4 with atol 1e-6 of the largest element, hit counts exact.  Whole steps against the fp64 oracle: those of
tests/test_engine_gpu.py::test_train_step_small, as tests/test_accumulate_gpu.py restates them -- loss 1e-4 * max(1, |loss|), gradient norm
1e-3 relative, parameters rtol 1e-4 and atol 1e-5.  (tests/test_momentum_gpu.py, whose geometry this file uses, holds only the update
rule to float64, with the engine's own gradients; a whole step through five conv layers has the project's whole-step bounds.)
Accuracies are compared on the device's own logits, as test_train_step_small does: a near tie may differ from fp64."""
import glob
import os
import pickle

import numpy as np
import pytest
import torch
import yaml

from oracle import lrcn_oracle as O
from tests import graph_cases as GC
from tests import label_smoothing_ref as LS
from tests import seq_len_ref as R
from tests.test_graph_gpu import device_feeds
from tests.test_ops_gpu import close, dev, host

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
MEAN = np.array([99.197148, 105.293620, 109.503945], np.float32)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5, 7), (4, 64), (3, 65), (9, 101), (6, 1000)]          # fewer classes than lanes | one pass | one element more | .. | 16 passes


@pytest.fixture(scope="module")
def ops():
    import vltf_amd.ops as ops_
    return ops_


def idev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.int32, device=DEV)


def bits(t):
    return t.view(torch.int32)


_CASES = {}


def case(b, c):
    """Logits 2 N(0, 1) and labels, every third row a hit by its LABEL being moved to the arg-max (the cancellation note of
    tests/test_seq_len_gpu.py::test_softmax_xent_with_lengths); made once per shape, never written."""
    if (b, c) not in _CASES:
        rng = np.random.default_rng(b * c)
        z = (rng.standard_normal((b, c)) * 2).astype(np.float32)
        onehot = O.labels_to_one_hot([[l] for l in rng.integers(0, c, b)], c)
        for r in range(0, b, 3):
            onehot[r] = 0
            onehot[r, np.argmax(z[r])] = 1
        _CASES[(b, c)] = (z, onehot)
    return _CASES[(b, c)]


def launch(ops, z, onehot, eps, k, rows_ws, lens=None, T=None, scale=None, live=None):
    """-> (stats[3], dlogits, rows workspace or None) of one ops.softmax_xent_ls; every output buffer holds NaN beforehand but stats."""
    n, c = z.shape
    zd = dev(z)
    if live is not None:
        zd[torch.from_numpy(~live).to(DEV)] = NAN
    dl = torch.full((n, c), NAN, device=DEV)
    stats = torch.zeros(3, device=DEV)
    rows = torch.full((3 * n,), NAN, device=DEV) if rows_ws else None
    ops.softmax_xent_ls(zd, dev(onehot, torch.int32), dl, stats, scale if scale is not None else 1.0 / n, rows, eps, k,
                        seq_len=None if lens is None else idev(lens), T=T)
    return stats, dl, rows


# ---- 1. the launch against float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_ws", [False, True], ids=["one-workgroup", "rows"])
@pytest.mark.parametrize("b,c", SHAPES)
def test_launch_against_fp64(ops, b, c, rows_ws):
    z, onehot = case(b, c)
    for eps in (0.1, 0.3):
        for k in (1, 2, 5, c, c + 3):
            want = LS.xent(z, onehot, eps, k)
            stats, dl, rows = launch(ops, z, onehot, eps, k, rows_ws)
            st = host(stats)
            print("b %d c %d eps %g k %d: loss %.8f want %.8f, hits %g / %g, top-k %g / %g" %
                  (b, c, eps, k, st[0] / b, want["loss"], st[1], want["hits"], st[2], want["topk"]))
            assert abs(st[0] / b - want["loss"]) < 1e-5 * max(1.0, abs(want["loss"]))
            assert want["hits"] > 0 and st[1] == want["hits"] and st[2] == want["topk"]
            if k >= c:
                assert st[2] == b                                              # every live row is a hit
            if k == 1:
                assert st[2] == st[1]
            close(host(dl), want["dlogits"], rtol=1e-4, atol_rel=1e-6, msg="dlogits eps %g k %d" % (eps, k))
            if rows_ws:
                rw = host(rows).reshape(3, b)
                assert np.isfinite(rw).all()
                assert np.array_equal(rw[1], (np.argmax(z, 1) == np.argmax(onehot, 1)).astype(np.float32))
                assert np.array_equal(rw[2], LS.topk_hits(z, onehot, k).astype(np.float32))
            again, dl2, _ = launch(ops, z, onehot, eps, k, rows_ws)          # a second call: the same bytes
            assert torch.equal(bits(again), bits(stats)) and torch.equal(bits(dl2), bits(dl))


def test_top_k_zero_leaves_the_third_sum_alone_and_sums_accumulate(ops):
    z, onehot = case(9, 101)
    for rows_ws in (False, True):
        n, c = z.shape
        stats = torch.tensor([0.0, 0.0, -7.0], device=DEV)
        rows = torch.full((3 * n,), NAN, device=DEV) if rows_ws else None
        ops.softmax_xent_ls(dev(z), dev(onehot, torch.int32), torch.empty((n, c), device=DEV), stats, 1.0 / n, rows, 0.1, 0)
        first = host(stats).copy()
        assert first[2] == -7.0 and first[0] > 0
        ops.softmax_xent_ls(dev(z), dev(onehot, torch.int32), torch.empty((n, c), device=DEV), stats, 1.0 / n, rows, 0.1, 2)
        second = host(stats)
        want = LS.xent(z, onehot, 0.1, 2)
        assert second[2] == -7.0 + want["topk"] and second[1] == 2 * first[1] and second[0] == np.float32(first[0] + first[0])


def test_host_checks(ops):
    from vltf_amd._ffi import VltfError
    z, onehot = case(4, 64)
    zd, yd = dev(z), dev(onehot, torch.int32)
    dl, stats, rows = torch.empty_like(zd), torch.zeros(3, device=DEV), torch.zeros(12, device=DEV)
    with pytest.raises(VltfError, match="int32"):
        ops.softmax_xent_ls(zd, yd.float(), dl, stats, 0.25, rows, 0.1, 2)
    with pytest.raises(VltfError, match="3\\*batch"):
        ops.softmax_xent_ls(zd, yd, dl, stats, 0.25, rows[:8], 0.1, 2)         # the 2 * batch workspace of softmax_xent is too small
    with pytest.raises(VltfError, match="3 floats"):
        ops.softmax_xent_ls(zd, yd, dl, stats[:2], 0.25, rows, 0.1, 2)
    with pytest.raises(VltfError, match="T"):
        ops.softmax_xent_ls(zd, yd, dl, stats, 0.25, rows, 0.1, 2, seq_len=idev([1]), T=3)
    for eps, k in ((-0.1, 2), (1.0, 2), (NAN, 2), (float("inf"), 2), (0.1, -1)):
        with pytest.raises(VltfError, match="smoothing|top_k"):
            ops.softmax_xent_ls(zd, yd, dl, stats, 0.25, rows, eps, k)
    torch.cuda.synchronize()
    assert not bool(stats.any())                                               # nothing was launched


# ---- 2. ties --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_ws", [False, True], ids=["one-workgroup", "rows"])
@pytest.mark.parametrize("b,c", [(200, 9), (7, 130)])
def test_ties(ops, b, c, rows_ws):
    """Integer-valued logits in [-3, 3]: the rank rule, lower index first, is exactly the stable argsort's."""
    rng = np.random.default_rng(b + c)
    z = rng.integers(-3, 4, (b, c)).astype(np.float32)
    labels = rng.integers(0, c, b)
    for r in range(0, b, 3):                              # every third row: the label at place 0 .. 5 of the stable descending order
        labels[r] = np.argsort(-z[r], kind="stable")[(r // 3) % 6]
    onehot = O.labels_to_one_hot([[l] for l in labels], c)
    plain = torch.zeros(2, device=DEV)
    ops.softmax_xent(dev(z), dev(onehot, torch.int32), torch.empty((b, c), device=DEV), plain, 1.0 / b,
                     torch.empty(2 * b, device=DEV) if rows_ws else None)
    top1 = float(np.sum(np.argmax(z, 1) == np.argmax(onehot, 1)))
    for k in (1, 2, 5):
        stats, _, _ = launch(ops, z, onehot, 0.1, k, rows_ws)
        st = host(stats)
        want = float(LS.topk_hits(z, onehot, k).sum())
        print("b %d c %d k %d: top-1 %g / %g, top-k %g / %g" % (b, c, k, st[1], top1, st[2], want))
        assert st[1] == top1 == host(plain)[1] and st[2] == want and 0 < want < b
    assert float(np.sum(LS.rank(z, onehot) != np.sum(z > z[np.arange(b), np.argmax(onehot, 1)][:, None], axis=1))) > 0   # ties did count


# ---- 3. smoothing 0 is bit for bit the launches of before ----------------------------------------------------------------------------
@pytest.mark.parametrize("rows_ws", [False, True], ids=["one-workgroup", "rows"])
@pytest.mark.parametrize("b,c", SHAPES + [(64, 101)])
def test_smoothing_zero_is_bitwise_the_plain_launch(ops, b, c, rows_ws):
    z, onehot = case(b, c)
    zd, yd = dev(z), dev(onehot, torch.int32)
    T = next(t for t in range(2, b + 1) if b % t == 0)
    lens = np.random.default_rng(b).integers(1, T + 1, b // T)
    lens[0] = 1 if b // T > 1 else max(1, T // 2)
    live = R.live_rows(lens, T)
    assert live.any() and not live.all()
    for kw, mask in ((dict(), None), (dict(seq_len=idev(lens), T=T), live)):
        zin = zd.clone()
        if mask is not None:
            zin[torch.from_numpy(~mask).to(DEV)] = NAN
        n_live = b if mask is None else int(mask.sum())
        dl0, st0 = torch.full((b, c), NAN, device=DEV), torch.zeros(2, device=DEV)
        rw0 = torch.full((2 * b,), NAN, device=DEV) if rows_ws else None
        ops.softmax_xent(zin, yd, dl0, st0, 1.0 / n_live, rw0, **kw)
        dl1, st1 = torch.full((b, c), NAN, device=DEV), torch.zeros(3, device=DEV)
        rw1 = torch.full((3 * b,), NAN, device=DEV) if rows_ws else None
        ops.softmax_xent_ls(zin, yd, dl1, st1, 1.0 / n_live, rw1, 0.0, 1, **kw)
        assert torch.equal(bits(st1[:2]), bits(st0)) and float(st0[0]) > 0
        assert torch.equal(bits(dl1), bits(dl0)) and bool(torch.isfinite(dl1).all())
        assert float(st1[2]) == float(st1[1])                                  # top_k 1 is the top-1 hit
        if rows_ws:
            assert torch.equal(bits(rw1[:2 * b]), bits(rw0)) and torch.equal(bits(rw1[2 * b:]), bits(rw1[b:2 * b]))


# ---- 4. lengths -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_ws", [False, True], ids=["one-workgroup", "rows"])
@pytest.mark.parametrize("clips,T,C", [(3, 4, 7), (8, 21, 1000)])
def test_lengths(ops, clips, T, C, rows_ws):
    rng = np.random.default_rng(clips * C)
    n = clips * T
    z = (rng.standard_normal((n, C)) * 2).astype(np.float32)
    onehot = O.labels_to_one_hot([[l] for l in rng.integers(0, C, n)], C)
    lens = rng.integers(1, T + 1, clips)
    lens[0], lens[1] = 1, T
    live = R.live_rows(lens, T)
    for r in np.flatnonzero(live)[::3]:
        onehot[r] = 0
        onehot[r, np.argmax(z[r])] = 1
    n_live = int(live.sum())
    for eps, k in ((0.1, 2), (0.3, 5)):
        want = LS.xent(z, onehot, eps, k, live)
        stats, dl, rows = launch(ops, z, onehot, eps, k, rows_ws, lens=lens, T=T, scale=1.0 / n_live, live=live)
        st, got = host(stats), host(dl)
        print("clips %d T %d C %d eps %g k %d: loss %.8f want %.8f, hits %g / %g, top-k %g / %g" %
              (clips, T, C, eps, k, st[0] / n_live, want["loss"], st[1], want["hits"], st[2], want["topk"]))
        assert abs(st[0] / n_live - want["loss"]) < 1e-5 * max(1.0, abs(want["loss"]))
        assert want["hits"] > 0 and st[1] == want["hits"] and st[2] == want["topk"]
        assert not got[~live].any(), "dlogits of a dead row is not exactly zero"
        close(got, want["dlogits"], rtol=1e-4, atol_rel=1e-6, msg="dlogits")
        if rows_ws:
            assert not host(rows).reshape(3, n)[:, ~live].any()


# ---- 5. engine steps ------------------------------------------------------------------------------------------------------------------
SHAPE, NCLS, FPC, B, HID = (67, 67, 3), 7, 3, 2, 8
LR, CLIP = 0.01, 0.5
EPS, TOPK = 0.1, 2
_DATA = {}


def small_cfg(**kw):
    from vltf_amd.engine import NetConfig
    kw = dict(dict(num_classes=NCLS, lstm_hidden=HID), **kw)
    return NetConfig(image_shape=SHAPE, fpc=FPC, frame_encoding_layer="fc6", **kw)


def data():
    """Parameters and 4 clips with labels, made once and never written."""
    if not _DATA:
        rng = np.random.default_rng(5)
        _DATA["p"] = O.init_params(rng, NCLS, "fc6", HID, 1, SHAPE, well_scaled=True)
        _DATA["frames"] = rng.integers(0, 256, (4 * FPC,) + SHAPE, dtype=np.uint8)
        _DATA["onehot"] = O.labels_to_one_hot([[l] for l in rng.integers(0, NCLS, 4)], NCLS)
        _DATA["oracle"] = {}
    return _DATA["p"], _DATA["frames"], _DATA["onehot"]


def oracle_step(clips):
    """O.lrcn_train_step fed y' on the first `clips` clips, computed once per clip count."""
    p, frames, onehot = data()
    if clips not in _DATA["oracle"]:
        x = frames[:clips * FPC].astype(np.float32) - MEAN
        _DATA["oracle"][clips] = O.lrcn_train_step(p, x, LS.smooth(onehot[:clips], EPS), FPC, lr=LR, clip_norm=CLIP)
    return _DATA["oracle"][clips]


def dev_batch(c0, c1):
    _, frames, onehot = data()
    return torch.tensor(frames[c0 * FPC:c1 * FPC], device=DEV), torch.tensor(onehot[c0:c1], device=DEV)


def check_step(out, eng, want, onehot, logits=None):
    """out / eng after one update against want = O.lrcn_train_step(.. y' ..); accuracies on the device's own logits."""
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
    eng = LRCNEngine(small_cfg(label_smoothing=EPS, top_k=TOPK), max_clips=B, device=DEV)
    eng.load_params(p)
    assert eng.stats.numel() == 3 and eng.loss_rows.numel() == 3 * B and eng.xent_ls
    out = eng.train_step_u8(*dev_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN)
    want = oracle_step(B)
    np.testing.assert_allclose(eng.logits_host(), want[4], rtol=1e-3, atol=1e-3)
    check_step(out, eng, want, onehot[:B])
    # a forward-only engine ignores both options
    infer = LRCNEngine(small_cfg(label_smoothing=EPS, top_k=TOPK), max_clips=B, device=DEV, training=False)
    assert infer.stats.numel() == 2 and not infer.xent_ls and infer.label_smoothing == 0.0 and infer.top_k == 0


def test_engine_refusals():
    from vltf_amd._ffi import VltfError
    from vltf_amd.engine import LRCNEngine
    for kw in (dict(label_smoothing=1.0), dict(label_smoothing=-0.1), dict(label_smoothing=NAN), dict(label_smoothing=True),
               dict(top_k=-1), dict(top_k=1.5), dict(top_k=True)):
        with pytest.raises(VltfError, match="label_smoothing|top_k"):
            LRCNEngine(small_cfg(**kw), max_clips=B, device=DEV)


def test_captured_step_equals_eager():
    """Step 1 is the warm-up, step 2 is captured and replayed, step 3 is a replay: two replays, each bit-equal to the eager engine in
    the three sums, the norm and every parameter; the first step is also the oracle's."""
    from vltf_amd.engine import LRCNEngine
    p, _, onehot = data()
    eager = LRCNEngine(small_cfg(label_smoothing=EPS, top_k=TOPK), max_clips=B, device=DEV)
    graph = LRCNEngine(small_cfg(label_smoothing=EPS, top_k=TOPK, step_graph=True), max_clips=B, device=DEV)
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
    eng = LRCNEngine(small_cfg(label_smoothing=EPS, top_k=TOPK, accumulate=2), max_clips=B, device=DEV)
    eng.load_params(p)
    first = eng.train_step_u8(*dev_batch(0, 2), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, micro=(0, 2))
    z0 = eng.logits_host().copy()
    assert "grad_norm" not in first and first["rows"] == 2
    assert first["topk_correct"] == float(LS.topk_hits(z0, onehot[:2], TOPK).sum()) and first["topk_accuracy"] == first["topk_correct"] / 2
    out = eng.train_step_u8(*dev_batch(2, 4), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, micro=(1, 2))
    z = np.concatenate([z0, eng.logits_host()])
    assert out["rows"] == 4 and eng.step_count == 1
    check_step(out, eng, oracle_step(4), onehot[:4], logits=z)


def test_per_frame_fc_head():
    """classifier fc without frame fusion: one logits row per FRAME (6 rows) of 11 classes."""
    from vltf_amd.engine import LRCNEngine
    ncls = 11
    rng = np.random.default_rng(12)
    cfg = small_cfg(num_classes=ncls, classifier="fc", frame_fusion=None, label_smoothing=EPS, top_k=TOPK)
    p = O.init_params(rng, ncls, "fc6", cfg.lstm_hidden, 1, SHAPE, classifier="fc", well_scaled=True)
    frames = rng.integers(0, 256, (B * FPC,) + SHAPE, dtype=np.uint8)
    onehot = O.labels_to_one_hot([[l] for l in rng.integers(0, ncls, B * FPC)], ncls)
    want = O.lrcn_train_step(p, frames.astype(np.float32) - MEAN, LS.smooth(onehot, EPS), FPC, lr=LR, clip_norm=CLIP, classifier="fc",
                             frame_fusion=None)
    eng = LRCNEngine(cfg, max_clips=B, device=DEV)
    eng.load_params(p)
    assert eng.loss_rows.numel() == 3 * B * FPC
    out = eng.train_step_u8(torch.tensor(frames, device=DEV), torch.tensor(onehot, device=DEV), lr=LR, clip_norm=CLIP, mean_bgr=MEAN)
    assert out["rows"] == B * FPC and eng.logits_host().shape == (B * FPC, ncls)
    check_step(out, eng, want, onehot)


def test_graph_engine_word_level_loss_with_lengths():
    """encdec_reshape of tests/graph_cases.py with per-clip lengths on both pipelines (those of tests/test_seq_len_gpu.py): the loss is
    a mean over the live words, smoothed over the vocabulary; against the graph oracle of tests/seq_len_ref.py fed y'."""
    from vltf_amd.graph import GraphEngine
    items = 5
    case, lens = GC.encdec(), {"enc": [1, 2, 2, 1, 2], "dec": [1, 4, 2, 3, 4]}
    pipes, ds = GC.specs_and_datasets(case, items)
    eng = GraphEngine(pipes, ds, case["V"], device=DEV, label_smoothing=EPS, top_k=TOPK)
    p = eng.init_params(seed=case["seed"], well_scaled=True)
    eng.load_params(p)
    raw, feeds = GC.inputs(case, items)
    fd = device_feeds(raw)
    got = eng.forward(fd, seq_len=lens).cpu().numpy()
    onehot = O.labels_to_one_hot([[l] for l in np.random.default_rng(0).integers(0, case["V"], got.shape[0])], case["V"])
    logits, mask, loss, grads, n_valid = R.model_with_lengths(p, case, feeds, lens, LS.smooth(onehot, EPS), items)
    assert eng.stats.numel() == 3 and eng.loss_rows.numel() == 3 * got.shape[0]
    out = eng.train_step(fd, torch.from_numpy(onehot).to(DEV), lr=LR, clip_norm=CLIP, seq_len=lens)
    clipped, gn = O.clip_by_global_norm(grads, CLIP)
    print("loss %.8f want %.8f, grad norm %.8f want %.8f, top-k %g of %d" % (out["loss"], loss, out["grad_norm"], gn, out["topk_correct"], n_valid))
    assert out["rows"] == n_valid == sum(lens["dec"])
    assert abs(out["loss"] - loss) < 1e-4 * max(1, abs(loss)) and abs(out["grad_norm"] - gn) < 1e-3 * gn
    assert out["accuracy"] == O.accuracy(got[mask], onehot[mask])
    assert out["topk_correct"] == float(LS.topk_hits(got[mask], onehot[mask], TOPK).sum()) and out["topk_accuracy"] == out["topk_correct"] / n_valid
    newp = eng.get_params()
    for k in p:
        np.testing.assert_allclose(newp[k], p[k].astype(np.float64) - LR * clipped[k], rtol=1e-4, atol=1e-5, err_msg="param " + k)


def test_options_off_is_the_engine_of_before(monkeypatch):
    """label_smoothing 0 and top_k 0, given or not: two sums, the 2 * rows workspace, ops.softmax_xent, the keys and bytes of a plain engine."""
    import vltf_amd.ops as ops_
    from vltf_amd.engine import LRCNEngine
    calls = []
    plain_launch = ops_.softmax_xent
    monkeypatch.setattr(ops_, "softmax_xent_ls", lambda *a, **k: calls.append("ls"))
    monkeypatch.setattr(ops_, "softmax_xent", lambda *a, **k: (calls.append("plain"), plain_launch(*a, **k))[1])
    p, _, _ = data()
    res = []
    for kw in (dict(label_smoothing=0.0, top_k=0), dict(label_smoothing=None, top_k=None), dict()):
        eng = LRCNEngine(small_cfg(**kw), max_clips=B, device=DEV)
        eng.load_params(p)
        assert eng.stats.numel() == 2 and eng.loss_rows.numel() == 2 * B and not eng.xent_ls
        out = eng.train_step_u8(*dev_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN)
        res.append((out, eng.get_params()))
    assert calls == ["plain"] * 3
    assert set(res[0][0]) == {"loss", "accuracy", "grad_norm", "rows", "loss_sum", "correct"}
    for out, params in res[:2]:
        assert out == res[2][0]
        for k in params:
            assert np.array_equal(params[k].view(np.int32), res[2][1][k].view(np.int32)), k


# ---- 6. run_task on the example -------------------------------------------------------------------------------------------------------
def test_run_task_on_the_example(tmp_path, monkeypatch):
    """examples/lrcn_label_smoothing.yml shrunk: the synthetic dataset and the small network of tests/test_run_task_gpu.py, two batches,
    one epoch, with the example's own label_smoothing; top_k is 2 in both phases, since the small network has 4 classes."""
    from tests.test_host_workflow import make_dataset
    from tests.test_run_task_gpu import RAW, write_cfg
    from vltf_amd import run_task
    monkeypatch.setenv("VLTF_PREFETCH", "0")
    monkeypatch.setenv("VLTF_CONV_MATH", "f32")
    monkeypatch.delenv("VLTF_STEP_GRAPH", raising=False)
    with open(os.path.join(ROOT, "examples", "lrcn_label_smoothing.yml")) as f:
        example = yaml.safe_load(f)["run"]
    assert example["train"]["label_smoothing"] == 0.1 and example["train"]["top_k"] == 5 and example["val"]["top_k"] == 5
    folder = str(tmp_path)
    train_path, _, _ = make_dataset(folder, "train.txt", nvid=4, cpv=(1, 2, 1, 1), shape=RAW, seed=1)
    val_path, _, vlabels = make_dataset(folder, "val.txt", nvid=3, cpv=(2, 1, 2), shape=RAW, seed=2)

    def cfg(name, path, phase, resume=None):
        out = write_cfg(folder, name, path, phase, resume=resume, epochs=1, det=True)
        with open(out) as f:
            c = yaml.safe_load(f)
        c["run"]["train"].update(label_smoothing=example["train"]["label_smoothing"], top_k=2)
        c["run"]["val"].update(top_k=2)
        with open(out, "w") as f:
            yaml.safe_dump(c, f)
        return out

    run = os.path.join(folder, "run")
    run_task.main(cfg("train.yml", train_path, "train"), seed=3)
    log = open(glob.glob(os.path.join(run, "log_e2e_train_scratch_*.log"))[0]).read()
    assert "Loss: label smoothing 0.1 (labels y (1 - eps) + eps / 4; the logged loss is the smoothed one), top-k accuracy k = 2" in log
    assert log.count(" top-2 accuracy : ") == 2 and "global step: 2" in log
    acc = run_task.main(cfg("val.yml", val_path, "val", resume="latest"))
    assert float(open(os.path.join(run, "accuracy_e2e_val_resume")).read()) == acc
    tot = glob.glob(os.path.join(run, "validation_logits_e2e_val_resume_*.total"))
    assert len(tot) == 1
    with open(tot[0], "rb") as f:
        logits = pickle.load(f)                                                   # written by this run
    onehot = O.labels_to_one_hot([[l] for l in vlabels], 4)
    want = float(np.mean(LS.topk_hits(logits, onehot, 2)))
    assert float(open(os.path.join(run, "accuracy_top2_e2e_val_resume")).read()) == want
    assert "Validation top-2 accuracy: %2.5f" % want in open(glob.glob(os.path.join(run, "log_e2e_val_resume_*.log"))[0]).read()
    assert acc <= want
