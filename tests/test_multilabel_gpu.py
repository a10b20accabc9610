"""The multi-label loss on the device (vl_sigmoid_xent, NetConfig.label_type "multiple"): the launch against the float64
closed form of tests/multilabel_ref.py in both launch forms, mixed labels, per-clip lengths, saturated logits and a zero-weight class,
accumulating sums and refusals, whole steps of LRCNEngine (eager, with mixup, captured, accumulated, a per-frame fc head) and of
GraphEngine with a loss under seq_len against the fp64 oracles run on the reference's dlogits, label_type single against an engine built
without the argument, and run_task on the example.

Tolerances are the project's for the loss launch and for whole steps, as tests/test_label_smoothing_gpu.py and tests/test_focal_gpu.py
state them: the launch -- loss 1e-5 * max(1, |loss|), dlogits rtol 1e-4 with atol 1e-6 of the largest element, hit and exact counts
exact, a second call the same bytes; whole steps -- loss 1e-4 * max(1, |loss|), gradient norm 1e-3 relative, parameters rtol 1e-4 and
atol 1e-5."""
import glob
import os
import pickle

import numpy as np
import pytest
import torch
import yaml

from oracle import lrcn_oracle as O
from tests import graph_cases as GC
from tests import mixup_ref as MX
from tests import multilabel_ref as ML
from tests import seq_len_ref as R
from tests.test_graph_gpu import device_feeds
from tests.test_label_smoothing_gpu import B, CLIP, FPC, LR, MEAN, NCLS, SHAPE, bits, data, idev, small_cfg
from tests.test_ops_gpu import close, dev, host

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# fewer classes than lanes | two passes and a remainder, a batch that is no multiple of 4 | the sum kernel's stride loop | 16 passes
SHAPES = [(5, 3), (7, 130), (261, 9), (8, 1000)]
# (weights, gamma, smoothing)
CASES = [(False, 0.0, 0.0), (True, 0.0, 0.0), (False, 2.0, 0.0), (True, 0.5, 0.0), (True, 2.0, 0.1)]
CASE_IDS = ["plain", "weights", "gamma2", "gamma0.5-weights", "gamma2-weights-eps0.1"]
LAM = 0.7


@pytest.fixture(scope="module")
def ops():
    import vltf_amd.ops as ops_
    return ops_


_CASES = {}


def case(b, c):
    """Logits 2 N(0, 1), multi-hot labels at density 0.2, weights in [0.25, 4); made once per shape, never written.  Every third row's
    labels are z > 0 (an exact match); of the other rows every second one carries its arg-max class (a hit) and the second of them has
    no label at all.  Row 0 then gets z == 0.0 under y = 0 (class 0: still predicted right) and under y = 1 (class 1: a miss)."""
    if (b, c) not in _CASES:
        rng = np.random.default_rng(b * c + 3)
        z = (rng.standard_normal((b, c)) * 2).astype(np.float32)
        y = (rng.random((b, c)) < 0.2).astype(np.int32)
        rest = [r for r in range(b) if r % 3]
        for r in range(0, b, 3):
            y[r] = z[r] > 0
        for r in rest[::2]:
            y[r, np.argmax(z[r])] = 1
        y[rest[1]] = 0
        z[0, 0], y[0, 0] = 0.0, 0
        z[0, 1], y[0, 1] = 0.0, 1
        want = ML.xent(z, y)
        assert 0 < want["hits"] < b and 0 < want["exact"] < b, (b, c, want["hits"], want["exact"])
        _CASES[(b, c)] = (z, y, rng.uniform(0.25, 4.0, c).astype(np.float32))
    return _CASES[(b, c)]


def launch(ops, z, y, rows_ws, q=None, gamma=0.0, eps=0.0, lam=1.0, rpc=1, lens=None, T=None, scale=None, live=None, stats=None,
           no_dlogits=False):
    """-> (stats[3], dlogits, rows workspace or None) of one ops.sigmoid_xent; every output buffer holds NaN beforehand but stats."""
    n, c = z.shape
    zd = dev(z)
    if live is not None:
        zd[torch.from_numpy(~live).to(DEV)] = NAN
    dl = None if no_dlogits else torch.full((n, c), NAN, device=DEV)
    stats = torch.zeros(3, device=DEV) if stats is None else stats
    rows = torch.full((3 * n,), NAN, device=DEV) if rows_ws else None
    ops.sigmoid_xent(zd, dev(y, torch.int32), dl, stats, scale if scale is not None else 1.0 / n, rows, eps, None if q is None else dev(q),
                     gamma, seq_len=None if lens is None else idev(lens), T=T, rows_per_clip=rpc, lam=lam)
    return stats, dl, rows


def check_launch(got, want, n_live, what):
    stats, dl, rows = got
    st = host(stats)
    print("%s: loss %.8f want %.8f, hits %g / %g, exact %g / %g" % (what, st[0] / n_live, want["loss"], st[1], want["hits"], st[2], want["exact"]))
    assert abs(st[0] / n_live - want["loss"]) < 1e-5 * max(1.0, abs(want["loss"]))
    assert st[1] == want["hits"] and st[2] == want["exact"]
    close(host(dl), want["dlogits"], rtol=1e-4, atol_rel=1e-6, msg="dlogits " + what)
    if rows is not None:
        rw = host(rows).reshape(3, -1)
        assert np.isfinite(rw).all()
        np.testing.assert_allclose(rw[0], want["row_losses"], rtol=1e-5, atol=1e-5)
        assert np.array_equal(rw[1], want["hit_rows"].astype(np.float32)) and np.array_equal(rw[2], want["exact_rows"].astype(np.float32))


# ---- 1. the launch against float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_ws", [False, True], ids=["one-workgroup", "rows"])
@pytest.mark.parametrize("use_q,gamma,eps", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("b,c", SHAPES)
def test_launch_against_fp64(ops, b, c, use_q, gamma, eps, rows_ws):
    z, y, q = case(b, c)
    q = q if use_q else None
    want = ML.xent(z, y, q, gamma, eps)
    got = launch(ops, z, y, rows_ws, q, gamma, eps)
    check_launch(got, want, b, "b %d c %d gamma %g eps %g" % (b, c, gamma, eps))
    again = launch(ops, z, y, rows_ws, q, gamma, eps)                          # a second call: the same bytes
    assert torch.equal(bits(again[0]), bits(got[0])) and torch.equal(bits(again[1]), bits(got[1]))


# ---- 2. mixed labels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_ws", [False, True], ids=["one-workgroup", "rows"])
@pytest.mark.parametrize("on_device", [False, True], ids=["argument", "device-word"])
@pytest.mark.parametrize("clips,rpc,c", [(5, 1, 130), (3, 3, 9)])
def test_mixed_labels(ops, clips, rpc, c, on_device, rows_ws):
    """An odd clip count: the middle clip is its own partner and reads no other label row.  lam 1 is the unmixed launch bit for bit."""
    n = clips * rpc
    rng = np.random.default_rng(n * c)
    z = (rng.standard_normal((n, c)) * 2).astype(np.float32)
    y = (rng.random((n, c)) < 0.2).astype(np.int32)
    y[0, np.argmax(z[0])] = 1
    q = rng.uniform(0.25, 4.0, c).astype(np.float32)
    assert not np.array_equal(y, y[MX.partner_rows(n, rpc)])
    for gamma, eps in ((0.0, 0.0), (2.0, 0.1)):
        want = ML.xent(z, y, q, gamma, eps, LAM, rpc)
        lam = torch.tensor([LAM], device=DEV) if on_device else LAM
        got = launch(ops, z, y, rows_ws, q, gamma, eps, lam=lam, rpc=rpc)
        check_launch(got, want, n, "clips %d rpc %d gamma %g" % (clips, rpc, gamma))
        mid = slice((clips // 2) * rpc, (clips // 2 + 1) * rpc)               # the middle clip alone: its own labels, unmixed
        alone = ML.xent(z, y, q, gamma, eps)
        close(host(got[1])[mid], alone["dlogits"][mid], rtol=1e-4, atol_rel=1e-6, msg="the middle clip")
        one = launch(ops, z, y, rows_ws, q, gamma, eps, lam=torch.ones(1, device=DEV) if on_device else 1.0, rpc=rpc)
        plain = launch(ops, z, y, rows_ws, q, gamma, eps)
        assert torch.equal(bits(one[0]), bits(plain[0])) and torch.equal(bits(one[1]), bits(plain[1]))


# ---- 3. lengths -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_ws", [False, True], ids=["one-workgroup", "rows"])
@pytest.mark.parametrize("clips,T,C", [(3, 4, 7), (8, 21, 1000)])
def test_lengths(ops, clips, T, C, rows_ws):
    rng = np.random.default_rng(clips * C + 2)
    n = clips * T
    z = (rng.standard_normal((n, C)) * 2).astype(np.float32)
    y = (rng.random((n, C)) < 0.2).astype(np.int32)
    q = rng.uniform(0.25, 4.0, C).astype(np.float32)
    lens = rng.integers(1, T + 1, clips)
    lens[0], lens[1] = 1, T
    live = R.live_rows(lens, T)
    for r in np.flatnonzero(live)[::3]:
        y[r] = z[r] > 0
    n_live = int(live.sum())
    for gamma, eps in ((0.0, 0.0), (2.0, 0.1)):
        want = ML.xent(z, y, q, gamma, eps, live=live)
        got = launch(ops, z, y, rows_ws, q, gamma, eps, lens=lens, T=T, scale=1.0 / n_live, live=live)   # NaN logits in the dead rows
        check_launch(got, want, n_live, "clips %d T %d C %d gamma %g" % (clips, T, C, gamma))
        assert want["exact"] > 0 and not host(got[1])[~live].any(), "dlogits of a dead row is not exactly zero"
        if rows_ws:
            assert not host(got[2]).reshape(3, n)[:, ~live].any()


# ---- 4. edge rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_ws", [False, True], ids=["one-workgroup", "rows"])
def test_saturated_logits_and_a_zero_weight_class(ops, rows_ws):
    """Row 0: z = +120 under y = 1 and y = 0, z = -120 under both.  Row 1: its only label is the class of weight 0.  Rows 2..5:
    ordinary.  Finite everywhere and the reference's numbers, at every gamma."""
    rng = np.random.default_rng(11)
    c = 70
    z = (rng.standard_normal((6, c)) * 2).astype(np.float32)
    y = (rng.random((6, c)) < 0.2).astype(np.int32)
    z[0, :4] = [120.0, 120.0, -120.0, -120.0]
    y[0, :4] = [1, 0, 1, 0]
    y[1] = 0
    y[1, 9] = 1
    q = rng.uniform(0.25, 4.0, c).astype(np.float32)
    q[9] = 0.0
    for gamma in (0.0, 0.5, 1.0, 2.0, 5.0):
        for eps in (0.0, 0.1):
            want = ML.xent(z, y, q, gamma, eps)
            got = launch(ops, z, y, rows_ws, q, gamma, eps)
            assert bool(torch.isfinite(got[1]).all()) and bool(torch.isfinite(got[0]).all())
            check_launch(got, want, 6, "gamma %g eps %g" % (gamma, eps))
            if eps == 0.0:
                dl = host(got[1])
                assert dl[1, 9] == 0.0 and want["dlogits"][1, 9] == 0.0           # a zero-weight positive: t = 1 leaves no negative term either
                assert dl[0, 0] == 0.0 and dl[0, 3] == 0.0 and dl[0, 1] > 0.0 and dl[0, 2] < 0.0          # saturated: the limits, no NaN


# ---- 5. accumulation and refusals -----------------------------------------------------------------------------------------------------
def test_sums_accumulate_and_dlogits_may_be_null(ops):
    z, y, q = case(7, 130)
    want = ML.xent(z, y, q, 2.0, 0.1)
    for rows_ws in (False, True):
        stats = torch.tensor([0.0, 0.0, -7.0], device=DEV)
        launch(ops, z, y, rows_ws, q, 2.0, 0.1, stats=stats)
        first = host(stats).copy()
        assert first[2] == -7.0 + want["exact"] and first[1] == want["hits"] and first[0] > 0
        launch(ops, z, y, rows_ws, q, 2.0, 0.1, stats=stats, no_dlogits=True)
        second = host(stats)
        assert second[2] == -7.0 + 2 * want["exact"] and second[1] == 2 * first[1] and second[0] == np.float32(first[0] + first[0])


def test_host_and_c_side_refusals(ops):
    from vltf_amd._ffi import VltfError
    z, y, q = case(8, 1000)
    zd, yd, qd = dev(z), dev(y, torch.int32), dev(q)
    dl, stats, rows = torch.empty_like(zd), torch.zeros(3, device=DEV), torch.zeros(24, device=DEV)
    with pytest.raises(VltfError, match="3\\*batch"):
        ops.sigmoid_xent(zd, yd, dl, stats, 0.125, rows[:16], 0.1, qd, 2.0)
    with pytest.raises(VltfError, match="3 floats"):
        ops.sigmoid_xent(zd, yd, dl, stats[:2], 0.125, rows, 0.1, qd, 2.0)
    with pytest.raises(VltfError, match="pos_weights holds 999"):
        ops.sigmoid_xent(zd, yd, dl, stats, 0.125, rows, 0.1, qd[:999], 2.0)
    with pytest.raises(VltfError, match="float32"):
        ops.sigmoid_xent(zd, yd, dl, stats, 0.125, rows, 0.1, qd.double(), 2.0)
    with pytest.raises(VltfError, match="int32"):
        ops.sigmoid_xent(zd, yd.float(), dl, stats, 0.125, rows, 0.1, qd, 2.0)
    with pytest.raises(VltfError, match="T"):
        ops.sigmoid_xent(zd, yd, dl, stats, 0.125, rows, 0.1, qd, 2.0, seq_len=idev([1, 1, 1]), T=3)
    with pytest.raises(VltfError, match="logits' shape"):
        ops.sigmoid_xent(zd, yd[:4], dl, stats, 0.125, rows, 0.1, qd, 2.0, lam=0.7)
    with pytest.raises(VltfError, match="one float32"):
        ops.sigmoid_xent(zd, yd, dl, stats, 0.125, rows, 0.1, qd, 2.0, lam=torch.ones(2, device=DEV))
    for kw in (dict(lam=0.7), dict(rows_per_clip=2), dict(lam=torch.tensor([0.7], device=DEV))):
        with pytest.raises(VltfError, match="seq_len cannot be combined"):
            ops.sigmoid_xent(zd, yd, dl, stats, 0.125, rows, 0.1, qd, 2.0, seq_len=idev([1, 2, 1, 2]), T=2, **kw)
    for eps, lam, gamma in ((-0.1, 1.0, 2.0), (1.0, 1.0, 2.0), (NAN, 1.0, 2.0), (0.1, 1.5, 2.0), (0.1, -0.5, 2.0), (0.1, 1.0, -0.5),
                            (0.1, 1.0, NAN), (0.1, 1.0, float("inf"))):
        with pytest.raises(VltfError, match="smoothing|lam|gamma"):
            ops.sigmoid_xent(zd, yd, dl, stats, 0.125, rows, eps, qd, gamma, lam=lam)
    with pytest.raises(VltfError, match="whole clips"):
        ops.sigmoid_xent(zd, yd, dl, stats, 0.125, rows, 0.1, qd, 2.0, rows_per_clip=3)
    torch.cuda.synchronize()
    assert not bool(stats.any()) and not bool(rows.any())                      # nothing was launched


# ---- 6. engine steps ------------------------------------------------------------------------------------------------------------------
Q = [0.5, 2.0, 1.0, 0.25, 3.0, 1.5, 0.75]               # NCLS positive-term weights
GAMMA, EPS = 2.0, 0.1
ON = dict(label_type="multiple", class_weights=Q, focal_gamma=GAMMA, label_smoothing=EPS)
LABELS = np.array([[1, 0, 0, 1, 0, 0, 1], [0, 0, 0, 0, 0, 0, 0], [0, 1, 1, 0, 0, 0, 0], [0, 0, 0, 0, 1, 0, 0]], np.int32)   # 4 clips x NCLS
_ORACLE = {}


def ml_batch(c0, c1):
    _, frames, _ = data()
    return torch.tensor(frames[c0 * FPC:c1 * FPC], device=DEV), torch.tensor(LABELS[c0:c1], device=DEV)


def oracle_step(clips, lam=1.0):
    """O.lrcn_train_step on the first `clips` clips (blended on the host when lam < 1) with its backward run on multilabel_ref's
    dlogits of the mixed and smoothed labels; computed once per case."""
    p, frames, _ = data()
    if (clips, lam) not in _ORACLE:
        x = (frames[:clips * FPC].astype(np.float32) - MEAN).reshape((clips, FPC) + SHAPE)
        with ML.oracle_loss(Q, GAMMA):
            _ORACLE[(clips, lam)] = O.lrcn_train_step(p, MX.blend(x, lam).reshape((clips * FPC,) + SHAPE), ML.targets(LABELS[:clips], lam, EPS),
                                                      FPC, lr=LR, clip_norm=CLIP)
    return _ORACLE[(clips, lam)]


def check_step(out, eng, want, labels, logits=None):
    """out / eng after one update against want = O.lrcn_train_step(..); hit@1 and the exact matches on the device's own logits."""
    newp, loss, gn = want[0], want[1], want[2]
    print("loss %.8f want %.8f, grad norm %.8f want %.8f, hit@1 %g, subset accuracy %g" %
          (out["loss"], loss, out["grad_norm"], gn, out["accuracy"], out["subset_accuracy"]))
    assert abs(out["loss"] - loss) < 1e-4 * max(1, abs(loss)) and abs(out["grad_norm"] - gn) < 1e-3 * gn
    z = eng.logits_host() if logits is None else logits
    assert out["correct"] == float(ML.hit1(z, labels).sum()) and out["accuracy"] == out["correct"] / len(z)
    assert out["subset_correct"] == float(ML.exact(z, labels).sum()) and out["subset_accuracy"] == out["subset_correct"] / len(z)
    assert "topk_correct" not in out
    got = eng.get_params()
    for k in newp:
        np.testing.assert_allclose(got[k], newp[k], rtol=1e-4, atol=1e-5, err_msg="param " + k)


def test_engine_eager_step():
    from vltf_amd.engine import LRCNEngine
    p, _, _ = data()
    eng = LRCNEngine(small_cfg(**ON), max_clips=B, device=DEV)
    eng.load_params(p)
    assert eng.stats.numel() == 3 and eng.loss_rows.numel() == 3 * B and eng.multilabel and eng.class_weights_dev.dtype == torch.float32
    out = eng.train_step_u8(*ml_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN)
    want = oracle_step(B)
    check_step(out, eng, want, LABELS[:B])
    plain = LRCNEngine(small_cfg(label_type="multiple"), max_clips=B, device=DEV)      # no option but the mode: still three columns
    assert plain.multilabel and not plain.xent_wf and not plain.xent_ls and plain.stats.numel() == 3 and plain.loss_rows.numel() == 3 * B
    plain.load_params(p)
    out = plain.train_step_u8(*ml_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN)
    loss, _ = ML.xent_mean(plain.logits_host(), ML.targets(LABELS[:B]))
    assert abs(out["loss"] - loss) < 1e-4 * max(1, abs(loss))


def test_engine_step_with_mixup():
    """Three clips: the middle one is its own partner.  The launch carries the engine's lambda word."""
    from vltf_amd.engine import LRCNEngine
    p, _, _ = data()
    eng = LRCNEngine(small_cfg(mixup_alpha=0.2, mixup_seed=7, **ON), max_clips=3, device=DEV)
    eng.load_params(p)
    out = eng.train_step_u8(*ml_batch(0, 3), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, mix_lambda=LAM)
    assert eng.mix_lambda_last == LAM
    check_step(out, eng, oracle_step(3, LAM), LABELS[:3])


def test_engine_refusals():
    from vltf_amd._ffi import VltfError
    from vltf_amd.composed import ComposedEngine, HeadConfig
    from vltf_amd.engine import LRCNEngine
    from vltf_amd.graph import GraphEngine
    with pytest.raises(VltfError, match="top_k = 2 is refused with label_type multiple"):
        LRCNEngine(small_cfg(label_type="multiple", top_k=2), max_clips=B, device=DEV)
    with pytest.raises(VltfError, match="label_type must be"):
        LRCNEngine(small_cfg(label_type="several"), max_clips=B, device=DEV)
    case_ = GC.encdec()
    pipes, ds = GC.specs_and_datasets(case_, 5)
    with pytest.raises(VltfError, match="top_k = 2 is refused with label_type multiple"):
        GraphEngine(pipes, ds, case_["V"], device=DEV, label_type="multiple", top_k=2)
    with pytest.raises(VltfError, match="label_type must be"):
        GraphEngine(pipes, ds, case_["V"], device=DEV, label_type="several")
    with pytest.raises(VltfError, match="label_type multiple is not built"):
        ComposedEngine(small_cfg(label_type="multiple"), HeadConfig(in_dim=6, fpc=4, num_classes=9), max_clips=2, device=DEV)


def test_captured_step_equals_eager():
    """Step 1 is the warm-up, step 2 is captured and replayed, step 3 is a replay: each bit-equal to the eager engine in the three sums,
    the norm and every parameter; the first step is also the oracle's.  The weights are a device pointer the replay reads."""
    from vltf_amd.engine import LRCNEngine
    p, _, _ = data()
    eager = LRCNEngine(small_cfg(**ON), max_clips=B, device=DEV)
    graph = LRCNEngine(small_cfg(step_graph=True, **ON), max_clips=B, device=DEV)
    eager.load_params(p)
    graph.load_params(p)
    for step, (c0, lr) in enumerate(((0, LR), (2, 0.02), (0, 0.005))):
        outs = [e.train_step_u8(*ml_batch(c0, c0 + B), lr=lr, clip_norm=CLIP, mean_bgr=MEAN) for e in (eager, graph)]
        assert set(outs[0]) == set(outs[1]) and "subset_correct" in outs[1]
        for k in ("loss_sum", "correct", "subset_correct", "grad_norm", "rows", "loss", "subset_accuracy"):
            assert outs[0][k] == outs[1][k], (step, k, outs[0][k], outs[1][k])
        pa, pb = eager.get_params(), graph.get_params()
        for k in pa:
            assert np.array_equal(pa[k].view(np.int32), pb[k].view(np.int32)), (step, k)
        if step == 0:
            check_step(outs[1], graph, oracle_step(B), LABELS[:B])
    assert len(graph._graphs) == 1


def test_accumulated_update_is_the_step_on_the_concatenated_batch():
    from vltf_amd.engine import LRCNEngine
    p, _, _ = data()
    eng = LRCNEngine(small_cfg(accumulate=2, **ON), max_clips=B, device=DEV)
    eng.load_params(p)
    first = eng.train_step_u8(*ml_batch(0, 2), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, micro=(0, 2))
    z0 = eng.logits_host().copy()
    assert "grad_norm" not in first and first["rows"] == 2 and "subset_correct" in first
    out = eng.train_step_u8(*ml_batch(2, 4), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, micro=(1, 2))
    z = np.concatenate([z0, eng.logits_host()])
    assert out["rows"] == 4 and eng.step_count == 1
    check_step(out, eng, oracle_step(4), LABELS[:4], logits=z)


def test_per_frame_fc_head():
    """classifier fc without frame fusion: one logits row per FRAME (6 rows) of 11 classes."""
    from vltf_amd.engine import LRCNEngine
    ncls = 11
    rng = np.random.default_rng(12)
    q = rng.uniform(0.25, 4.0, ncls).astype(np.float32)
    cfg = small_cfg(num_classes=ncls, classifier="fc", frame_fusion=None, **dict(ON, class_weights=q.tolist()))
    p = O.init_params(rng, ncls, "fc6", cfg.lstm_hidden, 1, SHAPE, classifier="fc", well_scaled=True)
    frames = rng.integers(0, 256, (B * FPC,) + SHAPE, dtype=np.uint8)
    labels = (rng.random((B * FPC, ncls)) < 0.3).astype(np.int32)
    labels[1] = 0
    with ML.oracle_loss(q, GAMMA):
        want = O.lrcn_train_step(p, frames.astype(np.float32) - MEAN, ML.targets(labels, 1.0, EPS), FPC, lr=LR, clip_norm=CLIP, classifier="fc",
                                 frame_fusion=None)
    eng = LRCNEngine(cfg, max_clips=B, device=DEV)
    eng.load_params(p)
    assert eng.loss_rows.numel() == 3 * B * FPC
    out = eng.train_step_u8(torch.tensor(frames, device=DEV), torch.tensor(labels, device=DEV), lr=LR, clip_norm=CLIP, mean_bgr=MEAN)
    assert out["rows"] == B * FPC and eng.logits_host().shape == (B * FPC, ncls)
    check_step(out, eng, want, labels)


def test_graph_engine_loss_with_lengths():
    """encdec_reshape of tests/graph_cases.py with per-clip lengths on both pipelines: the loss is a mean over the live steps, each a
    multi-hot row over the vocabulary; against the graph oracle of tests/seq_len_ref.py run on multilabel_ref's dlogits."""
    from vltf_amd.graph import GraphEngine
    items = 5
    case_, lens = GC.encdec(), {"enc": [1, 2, 2, 1, 2], "dec": [1, 4, 2, 3, 4]}
    q = np.random.default_rng(case_["V"]).uniform(0.25, 4.0, case_["V"]).astype(np.float32)
    pipes, ds = GC.specs_and_datasets(case_, items)
    eng = GraphEngine(pipes, ds, case_["V"], device=DEV, label_smoothing=EPS, class_weights=q.tolist(), focal_gamma=GAMMA, label_type="multiple")
    p = eng.init_params(seed=case_["seed"], well_scaled=True)
    eng.load_params(p)
    raw, feeds = GC.inputs(case_, items)
    fd = device_feeds(raw)
    got = eng.forward(fd, seq_len=lens).cpu().numpy()
    labels = (np.random.default_rng(0).random((got.shape[0], case_["V"])) < 0.2).astype(np.int32)
    with ML.oracle_loss(q, GAMMA):
        logits, mask, loss, grads, n_valid = R.model_with_lengths(p, case_, feeds, lens, ML.targets(labels, 1.0, EPS), items)
    assert eng.multilabel and eng.stats.numel() == 3 and eng.loss_rows.numel() == 3 * got.shape[0]
    out = eng.train_step(fd, torch.from_numpy(labels).to(DEV), lr=LR, clip_norm=CLIP, seq_len=lens)
    clipped, gn = O.clip_by_global_norm(grads, CLIP)
    print("loss %.8f want %.8f, grad norm %.8f want %.8f, exact %g of %d" % (out["loss"], loss, out["grad_norm"], gn, out["subset_correct"], n_valid))
    assert out["rows"] == n_valid == sum(lens["dec"])
    assert abs(out["loss"] - loss) < 1e-4 * max(1, abs(loss)) and abs(out["grad_norm"] - gn) < 1e-3 * gn
    assert out["correct"] == float(ML.hit1(got[mask], labels[mask]).sum())
    assert out["subset_correct"] == float(ML.exact(got[mask], labels[mask]).sum())
    newp = eng.get_params()
    for k in p:
        np.testing.assert_allclose(newp[k], p[k].astype(np.float64) - LR * clipped[k], rtol=1e-4, atol=1e-5, err_msg="param " + k)


def test_label_type_single_is_the_engine_of_before(monkeypatch):
    """label_type "single" / None, given or not: the workspace, the ops calls, the keys and the bytes of an engine built without the
    argument -- plain, with label smoothing and with mixup; ops.sigmoid_xent is never called."""
    import vltf_amd.ops as ops_
    from tests.test_label_smoothing_gpu import dev_batch
    from vltf_amd.engine import LRCNEngine
    calls = []

    def record(name):
        real = getattr(ops_, name)
        monkeypatch.setattr(ops_, name, lambda *a, **k: (calls.append(name), real(*a, **k))[1])

    for name in ("softmax_xent", "softmax_xent_ls", "softmax_xent_mix", "softmax_xent_wf", "sigmoid_xent"):
        record(name)
    p, _, _ = data()
    for base, name, cols in ((dict(), "softmax_xent", 2), (dict(label_smoothing=EPS, top_k=2), "softmax_xent_ls", 3),
                             (dict(mixup_alpha=0.2, mixup_seed=7), "softmax_xent_mix", 3)):
        res = []
        del calls[:]
        for kw in (dict(label_type="single"), dict(label_type=None), dict()):
            eng = LRCNEngine(small_cfg(**dict(base, **kw)), max_clips=B, device=DEV)
            eng.load_params(p)
            assert eng.stats.numel() == cols and eng.loss_rows.numel() == cols * B and not eng.multilabel
            out = eng.train_step_u8(*dev_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN)
            res.append((out, eng.logits_host().copy(), eng.get_params()))
        assert calls == [name] * 3
        for out, logits, params in res[:2]:
            assert out == res[2][0] and "subset_correct" not in out and np.array_equal(logits.view(np.int32), res[2][1].view(np.int32))
            for k in params:
                assert np.array_equal(params[k].view(np.int32), res[2][2][k].view(np.int32)), k
    eng = LRCNEngine(small_cfg(**ON), max_clips=B, device=DEV)                   # and multiple: the new launch alone
    eng.load_params(p)
    del calls[:]
    eng.train_step_u8(*ml_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN)
    assert calls == ["sigmoid_xent"]


# ---- 7. run_task on the example -------------------------------------------------------------------------------------------------------
def test_run_task_on_the_example(tmp_path, monkeypatch):
    """examples/lrcn_multilabel.yml shrunk: a synthetic multi-label dataset and the small network of tests/test_run_task_gpu.py, two
    batches, one epoch, with the example's own label_type and class_weights: balanced; the validation run writes the multi-label files,
    and map_<run_id> is multilabel_ref's brute-force number on the pickled logits."""
    from tests.test_run_task_gpu import RAW, write_cfg
    from vltf_amd import run_task, serialize
    from vltf_amd.settings_ import balanced_pos_weights
    monkeypatch.setenv("VLTF_PREFETCH", "0")
    monkeypatch.setenv("VLTF_CONV_MATH", "f32")
    monkeypatch.delenv("VLTF_STEP_GRAPH", raising=False)
    with open(os.path.join(ROOT, "examples", "lrcn_multilabel.yml")) as f:
        example = yaml.safe_load(f)["run"]
    assert example["network"]["label_type"] == "defs.label_type.multiple" and example["train"]["class_weights"] == "balanced"
    folder = str(tmp_path)
    rng = np.random.default_rng(1)

    def dataset(name, cpv, labels):
        path = os.path.join(folder, name)
        serialize.write_video_dataset(path, [rng.integers(0, 256, (c * 3,) + RAW, dtype=np.uint8) for c in cpv], labels, 3, list(cpv))
        return path

    tlabels, vlabels = [[0, 2], [1], [0, 1, 3], [2]], [[0, 1], [3], [1, 2]]
    train_path, val_path = dataset("train.txt", (1, 2, 1, 1), tlabels), dataset("val.txt", (2, 1, 2), vlabels)

    def cfg(name, path, phase, resume=None):
        out = write_cfg(folder, name, path, phase, resume=resume, epochs=1, det=True)
        with open(out) as f:
            c = yaml.safe_load(f)
        c["run"]["network"].update(label_type=example["network"]["label_type"])
        c["run"]["train"].update(class_weights=example["train"]["class_weights"])
        with open(out, "w") as f:
            yaml.safe_dump(c, f)
        return out

    run = os.path.join(folder, "run")
    run_task.main(cfg("train.yml", train_path, "train"), seed=3)
    log = open(glob.glob(os.path.join(run, "log_e2e_train_scratch_*.log"))[0]).read()
    q = np.asarray(balanced_pos_weights(tlabels, 4)[0], np.float32)
    assert q.tolist() == [1.0, 1.0, 1.0, 3.0]
    assert ("positive-term weights min %g (class %d), max %g (class %d)" % (q.min(), q.argmin(), q.max(), q.argmax())) in log
    assert "Loss: label_type multiple" in log and "global step: 2" in log and "subset accuracy : " in log
    acc = run_task.main(cfg("val.yml", val_path, "val", resume="latest"))
    tot = glob.glob(os.path.join(run, "validation_logits_e2e_val_resume_*.total"))
    assert len(tot) == 1
    with open(tot[0], "rb") as f:
        logits = pickle.load(f)                                                   # written by this run
    want = ML.metrics_brute(logits, O.labels_to_one_hot(vlabels, 4))
    read = lambda name: float(open(os.path.join(run, "%s_e2e_val_resume" % name)).read())
    assert read("accuracy") == acc == want["hit1"]
    assert read("map") == pytest.approx(want["map"], rel=1e-12) and read("subset_accuracy") == want["subset_accuracy"]
    assert read("f1_micro") == pytest.approx(want["f1_micro"], rel=1e-12) and read("f1_macro") == pytest.approx(want["f1_macro"], rel=1e-12)
    lines = [l.split() for l in open(os.path.join(run, "ap_per_class_e2e_val_resume")).read().splitlines()]
    assert [[int(v) for v in l[:2]] for l in lines] == [[0, 1], [1, 2], [2, 1], [3, 1]]
    np.testing.assert_allclose([float(l[2]) for l in lines], want["ap"], rtol=1e-12)
    assert "Validation mAP: %2.5f" % want["map"] in open(glob.glob(os.path.join(run, "log_e2e_val_resume_*.log"))[0]).read()
