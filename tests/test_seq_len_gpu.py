"""Per-clip sequence lengths on the device (vl_lstm_seq_fwd_len / _bwd_len, vl_temporal_fusion_*_len, vl_softmax_xent_len, and
GraphEngine / ComposedEngine `seq_len=`) against the existing oracle applied clip by clip to the live prefix
(tests/seq_len_ref.py, pinned in tests/test_seq_len.py).  Tolerances are those tests/test_ops_gpu.py and tests/test_graph_gpu.py
hold the same quantities to.  Dead rows of the kernels' inputs hold NaN: no output may depend on them."""
import math

import numpy as np
import pytest
import torch

from oracle import lrcn_oracle as O
from tests import graph_cases as GC
from tests import seq_len_ref as R
from tests.test_graph_gpu import device_feeds
from tests.test_ops_gpu import close, dev, host

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    import vltf_amd.ops as ops_
    return ops_


def mixed_lengths(b, T, H):
    lens = np.random.default_rng(b * H).integers(1, T + 1, b)
    lens[0], lens[1] = 1, T
    return lens


def idev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.int32, device=DEV)


def run_recurrence(ops, b, T, d, H, init, lens):
    """Forward + backward with lengths, NaN in every output buffer beforehand and in every dead row of gx / dout; every assertion of
    the op-level contract against the prefix oracle."""
    rng = np.random.default_rng(b * H)
    x = rng.standard_normal((b, T, d)).astype(np.float32)
    kern = (rng.standard_normal((d + H, 4 * H)) * (0.5 / math.sqrt(H))).astype(np.float32)
    bias = (rng.standard_normal(4 * H) * 0.1).astype(np.float32)
    s0 = (rng.standard_normal((b, H)) * 0.5).astype(np.float32) if init else None
    dout = rng.standard_normal((b, T, H)).astype(np.float32)
    want = R.lstm_layer(x, kern, bias, lens, s0=s0, dout=dout)
    live = R.live_rows(lens, T)
    dead = torch.from_numpy(~live).to(DEV)
    xd, kd, ld = dev(x.reshape(b * T, d)), dev(kern), idev(lens)
    s0d = dev(s0) if init else None
    gx = torch.empty((b * T, 4 * H), device=DEV)
    ops.gemm(xd, kd, gx, b * T, 4 * H, d, bias=dev(bias))
    gx[dead] = NAN
    act, cseq, hseq, hprev, dz = (torch.full((b * T, w), NAN, device=DEV) for w in (4 * H, H, H, H, 4 * H))
    ws = ops.lstm_seq_ws(b, T, H, DEV)
    ops.lstm_seq_fwd(gx, kd[d:], act, cseq, hseq, hprev, b, T, H, ws=ws, h0=s0d, c0=s0d, seq_len=ld)
    assert not ops.lstm_seq_timed_out(ws)
    doutd = dev(dout.reshape(b * T, H))
    doutd[dead] = NAN
    dh0, dc0 = (torch.full((b, H), NAN, device=DEV), torch.full((b, H), NAN, device=DEV)) if init else (None, None)
    ops.lstm_seq_bwd(doutd, kd[d:], act, cseq, dz, b, T, H, ws=ws, c0=s0d, dh0=dh0, dc0=dc0, seq_len=ld)
    assert not ops.lstm_seq_timed_out(ws)
    got = {k: host(v) for k, v in dict(act=act, cseq=cseq, hseq=hseq, hprev=hprev, dz=dz).items()}
    for k, v in got.items():
        assert np.isfinite(v).all(), k + " holds a non-finite value"
    for k in ("hseq", "dz", "act"):
        assert not got[k][~live].any(), "dead rows of %s are not exactly zero" % k
    tol = dict(rtol=3e-5, atol_rel=3e-5) if d >= 1024 else dict(rtol=1e-5, atol_rel=1e-6)
    close(got["cseq"].reshape(b, T, H)[:, T - 1], want["c_last"], msg="final c", **tol)
    close(got["hseq"].reshape(b, T, H), want["out"], msg="outputs", **tol)
    close(got["cseq"].reshape(b, T, H), want["c"], msg="cseq (dead rows: the carried c)", **tol)
    close(got["hprev"].reshape(b, T, H), want["hprev"], msg="hprev (dead rows: the carried h)", **tol)
    dk = torch.empty_like(kd)
    ops.gemm(xd, dz, dk, d, 4 * H, b * T, transa=True)
    ops.gemm(hprev, dz, dk[d:], H, 4 * H, b * T, transa=True)
    dx = torch.empty((b * T, d), device=DEV)
    ops.gemm(dz, kd, dx, b * T, d, 4 * H, transb=True)
    close(host(dk), want["dk"], rtol=1e-4, atol_rel=1e-5, msg="dkernel")
    close(host(dx).reshape(b, T, d), want["dx"], rtol=1e-4, atol_rel=1e-5, msg="dx")
    if init:
        close(host(dh0), want["dh0"], rtol=1e-4, atol_rel=1e-5, msg="dh0")
        close(host(dc0), want["dc0"], rtol=1e-4, atol_rel=1e-5, msg="dc0")


# 1 ---- recurrence, op level ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,T,d,H", [(5, 4, 24, 16), (11, 21, 50, 100), (8, 21, 300, 256), (64, 21, 300, 256), (8, 16, 4096, 256),
                                     (130, 5, 32, 256), (20, 7, 24, 512), (3, 4, 16, 600)])
@pytest.mark.parametrize("init", [False, True])
def test_recurrence_with_mixed_lengths(ops, b, T, d, H, init):
    """Cluster form at one clip per group, at 4 / 3 / 8 clips per group, over two launches (130 clips: the second launch's clip
    offset must reach the lengths), and the per-clip form (H = 600)."""
    run_recurrence(ops, b, T, d, H, init, mixed_lengths(b, T, H))


@pytest.mark.parametrize("init", [False, True])
@pytest.mark.parametrize("kind", ["all3", "short_group_long_group"])
def test_recurrence_decoder_shape_length_patterns(ops, kind, init):
    """Config 4's decoder (64 clips x 21 steps, 4 clips per group): every clip short; a whole group short next to a whole group long."""
    b, T, d, H = 64, 21, 300, 256
    if kind == "all3":
        lens = np.full(b, 3)
    else:
        lens = mixed_lengths(b, T, H)
        lens[0:4] = [1, 4, 2, 3]
        lens[4:8] = [18, 21, 19, 20]
        lens[8:12] = [1, T, 2, T - 1]
    run_recurrence(ops, b, T, d, H, init, lens)


# 2 ---- no lengths = the call as it was, bitwise ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,T,d,H", [(8, 21, 300, 256), (3, 4, 16, 600)])
def test_no_lengths_and_full_lengths_are_the_plain_call_bitwise(ops, b, T, d, H):
    rng = np.random.default_rng(b * H + 1)
    gx = dev((rng.standard_normal((b * T, 4 * H)) * 1.5).astype(np.float32))
    kh = dev((rng.standard_normal((H, 4 * H)) * 0.05).astype(np.float32))
    s0 = dev((rng.standard_normal((b, H)) * 0.5).astype(np.float32))
    dout = dev(rng.standard_normal((b * T, H)).astype(np.float32))
    ws = ops.lstm_seq_ws(b, T, H, DEV)
    res = []
    for kw in (None, dict(seq_len=None), dict(seq_len=idev(np.full(b, T)))):
        act, cseq, hseq, hprev, dz = (torch.zeros((b * T, w), device=DEV) for w in (4 * H, H, H, H, 4 * H))
        dh0, dc0 = torch.zeros((b, H), device=DEV), torch.zeros((b, H), device=DEV)
        if kw is None:
            ops.lstm_seq_fwd(gx, kh, act, cseq, hseq, hprev, b, T, H, 1.0, ws, s0, s0)
            ops.lstm_seq_bwd(dout, kh, act, cseq, dz, b, T, H, ws, s0, dh0, dc0)
        else:
            ops.lstm_seq_fwd(gx, kh, act, cseq, hseq, hprev, b, T, H, ws=ws, h0=s0, c0=s0, **kw)
            ops.lstm_seq_bwd(dout, kh, act, cseq, dz, b, T, H, ws=ws, c0=s0, dh0=dh0, dc0=dc0, **kw)
        assert not ops.lstm_seq_timed_out(ws)
        res.append([host(t).copy() for t in (hseq, cseq, dz, dh0)])
    assert np.abs(res[0][2]).max() > 0
    for other in res[1:]:
        for a, c in zip(res[0], other):
            assert np.array_equal(a, c)


# 3 ---- determinism ----------------------------------------------------------------------------------------------------------------------
def test_recurrence_with_lengths_is_deterministic_and_reentrant(ops):
    rng = np.random.default_rng(3)
    b, T, H = 24, 9, 256
    gx = dev((rng.standard_normal((b * T, 4 * H)) * 1.5).astype(np.float32))
    kh = dev((rng.standard_normal((H, 4 * H)) * 0.05).astype(np.float32))
    dout = dev(rng.standard_normal((b * T, H)).astype(np.float32))
    lens = idev(mixed_lengths(b, T, H))
    ws = ops.lstm_seq_ws(b, T, H, DEV)
    res = []
    for _ in range(2):
        act, cseq, hseq, hprev, dz = (torch.zeros((b * T, w), device=DEV) for w in (4 * H, H, H, H, 4 * H))
        ops.lstm_seq_fwd(gx, kh, act, cseq, hseq, hprev, b, T, H, ws=ws, seq_len=lens)
        ops.lstm_seq_bwd(dout, kh, act, cseq, dz, b, T, H, ws=ws, seq_len=lens)
        assert not ops.lstm_seq_timed_out(ws)
        res.append((host(hseq).copy(), host(dz).copy(), host(cseq).copy()))
    for a, c in zip(*res):
        assert np.array_equal(a, c)
    assert np.abs(res[0][1]).max() > 0


# 4 ---- fusion and loss, op level ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["avg", "last"])
def test_temporal_fusion_with_lengths(ops, method):
    rng = np.random.default_rng(11)
    b, T, H = 9, 7, 37
    x = rng.standard_normal((b, T, H)).astype(np.float32)
    d = rng.standard_normal((b, H)).astype(np.float32)
    lens = mixed_lengths(b, T, H)
    want_y, want_g = R.fusion(x.astype(np.float64), lens, method, d)
    xd = dev(x.reshape(b * T, H))
    xd[torch.from_numpy(~R.live_rows(lens, T)).to(DEV)] = NAN             # dead steps are not read
    y, g = torch.full((b, H), NAN, device=DEV), torch.full((b * T, H), NAN, device=DEV)
    ops.temporal_fusion_fwd(xd, y, b, T, H, method, seq_len=idev(lens))
    ops.temporal_fusion_bwd(dev(d), g, b, T, H, method, seq_len=idev(lens))
    close(host(y), want_y, rtol=1e-6, atol_rel=1e-7, msg=method)
    close(host(g).reshape(b, T, H), want_g, rtol=1e-6, atol_rel=1e-7, msg=method + " grad")
    assert not host(g)[~R.live_rows(lens, T)].any()


@pytest.mark.parametrize("clips,T,C", [(8, 21, 1000), (3, 4, 7)])
@pytest.mark.parametrize("rows_ws", [False, True])
def test_softmax_xent_with_lengths(ops, clips, T, C, rows_ws):
    rng = np.random.default_rng(clips * C)
    n = clips * T
    logits = (rng.standard_normal((n, C)) * 2).astype(np.float32)
    onehot = O.labels_to_one_hot([[l] for l in rng.integers(0, C, n)], C)
    lens = mixed_lengths(clips, T, C)
    live = R.live_rows(lens, T)
    # every third live row is a hit, so that the count is not trivially zero: its LABEL is moved to the arg-max, the logits stay as
    # drawn.  (Raising the label's logit by 20 instead makes p = 1 - 6e-5 in that row, and dlogits = p - 1 is then a cancellation whose
    # fp32 error -- one ulp of lse at |z| = 25 is 2e-6 -- exceeds atol_rel 1e-6 in any fp32 softmax, lengths or not: a plain fp32
    # restatement of the row arithmetic misses the bound on such inputs by the same 1.2e-8.)
    for r in np.flatnonzero(live)[::3]:
        onehot[r] = 0
        onehot[r, np.argmax(logits[r])] = 1
    loss_sum, hits, want_dl, loss = R.xent(logits, onehot, lens, T)
    ld = dev(logits)
    ld[torch.from_numpy(~live).to(DEV)] = NAN
    dl = torch.full((n, C), NAN, device=DEV)
    stats = torch.zeros(2, device=DEV)
    rows = torch.full((2 * n,), NAN, device=DEV) if rows_ws else None
    ops.softmax_xent(ld, dev(onehot, torch.int32), dl, stats, 1.0 / int(live.sum()), rows, seq_len=idev(lens), T=T)
    st, got = host(stats), host(dl)
    assert hits > 0 and st[1] == hits
    assert abs(st[0] / int(live.sum()) - loss) < 1e-5 * max(1.0, abs(loss))          # stats[0] = the SUM of the live rows' losses
    assert not got[~live].any(), "dlogits of a dead row is not exactly zero"
    close(got, want_dl, rtol=1e-4, atol_rel=1e-6, msg="dlogits")


# 5 - 7 ---- engine ----------------------------------------------------------------------------------------------------------------------
ITEMS = 5


def engine_case(name):
    """-> (case, lengths per pipeline): mixed, with 1 and fpc on every pipeline that gets lengths."""
    if name == "encdec_reshape":
        return GC.encdec(), {"enc": [1, 2, 2, 1, 2], "dec": [1, 4, 2, 3, 4]}
    if name == "encdec_avg":
        return GC.encdec(None, 1, "avg"), {"enc": [2, 1, 1, 2, 2], "dec": [4, 1, 3, 2, 4]}
    return R.single_lstm_case(6), {"net": [1, 6, 3, 5, 2]}


def build(case, items=ITEMS):
    from vltf_amd.graph import GraphEngine
    pipes, ds = GC.specs_and_datasets(case, items)
    eng = GraphEngine(pipes, ds, case["V"], device=DEV)
    p = eng.init_params(seed=case["seed"], well_scaled=True)
    eng.load_params(p)
    return eng, p


def labels_for(case, rows, seed=0):
    return O.labels_to_one_hot([[l] for l in np.random.default_rng(seed).integers(0, case["V"], rows)], case["V"])


@pytest.mark.parametrize("name", ["encdec_reshape", "encdec_avg", "single_last"])
def test_engine_with_mixed_lengths_matches_the_oracle(name):
    case, lens = engine_case(name)
    eng, p = build(case)
    raw, feeds = GC.inputs(case, ITEMS)
    fd = device_feeds(raw)
    got = eng.forward(fd, seq_len=lens).cpu().numpy()
    onehot = labels_for(case, got.shape[0])
    logits, mask, loss, grads, n_valid = R.model_with_lengths(p, case, feeds, lens, onehot, ITEMS)
    assert got.shape[0] == mask.shape[0] and np.isfinite(got).all()
    np.testing.assert_allclose(got[mask], logits, rtol=1e-3, atol=1e-3)
    out = eng.train_step(fd, torch.from_numpy(onehot).to(DEV), lr=0.01, clip_norm=0.5, seq_len=lens)
    assert abs(out["loss"] - loss) < 1e-4 * max(1, abs(loss))
    clipped, gn = O.clip_by_global_norm(grads, 0.5)
    assert abs(out["grad_norm"] - gn) < 1e-3 * gn
    if name == "encdec_reshape":
        assert out["rows"] == n_valid == sum(lens["dec"])
        acc = O.accuracy(logits, onehot[mask])
        assert abs(out["accuracy"] - acc) < 1e-6
    else:
        assert out["rows"] == ITEMS
    g = eng.get_grads()
    assert set(g) == set(p)
    for k in p:
        scale = np.abs(grads[k]).max() + 1e-12
        np.testing.assert_allclose(g[k], grads[k], rtol=2e-3, atol=2e-4 * scale, err_msg="grad " + k)
    newp = eng.get_params()
    for k in p:
        np.testing.assert_allclose(newp[k], p[k].astype(np.float64) - 0.01 * clipped[k], rtol=1e-4, atol=1e-5, err_msg="param " + k)
    assert any(np.abs(grads[k]).max() > 0 for k in p if k.endswith("dcnn/conv1W")), "no gradient reached a tower"


def test_engine_padding_is_inert():
    """Different frames / word vectors in the dead steps of both datasets change nothing: live-row logits, the loss and every
    parameter after the step are bitwise equal (every op works row by row or frame by frame, and a dead row enters each
    weight-gradient sum as x * 0, an exact zero in fp32)."""
    case, lens = engine_case("encdec_reshape")
    raw, _ = GC.inputs(case, ITEMS)
    res = []
    for fill_seed in (None, 99):
        eng, p = build(case)
        fed = {t: v.copy() for t, v in raw.items()}
        if fill_seed is not None:
            rng = np.random.default_rng(fill_seed)
            for tag, pipe in (("main", "enc"), ("aux", "dec")):
                T = case["data"][tag]["fpc"]
                dead = ~R.live_rows(lens[pipe], T)
                assert dead.any()
                v = fed[tag]
                v[dead] = rng.integers(0, 256, v[dead].shape, dtype=np.uint8) if v.dtype == np.uint8 else \
                    (rng.standard_normal(v[dead].shape) * 3).astype(np.float32)
            assert any(not np.array_equal(fed[t], raw[t]) for t in raw)
        fd = device_feeds(fed)
        got = eng.forward(fd, seq_len=lens).cpu().numpy()
        onehot = labels_for(case, got.shape[0])
        out = eng.train_step(fd, torch.from_numpy(onehot).to(DEV), lr=0.01, clip_norm=0.5, seq_len=lens)
        res.append((got[R.live_rows(lens["dec"], case["data"]["aux"]["fpc"])], out["loss"], eng.get_params()))
    assert np.array_equal(res[0][0], res[1][0])
    assert res[0][1] == res[1][1]
    for k in res[0][2]:
        assert np.array_equal(res[0][2][k], res[1][2][k]), "parameter %s moved with the padding" % k


def test_engine_uniform_length_is_the_shorter_model():
    """A 6-step model fed seq_len = 4 everywhere is the 4-step model on the first four frames of each clip."""
    long_case, short_case = R.single_lstm_case(6), R.single_lstm_case(4)
    raw, _ = GC.inputs(long_case, ITEMS)
    frames = raw["main"].reshape((ITEMS, 6) + raw["main"].shape[1:])
    short_raw = {"main": np.ascontiguousarray(frames[:, :4]).reshape((ITEMS * 4,) + raw["main"].shape[1:])}
    onehot = labels_for(long_case, ITEMS)
    res = []
    for case, r, kw in ((long_case, raw, dict(seq_len={"net": [4] * ITEMS})), (short_case, short_raw, {})):
        eng, p = build(case)
        fd = device_feeds(r)
        logits = eng.forward(fd, **kw).cpu().numpy()
        out = eng.train_step(fd, torch.from_numpy(onehot).to(DEV), lr=0.01, clip_norm=0.5, **kw)
        res.append((logits, out, eng.get_params(), p))
    assert all(np.array_equal(res[0][3][k], res[1][3][k]) for k in res[0][3])          # same parameters to start from
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=1e-3, atol=1e-3)
    assert abs(res[0][1]["loss"] - res[1][1]["loss"]) < 1e-4 * max(1, abs(res[1][1]["loss"]))
    for k in res[0][2]:
        np.testing.assert_allclose(res[0][2][k], res[1][2][k], rtol=1e-4, atol=1e-5, err_msg="param " + k)


# 8 ---- ComposedEngine --------------------------------------------------------------------------------------------------------------------
def test_composed_engine_passes_lengths_through():
    from vltf_amd.composed import ComposedEngine, HeadConfig
    from vltf_amd.engine import NetConfig
    case, _ = engine_case("encdec_reshape")
    lens = {"dec": [1, 4, 2, 3, 4]}
    eng, p = build(case)
    raw, _ = GC.inputs(case, ITEMS)
    fd = device_feeds(raw)
    want = eng.forward(fd, seq_len=lens).cpu().numpy()
    enc = NetConfig(image_shape=GC.SHAPE, num_classes=case["V"], fpc=2, frame_encoding_layer="fc6", classifier="lstm", lstm_hidden=6,
                    lstm_layers=1, fusion="state")
    head = HeadConfig(in_dim=5, fpc=4, num_classes=case["V"], lstm_hidden=8, lstm_layers=2, fusion="reshape")
    ce = ComposedEngine(enc, head, ITEMS, device=DEV)
    ce.load_params(p)
    got = ce.forward(fd["main"]["frames_u8"], fd["aux"], mean_bgr=GC.MEAN, seq_len=lens).cpu().numpy()
    assert np.array_equal(got, want)
    plain = ce.forward(fd["main"]["frames_u8"], fd["aux"], mean_bgr=GC.MEAN).cpu().numpy()
    live = R.live_rows(lens["dec"], 4)
    assert np.array_equal(plain[live], want[live]) and not np.array_equal(plain[~live], want[~live])
    onehot = labels_for(case, got.shape[0])
    a = ce.train_step(fd["main"]["frames_u8"], fd["aux"], torch.from_numpy(onehot).to(DEV), lr=0.01, clip_norm=0.5, mean_bgr=GC.MEAN,
                      seq_len=lens)
    b = eng.train_step(fd, torch.from_numpy(onehot).to(DEV), lr=0.01, clip_norm=0.5, seq_len=lens)
    assert a["rows"] == b["rows"] == sum(lens["dec"]) and a["loss"] == b["loss"]
