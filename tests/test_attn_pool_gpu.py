"""The attention pooling launches (csrc/pointwise.hip: attn_pool_fwd_kernel / attn_pool_bwd_kernel) against the fp64 reference of
tests/attn_pool_ref.py, then the engines that run on them.

Cases (attn_pool_ref.CASES as (batch, T, HO, A)): one element; widths below a wave; ragged last waves of A and HO with more steps than
waves; the flagship widths; widths above one pass of the 256-thread workgroup; A just past two waves; T = 64 with A one past a wave;
HO of four passes.  Every case runs at both input scales, without and with per-clip lengths (lstm_plan.lengths: a 0, a T, a -3 and a
T + 5, clamped to 1..T by the fusion's rule), and with lengths the dead rows of h, u and s hold NaN.

Tolerances are the project's classes (tests/test_lstm_geometry_gpu.TOL) as tests/test_attn_pool.py assigns them: s, alpha, y, du, dcp
act (3e-5, 3e-5); dh hseq (1e-5, 1e-6).  The backward runs FROM the reference's own s and alpha rounded to fp32.  Every output is a
Guarded view (sentinels around it, NaN inside beforehand)."""
import os
import socket

import numpy as np
import pytest
import torch

from tests import attn_pool_ref as R
from tests import lstm_plan as P
from tests.test_lstm_geometry_gpu import DEV, Guarded, put, same_bits, within

pytestmark = pytest.mark.gpu

CLASS = dict(s="act", alpha="act", y="act", dh="hseq", du="act", dcp="act")        # tests/test_attn_pool.py decides these
OUT = ("s", "alpha", "y", "du", "dh", "dcp")


@pytest.fixture(scope="module")
def ops():
    import vltf_amd.ops as ops_
    return ops_


def shapes(case):
    batch, T, HO, A = case
    return dict(s=(batch * T, A), alpha=(batch, T), y=(batch, HO), du=(batch * T, A), dh=(batch * T, HO), dcp=(batch, A))


def run_pool(ops, case, inp, lens, s32, alpha32, alias=False, what=""):
    """attn_pool_fwd on the inputs (NaN in the dead rows of h and u), attn_pool_bwd on the s and alpha given (NaN in the dead rows of s);
    the memory checks; -> {output: array}.  alias: s is written over u."""
    batch, T, HO, A = case
    nan = (lambda a: a) if lens is None else (lambda a: R.with_nan_in_dead_rows(a, T, lens))
    h, c, dy = put(nan(inp.h), DEV), put(inp.c, DEV), put(inp.dy, DEV)
    L = put(lens, DEV, torch.int32)
    o = {k: Guarded(shp, DEV) for k, shp in shapes(case).items()}
    if alias:
        o["s"].t.copy_(put(nan(inp.u), DEV))
        u = o["s"].t
    else:
        u = put(nan(inp.u), DEV)
    ops.attn_pool_fwd(u, c, h, o["s"].t, o["alpha"].t, o["y"].t, batch, T, HO, A, seq_len=L)
    ops.attn_pool_bwd(dy, h, put(nan(s32), DEV), put(alpha32, DEV), c, o["du"].t, o["dh"].t, o["dcp"].t, batch, T, HO, A, seq_len=L)
    return {k: g.settle(what + " " + k) for k, g in o.items()}


def run_ref(ops, case, ref, **kw):
    return run_pool(ops, case, ref.inp, ref.lens, ref.s32, ref.alpha32, **kw)


# ---- 1. the kernels against the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
@pytest.mark.parametrize("k", R.SCALES, ids=lambda k: "k%d" % k)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_attn_pool_against_the_reference(ops, case, k, lens):
    batch, T, HO, A = case
    what = "attn_pool %s k%d %s" % (R.case_id(case), k, "lens" if lens else "full")
    ref = R.reference(case, k, lens)
    got = run_ref(ops, case, ref, what=what)
    want = dict(ref.fwd._asdict(), **ref.bwd._asdict())
    for name in OUT:
        within(CLASS[name], got[name], want[name], what + " " + name)
    if lens:
        dead = ~R.live_mask(ref.lens, batch, T).reshape(-1)
        assert batch == 1 or (dead.any() and not dead.all())
        for name in ("s", "du", "dh"):
            assert not got[name][dead].any(), "%s: dead row of %s not zero" % (what, name)
        assert not got["alpha"].reshape(-1)[dead].any(), what + ": dead step of alpha not zero"
    # s written over u: the same bits
    same_bits(run_ref(ops, case, ref, alias=True, what=what + " aliased"), got, what + ": s aliasing u")


# ---- 2. bit for bit ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
def test_repeatable_and_a_clip_alone_equals_the_clip_in_a_batch(ops, lens):
    case = batch, T, HO, A = (5, 16, 256, 256)
    ref = R.reference(case, 1, lens)
    whole = run_ref(ops, case, ref, what="attn_pool")
    same_bits(run_ref(ops, case, ref, what="attn_pool again"), whole, "attn_pool: a second run")
    inp = ref.inp
    for b in range(batch):
        rows, row = slice(b * T, (b + 1) * T), slice(b, b + 1)
        one = R.Inputs(inp.h[rows], inp.u[rows], inp.c, inp.dy[row])
        alone = run_pool(ops, (1, T, HO, A), one, None if ref.lens is None else ref.lens[row], ref.s32[rows], ref.alpha32[row],
                         what="attn_pool clip %d alone" % b)
        part = {k: v[row] if v.shape[0] == batch else v[rows] for k, v in whole.items()}
        same_bits(alone, part, "attn_pool: clip %d alone against the batch of %d" % (b, batch))


# ---- 3. degenerate cases -----------------------------------------------------------------------------------------------------------------
def test_one_step_gives_weight_one_no_score_gradient_and_y_equal_to_h(ops):
    case = batch, T, HO, A = (3, 1, 37, 5)
    ref = R.reference(case, 3, False)
    got = run_ref(ops, case, ref, what="attn_pool T = 1")
    assert (got["alpha"] == 1.0).all() and not got["du"].any() and not got["dcp"].any()
    same_bits(dict(y=got["y"], dh=got["dh"]), dict(y=np.asarray(ref.inp.h), dh=np.asarray(ref.inp.dy)), "attn_pool T = 1")


def test_scores_of_two_hundred_stay_finite(ops):
    case = batch, T, HO, A = (2, 21, 250, 64)
    inp = R.inputs(*case)
    u = (np.where(np.arange(batch * T)[:, None] % T % 2 == 0, 50.0, -50.0) * np.ones((1, A))).astype(np.float32)
    c = np.full(A, 200.0 / A, np.float32)
    fwd = R.forward(inp.h, u, c, None, T)
    got = run_pool(ops, case, R.Inputs(inp.h, u, c, inp.dy), None, P.rounded(fwd.s), P.rounded(fwd.alpha), what="attn_pool +-200")
    np.testing.assert_allclose(got["alpha"].astype(np.float64).sum(axis=1), 1.0, rtol=0, atol=1e-6)
    assert (got["alpha"][:, 1::2] == 0).all()                       # exp(-400) is below the smallest fp32 subnormal
    within("act", got["y"], fwd.y, "attn_pool +-200 y")


@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
def test_a_zero_context_is_the_avg_fusion(ops, lens):
    case = batch, T, HO, A = (4, 7, 96, 130)
    ref = R.reference(case, 1, lens)
    zero = ref.inp._replace(c=np.zeros(A, np.float32))
    got = run_pool(ops, case, zero, ref.lens, ref.s32, ref.alpha32, what="attn_pool c = 0")
    L = put(ref.lens, DEV, torch.int32)
    avg = Guarded((batch, HO), DEV)
    h = ref.inp.h if ref.lens is None else R.with_nan_in_dead_rows(ref.inp.h, T, ref.lens)
    ops.temporal_fusion_fwd(put(h, DEV), avg.t, batch, T, HO, "avg", seq_len=L)
    within("hseq", got["y"], avg.settle("temporal_fusion_fwd avg"), "attn_pool c = 0 against temporal_fusion_fwd avg")
    Lc = R.fusion_lens(ref.lens, batch, T)
    within("act", got["alpha"], R.live_mask(ref.lens, batch, T) / Lc[:, None], "attn_pool c = 0 alpha")
    assert not got["du"].any()


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ops):
    """T = 1025, A = 0 and a null pointer raise; nothing is launched."""
    T = 1025
    case = (1, T, 2, 3)
    o = {k: Guarded(shp, DEV) for k, shp in shapes(case).items()}
    r = np.random.default_rng(0)
    f = lambda *shape: put(r.standard_normal(shape).astype(np.float32), DEV)
    u, c, h, dy, s, alpha = f(T, 3), f(3), f(T, 2), f(1, 2), f(T, 3), f(1, T)
    fwd = lambda T_=4, A=3, c_=c, u_=u: ops.attn_pool_fwd(u_, c_, h, o["s"].t, o["alpha"].t, o["y"].t, 1, T_, 2, A)
    bwd = lambda T_=4, A=3, c_=c, dy_=dy: ops.attn_pool_bwd(dy_, h, s, alpha, c_, o["du"].t, o["dh"].t, o["dcp"].t, 1, T_, 2, A)
    for call, kw, match in ((fwd, dict(T_=T), "exceeds 1024"), (bwd, dict(T_=T), "exceeds 1024"), (fwd, dict(A=0), "must be positive"),
                            (bwd, dict(A=0), "must be positive"), (fwd, dict(T_=0), "must be positive"), (fwd, dict(c_=None), "null pointer"),
                            (fwd, dict(u_=None), "null pointer"), (bwd, dict(c_=None), "null pointer"), (bwd, dict(dy_=None), "null pointer")):
        with pytest.raises(Exception, match=match):
            call(**kw)
    with pytest.raises(Exception, match="elements"):                # a tensor smaller than the launch would read
        ops.attn_pool_fwd(u, c, h, o["s"].t, o["alpha"].t, o["y"].t, 2, T - 1, 2, 3)
    torch.cuda.synchronize()
    assert all(g.untouched() for g in o.values()), "attn_pool: refused, yet an output was written"
    fwd()                                                           # (the arguments are good otherwise)
    torch.cuda.synchronize()
    assert all(o[k].untouched() for k in ("du", "dh", "dcp")) and not o["y"].untouched()


# ---- 5. LRCNEngine -----------------------------------------------------------------------------------------------------------------------
MEAN = np.array([99.197148, 105.293620, 109.503945], np.float32)
SHAPE, NCLS, FPC, CLIPS, ATTN = (67, 67, 3), 7, 3, 2, 5                      # the smoke() geometry of tests/test_gru_gpu.py
CELL_KW = dict(lstm=dict(), gru=dict(rnn_cell="gru"), blstm=dict(lstm_bidirectional=True))


@pytest.mark.parametrize("cell,layers,H,ATTN", [("lstm", 1, 8, 5), ("gru", 2, 8, 5), ("blstm", 1, 8, 5), ("lstm", 1, 128, 128)])
def test_lrcn_engine_train_step_against_the_reference(cell, layers, H, ATTN):
    """The last case runs the launches at two full waves of HO and A inside an engine.  Logits, loss, gradient norm, every gradient and the clipped SGD step against attn_pool_ref.model_train_step at the bounds of
    tests/test_gru_gpu.test_lrcn_engine_train_step_against_the_reference (seed 6 for the reason tests/test_blstm_gpu.py gives); a
    gradient reaches all three attention variables; attention_weights() is the reference's alpha."""
    from vltf_amd.engine import LRCNEngine, NetConfig, param_specs
    rng = np.random.default_rng(6)
    cfg = NetConfig(image_shape=SHAPE, num_classes=NCLS, fpc=FPC, frame_encoding_layer="fc6", lstm_hidden=H, lstm_layers=layers, fusion="attn",
                    attn_dim=ATTN, **CELL_KW[cell])
    eng = LRCNEngine(cfg, max_clips=CLIPS, device=DEV)
    p = R.init_params(rng, NCLS, "fc6", H, layers, SHAPE, cell, ATTN)
    assert {n: tuple(s) for n, s in param_specs(cfg)} == {n: v.shape for n, v in p.items()}
    eng.load_params(p)
    frames = rng.integers(0, 256, (CLIPS * FPC,) + SHAPE, dtype=np.uint8)
    onehot = np.eye(NCLS, dtype=np.int32)[rng.integers(0, NCLS, CLIPS)]
    x = frames.astype(np.float32) - MEAN
    newp, loss, gn, logits, grads, alpha = R.model_train_step(p, x, onehot, FPC, 0.01, 0.5, "fc6", H, layers, cell)
    fd = torch.tensor(frames, device=DEV)
    got_fwd = eng.forward_u8(fd, MEAN).cpu().numpy()
    assert got_fwd.shape == logits.shape
    np.testing.assert_allclose(got_fwd, logits, rtol=1e-3, atol=1e-3)
    got_alpha = eng.attention_weights().cpu().numpy()
    assert got_alpha.shape == (CLIPS, FPC) == alpha.shape
    np.testing.assert_allclose(got_alpha, alpha, rtol=1e-3, atol=1e-3)       # weights in [0, 1] behind the same tower as the logits
    np.testing.assert_allclose(got_alpha.astype(np.float64).sum(axis=1), 1.0, rtol=0, atol=1e-6)
    assert np.ptp(alpha, axis=1).min() > 1e-3                                # (the reference's weights are not the uniform ones)
    out = eng.train_step_u8(fd, torch.tensor(onehot, device=DEV), lr=0.01, clip_norm=0.5, mean_bgr=MEAN)
    assert abs(out["loss"] - loss) < 1e-4 * max(1, abs(loss))
    assert abs(out["grad_norm"] - gn) < 1e-3 * gn
    g = eng.get_grads()
    assert set(g) == set(p) and set(R.param_names()) <= set(g)
    for k in p:
        scale = np.abs(grads[k]).max() + 1e-12
        np.testing.assert_allclose(g[k], grads[k], rtol=2e-3, atol=2e-4 * scale, err_msg="grad " + k)
        assert scale > 1e-9, "no gradient reached " + k
    got = eng.get_params()
    for k in p:
        np.testing.assert_allclose(got[k], newp[k], rtol=1e-4, atol=1e-5, err_msg="param " + k)


@pytest.mark.parametrize("math", ("f32", "bf16x3", "bf16"))
def test_the_attention_products_are_fp32_under_every_conv_math(math):
    """8 clips x 16 frames, H = A = 128: all three attention products have 128 rows, columns and depth, the sizes from which ops.gemm
    WITH a workspace follows conv_math into split-bf16 arithmetic.  They are called without one, as the head's are: each is compared
    with the fp64 product of the operands THE DEVICE holds, at class act (3e-5, 3e-5) -- an fp32 product of depth 128 is two orders of
    magnitude inside it, a single-plane bf16 product (2^-9 per factor) two orders outside.  The pooling between them is held to the
    reference from the same operands."""
    from vltf_amd.engine import LRCNEngine, NetConfig, init_params
    clips, fpc, H, A = 8, 16, 128, 128
    n = clips * fpc
    cfg = NetConfig(image_shape=SHAPE, num_classes=NCLS, fpc=fpc, frame_encoding_layer="fc6", lstm_hidden=H, fusion="attn", attn_dim=A,
                    conv_math=math)
    p = init_params(cfg, seed=3, well_scaled=True)
    kn, bn, cn = R.param_names()
    p[bn] = (0.1 * np.random.default_rng(5).standard_normal(A)).astype(np.float32)
    eng = LRCNEngine(cfg, max_clips=clips, device=DEV)
    eng.load_params(p)
    rng = np.random.default_rng(12)
    frames = torch.from_numpy(rng.integers(0, 256, (n,) + SHAPE, dtype=np.uint8)).to(DEV)
    onehot = torch.from_numpy(np.eye(NCLS, dtype=np.int32)[rng.integers(0, NCLS, clips)]).to(DEV)
    out = eng.train_step_u8(frames, onehot, lr=0.01, clip_norm=0.0, mean_bgr=MEAN)
    assert np.isfinite(out["loss"]) and out["rows"] == clips
    host = lambda t: t.detach().cpu().numpy().astype(np.float64)
    hseq, s, alpha, du, dproj = (host(t) for t in (eng.lstm[-1]["hseq"][:n], eng.attn["us"][:n], eng.attention_weights(), eng.attn["du"][:n],
                                                   eng.attn["dproj"][:n]))
    W, b, c = (p[k].astype(np.float64) for k in (kn, bn, cn))
    assert np.abs(hseq).max() > 1e-2 and np.abs(du).max() > 0
    fwd = R.forward(hseq, hseq @ W + b, c, None, fpc)
    what = "attention products under conv_math %s: " % math
    within("act", s, fwd.s, what + "s = tanh(hseq W + b)")
    within("act", alpha, fwd.alpha, what + "alpha")
    within("act", host(eng.fused[:clips]), fwd.y, what + "y")
    within("act", host(eng.G[kn]), hseq.T @ du, what + "G[kernel] = hseq^T du")
    within("act", host(eng.G[bn]), du.sum(axis=0), what + "G[bias]")
    within("act", dproj, du @ W.T, what + "dproj = du W^T")


# ---- 6. the captured step ----------------------------------------------------------------------------------------------------------------
def test_lrcn_engine_captured_step_is_the_eager_step():
    """step_graph with dropout: the warm-up step, the captured one and three replays equal the eager engine's bit for bit -- the two
    attention launches take no host-varying argument and replay as they are."""
    from vltf_amd.engine import LRCNEngine, NetConfig, init_params
    engines = []
    kw = dict(image_shape=SHAPE, num_classes=NCLS, fpc=FPC, frame_encoding_layer="fc6", lstm_hidden=16, lstm_layers=2, fusion="attn",
              attn_dim=ATTN, dropout_keep_prob=0.5)
    params = init_params(NetConfig(**kw), seed=4, well_scaled=True)
    for sg in (False, True):
        e = LRCNEngine(NetConfig(step_graph=sg, **kw), max_clips=CLIPS, device=DEV)
        e.load_params(params)
        engines.append(e)
    rng = np.random.default_rng(11)
    for step in range(5):
        frames = torch.from_numpy(rng.integers(0, 256, (CLIPS * FPC,) + SHAPE, dtype=np.uint8)).to(DEV)
        onehot = torch.from_numpy(np.eye(NCLS, dtype=np.int32)[rng.integers(0, NCLS, CLIPS)]).to(DEV)
        outs = [e.train_step_u8(frames, onehot, 0.01 * 0.7 ** step, 5.0, MEAN) for e in engines]
        for k in ("loss_sum", "correct", "grad_norm", "rows"):
            assert outs[0][k] == outs[1][k], (step, k, outs[0][k], outs[1][k])
        assert np.array_equal(engines[0].logits_host(), engines[1].logits_host()), step
        assert torch.equal(engines[0].attention_weights(), engines[1].attention_weights()), step
    assert len(engines[1]._graphs) == 1
    pa, pb = engines[0].get_params(), engines[1].get_params()
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), k
    assert not np.array_equal(pa["attention_pool/context"], params["attention_pool/context"])


# ---- 7. GraphEngine: the vector-input pipeline of tests/test_gru_gpu.py with lengths ------------------------------------------------------
def test_graph_engine_with_lengths_against_the_reference():
    from tests import gru_ref
    from tests.test_gru_gpu import G_C, G_CLIPS, G_DIM, G_H, graph_engine
    T, lens = 5, np.array([5, 2, 1, 4])
    eng, p = graph_engine(T, fusion="attn")
    kn, bn, cn = R.param_names()
    assert p[kn].shape == (G_H, G_H) and p[cn].shape == (G_H, 1)              # attn_dim defaults to the output width
    x = (np.random.default_rng(8).standard_normal((G_CLIPS * T, G_DIM))).astype(np.float32)
    onehot = np.eye(G_C, dtype=np.int32)[np.random.default_rng(9).integers(0, G_C, G_CLIPS)]
    fd = {"main": torch.from_numpy(x).to(DEV)}
    got = eng.forward(fd, seq_len={"net": lens}).cpu().numpy()
    out, caches = gru_ref.stack_forward(x, p, T, G_H, 2, lens=lens)
    fused, pc = R.pool_layer_forward(out, p[kn], p[bn], p[cn], T, lens)
    want = fused @ p["output_fc_w"].astype(np.float64) + p["output_fc_b"]
    np.testing.assert_allclose(got, want, rtol=1e-3, atol=1e-3)
    # one step: every gradient against the reference
    from oracle import lrcn_oracle as O
    loss, d = O.softmax_xent_mean(want, onehot, np.float64)
    grads = {"output_fc_w": fused.T @ d, "output_fc_b": d.sum(0)}
    dout, grads[kn], grads[bn], grads[cn] = R.pool_layer_backward(d @ p["output_fc_w"].astype(np.float64).T, pc)
    grads.update(gru_ref.stack_backward(dout, caches)[1])
    res = eng.train_step(fd, torch.from_numpy(onehot).to(DEV), lr=0.01, clip_norm=0.0, seq_len={"net": lens})
    assert abs(res["loss"] - loss) < 1e-4 * max(1, abs(loss))
    g = eng.get_grads()
    assert set(g) == set(grads)
    for k in grads:
        scale = np.abs(grads[k]).max() + 1e-12
        np.testing.assert_allclose(g[k], grads[k], rtol=2e-3, atol=2e-4 * scale, err_msg="grad " + k)
        assert scale > 1e-9, "no gradient reached " + k


def test_graph_engine_padding_is_inert():
    """Other vectors in the dead steps change nothing: logits, the loss and every parameter after the step are bitwise equal."""
    from tests.test_gru_gpu import G_C, G_CLIPS, G_DIM, graph_engine
    T, lens = 5, [5, 2, 1, 4]
    live = R.live_mask(np.array(lens), G_CLIPS, T).reshape(-1)
    x = (np.random.default_rng(8).standard_normal((G_CLIPS * T, G_DIM))).astype(np.float32)
    onehot = torch.from_numpy(np.eye(G_C, dtype=np.int32)[np.random.default_rng(9).integers(0, G_C, G_CLIPS)]).to(DEV)
    res = []
    for fill in (None, 99):
        eng, _ = graph_engine(T, fusion="attn")
        fed = x.copy()
        if fill is not None:
            fed[~live] = (np.random.default_rng(fill).standard_normal(fed[~live].shape) * 3).astype(np.float32)
        fd = {"main": torch.from_numpy(fed).to(DEV)}
        got = eng.forward(fd, seq_len={"net": lens}).cpu().numpy()
        out = eng.train_step(fd, onehot, lr=0.01, clip_norm=0.5, seq_len={"net": lens})
        assert out["rows"] == G_CLIPS
        res.append((got, out["loss"], eng.get_params()))
    assert np.array_equal(res[0][0], res[1][0]) and res[0][1] == res[1][1]
    for k in res[0][2]:
        assert np.array_equal(res[0][2][k], res[1][2][k]), "parameter %s moved with the padding" % k


def test_graph_engine_uniform_length_is_the_shorter_model():
    """Clips of length 3 in a 5-step batch give what they give in a 3-step model: logits, loss and the step."""
    from tests.test_gru_gpu import G_C, G_CLIPS, G_DIM, graph_engine
    T, L = 5, 3
    x = (np.random.default_rng(8).standard_normal((G_CLIPS, T, G_DIM))).astype(np.float32)
    onehot = torch.from_numpy(np.eye(G_C, dtype=np.int32)[np.random.default_rng(9).integers(0, G_C, G_CLIPS)]).to(DEV)
    res = []
    for steps, kw in ((T, dict(seq_len={"net": [L] * G_CLIPS})), (L, {})):
        eng, p = graph_engine(steps, fusion="attn")
        fd = {"main": torch.from_numpy(np.ascontiguousarray(x[:, :steps]).reshape(-1, G_DIM)).to(DEV)}
        logits = eng.forward(fd, **kw).cpu().numpy()
        out = eng.train_step(fd, onehot, lr=0.01, clip_norm=0.5, **kw)
        res.append((logits, out, eng.get_params()))
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=1e-5, atol=1e-6)
    assert res[0][1]["rows"] == res[1][1]["rows"] == G_CLIPS
    assert abs(res[0][1]["loss"] - res[1][1]["loss"]) < 1e-5 * max(1, abs(res[1][1]["loss"]))
    for k in res[0][2]:
        np.testing.assert_allclose(res[0][2][k], res[1][2][k], rtol=1e-4, atol=1e-6, err_msg="param " + k)


# ---- 8. two ranks ------------------------------------------------------------------------------------------------------------------------
def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def dp_worker(rank, world, port, q):
    """tests/test_dp_gpu.worker with fusion attn: both ranks on cuda:0 over gloo, each on its half of the clips."""
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from vltf_amd import dp
    from vltf_amd.engine import LRCNEngine, NetConfig
    r, w, _ = dp.init_from_env(backend="gloo")
    assert (r, w) == (rank, world)
    shape, ncls, fpc, clips, hid = (67, 67, 3), 5, 2, 4, 6
    cfg = NetConfig(image_shape=shape, num_classes=ncls, fpc=fpc, lstm_hidden=hid, fusion="attn", attn_dim=4)
    rng = np.random.default_rng(11)                                  # identical on every rank
    p = R.init_params(rng, ncls, "fc6", hid, 1, shape, "lstm", 4)
    frames = rng.integers(0, 256, (clips * fpc,) + shape, dtype=np.uint8)
    onehot = np.eye(ncls, dtype=np.int32)[rng.integers(0, ncls, clips)]
    lo, hi = dp.shard_range(clips, rank, world)
    gar = dp.GradAllReduce()
    eng = LRCNEngine(cfg, max_clips=hi - lo, device="cuda:0", dp=gar)
    eng.load_params(p)
    gar.broadcast_params(eng.w)
    attn = [eng.offsets[n] for n in R.param_names()]
    covered = all(any(o <= a and a + n <= o + c for o, c in eng.grad_chunks) for a, n in attn)
    out = eng.train_step_u8(torch.tensor(frames[lo * fpc:hi * fpc], device="cuda:0"), torch.tensor(onehot[lo:hi], device="cuda:0"),
                            lr=0.05, clip_norm=0.5, mean_bgr=MEAN)
    got = eng.get_params()
    if rank == 0:
        ref = LRCNEngine(cfg, max_clips=clips, device="cuda:0")       # one engine, all the clips
        ref.load_params(p)
        want_out = ref.train_step_u8(torch.tensor(frames, device="cuda:0"), torch.tensor(onehot, device="cuda:0"), lr=0.05,
                                     clip_norm=0.5, mean_bgr=MEAN)
        want = ref.get_params()
        err = {k: float(np.abs(got[k] - want[k]).max() / (np.abs(want[k] - p[k]).max() + 1e-12)) for k in want}
        moved = min(float(np.abs(want[n] - p[n]).max()) for n in R.param_names())
        q.put(("ok", max(err.values()), abs(out["grad_norm"] - want_out["grad_norm"]) / want_out["grad_norm"], covered, moved))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_rank_step_equals_one_rank():
    """tests/test_dp_gpu.test_two_rank_step_equals_one_rank with the attention variables in the exchange, at its tolerance."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    for pr in procs:
        pr.join(300)
        assert pr.exitcode == 0, "rank exited with %s" % pr.exitcode
    tag, worst, gn_err, covered, moved = q.get(timeout=10)
    assert tag == "ok" and covered and moved > 0
    assert worst < 1e-3 and gn_err < 1e-5, (worst, gn_err)


# ---- 9. run_task.py on examples/lrcn_attn.yml --------------------------------------------------------------------------------------------
def test_run_task_on_the_example_trains_validates_and_resumes(tmp_path, monkeypatch):
    """examples/lrcn_attn.yml pointed at the synthetic dataset (its shapes, four classes, one 8-unit layer, attn_dim 5, batches of 2): two
    train steps with a checkpoint, a validation of it, and a second training run that resumes from it; the checkpoint holds the
    attention variables."""
    import glob
    import yaml
    from tests.test_host_workflow import make_dataset
    from tests.test_run_task_gpu import RAW, WANT
    from vltf_amd import run_task
    monkeypatch.setenv("VLTF_PREFETCH", "0")
    monkeypatch.setenv("VLTF_CONV_MATH", "f32")
    folder = str(tmp_path)
    train_path, _, _ = make_dataset(folder, "train.txt", nvid=4, cpv=(1, 1, 1, 1), shape=RAW, seed=1)
    val_path, _, _ = make_dataset(folder, "val.txt", nvid=3, cpv=(2, 1, 2), shape=RAW, seed=2)
    run = os.path.join(folder, "run")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def cfg(name, data_path, phase, resume=None, epochs=1):
        with open(os.path.join(root, "examples", "lrcn_attn.yml")) as f:
            c = yaml.safe_load(f)
        r = c["run"]
        r.update(resume_file=resume, run_folder=run, phase="defs.phase.%s" % phase)
        d = r["data"].pop("train_set")
        d.update(data_path=data_path, phase="defs.phase.%s" % phase, raw_image_shape=str(RAW), image_shape=str(WANT))
        if phase != "train":
            d["imgproc"] = ["defs.imgproc.center_crop", "defs.imgproc.sub_mean"]
        r["data"]["d"] = d
        r["network"]["num_classes"] = 4
        pipe = r["network"]["pipelines"][0]["lrcn"]
        assert pipe["lstm_params"][2] == "defs.fusion_method.attn" and pipe["attn_dim"] == 128
        pipe["lstm_params"] = [8, 1, "defs.fusion_method.attn"]
        pipe["attn_dim"] = 5
        r["train"].update(batch_size=2, epochs=epochs, base_lr=1e-4, lr_decay=["defs.decay.exp", "defs.periodicity.interval", 2, 0.9], clip_norm=5)
        r["val"]["batch_size"] = 2
        path = os.path.join(folder, name)
        with open(path, "w") as f:
            yaml.safe_dump(c, f)
        return path

    run_task.main(cfg("train.yml", train_path, "train"), seed=3)                           # 4 videos, batch 2: two steps
    ck = glob.glob(os.path.join(run, "checkpoints", "*.weights.npz"))
    assert len(ck) == 1
    saved = np.load(ck[0])
    names = R.param_names()
    assert all(n in saved.files for n in names) and saved["output_fc_w"].shape == (8, 4)
    assert [saved[n].shape for n in names] == [(8, 5), (5,), (5, 1)]
    log = open(glob.glob(os.path.join(run, "log_lrcn_attn_train_scratch_*.log"))[0]).read()
    assert "global step: 2" in log
    acc = run_task.main(cfg("val.yml", val_path, "val", resume="latest"))
    assert 0.0 <= acc <= 1.0 and float(open(os.path.join(run, "accuracy_lrcn_attn_val_resume")).read()) == acc
    run_task.main(cfg("resume.yml", train_path, "train", resume=ck[0][:-len(".weights.npz")], epochs=2), seed=5)
    log2 = open(glob.glob(os.path.join(run, "log_lrcn_attn_train_resume_*.log"))[0]).read()
    assert "Restored training snapshot of epoch 1" in log2 and "global step: 4" in log2
    after = np.load(max(glob.glob(os.path.join(run, "checkpoints", "*.weights.npz")), key=os.path.getmtime))
    assert any(not np.array_equal(after[n], saved[n]) for n in (names[0], names[2]))
