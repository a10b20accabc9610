"""The NetVLAD launches (csrc/netvlad.hip: netvlad_fwd_kernel / netvlad_bwd_kernel) against the fp64 reference of tests/netvlad_ref.py,
then the engines that run on them.

Cases (netvlad_ref.CASES as (batch, T, HO, K)): the smallest launch; odd widths below a wave and below a cluster slab; a ragged last
wave of HO with more steps than waves and a ragged slab; the flagship width at the default K and at the largest; HO of four passes of
the workgroup; K one past a half-wave over 64 steps (eight step slabs); the largest K at a narrow HO.  Every case runs at both score
scales, without and with per-clip lengths (lstm_plan.lengths: a 0, a T, a -3 and a T + 5, clamped to 1..T by the fusion's rule), and
with lengths the dead rows of h and s (and of the a the backward is handed) hold NaN.

Tolerances are the project's classes (tests/test_lstm_geometry_gpu.TOL) as tests/test_netvlad.py assigns them: every output hseq
(1e-5, 1e-6); the absolute term of ds is taken at no less than the magnitude of the terms that cancel inside it
(netvlad_ref.cancel_scale).  The backward runs FROM the reference's own a, r and y rounded to fp32.  Every output is a Guarded view
(sentinels around it, NaN inside beforehand)."""
import os

import numpy as np
import pytest
import torch

from tests import lstm_plan as P
from tests import netvlad_ref as R
from tests.test_lstm_geometry_gpu import DEV, TOL, Guarded, put, same_bits, within

pytestmark = pytest.mark.gpu

CLASS = dict(a="hseq", r="hseq", y="hseq", ds="hseq", dh="hseq", dcp="hseq")       # tests/test_netvlad.py decides these
OUT = ("a", "r", "y", "ds", "dh", "dcp")


@pytest.fixture(scope="module")
def ops():
    import vltf_amd.ops as ops_
    return ops_


def shapes(case):
    batch, T, HO, K = case
    return dict(a=(batch * T, K), r=(batch, K), y=(batch, K * HO), ds=(batch * T, K), dh=(batch * T, HO), dcp=(batch, K * HO))


def run_pool(ops, case, inp, lens, a32, r32, y32, alias=False, what=""):
    """netvlad_fwd on the inputs (NaN in the dead rows of h and s), netvlad_bwd on the a, r and y given (NaN in the dead rows of a);
    the memory checks; -> {output: array}.  alias: a is written over s."""
    batch, T, HO, K = case
    nan = (lambda a: a) if lens is None else (lambda a: R.with_nan_in_dead_rows(a, T, lens))
    h, c, dy = put(nan(inp.h), DEV), put(inp.c, DEV), put(inp.dy, DEV)
    L = put(lens, DEV, torch.int32)
    o = {k: Guarded(shp, DEV) for k, shp in shapes(case).items()}
    if alias:
        o["a"].t.copy_(put(nan(inp.s), DEV))
        s = o["a"].t
    else:
        s = put(nan(inp.s), DEV)
    ops.netvlad_fwd(s, c, h, o["a"].t, o["r"].t, o["y"].t, batch, T, HO, K, seq_len=L)
    ops.netvlad_bwd(dy, h, put(nan(a32), DEV), put(r32, DEV), put(y32, DEV), c, o["ds"].t, o["dh"].t, o["dcp"].t, batch, T, HO, K, seq_len=L)
    return {k: g.settle(what + " " + k) for k, g in o.items()}


def run_ref(ops, case, ref, **kw):
    return run_pool(ops, case, ref.inp, ref.lens, ref.a32, ref.r32, ref.y32, **kw)


def within_scaled(name, got, want, scale, what):
    """tests.test_lstm_geometry_gpu.within with the absolute term taken at `scale` (>= max|want|)."""
    rtol, atol_rel = TOL[name]
    want = np.asarray(want, np.float64)
    assert scale >= np.abs(want).max()
    err = np.abs(np.asarray(got, np.float64) - want)
    ratio = float((err / (atol_rel * scale + rtol * np.abs(want))).max())
    print("%s: worst error / bound %.3g" % (what, ratio))
    assert ratio <= 1.0, "%s: %s (worst error / bound %.3g)" % (what, name, ratio)


# ---- 1. the kernels against the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
@pytest.mark.parametrize("k", R.SCALES, ids=lambda k: "k%d" % k)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_netvlad_against_the_reference(ops, case, k, lens):
    batch, T, HO, K = case
    what = "netvlad %s k%d %s" % (R.case_id(case), k, "lens" if lens else "full")
    ref = R.reference(case, k, lens)
    got = run_ref(ops, case, ref, what=what)
    want = dict(ref.fwd._asdict(), **ref.bwd._asdict())
    for name in OUT:
        if name == "ds":
            within_scaled(CLASS[name], got[name], want[name], R.abs_scale(ref, name), what + " ds")
        else:
            within(CLASS[name], got[name], want[name], what + " " + name)
    if lens:
        dead = ~R.live_mask(ref.lens, batch, T).reshape(-1)
        assert batch == 1 or (dead.any() and not dead.all())
        for name in ("a", "ds", "dh"):
            assert not got[name][dead].any(), "%s: dead row of %s not zero" % (what, name)
    # a written over s: the same bits
    same_bits(run_ref(ops, case, ref, alias=True, what=what + " aliased"), got, what + ": a aliasing s")


# ---- 2. bit for bit ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
def test_repeatable_and_a_clip_alone_equals_the_clip_in_a_batch(ops, lens):
    case = batch, T, HO, K = (5, 16, 256, 8)
    ref = R.reference(case, 1, lens)
    whole = run_ref(ops, case, ref, what="netvlad")
    same_bits(run_ref(ops, case, ref, what="netvlad again"), whole, "netvlad: a second run")
    inp = ref.inp
    for b in range(batch):
        rows, row = slice(b * T, (b + 1) * T), slice(b, b + 1)
        one = R.Inputs(inp.h[rows], inp.s[rows], inp.c, inp.dy[row])
        alone = run_pool(ops, (1, T, HO, K), one, None if ref.lens is None else ref.lens[row], ref.a32[rows], ref.r32[row], ref.y32[row],
                         what="netvlad clip %d alone" % b)
        part = {k: v[row] if v.shape[0] == batch else v[rows] for k, v in whole.items()}
        same_bits(alone, part, "netvlad: clip %d alone against the batch of %d" % (b, batch))


# ---- 3. degenerate cases -----------------------------------------------------------------------------------------------------------------
def test_one_live_step_gives_unit_residuals_and_no_score_gradient(ops):
    """T = 1 at score scale 3: y_k is the unit vector of h - c_k over sqrt(K) whatever the scores; ds is zero in exact arithmetic and is
    held to hseq's absolute term at the magnitude of the cancelling terms a |dV_k| |h - c_k|."""
    case = batch, T, HO, K = (3, 1, 37, 3)
    ref = R.reference(case, 3, False)
    got = run_ref(ops, case, ref, what="netvlad T = 1")
    d = np.asarray(ref.inp.h, np.float64)[:, None, :] - np.asarray(ref.inp.c, np.float64)[None]
    unit = (d / np.linalg.norm(d, axis=2, keepdims=True) / np.sqrt(K)).reshape(batch, K * HO)
    within("hseq", got["y"], unit, "netvlad T = 1 y")
    assert np.abs(ref.bwd.ds).max() < 1e-6 * ref.ds_scale and ref.ds_scale > 0.1      # the reference's ds is rounding of the handed a, r, y
    within_scaled("hseq", got["ds"], ref.bwd.ds, ref.ds_scale, "netvlad T = 1 ds")
    assert np.abs(got["ds"]).max() <= 2 * TOL["hseq"][1] * ref.ds_scale


def test_scores_of_two_hundred_stay_finite(ops):
    """The epsilon branch in fp32: a starved cluster's a is zero, its r exactly 1e6 and its y zero; the fed clusters are held to the
    reference."""
    from tests.test_netvlad import saturated_inputs
    case, inp, s = saturated_inputs()
    batch, T, HO, K = case
    s = s.astype(np.float32)
    fwd = R.forward(inp.h, s, inp.c, None, T)
    got = run_pool(ops, case, R.Inputs(inp.h, s, inp.c, inp.dy), None, P.rounded(fwd.a), P.rounded(fwd.r), P.rounded(fwd.y), what="netvlad +-200")
    bwd = R.backward(inp.dy, inp.h, P.rounded(fwd.a), P.rounded(fwd.r), P.rounded(fwd.y), inp.c, None, T)
    assert (got["r"][:, 2:] == np.float32(1e6)).all() and not got["y"].reshape(batch, K, HO)[:, 2:].any()
    assert set(np.unique(got["a"])) == {0.0, 1.0}
    for name in ("a", "r", "y", "dh", "dcp"):
        within("hseq", got[name], dict(fwd._asdict(), **bwd._asdict())[name], "netvlad +-200 " + name)
    assert not got["ds"].any()                                       # a is 0 or 1 exactly: a (da - a . da) = 0


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ops):
    """Every limit missed and a null pointer raise by name; nothing is launched."""
    case = (1, 4, 2, 3)
    o = {k: Guarded(shp, DEV) for k, shp in shapes(case).items()}
    rg = np.random.default_rng(0)
    f = lambda *shape: put(rg.standard_normal(shape).astype(np.float32), DEV)
    s, c, h, dy, a, r, y = f(4, 3), f(3, 2), f(4, 2), f(1, 6), f(4, 3), f(1, 3), f(1, 6)
    # (sizes outside the limits are left to the launch, which refuses them before it reads anything)
    fwd = lambda T_=4, HO=2, K=3, c_=c, s_=s: ops.netvlad_fwd(s_, c_, h, o["a"].t, o["r"].t, o["y"].t, 1, T_, HO, K)
    bwd = lambda T_=4, HO=2, K=3, c_=c, dy_=dy: ops.netvlad_bwd(dy_, h, a, r, y, c_, o["ds"].t, o["dh"].t, o["dcp"].t, 1, T_, HO, K)
    for call in (fwd, bwd):
        for kw, match in ((dict(K=1), "K 1 is outside 2..64"), (dict(K=65), "K 65 is outside 2..64"), (dict(HO=0), "HO 0 is outside 1..1024"),
                          (dict(HO=1025, K=2), "HO 1025 is outside 1..1024"), (dict(HO=257, K=64), "K \\* HO = 16448 exceeds 16384"),
                          (dict(T_=0), "T 0 is outside 1..1024"), (dict(T_=1025), "T 1025 is outside 1..1024"), (dict(c_=None), "null pointer")):
            with pytest.raises(Exception, match=match):
                call(**kw)
    with pytest.raises(Exception, match="null pointer"):
        fwd(s_=None)
    with pytest.raises(Exception, match="null pointer"):
        bwd(dy_=None)
    with pytest.raises(Exception, match="elements"):                # a tensor smaller than the launch would read
        ops.netvlad_fwd(s, c, h, o["a"].t, o["r"].t, o["y"].t, 2, 4, 2, 3)
    torch.cuda.synchronize()
    assert all(g.untouched() for g in o.values()), "netvlad: refused, yet an output was written"
    fwd()                                                           # (the arguments are good otherwise)
    torch.cuda.synchronize()
    assert all(o[k].untouched() for k in ("ds", "dh", "dcp")) and not o["y"].untouched()


# ---- 5. LRCNEngine -----------------------------------------------------------------------------------------------------------------------
MEAN = np.array([99.197148, 105.293620, 109.503945], np.float32)
SHAPE, NCLS, FPC, CLIPS = (67, 67, 3), 7, 3, 2                               # the smoke() geometry of tests/test_gru_gpu.py
CELL_KW = dict(lstm=dict(), gru=dict(rnn_cell="gru"), blstm=dict(lstm_bidirectional=True),
               encoder=dict(rnn_cell="mhsa", sa_heads=2, sa_positions="relative", sa_block="encoder", sa_ffn_dim=32))


@pytest.mark.parametrize("cell,layers,H,K", [("lstm", 1, 8, 3), ("gru", 2, 8, 3), ("blstm", 1, 8, 3), ("encoder", 1, 16, 4)])
def test_lrcn_engine_train_step_against_the_reference(cell, layers, H, K):
    """Logits, loss, gradient norm, every gradient and the clipped SGD step against netvlad_ref.model_train_step at the bounds of
    tests/test_attn_pool_gpu.test_lrcn_engine_train_step_against_the_reference (seed 6 as there; the encoder case takes seed 7 and
    mhsa_ref.varied_frames for the reason tests/test_encoder_block_gpu.py gives); a gradient reaches all three NetVLAD variables;
    vlad_assignments() is the reference's a."""
    from tests import mhsa_ref
    from vltf_amd.engine import LRCNEngine, NetConfig, param_specs
    enc = cell == "encoder"
    rng = np.random.default_rng(7 if enc else 6)
    cfg = NetConfig(image_shape=SHAPE, num_classes=NCLS, fpc=FPC, frame_encoding_layer="fc6", lstm_hidden=H, lstm_layers=layers, fusion="vlad",
                    vlad_clusters=K, **CELL_KW[cell])
    eng = LRCNEngine(cfg, max_clips=CLIPS, device=DEV)
    p = R.init_params(rng, NCLS, "fc6", H, layers, SHAPE, cell, K, heads=2, T=FPC, F=32)
    assert {n: tuple(s) for n, s in param_specs(cfg)} == {n: v.shape for n, v in p.items()}
    HO = R.out_width(cell, H)
    assert p["output_fc_w"].shape == (K * HO, NCLS)
    eng.load_params(p)
    frames = mhsa_ref.varied_frames(rng, CLIPS, FPC, SHAPE) if enc else rng.integers(0, 256, (CLIPS * FPC,) + SHAPE, dtype=np.uint8)
    onehot = np.eye(NCLS, dtype=np.int32)[rng.integers(0, NCLS, CLIPS)]
    x = frames.astype(np.float32) - MEAN
    newp, loss, gn, logits, grads, a = R.model_train_step(p, x, onehot, FPC, 0.01, 0.5, "fc6", H, layers, cell, heads=2)
    fd = torch.tensor(frames, device=DEV)
    got_fwd = eng.forward_u8(fd, MEAN).cpu().numpy()
    assert got_fwd.shape == logits.shape
    np.testing.assert_allclose(got_fwd, logits, rtol=1e-3, atol=1e-3)
    got_a = eng.vlad_assignments().cpu().numpy()
    assert got_a.shape == (CLIPS, FPC, K) and a.shape == (CLIPS * FPC, K)
    np.testing.assert_allclose(got_a.reshape(-1, K), a, rtol=1e-3, atol=1e-3)    # weights in [0, 1] behind the same tower as the logits
    np.testing.assert_allclose(got_a.astype(np.float64).sum(axis=2), 1.0, rtol=0, atol=1e-6)
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
def test_the_netvlad_products_are_fp32_under_every_conv_math(math):
    """8 clips x 16 frames, H = 128, K = 64: the three NetVLAD products have 128 rows and depth 128 or 64, sizes from which ops.gemm
    WITH a workspace follows conv_math into split-bf16 arithmetic.  They are called without one, as the head's are: each is compared
    with the fp64 product of the operands THE DEVICE holds, at class act (3e-5, 3e-5) -- an fp32 product of depth 128 is two orders of
    magnitude inside it, a single-plane bf16 product (2^-9 per factor) two orders outside.  The pooling between them is held to the
    reference from the same operands."""
    from vltf_amd.engine import LRCNEngine, NetConfig, init_params
    clips, fpc, H, K = 8, 16, 128, 64
    n = clips * fpc
    cfg = NetConfig(image_shape=SHAPE, num_classes=NCLS, fpc=fpc, frame_encoding_layer="fc6", lstm_hidden=H, fusion="vlad", vlad_clusters=K,
                    conv_math=math)
    p = init_params(cfg, seed=3, well_scaled=True)
    kn, bn, cn = R.param_names()
    p[bn] = (0.1 * np.random.default_rng(5).standard_normal(K)).astype(np.float32)
    eng = LRCNEngine(cfg, max_clips=clips, device=DEV)
    eng.load_params(p)
    rng = np.random.default_rng(12)
    frames = torch.from_numpy(rng.integers(0, 256, (n,) + SHAPE, dtype=np.uint8)).to(DEV)
    onehot = torch.from_numpy(np.eye(NCLS, dtype=np.int32)[rng.integers(0, NCLS, clips)]).to(DEV)
    out = eng.train_step_u8(frames, onehot, lr=0.01, clip_norm=0.0, mean_bgr=MEAN)
    assert np.isfinite(out["loss"]) and out["rows"] == clips
    host = lambda t: t.detach().cpu().numpy().astype(np.float64)
    hseq, a, ds, dproj, dcp = (host(t) for t in (eng.lstm[-1]["hseq"][:n], eng.vlad["sa"][:n], eng.vlad["ds"][:n], eng.vlad["dproj"][:n],
                                                 eng.vlad["dcp"][:clips]))
    W, b, c = (p[k].astype(np.float64) for k in (kn, bn, cn))
    assert np.abs(hseq).max() > 1e-2 and np.abs(ds).max() > 0
    fwd = R.forward(hseq, hseq @ W + b, c, None, fpc, check_band=False)
    what = "NetVLAD products under conv_math %s: " % math
    within("act", a, fwd.a, what + "a = softmax(hseq W + beta)")
    within("act", host(eng.fused[:clips]), fwd.y, what + "y")
    within("act", host(eng.G[kn]), hseq.T @ ds, what + "G[kernel] = hseq^T ds")
    within("act", host(eng.G[bn]), ds.sum(axis=0), what + "G[bias]")
    within("act", host(eng.G[cn]), dcp.sum(axis=0).reshape(K, H), what + "G[centers]")
    within("act", dproj, ds @ W.T, what + "dproj = ds W^T")


# ---- 6. the captured step ----------------------------------------------------------------------------------------------------------------
def test_lrcn_engine_captured_step_is_the_eager_step():
    """step_graph with dropout: the warm-up step, the captured one and three replays equal the eager engine's bit for bit -- the two
    NetVLAD launches take no host-varying argument and replay as they are."""
    from vltf_amd.engine import LRCNEngine, NetConfig, init_params
    engines = []
    kw = dict(image_shape=SHAPE, num_classes=NCLS, fpc=FPC, frame_encoding_layer="fc6", lstm_hidden=16, lstm_layers=2, fusion="vlad",
              vlad_clusters=5, dropout_keep_prob=0.5)
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
        assert torch.equal(engines[0].vlad_assignments(), engines[1].vlad_assignments()), step
    assert len(engines[1]._graphs) == 1
    pa, pb = engines[0].get_params(), engines[1].get_params()
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), k
    assert not np.array_equal(pa["netvlad/centers"], params["netvlad/centers"])


# ---- 7. GraphEngine: the vector-input pipeline of tests/test_gru_gpu.py with lengths ------------------------------------------------------
def test_graph_engine_with_lengths_against_the_reference():
    from tests import gru_ref
    from tests.test_gru_gpu import G_C, G_CLIPS, G_DIM, G_H, graph_engine
    T, lens = 5, np.array([5, 2, 1, 4])
    eng, p = graph_engine(T, fusion="vlad")
    kn, bn, cn = R.param_names()
    assert p[kn].shape == (G_H, 8) and p[cn].shape == (8, G_H) and p["output_fc_w"].shape == (8 * G_H, G_C)   # vlad_clusters defaults to 8
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
        eng, _ = graph_engine(T, fusion="vlad")
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
        eng, p = graph_engine(steps, fusion="vlad")
        fd = {"main": torch.from_numpy(np.ascontiguousarray(x[:, :steps]).reshape(-1, G_DIM)).to(DEV)}
        logits = eng.forward(fd, **kw).cpu().numpy()
        out = eng.train_step(fd, onehot, lr=0.01, clip_norm=0.5, **kw)
        res.append((logits, out, eng.get_params()))
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=1e-5, atol=1e-6)
    assert res[0][1]["rows"] == res[1][1]["rows"] == G_CLIPS
    assert abs(res[0][1]["loss"] - res[1][1]["loss"]) < 1e-5 * max(1, abs(res[1][1]["loss"]))
    for k in res[0][2]:
        np.testing.assert_allclose(res[0][2][k], res[1][2][k], rtol=1e-4, atol=1e-6, err_msg="param " + k)


# ---- 8. run_task.py on examples/lrcn_netvlad.yml -----------------------------------------------------------------------------------------
def test_run_task_on_the_example_trains_validates_and_resumes(tmp_path, monkeypatch):
    """examples/lrcn_netvlad.yml pointed at the synthetic dataset (its shapes, four classes, one 8-unit layer, 3 centres, batches of 2):
    two train steps with a checkpoint, a validation of it, and a second training run that resumes from it; the checkpoint holds the
    NetVLAD variables and the (K HO, classes) head."""
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
        with open(os.path.join(root, "examples", "lrcn_netvlad.yml")) as f:
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
        assert pipe["lstm_params"][2] == "defs.fusion_method.vlad" and pipe["vlad_clusters"] == 8
        pipe["lstm_params"] = [8, 1, "defs.fusion_method.vlad"]
        pipe["vlad_clusters"] = 3
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
    assert all(n in saved.files for n in names) and saved["output_fc_w"].shape == (24, 4)
    assert [saved[n].shape for n in names] == [(8, 3), (3,), (3, 8)]
    log = open(glob.glob(os.path.join(run, "log_lrcn_netvlad_train_scratch_*.log"))[0]).read()
    assert "global step: 2" in log
    acc = run_task.main(cfg("val.yml", val_path, "val", resume="latest"))
    assert 0.0 <= acc <= 1.0 and float(open(os.path.join(run, "accuracy_lrcn_netvlad_val_resume")).read()) == acc
    run_task.main(cfg("resume.yml", train_path, "train", resume=ck[0][:-len(".weights.npz")], epochs=2), seed=5)
    log2 = open(glob.glob(os.path.join(run, "log_lrcn_netvlad_train_resume_*.log"))[0]).read()
    assert "Restored training snapshot of epoch 1" in log2 and "global step: 4" in log2
    after = np.load(max(glob.glob(os.path.join(run, "checkpoints", "*.weights.npz")), key=os.path.getmtime))
    assert any(not np.array_equal(after[n], saved[n]) for n in (names[0], names[2]))
