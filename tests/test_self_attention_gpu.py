"""The self-attention launches (csrc/self_attention.hip: mhsa_fwd_kernel / mhsa_bwd_kernel) against the fp64 reference of
tests/mhsa_ref.py, then the engines that run on them.

Cases (mhsa_ref.CASES as (batch, T, H, heads)): one step; dh = 8; dh = 50 with an odd T; the workload's shape; eight heads; dh = 96 in
one head; T = 64; T and dh both at their limits (the largest LDS request); dh = 65.  Every case runs at both input scales, without and
with per-clip lengths (lstm_plan.lengths: a 0, a T, a -3 and a T + 5, clamped to 0..T), with and without the position bias, and with
lengths the dead rows of qkv and dctx hold NaN.

Tolerances: P, ctx, dqkv and dposp take class act (3e-5, 3e-5) of tests/test_lstm_geometry_gpu.TOL, as tests/test_self_attention.py
decides.  The backward runs FROM the reference's own P rounded to fp32.  Every output is a Guarded view (sentinels around it, NaN inside
beforehand).

The issue names the engine cases (H, heads, layers, fusion) = (8, 2, 1, avg) and (8, 2, 1, attn); their head width 8 / 2 = 4 is below
the limit 8 <= dh that the same issue sets and has refused.  The limit stands (test_the_engine_cases_below_the_head_width_are_refused);
the two cases run at H = 16 with their heads, depth and fusion."""
import os
import socket

import numpy as np
import pytest
import torch

from tests import lstm_plan as LP
from tests import mhsa_ref as R
from tests.test_lstm_geometry_gpu import DEV, Guarded, put, same_bits, within

pytestmark = pytest.mark.gpu

OUT = ("P", "ctx", "dqkv", "dposp")


@pytest.fixture(scope="module")
def ops():
    import vltf_amd.ops as ops_
    return ops_


def shapes(case, positions=True):
    batch, T, H, heads = case
    s = dict(P=(batch, heads, T, T), ctx=(batch * T, H), dqkv=(batch * T, 3 * H))
    if positions:
        s["dposp"] = (batch, heads, 2 * T - 1)
    return s


def run_mhsa(ops, case, inp, lens, P32, positions=True, what=""):
    """mhsa_fwd on the inputs (NaN in the dead rows of qkv), mhsa_bwd on the P given (NaN in the dead rows of dctx and qkv); the memory
    checks; -> {output: array}."""
    batch, T, H, heads = case
    nan = (lambda a: a) if lens is None else (lambda a: R.with_nan_in_dead_rows(a, T, lens))
    qkv, dctx = put(nan(inp.qkv), DEV), put(nan(inp.dctx), DEV)
    pos = put(inp.pos, DEV) if positions else None
    L = put(lens, DEV, torch.int32)
    o = {k: Guarded(shp, DEV) for k, shp in shapes(case, positions).items()}
    ops.mhsa_fwd(qkv, pos, o["P"].t, o["ctx"].t, batch, T, H, heads, seq_len=L)
    ops.mhsa_bwd(dctx, qkv, put(P32, DEV), o["dqkv"].t, o["dposp"].t if positions else None, batch, T, H, heads, seq_len=L)
    return {k: g.settle(what + " " + k) for k, g in o.items()}


def run_ref(ops, case, ref, positions=True, **kw):
    return run_mhsa(ops, case, ref.inp, ref.lens, ref.P32, positions, **kw)


# ---- 1. the kernels against the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
@pytest.mark.parametrize("k", R.SCALES, ids=lambda k: "k%d" % k)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_mhsa_against_the_reference(ops, case, k, lens):
    batch, T, H, heads = case
    for positions in (True, False):
        what = "mhsa %s k%d %s %s" % (R.case_id(case), k, "lens" if lens else "full", "pos" if positions else "no pos")
        ref = R.reference(case, k, lens, positions)
        got = run_ref(ops, case, ref, positions, what=what)
        want = dict(ref.fwd._asdict(), **ref.bwd._asdict())
        for name in got:
            within("act", got[name], want[name], what + " " + name)
        if lens:
            dead = ~R.live_mask(ref.lens, batch, T).reshape(-1)
            assert batch == 1 or (dead.any() and not dead.all())             # (one clip: lstm_plan.lengths makes it T + 5, all live)
            for name in ("ctx", "dqkv"):
                assert not got[name][dead].any(), "%s: dead row of %s not zero" % (what, name)
            rows = got["P"].transpose(0, 2, 1, 3).reshape(batch * T, heads * T)
            cols = got["P"].transpose(0, 3, 1, 2).reshape(batch * T, heads * T)
            assert not rows[dead].any() and not cols[dead].any(), what + ": dead row or column of P not zero"
        live = R.live_mask(ref.lens, batch, T)
        sums = got["P"].astype(np.float64).sum(axis=3)
        np.testing.assert_allclose(sums, np.broadcast_to(live[:, None, :], sums.shape).astype(np.float64), rtol=0, atol=2e-6)


# ---- 2. bit for bit ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
def test_repeatable_and_a_clip_alone_equals_the_clip_in_a_batch(ops, lens):
    case = batch, T, H, heads = (5, 16, 256, 4)
    ref = R.reference(case, 1, lens)
    whole = run_ref(ops, case, ref, what="mhsa")
    same_bits(run_ref(ops, case, ref, what="mhsa again"), whole, "mhsa: a second run")
    inp = ref.inp
    for b in range(batch):
        rows, row = slice(b * T, (b + 1) * T), slice(b, b + 1)
        one = R.Inputs(inp.qkv[rows], inp.pos, inp.dctx[rows])
        alone = run_mhsa(ops, (1, T, H, heads), one, None if ref.lens is None else ref.lens[row], ref.P32[row], what="mhsa clip %d alone" % b)
        part = {k: v[row] if v.shape[0] == batch else v[rows] for k, v in whole.items()}
        same_bits(alone, part, "mhsa: clip %d alone against the batch of %d" % (b, batch))


# ---- 3. degenerate cases -----------------------------------------------------------------------------------------------------------------
def test_one_step_gives_weight_one_ctx_equal_to_v_and_no_score_gradient(ops):
    case = batch, T, H, heads = (3, 1, 24, 3)
    ref = R.reference(case, 3, False)
    got = run_ref(ops, case, ref, what="mhsa T = 1")
    assert (got["P"] == 1.0).all() and not got["dqkv"][:, :2 * H].any() and not got["dposp"].any()
    same_bits(dict(ctx=got["ctx"], dv=np.ascontiguousarray(got["dqkv"][:, 2 * H:])),
              dict(ctx=np.ascontiguousarray(ref.inp.qkv[:, 2 * H:]), dv=np.asarray(ref.inp.dctx)), "mhsa T = 1")


@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
def test_zero_queries_and_zero_bias_give_the_mean_of_v_over_the_live_steps(ops, lens):
    case = batch, T, H, heads = (4, 7, 96, 1)
    ref = R.reference(case, 1, lens)
    qkv = np.array(ref.inp.qkv)
    qkv[:, :H] = 0.0
    inp = R.Inputs(qkv, np.zeros_like(ref.inp.pos), ref.inp.dctx)
    got = run_mhsa(ops, case, inp, ref.lens, ref.P32, what="mhsa Q = 0")
    live = R.live_mask(ref.lens, batch, T)
    n = np.maximum(live.sum(axis=1), 1)
    v = np.where(live[:, :, None], np.asarray(qkv[:, 2 * H:], np.float64).reshape(batch, T, H), 0.0)
    mean = v.sum(axis=1) / n[:, None]
    want = np.where(live[:, :, None], mean[:, None, :], 0.0).reshape(batch * T, H)
    within("act", got["ctx"], want, "mhsa Q = 0 ctx")
    within("act", got["P"][:, 0], (live[:, :, None] & live[:, None, :]) / n[:, None, None], "mhsa Q = 0 P")


def test_scores_of_two_hundred_stay_finite(ops):
    case = batch, T, H, heads = (2, 21, 250, 5)
    dh = H // heads
    inp = R.inputs(*case)
    c = np.sqrt(200.0 / np.sqrt(dh))                                # Q . K / sqrt(dh) = +-c^2 sqrt(dh) = +-200
    qkv = np.array(inp.qkv)
    qkv[:, :H] = c
    qkv[:, H:2 * H] = np.where(np.arange(batch * T)[:, None] % T % 2 == 0, c, -c)
    pos = np.zeros_like(inp.pos)
    fwd = R.forward(qkv, pos, heads, None, T)
    got = run_mhsa(ops, case, R.Inputs(qkv, pos, inp.dctx), None, LP.rounded(fwd.P), what="mhsa +-200")
    np.testing.assert_allclose(got["P"].astype(np.float64).sum(axis=3), 1.0, rtol=0, atol=1e-6)
    assert (got["P"][:, :, :, 1::2] == 0).all()                     # exp(-400) is below the smallest fp32 subnormal
    within("act", got["ctx"], fwd.ctx, "mhsa +-200 ctx")


def test_a_constant_added_to_the_position_bias_stays_inside_the_tolerance(ops):
    case = batch, T, H, heads = (3, 16, 512, 8)
    ref = R.reference(case, 1, True)
    shifted = ref.inp._replace(pos=(np.asarray(ref.inp.pos) + np.float32(2.5)).astype(np.float32))
    got = run_mhsa(ops, case, shifted, ref.lens, ref.P32, what="mhsa pos + 2.5")
    want = dict(ref.fwd._asdict(), **ref.bwd._asdict())
    for name in OUT:
        within("act", got[name], want[name], "mhsa pos + 2.5 " + name)


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ops):
    """T = 65, dh = 4, dh = 129, heads not dividing H, wrong buffer sizes and a null pointer raise; nothing is launched.  Every buffer is
    large enough for every shape tried, through ops (which refuses first) and straight through the C entry points."""
    from vltf_amd import _ffi
    big = (2, 65, 1032, 8)
    o = {k: Guarded(shp, DEV) for k, shp in shapes(big).items()}
    f = lambda *shape: torch.zeros(shape, device=DEV)
    qkv, dctx, P, pos = f(2 * 65, 3 * 1032), f(2 * 65, 1032), f(2, 8, 65, 65), f(8, 129)
    fwd = lambda T=16, H=256, heads=4, qkv_=qkv, batch=2: ops.mhsa_fwd(qkv_, pos, o["P"].t, o["ctx"].t, batch, T, H, heads)
    bwd = lambda T=16, H=256, heads=4, dctx_=dctx, batch=2: ops.mhsa_bwd(dctx_, qkv, P, o["dqkv"].t, o["dposp"].t, batch, T, H, heads)
    cases = ((dict(T=65), "exceeds 64"), (dict(H=16, heads=4), "must lie in 8..128"), (dict(H=258, heads=2), "must lie in 8..128"),
             (dict(H=250, heads=4), "does not divide"), (dict(H=1032, heads=12), "exceeds 1024"), (dict(T=0), "must be positive"),
             (dict(heads=0), "must be positive"))
    for call in (fwd, bwd):
        for kw, match in cases:
            with pytest.raises(Exception, match=match):
                call(**kw)
    with pytest.raises(Exception, match="elements"):                # tensors smaller than the launch would read or write
        fwd(qkv_=f(2 * 16, 3 * 256 - 1))
    with pytest.raises(Exception, match="elements"):
        bwd(dctx_=f(2 * 16 - 1, 256))
    with pytest.raises(Exception, match="elements"):
        ops.mhsa_fwd(qkv, pos, f(2, 4, 16, 15), o["ctx"].t, 2, 16, 256, 4)
    with pytest.raises(Exception, match="elements"):
        ops.mhsa_bwd(dctx, qkv, P, o["dqkv"].t, f(2, 4, 30), 2, 16, 256, 4)
    with pytest.raises(Exception, match="null pointer"):
        ops.mhsa_fwd(None, pos, o["P"].t, o["ctx"].t, 2, 16, 256, 4)
    with pytest.raises(Exception, match="null pointer"):
        ops.mhsa_bwd(dctx, qkv, None, o["dqkv"].t, o["dposp"].t, 2, 16, 256, 4)
    # the C entry points refuse on their own
    p = lambda t: t.data_ptr()
    for kw, match in cases:
        T, H, heads = kw.get("T", 16), kw.get("H", 256), kw.get("heads", 4)
        with pytest.raises(Exception, match=match):
            _ffi.call("vl_mhsa_fwd", p(qkv), p(pos), None, p(o["P"].t), p(o["ctx"].t), 2, T, H, heads, ops.stream())
        with pytest.raises(Exception, match=match):
            _ffi.call("vl_mhsa_bwd", p(dctx), p(qkv), p(P), None, p(o["dqkv"].t), p(o["dposp"].t), 2, T, H, heads, ops.stream())
    torch.cuda.synchronize()
    assert all(g.untouched() for g in o.values()), "mhsa: refused, yet an output was written"
    fwd()                                                           # (the arguments are good otherwise)
    torch.cuda.synchronize()
    assert all(o[k].untouched() for k in ("dqkv", "dposp")) and not o["ctx"].untouched() and not o["P"].untouched()


def test_live_rows_copies_the_live_rows_and_zeroes_the_dead_ones(ops):
    """vl_live_rows, the input of the first layer under seq_len: NaN in the dead rows of x does not come through; lengths clamp to
    0..T; a buffer smaller than the launch is refused and nothing is written."""
    batch, T, W = 5, 7, 37
    lens = LP.lengths(batch, T)
    x = np.random.default_rng(3).standard_normal((batch * T, W)).astype(np.float32)
    live = R.live_mask(lens, batch, T).reshape(-1)
    y = Guarded((batch * T, W), DEV)
    with pytest.raises(Exception, match="elements"):
        ops.live_rows(put(x, DEV), y.t, batch + 1, T, W, put(np.append(lens, 1).astype(np.int32), DEV, torch.int32))
    torch.cuda.synchronize()
    assert y.untouched()
    ops.live_rows(put(R.with_nan_in_dead_rows(x, T, lens), DEV), y.t, batch, T, W, put(lens, DEV, torch.int32))
    got = y.settle("live_rows")
    assert np.array_equal(got[live], x[live]) and not got[~live].any() and (~live).any()


# ---- 5. LRCNEngine -----------------------------------------------------------------------------------------------------------------------
MEAN = np.array([99.197148, 105.293620, 109.503945], np.float32)
SHAPE, NCLS, FPC, CLIPS, ATTN = (67, 67, 3), 7, 3, 2, 5                      # the smoke() geometry of tests/test_gru_gpu.py


def test_the_engine_cases_below_the_head_width_are_refused():
    """(H, heads) = (8, 2) of the issue's list: dh = 4 misses 8 <= dh, and the engine says so before anything is allocated."""
    from vltf_amd._ffi import VltfError
    from vltf_amd.engine import LRCNEngine, NetConfig
    for fusion in ("avg", "attn"):
        cfg = NetConfig(image_shape=SHAPE, num_classes=NCLS, fpc=FPC, frame_encoding_layer="fc6", lstm_hidden=8, fusion=fusion,
                        rnn_cell="mhsa", sa_heads=2)
        with pytest.raises(VltfError, match="8 <= dh"):
            LRCNEngine(cfg, max_clips=CLIPS, device=DEV)


@pytest.mark.parametrize("H,heads,layers,fusion,positions", [(16, 2, 1, "avg", True), (8, 1, 2, "last", True), (16, 2, 1, "attn", True),
                                                             (128, 4, 1, "avg", True), (8, 1, 1, "avg", False)])
def test_lrcn_engine_train_step_against_the_reference(H, heads, layers, fusion, positions):
    """Logits, loss, gradient norm, every gradient and the clipped SGD step against mhsa_ref.model_train_step at the bounds of
    tests/test_attn_pool_gpu.test_lrcn_engine_train_step_against_the_reference; a gradient reaches every self-attention variable;
    self_attention_weights() is the reference's P of the last layer.  The last case has sa_positions none."""
    from vltf_amd.engine import LRCNEngine, NetConfig, param_specs
    rng = np.random.default_rng(6)
    attn_dim = ATTN if fusion == "attn" else None
    cfg = NetConfig(image_shape=SHAPE, num_classes=NCLS, fpc=FPC, frame_encoding_layer="fc6", lstm_hidden=H, lstm_layers=layers, fusion=fusion,
                    attn_dim=attn_dim, rnn_cell="mhsa", sa_heads=heads, sa_positions="relative" if positions else "none")
    eng = LRCNEngine(cfg, max_clips=CLIPS, device=DEV)
    p = R.init_params(rng, NCLS, "fc6", H, layers, SHAPE, heads, FPC, positions, attn_dim)
    assert {n: tuple(s) for n, s in param_specs(cfg)} == {n: v.shape for n, v in p.items()}
    frames = R.varied_frames(rng, CLIPS, FPC, SHAPE)                          # (frames that differ along a clip: mhsa_ref.varied_frames)
    onehot = np.eye(NCLS, dtype=np.int32)[rng.integers(0, NCLS, CLIPS)]
    x = frames.astype(np.float32) - MEAN
    R.tame_first_layer(p, x, "fc6", positions)                                # scores of order 1: no softmax is one-hot
    eng.load_params(p)
    newp, loss, gn, logits, grads, P = R.model_train_step(p, x, onehot, FPC, 0.01, 0.5, "fc6", H, layers, heads, fusion, positions)
    fd = torch.tensor(frames, device=DEV)
    got_fwd = eng.forward_u8(fd, MEAN).cpu().numpy()
    assert got_fwd.shape == logits.shape
    np.testing.assert_allclose(got_fwd, logits, rtol=1e-3, atol=1e-3)
    got_P = eng.self_attention_weights().cpu().numpy()
    assert got_P.shape == (CLIPS, heads, FPC, FPC) == P.shape
    np.testing.assert_allclose(got_P, P, rtol=1e-3, atol=1e-3)               # weights in [0, 1] behind the same tower as the logits
    np.testing.assert_allclose(got_P.astype(np.float64).sum(axis=3), 1.0, rtol=0, atol=1e-6)
    assert P.max() < 0.999                                                   # (the reference's weights are not one-hot)
    out = eng.train_step_u8(fd, torch.tensor(onehot, device=DEV), lr=0.01, clip_norm=0.5, mean_bgr=MEAN)
    assert abs(out["loss"] - loss) < 1e-4 * max(1, abs(loss))
    assert abs(out["grad_norm"] - gn) < 1e-3 * gn
    g = eng.get_grads()
    names = [n for l in range(layers) for n in R.param_names(l, positions=positions)]
    assert set(g) == set(p) and set(names) <= set(g)
    for k in p:
        scale = np.abs(grads[k]).max() + 1e-12
        np.testing.assert_allclose(g[k], grads[k], rtol=2e-3, atol=2e-4 * scale, err_msg="grad " + k)
        assert scale > 1e-9, "no gradient reached " + k
    got = eng.get_params()
    for k in p:
        np.testing.assert_allclose(got[k], newp[k], rtol=1e-4, atol=1e-5, err_msg="param " + k)


def tame_on_device(eng, p, frames):
    """mhsa_ref.tame_first_layer with the rms of the features the DEVICE computes (one forward); loads p into the engine."""
    eng.load_params(p)
    eng.forward_u8(frames, MEAN)
    rms = float(eng.feat[:frames.shape[0]].double().square().mean().sqrt())
    name = R.param_names(0)[0]
    p[name] = (p[name] / rms).astype(np.float32)
    eng.load_params(p)


# ---- 6. the output projection is fp32 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", ("f32", "bf16x3", "bf16"))
def test_the_output_projection_is_fp32_under_every_conv_math(math):
    """8 clips x 16 frames, H = 128, four heads: the output projection and its two gradients have 128 rows, columns and depth, the sizes
    from which ops.gemm WITH a workspace follows conv_math into split-bf16 arithmetic.  They are called without one, as attention_pool's
    are: each is compared with the fp64 product of the operands THE DEVICE holds, at class act (3e-5, 3e-5) -- an fp32 product of depth
    128 is two orders of magnitude inside it, a single-plane bf16 product (2^-9 per factor) two orders outside.  The attention between
    them is held to the reference from the qkv the device holds."""
    from vltf_amd.engine import LRCNEngine, NetConfig, init_params
    clips, fpc, H, heads = 8, 16, 128, 4
    n = clips * fpc
    cfg = NetConfig(image_shape=SHAPE, num_classes=NCLS, fpc=fpc, frame_encoding_layer="fc6", lstm_hidden=H, fusion="avg", rnn_cell="mhsa",
                    sa_heads=heads, conv_math=math)
    p = init_params(cfg, seed=3, well_scaled=True)
    names = R.param_names(0)
    r = np.random.default_rng(5)
    p[names[3]] = (0.1 * r.standard_normal(H)).astype(np.float32)
    p[names[4]] = (0.5 * r.standard_normal((heads, 2 * fpc - 1))).astype(np.float32)
    eng = LRCNEngine(cfg, max_clips=clips, device=DEV)
    rng = np.random.default_rng(12)
    frames = torch.from_numpy(rng.integers(0, 256, (n,) + SHAPE, dtype=np.uint8)).to(DEV)
    onehot = torch.from_numpy(np.eye(NCLS, dtype=np.int32)[rng.integers(0, NCLS, clips)]).to(DEV)
    tame_on_device(eng, p, frames)
    out = eng.train_step_u8(frames, onehot, lr=0.01, clip_norm=0.0, mean_bgr=MEAN)
    assert np.isfinite(out["loss"]) and out["rows"] == clips
    host = lambda t: t.detach().cpu().numpy().astype(np.float64)
    S = eng.mhsa[0]
    qkv, ctx, hseq, dout, dctx = (host(S[k][:n]) for k in ("qkv", "ctx", "hseq", "dout", "dctx"))
    Wo, bo, pos = (p[k].astype(np.float64) for k in names[2:])
    assert np.abs(ctx).max() > 1e-3 and np.abs(dout).max() > 0
    assert 0.1 < np.abs(qkv).mean() < 10                                     # (tame_on_device: scores of order 1)
    what = "self-attention products under conv_math %s: " % math
    fwd = R.forward(qkv, pos, heads, None, fpc)
    within("act", host(eng.self_attention_weights()), fwd.P, what + "P")
    within("act", ctx, fwd.ctx, what + "ctx")
    within("act", hseq, ctx @ Wo + bo, what + "hseq = ctx Wo + bo")
    within("act", host(eng.G[names[2]]), ctx.T @ dout, what + "G[out_kernel] = ctx^T dout")
    within("act", host(eng.G[names[3]]), dout.sum(axis=0), what + "G[out_bias]")
    within("act", dctx, dout @ Wo.T, what + "dctx = dout Wo^T")
    bwd = R.backward(dctx, qkv, host(eng.self_attention_weights()), heads, None, fpc)
    within("act", host(S["dqkv"][:n]), bwd.dqkv, what + "dqkv")
    within("act", host(eng.G[names[4]]), bwd.dposp.sum(axis=0), what + "G[position_bias]")


# ---- 7. the captured step ----------------------------------------------------------------------------------------------------------------
def test_lrcn_engine_captured_step_is_the_eager_step():
    """step_graph with dropout: the warm-up step, the captured one and three replays equal the eager engine's bit for bit -- the two
    self-attention launches take no host-varying argument and replay as they are."""
    from vltf_amd.engine import LRCNEngine, NetConfig, init_params
    engines = []
    kw = dict(image_shape=SHAPE, num_classes=NCLS, fpc=FPC, frame_encoding_layer="fc6", lstm_hidden=16, lstm_layers=2, fusion="avg",
              rnn_cell="mhsa", sa_heads=2, dropout_keep_prob=0.5)
    params = init_params(NetConfig(**kw), seed=4, well_scaled=True)
    rng = np.random.default_rng(11)
    some = torch.from_numpy(rng.integers(0, 256, (CLIPS * FPC,) + SHAPE, dtype=np.uint8)).to(DEV)
    for sg in (False, True):
        e = LRCNEngine(NetConfig(step_graph=sg, **kw), max_clips=CLIPS, device=DEV)
        if not sg:
            tame_on_device(e, params, some)                                  # (changes params: scores of order 1)
        e.load_params(params)
        engines.append(e)
    for step in range(5):
        frames = torch.from_numpy(rng.integers(0, 256, (CLIPS * FPC,) + SHAPE, dtype=np.uint8)).to(DEV)
        onehot = torch.from_numpy(np.eye(NCLS, dtype=np.int32)[rng.integers(0, NCLS, CLIPS)]).to(DEV)
        outs = [e.train_step_u8(frames, onehot, 0.01 * 0.7 ** step, 5.0, MEAN) for e in engines]
        for k in ("loss_sum", "correct", "grad_norm", "rows"):
            assert outs[0][k] == outs[1][k], (step, k, outs[0][k], outs[1][k])
        assert np.array_equal(engines[0].logits_host(), engines[1].logits_host()), step
        assert torch.equal(engines[0].self_attention_weights(), engines[1].self_attention_weights()), step
    assert len(engines[1]._graphs) == 1
    pa, pb = engines[0].get_params(), engines[1].get_params()
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), k
    pb_name = R.param_names(1)[4]
    assert not np.array_equal(pa[pb_name], params[pb_name])                  # the position bias trains


# ---- 8. GraphEngine: a vector-input pipeline with lengths ------------------------------------------------------------------------------
G_DIM, G_H, G_HEADS, G_C, G_CLIPS = 10, 16, 2, 5, 4


def graph_engine(T, layers=2, fusion="avg", seed=3, params=None):
    from vltf_amd.graph import DatasetInfo, GraphEngine, PipelineSpec, init_params_for, model_specs
    pipes = [PipelineSpec("net", ["main"], "nop", classifier="lstm", lstm_params=(G_H, layers, fusion), rnn_cell="mhsa", sa_heads=G_HEADS)]
    ds = {"main": DatasetInfo("vectors", T, 1, G_CLIPS, dim=G_DIM)}
    eng = GraphEngine(pipes, ds, G_C, device=DEV)
    p = params
    if p is None:
        p = init_params_for(model_specs(pipes, ds, G_C), seed=seed, well_scaled=True)
        for k in p:                                                 # biases (position_bias included) that are not zero
            if k.endswith("bias"):
                p[k] = (0.1 * np.random.default_rng(len(k)).standard_normal(p[k].shape)).astype(np.float32)
    eng.load_params(p)
    return eng, p


@pytest.mark.parametrize("fusion", ("avg", "last"))
def test_graph_engine_with_lengths_against_the_reference(fusion):
    from oracle import lrcn_oracle as O
    from tests import gru_ref
    T, lens = 5, np.array([5, 2, 1, 4])
    eng, p = graph_engine(T, fusion=fusion)
    x = (np.random.default_rng(8).standard_normal((G_CLIPS * T, G_DIM))).astype(np.float32)
    onehot = np.eye(G_C, dtype=np.int32)[np.random.default_rng(9).integers(0, G_C, G_CLIPS)]
    fd = {"main": torch.from_numpy(x).to(DEV)}
    got = eng.forward(fd, seq_len={"net": lens}).cpu().numpy()
    out, caches = R.stack_forward(x, p, T, 2, G_HEADS, lens=lens)
    fused = gru_ref.fuse(out, T, G_H, fusion, lens)
    want = fused @ p["output_fc_w"].astype(np.float64) + p["output_fc_b"]
    np.testing.assert_allclose(got, want, rtol=1e-3, atol=1e-3)
    loss, d = O.softmax_xent_mean(want, onehot, np.float64)
    grads = {"output_fc_w": fused.T @ d, "output_fc_b": d.sum(0)}
    dout = gru_ref.fuse_backward(d @ p["output_fc_w"].astype(np.float64).T, T, G_H, fusion, lens)
    grads.update(R.stack_backward(dout, caches)[1])
    res = eng.train_step(fd, torch.from_numpy(onehot).to(DEV), lr=0.01, clip_norm=0.0, seq_len={"net": lens})
    assert abs(res["loss"] - loss) < 1e-4 * max(1, abs(loss))
    g = eng.get_grads()
    assert set(g) == set(grads)
    for k in grads:
        scale = np.abs(grads[k]).max() + 1e-12
        np.testing.assert_allclose(g[k], grads[k], rtol=2e-3, atol=2e-4 * scale, err_msg="grad " + k)
        assert scale > 1e-9, "no gradient reached " + k


def test_graph_engine_padding_is_inert():
    """NaN (or other vectors) in the features of the padded frames change nothing: logits, the loss and every parameter after the step
    are bitwise equal, and finite."""
    T, lens = 5, [5, 2, 1, 4]
    live = R.live_mask(np.array(lens), G_CLIPS, T).reshape(-1)
    x = (np.random.default_rng(8).standard_normal((G_CLIPS * T, G_DIM))).astype(np.float32)
    onehot = torch.from_numpy(np.eye(G_C, dtype=np.int32)[np.random.default_rng(9).integers(0, G_C, G_CLIPS)]).to(DEV)
    res = []
    for fill in (None, "nan", 99):
        eng, _ = graph_engine(T)
        fed = x.copy()
        if fill == "nan":
            fed[~live] = np.nan
        elif fill is not None:
            fed[~live] = (np.random.default_rng(fill).standard_normal(fed[~live].shape) * 3).astype(np.float32)
        fd = {"main": torch.from_numpy(fed).to(DEV)}
        got = eng.forward(fd, seq_len={"net": lens}).cpu().numpy()
        out = eng.train_step(fd, onehot, lr=0.01, clip_norm=0.5, seq_len={"net": lens})
        assert out["rows"] == G_CLIPS and np.isfinite(got).all() and np.isfinite(out["loss"])
        res.append((got, out["loss"], eng.get_params()))
    for other in res[1:]:
        assert np.array_equal(res[0][0], other[0]) and res[0][1] == other[1]
        for k in res[0][2]:
            assert np.isfinite(other[2][k]).all() and np.array_equal(res[0][2][k], other[2][k]), "parameter %s moved with the padding" % k


def test_graph_engine_uniform_length_is_the_shorter_model():
    """Clips of length 3 in a 5-step batch give what they give in a 3-step model: logits, loss and the step.  The shorter model's
    position bias (heads, 2 L - 1) is the middle of the longer one's (heads, 2 T - 1): offsets -(L - 1) .. L - 1."""
    T, L = 5, 3
    x = (np.random.default_rng(8).standard_normal((G_CLIPS, T, G_DIM))).astype(np.float32)
    onehot = torch.from_numpy(np.eye(G_C, dtype=np.int32)[np.random.default_rng(9).integers(0, G_C, G_CLIPS)]).to(DEV)
    mid = slice(T - L, T - L + 2 * L - 1)
    is_pos = lambda k: k.endswith("position_bias")
    _, p_long = graph_engine(T)
    p_short = {k: np.ascontiguousarray(v[:, mid]) if is_pos(k) else v for k, v in p_long.items()}
    res = []
    for steps, kw, params in ((T, dict(seq_len={"net": [L] * G_CLIPS}), p_long), (L, {}, p_short)):
        eng, _ = graph_engine(steps, params=params)
        fd = {"main": torch.from_numpy(np.ascontiguousarray(x[:, :steps]).reshape(-1, G_DIM)).to(DEV)}
        logits = eng.forward(fd, **kw).cpu().numpy()
        out = eng.train_step(fd, onehot, lr=0.01, clip_norm=0.5, **kw)
        res.append((logits, out, eng.get_params()))
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=1e-5, atol=1e-6)
    assert res[0][1]["rows"] == res[1][1]["rows"] == G_CLIPS
    assert abs(res[0][1]["loss"] - res[1][1]["loss"]) < 1e-5 * max(1, abs(res[1][1]["loss"]))
    for k in res[0][2]:
        a = res[0][2][k][:, mid] if is_pos(k) else res[0][2][k]
        np.testing.assert_allclose(a, res[1][2][k], rtol=1e-4, atol=1e-6, err_msg="param " + k)
        if is_pos(k):                                                # offsets no live pair has: no gradient, not moved
            outer = np.ones(res[0][2][k].shape[1], bool)
            outer[mid] = False
            assert np.array_equal(res[0][2][k][:, outer], p_long[k][:, outer]) and not np.array_equal(a, p_short[k])


# ---- 9. two ranks ------------------------------------------------------------------------------------------------------------------------
def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def dp_worker(rank, world, port, q):
    """tests/test_dp_gpu.worker with rnn_cell mhsa: both ranks on cuda:0 over gloo, each on its half of the clips."""
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from vltf_amd import dp
    from vltf_amd.engine import LRCNEngine, NetConfig
    r, w, _ = dp.init_from_env(backend="gloo")
    assert (r, w) == (rank, world)
    shape, ncls, fpc, clips, hid, heads = (67, 67, 3), 5, 2, 4, 16, 2
    cfg = NetConfig(image_shape=shape, num_classes=ncls, fpc=fpc, lstm_hidden=hid, fusion="avg", rnn_cell="mhsa", sa_heads=heads)
    rng = np.random.default_rng(11)                                  # identical on every rank
    p = R.init_params(rng, ncls, "fc6", hid, 1, shape, heads, fpc)
    frames = R.varied_frames(rng, clips, fpc, shape)
    onehot = np.eye(ncls, dtype=np.int32)[rng.integers(0, ncls, clips)]
    R.tame_first_layer(p, frames.astype(np.float32) - MEAN, "fc6")   # (on the host: the same on every rank)
    # The tamed kernel (values / 30) has gradients x 30: the global norm is about 1150, and under tests/test_dp_gpu's clip_norm 0.5 every
    # update would shrink to a few ulps of its parameter (fc6b: 5 ulps), where `err` below measures the fp32 grid, not the exchange.
    # A clip norm above the global norm keeps the norm in the step and the updates at lr x gradient (at most 1e-4 of an ulp ratio).
    CLIP = 1e4
    lo, hi = dp.shard_range(clips, rank, world)
    gar = dp.GradAllReduce()
    eng = LRCNEngine(cfg, max_clips=hi - lo, device="cuda:0", dp=gar)
    eng.load_params(p)
    gar.broadcast_params(eng.w)
    sa = [eng.offsets[n] for n in R.param_names(0)]
    covered = all(any(o <= a and a + n <= o + c for o, c in eng.grad_chunks) for a, n in sa)
    out = eng.train_step_u8(torch.tensor(frames[lo * fpc:hi * fpc], device="cuda:0"), torch.tensor(onehot[lo:hi], device="cuda:0"),
                            lr=0.05, clip_norm=CLIP, mean_bgr=MEAN)
    got = eng.get_params()
    if rank == 0:
        ref = LRCNEngine(cfg, max_clips=clips, device="cuda:0")       # one engine, all the clips
        ref.load_params(p)
        want_out = ref.train_step_u8(torch.tensor(frames, device="cuda:0"), torch.tensor(onehot, device="cuda:0"), lr=0.05,
                                     clip_norm=CLIP, mean_bgr=MEAN)
        want = ref.get_params()
        err = {k: float(np.abs(got[k] - want[k]).max() / (np.abs(want[k] - p[k]).max() + 1e-12)) for k in want}
        moved = min(float(np.abs(want[n] - p[n]).max()) for n in R.param_names(0))
        q.put(("ok", max(err.values()), abs(out["grad_norm"] - want_out["grad_norm"]) / want_out["grad_norm"], covered, moved))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_rank_step_equals_one_rank():
    """tests/test_dp_gpu.test_two_rank_step_equals_one_rank with the self-attention variables in the exchange, at its tolerance."""
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


# ---- 10. run_task.py on examples/lrcn_self_attention.yml -------------------------------------------------------------------------------
def test_run_task_on_the_example_trains_validates_and_resumes(tmp_path, monkeypatch):
    """examples/lrcn_self_attention.yml pointed at the synthetic dataset (its shapes, four classes, one 16-wide layer of two heads,
    batches of 2, deterministic image processing): two epochs of three steps with a checkpoint each, a validation of the last, and a
    second training run that resumes from the first checkpoint and ends with exactly the weights of the uninterrupted run; the
    checkpoint holds the self-attention variables, and an engine built from it gives weights [clips, heads, T, T] whose rows sum to 1."""
    import glob
    import yaml
    from tests.test_host_workflow import make_dataset
    from tests.test_run_task_gpu import RAW, WANT
    from vltf_amd import run_task
    from vltf_amd.engine import LRCNEngine, NetConfig
    monkeypatch.setenv("VLTF_PREFETCH", "0")
    monkeypatch.setenv("VLTF_CONV_MATH", "f32")
    folder = str(tmp_path)
    train_path, _, _ = make_dataset(folder, "train.txt", shape=RAW, seed=1)
    val_path, _, _ = make_dataset(folder, "val.txt", nvid=3, cpv=(2, 1, 2), shape=RAW, seed=2)
    run = os.path.join(folder, "run")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def cfg(name, data_path, phase, resume=None):
        with open(os.path.join(root, "examples", "lrcn_self_attention.yml")) as f:
            c = yaml.safe_load(f)
        r = c["run"]
        r.update(resume_file=resume, run_folder=run, phase="defs.phase.%s" % phase)
        d = r["data"].pop("train_set")
        d.update(data_path=data_path, phase="defs.phase.%s" % phase, raw_image_shape=str(RAW), image_shape=str(WANT),
                 imgproc=["defs.imgproc.center_crop", "defs.imgproc.sub_mean"])
        r["data"]["d"] = d
        r["network"]["num_classes"] = 4
        pipe = r["network"]["pipelines"][0]["lrcn"]
        assert (pipe["rnn_cell"], pipe["sa_heads"], pipe["sa_positions"]) == ("mhsa", 4, "relative")
        pipe["lstm_params"] = [16, 1, "defs.fusion_method.avg"]
        pipe["sa_heads"] = 2
        r["train"].update(batch_size=2, epochs=2, base_lr=1e-2, lr_decay=["defs.decay.exp", "defs.periodicity.interval", 2, 0.9], clip_norm=5)
        r["val"]["batch_size"] = 2
        path = os.path.join(folder, name)
        with open(path, "w") as f:
            yaml.safe_dump(c, f)
        return path

    def checkpoints():
        return sorted(glob.glob(os.path.join(run, "checkpoints", "*.weights.npz")), key=os.path.getmtime)

    run_task.main(cfg("train.yml", train_path, "train"), seed=3)                           # 5 videos, batch 2: three steps an epoch
    ck = checkpoints()
    assert len(ck) == 2
    with np.load(ck[-1], allow_pickle=False) as z:
        full = {k: z[k] for k in z.files}
    names = R.param_names(0)
    assert all(n in full for n in names) and full["output_fc_w"].shape == (16, 4)
    assert [full[n].shape for n in names] == [(4096, 48), (48,), (16, 16), (16,), (2, 5)]
    assert full[names[4]].any()                                                            # the position bias left its zeros
    log = open(glob.glob(os.path.join(run, "log_lrcn_self_attention_train_scratch_*.log"))[0]).read()
    assert "global step: 6" in log
    acc = run_task.main(cfg("val.yml", val_path, "val", resume="latest"))
    assert 0.0 <= acc <= 1.0 and float(open(os.path.join(run, "accuracy_lrcn_self_attention_val_resume")).read()) == acc
    first = ck[0][:-len(".weights.npz")]
    run_task.main(cfg("resume.yml", train_path, "train", resume=first), seed=5)
    log2 = open(glob.glob(os.path.join(run, "log_lrcn_self_attention_train_resume_*.log"))[0]).read()
    assert "Restored training snapshot of epoch 1" in log2 and "global step: 6" in log2
    with np.load(checkpoints()[-1], allow_pickle=False) as z:
        resumed = {k: z[k] for k in z.files}
    assert set(resumed) == set(full)
    for k in full:
        np.testing.assert_array_equal(resumed[k], full[k], err_msg=k)
    # an engine on the trained weights
    eng = LRCNEngine(NetConfig(image_shape=WANT, num_classes=4, fpc=3, frame_encoding_layer="fc6", lstm_hidden=16, rnn_cell="mhsa", sa_heads=2),
                     max_clips=2, device=DEV, training=False)
    eng.load_params({k: v for k, v in full.items() if not k.startswith("__optimizer__/")})
    frames = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (6,) + WANT, dtype=np.uint8)).to(DEV)
    eng.forward_u8(frames, MEAN)
    w = eng.self_attention_weights()
    assert tuple(w.shape) == (2, 2, 3, 3)
    np.testing.assert_allclose(w.cpu().numpy().astype(np.float64).sum(axis=3), 1.0, rtol=0, atol=1e-6)
