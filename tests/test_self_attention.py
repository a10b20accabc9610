"""Multi-head self-attention over time (rnn_cell `mhsa`) without a GPU: tests/mhsa_ref.py against torch autograd in fp64 (the independent
oracle: the layer's output, P and every gradient, with and without per-clip lengths, with and without the position bias), the dead-row
contract of the reference, the float32 error of every kernel output (which decides the tolerance classes of
tests/test_self_attention_gpu.py), and the host plumbing: variable names, shapes and backward order, decay / trust-ratio classes,
initialisation, the learning-rate tier, the YAML keys with every refusal, checkpoint names, the example."""
import math
import os

import numpy as np
import pytest
import torch
import yaml

from tests import lstm_plan as LP
from tests import mhsa_ref as R
from tests.test_host_workflow import config, make_dataset

F64 = np.float64
# output -> tolerance class of tests/test_lstm_geometry_gpu.TOL (restated: that module needs a device to import its helpers' fixtures)
TOL = dict(act=(3e-5, 3e-5))
CLASS = dict(P="act", ctx="act", dqkv="act", dposp="act")


def layer_weights(case, d, k=1):
    """Wqkv [d][3H] ~ k N(0, 1) / sqrt(d) (so that qkv ~ k N(0, 1) for x ~ N(0, 1)), Wo [H][H] ~ N(0, 1) / sqrt(H), biases ~ 0.1 N(0, 1)."""
    batch, T, H, heads = case
    r = np.random.default_rng([batch, T, H, heads, k, 1])
    return (r.standard_normal((d, 3 * H)) * k / np.sqrt(d), r.standard_normal(3 * H) * 0.1, r.standard_normal((H, H)) / np.sqrt(H),
            r.standard_normal(H) * 0.1)


# ---- the reference against torch autograd ------------------------------------------------------------------------------------------
def torch_layer(x, Wqkv, bqkv, Wo, bo, pos, heads, T, L):
    """The layer written a second time in torch: torch.softmax with an ADDITIVE mask on the dead keys (-1e300: finite, so that a clip
    without a live key gives no NaN; exp of it is exactly 0 beside any live key), dead rows selected away with torch.where."""
    b = x.shape[0] // T
    H = Wo.shape[0]
    dh = H // heads
    live = torch.arange(T)[None, :] < torch.as_tensor(L)[:, None]                    # [B][T]
    rows = live.reshape(-1, 1)
    x = torch.where(rows, x, torch.zeros_like(x))
    qkv = x @ Wqkv + bqkv
    Q, K, V = (qkv[:, i * H:(i + 1) * H].reshape(b, T, heads, dh).permute(0, 2, 1, 3) for i in range(3))
    S = Q @ K.transpose(2, 3) / math.sqrt(dh)
    if pos is not None:
        S = S + pos[:, torch.as_tensor(R.rel_index(T))][None]
    mask = ((~live).to(S.dtype) * -1e300)[:, None, None, :]
    P = torch.softmax(S + mask, dim=3)
    ctx = (P @ V).permute(0, 2, 1, 3).reshape(b * T, H)
    y = torch.where(rows, ctx @ Wo + bo, torch.zeros_like(ctx))
    pair = live[:, None, :, None] & live[:, None, None, :]
    return y, torch.where(pair, P, torch.zeros_like(P))


@pytest.mark.parametrize("positions", (True, False), ids=("relative", "nopos"))
@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_the_reference_is_torch_autograd_in_fp64(case, lens, positions):
    """y, P, dx, dWqkv, dbqkv, dWo, dbo and dpos to 1e-10."""
    batch, T, H, heads = case
    d = 12
    r = np.random.default_rng([batch, T, H, heads, 2])
    x, dy = r.standard_normal((batch * T, d)), r.standard_normal((batch * T, H))
    Wqkv, bqkv, Wo, bo = layer_weights(case, d)
    pos = np.asarray(R.inputs(batch, T, H, heads, 1).pos, F64) if positions else None
    L = LP.lengths(batch, T) if lens else None
    y, cache = R.layer_forward(x, Wqkv, bqkv, Wo, bo, pos, heads, T, L)
    dx, grads = R.layer_backward(dy, cache)
    assert len(grads) == (5 if positions else 4)
    tens = [torch.tensor(np.asarray(a, F64), requires_grad=True) for a in (x, Wqkv, bqkv, Wo, bo)]
    tpos = torch.tensor(pos, requires_grad=True) if positions else None
    ty, tP = torch_layer(*tens, tpos, heads, T, R.live_lens(L, batch, T))
    ty.backward(torch.tensor(dy))
    tol = dict(rtol=0, atol=1e-10)
    np.testing.assert_allclose(y, ty.detach().numpy(), **tol)
    np.testing.assert_allclose(cache.fwd.P, tP.detach().numpy(), **tol)
    theirs = tens + ([tpos] if positions else [])
    for ours, t, name in zip([dx] + grads, theirs, ("dx", "dWqkv", "dbqkv", "dWo", "dbo", "dpos")):
        np.testing.assert_allclose(ours, t.grad.numpy(), err_msg=name, **tol)
    if positions:
        assert grads[4].shape == (heads, 2 * T - 1)


def test_the_lengths_exercise_the_clamp():
    """lstm_plan.lengths holds a 0, a T, a -3 and a T + 5; the launches' rule (the recurrence's) makes them 0, T, 0 and T."""
    lens = LP.lengths(5, 16)
    assert list(lens[:3]) == [0, 16, -3] and lens[-1] == 21
    assert list(R.live_lens(lens, 5, 16)[[0, 1, 2, 4]]) == [0, 16, 0, 16]
    assert list(R.live_lens(None, 2, 7)) == [7, 7]


@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_rows_of_p_sum_to_one_over_the_live_keys(case, lens):
    batch, T, H, heads = case
    for k in R.SCALES:
        ref = R.reference(case, k, lens)
        m = R.live_mask(ref.lens, batch, T)
        sums = ref.fwd.P.sum(axis=3)                                                 # [B][heads][T]
        np.testing.assert_allclose(sums, np.broadcast_to(m[:, None, :], sums.shape).astype(F64), rtol=0, atol=1e-13)
        assert (ref.fwd.P >= 0).all() and not ref.fwd.P[~(m[:, None, :, None] & m[:, None, None, :]).repeat(heads, axis=1)].any()


# ---- dead rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in R.CASES if c[0] > 1], ids=R.case_id)
def test_dead_rows_are_inert(case):
    """NaN in the dead rows of qkv and dctx changes nothing; dead rows of ctx, dqkv and P are zero."""
    batch, T, H, heads = case
    ref = R.reference(case, 1, True)
    dead = ~R.live_mask(ref.lens, batch, T).reshape(-1)
    assert dead.any() and not dead.all()
    nan = lambda a: R.with_nan_in_dead_rows(a, T, ref.lens)
    fwd = R.forward(nan(ref.inp.qkv), ref.inp.pos, heads, ref.lens, T)
    bwd = R.backward(nan(ref.inp.dctx), nan(ref.inp.qkv), ref.P32, heads, ref.lens, T)
    for a, b in zip(fwd + bwd, ref.fwd + ref.bwd):
        assert np.isfinite(a).all() and np.array_equal(a, b)
    assert not fwd.ctx[dead].any() and not bwd.dqkv[dead].any() and bwd.dqkv[~dead].any()
    P = fwd.P.transpose(0, 2, 1, 3).reshape(batch * T, heads, T)
    assert not P[dead].any() and not fwd.P.transpose(0, 3, 1, 2).reshape(batch * T, heads, T)[dead].any()


# ---- degenerate cases --------------------------------------------------------------------------------------------------------------
def test_one_step_gives_weight_one_and_no_score_gradient():
    case = batch, T, H, heads = (3, 1, 24, 3)
    inp = R.inputs(*case, 3)
    fwd = R.forward(inp.qkv, inp.pos, heads, None, T)
    bwd = R.backward(inp.dctx, inp.qkv, fwd.P, heads, None, T)
    assert (fwd.P == 1.0).all() and np.array_equal(fwd.ctx, np.asarray(inp.qkv[:, 2 * H:], F64))
    assert not bwd.dqkv[:, :2 * H].any() and not bwd.dposp.any() and np.array_equal(bwd.dqkv[:, 2 * H:], np.asarray(inp.dctx, F64))


def test_a_constant_added_to_the_position_bias_changes_nothing():
    case = batch, T, H, heads = (4, 7, 96, 1)
    inp = R.inputs(*case)
    L = LP.lengths(batch, T)
    a, b = (R.forward(inp.qkv, np.asarray(inp.pos, F64) + c, heads, L, T) for c in (0.0, 2.5))
    np.testing.assert_allclose(a.P, b.P, rtol=0, atol=1e-14)
    np.testing.assert_allclose(a.ctx, b.ctx, rtol=0, atol=1e-13)


# ---- tolerance classes -------------------------------------------------------------------------------------------------------------
def forward32(qkv, pos, heads, L, T):
    """The forward in plain float32 numpy, clip by clip and head by head."""
    f = np.float32
    H = qkv.shape[1] // 3
    b, dh = qkv.shape[0] // T, H // heads
    P, ctx = np.zeros((b, heads, T, T), f), np.zeros((b * T, H), f)
    scale = f(1.0 / math.sqrt(dh))
    rel = R.rel_index(T)
    for i, l in enumerate(L):
        rows = slice(i * T, i * T + l)
        for h in range(heads):
            q, k, v = (qkv[rows, j * H + h * dh:j * H + (h + 1) * dh] for j in range(3))
            s = (q @ k.T) * scale
            if pos is not None:
                s = s + pos[h][rel[:l, :l]]
            w = np.exp(s - s.max(axis=1, keepdims=True)) if l else s
            p = w / w.sum(axis=1, keepdims=True, dtype=f) if l else s
            assert s.dtype == p.dtype == f
            P[i, h, :l, :l] = p
            ctx[rows, h * dh:(h + 1) * dh] = p @ v
    return R.Forward(P, ctx)


def backward32(dctx, qkv, P, heads, L, T, positions):
    """The backward in plain float32 numpy, from P as given."""
    f = np.float32
    H = qkv.shape[1] // 3
    b, dh = qkv.shape[0] // T, H // heads
    dqkv = np.zeros((b * T, 3 * H), f)
    dposp = np.zeros((b, heads, 2 * T - 1), f)
    scale = f(1.0 / math.sqrt(dh))
    for i, l in enumerate(L):
        rows = slice(i * T, i * T + l)
        for h in range(heads):
            cols = [slice(j * H + h * dh, j * H + (h + 1) * dh) for j in range(3)]
            q, k, v = (qkv[rows, c] for c in cols)
            do, p = dctx[rows, h * dh:(h + 1) * dh], P[i, h, :l, :l]
            dp = do @ v.T
            ds = p * (dp - (dp * p).sum(axis=1, keepdims=True, dtype=f))
            assert ds.dtype == f
            dqkv[rows, cols[0]], dqkv[rows, cols[1]], dqkv[rows, cols[2]] = (ds @ k) * scale, (ds.T @ q) * scale, p.T @ do
            for r in range(T - l, T + l - 1):
                dposp[i, h, r] = np.trace(ds, offset=r - (T - 1), dtype=f)
    return R.Backward(dqkv, dposp if positions else None)


def test_float32_stays_inside_half_of_the_tolerance_classes():
    """Decides the classes of tests/test_self_attention_gpu.py: a plain float32 numpy evaluation of both launches (the backward from the
    reference's P rounded to fp32) against fp64 stays at or below 0.5 of class act's bound -- atol_rel * max|want| + rtol * |want| -- at
    every case, both scales, both length variants, with and without the position bias.  Measured with this evaluation, worst error / bound: P 0.101, ctx 0.163, dqkv 0.027, dposp
    0.079 (printed below): no class of this file's own is needed."""
    worst = {k: 0.0 for k in CLASS}
    for case in R.CASES:
        batch, T, H, heads = case
        for k in R.SCALES:
            for lens in (False, True):
                for positions in (True, False):
                    ref = R.reference(case, k, lens, positions)
                    L = [int(v) for v in R.live_lens(ref.lens, batch, T)]
                    inp = ref.inp
                    pos = inp.pos if positions else None
                    got = forward32(inp.qkv, pos, heads, L, T)._asdict()
                    got.update(backward32(inp.dctx, inp.qkv, ref.P32, heads, L, T, positions)._asdict())
                    want = dict(ref.fwd._asdict(), **ref.bwd._asdict())
                    for name, g in got.items():
                        if g is None:
                            assert want[name] is None
                            continue
                        assert g.dtype == np.float32
                        rtol, atol_rel = TOL[CLASS[name]]
                        w = np.asarray(want[name], F64)
                        bound = atol_rel * (float(np.abs(w).max()) or 1.0) + rtol * np.abs(w)
                        ratio = float((np.abs(g.astype(F64) - w) / bound).max())
                        worst[name] = max(worst[name], ratio)
                        assert ratio <= 0.5, "%s at case %s, k = %d, lens = %s: error / bound %.3f" % (name, case, k, lens, ratio)
    print("self-attention in float32, worst error / bound:", " ".join("%s %.3f" % kv for kv in sorted(worst.items())))


def test_the_classes_are_those_of_the_lstm_geometry_tests():
    """TOL above restates tests/test_lstm_geometry_gpu.TOL (read from its source: importing it would import its device helpers)."""
    import ast
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_lstm_geometry_gpu.py")).read()
    node = next(n for n in ast.parse(src).body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", None) == "TOL")
    theirs = {kw.arg: ast.literal_eval(kw.value) for kw in node.value.keywords}
    assert {k: theirs[k] for k in TOL} == TOL


# ---- host plumbing -----------------------------------------------------------------------------------------------------------------
def cfgs(**kw):
    from vltf_amd.engine import NetConfig
    base = dict(image_shape=(67, 67, 3), num_classes=7, fpc=3, lstm_hidden=16, lstm_layers=1, fusion="avg", rnn_cell="mhsa", sa_heads=2)
    base.update(kw)
    return NetConfig(**base)


TOWER = [("dcnn/fc6W", (256, 4096)), ("dcnn/fc6b", (4096,)), ("dcnn/conv5W", (3, 3, 192, 256)), ("dcnn/conv5b", (256,)),
         ("dcnn/conv4W", (3, 3, 192, 384)), ("dcnn/conv4b", (384,)), ("dcnn/conv3W", (3, 3, 256, 384)), ("dcnn/conv3b", (384,)),
         ("dcnn/conv2W", (5, 5, 48, 256)), ("dcnn/conv2b", (256,)), ("dcnn/conv1W", (11, 11, 3, 96)), ("dcnn/conv1b", (96,))]
SA = "self_attention/layer_%d/"


def layer_specs(l, d, H, heads, T, positions=True, scope=""):
    pre = scope + SA % l
    return [(pre + "qkv_kernel", (d, 3 * H)), (pre + "qkv_bias", (3 * H,)), (pre + "out_kernel", (H, H)), (pre + "out_bias", (H,))] + \
           ([(pre + "position_bias", (heads, 2 * T - 1))] if positions else [])


def test_param_specs_names_shapes_and_order():
    """Head, (attention_pool,) then the layers in forward order, each in the order of mhsa_names: the flat-buffer order of the GRU's list."""
    from vltf_amd.engine import mhsa_names, mhsa_specs, param_specs
    H, C, T = 16, 7, 3
    head = [("output_fc_w", (H, C)), ("output_fc_b", (C,))]
    assert mhsa_names(1) == R.param_names(1) == [n for n, _ in layer_specs(1, 5, H, 2, T)]
    assert mhsa_names(0, "p/", "none") == R.param_names(0, "p/", False)
    assert mhsa_specs(0, 4096, H, 2, T) == layer_specs(0, 4096, H, 2, T)
    assert param_specs(cfgs()) == head + layer_specs(0, 4096, H, 2, T) + TOWER
    assert param_specs(cfgs(lstm_layers=2)) == head + layer_specs(0, 4096, H, 2, T) + layer_specs(1, H, H, 2, T) + TOWER
    assert param_specs(cfgs(sa_positions="none")) == head + layer_specs(0, 4096, H, 2, T, False) + TOWER
    attn = [("attention_pool/kernel", (H, 5)), ("attention_pool/bias", (5,)), ("attention_pool/context", (5, 1))]
    assert param_specs(cfgs(fusion="attn", attn_dim=5)) == head + attn + layer_specs(0, 4096, H, 2, T) + TOWER
    # defaults: four heads where 4 divides H, else one; relative positions
    assert param_specs(cfgs(lstm_hidden=32, sa_heads=None))[6] == (SA % 0 + "position_bias", (4, 5))
    assert param_specs(cfgs(lstm_hidden=9, sa_heads=None))[6] == (SA % 0 + "position_bias", (1, 5))
    assert param_specs(cfgs(lstm_hidden=8, sa_heads=1, num_classes=8))[0][0] == SA % 0 + "qkv_kernel"      # H == C: no head


def test_initialisation_decay_trust_ratio_classes_and_tier():
    """Kernels glorot-uniform, the biases and position_bias zero; the two kernels and position_bias (rank 2) are decayed and
    trust-scaled, the two biases are neither; all carry lr_mult and train under train_from: classifier; the exchange chunks cover them."""
    from vltf_amd.engine import decay_ranges, finetune_plan, init_params, lamb_ranges, lars_ranges, param_specs
    from vltf_amd.graph import init_params_for
    cfg = cfgs(lr_mult=10.0, train_from="classifier", lstm_layers=2)
    specs = param_specs(cfg)
    offs, off = {}, 0
    for n, s in specs:
        offs[n] = (off, off + int(np.prod(s)))
        off += int(np.prod(s))
    names = R.param_names(0) + R.param_names(1)
    weights = [n for n in names if not n.endswith(("qkv_bias", "out_bias"))]
    biases = [n for n in names if n.endswith(("qkv_bias", "out_bias"))]
    assert len(weights) == 6 and len(biases) == 4
    for p in (init_params(cfg, seed=1), init_params_for(specs, seed=1)):
        for n in names:
            if n.endswith("kernel"):
                lim = np.sqrt(6.0 / sum(p[n].shape))
                assert p[n].std() > 0.4 * lim and np.abs(p[n]).max() <= lim        # uniform on [-lim, lim]: std lim / sqrt(3)
            else:
                assert not p[n].any(), n
        assert p[SA % 1 + "position_bias"].shape == (2, 5) and p[SA % 0 + "qkv_kernel"].shape == (4096, 48)
    plan = finetune_plan(cfg)
    assert plan.frozen and all(n.startswith("dcnn/") for n in plan.frozen)
    inside = lambda rng, lo, hi: any(a <= lo and hi <= b for a, b in rng)
    for n in names:
        lo, hi = offs[n]
        assert [m for a, b, m in plan.tiers if a <= lo and hi <= b] == [10.0], n               # the head's tier
        assert inside([(o, o + c) for o, c in plan.chunks], lo, hi), n
    ranges = decay_ranges(specs, plan, 5e-4)
    decayed, plain = [(a, b) for a, b, c in ranges if c > 0], [(a, b) for a, b, c in ranges if c == 0]
    lars, _, _ = lars_ranges(specs, plan, 0.0)
    lamb, _ = lamb_ranges(specs, plan, 0.0)
    for n in weights:
        lo, hi = offs[n]
        assert inside(decayed, lo, hi) and (lo, hi) in [(a, b) for a, b, _, t in lars if t >= 0] and (lo, hi) in [(r[0], r[1]) for r in lamb if r[4] >= 0], n
    for n in biases:
        lo, hi = offs[n]
        assert inside(plain, lo, hi) and not inside(decayed, lo, hi), n
        assert inside([(a, b) for a, b, _, t in lars if t < 0], lo, hi) and inside([(r[0], r[1]) for r in lamb if r[4] < 0], lo, hi), n


def test_engine_specs_and_refusals():
    from vltf_amd._ffi import VltfError
    from vltf_amd.composed import ComposedEngine, HeadConfig
    from vltf_amd.engine import NetConfig, check_mhsa, check_rnn_cell, param_specs
    from vltf_amd.graph import DatasetInfo, PipelineSpec, model_specs
    H, C, dim, T = 16, 5, 10, 4
    ds = {"main": DatasetInfo("vectors", T, 1, 3, dim=dim), "aux": DatasetInfo("vectors", 1, 1, 3, dim=7)}
    spec = lambda **kw: PipelineSpec("p", kw.pop("input", ["main"]), "nop", classifier=kw.pop("classifier", "lstm"), **kw)
    head = [("output_fc_w", (H, C)), ("output_fc_b", (C,))]
    # GraphEngine lists a pipeline's layers in backward order
    got = model_specs([spec(lstm_params=(H, 2, "avg"), rnn_cell="mhsa", sa_heads=2)], ds, C)
    assert got == head + layer_specs(1, H, H, 2, T) + layer_specs(0, dim, H, 2, T)
    got = model_specs([spec(lstm_params=(H, 1, "last"), rnn_cell="mhsa", sa_heads=1, sa_positions="none")], ds, C)
    assert got == head + layer_specs(0, dim, H, 1, T, False)
    two = [PipelineSpec("a", ["main"], "nop"), PipelineSpec("b", ["a"], "nop", classifier="lstm", lstm_params=(32, 1, "avg"), rnn_cell="mhsa")]
    assert ("b/" + SA % 0 + "position_bias", (4, 2 * T - 1)) in model_specs(two, ds, C)          # scoped like every other variable
    assert PipelineSpec("p", ["main"]).sa_heads is None and NetConfig().sa_positions is None and NetConfig().rnn_cell == "lstm"
    mh = dict(rnn_cell="mhsa", sa_heads=2)
    mhd = dict(rnn_cell="mhsa")                                                                                       # the default heads
    for match, pipe in (("sa_heads", spec(lstm_params=(H, 1, "avg"), sa_heads=2)),                                   # the keys without the cell
                        ("sa_positions", spec(lstm_params=(H, 1, "avg"), rnn_cell="gru", sa_positions="none")),
                        ("sa_heads", spec(classifier="fc", sa_heads=2)),
                        ("sa_heads", spec(lstm_params=(H, 1, "avg"), sa_heads=0, **mhd)),
                        ("sa_heads", spec(lstm_params=(H, 1, "avg"), sa_heads=2.0, **mhd)),
                        ("sa_heads", spec(lstm_params=(H, 1, "avg"), sa_heads=True, **mhd)),
                        ("sa_positions", spec(lstm_params=(H, 1, "avg"), sa_positions="absolute", **mh)),
                        ("H % heads == 0", spec(lstm_params=(H, 1, "avg"), sa_heads=3, **mhd)),
                        ("8 <= dh", spec(lstm_params=(H, 1, "avg"), sa_heads=4, **mhd)),                             # dh = 4
                        ("8 <= dh", spec(lstm_params=(8, 1, "avg"), **mhd)),                                          # the default four heads: dh = 2
                        ("dh = H / heads <= 128", spec(lstm_params=(258, 1, "avg"), **mh)),             # dh = 129
                        ("H <= 1024", spec(lstm_params=(1032, 1, "avg"), sa_heads=12, **mhd)),
                        ("lstm_bidirectional", spec(lstm_params=(H, 1, "avg"), lstm_bidirectional=True, **mh)),
                        ("classifier lstm", spec(classifier="fc", **mh)),
                        ("classifier lstm", spec(classifier=None, **mh)),
                        ("state input", spec(input=["main", "aux"], lstm_params=(H, 1, "avg"), **mh)),
                        ("fusion state", spec(lstm_params=(H, 1, "state"), **mh)),
                        ("must be lstm or gru", spec(lstm_params=(H, 1, "avg"), rnn_cell="transformer"))):
        with pytest.raises(VltfError, match=match):
            model_specs([pipe], ds, C)
    ds65 = {"main": DatasetInfo("vectors", 65, 1, 3, dim=dim)}
    with pytest.raises(VltfError, match="T <= 64"):
        model_specs([spec(lstm_params=(H, 1, "avg"), **mh)], ds65, C)
    # LRCNEngine's configuration
    for match, kw in (("sa_heads", dict(rnn_cell="lstm")), ("sa_positions", dict(rnn_cell="gru", sa_heads=None, sa_positions="none")),
                      ("sa_heads", dict(sa_heads=0)), ("sa_heads", dict(sa_heads="two")), ("sa_positions", dict(sa_positions="learned")),
                      ("H % heads == 0", dict(sa_heads=3)), ("8 <= dh", dict(sa_heads=4)), ("8 <= dh", dict(lstm_hidden=8, sa_heads=None)),
                      ("dh = H / heads <= 128", dict(lstm_hidden=129, sa_heads=1)), ("H <= 1024", dict(lstm_hidden=1032, sa_heads=12)),
                      ("T <= 64", dict(fpc=65)), ("lstm_bidirectional", dict(lstm_bidirectional=True)),
                      ("classifier lstm", dict(classifier="fc")), ("classifier lstm", dict(classifier="none")),
                      ("fusion state", dict(fusion="state")), ("must be lstm or gru", dict(rnn_cell="rnn", sa_heads=None))):
        with pytest.raises(VltfError, match=match):
            param_specs(cfgs(**kw))
    with pytest.raises(VltfError, match="state input"):
        check_rnn_cell("mhsa", state_input=True)
    assert check_mhsa("lstm") is None and check_mhsa("gru") is None
    assert check_mhsa("mhsa", 256, 16) == (4, "relative") and check_mhsa("mhsa", 250, 21, 5, "none") == (5, "none")
    assert check_mhsa("mhsa", 1024, 64, 8, "None") == (8, "relative") and check_mhsa("mhsa", 9, 1, "None") == (1, "relative")
    # the two-pipeline model keeps its LSTM
    for enc, head_cfg in ((cfgs(), HeadConfig(in_dim=4, fpc=3, num_classes=7)),):
        with pytest.raises(VltfError, match="not built for the two-pipeline model"):
            ComposedEngine(enc, head_cfg, 2, device="cpu")


def settings_for(folder, data_path, edit, name, phase="train"):
    from vltf_amd import settings_
    with open(config(folder, data_path, phase)) as f:
        cfg = yaml.safe_load(f)
    edit(cfg["run"]["network"]["pipelines"][0]["lrcn"], cfg["run"])
    out = os.path.join(folder, name)
    with open(out, "w") as f:
        yaml.safe_dump(cfg, f)
    s = settings_.Settings()
    return s, s.initialize(out)


AVG16 = [16, 1, "defs.fusion_method.avg"]


def test_the_yaml_keys(tmp_path):
    from vltf_amd import run_task
    folder = str(tmp_path)
    data_path, _, _ = make_dataset(folder, "train.txt")
    s, feeder = settings_for(folder, data_path, lambda p, r: p.update(lstm_params=AVG16, rnn_cell="mhsa", sa_heads=2, sa_positions="none"), "sa.yml")
    p = s.pipelines["lrcn"]
    assert (p.rnn_cell, p.sa_heads, p.sa_positions) == ("mhsa", 2, "none")
    cfg, _ = run_task.net_config(s, feeder.get_dataset_by_tag("main")[0])
    assert (cfg.rnn_cell, cfg.sa_heads, cfg.sa_positions, cfg.lstm_hidden, cfg.classifier) == ("mhsa", 2, "none", 16, "lstm")
    specs, _, _ = run_task.graph_config(s, feeder, 2)
    assert (specs[0].rnn_cell, specs[0].sa_heads, specs[0].sa_positions) == ("mhsa", 2, "none")
    # the defaults, None / "None" meaning absent
    for extra, want in ((dict(lstm_params=[32, 1, "defs.fusion_method.avg"]), (4, "relative")), (dict(sa_heads="None", sa_positions=None), (4, "relative")),
                        (dict(lstm_params=[9, 2, "defs.fusion_method.last"], sa_positions="relative"), (1, "relative"))):
        kw = dict(dict(lstm_params=[32, 1, "defs.fusion_method.avg"], rnn_cell="mhsa"), **extra)
        s, feeder = settings_for(folder, data_path, lambda p, r: p.update(**kw), "default.yml")
        assert (s.pipelines["lrcn"].sa_heads, s.pipelines["lrcn"].sa_positions) == want
        cfg, _ = run_task.net_config(s, feeder.get_dataset_by_tag("main")[0])
        assert (cfg.sa_heads, cfg.sa_positions) == want
    # without the cell: no keys, today's configuration
    s, feeder = settings_for(folder, data_path, lambda p, r: None, "plain.yml")
    assert (s.pipelines["lrcn"].rnn_cell, s.pipelines["lrcn"].sa_heads, s.pipelines["lrcn"].sa_positions) == ("lstm", None, None)
    cfg, _ = run_task.net_config(s, feeder.get_dataset_by_tag("main")[0])
    assert (cfg.rnn_cell, cfg.sa_heads, cfg.sa_positions) == ("lstm", None, None)
    assert run_task.graph_config(s, feeder, 2)[0][0].sa_heads is None
    mh = dict(lstm_params=AVG16, rnn_cell="mhsa", sa_heads=2)
    mhd = dict(lstm_params=AVG16, rnn_cell="mhsa")                                                                    # the default heads
    fc = lambda p: p.update(classifier="defs.classifier.fc", lstm_params=None)
    for match, edit in (("sa_heads", lambda p, r: p.update(sa_heads=2)),                                             # without the cell
                        ("sa_positions", lambda p, r: p.update(rnn_cell="gru", sa_positions="none")),
                        ("sa_heads", lambda p, r: p.update(sa_heads=0, **mhd)),
                        ("sa_heads", lambda p, r: p.update(sa_heads=2.5, **mhd)),
                        ("sa_heads", lambda p, r: p.update(sa_heads="two", **mhd)),
                        ("sa_positions", lambda p, r: p.update(sa_positions="sinusoidal", **mh)),
                        ("H % heads == 0", lambda p, r: p.update(sa_heads=3, **mhd)),
                        ("8 <= dh", lambda p, r: p.update(sa_heads=4, **mhd)),
                        ("8 <= dh", lambda p, r: p.update(rnn_cell="mhsa")),                                         # H = 8, four heads by default
                        ("dh = H / heads <= 128", lambda p, r: p.update(lstm_params=[129, 1, "defs.fusion_method.avg"], rnn_cell="mhsa")),
                        ("H <= 1024", lambda p, r: p.update(lstm_params=[1032, 1, "defs.fusion_method.avg"], rnn_cell="mhsa", sa_heads=12)),
                        ("lstm_bidirectional", lambda p, r: p.update(lstm_bidirectional=True, **mh)),
                        ("classifier lstm", lambda p, r: (fc(p), p.update(rnn_cell="mhsa"))),
                        ("classifier lstm", lambda p, r: (p.pop("classifier"), p.pop("lstm_params"), p.update(rnn_cell="mhsa"))),
                        ("sa_heads", lambda p, r: (fc(p), p.update(sa_heads=2))),
                        ("fusion state", lambda p, r: p.update(lstm_params=[16, 1, "defs.fusion_method.state"], rnn_cell="mhsa")),
                        ("must be lstm or gru", lambda p, r: p.update(rnn_cell="transformer"))):
        with pytest.raises(Exception, match=match):
            settings_for(folder, data_path, edit, "bad.yml")


def test_the_unknown_cell_message_still_names_lstm_and_gru():
    from vltf_amd._ffi import VltfError
    from vltf_amd.engine import RNN_CELLS, check_rnn_cell
    assert RNN_CELLS == ("lstm", "gru", "mhsa")
    with pytest.raises(VltfError, match="must be lstm or gru") as e:
        check_rnn_cell("rnn")
    assert "mhsa" in str(e.value) and "[rnn]" in str(e.value)
    assert [check_rnn_cell(c) for c in RNN_CELLS] == list(RNN_CELLS)


def test_the_example_parses():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "examples", "lrcn_self_attention.yml")) as f:
        cfg = yaml.safe_load(f)
    p = cfg["run"]["network"]["pipelines"][0]["lrcn"]
    assert p["lstm_params"] == [256, 1, "defs.fusion_method.avg"] and p["classifier"] == "defs.classifier.lstm"
    assert (p["rnn_cell"], p["sa_heads"], p["sa_positions"]) == ("mhsa", 4, "relative")
    assert cfg["run"]["run_id"] == "lrcn_self_attention"


class StubEngine:
    """What feeder.save / init_saveload need of an engine."""
    OPT_PREFIX, training = "opt/", False

    def __init__(self, cfg, seed):
        from vltf_amd.engine import init_params, param_specs
        self.specs, self.params = param_specs(cfg), init_params(cfg, seed=seed)

    def get_params(self):
        return self.params

    def load_params(self, params):
        assert set(params) == {n for n, _ in self.specs}
        self.params = dict(params)


def test_checkpoint_names(tmp_path):
    """A checkpoint holds the self-attention variables under their names and restores into an mhsa model; an LSTM or GRU checkpoint is
    refused by an mhsa model, and an mhsa checkpoint by an LSTM or GRU model."""
    from vltf_amd import settings_
    folder = str(tmp_path)
    data_path, _, _ = make_dataset(folder, "train.txt")
    s = settings_.Settings()
    feeder = s.initialize(config(folder, data_path))
    small = dict(image_shape=(16, 16, 3), num_classes=4)
    other = dict(sa_heads=None, **small)
    feeder.compute_save_interval()
    feeder.num_saves = 0                                                    # keep every checkpoint
    bases = {}
    for tag, cfg in (("mhsa", cfgs(**small)), ("lstm", cfgs(rnn_cell="lstm", **other)), ("gru", cfgs(rnn_cell="gru", **other))):
        saved = StubEngine(cfg, seed=1)
        bases[tag] = (feeder.save(saved, "ep_%s" % tag, 2), saved)
    base, saved = bases["mhsa"]
    with np.load(base + ".weights.npz") as z:
        names = set(z.files)
        assert z[SA % 0 + "position_bias"].shape == (2, 5) and z[SA % 0 + "qkv_kernel"].shape == (4096, 48)
    assert names == {n for n, _ in saved.specs} and set(R.param_names(0)) <= names
    s2 = settings_.Settings()
    f2 = s2.initialize(config(folder, data_path, resume_file=base))
    fresh = StubEngine(cfgs(**small), seed=2)
    f2.init_saveload(fresh, base)
    for n in saved.params:
        assert np.array_equal(fresh.params[n], saved.params[n]), n
    for tag in ("lstm", "gru"):
        with pytest.raises(Exception):
            f2.init_saveload(StubEngine(cfgs(**small), seed=2), bases[tag][0])
        with pytest.raises(Exception):
            f2.init_saveload(StubEngine(cfgs(rnn_cell=tag, **other), seed=2), base)
    with pytest.raises(Exception):                                          # nor one without the position bias
        f2.init_saveload(StubEngine(cfgs(sa_positions="none", **small), seed=2), base)
