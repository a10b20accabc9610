"""NetVLAD pooling over time (fusion `vlad`) without a GPU: tests/netvlad_ref.py against torch autograd in fp64 (the independent oracle:
y, a and every gradient, with and without per-clip lengths), the dead-row contract of the reference, the degenerate cases (one live
step, saturated scores and the epsilon branch), the float32 error of every kernel output in the kernels' order of operations (which
decides the tolerance classes of tests/test_netvlad_gpu.py), and the host plumbing: variable names, shapes and order, decay /
trust-ratio classes, initialisation, the learning-rate tier, the YAML keys with every refusal, checkpoint names, and the variable lists
of models WITHOUT the fusion against literal lists."""
import math
import os

import numpy as np
import pytest
import torch
import yaml

from tests import lstm_plan as P
from tests import netvlad_ref as R
from tests.test_attn_pool import PLAIN, TOWER, StubEngine, settings_for
from tests.test_host_workflow import config, make_dataset

F64 = np.float64
# output -> tolerance class of tests/test_lstm_geometry_gpu.TOL (restated: that module needs a device to import its helpers' fixtures),
# tightest first
TOL = dict(hseq=(1e-5, 1e-6), act=(3e-5, 3e-5))
CLASS = dict(a="hseq", r="hseq", y="hseq", ds="hseq", dh="hseq", dcp="hseq")


def layer_weights(case, k):
    """W [HO][K] ~ k N(0, 1) / sqrt(HO) (so that s = h W + beta ~ k N(0, 1)), beta [K] ~ 0.1 N(0, 1)."""
    batch, T, HO, K = case
    r = np.random.default_rng([batch, T, HO, K, k, 1])
    return r.standard_normal((HO, K)) * k / np.sqrt(HO), r.standard_normal(K) * 0.1


# ---- the reference against torch autograd ------------------------------------------------------------------------------------------
def torch_layer(x, W, beta, c, T, L):
    """The layer written a second time, clip by clip, in torch, the normalisation as tf.nn.l2_normalize writes it."""
    K = c.shape[0]
    ys, As = [], []
    for i, l in enumerate(L):
        hi = x[i * T:i * T + int(l)]
        a = torch.softmax(hi @ W + beta, dim=1)                                  # [l, K]
        V = a.t() @ hi - a.sum(dim=0)[:, None] * c                               # [K, HO]
        U = V * torch.rsqrt(torch.clamp((V * V).sum(dim=1, keepdim=True), min=R.EPS))
        ys.append(U.reshape(-1) / math.sqrt(K))
        As.append(torch.cat([a, torch.zeros(T - int(l), K, dtype=a.dtype)]))
    return torch.stack(ys), torch.cat(As)


@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_the_reference_is_torch_autograd_in_fp64(case, lens):
    """y, a, dx, dW, dbeta and dc to 1e-12."""
    batch, T, HO, K = case
    inp = R.inputs(batch, T, HO, K, 1)
    W, beta = layer_weights(case, 1)
    L = P.lengths(batch, T) if lens else None
    y, cache = R.pool_layer_forward(inp.h, W, beta, inp.c, T, L)
    dx, dW, db, dc = R.pool_layer_backward(inp.dy, cache)
    assert y.shape == (batch, K * HO) and dc.shape == (K, HO)
    tx, tW, tb, tc = (torch.tensor(np.asarray(a, F64), requires_grad=True) for a in (inp.h, W, beta, inp.c))
    ty, ta = torch_layer(tx, tW, tb, tc, T, R.fusion_lens(L, batch, T))
    ty.backward(torch.tensor(np.asarray(inp.dy, F64)))
    tol = dict(rtol=0, atol=1e-12)
    np.testing.assert_allclose(y, ty.detach().numpy(), **tol)
    np.testing.assert_allclose(cache.fwd.a, ta.detach().numpy(), **tol)
    for ours, theirs, name in ((dx, tx, "dx"), (dW, tW, "dW"), (db, tb, "db"), (dc, tc, "dc")):
        np.testing.assert_allclose(ours, theirs.grad.numpy(), err_msg=name, **tol)


def test_the_epsilon_branch_is_torch_autograd_in_fp64():
    """A starved cluster (|V_k|^2 below the epsilon) is scaled by the constant 1e6 in both directions, as the clamp's autograd does."""
    case = batch, T, HO, K = (2, 1, 6, 3)
    inp = R.inputs(*case)
    W = np.zeros((HO, K))
    beta = np.array([0.0, -40.0, 1.0])                                          # a_1 ~ e^-41: |V_1|^2 ~ 1e-35
    y, cache = R.pool_layer_forward(inp.h, W, beta, inp.c, T, None)
    assert (cache.fwd.r[:, 1] == R.RMAX).all() and (cache.fwd.r[:, [0, 2]] < R.RMAX).all()
    dx, dW, db, dc = R.pool_layer_backward(inp.dy, cache)
    tx, tW, tb, tc = (torch.tensor(np.asarray(a, F64), requires_grad=True) for a in (inp.h, W, beta, inp.c))
    ty, _ = torch_layer(tx, tW, tb, tc, T, [T] * batch)
    ty.backward(torch.tensor(np.asarray(inp.dy, F64)))
    np.testing.assert_allclose(y, ty.detach().numpy(), rtol=0, atol=1e-12)
    for ours, theirs, name in ((dx, tx, "dx"), (dW, tW, "dW"), (db, tb, "db"), (dc, tc, "dc")):
        np.testing.assert_allclose(ours, theirs.grad.numpy(), rtol=0, atol=1e-12, err_msg=name)


def test_no_drawn_cluster_sits_at_the_epsilon():
    """Every input the GPU tests draw keeps |V_k|^2 outside [1e-12 / 16, 16e-12] (asserted inside the reference), at both scales, with
    and without lengths; and the lengths hold a 0, a T, a -3 and a T + 5, which the fusion's rule makes 1, T, 1 and T."""
    for case in R.CASES:
        for k in R.SCALES:
            for lens in (False, True):
                ref = R.reference(case, k, lens)
                assert ref.fwd.y.shape == (case[0], case[2] * case[3])
    lens = P.lengths(5, 16)
    assert list(lens[:3]) == [0, 16, -3] and lens[-1] == 21
    assert list(R.fusion_lens(lens, 5, 16)[[0, 1, 2, 4]]) == [1, 16, 1, 16]


# ---- dead rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in R.CASES if c[0] > 1], ids=R.case_id)
def test_dead_rows_are_inert(case):
    """NaN in the dead rows of h, s and a changes nothing, and the gradients of the dead rows are zero."""
    batch, T, HO, K = case
    ref = R.reference(case, 1, True)
    dead = ~R.live_mask(ref.lens, batch, T).reshape(-1)
    assert dead.any() and not dead.all()
    nan = lambda a: R.with_nan_in_dead_rows(a, T, ref.lens)
    fwd = R.forward(nan(ref.inp.h), nan(ref.inp.s), ref.inp.c, ref.lens, T)
    bwd = R.backward(ref.inp.dy, nan(ref.inp.h), nan(ref.a32), ref.r32, ref.y32, ref.inp.c, ref.lens, T)
    for a, b in zip(fwd + bwd, ref.fwd + ref.bwd):
        assert np.isfinite(a).all() and np.array_equal(a, b)
    assert not fwd.a[dead].any() and not bwd.ds[dead].any() and not bwd.dh[dead].any()
    assert bwd.ds[~dead].any() and bwd.dh[~dead].any()
    np.testing.assert_allclose(fwd.a[~dead].sum(axis=1), 1.0, rtol=0, atol=1e-14)
    W, beta = layer_weights(case, 1)
    y, cache = R.pool_layer_forward(nan(ref.inp.h), W, beta, ref.inp.c, T, ref.lens)
    dx, dW, db, dc = R.pool_layer_backward(ref.inp.dy, cache)
    assert all(np.isfinite(a).all() for a in (y, dx, dW, db, dc)) and not dx[dead].any()


# ---- degenerate cases --------------------------------------------------------------------------------------------------------------
def test_one_live_step_gives_unit_residuals_and_no_score_gradient():
    """T = 1: y_k is the unit vector of h - c_k over sqrt(K) whatever the scores, and ds vanishes -- every da_tk is dV_k . (h - c_k) =
    dV_k . V_k / a_k = 0 by the projection.  ds is bounded by the class's absolute term at the magnitude of the CANCELLING terms
    a |dV_k| |h - c_k|, not at the result, which is zero."""
    case = batch, T, HO, K = (3, 1, 37, 3)
    inp = R.inputs(*case, 3)
    fwd = R.forward(inp.h, inp.s, inp.c, None, T)
    bwd = R.backward(inp.dy, inp.h, fwd.a, fwd.r, fwd.y, inp.c, None, T)
    d = np.asarray(inp.h, F64)[:, None, :] - np.asarray(inp.c, F64)[None]                      # [B][K][HO]
    unit = d / np.linalg.norm(d, axis=2, keepdims=True) / math.sqrt(K)
    np.testing.assert_allclose(fwd.y.reshape(batch, K, HO), unit, rtol=0, atol=1e-15)
    dV = -bwd.dcp.reshape(batch, K, HO) / fwd.a[:, :, None]                                     # m_k = a_k at T = 1
    mag = (fwd.a * np.linalg.norm(dV, axis=2) * np.linalg.norm(d, axis=2)).max()
    assert mag > 0.1 and np.abs(bwd.ds).max() <= TOL["act"][1] * 1e-8 * mag                     # fp64: far inside the class
    np.testing.assert_allclose(bwd.dh, np.einsum("bk,bkh->bh", fwd.a, dV), rtol=0, atol=1e-14)


def saturated_inputs():
    """(2, 21, 250, 5) with scores of +-200: cluster 0 takes every even step, cluster 1 every odd one, the other three starve."""
    case = batch, T, HO, K = (2, 21, 250, 5)
    inp = R.inputs(*case)
    s = np.full((batch * T, K), -200.0)
    s[np.arange(batch * T) % T % 2 == 0, 0] = 200.0
    s[np.arange(batch * T) % T % 2 == 1, 1] = 200.0
    return case, inp, s


def test_scores_of_two_hundred_stay_finite():
    """The epsilon branch: a starved cluster has r = 1e6 and a y that is zero in fp32; everything stays finite."""
    (batch, T, HO, K), inp, s = saturated_inputs()
    fwd = R.forward(inp.h, s, inp.c, None, T)
    bwd = R.backward(inp.dy, inp.h, P.rounded(fwd.a), P.rounded(fwd.r), P.rounded(fwd.y), inp.c, None, T)
    assert all(np.isfinite(a).all() for a in fwd + bwd)
    assert (fwd.r[:, 2:] == R.RMAX).all() and (fwd.r[:, :2] < 1.0).all()
    y32 = np.asarray(fwd.y, np.float32).reshape(batch, K, HO)
    assert not y32[:, 2:].any() and y32[:, :2].all()
    np.testing.assert_allclose(np.linalg.norm(fwd.y.reshape(batch, K, HO)[:, :2], axis=2), 1 / math.sqrt(K), rtol=0, atol=1e-15)
    np.testing.assert_allclose(fwd.a.sum(axis=1), 1.0, rtol=0, atol=1e-14)


# ---- tolerance classes -------------------------------------------------------------------------------------------------------------
f32 = np.float32


def lane_sum(x):
    """Sum over the last axis as a wave does it: lane l adds its elements l, l + 64, .. in order, then the xor shuffle tree."""
    n = x.shape[-1]
    pad = (-n) % 64
    x = np.concatenate([x, np.zeros(x.shape[:-1] + (pad,), f32)], axis=-1).reshape(x.shape[:-1] + (-1, 64))
    acc = np.zeros(x.shape[:-2] + (64,), f32)
    for i in range(x.shape[-2]):
        acc = acc + x[..., i, :]
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., np.arange(64) ^ o]
    assert acc.dtype == f32
    return acc[..., 0]


def block_sum(x):
    """Sum over the last axis as the forward's 256 threads do: thread t adds columns t, t + 256, .. in order, a tree per wave, then the
    four waves in order."""
    n = x.shape[-1]
    pad = (-n) % 256
    x = np.concatenate([x, np.zeros(x.shape[:-1] + (pad,), f32)], axis=-1).reshape(x.shape[:-1] + (-1, 256))
    acc = np.zeros(x.shape[:-2] + (256,), f32)
    for i in range(x.shape[-2]):
        acc = acc + x[..., i, :]
    w = lane_sum(acc.reshape(acc.shape[:-1] + (4, 64)))
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def forward32(h, s, c, L, T):
    """The forward in float32 numpy, in the kernel's order: the row softmax, V by steps ascending, the norm by block_sum."""
    K, HO = c.shape
    b = s.shape[0] // T
    a = np.zeros((b, T, K), f32)
    r = np.zeros((b, K), f32)
    y = np.zeros((b, K, HO), f32)
    isk = f32(1) / np.sqrt(f32(K))
    for i, l in enumerate(L):
        si, hi = s[i * T:i * T + l], h[i * T:i * T + l]
        e = np.exp(si - si.max(axis=1, keepdims=True))
        ai = e / lane_sum(e)[:, None]
        acc, m = np.zeros((K, HO), f32), np.zeros(K, f32)
        for t in range(l):
            acc = acc + ai[t][:, None] * hi[t][None, :]
            m = m + ai[t]
        V = acc - m[:, None] * c
        n2 = block_sum(V * V)
        ri = np.where(n2 > f32(R.EPS), f32(1) / np.sqrt(np.maximum(n2, f32(1e-30))), f32(R.RMAX)).astype(f32)
        a[i, :l], r[i], y[i] = ai, ri, V * (ri * isk)[:, None]
        assert ai.dtype == V.dtype == n2.dtype == f32
    return R.Forward(a.reshape(b * T, K), r, y.reshape(b, K * HO))


def backward32(dy, h, a, r, y, c, L, T):
    """The backward in float32 numpy, in the kernel's order, from a, r and y as given."""
    K, HO = c.shape
    b = dy.shape[0]
    ds, dh, dcp = np.zeros((b * T, K), f32), np.zeros((b * T, HO), f32), np.zeros((b, K, HO), f32)
    sk = np.sqrt(f32(K))
    isk = f32(1) / sk
    for i, l in enumerate(L):
        rows = slice(i * T, i * T + l)
        hi, ai, ri = h[rows], a[rows], r[i]
        yi, dyi = y[i].reshape(K, HO), dy[i].reshape(K, HO)
        dot = lane_sum(yi * dyi)
        dU, U = dyi * isk, yi * sk
        dV = np.where((ri < f32(R.RMAX))[:, None], ri[:, None] * (dU - U * dot[:, None]), ri[:, None] * dU).astype(f32)
        da = np.stack([lane_sum(dV * (hi[t][None, :] - c)) for t in range(l)])                    # [l][K]
        m = np.zeros(K, f32)
        for t in range(l):
            m = m + ai[t]
        ds[rows] = ai * (da - lane_sum(ai * da)[:, None])
        acc = np.zeros((l, HO), f32)
        for k in range(K):
            acc = acc + ai[:, k][:, None] * dV[k][None, :]
        dh[rows] = acc
        dcp[i] = dV * (-m)[:, None]
        assert dV.dtype == da.dtype == acc.dtype == f32
    return R.Backward(ds, dh, dcp.reshape(b, K * HO))


def float32_ratios():
    """{output: {class: worst error / bound}} over every case, both scales and both length variants; bound = atol_rel scale + rtol |want|,
    scale = max|want| (for ds no less than the cancelling terms: netvlad_ref.abs_scale)."""
    worst = {k: {c: 0.0 for c in TOL} for k in CLASS}
    for case in R.CASES:
        batch, T, HO, K = case
        for k in R.SCALES:
            for lens in (False, True):
                ref = R.reference(case, k, lens)
                L = [int(v) for v in R.fusion_lens(ref.lens, batch, T)]
                inp = ref.inp
                got = forward32(inp.h, inp.s, inp.c, L, T)._asdict()
                got.update(backward32(inp.dy, inp.h, ref.a32, ref.r32, ref.y32, inp.c, L, T)._asdict())
                want = dict(ref.fwd._asdict(), **ref.bwd._asdict())
                for name, g in got.items():
                    assert g.dtype == np.float32
                    w = np.asarray(want[name], F64)
                    for cls, (rtol, atol_rel) in TOL.items():
                        bound = atol_rel * R.abs_scale(ref, name) + rtol * np.abs(w)
                        worst[name][cls] = max(worst[name][cls], float((np.abs(g.astype(F64) - w) / bound).max()))
    return worst


def test_float32_in_the_kernels_order_decides_the_tolerance_classes():
    """Decides the classes of tests/test_netvlad_gpu.py: a float32 numpy restatement of both launches in the kernels' order of
    operations (the backward from the reference's a, r and y rounded to fp32) against fp64 stays at or below 0.5 of the class's bound
    at every case, both scales and both length variants, and each output has the TIGHTEST class for which that holds.  Measured with
    this restatement, worst error / bound under hseq (1e-5 / 1e-6), the tightest class there is: a 0.017, r 0.052, y 0.148, ds 0.069,
    dh 0.132, dcp 0.032 (under act, 3e-5 / 3e-5: all below 0.01).  So every output takes hseq, and with it the "no tighter class
    fits" half of the loop below has nothing to test -- no class of the geometry tests is tighter than hseq; it would only come into
    play for an output moved to act.  The figures are printed."""
    worst = float32_ratios()
    print("NetVLAD in float32, worst error / bound:", " ".join("%s %s" % (k, " ".join("%s %.3f" % kv for kv in v.items())) for k, v in sorted(worst.items())))
    order = list(TOL)
    for name, cls in CLASS.items():
        assert worst[name][cls] <= 0.5, (name, cls, worst[name])
        for tighter in order[:order.index(cls)]:
            assert worst[name][tighter] > 0.5, "%s would fit the tighter class %s: %r" % (name, tighter, worst[name])


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
    base = dict(image_shape=(67, 67, 3), num_classes=7, fpc=3, lstm_hidden=8, lstm_layers=1, fusion="vlad", vlad_clusters=3)
    base.update(kw)
    return NetConfig(**base)


def vlad(HO, K, scope=""):
    return [(scope + "netvlad/kernel", (HO, K)), (scope + "netvlad/bias", (K,)), (scope + "netvlad/centers", (K, HO))]


@pytest.mark.parametrize("cell", sorted(PLAIN))
def test_a_model_without_the_fusion_has_the_variables_it_had(cell):
    from vltf_amd.engine import NetConfig, param_specs
    kw, head = PLAIN[cell]
    cfg = NetConfig(image_shape=(67, 67, 3), num_classes=7, fpc=3, lstm_hidden=8, **kw)
    assert cfg.vlad_clusters is None and cfg.fusion == "avg"
    assert param_specs(cfg) == head + TOWER


def test_param_specs_names_shapes_and_order():
    from vltf_amd.engine import param_specs, vlad_names, vlad_specs
    H, K, C = 8, 3, 7
    assert [n for n, _ in vlad(H, K)] == vlad_names() == R.param_names() and vlad_specs(H, K) == vlad(H, K)
    # between the head and the recurrent layers, for every cell; the head reads K x HO columns
    for cell, (kw, plain) in PLAIN.items():
        HO = 16 if cell == "blstm" else 8
        want = [("output_fc_w", (K * HO, C)), ("output_fc_b", (C,))] + vlad(HO, K) + plain[2:]
        assert param_specs(cfgs(**kw)) == want + TOWER, cell
    for kw in (dict(rnn_cell="mhsa", sa_heads=1), dict(rnn_cell="mhsa", sa_heads=1, sa_block="encoder")):
        got = param_specs(cfgs(**kw))
        assert got[:5] == [("output_fc_w", (K * H, C)), ("output_fc_b", (C,))] + vlad(H, K) and got[5][0].startswith("self_attention")
    assert param_specs(cfgs(vlad_clusters=None))[:5] == [("output_fc_w", (8 * H, C)), ("output_fc_b", (C,))] + vlad(H, 8)      # the default
    # the width-equals-classes rule compares K x HO
    assert param_specs(cfgs(num_classes=24))[0] == ("netvlad/kernel", (H, K))
    assert param_specs(cfgs(lstm_hidden=7))[0] == ("output_fc_w", (21, 7))
    assert param_specs(cfgs(vlad_clusters=64, lstm_hidden=256))[4][1] == (64, 256)


def test_initialisation_decay_trust_ratio_classes_and_tier():
    """Kernel and centers glorot-uniform, the bias zero; kernel and centers are decayed and trust-scaled, the bias is neither; all three
    carry lr_mult and train under train_from: classifier; the exchange chunks cover them."""
    from vltf_amd.engine import decay_ranges, finetune_plan, init_params, lamb_ranges, lars_ranges, param_specs
    from vltf_amd.graph import init_params_for
    cfg = cfgs(lr_mult=10.0, train_from="classifier", vlad_clusters=33)
    specs = param_specs(cfg)
    offs, off = {}, 0
    for n, s in specs:
        offs[n] = (off, off + int(np.prod(s)))
        off += int(np.prod(s))
    kn, bn, cn = R.param_names()
    for p in (init_params(cfg, seed=1), init_params_for(specs, seed=1)):
        assert p[kn].shape == (8, 33) and p[bn].shape == (33,) and p[cn].shape == (33, 8)
        assert not p[bn].any()
        for n in (kn, cn):
            lim = np.sqrt(6.0 / sum(p[n].shape))
            assert p[n].std() > 0.4 * lim and np.abs(p[n]).max() <= lim            # uniform on [-lim, lim]: std lim / sqrt(3)
    plan = finetune_plan(cfg)
    assert plan.frozen and all(n.startswith("dcnn/") for n in plan.frozen)
    inside = lambda rng, lo, hi: any(a <= lo and hi <= b for a, b in rng)
    for n in (kn, bn, cn):
        lo, hi = offs[n]
        assert [m for a, b, m in plan.tiers if a <= lo and hi <= b] == [10.0], n               # the head's tier
        assert inside([(o, o + c) for o, c in plan.chunks], lo, hi), n
    ranges = decay_ranges(specs, plan, 5e-4)
    decayed, plain = [(a, b) for a, b, c in ranges if c > 0], [(a, b) for a, b, c in ranges if c == 0]
    lars, _, _ = lars_ranges(specs, plan, 0.0)
    lamb, _ = lamb_ranges(specs, plan, 0.0)
    for n in (kn, cn):
        lo, hi = offs[n]
        assert inside(decayed, lo, hi) and (lo, hi) in [(a, b) for a, b, _, t in lars if t >= 0] and (lo, hi) in [(r[0], r[1]) for r in lamb if r[4] >= 0]
    lo, hi = offs[bn]
    assert inside(plain, lo, hi) and not inside(decayed, lo, hi)
    assert inside([(a, b) for a, b, _, t in lars if t < 0], lo, hi) and inside([(r[0], r[1]) for r in lamb if r[4] < 0], lo, hi)
    plan = finetune_plan(cfgs())
    assert plan.tiers == [(0, plan.total, 1.0)] and not plan.frozen


def test_engine_specs_and_refusals():
    from vltf_amd._ffi import VltfError
    from vltf_amd.composed import ComposedEngine, HeadConfig
    from vltf_amd.engine import NetConfig, check_vlad, param_specs
    from vltf_amd.graph import DatasetInfo, PipelineSpec, model_specs
    H, C, dim, T, K = 6, 5, 10, 4, 3
    ds = {"main": DatasetInfo("vectors", T, 1, 3, dim=dim), "aux": DatasetInfo("vectors", 1, 1, 3, dim=7)}
    spec = lambda **kw: PipelineSpec("p", ["main"], "nop", classifier="lstm", **kw)
    got = model_specs([spec(lstm_params=(H, 2, "vlad"), vlad_clusters=K)], ds, C)
    want = [("output_fc_w", (K * H, C)), ("output_fc_b", (C,))] + vlad(H, K)
    rest = []
    for l, d in ((1, H), (0, dim)):
        pre = "rnn/multi_rnn_cell/cell_%d/basic_lstm_cell/" % l
        rest += [(pre + "kernel", (d + H, 4 * H)), (pre + "bias", (4 * H,))]
    assert got == want + rest
    assert model_specs([spec(lstm_params=(H, 1, "vlad"), lstm_bidirectional=True)], ds, C)[:3] == \
        [("output_fc_w", (16 * H, C)), ("output_fc_b", (C,)), ("netvlad/kernel", (2 * H, 8))]
    assert model_specs([spec(lstm_params=(H, 1, "vlad"), rnn_cell="gru")], ds, C)[4] == ("netvlad/centers", (8, H))
    two = [PipelineSpec("a", ["main"], "nop"), PipelineSpec("b", ["a"], "nop", classifier="lstm", lstm_params=(H, 1, "vlad"), vlad_clusters=K)]
    assert ("b/netvlad/centers", (K, H)) in model_specs(two, ds, C)                              # scoped like every other variable
    assert PipelineSpec("p", ["main"]).vlad_clusters is None and NetConfig().vlad_clusters is None
    # without the fusion: the list of before
    assert model_specs([spec(lstm_params=(H, 2, "avg"))], ds, C) == [("output_fc_w", (H, C)), ("output_fc_b", (C,))] + rest
    bad = lambda **kw: PipelineSpec("p", kw.pop("input", ["main"]), "nop", **kw)
    for match, pipe in (("vlad_clusters", bad(classifier="lstm", lstm_params=(H, 1, "avg"), vlad_clusters=4)),
                        ("vlad_clusters", bad(classifier="lstm", lstm_params=(H, 1, "vlad"), vlad_clusters=1)),
                        ("vlad_clusters", bad(classifier="lstm", lstm_params=(H, 1, "vlad"), vlad_clusters=65)),
                        ("vlad_clusters", bad(classifier="lstm", lstm_params=(H, 1, "vlad"), vlad_clusters=2.5)),
                        ("vlad_clusters", bad(classifier="lstm", lstm_params=(H, 1, "vlad"), vlad_clusters=True)),
                        ("16384", bad(classifier="lstm", lstm_params=(512, 1, "vlad"), vlad_clusters=33)),
                        ("classifier lstm", bad(classifier="fc", vlad_clusters=4)),
                        ("classifier lstm", bad(vlad_clusters=4)),
                        ("frame_fusion", bad(classifier="fc", frame_fusion=("early", "vlad"))),
                        ("frame_fusion", bad(classifier="fc", frame_fusion=("late", "vlad"))),
                        ("input_fusion", bad(input=["main", "main"], classifier="fc", input_fusion="vlad"))):
        with pytest.raises(VltfError, match=match):
            model_specs([pipe], ds, C)
    # LRCNEngine's configuration
    for match, kw in (("vlad_clusters", dict(fusion="avg")), ("vlad_clusters", dict(vlad_clusters=1)), ("vlad_clusters", dict(vlad_clusters=65)),
                      ("vlad_clusters", dict(vlad_clusters="many")), ("vlad_clusters", dict(vlad_clusters=2.0)),
                      ("16384", dict(vlad_clusters=64, lstm_hidden=257)), ("16384", dict(vlad_clusters=33, lstm_hidden=256, lstm_bidirectional=True)),
                      ("lstm_params", dict(classifier="fc", vlad_clusters=None)),
                      ("lstm_params", dict(classifier="none", vlad_clusters=None)), ("vlad_clusters", dict(classifier="fc", fusion="avg")),
                      ("frame_fusion", dict(classifier="fc", fusion="avg", vlad_clusters=None, frame_fusion=("early", "vlad"))),
                      ("frame_fusion", dict(classifier="fc", fusion="avg", vlad_clusters=None, frame_fusion=("late", "vlad")))):
        with pytest.raises(VltfError, match=match):
            param_specs(cfgs(**kw))
    assert check_vlad("avg") is None and check_vlad("vlad", None, "lstm", 12) == 8 and check_vlad("vlad", 64, "lstm", 256) == 64
    assert check_vlad("vlad", 2) == 2 and check_vlad("vlad", 16, "lstm", 1024) == 16
    # the two-pipeline model keeps its four fusions
    for enc, head in ((cfgs(), HeadConfig(in_dim=4, fpc=3, num_classes=7)),
                      (cfgs(fusion="avg", vlad_clusters=None), HeadConfig(in_dim=4, fpc=3, num_classes=7, fusion="vlad"))):
        with pytest.raises(VltfError, match="not built for the two-pipeline model"):
            ComposedEngine(enc, head, 2, device="cpu")


VLAD = [8, 1, "defs.fusion_method.vlad"]


def test_the_yaml_keys(tmp_path):
    from vltf_amd import run_task
    folder = str(tmp_path)
    data_path, _, _ = make_dataset(folder, "train.txt")
    s, feeder = settings_for(folder, data_path, lambda p, r: p.update(lstm_params=VLAD, vlad_clusters=5), "vlad.yml")
    assert s.pipelines["lrcn"].lstm_params == [8, 1, "vlad"] and s.pipelines["lrcn"].vlad_clusters == 5
    cfg, _ = run_task.net_config(s, feeder.get_dataset_by_tag("main")[0])
    assert (cfg.fusion, cfg.vlad_clusters, cfg.classifier) == ("vlad", 5, "lstm")
    specs, _, _ = run_task.graph_config(s, feeder, 2)
    assert specs[0].lstm_params[2] == "vlad" and specs[0].vlad_clusters == 5
    # the default is 8
    for extra in (dict(), dict(lstm_bidirectional=True), dict(rnn_cell="gru", vlad_clusters="None")):
        s, feeder = settings_for(folder, data_path, lambda p, r: p.update(lstm_params=VLAD, **extra), "default.yml")
        assert s.pipelines["lrcn"].vlad_clusters == 8
        assert run_task.net_config(s, feeder.get_dataset_by_tag("main")[0])[0].vlad_clusters == 8
    # without the fusion: no count, today's configuration
    s, feeder = settings_for(folder, data_path, lambda p, r: None, "plain.yml")
    assert s.pipelines["lrcn"].vlad_clusters is None
    cfg, _ = run_task.net_config(s, feeder.get_dataset_by_tag("main")[0])
    assert (cfg.fusion, cfg.vlad_clusters) == ("avg", None) and run_task.graph_config(s, feeder, 2)[0][0].vlad_clusters is None
    fc = lambda p: p.update(classifier="defs.classifier.fc", lstm_params=None)
    for match, edit in (("vlad_clusters", lambda p, r: p.update(vlad_clusters=5)),                                             # without the fusion
                        ("vlad_clusters", lambda p, r: p.update(lstm_params=VLAD, vlad_clusters=1)),
                        ("vlad_clusters", lambda p, r: p.update(lstm_params=VLAD, vlad_clusters=65)),
                        ("vlad_clusters", lambda p, r: p.update(lstm_params=VLAD, vlad_clusters=2.5)),
                        ("vlad_clusters", lambda p, r: p.update(lstm_params=VLAD, vlad_clusters="many")),
                        ("16384", lambda p, r: p.update(lstm_params=[512, 1, "defs.fusion_method.vlad"], vlad_clusters=64)),
                        ("vlad_clusters", lambda p, r: (fc(p), p.update(vlad_clusters=5))),                                     # classifier fc
                        ("vlad_clusters", lambda p, r: (p.pop("classifier"), p.pop("lstm_params"), p.update(vlad_clusters=5))), # no classifier
                        ("frame_fusion", lambda p, r: (fc(p), p.update(frame_fusion=["defs.fusion_type.early", "defs.fusion_method.vlad"]))),
                        ("frame_fusion", lambda p, r: (fc(p), p.update(frame_fusion=["defs.fusion_type.late", "defs.fusion_method.vlad"]))),
                        ("input_fusion", lambda p, r: p.update(input_fusion="defs.fusion_method.vlad"))):
        with pytest.raises(Exception, match=match):
            settings_for(folder, data_path, edit, "bad.yml")
    with pytest.raises(Exception, match="clip_fusion"):
        settings_for(folder, data_path, lambda p, r: r["val"].update(clip_fusion=["defs.fusion_type.late", "defs.fusion_method.vlad"]), "badval.yml",
                     phase="val")


def test_the_example_parses():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "examples", "lrcn_netvlad.yml")) as f:
        cfg = yaml.safe_load(f)
    p = cfg["run"]["network"]["pipelines"][0]["lrcn"]
    assert p["lstm_params"] == [256, 1, "defs.fusion_method.vlad"] and p["vlad_clusters"] == 8 and p["classifier"] == "defs.classifier.lstm"


def test_checkpoint_names(tmp_path):
    """A checkpoint holds the NetVLAD variables under their names, restores into a model with the fusion and is refused by one without."""
    from vltf_amd import settings_
    folder = str(tmp_path)
    data_path, _, _ = make_dataset(folder, "train.txt")
    s = settings_.Settings()
    feeder = s.initialize(config(folder, data_path))
    small = dict(image_shape=(16, 16, 3), num_classes=4)
    saved = StubEngine(cfgs(**small), seed=1)
    feeder.compute_save_interval()
    base = feeder.save(saved, "ep_1", 2)
    with np.load(base + ".weights.npz") as z:
        names = set(z.files)
        assert z["netvlad/centers"].shape == (3, 8) and z["netvlad/kernel"].shape == (8, 3) and z["output_fc_w"].shape == (24, 4)
    assert names == {n for n, _ in saved.specs} and set(R.param_names()) <= names
    s2 = settings_.Settings()
    f2 = s2.initialize(config(folder, data_path, resume_file=base))
    fresh = StubEngine(cfgs(**small), seed=2)
    f2.init_saveload(fresh, base)
    for n in saved.params:
        assert np.array_equal(fresh.params[n], saved.params[n]), n
    with pytest.raises(Exception):
        f2.init_saveload(StubEngine(cfgs(fusion="avg", vlad_clusters=None, **small), seed=2), base)
