"""Attention pooling over time (fusion `attn`) without a GPU: tests/attn_pool_ref.py against torch autograd in fp64 (the independent
oracle: y, alpha and every gradient, with and without per-clip lengths), the dead-row contract of the reference, the degenerate cases,
the float32 error of every kernel output (which decides the tolerance classes of tests/test_attn_pool_gpu.py), and the host plumbing:
variable names, shapes and order, decay / trust-ratio classes, initialisation, the learning-rate tier, the YAML keys with every refusal,
checkpoint names, and the variable lists of models WITHOUT the fusion against literal lists."""
import os

import numpy as np
import pytest
import torch
import yaml

from tests import attn_pool_ref as R
from tests import lstm_plan as P
from tests.test_host_workflow import config, make_dataset

F64 = np.float64
# output -> tolerance class of tests/test_lstm_geometry_gpu.TOL (restated: that module needs a device to import its helpers' fixtures)
TOL = dict(act=(3e-5, 3e-5), hseq=(1e-5, 1e-6))
CLASS = dict(s="act", alpha="act", y="act", dh="hseq", du="act", dcp="act")


def layer_weights(case, k):
    """W [HO][A] ~ k N(0, 1) / sqrt(HO) (so that u = h W + b ~ k N(0, 1)), b [A] ~ 0.1 N(0, 1)."""
    batch, T, HO, A = case
    r = np.random.default_rng([batch, T, HO, A, k, 1])
    return r.standard_normal((HO, A)) * k / np.sqrt(HO), r.standard_normal(A) * 0.1


# ---- the reference against torch autograd ------------------------------------------------------------------------------------------
def torch_layer(x, W, b, c, T, L):
    """The layer written a second time, clip by clip, in torch: softmax over the first L[i] steps of clip i."""
    ys, alphas = [], []
    for i, l in enumerate(L):
        hi = x[i * T:i * T + int(l)]
        e = torch.tanh(hi @ W + b) @ c.reshape(-1)
        a = torch.softmax(e, dim=0)
        ys.append(a @ hi)
        alphas.append(torch.cat([a, torch.zeros(T - int(l), dtype=a.dtype)]))
    return torch.stack(ys), torch.stack(alphas)


@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_the_reference_is_torch_autograd_in_fp64(case, lens):
    """y, alpha, dx, dW, db and dc to 1e-12."""
    batch, T, HO, A = case
    inp = R.inputs(batch, T, HO, A, 1)
    W, b = layer_weights(case, 1)
    c = np.asarray(inp.c, F64).reshape(A, 1)
    L = P.lengths(batch, T) if lens else None
    y, cache = R.pool_layer_forward(inp.h, W, b, c, T, L)
    dx, dW, db, dc = R.pool_layer_backward(inp.dy, cache)
    assert dc.shape == (A, 1)
    tx, tW, tb, tc = (torch.tensor(np.asarray(a, F64), requires_grad=True) for a in (inp.h, W, b, c))
    ty, talpha = torch_layer(tx, tW, tb, tc, T, R.fusion_lens(L, batch, T))
    ty.backward(torch.tensor(np.asarray(inp.dy, F64)))
    tol = dict(rtol=0, atol=1e-12)
    np.testing.assert_allclose(y, ty.detach().numpy(), **tol)
    np.testing.assert_allclose(cache.fwd.alpha, talpha.detach().numpy(), **tol)
    for ours, theirs, name in ((dx, tx, "dx"), (dW, tW, "dW"), (db, tb, "db"), (dc, tc, "dc")):
        np.testing.assert_allclose(ours, theirs.grad.numpy(), err_msg=name, **tol)


def test_the_lengths_exercise_the_clamp():
    """lstm_plan.lengths holds a 0, a T, a -3 and a T + 5; the fusion's rule makes them 1, T, 1 and T."""
    lens = P.lengths(5, 16)
    assert list(lens[:3]) == [0, 16, -3] and lens[-1] == 21
    assert list(R.fusion_lens(lens, 5, 16)[[0, 1, 2, 4]]) == [1, 16, 1, 16]
    assert list(R.fusion_lens(None, 2, 7)) == [7, 7]


# ---- dead rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in R.CASES if c[0] > 1], ids=R.case_id)
def test_dead_rows_are_inert(case):
    """NaN in the dead rows of h, u and s changes nothing, and the gradients of the dead rows are zero."""
    batch, T, HO, A = case
    ref = R.reference(case, 1, True)
    dead = ~R.live_mask(ref.lens, batch, T).reshape(-1)
    assert dead.any() and not dead.all()
    nan = lambda a: R.with_nan_in_dead_rows(a, T, ref.lens)
    fwd = R.forward(nan(ref.inp.h), nan(ref.inp.u), ref.inp.c, ref.lens, T)
    bwd = R.backward(ref.inp.dy, nan(ref.inp.h), nan(ref.s32), ref.alpha32, ref.inp.c, ref.lens, T)
    for a, b in zip(fwd + bwd, ref.fwd + ref.bwd):
        assert np.isfinite(a).all() and np.array_equal(a, b)
    assert not fwd.s[dead].any() and not fwd.alpha.reshape(-1)[dead].any() and not bwd.du[dead].any() and not bwd.dh[dead].any()
    assert bwd.du[~dead].any() and bwd.dh[~dead].any()
    np.testing.assert_allclose(fwd.alpha.sum(axis=1), 1.0, rtol=0, atol=1e-14)
    # the layer: a NaN row of x gives no NaN anywhere and a zero row of dx
    W, b = layer_weights(case, 1)
    y, cache = R.pool_layer_forward(nan(ref.inp.h), W, b, ref.inp.c, T, ref.lens)
    dx, dW, db, dc = R.pool_layer_backward(ref.inp.dy, cache)
    assert all(np.isfinite(a).all() for a in (y, dx, dW, db, dc)) and not dx[dead].any()


# ---- degenerate cases --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
def test_a_zero_context_is_the_avg_fusion(lens):
    from tests import gru_ref
    case = batch, T, HO, A = (4, 7, 96, 130)
    inp = R.inputs(*case)
    L = P.lengths(batch, T) if lens else None
    fwd = R.forward(inp.h, inp.u, np.zeros(A), L, T)
    Lc = R.fusion_lens(L, batch, T)
    want_alpha = R.live_mask(L, batch, T) / Lc[:, None]
    np.testing.assert_allclose(fwd.alpha, want_alpha, rtol=0, atol=1e-15)
    # the reference's avg fusion over the same live steps (gru_ref.fuse clamps to 0..T: hand it the fusion's lengths)
    np.testing.assert_allclose(fwd.y, gru_ref.fuse(inp.h, T, HO, "avg", None if L is None else Lc), rtol=0, atol=1e-14)


def test_one_step_gives_weight_one_and_no_score_gradient():
    case = batch, T, HO, A = (3, 1, 37, 5)
    inp = R.inputs(*case)
    fwd = R.forward(inp.h, inp.u, inp.c, None, T)
    bwd = R.backward(inp.dy, inp.h, fwd.s, fwd.alpha, inp.c, None, T)
    assert (fwd.alpha == 1.0).all() and np.array_equal(fwd.y, np.asarray(inp.h, F64))
    assert not bwd.du.any() and not bwd.dcp.any() and np.array_equal(bwd.dh, np.asarray(inp.dy, F64))


def test_scores_of_two_hundred_stay_finite():
    case = batch, T, HO, A = (2, 21, 250, 64)
    inp = R.inputs(*case)
    u = np.where(np.arange(batch * T)[:, None] % T % 2 == 0, 50.0, -50.0) * np.ones((1, A))  # s = +-1 exactly in fp64, + at even steps
    c = np.full(A, 200.0 / A)                                                               # e = +-200
    fwd = R.forward(inp.h, u, c, None, T)
    bwd = R.backward(inp.dy, inp.h, fwd.s, fwd.alpha, c, None, T)
    assert all(np.isfinite(a).all() for a in fwd + bwd)
    np.testing.assert_allclose(fwd.alpha.sum(axis=1), 1.0, rtol=0, atol=1e-14)
    assert fwd.alpha[:, 1::2].max() < 1e-170 and abs(fwd.alpha[:, ::2] - 1.0 / 11).max() < 1e-15


# ---- tolerance classes -------------------------------------------------------------------------------------------------------------
def forward32(h, u, c, L, T):
    """The forward in plain float32 numpy."""
    f = np.float32
    A = c.shape[0]
    b = u.shape[0] // T
    s = np.zeros((b, T, A), f)
    alpha = np.zeros((b, T), f)
    y = np.zeros((b, h.shape[1]), f)
    for i, l in enumerate(L):
        hi, ui = h[i * T:i * T + l], u[i * T:i * T + l]
        si = np.tanh(ui)
        e = si @ c
        w = np.exp(e - e.max())
        a = w / w.sum(dtype=f)
        s[i, :l], alpha[i, :l], y[i] = si, a, a @ hi
        assert si.dtype == e.dtype == a.dtype == f
    return R.Forward(s.reshape(b * T, A), alpha, y)


def backward32(dy, h, s, alpha, c, L, T):
    """The backward in plain float32 numpy, from s and alpha as given."""
    f = np.float32
    A = c.shape[0]
    b = dy.shape[0]
    du, dh, dcp = np.zeros((b * T, A), f), np.zeros((b * T, h.shape[1]), f), np.zeros((b, A), f)
    for i, l in enumerate(L):
        rows = slice(i * T, i * T + l)
        hi, si, a = h[rows], s[rows], alpha[i, :l]
        da = hi @ dy[i]
        de = a * (da - a @ da)
        du[rows] = de[:, None] * c[None, :] * (f(1) - si * si)
        dh[rows] = a[:, None] * dy[i][None, :]
        dcp[i] = de @ si
        assert du.dtype == dh.dtype == dcp.dtype == f and de.dtype == f
    return R.Backward(du, dh, dcp)


def test_float32_stays_inside_half_of_the_tolerance_classes():
    """Decides the classes of tests/test_attn_pool_gpu.py: a plain float32 numpy evaluation of both launches (the backward from the
    reference's s and alpha rounded to fp32) against fp64 stays at or below 0.5 of the class's bound -- atol_rel * max|want| + rtol *
    |want| -- at every case, both scales and both length variants.  s, alpha and y sit behind a tanhf like the LSTM's gates: act.  dh is
    one product: hseq.  du and dcp, products and sums of rounded factors, take act, the wider class: an evaluation that accumulates in a
    less favourable order than numpy's loses more than this one does.  Measured with this evaluation, worst error / bound: s 0.001,
    alpha 0.009, y 0.011, dh 0.005, du 0.009, dcp 0.008 (printed below)."""
    worst = {k: 0.0 for k in CLASS}
    for case in R.CASES:
        batch, T, HO, A = case
        for k in R.SCALES:
            for lens in (False, True):
                ref = R.reference(case, k, lens)
                L = [int(v) for v in R.fusion_lens(ref.lens, batch, T)]
                inp = ref.inp
                got = forward32(inp.h, inp.u, inp.c, L, T)._asdict()
                got.update(backward32(inp.dy, inp.h, ref.s32, ref.alpha32, inp.c, L, T)._asdict())
                want = dict(ref.fwd._asdict(), **ref.bwd._asdict())
                for name, g in got.items():
                    assert g.dtype == np.float32
                    rtol, atol_rel = TOL[CLASS[name]]
                    w = np.asarray(want[name], F64)
                    bound = atol_rel * (float(np.abs(w).max()) or 1.0) + rtol * np.abs(w)
                    ratio = float((np.abs(g.astype(F64) - w) / bound).max())
                    worst[name] = max(worst[name], ratio)
                    assert ratio <= 0.5, "%s at case %s, k = %d, lens = %s: error / bound %.3f" % (name, case, k, lens, ratio)
    print("attention pooling in float32, worst error / bound:", " ".join("%s %.3f" % kv for kv in sorted(worst.items())))


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
    base = dict(image_shape=(67, 67, 3), num_classes=7, fpc=3, lstm_hidden=8, lstm_layers=1, fusion="attn", attn_dim=5)
    base.update(kw)
    return NetConfig(**base)


TOWER = [("dcnn/fc6W", (256, 4096)), ("dcnn/fc6b", (4096,)), ("dcnn/conv5W", (3, 3, 192, 256)), ("dcnn/conv5b", (256,)),
         ("dcnn/conv4W", (3, 3, 192, 384)), ("dcnn/conv4b", (384,)), ("dcnn/conv3W", (3, 3, 256, 384)), ("dcnn/conv3b", (384,)),
         ("dcnn/conv2W", (5, 5, 48, 256)), ("dcnn/conv2b", (256,)), ("dcnn/conv1W", (11, 11, 3, 96)), ("dcnn/conv1b", (96,))]
LSTM0 = "rnn/multi_rnn_cell/cell_0/basic_lstm_cell/"
BI = "bidirectional_rnn/%s/multi_rnn_cell/cell_0/basic_lstm_cell/"
GRU = "rnn/multi_rnn_cell/cell_%d/gru_cell/"
# the variable lists of three models WITHOUT the fusion, as they were before it existed
PLAIN = {
    "lstm": (dict(), [("output_fc_w", (8, 7)), ("output_fc_b", (7,)), (LSTM0 + "kernel", (4104, 32)), (LSTM0 + "bias", (32,))]),
    "blstm": (dict(lstm_bidirectional=True),
              [("output_fc_w", (16, 7)), ("output_fc_b", (7,)), (BI % "fw" + "kernel", (4104, 32)), (BI % "fw" + "bias", (32,)),
               (BI % "bw" + "kernel", (4104, 32)), (BI % "bw" + "bias", (32,))]),
    "gru": (dict(rnn_cell="gru", lstm_layers=2),
            [("output_fc_w", (8, 7)), ("output_fc_b", (7,)), (GRU % 0 + "kernel", (4096, 24)), (GRU % 0 + "recurrent_kernel", (8, 24)),
             (GRU % 0 + "bias", (24,)), (GRU % 0 + "recurrent_bias", (24,)), (GRU % 1 + "kernel", (8, 24)),
             (GRU % 1 + "recurrent_kernel", (8, 24)), (GRU % 1 + "bias", (24,)), (GRU % 1 + "recurrent_bias", (24,))]),
}


@pytest.mark.parametrize("cell", sorted(PLAIN))
def test_a_model_without_the_fusion_has_the_variables_it_had(cell):
    """param_specs, the flat-buffer plan and the exchange chunks of an LSTM, a bidirectional and a GRU model with fusion avg: literal."""
    from vltf_amd.engine import NetConfig, finetune_plan, param_specs
    kw, head = PLAIN[cell]
    cfg = NetConfig(image_shape=(67, 67, 3), num_classes=7, fpc=3, lstm_hidden=8, **kw)
    assert cfg.attn_dim is None and cfg.fusion == "avg"
    specs = param_specs(cfg)
    assert specs == head + TOWER
    plan = finetune_plan(cfg)
    total, first = {"lstm": (3518175, 131423), "blstm": (3649591, 262839), "gru": (3485791, 99039)}[cell]
    assert plan.tiers == [(0, total, 1.0)] and plan.total == total == sum(int(np.prod(s)) for _, s in specs)
    tail = [(524288, 528384), (528384, 1991680), (1991680, 342400)]
    assert plan.chunks == [(0, first), (first, 524288)] + [(first + sum(c for c, _ in tail[:i + 1]), n) for i, (_, n) in enumerate(tail)]


def test_param_specs_names_shapes_and_order():
    from vltf_amd.engine import attn_names, param_specs
    H, A, C = 8, 5, 7
    attn = [("attention_pool/kernel", (H, A)), ("attention_pool/bias", (A,)), ("attention_pool/context", (A, 1))]
    assert [n for n, _ in attn] == attn_names() == R.param_names()
    # between the head and the recurrent layers, for every cell
    for cell, (kw, plain) in PLAIN.items():
        HO = 16 if cell == "blstm" else 8
        want = plain[:2] + [("attention_pool/kernel", (HO, A)), ("attention_pool/bias", (A,)), ("attention_pool/context", (A, 1))] + plain[2:]
        assert param_specs(cfgs(**kw)) == want + TOWER, cell
    assert param_specs(cfgs(attn_dim=None))[2:5] == [("attention_pool/kernel", (H, H)), ("attention_pool/bias", (H,)), ("attention_pool/context", (H, 1))]
    assert param_specs(cfgs(attn_dim=None, lstm_bidirectional=True))[2][1] == (16, 16)          # the default is the output width
    assert param_specs(cfgs(lstm_hidden=7))[0] == ("attention_pool/kernel", (7, A))            # H == C: no head
    assert param_specs(cfgs(attn_dim=1024))[4][1] == (1024, 1)


def test_initialisation_decay_trust_ratio_classes_and_tier():
    """Kernel and context glorot-uniform, the bias zero; kernel and context are decayed and trust-scaled, the bias is neither; all
    three carry lr_mult and train under train_from: classifier; the exchange chunks cover them."""
    from vltf_amd.engine import decay_ranges, finetune_plan, init_params, lamb_ranges, lars_ranges, param_specs
    from vltf_amd.graph import init_params_for
    cfg = cfgs(lr_mult=10.0, train_from="classifier", attn_dim=130)
    specs = param_specs(cfg)
    offs, off = {}, 0
    for n, s in specs:
        offs[n] = (off, off + int(np.prod(s)))
        off += int(np.prod(s))
    kn, bn, cn = R.param_names()
    for p in (init_params(cfg, seed=1), init_params_for(specs, seed=1)):
        assert p[kn].shape == (8, 130) and p[bn].shape == (130,) and p[cn].shape == (130, 1)
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
    # without lr_mult / train_from: one tier over everything, as for every other model
    plan = finetune_plan(cfgs())
    assert plan.tiers == [(0, plan.total, 1.0)] and not plan.frozen


def test_engine_specs_and_refusals():
    from vltf_amd._ffi import VltfError
    from vltf_amd.composed import ComposedEngine, HeadConfig
    from vltf_amd.engine import NetConfig, check_attn, param_specs
    from vltf_amd.graph import DatasetInfo, PipelineSpec, model_specs
    H, C, dim, T, A = 6, 5, 10, 4, 3
    ds = {"main": DatasetInfo("vectors", T, 1, 3, dim=dim), "aux": DatasetInfo("vectors", 1, 1, 3, dim=7)}
    spec = lambda **kw: PipelineSpec("p", ["main"], "nop", classifier="lstm", **kw)
    got = model_specs([spec(lstm_params=(H, 2, "attn"), attn_dim=A)], ds, C)
    want = [("output_fc_w", (H, C)), ("output_fc_b", (C,)), ("attention_pool/kernel", (H, A)), ("attention_pool/bias", (A,)),
            ("attention_pool/context", (A, 1))]
    for l, d in ((1, H), (0, dim)):
        pre = "rnn/multi_rnn_cell/cell_%d/basic_lstm_cell/" % l
        want += [(pre + "kernel", (d + H, 4 * H)), (pre + "bias", (4 * H,))]
    assert got == want
    assert model_specs([spec(lstm_params=(H, 1, "attn"), lstm_bidirectional=True)], ds, C)[2] == ("attention_pool/kernel", (2 * H, 2 * H))
    assert model_specs([spec(lstm_params=(H, 1, "attn"), rnn_cell="gru")], ds, C)[4] == ("attention_pool/context", (H, 1))
    two = [PipelineSpec("a", ["main"], "nop"), PipelineSpec("b", ["a"], "nop", classifier="lstm", lstm_params=(H, 1, "attn"), attn_dim=A)]
    assert ("b/attention_pool/context", (A, 1)) in model_specs(two, ds, C)                       # scoped like every other variable
    assert PipelineSpec("p", ["main"]).attn_dim is None and NetConfig().attn_dim is None
    # without the fusion: the list of before
    assert model_specs([spec(lstm_params=(H, 2, "avg"))], ds, C) == want[:2] + want[5:]
    bad = lambda **kw: PipelineSpec("p", kw.pop("input", ["main"]), "nop", **kw)
    for match, pipe in (("attn_dim", bad(classifier="lstm", lstm_params=(H, 1, "avg"), attn_dim=4)),
                        ("attn_dim", bad(classifier="lstm", lstm_params=(H, 1, "attn"), attn_dim=0)),
                        ("attn_dim", bad(classifier="lstm", lstm_params=(H, 1, "attn"), attn_dim=1025)),
                        ("attn_dim", bad(classifier="lstm", lstm_params=(H, 1, "attn"), attn_dim=2.5)),
                        ("attn_dim", bad(classifier="lstm", lstm_params=(H, 1, "attn"), attn_dim=True)),
                        ("classifier lstm", bad(classifier="fc", attn_dim=4)),
                        ("classifier lstm", bad(attn_dim=4)),
                        ("frame_fusion", bad(classifier="fc", frame_fusion=("early", "attn"))),
                        ("frame_fusion", bad(classifier="fc", frame_fusion=("late", "attn"))),
                        ("input_fusion", bad(input=["main", "main"], classifier="fc", input_fusion="attn"))):
        with pytest.raises(VltfError, match=match):
            model_specs([pipe], ds, C)
    # LRCNEngine's configuration
    for match, kw in (("attn_dim", dict(fusion="avg")), ("attn_dim", dict(attn_dim=0)), ("attn_dim", dict(attn_dim=1025)),
                      ("attn_dim", dict(attn_dim="wide")), ("lstm_params", dict(classifier="fc", attn_dim=None)),
                      ("lstm_params", dict(classifier="none", attn_dim=None)), ("attn_dim", dict(classifier="fc", fusion="avg")),
                      ("frame_fusion", dict(classifier="fc", fusion="avg", attn_dim=None, frame_fusion=("early", "attn"))),
                      ("frame_fusion", dict(classifier="fc", fusion="avg", attn_dim=None, frame_fusion=("late", "attn")))):
        with pytest.raises(VltfError, match=match):
            param_specs(cfgs(**kw))
    assert check_attn("avg") is None and check_attn("attn", None, "lstm", 12) == 12 and check_attn("attn", 1024) == 1024
    # the two-pipeline model keeps its four fusions
    for enc, head in ((cfgs(), HeadConfig(in_dim=4, fpc=3, num_classes=7)),
                      (cfgs(fusion="avg", attn_dim=None), HeadConfig(in_dim=4, fpc=3, num_classes=7, fusion="attn"))):
        with pytest.raises(VltfError, match="not built for the two-pipeline model"):
            ComposedEngine(enc, head, 2, device="cpu")


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


ATTN = [8, 1, "defs.fusion_method.attn"]


def test_the_yaml_keys(tmp_path):
    from vltf_amd import run_task
    folder = str(tmp_path)
    data_path, _, _ = make_dataset(folder, "train.txt")
    s, feeder = settings_for(folder, data_path, lambda p, r: p.update(lstm_params=ATTN, attn_dim=5), "attn.yml")
    assert s.pipelines["lrcn"].lstm_params == [8, 1, "attn"] and s.pipelines["lrcn"].attn_dim == 5
    cfg, _ = run_task.net_config(s, feeder.get_dataset_by_tag("main")[0])
    assert (cfg.fusion, cfg.attn_dim, cfg.classifier) == ("attn", 5, "lstm")
    specs, _, _ = run_task.graph_config(s, feeder, 2)
    assert specs[0].lstm_params[2] == "attn" and specs[0].attn_dim == 5
    # the default is the recurrent output width
    for extra, width in ((dict(), 8), (dict(lstm_bidirectional=True), 16), (dict(rnn_cell="gru", attn_dim="None"), 8)):
        s, feeder = settings_for(folder, data_path, lambda p, r: p.update(lstm_params=ATTN, **extra), "default.yml")
        assert s.pipelines["lrcn"].attn_dim == width
        assert run_task.net_config(s, feeder.get_dataset_by_tag("main")[0])[0].attn_dim == width
    # without the fusion: no width, today's configuration
    s, feeder = settings_for(folder, data_path, lambda p, r: None, "plain.yml")
    assert s.pipelines["lrcn"].attn_dim is None
    cfg, _ = run_task.net_config(s, feeder.get_dataset_by_tag("main")[0])
    assert (cfg.fusion, cfg.attn_dim) == ("avg", None) and run_task.graph_config(s, feeder, 2)[0][0].attn_dim is None
    fc = lambda p: p.update(classifier="defs.classifier.fc", lstm_params=None)
    for match, edit in (("attn_dim", lambda p, r: p.update(attn_dim=5)),                                                      # without the fusion
                        ("attn_dim", lambda p, r: p.update(lstm_params=ATTN, attn_dim=0)),
                        ("attn_dim", lambda p, r: p.update(lstm_params=ATTN, attn_dim=1025)),
                        ("attn_dim", lambda p, r: p.update(lstm_params=ATTN, attn_dim=2.5)),
                        ("attn_dim", lambda p, r: p.update(lstm_params=ATTN, attn_dim="wide")),
                        ("attn_dim", lambda p, r: (fc(p), p.update(attn_dim=5))),                                              # classifier fc
                        ("attn_dim", lambda p, r: (p.pop("classifier"), p.pop("lstm_params"), p.update(attn_dim=5))),          # no classifier
                        ("frame_fusion", lambda p, r: (fc(p), p.update(frame_fusion=["defs.fusion_type.early", "defs.fusion_method.attn"]))),
                        ("frame_fusion", lambda p, r: (fc(p), p.update(frame_fusion=["defs.fusion_type.late", "defs.fusion_method.attn"]))),
                        ("input_fusion", lambda p, r: p.update(input_fusion="defs.fusion_method.attn"))):
        with pytest.raises(Exception, match=match):
            settings_for(folder, data_path, edit, "bad.yml")
    with pytest.raises(Exception, match="clip_fusion"):
        settings_for(folder, data_path, lambda p, r: r["val"].update(clip_fusion=["defs.fusion_type.late", "defs.fusion_method.attn"]), "badval.yml",
                     phase="val")


def test_the_example_parses():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "examples", "lrcn_attn.yml")) as f:
        cfg = yaml.safe_load(f)
    p = cfg["run"]["network"]["pipelines"][0]["lrcn"]
    assert p["lstm_params"] == [256, 1, "defs.fusion_method.attn"] and p["attn_dim"] == 128 and p["classifier"] == "defs.classifier.lstm"


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
    """A checkpoint holds the attention variables under their names, restores into a model with the fusion and is refused by one without."""
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
        assert z["attention_pool/context"].shape == (5, 1) and z["attention_pool/kernel"].shape == (8, 5)
    assert names == {n for n, _ in saved.specs} and set(R.param_names()) <= names
    s2 = settings_.Settings()
    f2 = s2.initialize(config(folder, data_path, resume_file=base))
    fresh = StubEngine(cfgs(**small), seed=2)
    f2.init_saveload(fresh, base)
    for n in saved.params:
        assert np.array_equal(fresh.params[n], saved.params[n]), n
    with pytest.raises(Exception):
        f2.init_saveload(StubEngine(cfgs(fusion="avg", attn_dim=None, **small), seed=2), base)
