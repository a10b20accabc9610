"""Dilated temporal convolutions over time (rnn_cell `tcn`) without a GPU: tests/tcn_ref.py against torch autograd in fp64 (the
independent oracle: torch.nn.functional.conv1d with dilation over each clip's live prefix), the reference's contract, and the host
plumbing: variable names, shapes and order, decay / trust-ratio classes, initialisation, the learning-rate tier, the YAML keys with
every refusal, the example."""
import os

import numpy as np
import pytest
import torch
import yaml

from tests import lstm_plan as LP
from tests import tcn_ref as R
from tests.test_host_workflow import config, make_dataset

F64 = np.float64


# ---- the reference against torch autograd ------------------------------------------------------------------------------------------
def torch_layer(x, W1, b1, W2, b2, T, dilation, causal, L):
    """The layer written a second time in torch: per clip, conv1d with dilation over the live prefix, zero-padded (k - 1) d / 2 on each
    side or (k - 1) d on the left; dead rows are zeros."""
    b = x.shape[0] // T
    k, H = W1.shape[0], W1.shape[1]
    w = W1.permute(2, 1, 0)                                                   # (tap, in, out) -> conv1d's (out, in, tap)
    span = (k - 1) * dilation
    pad = (span, 0) if causal else (span // 2, span // 2)
    ys = []
    for c in range(b):
        n = int(L[c])
        xc = x[c * T:c * T + n]
        if n:
            u = torch.nn.functional.conv1d(torch.nn.functional.pad(xc.t()[None], pad), w, b1, dilation=dilation)[0].t()
            ys.append(xc + torch.relu(u) @ W2 + b2)
        ys.append(torch.zeros(T - n, H, dtype=x.dtype))
    return torch.cat(ys)


@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
@pytest.mark.parametrize("case", [c for c in R.CASES if c[2] <= 256], ids=R.case_id)
def test_the_reference_is_torch_autograd_in_fp64(case, lens):
    """y, dx, dW1, db1, dW2, db2 to 1e-10 (with lengths: NaN in the dead rows of x and dy)."""
    batch, T, H, k, dilation, causal = case
    r = np.random.default_rng(list(case) + [2])
    x, dy = r.standard_normal((batch * T, H)), r.standard_normal((batch * T, H))
    W1, b1 = r.standard_normal((k, H, H)) / np.sqrt(k * H), 0.1 * r.standard_normal(H)
    W2, b2 = r.standard_normal((H, H)) / np.sqrt(H), 0.1 * r.standard_normal(H)
    L = LP.lengths(batch, T) if lens else None
    nan = (lambda a: R.with_nan_in_dead_rows(a, T, L)) if lens else (lambda a: a)
    y, cache = R.layer_forward(nan(x), W1, b1, W2, b2, T, dilation, bool(causal), L)
    dx, grads = R.layer_backward(nan(dy), cache)
    tens = [torch.tensor(np.asarray(a, F64), requires_grad=True) for a in (x, W1, b1, W2, b2)]
    live = R.live_mask(L, batch, T).reshape(-1, 1)
    ty = torch_layer(*tens, T, dilation, bool(causal), R.live_lens(L, batch, T))
    ty.backward(torch.tensor(np.where(live, dy, 0.0)))
    tol = dict(rtol=0, atol=1e-10)
    np.testing.assert_allclose(y, ty.detach().numpy(), **tol)
    for ours, t, name in zip([dx] + grads, tens, ("dx", "dW1", "db1", "dW2", "db2")):
        np.testing.assert_allclose(ours, t.grad.numpy(), err_msg=name, **tol)
    assert not dx[~live.reshape(-1)].any() and not y[~live.reshape(-1)].any()


@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_the_launch_references(case, lens):
    """cols is a gather of x (every value of it is a value of x or +0.0), cols_bwd is its transpose plus dres (<dcols, cols_fwd(x)> =
    <cols_bwd(dcols), x>), the fp32 restatement is the fp64 sum to fp32 rounding, and dead rows take no part."""
    batch, T, C, taps, dilation, causal = case
    ref = R.reference(case, lens)
    geo = (ref.lens, batch, T, C, taps, dilation, causal)
    live = R.live_mask(ref.lens, batch, T).reshape(-1)
    x64 = np.where(live[:, None], ref.inp.x.astype(F64), 0.0)
    dc64 = np.where(live[:, None], ref.inp.dcols.astype(F64), 0.0)
    assert ref.cols.dtype == np.float32 and ref.dx32.dtype == np.float32
    np.testing.assert_allclose((dc64 * ref.cols).sum(), (ref.dx_nores * x64).sum(), rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(ref.dx - ref.dx_nores, np.where(live[:, None], ref.inp.dres, 0.0), rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref.dx32, ref.dx, rtol=0, atol=2e-6 * taps)
    assert not ref.cols[~live].any() and not ref.dx[~live].any()
    if lens:
        nan = lambda a: R.with_nan_in_dead_rows(a, T, ref.lens)
        assert np.array_equal(R.cols_fwd(nan(ref.inp.x), *geo), ref.cols)
        assert np.array_equal(R.cols_bwd(nan(ref.inp.dcols), nan(ref.inp.dres), *geo), ref.dx)
    j0 = taps - 1 if causal else (taps - 1) // 2
    assert np.array_equal(ref.cols.reshape(batch * T, taps, C)[live][:, j0], ref.inp.x[live])       # the zero-offset tap is the row


def test_the_stack_is_finite_differences():
    """stack_forward / stack_backward (embedding, two layers, exponential dilation, lengths) against central differences of a scalar."""
    T, d, H, layers, k = 5, 6, 8, 2, 3
    lens = np.array([5, 2, 0, 4])
    r = np.random.default_rng(4)
    p = R.init_stack(r, {}, d, H, layers, k)
    p = {n: v.astype(F64) for n, v in p.items()}
    x, dy = r.standard_normal((4 * T, d)), r.standard_normal((4 * T, H))
    live = R.live_mask(lens, 4, T).reshape(-1, 1)
    f = lambda: float((R.stack_forward(x, p, T, layers, lens=lens)[0] * np.where(live, dy, 0.0)).sum())
    out, caches = R.stack_forward(x, p, T, layers, lens=lens)
    assert R.relu_margin(caches) > 1e-3
    dx, grads = R.stack_backward(dy, caches)
    assert set(grads) == set(R.param_names(layers))
    for n in grads:
        idx = tuple(int(i) for i in np.unravel_index(int(np.abs(grads[n]).argmax()), grads[n].shape))
        keep = p[n][idx]
        p[n][idx] = keep + 1e-6
        hi = f()
        p[n][idx] = keep - 1e-6
        lo = f()
        p[n][idx] = keep
        np.testing.assert_allclose((hi - lo) / 2e-6, grads[n][idx], rtol=1e-5, err_msg=n)
    assert not dx[~live.reshape(-1)].any()


# ---- host plumbing -----------------------------------------------------------------------------------------------------------------
def cfgs(**kw):
    from vltf_amd.engine import NetConfig
    base = dict(image_shape=(67, 67, 3), num_classes=7, fpc=3, lstm_hidden=16, lstm_layers=1, fusion="avg", rnn_cell="tcn")
    base.update(kw)
    return NetConfig(**base)


TOWER = [("dcnn/fc6W", (256, 4096)), ("dcnn/fc6b", (4096,)), ("dcnn/conv5W", (3, 3, 192, 256)), ("dcnn/conv5b", (256,)),
         ("dcnn/conv4W", (3, 3, 192, 384)), ("dcnn/conv4b", (384,)), ("dcnn/conv3W", (3, 3, 256, 384)), ("dcnn/conv3b", (384,)),
         ("dcnn/conv2W", (5, 5, 48, 256)), ("dcnn/conv2b", (256,)), ("dcnn/conv1W", (11, 11, 3, 96)), ("dcnn/conv1b", (96,))]
TC = "temporal_conv/"


def embed_specs(d, H, scope=""):
    return [(scope + TC + "embed/kernel", (d, H)), (scope + TC + "embed/bias", (H,))]


def layer_specs(l, H, k, scope=""):
    pre = scope + TC + "layer_%d/" % l
    return [(pre + "conv_kernel", (k, H, H)), (pre + "conv_bias", (H,)), (pre + "out_kernel", (H, H)), (pre + "out_bias", (H,))]


def test_param_specs_names_shapes_and_order():
    """Head, (attention_pool / netvlad,) the embedding, then the layers ascending, each in the order the forward meets its variables."""
    from vltf_amd.engine import param_specs, tcn_specs, tcn_var
    H, C = 16, 7
    head = [("output_fc_w", (H, C)), ("output_fc_b", (C,))]
    assert [n for n, _ in tcn_specs(2, 5, H, 3)] == R.param_names(2) and [s for _, s in tcn_specs(2, 5, H, 3)] == R.param_shapes(2, 5, H, 3)
    assert [n for n, _ in tcn_specs(1, 5, H, 3, "p/")] == R.param_names(1, "p/")
    assert tcn_var("q/", None, "kernel") == R.var_name(None, "kernel", "q/") and tcn_var("", 3, "out_bias") == R.var_name(3, "out_bias")
    assert param_specs(cfgs()) == head + embed_specs(4096, H) + layer_specs(0, H, 3) + TOWER
    assert param_specs(cfgs(lstm_layers=2, tcn_kernel=5)) == head + embed_specs(4096, H) + layer_specs(0, H, 5) + layer_specs(1, H, 5) + TOWER
    assert param_specs(cfgs(tcn_kernel=4, tcn_causal=True, tcn_dilation="none")) == head + embed_specs(4096, H) + layer_specs(0, H, 4) + TOWER
    attn = [("attention_pool/kernel", (H, 5)), ("attention_pool/bias", (5,)), ("attention_pool/context", (5, 1))]
    assert param_specs(cfgs(fusion="attn", attn_dim=5)) == head + attn + embed_specs(4096, H) + layer_specs(0, H, 3) + TOWER
    vlad = [("netvlad/kernel", (H, 4)), ("netvlad/bias", (4,)), ("netvlad/centers", (4, H))]
    assert param_specs(cfgs(fusion="vlad", vlad_clusters=4)) == [("output_fc_w", (4 * H, C)), ("output_fc_b", (C,))] + vlad + \
        embed_specs(4096, H) + layer_specs(0, H, 3) + TOWER
    assert param_specs(cfgs(lstm_hidden=8, num_classes=8))[0][0] == TC + "embed/kernel"                  # H == C: no head
    # with every other cell the list is what it was: no temporal_conv variable
    for cell, kw in (("lstm", {}), ("gru", {}), ("mhsa", dict(sa_heads=2))):
        assert not [n for n, _ in param_specs(cfgs(rnn_cell=cell, **kw)) if "temporal_conv" in n]


def test_initialisation_decay_trust_ratio_classes_and_tier():
    """Kernels glorot-uniform (conv_kernel with Keras' Conv1D fans k H / k H), biases zero; the kernels (conv_kernel is rank 3) are
    decayed and trust-scaled, the biases are neither; all sit in the head's learning-rate tier and train under train_from: classifier;
    the exchange chunks cover them."""
    from vltf_amd.engine import decay_ranges, finetune_plan, init_params, lamb_ranges, lars_ranges, param_specs
    from vltf_amd.graph import init_params_for
    k, H = 5, 16
    cfg = cfgs(lr_mult=10.0, train_from="classifier", lstm_layers=2, tcn_kernel=k)
    specs = param_specs(cfg)
    offs, off = {}, 0
    for n, s in specs:
        offs[n] = (off, off + int(np.prod(s)))
        off += int(np.prod(s))
    names = R.param_names(2)
    weights = [n for n in names if n.endswith("kernel")]
    biases = [n for n in names if n.endswith("bias")]
    assert len(weights) == 5 and len(biases) == 5
    for p in (init_params(cfg, seed=1), init_params_for(specs, seed=1)):
        for n in names:
            if n.endswith("conv_kernel"):
                assert p[n].shape == (k, H, H)
                lim = np.sqrt(6.0 / (2 * k * H))
                assert p[n].std() > 0.4 * lim and 0.9 * lim < np.abs(p[n]).max() <= lim
            elif n.endswith("kernel"):
                lim = np.sqrt(6.0 / sum(p[n].shape))
                assert p[n].std() > 0.4 * lim and np.abs(p[n]).max() <= lim
            else:
                assert not p[n].any(), n
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
    from vltf_amd.engine import NetConfig, check_rnn_cell, check_tcn, param_specs, tcn_dilations
    from vltf_amd.graph import DatasetInfo, PipelineSpec, model_specs
    H, C, dim, T = 16, 5, 10, 4
    ds = {"main": DatasetInfo("vectors", T, 1, 3, dim=dim), "aux": DatasetInfo("vectors", 1, 1, 3, dim=7)}
    spec = lambda **kw: PipelineSpec("p", kw.pop("input", ["main"]), "nop", classifier=kw.pop("classifier", "lstm"), **kw)
    head = [("output_fc_w", (H, C)), ("output_fc_b", (C,))]
    tc = dict(rnn_cell="tcn")
    # GraphEngine lists a pipeline's variables in backward order
    got = model_specs([spec(lstm_params=(H, 2, "avg"), **tc)], ds, C)
    assert got == head + layer_specs(1, H, 3) + layer_specs(0, H, 3) + embed_specs(dim, H)
    got = model_specs([spec(lstm_params=(H, 1, "last"), tcn_kernel=2, tcn_causal=True, **tc)], ds, C)
    assert got == head + layer_specs(0, H, 2) + embed_specs(dim, H)
    two = [PipelineSpec("a", ["main"], "nop"), PipelineSpec("b", ["a"], "nop", classifier="lstm", lstm_params=(32, 1, "avg"), **tc)]
    assert ("b/" + TC + "layer_0/conv_kernel", (3, 32, 32)) in model_specs(two, ds, C)          # scoped like every other variable
    assert PipelineSpec("p", ["main"]).tcn_kernel is None and NetConfig().tcn_dilation is None and NetConfig().tcn_causal is None
    avg = dict(lstm_params=(H, 1, "avg"))
    for match, pipe in (("tcn_kernel is a key of rnn_cell tcn", spec(tcn_kernel=3, **avg)),                     # the keys without the cell
                        ("tcn_dilation is a key of rnn_cell tcn", spec(rnn_cell="gru", tcn_dilation="none", **avg)),
                        ("tcn_causal is a key of rnn_cell tcn", spec(rnn_cell="mhsa", sa_heads=2, tcn_causal=False, **avg)),
                        ("tcn_kernel is a key of rnn_cell tcn", spec(classifier="fc", tcn_kernel=3)),
                        ("tcn_causal is a key of rnn_cell tcn", spec(classifier=None, tcn_causal=True)),
                        ("sa_heads is a key of rnn_cell mhsa", spec(sa_heads=2, **avg, **tc)),                  # tcn is no mhsa
                        ("sa_block is a key of rnn_cell mhsa", spec(sa_block="encoder", **avg, **tc)),
                        ("tcn_kernel must be an integer in 1..9", spec(tcn_kernel=0, **avg, **tc)),
                        ("tcn_kernel must be an integer in 1..9", spec(tcn_kernel=10, tcn_causal=True, **avg, **tc)),
                        ("tcn_kernel must be an integer in 1..9", spec(tcn_kernel=3.0, **avg, **tc)),
                        ("tcn_kernel must be an integer in 1..9", spec(tcn_kernel=True, **avg, **tc)),
                        ("tcn_kernel must be odd unless tcn_causal", spec(tcn_kernel=4, **avg, **tc)),
                        ("tcn_dilation must be exponential or none", spec(tcn_dilation="linear", **avg, **tc)),
                        ("tcn_causal must be True or False", spec(tcn_causal="yes", **avg, **tc)),
                        ("at most 17 layers", spec(lstm_params=(H, 18, "avg"), **tc)),
                        ("H <= 1024", spec(lstm_params=(1028, 1, "avg"), **tc)),
                        ("lstm_bidirectional", spec(lstm_bidirectional=True, **avg, **tc)),
                        ("classifier lstm", spec(classifier="fc", **tc)),
                        ("classifier lstm", spec(classifier=None, **tc)),
                        ("state input", spec(input=["main", "aux"], **avg, **tc)),
                        ("fusion state", spec(lstm_params=(H, 1, "state"), **tc)),
                        ("must be lstm or gru", spec(rnn_cell="TCN", **avg))):
        with pytest.raises(VltfError, match=match):
            model_specs([pipe], ds, C)
    assert len(model_specs([spec(lstm_params=(H, 18, "avg"), tcn_dilation="none", **tc)], ds, C)) == 2 + 2 + 4 * 18
    # LRCNEngine's configuration
    for match, kw in (("tcn_kernel is a key of rnn_cell tcn", dict(rnn_cell="lstm", tcn_kernel=3)),
                      ("tcn_dilation is a key of rnn_cell tcn", dict(rnn_cell="gru", tcn_dilation="exponential")),
                      ("tcn_causal is a key of rnn_cell tcn", dict(rnn_cell="mhsa", sa_heads=2, tcn_causal=True)),
                      ("sa_heads is a key of rnn_cell mhsa", dict(sa_heads=2)), ("sa_positions is a key of rnn_cell mhsa", dict(sa_positions="none")),
                      ("tcn_kernel must be an integer", dict(tcn_kernel="three")), ("tcn_kernel must be odd", dict(tcn_kernel=2)),
                      ("tcn_dilation must be", dict(tcn_dilation="2")), ("tcn_causal must be", dict(tcn_causal=1)),
                      ("at most 17 layers", dict(lstm_layers=18)), ("H <= 1024", dict(lstm_hidden=1025)),
                      ("lstm_bidirectional", dict(lstm_bidirectional=True)), ("classifier lstm", dict(classifier="fc")),
                      ("classifier lstm", dict(classifier="none")), ("fusion state", dict(fusion="state")),
                      ("must be lstm or gru", dict(rnn_cell="conv"))):
        with pytest.raises(VltfError, match=match):
            param_specs(cfgs(**kw))
    with pytest.raises(VltfError, match="state input"):
        check_rnn_cell("tcn", state_input=True)
    assert check_tcn("lstm") is None and check_tcn("gru") is None and check_tcn("mhsa") is None
    assert check_tcn("tcn", 256, 2) == (3, "exponential", False) and check_tcn("tcn", 1024, 17, 9, "None", "None") == (9, "exponential", False)
    assert check_tcn("tcn", 7, 30, 4, "none", True) == (4, "none", True) and check_tcn("tcn", 7, 1, "None", None, False) == (3, "exponential", False)
    assert tcn_dilations("exponential", 4) == (1, 2, 4, 8) and tcn_dilations("none", 3) == (1, 1, 1) and tcn_dilations("exponential", 17)[-1] == 65536
    # the two-pipeline model keeps its LSTM
    with pytest.raises(VltfError, match=r"rnn_cell \[tcn\] is not built for the two-pipeline model"):
        ComposedEngine(cfgs(), HeadConfig(in_dim=4, fpc=3, num_classes=7), 2, device="cpu")


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


AVG16 = [16, 2, "defs.fusion_method.avg"]


def test_the_yaml_keys(tmp_path):
    from vltf_amd import run_task
    folder = str(tmp_path)
    data_path, _, _ = make_dataset(folder, "train.txt")
    keys = lambda o: (o.rnn_cell, o.tcn_kernel, o.tcn_dilation, o.tcn_causal)
    s, feeder = settings_for(folder, data_path, lambda p, r: p.update(lstm_params=AVG16, rnn_cell="tcn", tcn_kernel=4, tcn_dilation="none",
                                                                     tcn_causal=True), "tcn.yml")
    assert keys(s.pipelines["lrcn"]) == ("tcn", 4, "none", True)
    cfg, _ = run_task.net_config(s, feeder.get_dataset_by_tag("main")[0])
    assert keys(cfg) == ("tcn", 4, "none", True) and (cfg.lstm_hidden, cfg.lstm_layers, cfg.classifier) == (16, 2, "lstm")
    specs, _, _ = run_task.graph_config(s, feeder, 2)
    assert keys(specs[0]) == ("tcn", 4, "none", True)
    # the defaults, None / "None" meaning absent
    for extra in ({}, dict(tcn_kernel="None", tcn_dilation=None, tcn_causal="None"), dict(tcn_causal=False, tcn_dilation="exponential", tcn_kernel=3)):
        kw = dict(dict(lstm_params=AVG16, rnn_cell="tcn"), **extra)
        s, feeder = settings_for(folder, data_path, lambda p, r: p.update(**kw), "default.yml")
        assert keys(s.pipelines["lrcn"]) == ("tcn", 3, "exponential", False)
        cfg, _ = run_task.net_config(s, feeder.get_dataset_by_tag("main")[0])
        assert keys(cfg) == ("tcn", 3, "exponential", False)
        assert keys(run_task.graph_config(s, feeder, 2)[0][0]) == ("tcn", 3, "exponential", False)
    # without the cell: no keys, today's configuration
    s, feeder = settings_for(folder, data_path, lambda p, r: None, "plain.yml")
    assert keys(s.pipelines["lrcn"]) == ("lstm", None, None, None)
    cfg, _ = run_task.net_config(s, feeder.get_dataset_by_tag("main")[0])
    assert keys(cfg) == ("lstm", None, None, None)
    assert keys(run_task.graph_config(s, feeder, 2)[0][0]) == ("lstm", None, None, None)
    tc = dict(lstm_params=AVG16, rnn_cell="tcn")
    fc = lambda p: p.update(classifier="defs.classifier.fc", lstm_params=None)
    for match, edit in (("tcn_kernel is a key of rnn_cell tcn", lambda p, r: p.update(tcn_kernel=3)),                        # without the cell
                        ("tcn_dilation is a key of rnn_cell tcn", lambda p, r: p.update(rnn_cell="gru", tcn_dilation="none")),
                        ("tcn_causal is a key of rnn_cell tcn", lambda p, r: (fc(p), p.update(tcn_causal=True))),
                        ("sa_heads is a key of rnn_cell mhsa", lambda p, r: p.update(sa_heads=2, **tc)),
                        ("tcn_kernel must be an integer", lambda p, r: p.update(tcn_kernel=0, **tc)),
                        ("tcn_kernel must be an integer", lambda p, r: p.update(tcn_kernel=2.5, **tc)),
                        ("tcn_kernel must be odd", lambda p, r: p.update(tcn_kernel=4, **tc)),
                        ("tcn_dilation must be", lambda p, r: p.update(tcn_dilation="linear", **tc)),
                        ("tcn_causal must be", lambda p, r: p.update(tcn_causal="maybe", **tc)),
                        ("at most 17 layers", lambda p, r: p.update(lstm_params=[16, 18, "defs.fusion_method.avg"], rnn_cell="tcn")),
                        ("H <= 1024", lambda p, r: p.update(lstm_params=[1028, 1, "defs.fusion_method.avg"], rnn_cell="tcn")),
                        ("lstm_bidirectional", lambda p, r: p.update(lstm_bidirectional=True, **tc)),
                        ("classifier lstm", lambda p, r: (fc(p), p.update(rnn_cell="tcn"))),
                        ("classifier lstm", lambda p, r: (p.pop("classifier"), p.pop("lstm_params"), p.update(rnn_cell="tcn"))),
                        ("fusion state", lambda p, r: p.update(lstm_params=[16, 1, "defs.fusion_method.state"], rnn_cell="tcn")),
                        ("must be lstm or gru", lambda p, r: p.update(rnn_cell="tcnn"))):
        with pytest.raises(Exception, match=match):
            settings_for(folder, data_path, edit, "bad.yml")


def test_the_cell_is_admitted_beside_the_pinned_tuple():
    from vltf_amd._ffi import VltfError
    from vltf_amd.engine import RNN_CELLS, TEMPORAL_CELLS, check_rnn_cell
    assert RNN_CELLS == ("lstm", "gru", "mhsa") and TEMPORAL_CELLS == RNN_CELLS + ("tcn",)
    assert check_rnn_cell("tcn") == "tcn"
    with pytest.raises(VltfError, match="must be lstm or gru") as e:
        check_rnn_cell("rnn")
    assert "mhsa" in str(e.value) and "tcn" in str(e.value) and "[rnn]" in str(e.value)


def test_the_example_parses():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "examples", "lrcn_tcn.yml")) as f:
        cfg = yaml.safe_load(f)
    p = cfg["run"]["network"]["pipelines"][0]["lrcn"]
    assert p["lstm_params"] == [256, 2, "defs.fusion_method.avg"] and p["classifier"] == "defs.classifier.lstm"
    assert (p["rnn_cell"], p["tcn_kernel"], p["tcn_dilation"], p["tcn_causal"]) == ("tcn", 3, "exponential", False)
    assert cfg["run"]["run_id"] == "lrcn_tcn"


def test_the_example_goes_through_settings(tmp_path):
    """The example's pipeline keys, put on the test dataset, reach NetConfig."""
    from vltf_amd import run_task
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "examples", "lrcn_tcn.yml")) as f:
        ex = yaml.safe_load(f)["run"]["network"]["pipelines"][0]["lrcn"]
    folder = str(tmp_path)
    data_path, _, _ = make_dataset(folder, "train.txt")
    take = {k: ex[k] for k in ("lstm_params", "rnn_cell", "tcn_kernel", "tcn_dilation", "tcn_causal")}
    s, feeder = settings_for(folder, data_path, lambda p, r: p.update(**take), "example.yml")
    cfg, _ = run_task.net_config(s, feeder.get_dataset_by_tag("main")[0])
    assert (cfg.rnn_cell, cfg.lstm_hidden, cfg.lstm_layers, cfg.tcn_kernel, cfg.tcn_dilation, cfg.tcn_causal) == ("tcn", 256, 2, 3, "exponential", False)
