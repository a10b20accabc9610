"""sa_block encoder on the CPU: the fp64 reference of tests/encoder_block_ref.py against torch autograd, the host plumbing (variables,
refusals, YAML, checkpoints), the float32 restatement that decides the tolerance class of tests/test_encoder_block_gpu.py, and the
conditioning claim the block exists for.  No device."""
import math
import os

import numpy as np
import pytest
import torch
import yaml

from tests import encoder_block_ref as R
from tests import lstm_plan as LP
from tests import mhsa_ref as M
from tests.test_host_workflow import config, make_dataset
from tests.test_self_attention import TOWER, settings_for

F64 = np.float64
TOL = dict(act=(3e-5, 3e-5))                                     # tests/test_lstm_geometry_gpu.TOL["act"] (checked below)
T64 = lambda a: torch.tensor(np.asarray(a, F64), dtype=torch.float64, requires_grad=True)


# ---- 1. the reference is torch autograd in fp64 ----------------------------------------------------------------------------------------
def close64(got, want, what):
    want = np.asarray(want, F64)
    np.testing.assert_allclose(np.asarray(got, F64), want, rtol=0, atol=1e-10 * max(1.0, float(np.abs(want).max())), err_msg=what)


def live_rows(lens, clips, T):
    return torch.tensor(M.live_mask(lens, clips, T).reshape(-1, 1))


@pytest.mark.parametrize("residual", (True, False), ids=("residual", "plain"))
@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
@pytest.mark.parametrize("case", R.LN_CASES[:-1], ids=R.case_id)
def test_layer_norm_reference_is_torch_autograd(case, lens, residual):
    clips, T, W = case
    ref = R.ln_reference(case, 40, lens, residual)
    inp, m = ref.inp, live_rows(ref.lens, clips, T)
    x, r, gamma, beta = T64(inp.x), T64(inp.r), T64(inp.gamma), T64(inp.beta)
    s = x + r if residual else x
    y = torch.nn.functional.layer_norm(s, (W,), gamma, beta, R.EPS)
    close64(torch.where(m, y, 0.0).detach(), ref.fwd.y, "y")
    close64(torch.where(m, s, 0.0).detach(), ref.fwd.sum, "sum")
    # the backward from the fp64 forward's own s and stats (ln_reference's takes their fp32 roundings: the kernel's inputs)
    bwd = R.ln_backward(inp.dy, ref.fwd.sum, inp.gamma, ref.fwd.stats, inp.dres if residual else None, T, ref.lens)
    loss = (torch.where(m, y, 0.0) * torch.tensor(np.asarray(inp.dy, F64))).sum()
    if residual:
        loss = loss + (torch.where(m, s, 0.0) * torch.tensor(np.asarray(inp.dres, F64))).sum()
    loss.backward()
    close64(x.grad, bwd.dx, "dx")
    close64(gamma.grad, bwd.dgbp[:, :W].sum(axis=0), "dgamma")
    close64(beta.grad, bwd.dgbp[:, W:].sum(axis=0), "dbeta")
    if lens and clips > 1:
        dead = ~M.live_mask(ref.lens, clips, T).reshape(-1)
        assert dead.any() and not bwd.dx[dead].any() and not ref.fwd.y[dead].any() and not ref.fwd.stats[dead].any()
        assert not bwd.dgbp[M.live_lens(ref.lens, clips, T) == 0].any()


def test_gelu_reference_is_torch_autograd():
    u, df = R.gelu_inputs(4099)
    t = T64(u)
    f = torch.nn.functional.gelu(t)                              # approximate="none": the erf form
    close64(f.detach(), R.gelu(u), "gelu")
    (f * torch.tensor(np.asarray(df, F64))).sum().backward()
    close64(t.grad, R.gelu_grad(df, u), "gelu'")
    sat = R.gelu_grad(np.ones(2), np.array([-40.0, 40.0]))
    assert sat[0] == 0.0 and sat[1] == 1.0 and np.isfinite(R.gelu(np.array(R.GELU_VALUES))).all()


def torch_stack(feat, tp, T, layers, heads, lens, positions):
    """The stack with torch's own layer_norm, gelu and softmax; tp {name: tensor}."""
    rows, H = feat.shape[0], tp[R.var(-1, "gamma")].shape[0]
    b, dh = rows // T, H // heads
    m2 = torch.tensor(M.live_mask(lens, b, T))
    m = m2.reshape(-1, 1)
    ln = lambda x, l, which: torch.nn.functional.layer_norm(x, (H,), tp[R.var(l, which + "gamma")], tp[R.var(l, which + "beta")], R.EPS)
    x = torch.where(m, torch.where(m, feat, 0.0) @ tp[R.var(None, "kernel")] + tp[R.var(None, "bias")], 0.0)
    P = None
    for l in range(layers):
        v = lambda name: tp[R.var(l, name)]
        n1 = torch.where(m, ln(x, l, "norm1_"), 0.0)
        qkv = (n1 @ v("qkv_kernel") + v("qkv_bias")).reshape(b, T, 3, heads, dh).permute(2, 0, 3, 1, 4)
        S = qkv[0] @ qkv[1].transpose(2, 3) / math.sqrt(dh)
        if positions:
            S = S + v("position_bias")[:, torch.tensor(M.rel_index(T))][None]
        S = S.masked_fill(~m2[:, None, None, :], -1e300)
        P = torch.softmax(S, dim=3)
        ctx = (P @ qkv[2]).permute(0, 2, 1, 3).reshape(rows, H)
        a = torch.where(m, x + ctx @ v("out_kernel") + v("out_bias"), 0.0)
        n2 = ln(a, l, "norm2_")
        x = torch.where(m, a + torch.nn.functional.gelu(n2 @ v("ffn1_kernel") + v("ffn1_bias")) @ v("ffn2_kernel") + v("ffn2_bias"), 0.0)
    return torch.where(m, ln(x, -1, ""), 0.0), P


@pytest.mark.parametrize("positions", (True, False), ids=("relative", "nopos"))
@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
@pytest.mark.parametrize("layers", (1, 2))
def test_block_and_stack_reference_is_torch_autograd(layers, lens, positions):
    clips, T, d, H, F, heads = 4, 5, 10, 16, 24, 2
    rng = np.random.default_rng([layers, lens, positions])
    p = R.default_init(rng, R.param_shapes(layers, d, H, F, heads, T, positions=positions), perturb=0.2)
    feat = (3.0 * rng.standard_normal((clips * T, d))).astype(np.float32)
    dout = rng.standard_normal((clips * T, H))
    L = LP.lengths(clips, T) if lens else None
    out, cache = R.stack_forward(feat, p, T, layers, heads, L, positions=positions)
    dfeat, grads = R.stack_backward(dout, cache)
    tp = {k: T64(v) for k, v in p.items()}
    tf = T64(feat)
    tout, tP = torch_stack(tf, tp, T, layers, heads, L, positions)
    close64(tout.detach(), out, "out")
    (tout * torch.tensor(dout)).sum().backward()
    close64(tf.grad, dfeat, "dfeat")
    assert set(grads) == set(p) == set(R.param_names(layers, positions=positions))
    for k in p:
        close64(tp[k].grad, grads[k], k)
        assert np.abs(grads[k]).max() > 1e-6, k
    live = M.live_mask(L, clips, T)
    both = live[:, None, :, None] & live[:, None, None, :]
    close64(np.where(both, tP.detach().numpy(), 0.0), R.last_P(cache), "P")


# ---- 2. - 5. host plumbing ---------------------------------------------------------------------------------------------------------------
def cfgs(**kw):
    from vltf_amd.engine import NetConfig
    base = dict(image_shape=(67, 67, 3), num_classes=7, fpc=3, lstm_hidden=16, lstm_layers=1, fusion="avg", rnn_cell="mhsa", sa_heads=2,
                sa_block="encoder")
    base.update(kw)
    return NetConfig(**base)


def block_specs(layers, d, H, F, heads, T, positions=True, scope=""):
    return list(R.param_shapes(layers, d, H, F, heads, T, scope, positions).items())


def test_param_specs_names_shapes_and_order():
    """The head, (attention_pool,) the embedding, the layers ascending -- each layer in forward order --, the final norm, the tower;
    GraphEngine, which lists a pipeline's variables in backward order, has the final norm, the layers descending, the embedding."""
    from vltf_amd.engine import ENC_LAYER_VARS, encoder_specs, encoder_var, param_specs
    from vltf_amd.graph import DatasetInfo, PipelineSpec, model_specs
    H, C, T = 16, 7, 3
    head = [("output_fc_w", (H, C)), ("output_fc_b", (C,))]
    assert ENC_LAYER_VARS == R.LAYER_VARS and encoder_var("p/", None, "kernel") == R.var(None, "kernel", "p/")
    assert encoder_var("", -1, "gamma") == "self_attention/final_norm/gamma" and encoder_var("", 1, "ffn1_bias") == "self_attention/layer_1/ffn1_bias"
    assert encoder_specs(2, 4096, H, 64, 2, T) == block_specs(2, 4096, H, 64, 2, T)
    assert param_specs(cfgs()) == head + block_specs(1, 4096, H, 4 * H, 2, T) + TOWER                      # F defaults to 4 H
    assert param_specs(cfgs(lstm_layers=2, sa_ffn_dim=24)) == head + block_specs(2, 4096, H, 24, 2, T) + TOWER
    assert param_specs(cfgs(sa_positions="none", sa_ffn_dim=8)) == head + block_specs(1, 4096, H, 8, 2, T, False) + TOWER
    attn = [("attention_pool/kernel", (H, 5)), ("attention_pool/bias", (5,)), ("attention_pool/context", (5, 1))]
    assert param_specs(cfgs(fusion="attn", attn_dim=5)) == head + attn + block_specs(1, 4096, H, 64, 2, T) + TOWER
    names = [n for n, _ in block_specs(2, 4096, H, 64, 2, T)]
    assert names[:3] == ["self_attention/embed/kernel", "self_attention/embed/bias", "self_attention/layer_0/norm1_gamma"]
    assert names[-2:] == ["self_attention/final_norm/gamma", "self_attention/final_norm/beta"]
    assert dict(block_specs(2, 4096, H, 64, 2, T))["self_attention/layer_0/qkv_kernel"] == (H, 3 * H)    # H wide also in layer 0
    assert dict(block_specs(1, H, H, 64, 2, T))["self_attention/embed/kernel"] == (H, H)                  # the embedding also when d == H
    ds = {"main": DatasetInfo("vectors", T, 1, 3, dim=10)}
    got = model_specs([PipelineSpec("p", ["main"], "nop", classifier="lstm", lstm_params=(H, 2, "avg"), rnn_cell="mhsa", sa_heads=2,
                                    sa_block="encoder", sa_ffn_dim=24)], ds, C)
    fwd = block_specs(2, 10, H, 24, 2, T)
    groups = [fwd[:2], fwd[2:15], fwd[15:28], fwd[28:]]
    assert got == head + [s for grp in reversed(groups) for s in grp]


def test_plain_and_absent_give_exactly_todays_spec_list():
    from vltf_amd.engine import NetConfig, param_specs
    from vltf_amd.graph import DatasetInfo, PipelineSpec, model_specs
    from tests.test_self_attention import layer_specs
    H, C, T = 16, 7, 3
    head = [("output_fc_w", (H, C)), ("output_fc_b", (C,))]
    today = head + layer_specs(0, 4096, H, 2, T) + layer_specs(1, H, H, 2, T) + TOWER
    for block in (None, "None", "plain"):
        assert param_specs(cfgs(sa_block=block, lstm_layers=2)) == today
    assert NetConfig().sa_block is None and NetConfig().sa_ffn_dim is None and PipelineSpec("p", ["main"]).sa_block is None
    ds = {"main": DatasetInfo("vectors", T, 1, 3, dim=10)}
    spec = lambda **kw: PipelineSpec("p", ["main"], "nop", classifier="lstm", lstm_params=(H, 1, "avg"), rnn_cell="mhsa", sa_heads=2, **kw)
    assert model_specs([spec()], ds, C) == model_specs([spec(sa_block="plain")], ds, C) == head + layer_specs(0, 10, H, 2, T)
    # every other cell: untouched
    assert param_specs(cfgs(rnn_cell="gru", sa_heads=None, sa_block=None)) == param_specs(NetConfig(**dict(
        image_shape=(67, 67, 3), num_classes=7, fpc=3, lstm_hidden=16, lstm_layers=1, fusion="avg", rnn_cell="gru")))


def test_initialisation_decay_and_trust_classes():
    """Kernels glorot-uniform, gammas ones, betas, biases and position_bias zeros; rank-1 variables are neither decayed nor trust-scaled,
    the kernels and position_bias are; everything is in the head's tier."""
    from vltf_amd.engine import decay_ranges, finetune_plan, init_params, lamb_ranges, lars_ranges, param_specs
    from vltf_amd.graph import init_params_for
    cfg = cfgs(lr_mult=10.0, train_from="classifier", lstm_layers=2, sa_ffn_dim=24)
    specs = param_specs(cfg)
    offs, off = {}, 0
    for n, s in specs:
        offs[n] = (off, off + int(np.prod(s)))
        off += int(np.prod(s))
    names = R.param_names(2)
    for p in (init_params(cfg, seed=1), init_params_for(specs, seed=1)):
        for n in names:
            if n.endswith("kernel"):
                lim = np.sqrt(6.0 / sum(p[n].shape))
                assert p[n].std() > 0.4 * lim and np.abs(p[n]).max() <= lim
            elif n.endswith("gamma"):
                assert (p[n] == 1.0).all(), n
            else:
                assert not p[n].any(), n
    plan = finetune_plan(cfg)
    inside = lambda rng, lo, hi: any(a <= lo and hi <= b for a, b in rng)
    ranges = decay_ranges(specs, plan, 5e-4)
    decayed, plain = [(a, b) for a, b, c in ranges if c > 0], [(a, b) for a, b, c in ranges if c == 0]
    lars, _, _ = lars_ranges(specs, plan, 0.0)
    lamb, _ = lamb_ranges(specs, plan, 0.0)
    for n in names:
        lo, hi = offs[n]
        assert [m for a, b, m in plan.tiers if a <= lo and hi <= b] == [10.0], n
        if len(dict(specs)[n]) >= 2:
            assert inside(decayed, lo, hi) and (lo, hi) in [(a, b) for a, b, _, t in lars if t >= 0], n
            assert (lo, hi) in [(r[0], r[1]) for r in lamb if r[4] >= 0], n
        else:
            assert inside(plain, lo, hi) and not inside(decayed, lo, hi), n
            assert inside([(a, b) for a, b, _, t in lars if t < 0], lo, hi) and inside([(r[0], r[1]) for r in lamb if r[4] < 0], lo, hi), n


def test_refusals_by_message():
    from vltf_amd._ffi import VltfError
    from vltf_amd.composed import ComposedEngine, HeadConfig
    from vltf_amd.engine import check_mhsa, check_sa_block, param_specs
    from vltf_amd.graph import DatasetInfo, PipelineSpec, model_specs
    H, C, T = 16, 5, 4
    ds = {"main": DatasetInfo("vectors", T, 1, 3, dim=10), "aux": DatasetInfo("vectors", 1, 1, 3, dim=7)}
    spec = lambda **kw: PipelineSpec("p", kw.pop("input", ["main"]), "nop", classifier=kw.pop("classifier", "lstm"), **kw)
    enc = dict(rnn_cell="mhsa", sa_heads=2, sa_block="encoder")
    avg = dict(lstm_params=(H, 1, "avg"))
    for match, pipe in (("sa_block is a key of rnn_cell mhsa", spec(sa_block="encoder", **avg)),
                        ("sa_block is a key of rnn_cell mhsa", spec(rnn_cell="gru", sa_block="plain", **avg)),
                        ("sa_ffn_dim is a key of rnn_cell mhsa", spec(sa_ffn_dim=64, **avg)),
                        ("sa_block is a key of rnn_cell mhsa", spec(classifier="fc", sa_block="encoder")),
                        ("sa_ffn_dim is a key of sa_block encoder", spec(rnn_cell="mhsa", sa_heads=2, sa_ffn_dim=64, **avg)),
                        ("sa_ffn_dim is a key of sa_block encoder", spec(rnn_cell="mhsa", sa_heads=2, sa_block="plain", sa_ffn_dim=64, **avg)),
                        ("sa_block must be plain or encoder", spec(rnn_cell="mhsa", sa_heads=2, sa_block="decoder", **avg)),
                        ("sa_ffn_dim must be an integer in 8..4096", spec(sa_ffn_dim=7, **enc, **avg)),
                        ("sa_ffn_dim must be an integer in 8..4096", spec(sa_ffn_dim=4097, **enc, **avg)),
                        ("sa_ffn_dim must be an integer in 8..4096", spec(sa_ffn_dim=64.0, **enc, **avg)),
                        ("sa_ffn_dim must be an integer in 8..4096", spec(sa_ffn_dim="64", **enc, **avg)),
                        ("sa_ffn_dim must be an integer in 8..4096", spec(sa_ffn_dim=True, **enc, **avg)),
                        # mhsa's own limits and refusals stand
                        ("H % heads == 0", spec(lstm_params=(H, 1, "avg"), rnn_cell="mhsa", sa_heads=3, sa_block="encoder")),
                        ("8 <= dh", spec(lstm_params=(H, 1, "avg"), rnn_cell="mhsa", sa_heads=4, sa_block="encoder")),
                        ("H <= 1024", spec(lstm_params=(1032, 1, "avg"), rnn_cell="mhsa", sa_heads=12, sa_block="encoder")),
                        ("lstm_bidirectional", spec(lstm_bidirectional=True, **enc, **avg)),
                        ("classifier lstm", spec(classifier="fc", **enc)),
                        ("classifier lstm", spec(classifier=None, **enc)),
                        ("state input", spec(input=["main", "aux"], **enc, **avg)),
                        ("fusion state", spec(lstm_params=(H, 1, "state"), **enc))):
        with pytest.raises(VltfError, match=match):
            model_specs([pipe], ds, C)
    with pytest.raises(VltfError, match="T <= 64"):
        model_specs([spec(**enc, **avg)], {"main": DatasetInfo("vectors", 65, 1, 3, dim=10)}, C)
    for match, kw in (("sa_block is a key of rnn_cell mhsa", dict(rnn_cell="lstm", sa_heads=None)),
                      ("sa_ffn_dim is a key of rnn_cell mhsa", dict(rnn_cell="gru", sa_heads=None, sa_block=None, sa_ffn_dim=32)),
                      ("sa_ffn_dim is a key of sa_block encoder", dict(sa_block=None, sa_ffn_dim=32)),
                      ("sa_block must be plain or encoder", dict(sa_block="post_ln")),
                      ("sa_ffn_dim must be an integer in 8..4096", dict(sa_ffn_dim=4)),
                      ("sa_ffn_dim must be an integer in 8..4096", dict(sa_ffn_dim=8192)),
                      ("sa_ffn_dim must be an integer in 8..4096", dict(sa_ffn_dim=32.5)),
                      ("T <= 64", dict(fpc=65)), ("fusion state", dict(fusion="state")), ("lstm_bidirectional", dict(lstm_bidirectional=True)),
                      ("classifier lstm", dict(classifier="fc")), ("8 <= dh", dict(sa_heads=4))):
        with pytest.raises(VltfError, match=match):
            param_specs(cfgs(**kw))
    assert check_sa_block("lstm") is None and check_sa_block("mhsa", 16) is None and check_sa_block("mhsa", 16, "plain") is None
    assert check_sa_block("mhsa", 16, "encoder") == 64 and check_sa_block("mhsa", 1024, "encoder", "None") == 4096
    assert check_sa_block("mhsa", 16, "encoder", 8) == 8 and check_sa_block("mhsa", 16, "encoder", np.int64(4096)) == 4096
    assert check_mhsa("mhsa", 256, 16, sa_block="encoder", sa_ffn_dim=512) == (4, "relative")            # (heads, positions), as ever
    with pytest.raises(VltfError, match="not built for the two-pipeline model"):
        ComposedEngine(cfgs(), HeadConfig(in_dim=4, fpc=3, num_classes=7), 2, device="cpu")


AVG16 = [16, 1, "defs.fusion_method.avg"]


def test_the_yaml_keys(tmp_path):
    from vltf_amd import run_task
    folder = str(tmp_path)
    data_path, _, _ = make_dataset(folder, "train.txt")
    mh = dict(lstm_params=AVG16, rnn_cell="mhsa", sa_heads=2)
    s, feeder = settings_for(folder, data_path, lambda p, r: p.update(sa_block="encoder", sa_ffn_dim=24, **mh), "enc.yml")
    p = s.pipelines["lrcn"]
    assert (p.rnn_cell, p.sa_block, p.sa_ffn_dim) == ("mhsa", "encoder", 24)
    cfg, _ = run_task.net_config(s, feeder.get_dataset_by_tag("main")[0])
    assert (cfg.rnn_cell, cfg.sa_block, cfg.sa_ffn_dim, cfg.sa_heads) == ("mhsa", "encoder", 24, 2)
    specs, _, _ = run_task.graph_config(s, feeder, 2)
    assert (specs[0].sa_block, specs[0].sa_ffn_dim) == ("encoder", 24)
    s, feeder = settings_for(folder, data_path, lambda p, r: p.update(sa_block="encoder", sa_ffn_dim="None", **mh), "default.yml")
    assert (s.pipelines["lrcn"].sa_block, s.pipelines["lrcn"].sa_ffn_dim) == ("encoder", 64)               # 4 H
    for extra in (dict(), dict(sa_block="plain"), dict(sa_block=None, sa_ffn_dim=None)):                   # plain: today's configuration
        s, feeder = settings_for(folder, data_path, lambda p, r: p.update(**mh, **extra), "plain.yml")
        assert (s.pipelines["lrcn"].sa_block, s.pipelines["lrcn"].sa_ffn_dim) == (None, None)
        cfg, _ = run_task.net_config(s, feeder.get_dataset_by_tag("main")[0])
        assert (cfg.sa_block, cfg.sa_ffn_dim) == (None, None)
    for match, edit in (("sa_block is a key of rnn_cell mhsa", lambda p, r: p.update(sa_block="encoder")),
                        ("sa_ffn_dim is a key of rnn_cell mhsa", lambda p, r: p.update(rnn_cell="gru", sa_ffn_dim=32)),
                        ("sa_ffn_dim is a key of sa_block encoder", lambda p, r: p.update(sa_ffn_dim=32, **mh)),
                        ("sa_block must be plain or encoder", lambda p, r: p.update(sa_block="block", **mh)),
                        ("sa_ffn_dim must be an integer", lambda p, r: p.update(sa_block="encoder", sa_ffn_dim=7, **mh)),
                        ("sa_ffn_dim must be an integer", lambda p, r: p.update(sa_block="encoder", sa_ffn_dim=4097, **mh)),
                        ("sa_ffn_dim must be an integer", lambda p, r: p.update(sa_block="encoder", sa_ffn_dim=32.5, **mh)),
                        ("sa_ffn_dim must be an integer", lambda p, r: p.update(sa_block="encoder", sa_ffn_dim="wide", **mh))):
        with pytest.raises(Exception, match=match):
            settings_for(folder, data_path, edit, "bad.yml")


def test_the_example_parses():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "examples", "lrcn_encoder_block.yml")) as f:
        cfg = yaml.safe_load(f)
    p = cfg["run"]["network"]["pipelines"][0]["lrcn"]
    assert p["lstm_params"] == [256, 2, "defs.fusion_method.avg"] and p["classifier"] == "defs.classifier.lstm"
    assert (p["rnn_cell"], p["sa_heads"], p["sa_block"], p["sa_ffn_dim"]) == ("mhsa", 4, "encoder", 1024)
    assert cfg["run"]["run_id"] == "lrcn_encoder_block"


def test_a_plain_checkpoint_is_refused_by_an_encoder_model_and_the_reverse(tmp_path):
    from tests.test_self_attention import StubEngine
    from vltf_amd import settings_
    folder = str(tmp_path)
    data_path, _, _ = make_dataset(folder, "train.txt")
    s = settings_.Settings()
    feeder = s.initialize(config(folder, data_path))
    small = dict(image_shape=(16, 16, 3), num_classes=4)
    feeder.compute_save_interval()
    feeder.num_saves = 0
    bases = {tag: feeder.save(StubEngine(cfgs(sa_block=tag, **small), seed=1), "ep_%s" % tag, 2) for tag in ("plain", "encoder")}
    with np.load(bases["encoder"] + ".weights.npz") as z:
        assert set(R.param_names(1)) <= set(z.files) and z["self_attention/layer_0/ffn1_kernel"].shape == (16, 64)
    f2 = settings_.Settings().initialize(config(folder, data_path, resume_file=bases["encoder"]))
    fresh = StubEngine(cfgs(**small), seed=2)
    f2.init_saveload(fresh, bases["encoder"])
    assert (fresh.params["self_attention/final_norm/gamma"] == 1.0).all()
    with pytest.raises(Exception):
        f2.init_saveload(StubEngine(cfgs(**small), seed=2), bases["plain"])
    with pytest.raises(Exception):
        f2.init_saveload(StubEngine(cfgs(sa_block="plain", **small), seed=2), bases["encoder"])


# ---- 6. float32 decides the tolerance class -------------------------------------------------------------------------------------------
def ratio_of(got, want):
    rtol, atol_rel = TOL["act"]
    w = np.asarray(want, F64)
    bound = atol_rel * (float(np.abs(w).max()) or 1.0) + rtol * np.abs(w)
    return float((np.abs(np.asarray(got, F64) - w) / bound).max())


def test_float32_stays_inside_half_of_class_act():
    """A plain float32 numpy restatement of the four launches (encoder_block_ref with dt = float32; the backward from the reference's s
    and stats rounded to fp32) against fp64, over every kernel case, both input scales, with and without lengths, with and without the
    residual: worst error / bound per output at class act (3e-5, 3e-5), stats per column (mean and rstd differ by three orders of
    magnitude at scale 40).  At or below 0.5 everywhere, so the GPU tests take class act; the ratios are printed and stand in DESIGN 4.28."""
    f32 = np.float32
    worst = dict.fromkeys(("y", "sum", "mean", "rstd", "dx", "dgbp", "gelu", "dgelu"), 0.0)
    for case in R.LN_CASES:
        clips, T, W = case
        for scale in R.SCALES:
            for lens in (False, True):
                for residual in (True, False):
                    ref = R.ln_reference(case, scale, lens, residual)
                    inp = ref.inp
                    fwd = R.ln_forward(inp.x, inp.r if residual else None, inp.gamma, inp.beta, T, ref.lens, dt=f32)
                    bwd = R.ln_backward(inp.dy, ref.s32, inp.gamma, ref.stats32, inp.dres if residual else None, T, ref.lens, dt=f32)
                    assert fwd.y.dtype == f32 and bwd.dx.dtype == f32 and bwd.dgbp.dtype == f32
                    pairs = dict(y=(fwd.y, ref.fwd.y), sum=(fwd.sum, ref.fwd.sum), mean=(fwd.stats[:, 0], ref.fwd.stats[:, 0]),
                                 rstd=(fwd.stats[:, 1], ref.fwd.stats[:, 1]), dx=(bwd.dx, ref.bwd.dx), dgbp=(bwd.dgbp, ref.bwd.dgbp))
                    for name, (g, w) in pairs.items():
                        r = ratio_of(g, w)
                        worst[name] = max(worst[name], r)
                        assert r <= 0.5, "%s at case %s, scale %d, lens %s, residual %s: error / bound %.3f" % (name, case, scale, lens, residual, r)
    for count in R.GELU_COUNTS:
        u, df = R.gelu_inputs(count)
        for name, g, w in (("gelu", R.gelu(u, f32), R.gelu(u)), ("dgelu", R.gelu_grad(df, u, f32), R.gelu_grad(df, u))):
            assert g.dtype == f32
            r = ratio_of(g, w)
            worst[name] = max(worst[name], r)
            assert r <= 0.5, "%s at count %d: error / bound %.3f" % (name, count, r)
    print("encoder block launches in float32, worst error / bound:", " ".join("%s %.3f" % kv for kv in sorted(worst.items())))


def test_the_class_is_that_of_the_lstm_geometry_tests():
    import ast
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_lstm_geometry_gpu.py")).read()
    node = next(n for n in ast.parse(src).body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", None) == "TOL")
    theirs = {kw.arg: ast.literal_eval(kw.value) for kw in node.value.keywords}
    assert {k: theirs[k] for k in TOL} == TOL


def test_the_cases_reach_both_register_layouts_and_the_ragged_groups():
    """W % 4 == 0 (granules) and not (dwords); widths that leave the last register group partly filled; row counts that are no multiple
    of the four rows of a forward workgroup; step counts that are no multiple of the four rows a backward group takes; the limits."""
    Ws = [c[2] for c in R.LN_CASES]
    assert any(w % 4 for w in Ws) and any(w % 4 == 0 for w in Ws) and min(Ws) == 8 and max(Ws) == 1024
    assert any(w % 4 == 0 and (w // 4) % 64 for w in Ws) and any(w % 4 and w % 64 for w in Ws)
    assert any((c[0] * c[1]) % 4 for c in R.LN_CASES) and any(c[1] % 4 for c in R.LN_CASES) and any(c[1] > 4 for c in R.LN_CASES)
    assert max(c[1] for c in R.LN_CASES) == 64 and any(n % 4 for n in R.GELU_COUNTS) and max(R.GELU_COUNTS) > 4096
    for clips, T, _ in R.LN_CASES:
        if clips > 1:
            L = M.live_lens(LP.lengths(clips, T), clips, T)
            assert (L == 0).any() and (L == T).any()


# ---- 7. the conditioning claim ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers", (1, 2))
def test_default_initialisation_on_features_of_rms_40_is_trainable(layers):
    """What the block is for: on features of rms 40 (the tower's scale), at the default initialisation and with NO rescaling of any
    kernel, no softmax of the last layer is saturated and a gradient reaches every variable of the stack -- where the bare layer at
    the same features has one-hot softmaxes and exactly zero Q, K and position-bias gradients in fp32."""
    clips, T, d, H, F, heads = 4, 5, 64, 16, 64, 2
    rng = np.random.default_rng(40 + layers)
    feat = np.maximum(rng.standard_normal((clips * T, d)), 0.0)
    feat = (feat * 40.0 / np.sqrt(np.mean(feat ** 2))).astype(np.float32)
    assert abs(np.sqrt(np.mean(feat.astype(F64) ** 2)) - 40.0) < 1e-3
    p = R.default_init(rng, R.param_shapes(layers, d, H, F, heads, T))
    out, cache = R.stack_forward(feat, p, T, layers, heads)
    assert R.last_P(cache).max() < 0.999
    _, grads = R.stack_backward(rng.standard_normal(out.shape), cache)
    for k in R.param_names(layers):
        assert np.abs(grads[k]).max() > 1e-6, "no gradient reaches " + k
    # the bare layer on the same features: saturated
    q = M.param_names(0)
    lim = math.sqrt(6.0 / (d + 3 * H))
    bare = {q[0]: rng.uniform(-lim, lim, (d, 3 * H)), q[1]: np.zeros(3 * H), q[2]: np.eye(H), q[3]: np.zeros(H), q[4]: np.zeros((heads, 2 * T - 1))}
    _, caches = M.stack_forward(feat, bare, T, 1, heads)
    assert caches[-1].fwd.P.max() > 0.999
