"""sa_attn_dropout / sa_dropout / sa_drop_path on the CPU: the fp64 reference of tests/encoder_dropout_ref.py against torch autograd with
the masks applied as constants, the statistics of the mask restatement, the host plumbing (refusals, defaults, YAML, the planned
variables and buffers), and the float32 restatement that decides the tolerance class of tests/test_encoder_dropout_gpu.py.  No device."""
import math
import os

import numpy as np
import pytest
import torch
import yaml

from tests import encoder_block_ref as E
from tests import encoder_dropout_ref as D
from tests import lstm_plan as LP
from tests import mhsa_ref as M
from tests.test_encoder_block import T64, close64, ratio_of
from tests.test_host_workflow import make_dataset
from tests.test_self_attention import settings_for

F64, F32 = np.float64, np.float32
OPTIONS = dict(attn=dict(attn=0.4), elem=dict(elem=0.3), path=dict(path=0.5), all=dict(attn=0.4, elem=0.3, path=0.5))
ATTN_CASES = [(1, 1, 8, 1), (3, 2, 24, 3), (2, 21, 250, 5), (2, 64, 64, 1), (2, 64, 1024, 8)]          # of mhsa_ref.CASES: the GPU test's
KEEPS = (0.5, 0.9)


# ---- 1. the reference is torch autograd in fp64, the masks constants ---------------------------------------------------------------------
def tconst(a):
    return torch.tensor(np.asarray(a, F64))


def torch_attention(qkv, pos, b, T, H, heads, m2, Fw):
    dh = H // heads
    q = qkv.reshape(b, T, 3, heads, dh).permute(2, 0, 3, 1, 4)
    S = q[0] @ q[1].transpose(2, 3) / math.sqrt(dh)
    if pos is not None:
        S = S + pos[:, torch.tensor(M.rel_index(T))][None]
    S = S.masked_fill(~m2[:, None, None, :], -1e300)
    P = torch.softmax(S, dim=3)
    Pd = P if Fw is None else P * tconst(Fw)
    return (Pd @ q[2]).permute(0, 2, 1, 3).reshape(b * T, H), P


def torch_stack(feat, tp, T, layers, heads, lens, positions, dr):
    """tests/test_encoder_block.torch_stack with the factors of dr as constants."""
    rows, H = feat.shape[0], tp[E.var(-1, "gamma")].shape[0]
    b = rows // T
    m2 = torch.tensor(M.live_mask(lens, b, T))
    m = m2.reshape(-1, 1)
    ln = lambda x, l, which: torch.nn.functional.layer_norm(x, (H,), tp[E.var(l, which + "gamma")], tp[E.var(l, which + "beta")], E.EPS)
    x = torch.where(m, torch.where(m, feat, 0.0) @ tp[E.var(None, "kernel")] + tp[E.var(None, "bias")], 0.0)
    P = None
    for l in range(layers):
        v = lambda name: tp[E.var(l, name)]
        f0, f1 = dr.branch(l, 0, b, T, H), dr.branch(l, 1, b, T, H)
        n1 = torch.where(m, ln(x, l, "norm1_"), 0.0)
        ctx, P = torch_attention(n1 @ v("qkv_kernel") + v("qkv_bias"), v("position_bias") if positions else None, b, T, H, heads, m2,
                                 dr.weights(l, b, heads, T))
        o = ctx @ v("out_kernel") + v("out_bias")
        a = torch.where(m, x + (o if f0 is None else o * tconst(f0)), 0.0)
        n2 = ln(a, l, "norm2_")
        mo = torch.nn.functional.gelu(n2 @ v("ffn1_kernel") + v("ffn1_bias")) @ v("ffn2_kernel") + v("ffn2_bias")
        x = torch.where(m, a + (mo if f1 is None else mo * tconst(f1)), 0.0)
    return torch.where(m, ln(x, -1, ""), 0.0), P


@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
@pytest.mark.parametrize("keep", KEEPS)
def test_attention_launch_reference_is_torch_autograd(keep, lens):
    """Layer level: the dropped attention forward / backward (the kernels' contract) on a kernel case."""
    case = (3, 5, 24, 3)
    b, T, H, heads = case
    inp = M.inputs(*case)
    L = LP.lengths(b, T) if lens else None
    Fw = D.weight_factor(D.seed_of(3), D.salt_of(0, 1, "weights"), b, heads, T, D.keep_of(1 - keep), clip0=2)
    assert 0.0 < (Fw == 0).mean() < 1.0
    fwd = D.attn_forward(inp.qkv, inp.pos, heads, Fw, L, T)
    bwd = D.attn_backward(inp.dctx, inp.qkv, fwd.P, heads, Fw, L, T)
    m2 = torch.tensor(M.live_mask(L, b, T))
    m = m2.reshape(-1, 1)
    qkv, pos = T64(inp.qkv), T64(inp.pos)
    ctx, P = torch_attention(torch.where(m, qkv, 0.0), pos, b, T, H, heads, m2, Fw)
    close64(torch.where(m, ctx, 0.0).detach(), fwd.ctx, "ctx")
    live = M.live_mask(L, b, T)
    close64(np.where(live[:, None, :, None] & live[:, None, None, :], P.detach().numpy(), 0.0), fwd.P, "P (undropped)")
    (torch.where(m, ctx, 0.0) * tconst(inp.dctx)).sum().backward()
    close64(qkv.grad, bwd.dqkv, "dqkv")
    close64(pos.grad, bwd.dposp.sum(axis=0), "dpos")
    none = D.attn_forward(inp.qkv, inp.pos, heads, None, L, T)                     # without a factor: mhsa_ref itself
    want = M.forward(inp.qkv, inp.pos, heads, L, T)
    close64(none.P, want.P, "P, no dropout")
    close64(none.ctx, want.ctx, "ctx, no dropout")
    close64(fwd.P, want.P, "P is stored undropped")


@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
@pytest.mark.parametrize("option", ("elem", "path", "all"))
def test_add_norm_launch_reference_is_torch_autograd(option, lens):
    """Layer level: the dropped add-and-norm and the branch gradient on a kernel case."""
    case = (21, 5, 250)
    clips, T, W = case
    inp = E.ln_inputs(clips, T, W, 40)
    L = LP.lengths(clips, T) if lens else None
    o = OPTIONS[option]
    f = D.branch_factor(D.seed_of(5), D.salt_of(0, 0, "ffn_branch"), D.salt_of(0, 0, "path"), clips, T, W, 1, D.keep_of(o.get("elem", 0)),
                        D.path_keep(o.get("path", 0), 0, 1), clip0=3)
    assert 0.0 < (f == 0).mean() < 1.0
    fwd = D.ln_drop_forward(inp.x, inp.r, f, inp.gamma, inp.beta, T, L)
    m = torch.tensor(M.live_mask(L, clips, T).reshape(-1, 1))
    x, r, gamma, beta = T64(inp.x), T64(inp.r), T64(inp.gamma), T64(inp.beta)
    s = x + r * tconst(f)
    y = torch.nn.functional.layer_norm(s, (W,), gamma, beta, E.EPS)
    close64(torch.where(m, y, 0.0).detach(), fwd.y, "y")
    close64(torch.where(m, s, 0.0).detach(), fwd.sum, "sum")
    bwd = E.ln_backward(inp.dy, fwd.sum, inp.gamma, fwd.stats, inp.dres, T, L)
    ((torch.where(m, y, 0.0) * tconst(inp.dy)).sum() + (torch.where(m, s, 0.0) * tconst(inp.dres)).sum()).backward()
    close64(x.grad, bwd.dx, "dx")
    close64(r.grad, D.branch_grad(bwd.dx, f, T, L), "dr = ds f")


@pytest.mark.parametrize("option", sorted(OPTIONS))
@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
@pytest.mark.parametrize("layers", (1, 2))
def test_stack_reference_is_torch_autograd(layers, lens, option):
    """Stack level: each option alone and all three together, with and without lengths."""
    clips, T, d, H, F, heads = 4, 5, 10, 16, 24, 2
    rng = np.random.default_rng([layers, lens, len(option)])
    p = E.default_init(rng, E.param_shapes(layers, d, H, F, heads, T), perturb=0.2)
    feat = (3.0 * rng.standard_normal((clips * T, d))).astype(np.float32)
    dout = rng.standard_normal((clips * T, H))
    L = LP.lengths(clips, T) if lens else None
    dr = D.drop(seed=D.seed_of(7), node=1, clip0=4, layers=layers, **OPTIONS[option])
    out, cache = D.stack_forward(feat, p, T, layers, heads, dr, L)
    dfeat, grads = D.stack_backward(dout, cache)
    plain, _ = E.stack_forward(feat, p, T, layers, heads, L)
    assert np.abs(out - plain).max() > 1e-3, "the options change nothing"
    tp = {k: T64(v) for k, v in p.items()}
    tf = T64(feat)
    tout, tP = torch_stack(tf, tp, T, layers, heads, L, True, dr)
    close64(tout.detach(), out, "out")
    (tout * torch.tensor(dout)).sum().backward()
    close64(tf.grad, dfeat, "dfeat")
    assert set(grads) == set(p)
    for k in p:
        close64(tp[k].grad, grads[k], k)
    live = M.live_mask(L, clips, T)
    close64(np.where(live[:, None, :, None] & live[:, None, None, :], tP.detach().numpy(), 0.0), cache.blocks[-1].att.fwd.P, "P")
    # every rate 0: encoder_block_ref itself
    out0, cache0 = D.stack_forward(feat, p, T, layers, heads, D.drop(layers=layers), L)
    close64(out0, plain, "out, every rate 0")
    g0, g1 = D.stack_backward(dout, cache0)[1], E.stack_backward(dout, E.stack_forward(feat, p, T, layers, heads, L)[1])[1]
    for k in g1:
        close64(g0[k], g1[k], k + ", every rate 0")


@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
def test_plain_stack_reference_is_torch_autograd(lens):
    """sa_block plain with sa_attn_dropout: two bare layers."""
    clips, T, d, H, heads = 4, 5, 10, 16, 2
    rng = np.random.default_rng([11, lens])
    p = {}
    for l, din in enumerate((d, H)):
        for n, shp in zip(M.param_names(l), ((din, 3 * H), (3 * H,), (H, H), (H,), (heads, 2 * T - 1))):
            p[n] = (0.4 * rng.standard_normal(shp)).astype(np.float32)
    feat = rng.standard_normal((clips * T, d)).astype(np.float32)
    dout = rng.standard_normal((clips * T, H))
    L = LP.lengths(clips, T) if lens else None
    dr = D.drop(attn=0.4, seed=D.seed_of(2), layers=2)
    out, caches = D.plain_stack_forward(feat, p, T, 2, heads, dr, L)
    dfeat, grads = D.plain_stack_backward(dout, caches)
    tp, tf = {k: T64(v) for k, v in p.items()}, T64(feat)
    m2 = torch.tensor(M.live_mask(L, clips, T))
    m = m2.reshape(-1, 1)
    x = torch.where(m, tf, 0.0)
    for l in range(2):
        n = M.param_names(l)
        ctx, _ = torch_attention(x @ tp[n[0]] + tp[n[1]], tp[n[4]], clips, T, H, heads, m2, dr.weights(l, clips, heads, T))
        x = torch.where(m, ctx @ tp[n[2]] + tp[n[3]], 0.0)
    close64(x.detach(), out, "out")
    (x * torch.tensor(dout)).sum().backward()
    close64(tf.grad, dfeat, "dfeat")
    for k in p:
        close64(tp[k].grad, grads[k], k)


# ---- 2. statistics of the restatement (never of the device) ----------------------------------------------------------------------------
N_DRAWS = 1 << 20


@pytest.mark.parametrize("keep", KEEPS)
def test_kept_fraction_within_four_sigma(keep):
    for site in D.SITES:
        frac = D.kept(D.seed_of(1), D.salt_of(0, 0, site), np.arange(N_DRAWS), keep).mean()
        assert abs(frac - keep) <= 4 * math.sqrt(keep * (1 - keep) / N_DRAWS), (site, frac)


def test_streams_agree_at_chance():
    """Two sites, two layers, two nodes, two consecutive seeds, and the fc dropout's stream: pairwise agreement of the keep-0.5 masks is
    0.5 within 4 sigma at 2^20 draws."""
    from tests.fc_dropout_ref import keep_mask
    e = np.arange(N_DRAWS)
    base = D.kept(D.seed_of(9), D.salt_of(0, 0, "attn_branch"), e, 0.5)
    others = dict(site=D.kept(D.seed_of(9), D.salt_of(0, 0, "ffn_branch"), e, 0.5), weights=D.kept(D.seed_of(9), D.salt_of(0, 0, "weights"), e, 0.5),
                  path=D.kept(D.seed_of(9), D.salt_of(0, 0, "path"), e, 0.5), layer=D.kept(D.seed_of(9), D.salt_of(0, 1, "attn_branch"), e, 0.5),
                  node=D.kept(D.seed_of(9), D.salt_of(1, 0, "attn_branch"), e, 0.5), seed=D.kept(D.seed_of(10), D.salt_of(0, 0, "attn_branch"), e, 0.5),
                  fc6=keep_mask(D.seed_of(9), 0, N_DRAWS, 0.5), fc7=keep_mask(D.seed_of(9), 1, N_DRAWS, 0.5))
    for name, other in others.items():
        agree = (base == other).mean()
        assert abs(agree - 0.5) <= 4 * 0.5 / math.sqrt(N_DRAWS), (name, agree)
    salts = {D.salt_of(n, l, s) for n in range(3) for l in range(4) for s in D.SITES}
    assert len(salts) == 3 * 4 * 4 and all(D.STREAM + s != 0xFC00 + t for s in salts for t in range(64))


def test_the_linear_rule():
    p = 0.3
    want = {1: [0.7], 2: [0.85, 0.7], 3: [0.9, 0.8, 0.7]}
    for L, ks in want.items():
        got = [D.path_keep(p, l, L) for l in range(L)]
        assert got == [F32(k) for k in ks] and all(g.dtype == F32 for g in got)
    assert D.path_keep(0.0, 0, 1) == 1 and D.keep_of(0.0) == 1 and D.keep_of(0.1) == F32(0.9)


def test_counters_are_global():
    """Clips [2, 4) drawn with clip0 = 2 are clips 2 and 3 of a draw over [0, 4), at every site."""
    sd, T, W, heads = D.seed_of(4), 5, 12, 3
    assert np.array_equal(D.weight_mask(sd, 7, 2, heads, T, 0.5, clip0=2), D.weight_mask(sd, 7, 4, heads, T, 0.5)[2:])
    assert np.array_equal(D.elem_mask(sd, 7, 2, T, W, 0.5, clip0=2), D.elem_mask(sd, 7, 4, T, W, 0.5)[2 * T:])
    for branch in (0, 1):
        assert np.array_equal(D.path_mask(sd, 7, 2, branch, 0.5, clip0=2), D.path_mask(sd, 7, 4, branch, 0.5)[2:])
    both = np.stack([D.path_mask(sd, 7, 4096, br, 0.5) for br in (0, 1)])
    assert 0.4 < (both[0] == both[1]).mean() < 0.6                                   # the two branches of a layer draw separately
    f = D.branch_factor32(sd, 1, 3, 4, T, W, 0, 0.5, 0.5)
    assert f.dtype == F32 and set(np.unique(f)) <= {F32(0), F32(4)} and D.branch_factor32(sd, 1, 3, 4, T, W, 0, 1.0, 1.0).min() == 1
    assert np.array_equal(D.branch_factor(sd, 1, 3, 4, T, W, 0, 0.5, 0.5), f.astype(F64))


def test_the_engine_restates_the_same_definition():
    from vltf_amd import ops
    from vltf_amd.engine import SaDrop, dropout_seed, sa_keep, sa_path_keep
    assert ops.SA_DROP_STREAM == D.STREAM and ops.SA_DROP_SITES == D.SITES
    for node, layer, site in ((0, 0, "weights"), (3, 5, "path"), (1, 1023, "ffn_branch")):
        assert ops.sa_drop_salt(node, layer, site) == D.salt_of(node, layer, site)
    assert dropout_seed(12) == D.seed_of(12)
    for rate in (0.0, 0.1, 0.5, 1 / 3):
        assert sa_keep(rate) == float(D.keep_of(rate))
        for L in (1, 2, 3):
            assert [sa_path_keep(rate, l, L) for l in range(L)] == [float(D.path_keep(rate, l, L)) for l in range(L)]
    d = SaDrop.plan(0.1, None, 0.2, 2, node=3).bind(4, seed=9)
    assert d.branch and d.branch_kw(1, 1) == dict(keep=1.0, keep_path=float(D.path_keep(0.2, 1, 2)), salt_elem=D.salt_of(3, 1, "ffn_branch"),
                                                  salt_path=D.salt_of(3, 1, "path"), branch=1, clip0=4, seed=9, state=None)
    assert d.weights_kw(0) == dict(keep=float(D.keep_of(0.1)), salt=D.salt_of(3, 0, "weights"), clip0=4, seed=9, state=None)


# ---- 3. host logic -------------------------------------------------------------------------------------------------------------------------
def cfgs(**kw):
    from vltf_amd.engine import NetConfig
    base = dict(image_shape=(67, 67, 3), num_classes=7, fpc=3, lstm_hidden=16, lstm_layers=2, fusion="avg", rnn_cell="mhsa", sa_heads=2,
                sa_block="encoder")
    base.update(kw)
    return NetConfig(**base)


def test_defaults_and_the_planned_variables_and_buffers():
    """Absent, None and 0 are off: the variable list and the buffer set are those of a model without the keys; with a rate on, the
    variables stay and the only new buffers are do / dm per layer, in training, for the branch options."""
    from vltf_amd.engine import NetConfig, SaDrop, encoder_buffers, param_specs, sa_drop_of
    assert (NetConfig().sa_attn_dropout, NetConfig().sa_dropout, NetConfig().sa_drop_path, NetConfig().sa_drop_salt) == (None, None, None, 0)
    base = param_specs(cfgs())
    off = [dict(), dict(sa_attn_dropout=None, sa_dropout=None, sa_drop_path=None), dict(sa_attn_dropout=0, sa_dropout=0.0, sa_drop_path=0)]
    on = dict(sa_attn_dropout=0.1, sa_dropout=0.2, sa_drop_path=0.3)
    for kw in off + [on]:
        assert param_specs(cfgs(**kw)) == base
    assert param_specs(cfgs(sa_block=None, lstm_layers=1, sa_attn_dropout=0.1)) == param_specs(cfgs(sa_block=None, lstm_layers=1))
    for kw in off:
        assert sa_drop_of(cfgs(**kw), 2) is None
    assert SaDrop.plan(None, 0, 0.0, 2) is None

    def plan(training, drop):
        made = []

        def buf(*shape, **kw):
            made.append(shape)
            return len(made)
        e = encoder_buffers(buf, 12, 3, 16, 32, 2, "relative", 2, training, drop)
        return {k: v for k, v in e.items() if k != "layers"}, [sorted(S) for S in e["layers"]], made
    today = plan(True, None)
    d = sa_drop_of(cfgs(**on), 2)
    assert (d.attn, d.elem, d.path, d.layers, d.node, d.branch) == (0.1, 0.2, 0.3, 2, 0, True)
    assert plan(False, d) == plan(False, None)                                        # forward-only engines: nothing new
    assert plan(True, sa_drop_of(cfgs(sa_attn_dropout=0.1), 2)) == today              # the weights' dropout needs no buffer
    top, layers, made = plan(True, d)
    assert top == today[0] and [sorted(set(S) - {"do", "dm"}) for S in layers] == today[1] and all({"do", "dm"} <= set(S) for S in layers)
    assert len(made) == len(today[2]) + 4 and made.count((12, 16)) == today[2].count((12, 16)) + 4


def test_refusals_by_message():
    from vltf_amd._ffi import VltfError
    from vltf_amd.engine import check_mhsa, check_sa_block, param_specs
    from vltf_amd.graph import DatasetInfo, PipelineSpec, model_specs
    keys = ("sa_attn_dropout", "sa_dropout", "sa_drop_path")
    for k in keys:
        for cell in ("lstm", "gru"):
            with pytest.raises(VltfError, match="%s is a key of rnn_cell mhsa, but the cell is \\[%s\\]" % (k, cell)):
                param_specs(cfgs(rnn_cell=cell, sa_heads=None, sa_block=None, **{k: 0.1}))
        for bad in (True, False, "0.1", float("nan"), -0.1, 1.0, 1.5, [0.1]):
            with pytest.raises(VltfError, match="%s must be a rate in \\[0, 1\\)" % k):
                param_specs(cfgs(**{k: bad}))
            with pytest.raises(VltfError, match="%s must be a rate" % k):
                check_mhsa("mhsa", 16, 3, 2, sa_block="encoder", **{k: bad})
    for k in keys[1:]:
        for block in (None, "plain"):
            with pytest.raises(VltfError, match="%s is a key of sa_block encoder, but the block is \\[plain\\]" % k):
                param_specs(cfgs(sa_block=block, **{k: 0.1}))
        with pytest.raises(VltfError, match="%s is a key of sa_block encoder" % k):
            check_sa_block("mhsa", 16, None, None, **{k: 0.1})
    assert check_mhsa("mhsa", 16, 3, 2, sa_attn_dropout=0.5) == (2, "relative")      # the weights' dropout works with the plain layer
    assert check_mhsa("mhsa", 16, 3, 2, sa_block="encoder", sa_attn_dropout=0.999, sa_dropout=0, sa_drop_path=np.float32(0.5)) == (2, "relative")
    assert check_sa_block("mhsa", 16, "encoder", 24, 0.1, 0.2) == 24
    ds = {"main": DatasetInfo("vectors", 3, 1, 4, dim=10)}
    pipe = lambda **kw: [PipelineSpec("net", ["main"], "nop", classifier="lstm", lstm_params=(16, 1, "avg"), **kw)]
    with pytest.raises(VltfError, match="sa_dropout is a key of rnn_cell mhsa"):
        model_specs(pipe(sa_dropout=0.1), ds, 5)
    with pytest.raises(VltfError, match="sa_drop_path is a key of sa_block encoder"):
        model_specs(pipe(rnn_cell="mhsa", sa_heads=2, sa_drop_path=0.1), ds, 5)
    with pytest.raises(VltfError, match="sa_attn_dropout must be a rate"):
        model_specs(pipe(rnn_cell="mhsa", sa_heads=2, sa_attn_dropout=1.0), ds, 5)
    enc = dict(rnn_cell="mhsa", sa_heads=2, sa_block="encoder", sa_ffn_dim=24)
    assert model_specs(pipe(sa_attn_dropout=0.1, sa_dropout=0.1, sa_drop_path=0.1, **enc), ds, 5) == model_specs(pipe(**enc), ds, 5)


AVG16 = [16, 1, "defs.fusion_method.avg"]


def test_the_yaml_keys(tmp_path):
    from vltf_amd import run_task
    folder = str(tmp_path)
    data_path, _, _ = make_dataset(folder, "train.txt")
    mh = dict(lstm_params=AVG16, rnn_cell="mhsa", sa_heads=2)
    enc = dict(sa_block="encoder", sa_ffn_dim=24, **mh)
    s, feeder = settings_for(folder, data_path, lambda p, r: p.update(sa_attn_dropout=0.1, sa_dropout=0.2, sa_drop_path=0.3, **enc), "drop.yml")
    p = s.pipelines["lrcn"]
    assert (p.sa_attn_dropout, p.sa_dropout, p.sa_drop_path) == (0.1, 0.2, 0.3)
    cfg, _ = run_task.net_config(s, feeder.get_dataset_by_tag("main")[0])
    assert (cfg.sa_attn_dropout, cfg.sa_dropout, cfg.sa_drop_path, cfg.sa_block) == (0.1, 0.2, 0.3, "encoder")
    specs, _, _ = run_task.graph_config(s, feeder, 2)
    assert (specs[0].sa_attn_dropout, specs[0].sa_dropout, specs[0].sa_drop_path) == (0.1, 0.2, 0.3)
    s, _ = settings_for(folder, data_path, lambda p, r: p.update(sa_attn_dropout=0.25, **mh), "plain.yml")
    assert (s.pipelines["lrcn"].sa_attn_dropout, s.pipelines["lrcn"].sa_dropout, s.pipelines["lrcn"].sa_drop_path) == (0.25, None, None)
    for extra in (dict(), dict(sa_attn_dropout=0, sa_dropout=0.0, sa_drop_path=0), dict(sa_attn_dropout="None", sa_dropout=None, sa_drop_path="None")):
        s, feeder = settings_for(folder, data_path, lambda p, r: p.update(**enc, **extra), "off.yml")
        p = s.pipelines["lrcn"]
        assert (p.sa_attn_dropout, p.sa_dropout, p.sa_drop_path) == (None, None, None)
        cfg, _ = run_task.net_config(s, feeder.get_dataset_by_tag("main")[0])
        assert (cfg.sa_attn_dropout, cfg.sa_dropout, cfg.sa_drop_path) == (None, None, None)
    for match, edit in (("sa_attn_dropout is a key of rnn_cell mhsa", lambda p, r: p.update(sa_attn_dropout=0.1)),
                        ("sa_dropout is a key of rnn_cell mhsa", lambda p, r: p.update(rnn_cell="gru", sa_dropout=0.1)),
                        ("sa_dropout is a key of sa_block encoder", lambda p, r: p.update(sa_dropout=0.1, **mh)),
                        ("sa_drop_path is a key of sa_block encoder", lambda p, r: p.update(sa_block="plain", sa_drop_path=0.1, **mh)),
                        ("sa_drop_path must be a rate", lambda p, r: p.update(sa_drop_path=1.0, **enc)),
                        ("sa_dropout must be a rate", lambda p, r: p.update(sa_dropout=True, **enc)),
                        ("sa_attn_dropout must be a rate", lambda p, r: p.update(sa_attn_dropout="high", **enc)),
                        ("sa_attn_dropout must be a rate", lambda p, r: p.update(sa_attn_dropout=-0.5, **enc))):
        with pytest.raises(Exception, match=match):
            settings_for(folder, data_path, edit, "bad.yml")


def test_the_example_parses(tmp_path):
    from vltf_amd import run_task
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "examples", "lrcn_encoder_dropout.yml")) as f:
        cfg = yaml.safe_load(f)
    p = cfg["run"]["network"]["pipelines"][0]["lrcn"]
    assert p["lstm_params"] == [256, 2, "defs.fusion_method.avg"] and p["classifier"] == "defs.classifier.lstm"
    assert (p["rnn_cell"], p["sa_heads"], p["sa_block"], p["sa_ffn_dim"]) == ("mhsa", 4, "encoder", 1024)
    assert (p["sa_attn_dropout"], p["sa_dropout"], p["sa_drop_path"]) == (0.1, 0.1, 0.1)
    assert cfg["run"]["run_id"] == "lrcn_encoder_dropout"
    # ... and through the settings to the expected NetConfig / PipelineSpec
    folder = str(tmp_path)
    data_path, _, _ = make_dataset(folder, "train.txt")
    keys = ("lstm_params", "rnn_cell", "sa_heads", "sa_positions", "sa_block", "sa_ffn_dim", "sa_attn_dropout", "sa_dropout", "sa_drop_path")
    s, feeder = settings_for(folder, data_path, lambda q, r: q.update({k: p[k] for k in keys}), "example.yml")
    nc, _ = run_task.net_config(s, feeder.get_dataset_by_tag("main")[0])
    want = dict(rnn_cell="mhsa", lstm_hidden=256, lstm_layers=2, sa_heads=4, sa_positions="relative", sa_block="encoder", sa_ffn_dim=1024,
                sa_attn_dropout=0.1, sa_dropout=0.1, sa_drop_path=0.1)
    assert {k: getattr(nc, k) for k in want} == want
    spec = run_task.graph_config(s, feeder, 2)[0][0]
    assert {k: getattr(spec, k) for k in want if hasattr(spec, k)} == {k: v for k, v in want.items() if hasattr(spec, k)}
    assert (spec.sa_attn_dropout, spec.sa_dropout, spec.sa_drop_path) == (0.1, 0.1, 0.1)


# ---- 4. float32 decides the tolerance class ----------------------------------------------------------------------------------------------
def test_float32_decides_the_class_of_the_gpu_tests():
    """The plain float32 restatement (dt = float32) of the dropped launches against fp64 on the GPU test's own inputs: the attention
    cases at keep 0.5 / 0.9, with and without lengths and positions (the backward from the reference's P rounded to fp32); the add-and-norm
    over LN_CASES at both scales, the three option sets, with and without lengths.  Worst error / bound at class act (3e-5, 3e-5) per
    output; stats per column.  Everything stays below 0.5 of class act -- the factors (up to 4) scale value and error alike -- so the GPU
    tests take class act throughout.  The ratios are printed."""
    worst = {}

    def note(name, got, want, where):
        r = ratio_of(got, want)
        worst[name] = max(worst.get(name, 0.0), r)
        assert r <= 0.5, "%s at %s: error / bound %.3f" % (name, where, r)
    for case in ATTN_CASES:
        b, T, H, heads = case
        for keep in KEEPS:
            for lens in (False, True):
                for positions in (True, False):
                    ref = attn_reference(case, keep, lens, positions)
                    inp, pos = ref["inp"], ref["inp"].pos if positions else None
                    Fw32 = D.weight_factor(SEED, SALT_W, b, heads, T, keep, CLIP0, dt=F32)
                    fwd = D.attn_forward(inp.qkv, pos, heads, Fw32, ref["lens"], T, dt=F32)
                    bwd = D.attn_backward(inp.dctx, inp.qkv, ref["P32"], heads, Fw32, ref["lens"], T, positions, dt=F32)
                    assert fwd.ctx.dtype == F32 and bwd.dqkv.dtype == F32
                    where = "%s keep %s lens %s positions %s" % (case, keep, lens, positions)
                    note("P", fwd.P, ref["fwd"].P, where)
                    note("ctx", fwd.ctx, ref["fwd"].ctx, where)
                    note("dqkv", bwd.dqkv, ref["bwd"].dqkv, where)
                    if positions:
                        note("dposp", bwd.dposp, ref["bwd"].dposp, where)
    for case in E.LN_CASES:
        clips, T, W = case
        for scale in E.SCALES:
            for lens in (False, True):
                for option in ("elem", "path", "all"):
                    ref = ln_reference(case, scale, lens, option)
                    inp = ref["inp"]
                    fwd = D.ln_drop_forward(inp.x, inp.r, ref["f32"], inp.gamma, inp.beta, T, ref["lens"], dt=F32)
                    where = "%s scale %d lens %s %s" % (case, scale, lens, option)
                    assert fwd.y.dtype == F32 and np.array_equal(fwd.sum, ref["sum32"]), where       # the plain restatement IS the bitwise one
                    note("y", fwd.y, ref["fwd"].y, where)
                    note("sum", fwd.sum, ref["fwd"].sum, where)
                    note("mean", fwd.stats[:, 0], ref["fwd"].stats[:, 0], where)
                    note("rstd", fwd.stats[:, 1], ref["fwd"].stats[:, 1], where)
                    note("dr", ref["dr32"], D.branch_grad(inp.dy, ref["f"], T, ref["lens"]), where)
    print("dropped launches in float32, worst error / bound:", " ".join("%s %.3f" % kv for kv in sorted(worst.items())))


# the references the GPU tests share (computed once per process)
SEED, SALT_W, SALT_E, SALT_P, CLIP0 = D.seed_of(5), D.salt_of(1, 2, "weights"), D.salt_of(1, 2, "attn_branch"), D.salt_of(1, 2, "path"), 3
LN_OPTIONS = dict(elem=(0.5, 1.0), path=(1.0, 0.5), all=(0.5, 0.5))                     # (keep, keep_path): the factors reach 4
_CACHE = {}


def attn_reference(case, keep, lens, positions):
    key = ("attn", case, keep, lens, positions)
    if key not in _CACHE:
        b, T, H, heads = case
        inp = M.inputs(b, T, H, heads)
        L = LP.lengths(b, T) if lens else None
        pos = inp.pos if positions else None
        Fw = D.weight_factor(SEED, SALT_W, b, heads, T, keep, CLIP0)
        fwd = D.attn_forward(inp.qkv, pos, heads, Fw, L, T)
        P32 = LP.rounded(fwd.P)
        _CACHE[key] = dict(inp=inp, lens=L, fwd=fwd, P32=P32, bwd=D.attn_backward(inp.dctx, inp.qkv, P32, heads, Fw, L, T, positions))
    return _CACHE[key]


def ln_reference(case, scale, lens, option, branch=1):
    key = ("ln", case, scale, lens, option, branch)
    if key not in _CACHE:
        clips, T, W = case
        inp = E.ln_inputs(clips, T, W, scale)
        L = LP.lengths(clips, T) if lens else None
        keep, keep_path = LN_OPTIONS[option]
        args = (SEED, SALT_E, SALT_P, clips, T, W, branch, keep, keep_path, CLIP0)
        f, f32 = D.branch_factor(*args), D.branch_factor32(*args)
        _CACHE[key] = dict(inp=inp, lens=L, f=f, f32=f32, fwd=D.ln_drop_forward(inp.x, inp.r, f, inp.gamma, inp.beta, T, L),
                           sum32=D.drop_sum32(inp.x, inp.r, f32, T, L), dr32=D.branch_grad32(inp.dy, f32, T, L), keep=keep, keep_path=keep_path)
    return _CACHE[key]
