"""The bidirectional LSTM on the CPU: tests/blstm_ref.py against the oracle and against itself (central differences), the restated plan
of the bidirectional cluster launch (grid, exchange slices, tag span), and the host plumbing of `lstm_bidirectional` -- variable names,
shapes and order, the (2H, C) head, decay / LARS / LAMB ranges, the lr_mult tier, the YAML key and every refusal.  No GPU: no engine is
constructed on a device."""
import os

import numpy as np
import pytest
import yaml

from oracle import lrcn_oracle as O
from tests import blstm_ref as B
from tests import lstm_plan as P
from tests import seq_len_ref as SL
from tests.test_host_workflow import config, make_dataset

F64 = np.float64


# ---- the reference itself ------------------------------------------------------------------------------------------------------------------
def layer_inputs(batch, T, H, d, seed=3):
    r = np.random.default_rng(seed)
    x = r.standard_normal((batch * T, d))
    K = tuple(r.standard_normal((d + H, 4 * H)) * 0.4 for _ in range(2))
    b = tuple(r.standard_normal(4 * H) * 0.3 for _ in range(2))
    return x, K, b, r


def test_reverse_sequence_is_tf_reverse_sequence():
    T, lens = 4, np.array([4, 2, 0, 1, 9, -2], np.int32)
    a = np.arange(6 * T * 2, dtype=F64).reshape(6 * T, 2)
    got = B.reverse_sequence(a, T, lens).reshape(6, T, 2)
    a3 = a.reshape(6, T, 2)
    for b, L in enumerate(P.clamped(lens, T)):
        assert np.array_equal(got[b, :L], a3[b, :L][::-1]) and np.array_equal(got[b, L:], a3[b, L:])
    assert np.array_equal(B.reverse_sequence(got.reshape(-1, 2), T, lens), a)                 # an involution
    assert np.array_equal(B.reverse_sequence(a, T).reshape(6, T, 2), a3[:, ::-1])


def test_full_length_backward_direction_is_the_oracle_on_the_flipped_input():
    batch, T, H, d = 3, 5, 6, 4
    x, K, b, _ = layer_inputs(batch, T, H, d)
    out, cache = B.layer_forward(x, K, b, T, H)
    x3 = x.reshape(batch, T, d)
    fw, _, _ = O.lstm_layer_forward(x3, K[0], b[0])                           # (the oracle's forget bias is the reference's 1.0)
    bw, _, _ = O.lstm_layer_forward(np.ascontiguousarray(x3[:, ::-1]), K[1], b[1])
    assert np.abs(out[:, :H].reshape(batch, T, H) - fw).max() < 1e-12
    assert np.abs(out[:, H:].reshape(batch, T, H) - bw[:, ::-1]).max() < 1e-12
    # hprev of the backward cell at time t is its output at t + 1 (zeros at the last step)
    hp = cache.fwd[1].hprev.reshape(batch, T, H)
    assert np.abs(hp[:, :-1] - bw[:, ::-1][:, 1:]).max() < 1e-12 and not hp[:, -1].any()


def test_with_lengths_the_backward_direction_is_the_length_reference_on_reverse_sequence():
    batch, T, H, d = 4, 5, 6, 3
    x, K, b, _ = layer_inputs(batch, T, H, d, seed=4)
    lens = np.array([5, 2, 1, 3], np.int32)                                   # (seq_len_ref takes lengths >= 1)
    out, _ = B.layer_forward(x, K, b, T, H, lens=lens)
    xr = B.reverse_sequence(x, T, lens).reshape(batch, T, d)
    want = SL.lstm_layer(xr, K[1], b[1], lens)
    assert np.abs(out[:, H:] - B.reverse_sequence(want["out"].reshape(batch * T, H), T, lens)).max() < 1e-12
    assert np.abs(out[:, :H] - SL.lstm_layer(x.reshape(batch, T, d), K[0], b[0], lens)["out"].reshape(batch * T, H)).max() < 1e-12
    dead = ~B.live_mask(lens, batch, T).reshape(-1)
    assert not out[dead].any()


def test_reference_backward_is_the_gradient_of_the_reference_forward():
    """Central differences in fp64 at B = 2, T = 3, H = 5, lengths (3, 2), non-zero initial states: dx, dK, db, dh0, dc0 of both cells."""
    batch, T, H, d = 2, 3, 5, 4
    x, K, b, r = layer_inputs(batch, T, H, d, seed=6)
    lens = np.array([3, 2], np.int32)
    h0 = tuple(r.standard_normal((batch, H)) * 0.5 for _ in range(2))
    c0 = tuple(r.standard_normal((batch, H)) * 0.5 for _ in range(2))
    w = r.standard_normal((batch * T, 2 * H))
    live = B.live_mask(lens, batch, T).reshape(-1)

    def loss(x, K, b, h0, c0):
        out, _ = B.layer_forward(x, K, b, T, H, h0, c0, lens)
        return float((out * w).sum())

    _, cache = B.layer_forward(x, K, b, T, H, h0, c0, lens)
    dx, dK, db, dh0, dc0 = B.layer_backward(B.with_nan_in_dead_rows(w, T, lens), cache)      # dead rows of dout are never read
    args = dict(x=x, K=K, b=b, h0=h0, c0=c0)
    eps = 1e-6

    def numeric(name, k):
        base = args[name] if k is None else args[name][k]
        g = np.zeros_like(base)
        for i in np.ndindex(*base.shape):
            vals = []
            for s in (eps, -eps):
                v = base.copy()
                v[i] += s
                a = dict(args)
                a[name] = v if k is None else tuple(v if j == k else args[name][j] for j in range(2))
                vals.append(loss(**a))
            g[i] = (vals[0] - vals[1]) / (2 * eps)
        return g

    assert np.abs(numeric("x", None)[live] - dx[live]).max() < 1e-7
    assert not dx[~live].any()
    for k in range(2):
        for name, got in (("K", dK), ("b", db), ("h0", dh0), ("c0", dc0)):
            assert np.abs(numeric(name, k) - got[k]).max() < 1e-7, (name, k)


def test_fusion_of_the_2h_wide_sequence():
    batch, T, H = 3, 4, 2
    out = np.arange(batch * T * 2 * H, dtype=F64).reshape(batch * T, 2 * H)
    lens = np.array([4, 2, 1], np.int32)
    o = out.reshape(batch, T, 2 * H)
    last = B.fuse(out, T, H, "last", lens)
    for b, L in enumerate(lens):
        assert np.array_equal(last[b, :H], o[b, L - 1, :H]) and np.array_equal(last[b, H:], o[b, 0, H:])
    assert np.array_equal(B.fuse(out, T, H, "state"), np.concatenate([o[:, T - 1, :H], o[:, 0, H:]], axis=1))
    assert np.allclose(B.fuse(out, T, H, "avg", lens)[1], o[1, :2].mean(axis=0))
    d = np.ones((batch, 2 * H))
    g = B.fuse_backward(d, T, H, "last", lens).reshape(batch, T, 2 * H)
    assert g[1, 1, :H].all() and g[1, 0, H:].all() and g.sum() == batch * 2 * H


# ---- the plan ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cus", (256, 304, 64))
@pytest.mark.parametrize("H", (1, 37, 250, 256, 498, 512))
def test_the_bidirectional_plan(cus, H):
    mg = B.mg_bi(H, cus)
    assert mg >= 1 and 2 * mg <= P.max_groups(H, cus)
    T = 3
    words = (P.ws_bytes(H, cus) - P.STATUS_BYTES) // 8
    for batch in (1, mg, mg + 1, 8 * mg, 8 * mg + 1, 20 * mg + 3):
        plan = B.bi_plan(batch, T, H, cus)
        assert sum(l.nb for l in plan.launches) == batch and all(l.nb <= plan.chunk for l in plan.launches)
        assert B.tag_span(batch, T, H, cus) == len(plan.launches) * (T + 1)
        for l in plan.launches:
            assert l.grid == 2 * l.G * plan.W <= cus and l.G <= mg                       # every workgroup resident: one per CU
            assert all(1 <= g.nclips <= P.CPG for g in l.groups) and sum(g.nclips for g in l.groups) == l.nb
            for bwd in (False, True):
                spans = sorted(s for v in B.exchange_slices(plan, l, bwd).values() for s in v)
                assert len(spans) == 4 * l.G
                assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "exchange slices overlap"
                assert spans[0][0] >= 0 and spans[-1][1] <= words, "exchange slices leave the workspace"
    # one clip per group in both plans up to mg clips: the forward half can equal the unidirectional launch bit for bit
    for batch in range(1, mg + 1):
        assert P.group_sizes(P.cluster_plan(batch, T, H, cus)) == [[g.nclips for g in B.bi_plan(batch, T, H, cus).launches[0].groups]] == [[1] * batch]


def test_the_benchmark_geometry_fills_the_device_once():
    plan = B.bi_plan(64, 16, 256, 256)
    assert [(l.G, l.cpg, l.grid) for l in plan.launches] == [(8, 8, 256)]
    assert B.tag_span(64, 16, 512, 4 * 16) == 0 or B.mg_bi(512, 64) >= 1
    assert B.mg_bi(512, 32) == 0 and B.tag_span(4, 3, 512, 32) == 0 and B.tag_span(4, 3, 513, 256) == 0


# ---- host plumbing ---------------------------------------------------------------------------------------------------------------------------
def cfgs(**kw):
    from vltf_amd.engine import NetConfig
    base = dict(image_shape=(67, 67, 3), num_classes=7, fpc=3, lstm_hidden=8, lstm_layers=2)
    base.update(kw)
    return NetConfig(**base)


def test_param_specs_names_shapes_and_order():
    from vltf_amd.engine import blstm_names, param_specs
    cfg = cfgs(lstm_bidirectional=True)
    specs = param_specs(cfg)
    H, D, C = 8, 4096, 7
    want = [("output_fc_w", (2 * H, C)), ("output_fc_b", (C,))]
    for l, d in ((0, D), (1, 2 * H)):
        pre = "bidirectional_rnn/%s/multi_rnn_cell/cell_%d/basic_lstm_cell/"
        want += [(pre % ("fw", l) + "kernel", (d + H, 4 * H)), (pre % ("fw", l) + "bias", (4 * H,)),
                 (pre % ("bw", l) + "kernel", (d + H, 4 * H)), (pre % ("bw", l) + "bias", (4 * H,))]
    assert specs[:len(want)] == want
    assert [n for n, _ in want[2:6]] == blstm_names(0) == B.param_names(0)
    assert specs[len(want):] == param_specs(cfgs(classifier="none"))                       # the tower's, untouched
    assert param_specs(cfgs(lstm_bidirectional=True, fusion="state"))[0] == ("fc_convert_w", (2 * H, C))
    assert param_specs(cfgs(lstm_bidirectional=True, lstm_hidden=4, num_classes=8))[0][0].startswith("bidirectional_rnn/fw")   # 2H == C: no head
    # without the key: today's list
    uni = param_specs(cfgs())
    assert uni == param_specs(cfgs(lstm_bidirectional=False)) and not any("bidirectional" in n for n, _ in uni)
    assert uni[0] == ("output_fc_w", (H, C)) and uni[2][0] == "rnn/multi_rnn_cell/cell_0/basic_lstm_cell/kernel"


def test_initialisation_ranges_and_tiers():
    from vltf_amd.engine import decay_ranges, finetune_plan, init_params, is_regular, lamb_ranges, lars_ranges, param_specs
    cfg = cfgs(lstm_bidirectional=True, lr_mult=10.0, train_from="classifier")
    specs = param_specs(cfg)
    p = init_params(cfg, seed=1)
    offs, off = {}, 0
    for n, s in specs:
        offs[n] = (off, off + int(np.prod(s)))
        off += int(np.prod(s))
    names = B.param_names(0) + B.param_names(1)
    for n in names:
        assert not is_regular(n)
        if n.endswith("bias"):
            assert not p[n].any()
        else:
            lim = np.sqrt(6.0 / sum(p[n].shape))
            assert p[n].std() > 0 and np.abs(p[n]).max() <= lim
    plan = finetune_plan(cfg)
    # the classifier tier: everything from the head to the last LSTM variable trains at lr_mult; train_from classifier freezes the tower
    lstm_hi = offs[names[-1]][1]
    assert any(lo <= 0 and hi >= lstm_hi and m == 10.0 for lo, hi, m in plan.tiers)
    assert all(hi <= lstm_hi for lo, hi, m in plan.tiers), plan.tiers
    inside = lambda rng, lo, hi: any(a <= lo and hi <= b for a, b in rng)
    decayed = [(a, b) for a, b, c in decay_ranges(specs, plan, 5e-4) if c > 0]
    plain = [(a, b) for a, b, c in decay_ranges(specs, plan, 5e-4) if c == 0]
    lars, lsegs, _ = lars_ranges(specs, plan, 0.0)
    lamb, msegs = lamb_ranges(specs, plan, 0.0)
    for n in names:
        lo, hi = offs[n]
        if n.endswith("kernel"):
            assert inside(decayed, lo, hi) and (lo, hi) in [(a, b) for a, b, _, t in lars if t >= 0] and (lo, hi) in [(r[0], r[1]) for r in lamb if r[4] >= 0]
        else:
            assert inside(plain, lo, hi) and not inside(decayed, lo, hi)
            assert inside([(a, b) for a, b, _, t in lars if t < 0], lo, hi) and inside([(r[0], r[1]) for r in lamb if r[4] < 0], lo, hi)
    kernels = [n for n in names if n.endswith("kernel")]
    assert [s[0] for s in lsegs if "lstm" in s[0]] == kernels == [s[0] for s in msegs if "lstm" in s[0]] and len(kernels) == 4


def test_graph_engine_specs_and_refusals():
    from vltf_amd._ffi import VltfError
    from vltf_amd.composed import ComposedEngine, HeadConfig
    from vltf_amd.engine import param_specs
    from vltf_amd.graph import DatasetInfo, PipelineSpec, model_specs
    H, C, dim, T = 6, 5, 10, 4
    ds = {"main": DatasetInfo("vectors", T, 1, 3, dim=dim), "aux": DatasetInfo("vectors", 1, 1, 3, dim=7)}
    spec = lambda **kw: PipelineSpec("p", ["main"], "nop", classifier="lstm", lstm_params=(H, 2, "reshape"), **kw)
    for scope, pipes in (("", [spec(lstm_bidirectional=True)]),
                         ("p/", [PipelineSpec("f", ["main"], "fc", fc_output_dim=dim + 1),
                                 PipelineSpec("p", ["f"], "nop", classifier="lstm", lstm_params=(H, 2, "reshape"), lstm_bidirectional=True)])):
        got = [(n, shp) for n, shp in model_specs(pipes, ds, C) if not n.startswith("f/")]
        d0 = dim + 1 if scope else dim
        want = [(scope + "output_fc_w", (2 * H, C)), (scope + "output_fc_b", (C,))]
        for l, d in ((1, 2 * H), (0, d0)):                                                # backward order, as the unidirectional list
            want += [(n, (d + H, 4 * H) if n.endswith("kernel") else (4 * H,)) for n in B.param_names(l, scope)]
        assert got == want
    uni = model_specs([spec()], ds, C)
    assert uni == model_specs([spec(lstm_bidirectional=False)], ds, C) and not any("bidirectional" in n for n, _ in uni)
    with pytest.raises(VltfError, match="hidden size <= 512"):
        model_specs([PipelineSpec("p", ["main"], "nop", classifier="lstm", lstm_params=(513, 1, "avg"), lstm_bidirectional=True)], ds, C)
    with pytest.raises(VltfError, match="state input"):
        model_specs([PipelineSpec("p", ["main", "aux"], "nop", classifier="lstm", lstm_params=(H, 1, "avg"), lstm_bidirectional=True)], ds, C)
    with pytest.raises(VltfError, match="needs classifier lstm"):
        model_specs([PipelineSpec("p", ["main"], "nop", classifier="fc", lstm_bidirectional=True)], ds, C)
    # LRCNEngine's configuration: hidden size, classifier
    with pytest.raises(VltfError, match="hidden size <= 512"):
        param_specs(cfgs(lstm_bidirectional=True, lstm_hidden=513))
    for cls in ("fc", "none"):
        with pytest.raises(VltfError, match="needs classifier lstm"):
            param_specs(cfgs(lstm_bidirectional=True, classifier=cls))
    # the two-pipeline model refuses it before anything is built
    with pytest.raises(VltfError, match="lstm_bidirectional is not built for the two-pipeline model"):
        ComposedEngine(cfgs(lstm_bidirectional=True), HeadConfig(in_dim=4, fpc=3, num_classes=7), 2, device="cpu")


def pipeline_of(cfg_path):
    with open(cfg_path) as f:
        return yaml.safe_load(f)


def test_the_yaml_key(tmp_path):
    from vltf_amd import run_task, settings_
    folder = str(tmp_path)
    data_path, _, _ = make_dataset(folder, "train.txt")

    def settings(edit, name):
        path = config(folder, data_path)
        cfg = pipeline_of(path)
        edit(cfg["run"]["network"]["pipelines"][0]["lrcn"])
        out = os.path.join(folder, name)
        with open(out, "w") as f:
            yaml.safe_dump(cfg, f)
        s = settings_.Settings()
        return s, s.initialize(out)

    s, feeder = settings(lambda p: p.update(lstm_bidirectional=True), "bi.yml")
    p = s.pipelines["lrcn"]
    assert p.lstm_bidirectional is True
    cfg, _ = run_task.net_config(s, feeder.get_dataset_by_tag("main")[0])
    assert cfg.lstm_bidirectional is True and cfg.lstm_hidden == 8
    specs, _, _ = run_task.graph_config(s, feeder, 2)
    assert specs[0].lstm_bidirectional is True
    s, feeder = settings(lambda p: None, "uni.yml")
    assert s.pipelines["lrcn"].lstm_bidirectional is False
    assert run_task.net_config(s, feeder.get_dataset_by_tag("main")[0])[0].lstm_bidirectional is False
    s, _ = settings(lambda p: p.update(lstm_bidirectional="None"), "none.yml")
    assert s.pipelines["lrcn"].lstm_bidirectional is False
    for edit in (lambda p: p.update(lstm_bidirectional=True, classifier="defs.classifier.fc", lstm_params=None),
                 lambda p: (p.update(lstm_bidirectional=True), p.pop("classifier"), p.pop("lstm_params")),
                 lambda p: p.update(lstm_bidirectional=True, lstm_params=[513, 1, "defs.fusion_method.avg"]),
                 lambda p: p.update(lstm_bidirectional="maybe")):
        with pytest.raises(Exception):
            settings(edit, "bad.yml")


def test_the_example_parses():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "examples", "lrcn_blstm.yml")) as f:
        cfg = yaml.safe_load(f)
    p = cfg["run"]["network"]["pipelines"][0]["lrcn"]
    assert p["lstm_bidirectional"] is True and p["classifier"] == "defs.classifier.lstm"
