"""The GRU classifier without a GPU: tests/gru_ref.py against torch.nn.GRU in fp64 (the independent oracle: outputs and every gradient,
one and two layers, with and without h0, through the z|r|n <-> r|z|n permutation), the dead-row contract of the reference, the float32
error of the candidate's raw dot product (which decides hcand's tolerance class in tests/test_gru_gpu.py), and the host plumbing:
variable names and shapes, decay / trust-ratio classes, initialisation, the YAML key with every refusal, checkpoint names."""
import os

import numpy as np
import pytest
import torch
import yaml

from tests import gru_ref as R
from tests import lstm_plan as P
from tests.test_host_workflow import config, make_dataset

F64 = np.float64
CUS = 256                                                        # the device the case lists are written for (any count gives valid cases)


# ---- the reference against torch.nn.GRU ----------------------------------------------------------------------------------------------------
def torch_gru(params, d, H, layers):
    """torch.nn.GRU in fp64 holding `params` (gru_ref.param_names), gates permuted to torch's r | z | n, weights transposed."""
    m = torch.nn.GRU(d, H, num_layers=layers, batch_first=True).double()
    with torch.no_grad():
        for l in range(layers):
            K, U, b, rb = (params[n] for n in R.param_names(l))
            for name, v in (("weight_ih", R.to_torch_gates(K, H).T), ("weight_hh", R.to_torch_gates(U, H).T), ("bias_ih", R.to_torch_gates(b, H)),
                            ("bias_hh", R.to_torch_gates(rb, H))):
                getattr(m, "%s_l%d" % (name, l)).copy_(torch.tensor(np.ascontiguousarray(v), dtype=torch.float64))
    return m


def stack_params(rng, d, H, layers):
    p = {}
    for l in range(layers):
        K, U, b, rb = R.param_names(l)
        p[K], p[U] = rng.standard_normal((d if l == 0 else H, 3 * H)) * 0.4, rng.standard_normal((H, 3 * H)) * 0.4
        p[b], p[rb] = rng.standard_normal(3 * H) * 0.5, rng.standard_normal(3 * H) * 0.5
    return p


@pytest.mark.parametrize("with_h0", (False, True), ids=("zero-state", "h0"))
@pytest.mark.parametrize("layers", (1, 2))
def test_the_reference_is_torch_gru_in_fp64(layers, with_h0):
    """Outputs, dx, dh0 and all four parameter gradients of every layer to 1e-12."""
    B, T, d, H = 3, 5, 7, 6
    rng = np.random.default_rng(layers + 10 * with_h0)
    p = stack_params(rng, d, H, layers)
    x, dout = rng.standard_normal((B * T, d)), rng.standard_normal((B * T, H))
    h0 = [rng.standard_normal((B, H)) * 0.5 if with_h0 else None for _ in range(layers)]
    # ours: layer by layer (stack_forward takes no h0; the layer functions do)
    xin, caches = x, []
    for l in range(layers):
        K, U, b, rb = (p[n] for n in R.param_names(l))
        xin, c = R.layer_forward(xin, K, U, b, rb, T, H, h0=h0[l])
        caches.append(c)
    out, g, dh0, d_ = xin, {}, [None] * layers, dout
    for l in reversed(range(layers)):
        d_, dK, dU, db, drb, dh0[l] = R.layer_backward(d_, caches[l])
        g.update(zip(R.param_names(l), (dK, dU, db, drb)))
    # torch
    m = torch_gru(p, d, H, layers)
    tx = torch.tensor(x.reshape(B, T, d), requires_grad=True)
    th0 = torch.tensor(np.stack(h0), requires_grad=True) if with_h0 else None
    tout, _ = m(tx, th0)
    tout.backward(torch.tensor(dout.reshape(B, T, H)))
    tol = dict(rtol=0, atol=1e-12)
    np.testing.assert_allclose(out, tout.detach().numpy().reshape(B * T, H), **tol)
    np.testing.assert_allclose(d_, tx.grad.numpy().reshape(B * T, d), **tol)
    for l in range(layers):
        K, U, b, rb = R.param_names(l)
        for ours, theirs, tr in ((K, "weight_ih", True), (U, "weight_hh", True), (b, "bias_ih", False), (rb, "bias_hh", False)):
            tg = getattr(m, "%s_l%d" % (theirs, l)).grad.numpy()
            np.testing.assert_allclose(g[ours], R.to_torch_gates(tg.T if tr else tg, H), err_msg=ours, **tol)
        if with_h0:
            np.testing.assert_allclose(dh0[l], th0.grad.numpy()[l], **tol)


def test_a_short_clip_in_a_longer_batch_is_the_short_model():
    """A clip of length L in a T-step batch gives what an L-step torch.nn.GRU gives; dead rows are zero; NaN in the dead rows of gx and
    dout does not spread."""
    B, T, d, H = 4, 6, 5, 4
    rng = np.random.default_rng(3)
    p = stack_params(rng, d, H, 1)
    K, U, b, rb = (p[n] for n in R.param_names(0))
    x, dout, h0 = rng.standard_normal((B * T, d)), rng.standard_normal((B * T, H)), rng.standard_normal((B, H)) * 0.5
    lens = np.array([6, 3, 0, 1], np.int32)
    live = R.live_mask(lens, B, T).reshape(-1)
    gx = R.with_nan_in_dead_rows(x @ K + b, T, lens)
    fwd = R.forward_ref(gx, U, T, rb, h0, lens)
    bwd = R.backward_ref(R.with_nan_in_dead_rows(dout, T, lens), U, T, fwd.act, fwd.hcand, fwd.hprev, lens)
    for a in fwd + bwd:
        assert np.isfinite(a).all()
    for a in (fwd.act, fwd.hcand, fwd.hseq, bwd.dgx, bwd.dgh):
        assert not a[~live].any() and a[live].any()
    m = torch_gru(p, d, H, 1)
    for c, L in enumerate(lens):
        hp = fwd.hprev.reshape(B, T, H)[c]
        np.testing.assert_array_equal(hp[0], h0[c])
        if L == 0:
            assert not bwd.dh0[c].any() and (hp == h0[c]).all()                                   # the carried h is h0 throughout
            continue
        tx = torch.tensor(x.reshape(B, T, d)[c:c + 1, :L], requires_grad=True)
        th0 = torch.tensor(h0[None, c:c + 1], requires_grad=True)
        tout, tn = m(tx, th0)
        tout.backward(torch.tensor(dout.reshape(B, T, H)[c:c + 1, :L]))
        np.testing.assert_allclose(fwd.hseq.reshape(B, T, H)[c, :L], tout.detach().numpy()[0], rtol=0, atol=1e-12)
        np.testing.assert_allclose(bwd.dh0[c], th0.grad.numpy()[0, 0], rtol=0, atol=1e-12)
        np.testing.assert_allclose((bwd.dgx.reshape(B, T, 3 * H)[c] @ K.T)[:L], tx.grad.numpy()[0], rtol=0, atol=1e-12)
        if L < T:
            np.testing.assert_allclose(hp[L:], np.broadcast_to(tn.detach().numpy()[0, 0], (T - L, H)), rtol=0, atol=1e-12)   # carried


def test_the_reference_backward_reads_what_it_is_given():
    """backward_ref runs from act / hcand / hprev AS GIVEN (the fp32 rounding in `reference`), not from a forward of its own."""
    ref = R.reference(3, 4, 20)
    assert ref.act32.dtype == np.float32 and ref.bwd.dgx.shape == (12, 60) and ref.bwd.dh0.shape == (3, 20)
    exact = R.backward_ref(ref.inp.dout, ref.inp.rk, 4, ref.fwd.act, ref.fwd.hcand, ref.fwd.hprev)
    assert 0 < np.abs(exact.dgx - ref.bwd.dgx).max() < 1e-5


def test_hcand_in_float32_stays_inside_dgx_tolerance_class():
    """hcand = hprev @ U_n + b is a raw dot product with no tolerance class of its own.  A float32 numpy evaluation of it, from the fp32
    rounding of the reference's hprev, stays inside dgx's class (rtol 1e-5, atol 1e-6 of the largest element) against fp64 at every case
    of tests/test_gru_gpu.py, so hcand takes that class there.  Measured worst error / bound over the cases at 256 compute units: 0.193 (printed below)."""
    rtol, atol_rel = 1e-5, 1e-6
    worst = 0.0
    for case in R.CASES + [P.Case("3*mg", 3, 498)]:
        batch, T, H = P.resolve(case, CUS)
        for lens in (False, True):
            ref = R.reference(batch, T, H, lens=lens)
            live = R.live_mask(ref.lens, batch, T).reshape(-1)
            got = ref.hprev32 @ ref.inp.rk[:, 2 * H:] + ref.inp.rb[2 * H:]
            assert got.dtype == np.float32
            want = ref.fwd.hcand
            bound = atol_rel * np.abs(want).max() + rtol * np.abs(want)
            worst = max(worst, float((np.abs(got.astype(F64) - want)[live] / bound[live]).max()) if live.any() else 0.0)
    print("hcand in float32: worst error / bound %.3f" % worst)
    assert worst < 1.0, worst


# ---- host plumbing -----------------------------------------------------------------------------------------------------------------------------
def cfgs(**kw):
    from vltf_amd.engine import NetConfig
    base = dict(image_shape=(67, 67, 3), num_classes=7, fpc=3, lstm_hidden=8, lstm_layers=2, rnn_cell="gru")
    base.update(kw)
    return NetConfig(**base)


def test_param_specs_names_shapes_and_order():
    from vltf_amd.engine import gru_names, param_specs
    specs = param_specs(cfgs())
    H, D, C = 8, 4096, 7
    want = [("output_fc_w", (H, C)), ("output_fc_b", (C,))]
    for l, d in ((0, D), (1, H)):
        pre = "rnn/multi_rnn_cell/cell_%d/gru_cell/" % l
        want += [(pre + "kernel", (d, 3 * H)), (pre + "recurrent_kernel", (H, 3 * H)), (pre + "bias", (3 * H,)), (pre + "recurrent_bias", (3 * H,))]
    assert specs[:len(want)] == want
    assert [n for n, _ in want[2:6]] == gru_names(0) == R.param_names(0)
    assert specs[len(want):] == param_specs(cfgs(classifier="none", rnn_cell="lstm"))        # the tower's, untouched
    assert param_specs(cfgs(fusion="state"))[0] == ("fc_convert_w", (H, C))
    assert param_specs(cfgs(lstm_hidden=7))[0][0] == gru_names(0)[0]                          # H == C: no head
    # without the key: today's list
    lstm = param_specs(cfgs(rnn_cell="lstm"))
    from vltf_amd.engine import NetConfig
    assert NetConfig().rnn_cell == "lstm" and not any("gru" in n for n, _ in lstm)
    assert lstm[2] == ("rnn/multi_rnn_cell/cell_0/basic_lstm_cell/kernel", (D + H, 4 * H))


def test_initialisation_decay_and_trust_ratio_classes():
    """Kernels glorot-uniform, both biases zero; decay_ranges gives both biases coefficient 0 and both kernels the decay; LARS and LAMB
    trust-scale the kernels only."""
    from vltf_amd.engine import decay_ranges, finetune_plan, init_params, lamb_ranges, lars_ranges, param_specs
    cfg = cfgs(lr_mult=10.0, train_from="classifier")
    specs = param_specs(cfg)
    p = init_params(cfg, seed=1)
    offs, off = {}, 0
    for n, s in specs:
        offs[n] = (off, off + int(np.prod(s)))
        off += int(np.prod(s))
    names = R.param_names(0) + R.param_names(1)
    for n in names:
        if n.endswith("bias"):
            assert not p[n].any() and p[n].ndim == 1
        else:
            lim = np.sqrt(6.0 / sum(p[n].shape))
            assert p[n].std() > 0 and np.abs(p[n]).max() <= lim and p[n].ndim == 2
    plan = finetune_plan(cfg)
    inside = lambda rng, lo, hi: any(a <= lo and hi <= b for a, b in rng)
    ranges = decay_ranges(specs, plan, 5e-4)
    decayed, plain = [(a, b) for a, b, c in ranges if c > 0], [(a, b) for a, b, c in ranges if c == 0]
    lars, _, _ = lars_ranges(specs, plan, 0.0)
    lamb, _ = lamb_ranges(specs, plan, 0.0)
    for n in names:
        lo, hi = offs[n]
        if n.endswith("kernel"):
            assert inside(decayed, lo, hi) and (lo, hi) in [(a, b) for a, b, _, t in lars if t >= 0] and (lo, hi) in [(r[0], r[1]) for r in lamb if r[4] >= 0]
        else:
            assert inside(plain, lo, hi) and not inside(decayed, lo, hi), n
            assert inside([(a, b) for a, b, _, t in lars if t < 0], lo, hi) and inside([(r[0], r[1]) for r in lamb if r[4] < 0], lo, hi)


def test_engine_specs_and_refusals():
    from vltf_amd._ffi import VltfError
    from vltf_amd.composed import ComposedEngine, HeadConfig
    from vltf_amd.engine import param_specs
    from vltf_amd.graph import DatasetInfo, PipelineSpec, model_specs
    H, C, dim, T = 6, 5, 10, 4
    ds = {"main": DatasetInfo("vectors", T, 1, 3, dim=dim), "aux": DatasetInfo("vectors", 1, 1, 3, dim=7)}
    spec = lambda **kw: PipelineSpec("p", ["main"], "nop", classifier="lstm", lstm_params=(H, 2, "reshape"), **kw)
    got = model_specs([spec(rnn_cell="gru")], ds, C)
    want = [("output_fc_w", (H, C)), ("output_fc_b", (C,))]
    for l, d in ((1, H), (0, dim)):                                                        # backward order, as the LSTM list
        want += list(zip(R.param_names(l), ((d, 3 * H), (H, 3 * H), (3 * H,), (3 * H,))))
    assert got == want
    assert model_specs([spec()], ds, C) == model_specs([spec(rnn_cell="lstm")], ds, C) and PipelineSpec("p", ["main"]).rnn_cell == "lstm"
    bad = lambda **kw: PipelineSpec("p", kw.pop("input", ["main"]), "nop", **kw)
    for match, pipe in (("hidden size <= 512", bad(classifier="lstm", lstm_params=(513, 1, "avg"), rnn_cell="gru")),
                        ("lstm_bidirectional", bad(classifier="lstm", lstm_params=(H, 1, "avg"), rnn_cell="gru", lstm_bidirectional=True)),
                        ("state input", bad(input=["main", "aux"], classifier="lstm", lstm_params=(H, 1, "avg"), rnn_cell="gru")),
                        ("classifier lstm", bad(classifier="fc", rnn_cell="gru")),
                        ("classifier lstm", bad(rnn_cell="gru")),
                        ("must be lstm or gru", bad(classifier="lstm", lstm_params=(H, 1, "avg"), rnn_cell="rnn"))):
        with pytest.raises(VltfError, match=match):
            model_specs([pipe], ds, C)
    # LRCNEngine's configuration
    for match, kw in (("hidden size <= 512", dict(lstm_hidden=513)), ("lstm_bidirectional", dict(lstm_bidirectional=True)),
                      ("classifier lstm", dict(classifier="fc")), ("classifier lstm", dict(classifier="none")),
                      ("must be lstm or gru", dict(rnn_cell="GRU"))):
        with pytest.raises(VltfError, match=match):
            param_specs(cfgs(**kw))
    assert param_specs(cfgs(lstm_hidden=512))[2][1] == (4096, 1536)
    # the two-pipeline model refuses it before anything is built
    with pytest.raises(VltfError, match="not built for the two-pipeline model"):
        ComposedEngine(cfgs(), HeadConfig(in_dim=4, fpc=3, num_classes=7), 2, device="cpu")


def settings_for(folder, data_path, edit, name):
    from vltf_amd import settings_
    with open(config(folder, data_path)) as f:
        cfg = yaml.safe_load(f)
    edit(cfg["run"]["network"]["pipelines"][0]["lrcn"])
    out = os.path.join(folder, name)
    with open(out, "w") as f:
        yaml.safe_dump(cfg, f)
    s = settings_.Settings()
    return s, s.initialize(out)


def test_the_yaml_key(tmp_path):
    from vltf_amd import run_task
    folder = str(tmp_path)
    data_path, _, _ = make_dataset(folder, "train.txt")
    s, feeder = settings_for(folder, data_path, lambda p: p.update(rnn_cell="gru"), "gru.yml")
    assert s.pipelines["lrcn"].rnn_cell == "gru"
    cfg, _ = run_task.net_config(s, feeder.get_dataset_by_tag("main")[0])
    assert cfg.rnn_cell == "gru" and cfg.lstm_hidden == 8 and cfg.classifier == "lstm"
    specs, _, _ = run_task.graph_config(s, feeder, 2)
    assert specs[0].rnn_cell == "gru"
    for value in (None, "None", "lstm"):
        s, feeder = settings_for(folder, data_path, (lambda p: None) if value is None else (lambda p: p.update(rnn_cell=value)), "lstm.yml")
        assert s.pipelines["lrcn"].rnn_cell == "lstm"
        assert run_task.net_config(s, feeder.get_dataset_by_tag("main")[0])[0].rnn_cell == "lstm"
        assert run_task.graph_config(s, feeder, 2)[0][0].rnn_cell == "lstm"
    for edit in (lambda p: p.update(rnn_cell="gru", classifier="defs.classifier.fc", lstm_params=None),           # classifier fc
                 lambda p: (p.update(rnn_cell="gru"), p.pop("classifier"), p.pop("lstm_params")),                   # no classifier
                 lambda p: p.update(rnn_cell="gru", lstm_params=[513, 1, "defs.fusion_method.avg"]),                # H > 512
                 lambda p: p.update(rnn_cell="gru", lstm_bidirectional=True),                                       # bidirectional
                 lambda p: p.update(rnn_cell="rnn")):                                                               # another value
        with pytest.raises(Exception):
            settings_for(folder, data_path, edit, "bad.yml")


def test_the_yaml_key_with_a_state_input(tmp_path):
    """A second input without an input_fusion is the LSTM's state: parsed with the LSTM cell, refused with the GRU."""
    from vltf_amd import settings_
    folder = str(tmp_path)
    data_path, _, _ = make_dataset(folder, "train.txt")

    def parse(cell):
        with open(config(folder, data_path)) as f:
            cfg = yaml.safe_load(f)
        pipes = cfg["run"]["network"]["pipelines"]
        pipes.insert(0, {"enc": {"input": "defs.dataset_tag.main", "representation": "defs.representation.dcnn", "frame_encoding_layer": "fc6",
                                 "classifier": "defs.classifier.fc", "frame_fusion": ["defs.fusion_type.early", "defs.fusion_method.avg"]}})
        pipes[1]["lrcn"].update(input=["defs.dataset_tag.main", "enc"], rnn_cell=cell)
        out = os.path.join(folder, "two_%s.yml" % cell)
        with open(out, "w") as f:
            yaml.safe_dump(cfg, f)
        s = settings_.Settings()
        s.initialize(out)
        return s

    assert parse("lstm").pipelines["lrcn"].input == ["main", "enc"]
    with pytest.raises(Exception, match="state input"):
        parse("gru")


def test_the_example_parses():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "examples", "lrcn_gru.yml")) as f:
        cfg = yaml.safe_load(f)
    p = cfg["run"]["network"]["pipelines"][0]["lrcn"]
    assert p["rnn_cell"] == "gru" and p["classifier"] == "defs.classifier.lstm" and p["lstm_params"][0] <= 512


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
    """A checkpoint holds the GRU variables under their names, restores into a GRU network and is refused by an LSTM one."""
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
    assert names == {n for n, _ in saved.specs} and set(R.param_names(0) + R.param_names(1)) <= names
    assert not any("basic_lstm_cell" in n for n in names)
    s2 = settings_.Settings()
    f2 = s2.initialize(config(folder, data_path, resume_file=base))
    fresh = StubEngine(cfgs(**small), seed=2)
    f2.init_saveload(fresh, base)
    for n in saved.params:
        assert np.array_equal(fresh.params[n], saved.params[n]), n
    with pytest.raises(Exception):
        f2.init_saveload(StubEngine(cfgs(rnn_cell="lstm", **small), seed=2), base)
