"""The GRU recurrence kernels (csrc/lstm_cluster.hip: gru_cluster_fwd_kernel / gru_cluster_bwd_kernel) against the fp64 reference of
tests/gru_ref.py on every branch of the launcher they share with the LSTM kernels, then the engines that run on them.

Cases (gru_ref.CASES, batches in mg = groups per launch and chunk = 8 mg): groups of one clip; a ragged launch with groups of 2 and 1; two
launches at Hp = 512 with the last clip alone in the second; W = 3 workgroups at H = 37 (gather class 1, a ragged last workgroup);
H = 250 (pad rows Hp = 252, four reduction slices with a ragged last one); H = 256; T = 1, 2, 21.  (3, 3, 250) plans three groups of ONE
clip on any device with 48 compute units or more, i.e. the 1 x 4 reduction split, not the 2 x 2 one: groups of three clips -- the 2 x 2
split and the 4-wide partial publish -- are reached by the added case ("3*mg", 3, 498).  Every case runs without and with per-clip lengths
(lstm_plan.lengths: 0, T, -3 and T + 5 among them), and with lengths the dead rows of gx and dout hold NaN.

Tolerances are the project's classes (tests/test_lstm_geometry_gpu.TOL): act (3e-5, 3e-5); hseq, hprev, dgx, dgh (1e-5, 1e-6); dh0
(1e-4, 1e-5).  hcand, a raw dot product, takes dgx's class: tests/test_gru.py shows that a float32 numpy evaluation of hprev @ U_n + b
stays inside it against fp64 at every case here.  The backward runs FROM the reference's own act, hcand and hprev rounded to fp32.

Every output is a Guarded view (sentinels around it, NaN inside beforehand), the workspace is exactly lstm_seq_ws's size in front of a
sentinel tail, and every run ends with the time-out word clear.  The time-out hooks are not exercised here: gather_granules is shared with
the LSTM kernels and covered in their tests."""
import numpy as np
import pytest
import torch

from tests import gru_ref as R
from tests import lstm_plan as P
from tests.test_lstm_geometry_gpu import DEV, Guarded, St, Workspace, cus, put, same_bits, within

pytestmark = pytest.mark.gpu

CASES = R.CASES + [P.Case("3*mg", 3, 498)]
CLASS = dict(act="act", hcand="dz", hseq="hseq", hprev="hprev", dgx="dz", dgh="dz", dh0="dh0")       # output -> tolerance class
SEQ_OUT = (("act", 3), ("hcand", 1), ("hseq", 1), ("hprev", 1), ("dgx", 3), ("dgh", 3))


@pytest.fixture(scope="module")
def ops():
    import vltf_amd.ops as ops_
    return ops_


def run_gru(ops, ref, batch, T, H, ws=None, st=None, dh0=True, what=""):
    """gru_seq_fwd on ref's inputs (NaN in the dead rows of gx and dout), gru_seq_bwd on ref's OWN act, hcand, hprev; the memory checks."""
    inp = ref.inp
    ws = ws or Workspace(ops, batch, T, H, DEV)
    nan = (lambda a: a if a is None or ref.lens is None else R.with_nan_in_dead_rows(a, T, ref.lens))
    gx, rk, rb, h0, dout = (put(a, DEV) for a in (nan(inp.gx), inp.rk, inp.rb, inp.h0, nan(inp.dout)))
    lens = put(ref.lens, DEV, torch.int32)
    o = {k: Guarded((batch * T, w * H), DEV) for k, w in SEQ_OUT}
    o["dh0"] = Guarded((batch, H), DEV)
    kw = dict(ws=ws.t, seq_len=lens) if st is None else dict(ws=ws.t, state=st.state)
    ops.gru_seq_fwd(gx, rk, o["act"].t, o["hcand"].t, o["hseq"].t, o["hprev"].t, batch, T, H, rb=rb, h0=h0,
                    **kw, **({} if st is None else dict(tag_offset=st.fwd)))
    ws.settle(ops, what + " forward")
    ops.gru_seq_bwd(dout, rk, put(ref.act32, DEV), put(ref.hcand32, DEV), put(ref.hprev32, DEV), o["dgx"].t, o["dgh"].t, batch, T, H,
                    dh0=o["dh0"].t if dh0 else None, **kw, **({} if st is None else dict(tag_offset=st.bwd)))
    ws.settle(ops, what + " backward")
    got = {}
    for k, g in o.items():
        if k == "dh0" and not dh0:
            assert g.untouched(), "%s: dh0 was not asked for, yet it was written" % what
        else:
            got[k] = g.settle(what + " " + k)
    return got


def check(ops, case, what=None, **variant):
    batch, T, H = case
    what = what or "gru_seq %s %s" % (P.case_id(case), variant)
    span = P.tag_span(batch, T, H, cus())
    assert ops.gru_seq_tag_span(batch, T, H) == span, "%s: gru_seq_tag_span %d, the plan says %d" % (what, ops.gru_seq_tag_span(batch, T, H), span)
    ref = R.reference(batch, T, H, **variant)
    got = run_gru(ops, ref, batch, T, H, what=what)
    for k, v in got.items():
        within(CLASS[k], v, getattr(ref.fwd, k) if k in R.Forward._fields else getattr(ref.bwd, k), what + " " + k)
    if ref.lens is not None:
        dead = ~R.live_mask(ref.lens, batch, T).reshape(-1)
        assert batch == 1 or (dead.any() and not dead.all())      # (one clip: lstm_plan.lengths gives it T + 5, clamped to T -- all live)
        for k in ("act", "hcand", "hseq", "dgx", "dgh"):
            assert not got[k][dead].any(), "%s: dead row of %s not zero" % (what, k)
    return got


# ---- the launcher's branches ----------------------------------------------------------------------------------------------------------
def test_the_cases_reach_their_branches_on_this_device():
    plan = lambda c: P.cluster_plan(*P.resolve(c, cus()), cus())
    ones, ragged, two, h37, h250, h256, t1, t2, t21, threes = (plan(c) for c in CASES)
    assert (ones.W, ones.Hp) == (32, 500) and P.group_sizes(ones) == [[1] * ones.maxG]
    assert len(ragged.launches) == 1 and {1, 2} == set(P.group_sizes(ragged)[0])
    assert len(two.launches) == 2 and two.Hp == 512 and two.launches[0].nb == two.chunk and two.launches[1].nb == 1
    assert {g.nclips for g in two.launches[0].groups} == {8} and {(g.S, g.publish) for g in two.launches[0].groups} == {(4, 8)}
    assert 4 * (two.Hp * 48 + 8 * two.Hp + 8 * 48 + 48) <= 150 * 1024                            # the forward kernel's LDS at Hp = 512
    assert (h37.W, h37.bwd_gather) == (3, 4) and [g.gather for g in h37.launches[0].groups] == [1]
    assert (h250.Hp, h250.W) == (252, 16)
    assert all(P.reduction_slices(250, g.KP)[-1] == (192, 250) for g in h250.launches[0].groups)  # a last slice that is no multiple of 16
    assert (h256.W, h256.bwd_gather) == (16, 16) and any(g.gather == 2 for g in h256.launches[0].groups)
    assert all(len(p.launches) == 1 and len(p.launches[0].groups) > 1 for p in (t1, t2, t21))
    assert {(g.nclips, g.S, g.KP, g.publish) for g in threes.launches[0].groups} == {(3, 2, 2, 4)}  # the 2 x 2 reduction split
    assert {p.bwd_gather for p in (ones, h37, h256)} == {4, 16, 32}


@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
@pytest.mark.parametrize("case", CASES, ids=P.case_id)
def test_gru_cluster_against_the_reference(ops, case, lens):
    check(ops, P.resolve(case, cus()), lens=lens)


# ---- variants ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", (dict(h0=False), dict(rb=False), dict(h0=False, rb=False, lens=True)), ids=("no-h0", "no-rb", "neither-lens"))
def test_gru_without_initial_state_or_recurrent_bias(ops, variant):
    check(ops, P.resolve(R.VARIANT_CASE, cus()), **variant)


def test_gru_without_dout_gives_exact_zeros(ops):
    got = check(ops, P.resolve(R.VARIANT_CASE, cus()), dout=False)
    for k in ("dgx", "dgh", "dh0"):
        assert not got[k].any(), "gru_seq: %s not exactly zero without dout" % k


def test_gru_dh0_not_asked_for_is_untouched(ops):
    batch, T, H = P.resolve(R.VARIANT_CASE, cus())
    ref = R.reference(batch, T, H)
    got = run_gru(ops, ref, batch, T, H, dh0=False, what="gru_seq no dh0")
    assert "dh0" not in got
    same_bits(got, {k: v for k, v in run_gru(ops, ref, batch, T, H, what="gru_seq").items() if k != "dh0"}, "gru_seq: with and without dh0")


# ---- structure, bit for bit -----------------------------------------------------------------------------------------------------------------
def test_gru_is_repeatable_on_one_workspace(ops):
    batch, T, H = P.resolve(R.VARIANT_CASE, cus())
    ws, ref = Workspace(ops, batch, T, H, DEV), R.reference(batch, T, H)
    first = run_gru(ops, ref, batch, T, H, ws=ws, what="gru_seq")
    same_bits(first, run_gru(ops, ref, batch, T, H, ws=ws, what="gru_seq again"), "gru_seq: second run on the same workspace")


def test_an_lstm_launch_between_two_gru_launches_on_one_workspace_changes_nothing(ops):
    """The shared tag counter: the LSTM launches' tags on the same exchange words can never match a GRU launch's."""
    batch, T, H = P.resolve(R.VARIANT_CASE, cus())
    ws, ref = Workspace(ops, batch, T, H, DEV), R.reference(batch, T, H)
    first = run_gru(ops, ref, batch, T, H, ws=ws, what="gru_seq")
    lref = P.reference(batch, T, H)
    gx, kh, h0, c0, dout = (put(a, DEV) for a in lref.inp)
    lo = {k: torch.empty(batch * T, w * H, device=DEV) for k, w in (("act", 4), ("cseq", 1), ("hseq", 1), ("hprev", 1), ("dz", 4))}
    ops.lstm_seq_fwd(gx, kh, lo["act"], lo["cseq"], lo["hseq"], lo["hprev"], batch, T, H, ws=ws.t, h0=h0, c0=c0)
    ops.lstm_seq_bwd(dout, kh, put(lref.act32, DEV), put(lref.cseq32, DEV), lo["dz"], batch, T, H, ws=ws.t, c0=c0)
    ws.settle(ops, "lstm_seq between the GRU launches")
    within("hseq", lo["hseq"].cpu().numpy(), lref.fwd.hseq, "lstm_seq on the GRU's workspace")
    within("dz", lo["dz"].cpu().numpy(), lref.bwd.dz, "lstm_seq on the GRU's workspace")
    same_bits(first, run_gru(ops, ref, batch, T, H, ws=ws, what="gru_seq after the LSTM launches"), "gru_seq: after LSTM launches on the same workspace")


@pytest.mark.parametrize("case", (CASES[2], R.VARIANT_CASE), ids=P.case_id)
def test_replay_safe_forms_called_eagerly_give_the_eager_bits(ops, case):
    batch, T, H = P.resolve(case, cus())
    span = ops.gru_seq_tag_span(batch, T, H)
    assert span == P.tag_span(batch, T, H, cus()) > 0
    ref = R.reference(batch, T, H)
    plain = run_gru(ops, ref, batch, T, H, what="gru_seq plain")
    state, ws = ops.step_state(DEV), Workspace(ops, batch, T, H, DEV)
    for origin in (1, 1 + 2 * span):
        ops.step_state_set(state, 0, 0.0, origin)
        got = run_gru(ops, ref, batch, T, H, ws=ws, st=St(state, 0, span), what="gru_seq_st origin %d" % origin)
        same_bits(got, plain, "gru_seq_st origin %d against the eager entry points" % origin)


def test_the_last_clip_alone_in_a_second_launch_equals_a_batch_of_one(ops):
    batch, T, H = P.resolve(CASES[2], cus())
    assert P.cluster_plan(batch, T, H, cus()).launches[-1].nb == 1 and batch > 1
    ref = R.reference(batch, T, H)
    whole = run_gru(ops, ref, batch, T, H, what="gru_seq")
    rows, row = slice((batch - 1) * T, batch * T), slice(batch - 1, batch)
    inp = ref.inp
    one = R.Ref(R.Inputs(inp.gx[rows], inp.rk, inp.rb, inp.h0[row], inp.dout[rows]), None, None, ref.act32[rows], ref.hcand32[rows],
                ref.hprev32[rows], None)
    alone = run_gru(ops, one, 1, T, H, what="gru_seq last clip alone")
    last = {k: v[-T:] if v.shape[0] == batch * T else v[-1:] for k, v in whole.items()}
    same_bits(alone, last, "gru_seq: the clip alone in the last launch against a batch-1 call")


def test_gru_refusals_write_nothing(ops):
    """H = 513: "bad shape"; lengths with a step state; a workspace one word short: "workspace".  Nothing is launched."""
    batch, T, H = 2, 2, 16
    ref = R.reference(batch, T, H)
    gx, rk, rb, h0, dout = (put(a, DEV) for a in ref.inp)
    lens, state = put(P.lengths(batch, T), DEV, torch.int32), ops.step_state(DEV)
    o = {k: Guarded((batch * T, w * H), DEV) for k, w in SEQ_OUT}
    o["dh0"] = Guarded((batch, H), DEV)
    ws = ops.lstm_seq_ws(batch, T, H, DEV)
    big = ops.lstm_seq_ws(batch, T, 513, DEV)
    fwd = lambda h, w, **kw: ops.gru_seq_fwd(gx, rk, o["act"].t, o["hcand"].t, o["hseq"].t, o["hprev"].t, batch, T, h, ws=w, rb=rb, h0=h0, **kw)
    bwd = lambda h, w, **kw: ops.gru_seq_bwd(dout, rk, put(ref.act32, DEV), put(ref.hcand32, DEV), put(ref.hprev32, DEV), o["dgx"].t, o["dgh"].t,
                                             batch, T, h, ws=w, dh0=o["dh0"].t, **kw)
    for call in (fwd, bwd):
        for h, w, kw, match in ((513, big, {}, "bad shape"), (513, big, dict(state=state), "bad shape"), (0, ws, {}, "bad shape"),
                                (H, ws[:-1], {}, "workspace"), (H, ws[:-1], dict(state=state), "workspace"),
                                (H, ws, dict(state=state, seq_len=lens), "no lengths")):
            with pytest.raises(Exception, match=match):
                call(h, w, **kw)
    assert ops.gru_seq_tag_span(batch, T, 513) == 0
    torch.cuda.synchronize()
    assert all(g.untouched() for g in o.values()), "gru_seq: refused, yet an output was written"
    assert not ws.any() and not big.any(), "gru_seq: refused, yet the workspace was written"


# ---- LRCNEngine with the GRU classifier --------------------------------------------------------------------------------------------------
MEAN = np.array([99.197148, 105.293620, 109.503945], np.float32)
SHAPE, NCLS, FPC, CLIPS = (67, 67, 3), 7, 3, 2                      # the smoke() geometry


@pytest.mark.parametrize("layers,fusion", [(2, "avg"), (1, "last")])
def test_lrcn_engine_train_step_against_the_reference(layers, fusion):
    """Logits, loss, every gradient and the clipped SGD step against oracle.alexnet_forward followed by gru_ref, at the bounds of
    tests/test_blstm_gpu.test_lrcn_engine_train_step_against_the_reference (seed 6 for the reason given there)."""
    from vltf_amd.engine import LRCNEngine, NetConfig, param_specs
    rng = np.random.default_rng(6)
    H = 8
    cfg = NetConfig(image_shape=SHAPE, num_classes=NCLS, fpc=FPC, frame_encoding_layer="fc6", lstm_hidden=H, lstm_layers=layers, fusion=fusion,
                    rnn_cell="gru")
    eng = LRCNEngine(cfg, max_clips=CLIPS, device=DEV)
    p = R.init_params(rng, NCLS, "fc6", H, layers, SHAPE, fusion)
    assert {n: tuple(s) for n, s in param_specs(cfg)} == {n: v.shape for n, v in p.items()}
    eng.load_params(p)
    frames = rng.integers(0, 256, (CLIPS * FPC,) + SHAPE, dtype=np.uint8)
    onehot = np.eye(NCLS, dtype=np.int32)[rng.integers(0, NCLS, CLIPS)]
    x = frames.astype(np.float32) - MEAN
    newp, loss, gn, logits, grads = R.model_train_step(p, x, onehot, FPC, 0.01, 0.5, "fc6", H, layers, fusion)
    fd = torch.tensor(frames, device=DEV)
    got_fwd = eng.forward_u8(fd, MEAN).cpu().numpy()
    assert got_fwd.shape == logits.shape
    np.testing.assert_allclose(got_fwd, logits, rtol=1e-3, atol=1e-3)
    out = eng.train_step_u8(fd, torch.tensor(onehot, device=DEV), lr=0.01, clip_norm=0.5, mean_bgr=MEAN)
    assert abs(out["loss"] - loss) < 1e-4 * max(1, abs(loss))
    assert abs(out["grad_norm"] - gn) < 1e-3 * gn
    g = eng.get_grads()
    assert set(g) == set(p)
    for k in p:
        scale = np.abs(grads[k]).max() + 1e-12
        np.testing.assert_allclose(g[k], grads[k], rtol=2e-3, atol=2e-4 * scale, err_msg="grad " + k)
        assert scale > 1e-9, "no gradient reached " + k
    got = eng.get_params()
    for k in p:
        np.testing.assert_allclose(got[k], newp[k], rtol=1e-4, atol=1e-5, err_msg="param " + k)


def test_lrcn_engine_captured_step_is_the_eager_step():
    """step_graph: the warm-up step, the captured one and three replays equal the eager engine's bit for bit (the GRU launches run on the
    graph workspace with replay-safe tags that move between replays)."""
    from vltf_amd.engine import LRCNEngine, NetConfig, init_params
    engines = []
    kw = dict(image_shape=SHAPE, num_classes=NCLS, fpc=FPC, frame_encoding_layer="fc6", lstm_hidden=16, lstm_layers=2, fusion="avg",
              rnn_cell="gru", dropout_keep_prob=0.5)
    params = init_params(NetConfig(**kw), seed=4, well_scaled=True)
    for sg in (False, True):
        e = LRCNEngine(NetConfig(step_graph=sg, **kw), max_clips=CLIPS, device=DEV)
        e.load_params(params)
        engines.append(e)
    rng = np.random.default_rng(11)
    for step in range(5):
        frames = torch.from_numpy(rng.integers(0, 256, (CLIPS * FPC,) + SHAPE, dtype=np.uint8)).to(DEV)
        onehot = torch.from_numpy(np.eye(NCLS, dtype=np.int32)[rng.integers(0, NCLS, CLIPS)]).to(DEV)
        outs = [e.train_step_u8(frames, onehot, 0.01 * 0.7 ** step, 5.0, MEAN) for e in engines]
        for k in ("loss_sum", "correct", "grad_norm", "rows"):
            assert outs[0][k] == outs[1][k], (step, k, outs[0][k], outs[1][k])
        assert np.array_equal(engines[0].logits_host(), engines[1].logits_host()), step
    assert len(engines[1]._graphs) == 1 and engines[1].graph_tag_next > 1
    pa, pb = engines[0].get_params(), engines[1].get_params()
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), k


# ---- GraphEngine: a vector-input pipeline with lengths -----------------------------------------------------------------------------------------
G_DIM, G_H, G_C, G_CLIPS = 10, 6, 5, 4


def graph_engine(T, layers=2, fusion="reshape", seed=3):
    from vltf_amd.graph import DatasetInfo, GraphEngine, PipelineSpec, init_params_for, model_specs
    pipes = [PipelineSpec("net", ["main"], "nop", classifier="lstm", lstm_params=(G_H, layers, fusion), rnn_cell="gru")]
    ds = {"main": DatasetInfo("vectors", T, 1, G_CLIPS, dim=G_DIM)}
    eng = GraphEngine(pipes, ds, G_C, device=DEV)
    p = init_params_for(model_specs(pipes, ds, G_C), seed=seed, well_scaled=True)
    for k in p:                                                     # biases that are not zero: a bias gradient on the wrong bias would show
        if k.endswith("bias"):
            p[k] = (0.1 * np.random.default_rng(len(k)).standard_normal(p[k].shape)).astype(np.float32)
    eng.load_params(p)
    return eng, p


@pytest.mark.parametrize("fusion", ("reshape", "last"))
def test_graph_engine_with_lengths_against_the_reference(fusion):
    T, lens = 5, [5, 2, 1, 4]
    eng, p = graph_engine(T, fusion=fusion)
    x = (np.random.default_rng(8).standard_normal((G_CLIPS * T, G_DIM))).astype(np.float32)
    got = eng.forward({"main": torch.from_numpy(x).to(DEV)}, seq_len={"net": lens}).cpu().numpy()
    out, _ = R.stack_forward(x, p, T, G_H, 2, lens=np.array(lens))
    head = R.head_name(fusion)
    want = R.fuse(out, T, G_H, fusion, np.array(lens)) @ p[head + "_w"].astype(np.float64) + p[head + "_b"]
    live = R.live_mask(np.array(lens), G_CLIPS, T).reshape(-1) if fusion == "reshape" else slice(None)
    np.testing.assert_allclose(got[live], want[live], rtol=1e-3, atol=1e-3)


def test_graph_engine_padding_is_inert():
    """Other vectors in the dead steps change nothing: live-row logits, the loss and every parameter after the step are bitwise equal."""
    T, lens = 5, [5, 2, 1, 4]
    live = R.live_mask(np.array(lens), G_CLIPS, T).reshape(-1)
    x = (np.random.default_rng(8).standard_normal((G_CLIPS * T, G_DIM))).astype(np.float32)
    onehot = torch.from_numpy(np.eye(G_C, dtype=np.int32)[np.random.default_rng(9).integers(0, G_C, G_CLIPS * T)]).to(DEV)
    res = []
    for fill in (None, 99):
        eng, _ = graph_engine(T)
        fed = x.copy()
        if fill is not None:
            fed[~live] = (np.random.default_rng(fill).standard_normal(fed[~live].shape) * 3).astype(np.float32)
        fd = {"main": torch.from_numpy(fed).to(DEV)}
        got = eng.forward(fd, seq_len={"net": lens}).cpu().numpy()
        out = eng.train_step(fd, onehot, lr=0.01, clip_norm=0.5, seq_len={"net": lens})
        assert out["rows"] == sum(lens)
        res.append((got[live], out["loss"], eng.get_params()))
    assert np.array_equal(res[0][0], res[1][0]) and res[0][1] == res[1][1]
    for k in res[0][2]:
        assert np.array_equal(res[0][2][k], res[1][2][k]), "parameter %s moved with the padding" % k


def test_graph_engine_uniform_length_is_the_shorter_model():
    """Clips of length 3 in a 5-step batch give what they give in a 3-step model: logits, loss and the step."""
    T, L = 5, 3
    x = (np.random.default_rng(8).standard_normal((G_CLIPS, T, G_DIM))).astype(np.float32)
    labels = np.random.default_rng(9).integers(0, G_C, (G_CLIPS, T))
    res = []
    for steps, kw in ((T, dict(seq_len={"net": [L] * G_CLIPS})), (L, {})):
        eng, p = graph_engine(steps)
        fd = {"main": torch.from_numpy(np.ascontiguousarray(x[:, :steps]).reshape(-1, G_DIM)).to(DEV)}
        onehot = torch.from_numpy(np.eye(G_C, dtype=np.int32)[labels[:, :steps].reshape(-1)]).to(DEV)
        logits = eng.forward(fd, **kw).cpu().numpy().reshape(G_CLIPS, steps, G_C)[:, :L]
        out = eng.train_step(fd, onehot, lr=0.01, clip_norm=0.5, **kw)
        res.append((logits, out, eng.get_params()))
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=1e-5, atol=1e-6)
    assert res[0][1]["rows"] == res[1][1]["rows"] == G_CLIPS * L
    assert abs(res[0][1]["loss"] - res[1][1]["loss"]) < 1e-5 * max(1, abs(res[1][1]["loss"]))
    for k in res[0][2]:
        np.testing.assert_allclose(res[0][2][k], res[1][2][k], rtol=1e-4, atol=1e-6, err_msg="param " + k)


# ---- run_task.py on examples/lrcn_gru.yml ------------------------------------------------------------------------------------------------------
def test_run_task_on_the_example_trains_validates_and_resumes(tmp_path, monkeypatch):
    """examples/lrcn_gru.yml pointed at the synthetic dataset (its shapes, four classes, two 8-unit layers, batches of 2): two train steps
    with a checkpoint, a validation of it, and a second training run that resumes from it; the checkpoint holds the GRU variables."""
    import glob
    import os
    import yaml
    from tests.test_host_workflow import make_dataset
    from tests.test_run_task_gpu import RAW, WANT
    from vltf_amd import run_task
    monkeypatch.setenv("VLTF_PREFETCH", "0")
    monkeypatch.setenv("VLTF_CONV_MATH", "f32")
    folder = str(tmp_path)
    train_path, _, _ = make_dataset(folder, "train.txt", nvid=4, cpv=(1, 1, 1, 1), shape=RAW, seed=1)
    val_path, _, _ = make_dataset(folder, "val.txt", nvid=3, cpv=(2, 1, 2), shape=RAW, seed=2)
    run = os.path.join(folder, "run")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def cfg(name, data_path, phase, resume=None, epochs=1):
        with open(os.path.join(root, "examples", "lrcn_gru.yml")) as f:
            c = yaml.safe_load(f)
        r = c["run"]
        r.update(resume_file=resume, run_folder=run, phase="defs.phase.%s" % phase)
        d = r["data"].pop("train_set")
        d.update(data_path=data_path, phase="defs.phase.%s" % phase, raw_image_shape=str(RAW), image_shape=str(WANT))
        if phase != "train":
            d["imgproc"] = ["defs.imgproc.center_crop", "defs.imgproc.sub_mean"]
        r["data"]["d"] = d
        r["network"]["num_classes"] = 4
        pipe = r["network"]["pipelines"][0]["lrcn"]
        assert pipe["rnn_cell"] == "gru"
        pipe["lstm_params"] = [8, 2, "defs.fusion_method.avg"]
        r["train"].update(batch_size=2, epochs=epochs, base_lr=1e-4, lr_decay=["defs.decay.exp", "defs.periodicity.interval", 2, 0.9], clip_norm=5)
        r["val"]["batch_size"] = 2
        path = os.path.join(folder, name)
        with open(path, "w") as f:
            yaml.safe_dump(c, f)
        return path

    run_task.main(cfg("train.yml", train_path, "train"), seed=3)                           # 4 videos, batch 2: two steps
    ck = glob.glob(os.path.join(run, "checkpoints", "*.weights.npz"))
    assert len(ck) == 1
    saved = np.load(ck[0])
    names = [n for l in range(2) for n in R.param_names(l)]
    assert all(n in saved.files for n in names) and saved["output_fc_w"].shape == (8, 4)
    assert [saved[n].shape for n in names] == [(4096, 24), (8, 24), (24,), (24,), (8, 24), (8, 24), (24,), (24,)]
    assert not any("basic_lstm_cell" in n for n in saved.files)
    log = open(glob.glob(os.path.join(run, "log_lrcn_gru_train_scratch_*.log"))[0]).read()
    assert "global step: 2" in log
    acc = run_task.main(cfg("val.yml", val_path, "val", resume="latest"))
    assert 0.0 <= acc <= 1.0 and float(open(os.path.join(run, "accuracy_lrcn_gru_val_resume")).read()) == acc
    run_task.main(cfg("resume.yml", train_path, "train", resume=ck[0][:-len(".weights.npz")], epochs=2), seed=5)
    log2 = open(glob.glob(os.path.join(run, "log_lrcn_gru_train_resume_*.log"))[0]).read()
    assert "Restored training snapshot of epoch 1" in log2 and "global step: 4" in log2
    after = np.load(max(glob.glob(os.path.join(run, "checkpoints", "*.weights.npz")), key=os.path.getmtime))
    assert any(not np.array_equal(after[n], saved[n]) for n in names if n.endswith("kernel"))
