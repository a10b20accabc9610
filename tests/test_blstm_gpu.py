"""The bidirectional LSTM launch (vl_lstm_seq_bi_fwd / _bwd, csrc/lstm_cluster.hip) against the fp64 reference of tests/blstm_ref.py
on the smallest shapes at which each branch can go wrong, and its structural properties bit for bit: the backward half mirrors the
forward half on mirrored inputs, the forward half equals the unidirectional launch where both plans hold one clip per group, strided
hseq / dout equal the dense call and leave their padding alone, two calls on one workspace agree, the replay-safe entry points called
eagerly give the eager bits, and the refusals write nothing.

mg and chunk in the case lists are mg_bi = CUs / (2 ceil(H / 16)) and 8 mg_bi.  The tolerances, the guarded outputs and the workspace
with a sentinel tail are those of tests/test_lstm_geometry_gpu.py.  The backward launch is handed the REFERENCE's act and cseq rounded to
fp32, not the forward kernel's.  With lengths (lstm_plan.lengths: a 0, a T, a -3 and a T + 5 among them) every dead row of gx and dout
holds NaN."""
import functools

import numpy as np
import pytest
import torch

from tests import blstm_ref as B
from tests import lstm_plan as P
from tests.test_lstm_geometry_gpu import DEV, GUARD, SENTINEL, Guarded, St, Workspace, cus, get, put, same_bits, within

pytestmark = pytest.mark.gpu

CASES = [P.Case("mg", 3, 498), P.Case("mg+1", 3, 498), P.Case("chunk+1", 3, 512), P.Case(1, 3, 37), P.Case(3, 3, 250), P.Case("mg+1", 3, 256)] + \
        [P.Case("mg+1", T, 498) for T in (1, 2, 21)]
VARIANT_CASE = P.Case("mg+1", 3, 498)
VARIANTS = [v for v in P.VARIANTS if not v.lens]
FWD, BWD = ("act", "cseq", "hseq", "hprev"), ("dz", "dh0", "dc0")
WIDTH = dict(act=4, cseq=1, hseq=1, hprev=1, dz=4)


@pytest.fixture(scope="module")
def ops():
    import vltf_amd.ops as ops_
    return ops_


@functools.lru_cache(maxsize=4)
def reference(batch, T, H, variant=P.PLAIN, lens=False):
    """Inputs (pairs), lengths, fp64 forward, its fp32 rounding, the fp64 backward from that rounding."""
    inp = B.inputs(batch, T, H)
    L = P.lengths(batch, T) if lens else None
    h0 = tuple(i.h0 if variant.state in ("h0", "both") else None for i in inp)
    c0 = tuple(i.c0 if variant.state in ("c0", "both") else None for i in inp)
    dout = tuple(i.dout if variant.dout else None for i in inp)
    fwd = B.forward_ref(tuple(i.gx for i in inp), tuple(i.kh for i in inp), T, h0, c0, variant.forget_bias, L)
    act32, cseq32 = tuple(P.rounded(f.act) for f in fwd), tuple(P.rounded(f.cseq) for f in fwd)
    bwd = B.backward_ref(dout, tuple(i.kh for i in inp), T, act32, cseq32, c0, L)
    return dict(inp=inp, lens=L, h0=h0, c0=c0, dout=dout, fwd=fwd, act32=act32, cseq32=cseq32, bwd=bwd)


def run_bi(ops, batch, T, H, gx, kh, h0, c0, dout, act_in, cseq_in, lens=None, variant=P.PLAIN, ws=None, st=None, pad=0, what=""):
    """One bidirectional forward launch and one backward launch on the given host arrays (pairs) -> {name: (fw array, bw array)}.
    pad > 0: hseq and dout live in [B T][2H + pad] tensors whose padding columns hold NaN and must stay untouched."""
    ws = ws or Workspace(ops, batch, T, H, DEV)
    n = batch * T
    if lens is not None:
        gx = tuple(B.with_nan_in_dead_rows(a, T, lens) for a in gx)
        dout = tuple(None if a is None else B.with_nan_in_dead_rows(a, T, lens) for a in dout)
    dev2 = lambda pair: tuple(put(a, DEV) for a in pair)
    gx_d, kh_d, h0_d, c0_d, act_d, cseq_d = (dev2(p) for p in (gx, kh, h0, c0, act_in, cseq_in))
    L = put(lens, DEV, torch.int32)
    o = {k: (Guarded((n, w * H), DEV), Guarded((n, w * H), DEV)) for k, w in WIDTH.items() if k != "hseq" or not pad}
    o.update({k: (Guarded((batch, H), DEV), Guarded((batch, H), DEV)) for k in ("dh0", "dc0")})
    ld = 2 * H + pad
    if pad:
        wide = Guarded((n, ld), DEV)
        hseq, hseq_ld = (wide.t[:, :H], wide.t[:, H:2 * H]), ld
        dwide = torch.full((n, ld), float("nan"), device=DEV)
        for d in range(2):
            if dout[d] is not None:
                dwide[:, d * H:(d + 1) * H] = put(dout[d], DEV)
        dout_d, dout_ld = tuple(None if dout[d] is None else dwide[:, d * H:(d + 1) * H] for d in range(2)), ld
    else:
        hseq, hseq_ld = tuple(g.t for g in o["hseq"]), None
        dout_d, dout_ld = dev2(dout), None
    t2 = lambda k: tuple(g.t for g in o[k])
    asked = dict(dh0=variant.grads in ("dh0", "both"), dc0=variant.grads in ("dc0", "both"))
    stf = {} if st is None else dict(state=st.state, tag_offset=st.fwd)
    stb = {} if st is None else dict(state=st.state, tag_offset=st.bwd)
    ops.lstm_seq_bi_fwd(gx_d, kh_d, t2("act"), t2("cseq"), hseq, t2("hprev"), batch, T, H, forget_bias=variant.forget_bias, ws=ws.t, h0=h0_d,
                        c0=c0_d, seq_len=L, hseq_ld=hseq_ld, **stf)
    ws.settle(ops, what + " forward")
    ops.lstm_seq_bi_bwd(dout_d, kh_d, act_d, cseq_d, t2("dz"), batch, T, H, ws=ws.t, c0=c0_d, dh0=t2("dh0") if asked["dh0"] else None,
                        dc0=t2("dc0") if asked["dc0"] else None, seq_len=L, dout_ld=dout_ld, **stb)
    ws.settle(ops, what + " backward")
    got = {}
    for k, pair in o.items():
        if not asked.get(k, True):
            assert all(g.untouched() for g in pair), "%s: %s was not asked for, yet it was written" % (what, k)
        else:
            got[k] = tuple(g.settle("%s %s[%d]" % (what, k, d)) for d, g in enumerate(pair))
    if pad:
        w = get(wide.flat)
        body = w[GUARD:-GUARD].reshape(n, ld)
        assert (w[:GUARD] == SENTINEL).all() and (w[-GUARD:] == SENTINEL).all(), what + ": guard around the strided hseq written"
        assert np.isnan(body[:, 2 * H:]).all(), what + ": padding columns of hseq written"
        got["hseq"] = (body[:, :H].copy(), body[:, H:2 * H].copy())
        assert np.isfinite(got["hseq"][0]).all() and np.isfinite(got["hseq"][1]).all(), what + ": hseq element not written"
    return got


def run_ref(ops, ref, batch, T, H, **kw):
    inp = ref["inp"]
    return run_bi(ops, batch, T, H, tuple(i.gx for i in inp), tuple(i.kh for i in inp), ref["h0"], ref["c0"], ref["dout"], ref["act32"],
                  ref["cseq32"], lens=ref["lens"], **kw)


def same_pairs(a, b, what):
    for d in range(2):
        same_bits({k: v[d] for k, v in a.items()}, {k: v[d] for k, v in b.items()}, "%s [direction %d]" % (what, d))


def check_bi(ops, case, lens=False, variant=P.PLAIN):
    batch, T, H = case
    what = "lstm_seq_bi %s%s%s" % (P.case_id(case), " lens" if lens else "", "" if variant == P.PLAIN else " " + P.case_id(variant))
    assert ops.lstm_seq_bi_tag_span(batch, T, H) == B.tag_span(batch, T, H, cus()), what + ": tag span"
    ref = reference(batch, T, H, variant, lens)
    got = run_ref(ops, ref, batch, T, H, variant=variant, what=what)
    for k, pair in got.items():
        for d in range(2):
            want = getattr(ref["fwd"][d], k) if k in FWD else getattr(ref["bwd"][d], k)
            within(k, pair[d], want, "%s [direction %d]" % (what, d))
    if lens:
        dead = ~B.live_mask(ref["lens"], batch, T).reshape(-1)
        assert not dead.all() and (dead.any() or batch < 3)                # one clip: lstm_plan.lengths gives it T + 5, all rows live
        for k in ("act", "hseq", "dz"):
            assert not got[k][0][dead].any() and not got[k][1][dead].any(), "%s: dead row of %s not zero" % (what, k)
    if not variant.dout:
        for k in BWD:
            assert k not in got or not (got[k][0].any() or got[k][1].any()), "%s: %s not exactly zero without dout" % (what, k)


# ---- against the fp64 reference ----------------------------------------------------------------------------------------------------------
def test_the_cases_reach_their_branches_on_this_device():
    plans = [B.bi_plan(*B.resolve(c, cus()), cus()) for c in CASES]
    full, ragged, multi, tiny, odd, h256 = plans[:6]
    assert [g.nclips for g in full.launches[0].groups] == [1] * full.mg and len(full.launches) == 1
    assert sorted({g.nclips for g in ragged.launches[0].groups}) == [1, 2] and len(ragged.launches) == 1
    assert [l.nb for l in multi.launches] == [multi.chunk, 1] and multi.Hp == 512
    assert (tiny.W, odd.Hp, odd.W, h256.W) == (3, 252, 16, 16) and len(h256.launches[0].groups) > 1
    assert all(l.grid <= cus() for p in plans for l in p.launches)


@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
@pytest.mark.parametrize("case", CASES, ids=P.case_id)
def test_blstm_against_the_reference(ops, case, lens):
    check_bi(ops, B.resolve(case, cus()), lens)


@pytest.mark.parametrize("variant", VARIANTS, ids=P.case_id)
def test_blstm_variants(ops, variant):
    """h0 / c0 / neither, dh0 / dc0 / neither, forget bias 0 and 2.5, dout = None."""
    check_bi(ops, B.resolve(VARIANT_CASE, cus()), variant=variant)


# ---- structure, bit for bit ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
def test_the_backward_half_mirrors_the_forward_half(ops, lens):
    """kh_bw = kh_fw, gx_bw = reverse_sequence(gx_fw), equal initial states, dout_bw = reverse_sequence(dout_fw): every tensor of the backward
    half is the reverse_sequence of the forward half's (dead rows stay where they are and are equal), dh0 and dc0 are equal."""
    batch, T, H = B.resolve(P.Case("mg+1", 4, 498), cus())
    f = P.inputs(batch, T, H)
    L = P.lengths(batch, T) if lens else None
    rs = lambda a: B.reverse_sequence(a, T, L)
    fw = P.forward_ref(f.gx, f.kh, T, f.h0, f.c0, 1.0, L)
    act32, cseq32 = P.rounded(fw.act), P.rounded(fw.cseq)
    got = run_bi(ops, batch, T, H, (f.gx, rs(f.gx)), (f.kh, f.kh), (f.h0, f.h0), (f.c0, f.c0), (f.dout, rs(f.dout)), (act32, rs(act32)),
                 (cseq32, rs(cseq32)), lens=L, what="mirror")
    for k, (a, b) in got.items():
        want = rs(a) if k in WIDTH else a
        assert np.array_equal(want.view(np.int32), b.view(np.int32)), "mirror%s: %s of the backward half is not the forward half's, reversed" % (" lens" if lens else "", k)
    within("hseq", got["hseq"][0], fw.hseq, "mirror")


@pytest.mark.parametrize("case", (P.Case(3, 3, 498), P.Case(1, 3, 37)), ids=P.case_id)
def test_the_forward_half_is_the_unidirectional_launch(ops, case):
    """batch <= mg_bi: both plans hold one clip per group, so the forward direction's arithmetic is the unidirectional launch's."""
    batch, T, H = case
    assert batch <= B.mg_bi(H, cus())
    ref = reference(batch, T, H)
    got = run_ref(ops, ref, batch, T, H, what="half")
    f = ref["inp"][0]
    n = batch * T
    o = {k: Guarded((n, w * H), DEV) for k, w in WIDTH.items()}
    o.update(dh0=Guarded((batch, H), DEV), dc0=Guarded((batch, H), DEV))
    ws = Workspace(ops, batch, T, H, DEV)
    kh, h0, c0 = put(f.kh, DEV), put(f.h0, DEV), put(f.c0, DEV)
    ops.lstm_seq_fwd(put(f.gx, DEV), kh, o["act"].t, o["cseq"].t, o["hseq"].t, o["hprev"].t, batch, T, H, ws=ws.t, h0=h0, c0=c0)
    ops.lstm_seq_bwd(put(f.dout, DEV), kh, put(ref["act32"][0], DEV), put(ref["cseq32"][0], DEV), o["dz"].t, batch, T, H, ws=ws.t, c0=c0,
                     dh0=o["dh0"].t, dc0=o["dc0"].t)
    ws.settle(ops, "unidirectional")
    same_bits({k: g.settle(k) for k, g in o.items()}, {k: v[0] for k, v in got.items()}, "forward half against lstm_seq_fwd / _bwd")


@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
def test_strided_hseq_and_dout(ops, lens):
    """Row stride 2H + 3 with NaN in the three padding columns: the dense call's bits, the padding untouched."""
    batch, T, H = B.resolve(P.Case("mg+1", 3, 250), cus())
    ref = reference(batch, T, H, P.PLAIN, lens)
    same_pairs(run_ref(ops, ref, batch, T, H, pad=3, what="strided"), run_ref(ops, ref, batch, T, H, what="dense"), "row stride 2H + 3 against dense")


def test_blstm_is_repeatable_on_one_workspace(ops):
    batch, T, H = B.resolve(P.Case("chunk+1", 3, 498), cus())
    ref, ws = reference(batch, T, H), Workspace(ops, batch, T, H, DEV)
    first = run_ref(ops, ref, batch, T, H, ws=ws, what="first")
    same_pairs(first, run_ref(ops, ref, batch, T, H, ws=ws, what="again"), "second run on the same workspace")
    ops.lstm_seq_check(ws.t)


def test_replay_safe_entry_points_called_eagerly(ops):
    """Two launches per call; tag origin 1 with offsets 0 and span, then an origin 2 span further on the same workspace."""
    batch, T, H = B.resolve(P.Case("chunk+1", 3, 498), cus())
    span = ops.lstm_seq_bi_tag_span(batch, T, H)
    assert span == 2 * (T + 1) == B.tag_span(batch, T, H, cus())
    ref = reference(batch, T, H)
    plain = run_ref(ops, ref, batch, T, H, what="eager")
    state, ws = ops.step_state(DEV), Workspace(ops, batch, T, H, DEV)
    for origin in (1, 1 + 2 * span):
        ops.step_state_set(state, 0, 0.0, origin)
        same_pairs(run_ref(ops, ref, batch, T, H, ws=ws, st=St(state, 0, span), what="st origin %d" % origin), plain, "_st origin %d against eager" % origin)


def test_refusals(ops):
    """A capturing stream (both eager entry points); H = 513, H = 0 and a short workspace: an error, nothing written."""
    from vltf_amd._ffi import VltfError
    batch, T, H = 2, 2, 16
    z = lambda *s: torch.zeros(s, device=DEV)
    pair = lambda *s: (z(*s), z(*s))
    n = batch * T
    gx, kh, cseq_in = pair(n, 4 * H), pair(H, 4 * H), pair(n, H)
    o = {k: (Guarded((n, w * H), DEV), Guarded((n, w * H), DEV)) for k, w in WIDTH.items()}
    t2 = lambda k: tuple(g.t for g in o[k])
    ws = ops.lstm_seq_ws(batch, T, H, DEV)
    fwd = lambda h=H, w=ws: ops.lstm_seq_bi_fwd(gx, kh, t2("act"), t2("cseq"), t2("hseq"), t2("hprev"), batch, T, h, ws=w)
    bwd = lambda h=H, w=ws: ops.lstm_seq_bi_bwd(None, kh, gx, cseq_in, t2("dz"), batch, T, h, ws=w)
    for call in (fwd, bwd):
        g = torch.cuda.CUDAGraph()
        with pytest.raises(VltfError, match="captured"):
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                call()
        for h, w, match in ((513, ops.lstm_seq_ws(batch, T, 513, DEV), "bad shape"), (0, ws, "bad shape"), (H, ws[:-1], "workspace")):
            with pytest.raises(VltfError, match=match):
                call(h, w)
    torch.cuda.synchronize()
    assert all(g.untouched() for pr in o.values() for g in pr), "lstm_seq_bi: refused, yet an output was written"
    assert not ws.any(), "lstm_seq_bi: refused, yet the workspace was written"
    assert ops.lstm_seq_bi_tag_span(batch, T, 513) == 0
    fwd()                                                         # outside a capture: runs
    ops.lstm_seq_check(ws)


# ---- LRCNEngine, bidirectional ---------------------------------------------------------------------------------------------------------------
MEAN = np.array([99.197148, 105.293620, 109.503945], np.float32)
SHAPE, NCLS, FPC, CLIPS = (67, 67, 3), 7, 3, 2                      # the smallest geometry of tests/test_engine_gpu.py


def lrcn(layers, fusion, hid=8, **kw):
    from vltf_amd.engine import LRCNEngine, NetConfig
    cfg = NetConfig(image_shape=SHAPE, num_classes=NCLS, fpc=FPC, frame_encoding_layer="fc6", lstm_hidden=hid, lstm_layers=layers,
                    fusion=fusion, lstm_bidirectional=True, **kw)
    return cfg, LRCNEngine(cfg, max_clips=CLIPS, device=DEV)


@pytest.mark.parametrize("layers,fusion", [(2, "avg"), (1, "last")])
def test_lrcn_engine_train_step_against_the_reference(layers, fusion):
    """Logits, loss, every gradient and the clipped SGD step against oracle.alexnet_forward followed by blstm_ref, at the bounds
    tests/test_engine_gpu.py holds the unidirectional engine to."""
    from vltf_amd.engine import param_specs
    # seed 6: with seed 5 the frames of the 2-layer case hold a near-tie in the AlexNet tower that fp32 arithmetic resolves the other way
    # -- the ORACLE's own fp32 run then differs from its fp64 run in 1276 of conv1W's 34,848 gradient elements (5e-2 of the largest), the
    # discrete gate flip tests/test_engine_gpu.py describes; with seed 6 its fp32 run agrees to 6e-7 in both cases
    rng = np.random.default_rng(6)
    H = 8
    cfg, eng = lrcn(layers, fusion, H)
    p = B.init_params(rng, NCLS, "fc6", H, layers, SHAPE, fusion)
    assert {n: tuple(s) for n, s in param_specs(cfg)} == {n: v.shape for n, v in p.items()}
    eng.load_params(p)
    frames = rng.integers(0, 256, (CLIPS * FPC,) + SHAPE, dtype=np.uint8)
    onehot = np.eye(NCLS, dtype=np.int32)[rng.integers(0, NCLS, CLIPS)]
    x = frames.astype(np.float32) - MEAN
    newp, loss, gn, logits, grads = B.model_train_step(p, x, onehot, FPC, 0.01, 0.5, "fc6", H, layers, fusion)
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
    """step_graph: the warm-up step, the captured one and three replays equal the eager engine's bit for bit (the bidirectional launches
    run on the graph workspace with replay-safe tags that move between replays)."""
    from vltf_amd.engine import LRCNEngine, NetConfig, init_params
    engines = []
    kw = dict(image_shape=SHAPE, num_classes=NCLS, fpc=FPC, frame_encoding_layer="fc6", lstm_hidden=16, lstm_layers=2, fusion="avg",
              lstm_bidirectional=True, dropout_keep_prob=0.5)
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
    pipes = [PipelineSpec("net", ["main"], "nop", classifier="lstm", lstm_params=(G_H, layers, fusion), lstm_bidirectional=True)]
    ds = {"main": DatasetInfo("vectors", T, 1, G_CLIPS, dim=G_DIM)}
    eng = GraphEngine(pipes, ds, G_C, device=DEV)
    p = init_params_for(model_specs(pipes, ds, G_C), seed=seed, well_scaled=True)
    for k in p:                                                     # biases that are not zero: a bias on the wrong direction would show
        if k.endswith("bias"):
            p[k] = (0.1 * np.random.default_rng(len(k)).standard_normal(p[k].shape)).astype(np.float32)
    eng.load_params(p)
    return eng, p


def graph_reference(p, x, T, layers, fusion, lens):
    out, _ = B.stack_forward(x, p, T, G_H, layers, lens=lens)
    fused = B.fuse(out, T, G_H, fusion, lens)
    head = B.head_name(fusion)
    return fused @ p[head + "_w"].astype(np.float64) + p[head + "_b"]


@pytest.mark.parametrize("fusion", ("reshape", "last"))
def test_graph_engine_with_lengths_against_the_reference(fusion):
    T, lens = 5, [5, 2, 1, 4]
    eng, p = graph_engine(T, fusion=fusion)
    x = (np.random.default_rng(8).standard_normal((G_CLIPS * T, G_DIM))).astype(np.float32)
    got = eng.forward({"main": torch.from_numpy(x).to(DEV)}, seq_len={"net": lens}).cpu().numpy()
    want = graph_reference(p, x, T, 2, fusion, np.array(lens))
    live = B.live_mask(np.array(lens), G_CLIPS, T).reshape(-1) if fusion == "reshape" else slice(None)
    np.testing.assert_allclose(got[live], want[live], rtol=1e-3, atol=1e-3)


def test_graph_engine_padding_is_inert():
    """Other vectors in the dead steps change nothing: live-row logits, the loss and every parameter after the step are bitwise equal."""
    T, lens = 5, [5, 2, 1, 4]
    live = B.live_mask(np.array(lens), G_CLIPS, T).reshape(-1)
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
    """Clips of length 3 in a 5-step batch give what they give in a 3-step model: logits, loss and the step (the backward cell starts at
    the clip's last LIVE step, not at the batch's last step)."""
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


# ---- run_task.py ---------------------------------------------------------------------------------------------------------------------------------
def test_run_task_trains_validates_and_resumes(tmp_path, monkeypatch):
    """A bidirectional YAML over the synthetic dataset: two train steps with a checkpoint, a validation of it, and a second training run
    that resumes from it; the checkpoint holds the bidirectional variables."""
    import glob
    import os
    import yaml
    from tests.test_host_workflow import make_dataset
    from tests.test_run_task_gpu import RAW, write_cfg
    from vltf_amd import run_task
    monkeypatch.setenv("VLTF_PREFETCH", "0")
    monkeypatch.setenv("VLTF_CONV_MATH", "f32")
    folder = str(tmp_path)
    train_path, _, _ = make_dataset(folder, "train.txt", nvid=4, cpv=(1, 1, 1, 1), shape=RAW, seed=1)
    val_path, _, _ = make_dataset(folder, "val.txt", nvid=3, cpv=(2, 1, 2), shape=RAW, seed=2)

    def cfg(name, data_path, phase, **kw):
        path = write_cfg(folder, name, data_path, phase, **kw)
        with open(path) as f:
            c = yaml.safe_load(f)
        c["run"]["network"]["pipelines"][0]["lrcn"].update(lstm_bidirectional=True, lstm_params=[8, 2, "defs.fusion_method.avg"])
        with open(path, "w") as f:
            yaml.safe_dump(c, f)
        return path

    run = os.path.join(folder, "run")
    run_task.main(cfg("train.yml", train_path, "train", epochs=1), seed=3)                 # 4 videos, batch 2: two steps
    ck = glob.glob(os.path.join(run, "checkpoints", "*.weights.npz"))
    assert len(ck) == 1
    saved = np.load(ck[0])
    names = [n for l in range(2) for n in B.param_names(l)]
    assert all(n in saved.files for n in names) and saved["output_fc_w"].shape == (16, 4)
    assert saved[names[0]].shape == (4096 + 8, 32) and saved[names[4]].shape == (16 + 8, 32)
    log = open(glob.glob(os.path.join(run, "log_e2e_train_scratch_*.log"))[0]).read()
    assert "global step: 2" in log
    acc = run_task.main(cfg("val.yml", val_path, "val", resume="latest"))
    assert 0.0 <= acc <= 1.0 and float(open(os.path.join(run, "accuracy_e2e_val_resume")).read()) == acc
    run_task.main(cfg("resume.yml", train_path, "train", resume=ck[0][:-len(".weights.npz")], epochs=2), seed=5)
    log2 = open(glob.glob(os.path.join(run, "log_e2e_train_resume_*.log"))[0]).read()
    assert "Restored training snapshot of epoch 1" in log2 and "global step: 4" in log2
    after = np.load(max(glob.glob(os.path.join(run, "checkpoints", "*.weights.npz")), key=os.path.getmtime))
    assert any(not np.array_equal(after[n], saved[n]) for n in names if n.endswith("kernel"))
