"""The LSTM recurrence kernels against fp64 references on every launch branch: the cluster form of csrc/lstm_cluster.hip with every
group size 1..8 (all three reduction splits, dead pair rows, all four publish widths), ragged last groups that mix those classes in one
launch, two and three launches with a ragged or one-clip last launch, every forward gather unroll (the wide one past 2048 granules
included) and every backward one, pad rows (H no multiple of 4) and a ragged last workgroup (H no multiple of 16), T = 1, 2 and 21;
the per-clip form of csrc/pointwise.hip at H = 513, 1021 and 1024; the step kernels across two workgroups; h0 and c0 as different
tensors and one without the other, dh0 / dc0 each alone, forget biases 0 and 2.5, dout = None, per-clip lengths outside 0..T; the
replay-safe (_st) entry points called eagerly; the refusals.  The cases, their inputs, fp64 references and the restated launch
arithmetic are in tests/lstm_plan.py; tests/test_lstm_geometry.py (CPU) shows that the lists reach those branches and runs the check
functions below against a float32 stand-in with and without defects.

What is compared: the forward's act (the gates: 3e-5 of the largest element, the per-op bound of DESIGN section 2), the WHOLE cseq,
hseq and hprev (`close(rtol=1e-5, atol_rel=1e-6)`); the backward's dz (the same), dh0 and dc0 (`close(1e-4, 1e-5)`) -- directly, and
FROM the reference's own act and cseq rounded to fp32, not from the forward kernel's.  The step kernels' dc is held to dc0's bound.

Every output is a view into a larger allocation (Guarded): sentinels before and behind it must still be there afterwards, the interior
starts as NaN and ends finite.  The workspace is a view of exactly lstm_seq_ws's size in front of a sentinel tail.  dh0 / dc0 that were
not asked for are not touched.  Every run ends with the time-out word of its workspace clear."""
import collections

import numpy as np
import pytest
import torch

from tests import lstm_plan as P
from tests.test_ops_gpu import close, dev, host

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL, GUARD = 12345.0, 64
TOL = dict(act=(3e-5, 3e-5), cseq=(1e-5, 1e-6), hseq=(1e-5, 1e-6), hprev=(1e-5, 1e-6), dz=(1e-5, 1e-6), dh0=(1e-4, 1e-5), dc0=(1e-4, 1e-5),
           dc=(1e-4, 1e-5))
WORST = {}                                                       # output -> worst error / bound seen in this process


@pytest.fixture(scope="module")
def ops():
    import vltf_amd.ops as ops_
    yield ops_
    print("\nlstm geometry, worst error / bound:", " ".join("%s %.3f" % kv for kv in sorted(WORST.items())))


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def cus_of(ops):
    return getattr(ops, "cus", None) or cus()


def put(a, device, dtype=torch.float32):
    if a is None:
        return None
    return dev(a, dtype) if device == DEV else torch.tensor(np.ascontiguousarray(a), dtype=dtype)


def get(t):
    return host(t) if t.is_cuda else t.detach().numpy().copy()


def bits(t):
    return t.contiguous().view(torch.int32)


class Guarded:
    """An output inside a larger allocation: sentinels around it, NaN (or `fill`) inside."""

    def __init__(self, shape, device, fill=float("nan")):
        self.shape = tuple(shape)
        numel = int(np.prod(shape))
        self.flat = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=device)
        self.t = self.flat[GUARD:GUARD + numel].view(self.shape)
        self.t.fill_(fill)
        self.init = self.flat.clone()

    def untouched(self):
        return torch.equal(bits(self.flat), bits(self.init))

    def settle(self, what):
        a = get(self.flat)
        assert (a[:GUARD] == SENTINEL).all() and (a[-GUARD:] == SENTINEL).all(), what + ": guard around the tensor written"
        got = a[GUARD:-GUARD].reshape(self.shape)
        assert np.isfinite(got).all(), what + ": element not written (or not finite)"
        return got


class Workspace:
    """A zeroed workspace of exactly lstm_seq_ws's size -- checked against the restated vl_lstm_seq_ws_bytes -- with a sentinel behind it."""

    def __init__(self, ops, batch, T, H, device):
        n = ops.lstm_seq_ws(batch, T, H, device).numel()
        assert n * 4 == P.ws_bytes(H, cus_of(ops)), "lstm_seq_ws(%d, %d, %d): %d bytes, the plan says %d" % (batch, T, H, n * 4, P.ws_bytes(H, cus_of(ops)))
        self.flat = torch.zeros(n + GUARD, dtype=torch.float32, device=device)
        self.flat[n:] = SENTINEL
        self.t = self.flat[:n]

    def settle(self, ops, what):
        assert not ops.lstm_seq_timed_out(self.t), what + ": a workgroup timed out waiting for its peers"
        assert (get(self.flat[-GUARD:]) == SENTINEL).all(), what + ": written past the workspace"


def within(name, got, want, what):
    """close() at the output's tolerance; the worst error / bound is kept in WORST and named in the message."""
    rtol, atol_rel = TOL[name]
    want = np.asarray(want, np.float64)
    scale = float(np.abs(want).max()) or 1.0
    ratio = float((np.abs(np.asarray(got, np.float64) - want) / (atol_rel * scale + rtol * np.abs(want))).max())
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    close(got, want, rtol=rtol, atol_rel=atol_rel, msg="%s: %s (worst error / bound %.3g)" % (what, name, ratio))


St = collections.namedtuple("St", "state fwd bwd")                # a step state and the tag offsets of the two directions
SEQ_OUT = (("act", 4), ("cseq", 1), ("hseq", 1), ("hprev", 1), ("dz", 4))


def run_seq(ops, ref, batch, T, H, device, variant=P.PLAIN, ws=None, st=None, what=""):
    """lstm_seq_fwd on ref's inputs, lstm_seq_bwd on ref's OWN act and cseq; the memory checks; -> {output: array}."""
    inp = ref.inp
    ws = ws or Workspace(ops, batch, T, H, device)
    gx, kh, h0, c0, dout = (put(a, device) for a in inp)
    lens = put(ref.lens, device, torch.int32)
    o = {k: Guarded((batch * T, w * H), device) for k, w in SEQ_OUT}
    o.update(dh0=Guarded((batch, H), device), dc0=Guarded((batch, H), device))
    asked = dict(dh0=variant.grads in ("dh0", "both"), dc0=variant.grads in ("dc0", "both"))
    fwd = (gx, kh, o["act"].t, o["cseq"].t, o["hseq"].t, o["hprev"].t, batch, T, H)
    bwd = (dout, kh, put(ref.act32, device), put(ref.cseq32, device), o["dz"].t, batch, T, H)
    grads = dict(dh0=o["dh0"].t if asked["dh0"] else None, dc0=o["dc0"].t if asked["dc0"] else None)
    if st is not None:
        assert lens is None
        ops.lstm_seq_fwd_st(*fwd, forget_bias=variant.forget_bias, ws=ws.t, state=st.state, tag_offset=st.fwd, h0=h0, c0=c0)
    else:
        ops.lstm_seq_fwd(*fwd, forget_bias=variant.forget_bias, ws=ws.t, h0=h0, c0=c0, seq_len=lens)
    ws.settle(ops, what + " forward")
    if st is not None:
        ops.lstm_seq_bwd_st(*bwd, ws=ws.t, state=st.state, tag_offset=st.bwd, c0=c0, **grads)
    else:
        ops.lstm_seq_bwd(*bwd, ws=ws.t, c0=c0, seq_len=lens, **grads)
    ws.settle(ops, what + " backward")
    got = {}
    for k, g in o.items():
        if not asked.get(k, True):
            assert g.untouched(), "%s: %s was not asked for, yet it was written" % (what, k)
        else:
            got[k] = g.settle(what + " " + k)
    return got


def same_bits(a, b, what):
    for k in a:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), "%s: %s differs in its bits" % (what, k)


# ---- the checks (tests/test_lstm_geometry.py runs them on the CPU against a stand-in) ---------------------------------------------------
def check_seq(ops, case, device=DEV, variant=P.PLAIN):
    batch, T, H = case
    what = "lstm_seq " + P.case_id(case) + ("" if variant == P.PLAIN else " " + P.case_id(variant))
    span = P.tag_span(batch, T, H, cus_of(ops))
    assert ops.lstm_seq_tag_span(batch, T, H) == span, "%s: lstm_seq_tag_span %d, the plan says %d" % (what, ops.lstm_seq_tag_span(batch, T, H), span)
    ref = P.reference(batch, T, H, variant)
    got = run_seq(ops, ref, batch, T, H, device, variant, what=what)
    for k, v in got.items():
        within(k, v, getattr(ref.fwd, k) if k in P.Forward._fields else getattr(ref.bwd, k), what)
    if ref.lens is not None:
        dead = ~(np.arange(T)[None, :] < P.clamped(ref.lens, T)[:, None]).reshape(-1)
        assert dead.any() and not dead.all()
        for k in ("act", "hseq", "dz"):
            assert not got[k][dead].any(), "%s: dead row of %s not zero" % (what, k)
    if not variant.dout:
        for k in ("dz", "dh0", "dc0"):
            assert k not in got or not got[k].any(), "%s: %s not exactly zero without dout" % (what, k)
    return got


def one_clip(ref, b, T):
    """The reference cut to clip b: what a batch-1 call on that clip's data is handed."""
    rows, row = slice(b * T, (b + 1) * T), slice(b, b + 1)
    inp = ref.inp
    return P.Ref(P.Inputs(inp.gx[rows], inp.kh, inp.h0[row], inp.c0[row], inp.dout[rows]), None, None, ref.act32[rows], ref.cseq32[rows], None)


def check_last_clip_alone(ops, case, device=DEV):
    """The last clip sits alone in the last launch: its rows equal, bit for bit, a batch-1 call on its data (both take the one-clip path)."""
    batch, T, H = case
    what = "lstm_seq " + P.case_id(case)
    assert P.cluster_plan(batch, T, H, cus_of(ops)).launches[-1].nb == 1 and batch > 1
    whole = check_seq(ops, case, device)
    alone = run_seq(ops, one_clip(P.reference(batch, T, H), batch - 1, T), 1, T, H, device, what=what + " last clip alone")
    last = {k: v[-T:] if v.shape[0] == batch * T else v[-1:] for k, v in whole.items()}
    same_bits(alone, last, what + ": the clip alone in the last launch against a batch-1 call")


def check_repeatable(ops, case, device=DEV):
    """Twice on ONE workspace: the same bits (stale exchange words of the first run must not serve the second)."""
    batch, T, H = case
    what = "lstm_seq " + P.case_id(case)
    ws, ref = Workspace(ops, batch, T, H, device), P.reference(batch, T, H)
    first = run_seq(ops, ref, batch, T, H, device, ws=ws, what=what)
    same_bits(first, run_seq(ops, ref, batch, T, H, device, ws=ws, what=what + " again"), what + ": second run on the same workspace")


def check_st(ops, case, device=DEV):
    """lstm_seq_fwd_st / _bwd_st called eagerly, tag origin 1, offsets 0 and span: the plain entry points' bits; then the origin
    2 span further on the same workspace: the same bits again."""
    batch, T, H = case
    what = "lstm_seq_st " + P.case_id(case)
    span = ops.lstm_seq_tag_span(batch, T, H)
    assert span == P.tag_span(batch, T, H, cus_of(ops)), what + ": tag span"
    ref = P.reference(batch, T, H)
    plain = run_seq(ops, ref, batch, T, H, device, what=what + " plain")
    for k, v in plain.items():
        within(k, v, getattr(ref.fwd, k) if k in P.Forward._fields else getattr(ref.bwd, k), what)
    state, ws = ops.step_state(device), Workspace(ops, batch, T, H, device)
    for origin in (1, 1 + 2 * span):
        ops.step_state_set(state, 0, 0.0, origin)
        got = run_seq(ops, ref, batch, T, H, device, ws=ws, st=St(state, 0, span), what="%s origin %d" % (what, origin))
        same_bits(got, plain, "%s origin %d against the plain entry points" % (what, origin))


def check_refusals(ops, device=DEV):
    """H = 1025 and H = 0: "bad shape"; a workspace one word short: "workspace"; nothing is launched."""
    batch, T, H = 2, 2, 16
    ref = P.reference(batch, T, H)
    gx, kh, h0, c0, dout = (put(a, device) for a in ref.inp)
    o = {k: Guarded((batch * T, w * H), device) for k, w in SEQ_OUT}
    ws = ops.lstm_seq_ws(batch, T, H, device)
    fwd = lambda h, w: ops.lstm_seq_fwd(gx, kh, o["act"].t, o["cseq"].t, o["hseq"].t, o["hprev"].t, batch, T, h, ws=w, h0=h0, c0=c0)
    bwd = lambda h, w: ops.lstm_seq_bwd(dout, kh, put(ref.act32, device), put(ref.cseq32, device), o["dz"].t, batch, T, h, ws=w, c0=c0)
    for call in (fwd, bwd):
        for h, w, match in ((1025, ws, "bad shape"), (0, ws, "bad shape"), (H, ws[:-1], "workspace")):
            with pytest.raises(Exception, match=match):
                call(h, w)
    if device == DEV:
        torch.cuda.synchronize()
    assert all(g.untouched() for g in o.values()), "lstm_seq: refused, yet an output was written"
    assert not ws.any(), "lstm_seq: refused, yet the workspace was written"


def check_step(ops, case, device=DEV, forget_bias=1.0, dout=True):
    """lstm_step_fwd over t = 0 .. T - 1 (gh = None at t = 0), lstm_step_bwd over t = T - 1 .. 0, each against one fp64 step."""
    batch, T, H = case
    what = "lstm_step %s fb=%g dout=%d" % (P.case_id(case), forget_bias, dout)
    ref = P.step_reference(batch, T, H, forget_bias, dout)
    gx, gh = put(ref.inp.gx, device), put(ref.gh, device)
    o = {k: Guarded((batch * T, w * H), device) for k, w in SEQ_OUT}
    o["dc"] = Guarded((batch, H), device, fill=0.0)
    for t in range(T):
        ops.lstm_step_fwd(gx, gh[t] if t > 0 else None, o["act"].t, o["cseq"].t, o["hseq"].t, o["hprev"].t, batch, T, t, H, forget_bias=forget_bias)
    d, dh_next, act, cseq = put(ref.inp.dout, device), put(ref.dh_next, device), put(ref.act32, device), put(ref.cseq32, device)
    for t in reversed(range(T)):
        ops.lstm_step_bwd(d, dh_next[t] if t < T - 1 else None, act, cseq, o["dc"].t, o["dz"].t, batch, T, t, H)
    for k, g in o.items():
        want = getattr(ref.fwd, k) if k in P.Forward._fields else (ref.bwd.dz if k == "dz" else ref.bwd.dc0)
        got = g.settle(what + " " + k)
        within(k, got, want, what)
        if not dout and k in ("dz", "dc"):
            assert not got.any(), "%s: %s not exactly zero without dout" % (what, k)


def branches_reached(cus):
    """Every case's plan at `cus` compute units holds the branch the case is listed for; together the lists reach every forward
    gather class, every backward one, every group size and three launches."""
    plan = lambda c: P.cluster_plan(*P.resolve(c, cus), cus)
    for k, c in enumerate(P.FULL, 1):
        p = plan(c)
        assert (p.W, p.Hp, c.H % P.LU) == (32, 500, 2) and P.group_sizes(p) == [[k] * p.maxG], (c, P.group_sizes(p))
        assert {(g.S, g.publish) for g in p.launches[0].groups} == {((1, 1), (1, 2), (2, 4), (2, 4), (4, 8), (4, 8), (4, 8), (4, 8))[k - 1]}
    rag = [plan(c) for c in P.RAGGED]
    assert all(len(p.launches) == 1 for p in rag)
    assert sum(len({g.publish for g in p.launches[0].groups}) > 1 for p in rag) >= 3                 # publish widths mixed in one launch
    assert sum(len({g.S for g in p.launches[0].groups}) > 1 for p in rag) >= 2                       # reduction splits mixed
    assert {1, 2} <= {p.launches[0].groups[-1].nclips for p in rag}
    assert any({5, 3} <= set(P.group_sizes(p)[0]) or {5, 4} <= set(P.group_sizes(p)[0]) for p in rag)  # dead pair rows beside full ones
    multi = [plan(c) for c in P.MULTI]
    assert [len(p.launches) for p in multi] == [2, 2, 3, 2]
    assert multi[0].lds_fwd == 149504 <= 150 * 1024 and multi[0].Hp == 512 and multi[3].Hp == 500
    assert multi[0].launches[1].nb == multi[3].launches[1].nb == 1
    second = P.group_sizes(multi[1])[1]
    assert len(second) > 1 and second[-1] < second[0]                                                # a ragged second launch
    assert all(l.nb == p.chunk for p in multi for l in p.launches[:-1]) and multi[2].launches[2].nb == 3
    g37, g256, g512, g257, g250 = (plan(c) for c in P.GATHER)
    assert (g37.W, g37.bwd_gather, g256.W, g256.bwd_gather, g257.W, g257.bwd_gather) == (3, 4, 16, 16, 17, 32)
    assert [g.nclips * 256 for g in g256.launches[0].groups] == [256] and g256.launches[0].groups[0].gather == 1
    assert any(g.nclips * 256 == 512 and g.gather == 2 for g in g512.launches[0].groups)
    assert all(g.nclips == 8 and g.gather == 16 for g in g257.launches[0].groups) and len(g257.launches) == 1
    assert 8 * 257 == 2056 and 2056 % 256 == 8 < 64                                                  # wave 0: lanes with 9 and with 8 slots
    assert (g250.Hp, g250.W) == (252, 16) and P.group_sizes(g250) == [[1, 1, 1]]
    assert [c.T for c in P.TIME] == [1, 2, 21] and all(len(plan(c).launches) == 1 and len(plan(c).launches[0].groups) > 1 for c in P.TIME)
    plans = [plan(c) for c in P.CLUSTER]
    groups = [g for p in plans for l in p.launches for g in l.groups]
    assert {g.gather for g in groups} == {1, 2, 8, 16} and {p.bwd_gather for p in plans} == {4, 16, 32}
    assert {g.nclips for g in groups} == set(range(1, 9)) and {g.publish for g in groups} == {1, 2, 4, 8}
    assert max(len(p.launches) for p in plans) >= 3
    per = [P.perclip_plan(c.H) for c in P.PERCLIP]
    assert [(p.HP, p.kq, p.fwd_tail, p.bwd_tail) for p in per] == [(576, 1, 1, 4), (1024, 1, 13, 4), (1024, 1, 0, 0)]
    assert per[1].threads - 1021 == 3 and per[2].threads == 1024
    assert P.step_workgroups(P.STEP.batch, P.STEP.H) == 2 and (P.STEP.batch * P.STEP.H) % 256


# ---- the tests ------------------------------------------------------------------------------------------------------------------------
def test_the_case_lists_reach_their_branches_on_this_device():
    branches_reached(cus())


@pytest.mark.parametrize("case", P.CLUSTER, ids=P.case_id)
def test_lstm_cluster(ops, case):
    """Group sizes 1..8, ragged last groups, 2 and 3 launches, every gather class, T = 1, 2, 21: act, cseq, hseq, hprev, dz, dh0, dc0."""
    check_seq(ops, P.resolve(case, cus()))


@pytest.mark.parametrize("case", P.PERCLIP, ids=P.case_id)
def test_lstm_perclip(ops, case):
    """H = 513 (tails 1 and 4), 1021 (idle lanes, tail 13), 1024 (a full 1024-thread workgroup)."""
    check_seq(ops, case)


@pytest.mark.parametrize("variant", P.VARIANTS, ids=P.case_id)
@pytest.mark.parametrize("case", P.VARIANT_CASES, ids=P.case_id)
def test_lstm_seq_variants(ops, case, variant):
    """h0 / c0 / neither, dh0 / dc0 / neither, forget bias 0 and 2.5, dout = None, lengths with 0, T, -3 and T + 5."""
    check_seq(ops, P.resolve(case, cus()), variant=variant)


@pytest.mark.parametrize("case", (P.MULTI[0], P.MULTI[3]), ids=P.case_id)
def test_a_clip_alone_in_the_last_launch_equals_a_batch_of_one(ops, case):
    check_last_clip_alone(ops, P.resolve(case, cus()))


def test_lstm_cluster_is_repeatable_on_one_workspace(ops):
    check_repeatable(ops, P.resolve(P.FULL[6], cus()))


@pytest.mark.parametrize("case", P.ST_CASES, ids=P.case_id)
def test_replay_safe_entry_points_called_eagerly(ops, case):
    check_st(ops, P.resolve(case, cus()))


def test_lstm_seq_refusals(ops):
    check_refusals(ops)


@pytest.mark.parametrize("forget_bias,dout", [(1.0, True), (0.0, True), (2.5, True), (1.0, False)])
def test_lstm_step_kernels(ops, forget_bias, dout):
    """batch H = 500: two workgroups, the second ragged."""
    check_step(ops, P.STEP, forget_bias=forget_bias, dout=dout)
