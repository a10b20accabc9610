"""The CPU half of tests/test_lstm_geometry_gpu.py (no GPU needed).  Coverage: at 256 and at 64 compute units the case lists of
tests/lstm_plan.py reach every launch branch they are there for, by the restated launch arithmetic; the references of lstm_plan are
the oracle's (1e-12).  Discrimination: the very check functions of the GPU half run here against a numpy float32 stand-in with the
`ops` signatures -- it follows the plan: launches, groups, pair rows, reduction slices, pad rows, one partial per source workgroup --
and pass, which also shows that float32 arithmetic stays inside every tolerance on each chosen input, and fail for each defect the
harness is there to catch."""
import numpy as np
import pytest
import torch

from oracle import lrcn_oracle as O
from tests import lstm_plan as P
from tests import seq_len_ref
from tests import test_lstm_geometry_gpu as G

CUS = (256, 64)
F32 = np.float32


# ---- coverage -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cus", CUS)
def test_the_case_lists_reach_their_branches(cus):
    G.branches_reached(cus)


def test_the_batches_at_256_compute_units_are_the_ones_the_cases_were_chosen_by():
    sizes = lambda c: P.group_sizes(P.cluster_plan(*P.resolve(c, 256), 256))
    assert (P.max_groups(498, 256), P.max_groups(512, 256), P.max_groups(257, 256), P.max_groups(256, 256)) == (8, 8, 15, 16)
    assert [P.resolve(c, 256).batch for c in P.RAGGED] == [9, 17, 33, 49] and sizes(P.RAGGED[2]) == [[5, 5, 5, 5, 5, 5, 3]]
    assert [P.resolve(c, 256).batch for c in P.MULTI] == [65, 73, 131, 65] and sizes(P.MULTI[1])[1] == [2, 2, 2, 2, 1]
    assert max(P.resolve(c, 256).batch * c.T * 4 * c.H * 4 for c in P.CLUSTER) < 4 * 2 ** 20                    # the gates of the largest case
    assert [P.resolve(c, 64).batch for c in P.MULTI] == [17, 19, 35, 17]


def test_the_130_clip_case_of_test_ops_gpu_is_one_launch():
    """(130, 5, 32, 128) of test_lstm_persistent_kernels: W = 8, so one launch holds 256 clips; (130, 5, 32, 256) of test_seq_len_gpu splits."""
    assert len(P.cluster_plan(130, 5, 128, 256).launches) == 1 and len(P.cluster_plan(130, 5, 256, 256).launches) == 2
    assert {g.gather for c in ((20, 7, 512), (64, 16, 256), (130, 5, 256)) for l in P.cluster_plan(*c, 256).launches for g in l.groups} <= {1, 2, 8}


def test_the_per_clip_form_never_splits_its_reduction():
    assert {P.perclip_plan(H).kq for H in range(513, 1025)} == {1} and {P.perclip_plan(H).kq for H in (64, 256, 257, 512)} == {4, 2}
    assert all(P.perclip_plan(H).threads <= 1024 and P.perclip_plan(H).lds_fwd <= 64 * 1024 for H in range(513, 1025))


@pytest.mark.parametrize("cus", CUS)
def test_lds_and_workspace_of_every_hidden_size(cus):
    for H in range(1, 513):
        p = P.cluster_plan(1, 1, H, cus)
        assert max(p.lds_fwd, p.lds_bwd) <= 150 * 1024 and p.W * p.maxG <= max(cus, p.W)
        assert P.ws_bytes(H, cus) == 256 + max(8 * p.xch_bwd, 16 * H * H) and p.xch_bwd >= p.xch_fwd
    assert P.ws_bytes(600, cus) == 256 + 16 * 600 * 600 and P.ws_bytes(0, cus) == 0
    assert P.tag_span(600, 4, 600, cus) == 0 and P.tag_span(1, 7, 512, cus) == 8


# ---- the references are the oracle's ------------------------------------------------------------------------------------------------------
def as_layer(kh, forget_bias):
    """The layer of the oracle whose input projection is the identity: x = gx, kernel = [I; kh], the forget-bias shift in the bias."""
    H = kh.shape[0]
    bias = np.zeros(4 * H)
    bias[2 * H:3 * H] = forget_bias - O.FORGET_BIAS
    return np.concatenate([np.eye(4 * H), kh.astype(np.float64)], axis=0), bias


@pytest.mark.parametrize("forget_bias", [1.0, 0.0, 2.5])
def test_the_references_are_the_oracle(forget_bias):
    b, T, H = 3, 5, 7
    inp = P.inputs(b, T, H)
    kernel, bias = as_layer(inp.kh, forget_bias)
    out, _, cache = O.lstm_layer_forward(inp.gx.reshape(b, T, 4 * H), kernel, bias, h0=inp.h0, c0=inp.c0)
    fwd = P.forward_ref(inp.gx, inp.kh, T, inp.h0, inp.c0, forget_bias)
    np.testing.assert_allclose(fwd.hseq.reshape(b, T, H), out, rtol=0, atol=1e-12)
    np.testing.assert_allclose(fwd.cseq.reshape(b, T, H), np.stack(cache["cs"], axis=1), rtol=0, atol=1e-12)
    np.testing.assert_allclose(fwd.act.reshape(b, T, 4 * H), np.stack([np.concatenate(g[:4], axis=1) for g in cache["gates"]], axis=1), rtol=0, atol=1e-12)
    np.testing.assert_allclose(fwd.hprev.reshape(b, T, H), np.stack([g[5] for g in cache["gates"]], axis=1), rtol=0, atol=1e-12)
    dz, _, _, dh0, dc0 = O.lstm_layer_backward(kernel, cache, inp.dout.reshape(b, T, H))              # dx = dz I
    bwd = P.backward_ref(inp.dout, inp.kh, T, fwd.act, fwd.cseq, inp.c0)
    for got, want in ((bwd.dz.reshape(b, T, 4 * H), dz), (bwd.dh0, dh0), (bwd.dc0, dc0)):
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


def test_the_references_with_lengths_are_the_oracle_on_the_live_prefix():
    b, T, H = 6, 5, 7
    inp, lens = P.inputs(b, T, H), P.lengths(b, T)
    assert set(lens[[0, 1, 2, -1]]) == {0, T, -3, T + 5}
    kernel, bias = as_layer(inp.kh, 1.0)
    L = P.clamped(lens, T)
    some = np.flatnonzero(L > 0)                                  # the oracle cannot unroll zero steps: the empty clips are checked below
    r = seq_len_ref.lstm_layer(inp.gx.reshape(b, T, 4 * H)[some], kernel, bias, L[some], s0=inp.h0[some],
                               dout=inp.dout.reshape(b, T, H)[some].astype(np.float64))
    fwd = P.forward_ref(inp.gx, inp.kh, T, inp.h0, inp.h0, 1.0, lens)
    bwd = P.backward_ref(inp.dout, inp.kh, T, fwd.act, fwd.cseq, inp.h0, lens)
    for got, want in ((fwd.hseq, r["out"]), (fwd.cseq, r["c"]), (fwd.hprev, r["hprev"]), (bwd.dz, r["dx"]), (bwd.dh0, r["dh0"]), (bwd.dc0, r["dc0"])):
        np.testing.assert_allclose(got.reshape((b,) + want.shape[1:])[some], want, rtol=0, atol=1e-12)
    for i in np.flatnonzero(L == 0):
        rows = slice(i * T, (i + 1) * T)
        assert not fwd.act[rows].any() and not fwd.hseq[rows].any() and not bwd.dz[rows].any() and not bwd.dh0[i].any() and not bwd.dc0[i].any()
        assert (fwd.cseq[rows] == inp.h0[i]).all() and (fwd.hprev[rows] == inp.h0[i]).all()


def test_the_step_references_are_the_sequence_references():
    b, T, H = 3, 4, 7
    inp = P.inputs(b, T, H)
    kh = inp.kh.astype(np.float64)
    seq = P.forward_ref(inp.gx, inp.kh, T, forget_bias=2.5)
    gh = [np.zeros((b, 4 * H))] + [seq.hseq.reshape(b, T, H)[:, t - 1] @ kh for t in range(1, T)]
    for got, want in zip(P.forward_ref(inp.gx, None, T, forget_bias=2.5, gh=gh), seq):
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    bseq = P.backward_ref(inp.dout, inp.kh, T, seq.act, seq.cseq)
    dh_next = [bseq.dz.reshape(b, T, 4 * H)[:, t + 1] @ kh.T for t in range(T - 1)] + [None]
    step = P.backward_ref(inp.dout, None, T, seq.act, seq.cseq, dh_next=dh_next)
    np.testing.assert_allclose(step.dz, bseq.dz, rtol=0, atol=1e-12)
    np.testing.assert_allclose(step.dc0, bseq.dc0, rtol=0, atol=1e-12)
    ref = P.step_reference(b, T, H, 2.5)
    assert np.abs(ref.fwd.hseq - seq.hseq).max() < 1e-6 and np.abs(ref.bwd.dz - P.backward_ref(inp.dout, inp.kh, T, ref.act32, ref.cseq32).dz).max() < 1e-6


# ---- the stand-in -------------------------------------------------------------------------------------------------------------------
DEFECTS = ("clip offset", "seq_len offset", "ragged workgroup", "pad rows", "last slice", "pair partner", "stale gather", "forget bias 1",
           "h0 c0 swapped", "c0 ignored", "partial left out", "dead row", "unwritten", "guard", "past the workspace")


def gates(z, H, forget_bias):
    return O.sigmoid(z[:, :H]), np.tanh(z[:, H:2 * H]), O.sigmoid(z[:, 2 * H:3 * H] + F32(forget_bias)), O.sigmoid(z[:, 3 * H:])


def nd(t):
    return None if t is None else t.numpy()


class StandIn:
    """The operators' contracts in numpy float32 on CPU tensors, cut as the plan says -- and, on request, one defect."""

    def __init__(self, defect=None, cus=64):
        assert defect is None or defect in DEFECTS
        self.defect, self.cus = defect, cus

    # -- plumbing
    def lstm_seq_ws(self, batch, T, H, device):
        return torch.zeros(P.ws_bytes(H, self.cus) // 4)

    def lstm_seq_tag_span(self, batch, T, H):
        return P.tag_span(batch, T, H, self.cus)

    def lstm_seq_timed_out(self, ws):
        return False

    def step_state(self, device):
        return torch.zeros(16, dtype=torch.int32)

    def step_state_set(self, state, step, lr, tag_origin):
        state[2] = tag_origin

    def accept(self, name, batch, T, H, ws):
        if not (batch > 0 and T > 0 and 0 < H <= 1024):
            raise RuntimeError("%s: bad shape (hidden size must be <= 1024)" % name)
        if ws is None or ws.numel() * 4 < P.ws_bytes(H, self.cus):
            raise RuntimeError("%s: workspace smaller than vl_lstm_seq_ws_bytes" % name)
        ws[-1] = 1.0                                             # the last exchange word is the workspace's to write
        if self.defect == "past the workspace":
            ws.as_strided((1,), (1,), ws.storage_offset() + ws.numel()).zero_()

    def stray(self, out):
        if self.defect == "guard":
            out.as_strided((1,), (1,), out.storage_offset() - 1).zero_()
        if self.defect == "unwritten":
            out.view(-1)[-1] = float("nan")

    def shape(self, batch, T, H):
        """(W, Hp, [(read offset, lengths offset, write offset, clips, KP)] of every group of every launch)."""
        if H > P.LH_MAX:                                          # the per-clip form: a clip is its own workgroup, one slice, no pad rows
            return 1, H, [(b, b, b, 1, 1) for b in range(batch)]
        plan = P.cluster_plan(batch, T, H, self.cus)
        return plan.W, plan.Hp, [(0 if self.defect == "clip offset" and k else l.b0 + g.clip0, 0 if self.defect == "seq_len offset" and k else l.b0 + g.clip0,
                                  l.b0 + g.clip0, g.nclips, g.KP) for k, l in enumerate(plan.launches) for g in l.groups]

    def units(self, W, H):
        """The hidden units that are written."""
        return (W - 1) * P.LU if self.defect == "ragged workgroup" and H % P.LU else H

    # -- the sequence kernels
    def lstm_seq_fwd(self, gx, kh, act, cseq, hseq, hprev, batch, T, H, forget_bias=1.0, ws=None, h0=None, c0=None, seq_len=None):
        self.accept("vl_lstm_seq_fwd", batch, T, H, ws)
        if self.defect == "h0 c0 swapped":
            h0, c0 = c0, h0
        if self.defect == "forget bias 1":
            forget_bias = 1.0
        gx3, kh, h0, c0, lens = gx.numpy().reshape(batch, T, 4 * H), kh.numpy(), nd(h0), nd(c0), nd(seq_len)
        out = [t.numpy().reshape(batch, T, -1) for t in (act, cseq, hseq, hprev)]
        W, Hp, groups = self.shape(batch, T, H)
        U = self.units(W, H)
        Ks = np.zeros((Hp, 4 * H), F32)
        Ks[:H] = kh
        for rd, ld, wr, n, KP in groups:
            S = 4 // KP
            hb = np.zeros((P.CPG, Hp), F32)                      # rows of clips the group does not have, and columns H .. Hp - 1: zeros
            if h0 is not None:
                hb[:n, :H] = h0[rd:rd + n]
            if self.defect == "pad rows":
                hb[:, H:], Ks[H:] = 1, 1
            c = np.zeros((n, H), F32) if c0 is None else c0[rd:rd + n].copy()
            L = np.full(n, T) if lens is None else np.clip(lens[ld:ld + n], 0, T)
            slices = P.reduction_slices(H, KP)
            if self.defect == "last slice" and KP == 4:
                slices = slices[:-1]
            published = []
            for t in range(T):
                live = (t < L)[:, None]
                if self.defect == "stale gather" and t >= 3:     # one granule: the same-parity buffer's word of two steps ago is taken
                    hb[0, 0] = published[t - 3][0, 0]
                rows = hb[:n].copy()
                if self.defect == "pair partner" and n > 1 and n % 2:
                    rows[n - 1] = hb[n - 1 - S if n - 1 >= S else n - 1 + S]
                z = np.zeros((n, 4 * H), F32)
                for kb, ke in slices:                            # whole quads: the last one may reach into the pad rows
                    ke = min(Hp, P.ceil_div(ke, 4) * 4)
                    z += rows[:, kb:ke] @ Ks[kb:ke]
                gi, gj, gf, go = gates(gx3[rd:rd + n, t] + z, H, forget_bias)
                hp = hb[:n, :H].copy()
                cn = c * gf + gi * gj
                hn = np.tanh(cn) * go
                c = np.where(live, cn, c)
                a = np.where(live, np.concatenate([gi, gj, gf, go], axis=1), F32(0))
                for q in range(4):
                    out[0][wr:wr + n, t, q * H:q * H + U] = a[:, q * H:q * H + U]
                out[1][wr:wr + n, t, :U] = c[:, :U]
                out[2][wr:wr + n, t, :U] = np.where(live, hn, hp if self.defect == "dead row" else F32(0))[:, :U]
                out[3][wr:wr + n, t, :U] = hp[:, :U]
                hb[:n, :H] = np.where(live, hn, hp)
                published.append(hb[:n, :H].copy())
        self.stray(hseq)

    def lstm_seq_bwd(self, dout, kh, act, cseq, dz, batch, T, H, ws=None, c0=None, dh0=None, dc0=None, seq_len=None):
        self.accept("vl_lstm_seq_bwd", batch, T, H, ws)
        kh, c0, lens = kh.numpy(), nd(c0), nd(seq_len)
        act3, cseq3, dz3 = (t.numpy().reshape(batch, T, -1) for t in (act, cseq, dz))
        dout3 = None if dout is None else dout.numpy().reshape(batch, T, H)
        W, Hp, groups = self.shape(batch, T, H)
        U = self.units(W, H)
        cols = [np.concatenate([q * H + np.arange(w * P.LU, min(H, (w + 1) * P.LU)) for q in range(4)]) for w in range(W)] if H <= P.LH_MAX else \
            [np.arange(4 * H)]
        for rd, ld, wr, n, _ in groups:
            L = np.full(n, T) if lens is None else np.clip(lens[ld:ld + n], 0, T)
            dc, dh = np.zeros((n, H), F32), np.zeros((n, H), F32)
            for t in reversed(range(T)):
                live = (t < L)[:, None]
                gi, gj, gf, go = (act3[rd:rd + n, t, q * H:(q + 1) * H] for q in range(4))
                cp = cseq3[rd:rd + n, t - 1] if t > 0 else (np.zeros((n, H), F32) if c0 is None or self.defect == "c0 ignored" else c0[rd:rd + n])
                din = dh if dout3 is None else dout3[rd:rd + n, t] + dh
                tc = np.tanh(cseq3[rd:rd + n, t])
                dcv = dc + din * go * (1 - tc * tc)
                z = np.concatenate([dcv * gj * gi * (1 - gi), dcv * gi * (1 - gj * gj), dcv * cp * gf * (1 - gf), din * tc * go * (1 - go)], axis=1)
                z = np.where(live, z, F32(0)).astype(F32)
                dc = np.where(live, dcv * gf, dc).astype(F32)
                for q in range(4):
                    dz3[wr:wr + n, t, q * H:q * H + U] = z[:, q * H:q * H + U]
                if t > 0 or dh0 is not None:                     # one partial per source workgroup, summed in workgroup order
                    dh = np.zeros((n, H), F32)
                    for w, cw in enumerate(cols):
                        if not (self.defect == "partial left out" and w == len(cols) - 1):
                            dh += z[:, cw] @ kh[:, cw].T
            if dh0 is not None:
                dh0.numpy()[wr:wr + n, :U] = dh[:, :U]
            if dc0 is not None:
                dc0.numpy()[wr:wr + n, :U] = dc[:, :U]
        self.stray(dz)

    def lstm_seq_fwd_st(self, gx, kh, act, cseq, hseq, hprev, batch, T, H, forget_bias=1.0, ws=None, state=None, tag_offset=0, h0=None, c0=None):
        assert state is not None and int(state[2]) >= 1
        self.lstm_seq_fwd(gx, kh, act, cseq, hseq, hprev, batch, T, H, forget_bias, ws, h0, c0)

    def lstm_seq_bwd_st(self, dout, kh, act, cseq, dz, batch, T, H, ws=None, state=None, tag_offset=0, c0=None, dh0=None, dc0=None):
        assert state is not None and int(state[2]) >= 1
        self.lstm_seq_bwd(dout, kh, act, cseq, dz, batch, T, H, ws, c0, dh0, dc0)

    # -- the step kernels
    def lstm_step_fwd(self, gx, gh, act, cseq, hseq, hprev, batch, T, t, H, forget_bias=1.0):
        if self.defect == "forget bias 1":
            forget_bias = 1.0
        act3, cseq3, hseq3, hprev3 = (a.numpy().reshape(batch, T, -1) for a in (act, cseq, hseq, hprev))
        z = gx.numpy().reshape(batch, T, 4 * H)[:, t]
        gi, gj, gf, go = gates(z if gh is None else z + gh.numpy(), H, forget_bias)
        c = gi * gj if t == 0 else cseq3[:, t - 1] * gf + gi * gj
        act3[:, t], cseq3[:, t], hseq3[:, t] = np.concatenate([gi, gj, gf, go], axis=1), c, np.tanh(c) * go
        hprev3[:, t] = 0 if t == 0 else hseq3[:, t - 1]
        if t == T - 1:
            self.stray(hseq)

    def lstm_step_bwd(self, dout, dh_next, act, cseq, dc, dz, batch, T, t, H):
        act3, cseq3, dz3 = (a.numpy().reshape(batch, T, -1) for a in (act, cseq, dz))
        din = np.zeros((batch, H), F32) if dout is None else dout.numpy().reshape(batch, T, H)[:, t]
        if dh_next is not None:
            din = din + dh_next.numpy()
        gi, gj, gf, go = (act3[:, t, q * H:(q + 1) * H] for q in range(4))
        cp = cseq3[:, t - 1] if t > 0 else np.zeros((batch, H), F32)
        tc = np.tanh(cseq3[:, t])
        dcv = dc.numpy() + din * go * (1 - tc * tc)
        dz3[:, t] = np.concatenate([dcv * gj * gi * (1 - gi), dcv * gi * (1 - gj * gj), dcv * cp * gf * (1 - gf), din * tc * go * (1 - go)], axis=1)
        dc.numpy()[...] = dcv * gf
        if t == 0:
            self.stray(dz)


# ---- discrimination -----------------------------------------------------------------------------------------------------------------
CPU_CUS = 64
R = lambda c: P.resolve(c, CPU_CUS)


def jobs():
    """(check, case, keywords) of everything the GPU half runs."""
    out = [(G.check_seq, R(c), {}) for c in P.CLUSTER + P.PERCLIP]
    out += [(G.check_seq, R(c), dict(variant=v)) for c in P.VARIANT_CASES for v in P.VARIANTS]
    out += [(G.check_last_clip_alone, R(c), {}) for c in (P.MULTI[0], P.MULTI[3])] + [(G.check_repeatable, R(P.FULL[6]), {})]
    out += [(G.check_st, R(c), {}) for c in P.ST_CASES]
    out += [(G.check_step, P.STEP, dict(forget_bias=fb, dout=d)) for fb, d in ((1.0, True), (0.0, True), (2.5, True), (1.0, False))]
    return out


def job_id(j):
    return j[0].__name__[6:] + "-" + P.case_id(j[1]) + "".join("-" + (P.case_id(v) if isinstance(v, tuple) else "%s=%g" % (k, v)) for k, v in j[2].items())


@pytest.mark.parametrize("job", jobs(), ids=job_id)
def test_a_correct_stand_in_passes(job):
    """Float32 arithmetic is inside every tolerance on each chosen input."""
    check, case, kw = job
    check(StandIn(cus=CPU_CUS), case, "cpu", **kw)


def test_a_correct_stand_in_is_refused_like_the_library():
    G.check_refusals(StandIn(cus=CPU_CUS), "cpu")


LENS, FB0 = dict(variant=P.Variant(lens=True)), dict(variant=P.Variant(forget_bias=0.0))
CAUGHT = [
    ("clip offset", G.check_seq, R(P.MULTI[0]), {}, "Not equal to tolerance"),
    ("clip offset", G.check_seq, R(P.MULTI[2]), {}, "Not equal to tolerance"),
    ("seq_len offset", G.check_seq, R(P.MULTI[0]), LENS, "Not equal to tolerance"),
    ("ragged workgroup", G.check_seq, R(P.FULL[0]), {}, "not written"),
    ("ragged workgroup", G.check_seq, R(P.GATHER[0]), {}, "not written"),
    ("pad rows", G.check_seq, R(P.FULL[1]), {}, "Not equal to tolerance"),
    ("pad rows", G.check_seq, R(P.GATHER[4]), {}, "Not equal to tolerance"),
    ("last slice", G.check_seq, R(P.FULL[0]), {}, "Not equal to tolerance"),
    ("last slice", G.check_seq, R(P.FULL[1]), {}, "Not equal to tolerance"),
    ("pair partner", G.check_seq, R(P.FULL[2]), {}, "Not equal to tolerance"),
    ("pair partner", G.check_seq, R(P.FULL[4]), {}, "Not equal to tolerance"),
    ("pair partner", G.check_seq, R(P.RAGGED[2]), {}, "Not equal to tolerance"),
    ("stale gather", G.check_seq, R(P.TIME[2]), {}, "Not equal to tolerance"),
    ("forget bias 1", G.check_seq, R(P.VARIANT_CASES[0]), FB0, "act"),
    ("forget bias 1", G.check_seq, R(P.PERCLIP[0]), dict(variant=P.Variant(forget_bias=2.5)), "act"),
    ("forget bias 1", G.check_step, P.STEP, dict(forget_bias=2.5), "act"),
    ("h0 c0 swapped", G.check_seq, R(P.FULL[0]), {}, "Not equal to tolerance"),
    ("h0 c0 swapped", G.check_seq, R(P.PERCLIP[1]), {}, "Not equal to tolerance"),
    ("c0 ignored", G.check_seq, R(P.FULL[0]), {}, "dz"),
    ("c0 ignored", G.check_seq, R(P.VARIANT_CASES[3]), dict(variant=P.Variant(state="c0")), "dz"),
    ("partial left out", G.check_seq, R(P.FULL[0]), {}, "dz"),
    ("partial left out", G.check_seq, R(P.GATHER[0]), dict(variant=P.Variant(grads="dh0")), "dz"),
    ("dead row", G.check_seq, R(P.VARIANT_CASES[1]), LENS, "hseq"),
    ("unwritten", G.check_seq, R(P.FULL[0]), {}, "not written"),
    ("unwritten", G.check_step, P.STEP, {}, "not written"),
    ("guard", G.check_seq, R(P.FULL[0]), {}, "guard around the tensor written"),
    ("guard", G.check_seq, R(P.PERCLIP[1]), {}, "guard around the tensor written"),
    ("guard", G.check_step, P.STEP, {}, "guard around the tensor written"),
    ("past the workspace", G.check_seq, R(P.MULTI[2]), {}, "written past the workspace"),
]


def test_every_listed_defect_is_tried():
    assert {c[0] for c in CAUGHT} == set(DEFECTS)


@pytest.mark.parametrize("defect,check,case,kw,message", CAUGHT,
                         ids=lambda v: v if isinstance(v, str) else getattr(v, "__name__", None) or (P.case_id(v) if isinstance(v, tuple) else "kw"))
def test_each_defect_is_caught(defect, check, case, kw, message):
    check(StandIn(cus=CPU_CUS), case, "cpu", **kw)               # the same case passes without the defect
    with pytest.raises(AssertionError, match=message):
        check(StandIn(defect, CPU_CUS), case, "cpu", **kw)
