"""The launch arithmetic of the LSTM recurrence restated in plain Python for the tests: vl_lstm_cluster_run of csrc/lstm_cluster.hip
(launches, groups, clips per group from H and the CU count) with what its kernels derive from a group's clip count (reduction split,
pair rows, gather unroll, partial-publish width), vl_lstm_seq_ws_bytes, vl_lstm_seq_tag_span, the per-clip form and the step kernels
of csrc/pointwise.hip -- and the case lists, seeded inputs and fp64 references that tests/test_lstm_geometry.py (CPU) and
tests/test_lstm_geometry_gpu.py share.  Nothing here imports the package: the kernels are checked AGAINST these.  Every plan is a
function of (batch, T, H, CUs); batches are written in mg = maxG(H, CUs), the groups one launch holds, and chunk = 8 mg, its clips.

The reduction splits kq = 2 and kq = 4 of the per-clip form cannot be reached in the product build: they need H <= 512 (HP <= 512),
where vl_lstm_seq_fwd / _bwd take the cluster form, and the switch that forces the per-clip form there (VL_LSTM_PERCLIP) is compiled
out of that build.  perclip_plan therefore answers kq = 1 for every H the per-clip form is given (tests/test_lstm_geometry.py sweeps
513..1024); the code is left alone.

The references take THE KERNEL'S OWN INPUTS: forward_ref the input projections gx, the recurrent weights kh, h0, c0, the forget bias
and optional lengths; backward_ref dout, kh, and act / cseq as forward_ref gives them ROUNDED TO fp32 (`rounded`), so that a wrong
forward can neither hide nor excuse the backward.  They are few-line restatements; tests/test_lstm_geometry.py proves them equal to
oracle.lstm_layer_forward / _backward and tests.seq_len_ref.lstm_layer to 1e-12 (the oracle hard-codes the forget bias 1.0: another
one is a shift of the f segment of the bias)."""
import collections
import functools

import numpy as np

from oracle import lrcn_oracle as O

F64 = np.float64
LU, LC, CPG, LNT, LH_MAX, STATUS_BYTES = 16, 64, 8, 256, 512, 256


def ceil_div(a, b):
    return -(-a // b)


# ---- launchers ----------------------------------------------------------------------------------------------------------------------
Group = collections.namedtuple("Group", "clip0 nclips S KP gather publish")
# clip0    first clip of the group within its launch; nclips: 1..8
# S, KP    forward: S clip pairs (rows slot, slot + S) x KP = 4 / S slices of the reduction over h
# gather   forward gather unroll of the busiest thread: 1, 2, 8 or 16 granules (ceil(nclips H / 256))
# publish  backward publish_partials<NC>: 1, 2, 4 or 8
Launch = collections.namedtuple("Launch", "b0 nb G cpg groups")
ClusterPlan = collections.namedtuple("ClusterPlan", "W Hp maxG chunk launches bwd_gather lds_fwd lds_bwd xch_fwd xch_bwd")
# bwd_gather  4, 16 or 32 source workgroups per gather, from W;  xch_*: exchange granules (8 bytes each) the launcher asks for


def max_groups(H, cus):
    """mg: the groups of W = ceil(H / 16) workgroups that are resident at once, one workgroup per CU."""
    return max(1, cus // ceil_div(H, LU))


def group_of(clip0, nclips, H):
    S = 4 if nclips > 4 else (2 if nclips > 2 else 1)
    share = ceil_div(nclips * H, LNT)
    gather = 1 if share <= 1 else (2 if share <= 2 else (8 if share <= 8 else CPG * LH_MAX // LNT))
    publish = 8 if nclips > 4 else (4 if nclips > 2 else (2 if nclips > 1 else 1))
    return Group(clip0, nclips, S, 4 // S, gather, publish)


def cluster_plan(batch, T, H, cus):
    """What vl_lstm_cluster_run launches for 1 <= H <= 512."""
    assert 1 <= H <= LH_MAX
    W, Hp = ceil_div(H, LU), ceil_div(H, 4) * 4
    mg = max_groups(H, cus)
    chunk = mg * CPG
    launches = []
    for b0 in range(0, batch, chunk):
        nb = min(batch - b0, chunk)
        G = min(nb, mg)
        cpg = ceil_div(nb, G)
        G = ceil_div(nb, cpg)
        launches.append(Launch(b0, nb, G, cpg, tuple(group_of(g * cpg, min(cpg, nb - g * cpg), H) for g in range(G))))
    return ClusterPlan(W, Hp, mg, chunk, tuple(launches), 4 if W <= 4 else (16 if W <= 16 else LH_MAX // LU),
                       4 * (Hp * LC + CPG * Hp + CPG * LC), 4 * (LC * Hp + CPG * LC), 2 * mg * CPG * Hp, 2 * mg * W * CPG * Hp)


def group_sizes(plan):
    return [[g.nclips for g in l.groups] for l in plan.launches]


def reduction_slices(H, KP):
    """[kbeg, kend) of the KP slices of the forward reduction (quads of 4: Hp is a multiple of 4, rows H .. Hp - 1 hold zeros)."""
    klen = ceil_div(ceil_div(H, KP), 4) * 4
    return [(k * klen, max(k * klen, min(H, (k + 1) * klen))) for k in range(KP)]


def ws_bytes(H, cus):
    """vl_lstm_seq_ws_bytes: the cluster form's status block and exchange, or the per-clip backward's transposed kh, whichever is larger."""
    if H < 1:
        return 0
    cluster = 0
    if H <= LH_MAX:
        p = cluster_plan(1, 1, H, cus)
        cluster = STATUS_BYTES + 8 * max(p.xch_fwd, p.xch_bwd)
    return max(cluster, STATUS_BYTES + 16 * H * H)


def tag_span(batch, T, H, cus):
    """vl_lstm_seq_tag_span: launches x (T + 1); 0 for the per-clip form."""
    if batch < 1 or T < 1 or not 1 <= H <= LH_MAX:
        return 0
    return ceil_div(batch, max_groups(H, cus) * CPG) * (T + 1)


PerclipPlan = collections.namedtuple("PerclipPlan", "HP kq threads fwd_blocks fwd_tail bwd_blocks bwd_tail lds_fwd lds_bwd")
# fwd: each of the kq slices of the reduction over H in blocks of 16 rows + a tail; bwd: over the 4 H gate columns likewise


def perclip_plan(H):
    """vl_lstm_perclip_fwd / _bwd: one workgroup of HP kq threads per clip."""
    HP = ceil_div(H, 64) * 64
    kq = 4 if HP * 4 <= 1024 else (2 if HP * 2 <= 1024 else 1)
    klen, glen = ceil_div(H, kq), ceil_div(4 * H, kq)
    return PerclipPlan(HP, kq, HP * kq, klen // 16, klen % 16, glen // 16, glen % 16, 4 * (1 + 4 * kq) * H, 4 * (4 + kq) * H)


def step_workgroups(batch, H):
    return ceil_div(batch * H, 256)


# ---- cases --------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "batch T H")                # batch: a number, or an expression in mg and chunk (resolve)

FULL = [Case("%d*mg" % k if k > 1 else "mg", 3, 498) for k in range(1, 9)]
RAGGED = [Case(b, 3, 498) for b in ("mg+1", "2*mg+1", "4*mg+1", "6*mg+1")]
MULTI = [Case(b, 3, 512) for b in ("chunk+1", "chunk+mg+1", "2*chunk+3")] + [Case("chunk+1", 3, 498)]
GATHER = [Case(1, 3, 37), Case(1, 3, 256), Case("mg+1", 3, 256), Case("chunk", 3, 257), Case(3, 3, 250)]
TIME = [Case("mg+1", T, 498) for T in (1, 2, 21)]
PERCLIP = [Case(9, 4, 513), Case(2, 3, 1021), Case(3, 3, 1024)]
STEP = Case(5, 3, 100)
CLUSTER = FULL + RAGGED + MULTI + GATHER + TIME
ST_CASES = [MULTI[0], FULL[2], Case(3, 4, 600)]                  # replay-safe entry points: 2 launches, 1 launch, the per-clip form

Variant = collections.namedtuple("Variant", "state grads forget_bias dout lens", defaults=("both", "both", 1.0, True, False))
# state   initial state handed to the forward (and c0 to the backward): "none", "h0", "c0", "both"
# grads   outputs asked of the backward: "none", "dh0", "dc0", "both";  dout False: dout = None;  lens: the *_len entry points
PLAIN = Variant()
VARIANTS = [Variant(state=s) for s in ("none", "h0", "c0")] + [Variant(grads=g) for g in ("none", "dh0", "dc0")] + \
           [Variant(forget_bias=0.0), Variant(forget_bias=2.5), Variant(dout=False), Variant(lens=True)]
VARIANT_CASES = [FULL[4], RAGGED[2], MULTI[0], PERCLIP[0]]


def resolve(case, cus):
    """The case with its batch size as a number."""
    if isinstance(case.batch, int):
        return case
    mg = max_groups(case.H, cus)
    return case._replace(batch=int(eval(case.batch, {"__builtins__": {}}, {"mg": mg, "chunk": CPG * mg})))


def case_id(c):
    return "-".join("%g" % v if isinstance(v, float) else str(int(v) if isinstance(v, bool) else v) for v in c)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


Inputs = collections.namedtuple("Inputs", "gx kh h0 c0 dout")


@functools.lru_cache(maxsize=8)
def inputs(batch, T, H):
    """gx [B T][4H] ~ 1.5 N(0,1), kh [H][4H] ~ N(0,1) 0.5 / sqrt(H), h0 and c0 [B][H] ~ 0.5 N(0,1) -- DIFFERENT tensors --, dout ~ N(0,1)."""
    r = np.random.default_rng([batch, T, H])
    f = lambda shape, scale: (r.standard_normal(shape) * scale).astype(np.float32)
    return Inputs(*frozen(f((batch * T, 4 * H), 1.5), f((H, 4 * H), 0.5 / np.sqrt(H)), f((batch, H), 0.5), f((batch, H), 0.5), f((batch * T, H), 1.0)))


def lengths(batch, T):
    """Per-clip lengths in 0..T with a 0, a T, and the values the entry points clamp (vltf.h): a -3 and, on the LAST clip, a T + 5."""
    lens = np.random.default_rng([batch, T, 7]).integers(0, T + 1, batch).astype(np.int32)
    for i, v in zip((0, 1, 2, batch - 1), (0, T, -3, T + 5)):
        if i < batch:
            lens[i] = v
    return frozen(lens)


def clamped(lens, T):
    return np.clip(np.asarray(lens, np.int64), 0, T)


# ---- references ---------------------------------------------------------------------------------------------------------------------
Forward = collections.namedtuple("Forward", "act cseq hseq hprev")          # [B T][4H], [B T][H] x 3, fp64
Backward = collections.namedtuple("Backward", "dz dh0 dc0")                # [B T][4H], [B][H] x 2, fp64


def gates(z, H, forget_bias):
    return O.sigmoid(z[:, :H]), np.tanh(z[:, H:2 * H]), O.sigmoid(z[:, 2 * H:3 * H] + forget_bias), O.sigmoid(z[:, 3 * H:])


def live(lens, batch, T, t):
    return np.ones((batch, 1), bool) if lens is None else (t < clamped(lens, T))[:, None]


def forward_ref(gx, kh, T, h0=None, c0=None, forget_bias=1.0, lens=None, gh=None):
    """gx [B T][4H].  z_t = gx_t + h_{t-1} kh (gh [T][B][4H]: the recurrent term of every step handed in instead -- the step
    kernels' contract); i, j, f, o; c = c sigmoid(f + forget_bias) + sigmoid(i) tanh(j); h = tanh(c) sigmoid(o).  A dead step
    t >= lens[b]: gates and output 0, c and h carried."""
    H = gx.shape[1] // 4
    gx = np.asarray(gx, F64).reshape(-1, T, 4 * H)
    b = gx.shape[0]
    kh = None if kh is None else np.asarray(kh, F64)
    h = np.zeros((b, H)) if h0 is None else np.asarray(h0, F64)
    c = np.zeros((b, H)) if c0 is None else np.asarray(c0, F64)
    out = Forward(np.zeros((b, T, 4 * H)), np.zeros((b, T, H)), np.zeros((b, T, H)), np.zeros((b, T, H)))
    for t in range(T):
        m = live(lens, b, T, t)
        gi, gj, gf, go = gates(gx[:, t] + (h @ kh if gh is None else np.asarray(gh[t], F64)), H, forget_bias)
        out.hprev[:, t] = h
        c = np.where(m, c * gf + gi * gj, c)
        hn = np.tanh(c) * go
        out.act[:, t] = np.where(m, np.concatenate([gi, gj, gf, go], axis=1), 0)
        out.cseq[:, t] = c
        out.hseq[:, t] = np.where(m, hn, 0)
        h = np.where(m, hn, h)
    return Forward(*frozen(*(a.reshape(b * T, -1) for a in out)))


def rounded(a):
    """What the backward kernel is handed of a forward reference: its fp32 rounding."""
    return frozen(np.asarray(a, np.float32))


def backward_ref(dout, kh, T, act, cseq, c0=None, lens=None, dh_next=None):
    """BPTT from the activated gates act and the cell states cseq as given; dout None = zeros.  dz of a dead step is 0.
    dh_next [T][B][H]: d/dh from the step after, handed in instead of dz_{t+1} kh^T (the step kernels' contract; entry T - 1 unused)."""
    H = act.shape[1] // 4
    act, cseq = np.asarray(act, F64).reshape(-1, T, 4 * H), np.asarray(cseq, F64).reshape(-1, T, H)
    b = act.shape[0]
    dout = np.zeros((b, T, H)) if dout is None else np.asarray(dout, F64).reshape(b, T, H)
    kh = None if kh is None else np.asarray(kh, F64)
    dz = np.zeros((b, T, 4 * H))
    dh, dc = np.zeros((b, H)), np.zeros((b, H))
    for t in reversed(range(T)):
        m = live(lens, b, T, t)
        gi, gj, gf, go = (act[:, t, q * H:(q + 1) * H] for q in range(4))
        cp = cseq[:, t - 1] if t > 0 else (np.zeros((b, H)) if c0 is None else np.asarray(c0, F64))
        if dh_next is not None:
            dh = np.asarray(dh_next[t], F64) if t < T - 1 else np.zeros((b, H))
        din = dout[:, t] + dh
        tc = np.tanh(cseq[:, t])
        dcv = dc + din * go * (1 - tc * tc)
        z = np.concatenate([dcv * gj * gi * (1 - gi), dcv * gi * (1 - gj * gj), dcv * cp * gf * (1 - gf), din * tc * go * (1 - go)], axis=1)
        dz[:, t] = np.where(m, z, 0)
        dc = np.where(m, dcv * gf, dc)
        if kh is not None:
            dh = dz[:, t] @ kh.T
    return Backward(*frozen(dz.reshape(b * T, 4 * H), dh, dc))


Ref = collections.namedtuple("Ref", "inp lens fwd act32 cseq32 bwd")


@functools.lru_cache(maxsize=8)
def reference(batch, T, H, variant=PLAIN):
    """Inputs, fp64 forward, its fp32 rounding, and the fp64 backward FROM that rounding, of a resolved case under a variant."""
    inp = inputs(batch, T, H)
    lens = lengths(batch, T) if variant.lens else None
    h0 = inp.h0 if variant.state in ("h0", "both") else None
    c0 = inp.c0 if variant.state in ("c0", "both") else None
    fwd = forward_ref(inp.gx, inp.kh, T, h0, c0, variant.forget_bias, lens)
    act32, cseq32 = rounded(fwd.act), rounded(fwd.cseq)
    bwd = backward_ref(inp.dout if variant.dout else None, inp.kh, T, act32, cseq32, c0, lens)
    return Ref(inp._replace(h0=h0, c0=c0, dout=inp.dout if variant.dout else None), lens, fwd, act32, cseq32, bwd)


StepRef = collections.namedtuple("StepRef", "inp gh fwd act32 cseq32 dh_next bwd")


@functools.lru_cache(maxsize=4)
def step_reference(batch, T, H, forget_bias=1.0, dout=True):
    """The step kernels' inputs and references: gh_t = fp32(h_{t-1} kh) and dh_next_t = fp32(dz_{t+1} kh^T) of the sequence reference
    (zero initial state) are INPUTS of the step kernels (the host computes them with vl_gemm); each step is then one fp64 step from
    them.  The step kernels take c_{t-1} from their own earlier output."""
    inp = inputs(batch, T, H)
    seq = forward_ref(inp.gx, inp.kh, T, forget_bias=forget_bias)
    gh = frozen(np.stack([np.zeros((batch, 4 * H), np.float32)] +
                         [(seq.hseq.reshape(batch, T, H)[:, t - 1] @ inp.kh.astype(F64)).astype(np.float32) for t in range(1, T)]))
    fwd = forward_ref(inp.gx, None, T, forget_bias=forget_bias, gh=gh)
    act32, cseq32 = rounded(fwd.act), rounded(fwd.cseq)
    d = inp.dout if dout else None
    bseq = backward_ref(d, inp.kh, T, act32, cseq32)
    dh_next = frozen(np.stack([(bseq.dz.reshape(batch, T, 4 * H)[:, t + 1] @ inp.kh.astype(F64).T).astype(np.float32) for t in range(T - 1)] +
                              [np.zeros((batch, H), np.float32)]))
    return StepRef(inp._replace(dout=d), gh, fwd, act32, cseq32, dh_next, backward_ref(d, None, T, act32, cseq32, dh_next=dh_next))
