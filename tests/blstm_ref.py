"""The bidirectional LSTM layer in plain Python for the tests: the fp64 reference of vl_lstm_seq_bi_fwd / _bwd (tf.nn.bidirectional_dynamic_rnn
with concatenated outputs, the backward cell over tf.reverse_sequence of the live prefix), a whole layer and a stack of layers with their
gradients (stack_bidirectional_dynamic_rnn), the fusion of the 2H-wide sequence, and the launch plan of the bidirectional cluster launch
restated from csrc/lstm_cluster.hip.  Built on tests/lstm_plan.forward_ref / backward_ref: the backward direction IS the unidirectional
reference on the reversed sequence, reversed back.  Nothing here imports the package: the kernels and engines are checked AGAINST these.

Rows are [B T] (clip-major) everywhere; `lens` are per-clip lengths (None = T), clamped to 0..T as the kernels do."""
import collections

import numpy as np

from tests import lstm_plan as P

F64 = np.float64


# ---- reverse_sequence -----------------------------------------------------------------------------------------------------------------
def tau(lens, batch, T):
    """[B][T] int: the time index that processing step s of the backward cell works on: L - 1 - s for s < L, s for the dead steps."""
    L = np.full(batch, T, np.int64) if lens is None else P.clamped(lens, T)
    s = np.arange(T)[None, :]
    return np.where(s < L[:, None], L[:, None] - 1 - s, s)


def reverse_sequence(a, T, lens=None):
    """tf.reverse_sequence over the time axis of a [B T][w] array: the first L_b rows of clip b reversed, the rest where they are.
    An involution: it maps time order to the backward cell's processing order and back."""
    if a is None:
        return None
    a = np.asarray(a)
    b = a.shape[0] // T
    idx = tau(lens, b, T) + (np.arange(b) * T)[:, None]
    return a[idx.reshape(-1)]


# ---- the two recurrences of one layer (the kernels' contract) -------------------------------------------------------------------------------
def forward_ref(gx, kh, T, h0=(None, None), c0=(None, None), forget_bias=1.0, lens=None):
    """(forward, backward) pairs in, a pair of lstm_plan.Forward out, every tensor of the backward cell indexed by TIME."""
    fw = P.forward_ref(gx[0], kh[0], T, h0[0], c0[0], forget_bias, lens)
    bw = P.forward_ref(reverse_sequence(gx[1], T, lens), kh[1], T, h0[1], c0[1], forget_bias, lens)
    return fw, P.Forward(*(P.frozen(reverse_sequence(a, T, lens)) for a in bw))


def backward_ref(dout, kh, T, act, cseq, c0=(None, None), lens=None):
    """BPTT of both cells from act / cseq as given (time-indexed); dout pair, either half may be None -> a pair of lstm_plan.Backward."""
    fw = P.backward_ref(dout[0], kh[0], T, act[0], cseq[0], c0[0], lens)
    rs = lambda a: reverse_sequence(a, T, lens)
    bw = P.backward_ref(rs(dout[1]), kh[1], T, rs(act[1]), rs(cseq[1]), c0[1], lens)
    return fw, P.Backward(P.frozen(rs(bw.dz)), bw.dh0, bw.dc0)


# ---- a layer and a stack ------------------------------------------------------------------------------------------------------------------
LayerCache = collections.namedtuple("LayerCache", "x K T H lens c0 fwd")


def layer_forward(x, K, b, T, H, h0=(None, None), c0=(None, None), lens=None, forget_bias=1.0):
    """x [B T][d]; K = (K_fw, K_bw), each [d + H][4H]; b = (b_fw, b_bw) -> out [B T][2H] (forward half first), cache."""
    x = np.asarray(x, F64)
    d = x.shape[1]
    K = tuple(np.asarray(k, F64) for k in K)
    gx = tuple(x @ K[i][:d] + np.asarray(b[i], F64) for i in range(2))
    fwd = forward_ref(gx, tuple(k[d:] for k in K), T, h0, c0, forget_bias, lens)
    return np.concatenate([fwd[0].hseq, fwd[1].hseq], axis=1), LayerCache(x, K, T, H, lens, c0, fwd)


def layer_backward(dout, cache):
    """dout [B T][2H] -> dx, (dK_fw, dK_bw), (db_fw, db_bw), (dh0_fw, dh0_bw), (dc0_fw, dc0_bw).  Dead rows of dout are ignored."""
    x, K, T, H, lens, c0, fwd = cache
    d = x.shape[1]
    dout = np.asarray(dout, F64)
    bwd = backward_ref((dout[:, :H], dout[:, H:]), tuple(k[d:] for k in K), T, tuple(f.act for f in fwd), tuple(f.cseq for f in fwd), c0, lens)
    dx = sum(bwd[i].dz @ K[i][:d].T for i in range(2))
    dK = tuple(np.concatenate([x.T @ bwd[i].dz, fwd[i].hprev.T @ bwd[i].dz], axis=0) for i in range(2))
    return dx, dK, tuple(bwd[i].dz.sum(axis=0) for i in range(2)), tuple(bwd[i].dh0 for i in range(2)), tuple(bwd[i].dc0 for i in range(2))


def param_names(layer, scope=""):
    """TF's variable names of one bidirectional layer, in the order the engines keep them: fw kernel, fw bias, bw kernel, bw bias."""
    return [scope + "bidirectional_rnn/%s/multi_rnn_cell/cell_%d/basic_lstm_cell/%s" % (d, layer, v) for d in ("fw", "bw") for v in ("kernel", "bias")]


def stack_forward(x, params, T, H, layers, lens=None, scope=""):
    """stack_bidirectional_dynamic_rnn: layer l + 1 reads the whole 2H-wide output of layer l -> out [B T][2H], caches."""
    caches = []
    for l in range(layers):
        kf, bf, kb, bb = (params[n] for n in param_names(l, scope))
        x, c = layer_forward(x, (kf, kb), (bf, bb), T, H, lens=lens)
        caches.append(c)
    return x, caches


def stack_backward(dout, caches, scope=""):
    """-> dx of the stack's input, {name: gradient}."""
    grads = {}
    for l in reversed(range(len(caches))):
        dout, dK, db, _, _ = layer_backward(dout, caches[l])
        grads.update(zip(param_names(l, scope), (dK[0], db[0], dK[1], db[1])))
    return dout, grads


def live_mask(lens, batch, T):
    return np.ones((batch, T), bool) if lens is None else np.arange(T)[None, :] < P.clamped(lens, T)[:, None]


def fuse(out, T, H, fusion, lens=None):
    """The 2H-wide sequence -> what the head reads.  avg: the mean over the live steps; reshape: every row; last / state: each direction's
    FINAL output, the forward half at time L - 1 and the backward half at time 0 (Keras Bidirectional(return_sequences=False))."""
    out = np.asarray(out, F64)
    b = out.shape[0] // T
    if fusion == "reshape":
        return out
    o = out.reshape(b, T, 2 * H)
    L = np.full(b, T, np.int64) if lens is None else P.clamped(lens, T)
    if fusion == "avg":
        return (o * live_mask(lens, b, T)[:, :, None]).sum(axis=1) / np.maximum(L, 1)[:, None]
    assert fusion in ("last", "state"), fusion
    return np.concatenate([o[np.arange(b), np.maximum(L - 1, 0), :H], o[:, 0, H:]], axis=1)


def fuse_backward(dfused, T, H, fusion, lens=None):
    """d(fused) -> dout [B T][2H]."""
    dfused = np.asarray(dfused, F64)
    if fusion == "reshape":
        return dfused
    b = dfused.shape[0]
    L = np.full(b, T, np.int64) if lens is None else P.clamped(lens, T)
    d = np.zeros((b, T, 2 * H))
    if fusion == "avg":
        d[:] = (dfused / np.maximum(L, 1)[:, None])[:, None, :] * live_mask(lens, b, T)[:, :, None]
    else:
        d[np.arange(b), np.maximum(L - 1, 0), :H] = dfused[:, :H]
        d[:, 0, H:] = dfused[:, H:]
    return d.reshape(b * T, 2 * H)


# ---- the LRCN model with a bidirectional classifier (oracle.alexnet_forward, then the stack above) --------------------------------------------
def head_name(fusion):
    return "fc_convert" if fusion == "state" else "output_fc"


def init_params(rng, num_classes, final_layer, H, layers, image_shape, fusion="avg"):
    """The oracle's well-scaled AlexNet parameters plus the bidirectional stack's (kernels glorot-uniform, biases small and NOT zero, so
    that a bias gradient landing on the wrong direction shows) and the (2H, C) head."""
    import math
    from oracle import lrcn_oracle as O
    p = O.init_params(rng, num_classes, final_layer, H, layers, image_shape, classifier="none", well_scaled=True)
    d = {"fc6": 4096, "fc7": 4096}.get(final_layer, num_classes)
    for l in range(layers):
        for n in param_names(l):
            if n.endswith("kernel"):
                lim = math.sqrt(6.0 / (d + 5 * H))
                p[n] = rng.uniform(-lim, lim, (d + H, 4 * H)).astype(np.float32)
            else:
                p[n] = (0.1 * rng.standard_normal(4 * H)).astype(np.float32)
        d = 2 * H
    if 2 * H != num_classes:
        p[head_name(fusion) + "_w"] = O.truncated_normal(rng, (2 * H, num_classes), math.sqrt(2.0 / (2 * H)))
        p[head_name(fusion) + "_b"] = np.full(num_classes, 0.1, np.float32)
    return p


def model_train_step(p, frames, onehot, fpc, lr, clip_norm, final_layer, H, layers, fusion):
    """One clipped SGD step in fp64 -> (new_params, loss, global_norm, logits, grads)."""
    from oracle import lrcn_oracle as O
    feat, ccache = O.alexnet_forward(p, frames, final_layer, F64, True)
    out, caches = stack_forward(feat, p, fpc, H, layers)
    fused = fuse(out, fpc, H, fusion)
    head = head_name(fusion)
    logits = O.xw_plus_b(fused, p[head + "_w"], p[head + "_b"], F64) if head + "_w" in p else fused
    loss, d = O.softmax_xent_mean(logits, onehot, F64)
    g = {}
    if head + "_w" in p:
        g[head + "_w"], g[head + "_b"] = fused.T @ d, d.sum(0)
        d = d @ np.asarray(p[head + "_w"], F64).T
    dfeat, lg = stack_backward(fuse_backward(d, fpc, H, fusion), caches)
    g.update(lg)
    g.update(O.alexnet_backward(p, ccache, dfeat, final_layer, F64))
    clipped, gn = O.clip_by_global_norm(g, clip_norm)
    return {k: (np.asarray(p[k], F64) - lr * clipped[k]).astype(np.float32) for k in p}, loss, gn, logits, g


# ---- the launch plan ------------------------------------------------------------------------------------------------------------------------
BiLaunch = collections.namedtuple("BiLaunch", "b0 nb G cpg grid groups")     # groups: lstm_plan.Group, the SAME for both directions
BiPlan = collections.namedtuple("BiPlan", "W Hp mg chunk launches")


def mg_bi(H, cus):
    """Groups per direction that one launch holds: both directions' workgroups resident at once, one per CU (0: the launch is refused)."""
    return cus // (2 * P.ceil_div(H, P.LU))


def bi_plan(batch, T, H, cus):
    """What vl_lstm_cluster_run_bi launches for 1 <= H <= 512 and mg_bi >= 1."""
    assert 1 <= H <= P.LH_MAX and mg_bi(H, cus) >= 1
    W, Hp, mg = P.ceil_div(H, P.LU), P.ceil_div(H, 4) * 4, mg_bi(H, cus)
    chunk, launches = mg * P.CPG, []
    for b0 in range(0, batch, chunk):
        nb = min(batch - b0, chunk)
        G = min(nb, mg)
        cpg = P.ceil_div(nb, G)
        G = P.ceil_div(nb, cpg)
        launches.append(BiLaunch(b0, nb, G, cpg, 2 * G * W, tuple(P.group_of(g * cpg, min(cpg, nb - g * cpg), H) for g in range(G))))
    return BiPlan(W, Hp, mg, chunk, tuple(launches))


def exchange_slices(plan, launch, bwd):
    """{(direction, group): [(first, past-the-end), ...]} in exchange words (8 bytes, after the status block): the words of virtual group
    direction * G + group in both parity blocks.  Forward: [parity][2G][8][Hp]; backward: [parity][2G][W][8][Hp]."""
    per = P.CPG * plan.Hp * (plan.W if bwd else 1)
    VG = 2 * launch.G
    return {(d, g): [((par * VG + d * launch.G + g) * per, (par * VG + d * launch.G + g + 1) * per) for par in range(2)]
            for d in range(2) for g in range(launch.G)}


def tag_span(batch, T, H, cus):
    """vl_lstm_seq_bi_tag_span: launches x (T + 1); 0 where the entry points refuse."""
    if batch < 1 or T < 1 or not 1 <= H <= P.LH_MAX or mg_bi(H, cus) < 1:
        return 0
    return P.ceil_div(batch, mg_bi(H, cus) * P.CPG) * (T + 1)


def resolve(case, cus):
    """An lstm_plan.Case whose batch is written in mg and chunk, with mg = mg_bi and chunk = 8 mg_bi."""
    if isinstance(case.batch, int):
        return case
    mg = mg_bi(case.H, cus)
    return case._replace(batch=int(eval(case.batch, {"__builtins__": {}}, {"mg": mg, "chunk": P.CPG * mg})))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def inputs(batch, T, H):
    """A pair of lstm_plan.Inputs: the forward direction's are lstm_plan.inputs(batch, T, H), the backward direction's come from a second
    seed (different weights, states, projections and gradients)."""
    r = np.random.default_rng([batch, T, H, 2])
    f = lambda shape, scale: (r.standard_normal(shape) * scale).astype(np.float32)
    bw = P.Inputs(*P.frozen(f((batch * T, 4 * H), 1.5), f((H, 4 * H), 0.5 / np.sqrt(H)), f((batch, H), 0.5), f((batch, H), 0.5), f((batch * T, H), 1.0)))
    return P.inputs(batch, T, H), bw


def with_nan_in_dead_rows(a, T, lens):
    """A copy of a [B T][w] array with NaN in every dead row (the kernels must not read them)."""
    a = np.array(a, copy=True)
    a[~live_mask(lens, a.shape[0] // T, T).reshape(-1)] = np.nan
    return a
