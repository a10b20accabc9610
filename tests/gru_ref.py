"""The reset-after GRU (Keras GRU(reset_after=True), CudnnGRU, torch.nn.GRU; gate blocks z | r | n) in plain Python for the tests: the
fp64 reference of vl_gru_seq_fwd / _bwd taking THE KERNEL'S OWN INPUTS (the backward reads act, hcand and hprev as the forward reference
gives them rounded to fp32, as tests/lstm_plan.py does), a layer and a stack of layers with their gradients, the fusion of the sequence
and an LRCN train step composed from the oracle's tower functions the way tests/blstm_ref.py composes it.  The launch arithmetic, the
case lists, lengths and the rounding come from tests/lstm_plan.py: the GRU launches use vl_lstm_cluster_run's plan.  Nothing here imports
the package: the kernels and engines are checked AGAINST these; tests/test_gru.py proves them equal to torch.nn.GRU in fp64.

Rows are [B T] (clip-major) everywhere; `lens` are per-clip lengths (None = T), clamped to 0..T as the kernels do."""
import collections
import functools
import math

import numpy as np

from tests import lstm_plan as P

F64 = np.float64


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


# ---- cases (the smallest that reach each launcher branch; batches in mg and chunk, lstm_plan.resolve) -----------------------------------
Case = P.Case
CASES = [Case("mg", 3, 498), Case("mg+1", 3, 498), Case("chunk+1", 3, 512), Case(1, 3, 37), Case(3, 3, 250), Case("mg+1", 3, 256)] + \
        [Case("mg+1", T, 498) for T in (1, 2, 21)]
VARIANT_CASE = Case("mg+1", 3, 498)

# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
Inputs = collections.namedtuple("Inputs", "gx rk rb h0 dout")


@functools.lru_cache(maxsize=8)
def inputs(batch, T, H):
    """Seeded like lstm_plan.inputs: gx [B T][3H] ~ 1.5 N(0,1), rk [H][3H] ~ N(0,1) 0.5 / sqrt(H), h0 [B][H] ~ 0.5 N(0,1), dout ~ N(0,1),
    plus rb [3H] ~ 0.5 N(0,1)."""
    r = np.random.default_rng([batch, T, H])
    f = lambda shape, scale: (r.standard_normal(shape) * scale).astype(np.float32)
    gx, rk, h0, dout = f((batch * T, 3 * H), 1.5), f((H, 3 * H), 0.5 / np.sqrt(H)), f((batch, H), 0.5), f((batch * T, H), 1.0)
    return Inputs(*P.frozen(gx, rk, f((3 * H,), 0.5), h0, dout))


def live_mask(lens, batch, T):
    return np.ones((batch, T), bool) if lens is None else np.arange(T)[None, :] < P.clamped(lens, T)[:, None]


def with_nan_in_dead_rows(a, T, lens):
    """A copy of a [B T][w] array with NaN in every dead row (the kernels must not read them)."""
    a = np.array(a, copy=True)
    a[~live_mask(lens, a.shape[0] // T, T).reshape(-1)] = np.nan
    return a


# ---- the recurrence (the kernels' contract) -----------------------------------------------------------------------------------------------
Forward = collections.namedtuple("Forward", "act hcand hseq hprev")         # [B T][3H], [B T][H] x 3, fp64
Backward = collections.namedtuple("Backward", "dgx dgh dh0")               # [B T][3H] x 2, [B][H], fp64


def forward_ref(gx, rk, T, rb=None, h0=None, lens=None):
    """gh_t = h_{t-1} rk + rb; z = s(gx_z + gh_z), r = s(gx_r + gh_r), n = tanh(gx_n + r gh_n); h = z h_{t-1} + (1 - z) n.  A dead step
    t >= lens[b]: act, hcand and the output 0, h carried.  Dead rows of gx are never touched (they may hold NaN)."""
    H = gx.shape[1] // 3
    gx = np.asarray(gx, F64).reshape(-1, T, 3 * H)
    b = gx.shape[0]
    rk = np.asarray(rk, F64)
    rb = np.zeros(3 * H) if rb is None else np.asarray(rb, F64)
    h = np.zeros((b, H)) if h0 is None else np.asarray(h0, F64)
    out = Forward(np.zeros((b, T, 3 * H)), np.zeros((b, T, H)), np.zeros((b, T, H)), np.zeros((b, T, H)))
    for t in range(T):
        m = P.live(lens, b, T, t)
        x = np.where(m, gx[:, t], 0.0)
        gh = h @ rk + rb
        z, r = sigmoid(x[:, :H] + gh[:, :H]), sigmoid(x[:, H:2 * H] + gh[:, H:2 * H])
        n = np.tanh(x[:, 2 * H:] + r * gh[:, 2 * H:])
        hn = z * h + (1 - z) * n
        out.hprev[:, t] = h
        out.act[:, t] = np.where(m, np.concatenate([z, r, n], axis=1), 0)
        out.hcand[:, t] = np.where(m, gh[:, 2 * H:], 0)
        out.hseq[:, t] = np.where(m, hn, 0)
        h = np.where(m, hn, h)
    return Forward(*P.frozen(*(a.reshape(b * T, -1) for a in out)))


def backward_ref(dout, rk, T, act, hcand, hprev, lens=None):
    """BPTT from act, hcand, hprev as given; dout None = zeros.  dgx / dgh of a dead step are 0; dead rows of dout are never touched."""
    H = act.shape[1] // 3
    act, hcand, hprev = (np.asarray(a, F64).reshape(-1, T, a.shape[1]) for a in (act, hcand, hprev))
    b = act.shape[0]
    dout = np.zeros((b, T, H)) if dout is None else np.asarray(dout, F64).reshape(b, T, H)
    rk = np.asarray(rk, F64)
    dgx, dgh = np.zeros((b, T, 3 * H)), np.zeros((b, T, 3 * H))
    dh = np.zeros((b, H))
    for t in reversed(range(T)):
        m = P.live(lens, b, T, t)
        z, r, n = (act[:, t, q * H:(q + 1) * H] for q in range(3))
        din = np.where(m, dout[:, t], 0.0) + dh
        dn = din * (1 - z) * (1 - n * n)
        dz = din * (hprev[:, t] - n) * z * (1 - z)
        dr = dn * hcand[:, t] * r * (1 - r)
        dgx[:, t] = np.where(m, np.concatenate([dz, dr, dn], axis=1), 0)
        dgh[:, t] = np.where(m, np.concatenate([dz, dr, dn * r], axis=1), 0)
        dh = np.where(m, din * z + dgh[:, t] @ rk.T, dh)
    return Backward(*P.frozen(dgx.reshape(b * T, 3 * H), dgh.reshape(b * T, 3 * H), dh))


Ref = collections.namedtuple("Ref", "inp lens fwd act32 hcand32 hprev32 bwd")


@functools.lru_cache(maxsize=8)
def reference(batch, T, H, lens=False, h0=True, rb=True, dout=True):
    """Inputs, fp64 forward, its fp32 rounding, and the fp64 backward FROM that rounding, of a resolved case.  lens: lstm_plan.lengths."""
    inp = inputs(batch, T, H)
    inp = inp._replace(h0=inp.h0 if h0 else None, rb=inp.rb if rb else None, dout=inp.dout if dout else None)
    L = P.lengths(batch, T) if lens else None
    fwd = forward_ref(inp.gx, inp.rk, T, inp.rb, inp.h0, L)
    act32, hcand32, hprev32 = P.rounded(fwd.act), P.rounded(fwd.hcand), P.rounded(fwd.hprev)
    return Ref(inp, L, fwd, act32, hcand32, hprev32, backward_ref(inp.dout, inp.rk, T, act32, hcand32, hprev32, L))


# ---- torch.nn.GRU's layout ---------------------------------------------------------------------------------------------------------------
def to_torch_gates(a, H, axis=-1):
    """z | r | n (Keras, ours) -> r | z | n (torch) along `axis`; its own inverse."""
    z, r, n = np.split(np.asarray(a), 3, axis=axis)
    return np.concatenate([r, z, n], axis=axis)


# ---- a layer and a stack ------------------------------------------------------------------------------------------------------------------
def param_names(layer, scope=""):
    """The variable names of one GRU layer, in flat-buffer order: kernel (d, 3H), recurrent_kernel (H, 3H), bias, recurrent_bias (3H,)."""
    return [scope + "rnn/multi_rnn_cell/cell_%d/gru_cell/%s" % (layer, v) for v in ("kernel", "recurrent_kernel", "bias", "recurrent_bias")]


LayerCache = collections.namedtuple("LayerCache", "x K U T H lens fwd")


def layer_forward(x, K, U, b, rb, T, H, h0=None, lens=None):
    """x [B T][d]; K [d][3H], U [H][3H], b and rb [3H] -> out [B T][H], cache."""
    x = np.asarray(x, F64)
    K, U = np.asarray(K, F64), np.asarray(U, F64)
    fwd = forward_ref(x @ K + np.asarray(b, F64), U, T, rb, h0, lens)
    return fwd.hseq, LayerCache(x, K, U, T, H, lens, fwd)


def layer_backward(dout, cache):
    """dout [B T][H] -> dx, dK, dU, db, drb, dh0.  Dead rows of dout are ignored."""
    x, K, U, T, H, lens, fwd = cache
    bwd = backward_ref(dout, U, T, fwd.act, fwd.hcand, fwd.hprev, lens)
    return bwd.dgx @ K.T, x.T @ bwd.dgx, fwd.hprev.T @ bwd.dgh, bwd.dgx.sum(axis=0), bwd.dgh.sum(axis=0), bwd.dh0


def stack_forward(x, params, T, H, layers, lens=None, scope=""):
    caches = []
    for l in range(layers):
        K, U, b, rb = (params[n] for n in param_names(l, scope))
        x, c = layer_forward(x, K, U, b, rb, T, H, lens=lens)
        caches.append(c)
    return x, caches


def stack_backward(dout, caches, scope=""):
    """-> dx of the stack's input, {name: gradient}."""
    grads = {}
    for l in reversed(range(len(caches))):
        dout, dK, dU, db, drb, _ = layer_backward(dout, caches[l])
        grads.update(zip(param_names(l, scope), (dK, dU, db, drb)))
    return dout, grads


def fuse(out, T, H, fusion, lens=None):
    """The sequence -> what the head reads.  avg: the mean over the live steps; reshape: every row; last / state: the output at L - 1."""
    out = np.asarray(out, F64)
    b = out.shape[0] // T
    if fusion == "reshape":
        return out
    o = out.reshape(b, T, H)
    L = np.full(b, T, np.int64) if lens is None else P.clamped(lens, T)
    if fusion == "avg":
        return (o * live_mask(lens, b, T)[:, :, None]).sum(axis=1) / np.maximum(L, 1)[:, None]
    assert fusion in ("last", "state"), fusion
    return o[np.arange(b), np.maximum(L - 1, 0)]


def fuse_backward(dfused, T, H, fusion, lens=None):
    dfused = np.asarray(dfused, F64)
    if fusion == "reshape":
        return dfused
    b = dfused.shape[0]
    L = np.full(b, T, np.int64) if lens is None else P.clamped(lens, T)
    d = np.zeros((b, T, H))
    if fusion == "avg":
        d[:] = (dfused / np.maximum(L, 1)[:, None])[:, None, :] * live_mask(lens, b, T)[:, :, None]
    else:
        d[np.arange(b), np.maximum(L - 1, 0)] = dfused
    return d.reshape(b * T, H)


# ---- the LRCN model with a GRU classifier (oracle.alexnet_forward, then the stack above) ------------------------------------------------------
def head_name(fusion):
    return "fc_convert" if fusion == "state" else "output_fc"


def init_params(rng, num_classes, final_layer, H, layers, image_shape, fusion="avg"):
    """The oracle's well-scaled AlexNet parameters plus the GRU stack's (kernels glorot-uniform, biases small and NOT zero, so that a bias
    gradient landing on the wrong bias shows) and the (H, C) head."""
    from oracle import lrcn_oracle as O
    p = O.init_params(rng, num_classes, final_layer, H, layers, image_shape, classifier="none", well_scaled=True)
    d = {"fc6": 4096, "fc7": 4096}.get(final_layer, num_classes)
    for l in range(layers):
        for n in param_names(l):
            if n.endswith("kernel"):
                rows = H if n.endswith("recurrent_kernel") else d
                lim = math.sqrt(6.0 / (rows + 3 * H))
                p[n] = rng.uniform(-lim, lim, (rows, 3 * H)).astype(np.float32)
            else:
                p[n] = (0.1 * rng.standard_normal(3 * H)).astype(np.float32)
        d = H
    if H != num_classes:
        p[head_name(fusion) + "_w"] = O.truncated_normal(rng, (H, num_classes), math.sqrt(2.0 / H))
        p[head_name(fusion) + "_b"] = np.full(num_classes, 0.1, np.float32)
    return p


def model_forward(p, frames, fpc, final_layer, H, layers, fusion, lens=None):
    """-> logits, (ccache, caches, fused)."""
    from oracle import lrcn_oracle as O
    feat, ccache = O.alexnet_forward(p, frames, final_layer, F64, True)
    out, caches = stack_forward(feat, p, fpc, H, layers, lens)
    fused = fuse(out, fpc, H, fusion, lens)
    head = head_name(fusion)
    logits = O.xw_plus_b(fused, p[head + "_w"], p[head + "_b"], F64) if head + "_w" in p else fused
    return logits, (ccache, caches, fused)


def model_train_step(p, frames, onehot, fpc, lr, clip_norm, final_layer, H, layers, fusion):
    """One clipped SGD step in fp64 -> (new_params, loss, global_norm, logits, grads)."""
    from oracle import lrcn_oracle as O
    logits, (ccache, caches, fused) = model_forward(p, frames, fpc, final_layer, H, layers, fusion)
    head = head_name(fusion)
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
