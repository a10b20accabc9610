"""Multi-head self-attention over the frames of a clip (rnn_cell `mhsa`: Keras MultiHeadAttention(num_heads, key_dim = H / heads,
output_shape = H) called with query = value = x, plus a learned relative-position bias on the scores) in plain fp64 numpy for the
tests: the reference of vl_mhsa_fwd / _bwd taking THE KERNEL'S OWN INPUTS (the backward reads P as given, the tests hand it the forward
reference's rounded to fp32, as tests/attn_pool_ref.py does), the whole layer with its two projections and parameter gradients, and an
LRCN train step composed from the oracle's tower and head and the fusions of tests/gru_ref.py / tests/attn_pool_ref.py.  Nothing here
imports the package: the kernels and engines are checked AGAINST these; tests/test_self_attention.py proves them equal to torch autograd
in fp64.

Per clip b with L = min(max(lens[b], 0), T) live steps (the recurrence's clamp: the layer stands where a recurrence stands; None = T)
and per head h of width dh = H / heads (columns h dh .. (h + 1) dh of each of qkv's blocks Q | K | V):
    S[q][k] = Q_q . K_k / sqrt(dh) + pos[h][k - q + T - 1]     P[q] = softmax over k < L of S[q]     ctx_q = sum_k P[q][k] V_k
Dead query rows and dead key columns of P, and dead rows of ctx and dqkv, are zeros.  Rows are [B T] (clip-major) everywhere."""
import collections
import functools
import math

import numpy as np

from tests import lstm_plan as LP

F64 = np.float64

# (batch, T, H, heads): degenerate, one step; dh = 8; dh = 50 with an odd T; the workload's shape; eight heads; dh = 96 in one head;
# T = 64; T and dh both at their limits; dh = 65, not a multiple of 4
CASES = [(1, 1, 8, 1), (3, 2, 24, 3), (2, 21, 250, 5), (5, 16, 256, 4), (3, 16, 512, 8), (4, 7, 96, 1), (2, 64, 64, 1), (2, 64, 1024, 8),
         (3, 5, 130, 2)]
SCALES = (1, 3)


def case_id(case):
    return "x".join(str(v) for v in case)


def live_lens(lens, batch, T):
    """[B] int64: the live steps per clip as the launches clamp them, 0..T (None: T)."""
    return np.full(batch, T, np.int64) if lens is None else LP.clamped(lens, T)


def live_mask(lens, batch, T):
    return np.arange(T)[None, :] < live_lens(lens, batch, T)[:, None]


def with_nan_in_dead_rows(a, T, lens):
    """A copy of a [B T][w] array with NaN in every dead row (the kernels must not read them)."""
    a = np.array(a, copy=True)
    a[~live_mask(lens, a.shape[0] // T, T).reshape(-1)] = np.nan
    return a


Inputs = collections.namedtuple("Inputs", "qkv pos dctx")


@functools.lru_cache(maxsize=None)
def inputs(batch, T, H, heads, k=1):
    """qkv [B T][3H] ~ k N(0, 1) (so a score Q . K / sqrt(dh) ~ k^2 N(0, 1)); pos [heads][2T - 1] ~ k N(0, 1); dctx [B T][H] ~ N(0, 1)."""
    r = np.random.default_rng([batch, T, H, heads, k])
    f = lambda shape, scale: (r.standard_normal(shape) * scale).astype(np.float32)
    return Inputs(*LP.frozen(f((batch * T, 3 * H), float(k)), f((heads, 2 * T - 1), float(k)), f((batch * T, H), 1.0)))


def rel_index(T):
    """[T][T] of k - q + T - 1: the column of pos a (query q, key k) pair reads."""
    return np.arange(T)[None, :] - np.arange(T)[:, None] + T - 1


def split_heads(a, b, T, heads):
    """[B T][H] -> [B][heads][T][dh]."""
    return a.reshape(b, T, heads, -1).transpose(0, 2, 1, 3)


def merge_heads(a):
    """[B][heads][T][dh] -> [B T][H]."""
    b, heads, T, dh = a.shape
    return a.transpose(0, 2, 1, 3).reshape(b * T, heads * dh)


# ---- the two launches (the kernels' contract) ------------------------------------------------------------------------------------------
Forward = collections.namedtuple("Forward", "P ctx")               # [B][heads][T][T], [B T][H]
Backward = collections.namedtuple("Backward", "dqkv dposp")        # [B T][3H] (dead rows 0), [B][heads][2T - 1] (None without pos)


def _qkv(qkv, m, b, T, H, heads):
    x = np.where(m.reshape(-1, 1), np.asarray(qkv, F64), 0.0)       # a dead row takes no part (it may hold NaN)
    return (split_heads(x[:, i * H:(i + 1) * H], b, T, heads) for i in range(3))


def forward(qkv, pos, heads, lens=None, T=None):
    """qkv [B T][3H], pos [heads][2T - 1] or None."""
    H = np.asarray(qkv).shape[1] // 3
    b = np.asarray(qkv).shape[0] // T
    m = live_mask(lens, b, T)
    Q, K, V = _qkv(qkv, m, b, T, H, heads)
    S = Q @ K.transpose(0, 1, 3, 2) / math.sqrt(H // heads)
    if pos is not None:
        S = S + np.asarray(pos, F64)[:, rel_index(T)][None]
    pair = m[:, None, :, None] & m[:, None, None, :]
    S = np.where(pair, S, -np.inf)
    mx = S.max(axis=3, keepdims=True)
    w = np.exp(S - np.where(np.isfinite(mx), mx, 0.0))              # (a dead pair: exp(-inf) = 0)
    z = w.sum(axis=3, keepdims=True)
    P = np.where(pair, w / np.where(z > 0, z, 1.0), 0.0)
    return Forward(*LP.frozen(P, merge_heads(P @ V)))


def backward(dctx, qkv, P, heads, lens=None, T=None, positions=True):
    """From P AS GIVEN: dV = P^T dctx, dP = dctx V^T, dS = P o (dP - rowsum(dP o P)), dQ = dS K / sqrt(dh), dK = dS^T Q / sqrt(dh), and
    the per-clip partials dposp[b][h][r] = sum over q, k with k - q + T - 1 = r of dS."""
    H = np.asarray(qkv).shape[1] // 3
    b = np.asarray(qkv).shape[0] // T
    m = live_mask(lens, b, T)
    Q, K, V = _qkv(qkv, m, b, T, H, heads)
    dO = split_heads(np.where(m.reshape(-1, 1), np.asarray(dctx, F64), 0.0), b, T, heads)
    pair = m[:, None, :, None] & m[:, None, None, :]
    P = np.where(pair, np.asarray(P, F64).reshape(b, heads, T, T), 0.0)
    dV = P.transpose(0, 1, 3, 2) @ dO
    dP = dO @ V.transpose(0, 1, 3, 2)
    dS = P * (dP - (dP * P).sum(axis=3, keepdims=True))
    scale = 1.0 / math.sqrt(H // heads)
    dQ, dK = dS @ K * scale, dS.transpose(0, 1, 3, 2) @ Q * scale
    dqkv = np.concatenate([merge_heads(dQ), merge_heads(dK), merge_heads(dV)], axis=1)
    dposp = None
    if positions:
        dposp = np.zeros((b, heads, 2 * T - 1))
        rel = rel_index(T)
        for r in range(2 * T - 1):
            dposp[:, :, r] = (dS * (rel == r)).sum(axis=(2, 3))
        LP.frozen(dposp)
    return Backward(LP.frozen(dqkv), dposp)


Ref = collections.namedtuple("Ref", "inp lens fwd P32 bwd")


@functools.lru_cache(maxsize=None)
def reference(case, k=1, lens=False, positions=True):
    """Inputs, fp64 forward, its fp32 rounding, and the fp64 backward FROM that rounding.  lens: lstm_plan.lengths (a 0, a T, a -3, a
    T + 5).  positions False: pos = None."""
    batch, T, H, heads = case
    inp = inputs(batch, T, H, heads, k)
    L = LP.lengths(batch, T) if lens else None
    fwd = forward(inp.qkv, inp.pos if positions else None, heads, L, T)
    P32 = LP.rounded(fwd.P)
    return Ref(inp, L, fwd, P32, backward(inp.dctx, inp.qkv, P32, heads, L, T, positions))


# ---- the layer: the two projections, the attention, every gradient ---------------------------------------------------------------------
VARS = ("qkv_kernel", "qkv_bias", "out_kernel", "out_bias", "position_bias")


def param_names(layer, scope="", positions=True):
    """qkv_kernel (d, 3H), qkv_bias (3H,), out_kernel (H, H), out_bias (H,), position_bias (heads, 2T - 1), in flat-buffer order."""
    return [scope + "self_attention/layer_%d/%s" % (layer, v) for v in (VARS if positions else VARS[:4])]


LayerCache = collections.namedtuple("LayerCache", "x Wqkv Wo qkv heads T lens fwd positions")


def layer_forward(x, Wqkv, bqkv, Wo, bo, pos, heads, T, lens=None):
    """x [B T][d] -> y [B T][H] (a dead row is zeros HERE: nothing downstream may read it), cache.  A dead row of x takes no part."""
    x = np.asarray(x, F64)
    m = live_mask(lens, x.shape[0] // T, T).reshape(-1, 1)
    x = np.where(m, x, 0.0)
    Wqkv, Wo = np.asarray(Wqkv, F64), np.asarray(Wo, F64)
    qkv = x @ Wqkv + np.asarray(bqkv, F64)
    fwd = forward(qkv, pos, heads, lens, T)
    y = np.where(m, fwd.ctx @ Wo + np.asarray(bo, F64), 0.0)
    return y, LayerCache(x, Wqkv, Wo, qkv, heads, T, lens, fwd, pos is not None)


def layer_backward(dy, cache):
    """dy [B T][H] (dead rows ignored) -> dx, [dWqkv, dbqkv, dWo, dbo (, dpos)]."""
    x, Wqkv, Wo, qkv, heads, T, lens, fwd, positions = cache
    dy = np.where(live_mask(lens, x.shape[0] // T, T).reshape(-1, 1), np.asarray(dy, F64), 0.0)
    bwd = backward(dy @ Wo.T, qkv, fwd.P, heads, lens, T, positions)
    grads = [x.T @ bwd.dqkv, bwd.dqkv.sum(axis=0), fwd.ctx.T @ dy, dy.sum(axis=0)]
    if positions:
        grads.append(bwd.dposp.sum(axis=0))
    return bwd.dqkv @ Wqkv.T, grads


def stack_forward(x, params, T, layers, heads, lens=None, scope="", positions=True):
    caches = []
    for l in range(layers):
        names = param_names(l, scope, positions)
        x, c = layer_forward(x, *(params[n] for n in names[:4]), params[names[4]] if positions else None, heads, T, lens)
        caches.append(c)
    return x, caches


def stack_backward(dout, caches, scope=""):
    """-> dx of the stack's input, {name: gradient}."""
    grads = {}
    for l in reversed(range(len(caches))):
        dout, g = layer_backward(dout, caches[l])
        grads.update(zip(param_names(l, scope, caches[l].positions), g))
    return dout, grads


# ---- the LRCN model with self-attention layers (oracle.alexnet_forward, the stack above, a fusion, the head) ---------------------------
def init_params(rng, num_classes, final_layer, H, layers, image_shape, heads, T, positions=True, attn_dim=None):
    """The oracle's well-scaled AlexNet parameters plus the stack's (kernels glorot-uniform; the biases and the position bias small and
    NOT zero, so that a gradient landing on the wrong variable shows), the (H, C) head and, with attn_dim, attention_pool's variables."""
    from oracle import lrcn_oracle as O
    p = O.init_params(rng, num_classes, final_layer, H, layers, image_shape, classifier="none", well_scaled=True)
    d = {"fc6": 4096, "fc7": 4096}.get(final_layer, num_classes)
    for l in range(layers):
        shapes = ((d, 3 * H), (3 * H,), (H, H), (H,), (heads, 2 * T - 1))
        for n, shp in zip(param_names(l, positions=positions), shapes):
            if n.endswith("kernel"):
                lim = math.sqrt(6.0 / (shp[0] + shp[1]))
                p[n] = rng.uniform(-lim, lim, shp).astype(np.float32)
            else:
                p[n] = (0.1 * rng.standard_normal(shp)).astype(np.float32)
        d = H
    if H != num_classes:
        p["output_fc_w"] = O.truncated_normal(rng, (H, num_classes), math.sqrt(2.0 / H))
        p["output_fc_b"] = np.full(num_classes, 0.1, np.float32)
    if attn_dim:
        from tests import attn_pool_ref
        kn, bn, cn = attn_pool_ref.param_names()
        lim = math.sqrt(6.0 / (H + attn_dim))
        p[kn] = rng.uniform(-lim, lim, (H, attn_dim)).astype(np.float32)
        p[bn] = (0.1 * rng.standard_normal(attn_dim)).astype(np.float32)
        lim = math.sqrt(6.0 / (attn_dim + 1))
        p[cn] = rng.uniform(-lim, lim, (attn_dim, 1)).astype(np.float32)
    return p


def varied_frames(rng, clips, fpc, shape):
    """uint8 frames [clips fpc] + shape that DIFFER along a clip: coarse random blocks (14 x 14 pixels) at a contrast of 0.15, 0.6 or 1
    by time step.  Frames of independent pixel noise all give nearly the same features (they vary by 8 % along a clip); a self-attention
    layer, which has no state, then gives nearly the same output at every step, and whatever depends on the differences between steps --
    the gradients of attention_pool behind it, of position_bias -- is a difference of nearly equal fp32 numbers.  With these frames the
    features vary by 38 % and those gradients are three orders of magnitude above their fp32 noise (measured with the fp64 reference)."""
    n = clips * fpc
    h, w, c = shape
    blocks = np.kron(rng.integers(0, 256, (n, -(-h // 14), -(-w // 14), c)), np.ones((1, 14, 14, 1), np.int64))[:, :h, :w]
    amp = np.array([0.15, 0.6, 1.0])[np.arange(n) % fpc % 3][:, None, None, None]
    return np.clip(np.rint(104 + amp * (blocks - 128)), 0, 255).astype(np.uint8)


def tame_first_layer(p, frames, final_layer, positions=True):
    """Divides layer 0's qkv_kernel by the rms of the tower's features of `frames` (in place; -> the rms).  Behind mean-subtracted
    pixels the features are of the order of 50, so q . k / sqrt(dh) would be in the thousands, every softmax one-hot and the gradients
    of Q, K and position_bias exactly zero in fp32: a test on such a model would hold for a kernel without its softmax backward.  With
    qkv of order 1 the scores are of order 1, as behind a trained tower."""
    from oracle import lrcn_oracle as O
    feat, _ = O.alexnet_forward(p, frames, final_layer, F64, True)
    rms = float(np.sqrt(np.mean(np.square(feat))))
    name = param_names(0, positions=positions)[0]
    p[name] = (p[name] / rms).astype(np.float32)
    return rms


def model_train_step(p, frames, onehot, fpc, lr, clip_norm, final_layer, H, layers, heads, fusion, positions=True):
    """One clipped SGD step in fp64 -> (new_params, loss, global_norm, logits, grads, P of the last layer)."""
    from oracle import lrcn_oracle as O
    from tests import attn_pool_ref, gru_ref
    feat, ccache = O.alexnet_forward(p, frames, final_layer, F64, True)
    out, caches = stack_forward(feat, p, fpc, layers, heads, positions=positions)
    g = {}
    if fusion == "attn":
        kn, bn, cn = attn_pool_ref.param_names()
        fused, pc = attn_pool_ref.pool_layer_forward(out, p[kn], p[bn], p[cn], fpc)
    else:
        fused = gru_ref.fuse(out, fpc, H, fusion)
    logits = O.xw_plus_b(fused, p["output_fc_w"], p["output_fc_b"], F64) if "output_fc_w" in p else fused
    loss, d = O.softmax_xent_mean(logits, onehot, F64)
    if "output_fc_w" in p:
        g["output_fc_w"], g["output_fc_b"] = fused.T @ d, d.sum(0)
        d = d @ np.asarray(p["output_fc_w"], F64).T
    if fusion == "attn":
        dout, g[kn], g[bn], g[cn] = attn_pool_ref.pool_layer_backward(d, pc)
    else:
        dout = gru_ref.fuse_backward(d, fpc, H, fusion)
    dfeat, lg = stack_backward(dout, caches)
    g.update(lg)
    g.update(O.alexnet_backward(p, ccache, dfeat, final_layer, F64))
    clipped, gn = O.clip_by_global_norm(g, clip_norm)
    return {k: (np.asarray(p[k], F64) - lr * clipped[k]).astype(np.float32) for k in p}, loss, gn, logits, g, caches[-1].fwd.P
