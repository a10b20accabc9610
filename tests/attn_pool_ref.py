"""Attention pooling over time (fusion `attn`: Raffel & Ellis 2015 feed-forward attention, the word-attention layer of Yang et al.
2016) in plain fp64 numpy for the tests: the reference of vl_attn_pool_fwd / _bwd taking THE KERNEL'S OWN INPUTS (the backward reads s
and alpha as given, the tests hand it the forward reference's rounded to fp32, as tests/gru_ref.py does), the whole layer with its
projection and parameter gradients, and an LRCN train step composed from the oracle's tower and LSTM functions and the stacks of
tests/gru_ref.py / tests/blstm_ref.py.  Nothing here imports the package: the kernels and engines are checked AGAINST these;
tests/test_attn_pool.py proves them equal to torch autograd in fp64.

Per clip b with L = min(max(lens[b], 1), T) live steps (the temporal fusion's rule, NOT the recurrence's 0..T clamp; None = T):
    s_t = tanh(u_t),  e_t = s_t . c,  alpha = softmax(e_0 .. e_{L-1}),  alpha_t = 0 for t >= L,  y = sum_t alpha_t h_t
Rows are [B T] (clip-major) everywhere."""
import collections
import functools
import math

import numpy as np

from tests import lstm_plan as P

F64 = np.float64

# (batch, T, HO, A): one element; odd widths below a wave; a ragged last wave of A and of HO over several steps per wave; the flagship
# width; both widths above one pass of the workgroup; A just above two waves; T above the wave count with A one past a wave; HO of four
# passes with a narrow scorer
CASES = [(1, 1, 1, 1), (3, 2, 37, 5), (2, 21, 250, 64), (5, 16, 256, 256), (3, 16, 512, 512), (4, 7, 96, 130), (2, 64, 64, 65),
         (3, 5, 1024, 48)]
SCALES = (1, 3)


def case_id(case):
    return "x".join(str(v) for v in case)


def fusion_lens(lens, batch, T):
    """[B] int64: the live steps per clip as the fusion kernels clamp them, 1..T (None: T)."""
    return np.full(batch, T, np.int64) if lens is None else np.clip(np.asarray(lens, np.int64), 1, T)


def live_mask(lens, batch, T):
    return np.arange(T)[None, :] < fusion_lens(lens, batch, T)[:, None]


def with_nan_in_dead_rows(a, T, lens):
    """A copy of a [B T][w] array with NaN in every dead row (the kernels must not read them)."""
    a = np.array(a, copy=True)
    a[~live_mask(lens, a.shape[0] // T, T).reshape(-1)] = np.nan
    return a


Inputs = collections.namedtuple("Inputs", "h u c dy")


@functools.lru_cache(maxsize=None)
def inputs(batch, T, HO, A, k=1):
    """h [B T][HO], dy [B][HO] ~ N(0, 1); u [B T][A] ~ k N(0, 1); c [A] ~ k N(0, 1) / sqrt(A)."""
    r = np.random.default_rng([batch, T, HO, A, k])
    f = lambda shape, scale: (r.standard_normal(shape) * scale).astype(np.float32)
    return Inputs(*P.frozen(f((batch * T, HO), 1.0), f((batch * T, A), float(k)), f((A,), k / math.sqrt(A)), f((batch, HO), 1.0)))


# ---- the two launches (the kernels' contract) ------------------------------------------------------------------------------------------
Forward = collections.namedtuple("Forward", "s alpha y")            # [B T][A] (dead rows 0), [B][T] (dead steps 0), [B][HO]
Backward = collections.namedtuple("Backward", "du dh dcp")          # [B T][A], [B T][HO] (dead rows 0), [B][A]


def forward(h, u, c, lens=None, T=None):
    """h [B T][HO], u [B T][A], c [A] (or [A, 1]).  Dead rows of h and u are never touched (they may hold NaN)."""
    c = np.asarray(c, F64).reshape(-1)
    A = c.shape[0]
    b = np.asarray(u).shape[0] // T
    m = live_mask(lens, b, T)
    u3 = np.where(m[:, :, None], np.asarray(u, F64).reshape(b, T, A), 0.0)
    h3 = np.where(m[:, :, None], np.asarray(h, F64).reshape(b, T, -1), 0.0)
    s = np.where(m[:, :, None], np.tanh(u3), 0.0)
    e = np.where(m, s @ c, -np.inf)
    w = np.exp(e - e.max(axis=1, keepdims=True))
    alpha = w / w.sum(axis=1, keepdims=True)
    y = (alpha[:, :, None] * h3).sum(axis=1)
    return Forward(*P.frozen(s.reshape(b * T, A), alpha, y))


def backward(dy, h, s, alpha, c, lens=None, T=None):
    """From s and alpha AS GIVEN: da_t = dy . h_t, de_t = alpha_t (da_t - sum_r alpha_r da_r), du = de_t c_a (1 - s^2), the direct term
    dh = alpha_t dy, and the per-clip partials dcp[b] = sum_t de_t s_t of c's gradient."""
    c = np.asarray(c, F64).reshape(-1)
    A = c.shape[0]
    dy = np.asarray(dy, F64)
    b = dy.shape[0]
    m = live_mask(lens, b, T)
    h3 = np.where(m[:, :, None], np.asarray(h, F64).reshape(b, T, -1), 0.0)
    s3 = np.where(m[:, :, None], np.asarray(s, F64).reshape(b, T, A), 0.0)
    al = np.where(m, np.asarray(alpha, F64).reshape(b, T), 0.0)
    da = np.einsum("bh,bth->bt", dy, h3)
    de = al * (da - (al * da).sum(axis=1, keepdims=True))
    du = de[:, :, None] * c[None, None, :] * (1.0 - s3 * s3)
    dh = al[:, :, None] * dy[:, None, :]
    dcp = np.einsum("bt,bta->ba", de, s3)
    return Backward(*P.frozen(du.reshape(b * T, A), dh.reshape(b * T, -1), dcp))


Ref = collections.namedtuple("Ref", "inp lens fwd s32 alpha32 bwd")


@functools.lru_cache(maxsize=None)
def reference(case, k=1, lens=False):
    """Inputs, fp64 forward, its fp32 rounding, and the fp64 backward FROM that rounding.  lens: lstm_plan.lengths (a 0, a T, a -3, a T + 5)."""
    batch, T, HO, A = case
    inp = inputs(batch, T, HO, A, k)
    L = P.lengths(batch, T) if lens else None
    fwd = forward(inp.h, inp.u, inp.c, L, T)
    s32, alpha32 = P.rounded(fwd.s), P.rounded(fwd.alpha)
    return Ref(inp, L, fwd, s32, alpha32, backward(inp.dy, inp.h, s32, alpha32, inp.c, L, T))


# ---- the layer: projection, pooling, every gradient ------------------------------------------------------------------------------------
def param_names(scope=""):
    """kernel (HO, A), bias (A,), context (A, 1), in flat-buffer order."""
    return [scope + "attention_pool/" + v for v in ("kernel", "bias", "context")]


PoolCache = collections.namedtuple("PoolCache", "x W c T lens fwd")


def pool_layer_forward(x, W, b, c, T, lens=None):
    """x [B T][HO] -> y [B][HO], cache.  A dead row of x takes no part (it is zeroed before the projection, so it may hold NaN)."""
    x = np.asarray(x, F64)
    x = np.where(live_mask(lens, x.shape[0] // T, T).reshape(-1, 1), x, 0.0)
    W = np.asarray(W, F64)
    fwd = forward(x, x @ W + np.asarray(b, F64), c, lens, T)
    return fwd.y, PoolCache(x, W, np.asarray(c, F64), T, lens, fwd)


def pool_layer_backward(dy, cache):
    """dy [B][HO] -> dx [B T][HO] (dead rows 0), dW, db, dc (the shape of c)."""
    x, W, c, T, lens, fwd = cache
    bwd = backward(dy, x, fwd.s, fwd.alpha, c, lens, T)
    return bwd.dh + bwd.du @ W.T, x.T @ bwd.du, bwd.du.sum(axis=0), bwd.dcp.sum(axis=0).reshape(c.shape)


# ---- the LRCN model with attention pooling (oracle.alexnet_forward, a recurrent stack, the layer above, the head) ----------------------
CELLS = ("lstm", "gru", "blstm")


def out_width(cell, H):
    return 2 * H if cell == "blstm" else H


def init_params(rng, num_classes, final_layer, H, layers, image_shape, cell, A):
    """The cell's own test initialiser (oracle / gru_ref / blstm_ref, head output_fc) plus the attention variables: kernel and context
    glorot-uniform, the bias small and NOT zero so that a gradient on the wrong variable shows."""
    from oracle import lrcn_oracle as O
    from tests import blstm_ref, gru_ref
    if cell == "lstm":
        p = O.init_params(rng, num_classes, final_layer, H, layers, image_shape, well_scaled=True)
    else:
        p = (gru_ref if cell == "gru" else blstm_ref).init_params(rng, num_classes, final_layer, H, layers, image_shape, "avg")
    HO = out_width(cell, H)
    kn, bn, cn = param_names()
    lim = math.sqrt(6.0 / (HO + A))
    p[kn] = rng.uniform(-lim, lim, (HO, A)).astype(np.float32)
    p[bn] = (0.1 * rng.standard_normal(A)).astype(np.float32)
    lim = math.sqrt(6.0 / (A + 1))
    p[cn] = rng.uniform(-lim, lim, (A, 1)).astype(np.float32)
    return p


def _stack_forward(p, feat, fpc, H, layers, cell):
    from oracle import lrcn_oracle as O
    from tests import blstm_ref, gru_ref
    if cell == "gru":
        return gru_ref.stack_forward(feat, p, fpc, H, layers)
    if cell == "blstm":
        return blstm_ref.stack_forward(feat, p, fpc, H, layers)
    x, caches = np.asarray(feat, F64).reshape(-1, fpc, feat.shape[1]), []
    for l in range(layers):
        pre = "rnn/multi_rnn_cell/cell_%d/basic_lstm_cell/" % l
        x, _, lc = O.lstm_layer_forward(x, p[pre + "kernel"], p[pre + "bias"])
        caches.append(lc)
    return x.reshape(-1, H), caches


def _stack_backward(p, dout, caches, fpc, H, cell):
    from oracle import lrcn_oracle as O
    from tests import blstm_ref, gru_ref
    if cell == "gru":
        return gru_ref.stack_backward(dout, caches)
    if cell == "blstm":
        return blstm_ref.stack_backward(dout, caches)
    g, d = {}, dout.reshape(-1, fpc, H)
    for l in reversed(range(len(caches))):
        pre = "rnn/multi_rnn_cell/cell_%d/basic_lstm_cell/" % l
        d, dk, db, _, _ = O.lstm_layer_backward(p[pre + "kernel"], caches[l], d)
        g[pre + "kernel"], g[pre + "bias"] = dk, db
    return d.reshape(-1, d.shape[-1]), g


def model_train_step(p, frames, onehot, fpc, lr, clip_norm, final_layer, H, layers, cell):
    """One clipped SGD step in fp64 -> (new_params, loss, global_norm, logits, grads, alpha)."""
    from oracle import lrcn_oracle as O
    assert cell in CELLS, cell
    feat, ccache = O.alexnet_forward(p, frames, final_layer, F64, True)
    out, caches = _stack_forward(p, feat, fpc, H, layers, cell)
    kn, bn, cn = param_names()
    fused, pc = pool_layer_forward(out, p[kn], p[bn], p[cn], fpc)
    logits = O.xw_plus_b(fused, p["output_fc_w"], p["output_fc_b"], F64) if "output_fc_w" in p else fused
    loss, d = O.softmax_xent_mean(logits, onehot, F64)
    g = {}
    if "output_fc_w" in p:
        g["output_fc_w"], g["output_fc_b"] = fused.T @ d, d.sum(0)
        d = d @ np.asarray(p["output_fc_w"], F64).T
    dout, g[kn], g[bn], g[cn] = pool_layer_backward(d, pc)
    dfeat, lg = _stack_backward(p, dout, caches, fpc, H, cell)
    g.update(lg)
    g.update(O.alexnet_backward(p, ccache, dfeat, final_layer, F64))
    clipped, gn = O.clip_by_global_norm(g, clip_norm)
    return {k: (np.asarray(p[k], F64) - lr * clipped[k]).astype(np.float32) for k in p}, loss, gn, logits, g, pc.fwd.alpha
