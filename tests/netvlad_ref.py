"""NetVLAD pooling over time (fusion `vlad`: Arandjelovic et al. 2016, ActionVLAD of Girdhar et al. 2017, the temporal form of Miech
et al. 2017) in plain fp64 numpy for the tests: the reference of vl_netvlad_fwd / _bwd taking THE KERNEL'S OWN INPUTS (the backward
reads a, r and y as given, the tests hand it the forward reference's rounded to fp32, as tests/attn_pool_ref.py does), the whole layer
with its projection and parameter gradients, and an LRCN train step composed from the oracle's tower and LSTM functions and the stacks
of tests/gru_ref.py / tests/blstm_ref.py / tests/encoder_block_ref.py.  Nothing here imports the package: the kernels and engines are
checked AGAINST these; tests/test_netvlad.py proves them equal to torch autograd in fp64.

Per clip b with L = min(max(lens[b], 1), T) live steps (the temporal fusion's rule; None = T), rows h_t in R^HO, centres c_k, scores s_t:
    a_t = softmax_k(s_t) for t < L, 0 for t >= L;   m_k = sum_t a_tk;   V_k = sum_t a_tk h_t - m_k c_k
    r_k = rsqrt(max(|V_k|^2, 1e-12));   y[k HO + j] = V_k[j] r_k / sqrt(K)
The second (whole-descriptor) normalisation of the papers is the constant 1 / sqrt(K): behind the intra-normalisation every |U_k| is 1.
Rows are [B T] (clip-major) everywhere."""
import collections
import functools
import math

import numpy as np

from tests import lstm_plan as P

F64 = np.float64
EPS = 1e-12                  # tf.nn.l2_normalize's epsilon, on |V_k|^2
RMAX = 1e6                   # rsqrt(EPS): the scale of a cluster below the epsilon
BAND = 16.0                  # no drawn cluster may have |V_k|^2 inside [EPS / BAND, EPS BAND]: fp32 and fp64 could take different branches

# (batch, T, HO, K)
CASES = [(1, 1, 2, 2), (3, 2, 37, 3), (2, 21, 250, 5), (5, 16, 256, 8), (2, 16, 256, 64), (3, 5, 1024, 16), (2, 64, 64, 33),
         (4, 7, 96, 64)]
SCALES = (1, 3)
# extra seed words for the draws in which a cluster's |V_k|^2 fell inside the band around the epsilon (forward asserts that none does):
# at K = 64 a one-step clip with a score spread of ~20 reaches it
SALT = {(4, 7, 96, 64, 3): [2]}


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


Inputs = collections.namedtuple("Inputs", "h s c dy")


@functools.lru_cache(maxsize=None)
def inputs(batch, T, HO, K, k=1):
    """h [B T][HO], dy [B][K HO] ~ N(0, 1); s [B T][K] ~ k N(0, 1); c [K][HO] ~ 0.5 N(0, 1)."""
    r = np.random.default_rng([batch, T, HO, K, k] + SALT.get((batch, T, HO, K, k), []))
    f = lambda shape, scale: (r.standard_normal(shape) * scale).astype(np.float32)
    return Inputs(*P.frozen(f((batch * T, HO), 1.0), f((batch * T, K), float(k)), f((K, HO), 0.5), f((batch, K * HO), 1.0)))


# ---- the two launches (the kernels' contract) ------------------------------------------------------------------------------------------
Forward = collections.namedtuple("Forward", "a r y")                # [B T][K] (dead rows 0), [B][K], [B][K HO]
Backward = collections.namedtuple("Backward", "ds dh dcp")          # [B T][K], [B T][HO] (dead rows 0), [B][K HO]


def _live3(x, m, b, T):
    return np.where(m[:, :, None], np.asarray(x, F64).reshape(b, T, -1), 0.0)


def forward(h, s, c, lens=None, T=None, check_band=True):
    """h [B T][HO], s [B T][K], c [K][HO].  Dead rows of h and s are never touched (they may hold NaN)."""
    c = np.asarray(c, F64)
    K, HO = c.shape
    b = np.asarray(s).shape[0] // T
    m = live_mask(lens, b, T)
    s3, h3 = _live3(s, m, b, T), _live3(h, m, b, T)
    e = np.exp(s3 - s3.max(axis=2, keepdims=True))
    a = np.where(m[:, :, None], e / e.sum(axis=2, keepdims=True), 0.0)
    mk = a.sum(axis=1)
    V = np.einsum("btk,bth->bkh", a, h3) - mk[:, :, None] * c[None]
    n2 = (V * V).sum(axis=2)
    if check_band:
        assert not ((n2 >= EPS / BAND) & (n2 <= EPS * BAND)).any(), "a cluster's |V|^2 sits at the epsilon: draw other inputs"
    r = np.where(n2 > EPS, 1.0 / np.sqrt(np.maximum(n2, EPS)), RMAX)
    y = V * r[:, :, None] / math.sqrt(K)
    return Forward(*P.frozen(a.reshape(b * T, K), r, y.reshape(b, K * HO)))


def _dV(dy, r, y, b, K, HO):
    r = np.asarray(r, F64).reshape(b, K)
    U = math.sqrt(K) * np.asarray(y, F64).reshape(b, K, HO)
    dU = np.asarray(dy, F64).reshape(b, K, HO) / math.sqrt(K)
    proj = r[:, :, None] * (dU - U * (U * dU).sum(axis=2, keepdims=True))
    return np.where((r < RMAX)[:, :, None], proj, r[:, :, None] * dU)


def cancel_scale(dy, h, a, r, y, c, lens=None, T=None):
    """max over the live (b, t, k) of a_tk |dV_k| |h_t - c_k|: the magnitude of the terms that cancel inside ds.  da_tk is the dot
    product dV_k . (h_t - c_k), whose rounding error is a multiple of eps |dV_k| |h_t - c_k| however small the product itself is -- and
    with one live step it is exactly zero, by the normalisation's projection -- and ds_tk = a_tk (da_tk - sum_j a_tj da_tj).  The
    absolute term of ds's bound is therefore taken at max(max|ds|, this)."""
    c = np.asarray(c, F64)
    K, HO = c.shape
    b = np.asarray(dy).shape[0]
    m = live_mask(lens, b, T)
    h3, a3 = _live3(h, m, b, T), _live3(a, m, b, T)
    dV = _dV(dy, r, y, b, K, HO)
    dist = np.sqrt(((h3[:, :, None, :] - c[None, None]) ** 2).sum(axis=3))                       # [B][T][K]
    return float((a3 * np.linalg.norm(dV, axis=2)[:, None, :] * dist).max())


def backward(dy, h, a, r, y, c, lens=None, T=None):
    """From a, r and y AS GIVEN: U = sqrt(K) y, dU = dy / sqrt(K), dV_k = r_k (dU_k - U_k (U_k . dU_k)) where r_k < 1e6 else r_k dU_k,
    da_tk = dV_k . (h_t - c_k), the direct term dh_t = sum_k a_tk dV_k, ds_t = a_t o (da_t - sum_k a_tk da_tk) and the per-clip
    partials dcp[b][k] = -m_k dV_k of the centres' gradient."""
    c = np.asarray(c, F64)
    K, HO = c.shape
    dy = np.asarray(dy, F64)
    b = dy.shape[0]
    m = live_mask(lens, b, T)
    h3 = _live3(h, m, b, T)
    a3 = _live3(a, m, b, T)
    dV = _dV(dy, r, y, b, K, HO)
    da = np.einsum("bkh,bth->btk", dV, h3) - np.einsum("bkh,kh->bk", dV, c)[:, None, :]
    da = np.where(m[:, :, None], da, 0.0)
    dh = np.einsum("btk,bkh->bth", a3, dV)
    ds = a3 * (da - (a3 * da).sum(axis=2, keepdims=True))
    dcp = -a3.sum(axis=1)[:, :, None] * dV
    return Backward(*P.frozen(ds.reshape(b * T, K), dh.reshape(b * T, HO), dcp.reshape(b, K * HO)))


Ref = collections.namedtuple("Ref", "inp lens fwd a32 r32 y32 bwd ds_scale")


@functools.lru_cache(maxsize=None)
def reference(case, k=1, lens=False):
    """Inputs, fp64 forward, its fp32 rounding, and the fp64 backward FROM that rounding.  lens: lstm_plan.lengths (a 0, a T, a -3, a T + 5)."""
    batch, T, HO, K = case
    inp = inputs(batch, T, HO, K, k)
    L = P.lengths(batch, T) if lens else None
    fwd = forward(inp.h, inp.s, inp.c, L, T)
    a32, r32, y32 = P.rounded(fwd.a), P.rounded(fwd.r), P.rounded(fwd.y)
    return Ref(inp, L, fwd, a32, r32, y32, backward(inp.dy, inp.h, a32, r32, y32, inp.c, L, T),
               cancel_scale(inp.dy, inp.h, a32, r32, y32, inp.c, L, T))


def abs_scale(ref, name):
    """The magnitude at which the absolute term of output `name`'s bound is taken: max|want|, and for ds no less than cancel_scale."""
    want = np.abs(np.asarray(getattr(ref.fwd, name) if name in Forward._fields else getattr(ref.bwd, name), F64)).max()
    return float(max(want, ref.ds_scale) if name == "ds" else want) or 1.0


# ---- the layer: projection, pooling, every gradient ------------------------------------------------------------------------------------
def param_names(scope=""):
    """kernel (HO, K), bias (K,), centers (K, HO), in flat-buffer order."""
    return [scope + "netvlad/" + v for v in ("kernel", "bias", "centers")]


PoolCache = collections.namedtuple("PoolCache", "x W c T lens fwd")


def pool_layer_forward(x, W, beta, c, T, lens=None, check_band=True):
    """x [B T][HO] -> y [B][K HO], cache.  A dead row of x takes no part (it is zeroed before the projection, so it may hold NaN)."""
    x = np.asarray(x, F64)
    x = np.where(live_mask(lens, x.shape[0] // T, T).reshape(-1, 1), x, 0.0)
    W = np.asarray(W, F64)
    fwd = forward(x, x @ W + np.asarray(beta, F64), c, lens, T, check_band)
    return fwd.y, PoolCache(x, W, np.asarray(c, F64), T, lens, fwd)


def pool_layer_backward(dy, cache):
    """dy [B][K HO] -> dx [B T][HO] (dead rows 0), dW, dbeta, dc (K, HO)."""
    x, W, c, T, lens, fwd = cache
    bwd = backward(dy, x, fwd.a, fwd.r, fwd.y, c, lens, T)
    return bwd.dh + bwd.ds @ W.T, x.T @ bwd.ds, bwd.ds.sum(axis=0), bwd.dcp.sum(axis=0).reshape(c.shape)


# ---- the LRCN model with NetVLAD pooling (oracle.alexnet_forward, a recurrent stack, the layer above, the head) ------------------------
CELLS = ("lstm", "gru", "blstm", "encoder")


def out_width(cell, H):
    return 2 * H if cell == "blstm" else H


def init_params(rng, num_classes, final_layer, H, layers, image_shape, cell, K, heads=None, T=None, F=None):
    """The cell's own test initialiser (oracle / gru_ref / blstm_ref / encoder_block_ref) with the head output_fc (K HO, classes), plus
    the NetVLAD variables: kernel and centers glorot-uniform, the bias small and NOT zero so that a gradient on the wrong variable shows."""
    from oracle import lrcn_oracle as O
    from tests import blstm_ref, encoder_block_ref, gru_ref
    if cell == "lstm":
        p = O.init_params(rng, num_classes, final_layer, H, layers, image_shape, well_scaled=True)
    elif cell == "encoder":
        p = encoder_block_ref.init_params(rng, num_classes, final_layer, H, layers, image_shape, heads, T, F)
    else:
        p = (gru_ref if cell == "gru" else blstm_ref).init_params(rng, num_classes, final_layer, H, layers, image_shape, "avg")
    HO = out_width(cell, H)
    p["output_fc_w"] = O.truncated_normal(rng, (K * HO, num_classes), math.sqrt(2.0 / (K * HO)))
    p["output_fc_b"] = np.full(num_classes, 0.1, np.float32)
    kn, bn, cn = param_names()
    lim = math.sqrt(6.0 / (HO + K))
    p[kn] = rng.uniform(-lim, lim, (HO, K)).astype(np.float32)
    p[bn] = (0.1 * rng.standard_normal(K)).astype(np.float32)
    p[cn] = rng.uniform(-lim, lim, (K, HO)).astype(np.float32)
    return p


def _stack_forward(p, feat, fpc, H, layers, cell, heads):
    from tests import attn_pool_ref, encoder_block_ref
    if cell == "encoder":
        return encoder_block_ref.stack_forward(feat, p, fpc, layers, heads)
    return attn_pool_ref._stack_forward(p, feat, fpc, H, layers, cell)


def _stack_backward(p, dout, caches, fpc, H, cell):
    from tests import attn_pool_ref, encoder_block_ref
    if cell == "encoder":
        return encoder_block_ref.stack_backward(dout, caches)
    return attn_pool_ref._stack_backward(p, dout, caches, fpc, H, cell)


def model_train_step(p, frames, onehot, fpc, lr, clip_norm, final_layer, H, layers, cell, heads=None):
    """One clipped SGD step in fp64 -> (new_params, loss, global_norm, logits, grads, a)."""
    from oracle import lrcn_oracle as O
    assert cell in CELLS, cell
    feat, ccache = O.alexnet_forward(p, frames, final_layer, F64, True)
    out, caches = _stack_forward(p, feat, fpc, H, layers, cell, heads)
    kn, bn, cn = param_names()
    fused, pc = pool_layer_forward(out, p[kn], p[bn], p[cn], fpc)
    logits = O.xw_plus_b(fused, p["output_fc_w"], p["output_fc_b"], F64)
    loss, d = O.softmax_xent_mean(logits, onehot, F64)
    g = {"output_fc_w": fused.T @ d, "output_fc_b": d.sum(0)}
    d = d @ np.asarray(p["output_fc_w"], F64).T
    dout, g[kn], g[bn], g[cn] = pool_layer_backward(d, pc)
    dfeat, lg = _stack_backward(p, dout, caches, fpc, H, cell)
    g.update(lg)
    g.update(O.alexnet_backward(p, ccache, dfeat, final_layer, F64))
    clipped, gn = O.clip_by_global_norm(g, clip_norm)
    return {k: (np.asarray(p[k], F64) - lr * clipped[k]).astype(np.float32) for k in p}, loss, gn, logits, g, pc.fwd.a
