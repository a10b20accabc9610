"""The pre-LN Transformer encoder block around the self-attention layer (sa_block `encoder`) in plain numpy for the tests:
the four launches of csrc/layer_norm.hip taking THE KERNELS' OWN INPUTS (the backward reads `s` and `stats` as given; the tests hand it
the forward reference's rounded to fp32), the block, the stack with its embedding and final norm and every gradient, and an LRCN train
step in the shape of tests/mhsa_ref.model_train_step.  The attention inside a block is tests/mhsa_ref's.  Nothing here imports the
package: the kernels and engines are checked AGAINST these; tests/test_encoder_block.py proves them equal to torch autograd in fp64.

Every launch function takes `dt`: np.float64 is the reference; np.float32 is the PLAIN FLOAT32 RESTATEMENT (the same formulas with
every intermediate in fp32, numpy's own summation order), whose distance from the reference says how much of a tolerance fp32
arithmetic itself uses up at these shapes and scales -- the tolerance class is decided from it, never from a kernel's output.

Rows are [clips T][W] (clip-major).  Per clip b, L = min(max(lens[b], 0), T) live steps (None: T); a dead row of an input takes no
part (it may hold NaN) and a dead row of y, sum, stats and dx is zeros."""
import collections
import functools
import math

import numpy as np

from tests import lstm_plan as LP
from tests import mhsa_ref as M

F64 = np.float64
EPS = 1e-5

# (clips, T, W): the smallest width, one row; W = 24 (granules on 6 lanes); W = 250 (no multiple of 4: the dword layout, a ragged last
# register) with 105 rows (a ragged last forward workgroup); the workload's width; W = 72 (granule 17 past the first 64-lane round is
# absent: one register group partly filled); W = 65 (dword layout, one element in the second register); the widest row with the most steps
LN_CASES = [(1, 1, 8), (2, 3, 24), (21, 5, 250), (16, 4, 256), (7, 4, 72), (16, 3, 65), (2, 64, 1024)]
SCALES = (1, 40)                     # 40: values of scale 40 at an offset of 40, the tower's feature scale (E[x^2] - mean^2 would lose the variance)
GELU_COUNTS = (1, 3, 4, 255, 4099)
GELU_VALUES = (0.0, 1e-3, -1e-3, 1.0, -1.0, 5.0, -5.0, 12.0, -12.0, 40.0, -40.0)


def case_id(case):
    return "x".join(str(v) for v in case)


# ---- the layer-norm launches -------------------------------------------------------------------------------------------------------------
LnInputs = collections.namedtuple("LnInputs", "x r gamma beta dy dres")
LnForward = collections.namedtuple("LnForward", "sum y stats")              # [rows][W], [rows][W], [rows][2] = mean, rstd
LnBackward = collections.namedtuple("LnBackward", "dx dgbp")                # [rows][W], [clips][2W] = dgamma | dbeta partials


@functools.lru_cache(maxsize=None)
def ln_inputs(clips, T, W, scale=1):
    """x, r ~ scale N(0, 1) + (40 where scale is 40); gamma ~ 1 + 0.3 N, beta ~ 0.3 N; dy, dres ~ N(0, 1)."""
    rng = np.random.default_rng([clips, T, W, scale])
    off = 40.0 if scale == 40 else 0.0
    f = lambda shape, k=1.0, o=0.0: (rng.standard_normal(shape) * k + o).astype(np.float32)
    rows = clips * T
    return LnInputs(*LP.frozen(f((rows, W), scale, off), f((rows, W), scale, off), f(W, 0.3, 1.0), f(W, 0.3), f((rows, W)), f((rows, W))))


def _live(a, m, dt):
    return np.where(m, np.asarray(a, dt), dt(0))


def ln_forward(x, r, gamma, beta, T, lens=None, eps=EPS, dt=F64):
    """s = x + r (r None: x); mean, then the variance of the centred values; y = (s - mean) rstd gamma + beta."""
    rows, W = np.asarray(x).shape
    m = M.live_mask(lens, rows // T, T).reshape(-1, 1)
    s = _live(x, m, dt)
    if r is not None:
        s = s + _live(r, m, dt)
    mean = s.sum(axis=1, keepdims=True, dtype=dt) / dt(W)
    c = s - mean
    var = (c * c).sum(axis=1, keepdims=True, dtype=dt) / dt(W)
    rstd = dt(1) / np.sqrt(var + dt(eps))
    y = c * rstd * np.asarray(gamma, dt) + np.asarray(beta, dt)
    stats = np.concatenate([mean, rstd], axis=1)
    return LnForward(*LP.frozen(np.where(m, s, dt(0)), np.where(m, y, dt(0)), np.where(m, stats, dt(0))))


def ln_backward(dy, s, gamma, stats, dres, T, lens=None, dt=F64):
    """From s and stats AS GIVEN: x^ = (s - mean) rstd, dy^ = dy gamma, dx = rstd (dy^ - mean(dy^) - x^ mean(dy^ x^)) + dres; the
    per-clip partials of dgamma = sum dy x^ and dbeta = sum dy over the clip's live rows."""
    rows, W = np.asarray(dy).shape
    clips = rows // T
    m = M.live_mask(lens, clips, T).reshape(-1, 1)
    dy, s, stats = _live(dy, m, dt), _live(s, m, dt), _live(stats, m, dt)
    mean, rstd = stats[:, :1], stats[:, 1:]
    xh = (s - mean) * rstd
    dyh = dy * np.asarray(gamma, dt)
    m1 = dyh.sum(axis=1, keepdims=True, dtype=dt) / dt(W)
    m2 = (dyh * xh).sum(axis=1, keepdims=True, dtype=dt) / dt(W)
    dx = rstd * (dyh - m1 - xh * m2)
    if dres is not None:
        dx = dx + _live(dres, m, dt)
    dgbp = np.concatenate([np.where(m, dy * xh, dt(0)).reshape(clips, T, W).sum(axis=1, dtype=dt),
                           np.where(m, dy, dt(0)).reshape(clips, T, W).sum(axis=1, dtype=dt)], axis=1)
    return LnBackward(*LP.frozen(np.where(m, dx, dt(0)), dgbp))


LnRef = collections.namedtuple("LnRef", "inp lens fwd s32 stats32 bwd")


@functools.lru_cache(maxsize=None)
def ln_reference(case, scale=1, lens=False, residual=True):
    """Inputs, the fp64 forward, its sum and stats rounded to fp32, and the fp64 backward FROM those roundings.  residual False: no r,
    no sum and no dres (the backward's s is then x itself)."""
    clips, T, W = case
    inp = ln_inputs(clips, T, W, scale)
    L = LP.lengths(clips, T) if lens else None
    fwd = ln_forward(inp.x, inp.r if residual else None, inp.gamma, inp.beta, T, L)
    s32, stats32 = LP.rounded(fwd.sum), LP.rounded(fwd.stats)
    return LnRef(inp, L, fwd, s32, stats32, ln_backward(inp.dy, s32, inp.gamma, stats32, inp.dres if residual else None, T, L))


# ---- GELU, the exact form ----------------------------------------------------------------------------------------------------------------
_erfc = np.vectorize(math.erfc, otypes=[F64])


def _cdf(u, dt):
    """Phi(u) = erfc(-u / sqrt 2) / 2 (erfc: no cancellation in the left tail)."""
    if dt == F64:
        return 0.5 * _erfc(-u / math.sqrt(2.0))
    return (dt(0.5) * _erfc((-u * dt(math.sqrt(0.5))).astype(F64)).astype(dt)).astype(dt)       # (fp32: erfc itself correctly rounded)


def gelu(u, dt=F64):
    u = np.asarray(u, dt)
    return u * _cdf(u, dt)


def gelu_grad(df, u, dt=F64):
    """du = df (Phi(u) + u phi(u))."""
    u = np.asarray(u, dt)
    return np.asarray(df, dt) * (_cdf(u, dt) + u * (dt(1.0 / math.sqrt(2.0 * math.pi)) * np.exp(dt(-0.5) * u * u)))


@functools.lru_cache(maxsize=None)
def gelu_inputs(count):
    """u: GELU_VALUES first (as many as fit), then 3 N(0, 1); df ~ N(0, 1)."""
    rng = np.random.default_rng([count, 11])
    u = (3.0 * rng.standard_normal(count)).astype(np.float32)
    k = min(count, len(GELU_VALUES))
    u[:k] = GELU_VALUES[:k]
    return LP.frozen(u, rng.standard_normal(count).astype(np.float32))


# ---- the block, the stack ----------------------------------------------------------------------------------------------------------------
LAYER_VARS = ("norm1_gamma", "norm1_beta", "qkv_kernel", "qkv_bias", "out_kernel", "out_bias", "position_bias", "norm2_gamma", "norm2_beta",
              "ffn1_kernel", "ffn1_bias", "ffn2_kernel", "ffn2_bias")


def var(layer, name, scope=""):
    """layer None: the embedding (kernel | bias); layer -1: the final norm (gamma | beta)."""
    where = "embed" if layer is None else "final_norm" if layer < 0 else "layer_%d" % layer
    return "%sself_attention/%s/%s" % (scope, where, name)


def layer_names(layer, scope="", positions=True):
    return [var(layer, v, scope) for v in LAYER_VARS if positions or v != "position_bias"]


def param_names(layers, scope="", positions=True):
    """The stack's variables in LRCNEngine's flat-buffer order: the embedding, the layers ascending, the final norm."""
    names = [var(None, "kernel", scope), var(None, "bias", scope)]
    for l in range(layers):
        names += layer_names(l, scope, positions)
    return names + [var(-1, "gamma", scope), var(-1, "beta", scope)]


def param_shapes(layers, d, H, F, heads, T, scope="", positions=True):
    shp = dict(norm1_gamma=(H,), norm1_beta=(H,), qkv_kernel=(H, 3 * H), qkv_bias=(3 * H,), out_kernel=(H, H), out_bias=(H,),
               position_bias=(heads, 2 * T - 1), norm2_gamma=(H,), norm2_beta=(H,), ffn1_kernel=(H, F), ffn1_bias=(F,), ffn2_kernel=(F, H),
               ffn2_bias=(H,))
    out = {var(None, "kernel", scope): (d, H), var(None, "bias", scope): (H,), var(-1, "gamma", scope): (H,), var(-1, "beta", scope): (H,)}
    for l in range(layers):
        out.update({var(l, v, scope): shp[v] for v in LAYER_VARS if positions or v != "position_bias"})
    return {n: out[n] for n in param_names(layers, scope, positions)}


def default_init(rng, shapes, perturb=0.0):
    """The engines' initialisers: kernels glorot-uniform, gammas ones, betas, biases and the position bias zeros.  perturb > 0 adds
    perturb N(0, 1) to everything that is not a kernel (tests that must see a gradient land on the right variable)."""
    p = {}
    for n, shp in shapes.items():
        if n.endswith("kernel"):
            lim = math.sqrt(6.0 / (shp[0] + shp[1]))
            p[n] = rng.uniform(-lim, lim, shp).astype(np.float32)
        else:
            base = np.ones(shp) if n.endswith("gamma") else np.zeros(shp)
            p[n] = (base + perturb * rng.standard_normal(shp)).astype(np.float32)
    return p


BlockCache = collections.namedtuple("BlockCache", "x ln1 n1 att a ln2 n2 u f W1 W2 g1 g2 T lens")


def block_forward(x, p, layer, heads, T, lens=None, scope="", positions=True):
    """x [rows][H], the residual stream (dead rows zeros) -> the stream behind the block, cache."""
    g = lambda v: np.asarray(p[var(layer, v, scope)], F64)
    m = M.live_mask(lens, x.shape[0] // T, T).reshape(-1, 1)
    ln1 = ln_forward(x, None, g("norm1_gamma"), g("norm1_beta"), T, lens)
    o, att = M.layer_forward(ln1.y, g("qkv_kernel"), g("qkv_bias"), g("out_kernel"), g("out_bias"), g("position_bias") if positions else None,
                             heads, T, lens)
    ln2 = ln_forward(x, o, g("norm2_gamma"), g("norm2_beta"), T, lens)
    u = ln2.y @ g("ffn1_kernel") + g("ffn1_bias")
    f = gelu(u)
    out = np.where(m, ln2.sum + f @ g("ffn2_kernel") + g("ffn2_bias"), 0.0)
    return out, BlockCache(x, ln1, ln1.y, att, ln2.sum, ln2, ln2.y, u, f, g("ffn1_kernel"), g("ffn2_kernel"), g("norm1_gamma"), g("norm2_gamma"),
                           T, lens)


def block_backward(dout, c, layer, scope="", positions=True):
    """dout: the gradient of the stream behind the block (dead rows ignored) -> of the stream in front of it, {name: gradient}."""
    T, lens = c.T, c.lens
    m = M.live_mask(lens, c.x.shape[0] // T, T).reshape(-1, 1)
    dout = np.where(m, np.asarray(dout, F64), 0.0)
    grads = {}
    n = lambda v: var(layer, v, scope)
    grads[n("ffn2_kernel")], grads[n("ffn2_bias")] = c.f.T @ dout, dout.sum(axis=0)
    du = gelu_grad(dout @ c.W2.T, c.u)
    grads[n("ffn1_kernel")], grads[n("ffn1_bias")] = c.n2.T @ du, du.sum(axis=0)
    b2 = ln_backward(du @ c.W1.T, c.a, c.g2, c.ln2.stats, dout, T, lens)
    W = c.x.shape[1]
    grads[n("norm2_gamma")], grads[n("norm2_beta")] = b2.dgbp[:, :W].sum(axis=0), b2.dgbp[:, W:].sum(axis=0)
    da = b2.dx
    dn1, ag = M.layer_backward(da, c.att)
    for k, v in zip(("qkv_kernel", "qkv_bias", "out_kernel", "out_bias", "position_bias"), ag):
        grads[n(k)] = v
    b1 = ln_backward(dn1, c.x, c.g1, c.ln1.stats, da, T, lens)
    grads[n("norm1_gamma")], grads[n("norm1_beta")] = b1.dgbp[:, :W].sum(axis=0), b1.dgbp[:, W:].sum(axis=0)
    return b1.dx, grads


StackCache = collections.namedtuple("StackCache", "feat We blocks xL lnf gf T lens layers positions")


def stack_forward(feat, p, T, layers, heads, lens=None, scope="", positions=True):
    """feat [rows][d] -> the final norm's output [rows][H] (dead rows zeros), cache.  A dead row of feat takes no part."""
    feat = np.asarray(feat, F64)
    m = M.live_mask(lens, feat.shape[0] // T, T).reshape(-1, 1)
    feat = np.where(m, feat, 0.0)
    We = np.asarray(p[var(None, "kernel", scope)], F64)
    x = np.where(m, feat @ We + np.asarray(p[var(None, "bias", scope)], F64), 0.0)
    blocks = []
    for l in range(layers):
        x, c = block_forward(x, p, l, heads, T, lens, scope, positions)
        blocks.append(c)
    gf = np.asarray(p[var(-1, "gamma", scope)], F64)
    lnf = ln_forward(x, None, gf, p[var(-1, "beta", scope)], T, lens)
    return lnf.y, StackCache(feat, We, blocks, x, lnf, gf, T, lens, layers, positions)


def stack_backward(dout, c, scope=""):
    """-> dfeat, {name: gradient}."""
    W = c.xL.shape[1]
    bf = ln_backward(dout, c.xL, c.gf, c.lnf.stats, None, c.T, c.lens)
    grads = {var(-1, "gamma", scope): bf.dgbp[:, :W].sum(axis=0), var(-1, "beta", scope): bf.dgbp[:, W:].sum(axis=0)}
    dx = bf.dx
    for l in reversed(range(c.layers)):
        dx, g = block_backward(dx, c.blocks[l], l, scope, c.positions)
        grads.update(g)
    grads[var(None, "kernel", scope)], grads[var(None, "bias", scope)] = c.feat.T @ dx, dx.sum(axis=0)
    return dx @ c.We.T, grads


def last_P(c):
    """The attention weights [clips][heads][T][T] of the last block."""
    return c.blocks[-1].att.fwd.P


# ---- the LRCN model with encoder blocks (oracle.alexnet_forward, the stack above, a fusion, the head) ----------------------------------
def init_params(rng, num_classes, final_layer, H, layers, image_shape, heads, T, F, positions=True, attn_dim=None):
    """The oracle's well-scaled AlexNet parameters, the stack at the engines' DEFAULT initialisation (default_init: nothing rescaled,
    no tame_first_layer), the (H, C) head and, with attn_dim, attention_pool's variables as tests/mhsa_ref.init_params draws them."""
    from oracle import lrcn_oracle as O
    p = O.init_params(rng, num_classes, final_layer, H, layers, image_shape, classifier="none", well_scaled=True)
    d = {"fc6": 4096, "fc7": 4096}.get(final_layer, num_classes)
    p.update(default_init(rng, param_shapes(layers, d, H, F, heads, T, positions=positions)))
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


def model_train_step(p, frames, onehot, fpc, lr, clip_norm, final_layer, H, layers, heads, fusion, positions=True):
    """One clipped SGD step in fp64 -> (new_params, loss, global_norm, logits, grads, P of the last block)."""
    from oracle import lrcn_oracle as O
    from tests import attn_pool_ref, gru_ref
    feat, ccache = O.alexnet_forward(p, frames, final_layer, F64, True)
    out, cache = stack_forward(feat, p, fpc, layers, heads, positions=positions)
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
    dfeat, sg = stack_backward(dout, cache)
    g.update(sg)
    g.update(O.alexnet_backward(p, ccache, dfeat, final_layer, F64))
    clipped, gn = O.clip_by_global_norm(g, clip_norm)
    return {k: (np.asarray(p[k], F64) - lr * clipped[k]).astype(np.float32) for k in p}, loss, gn, logits, g, last_P(cache)
