"""The dropouts of the self-attention model (sa_attn_dropout, sa_dropout, sa_drop_path) in plain numpy for the tests: the
mask definition of include/vltf.h with its streams, counters and clip0; the dropped attention forward / backward on tests/mhsa_ref's
pieces; the dropped add-and-norm and the branch gradient on tests/encoder_block_ref's; the block, the stack and an LRCN train step with
the three options.  Nothing here imports the package: the kernels and engines are checked AGAINST these; tests/test_encoder_dropout.py
proves them equal to torch autograd in fp64 with the masks applied as constants.

Every function takes `dt`: np.float64 is the reference, np.float32 the PLAIN FLOAT32 RESTATEMENT (encoder_block_ref's convention), whose
distance from the reference decides a tolerance class.  The masks themselves are exact in either: integers and one fp32 compare.
branch_factor32 / drop_sum32 / branch_grad32 are the BITWISE restatement of the branch arithmetic: the device must equal them bit for bit.

MASK DEFINITION (the generator of tests/fc_dropout_ref.keep_mask under a stream constant of its own):
    s = seed ^ splitmix64(0x5AD000000000 + salt);  h = splitmix64(s ^ splitmix64(e));  kept = (h >> 40) * 2^-24 < keep    (fp32 compare)
    salt = node << 12 | layer << 2 | site,  site 0 = attention weights, 1 = attention-branch elements, 2 = feed-forward-branch
    elements, 3 = path draws;  counters of the GLOBAL batch, clip0 = the index in it of the first clip given:
        weights          e = (((clip0 + b) heads + h) T + q) T + k
        branch elements  e = ((clip0 + b) T + t) W + col
        path             e = 2 (clip0 + b) + branch         branch 0 = attention, 1 = feed-forward
Rows are [clips T][W] (clip-major); lens as everywhere: dead rows take no part, their draws are unused."""
import collections
import math

import numpy as np

from tests import encoder_block_ref as E
from tests import lstm_plan as LP
from tests import mhsa_ref as M
from tests.fc_dropout_ref import _splitmix64_int, splitmix64

F64, F32 = np.float64, np.float32
_M64 = (1 << 64) - 1
STREAM = 0x5AD000000000
SITES = ("weights", "attn_branch", "ffn_branch", "path")


# ---- the masks ---------------------------------------------------------------------------------------------------------------------------
def salt_of(node, layer, site):
    return (int(node) << 12) | (int(layer) << 2) | SITES.index(site)


def seed_of(draw_index):
    """The seed of the step with this draw index (the engines' dropout_seed; the _st launches form it from the step state)."""
    return ((int(draw_index) << 20) ^ 0x5DEECE66D) & _M64


def keep_of(rate):
    """The keep of a rate as a launch gets it: the fp32 nearest to 1 - rate."""
    return F32(1.0 - float(rate))


def path_keep(rate, layer, layers):
    """k_l = 1 - p (l + 1) / L, Huang et al.'s linear rule, as the fp32 a launch gets."""
    return F32(1.0 - float(rate) * (int(layer) + 1) / int(layers))


def uniforms(seed, salt, counters):
    """float32 u in [0, 1) of the draws at `counters` (any shape of non-negative integers) of the stream (seed, salt)."""
    s = np.uint64((int(seed) & _M64) ^ _splitmix64_int((STREAM + int(salt)) & _M64))
    h = splitmix64(s ^ splitmix64(np.asarray(counters).astype(np.uint64)))
    return (h >> np.uint64(40)).astype(F32) * F32(1.0 / 16777216.0)                     # 24 bits: exact in float32


def kept(seed, salt, counters, keep):
    return uniforms(seed, salt, counters) < F32(keep)


def weight_mask(seed, salt, clips, heads, T, keep, clip0=0):
    """bool [clips][heads][T][T]."""
    n = clips * heads * T * T
    return kept(seed, salt, int(clip0) * heads * T * T + np.arange(n, dtype=np.int64), keep).reshape(clips, heads, T, T)


def elem_mask(seed, salt, clips, T, W, keep, clip0=0):
    """bool [clips T][W]."""
    n = clips * T * W
    return kept(seed, salt, int(clip0) * T * W + np.arange(n, dtype=np.int64), keep).reshape(clips * T, W)


def path_mask(seed, salt, clips, branch, keep_path, clip0=0):
    """bool [clips]: which clips keep branch 0 | 1."""
    return kept(seed, salt, 2 * (int(clip0) + np.arange(clips, dtype=np.int64)) + int(branch), keep_path)


# ---- the branch factor and the three places it enters -----------------------------------------------------------------------------------
def branch_factor32(seed, salt_elem, salt_path, clips, T, W, branch, keep, keep_path, clip0=0):
    """float32 [clips T][W], BITWISE: fe = kept_e ? 1.0f / keep : 0, fp = path_kept ? 1.0f / keep_path : 0, f = fmul(fe, fp); a factor
    whose keep is 1 is exactly 1 (and draws nothing)."""
    keep, keep_path = F32(keep), F32(keep_path)
    fe = np.ones((clips * T, W), F32)
    if keep < 1:
        fe = np.where(elem_mask(seed, salt_elem, clips, T, W, keep, clip0), F32(1) / keep, F32(0)).astype(F32)
    fp = np.ones(clips, F32)
    if keep_path < 1:
        fp = np.where(path_mask(seed, salt_path, clips, branch, keep_path, clip0), F32(1) / keep_path, F32(0)).astype(F32)
    f = fe * np.repeat(fp, T)[:, None]
    assert f.dtype == F32
    return f


def branch_factor(seed, salt_elem, salt_path, clips, T, W, branch, keep, keep_path, clip0=0, dt=F64):
    """The same factor in dt: mask / keep x path mask / keep_path with the keeps the launch got (fp32 values) -- fp64: the reference."""
    if dt == F32:
        return branch_factor32(seed, salt_elem, salt_path, clips, T, W, branch, keep, keep_path, clip0)
    keep, keep_path = F32(keep), F32(keep_path)
    fe = elem_mask(seed, salt_elem, clips, T, W, keep, clip0) / F64(keep) if keep < 1 else np.ones((clips * T, W))
    fp = path_mask(seed, salt_path, clips, branch, keep_path, clip0) / F64(keep_path) if keep_path < 1 else np.ones(clips)
    return fe * np.repeat(fp, T)[:, None]


def _dead_to_zero(a, T, lens):
    rows = a.shape[0]
    return np.where(M.live_mask(lens, rows // T, T).reshape(-1, 1), a, a.dtype.type(0))


def drop_sum32(x, r, f32, T, lens=None):
    """float32 [rows][W], BITWISE: sum = fadd(x, fmul(r, f)), no fma; dead rows zeros (x and r are not read there)."""
    x, r = np.asarray(x, F32), np.asarray(r, F32)
    m = M.live_mask(lens, x.shape[0] // T, T).reshape(-1, 1)
    with np.errstate(invalid="ignore"):
        rf = np.where(m, r, F32(0)) * f32
        s = np.where(m, x, F32(0)) + rf
    assert s.dtype == F32
    return _dead_to_zero(s, T, lens)


def branch_grad32(ds, f32, T, lens=None):
    """float32 [rows][W], BITWISE: dr = fmul(ds, f); dead rows zeros."""
    ds = np.asarray(ds, F32)
    m = M.live_mask(lens, ds.shape[0] // T, T).reshape(-1, 1)
    d = np.where(m, ds, F32(0)) * f32
    assert d.dtype == F32
    return d


def ln_drop_forward(x, r, f, gamma, beta, T, lens=None, eps=E.EPS, dt=F64):
    """The dropped add-and-norm: encoder_block_ref.ln_forward of x and r f (f: branch_factor in dt).  -> LnForward(sum, y, stats)."""
    m = M.live_mask(lens, np.asarray(x).shape[0] // T, T).reshape(-1, 1)
    rf = np.where(m, np.asarray(r, dt), dt(0)) * np.asarray(f, dt)
    return E.ln_forward(x, rf, gamma, beta, T, lens, eps, dt)


def branch_grad(ds, f, T, lens=None, dt=F64):
    m = M.live_mask(lens, np.asarray(ds).shape[0] // T, T).reshape(-1, 1)
    return np.where(m, np.asarray(ds, dt), dt(0)) * np.asarray(f, dt)


# ---- the dropped attention (the kernels' contract) -----------------------------------------------------------------------------------
def weight_factor(seed, salt, clips, heads, T, keep, clip0=0, dt=F64):
    """[clips][heads][T][T] in dt: kept ? 1 / keep : 0 -- fp32: the launch's own fl(1.0f / keep); fp64: 1 / keep of the fp32 keep."""
    keep = F32(keep)
    if keep >= 1:
        return np.ones((clips, heads, T, T), dt)
    inv = F32(1) / keep if dt == F32 else 1.0 / F64(keep)
    return np.where(weight_mask(seed, salt, clips, heads, T, keep, clip0), inv, dt(0)).astype(dt)


def _qkv(qkv, m, b, T, H, heads, dt):
    x = np.where(m.reshape(-1, 1), np.asarray(qkv, dt), dt(0))
    return (M.split_heads(x[:, i * H:(i + 1) * H], b, T, heads) for i in range(3))


def attn_forward(qkv, pos, heads, Fw, lens=None, T=None, dt=F64):
    """mhsa_ref.forward with ctx = (P o Fw) V; P is returned UNDROPPED.  Fw: weight_factor, or None for no dropout."""
    H = np.asarray(qkv).shape[1] // 3
    b = np.asarray(qkv).shape[0] // T
    m = M.live_mask(lens, b, T)
    Q, K, V = _qkv(qkv, m, b, T, H, heads, dt)
    S = (Q @ K.transpose(0, 1, 3, 2)) * dt(1.0 / math.sqrt(H // heads))
    if pos is not None:
        S = S + np.asarray(pos, dt)[:, M.rel_index(T)][None]
    pair = m[:, None, :, None] & m[:, None, None, :]
    S = np.where(pair, S, dt(-np.inf))
    mx = S.max(axis=3, keepdims=True)
    w = np.exp(S - np.where(np.isfinite(mx), mx, dt(0)))
    z = w.sum(axis=3, keepdims=True, dtype=dt)
    P = np.where(pair, w / np.where(z > 0, z, dt(1)), dt(0)).astype(dt)
    Pd = P if Fw is None else P * np.asarray(Fw, dt)
    return M.Forward(*LP.frozen(P, M.merge_heads(Pd @ V)))


def attn_backward(dctx, qkv, P, heads, Fw, lens=None, T=None, positions=True, dt=F64):
    """From the UNDROPPED P as given: dV = (P o Fw)^T dctx, dP = (dctx V^T) o Fw, dS = P o (dP - rowsum(dP o P)), the rest as
    mhsa_ref.backward."""
    H = np.asarray(qkv).shape[1] // 3
    b = np.asarray(qkv).shape[0] // T
    m = M.live_mask(lens, b, T)
    Q, K, V = _qkv(qkv, m, b, T, H, heads, dt)
    dO = M.split_heads(np.where(m.reshape(-1, 1), np.asarray(dctx, dt), dt(0)), b, T, heads)
    pair = m[:, None, :, None] & m[:, None, None, :]
    P = np.where(pair, np.asarray(P, dt).reshape(b, heads, T, T), dt(0))
    Fw = np.ones_like(P) if Fw is None else np.asarray(Fw, dt)
    dV = (P * Fw).transpose(0, 1, 3, 2) @ dO
    dP = (dO @ V.transpose(0, 1, 3, 2)) * Fw
    dS = P * (dP - (dP * P).sum(axis=3, keepdims=True, dtype=dt))
    scale = dt(1.0 / math.sqrt(H // heads))
    dQ, dK = dS @ K * scale, dS.transpose(0, 1, 3, 2) @ Q * scale
    dqkv = np.concatenate([M.merge_heads(dQ), M.merge_heads(dK), M.merge_heads(dV)], axis=1)
    dposp = None
    if positions:
        dposp = np.zeros((b, heads, 2 * T - 1), dt)
        rel = M.rel_index(T)
        for r in range(2 * T - 1):
            dposp[:, :, r] = (dS * (rel == r)).sum(axis=(2, 3), dtype=dt)
        LP.frozen(dposp)
    return M.Backward(LP.frozen(dqkv), dposp)


# ---- the options of a model, the block, the stack ---------------------------------------------------------------------------------------
class Drop(collections.namedtuple("Drop", "attn elem path seed node clip0 layers")):
    """The three rates (0 = off) and what the draws of one training pass come from."""

    def weights(self, layer, clips, heads, T, dt=F64):
        if not self.attn:
            return None
        return weight_factor(self.seed, salt_of(self.node, layer, "weights"), clips, heads, T, keep_of(self.attn), self.clip0, dt)

    def branch(self, layer, branch, clips, T, W, dt=F64):
        """The factor of branch 0 | 1 of `layer`, or None with both branch options off."""
        if not (self.elem or self.path):
            return None
        return branch_factor(self.seed, salt_of(self.node, layer, SITES[1 + branch]), salt_of(self.node, layer, "path"), clips, T, W, branch,
                             keep_of(self.elem), path_keep(self.path, layer, self.layers), self.clip0, dt)


def drop(attn=0.0, elem=0.0, path=0.0, seed=0, node=0, clip0=0, layers=1):
    return Drop(float(attn or 0), float(elem or 0), float(path or 0), int(seed), int(node), int(clip0), int(layers))


LayerCache = collections.namedtuple("LayerCache", "x Wqkv Wo qkv heads T lens fwd positions Fw")


def layer_forward(x, Wqkv, bqkv, Wo, bo, pos, heads, T, Fw, lens=None, dt=F64):
    """mhsa_ref.layer_forward with the weights dropped by Fw (None: no dropout)."""
    x = np.asarray(x, dt)
    m = M.live_mask(lens, x.shape[0] // T, T).reshape(-1, 1)
    x = np.where(m, x, dt(0))
    Wqkv, Wo = np.asarray(Wqkv, dt), np.asarray(Wo, dt)
    qkv = x @ Wqkv + np.asarray(bqkv, dt)
    fwd = attn_forward(qkv, pos, heads, Fw, lens, T, dt)
    y = np.where(m, fwd.ctx @ Wo + np.asarray(bo, dt), dt(0))
    return y, LayerCache(x, Wqkv, Wo, qkv, heads, T, lens, fwd, pos is not None, Fw)


def layer_backward(dy, c, dt=F64):
    dy = np.where(M.live_mask(c.lens, c.x.shape[0] // c.T, c.T).reshape(-1, 1), np.asarray(dy, dt), dt(0))
    bwd = attn_backward(dy @ c.Wo.T, c.qkv, c.fwd.P, c.heads, c.Fw, c.lens, c.T, c.positions, dt)
    grads = [c.x.T @ bwd.dqkv, bwd.dqkv.sum(axis=0), c.fwd.ctx.T @ dy, dy.sum(axis=0)]
    if c.positions:
        grads.append(bwd.dposp.sum(axis=0))
    return bwd.dqkv @ c.Wqkv.T, grads


def plain_stack_forward(x, params, T, layers, heads, dr, lens=None, scope="", positions=True, dt=F64):
    """mhsa_ref.stack_forward (sa_block plain) with sa_attn_dropout."""
    caches = []
    clips = np.asarray(x).shape[0] // T
    for l in range(layers):
        names = M.param_names(l, scope, positions)
        x, c = layer_forward(x, *(params[n] for n in names[:4]), params[names[4]] if positions else None, heads, T,
                             dr.weights(l, clips, heads, T, dt), lens, dt)
        caches.append(c)
    return x, caches


def plain_stack_backward(dout, caches, scope="", dt=F64):
    grads = {}
    for l in reversed(range(len(caches))):
        dout, g = layer_backward(dout, caches[l], dt)
        grads.update(zip(M.param_names(l, scope, caches[l].positions), g))
    return dout, grads


BlockCache = collections.namedtuple("BlockCache", "x ln1 n1 att a ln2 n2 u f W1 W2 g1 g2 T lens f0 f1")


def block_forward(x, p, layer, heads, T, dr, lens=None, scope="", positions=True, dt=F64):
    """encoder_block_ref.block_forward with a = x + o f0, x' = a + m f1 and the dropped weights inside the attention."""
    g = lambda v: np.asarray(p[E.var(layer, v, scope)], dt)
    rows, W = np.asarray(x).shape
    clips = rows // T
    m = M.live_mask(lens, clips, T).reshape(-1, 1)
    f0, f1 = dr.branch(layer, 0, clips, T, W, dt), dr.branch(layer, 1, clips, T, W, dt)
    one = np.ones((rows, W), dt)
    ln1 = E.ln_forward(x, None, g("norm1_gamma"), g("norm1_beta"), T, lens, dt=dt)
    o, att = layer_forward(ln1.y, g("qkv_kernel"), g("qkv_bias"), g("out_kernel"), g("out_bias"), g("position_bias") if positions else None,
                           heads, T, dr.weights(layer, clips, heads, T, dt), lens, dt)
    ln2 = ln_drop_forward(x, o, one if f0 is None else f0, g("norm2_gamma"), g("norm2_beta"), T, lens, dt=dt)
    u = ln2.y @ g("ffn1_kernel") + g("ffn1_bias")
    f = E.gelu(u, dt)
    mo = f @ g("ffn2_kernel") + g("ffn2_bias")
    out = np.where(m, ln2.sum + mo * (one if f1 is None else f1), dt(0))
    return out, BlockCache(x, ln1, ln1.y, att, ln2.sum, ln2, ln2.y, u, f, g("ffn1_kernel"), g("ffn2_kernel"), g("norm1_gamma"),
                           g("norm2_gamma"), T, lens, f0, f1)


def block_backward(dout, c, layer, scope="", positions=True, dt=F64):
    T, lens = c.T, c.lens
    m = M.live_mask(lens, c.x.shape[0] // T, T).reshape(-1, 1)
    dout = np.where(m, np.asarray(dout, dt), dt(0))
    grads = {}
    n = lambda v: E.var(layer, v, scope)
    dm = dout if c.f1 is None else dout * c.f1                        # the gradient that enters the feed-forward branch
    grads[n("ffn2_kernel")], grads[n("ffn2_bias")] = c.f.T @ dm, dm.sum(axis=0)
    du = E.gelu_grad(dm @ c.W2.T, c.u, dt)
    grads[n("ffn1_kernel")], grads[n("ffn1_bias")] = c.n2.T @ du, du.sum(axis=0)
    b2 = E.ln_backward(du @ c.W1.T, c.a, c.g2, c.ln2.stats, dout, T, lens, dt)
    W = c.x.shape[1]
    grads[n("norm2_gamma")], grads[n("norm2_beta")] = b2.dgbp[:, :W].sum(axis=0), b2.dgbp[:, W:].sum(axis=0)
    da = b2.dx
    do = da if c.f0 is None else da * c.f0                            # ... the attention branch
    dn1, ag = layer_backward(do, c.att, dt)
    for k, v in zip(("qkv_kernel", "qkv_bias", "out_kernel", "out_bias", "position_bias"), ag):
        grads[n(k)] = v
    b1 = E.ln_backward(dn1, c.x, c.g1, c.ln1.stats, da, T, lens, dt)
    grads[n("norm1_gamma")], grads[n("norm1_beta")] = b1.dgbp[:, :W].sum(axis=0), b1.dgbp[:, W:].sum(axis=0)
    return b1.dx, grads


def stack_forward(feat, p, T, layers, heads, dr, lens=None, scope="", positions=True, dt=F64):
    """encoder_block_ref.stack_forward with the options of dr (a Drop whose `layers` is this stack's)."""
    feat = np.asarray(feat, dt)
    m = M.live_mask(lens, feat.shape[0] // T, T).reshape(-1, 1)
    feat = np.where(m, feat, dt(0))
    We = np.asarray(p[E.var(None, "kernel", scope)], dt)
    x = np.where(m, feat @ We + np.asarray(p[E.var(None, "bias", scope)], dt), dt(0))
    blocks = []
    for l in range(layers):
        x, c = block_forward(x, p, l, heads, T, dr, lens, scope, positions, dt)
        blocks.append(c)
    gf = np.asarray(p[E.var(-1, "gamma", scope)], dt)
    lnf = E.ln_forward(x, None, gf, p[E.var(-1, "beta", scope)], T, lens, dt=dt)
    return lnf.y, E.StackCache(feat, We, blocks, x, lnf, gf, T, lens, layers, positions)


def stack_backward(dout, c, scope="", dt=F64):
    W = c.xL.shape[1]
    bf = E.ln_backward(dout, c.xL, c.gf, c.lnf.stats, None, c.T, c.lens, dt)
    grads = {E.var(-1, "gamma", scope): bf.dgbp[:, :W].sum(axis=0), E.var(-1, "beta", scope): bf.dgbp[:, W:].sum(axis=0)}
    dx = bf.dx
    for l in reversed(range(c.layers)):
        dx, g = block_backward(dx, c.blocks[l], l, scope, c.positions, dt)
        grads.update(g)
    grads[E.var(None, "kernel", scope)], grads[E.var(None, "bias", scope)] = c.feat.T @ dx, dx.sum(axis=0)
    return dx @ c.We.T, grads


# ---- the LRCN model with the options (oracle.alexnet_forward, a stack above, a fusion, the head) ---------------------------------------
def model_train_step(p, frames, onehot, fpc, lr, clip_norm, final_layer, H, layers, heads, fusion, dr, block="encoder", positions=True,
                     dt=F64):
    """One clipped SGD step -> (new_params, loss, global_norm, logits, grads, UNDROPPED P of the last layer).  block: encoder | plain."""
    from oracle import lrcn_oracle as O
    from tests import gru_ref
    feat, ccache = O.alexnet_forward(p, frames, final_layer, dt, True)
    if block == "encoder":
        out, cache = stack_forward(feat, p, fpc, layers, heads, dr, positions=positions, dt=dt)
    else:
        out, cache = plain_stack_forward(feat, p, fpc, layers, heads, dr, positions=positions, dt=dt)
    g = {}
    fused = gru_ref.fuse(out, fpc, H, fusion)
    logits = O.xw_plus_b(fused, p["output_fc_w"], p["output_fc_b"], dt) if "output_fc_w" in p else fused
    loss, d = O.softmax_xent_mean(logits, onehot, dt)
    if "output_fc_w" in p:
        g["output_fc_w"], g["output_fc_b"] = fused.T @ d, d.sum(0)
        d = d @ np.asarray(p["output_fc_w"], dt).T
    dout = gru_ref.fuse_backward(d, fpc, H, fusion)
    dfeat, sg = stack_backward(dout, cache, dt=dt) if block == "encoder" else plain_stack_backward(dout, cache, dt=dt)
    g.update(sg)
    g.update(O.alexnet_backward(p, ccache, dfeat, final_layer, dt))
    clipped, gn = O.clip_by_global_norm(g, clip_norm)
    P = cache.blocks[-1].att.fwd.P if block == "encoder" else cache[-1].fwd.P
    return {k: (np.asarray(p[k], F64) - lr * clipped[k]).astype(np.float32) for k in p}, loss, gn, logits, g, P
