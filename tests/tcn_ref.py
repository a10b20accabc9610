"""Dilated temporal convolutions over the frames of a clip (rnn_cell `tcn`: the dilated residual layer of MS-TCN, in Keras terms
Conv1D(H, k, dilation_rate=d, padding="same" | "causal", activation="relu") -> Conv1D(H, 1) -> residual add, behind a 1x1 embedding)
in plain fp64 numpy for the tests: the contract of vl_tconv_cols_fwd / _bwd as loops, an fp32 restatement of the backward's sum in
ascending tap order for the bit-for-bit comparison, the whole layer with its parameter gradients, and an LRCN train step composed from
the oracle's tower and head and the fusions of tests/gru_ref.py / attn_pool_ref.py / netvlad_ref.py.  Nothing here imports the
package: the kernels and engines are checked AGAINST these; tests/test_tcn.py proves the layer equal to torch autograd in fp64.

Rows are clip-major, r = b T + t.  Clip b has L = min(max(lens[b], 0), T) live steps (None = T).  Tap j of `taps` reads at offset
(j - (taps - 1) // 2) dilation in the centred form and (j - (taps - 1)) dilation in the causal one."""
import collections
import functools
import math

import numpy as np

from tests import lstm_plan as LP

F64 = np.float64

# (batch, T, C, taps, dilation, causal): one step; C not a multiple of 4 ... ; C = 250; the workload's shape at layer 2; dilation >= T;
# five taps with C = 130; nine causal taps with C odd; even taps, causal; one tap: the copy; the width limit
CASES = [(1, 1, 8, 3, 1, 0), (3, 2, 24, 3, 1, 0), (2, 21, 250, 3, 2, 0), (5, 16, 256, 3, 4, 0), (2, 16, 256, 3, 16, 0), (3, 5, 130, 5, 1, 0),
         (2, 9, 7, 9, 1, 1), (4, 7, 96, 4, 2, 1), (2, 6, 3, 1, 1, 0), (2, 64, 1024, 3, 32, 0)]


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


def offsets(taps, dilation, causal):
    j0 = taps - 1 if causal else (taps - 1) // 2
    return [(j - j0) * dilation for j in range(taps)]


# ---- the two launches: the loops of the contract ----------------------------------------------------------------------------------------
def cols_fwd(x, lens, batch, T, C, taps, dilation, causal):
    """cols[b T + t][j C + c] = x[b T + t + off_j][c] where t < L_b and 0 <= t + off_j < L_b, +0.0 elsewhere; the dtype of x.  A dead row
    of x is never read (it may hold NaN)."""
    x = np.asarray(x).reshape(batch, T, C)
    cols = np.zeros((batch, T, taps, C), x.dtype)
    L = live_lens(lens, batch, T)
    for b in range(batch):
        for j, off in enumerate(offsets(taps, dilation, causal)):
            for t in range(int(L[b])):
                if 0 <= t + off < L[b]:
                    cols[b, t, j] = x[b, t + off]
    return cols.reshape(batch * T, taps * C)


def cols_bwd(dcols, dres, lens, batch, T, C, taps, dilation, causal, dtype=F64):
    """dx[b T + t][c] = dres[b T + t][c] + sum over j ASCENDING with 0 <= t - off_j < L_b of dcols[b T + t - off_j][j C + c] for t < L_b,
    +0.0 in the dead rows.  The sum starts from the dres term (from +0.0 when dres is None) and adds in `dtype`: float64 is the
    reference, float32 the restatement of the launch's own arithmetic, equal to it bit for bit."""
    dcols = np.asarray(dcols).astype(dtype).reshape(batch, T, taps, C)
    dx = np.zeros((batch, T, C), dtype)
    res = None if dres is None else np.asarray(dres).astype(dtype).reshape(batch, T, C)
    L = live_lens(lens, batch, T)
    offs = offsets(taps, dilation, causal)
    for b in range(batch):
        for t in range(int(L[b])):
            acc = np.zeros(C, dtype) if res is None else res[b, t].copy()
            for j, off in enumerate(offs):
                if 0 <= t - off < L[b]:
                    acc = (acc + dcols[b, t - off, j]).astype(dtype)
            dx[b, t] = acc
    return dx.reshape(batch * T, C)


Inputs = collections.namedtuple("Inputs", "x dcols dres")


@functools.lru_cache(maxsize=None)
def inputs(case):
    """x [B T][C], dcols [B T][taps C], dres [B T][C] ~ N(0, 1), fp32."""
    batch, T, C, taps, dilation, causal = case
    r = np.random.default_rng(list(case))
    f = lambda *shape: r.standard_normal(shape).astype(np.float32)
    return Inputs(*LP.frozen(f(batch * T, C), f(batch * T, taps * C), f(batch * T, C)))


Ref = collections.namedtuple("Ref", "inp lens cols dx dx32 dx_nores dx32_nores")


@functools.lru_cache(maxsize=None)
def reference(case, lens=False):
    """Inputs, cols (fp32, exact), dx in fp64 and in the fp32 ascending-order restatement, with and without dres.  lens:
    lstm_plan.lengths (a 0, a T, a -3, a T + 5)."""
    batch, T, C, taps, dilation, causal = case
    inp = inputs(case)
    L = LP.lengths(batch, T) if lens else None
    geo = (L, batch, T, C, taps, dilation, causal)
    return Ref(inp, L, cols_fwd(inp.x, *geo), cols_bwd(inp.dcols, inp.dres, *geo), cols_bwd(inp.dcols, inp.dres, *geo, dtype=np.float32),
               cols_bwd(inp.dcols, None, *geo), cols_bwd(inp.dcols, None, *geo, dtype=np.float32))


# ---- the layer: x + relu(conv_{k, d}(x) + b1) W2 + b2, every gradient ------------------------------------------------------------------
VARS = ("conv_kernel", "conv_bias", "out_kernel", "out_bias")
RELU_BAND = 1e-4                  # no ReLU pre-activation may lie within this fraction of its layer's rms from zero (model_train_step)


def var_name(layer, var, scope=""):
    """layer None: the embedding (kernel | bias)."""
    return "%stemporal_conv/%s/%s" % (scope, "embed" if layer is None else "layer_%d" % layer, var)


def param_names(layers, scope=""):
    """The stack's variables in flat-buffer order: the embedding, then the layers ascending."""
    return [var_name(None, v, scope) for v in ("kernel", "bias")] + [var_name(l, v, scope) for l in range(layers) for v in VARS]


def param_shapes(layers, d, H, k):
    return [(d, H), (H,)] + [(k, H, H), (H,), (H, H), (H,)] * layers


def dilations(mode, layers):
    return [2 ** l if mode == "exponential" else 1 for l in range(layers)]


LayerCache = collections.namedtuple("LayerCache", "cols z u W1 W2 geo")


def layer_forward(x, W1, b1, W2, b2, T, dilation, causal, lens=None):
    """x [B T][H] -> y [B T][H] (a dead row is zeros HERE: nothing downstream may read it), cache.  W1 (k, H, H): tap, in, out."""
    x = np.asarray(x, F64)
    k, H = W1.shape[0], W1.shape[1]
    batch = x.shape[0] // T
    m = live_mask(lens, batch, T).reshape(-1, 1)
    geo = (lens, batch, T, H, k, dilation, causal)
    cols = cols_fwd(np.where(m, x, 0.0), *geo)
    W1f, W2 = np.asarray(W1, F64).reshape(k * H, H), np.asarray(W2, F64)
    u = cols @ W1f + np.asarray(b1, F64)
    z = np.maximum(u, 0.0)
    y = np.where(m, x + z @ W2 + np.asarray(b2, F64), 0.0)
    return y, LayerCache(cols, z, u, W1f, W2, geo)


def layer_backward(dy, cache):
    """dy [B T][H] (dead rows ignored) -> dx (dead rows 0), [dW1 (k, H, H), db1, dW2, db2]."""
    cols, z, u, W1f, W2, geo = cache
    lens, batch, T, H, k = geo[:5]
    dy = np.where(live_mask(lens, batch, T).reshape(-1, 1), np.asarray(dy, F64), 0.0)
    dz = (dy @ W2.T) * (u > 0)
    grads = [(cols.T @ dz).reshape(k, H, H), dz.sum(axis=0), z.T @ dy, dy.sum(axis=0)]
    return cols_bwd(dz @ W1f.T, dy, *geo), grads


def stack_forward(x, params, T, layers, mode="exponential", causal=False, lens=None, scope=""):
    """The embedding and the layers on x [B T][d] -> the stack's output, caches (caches[0] is the embedding's zeroed input)."""
    x = np.asarray(x, F64)
    m = live_mask(lens, x.shape[0] // T, T).reshape(-1, 1)
    x = np.where(m, x, 0.0)
    We = np.asarray(params[var_name(None, "kernel", scope)], F64)
    h = np.where(m, x @ We + np.asarray(params[var_name(None, "bias", scope)], F64), 0.0)
    caches = [(x, We)]
    for l, dil in enumerate(dilations(mode, layers)):
        h, c = layer_forward(h, *(params[var_name(l, v, scope)] for v in VARS), T, dil, causal, lens)
        caches.append(c)
    return h, caches


def stack_backward(dout, caches, scope=""):
    """-> dx of the stack's input, {name: gradient}."""
    grads = {}
    for l in reversed(range(len(caches) - 1)):
        dout, g = layer_backward(dout, caches[l + 1])
        grads.update(zip((var_name(l, v, scope) for v in VARS), g))
    x, We = caches[0]
    grads[var_name(None, "kernel", scope)] = x.T @ dout
    grads[var_name(None, "bias", scope)] = dout.sum(axis=0)
    return dout @ We.T, grads


def relu_margin(caches):
    """The smallest |pre-activation| / rms(pre-activations of its layer) over the live rows of every layer."""
    worst = np.inf
    for c in caches[1:]:
        lens, batch, T = c.geo[:3]
        u = c.u[live_mask(lens, batch, T).reshape(-1)]
        if u.size:
            worst = min(worst, float(np.abs(u).min() / np.sqrt(np.mean(np.square(u)))))
    return worst


def init_stack(rng, p, d, H, layers, k, scope=""):
    """The stack's variables into p: kernels glorot-uniform (conv_kernel with Keras' Conv1D fans k H / k H), biases small and NOT zero,
    so that a gradient landing on the wrong variable shows."""
    for n, shp in zip(param_names(layers, scope), param_shapes(layers, d, H, k)):
        if len(shp) == 1:
            p[n] = (0.1 * rng.standard_normal(shp)).astype(np.float32)
        else:
            fan_in, fan_out = (shp[0] * shp[1], shp[0] * shp[2]) if len(shp) == 3 else shp
            lim = math.sqrt(6.0 / (fan_in + fan_out))
            p[n] = rng.uniform(-lim, lim, shp).astype(np.float32)
    return p


# ---- the LRCN model with the convolution stack (oracle.alexnet_forward, the stack above, a fusion, the head) ---------------------------
def init_params(rng, num_classes, final_layer, H, layers, image_shape, k, fusion="avg", attn_dim=None, vlad_k=None):
    """The oracle's well-scaled AlexNet parameters plus the stack's, the head and, for fusion attn / vlad, the pooling's variables."""
    from oracle import lrcn_oracle as O
    p = O.init_params(rng, num_classes, final_layer, H, layers, image_shape, classifier="none", well_scaled=True)
    d = {"fc6": 4096, "fc7": 4096}.get(final_layer, num_classes)
    init_stack(rng, p, d, H, layers, k)
    HW = (vlad_k if fusion == "vlad" else 1) * H
    if HW != num_classes:
        p["output_fc_w"] = O.truncated_normal(rng, (HW, num_classes), math.sqrt(2.0 / HW))
        p["output_fc_b"] = np.full(num_classes, 0.1, np.float32)
    if fusion == "attn":
        from tests import attn_pool_ref
        A = attn_dim or H
        kn, bn, cn = attn_pool_ref.param_names()
        lim = math.sqrt(6.0 / (H + A))
        p[kn] = rng.uniform(-lim, lim, (H, A)).astype(np.float32)
        p[bn] = (0.1 * rng.standard_normal(A)).astype(np.float32)
        lim = math.sqrt(6.0 / (A + 1))
        p[cn] = rng.uniform(-lim, lim, (A, 1)).astype(np.float32)
    if fusion == "vlad":
        from tests import netvlad_ref
        kn, bn, cn = netvlad_ref.param_names()
        lim = math.sqrt(6.0 / (H + vlad_k))
        p[kn] = rng.uniform(-lim, lim, (H, vlad_k)).astype(np.float32)
        p[bn] = (0.1 * rng.standard_normal(vlad_k)).astype(np.float32)
        p[cn] = rng.uniform(-lim, lim, (vlad_k, H)).astype(np.float32)
    return p


def tame_embedding(p, frames, final_layer):
    """Divides the embedding kernel by the rms of the tower's features of `frames` (in place; -> the rms).  Behind mean-subtracted
    pixels the features are of the order of 50; with an embedding of order 1 the stack's activations are of order 1, as behind a
    trained tower, and the biases (0.1) matter."""
    from oracle import lrcn_oracle as O
    feat, _ = O.alexnet_forward(p, frames, final_layer, F64, True)
    rms = float(np.sqrt(np.mean(np.square(feat))))
    name = var_name(None, "kernel")
    p[name] = (p[name] / rms).astype(np.float32)
    return rms


def head_step(p, out, onehot, T, H, fusion, lens=None, scope="", softmax_xent=None, check_band=True):
    """From the stack's output to the loss and back: -> (logits, loss, dout, {name: gradient}).  softmax_xent(logits, onehot) ->
    (loss, dlogits)."""
    from tests import attn_pool_ref, gru_ref, netvlad_ref
    g = {}
    if fusion == "attn":
        kn, bn, cn = attn_pool_ref.param_names(scope)
        fused, pc = attn_pool_ref.pool_layer_forward(out, p[kn], p[bn], p[cn], T, lens)
    elif fusion == "vlad":
        kn, bn, cn = netvlad_ref.param_names(scope)
        fused, pc = netvlad_ref.pool_layer_forward(out, p[kn], p[bn], p[cn], T, lens, check_band)
    else:
        fused = gru_ref.fuse(out, T, H, fusion, lens)
    wn, bnm = scope + "output_fc_w", scope + "output_fc_b"
    logits = fused @ np.asarray(p[wn], F64) + np.asarray(p[bnm], F64) if wn in p else fused
    loss, d = softmax_xent(logits, onehot)
    if wn in p:
        g[wn], g[bnm] = fused.T @ d, d.sum(0)
        d = d @ np.asarray(p[wn], F64).T
    if fusion == "attn":
        dout, g[kn], g[bn], g[cn] = attn_pool_ref.pool_layer_backward(d, pc)
    elif fusion == "vlad":
        dout, g[kn], g[bn], g[cn] = netvlad_ref.pool_layer_backward(d, pc)
    else:
        dout = gru_ref.fuse_backward(d, T, H, fusion, lens)
    return logits, loss, dout, g


def model_train_step(p, frames, onehot, fpc, lr, clip_norm, final_layer, H, layers, fusion, mode="exponential", causal=False):
    """One clipped SGD step in fp64 -> (new_params, loss, global_norm, logits, grads).  Asserts that no ReLU pre-activation of the
    stack lies within RELU_BAND of its layer's rms from zero: a flipped ReLU is then not what a failure against this means."""
    from oracle import lrcn_oracle as O
    feat, ccache = O.alexnet_forward(p, frames, final_layer, F64, True)
    out, caches = stack_forward(feat, p, fpc, layers, mode, causal)
    margin = relu_margin(caches)
    assert margin > RELU_BAND, "a ReLU pre-activation lies %.3g of its layer's rms from zero: pick another seed" % margin
    logits, loss, dout, g = head_step(p, out, onehot, fpc, H, fusion, softmax_xent=lambda lg, oh: O.softmax_xent_mean(lg, oh, F64))
    dfeat, lg = stack_backward(dout, caches)
    g.update(lg)
    g.update(O.alexnet_backward(p, ccache, dfeat, final_layer, F64))
    clipped, gn = O.clip_by_global_norm(g, clip_norm)
    new = {k: (np.asarray(v, F64) - lr * clipped[k]) if k in clipped else np.asarray(v, F64) for k, v in p.items()}
    return new, float(loss), float(gn), logits, g
