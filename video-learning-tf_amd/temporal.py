"""The temporal models and poolings over time of the recurrent classifier, for both engines.

What describes a model and belongs to neither engine lives here: variable names and specs, the checks of the YAML keys, the device
buffers, and a forward / backward function pair per model.  LRCNEngine (engine.py) and PipeNode (graph.py) call the same pairs and
differ only in what they pass: the variable scope, the length keyword lk, the recurrence keywords rk and where a
parameter gradient runs (param_grads)."""
import copy

import numpy as np

from . import ops
from ._ffi import VltfError

FORGET_BIAS = 1.0        # BasicLSTMCell default (lstm.py:17)


BLSTM_MAX_HIDDEN = 512      # the bidirectional launch exists in the cluster form only (vltf.h: vl_lstm_seq_bi_fwd)


def blstm_names(layer, scope=""):
    """TF's variable names of one bidirectional layer (stack_bidirectional_dynamic_rnn's scopes), in flat-buffer order: forward kernel
    and bias, backward kernel and bias.  Kernels are (d + H, 4H) with d the encode width for layer 0 and 2H above it."""
    return [scope + "bidirectional_rnn/%s/multi_rnn_cell/cell_%d/basic_lstm_cell/%s" % (d, layer, v) for d in ("fw", "bw") for v in ("kernel", "bias")]


def check_blstm(hidden, what="lstm_bidirectional"):
    """Refuses a bidirectional LSTM whose hidden size the one-launch form cannot take."""
    if not 1 <= int(hidden) <= BLSTM_MAX_HIDDEN:
        raise VltfError("%s: the bidirectional recurrence runs both directions in one cluster launch and needs a hidden size <= %d, got %d"
                        % (what, BLSTM_MAX_HIDDEN, hidden))


RNN_CELLS = ("lstm", "gru", "mhsa")
TEMPORAL_CELLS = RNN_CELLS + ("tcn",)   # what check_rnn_cell admits: the recurrences, self-attention and the temporal convolution (tcn_specs)
GRU_MAX_HIDDEN = ops.GRU_MAX_HIDDEN     # the GRU recurrence exists in the cluster form only (vltf.h: vl_gru_seq_fwd)


def gru_names(layer, scope=""):
    """The variable names of one GRU layer (Keras GRU(reset_after=True) under multi_rnn_cell's scopes), in flat-buffer order: kernel
    (d, 3H), recurrent_kernel (H, 3H), bias (3H,), recurrent_bias (3H,); gate blocks z | r | n.  The two biases are Keras' (2, 3H) bias
    split into its rows ON PURPOSE: decay_ranges, LARS and LAMB treat rank >= 2 as a weight, and a rank-2 bias would be decayed and
    trust-scaled."""
    return [scope + "rnn/multi_rnn_cell/cell_%d/gru_cell/%s" % (layer, v) for v in ("kernel", "recurrent_kernel", "bias", "recurrent_bias")]


def gru_specs(layer, d, H, scope=""):
    """[(name, shape)] of gru_names(layer) for an input of width d."""
    return list(zip(gru_names(layer, scope), ((d, 3 * H), (H, 3 * H), (3 * H,), (3 * H,))))


def check_rnn_cell(cell, classifier="lstm", hidden=1, bidirectional=False, state_input=False, what="rnn_cell"):
    """Refuses what the GRU classifier is not built for; -> the cell.  `classifier`: "lstm" where the pipeline has the recurrent classifier."""
    if cell not in TEMPORAL_CELLS:
        raise VltfError("%s must be lstm or gru (or mhsa, the self-attention layer), got [%s] (tcn, the dilated temporal convolution, "
                        "is the fourth)" % (what, cell))
    if cell == "tcn":
        if classifier != "lstm":
            raise VltfError("%s: tcn is the temporal layer of classifier lstm, but the classifier is [%s]" % (what, classifier))
        if bidirectional:
            raise VltfError("%s: tcn with lstm_bidirectional is not built (centred taps read both directions already; the "
                            "bidirectional launch runs LSTM cells)" % what)
        if state_input:
            raise VltfError("%s: tcn takes no state input: the reference hands an LSTM ONE vector as c = h, and a temporal "
                            "convolution has no state" % what)
    if cell == "mhsa":
        if classifier != "lstm":
            raise VltfError("%s: mhsa is the temporal layer of classifier lstm, but the classifier is [%s]" % (what, classifier))
        if bidirectional:
            raise VltfError("%s: mhsa with lstm_bidirectional is not built (self-attention reads both directions already; the "
                            "bidirectional launch runs LSTM cells)" % what)
        if state_input:
            raise VltfError("%s: mhsa takes no state input: the reference hands an LSTM ONE vector as c = h, and a self-attention layer "
                            "has no state" % what)
    if cell == "gru":
        if classifier != "lstm":
            raise VltfError("%s: gru is the recurrent cell of classifier lstm, but the classifier is [%s]" % (what, classifier))
        if bidirectional:
            raise VltfError("%s: gru with lstm_bidirectional is not built (the bidirectional launch runs LSTM cells)" % what)
        if state_input:
            raise VltfError("%s: gru takes no state input: the reference hands an LSTM ONE vector as c = h, and a GRU has no cell state" % what)
        if not 1 <= int(hidden) <= GRU_MAX_HIDDEN:
            raise VltfError("%s: the GRU recurrence runs in the cluster form only and needs a hidden size <= %d, got %d"
                            % (what, GRU_MAX_HIDDEN, hidden))
    return cell


# ---- rnn_cell tcn: a stack of dilated residual 1-D convolutions over the frames of a clip ------------------------------
TCN_DILATIONS = ("exponential", "none")
TCN_MAX_LAYERS = 17                     # exponential: layer l dilates by 2^l, and the launches take a dilation <= 65536 = 2^16
TCN_LAYER_VARS = ("conv_kernel", "conv_bias", "out_kernel", "out_bias")


def tcn_var(scope, layer, var):
    """The name of a variable of the convolution stack: layer None = the embedding (var kernel | bias) in front of the layers."""
    return "%stemporal_conv/%s/%s" % (scope, "embed" if layer is None else "layer_%d" % layer, var)


def tcn_specs(layers, d, H, k, scope="", backward=False):
    """[(name, shape)] of the convolution stack in flat-buffer order: the embedding kernel (d, H) and bias (H,), then the layers
    ascending with conv_kernel (k, H, H), conv_bias (H,), out_kernel (H, H), out_bias (H,).  conv_kernel is rank 3 (Keras' Conv1D
    layout: tap, in, out) and its flat form is the (k H, H) operand of the product; like every variable of rank >= 2 it is a weight for
    decay_ranges, LARS and LAMB, and the biases are exempt.  backward (GraphEngine, whose head_specs list the layers descending): the
    layers descending, then the embedding."""
    shapes = dict(conv_kernel=(k, H, H), conv_bias=(H,), out_kernel=(H, H), out_bias=(H,))
    groups = [[(tcn_var(scope, None, "kernel"), (d, H)), (tcn_var(scope, None, "bias"), (H,))]]
    for l in range(layers):
        groups.append([(tcn_var(scope, l, v), shapes[v]) for v in TCN_LAYER_VARS])
    return [s for grp in (reversed(groups) if backward else groups) for s in grp]


def tcn_dilations(mode, layers):
    """The dilation of every layer: 2^l (exponential) or 1 (none)."""
    return tuple(1 << l if mode == "exponential" else 1 for l in range(int(layers)))


def check_tcn(cell, hidden=1, layers=1, tcn_kernel=None, tcn_dilation=None, tcn_causal=None, fusion="avg", what="rnn_cell"):
    """-> (k, dilation mode, causal) of rnn_cell tcn, or None for every other cell.  Refused by name, before anything is allocated:
    tcn_kernel / tcn_dilation / tcn_causal without tcn; with it, fusion state, a width above the launches' (vltf.h:
    vl_tconv_cols_fwd), a kernel outside 1..9 or even without tcn_causal, a dilation rule that is neither, more than 17 layers under
    the exponential rule."""
    given = lambda v: not (v is None or (isinstance(v, str) and v == "None"))
    if cell != "tcn":
        for k, v in (("tcn_kernel", tcn_kernel), ("tcn_dilation", tcn_dilation), ("tcn_causal", tcn_causal)):
            if given(v):
                raise VltfError("%s is a key of rnn_cell tcn, but the cell is [%s]" % (k, cell))
        return None
    H, L = int(hidden), int(layers)
    if fusion == "state":
        raise VltfError("%s: tcn with fusion state is not built: a temporal convolution has no final state (use last)" % what)
    if not 1 <= H <= ops.TCONV_MAX_WIDTH:
        raise VltfError("%s: tcn needs a width H <= %d, got %d" % (what, ops.TCONV_MAX_WIDTH, H))
    causal = tcn_causal if given(tcn_causal) else False
    if not isinstance(causal, (bool, np.bool_)):
        raise VltfError("tcn_causal must be True or False, got [%s]" % (tcn_causal,))
    causal = bool(causal)
    k = tcn_kernel if given(tcn_kernel) else 3
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= ops.TCONV_MAX_TAPS:
        raise VltfError("tcn_kernel must be an integer in 1..%d, got [%s]" % (ops.TCONV_MAX_TAPS, k))
    if int(k) % 2 == 0 and not causal:
        raise VltfError("tcn_kernel must be odd unless tcn_causal (a centred kernel has a middle tap), got [%s]" % (k,))
    mode = tcn_dilation if given(tcn_dilation) else "exponential"
    if mode not in TCN_DILATIONS:
        raise VltfError("tcn_dilation must be exponential or none, got [%s]" % (mode,))
    if mode == "exponential" and L > TCN_MAX_LAYERS:
        raise VltfError("%s: tcn with tcn_dilation exponential needs at most %d layers (layer l dilates by 2^l <= %d), got %d"
                        % (what, TCN_MAX_LAYERS, ops.TCONV_MAX_DILATION, L))
    return int(k), mode, causal


def tcn_buffers(buf, rows, H, k, layers, training):
    """-> E = dict(x0, layers=[S ...]): the embedding's output x0; per layer the taps cols [rows, k H], z = relu(cols W1 + b1), m = z W2
    + b2 and hseq = the layer's input + m (the name the other layer kinds give a layer's output; the last one is what the fusions
    read).  cols and z of every layer are kept for the backward.  Training: dx0 in front; per layer dout (the gradient of hseq), dz and
    dcols -- every layer has its own, because the parameter gradients read them from the second stream while the chain goes on."""
    E = dict(x0=buf(rows, H), layers=[])
    if training:
        E["dx0"] = buf(rows, H)
    for _ in range(layers):
        S = dict(cols=buf(rows, k * H), z=buf(rows, H), m=buf(rows, H), hseq=buf(rows, H))
        if training:
            S.update(dout=buf(rows, H), dz=buf(rows, H), dcols=buf(rows, k * H))
        E["layers"].append(S)
    return E


def tcn_forward(E, P, scope, xin, rows, b, T, d, H, tc, ws, lk):
    """The convolution stack on xin [rows, d] -> the last layer's output.  The embedding takes the workspace (it follows conv_math, as
    the encoder block's embedding); a layer's two products do not (fp32 always, as the self-attention output projection).  Per layer:
    ONE launch moves the taps into cols, the convolution is cols W1 with bias and ReLU in the product, then z W2 + b2 and the residual
    add.  tc: (k, dilations, causal).  lk: {} or {seq_len: lengths} -- the taps launch never reads a dead row and zeroes the dead rows
    of cols, so a dead row of z, m and hseq holds a finite value (a function of the biases) that nothing reads.  No launch takes a
    host-varying argument: a captured step replays them as they are."""
    v = lambda l, name: P[tcn_var(scope, l, name)]
    k, dils, causal = tc
    ops.gemm(xin, v(None, "kernel"), E["x0"], rows, H, d, bias=v(None, "bias"), ws=ws)
    x = E["x0"]
    for l, S in enumerate(E["layers"]):
        ops.tconv_cols_fwd(x, S["cols"], b, T, H, k, dils[l], causal, **lk)
        ops.gemm(S["cols"], v(l, "conv_kernel"), S["z"], rows, H, k * H, bias=v(l, "conv_bias"), relu=True)
        ops.gemm(S["z"], v(l, "out_kernel"), S["m"], rows, H, H, bias=v(l, "out_bias"))
        ops.eltwise2(x, S["m"], S["hseq"], "add", rows * H)
        x = S["hseq"]
    return x


def tcn_backward(E, P, G, scope, rows, b, T, H, tc, lk, param_grads):
    """From layers[-1]["dout"] (the gradient of the stack's output) to E["dx0"] (the gradient of the embedding's output) and every
    gradient of the stack but the embedding's, which the caller forms as it forms its first layer's.  Per layer, with dy = dout:
    dz = relu_grad(dy W2^T, z), dcols = dz W1^T, and ONE launch gathers dcols back over the taps and adds dy, the gradient of the
    residual path, so it finishes the layer's input gradient.  Dead rows of dy are zeros (the fusions write them) and the launch keeps
    them zero down the stack.  param_grads(launch): as encoder_backward's."""
    v = lambda l, name: P[tcn_var(scope, l, name)]
    g = lambda l, name: G[tcn_var(scope, l, name)]
    k, dils, causal = tc
    layers = E["layers"]
    for l in reversed(range(len(layers))):
        S = layers[l]
        dy = S["dout"]
        ops.gemm(dy, v(l, "out_kernel"), S["dz"], rows, H, H, transb=True)

        def out_grads(ws_, sws, S=S, l=l, dy=dy):
            ops.gemm(S["z"], dy, g(l, "out_kernel"), H, H, rows, transa=True)
            ops.colsum(dy, g(l, "out_bias"), sws, rows, H)
        param_grads(out_grads)
        ops.relu_grad(S["dz"], S["z"], rows * H)
        ops.gemm(S["dz"], v(l, "conv_kernel"), S["dcols"], rows, k * H, H, transb=True)

        def conv_grads(ws_, sws, S=S, l=l):
            ops.gemm(S["cols"], S["dz"], g(l, "conv_kernel"), k * H, H, rows, transa=True)
            ops.colsum(S["dz"], g(l, "conv_bias"), sws, rows, H)
        param_grads(conv_grads)
        ops.tconv_cols_bwd(S["dcols"], dy, layers[l - 1]["dout"] if l else E["dx0"], b, T, H, k, dils[l], causal, **lk)
    return E["dx0"]


def embed_grads(G, var, scope, x, dx0, rows, d, H, param_grads):
    """The parameter gradients of the embedding in front of the encoder blocks (var = encoder_var) or of the convolution layers
    (var = tcn_var): x^T dx0 and the column sums of dx0, the gradient tcn_backward / encoder_backward returned."""
    def launch(ws, sws):
        ops.gemm(x, dx0, G[var(scope, None, "kernel")], d, H, rows, transa=True, ws=ws)
        ops.colsum(dx0, G[var(scope, None, "bias")], sws, rows, H)
    param_grads(launch)


SA_POSITIONS = ("relative", "none")


def mhsa_names(layer, scope="", positions="relative"):
    """The variable names of one self-attention layer, in flat-buffer order: qkv_kernel (d, 3H), qkv_bias (3H,), out_kernel (H, H),
    out_bias (H,) and, with relative positions, position_bias (heads, 2T - 1) -- rank 2 ON PURPOSE, as attention_pool/context is: it is
    a weight, and decay_ranges, LARS and LAMB treat rank >= 2 as one; the two biases are exempt as every bias is."""
    vs = ("qkv_kernel", "qkv_bias", "out_kernel", "out_bias") + (("position_bias",) if positions == "relative" else ())
    return [scope + "self_attention/layer_%d/%s" % (layer, v) for v in vs]


def mhsa_specs(layer, d, H, heads, T, scope="", positions="relative"):
    """[(name, shape)] of mhsa_names(layer) for an input of width d, `heads` heads and T steps."""
    return list(zip(mhsa_names(layer, scope, positions), ((d, 3 * H), (3 * H,), (H, H), (H,), (heads, 2 * T - 1))))


SA_BLOCKS = ("plain", "encoder")
SA_FFN_MIN, SA_FFN_MAX = 8, 4096


def check_sa_rate(key, rate):
    """A dropout rate of the self-attention model (sa_attn_dropout, sa_dropout, sa_drop_path) as a float in [0, 1); None read as 0
    (off).  Refused by the key's name: bools, strings, NaN, values outside [0, 1)."""
    if rate is None or (isinstance(rate, str) and rate == "None"):
        return 0.0
    if isinstance(rate, (bool, str)) or not isinstance(rate, (int, float, np.integer, np.floating)) or not 0.0 <= float(rate) < 1.0:
        raise VltfError("%s must be a rate in [0, 1), got [%s]" % (key, rate))
    return float(rate)


def check_sa_block(cell, hidden=1, sa_block=None, sa_ffn_dim=None, sa_dropout=None, sa_drop_path=None):
    """-> the feed-forward width F of sa_block encoder (sa_ffn_dim, default 4 H), or None for sa_block plain (the default: the bare
    attention layer of mhsa_names) and for every other cell.  Refused by name: a key without rnn_cell mhsa; sa_ffn_dim, sa_dropout or
    sa_drop_path without sa_block encoder; a block that is neither; F not an integer in 8..4096; a rate check_sa_rate refuses."""
    given = lambda v: not (v is None or (isinstance(v, str) and v == "None"))
    if cell != "mhsa":
        for k, v in (("sa_block", sa_block), ("sa_ffn_dim", sa_ffn_dim), ("sa_dropout", sa_dropout), ("sa_drop_path", sa_drop_path)):
            if given(v):
                raise VltfError("%s is a key of rnn_cell mhsa, but the cell is [%s]" % (k, cell))
        return None
    block = sa_block if given(sa_block) else "plain"
    if block not in SA_BLOCKS:
        raise VltfError("sa_block must be plain or encoder, got [%s]" % (block,))
    for k, v in (("sa_dropout", sa_dropout), ("sa_drop_path", sa_drop_path)):
        check_sa_rate(k, v)
        if block == "plain" and given(v):
            raise VltfError("%s is a key of sa_block encoder, but the block is [plain]" % k)
    if block == "plain":
        if given(sa_ffn_dim):
            raise VltfError("sa_ffn_dim is a key of sa_block encoder, but the block is [plain]")
        return None
    F = sa_ffn_dim if given(sa_ffn_dim) else 4 * int(hidden)
    if isinstance(F, bool) or not isinstance(F, (int, np.integer)) or not SA_FFN_MIN <= int(F) <= SA_FFN_MAX:
        raise VltfError("sa_ffn_dim must be an integer in %d..%d, got [%s]" % (SA_FFN_MIN, SA_FFN_MAX, F))
    return int(F)


def check_mhsa(cell, hidden=1, T=1, sa_heads=None, sa_positions=None, fusion="avg", what="rnn_cell", sa_block=None, sa_ffn_dim=None,
               sa_attn_dropout=None, sa_dropout=None, sa_drop_path=None):
    """-> (heads, positions) of rnn_cell mhsa, or None for every other cell.  Refused: sa_heads / sa_positions / sa_block / sa_ffn_dim /
    sa_attn_dropout / sa_dropout / sa_drop_path without mhsa; with it, fusion state, whatever misses a limit of the launches (vltf.h:
    vl_mhsa_fwd), a rate check_sa_rate refuses and what check_sa_block refuses, before anything is allocated.  The block's
    feed-forward width is check_sa_block's answer, the rates' plan is sa_drop_of's."""
    given = lambda v: not (v is None or (isinstance(v, str) and v == "None"))
    if cell != "mhsa":
        check_sa_block(cell, hidden, sa_block, sa_ffn_dim, sa_dropout, sa_drop_path)
        for k, v in (("sa_heads", sa_heads), ("sa_positions", sa_positions), ("sa_attn_dropout", sa_attn_dropout)):
            if given(v):
                raise VltfError("%s is a key of rnn_cell mhsa, but the cell is [%s]" % (k, cell))
        return None
    check_sa_rate("sa_attn_dropout", sa_attn_dropout)
    H, T = int(hidden), int(T)
    if fusion == "state":
        raise VltfError("%s: mhsa with fusion state is not built: a self-attention layer has no final state (use last)" % what)
    if not 1 <= T <= ops.MHSA_MAX_T:
        raise VltfError("%s: mhsa needs 1 <= T <= %d steps per clip (a head's score tile lives in LDS), got %d" % (what, ops.MHSA_MAX_T, T))
    if not 1 <= H <= ops.MHSA_MAX_HIDDEN:
        raise VltfError("%s: mhsa needs a width H <= %d, got %d" % (what, ops.MHSA_MAX_HIDDEN, H))
    check_sa_block(cell, H, sa_block, sa_ffn_dim, sa_dropout, sa_drop_path)
    if not given(sa_heads):
        heads = 4 if H % 4 == 0 else 1
    elif isinstance(sa_heads, bool) or not isinstance(sa_heads, (int, np.integer)) or int(sa_heads) < 1:
        raise VltfError("sa_heads must be a positive integer, got [%s]" % (sa_heads,))
    else:
        heads = int(sa_heads)
    if H % heads:
        raise VltfError("%s: mhsa needs H %% heads == 0: sa_heads %d does not divide the width %d" % (what, heads, H))
    if not ops.MHSA_MIN_HEAD <= H // heads <= ops.MHSA_MAX_HEAD:
        raise VltfError("%s: mhsa needs a head width %d <= dh = H / heads <= %d, got %d / %d = %d"
                        % (what, ops.MHSA_MIN_HEAD, ops.MHSA_MAX_HEAD, H, heads, H // heads))
    positions = sa_positions if given(sa_positions) else "relative"
    if positions not in SA_POSITIONS:
        raise VltfError("sa_positions must be relative or none, got [%s]" % (positions,))
    return heads, positions


class SaDrop:
    """The dropouts of the self-attention model in one engine: the three rates as keeps, the node salt, and -- bound to a
    training pass by bind() -- what its launches draw with (clip0 and the seed, or the step state of a captured step).  None stands
    for "every rate is 0" wherever one is passed: then no drop launch is called and no buffer of theirs exists."""

    def __init__(self, attn, elem, path, layers, node=0):
        self.attn, self.elem, self.path, self.layers, self.node = float(attn), float(elem), float(path), int(layers), int(node)
        self.attn_keep, self.elem_keep = sa_keep(attn), sa_keep(elem)
        self.branch = self.elem > 0 or self.path > 0           # the two residual branches are dropped (sa_block encoder)
        self.kw = None

    @staticmethod
    def plan(attn, elem, path, layers, node=0):
        """-> a SaDrop, or None with every rate None / 0 (the rates as check_mhsa let them through)."""
        rates = [check_sa_rate(k, v) for k, v in (("sa_attn_dropout", attn), ("sa_dropout", elem), ("sa_drop_path", path))]
        return SaDrop(*rates, layers, node) if any(r > 0 for r in rates) else None

    def path_keep(self, layer):
        return sa_path_keep(self.path, layer, self.layers)

    def salt(self, layer, site):
        return ops.sa_drop_salt(self.node, layer, site)

    def bind(self, clip0, seed=None, state=None):
        d = copy.copy(self)
        d.kw = dict(clip0=int(clip0), seed=seed, state=state)
        return d

    def branch_kw(self, layer, branch):
        """The arguments of add_layer_norm_drop_fwd / branch_drop_grad for branch 0 (attention) | 1 (feed-forward) of `layer`."""
        return dict(keep=self.elem_keep, keep_path=self.path_keep(layer), salt_elem=self.salt(layer, ops.SA_DROP_SITES[1 + branch]),
                    salt_path=self.salt(layer, "path"), branch=branch, **self.kw)

    def weights_kw(self, layer):
        return dict(keep=self.attn_keep, salt=self.salt(layer, "weights"), **self.kw)


def sa_keep(rate):
    """The keep probability of a rate as the launches get it: the fp32 nearest to 1 - rate, formed in double."""
    return float(np.float32(1.0 - float(rate)))


def sa_path_keep(rate, layer, layers):
    """k_l = 1 - p (l + 1) / L (Huang et al. 2016, the linear rule; it drops in a one-layer model too), as the fp32 the launches get."""
    return float(np.float32(1.0 - float(rate) * (int(layer) + 1) / int(layers)))


def sa_drop_of(cfg, layers, node=None):
    """The SaDrop of a NetConfig / PipelineSpec (its sa_attn_dropout, sa_dropout, sa_drop_path), or None where all are off."""
    return SaDrop.plan(getattr(cfg, "sa_attn_dropout", None), getattr(cfg, "sa_dropout", None), getattr(cfg, "sa_drop_path", None),
                       layers, getattr(cfg, "sa_drop_salt", 0) if node is None else node)


def mhsa_buffers(buf, rows, T, H, heads, positions, training):
    """The device buffers of one self-attention layer: the projection qkv, the weights P [clips, heads, T, T], the heads' outputs ctx,
    the layer's output hseq (and, training, dout, dctx, dqkv and the per-clip partials dposp of the position bias's gradient)."""
    clips = rows // T
    S = dict(qkv=buf(rows, 3 * H), P=buf(clips * heads, T * T), ctx=buf(rows, H), hseq=buf(rows, H))
    if training:
        S.update(dout=buf(rows, H), dctx=buf(rows, H), dqkv=buf(rows, 3 * H))
        if positions == "relative":
            S["dposp"] = buf(clips, heads * (2 * T - 1))
    return S


def mhsa_forward(layers, P, scope, xin, rows, b, T, d, H, heads, positions, ws, lk, drop=None):
    """The plain self-attention layers (mhsa_buffers) on xin [rows, d] -> the last layer's output.  Per layer: the qkv projection of
    all rows as the GRU's input projection is called (with the workspace: it follows conv_math), ONE launch for every (clip, head),
    then the output projection as attention_pool's (no workspace: fp32 always).  lk: {} or {seq_len: lengths} -- the launch never reads
    a dead row of qkv and writes zeros in the dead rows of ctx, so a dead row of a layer's output is out_bias, which nothing reads; the
    caller hands the FIRST layer its input through ops.live_rows, because x^T dqkv reads every row of x.  drop: a bound SaDrop in a
    training forward with sa_attn_dropout on, else None.  Without it no launch takes a host-varying argument."""
    for l, S in enumerate(layers):
        names = mhsa_names(l, scope, positions)
        ops.gemm(xin, P[names[0]], S["qkv"], rows, 3 * H, d, bias=P[names[1]], ws=ws)
        pos = P[names[4]] if positions == "relative" else None
        if drop is not None:
            ops.mhsa_drop_fwd(S["qkv"], pos, S["P"], S["ctx"], b, T, H, heads, **drop.weights_kw(l), **lk)
        else:
            ops.mhsa_fwd(S["qkv"], pos, S["P"], S["ctx"], b, T, H, heads, **lk)
        ops.gemm(S["ctx"], P[names[2]], S["hseq"], rows, H, H, bias=P[names[3]])
        xin, d = S["hseq"], H
    return xin


def mhsa_backward(layers, P, G, scope, x0, rows, b, T, d, H, heads, positions, ws, lk, param_grads, drop=None):
    """From layers[-1]["dout"] down to the first layer's dqkv, which is returned: the caller forms the gradient of x0, the stack's
    input, from it (dqkv Wqkv^T).  Per layer: through the output projection (no workspace), ONE launch for every (clip, head), the
    parameter gradients through param_grads, and above the first layer the input gradient into the dout of the layer below."""
    for l in reversed(range(len(layers))):
        S = layers[l]
        names = mhsa_names(l, scope, positions)
        din = d if l == 0 else H
        xin = x0 if l == 0 else layers[l - 1]["hseq"]
        ops.gemm(S["dout"], P[names[2]], S["dctx"], rows, H, H, transb=True)
        if drop is not None:
            ops.mhsa_drop_bwd(S["dctx"], S["qkv"], S["P"], S["dqkv"], S.get("dposp"), b, T, H, heads, **drop.weights_kw(l), **lk)
        else:
            ops.mhsa_bwd(S["dctx"], S["qkv"], S["P"], S["dqkv"], S.get("dposp"), b, T, H, heads, **lk)

        def mhsa_grads(ws_, sws, S=S, names=names, din=din, xin=xin):
            ops.gemm(S["ctx"], S["dout"], G[names[2]], H, H, rows, transa=True)
            ops.colsum(S["dout"], G[names[3]], sws, rows, H)
            ops.gemm(xin, S["dqkv"], G[names[0]], din, 3 * H, rows, transa=True, ws=ws_)
            ops.colsum(S["dqkv"], G[names[1]], sws, rows, 3 * H)
            if "dposp" in S:                                                  # the B per-clip partials, summed in a fixed order
                ops.colsum(S["dposp"], G[names[4]], sws, b, heads * (2 * T - 1))
        param_grads(mhsa_grads)
        if l > 0:
            ops.gemm(S["dqkv"], P[names[0]], layers[l - 1]["dout"], rows, H, 3 * H, transb=True, ldb=3 * H, ws=ws)
    return layers[0]["dqkv"]


# ---- sa_block encoder: the pre-LN Transformer encoder block around the self-attention layer ----------------------------
ENC_LAYER_VARS = ("norm1_gamma", "norm1_beta", "qkv_kernel", "qkv_bias", "out_kernel", "out_bias", "position_bias", "norm2_gamma",
                  "norm2_beta", "ffn1_kernel", "ffn1_bias", "ffn2_kernel", "ffn2_bias")


def encoder_var(scope, layer, var):
    """The name of a variable of the block stack: layer None = the embedding (var kernel | bias) in front of the blocks, layer -1 = the
    final norm (gamma | beta) behind them."""
    where = "embed" if layer is None else "final_norm" if layer < 0 else "layer_%d" % layer
    return "%sself_attention/%s/%s" % (scope, where, var)


def encoder_specs(layers, d, H, F, heads, T, scope="", positions="relative", backward=False):
    """[(name, shape)] of the block stack in flat-buffer order: the embedding, the layers ascending with each layer's variables in the
    order the forward meets them (ENC_LAYER_VARS), the final norm -- the layout of mhsa_specs' list (layers ascending, forward order
    inside a layer), which the backward walks from its end to its start.  backward (GraphEngine, whose head_specs list the layers
    descending): the final norm, the layers descending, the embedding.  Gammas, betas and biases are rank 1: exempt from decay and
    trust scaling as every bias is; position_bias is rank 2 on purpose (mhsa_names)."""
    shapes = dict(norm1_gamma=(H,), norm1_beta=(H,), qkv_kernel=(H, 3 * H), qkv_bias=(3 * H,), out_kernel=(H, H), out_bias=(H,),
                  position_bias=(heads, 2 * T - 1), norm2_gamma=(H,), norm2_beta=(H,), ffn1_kernel=(H, F), ffn1_bias=(F,),
                  ffn2_kernel=(F, H), ffn2_bias=(H,))
    groups = [[(encoder_var(scope, None, "kernel"), (d, H)), (encoder_var(scope, None, "bias"), (H,))]]
    for l in range(layers):
        groups.append([(encoder_var(scope, l, v), shapes[v]) for v in ENC_LAYER_VARS if v != "position_bias" or positions == "relative"])
    groups.append([(encoder_var(scope, -1, "gamma"), (H,)), (encoder_var(scope, -1, "beta"), (H,))])
    return [s for grp in (reversed(groups) if backward else groups) for s in grp]


def encoder_buffers(buf, rows, T, H, F, heads, positions, layers, training, drop=None):
    """-> E = dict(x0, n0, st0, layers=[S ...]): the embedding's output x0 (the residual stream entering layer 0), its norm n0 with the
    stats st0; per layer qkv, P, ctx, the attention's output o, a = stream + o, n2 = LN(a) with st2, u, f = gelu(u), m, the stream xs
    leaving the layer and hseq = LN(xs) with sty -- the next layer's norm1, or behind the last layer the final norm, which is what the
    fusions read (hence the name the other layer kinds use).  Training: per layer dout (the gradient of hseq), dxs (of xs), df (du in
    place), dn2, da, dctx, dqkv, dposp and the per-clip partials gb2 / gby of the two norms' gradients; dn0, dx0, gb0 in front.  Every
    layer has its own: the parameter gradients read them from the second stream while the chain goes on.  drop (a SaDrop that drops
    the branches, training): per layer do and dm, the gradients that enter the two dropped branches (vl_branch_drop_grad)."""
    clips = rows // T
    E = dict(x0=buf(rows, H), n0=buf(rows, H), st0=buf(rows, 2), layers=[])
    if training:
        E.update(dn0=buf(rows, H), dx0=buf(rows, H), gb0=buf(clips, 2 * H))
    for _ in range(layers):
        S = dict(qkv=buf(rows, 3 * H), P=buf(clips * heads, T * T), ctx=buf(rows, H), o=buf(rows, H), a=buf(rows, H), n2=buf(rows, H),
                 st2=buf(rows, 2), u=buf(rows, F), f=buf(rows, F), m=buf(rows, H), xs=buf(rows, H), hseq=buf(rows, H), sty=buf(rows, 2))
        if training:
            S.update(dout=buf(rows, H), dxs=buf(rows, H), df=buf(rows, F), dn2=buf(rows, H), da=buf(rows, H), dctx=buf(rows, H),
                     dqkv=buf(rows, 3 * H), gb2=buf(clips, 2 * H), gby=buf(clips, 2 * H))
            if positions == "relative":
                S["dposp"] = buf(clips, heads * (2 * T - 1))
            if drop is not None and drop.branch:
                S.update(do=buf(rows, H), dm=buf(rows, H))
        E["layers"].append(S)
    return E


def encoder_forward(E, P, scope, xin, rows, b, T, d, H, F, heads, positions, ws, lk, drop=None):
    """The block stack on xin [rows, d] -> the final norm's output.  The embedding and the qkv projections take the workspace (they
    follow conv_math, as the GRU's input projection); the output projection and the two feed-forward products do not (fp32 always, as
    attention_pool's).  Every residual add is inside the norm launch that follows it.  lk: {} or {seq_len: lengths} -- no launch reads
    a dead row of what a launch wrote, and a dead row of a product's output (a bias) is read by nothing.  drop: a bound SaDrop in a
    TRAINING forward with a rate on (the drop forms of the attention and of the two add-and-norm launches), else None."""
    v = lambda l, name: P[encoder_var(scope, l, name)]
    layers = E["layers"]

    def add_norm(l, branch, x, r, sum, y, gamma, beta, stats):
        if drop is not None and drop.branch:
            ops.add_layer_norm_drop_fwd(x, r, sum, y, gamma, beta, stats, b, T, H, **drop.branch_kw(l, branch), **lk)
        else:
            ops.add_layer_norm_fwd(x, r, sum, y, gamma, beta, stats, b, T, H, **lk)

    ops.gemm(xin, v(None, "kernel"), E["x0"], rows, H, d, bias=v(None, "bias"), ws=ws)
    ops.add_layer_norm_fwd(E["x0"], None, None, E["n0"], v(0, "norm1_gamma"), v(0, "norm1_beta"), E["st0"], b, T, H, **lk)
    xs, nin = E["x0"], E["n0"]
    for l, S in enumerate(layers):
        ops.gemm(nin, v(l, "qkv_kernel"), S["qkv"], rows, 3 * H, H, bias=v(l, "qkv_bias"), ws=ws)
        pos = v(l, "position_bias") if positions == "relative" else None
        if drop is not None and drop.attn > 0:
            ops.mhsa_drop_fwd(S["qkv"], pos, S["P"], S["ctx"], b, T, H, heads, **drop.weights_kw(l), **lk)
        else:
            ops.mhsa_fwd(S["qkv"], pos, S["P"], S["ctx"], b, T, H, heads, **lk)
        ops.gemm(S["ctx"], v(l, "out_kernel"), S["o"], rows, H, H, bias=v(l, "out_bias"))
        add_norm(l, 0, xs, S["o"], S["a"], S["n2"], v(l, "norm2_gamma"), v(l, "norm2_beta"), S["st2"])
        ops.gemm(S["n2"], v(l, "ffn1_kernel"), S["u"], rows, F, H, bias=v(l, "ffn1_bias"))
        ops.gelu_fwd(S["u"], S["f"], rows * F)
        ops.gemm(S["f"], v(l, "ffn2_kernel"), S["m"], rows, H, F, bias=v(l, "ffn2_bias"))
        last = l + 1 == len(layers)
        gy, by = (v(-1, "gamma"), v(-1, "beta")) if last else (v(l + 1, "norm1_gamma"), v(l + 1, "norm1_beta"))
        add_norm(l, 1, S["a"], S["m"], S["xs"], S["hseq"], gy, by, S["sty"])
        xs, nin = S["xs"], S["hseq"]
    return nin


def encoder_backward(E, P, G, scope, xin, rows, b, T, d, H, F, heads, positions, ws, lk, param_grads, drop=None):
    """From layers[-1]["dout"] (the gradient of the final norm's output) to E["dx0"] (the gradient of the embedding's output) and every
    gradient of the stack but the embedding's, which the caller forms as it forms its first layer's.  The gradient on the residual
    stream enters each norm's backward as dres: there is no add launch.  param_grads(launch): launch(ws, small_ws) forms parameter
    gradients from buffers that are complete on the calling stream (LRCNEngine: on the second stream).  drop: the bound SaDrop the
    forward ran with, or None.  With the branches dropped, the gradient that enters a branch is the stream's gradient times the
    branch's factor (vl_branch_drop_grad: dm from dxs, do from da), and the products and parameter gradients behind it read that."""
    v = lambda l, name: P[encoder_var(scope, l, name)]
    g = lambda l, name: G[encoder_var(scope, l, name)]
    layers = E["layers"]
    branch = drop is not None and drop.branch

    def norm_grads(l, which, part, sws):                      # the per-clip partials, summed over the clips in a fixed order
        names = ("gamma", "beta") if l < 0 else (which + "_gamma", which + "_beta")
        ops.colsum(part, g(l, names[0]), sws, b, H, lda=2 * H)
        ops.colsum(part.view(-1)[H:], g(l, names[1]), sws, b, H, lda=2 * H)

    top = layers[-1]
    ops.layer_norm_bwd(top["dout"], top["xs"], v(-1, "gamma"), top["sty"], None, top["dxs"], top["gby"], b, T, H, **lk)
    param_grads(lambda ws_, sws: norm_grads(-1, None, top["gby"], sws))
    for l in reversed(range(len(layers))):
        S = layers[l]
        below = layers[l - 1] if l else None
        xs_in, nin, st_in = (below["xs"], below["hseq"], below["sty"]) if l else (E["x0"], E["n0"], E["st0"])
        dnin, dxs_in, gb_in = (below["dout"], below["dxs"], below["gby"]) if l else (E["dn0"], E["dx0"], E["gb0"])
        # the feed-forward block: dm = dxs; df = dm W2^T, du = df gelu'(u) in place, dn2 = du W1^T; norm2 with the stream's gradient
        dm = S["dm"] if branch else S["dxs"]
        if branch:
            ops.branch_drop_grad(S["dxs"], dm, b, T, H, **drop.branch_kw(l, 1), **lk)
        ops.gemm(dm, v(l, "ffn2_kernel"), S["df"], rows, F, H, transb=True)

        def ffn2_grads(ws_, sws, S=S, l=l, dm=dm):
            ops.gemm(S["f"], dm, g(l, "ffn2_kernel"), F, H, rows, transa=True)
            ops.colsum(dm, g(l, "ffn2_bias"), sws, rows, H)
        param_grads(ffn2_grads)
        ops.gelu_bwd(S["df"], S["u"], S["df"], rows * F)
        ops.gemm(S["df"], v(l, "ffn1_kernel"), S["dn2"], rows, H, F, transb=True)
        ops.layer_norm_bwd(S["dn2"], S["a"], v(l, "norm2_gamma"), S["st2"], S["dxs"], S["da"], S["gb2"], b, T, H, **lk)

        def ffn1_grads(ws_, sws, S=S, l=l):
            ops.gemm(S["n2"], S["df"], g(l, "ffn1_kernel"), H, F, rows, transa=True)
            ops.colsum(S["df"], g(l, "ffn1_bias"), sws, rows, F)
            norm_grads(l, "norm2", S["gb2"], sws)
        param_grads(ffn1_grads)
        # the attention: do = da; through the output projection, ONE launch for every (clip, head), the qkv projection; norm1
        do = S["do"] if branch else S["da"]
        if branch:
            ops.branch_drop_grad(S["da"], do, b, T, H, **drop.branch_kw(l, 0), **lk)
        ops.gemm(do, v(l, "out_kernel"), S["dctx"], rows, H, H, transb=True)
        if drop is not None and drop.attn > 0:
            ops.mhsa_drop_bwd(S["dctx"], S["qkv"], S["P"], S["dqkv"], S.get("dposp"), b, T, H, heads, **drop.weights_kw(l), **lk)
        else:
            ops.mhsa_bwd(S["dctx"], S["qkv"], S["P"], S["dqkv"], S.get("dposp"), b, T, H, heads, **lk)
        ops.gemm(S["dqkv"], v(l, "qkv_kernel"), dnin, rows, H, 3 * H, transb=True, ldb=3 * H, ws=ws)
        ops.layer_norm_bwd(dnin, xs_in, v(l, "norm1_gamma"), st_in, S["da"], dxs_in, gb_in, b, T, H, **lk)

        def attn_grads(ws_, sws, S=S, l=l, nin=nin, gb_in=gb_in, do=do):
            ops.gemm(S["ctx"], do, g(l, "out_kernel"), H, H, rows, transa=True)
            ops.colsum(do, g(l, "out_bias"), sws, rows, H)
            ops.gemm(nin, S["dqkv"], g(l, "qkv_kernel"), H, 3 * H, rows, transa=True, ws=ws_)
            ops.colsum(S["dqkv"], g(l, "qkv_bias"), sws, rows, 3 * H)
            if "dposp" in S:
                ops.colsum(S["dposp"], g(l, "position_bias"), sws, b, heads * (2 * T - 1))
            norm_grads(l, "norm1", gb_in, sws)
        param_grads(attn_grads)
    return E["dx0"]


ATTN_MAX_DIM = 1024


def attn_names(scope=""):
    """The variable names of the attention pooling of fusion `attn`, in flat-buffer order: kernel (HO, A), bias (A,), context (A, 1).
    The context is rank 2 ON PURPOSE: it is a weight, and decay_ranges, LARS and LAMB treat rank >= 2 as one; the bias is exempt as
    every bias is."""
    return [scope + "attention_pool/" + v for v in ("kernel", "bias", "context")]


def attn_specs(HO, A, scope=""):
    """[(name, shape)] of attn_names for a recurrent output of width HO and an attention width A."""
    return list(zip(attn_names(scope), ((HO, A), (A,), (A, 1))))


def check_attn(fusion, attn_dim=None, classifier="lstm", out_width=1, what="attn_dim"):
    """-> the attention width A of fusion `attn` (attn_dim, default out_width: the recurrent output width), or None for every other
    fusion.  Refused: fusion attn without the recurrent classifier, attn_dim without fusion attn, attn_dim not an integer in 1..1024."""
    if fusion == "attn" and classifier != "lstm":
        raise VltfError("lstm_params: fusion attn pools the outputs of the recurrent classifier, but the classifier is [%s]" % classifier)
    if fusion != "attn":
        if attn_dim not in (None, "None"):
            raise VltfError("%s is the width of fusion attn's scorer, but the fusion is [%s]" % (what, fusion))
        return None
    if attn_dim in (None, "None"):
        return int(out_width)
    if isinstance(attn_dim, bool) or not isinstance(attn_dim, (int, np.integer)) or not 1 <= int(attn_dim) <= ATTN_MAX_DIM:
        raise VltfError("%s must be an integer in 1..%d, got [%s]" % (what, ATTN_MAX_DIM, attn_dim))
    return int(attn_dim)


def attn_buffers(buf, clips, T, HO, A, training):
    """The device buffers of fusion attn: us (the projection u, then s = tanh(u) in place), the weights alpha (and, training, the
    per-clip partials dcp of the context gradient, du, and dproj = du W^T)."""
    S = dict(us=buf(clips * T, A), alpha=buf(clips, T))
    if training:
        S.update(dcp=buf(clips, A), du=buf(clips * T, A), dproj=buf(clips * T, HO))
    return S


def attn_forward(S, P, scope, hseq, fused, rows, b, T, HO, A, lk):
    """fusion attn on the last layer's outputs hseq [rows, HO] -> fused [b, HO].  u = hseq W + bias over all rows (a dead row of hseq
    is zero, its u is never read), then ONE launch: s = tanh(u) in place, scores, softmax, weighted sum.  The attention's dense
    products are called as the head's are, WITHOUT a workspace: fp32 whatever conv_math says (vl_gemm takes its split-bf16 branch only
    when it is handed the workspace for the operand images)."""
    Wa, ba, ca = (P[k] for k in attn_names(scope))
    ops.gemm(hseq, Wa, S["us"], rows, A, HO, bias=ba)
    ops.attn_pool_fwd(S["us"], ca, hseq, S["us"], S["alpha"], fused, b, T, HO, A, **lk)


def attn_backward(S, P, G, scope, d, hseq, dout, rows, b, T, HO, A, lk, param_grads):
    """From d, the gradient of fused, to dout, the gradient of hseq.  ONE launch: du, the direct term alpha_t dy straight into dout
    (zeros in the dead rows of both) and the per-clip partials of the context gradient; then the projected term du W^T is added."""
    names = attn_names(scope)
    ops.attn_pool_bwd(d, hseq, S["us"], S["alpha"], P[names[2]], S["du"], dout, S["dcp"], b, T, HO, A, **lk)

    def attn_grads(ws_, sws):
        ops.gemm(hseq, S["du"], G[names[0]], HO, A, rows, transa=True)
        ops.colsum(S["du"], G[names[1]], sws, rows, A)
        ops.colsum(S["dcp"], G[names[2]], sws, b, A)
    param_grads(attn_grads)
    ops.gemm(S["du"], P[names[0]], S["dproj"], rows, HO, A, transb=True)
    ops.eltwise2(dout, S["dproj"], dout, "add", rows * HO)


VLAD_MIN_K, VLAD_MAX_K, VLAD_MAX_HO, VLAD_MAX_WIDTH, VLAD_DEFAULT_K = 2, 64, 1024, 16384, 8


def vlad_names(scope=""):
    """The variable names of the NetVLAD pooling of fusion `vlad`, in flat-buffer order (the order in which the backward produces
    them): kernel (HO, K), bias (K,), centers (K, HO).  kernel and centers are rank 2: weights for decay_ranges, LARS and LAMB; the
    bias is exempt as every bias is."""
    return [scope + "netvlad/" + v for v in ("kernel", "bias", "centers")]


def vlad_specs(HO, K, scope=""):
    """[(name, shape)] of vlad_names for a recurrent output of width HO and K centres."""
    return list(zip(vlad_names(scope), ((HO, K), (K,), (K, HO))))


def check_vlad(fusion, vlad_clusters=None, classifier="lstm", out_width=1, what="vlad_clusters"):
    """-> the number of centres K of fusion `vlad` (vlad_clusters, default 8), or None for every other fusion.  The descriptor the head
    reads is K * out_width wide.  Refused: fusion vlad without the recurrent classifier, vlad_clusters without fusion vlad,
    vlad_clusters not an integer in 2..64, an output width above 1024, K * out_width above 16384 (the launches' limits, vltf.h)."""
    if fusion == "vlad" and classifier != "lstm":
        raise VltfError("lstm_params: fusion vlad pools the outputs of the recurrent classifier, but the classifier is [%s]" % classifier)
    if fusion != "vlad":
        if vlad_clusters not in (None, "None"):
            raise VltfError("%s is the number of centres of fusion vlad, but the fusion is [%s]" % (what, fusion))
        return None
    K = VLAD_DEFAULT_K if vlad_clusters in (None, "None") else vlad_clusters
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not VLAD_MIN_K <= int(K) <= VLAD_MAX_K:
        raise VltfError("%s must be an integer in %d..%d, got [%s]" % (what, VLAD_MIN_K, VLAD_MAX_K, K))
    if int(out_width) > VLAD_MAX_HO:
        raise VltfError("%s: fusion vlad takes a recurrent output of width 1..%d, got [%d]" % (what, VLAD_MAX_HO, out_width))
    if int(K) * int(out_width) > VLAD_MAX_WIDTH:
        raise VltfError("%s: the descriptor of fusion vlad is %d x %d = %d wide, above %d" %
                        (what, int(K), int(out_width), int(K) * int(out_width), VLAD_MAX_WIDTH))
    return int(K)


def vlad_buffers(buf, clips, T, HO, K, training):
    """The device buffers of fusion vlad: sa (the projection s, then the assignments a in place), the per-cluster scales r (and,
    training, the per-clip partials dcp of the centres' gradient, ds, and dproj = ds W^T)."""
    S = dict(sa=buf(clips * T, K), r=buf(clips, K))
    if training:
        S.update(dcp=buf(clips, K * HO), ds=buf(clips * T, K), dproj=buf(clips * T, HO))
    return S


def vlad_forward(S, P, scope, hseq, fused, rows, b, T, HO, K, lk):
    """fusion vlad on the last layer's outputs hseq [rows, HO] -> fused [b, K HO].  s = hseq W + beta over all rows (no workspace, as
    attn's and the head's products: fp32 whatever conv_math says), then ONE launch, which reads no dead row of hseq or s: the soft
    assignment in place, the residual sums per centre, the intra-normalisation, into K x HO columns."""
    Wv, bv, cv = (P[k] for k in vlad_names(scope))
    ops.gemm(hseq, Wv, S["sa"], rows, K, HO, bias=bv)
    ops.netvlad_fwd(S["sa"], cv, hseq, S["sa"], S["r"], fused, b, T, HO, K, **lk)


def vlad_backward(S, P, G, scope, d, hseq, fused, dout, rows, b, T, HO, K, lk, param_grads):
    """From d, the gradient of fused, to dout, the gradient of hseq.  ONE launch: ds, the direct term sum_k a_tk dV_k straight into
    dout (zeros in the dead rows of both) and the per-clip partials of the centres' gradient; then the projected term ds W^T is added."""
    names = vlad_names(scope)
    ops.netvlad_bwd(d, hseq, S["sa"], S["r"], fused, P[names[2]], S["ds"], dout, S["dcp"], b, T, HO, K, **lk)

    def vlad_grads(ws_, sws):
        ops.gemm(hseq, S["ds"], G[names[0]], HO, K, rows, transa=True)
        ops.colsum(S["ds"], G[names[1]], sws, rows, K)
        ops.colsum(S["dcp"], G[names[2]], sws, b, K * HO)
    param_grads(vlad_grads)
    ops.gemm(S["ds"], P[names[0]], S["dproj"], rows, HO, K, transb=True)
    ops.eltwise2(dout, S["dproj"], dout, "add", rows * HO)


def gru_buffers(buf, rows, H, training):
    """The device buffers of one GRU layer: projections gx, activated gates act, the candidate's recurrent term hcand, outputs hseq,
    entering outputs hprev (and, training, the gradients dgx / dgh of the two pre-activation terms and dout of the output)."""
    S = dict(gx=buf(rows, 3 * H), act=buf(rows, 3 * H), hcand=buf(rows, H), hseq=buf(rows, H), hprev=buf(rows, H))
    if training:
        S.update(dgx=buf(rows, 3 * H), dgh=buf(rows, 3 * H), dout=buf(rows, H))
    return S


def gru_forward(layers, P, scope, xin, rows, b, T, d, H, ws, rk):
    """The GRU layers (gru_buffers) on xin [rows, d] -> the last layer's output.  Per layer: the input projection of all rows
    (z | r | n), then the recurrence with its own recurrent_kernel / recurrent_bias.  rk(span) -> the keywords of a cluster-recurrence
    launch that uses `span` exchange tags: its workspace and, as the caller runs, the lengths or the step state and tag offset."""
    for l, S in enumerate(layers):
        K, U, bk, rb = (P[k] for k in gru_names(l, scope))
        ops.gemm(xin, K, S["gx"], rows, 3 * H, d, bias=bk, ws=ws)
        ops.gru_seq_fwd(S["gx"], U, S["act"], S["hcand"], S["hseq"], S["hprev"], b, T, H, rb=rb, **rk(ops.gru_seq_tag_span(b, T, H)))
        xin, d = S["hseq"], H
    return xin


def gru_backward(layers, P, G, scope, x0, rows, b, T, d, H, ws, rk, param_grads):
    """From layers[-1]["dout"] down to the first layer's gate gradient dgx, which is returned: the caller forms the gradient of x0,
    the stack's input, from it (dgx K^T; LRCNEngine fuses the tower's ReluGrad into that product)."""
    for l in reversed(range(len(layers))):
        S = layers[l]
        names = gru_names(l, scope)
        din = d if l == 0 else H
        xin = x0 if l == 0 else layers[l - 1]["hseq"]
        ops.gru_seq_bwd(S["dout"], P[names[1]], S["act"], S["hcand"], S["hprev"], S["dgx"], S["dgh"], b, T, H,
                        **rk(ops.gru_seq_tag_span(b, T, H)))

        def gru_grads(ws_, sws, S=S, names=names, din=din, xin=xin):
            ops.gemm(xin, S["dgx"], G[names[0]], din, 3 * H, rows, transa=True, ws=ws_)
            ops.gemm(S["hprev"], S["dgh"], G[names[1]], H, 3 * H, rows, transa=True, ws=ws_)
            ops.colsum(S["dgx"], G[names[2]], sws, rows, 3 * H)
            ops.colsum(S["dgh"], G[names[3]], sws, rows, 3 * H)
        param_grads(gru_grads)
        if l > 0:
            ops.gemm(S["dgx"], P[names[0]], layers[l - 1]["dout"], rows, H, 3 * H, transb=True, ldb=3 * H, ws=ws)
    return layers[0]["dgx"]


def blstm_buffers(buf, rows, H, training):
    """The device buffers of one bidirectional layer.  Per direction, as (forward, backward) pairs: projections gx, gates act, cell
    states cseq, entering outputs hprev (and dz when training); ONE [rows][2H] output hseq and ONE gradient dout of it, whose halves
    (hhalf, dhalf: views at row stride 2H) the recurrence launch writes and reads in place."""
    pair = lambda w: (buf(rows, w), buf(rows, w))
    S = dict(gx=pair(4 * H), act=pair(4 * H), cseq=pair(H), hprev=pair(H), hseq=buf(rows, 2 * H))
    S["hhalf"] = (S["hseq"][:, :H], S["hseq"][:, H:])
    if training:
        S.update(dz=pair(4 * H), dout=buf(rows, 2 * H))
        S["dhalf"] = (S["dout"][:, :H], S["dout"][:, H:])
    return S


def blstm_forward(layers, P, scope, xin, rows, b, T, d, H, ws, rk):
    """The bidirectional layers (blstm_buffers) on xin [rows, d] -> the last layer's output [rows, 2H].  Per layer: both input
    projections, then both recurrences in ONE launch, the halves of hseq written in place.  rk: as gru_forward's."""
    for l, S in enumerate(layers):
        Kf, bf, Kb, bb = (P[k] for k in blstm_names(l, scope))
        ops.gemm(xin, Kf, S["gx"][0], rows, 4 * H, d, bias=bf, ws=ws)
        ops.gemm(xin, Kb, S["gx"][1], rows, 4 * H, d, bias=bb, ws=ws)
        ops.lstm_seq_bi_fwd(S["gx"], (Kf[d:], Kb[d:]), S["act"], S["cseq"], S["hhalf"], S["hprev"], b, T, H, FORGET_BIAS, hseq_ld=2 * H,
                            **rk(ops.lstm_seq_bi_tag_span(b, T, H)))
        xin, d = S["hseq"], 2 * H
    return xin


def blstm_backward(layers, P, G, scope, x0, rows, b, T, d, H, ws, rk, param_grads, dx, dx_bw):
    """From layers[-1]["dout"] down to dx, the gradient of x0, the stack's input; dx None: nobody reads it (a frozen tower, a
    pipeline whose input takes no gradient) and the first layer's input-gradient products are not launched.  A layer's input gradient
    is the SUM of both directions' dz Kx^T: the forward direction's into the target, the backward direction's into dx_bw, one add."""
    for l in reversed(range(len(layers))):
        S = layers[l]
        names = blstm_names(l, scope)
        Kf, Kb = P[names[0]], P[names[2]]
        din = d if l == 0 else 2 * H
        xin = x0 if l == 0 else layers[l - 1]["hseq"]
        ops.lstm_seq_bi_bwd(S["dhalf"], (Kf[din:], Kb[din:]), S["act"], S["cseq"], S["dz"], b, T, H, dout_ld=2 * H,
                            **rk(ops.lstm_seq_bi_tag_span(b, T, H)))

        def blstm_grads(ws_, sws, S=S, names=names, din=din, xin=xin):
            for k in range(2):                                                    # each direction's three products and bias sum
                gK, gb = G[names[2 * k]], G[names[2 * k + 1]]
                ops.gemm(xin, S["dz"][k], gK, din, 4 * H, rows, transa=True, ws=ws_)
                ops.gemm(S["hprev"][k], S["dz"][k], gK[din:], H, 4 * H, rows, transa=True, ws=ws_)
                ops.colsum(S["dz"][k], gb, sws, rows, 4 * H)
        param_grads(blstm_grads)
        target = layers[l - 1]["dout"] if l > 0 else dx
        if target is None:
            continue
        ops.gemm(S["dz"][0], Kf, target, rows, din, 4 * H, transb=True, ldb=4 * H, ws=ws)
        ops.gemm(S["dz"][1], Kb, dx_bw, rows, din, 4 * H, transb=True, ldb=4 * H, ws=ws)
        ops.eltwise2(target, dx_bw, target, "add", rows * din)
