"""LRCNEngine: the two executor calls of the reference, on MI355X.

The reference assembles a TF graph once (models/model.py:18-155: dcnn representation ->
lstm | fc classifier -> logits; train.py:112-222: loss, clip, SGD) and then calls
  sess.run([summaries, loss, lr, global_step, optimizer], fdict)      run_task.py:44   -> train_step_*
  sess.run(model.logits, fdict)                                       run_task.py:95   -> forward_*
This class is that graph: a fixed plan of C-ABI kernel launches (vltf_amd.ops) over buffers
allocated once.  torch tensors are device memory only; no torch math runs on the data path.

Activations are NCHW; parameters keep the reference's layouts and TF variable names
(SURVEY.md section 5), stored in one flat fp32 buffer (and one flat gradient buffer) ordered
classifier -> fc -> conv5..conv1, i.e. the order backward produces gradients, so the
data-parallel all-reduce of the first (large: fc6 = 85 % of bytes) bucket overlaps the conv backward.
"""
import collections
import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import contextlib
import gc
import os
import time

import numpy as np
import torch

from . import ops
from ._ffi import MAX_DECAY_RANGES, VltfError
# the temporal models and poolings over time, shared with graph.py (re-exported: `from vltf_amd.engine import ...` keeps working)
from .temporal import (ATTN_MAX_DIM, BLSTM_MAX_HIDDEN, ENC_LAYER_VARS, FORGET_BIAS, GRU_MAX_HIDDEN, RNN_CELLS, SA_BLOCKS, SA_FFN_MAX,  # noqa: F401
                       SA_FFN_MIN, SA_POSITIONS, TCN_DILATIONS, TCN_LAYER_VARS, TCN_MAX_LAYERS, TEMPORAL_CELLS, VLAD_DEFAULT_K, VLAD_MAX_HO,
                       VLAD_MAX_K, VLAD_MAX_WIDTH, VLAD_MIN_K, SaDrop, attn_backward, attn_buffers, attn_forward, attn_names, attn_specs,
                       blstm_backward, blstm_buffers, blstm_forward, blstm_names, check_attn, check_blstm, check_mhsa, check_rnn_cell,
                       check_sa_block, check_sa_rate, check_tcn, check_vlad, embed_grads, encoder_backward, encoder_buffers, encoder_forward,
                       encoder_specs, encoder_var, gru_backward, gru_buffers, gru_forward, gru_names, gru_specs, mhsa_backward, mhsa_buffers,
                       mhsa_forward, mhsa_names, mhsa_specs, sa_drop_of, sa_keep, sa_path_keep, tcn_backward, tcn_buffers, tcn_dilations,
                       tcn_forward, tcn_specs, tcn_var, vlad_backward, vlad_buffers, vlad_forward, vlad_names, vlad_specs)

# name, kh, kw, cout, stride, groups, lrn, pool        (alexnet.py:60-211)
CONV_LAYERS = (
    ("conv1", 11, 11, 96, 4, 1, True, True),
    ("conv2", 5, 5, 256, 1, 2, True, True),
    ("conv3", 3, 3, 384, 1, 1, False, False),
    ("conv4", 3, 3, 384, 1, 2, False, False),
    ("conv5", 3, 3, 256, 1, 2, False, True),
)
FC_DIM = 4096
LRN = dict(radius=2, alpha=2e-5, beta=0.75, bias=1.0)     # alexnet.py:81-84


@dataclass
class NetConfig:
    """The subset of the `network:` / `train:` YAML keys (settings_.py:167-289) that shapes the graph."""
    image_shape: Tuple[int, int, int] = (227, 227, 3)
    num_classes: int = 101
    fpc: int = 16                               # frames per clip (from the .size file, dataset_.py:728)
    frame_encoding_layer: str = "fc6"           # alexnet.py:233-275: "fc6" | "fc7" | anything else -> fc8
    classifier: str = "lstm"                    # defs.classifier.{lstm, fc}; "none": a feature pipeline (classifier: None, model.py:110-112)
    lstm_hidden: int = 256
    lstm_layers: int = 1
    fusion: str = "avg"                         # lstm_params[2]: defs.fusion_method.{avg, last, reshape, state, attn, vlad}
    attn_dim: Optional[int] = None              # fusion attn: width A of the attention scorer (attn_specs); None = the recurrent output width
    vlad_clusters: Optional[int] = None         # fusion vlad: the number K of NetVLAD centres (vlad_specs), 2..64, K * output width <= 16384; None = 8
    lstm_bidirectional: bool = False            # every LSTM layer a forward and a backward cell, outputs concatenated (blstm_names); H <= 512
    rnn_cell: str = "lstm"                      # the recurrent cell of classifier lstm: "lstm" (BasicLSTMCell) | "gru" (reset-after, gru_names); H <= 512
                                                # | "mhsa": every layer a multi-head self-attention layer over the fpc frames (mhsa_names)
    sa_heads: Optional[int] = None              # rnn_cell mhsa: heads (divides lstm_hidden); None = 4 where 4 divides it, else 1
    sa_positions: Optional[str] = None          # rnn_cell mhsa: "relative" (None: a learned bias per head and offset) | "none"
    tcn_kernel: Optional[int] = None            # rnn_cell tcn: the taps k of every layer's dilated convolution, 1..9, odd unless tcn_causal; None = 3
    tcn_dilation: Optional[str] = None          # rnn_cell tcn: "exponential" (None: layer l dilates by 2^l, lstm_layers <= 17) | "none" (1 everywhere)
    tcn_causal: Optional[bool] = None           # rnn_cell tcn: True = a step sees itself and the past only; None / False = centred taps
    sa_block: Optional[str] = None              # rnn_cell mhsa: "plain" (None: the bare attention layer) | "encoder": the pre-LN encoder block (encoder_specs)
    sa_ffn_dim: Optional[int] = None            # sa_block encoder: the feed-forward width F, 8..4096; None = 4 lstm_hidden
    sa_attn_dropout: Optional[float] = None     # rnn_cell mhsa: dropout rate on the softmax weights of a training forward, [0, 1); None / 0 = off
    sa_dropout: Optional[float] = None          # sa_block encoder: dropout rate on the elements of the two residual branches; None / 0 = off
    sa_drop_path: Optional[float] = None        # sa_block encoder: stochastic depth, layer l of L keeps a clip's branch with 1 - p (l + 1) / L; None / 0 = off
    sa_drop_salt: int = 0                       # which mask streams the self-attention dropouts draw from (SaDrop): 0 for an LRCNEngine of its own
    frame_fusion: Optional[Tuple[str, str]] = None   # classifier fc: (early|late, avg|last) (model.py:103-106,149-151)
    dropout_keep_prob: float = 0.0              # <= 0 disables (lstm.py:52)
    optimizer: str = "sgd"                      # defs.optim.{sgd, adam}
    conv_math: str = "f32"                      # "f32" | "bf16x3" | "bf16x6" | "bf16" (ops.set_conv_math: opt-in bf16-MFMA conv products)
    step_graph: bool = False                    # train_step_u8 / forward_u8 captured once per input key and replayed (LRCNEngine docstring)
    lr_mult: Optional[float] = None             # train.lr_mult: learning-rate factor of the `modified` variables (finetune_plan); None = 1
    train_from: Optional[str] = None            # first trainable dcnn layer (TRAIN_FROM): every dcnn layer before it is frozen
    momentum: float = 0.0                       # train.momentum: tf.train.MomentumOptimizer's, in [0, 1); 0 = plain SGD (optimizer sgd only)
    nesterov: bool = False                      # train.nesterov: use_nesterov of the same (needs momentum > 0)
    weight_decay: float = 0.0                   # train.weight_decay: L2 coefficient of the trained weight tensors (decay_ranges); 0 = off
    accumulate: int = 1                         # train.accumulate: most micro-batches one update may sum (train_step_*(micro=(i, k))); 1 = off
    fc_dropout_keep_prob: float = 0.0           # train.fc_dropout_keep_prob: dropout on relu(fc6) / relu(fc7) (Caffe's drop6 / drop7); 0 = off
    fc_dropout_salt: int = 0                    # which mask stream this tower draws from (fc_dropout_salt): a GraphEngine numbers its towers
    tensor_stats_interval: int = 0              # logging.tensor_stats_interval: per-variable statistics every N updates (stat_segments); 0 = off
    ema_decay: float = 0.0                      # train.ema_decay: tf.train.ExponentialMovingAverage's decay, in (0, 1); 0 = no shadow weights
    ema_warmup: bool = False                    # train.ema_warmup: its num_updates form, decay min(decay, (1 + n) / (10 + n)) (ema_rate)
    lars_eeta: float = 0.0                      # train.lars_eeta: tf.contrib.opt.LARSOptimizer's eeta, > 0 (needs momentum > 0); 0 = no LARS
    lars_epsilon: float = 0.0                   # train.lars_epsilon: its epsilon, >= 0, added to the trust ratio's denominator (lars_ranges)
    lamb: bool = False                          # train.lamb: LAMB (tfa.optimizers.LAMB) in the place of the Adam update; optimizer adam only
    lamb_epsilon: Optional[float] = None        # train.lamb_epsilon: its epsilon, > 0; None = 1e-6 when lamb is on (check_lamb)
    label_smoothing: float = 0.0                # train.label_smoothing: tf.losses.softmax_cross_entropy's, in [0, 1); 0 = hard labels
    top_k: int = 0                              # train.top_k: also count the rows whose label is among the k largest logits; 0 = off
    mixup_alpha: float = 0.0                    # train.mixup_alpha: mixup's Beta(alpha, alpha) (clips and labels blended in pairs); 0 = off
    mixup_seed: int = 0                         # train.mixup_seed: the key of the blend-weight draws (mixup_lambda)
    cutmix_alpha: float = 0.0                   # train.cutmix_alpha: CutMix / VideoMix's Beta(alpha, alpha) (a box swapped in pairs); 0 = off
    cutmix_seed: int = 0                        # train.cutmix_seed: the key of the box draws (cutmix_box)
    cutmix_mode: Optional[str] = None           # train.cutmix_mode: spatial | temporal | cuboid; None = spatial when cutmix is on
    cutmix_prob: Optional[float] = None         # train.cutmix_prob: with mixup on too, the chance that a batch is cut; None = 0.5
    class_weights: Optional[Sequence[float]] = None   # train.class_weights: num_classes weights inside the loss's class sum; None = ones
    focal_gamma: float = 0.0                    # train.focal_gamma: the focal loss's focusing parameter (Lin et al. 2017), >= 0; 0 = off
    erase_prob: float = 0.0                     # train.erase_prob: random erasing (Zhong et al. 2017), the chance that a clip gets a box; 0 = off
    erase_scale: Optional[Sequence[float]] = None     # train.erase_scale: the box's share of the frame area (lo, hi); None = (0.02, 0.33)
    erase_ratio: Optional[Sequence[float]] = None     # train.erase_ratio: its aspect ratio h / w, log-uniform in (lo, hi); None = (0.3, 3.3)
    erase_frames: Optional[Sequence[float]] = None    # train.erase_frames: the share of the clip's frames it spans (lo, hi); None = (1, 1)
    erase_mode: Optional[str] = None            # train.erase_mode: zero | clip | pixel, the fill; None = zero
    erase_std: Optional[float] = None           # train.erase_std: the standard deviation of a noise fill; None = 57.63
    erase_seed: int = 0                         # train.erase_seed: the key of the draws (erase_row)
    label_type: str = "single"                  # network.label_type: single (softmax loss) | multiple (sigmoid loss on multi-hot rows)

    def encode_dim(self):
        return FC_DIM if self.frame_encoding_layer in ("fc6", "fc7") else self.num_classes

    def out_dim(self):
        """Width of the pipeline's output rows: num_classes after a classifier, the encode width of a feature pipeline."""
        return self.encode_dim() if self.classifier == "none" else self.num_classes


def tf_same_out(n, s):
    return -(-n // s)


def param_specs(cfg: NetConfig):
    """[(tf_variable_name, shape)] in flat-buffer order (classifier, fc8..fc6, conv5..conv1)."""
    h, w, c = cfg.image_shape
    convs = []
    for name, kh, kw, co, s, g, _, pool in CONV_LAYERS:
        convs.append([("dcnn/%sW" % name, (kh, kw, c // g, co)), ("dcnn/%sb" % name, (co,))])
        h, w, c = tf_same_out(h, s), tf_same_out(w, s), co
        if pool:
            h, w = ops.pool_out(h), ops.pool_out(w)
    specs = []
    dim = cfg.encode_dim()
    check_rnn_cell(cfg.rnn_cell, cfg.classifier, cfg.lstm_hidden, cfg.lstm_bidirectional)
    if cfg.lstm_bidirectional and cfg.classifier != "lstm":
        raise VltfError("lstm_bidirectional needs classifier lstm, not [%s]" % cfg.classifier)
    # fusion attn: its three variables sit between the head and the recurrent layers, the order in which the backward produces them
    A = check_attn(cfg.fusion, cfg.attn_dim, cfg.classifier, (2 if cfg.lstm_bidirectional else 1) * cfg.lstm_hidden)
    if cfg.frame_fusion and len(cfg.frame_fusion) > 1 and cfg.frame_fusion[1] == "attn":
        raise VltfError("frame_fusion: attn is a fusion of the recurrent classifier (lstm_params), not a frame fusion")
    # fusion vlad: as attn's, its three variables sit between the head and the recurrent layers; the head reads K x HO columns
    KV = check_vlad(cfg.fusion, cfg.vlad_clusters, cfg.classifier, (2 if cfg.lstm_bidirectional else 1) * cfg.lstm_hidden)
    if cfg.frame_fusion and len(cfg.frame_fusion) > 1 and cfg.frame_fusion[1] == "vlad":
        raise VltfError("frame_fusion: vlad is a fusion of the recurrent classifier (lstm_params), not a frame fusion")
    kv = KV or 1
    sa = check_mhsa(cfg.rnn_cell, cfg.lstm_hidden, cfg.fpc, cfg.sa_heads, cfg.sa_positions, cfg.fusion, sa_block=cfg.sa_block,
                    sa_ffn_dim=cfg.sa_ffn_dim, sa_attn_dropout=cfg.sa_attn_dropout, sa_dropout=cfg.sa_dropout,
                    sa_drop_path=cfg.sa_drop_path)
    tc = check_tcn(cfg.rnn_cell, cfg.lstm_hidden, cfg.lstm_layers, cfg.tcn_kernel, cfg.tcn_dilation, cfg.tcn_causal, cfg.fusion)
    if tc:
        H = cfg.lstm_hidden
        if kv * H != cfg.num_classes:                     # the head's names are the LSTM classifier's
            specs += [("output_fc_w", (kv * H, cfg.num_classes)), ("output_fc_b", (cfg.num_classes,))]
        specs += attn_specs(H, A) if A else []
        specs += vlad_specs(H, KV) if KV else []
        specs += tcn_specs(cfg.lstm_layers, dim, H, tc[0])
    elif sa:
        H = cfg.lstm_hidden
        if kv * H != cfg.num_classes:                     # the head's names are the LSTM classifier's
            specs += [("output_fc_w", (kv * H, cfg.num_classes)), ("output_fc_b", (cfg.num_classes,))]
        specs += attn_specs(H, A) if A else []
        specs += vlad_specs(H, KV) if KV else []
        d = dim
        F = check_sa_block(cfg.rnn_cell, H, cfg.sa_block, cfg.sa_ffn_dim)
        if F:
            specs += encoder_specs(cfg.lstm_layers, d, H, F, sa[0], cfg.fpc, positions=sa[1])
        for l in range(0 if F else cfg.lstm_layers):
            specs += mhsa_specs(l, d, H, sa[0], cfg.fpc, positions=sa[1])
            d = H
    elif cfg.classifier == "lstm" and cfg.rnn_cell == "gru":
        H = cfg.lstm_hidden
        if kv * H != cfg.num_classes:                     # the head's names are the LSTM classifier's
            head = "fc_convert" if cfg.fusion == "state" else "output_fc"
            specs += [(head + "_w", (kv * H, cfg.num_classes)), (head + "_b", (cfg.num_classes,))]
        specs += attn_specs(H, A) if A else []
        specs += vlad_specs(H, KV) if KV else []
        d = dim
        for l in range(cfg.lstm_layers):
            specs += gru_specs(l, d, H)
            d = H
    elif cfg.classifier == "lstm" and cfg.lstm_bidirectional:
        check_blstm(cfg.lstm_hidden)
        H = cfg.lstm_hidden
        if kv * 2 * H != cfg.num_classes:                 # the head reads the 2H-wide fused vector (fusion vlad: K of them)
            head = "fc_convert" if cfg.fusion == "state" else "output_fc"
            specs += [(head + "_w", (kv * 2 * H, cfg.num_classes)), (head + "_b", (cfg.num_classes,))]
        specs += attn_specs(2 * H, A) if A else []
        specs += vlad_specs(2 * H, KV) if KV else []
        d = dim
        for l in range(cfg.lstm_layers):
            specs += [(n, (d + H, 4 * H) if n.endswith("kernel") else (4 * H,)) for n in blstm_names(l)]
            d = 2 * H
    elif cfg.classifier == "lstm":
        if kv * cfg.lstm_hidden != cfg.num_classes:
            # fusion `state`: logits = convert_dim_fc(final h) under its default name (model.py:137-141), else "output_fc" (lstm.py:90)
            head = "fc_convert" if cfg.fusion == "state" else "output_fc"
            specs += [(head + "_w", (kv * cfg.lstm_hidden, cfg.num_classes)), (head + "_b", (cfg.num_classes,))]
        specs += attn_specs(cfg.lstm_hidden, A) if A else []
        specs += vlad_specs(cfg.lstm_hidden, KV) if KV else []
        d = dim
        for l in range(cfg.lstm_layers):
            pre = "rnn/multi_rnn_cell/cell_%d/basic_lstm_cell/" % l
            specs += [(pre + "kernel", (d + cfg.lstm_hidden, 4 * cfg.lstm_hidden)), (pre + "bias", (4 * cfg.lstm_hidden,))]
            d = cfg.lstm_hidden
    elif cfg.classifier == "fc":
        if dim != cfg.num_classes:
            specs += [("fc_convert_w", (dim, cfg.num_classes)), ("fc_convert_b", (cfg.num_classes,))]
    elif cfg.classifier == "none":
        pass
    else:
        raise VltfError("Undefined classifier [%s]" % cfg.classifier)
    if cfg.frame_encoding_layer not in ("fc6", "fc7"):
        specs += [("dcnn/fc8W", (FC_DIM, cfg.num_classes)), ("dcnn/fc8b", (cfg.num_classes,))]
    if cfg.frame_encoding_layer != "fc6":
        specs += [("dcnn/fc7W", (FC_DIM, FC_DIM)), ("dcnn/fc7b", (FC_DIM,))]
    specs += [("dcnn/fc6W", (h * w * c, FC_DIM)), ("dcnn/fc6b", (FC_DIM,))]
    for pair in reversed(convs):
        specs += pair
    return specs


# ---- fine-tuning plan: learning-rate tiers, frozen layers, exchange chunks (host only) ------------------------------------------
TRAIN_FROM = ("conv1", "conv2", "conv3", "conv4", "conv5", "fc6", "fc7", "fc8", "classifier")
FC6_CHUNKS = 4          # row blocks of the fc6 weight gradient = all-reduce chunks of the data-parallel exchange


def dcnn_layers(cfg: NetConfig):
    """Names of the dcnn layers the pipeline has, first to last (alexnet.py:60-280: the tower ends at frame_encoding_layer)."""
    layers = [c[0] for c in CONV_LAYERS] + ["fc6"]
    if cfg.frame_encoding_layer != "fc6":
        layers.append("fc7")
    if cfg.frame_encoding_layer not in ("fc6", "fc7"):
        layers.append("fc8")
    return layers


def frozen_layers(cfg: NetConfig):
    """The dcnn layers cfg.train_from freezes (every one before it; `classifier`: all of them).  Refuses a name the pipeline lacks."""
    if cfg.train_from is None:
        return []
    layers = dcnn_layers(cfg)
    if cfg.train_from not in TRAIN_FROM:
        raise VltfError("train_from [%s] is not one of %s" % (cfg.train_from, ", ".join(TRAIN_FROM)))
    if cfg.train_from == "classifier":
        return layers
    if cfg.train_from not in layers:
        raise VltfError("train_from [%s]: with frame_encoding_layer [%s] the pipeline has no such layer (it has %s)" %
                        (cfg.train_from, cfg.frame_encoding_layer, ", ".join(layers)))
    return layers[:layers.index(cfg.train_from)]


_REGULAR_LEAVES = {l + k for l in [c[0] for c in CONV_LAYERS] + ["fc6", "fc7"] for k in ("W", "b")}


def is_regular(name):
    """The reference's `train_regular` variables (alexnet.py:214,231,251): the dcnn's, whatever pipeline scope they carry, but fc8
    (alexnet.py:280: re-initialised, so it learns with the modified ones).  Every other variable -- fc8, the LSTM's, the fc heads --
    is `train_modified` and gets lr * lr_mult (train.py:180)."""
    parts = name.split("/")
    return len(parts) in (2, 3) and parts[-2] == "dcnn" and parts[-1] in _REGULAR_LEAVES


def check_lr_mult(lr_mult):
    """None -> 1.0; anything but a finite float > 0 is refused (layers are held fixed with train_from, not with a zero factor)."""
    if lr_mult is None:
        return 1.0
    m = float(lr_mult)
    if not (m > 0.0 and math.isfinite(m)):
        raise VltfError("lr_mult must be a finite number > 0, got %r (use train_from to hold layers fixed)" % (lr_mult,))
    return m


def check_momentum(optimizer, momentum, nesterov):
    """(momentum, nesterov) of an SGD run, None read as 0 / False.  Refused: momentum outside [0, 1), nesterov without momentum, either
    with Adam (which keeps its own first moment)."""
    m = 0.0 if momentum is None else float(momentum)
    nesterov = bool(nesterov)
    if not (0.0 <= m < 1.0):
        raise VltfError("momentum must lie in [0, 1), got %r" % (momentum,))
    if nesterov and m == 0.0:
        raise VltfError("nesterov needs momentum > 0")
    if optimizer == "adam" and (m > 0.0 or nesterov):
        raise VltfError("momentum / nesterov belong to optimizer sgd; adam has its own first moment")
    return m, nesterov


def check_lars(optimizer, momentum, eeta, epsilon):
    """(eeta, epsilon) of tf.contrib.opt.LARSOptimizer, None read as 0; eeta 0 = off.  Refused: either value not a number, negative or
    not finite; an epsilon without an eeta; LARS with Adam; LARS without momentum > 0 (TF's optimizer is a momentum optimizer, and
    vl_momentum_apply's rule is not defined at momentum 0)."""
    vals = []
    for key, v in (("lars_eeta", eeta), ("lars_epsilon", epsilon)):
        if v is not None and (isinstance(v, (bool, np.bool_, str, bytes)) or not isinstance(v, (int, float, np.integer, np.floating))):
            raise VltfError("%s must be a finite number >= 0 (0 / None = off), got %r" % (key, v))
        f = 0.0 if v is None else float(v)
        if not (f >= 0.0 and math.isfinite(f)):       # (NaN fails)
            raise VltfError("%s must be a finite number >= 0 (0 / None = off), got %r" % (key, v))
        vals.append(f)
    e, eps = vals
    if e == 0.0:
        if eps > 0.0:
            raise VltfError("lars_epsilon needs lars_eeta > 0")
        return 0.0, 0.0
    if optimizer == "adam":
        raise VltfError("lars_eeta belongs to optimizer sgd with momentum; adam scales its own step per element")
    if not (momentum is not None and float(momentum) > 0.0):
        raise VltfError("lars_eeta needs momentum > 0: LARS is a momentum optimizer")
    return e, eps


LAMB_EPSILON = 1e-6       # tfa.optimizers.LAMB's default epsilon


def check_lamb(optimizer, lamb, lamb_epsilon):
    """(lamb, epsilon) of a run, None read as off / the default.  lamb is True or False; on, the epsilon defaults to LAMB_EPSILON (TFA's).
    Refused: lamb that is not a bool; lamb with any optimizer but adam (it is Adam's moments with a trust ratio); an epsilon that is not
    a number, not finite or <= 0; an epsilon given without lamb (it names a rule that is off, a likely slip)."""
    if lamb is not None and not isinstance(lamb, (bool, np.bool_)):
        raise VltfError("lamb must be True or False, got %r" % (lamb,))
    on = bool(lamb)
    eps = None
    if lamb_epsilon is not None:
        if isinstance(lamb_epsilon, (bool, np.bool_, str, bytes)) or not isinstance(lamb_epsilon, (int, float, np.integer, np.floating)):
            raise VltfError("lamb_epsilon must be a finite number > 0, got %r" % (lamb_epsilon,))
        eps = float(lamb_epsilon)
        if not (eps > 0.0 and math.isfinite(eps)):        # (NaN fails)
            raise VltfError("lamb_epsilon must be a finite number > 0, got %r" % (lamb_epsilon,))
        if not (float(np.float32(eps)) > 0.0 and math.isfinite(float(np.float32(eps)))):
            raise VltfError("lamb_epsilon must be a positive finite float32, got %r" % (lamb_epsilon,))
    if not on:
        if eps is not None:
            raise VltfError("lamb_epsilon needs lamb: True")
        return False, 0.0
    if optimizer != "adam":
        raise VltfError("lamb belongs to optimizer adam (it keeps Adam's moments); got optimizer %r" % (optimizer,))
    return True, LAMB_EPSILON if eps is None else eps


def lamb_corrections(n):
    """(c1, c2) = (1 / (1 - 0.9^t), 1 / (1 - 0.999^t)) of the update applied after n earlier ones, t = n + 1 (n = step_count before its
    increment: updates, not micro-batches), in double and rounded to float32 once.  The ONE place they are computed: the eager launches
    take them as arguments, a replayed step reads them from the step state (ops.step_state_set_lamb)."""
    t = int(n) + 1
    if t < 1:
        raise VltfError("lamb_corrections: n must be >= 0, got %r" % (n,))
    return float(np.float32(1.0 / (1.0 - 0.9 ** t))), float(np.float32(1.0 / (1.0 - 0.999 ** t)))


def check_ema(decay, warmup):
    """(decay, warmup) of the weight average, None read as 0 / False; 0 = off.  Refused: a decay that is not a number, not finite or
    outside (0, 1), and warm-up without a decay."""
    if isinstance(decay, (bool, np.bool_, str, bytes)) or (decay is not None and not isinstance(decay, (int, float, np.integer, np.floating))):
        raise VltfError("ema_decay must be a number in (0, 1) (or 0 / None for none), got %r" % (decay,))
    if warmup is not None and not isinstance(warmup, (bool, np.bool_)):
        raise VltfError("ema_warmup must be True or False, got %r" % (warmup,))
    d = 0.0 if decay is None else float(decay)
    warmup = bool(warmup)
    if not (d == 0.0 or 0.0 < d < 1.0):           # (NaN fails both)
        raise VltfError("ema_decay must lie in (0, 1) (or be 0 / None for none), got %r" % (decay,))
    if warmup and d == 0.0:
        raise VltfError("ema_warmup needs ema_decay > 0")
    return d, warmup


def ema_rate(decay, warmup, n):
    """The rate 1 - decay_n of the update applied after n earlier ones (n = step_count before its increment: updates, not
    micro-batches), as the float32 the launch gets.  Without warm-up float32(1 - decay); with it TF's min(decay, (1 + n) / (10 + n))
    written for 1 - decay, max(1 - decay, 9 / (10 + n)), in double and rounded once, so nothing is lost to cancellation near 1.  The
    ONE place the rate is computed: the eager launch takes it as an argument, a replayed step reads it from the step state."""
    r = 1.0 - float(decay)
    if warmup:
        r = max(r, 9.0 / (10.0 + int(n)))
    return float(np.float32(r))


def ema_extra_bytes(count):
    """Device memory the shadow weights cost: one float per parameter (178 MB at the 44.6 M of the full LRCN)."""
    return 4 * int(count)


def check_weight_decay(weight_decay):
    """The L2 coefficient of a run as a float, None read as 0 (off).  Refused: negative, NaN, infinite, not a number."""
    if weight_decay is None:
        return 0.0
    if isinstance(weight_decay, (bool, str, bytes)) or not isinstance(weight_decay, (int, float, np.integer, np.floating)):
        raise VltfError("weight_decay must be a finite number >= 0, got %r" % (weight_decay,))
    d = float(weight_decay)
    if not (d >= 0.0 and math.isfinite(d)):
        raise VltfError("weight_decay must be a finite number >= 0, got %r" % (weight_decay,))
    return d


def check_fc_dropout(keep_prob):
    """The keep probability of the fc6 / fc7 dropout as a float, None or 0 read as 0 (off).  Accepted: (0, 1]; 1 launches nothing.
    Refused: negative, above 1, NaN, infinite, not a number."""
    if keep_prob is None:
        return 0.0
    if isinstance(keep_prob, (bool, str, bytes)) or not isinstance(keep_prob, (int, float, np.integer, np.floating)):
        raise VltfError("fc_dropout_keep_prob must be a number in [0, 1] (0 = off), got %r" % (keep_prob,))
    k = float(keep_prob)
    if not (0.0 <= k <= 1.0):                     # (NaN fails both)
        raise VltfError("fc_dropout_keep_prob must be a number in [0, 1] (0 = off), got %r" % (keep_prob,))
    return k


def check_label_smoothing(label_smoothing):
    """The label smoothing of the loss as a float, None read as 0 (off).  Accepted: [0, 1).  Refused: negative, 1 or above, NaN,
    infinite, not a number (booleans included)."""
    if label_smoothing is None:
        return 0.0
    if isinstance(label_smoothing, (bool, np.bool_, str, bytes)) or not isinstance(label_smoothing, (int, float, np.integer, np.floating)):
        raise VltfError("label_smoothing must be a number in [0, 1) (0 / None = off), got %r" % (label_smoothing,))
    s = float(label_smoothing)
    if not (0.0 <= s < 1.0):                      # (NaN fails both, inf the second)
        raise VltfError("label_smoothing must be a number in [0, 1) (0 / None = off), got %r" % (label_smoothing,))
    return s


def check_class_weights(class_weights, num_classes):
    """The class weights of the loss as a float32 array of num_classes entries, or None (off: every class weighs 1).  Refused: anything
    but a sequence of numbers (strings and booleans included), a length other than num_classes, a negative, NaN or infinite entry, and
    weights that are all zero (no row would carry a loss)."""
    if class_weights is None:
        return None
    msg = "class_weights must be %d finite numbers >= 0, not all zero (None = off), got %%s" % num_classes
    if isinstance(class_weights, (str, bytes)) or np.isscalar(class_weights):
        raise VltfError(msg % repr(class_weights))
    try:
        vals = list(class_weights)
    except TypeError:
        raise VltfError(msg % repr(class_weights))
    if len(vals) != num_classes:
        raise VltfError(msg % ("%d entries" % len(vals)))
    for v in vals:
        if isinstance(v, (bool, np.bool_, str, bytes)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise VltfError(msg % ("the entry %r" % (v,)))
        if not (math.isfinite(float(v)) and float(v) >= 0.0):
            raise VltfError(msg % ("the entry %r" % (v,)))
    with np.errstate(over="ignore"):
        w = np.asarray(vals, np.float64).astype(np.float32)
    if not np.isfinite(w).all():                  # (a number beyond float32's range)
        raise VltfError(msg % "an entry beyond float32")
    if not (w > 0).any():
        raise VltfError(msg % "all zeros")
    return w


def check_focal_gamma(focal_gamma):
    """The focusing parameter of the focal loss as a float, None read as 0 (off).  Accepted: finite and >= 0.  Refused: negative, NaN,
    infinite, not a number (booleans included)."""
    if focal_gamma is None:
        return 0.0
    if isinstance(focal_gamma, (bool, np.bool_, str, bytes)) or not isinstance(focal_gamma, (int, float, np.integer, np.floating)):
        raise VltfError("focal_gamma must be a finite number >= 0 (0 / None = off), got %r" % (focal_gamma,))
    g = float(focal_gamma)
    if not (math.isfinite(g) and 0.0 <= g <= 3.0e38):
        raise VltfError("focal_gamma must be a finite number >= 0 (0 / None = off), got %r" % (focal_gamma,))
    return g


LABEL_TYPES = ("single", "multiple")


def check_label_type(label_type):
    """network.label_type as "single" (one class per row: the softmax loss launches) or "multiple" (multi-hot rows: independent
    sigmoids per class, ops.sigmoid_xent).  None reads as "single".  Refused: anything else, other spellings included."""
    if label_type is None:
        return "single"
    if not isinstance(label_type, str) or label_type not in LABEL_TYPES:
        raise VltfError("label_type must be one of %s (None = single), got %r" % (", ".join(LABEL_TYPES), label_type))
    return label_type


def check_top_k(top_k):
    """The k of the top-k accuracy as an int, None read as 0 (off).  A k above the row width is allowed (every live row is a hit).
    Refused: bools, strings, floats that are not whole (NaN and inf among them), values < 0."""
    if top_k is None:
        return 0
    if isinstance(top_k, (bool, np.bool_, str, bytes)) or not isinstance(top_k, (int, float, np.integer, np.floating)):
        raise VltfError("top_k must be a whole number >= 0 (0 / None = off), got %r" % (top_k,))
    if isinstance(top_k, (float, np.floating)) and not (math.isfinite(top_k) and float(top_k) == int(top_k)):
        raise VltfError("top_k must be a whole number >= 0 (0 / None = off), got %r" % (top_k,))
    k = int(top_k)
    if not (0 <= k <= 0x7fffffff):
        raise VltfError("top_k must be a whole number >= 0 (0 / None = off), got %r" % (top_k,))
    return k


def check_mixup(alpha, seed=None):
    """(alpha, seed) of mixup as (float, int), None read as 0 (off).  alpha: a finite number >= 0, the Beta(alpha, alpha) the blend
    weight is drawn from.  seed: a whole number in [0, 2^64), the key of the draws (mixup_lambda).  Refused: bools and strings for
    either, a negative, NaN or infinite alpha, a seed that is not whole or negative, and a seed other than 0 without an alpha."""
    if alpha is None:
        a = 0.0
    else:
        if isinstance(alpha, (bool, np.bool_, str, bytes)) or not isinstance(alpha, (int, float, np.integer, np.floating)):
            raise VltfError("mixup_alpha must be a finite number >= 0 (0 / None = off), got %r" % (alpha,))
        a = float(alpha)
        if not (math.isfinite(a) and a >= 0.0):
            raise VltfError("mixup_alpha must be a finite number >= 0 (0 / None = off), got %r" % (alpha,))
    if seed is None:
        s = 0
    else:
        if isinstance(seed, (bool, np.bool_, str, bytes)) or not isinstance(seed, (int, float, np.integer, np.floating)):
            raise VltfError("mixup_seed must be a whole number >= 0, got %r" % (seed,))
        if isinstance(seed, (float, np.floating)) and not (math.isfinite(seed) and float(seed) == int(seed)):
            raise VltfError("mixup_seed must be a whole number >= 0, got %r" % (seed,))
        s = int(seed)
        if not (0 <= s < 2 ** 64):
            raise VltfError("mixup_seed must be a whole number >= 0 (below 2^64), got %r" % (seed,))
    if s != 0 and a == 0.0:
        raise VltfError("mixup_seed %d is given without mixup_alpha: mixup is off and nothing would be drawn" % s)
    return a, s


def fold_lambda(lam):
    """max(lam, 1 - lam) of a blend weight in [0, 1]: under the pairing i <-> B - 1 - i swapping lam and 1 - lam only swaps the
    partners, so the fold loses nothing, and a row's own label is always the dominant one.  Refused: outside [0, 1], NaN, not a number."""
    if isinstance(lam, (bool, np.bool_, str, bytes)) or not isinstance(lam, (int, float, np.integer, np.floating)):
        raise VltfError("mix_lambda must be a number in [0, 1], got %r" % (lam,))
    lam = float(lam)
    if not (0.0 <= lam <= 1.0):                   # (NaN fails both)
        raise VltfError("mix_lambda must be a number in [0, 1], got %r" % (lam,))
    return max(lam, 1.0 - lam)


def mixup_lambda(alpha, seed, draw_index):
    """The folded blend weight of the step with this draw index (LRCNEngine._draw_index): one Beta(alpha, alpha) draw from a Philox
    generator keyed by (seed, draw_index), then fold_lambda.  A pure function of its arguments: every rank draws the same value, every
    micro-step of an accumulated update its own, and a resumed run continues the sequence."""
    alpha, seed = check_mixup(alpha, seed)
    if alpha == 0.0:
        return 1.0
    rng = np.random.Generator(np.random.Philox(key=np.array([seed, int(draw_index)], np.uint64)))
    return fold_lambda(float(rng.beta(alpha, alpha)))


CUTMIX_MODES = ("spatial", "temporal", "cuboid")


def check_cutmix(alpha, seed=None, mode=None, prob=None):
    """(alpha, seed, mode, prob) of CutMix / VideoMix as (float, int, str, float), None read as off / the default.  alpha: a finite
    number >= 0, the Beta(alpha, alpha) the cut fraction is drawn from (0 = off).  seed: a whole number in [0, 2^64), the key of the
    draws (cutmix_box).  mode: which axes the box spans -- 'spatial' (every frame, a y-x rectangle; the default), 'temporal' (whole
    frames, a run of t) or 'cuboid' (all three).  prob: with mixup on as well, the chance in [0, 1] that a batch is cut and not blended
    (default 0.5).  Refused: bools and strings for a number, a negative, NaN or infinite alpha, a seed that is not whole or negative,
    an unknown mode, a prob outside [0, 1], and a seed, mode or prob without an alpha."""
    def number(v, name, what):
        if isinstance(v, (bool, np.bool_, str, bytes)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise VltfError("%s must be %s, got %r" % (name, what, v))
        return v

    a = 0.0
    if alpha is not None:
        a = float(number(alpha, "cutmix_alpha", "a finite number >= 0 (0 / None = off)"))
        if not (math.isfinite(a) and a >= 0.0):
            raise VltfError("cutmix_alpha must be a finite number >= 0 (0 / None = off), got %r" % (alpha,))
    s = 0
    if seed is not None:
        number(seed, "cutmix_seed", "a whole number >= 0")
        if isinstance(seed, (float, np.floating)) and not (math.isfinite(seed) and float(seed) == int(seed)):
            raise VltfError("cutmix_seed must be a whole number >= 0, got %r" % (seed,))
        s = int(seed)
        if not (0 <= s < 2 ** 64):
            raise VltfError("cutmix_seed must be a whole number >= 0 (below 2^64), got %r" % (seed,))
    if mode is not None and (not isinstance(mode, str) or mode not in CUTMIX_MODES):
        raise VltfError("cutmix_mode must be one of %s, got %r" % (" | ".join(CUTMIX_MODES), mode))
    pr = 0.5
    if prob is not None:
        pr = float(number(prob, "cutmix_prob", "a number in [0, 1]"))
        if not (0.0 <= pr <= 1.0):                # (NaN fails both)
            raise VltfError("cutmix_prob must be a number in [0, 1], got %r" % (prob,))
    if a == 0.0:
        for name, given in (("cutmix_seed", s != 0), ("cutmix_mode", mode is not None), ("cutmix_prob", prob is not None)):
            if given:
                raise VltfError("%s is given without cutmix_alpha: CutMix is off and nothing would be drawn" % name)
    return a, s, mode if mode is not None else "spatial", pr


def cutmix_lambda(box, fpc, h, w):
    """The label weight of a cut: 1 - volume(box) / (fpc * h * w), from the integers in fp64, then rounded to the fp32 the device word
    holds.  1.0 exactly when the box is empty."""
    t0, t1, y0, y1, x0, x1 = (int(v) for v in box)
    vol = max(t1 - t0, 0) * max(y1 - y0, 0) * max(x1 - x0, 0)
    return float(np.float32(1.0 - vol / float(fpc * h * w)))


def check_cut_box(box, fpc, h, w):
    """A caller's box (t0, t1, y0, y1, x0, x1) as six ints.  Refused: anything but six whole numbers, a range that leaves
    [0, fpc] x [0, h] x [0, w] or is reversed, and a volume above half the clip (the own label has to stay the dominant one)."""
    try:
        vals = tuple(int(v) for v in box)
        ok = len(vals) == 6 and all(not isinstance(v, (bool, np.bool_, str, bytes)) and float(v) == int(v) for v in box)
    except (TypeError, ValueError):
        vals, ok = (), False
    if not ok:
        raise VltfError("cut_box must be six whole numbers (t0, t1, y0, y1, x0, x1), got %r" % (box,))
    for a, (name, n) in enumerate((("t", fpc), ("y", h), ("x", w))):
        lo, hi = vals[2 * a], vals[2 * a + 1]
        if lo < 0 or hi > n or lo > n or hi < 0:
            raise VltfError("cut_box: the %s range [%d, %d) leaves the frame's [0, %d]" % (name, lo, hi, n))
        if lo > hi:
            raise VltfError("cut_box: the %s range [%d, %d) is reversed" % (name, lo, hi))
    vol = (vals[1] - vals[0]) * (vals[3] - vals[2]) * (vals[5] - vals[4])
    if 2 * vol > fpc * h * w:
        raise VltfError("cut_box: the volume %d is above half the clip (%d x %d x %d): the partner's label would dominate"
                        % (vol, fpc, h, w))
    return vals


def cutmix_box(alpha, seed, mode, draw_index, fpc, h, w):
    """((t0, t1, y0, y1, x0, x1), u) of the step with this draw index (LRCNEngine._draw_index): the half-open box that clip i and clip
    B - 1 - i exchange, and the uniform number that decides between CutMix and mixup when both are on (u < cutmix_prob: cut).  One
    Philox generator keyed by (seed, draw_index), drawn from in a fixed order whatever the mode: lam0 = Beta(alpha, alpha) folded to
    max(lam0, 1 - lam0) (the cut is at most half the clip); the centres ct, cy, cx, uniform over fpc, h, w; last u.  The extents are
    (fpc, int(h r), int(w r)) with r = sqrt(1 - lam0) for 'spatial', (int(fpc (1 - lam0)), h, w) for 'temporal' and
    (int(fpc r), int(h r), int(w r)) with r = cbrt(1 - lam0) for 'cuboid'; an axis runs over [c - b // 2, c - b // 2 + b) clipped
    to it (timm's rule), a full-extent axis over all of it.  A pure function of its arguments: every rank draws the same box, every
    micro-step its own, and a resumed run continues the sequence."""
    alpha, seed, mode, _ = check_cutmix(alpha, seed, mode)
    fpc, h, w = int(fpc), int(h), int(w)
    if alpha == 0.0:
        return (0, 0, 0, 0, 0, 0), 1.0
    rng = np.random.Generator(np.random.Philox(key=np.array([seed, int(draw_index)], np.uint64)))
    lam0 = fold_lambda(float(rng.beta(alpha, alpha)))
    cut = 1.0 - lam0
    if mode == "spatial":
        r = math.sqrt(cut)
        ext = (fpc, int(h * r), int(w * r))
    elif mode == "temporal":
        ext = (int(fpc * cut), h, w)
    else:
        r = float(np.cbrt(cut))
        ext = (int(fpc * r), int(h * r), int(w * r))
    centres = [int(rng.integers(n)) for n in (fpc, h, w)]
    box = []
    for c, b, n in zip(centres, ext, (fpc, h, w)):
        lo = c - b // 2
        box += [0, n] if b >= n else [min(max(lo, 0), n), min(max(lo + b, 0), n)]
    u = float(rng.random())
    return tuple(box), u


ERASE_MODES = ops.ERASE_MODES                    # zero | clip | pixel: vl_erase_boxes' mode 0, 1, 2
ERASE_DEFAULTS = dict(scale=(0.02, 0.33), ratio=(0.3, 3.3), frames=(1.0, 1.0), mode="zero", std=57.63, seed=0)
ERASE_ATTEMPTS = 10                              # torchvision's RandomErasing.get_params tries as often
EraseConfig = collections.namedtuple("EraseConfig", "prob scale ratio frames mode std seed")


def check_erase(prob=None, scale=None, ratio=None, frames=None, mode=None, std=None, seed=None):
    """The options of random erasing (Zhong et al. 2017; torchvision RandomErasing, timm reprob / remode) as an EraseConfig, None read
    as off / the default.  prob: the chance in [0, 1] that a clip gets a box (0 = off).  scale: (lo, hi) of the box's share of the
    frame's area, 0 < lo <= hi <= 1 (default (0.02, 0.33)).  ratio: (lo, hi) of its aspect ratio h / w, drawn log-uniformly,
    0 < lo <= hi (default (0.3, 3.3)).  frames: (lo, hi) of the share of the clip's frames the box spans, 0 < lo <= hi <= 1 (default
    (1, 1): every frame).  mode: the fill -- 'zero' (the mean colour of a mean-subtracted input; the default), 'clip' (one normal-like
    value per clip and channel) or 'pixel' (one per element).  std: the standard deviation of a noise fill, finite and >= 0 (default
    57.63: ImageNet's per-channel deviation on the 0..255 scale).  seed: a whole number in [0, 2^64), the key of the draws (erase_row).
    Refused: bools and strings for a number, a prob outside [0, 1], a range that is not two numbers 0 < lo <= hi (<= 1 for scale and
    frames), an unknown mode, a negative, NaN or infinite std, a seed that is not whole or outside [0, 2^64), and any other option
    given while prob is 0 or absent."""
    def number(v, name, what):
        if isinstance(v, (bool, np.bool_, str, bytes)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise VltfError("%s must be %s, got %r" % (name, what, v))
        return v

    def span(v, name, cap):
        what = "two numbers 0 < lo <= hi%s" % (" <= 1" if cap else "")
        if isinstance(v, (str, bytes)) or not isinstance(v, (list, tuple, np.ndarray)) or len(v) != 2:
            raise VltfError("%s must be %s, got %r" % (name, what, v))
        lo, hi = (float(number(x, name, what)) for x in v)
        if not (0.0 < lo <= hi and math.isfinite(hi) and (not cap or hi <= 1.0)):
            raise VltfError("%s must be %s, got %r" % (name, what, v))
        return lo, hi

    pr = 0.0
    if prob is not None:
        pr = float(number(prob, "erase_prob", "a number in [0, 1] (0 / None = off)"))
        if not (0.0 <= pr <= 1.0):                # (NaN fails both)
            raise VltfError("erase_prob must be a number in [0, 1] (0 / None = off), got %r" % (prob,))
    sd = 0
    if seed is not None:
        number(seed, "erase_seed", "a whole number >= 0")
        if isinstance(seed, (float, np.floating)) and not (math.isfinite(seed) and float(seed) == int(seed)):
            raise VltfError("erase_seed must be a whole number >= 0, got %r" % (seed,))
        sd = int(seed)
        if not (0 <= sd < 2 ** 64):
            raise VltfError("erase_seed must be a whole number >= 0 (below 2^64), got %r" % (seed,))
    sc = span(scale, "erase_scale", True) if scale is not None else ERASE_DEFAULTS["scale"]
    ra = span(ratio, "erase_ratio", False) if ratio is not None else ERASE_DEFAULTS["ratio"]
    fr = span(frames, "erase_frames", True) if frames is not None else ERASE_DEFAULTS["frames"]
    if mode is not None and (not isinstance(mode, str) or mode not in ERASE_MODES):
        raise VltfError("erase_mode must be one of %s, got %r" % (" | ".join(ERASE_MODES), mode))
    st = ERASE_DEFAULTS["std"]
    if std is not None:
        st = float(number(std, "erase_std", "a finite number >= 0"))
        if not (math.isfinite(st) and st >= 0.0):
            raise VltfError("erase_std must be a finite number >= 0, got %r" % (std,))
    if pr == 0.0:
        for name, given in (("erase_scale", scale is not None), ("erase_ratio", ratio is not None), ("erase_frames", frames is not None),
                            ("erase_mode", mode is not None), ("erase_std", std is not None), ("erase_seed", sd != 0)):
            if given:
                raise VltfError("%s is given without erase_prob: random erasing is off and nothing would be drawn" % name)
    return EraseConfig(pr, sc, ra, fr, mode if mode is not None else ERASE_DEFAULTS["mode"], st, sd)


def erase_config(cfg):
    """An EraseConfig from one, or from anything with NetConfig's erase_* fields."""
    if isinstance(cfg, EraseConfig):
        return cfg
    return check_erase(cfg.erase_prob, cfg.erase_scale, cfg.erase_ratio, cfg.erase_frames, cfg.erase_mode, cfg.erase_std, cfg.erase_seed)


def check_erase_boxes(boxes, clips, fpc, h, w):
    """A caller's boxes, one (t0, t1, y0, y1, x0, x1) per clip, as a list of six-int tuples.  Refused: anything but `clips` rows of six
    whole numbers, a range that leaves [0, fpc] x [0, h] x [0, w] or is reversed.  (CutMix's half-volume rule has no place here: the
    labels do not change.)"""
    try:
        rows = [tuple(box) for box in boxes]
    except TypeError:
        rows = None
    if rows is None or len(rows) != clips:
        raise VltfError("erase_boxes must be %d boxes (t0, t1, y0, y1, x0, x1), one per clip, got %r" % (clips, boxes))
    out = []
    for i, box in enumerate(rows):
        try:
            vals = tuple(int(v) for v in box)
            ok = len(vals) == 6 and all(not isinstance(v, (bool, np.bool_, str, bytes)) and float(v) == int(v) for v in box)
        except (TypeError, ValueError):
            vals, ok = (), False
        if not ok:
            raise VltfError("erase_boxes: box %d must be six whole numbers (t0, t1, y0, y1, x0, x1), got %r" % (i, box))
        for a, (name, n) in enumerate((("t", fpc), ("y", h), ("x", w))):
            lo, hi = vals[2 * a], vals[2 * a + 1]
            if lo < 0 or hi > n or lo > n or hi < 0:
                raise VltfError("erase_boxes: box %d: the %s range [%d, %d) leaves the frame's [0, %d]" % (i, name, lo, hi, n))
            if lo > hi:
                raise VltfError("erase_boxes: box %d: the %s range [%d, %d) is reversed" % (i, name, lo, hi))
        out.append(vals)
    return out


def erase_row(cfg, draw_index, global_clip, fpc, h, w):
    """The eight ints (t0, t1, y0, y1, x0, x1, key_lo, key_hi) of one clip's row of the erase table (vl_erase_boxes) in the step with
    this draw index (LRCNEngine._draw_index).  cfg: an EraseConfig (check_erase) or a NetConfig.  One Philox generator with the key
    (seed, draw_index) and the counter (global_clip, 0, 0, 0), drawn from in a fixed order: the 64-bit noise key (always, so that an
    override of the boxes keeps the keys); u, the clip is erased iff u < prob; then up to ten attempts of torchvision's get_params --
    area = h w U(scale), r = exp(U(log ratio)), bh = int(round(sqrt(area r))), bw = int(round(sqrt(area / r))), accepted iff
    0 < bh < h and 0 < bw < w, then y0 = integers(h - bh + 1), x0 = integers(w - bw + 1); last the frame run, L = max(1,
    int(round(fpc U(frames)))) frames from t0 = integers(fpc - L + 1).  A clip that is not erased, or with no attempt accepted, has the
    empty box (six zeros) and its key.  The key words are int32 (the low and the high half's bits).  A pure function of its arguments:
    rank r of a data-parallel run passes global_clip = r B + i, every micro-step its own draw index, and a resumed run continues the
    sequence."""
    e = erase_config(cfg)
    fpc, h, w = int(fpc), int(h), int(w)
    rng = np.random.Generator(np.random.Philox(key=np.array([e.seed, int(draw_index)], np.uint64),
                                               counter=np.array([int(global_clip), 0, 0, 0], np.uint64)))
    key = int(rng.integers(0, 2 ** 64, dtype=np.uint64))
    words = tuple(int(np.uint32(v).astype(np.int32)) for v in (key & 0xFFFFFFFF, key >> 32))
    box = (0, 0, 0, 0, 0, 0)
    if float(rng.random()) < e.prob:
        for _ in range(ERASE_ATTEMPTS):
            area = h * w * float(rng.uniform(e.scale[0], e.scale[1]))
            r = math.exp(float(rng.uniform(math.log(e.ratio[0]), math.log(e.ratio[1]))))
            bh, bw = int(round(math.sqrt(area * r))), int(round(math.sqrt(area / r)))
            if 0 < bh < h and 0 < bw < w:
                y0, x0 = int(rng.integers(h - bh + 1)), int(rng.integers(w - bw + 1))
                n = max(1, int(round(fpc * float(rng.uniform(e.frames[0], e.frames[1])))))
                t0 = int(rng.integers(fpc - n + 1))
                box = (t0, t0 + n, y0, y0 + bh, x0, x0 + bw)
                break
    return box + words


def erase_table(cfg, draw_index, rank, batch, fpc, h, w, boxes=None, clips=None):
    """int32 [clips][8]: erase_row of the global clips rank * batch + i, i < clips (default: batch), of a rank whose batch holds up to
    `batch` clips; boxes (check_erase_boxes) replace the drawn boxes and leave the keys."""
    clips = int(batch) if clips is None else int(clips)
    rows = [erase_row(cfg, draw_index, int(rank) * int(batch) + i, fpc, h, w) for i in range(clips)]
    if boxes is not None:
        rows = [tuple(box) + row[6:] for box, row in zip(boxes, rows)]
    return np.array(rows, np.int32).reshape(clips, 8)


def dropout_seed(draw_index):
    """The seed of every dropout launch of the step with this draw index (LRCNEngine._draw_index); the _st launches of a captured
    step form the same value on the device from the step state's count."""
    return (int(draw_index) << 20) ^ 0x5DEECE66D


FC_DROPOUT_LAYERS = ("fc6", "fc7")


def fc_dropout_salt(cfg: NetConfig, layer):
    """The salt of one fc layer's masks (vl_fc_dropout_fwd): fc6 and fc7 of one tower differ in the low bit, towers in the bits above
    it (cfg.fc_dropout_salt: 0 for an LRCNEngine of its own, 1 + the node index inside a GraphEngine)."""
    return ((int(cfg.fc_dropout_salt) << 1) | FC_DROPOUT_LAYERS.index(layer)) & 0xFFFFFFFF


def check_accumulate(accumulate):
    """The micro-batches per update of a run as an int, None read as 1 (off).  Refused: bools, strings, floats that are not whole,
    values < 1."""
    if accumulate is None:
        return 1
    bad = isinstance(accumulate, (bool, np.bool_, str, bytes)) or not isinstance(accumulate, (int, float, np.integer, np.floating))
    if bad or not math.isfinite(accumulate) or accumulate != int(accumulate) or int(accumulate) < 1:
        raise VltfError("accumulate must be a whole number >= 1, got %r" % (accumulate,))
    return int(accumulate)


def check_tensor_stats_interval(interval):
    """Updates between two per-variable statistics launches as an int, None or 0 read as 0 (off).  Refused: bools, strings, floats,
    negative values -- anything but a whole number >= 1."""
    if interval is None:
        return 0
    if isinstance(interval, (bool, np.bool_)) or not isinstance(interval, (int, np.integer)) or int(interval) < 0:
        raise VltfError("tensor_stats_interval must be an integer >= 1 (None or 0 = off), got %r" % (interval,))
    return int(interval)


class MicroSequence:
    """The order of the micro-steps of accumulated updates, shared by both engines: train_step_*(micro=(i, k)) calls must come as
    (0, k), (1, k) .. (k - 1, k) with k <= limit; micro=None is the plain step and stands alone.  Anything else is refused, and a
    refusal abandons the group in progress: the next call must start one.  `rows` sums the rows of a group's calls on the host."""

    def __init__(self, limit):
        self.limit, self.next, self.rows = limit, None, 0

    def reset(self):
        self.next = None

    def open(self):
        """A group has begun and has not seen its final micro-step."""
        return self.next is not None

    def enter(self, micro):
        """Checks the call against the sequence and advances it; returns None (plain step) or (i, k)."""
        pending, self.next = self.next, None
        if micro is None:
            if pending is not None:
                raise VltfError("a plain step inside an accumulated update: micro-step %d of %d was due (the group is abandoned)" % pending)
            return None
        try:
            i, k = micro
            ok = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in (i, k))
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise VltfError("micro must be (i, k), two ints, got %r" % (micro,))
        i, k = int(i), int(k)
        if not (0 <= i < k <= self.limit):
            raise VltfError("micro = (%d, %d): need 0 <= i < k <= accumulate = %d" % (i, k, self.limit))
        if (i, k) != (pending or (0, k)):
            raise VltfError("micro = (%d, %d) is out of sequence: %s was due (the group is abandoned; start again at i = 0)" %
                            (i, k, "(%d, %d)" % pending if pending else "the first micro-step (0, k)"))
        if i < k - 1:
            self.next = (i + 1, k)
        return i, k

    def add_rows(self, mi, rows):
        """Rows of the update so far, this call's included."""
        if mi is None:
            return rows
        self.rows = rows + (self.rows if mi[0] else 0)
        return self.rows

    @staticmethod
    def role(mi):
        """(launch sequence of the call, k): the micro part of a captured step's key."""
        if mi is None or mi[1] == 1:
            return "single", 1
        i, k = mi
        return ("first" if i == 0 else "last" if i == k - 1 else "middle"), k


def decay_ranges(specs, plan, weight_decay):
    """[(begin, end, decay)] for ops.l2_regularize: every trainable range of plan.tiers cut at the variable extents of specs, decay =
    weight_decay for a variable of rank >= 2 (conv / fc weights, LSTM kernels, the fc heads) and 0 for rank 1 (every bias), adjacent
    entries with one coefficient merged.  Frozen variables lie outside plan.tiers and so outside every entry: never read, never
    written, not in the regulariser.  Host only."""
    d = check_weight_decay(weight_decay)
    out, off = [], 0
    for _, shp in specs:
        n = int(np.prod(shp))
        c = d if len(shp) >= 2 else 0.0
        for lo, hi, _ in plan.tiers:
            a, b = max(lo, off), min(hi, off + n)
            if b <= a:
                continue
            if out and out[-1][1] == a and out[-1][2] == c:
                out[-1] = (out[-1][0], b, c)
            else:
                out.append((a, b, c))
        off += n
    if len(out) > MAX_DECAY_RANGES:
        raise VltfError("this model needs %d weight-decay ranges (runs of weights and of biases in the flat parameter buffer, frozen "
                        "ranges between them); the regulariser kernel takes %d" % (len(out), MAX_DECAY_RANGES))
    return out


def stat_segments(specs, plan):
    """[(name, begin, end)] for ops.tensor_stats: every variable of specs that lies inside plan.tiers, in flat order, one segment per
    variable, nothing merged.  Frozen variables lie outside plan.tiers and are absent: their range of g is never read.  Host only."""
    out, off = [], 0
    for name, shp in specs:
        n = int(np.prod(shp))
        if n > 0 and any(lo <= off and off + n <= hi for lo, hi, _ in plan.tiers):
            out.append((name, off, off + n))
        off += n
    return out


def lars_ranges(specs, plan, weight_decay):
    """The tables of a LARS update, host only: (ranges, segments, decays).
    ranges   [(begin, end, lr_mult, trust_index)] for ops.lars_apply: every variable of specs inside plan.tiers, in flat order, with its
             tier's factor.  A variable of rank >= 2 is an entry of its own whose trust_index counts those variables from 0; variables of
             rank 1 (every bias: TF's skip_list, the exemption decay_ranges makes) get -1, adjacent ones with one factor merged.
    segments [(name, begin, end)] for ops.tensor_stats: the entries with a trust index, in that order -- biases need no norms.
    decays   the coefficient decay_ranges gives each of them (weight_decay, or 0 when it is off).
    Frozen variables lie outside plan.tiers and are absent from all three."""
    d = check_weight_decay(weight_decay)
    ranges, segs, decays, off = [], [], [], 0
    for name, shp in specs:
        n = int(np.prod(shp))
        mult = next((float(m) for lo, hi, m in plan.tiers if lo <= off and off + n <= hi), None)
        if n > 0 and mult is not None:
            if len(shp) >= 2:
                ranges.append((off, off + n, mult, len(segs)))
                segs.append((name, off, off + n))
                decays.append(d)
            elif ranges and ranges[-1][3] == -1 and ranges[-1][1] == off and ranges[-1][2] == mult:
                ranges[-1] = (ranges[-1][0], off + n, mult, -1)
            else:
                ranges.append((off, off + n, mult, -1))
        off += n
    return ranges, segs, decays


def lamb_ranges(specs, plan, weight_decay):
    """The tables of a LAMB update, host only: (ranges, segments).
    ranges   [(begin, end, lr_mult, decay, trust_index)] for ops.lamb_moments / ops.lamb_apply: every variable of specs inside
             plan.tiers, in flat order, with its tier's factor.  A variable of rank >= 2 is an entry of its own with the coefficient
             decay_ranges gives it (weight_decay, or 0 when it is off) and a trust_index that counts those variables from 0; variables of
             rank 1 (every bias) get decay 0 and index -1, adjacent ones with one factor merged -- lars_ranges' rules.
    segments [(name, begin, end)]: the entries with a trust index, in that order.
    Frozen variables lie outside plan.tiers and are absent from both."""
    d = check_weight_decay(weight_decay)
    ranges, segs, off = [], [], 0
    for name, shp in specs:
        n = int(np.prod(shp))
        mult = next((float(m) for lo, hi, m in plan.tiers if lo <= off and off + n <= hi), None)
        if n > 0 and mult is not None:
            if len(shp) >= 2:
                ranges.append((off, off + n, mult, d, len(segs)))
                segs.append((name, off, off + n))
            elif ranges and ranges[-1][4] == -1 and ranges[-1][1] == off and ranges[-1][2] == mult:
                ranges[-1] = (ranges[-1][0], off + n, mult, 0.0, -1)
            else:
                ranges.append((off, off + n, mult, 0.0, -1))
        off += n
    return ranges, segs


def clip_scale_of(sumsq, clip_norm):
    """The factor the update applies to the gradient: clip_norm / max(sqrt(sumsq), clip_norm), or 1 without a clip."""
    if not clip_norm or clip_norm <= 0.0:
        return 1.0
    return float(clip_norm) / max(math.sqrt(sumsq), float(clip_norm))


def tensor_stats_report(segments, rows, tiers, lr, clip_norm, sumsq):
    """(OrderedDict {name: {...}}, grads_norm_mean) from the rows of ops.tensor_stats (ops.STAT_DTYPE records or mappings with those
    fields), one per entry of segments [(name, begin, end)].  tiers: plan.tiers, whose factor is the variable's lr_mult; lr, clip_norm
    and sumsq (the global sum of squares the update reads) are those of the step.  mean and std are over the finite elements; std =
    sqrt(max(sumsq / n - mean^2, 0)).  sgd_update_ratio = lr * lr_mult * clip_scale * grad_norm / weight_norm is the plain-SGD figure
    whatever the optimizer, None when weight_norm is 0.  grads_norm_mean is the mean over the variables of clip_scale * grad_norm (the
    reference's `grads_norm`, train.py:215-222, taken of the clipped gradients).  Host only."""
    scale = clip_scale_of(sumsq, clip_norm)
    out, norms = collections.OrderedDict(), []
    for (name, lo, hi), r in zip(segments, rows):
        n = hi - lo
        mult = next((float(m) for a, b, m in tiers if a <= lo and hi <= b), 1.0)
        d = {}
        for key, p, bad in (("grad", "g", int(r["g_nonfinite"])), ("weight", "w", int(r["w_nonfinite"]))):
            s, q, fin = float(r[p + "_sum"]), float(r[p + "_sumsq"]), n - bad
            mean = s / fin if fin else float("nan")
            d[key + "_norm"] = math.sqrt(q)
            d[key + "_mean"] = mean
            d[key + "_std"] = math.sqrt(max(q / fin - mean * mean, 0.0)) if fin else float("nan")
            d[key + "_min"], d[key + "_max"] = float(r[p + "_min"]), float(r[p + "_max"])
            d[key + "_nonfinite"] = bad
        d["grad_zero_fraction"] = int(r["g_zero"]) / n
        d["lr_mult"] = mult
        d["sgd_update_ratio"] = lr * mult * scale * d["grad_norm"] / d["weight_norm"] if d["weight_norm"] > 0.0 else None
        out[name] = d
        norms.append(scale * d["grad_norm"])
    return out, (sum(norms) / len(norms) if norms else float("nan"))


def base_grad_chunks(cfg: NetConfig):
    """[(offset, count)] of the flat gradient in the order backward completes them, for a model with nothing frozen (dp.py).
    fc6W (85 % of the bytes) goes in FC6_CHUNKS row blocks, each reduced as soon as the GEMM that produces it is queued; also returns
    those row blocks [(row0, row1)]."""
    specs = param_specs(cfg)
    offsets, off = {}, 0
    for name, shp in specs:
        offsets[name] = off
        off += int(np.prod(shp))
    total = off
    first_conv = offsets["dcnn/conv5W"]
    f6o = offsets["dcnn/fc6W"]
    rows6 = dict(specs)["dcnn/fc6W"][0]
    nch = max(1, min(FC6_CHUNKS, rows6 // 128))
    edges = [(-(-rows6 * i // nch) + 127) // 128 * 128 if 0 < i < nch else (0 if i == 0 else rows6) for i in range(nch + 1)]
    row_blocks = [(edges[i], edges[i + 1]) for i in range(nch) if edges[i + 1] > edges[i]]
    chunks = [(0, f6o)] if f6o > 0 else []
    for bi, (r0, r1) in enumerate(row_blocks):
        lo, hi = f6o + r0 * FC_DIM, f6o + r1 * FC_DIM
        if bi == len(row_blocks) - 1:
            hi = first_conv                                   # fc6b rides with the last block
        chunks.append((lo, hi - lo))
    # conv5..conv3 (8.0 of the 9.3 MB of conv gradients) go out as soon as conv3's weight gradient is queued, while conv2 / conv1
    # backward (40 % of the conv backward) still runs; only conv2 + conv1 (1.4 MB) are left for the end of the step
    conv_lo = offsets["dcnn/conv2W"]
    chunks.append((first_conv, conv_lo - first_conv))
    chunks.append((conv_lo, total - conv_lo))
    assert sum(c for _, c in chunks) == total and all(chunks[i][0] + chunks[i][1] == chunks[i + 1][0] for i in range(len(chunks) - 1))
    return chunks, row_blocks


@dataclass
class TrainPlan:
    tiers: list             # [(begin, end, lr_mult)]: the trainable ranges of the flat buffer, sorted, adjacent equal factors merged
    frozen: list            # names of the variables that are never updated, in flat order
    chunks: list            # [(offset, count)]: the data-parallel exchange, covering exactly the trainable ranges
    total: int              # elements of the flat buffer

    def full_range(self):
        """One tier over everything with factor 1: the plain norm / update calls apply (and keep their bits)."""
        return self.tiers == [(0, self.total, 1.0)]

    def trainable_bytes(self):
        return 4 * sum(c for _, c in self.chunks)


def tier_plan(specs, frozen, lr_mult, base_chunks):
    """The plan of any variable list: specs [(name, shape)] in flat order, frozen variable names, the factor of the modified
    variables, and the exchange chunks of the unfrozen model.  A chunk keeps its boundaries wherever its range is still trainable and is
    cut to the trainable part otherwise, in the same order: with nothing frozen the chunk list is base_chunks item for item."""
    m = check_lr_mult(lr_mult)
    frozen = set(frozen)
    tiers, spans, off = [], [], 0
    for name, shp in specs:
        n = int(np.prod(shp))
        if name not in frozen:
            f = 1.0 if is_regular(name) else m
            if tiers and tiers[-1][1] == off and tiers[-1][2] == f:
                tiers[-1] = (tiers[-1][0], off + n, f)
            else:
                tiers.append((off, off + n, f))
            if spans and spans[-1][1] == off:
                spans[-1] = (spans[-1][0], off + n)
            else:
                spans.append((off, off + n))
        off += n
    chunks = []
    for lo, cnt in base_chunks:
        for a, b in spans:
            x, y = max(lo, a), min(lo + cnt, b)
            if y > x:
                chunks.append((x, y - x))
    return TrainPlan(tiers, [n for n, _ in specs if n in frozen], chunks, off)


def finetune_plan(cfg: NetConfig):
    """TrainPlan of a one-pipeline model from its config alone (no device): cfg.lr_mult sorts the variables into two learning-rate
    tiers, cfg.train_from freezes the dcnn layers before it."""
    layers = frozen_layers(cfg)
    frozen = ["dcnn/%s%s" % (l, k) for l in layers for k in ("W", "b")]
    return tier_plan(param_specs(cfg), frozen, cfg.lr_mult, base_grad_chunks(cfg)[0])


def init_params(cfg: NetConfig, seed=0, stddev=0.05, well_scaled=False):
    """Reference initialisers: W ~ truncated_normal(sigma=0.05) re-drawn beyond 2 sigma, b = 0.1
    (alexnet.py:40-46, tf_util.py:44-45); LSTM kernel glorot-uniform, bias 0 (TF defaults).
    well_scaled uses sigma = sqrt(2/fan_in) instead so activations stay O(1)."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, shp in param_specs(cfg):
        if name.endswith("conv_kernel") and len(shp) == 3:        # Keras' Conv1D fans: taps x in, taps x out
            lim = math.sqrt(6.0 / (shp[0] * shp[1] + shp[0] * shp[2]))
            out[name] = rng.uniform(-lim, lim, shp).astype(np.float32)
        elif name.endswith("kernel") or name.endswith("attention_pool/context") or name.endswith("netvlad/centers"):
            lim = math.sqrt(6.0 / (shp[0] + shp[1]))
            out[name] = rng.uniform(-lim, lim, shp).astype(np.float32)
        elif name.endswith("bias") or name.endswith("beta"):
            out[name] = np.zeros(shp, np.float32)
        elif name.endswith("gamma"):
            out[name] = np.ones(shp, np.float32)
        elif len(shp) > 1:
            sd = math.sqrt(2.0 / int(np.prod(shp[:-1]))) if well_scaled else stddev
            v = rng.standard_normal(shp)
            bad = np.abs(v) > 2.0
            while bad.any():
                v[bad] = rng.standard_normal(int(bad.sum()))
                bad = np.abs(v) > 2.0
            out[name] = (v * sd).astype(np.float32)
        else:
            out[name] = np.full(shp, 0.1, np.float32)
    return out


class LRCNEngine:
    """NetConfig.step_graph: train_step_u8 and forward_u8 run the first call of each input key (kind, frame count, raw frame shape,
    resize chain, crop / mirror / mean given, clip_norm, loss scale, dropout) eagerly, capture the second as a hipGraph
    (torch.cuda.graph, thread-local capture mode: the feeder uploads from its own thread meanwhile) and replay it from then on.  A
    graph reads its inputs from static device buffers and its per-step scalars (lr, the step count behind Adam's bias correction
    and the dropout seed, the origin of its LSTM exchange tags) from a device block (vl_step_state): before each replay the host
    copies the caller's tensors into the buffers, writes the block (ops.step_state_set) and replays.  Its LSTM launches run on a
    workspace of their own (lstm_ws_graph) whose tag stream the engine keeps: graph_tag_next, advanced by the graph's span per
    replay.  The host step_count stays the only count (checkpoints, load_opt_state).  Not with data parallelism, not with a probe.
    With NetConfig.accumulate > 1 the key also holds the micro-step's role (first / middle / last / single) and k: three launch sequences,
    three graphs; the state's count is then the dropout draw index and Adam's step size follows step_count (ops.step_state_set_micro).
    With NetConfig.tensor_stats_interval > 0 the key also holds whether the update is a stats step (_stats_due): two launch sequences.
    With NetConfig.ema_decay > 0 the captured update is followed by the weight average's launch, which reads its rate from the block:
    ops.step_state_set_ema writes it (engine.ema_rate of the host's step_count) before every replay that applies an update.
    With NetConfig.mixup_alpha > 0 the captured step holds the blend and the mixed-label loss launch; both read the blend weight from
    a one-float device word (mix_lam) the host fills before every step, eager or replayed (_mix_write): the block stays as it is.
    With NetConfig.cutmix_alpha > 0 the captured step holds the box swap too, which reads its six-int32 box (cut_box) the same way.
    With NetConfig.erase_prob > 0 it holds the erase launch ahead of both, which reads its int32 [max_clips][8] table (erase_table,
    _erase_write) the same way."""
    FC6_CHUNKS = FC6_CHUNKS
    GRAPH_TAG_LIMIT = 0xFFF00000    # tags of lstm_ws_graph stay below this (the eager counter's limit, csrc/lstm_cluster.hip)

    def __init__(self, cfg: NetConfig, max_clips: int, device="cuda:0", training=True, dp=None, flat=None):
        """flat: optional (w, g) slices of a larger flat parameter / gradient buffer to live in (vltf_amd.composed: several
        pipelines share one buffer so that the global-norm clip and the update run over all of them at once)."""
        if not torch.cuda.is_available():
            raise VltfError("LRCNEngine needs a HIP device; there is no CPU fallback")
        if cfg.step_graph and dp is not None:
            raise VltfError("step_graph is refused with data parallelism: capturing the gradient exchange's collectives is unmeasured "
                            "on this stack")
        self.momentum, self.nesterov = check_momentum(cfg.optimizer, cfg.momentum, cfg.nesterov)
        self.weight_decay = check_weight_decay(cfg.weight_decay)
        self.accumulate = check_accumulate(cfg.accumulate)
        self.ema_decay, self.ema_warmup = check_ema(cfg.ema_decay, cfg.ema_warmup)
        self.lars_eeta, self.lars_epsilon = check_lars(cfg.optimizer, self.momentum, cfg.lars_eeta, cfg.lars_epsilon)
        self.lamb_on, self.lamb_epsilon = check_lamb(cfg.optimizer, cfg.lamb, cfg.lamb_epsilon)
        if self.lamb_on and cfg.classifier == "none":
            raise VltfError("a feature pipeline (classifier none) has no step of its own: give lamb to the GraphEngine it trains in")
        if self.lars_eeta > 0.0 and cfg.classifier == "none":
            raise VltfError("a feature pipeline (classifier none) has no step of its own: give lars_eeta to the GraphEngine it trains in")
        if self.ema_decay > 0.0 and cfg.classifier == "none":
            raise VltfError("a feature pipeline (classifier none) has no step of its own: give ema_decay to the GraphEngine it trains in")
        self.fc_keep = check_fc_dropout(cfg.fc_dropout_keep_prob)      # 0: off; 1: on paper only, nothing is launched
        self.cfg, self.B, self.T = cfg, max_clips, cfg.fpc
        self.N = max_clips * cfg.fpc
        self.dev = torch.device(device)
        self.training = training
        self.dp = dp
        self.step_count = 0
        torch.cuda.set_device(self.dev)
        N, dev = self.N, self.dev

        def buf(*shape, dtype=torch.float32):
            return torch.empty(shape, dtype=dtype, device=dev)

        # ---- parameters: flat buffers + named views
        self.specs = param_specs(cfg)
        total = sum(int(np.prod(s)) for _, s in self.specs)
        if flat is not None:
            self.w, self.g = flat
            if self.w.numel() != total or (training and self.g.numel() != total):
                raise VltfError("flat parameter buffer has %d elements, the network needs %d" % (self.w.numel(), total))
        else:
            self.w = torch.zeros(total, device=dev)
            self.g = torch.zeros(total, device=dev) if training else None
        self.P, self.G, self.offsets = {}, {}, {}
        off = 0
        for name, shp in self.specs:
            n = int(np.prod(shp))
            self.P[name] = self.w[off:off + n].view(shp)
            if training:
                self.G[name] = self.g[off:off + n].view(shp)
            self.offsets[name] = (off, n)
            off += n
        # learning-rate tiers, frozen layers and the data-parallel exchange's chunks (finetune_plan): with nothing frozen the chunks
        # are those of base_grad_chunks, in the order backward completes them
        self.fc6_row_blocks = base_grad_chunks(cfg)[1]
        self.plan = finetune_plan(cfg)
        self.grad_chunks = self.plan.chunks
        cut = len(frozen_layers(cfg))                          # dcnn layers [0, cut) are frozen: conv1..conv5, fc6, (fc7), (fc8)
        self.first_conv = min(cut, len(CONV_LAYERS))           # first trainable conv layer; 5: the conv stack is frozen
        self.fc_trains = {l: i >= cut for i, l in enumerate(dcnn_layers(cfg))}
        self.dcnn_trains = cut < len(dcnn_layers(cfg))         # False: no gradient goes down into the tower at all
        if training and cfg.classifier != "none" and not self.plan.tiers:
            raise VltfError("train_from [%s] leaves this model nothing to train" % cfg.train_from)
        if cfg.optimizer == "adam" and training:
            self.adam_m, self.adam_v = torch.zeros(total, device=dev), torch.zeros(total, device=dev)
        self.mom = torch.zeros(total, device=dev) if self.momentum > 0.0 and training else None    # the momentum accumulator
        # gradient accumulation (train_step_*(micro=(i, k))): the running sum of an update's micro-step gradients.  Written by the first
        # micro-step's store over plan.tiers, so it needs no fill; frozen ranges are never touched.  Allocated here, never in a capture.
        self.gacc = torch.empty(total, device=dev) if self.accumulate > 1 and training else None
        # the weight average's shadow (ema_decay): a copy of the whole flat w from the moment the weights are set (load_params) until the
        # first update; each update then averages the trained ranges only, so a frozen range stays equal to its weights.
        self.ema = torch.zeros(total, device=dev) if self.ema_decay > 0.0 and training else None
        self.micro = MicroSequence(self.accumulate)
        self._mi = None                       # the (i, k) of the train step being issued; None: a plain step

        # ---- conv stack plan.  Tensors a conv gathers from (its x, and the dy its dgrad reads) are stored
        # with a zero halo equal to the conv's SAME padding, so the im2col gather is test-free (vltf.h).
        def zbuf(n_, c_, h_, w_, halo, dtype=torch.float32):
            return torch.zeros((n_, c_, h_ + 2 * halo, w_ + 2 * halo), dtype=dtype, device=dev)

        h, w, c = cfg.image_shape
        convs = []
        for name, kh, kw, co, s, g, lrn, pool in CONV_LAYERS:
            conv = ops.Conv(c, h, w, co, kh, kw, s, g)
            convs.append(conv)
            h, w, c = conv.oh, conv.ow, co
            if pool:
                h, w = ops.pool_out(h), ops.pool_out(w)
        pads = [cv.same_pad() for cv in convs]
        h, w, c = cfg.image_shape
        self.x0_halo = pads[0]
        # conv1 is strided: its input is stored column-phase-split so that the taps of consecutive output columns are
        # consecutive addresses (vl_conv_set_x_phase_split); x0 is only ever read by conv1 (forward and wgrad)
        convs[0].set_halo(pads[0], 0, 0, 0)
        self.x0_phase = convs[0].set_x_phase_split(True) if pads[0] > 0 else 1
        self.x0 = torch.zeros(ops.phase_split_shape(N, c, h, w, self.x0_halo, self.x0_phase), device=dev)
        self.layers = []
        max_w = 0
        ws_bytes = 4
        for li, (name, kh, kw, co, s, g, lrn, pool) in enumerate(CONV_LAYERS):
            conv = convs[li]
            nxt = pads[li + 1] if li + 1 < len(convs) else 0
            L = dict(name=name, conv=conv, lrn=lrn, pool=pool, cin=c, h=h, w=w)
            L["x_halo"] = pads[li]
            L["y_halo"] = 0 if (lrn or pool) else nxt            # y feeds the next conv directly (conv3, conv4)
            L["dy_halo"] = pads[li] if li > 0 else 0             # dy is gathered by this layer's dgrad (not conv1)
            L["y"] = zbuf(N, co, conv.oh, conv.ow, L["y_halo"])
            if training:
                L["dy"] = zbuf(N, co, conv.oh, conv.ow, L["dy_halo"])
            out, out_halo = L["y"], L["y_halo"]
            h, w, c = conv.oh, conv.ow, co
            if pool:
                ph, pw = ops.pool_out(h), ops.pool_out(w)
                L["hwc"] = name == "conv5"       # pool5 writes the (h, w, c)-flat order fc6 reads (alexnet.py:228)
                L["p_halo"] = 0 if L["hwc"] else nxt
                L["p"] = buf(N, ph, pw, c) if L["hwc"] else zbuf(N, c, ph, pw, L["p_halo"])
                L["arg"] = torch.zeros(L["p"].shape, dtype=torch.uint8, device=dev)
                if training:
                    L["dp"] = buf(N, ph, pw, c) if L["hwc"] else zbuf(N, c, ph, pw, L["p_halo"])   # same layout as p / arg
                out, out_halo = L["p"], L["p_halo"]
                h, w = ph, pw
            L["out"], L["out_halo"] = out, out_halo
            max_w = max(max_w, kh * kw * (conv.cin // g) * co)
            self.layers.append(L)
        for li, L in enumerate(self.layers):
            prev = self.layers[li - 1] if li > 0 else None
            dx_halo = 0
            if prev is not None:                                 # dgrad writes into the previous layer's dp (pool) or dy
                dx_halo = prev["p_halo"] if prev["pool"] else prev["dy_halo"]
            L["conv"].set_halo(L["x_halo"], L["y_halo"], L["dy_halo"], dx_halo)
            if training:
                ws_bytes = max(ws_bytes, L["conv"].wgrad_ws_bytes(N))
        # conv_math "bf16" is a bf16 PATH for the stride-1 layers (csrc/conv_c8.hip): their operands live in memory as packed bf16
        # ("c8": 8 channels of a pixel per 16-byte chunk) next to the fp32 tensors the pool / LRN / bias-gradient kernels read.
        # xb: the layer's input; dyb: the gradient its dgrad / wgrad read; wb / wbt: the packed weights (rebuilt every step).
        self.c8 = cfg.conv_math == "bf16"
        self._xb_fed = False                          # feed_u8 wrote conv1's packed input directly
        if self.c8:
            def cbuf(c_, h_, w_, halo):
                return torch.zeros(ops.c8_shape(N, c_, h_, w_, halo), dtype=torch.bfloat16, device=dev)
            for L in self.layers[1:]:
                conv = L["conv"]
                L["xb"] = cbuf(conv.cin, conv.h, conv.w, L["x_halo"])
                L["wb"] = torch.zeros(conv.c8_w_bytes(False), dtype=torch.uint8, device=dev)
                if training:
                    L["dyb"] = cbuf(conv.cout, conv.oh, conv.ow, L["dy_halo"])
                    L["wbt"] = torch.zeros(conv.c8_w_bytes(True), dtype=torch.uint8, device=dev)
                    ws_bytes = max(ws_bytes, conv.c8_wgrad_ws_bytes(N))
            # the LRN layers' conv outputs are written packed only (no halo): lrn_pool_fwd_c8 / pool_lrn_bwd_c8 read them packed
            for L in self.layers:
                if L["lrn"] and L["pool"]:
                    L["yb"] = cbuf(L["conv"].cout, L["conv"].oh, L["conv"].ow, 0)
            # conv1 (strided, 3 channels) runs the same kernels as the equivalent stride-1 layer over its space-to-depth input
            L0 = self.layers[0]
            eq = L0["eq"] = L0["conv"].s2d_layer()
            L0["xb"] = cbuf(eq.cin, eq.h, eq.w, eq.x_halo)
            L0["ws2d"] = torch.zeros(eq.w_shape, device=dev)
            L0["wb"] = torch.zeros(eq.c8_w_bytes(False), dtype=torch.uint8, device=dev)
            if training:
                L0["dyb"] = cbuf(eq.cout, eq.oh, eq.ow, eq.dy_halo)
                L0["dws2d"] = torch.zeros(eq.w_shape, device=dev)
                ws_bytes = max(ws_bytes, eq.c8_wgrad_ws_bytes(N))
        self.flat_dim = h * w * c
        if self.c8 and N % 8 == 0 and os.environ.get("VLTF_FC6_KC8", "1") != "0":      # (0: A/B against the split-product GEMM)
            # fc6's three products on the wgrad kernel (ops.gemm_kc8: reduction-major packed operands), DESIGN 4.7
            F = self.flat_dim
            kb = lambda count: torch.zeros(count, dtype=torch.bfloat16, device=dev)
            self.k_act = kb(N * max(F, FC_DIM))            # the activation operand of the forward / input-gradient product
            self.k_w = kb(F * FC_DIM)                      # fc6W, reduction-major for the forward, then for the input gradient
            if training:
                self.k_p5, self.k_d6 = kb(N * F), kb(N * FC_DIM)
            H4_, D_ = 4 * cfg.lstm_hidden, cfg.encode_dim()
            for (gm, gn, gk) in ((N, FC_DIM, F), (N, F, FC_DIM), (F, FC_DIM, N), (N, H4_, D_), (D_, H4_, N), (N, D_, H4_)):
                ws_bytes = max(ws_bytes, ops.gemm_kc8_ws_bytes(gm, gn, gk))
        self.f6 = buf(N, FC_DIM)
        self.f7 = buf(N, FC_DIM) if cfg.frame_encoding_layer != "fc6" else None
        self.f8 = buf(N, cfg.num_classes) if cfg.frame_encoding_layer not in ("fc6", "fc7") else None
        self.feat = self.f8 if self.f8 is not None else (self.f7 if self.f7 is not None else self.f6)
        D, C, H, B, T = cfg.encode_dim(), cfg.num_classes, cfg.lstm_hidden, self.B, self.T
        if cfg.conv_math != "f32":                                # operand images of the split-product GEMMs (fc6 is the largest)
            for (gm, gn, gk) in ((N, FC_DIM, self.flat_dim), (N, self.flat_dim, FC_DIM), (self.flat_dim, FC_DIM, N), (N, 4 * H, D)):
                ws_bytes = max(ws_bytes, ops.gemm_split_ws_bytes(gm, gn, gk))
        self.ws = torch.empty(max(ws_bytes, 64 << 20) // 4, device=dev)       # wgrad slabs / split-K slabs / GEMM operand images
        # rnn_cell mhsa: (heads, positions) of the self-attention layers, else None (refusals: param_specs -> check_mhsa)
        self.sa = check_mhsa(cfg.rnn_cell, H, T, cfg.sa_heads, cfg.sa_positions, cfg.fusion) if cfg.classifier == "lstm" else None
        # sa_block encoder: the feed-forward width of the blocks, else None (refusals: param_specs -> check_mhsa -> check_sa_block)
        self.sa_ffn = check_sa_block(cfg.rnn_cell, H, cfg.sa_block, cfg.sa_ffn_dim) if self.sa else None
        # sa_attn_dropout / sa_dropout / sa_drop_path: what a TRAINING forward draws with, else None (refusals: param_specs -> check_mhsa)
        self.sa_drop = sa_drop_of(cfg, cfg.lstm_layers) if self.sa and training else None
        # rnn_cell tcn: (k, dilations, causal) of the convolution stack, else None (refusals: param_specs -> check_tcn)
        self.tc = None
        if cfg.classifier == "lstm":
            tc = check_tcn(cfg.rnn_cell, H, cfg.lstm_layers, cfg.tcn_kernel, cfg.tcn_dilation, cfg.tcn_causal, cfg.fusion)
            self.tc = (tc[0], tcn_dilations(tc[1], cfg.lstm_layers), tc[2]) if tc else None
        self._sa_drop = None                                        # the SaDrop bound to the pass the last forward ran, for its backward
        # colsum / bias / sumsq partials (rnn_cell mhsa: the position bias's gradient is a column sum heads (2T - 1) wide, the
        # block's ffn1_bias F wide)
        # (fusion vlad: the centres' gradient is a column sum K HO wide)
        ho_ = (2 if cfg.lstm_bidirectional else 1) * H
        vlad_w = (check_vlad(cfg.fusion, cfg.vlad_clusters, cfg.classifier, ho_) or 0) * ho_ if cfg.classifier == "lstm" else 0
        self.small_ws = buf(64 * max(4 * H, FC_DIM, 1024, C, self.sa[0] * (2 * T - 1) if self.sa else 0, self.sa_ffn or 0, vlad_w))
        if training:
            self.wt = buf(max_w)
            self.df6 = buf(N, FC_DIM)
            self.df7 = buf(N, FC_DIM) if self.f7 is not None else None
            self.df8 = buf(N, C) if self.f8 is not None else None
            self.dfeat = self.df8 if self.df8 is not None else (self.df7 if self.df7 is not None else self.df6)
        # ---- classifier
        if cfg.classifier == "lstm":
            if cfg.fusion not in ops.FUSION_CODE and cfg.fusion not in ("state", "reshape", "attn", "vlad"):
                raise VltfError("Undefined frame fusion type : %s" % cfg.fusion)          # tf_util.py:28-29
            # `state` = final h of the last layer = its output at t = T-1 (full-length sequences, lstm.py:136), no dropout;
            # `reshape` (tf_util.py:26-27) keeps every step: one logits row per frame, labels [clips * fpc, classes]
            self.lstm_fusion = "last" if cfg.fusion == "state" else cfg.fusion
            self.per_step = cfg.fusion == "reshape"
            self.head = "fc_convert" if cfg.fusion == "state" else "output_fc"
            self.lstm, self.blstm, self.gru = [], [], []                # per-layer buffers: unidirectional, bidirectional or GRU layers
            self.bi = bool(cfg.lstm_bidirectional)
            self.is_gru = cfg.rnn_cell == "gru"                         # (refusals: param_specs -> check_rnn_cell)
            self.mhsa, self._mhsa_clips = [], 0                         # rnn_cell mhsa: self-attention layers (self.sa above)
            self.enc = None                                             # sa_block encoder: encoder_buffers; self.mhsa is then its layers
            if self.sa_ffn:
                self.enc = encoder_buffers(buf, N, T, H, self.sa_ffn, self.sa[0], self.sa[1], cfg.lstm_layers, training, self.sa_drop)
                self.mhsa = self.enc["layers"]
            self.tcn, self.tconv = None, []                             # rnn_cell tcn: tcn_buffers and its layers (self.tc above)
            if self.tc:
                self.tcn = tcn_buffers(buf, N, H, self.tc[0], cfg.lstm_layers, training)
                self.tconv = self.tcn["layers"]
            HO = self.lstm_out = 2 * H if self.bi else H                # width of a layer's output, of the fused vector and of the head's input
            if self.bi and ops.lstm_seq_bi_tag_span(1, 1, H) == 0:      # (H itself was checked by param_specs)
                raise VltfError("lstm_bidirectional: this device has too few compute units to hold both directions of hidden size %d in "
                                "one launch" % H)
            for l in range(cfg.lstm_layers):
                if self.bi:
                    self.blstm.append(blstm_buffers(buf, N, H, training))
                    continue
                if self.is_gru:
                    self.gru.append(gru_buffers(buf, N, H, training))
                    continue
                if self.sa_ffn or self.tc:
                    continue
                if self.sa:
                    self.mhsa.append(mhsa_buffers(buf, N, T, H, self.sa[0], self.sa[1], training))
                    continue
                S = dict(gx=buf(N, 4 * H), act=buf(N, 4 * H), cseq=buf(N, H), hseq=buf(N, H), hprev=buf(N, H))
                if training:
                    S.update(dz=buf(N, 4 * H), dout=buf(N, H))
                self.lstm.append(S)
            self.gh = buf(B, 4 * H)
            self.lstm_ws = ops.lstm_seq_ws(B, T, H, dev) if H <= 1024 else None
            R = N if self.per_step else B                             # logits rows
            # fusion vlad (check_vlad: param_specs): NetVLAD pooling; the fused vector and the head's input are K x HO wide
            self.vlad_k = check_vlad(cfg.fusion, cfg.vlad_clusters, cfg.classifier, HO)
            self.vlad = vlad_buffers(buf, B, T, HO, self.vlad_k, training) if self.vlad_k else None
            self._vlad_clips = 0
            HW = self.head_in = (self.vlad_k or 1) * HO               # width of the fused vector = the head's input
            self.fused = buf(R, HW)
            self.dropped = buf(R, HW)
            self.drop_mask = buf(R, HW, dtype=torch.uint8)
            self.logits = buf(R, C) if HW != C else self.dropped
            # fusion attn (check_attn: param_specs): learned attention pooling in the place of avg / last
            self.attn_dim = check_attn(cfg.fusion, cfg.attn_dim, cfg.classifier, HO)
            self.attn = attn_buffers(buf, B, T, HO, self.attn_dim, training) if self.attn_dim else None
            self._attn_clips = 0
            if training:
                self.dh, self.dc = buf(B, H), buf(B, H)
                self.dfused, self.ddropped = buf(R, HW), buf(R, HW)
                if self.bi:
                    self.dx_bw = buf(N, max(D, HO))                   # the backward direction's share of a layer's input gradient
        else:
            ff = cfg.frame_fusion
            if cfg.classifier == "none" and ff and ff[0] == "late":
                raise VltfError("Specified late fusion with no classifier selected")       # model.py:36-37
            if ff and ff[0] in ("early", "late") and ff[1] not in ("avg", "last", "reshape"):
                raise VltfError("Undefined frame fusion type : %s" % ff[1])              # apply_temporal_fusion, tf_util.py:28-29
            if ff and ff[1] == "reshape":
                ff = None        # aggregate_clip_vectors with `reshape` (tf_util.py:126-133,26-27): [N, d] -> [B, T, d] -> [N, d], the identity
            self.early = bool(ff and ff[0] == "early" and T > 1)
            self.late = bool(ff and ff[0] == "late" and T > 1)
            self.ff_method = ff[1] if ff else None
            C = cfg.out_dim()                  # a feature pipeline (classifier none) ends at the encode width: no fc, D == C below
            rows = B if self.early else N
            self.fc_in = buf(B, D) if self.early else self.feat
            self.fc_out = buf(rows, C) if D != C else self.fc_in
            self.logits = buf(B, C) if self.late else self.fc_out
            if training:
                self.dfc_out = buf(rows, C) if self.late else None
                self.dfc_in = buf(B, D) if self.early else None
        self.rows_out = self.logits.shape[0]
        if training:
            self.dlogits = buf(*self.logits.shape)
        self._loss_setup(cfg.label_smoothing, cfg.top_k, self.rows_out, cfg.class_weights, cfg.focal_gamma, label_type=cfg.label_type)
        self._mix_setup(cfg.mixup_alpha, cfg.mixup_seed, self.rows_out)
        self._erase_setup()
        self.ss = torch.zeros(1, device=dev)
        # L2 weight decay: ops.l2_regularize takes the norm's place in _finish_step and returns {sum g'^2, regulariser}; the update calls
        # and _fetch read the first word through self.ss.  Off: nothing is allocated, the norm calls are the ones of before.
        self.decay, self.ss2 = None, None
        if self.weight_decay > 0.0 and cfg.classifier == "none":
            raise VltfError("a feature pipeline (classifier none) has no step of its own: give weight_decay to the GraphEngine it trains in")
        if self.weight_decay > 0.0 and training and not self.lamb_on:      # under LAMB the decay is decoupled: it enters through u alone
            self.decay = decay_ranges(self.specs, self.plan, self.weight_decay)
            self.ss2 = torch.zeros(2, device=dev)
            self.ss = self.ss2[:1]
        if check_tensor_stats_interval(cfg.tensor_stats_interval) > 0 and cfg.classifier == "none":
            raise VltfError("a feature pipeline (classifier none) has no step of its own: give tensor_stats_interval to the GraphEngine "
                            "it trains in")
        self._stats_setup(cfg.tensor_stats_interval)
        self._lars_setup()
        self._lamb_setup()
        self._skip = torch.zeros(1, dtype=torch.int32, device=dev)      # ops.step_guard: the optimizer launch's skip word
        self.probe, self.probe_events = None, []
        self._resizers = {}
        self.mean_dev = torch.zeros(3, device=dev)
        # ---- captured steps (cfg.step_graph, class docstring)
        self.step_graph = cfg.step_graph
        self.lstm_ws_graph = None
        self._tag_off = None                  # while a step is being captured: the tag offset of its next LSTM launch
        if self.step_graph:
            self.state = ops.step_state(dev)
            if getattr(self, "lstm_ws", None) is not None:
                self.lstm_ws_graph = ops.lstm_seq_ws(B, T, H, dev)     # zeroed; never handed to an eager launch
            self.graph_tag_next = 1
            self._graphs, self._graph_warm = {}, set()
            self.graph_capture_ms = []

    # ---- live kernel timing (bench.py roofline): HIP events around labelled launches -------------
    def set_probe(self, labels):
        """labels: iterable of '<layer>.<fwd|dgrad|wgrad>' whose launches get bracketed by events
        recorded on the launch stream.  None disables."""
        if labels and self.step_graph:
            raise VltfError("step_graph is refused with a per-launch timing probe: a replayed graph has no launches to bracket")
        self.probe = set(labels) if labels else None
        self.probe_events = []

    def _run(self, label, fn, *args, **kw):
        if self.probe is not None and label in self.probe:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(*args, **kw)
            e1.record()
            self.probe_events.append((label, e0, e1))
        else:
            fn(*args, **kw)

    def probe_times_ms(self):
        torch.cuda.synchronize(self.dev)
        out = [(l, a.elapsed_time(b)) for l, a, b in self.probe_events]
        self.probe_events = []
        return out

    # ---- parameters ----------------------------------------------------------------------------
    def load_params(self, params: dict):
        """params: {tf variable name: numpy array in the reference layout}.  Unknown / missing names fail."""
        missing = [n for n, _ in self.specs if n not in params]
        extra = [n for n in params if n not in self.P]
        if missing or extra:
            raise VltfError("parameter set mismatch: missing %s, unexpected %s" % (missing, extra))
        for name, shp in self.specs:
            a = np.asarray(params[name], np.float32)
            if tuple(a.shape) != tuple(shp):
                raise VltfError("parameter %s has shape %s, expected %s" % (name, a.shape, shp))
            self.P[name].copy_(torch.from_numpy(np.ascontiguousarray(a)))
        self._ema_follow()

    def get_params(self):
        torch.cuda.synchronize(self.dev)
        return {n: self.P[n].detach().cpu().numpy().copy() for n, _ in self.specs}

    # ---- exponential moving average of the weights (ema_decay; shared with GraphEngine) ---------------------------------------------------
    def _ema_follow(self):
        """The weights were just set: before the first update the shadow starts as their copy (TF: a shadow variable is initialised with
        its variable's initial value)."""
        if getattr(self, "ema", None) is not None and self.step_count == 0:
            self.ema.copy_(self.w)

    def _ema_launch(self, skip):
        """_finish_step, right behind the optimizer launch (step_count already counts this update): one ranged launch over the trained
        ranges, under the update's skip word.  Captured: the rate comes from the step state (_graph_step writes it before the replay)."""
        if self.ema is None:
            return
        if getattr(self, "_tag_off", None) is not None:
            ops.ema_update_st(self.ema, self.w, self.state, skip=skip, ranges=self._acc_tiers())
        else:
            ops.ema_update(self.ema, self.w, ema_rate(self.ema_decay, self.ema_warmup, self.step_count - 1), skip=skip,
                           ranges=self._acc_tiers())

    def _ema_required(self):
        if getattr(self, "ema", None) is None:
            raise VltfError("this engine keeps no averaged weights (ema_decay is 0, or it was built with training=False)")
        return self.ema

    def _flat_f32(self, flat, what):
        a = np.asarray(flat, np.float32)
        if a.shape != (self.w.numel(),):
            raise VltfError("%s has shape %s, expected (%d,)" % (what, a.shape, self.w.numel()))
        return torch.from_numpy(np.ascontiguousarray(a))

    def get_ema_params(self):
        """{name: array} of the averaged weights, by the engine's specs (frozen variables: their weights)."""
        ema = self._ema_required()
        torch.cuda.synchronize(self.dev)
        flat = ema.detach().cpu().numpy()
        out, off = {}, 0
        for name, shp in self.specs:
            n = int(np.prod(shp))
            out[name] = flat[off:off + n].reshape(shp).copy()
            off += n
        return out

    def load_ema(self, flat):
        """Sets the shadow from a flat array of `count` floats (get_opt_state's __optimizer__/ema)."""
        self._ema_required().copy_(self._flat_f32(flat, "the averaged weights"))

    def use_ema_weights(self, flat):
        """Validation: a stored shadow (get_opt_state's __optimizer__/ema) becomes the weights of an engine built with training=False."""
        if self.training:
            raise VltfError("use_ema_weights is for an engine built with training=False: a training engine keeps its own shadow (load_ema)")
        self.w.copy_(self._flat_f32(flat, "the averaged weights"))

    def get_grads(self):
        torch.cuda.synchronize(self.dev)
        frozen = set(self.plan.frozen)                  # their range of g is never written: it holds nothing to hand out
        return {n: self.G[n].detach().cpu().numpy().copy() for n, _ in self.specs if n not in frozen}

    # ---- per-variable statistics (tensor_stats_interval; shared with GraphEngine) --------------------------------------------------------
    def _stats_setup(self, interval):
        """Off (None / 0, or an engine that does not train): nothing is allocated and no launch, graph key or result key changes.  On:
        one segment per trained variable (stat_segments), the rows and the chunk workspace of ops.tensor_stats and a word that keeps the
        stats step's global sum of squares -- allocated here, never inside a capture."""
        self.tensor_stats_interval = check_tensor_stats_interval(interval)
        self.stat_segs, self._stats_meta, self._stats_last = None, None, None
        if self.tensor_stats_interval > 0 and self.training:
            self.stat_segs = stat_segments(self.specs, self.plan)
            self.stat_out = torch.empty(len(self.stat_segs) * ops.STAT_ROW_BYTES, dtype=torch.uint8, device=self.dev)
            self.stat_ws = torch.empty(ops.tensor_stats_ws_bytes(self.stat_segs), dtype=torch.uint8, device=self.dev)
            self.stat_ss = torch.zeros(1, device=self.dev)

    def _stats_due(self):
        """The update about to be applied (0-based index step_count) is a stats step."""
        return self.stat_segs is not None and self.step_count % self.tensor_stats_interval == 0

    def _stats_launch(self, lr, clip_norm):
        """_finish_step, between the norm and the update: g is what the optimizer is about to consume (reduced over the ranks, summed over
        the micro-steps, regularised, not yet clipped), w what the forward pass used.  Read-only, so the skip word does not concern it."""
        ops.tensor_stats(self.w, self.g, self.stat_segs, self.stat_out, self.stat_ws)
        self.stat_ss.copy_(self.ss)               # the next step's norm overwrites self.ss; a caller with fetch=False may look later
        self._stats_note(lr, clip_norm)

    def _stats_note(self, lr, clip_norm):
        """Host side of a stats step: rows wait on the device for _stats_collect (a replayed step calls this with the replay's lr)."""
        self._stats_meta = dict(update=self.step_count, lr=float(lr), clip_norm=float(clip_norm or 0.0))

    def _stats_collect(self):
        """Reads the rows of the last stats step (the caller has synchronised) and derives the report."""
        meta, self._stats_meta = self._stats_meta, None
        rows = ops.stat_rows(self.stat_out, len(self.stat_segs))
        ss = float(self.stat_ss.item())
        stats, mean = tensor_stats_report(self.stat_segs, rows, self.plan.tiers, meta["lr"], meta["clip_norm"], ss)
        if getattr(self, "lars", None) is not None:          # the trust ratios of that update (kept by _lars_trust_launch)
            for name, t in self._lars_named(self.lars["stat_trust"]).items():
                stats[name]["lars_trust"] = t
        if getattr(self, "lamb", None) is not None:          # LAMB's, kept by _lamb_launch
            for name, t in self._lamb_named(self.lamb["stat_trust"]).items():
                stats[name]["lamb_trust"] = t
        self._stats_last = dict(update=meta["update"], tensor_stats=stats, grads_norm_mean=mean)
        return self._stats_last

    def _stats_result(self, out):
        """_fetch: the step just finished was a stats step -> its result gains tensor_stats and grads_norm_mean."""
        if self._stats_meta is not None and self._stats_meta["update"] == self.step_count - 1:
            st = self._stats_collect()
            out["tensor_stats"], out["grads_norm_mean"] = st["tensor_stats"], st["grads_norm_mean"]
        return out

    def tensor_stats(self):
        """The most recent stats step's {variable name: {...}} (tensor_stats_report), or None.  After a step with fetch=False it
        synchronises first."""
        if self._stats_meta is not None:
            torch.cuda.synchronize(self.dev)
            self._stats_collect()
        return None if self._stats_last is None else self._stats_last["tensor_stats"]

    # ---- label smoothing / top-k accuracy (label_smoothing, top_k; setup and fetch shared with GraphEngine) -------------------------------------
    def _loss_setup(self, label_smoothing, top_k, rows, class_weights=None, focal_gamma=0.0, num_classes=None, label_type="single"):
        """All off (or an engine that does not train: validation computes no loss): the two sums and the 2 * rows workspace of
        ops.softmax_xent, as ever.  Label smoothing or top-k on: three sums and 3 * rows, for ops.softmax_xent_ls.  Class weights or a
        focal gamma on (xent_wf): the same three columns, for ops.softmax_xent_wf, and the weights on the device
        (class_weights_dev; None = ones), read by the launch as it runs.  label_type "multiple" (DESIGN 4.26): always three sums and
        3 * rows, for ops.sigmoid_xent -- {loss, hit@1 rows, exact-match rows}; the smoothing, the focal gamma and the mixed labels go
        to that launch, the class weights are its positive-term weights, and top_k is refused (a multi-hot row has no one label to
        rank)."""
        self.label_smoothing, self.top_k = check_label_smoothing(label_smoothing), check_top_k(top_k)
        self.label_type = check_label_type(label_type)
        self.multilabel = self.label_type == "multiple"
        if self.multilabel and self.top_k > 0:
            raise VltfError("top_k = %d is refused with label_type multiple: a multi-hot row has no one label whose rank could be "
                            "counted (accuracy is hit@1, subset_accuracy the exact match)" % self.top_k)
        self.class_weights = check_class_weights(class_weights, self.cfg.num_classes if num_classes is None else num_classes)
        self.focal_gamma = check_focal_gamma(focal_gamma)
        if not self.training:
            self.label_smoothing, self.top_k, self.class_weights, self.focal_gamma = 0.0, 0, None, 0.0
        self.xent_ls = self.label_smoothing > 0.0 or self.top_k > 0
        self.xent_wf = self.class_weights is not None or self.focal_gamma > 0.0
        self.class_weights_dev = None if self.class_weights is None else torch.from_numpy(self.class_weights).to(self.dev)
        cols = 3 if self.xent_ls or self.xent_wf or self.multilabel else 2
        self.stats = torch.zeros(cols, device=self.dev)
        self.loss_rows = torch.zeros(cols * rows, device=self.dev)      # per-row losses | hits (| top-k hits): the loss launch's workspace

    def _xent_launch(self, logits, onehot, dlogits, grad_scale):
        """The loss launch of a train step: stats += {loss sum, hits (, top-k hits)}, dlogits = (softmax - labels') * grad_scale."""
        if self.multilabel:                       # multi-hot rows: sigmoids per class; stats += {loss sum, hit@1 rows, exact-match rows}
            ops.sigmoid_xent(logits, onehot, dlogits, self.stats, grad_scale, self.loss_rows, self.label_smoothing, self.class_weights_dev,
                             self.focal_gamma,
                             **({} if self.mix_lam is None else dict(rows_per_clip=self.rows_out // self.B, lam=self.mix_lam)))
        elif self.xent_wf:                        # class weights / focal loss, on mixed labels when mixup or CutMix is on
            ops.softmax_xent_wf(logits, onehot, dlogits, self.stats, grad_scale, self.loss_rows, self.label_smoothing, self.top_k,
                                self.class_weights_dev, self.focal_gamma,
                                **({} if self.mix_lam is None else dict(rows_per_clip=self.rows_out // self.B, lam=self.mix_lam)))
        elif self.mix_lam is not None:              # mixup: the labels of the blended clips, the weight read from the device
            ops.softmax_xent_mix(logits, onehot, dlogits, self.stats, grad_scale, self.loss_rows, self.rows_out // self.B,
                                 self.label_smoothing, self.top_k, self.mix_lam)
        elif self.xent_ls:
            ops.softmax_xent_ls(logits, onehot, dlogits, self.stats, grad_scale, self.loss_rows, self.label_smoothing, self.top_k)
        else:
            ops.softmax_xent(logits, onehot, dlogits, self.stats, grad_scale, self.loss_rows)

    def _fetch_topk(self, out, st, rows):
        """_fetch: with top_k > 0 the result gains the top-k accuracy of the rows so far and the count behind it."""
        if getattr(self, "top_k", 0) > 0:
            out["topk_accuracy"], out["topk_correct"] = float(st[2]) / max(rows, 1), float(st[2])
        if getattr(self, "multilabel", False):    # label_type multiple: `accuracy` is hit@1; the third sum counts the exact-match rows
            out["subset_accuracy"], out["subset_correct"] = float(st[2]) / max(rows, 1), float(st[2])
        return out

    # ---- mixup (mixup_alpha, mixup_seed) and CutMix / VideoMix (cutmix_*) -----------------------------------
    def _mix_setup(self, alpha, seed, rows):
        """Off (both alphas 0, or an engine that does not train): nothing is allocated and no launch changes.  On: the one-float device
        word the loss launch reads (mix_lam; written before every step, outside any capture), and the three sums and 3 * rows workspace
        of ops.softmax_xent_mix when label smoothing / top-k have not asked for them already.  Mixup's blend reads the same word.
        CutMix adds the six-int32 box its launch reads (cut_box); with both on the blend reads a word of its own (blend_lam), which
        holds 1 for a batch that is cut, while mix_lam holds the weight of the method the batch uses."""
        cfg = self.cfg
        self.mixup_alpha, self.mixup_seed = check_mixup(alpha, seed)
        self.cutmix_alpha, self.cutmix_seed, self.cutmix_mode, self.cutmix_prob = check_cutmix(cfg.cutmix_alpha, cfg.cutmix_seed,
                                                                                               cfg.cutmix_mode, cfg.cutmix_prob)
        self.mix_lam = self.blend_lam = self.cut_box = None
        if not self.training or self.mixup_alpha == 0.0:
            self.mixup_alpha, self.mixup_seed = 0.0, 0
        if not self.training or self.cutmix_alpha == 0.0:
            self.cutmix_alpha, self.cutmix_seed = 0.0, 0
        if self.mixup_alpha == 0.0 and self.cutmix_alpha == 0.0:
            return
        self.mix_lam = torch.ones(1, device=self.dev)
        if self.mixup_alpha > 0.0:
            self.blend_lam = self.mix_lam
        if self.cutmix_alpha > 0.0:
            self.cut_box = torch.zeros(6, dtype=torch.int32, device=self.dev)
            self.cut_box_last = (0, 0, 0, 0, 0, 0)
            if self.mixup_alpha > 0.0:
                self.blend_lam = torch.ones(1, device=self.dev)
        if not (self.xent_ls or self.xent_wf or self.multilabel):
            self.stats = torch.zeros(3, device=self.dev)
            self.loss_rows = torch.zeros(3 * rows, device=self.dev)

    def _mix_write(self, mix_lambda, mi, cut_box=None):
        """Before a train step, eager or replayed: the step's label weight (and, with CutMix on, its box) go to the device words on the
        stream, and are kept as self.mix_lambda_last / self.cut_box_last.  Mixup alone: the caller's mix_lambda folded, or the draw of
        the step's draw index.  CutMix alone: the caller's cut_box, or cutmix_box's draw; the weight is cutmix_lambda of the box.  Both
        on: the batch is cut when cutmix_box's u < cutmix_prob, else blended with mixup_lambda's weight (a caller's cut_box or
        mix_lambda decides instead); the method not chosen gets its identity, an empty box or a blend weight of 1."""
        if cut_box is not None:
            if self.cut_box is None:
                raise VltfError("cut_box is given, but CutMix is off on this engine (NetConfig.cutmix_alpha is 0)")
            if mix_lambda is not None:
                raise VltfError("cut_box and mix_lambda are given together: a batch is either cut or blended")
        if mix_lambda is not None and self.blend_lam is None:
            raise VltfError("mix_lambda is given, but mixup is off on this engine (NetConfig.mixup_alpha is 0)")
        if self.mix_lam is None:
            return
        draw = self._draw_index(mi)
        if self.cut_box is None:                  # mixup alone: as before
            lam = fold_lambda(mix_lambda) if mix_lambda is not None else mixup_lambda(self.mixup_alpha, self.mixup_seed, draw)
            ops.fill(self.mix_lam, lam)
            self.mix_lambda_last = lam
            return
        fpc, (h, w) = self.T, self.cfg.image_shape[:2]
        if cut_box is not None:
            box, cut = check_cut_box(cut_box, fpc, h, w), True
        elif mix_lambda is not None:
            box, cut = None, False
        else:
            box, u = cutmix_box(self.cutmix_alpha, self.cutmix_seed, self.cutmix_mode, draw, fpc, h, w)
            cut = self.blend_lam is None or u < self.cutmix_prob
        if cut:
            lam = cutmix_lambda(box, fpc, h, w)
        else:
            box = (0, 0, 0, 0, 0, 0)
            lam = fold_lambda(mix_lambda) if mix_lambda is not None else mixup_lambda(self.mixup_alpha, self.mixup_seed, draw)
        self.cut_box.copy_(torch.tensor(box, dtype=torch.int32))
        ops.fill(self.mix_lam, lam)
        if self.blend_lam is not None:
            ops.fill(self.blend_lam, 1.0 if cut else lam)
        self.mix_lambda_last, self.cut_box_last = lam, tuple(box)

    def _mix_launch(self, n, b):
        """The blend and / or the cut of the clips just fed, in place, in the layout conv1 reads: the packed space-to-depth input when
        feed_u8 wrote it directly (bf16 path), else x0 (frames fed as fp32 on the bf16 path are mixed there, ahead of the pack).  Clip i
        with clip b - 1 - i; the halo and padding zeros blend to zero, and the cut leaves them alone."""
        if self.mix_lam is None:
            return
        packed = self.c8 and self._xb_fed
        if self.blend_lam is not None:
            ops.mixup_pairs(self.layers[0]["xb"][:n] if packed else self.x0[:n], b, self.blend_lam)
        if self.cut_box is not None:
            if packed:
                self.layers[0]["conv"].cutmix_pairs_s2d(self.layers[0]["xb"][:n], b, self.T, self.cut_box)
            else:
                ops.cutmix_pairs(self.x0[:n], b, self.T, self.cfg.image_shape[:2], self.x0_halo, self.x0_phase, self.cut_box)

    # ---- random erasing (erase_*) ------------------------------------------------------------------------------------------
    def _erase_setup(self):
        """Off (erase_prob 0, or an engine that does not train): nothing is allocated and no launch is added.  On: the int32
        [max_clips][8] table the launch reads (erase_row per clip; written before every step, outside any capture)."""
        self.erase = erase_config(self.cfg)
        self.erase_table = self.erase_table_last = None
        if not self.training or self.erase.prob == 0.0:
            self.erase = None
            return
        self.erase_table = torch.zeros((self.B, 8), dtype=torch.int32, device=self.dev)
        self.erase_mode_id, self.erase_scale = ERASE_MODES.index(self.erase.mode), ops.erase_scale(self.erase.std)

    def _erase_write(self, erase_boxes, mi, frames):
        """Before a train step, eager or replayed: the table of the step's clips goes to the device on the stream -- erase_row of the
        step's draw index for the clips rank * max_clips + i, the caller's erase_boxes in the place of the drawn boxes (the keys stay
        the drawn ones) -- and is kept as self.erase_table_last."""
        if self.erase is None:
            if erase_boxes is not None:
                raise VltfError("erase_boxes is given, but random erasing is off on this engine (NetConfig.erase_prob is 0)")
            return
        b = self._check_frames(int(frames.shape[0]))
        fpc, (h, w) = self.T, self.cfg.image_shape[:2]
        boxes = check_erase_boxes(erase_boxes, b, fpc, h, w) if erase_boxes is not None else None
        rank = self.dp.rank if self.dp is not None else 0
        table = erase_table(self.erase, self._draw_index(mi), rank, self.B, fpc, h, w, boxes, clips=b)
        self.erase_table[:b].copy_(torch.from_numpy(table))
        self.erase_table_last = table

    def _erase_launch(self, n, b):
        """Every clip's box of the frames just fed is overwritten in place, in the layout conv1 reads (as _mix_launch chooses it), ahead
        of the blend / the cut: erase each sample, then mix (timm's order)."""
        if self.erase is None:
            return
        if self.c8 and self._xb_fed:
            self.layers[0]["conv"].erase_boxes_s2d(self.layers[0]["xb"][:n], b, self.T, self.erase_table[:b], self.erase_mode_id,
                                                   self.erase_scale)
        else:
            ops.erase_boxes(self.x0[:n], b, self.T, self.cfg.image_shape[:2], self.x0_halo, self.x0_phase, self.erase_table[:b],
                            self.erase_mode_id, self.erase_scale)

    # ---- LARS (lars_eeta; shared with GraphEngine) ----------------------------------------------------------------------------------------
    def _lars_setup(self):
        """Off (lars_eeta 0, or an engine that does not train): nothing is allocated and no launch changes.  On: the tables of lars_ranges,
        rows and a chunk workspace of its own for the tensor_stats launch over the raw gradient (not the logging option's: that one runs
        on the regularised gradient, and only when due) and the trust table -- allocated here, never inside a capture.  No optimizer
        state: the momentum accumulator is all a checkpoint needs."""
        self.lars = None
        if not (self.lars_eeta > 0.0 and self.training):
            return
        ranges, segs, decays = lars_ranges(self.specs, self.plan, self.weight_decay)
        n = len(segs)
        L = dict(ranges=ranges, segs=segs, decays=decays, names=[name for name, _, _ in stat_segments(self.specs, self.plan)],
                 trust=torch.ones(max(n, 1), device=self.dev), stat_trust=None)
        if n:
            L["rows"] = torch.empty(n * ops.STAT_ROW_BYTES, dtype=torch.uint8, device=self.dev)
            L["ws"] = torch.empty(ops.tensor_stats_ws_bytes(segs), dtype=torch.uint8, device=self.dev)
        if self.stat_segs is not None:            # a stats step keeps its update's table for _stats_collect, as stat_ss keeps the norm
            L["stat_trust"] = torch.ones(max(n, 1), device=self.dev)
        self.lars = L

    def _lars_stats_launch(self):
        """_finish_step, before the regulariser: Σw² and Σg² of every weight tensor while g is still the raw gradient."""
        if self.lars is not None and self.lars["segs"]:
            ops.tensor_stats(self.w, self.g, self.lars["segs"], self.lars["rows"], self.lars["ws"])

    def _lars_trust_launch(self, clip_norm, stats_step):
        """_finish_step, behind the norm: the rows and the clip scale (of the regularised gradient) -> the trust table."""
        L = self.lars
        if L["segs"]:
            ops.lars_trust(L["rows"], L["decays"], L["trust"], self.lars_eeta, self.lars_epsilon, clip_norm, self.ss, 1.0)
        if stats_step and L["stat_trust"] is not None:
            L["stat_trust"].copy_(L["trust"])

    def _lars_named(self, table):
        t = table.detach().cpu().numpy()
        idx = {name: k for k, (name, _, _) in enumerate(self.lars["segs"])}
        return collections.OrderedDict((name, float(t[idx[name]]) if name in idx else 1.0) for name in self.lars["names"])

    def lars_trust(self):
        """{variable name: trust ratio} of the most recent update, every trained variable in flat order: what the device computed for
        the weight tensors, 1.0 for the biases (and for everything before the first update).  Frozen variables are absent.  Synchronises."""
        if getattr(self, "lars", None) is None:
            raise VltfError("this engine computes no trust ratios (lars_eeta is 0, or it was built with training=False)")
        torch.cuda.synchronize(self.dev)
        return self._lars_named(self.lars["trust"])

    # ---- LAMB (lamb, lamb_epsilon; shared with GraphEngine) ---------------------------------------------------------------------------------
    def _lamb_setup(self):
        """Off (lamb False, or an engine that does not train): nothing is allocated and no launch changes.  On: the table of lamb_ranges,
        the rows, the trust table and the chunk workspace of ops.lamb_moments -- allocated here, never inside a capture.  The optimizer
        state is Adam's: adam_m, adam_v and step_count are all a checkpoint needs."""
        self.lamb = None
        if not (self.lamb_on and self.training):
            return
        ranges, segs = lamb_ranges(self.specs, self.plan, self.weight_decay)
        if not ranges:
            raise VltfError("lamb: the plan trains no variable")
        n = len(segs)
        L = dict(ranges=ranges, segs=segs, names=[name for name, _, _ in stat_segments(self.specs, self.plan)],
                 trust=torch.ones(max(n, 1), device=self.dev), stat_trust=None,
                 rows=torch.zeros(max(n, 1) * ops.LAMB_ROW_BYTES, dtype=torch.uint8, device=self.dev),
                 ws=torch.empty(ops.lamb_moments_ws_bytes(ranges), dtype=torch.uint8, device=self.dev))
        if self.stat_segs is not None:            # a stats step keeps its update's table for _stats_collect, as stat_ss keeps the norm
            L["stat_trust"] = torch.ones(max(n, 1), device=self.dev)
        self.lamb = L

    def _lamb_launch(self, lr, clip_norm, skip, stats_step, captured):
        """_finish_step, in the place of the Adam launch (step_count already counts this update): the moments and the trust table, then
        the weights.  Captured: lr, c1 and c2 come from the step state (_graph_step writes them before the replay)."""
        L = self.lamb
        if captured:
            ops.lamb_moments_st(self.w, self.g, self.adam_m, self.adam_v, L["ranges"], L["rows"], L["trust"], L["ws"], self.state,
                                self.lamb_epsilon, clip_norm, self.ss, 1.0, skip=skip)
        else:
            c1, c2 = lamb_corrections(self.step_count - 1)
            ops.lamb_moments(self.w, self.g, self.adam_m, self.adam_v, L["ranges"], L["rows"], L["trust"], L["ws"], c1, c2,
                             self.lamb_epsilon, clip_norm, self.ss, 1.0, skip=skip)
        if stats_step and L["stat_trust"] is not None:
            L["stat_trust"].copy_(L["trust"])
        if captured:
            ops.lamb_apply_st(self.w, self.adam_m, self.adam_v, L["ranges"], L["trust"], self.state, self.lamb_epsilon, skip=skip)
        else:
            ops.lamb_apply(self.w, self.adam_m, self.adam_v, L["ranges"], L["trust"], lr, c1, c2, self.lamb_epsilon, skip=skip)

    def _lamb_named(self, table):
        t = table.detach().cpu().numpy()
        idx = {name: k for k, (name, _, _) in enumerate(self.lamb["segs"])}
        return collections.OrderedDict((name, float(t[idx[name]]) if name in idx else 1.0) for name in self.lamb["names"])

    def lamb_trust(self):
        """{variable name: trust ratio} of the most recent update, every trained variable in flat order: what the device computed for
        the weight tensors, 1.0 for the biases (and for everything before the first update).  Frozen variables are absent.  Synchronises."""
        if getattr(self, "lamb", None) is None:
            raise VltfError("this engine computes no trust ratios (lamb is off, or it was built with training=False)")
        torch.cuda.synchronize(self.dev)
        return self._lamb_named(self.lamb["trust"])

    # ---- optimizer state (what tf.train.Saver() keeps besides the weights, feeder.py:201: Adam slots + beta powers) -------
    OPT_PREFIX = "__optimizer__/"

    def get_opt_state(self):
        """{reserved name: array} to store beside the weights; step_count drives Adam's bias correction and the dropout seed."""
        if self.micro.open():
            self.micro.reset()
            raise VltfError("optimizer state is taken at update boundaries only: an accumulated update is in progress (it is abandoned)")
        torch.cuda.synchronize(self.dev)
        st = {self.OPT_PREFIX + "step_count": np.array([self.step_count], np.int64)}
        if self.cfg.optimizer == "adam" and self.training:
            st[self.OPT_PREFIX + "adam_m"] = self.adam_m.detach().cpu().numpy().copy()
            st[self.OPT_PREFIX + "adam_v"] = self.adam_v.detach().cpu().numpy().copy()
        if self.mom is not None:
            st[self.OPT_PREFIX + "momentum"] = self.mom.detach().cpu().numpy().copy()
        if getattr(self, "ema", None) is not None:
            st[self.OPT_PREFIX + "ema"] = self.ema.detach().cpu().numpy().copy()
        return st

    def load_opt_state(self, state, global_step=None):
        """Restores get_opt_state(); returns the names that were expected but absent (fresh optimizer for those)."""
        missing = []
        key = self.OPT_PREFIX + "step_count"
        if key in state:
            self.step_count = int(np.asarray(state[key]).ravel()[0])
        else:
            missing.append(key)
            if global_step is not None:
                self.step_count = int(global_step)
        slots = []
        if self.cfg.optimizer == "adam" and self.training:
            slots = [("adam_m", self.adam_m), ("adam_v", self.adam_v)]
        elif self.mom is not None:
            slots = [("momentum", self.mom)]
        for name, t in slots:
            a = state.get(self.OPT_PREFIX + name)
            if a is None:
                missing.append(self.OPT_PREFIX + name)
                continue
            a = np.asarray(a, np.float32)
            if a.shape != (t.numel(),):
                raise VltfError("optimizer state %s has shape %s, expected (%d,)" % (name, a.shape, t.numel()))
            t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        if getattr(self, "ema", None) is not None:
            a = state.get(self.OPT_PREFIX + "ema")
            if a is None:                         # a checkpoint from a run without the average: it starts at the loaded weights
                missing.append(self.OPT_PREFIX + "ema")
                self.ema.copy_(self.w)
            else:
                self.load_ema(a)
        return missing

    def check_status(self):
        """Raises when a cluster-form LSTM launch since the last check timed out (ops.lstm_seq_check: the flag is sticky over the
        launches of a step and reset here).  Synchronises; called wherever results are fetched to the host."""
        if getattr(self, "lstm_ws", None) is not None:
            try:
                ops.lstm_seq_check(self.lstm_ws, self.lstm_ws_graph)
            except VltfError:
                self.micro.reset()            # an accumulated update in progress holds an invalid gradient: it is abandoned
                raise

    def logits_host(self, rows=None):
        torch.cuda.synchronize(self.dev)
        self.check_status()
        return self.logits[:rows if rows is not None else self._rows].detach().cpu().numpy().copy()

    # ---- input ---------------------------------------------------------------------------------
    def _check_frames(self, n):
        if n <= 0 or n % self.T or n > self.N:
            raise VltfError("got %d frames: need a positive multiple of fpc=%d, at most %d" % (n, self.T, self.N))
        return n // self.T

    def feed_u8(self, frames_u8, mean_bgr=None, crop_y=None, crop_x=None, mirror=None, resize=None, crop_box=None):
        """frames uint8 [n, raw_h, raw_w, 3] on device (TFRecord image_raw bytes) -> x0 (dataset_.py:481-501).
        resize: [((h, w), (oh, ow)), ...] imresize steps applied first (imgproc raw_resize / resize: PIL bilinear on uint8).
        crop_box: device int32 [n, 4] = (y0, x0, bh, bw) per frame of the frame the feed receives (after `resize`): random resized
        crop, the box resampled bilinearly to the network input (ops.input_prep_u8_box); not with crop_y / crop_x."""
        n = frames_u8.shape[0]
        b = self._check_frames(n)
        self._check_crop_box(crop_box, crop_y, crop_x)
        for src_hw, dst_hw in (resize or ()):
            key = (tuple(src_hw), tuple(dst_hw))
            if key not in self._resizers:
                self._resizers[key] = ops.Resize(src_hw[0], src_hw[1], dst_hw[0], dst_hw[1])
            frames_u8 = self._resizers[key](frames_u8)
        mean = None
        if mean_bgr is not None:
            self.mean_dev.copy_(torch.as_tensor(np.asarray(mean_bgr, np.float32)), non_blocking=True)
            mean = self.mean_dev
        return self._feed_dev(frames_u8, n, b, mean, crop_y, crop_x, mirror, crop_box)

    @staticmethod
    def _check_crop_box(crop_box, crop_y, crop_x):
        """Before anything is launched: a box per frame takes the place of the crop offsets, never both."""
        if crop_box is not None and (crop_y is not None or crop_x is not None):
            raise VltfError("crop_box (random resized crop) is refused together with crop_y / crop_x: a frame is either cropped at an "
                            "offset or resampled from its box")

    def _feed_dev(self, frames_u8, n, b, mean, crop_y, crop_x, mirror, crop_box=None):
        """feed_u8 from here on, every input on the device (what a captured step runs)."""
        if self.c8:     # bf16 path: the frames go straight into conv1's packed (space-to-depth) input; x0 is not written
            if crop_box is not None:
                self.layers[0]["conv"].input_prep_u8_box_s2d(frames_u8, self.layers[0]["xb"][:n], crop_box, mirror, mean)
            else:
                self.layers[0]["conv"].input_prep_u8_s2d(frames_u8, self.layers[0]["xb"][:n], crop_y, crop_x, mirror, mean)
            self._xb_fed = True
            return n, b
        if crop_box is not None:
            ops.input_prep_u8_box(frames_u8, self.x0[:n], crop_box, mirror, mean, halo=self.x0_halo, phase=self.x0_phase,
                                  out_hw=self.cfg.image_shape[:2])
            return n, b
        ops.input_prep_u8(frames_u8, self.x0[:n], crop_y, crop_x, mirror, mean, halo=self.x0_halo, phase=self.x0_phase,
                          out_hw=self.cfg.image_shape[:2])
        return n, b

    def feed_f32_nhwc(self, frames):
        """The reference's placeholder format: float32 NHWC, already cropped / mean-subtracted (model.py:54)."""
        n = frames.shape[0]
        b = self._check_frames(n)
        ops.nhwc_to_nchw(frames, self.x0[:n], halo=self.x0_halo, phase=self.x0_phase)
        self._xb_fed = False
        return n, b

    def _fc6_kc8(self, n):
        """fc6 runs on the packed-operand product kernel: bf16 path, whole 8-frame blocks."""
        return self.c8 and hasattr(self, "k_w") and n % 8 == 0

    def _lstm_kc8(self, n, l):
        """The first LSTM layer's three whole-sequence products (input projection, kernel gradient, input gradient) run on the
        packed-operand kernel too (bf16 path): the same arithmetic as the split-product GEMM in mode 1 -- operands rounded to bf16, fp32
        accumulation -- without its operand images.  They reuse fc6's operand buffers (the launches are serial on one stream)."""
        D, H4 = self.cfg.encode_dim(), 4 * self.cfg.lstm_hidden
        if getattr(self, "bi", False) or getattr(self, "is_gru", False):   # a bidirectional or GRU layer's dense products run on ops.gemm
            return False
        if getattr(self, "sa", None) or getattr(self, "tc", None):         # a self-attention or convolution layer's too
            return False
        return (l == 0 and self._fc6_kc8(n) and os.environ.get("VLTF_LSTM_KC8", "1") != "0" and D % 8 == 0 and H4 % 8 == 0
                and D * H4 <= self.k_w.numel() and n * max(D, H4) <= self.k_act.numel() and (not self.training or n * H4 <= self.k_d6.numel()))

    # ---- forward -------------------------------------------------------------------------------
    def _forward(self, n, b, train):
        P, cfg = self.P, self.cfg
        ops.set_conv_math(cfg.conv_math)             # process-wide switch: set per call so that engines of both kinds can coexist
        x = self.x0[:n]
        for li, L in enumerate(self.layers):
            name = L["name"]
            nxt = self.layers[li + 1] if li + 1 < len(self.layers) else None
            if self.c8 and li == 0:
                conv = L["conv"]
                if not self._xb_fed:                      # fed as fp32 frames (feed_f32_nhwc): pack x0
                    conv.s2d_c8_from_x0(x, L["xb"][:n])
                conv.s2d_weights(P["dcnn/%sW" % name], L["ws2d"])
                L["eq"].c8_pack_w(L["ws2d"], L["wb"], False)
                self._run(name + ".fwd", L["eq"].c8_fwd, L["xb"][:n], L["wb"], P["dcnn/%sb" % name], yb=L["yb"][:n], relu=True)
            elif self.c8:
                # bf16 path: packed operands; a conv that feeds the next conv directly also writes that conv's packed input
                L["conv"].c8_pack_w(P["dcnn/%sW" % name], L["wb"], False)
                yb = nxt["xb"][:n] if (nxt is not None and not L["pool"]) else (L["yb"][:n] if "yb" in L else None)
                y = L["y"][:n] if yb is None else None       # fp32 output only where the plain max-pool reads it (conv5)
                self._run(name + ".fwd", L["conv"].c8_fwd, L["xb"][:n], L["wb"], P["dcnn/%sb" % name], y=y, yb=yb, relu=True)
            else:
                self._run(name + ".fwd", L["conv"].fwd, x, P["dcnn/%sW" % name], P["dcnn/%sb" % name], L["y"][:n], relu=True)
            x = L["y"][:n]
            if L["lrn"] and L["pool"] and self.c8:
                # bf16 path: the pooled output is only ever the next conv's packed operand -- written packed, fp32 p stays unused
                ops.lrn_pool_fwd_c8(L["yb"][:n], nxt["xb"][:n], L["arg"][:n], p_halo=L["p_halo"], channels=L["conv"].cout, **LRN)
                x = None
            elif L["lrn"] and L["pool"]:
                # LRN + pool in one pass: the LRN output is only ever the pool's input and is never stored
                ops.lrn_pool_fwd(x, L["p"][:n], L["arg"][:n], p_halo=L["p_halo"], **LRN)
                x = L["p"][:n]
            elif L["pool"]:
                ops.maxpool_fwd(x, L["p"][:n], L["arg"][:n], hwc=L["hwc"], y_halo=L["p_halo"])
                x = L["p"][:n]
            if self.c8 and L["pool"] and not L["lrn"] and nxt is not None:
                ops.pack_c8(x, nxt["xb"][:n], L["p_halo"], nxt["x_halo"])
        if self._fc6_kc8(n):
            F = self.flat_dim
            a = self.k_act[:n * F].view(ops.kc8_shape(F, n))
            w = self.k_w.view(ops.kc8_shape(F, FC_DIM))
            ops.pack_kc8(x, a, F, n, 1, F)                                    # (position f, channel frame) = pool5[frame][f]
            ops.pack_kc8(P["dcnn/fc6W"], w, F, FC_DIM, FC_DIM, 1)
            ops.gemm_kc8(a, w, self.f6, n, FC_DIM, F, bias=P["dcnn/fc6b"], relu=True, ws=self.ws)
        else:
            ops.gemm(x, P["dcnn/fc6W"], self.f6, n, FC_DIM, self.flat_dim, bias=P["dcnn/fc6b"], relu=True, ws=self.ws)
        self._fc_drop = train and 0.0 < self.fc_keep < 1.0      # this pass dropped f6 / f7: their ReluGrad sites divide by keep
        if self._fc_drop:
            self._fc_dropout("fc6", self.f6[:n])
        if self.f7 is not None:
            ops.gemm(self.f6, P["dcnn/fc7W"], self.f7, n, FC_DIM, FC_DIM, bias=P["dcnn/fc7b"], relu=True, ws=self.ws)
            if self._fc_drop:
                self._fc_dropout("fc7", self.f7[:n])
        if self.f8 is not None:
            ops.gemm(self.f7, P["dcnn/fc8W"], self.f8, n, cfg.num_classes, FC_DIM, bias=P["dcnn/fc8b"], ws=self.ws)
        D, C, H, T = cfg.encode_dim(), cfg.num_classes, cfg.lstm_hidden, self.T
        if cfg.classifier == "lstm":
            xin, d = self.feat, D
            HO = self.lstm_out
            if self.blstm:
                xin, d = blstm_forward(self.blstm, P, "", xin, n, b, T, d, H, self.ws, self._rk), HO
            if self.gru:
                xin, d = gru_forward(self.gru, P, "", xin, n, b, T, d, H, self.ws, self._rk), H
            self._sa_drop = self._sa_drop_bound() if train and self.sa_drop is not None else None
            if self.mhsa:
                self._mhsa_clips = b
            if self.enc:
                # sa_block encoder: embedding, L blocks, final norm (encoder_forward); without a dropout rate no launch takes a
                # host-varying argument, with one the seed is the only such (a captured step: the _st forms)
                xin, d = encoder_forward(self.enc, P, "", xin, n, b, T, d, H, self.sa_ffn, self.sa[0], self.sa[1], self.ws, {},
                                         self._sa_drop), H
            elif self.mhsa:
                xin, d = mhsa_forward(self.mhsa, P, "", xin, n, b, T, d, H, self.sa[0], self.sa[1], self.ws, {}, self._sa_drop), H
            if self.tcn:
                # rnn_cell tcn: embedding, then per layer the taps launch, two products and the residual add (tcn_forward)
                xin, d = tcn_forward(self.tcn, P, "", xin, n, b, T, d, H, self.tc, self.ws, {}), H
            for l, S in enumerate(self.lstm):
                pre = "rnn/multi_rnn_cell/cell_%d/basic_lstm_cell/" % l
                K = P[pre + "kernel"]
                # hoisted input projection for all (clip, t) rows, then the serial recurrence
                if self._lstm_kc8(n, l):
                    a = self.k_act[:n * d].view(ops.kc8_shape(d, n))
                    w = self.k_w[:d * 4 * H].view(ops.kc8_shape(d, 4 * H))
                    ops.pack_kc8(xin, a, d, n, 1, d)                                  # (position j, channel frame) = x[frame][j]
                    ops.pack_kc8(K, w, d, 4 * H, 4 * H, 1)                            # (position j, channel column) = K[j][column]
                    ops.gemm_kc8(a, w, S["gx"], n, 4 * H, d, bias=P[pre + "bias"], ws=self.ws)
                else:
                    ops.gemm(xin, K, S["gx"], n, 4 * H, d, bias=P[pre + "bias"], ws=self.ws)
                if H <= 1024 and self._tag_off is not None:           # captured: replay-safe tags on the graph workspace
                    ops.lstm_seq_fwd_st(S["gx"], K[d:], S["act"], S["cseq"], S["hseq"], S["hprev"], b, T, H, FORGET_BIAS,
                                        ws=self.lstm_ws_graph, state=self.state, tag_offset=self._tag_off)
                    self._tag_off += ops.lstm_seq_tag_span(b, T, H)
                elif H <= 1024:
                    ops.lstm_seq_fwd(S["gx"], K[d:], S["act"], S["cseq"], S["hseq"], S["hprev"], b, T, H, FORGET_BIAS, ws=self.lstm_ws)
                else:
                    for t in range(T):
                        if t > 0:
                            ops.gemm(S["hseq"][t - 1:], K[d:], self.gh, b, 4 * H, H, lda=T * H)
                        ops.lstm_step_fwd(S["gx"], self.gh if t > 0 else None, S["act"], S["cseq"], S["hseq"], S["hprev"], b, T,
                                          t, H, FORGET_BIAS)
                xin, d = S["hseq"], H
            r = n if self.per_step else b
            if self.per_step:
                v = xin                                                  # every step's output of the last layer
            elif self.bi and self.lstm_fusion == "last":
                # each direction's FINAL output: the forward half at t = T - 1, the backward half at t = 0
                o3 = xin[:b * T].view(b, T, HO)
                ops.copy2d(o3[:, T - 1, :H], self.fused, b, H, src_ld=T * HO, dst_ld=HO)
                ops.copy2d(o3[:, 0, H:], self.fused[:, H:], b, H, src_ld=T * HO, dst_ld=HO)
                v = self.fused
            elif self.attn is not None:
                attn_forward(self.attn, P, "", xin, self.fused, n, b, T, HO, self.attn_dim, {})
                self._attn_clips = b
                v = self.fused
            elif self.vlad is not None:
                vlad_forward(self.vlad, P, "", xin, self.fused, n, b, T, HO, self.vlad_k, {})
                self._vlad_clips = b
                v = self.fused
            else:
                ops.temporal_fusion_fwd(xin, self.fused, b, T, HO, self.lstm_fusion)
                v = self.fused
            self._dropout = train and cfg.dropout_keep_prob > 0 and cfg.fusion != "state"
            if self._dropout and self._tag_off is not None:          # captured: the seed follows the step state's count
                ops.dropout_fwd_st(v[:r], self.dropped[:r], self.drop_mask[:r], cfg.dropout_keep_prob, self.state)
                v = self.dropped
            elif self._dropout:
                ops.dropout_fwd(v[:r], self.dropped[:r], self.drop_mask[:r], cfg.dropout_keep_prob,
                                (self._draw_index() << 20) ^ 0x5DEECE66D)
                v = self.dropped
            self._v = v
            HW = self.head_in
            if HW != C:
                ops.gemm(v, P[self.head + "_w"], self.logits, r, C, HW, bias=P[self.head + "_b"])
            elif v is not self.logits:
                self.logits[:r].copy_(v[:r])
            self._rows = r
        else:
            C = cfg.out_dim()
            v, rows = self.feat, n
            if self.early:
                ops.temporal_fusion_fwd(self.feat, self.fc_in, b, T, D, self.ff_method)
                v, rows = self.fc_in, b
            if D != C:
                ops.gemm(v, P["fc_convert_w"], self.fc_out, rows, C, D, bias=P["fc_convert_b"])
            if self.late:
                ops.temporal_fusion_fwd(self.fc_out, self.logits, b, T, C, self.ff_method)
                rows = b
            self._rows = rows
        return self._rows

    def forward_u8(self, frames_u8, mean_bgr=None, crop_y=None, crop_x=None, mirror=None, resize=None, crop_box=None):
        """sess.run(model.logits, fdict) (run_task.py:95).  Returns a device view [rows, classes]."""
        self._check_crop_box(crop_box, crop_y, crop_x)
        if self.step_graph:
            done, out = self._graph_step(False, frames_u8, mean_bgr, crop_y, crop_x, mirror, resize, crop_box=crop_box)
            if done:
                return out
        n, b = self.feed_u8(frames_u8, mean_bgr, crop_y, crop_x, mirror, resize, crop_box)
        rows = self._forward(n, b, train=False)
        return self.logits[:rows]

    def attention_weights(self):
        """Device view [clips, T] of the weights alpha the last forward gave each time step (fusion attn); rows sum to 1."""
        if getattr(self, "attn", None) is None:
            raise VltfError("attention_weights: the model has no attention pooling (lstm_params fusion attn)")
        return self.attn["alpha"][:self._attn_clips]

    def vlad_assignments(self):
        """Device view [clips, T, K] of the soft assignments a the last forward gave each time step (fusion vlad): a live row sums to
        1 over the centres, a dead row is zero."""
        if getattr(self, "vlad", None) is None:
            raise VltfError("vlad_assignments: the model has no NetVLAD pooling (lstm_params fusion vlad)")
        return self.vlad["sa"][:self._vlad_clips * self.T].view(self._vlad_clips, self.T, self.vlad_k)

    def self_attention_weights(self, layer=-1):
        """Device view [clips, heads, T, T] of the weights P the last forward gave (rnn_cell mhsa; the last layer's by default): row q
        of a clip and head sums to 1 over the keys."""
        if not getattr(self, "mhsa", None):
            raise VltfError("self_attention_weights: the model has no self-attention layer (rnn_cell mhsa)")
        T = self.cfg.fpc
        return self.mhsa[layer]["P"][:self._mhsa_clips * self.sa[0]].view(self._mhsa_clips, self.sa[0], T, T)

    def forward_f32(self, frames_nhwc):
        n, b = self.feed_f32_nhwc(frames_nhwc)
        rows = self._forward(n, b, train=False)
        return self.logits[:rows]

    # ---- backward ------------------------------------------------------------------------------
    def _backward(self, n, b):
        P, G, cfg = self.P, self.G, self.cfg
        ops.set_conv_math(cfg.conv_math)             # process-wide switch (see _forward): another engine may have run in between
        self._frames_now = n
        D, C, H, T = cfg.encode_dim(), cfg.num_classes, cfg.lstm_hidden, self.T
        sw = self.small_ws
        kconv = self.first_conv                      # first trainable conv layer: nothing is computed for the layers before it
        self._next_chunk = 0
        # a frozen conv stack leaves the second stream nothing to run beside: it is not forked
        side = self._side_stream() if kconv < len(self.layers) else None
        if side is not None:
            # the flipped / transposed weights every dgrad reads, all layers now, on the second stream (idle until fc6): a transpose
            # in front of its dgrad sits on the backward's critical chain while the weight gradient on the other stream takes the CUs
            # (round 3, same box: 8 clips 5.71 -> 5.42 ms, 16 clips 9.90 -> 9.81, 64 clips on two streams 35.25 -> 35.05; which of
            # dgrad / wgrad the host issues first made no difference)
            side.wait_stream(torch.cuda.current_stream(self.dev))
            with torch.cuda.stream(side):
                for L in self.layers[kconv + 1:]:      # (a layer's dgrad runs only where the layer below it trains)
                    L["conv"].wt_transpose(P["dcnn/%sW" % L["name"]], L["wt"])
                self._wt_ready.record(side)          # the first dgrad waits for this (below), nothing else on the launch stream does
        main = torch.cuda.current_stream(self.dev)

        def param_grads(launch):
            """The chain of INPUT gradients is the backward's critical path and stays on the launch stream; a parameter gradient only has
            to be done by the end of the pass: with a second stream it runs there (from where the launch stream stands now, on the
            second stream's own scratch), beside the chain.  Head / LSTM / fc6 parameter gradients there instead of on the chain
            (round 3, same box): 8 clips 5.43 -> 5.32 ms, 64 clips 35.0 -> 34.75."""
            if side is None:
                launch(self.ws, sw)
            else:
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    launch(self.ws_side, self.small_ws_side)

        if cfg.classifier == "lstm":
            d, r = self.dlogits, self._rows
            HO, HW = self.lstm_out, self.head_in
            if HW != C:
                def head_grads(ws, sws, r=r):
                    ops.gemm(self._v, self.dlogits, G[self.head + "_w"], HW, C, r, transa=True)
                    ops.colsum(self.dlogits, G[self.head + "_b"], sws, r, C)
                param_grads(head_grads)
                ops.gemm(self.dlogits, P[self.head + "_w"], self.ddropped, r, HW, C, transb=True)
                d = self.ddropped
            if self._dropout:
                ops.dropout_bwd(d[:r], self.drop_mask[:r], self.dfused[:r], cfg.dropout_keep_prob)
                d = self.dfused
            top = (self.blstm or self.gru or self.mhsa or self.tconv or self.lstm)[-1]
            if self.per_step:
                top["dout"][:r].copy_(d[:r])
            elif self.bi and self.lstm_fusion == "last":
                ops.fill(top["dout"][:b * T], 0.0)
                g3 = top["dout"][:b * T].view(b, T, HO)
                ops.copy2d(d, g3[:, T - 1, :H], b, H, src_ld=HO, dst_ld=T * HO)
                ops.copy2d(d[:, H:], g3[:, 0, H:], b, H, src_ld=HO, dst_ld=T * HO)
            elif self.attn is not None:
                attn_backward(self.attn, P, G, "", d, top["hseq"], top["dout"], n, b, T, HO, self.attn_dim, {}, param_grads)
            elif self.vlad is not None:
                vlad_backward(self.vlad, P, G, "", d, top["hseq"], self.fused, top["dout"], n, b, T, HO, self.vlad_k, {}, param_grads)
            else:
                ops.temporal_fusion_bwd(d, top["dout"], b, T, HO, self.lstm_fusion)
            if self.blstm:
                # dfeat None: a frozen tower, nobody reads it; the ReluGrad of fc6 / fc7 applies to the sum of both directions' products
                blstm_backward(self.blstm, P, G, "", self.feat, n, b, T, D, H, self.ws, self._rk, param_grads,
                               self.dfeat if self.dcnn_trains else None, self.dx_bw)
                if self.dcnn_trains and self.f8 is None:
                    self._relu_grad(self.dfeat, self.feat, n * D)
            if self.gru:
                dgx = gru_backward(self.gru, P, G, "", self.feat, n, b, T, D, H, self.ws, self._rk, param_grads)
                self._feat_grad(dgx, P[gru_names(0)[0]], n, 3 * H)
            if self.enc:
                # sa_block encoder: the blocks (encoder_backward), then the embedding as the GRU's input projection
                dx0 = encoder_backward(self.enc, P, G, "", self.feat, n, b, T, D, H, self.sa_ffn, self.sa[0], self.sa[1], self.ws, {},
                                       param_grads, self._sa_drop)
                embed_grads(G, encoder_var, "", self.feat, dx0, n, D, H, param_grads)
                self._feat_grad(dx0, P[encoder_var("", None, "kernel")], n, H)
            elif self.mhsa:
                dqkv = mhsa_backward(self.mhsa, P, G, "", self.feat, n, b, T, D, H, self.sa[0], self.sa[1], self.ws, {}, param_grads,
                                     self._sa_drop)
                self._feat_grad(dqkv, P[mhsa_names(0, positions=self.sa[1])[0]], n, 3 * H)
            if self.tcn:
                # rnn_cell tcn: the layers (tcn_backward), then the embedding as the GRU's input projection
                dx0 = tcn_backward(self.tcn, P, G, "", n, b, T, H, self.tc, {}, param_grads)
                embed_grads(G, tcn_var, "", self.feat, dx0, n, D, H, param_grads)
                self._feat_grad(dx0, P[tcn_var("", None, "kernel")], n, H)
            for l in reversed(range(len(self.lstm))):
                S = self.lstm[l]
                pre = "rnn/multi_rnn_cell/cell_%d/basic_lstm_cell/" % l
                K = P[pre + "kernel"]
                din = D if l == 0 else H
                xin = self.feat if l == 0 else self.lstm[l - 1]["hseq"]
                if H <= 1024 and self._tag_off is not None:
                    ops.lstm_seq_bwd_st(S["dout"], K[din:], S["act"], S["cseq"], S["dz"], b, T, H, ws=self.lstm_ws_graph, state=self.state,
                                        tag_offset=self._tag_off)
                    self._tag_off += ops.lstm_seq_tag_span(b, T, H)
                elif H <= 1024:
                    ops.lstm_seq_bwd(S["dout"], K[din:], S["act"], S["cseq"], S["dz"], b, T, H, ws=self.lstm_ws)
                else:
                    ops.fill(self.dc, 0.0)
                    for t in reversed(range(T)):
                        ops.lstm_step_bwd(S["dout"], self.dh if t < T - 1 else None, S["act"], S["cseq"], self.dc, S["dz"], b, T, t, H)
                        if t > 0:
                            ops.gemm(S["dz"][t:], K[din:], self.dh, b, H, 4 * H, transb=True, lda=T * 4 * H)
                lk = self._lstm_kc8(n, l)

                def lstm_grads(ws, sws, S=S, pre=pre, din=din, xin=xin, lk=lk):
                    if lk:                                                                # (bf16 path: one stream)
                        a = self.k_act[:n * din].view(ops.kc8_shape(n, din))
                        zb = self.k_d6[:n * 4 * H].view(ops.kc8_shape(n, 4 * H))
                        ops.pack_kc8(xin, a, n, din, din, 1)                              # (position frame, channel j)
                        ops.pack_kc8(S["dz"], zb, n, 4 * H, 4 * H, 1)                     # (position frame, channel column)
                        ops.gemm_kc8(a, zb, G[pre + "kernel"], din, 4 * H, n, ws=ws)
                    else:
                        ops.gemm(xin, S["dz"], G[pre + "kernel"], din, 4 * H, n, transa=True, ws=ws)
                    ops.gemm(S["hprev"], S["dz"], G[pre + "kernel"][din:], H, 4 * H, n, transa=True, ws=ws)
                    ops.colsum(S["dz"], G[pre + "bias"], sws, n, 4 * H)
                param_grads(lstm_grads)
                if l == 0 and not self.dcnn_trains:
                    pass                                                              # frozen tower: nobody reads dfeat
                elif l == 0 and lk:
                    a = self.k_act[:n * 4 * H].view(ops.kc8_shape(4 * H, n))
                    w = self.k_w[:D * 4 * H].view(ops.kc8_shape(4 * H, D))
                    ops.pack_kc8(S["dz"], a, 4 * H, n, 1, 4 * H)                      # (position column, channel frame) = dz[frame][column]
                    ops.pack_kc8(K, w, 4 * H, D, 1, 4 * H)                            # (position column, channel j) = K[j][column]
                    ops.gemm_kc8(a, w, self.dfeat, n, D, 4 * H, ws=self.ws)
                    if self.f8 is None:
                        self._relu_grad(self.dfeat, self.feat, n * D)                 # ReluGrad of fc6 / fc7
                elif l == 0:
                    self._feat_grad(S["dz"], K, n, 4 * H)
                else:
                    ops.gemm(S["dz"], K, self.lstm[l - 1]["dout"], n, H, 4 * H, transb=True, ldb=4 * H, ws=self.ws)
        else:
            Co = cfg.out_dim()                # width of the pipeline output (= D for a feature pipeline)
            d, rows = self.dlogits, self._rows
            if self.late:
                ops.temporal_fusion_bwd(self.dlogits, self.dfc_out, b, T, Co, self.ff_method)
                d, rows = self.dfc_out, b * T
            relu_mask = self.feat if (self.f8 is None and not self.early) else None
            target = self.dfc_in if self.early else self.dfeat
            if D != Co:
                ops.gemm(self.fc_in, d, G["fc_convert_w"], D, Co, rows, transa=True)
                ops.colsum(d, G["fc_convert_b"], sw, rows, Co)
                if self.dcnn_trains:
                    ops.gemm(d, P["fc_convert_w"], target, rows, D, Co, transb=True, relu_mask=self._fused_mask(relu_mask))
                    self._relu_grad_behind(target, relu_mask, rows * D)
            elif self.dcnn_trains:
                target[:rows].copy_(d[:rows])
                if relu_mask is not None:        # no fc in between (a feature pipeline): the encode layer's ReluGrad applies here
                    self._relu_grad(target, relu_mask, rows * D)
            if self.early and self.dcnn_trains:
                # ReluGrad of the encode layer applies per frame after un-fusing
                ops.temporal_fusion_bwd(self.dfc_in, self.dfeat, b, T, D, self.ff_method)
                if self.f8 is None:
                    self._relu_grad(self.dfeat, self.feat, n * D)
        # ---- fc8 / fc7 / fc6 (dfeat already carries the ReluGrad of the encode layer).  A layer gets its parameter gradients where it
        # trains and hands a gradient down where the layer below it trains; below the first trainable layer nothing is launched.
        trains = self.fc_trains
        d = self.dfeat
        if self.f8 is not None and trains["fc8"]:
            ops.gemm(self.f7, d, G["dcnn/fc8W"], FC_DIM, C, n, transa=True, ws=self.ws)
            ops.colsum(d, G["dcnn/fc8b"], sw, n, C)
            if trains["fc7"]:
                ops.gemm(d, P["dcnn/fc8W"], self.df7, n, FC_DIM, C, transb=True, relu_mask=self._fused_mask(self.f7), ws=self.ws)
                self._relu_grad_behind(self.df7, self.f7, n * FC_DIM)
            d = self.df7
        if self.f7 is not None and trains["fc7"]:
            ops.gemm(self.f6, d, G["dcnn/fc7W"], FC_DIM, FC_DIM, n, transa=True, ws=self.ws)
            ops.colsum(d, G["dcnn/fc7b"], sw, n, FC_DIM)
            if trains["fc6"]:
                ops.gemm(d, P["dcnn/fc7W"], self.df6, n, FC_DIM, FC_DIM, transb=True, relu_mask=self._fused_mask(self.f6), ws=self.ws)
                self._relu_grad_behind(self.df6, self.f6, n * FC_DIM)
            d = self.df6
        L5 = self.layers[-1]
        kc8 = self._fc6_kc8(n)
        f6o = self.offsets["dcnn/fc6W"][0]
        convs_train = kconv < len(self.layers)
        if not trains["fc6"]:
            param_grads(lambda ws, sws: self._issue(f6o))         # everything above fc6, from the stream its parameter gradients ran on
        elif kc8:
            # bf16 path (one stream): weight gradient in one pass on the packed-operand kernel (the exchange chunks follow it)
            ops.colsum(d, G["dcnn/fc6b"], sw, n, FC_DIM)
            F = self.flat_dim
            a = self.k_p5[:n * F].view(ops.kc8_shape(n, F))
            b_ = self.k_d6[:n * FC_DIM].view(ops.kc8_shape(n, FC_DIM))
            ops.pack_kc8(L5["p"], a, n, F, F, 1)                              # (position frame, channel f)
            ops.pack_kc8(d, b_, n, FC_DIM, FC_DIM, 1)
            if self.dp is None:
                ops.gemm_kc8(a, b_, G["dcnn/fc6W"], F, FC_DIM, n, ws=self.ws)
            else:
                # the exchange starts here, as on the fp32 path: a row block of fc6W = a range of the packed operand's 8-row
                # blocks (block edges are multiples of 128), each block's all-reduce issued right behind its product
                self._issue(f6o)
                for r0, r1 in self.fc6_row_blocks:
                    ops.gemm_kc8(a[r0 // 8:r1 // 8], b_, G["dcnn/fc6W"][r0:r1], r1 - r0, FC_DIM, n, ws=self.ws)
                    self._issue(self._fc6_block_end(r1))
            if convs_train:
                a = self.k_act[:n * FC_DIM].view(ops.kc8_shape(FC_DIM, n))
                w = self.k_w.view(ops.kc8_shape(FC_DIM, F))
                ops.pack_kc8(d, a, FC_DIM, n, 1, FC_DIM)                          # (position j, channel frame) = dfc6[frame][j]
                ops.pack_kc8(P["dcnn/fc6W"], w, FC_DIM, F, 1, FC_DIM)             # (position j, channel f) = W[f][j]
                ops.gemm_kc8(a, w, L5["dp"], n, F, FC_DIM, ws=self.ws)
        else:
            def fc6_grads(ws, sws, d=d):
                ops.colsum(d, G["dcnn/fc6b"], sws, n, FC_DIM)
                if self.dp is None:
                    ops.gemm(L5["p"], d, G["dcnn/fc6W"], self.flat_dim, FC_DIM, n, transa=True, ws=ws)
                    return
                # the exchange starts here: everything produced so far, then fc6W block by block -- block i is on the wire
                # (RCCL's stream, which waits for the stream these launches are on) while block i+1 is computed, and the whole 85 % of
                # the bytes before the conv backward is far along
                self._issue(f6o)
                flat_p = L5["p"].view(self.N, self.flat_dim)
                for r0, r1 in self.fc6_row_blocks:
                    ops.gemm(flat_p[:, r0:], d, G["dcnn/fc6W"][r0:r1], r1 - r0, FC_DIM, n, transa=True, lda=self.flat_dim)
                    self._issue(self._fc6_block_end(r1))
            param_grads(fc6_grads)
            if convs_train:
                ops.gemm(d, P["dcnn/fc6W"], L5["dp"], n, self.flat_dim, FC_DIM, transb=True, ws=self.ws)     # the chain: into pool5's gradient
        # ---- conv stack, last to first
        if side is not None:
            main.wait_event(self._wt_ready)

        def on_side(launch):
            side.wait_stream(torch.cuda.current_stream(self.dev))
            with torch.cuda.stream(side):
                launch()

        issue_at = max(kconv, 2)        # conv5 .. conv3 (or .. the first trainable layer) go out behind this layer's weight gradient
        if convs_train:
            issue_hi = sum(self.offsets["dcnn/%sb" % self.layers[issue_at]["name"]])      # flat offset behind that layer's gradients
        for li in reversed(range(kconv, len(self.layers))):
            L = self.layers[li]
            name, conv = L["name"], L["conv"]
            x_in = self.layers[li - 1]["out"][:n] if li > 0 else self.x0[:n]
            dy = L["dy"][:n]
            if L["pool"] and L["lrn"] and self.c8:
                # bf16 path: the gradient is only ever read packed (wgrad, dgrad, bias gradient) -- written packed, fp32 dy stays unused
                ops.pool_lrn_bwd_c8(L["yb"][:n], L["dp"][:n], L["arg"][:n], L["dyb"][:n], p_halo=L["p_halo"],
                                    dxb_halo=(L["eq"].dy_halo if li == 0 else L["dy_halo"]), relu_fused=True, **LRN)
            elif L["pool"] and L["lrn"]:
                # pool -> LRN -> ReLU backward in one pass: d(lrn out) is never written
                ops.pool_lrn_bwd(L["y"][:n], L["dp"][:n], L["arg"][:n], dy, p_halo=L["p_halo"], dx_halo=L["dy_halo"],
                                 relu_fused=True, **LRN)
            elif L["pool"]:
                self._pool_bwd(L, n, dy, L["y"][:n], L["dy_halo"])
            # else: dy was written (ReluGrad fused) by the next layer's dgrad epilogue
            if self.c8 and li == 0:
                eq = L["eq"]
                self._run(name + ".wgrad", eq.c8_wgrad, L["xb"][:n], L["dyb"][:n], L["dws2d"], self.ws)
                conv.s2d_weights(L["dws2d"], G["dcnn/%sW" % name], grad=True)
                ops.bias_grad_c8(L["dyb"][:n], G["dcnn/%sb" % name], sw, conv.cout, eq.dy_halo)
                continue
            if self.c8:
                if L["pool"] and not L["lrn"]:
                    ops.pack_c8(dy, L["dyb"][:n], L["dy_halo"], L["dy_halo"])
                self._run(name + ".wgrad", conv.c8_wgrad, L["xb"][:n], L["dyb"][:n], G["dcnn/%sW" % name], self.ws)
                ops.bias_grad_c8(L["dyb"][:n], G["dcnn/%sb" % name], sw, conv.cout, L["dy_halo"])
                if li == issue_at:
                    self._issue(issue_hi)
                if li == kconv:
                    continue                          # the layer below is frozen: no input gradient
                prev = self.layers[li - 1]
                conv.c8_pack_w(P["dcnn/%sW" % name], L["wbt"], True)
                if prev["pool"]:
                    self._run(name + ".dgrad", conv.c8_dgrad, L["dyb"][:n], L["wbt"], dx=prev["dp"][:n])
                else:      # straight into the previous conv's packed gradient; its ReluGrad reads this layer's packed input
                    self._run(name + ".dgrad", conv.c8_dgrad, L["dyb"][:n], L["wbt"], dxb=prev["dyb"][:n], relu_mask_c8=L["xb"][:n])
                continue
            # the side stream's OWN scratch: nothing the main stream launches meanwhile can touch it, whatever takes a workspace there later
            # conv1's weight gradient is the last launch of the pass and nothing on the chain follows it: on the launch stream it runs
            # beside what the second stream still holds instead of queueing behind it (64 clips 34.76 -> 34.71 ms, 8 clips 5.33 -> 5.29)
            last_on_main = side is not None and li == 0
            wws, wsw = (self.ws_side, self.small_ws_side) if (side is not None and not last_on_main) else (self.ws, sw)

            def wgrad(name=name, conv=conv, x_in=x_in, dy=dy, wws=wws, wsw=wsw, li=li):
                if conv.fuses_bias():      # bias gradient comes out of the same pass over dy
                    self._run(name + ".wgrad", conv.wgrad, x_in, dy, G["dcnn/%sW" % name], wws, db=G["dcnn/%sb" % name])
                else:
                    self._run(name + ".wgrad", conv.wgrad, x_in, dy, G["dcnn/%sW" % name], wws)
                    ops.bias_grad_nchw(dy, G["dcnn/%sb" % name], wsw)
                if li == issue_at:
                    # issued from the stream the weight gradients ran on: RCCL's stream waits for that stream only
                    self._issue(issue_hi)

            if side is None or last_on_main:
                wgrad()                               # (conv1's: the chain ends here -- beside what the second stream still holds)
            else:
                on_side(wgrad)                        # beside this layer's dgrad / the next pool backward
            if li > kconv:
                prev = self.layers[li - 1]
                wt = self.wt
                if side is not None:
                    wt = L["wt"]                      # transposed at the start of the backward pass
                else:
                    conv.wt_transpose(P["dcnn/%sW" % name], wt)
                if prev["pool"]:
                    self._run(name + ".dgrad", conv.dgrad, dy, wt, prev["dp"][:n])     # into the pool output gradient
                else:
                    self._run(name + ".dgrad", conv.dgrad, dy, wt, prev["dy"][:n], relu_mask=prev["y"][:n])
        if side is not None:
            torch.cuda.current_stream(self.dev).wait_stream(side)
        self._issue(self.plan.total)

    # ---- dropout on relu(fc6) / relu(fc7) (cfg.fc_dropout_keep_prob) ------------------------------------------------------------
    # In place and mask-free: a dropped output is > 0 exactly where the ReLU was active and the draw kept, so the ReluGrad sites of
    # f6 / f7 keep reading the same tensor and only gain the division by keep (vl_relu_dropout_grad).
    def _fc_dropout(self, layer, y):
        salt = fc_dropout_salt(self.cfg, layer)
        if self._tag_off is not None:             # captured: the seed follows the step state's count
            ops.fc_dropout_fwd_st(y, self.fc_keep, self.state, salt)
        else:
            ops.fc_dropout_fwd(y, self.fc_keep, dropout_seed(self._draw_index()), salt)

    def _sa_drop_bound(self):
        """self.sa_drop bound to the pass being issued: clip0 = rank * max_clips (the counters are those of the global batch), the seed
        of this draw index, or -- captured -- the step state it is formed from when the launches run."""
        clip0 = self.dp.rank * self.B if self.dp is not None else 0
        if self._tag_off is not None:
            return self.sa_drop.bind(clip0, state=self.state)
        return self.sa_drop.bind(clip0, seed=dropout_seed(self._draw_index()))

    def _rk(self, span):
        """The keywords of a cluster-recurrence launch that uses `span` exchange tags (temporal.gru_forward): eager the engine's
        workspace; captured the graph workspace with replay-safe tags from the step state, and the tag offset moves on."""
        if self._tag_off is None:
            return dict(ws=self.lstm_ws)
        kw = dict(ws=self.lstm_ws_graph, state=self.state, tag_offset=self._tag_off)
        self._tag_off += span
        return kw

    def _feat_grad(self, dg, K, n, W):
        """dfeat = dg K^T, the gradient of the temporal model's bottom input from its first layer's dg [n, W], with the ReluGrad of
        fc6 / fc7 fused into the product (behind it after a pass that dropped them).  A frozen tower: nobody reads dfeat."""
        if not self.dcnn_trains:
            return
        D = self.cfg.encode_dim()
        relu_mask = self.feat if self.f8 is None else None
        ops.gemm(dg, K, self.dfeat, n, D, W, transb=True, ldb=W, relu_mask=self._fused_mask(relu_mask), ws=self.ws)
        self._relu_grad_behind(self.dfeat, relu_mask, n * D)

    def _relu_grad(self, d, y, count):
        """ReluGrad of f6 / f7 on its own launch; after a forward pass that dropped them, with the dropout's gradient."""
        if self._fc_drop:
            ops.relu_dropout_grad(d, y, self.fc_keep, count)
        else:
            ops.relu_grad(d, y, count)

    def _fused_mask(self, relu_mask):
        """The relu_mask= a GEMM epilogue gets: after a forward pass that dropped f6 / f7 none -- _relu_grad_behind follows the GEMM."""
        return None if self._fc_drop else relu_mask

    def _relu_grad_behind(self, d, relu_mask, count):
        if self._fc_drop and relu_mask is not None:
            ops.relu_dropout_grad(d, relu_mask, self.fc_keep, count)

    def _draw_index(self, mi=None):
        """What the dropout seed is formed from: the micro-steps of one update draw different masks; with accumulate 1 the step count.
        mi: the micro-step (default: the one being issued)."""
        mi = mi if mi is not None else self._mi
        return self.step_count * self.accumulate + (mi[0] if mi is not None else 0)

    def _acc_tiers(self):
        return None if self.plan.full_range() else self.plan.tiers

    def _issue(self, hi):
        """Data parallel: starts the exchange of every chunk of the plan not yet issued that ends at or before flat offset `hi`.  The
        flat buffer is in the order backward produces the gradients, so the caller names the end of what the launches queued so far (on
        the current stream) have written."""
        if self.dp is None:
            return
        mi = self._mi
        if mi is not None and mi[0] < mi[1] - 1:
            return                                # a non-final micro-step: the exchange happens once per update
        while self._next_chunk < len(self.grad_chunks) and sum(self.grad_chunks[self._next_chunk]) <= hi:
            lo, cnt = self.grad_chunks[self._next_chunk]
            if mi is not None and mi[1] > 1:      # the final micro-step: g = gacc + g over the chunk, right before it goes out
                ops.grad_accumulate(self.gacc, self.g, ops.ACC_FINAL, [(lo, lo + cnt, 1.0)])
            self.dp.reduce_async(self.g, lo, cnt)
            self._next_chunk += 1

    def _fc6_block_end(self, r1):
        """Flat offset behind the fc6W row block ending at row r1; fc6b rides with the last block."""
        f6o, f6n = self.offsets["dcnn/fc6W"]
        end = f6o + r1 * FC_DIM
        return end if end < f6o + f6n else f6o + f6n + FC_DIM

    def _side_stream(self):
        """Second HIP stream of the backward pass, or None (VLTF_WGRAD_STREAM=0; the bf16 path).  Independent launches -- the dgrad
        weight transposes at the start of the pass, fc6's input gradient beside its weight-gradient blocks, a layer's weight gradient
        beside its input gradient and the next pool / LRN backward -- fill the CUs the tail of a launch leaves idle: same box, one
        stream -> two: 8 clips 5.71 -> 5.42 ms, 16 clips 10.1 -> 9.81, 32 clips 18.5 -> 18.2, 64 clips 35.64 -> 35.05 (round 3, once the
        transposes had left the critical chain; round 2 kept the full batch on one stream for a gain of 0.4 ms).  A bracket or a
        rocprof average of a launch that has a neighbour times both: bench.py takes its per-launch table from extra steps with
        VLTF_WGRAD_STREAM=0 and the dominant symbol, live, from its forward launches, which always run alone.
        Other schedules measured at 64 clips and dropped (35.75 ms on one stream then): conv5..conv3's weight gradients held back
        until conv2's pool / LRN backward, to hide that HBM-bound kernel under MFMA-bound ones -- 35.8 ms, next to a 135 KB-of-LDS
        wgrad workgroup a CU holds ONE pool / LRN workgroup, which then crawls (1.33 ms instead of 0.65) while the chain of input
        gradients waits for it; conv3's two launches each alone with the others paired -- 35.85, the joins cost what the pairs
        win; only conv2's weight gradient on the second stream, behind conv2's input gradient, so that it runs beside conv1's pool /
        LRN backward (off the critical chain) -- 36.03: an HBM-bound kernel beside an MFMA-bound one costs the latter more than it
        hides; which of dgrad / wgrad the host issues first: no difference.
        fp32 and the split-bf16 arithmetics (bf16x3 22.3 -> 21.5 ms).  Round 3 kept the latter on one stream because conv2's
        `pool_lrn_bwd` came out different from run to run beside conv3's split-product weight gradient.  Round 4 found the cause
        (DESIGN 6): not a race -- hipcc's SLP vectoriser had formed `v_pk_add_f32 ... op_sel:[0,1]` in that kernel, a packed-fp32 form
        that on MI355X returns src0.lo + 0 in lanes 48..63 while a kernel mixing v_cvt_pk / v_pk_add and bf16 MFMAs shares the CU
        (tools/ubench/pk_opsel_raw.hip reproduces it in 100 lines).  The library is built without SLP vectorisation and
        tests/test_isa_lint.py refuses the form in the built code objects.  The packed-bf16 PATH stays on one stream because it is
        slower on two (8.3 vs 8.2 ms)."""
        if os.environ.get("VLTF_WGRAD_STREAM", "") == "0" or self.cfg.conv_math == "bf16":
            return None
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream(device=self.dev)
            # Invariant of the two-stream backward: a launch on the side stream reads tensors the main stream has finished (it waits
            # for the main stream at the start of every layer), writes only its own gradient tensors, and takes its scratch from
            # THESE buffers, never from self.ws / self.small_ws -- so no main-stream launch between the fork and the join can race it.
            self.ws_side = torch.empty_like(self.ws)              # wgrad slabs / split-k slabs of what runs on the side stream
            self.small_ws_side = torch.empty_like(self.small_ws)
            for L in self.layers[1:]:
                L["wt"] = torch.empty(L["conv"].w_shape, device=self.dev).view(-1)
            self._wt_ready = torch.cuda.Event()
        return self._side

    def _pool_bwd(self, L, n, dx, relu_mask, dx_halo):
        ops.maxpool_bwd(L["dp"][:n], L["arg"][:n], dx, relu_mask=relu_mask, hwc=L["hwc"], dy_halo=L["p_halo"], dx_halo=dx_halo)

    # ---- train step ----------------------------------------------------------------------------
    def _train(self, n, b, onehot, lr, clip_norm, fetch, global_rows=None, mi=None):
        """mi: None, or the (i, k) MicroSequence.enter admitted (micro-step i of an update of k)."""
        if not self.training:
            raise VltfError("engine was built with training=False")
        if self.cfg.classifier == "none":
            raise VltfError("a feature pipeline (classifier none) has no loss of its own: it trains inside a GraphEngine")
        if onehot.dtype != torch.int32 or tuple(onehot.shape) != (self._rows_for(b, n), self.cfg.num_classes):
            raise VltfError("labels must be int32 one-hot of shape (%d, %d)" % (self._rows_for(b, n), self.cfg.num_classes))
        self._mi = mi
        try:
            self._erase_launch(n, b)              # random erasing: each clip's own box, ahead of the blend / the cut
            self._mix_launch(n, b)                # mixup: the clips just fed are blended in pairs before conv1 reads them
            rows = self._forward(n, b, train=True)
            world = self.dp.world if self.dp is not None else 1
            i, k = mi if mi is not None else (0, 1)
            if i == 0:                            # loss_sum / correct sum on the device over the micro-steps of an update
                ops.fill(self.stats, 0.0)
            # mean over the GLOBAL batch (train.py:123): each rank scales its rows by 1/global_rows and the all-reduce sums.
            # global_rows defaults to rows*world*k (equal shards, equal micro-batches); a workflow with ragged shards or unequal
            # micro-batches passes the true count of the whole update on every call.
            self._xent_launch(self.logits[:rows], onehot, self.dlogits, 1.0 / (global_rows or rows * world * k))
            self._backward(n, b)
        finally:
            self._mi = None
        total_rows = self.micro.add_rows(mi, rows)
        if i < k - 1:                             # not the update's last micro-step: g joins the running sum, nothing else happens
            ops.grad_accumulate(self.gacc, self.g, ops.ACC_STORE if i == 0 else ops.ACC_ADD, self._acc_tiers())
            return self._fetch(total_rows, fetch, partial=True)
        if k > 1 and self.dp is None:             # (data parallel: _issue added each chunk before it went out)
            ops.grad_accumulate(self.gacc, self.g, ops.ACC_FINAL, self._acc_tiers())
        return self._finish_step(total_rows, lr, clip_norm, fetch)

    def train_step_empty(self, lr, clip_norm=0.0, fetch=True, micro=None):
        """This rank's shard of the global batch is empty (fewer videos than ranks in a short last batch): contribute zero
        gradients to the exchange and apply the same update as every other rank.  As a micro-step it adds nothing to the update's sum."""
        if self.dp is None:
            raise VltfError("train_step_empty is a data-parallel call")
        mi = self.micro.enter(micro)
        i, k = mi if mi is not None else (0, 1)
        if i == 0:
            ops.fill(self.stats, 0.0)
        total_rows = self.micro.add_rows(mi, 0)
        if i < k - 1:
            if i == 0:                            # the group's sum must be defined for the micro-steps that follow
                for lo, hi, _ in self.plan.tiers:
                    ops.fill(self.gacc[lo:hi], 0.0)
            return self._fetch(total_rows, fetch, partial=True)
        for lo, hi, _ in self.plan.tiers:                # (frozen ranges of g are never written, read or exchanged)
            ops.fill(self.g[lo:hi], 0.0)
        for lo, cnt in self.grad_chunks:
            if k > 1:
                ops.grad_accumulate(self.gacc, self.g, ops.ACC_FINAL, [(lo, lo + cnt, 1.0)])
            self.dp.reduce_async(self.g, lo, cnt)
        return self._finish_step(total_rows, lr, clip_norm, fetch)

    def _finish_step(self, rows, lr, clip_norm, fetch):
        if self.dp is not None:
            self.dp.wait()
        tiers = None if self.plan.full_range() else self.plan.tiers      # None: the plain calls (one full-range tier, same bits)
        self._lars_stats_launch()                 # LARS: the norms of the raw gradient, before the regulariser writes over it
        if self.decay is not None:                # g <- g + decay w in place; self.ss = self.ss2[:1] is the regularised gradient's norm
            ops.l2_regularize(self.w, self.g, self.decay, self.ss2, self.small_ws)
        elif tiers is None:
            ops.sumsq(self.g, self.ss, self.small_ws)
        else:
            ops.sumsq_tiers(self.g, tiers, self.ss, self.small_ws)
        stats_step = self._stats_due()
        if stats_step:
            self._stats_launch(lr, clip_norm)
        self.step_count += 1
        # a step whose LSTM cluster launch timed out must not reach the weights -- also with fetch=False, where the host reads the
        # status only later: the optimizer launch drops the update on the device (ops.step_guard), check_status raises at the next fetch
        skip = ops.step_guard(self._skip, getattr(self, "lstm_ws", None), self.lstm_ws_graph)
        if self.lars is not None:
            self._lars_trust_launch(clip_norm, stats_step)
        if self.lamb is not None:                 # LAMB: two launches in the place of Adam's; g stays the raw gradient
            self._lamb_launch(lr, clip_norm, skip, stats_step, self._tag_off is not None)
        elif self._tag_off is not None:           # captured: lr and Adam's step size from the step state (written before each replay)
            if self.cfg.optimizer == "adam" and tiers is not None:
                ops.adam_apply_tiers_st(self.w, self.g, self.adam_m, self.adam_v, tiers, self.state, clip_norm, self.ss, 1.0, skip=skip)
            elif self.cfg.optimizer == "adam":
                ops.adam_apply_st(self.w, self.g, self.adam_m, self.adam_v, self.state, clip_norm, self.ss, 1.0, skip=skip)
            elif self.lars is not None:
                ops.lars_apply_st(self.w, self.g, self.mom, self.lars["ranges"], self.lars["trust"], self.state, self.momentum,
                                  self.nesterov, clip_norm, self.ss, 1.0, skip=skip)
            elif self.mom is not None:
                ops.momentum_apply_st(self.w, self.g, self.mom, self.state, self.momentum, self.nesterov, clip_norm, self.ss, 1.0,
                                      skip=skip, tiers=tiers)
            elif tiers is not None:
                ops.sgd_apply_tiers_st(self.w, self.g, tiers, self.state, clip_norm, self.ss, 1.0, skip=skip)
            else:
                ops.sgd_apply_st(self.w, self.g, self.state, clip_norm, self.ss, 1.0, skip=skip)
        elif tiers is not None and self.cfg.optimizer == "adam":
            ops.adam_apply_tiers(self.w, self.g, self.adam_m, self.adam_v, tiers, lr, self.step_count, clip_norm, self.ss, 1.0, skip=skip)
        elif self.cfg.optimizer == "adam":
            ops.adam_apply(self.w, self.g, self.adam_m, self.adam_v, lr, self.step_count, clip_norm, self.ss, 1.0, skip=skip)
        elif self.lars is not None:
            ops.lars_apply(self.w, self.g, self.mom, self.lars["ranges"], self.lars["trust"], lr, self.momentum, self.nesterov, clip_norm,
                           self.ss, 1.0, skip=skip)
        elif self.mom is not None:
            ops.momentum_apply(self.w, self.g, self.mom, lr, self.momentum, self.nesterov, clip_norm, self.ss, 1.0, skip=skip, tiers=tiers)
        elif tiers is not None:
            ops.sgd_apply_tiers(self.w, self.g, tiers, lr, clip_norm, self.ss, 1.0, skip=skip)
        else:
            ops.sgd_apply(self.w, self.g, lr, clip_norm, self.ss, 1.0, skip=skip)
        self._ema_launch(skip)
        return self._fetch(rows, fetch)

    def _fetch(self, rows, fetch, partial=False):
        """partial: a micro-step before the update's last -- the running sums of the update so far, no norm yet."""
        if not fetch:
            return None
        torch.cuda.synchronize(self.dev)
        self.check_status()
        st = self.stats.cpu().numpy()
        if partial:
            return self._fetch_topk({"loss": float(st[0]) / max(rows, 1), "accuracy": float(st[1]) / max(rows, 1), "rows": rows,
                                     "loss_sum": float(st[0]), "correct": float(st[1])}, st, rows)
        out = {"loss": float(st[0]) / max(rows, 1), "accuracy": float(st[1]) / max(rows, 1), "grad_norm": math.sqrt(float(self.ss.item())),
               "rows": rows, "loss_sum": float(st[0]), "correct": float(st[1])}
        self._fetch_topk(out, st, rows)
        if self.ss2 is not None:                  # the regulariser at the weights the forward pass used; `loss` stays the data loss
            out["reg_loss"] = float(self.ss2[1].item())
        return self._stats_result(out)

    def _rows_for(self, b, n):
        if self.cfg.classifier == "lstm":
            return n if self.per_step else b
        return b if (self.early or self.late) else n

    def train_step_u8(self, frames_u8, onehot, lr, clip_norm=0.0, mean_bgr=None, crop_y=None, crop_x=None, mirror=None,
                      fetch=True, global_rows=None, resize=None, micro=None, mix_lambda=None, cut_box=None, crop_box=None,
                      erase_boxes=None):
        """sess.run([summaries, loss, lr, global_step, optimizer], fdict) (run_task.py:44).
        crop_box: a box per frame in the place of crop_y / crop_x (feed_u8); refused together with them.
        micro = (i, k): micro-step i of an update that sums k of them (k <= cfg.accumulate), called in order i = 0 .. k - 1.  Only the
        last one exchanges, regularises, clips and updates, with its lr; the others return the running loss of the update and no
        grad_norm.  The loss is scaled by 1 / (rows * world * k) unless global_rows gives the rows of the whole update.
        mix_lambda: with mixup on (cfg.mixup_alpha > 0), this step's blend weight in [0, 1] in the place of the draw (folded to
        max(lam, 1 - lam)); refused with mixup off.
        cut_box: with CutMix on (cfg.cutmix_alpha > 0), this step's box (t0, t1, y0, y1, x0, x1) in the place of the draw; refused with
        CutMix off, outside the frame, reversed, above half the clip's volume, or together with mix_lambda (check_cut_box).
        erase_boxes: with random erasing on (cfg.erase_prob > 0), one box (t0, t1, y0, y1, x0, x1) per clip in the place of the drawn
        ones (the noise keys are still drawn); refused with erasing off, outside the frame or reversed (check_erase_boxes)."""
        self._check_crop_box(crop_box, crop_y, crop_x)
        mi = self.micro.enter(micro)
        try:
            self._mix_write(mix_lambda, mi, cut_box)
            self._erase_write(erase_boxes, mi, frames_u8)
            if self.step_graph:
                done, out = self._graph_step(True, frames_u8, mean_bgr, crop_y, crop_x, mirror, resize, onehot, lr, clip_norm, fetch,
                                             global_rows, mi, crop_box=crop_box)
                if done:
                    return out
            n, b = self.feed_u8(frames_u8, mean_bgr, crop_y, crop_x, mirror, resize, crop_box)
            return self._train(n, b, onehot, lr, clip_norm, fetch, global_rows, mi)
        except VltfError:
            self.micro.reset()
            raise

    def train_step_f32(self, frames_nhwc, onehot, lr, clip_norm=0.0, fetch=True, global_rows=None, micro=None, mix_lambda=None,
                       cut_box=None, erase_boxes=None):
        mi = self.micro.enter(micro)
        try:
            self._mix_write(mix_lambda, mi, cut_box)
            self._erase_write(erase_boxes, mi, frames_nhwc)
            n, b = self.feed_f32_nhwc(frames_nhwc)
            return self._train(n, b, onehot, lr, clip_norm, fetch, global_rows, mi)
        except VltfError:
            self.micro.reset()
            raise

    # ---- captured steps (NetConfig.step_graph, class docstring) ---------------------------------------------------------------
    def _graph_step(self, train, frames_u8, mean_bgr, crop_y, crop_x, mirror, resize, onehot=None, lr=0.0, clip_norm=0.0, fetch=True,
                    global_rows=None, mi=None, crop_box=None):
        """(True, the call's result) when the call was replayed; (False, None) when it runs eagerly (the first call of its key)."""
        rz = tuple((tuple(int(v) for v in s_), tuple(int(v) for v in d_)) for s_, d_ in (resize or ()))
        key = ("train" if train else "forward", int(frames_u8.shape[0]), tuple(frames_u8.shape[1:]), rz, crop_y is not None,
               crop_x is not None, mirror is not None, mean_bgr is not None, float(clip_norm) if train else None,
               global_rows if train else None, self.cfg.dropout_keep_prob if train else None, crop_box is not None)
        if train and self.accumulate > 1:     # first / middle / last micro-steps are different launch sequences: a graph each
            key += MicroSequence.role(mi)
        final = mi is None or mi[0] == mi[1] - 1
        stats = train and final and self._stats_due()
        if train and self.stat_segs is not None:  # a stats step and a plain step are different launch sequences too
            key += (stats,)
        g = self._graphs.get(key)
        if g is None:
            if key not in self._graph_warm:   # warm-up: one-time set-up (function attributes, tables, resizers, side-stream buffers)
                self._graph_warm.add(key)
                return False, None
            g = self._graphs[key] = self._capture(train, frames_u8, mean_bgr, crop_y, crop_x, mirror, resize, onehot, clip_norm,
                                                  global_rows, mi, crop_box)
        for name, t in (("frames", frames_u8), ("crop_y", crop_y), ("crop_x", crop_x), ("mirror", mirror), ("onehot", onehot),
                        ("crop_box", crop_box)):
            dst = g["inputs"].get(name)
            if dst is None:
                continue
            if t.dtype != dst.dtype or tuple(t.shape) != tuple(dst.shape) or t.device != dst.device:
                raise VltfError("%s: %s %s on %s, the captured step reads %s %s" % (name, t.dtype, tuple(t.shape), t.device, dst.dtype,
                                                                                  tuple(dst.shape)))
            dst.copy_(t)
        if mean_bgr is not None:
            self.mean_dev.copy_(torch.as_tensor(np.asarray(mean_bgr, np.float32)), non_blocking=True)
        draw = self._draw_index(mi)
        if draw == self.step_count:
            ops.step_state_set(self.state, self.step_count, lr, self._graph_tag_origin(g["span"]))
        else:                                     # accumulation: the dropout seed follows the draw index, Adam's step size the update count
            ops.step_state_set_micro(self.state, self.step_count, draw, lr, self._graph_tag_origin(g["span"]))
        if train and final and self.ema is not None:      # the update this replay applies follows step_count earlier ones
            ops.step_state_set_ema(self.state, ema_rate(self.ema_decay, self.ema_warmup, self.step_count))
        if train and final and self.lamb is not None:     # likewise LAMB's bias corrections
            ops.step_state_set_lamb(self.state, *lamb_corrections(self.step_count))
        g["graph"].replay()
        self._rows = g["rows"]
        if not train:
            return True, self.logits[:g["rows"]]
        total_rows = self.micro.add_rows(mi, g["rows"])
        if mi is not None and mi[0] < mi[1] - 1:
            return True, self._fetch(total_rows, fetch, partial=True)
        if stats:
            self._stats_note(lr, clip_norm)
        self.step_count += 1
        return True, self._fetch(total_rows, fetch)

    def _graph_tag_origin(self, span):
        """Tag origin of the next replay on lstm_ws_graph (its launches use origin + 1 .. origin + span - 1).  Past the limit the exchange
        words are zeroed on the stream, outside any graph, and the tags start over at 1."""
        if self.graph_tag_next + span > self.GRAPH_TAG_LIMIT:
            ops.lstm_seq_ws_clear(self.lstm_ws_graph)
            self.graph_tag_next = 1
        origin = self.graph_tag_next
        self.graph_tag_next += span
        return origin

    def _capture(self, train, frames_u8, mean_bgr, crop_y, crop_x, mirror, resize, onehot, clip_norm, global_rows, mi=None,
                 crop_box=None):
        """Captures one call over static input buffers.  Nothing runs and no host state moves: the replay that follows is the step."""
        t0 = time.perf_counter()
        inputs = {name: torch.empty_like(t) for name, t in (("frames", frames_u8), ("crop_y", crop_y), ("crop_x", crop_x),
                                                              ("mirror", mirror), ("onehot", onehot), ("crop_box", crop_box))
                  if t is not None}
        n = frames_u8.shape[0]
        b = self._check_frames(n)
        # every buffer the capture bakes in lives as long as the graph: the resize chain's outputs and intermediates are the graph's
        # own (a resizer's shared intermediate is replaced when a larger batch comes, and would then be freed under the graph)
        chain = []
        for src_hw, dst_hw in (resize or ()):
            rs = self._resizers[(tuple(src_hw), tuple(dst_hw))]                               # made by the warm-up call
            need = rs.tmp_bytes(n)
            chain.append((rs, torch.empty((n, rs.oh, rs.ow, 3), dtype=torch.uint8, device=self.dev),
                          torch.empty(need, dtype=torch.uint8, device=self.dev) if need else None))
        graph = torch.cuda.CUDAGraph()
        step_count, acc_rows = self.step_count, self.micro.rows
        self._tag_off = 0
        # No finaliser may run inside the capture: releasing a conv or resize descriptor frees device tables (hipFree), which a thread-local
        # capture on this thread does not allow -- it invalidates the capture.  Engines that sit in reference cycles (a GraphEngine and the
        # towers it owns) are released by the cycle collector only, at a moment of its choosing: collect them now, and keep the collector
        # off until the capture has ended.
        gc.collect()
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                frames = inputs["frames"]
                for rs, dst, tmp in chain:
                    frames = rs(frames, dst=dst, tmp=tmp)
                self._feed_dev(frames, n, b, self.mean_dev if mean_bgr is not None else None, inputs.get("crop_y"), inputs.get("crop_x"),
                               inputs.get("mirror"), inputs.get("crop_box"))
                if train:
                    self._train(n, b, inputs["onehot"], 0.0, clip_norm, False, global_rows, mi)
                    rows = self._rows
                else:
                    rows = self._forward(n, b, train=False)
            span = self._tag_off
        finally:
            if gc_was_on:
                gc.enable()
            self._tag_off = None
            self.step_count, self.micro.rows = step_count, acc_rows
        self.graph_capture_ms.append((time.perf_counter() - t0) * 1e3)
        return dict(graph=graph, inputs=inputs, rows=rows, span=span, resize_buffers=[(dst, tmp) for _, dst, tmp in chain])
