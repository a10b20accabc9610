"""GraphEngine: the reference's Model for ANY ordered list of pipelines (models/model.py:18-162).

Model.__init__ builds the pipelines in the order of the YAML list; an input of a pipeline is a dataset tag (a placeholder fed
from that dataset) or the output of an earlier pipeline; the LAST pipeline's output is the logits the loss is taken on
(model.py:157-162).  Model.build_pipeline (model.py:18-155) gives every pipeline the same five stages, each optional:

  inputs -> [input_fusion avg | maximum | concat | ibias  (apply_tensor_list_fusion, tf_util.py:136-179)]
         -> representation dcnn | nop | fc                (vectorizer.py: AlexNet tower / identity / convert_dim_fc "fc_convert")
         -> [early frame fusion                           (aggregate_clip_vectors, tf_util.py:126-133)]
         -> classifier None | fc | lstm                   (None: a feature pipeline, model.py:110-112; lstm: without input_fusion a
                                                           SECOND input is the LSTM's state vector, model.py:128-134)
         -> [late frame fusion]

Here a pipeline is a PipeNode: an optional AlexNet tower (an LRCNEngine built as a feature pipeline: conv stack + fc6..fc8 and
their backward, nothing else) and the generic stages around it, all on the C-ABI kernels of vltf_amd.ops.  Examples it builds:
the two-stream LRCN (dcnn on `main`, dcnn on `aux`, a third pipeline fusing them by avg | maximum | concat into an LSTM), the
encoder-decoder of BASELINE config 4 (vltf_amd.composed.ComposedEngine is this class behind its old two-pipeline interface),
feature pipelines consumed by several later ones (their gradients add up).

Variables: with more than one pipeline every variable is scoped "<pipeline>/<tf name>" (in the reference a second dcnn gets TF's
automatic "dcnn_1/" scope and a second LSTM / fc_convert cannot be created at all: tf.get_variable refuses the duplicate name).
ALL parameters live in one flat buffer ordered last pipeline first and, inside a pipeline, head before tower = the order backward
produces the gradients; global-norm clip, update and the data-parallel exchange run over the whole buffer as for one pipeline.
A pipeline the last one does not depend on is never evaluated by sess.run(logits) and is not built (a warning says so).

Per-clip sequence lengths (tf.nn.dynamic_rnn's sequence_length, lstm.py:132-142; the `nonzero` value of the LSTM.build plug point):
forward / train_step take seq_len = {pipeline name: host int32 lengths, one per clip of that `classifier: lstm` pipeline}.  Steps
at or beyond a clip's length are dead: the recurrence of every layer carries the state through them and outputs zero, fusion
state | last | avg read the live prefix only, and when the last pipeline's fusion is `reshape` the loss, its gradient and the
accuracy are taken over the live rows (the reference's non_padding_index, dataset_.py:327-383).  A self-attention layer (rnn_cell
mhsa) attends over the live keys only and never reads a dead row of its projections; the first layer takes its input through
ops.live_rows, so that a padded frame's features reach no product; with sa_block encoder it is the embedding that reads
through ops.live_rows, and the norm launches skip dead rows and write zeros there.  include/vltf.h states the
contract of the kernels; without seq_len every call is what it was.

The oracle of this class is oracle.lrcn_oracle.model_forward / model_backward (cross-checked against torch autograd)."""
import math
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import ops
from ._ffi import MAX_LR_TIERS, VltfError
from .engine import (FORGET_BIAS, LRCNEngine, MicroSequence, NetConfig, check_accumulate, check_class_weights, check_cutmix, check_ema,
                     check_erase, check_fc_dropout, check_focal_gamma, check_label_smoothing, check_label_type, check_lamb, check_lars,
                     check_mixup, check_momentum, check_top_k, check_weight_decay, dcnn_layers, decay_ranges, dropout_seed, finetune_plan,
                     frozen_layers, param_specs, tier_plan)
from .temporal import (attn_backward, attn_buffers, attn_forward, attn_specs, blstm_backward, blstm_buffers, blstm_forward, blstm_names,
                       check_attn, check_blstm, check_mhsa, check_rnn_cell, check_sa_block, check_tcn, check_vlad, embed_grads,
                       encoder_backward, encoder_buffers, encoder_forward, encoder_specs, encoder_var, gru_backward, gru_buffers,
                       gru_forward, gru_names, gru_specs, mhsa_backward, mhsa_buffers, mhsa_forward, mhsa_names, mhsa_specs, sa_drop_of,
                       tcn_backward, tcn_buffers, tcn_dilations, tcn_forward, tcn_specs, tcn_var, vlad_buffers, vlad_backward,
                       vlad_forward, vlad_specs)


@dataclass
class PipelineSpec:
    """One entry of `network: pipelines:` (settings_.py:167-208)."""
    name: str
    input: List[str]                                # dataset tags and / or names of earlier pipelines
    representation: str = "nop"                     # dcnn | nop | fc
    frame_encoding_layer: Optional[str] = None      # dcnn
    fc_output_dim: Optional[int] = None             # fc
    classifier: Optional[str] = None                # None | fc | lstm
    lstm_params: Optional[Tuple[int, int, str]] = None   # (hidden, layers, fusion avg | last | reshape | state | attn | vlad)
    attn_dim: Optional[int] = None                  # fusion attn: the width of the attention scorer (engine.attn_specs); None = the LSTM's output width
    vlad_clusters: Optional[int] = None             # fusion vlad: the number of NetVLAD centres (engine.vlad_specs), 2..64; None = 8
    lstm_bidirectional: bool = False                # classifier lstm: a forward and a backward cell per layer, outputs concatenated (2H wide)
    rnn_cell: str = "lstm"                          # classifier lstm: its cell, lstm | gru (engine.gru_names; no state input, H <= 512)
                                                    # | mhsa: every layer a multi-head self-attention layer over the frames (engine.mhsa_names)
    sa_heads: Optional[int] = None                  # rnn_cell mhsa: heads (divides the width); None = 4 where 4 divides it, else 1
    sa_positions: Optional[str] = None              # rnn_cell mhsa: relative (None) | none
    tcn_kernel: Optional[int] = None                # rnn_cell tcn (engine.tcn_specs): the taps of every layer's dilated convolution, 1..9; None = 3
    tcn_dilation: Optional[str] = None              # rnn_cell tcn: exponential (None: layer l dilates by 2^l) | none
    tcn_causal: Optional[bool] = None               # rnn_cell tcn: True = a step sees itself and the past only; None / False = centred
    sa_block: Optional[str] = None                  # rnn_cell mhsa: plain (None) | encoder: the pre-LN encoder block (engine.encoder_specs)
    sa_ffn_dim: Optional[int] = None                # sa_block encoder: the feed-forward width, 8..4096; None = 4 x the width
    sa_attn_dropout: Optional[float] = None         # rnn_cell mhsa: dropout rate on the softmax weights in a training forward, [0, 1); None / 0 = off
    sa_dropout: Optional[float] = None              # sa_block encoder: dropout rate on the elements of the two residual branches; None / 0 = off
    sa_drop_path: Optional[float] = None            # sa_block encoder: stochastic depth, the linear rule 1 - p (l + 1) / L; None / 0 = off
    frame_fusion: Optional[Tuple[str, str]] = None  # (early | late | none, avg | last | reshape)
    input_fusion: Optional[str] = None              # avg | maximum | concat | ibias
    train_from: Optional[str] = None                # dcnn: first trainable layer of the tower (engine.TRAIN_FROM); not a reference key


@dataclass
class DatasetInfo:
    """What the graph needs to know about the dataset behind a tag (dataset_.py: the .size sidecar decides mode, fpc, cpv)."""
    mode: str                                       # "video" (frames) | "vectors"
    fpc: int
    cpv: int
    max_clips: int                                  # most clips of this dataset in one batch
    image_shape: Optional[Tuple[int, int, int]] = None
    dim: Optional[int] = None                       # vectors


@dataclass
class _Src:
    kind: str               # "video" | "vectors" | "pipe"
    ref: object             # dataset tag, or the producing PipeNode
    dim: int
    cpv: int
    fpc: int
    max_rows: int
    rows: int = 0
    tensor: object = None


def _trunc_normal(rng, shape, sd):
    v = rng.standard_normal(shape)
    bad = np.abs(v) > 2.0
    while bad.any():
        v[bad] = rng.standard_normal(int(bad.sum()))
        bad = np.abs(v) > 2.0
    return (v * sd).astype(np.float32)


class PipeNode:
    """One pipeline of the graph (Model.build_pipeline, model.py:18-155)."""

    def __init__(self, g, spec: PipelineSpec, srcs, index):
        self.g, self.spec, self.srcs, self.index = g, spec, srcs, index
        self.scope = spec.name + "/" if g.scoped else ""
        s, C = spec, g.num_classes
        ftype, fmethod = s.frame_fusion if s.frame_fusion else (None, None)
        if ftype == "none":
            ftype = None
        if ftype is not None and fmethod == "attn":
            raise VltfError("pipeline [%s]: frame_fusion attn is not built: attention pooling is a fusion of the recurrent classifier "
                            "(lstm_params)" % s.name)
        if ftype is not None and fmethod == "vlad":
            raise VltfError("pipeline [%s]: frame_fusion vlad is not built: NetVLAD pooling is a fusion of the recurrent classifier "
                            "(lstm_params)" % s.name)
        if ftype is not None and fmethod not in ("avg", "last", "reshape"):
            raise VltfError("Undefined frame fusion type : %s" % fmethod)                 # apply_temporal_fusion, tf_util.py:28-29
        if s.input_fusion == "vlad":
            raise VltfError("pipeline [%s]: input_fusion vlad is not built: NetVLAD pooling is a fusion of the recurrent classifier "
                            "(lstm_params)" % s.name)
        if s.classifier != "lstm" and (s.vlad_clusters not in (None, "None") or (s.lstm_params and s.lstm_params[2] == "vlad")):
            raise VltfError("pipeline [%s]: lstm_params fusion vlad / vlad_clusters need classifier lstm, not [%s]" % (s.name, s.classifier))
        if s.input_fusion == "attn":
            raise VltfError("pipeline [%s]: input_fusion attn is not built: attention pooling is a fusion of the recurrent classifier "
                            "(lstm_params)" % s.name)
        lf = s.lstm_params[2] if (s.classifier == "lstm" and s.lstm_params) else None
        if s.classifier != "lstm" and (s.attn_dim not in (None, "None") or (s.lstm_params and s.lstm_params[2] == "attn")):
            raise VltfError("pipeline [%s]: lstm_params fusion attn / attn_dim need classifier lstm, not [%s]" % (s.name, s.classifier))
        if s.classifier is None and ftype == "late":
            raise VltfError("Specified late fusion with no classifier selected")          # model.py:36-37
        if s.classifier not in (None, "fc", "lstm"):
            raise VltfError("Undefined classifier [%s]" % s.classifier)
        self.is_gru = check_rnn_cell(s.rnn_cell, s.classifier, s.lstm_params[0] if (s.classifier == "lstm" and s.lstm_params) else 1, s.lstm_bidirectional,
                                     what="pipeline [%s]: rnn_cell" % s.name) == "gru"
        if s.representation not in ("dcnn", "nop", "fc"):
            raise VltfError("Undefined representation [%s]" % s.representation)
        if s.input_fusion not in (None, "avg", "maximum", "concat", "ibias"):
            raise VltfError("Unknown fusion method: [%s]" % s.input_fusion)               # tf_util.py:178-179
        if s.train_from is not None and s.representation != "dcnn":
            raise VltfError("pipeline [%s]: train_from freezes dcnn layers, the representation is [%s]" % (s.name, s.representation))
        self.cpv_out = srcs[-1].cpv            # model.py:44-59: `cpv` is the loop variable = the LAST input's, whatever the fusion does
        # ---- stage 0: the pipeline's main tensor after the optional input fusion: (dim, fpc, max rows) ----------------------------
        self.tower = None
        self.fusion = s.input_fusion
        self.state_src = None
        if s.representation == "dcnn":
            # the placeholder(s) hold frames; DCNN.build wants rank-3 items (vectorizer.py:47)
            seq = srcs if self.fusion else srcs[:1]
            if any(x.kind != "video" for x in seq):
                raise VltfError("The [dcnn] vectorizer required input tensors of rank [3], but pipeline [%s] feeds it vectors" % s.name)
            if self.fusion not in (None, "avg", "maximum"):
                raise VltfError("input_fusion [%s] of frame tensors is not built (avg | maximum of equally shaped frames only)" % self.fusion)
            shapes = {tuple(g.datasets[x.ref].image_shape) for x in seq}
            if len(shapes) != 1 or len({(x.fpc, x.max_rows) for x in seq}) != 1:
                raise VltfError("pipeline [%s]: the fused frame datasets differ in shape / frames per clip" % s.name)
            self.fpc = seq[0].fpc
            cfg = NetConfig(image_shape=shapes.pop(), num_classes=C, fpc=self.fpc, frame_encoding_layer=s.frame_encoding_layer,
                            classifier="none", optimizer=g.optimizer, conv_math=g.conv_math, train_from=s.train_from,
                            fc_dropout_keep_prob=getattr(g, "fc_dropout_keep_prob", 0.0), fc_dropout_salt=1 + index)
            self.tower_cfg = cfg
            self.tower_trains = len(frozen_layers(cfg)) < len(dcnn_layers(cfg))     # False: the tower's backward is never called
            self.x_dim, self.max_rows0 = cfg.encode_dim(), seq[0].max_rows
        elif self.fusion in ("avg", "maximum"):
            if len({(x.dim, x.max_rows) for x in srcs}) != 1:
                raise VltfError("pipeline [%s]: input_fusion %s needs equally shaped inputs (widths / rows %s)" %
                                (s.name, self.fusion, [(x.dim, x.max_rows) for x in srcs]))
            self.x_dim, self.fpc, self.max_rows0 = srcs[0].dim, srcs[0].fpc, srcs[0].max_rows
        elif self.fusion in ("concat", "ibias"):
            if len(srcs) != 2:
                raise VltfError("pipeline [%s]: input_fusion %s takes exactly two inputs (tf_util.py:137-140,184)" % (s.name, self.fusion))
            a, b = srcs
            self.ratio = int(a.cpv / b.cpv)
            if self.fusion == "concat" and self.ratio == 1:          # tf.concat(inputs, axis=1), tf_util.py:147-148
                if a.max_rows != b.max_rows:
                    raise VltfError("input_fusion concat at clips-per-video ratio 1 concatenates row by row: the inputs of pipeline "
                                    "[%s] have %d and %d rows per batch; it needs a ratio > 1 to tile a per-clip vector over a "
                                    "sequence" % (s.name, a.max_rows, b.max_rows))
                self.x_dim, self.fpc, self.max_rows0 = a.dim + b.dim, a.fpc, a.max_rows
            elif self.fusion == "concat":                            # vec_seq_concat, vector first (tf_util.py:99-124,150-152)
                self._check_aux_rows(a, b)
                self.x_dim, self.fpc, self.max_rows0 = a.dim + b.dim, a.fpc, a.max_rows
            else:                                                    # ibias: the vector becomes time step 0 (tf_util.py:154-176)
                if a.dim != b.dim:
                    raise VltfError("input_fusion ibias needs equal widths (the sequence %d, the vector %d)" % (a.dim, b.dim))
                self._check_aux_rows(a, b)
                self.x_dim, self.fpc, self.max_rows0 = a.dim, a.fpc + 1, a.max_rows // a.fpc * (a.fpc + 1)
        else:
            self.x_dim, self.fpc, self.max_rows0 = srcs[0].dim, srcs[0].fpc, srcs[0].max_rows
        if s.representation != "dcnn" and any(x.kind == "video" for x in (srcs if self.fusion else srcs[:1])):
            # a frame placeholder is rank 4: convert_dim_fc / the LSTM's reshape cannot take it (only DCNN.build can)
            raise VltfError("pipeline [%s]: representation %s cannot take the frame dataset [%s] (representation dcnn does)" %
                            (s.name, s.representation, [x.ref for x in srcs if x.kind == "video"][0]))
        if self.fusion is None and len(srcs) > 1:
            if s.classifier != "lstm":
                raise VltfError("pipeline [%s] has %d inputs but neither an input_fusion nor an LSTM classifier that would take the "
                                "second one as its state" % (s.name, len(srcs)))
            if len(srcs) != 2:
                raise VltfError("pipeline [%s]: an LSTM takes one state input (tf_util.py:184: too many values to unpack)" % s.name)
            self.state_src = srcs[1]
            check_rnn_cell(s.rnn_cell, state_input=True, what="pipeline [%s]: rnn_cell" % s.name)
            if self.state_src.kind == "video":
                raise VltfError("pipeline [%s]: the LSTM's state input must be vectors or a pipeline output, [%s] holds frames" %
                                (s.name, self.state_src.ref))
            self.state_ratio = int(srcs[0].cpv / srcs[1].cpv)
            if self.state_ratio < 1 or srcs[1].max_rows * self.state_ratio * self.fpc != self.max_rows0:
                raise VltfError("pipeline [%s]: the state input has %d rows per batch, the sequence %d clips at clips-per-video ratio "
                                "%d" % (s.name, srcs[1].max_rows, self.max_rows0 // self.fpc, self.state_ratio))
        # ---- stage 1: representation ------------------------------------------------------------------------------------------------
        dim = self.x_dim
        self.rep_fc = s.representation == "fc" and s.fc_output_dim != dim
        if s.representation == "fc":
            if not s.fc_output_dim:
                raise VltfError("pipeline [%s]: representation fc needs fc_output_dim" % s.name)
            dim = int(s.fc_output_dim)
        self.feat_dim = dim
        # ---- stage 2: early fusion ---------------------------------------------------------------------------------------------------
        self.early = ftype == "early" and self.fpc > 1 and fmethod != "reshape"      # `reshape` of [B, T, d] back to [B*T, d]: identity
        self.fmethod = fmethod
        out_fpc = 1 if (ftype == "early" and self.fpc > 1) else self.fpc              # model.py:103-106
        rows = self.max_rows0 // self.fpc if self.early else self.max_rows0
        # ---- stage 3: classifier ----------------------------------------------------------------------------------------------------------
        self.cls = s.classifier
        self.late = False
        if self.cls is None:
            self.tc = check_tcn(s.rnn_cell, tcn_kernel=s.tcn_kernel, tcn_dilation=s.tcn_dilation, tcn_causal=s.tcn_causal)   # the keys alone: refused
            self.out_dim, self.fpc_out, self.max_rows = dim, out_fpc, rows
        else:
            if self.cls == "fc":
                self.cls_fc = dim != C
                if self.cls_fc and self.rep_fc:
                    raise VltfError("Variable %sfc_convert_w already exists (representation fc and classifier fc of one pipeline)" % self.scope)
            else:
                if self.fpc == 1:
                    raise VltfError("The LSTM classifier requires an fpc greater than 1")                     # model.py:121
                if ftype is not None:
                    raise VltfError("The LSTM classifier should be used only with [none] fusion, but it's [%s]" % ftype)
                self.H, self.L, self.lfusion = int(s.lstm_params[0]), int(s.lstm_params[1]), s.lstm_params[2]
                if self.lfusion not in ("avg", "last", "reshape", "state", "attn", "vlad"):
                    raise VltfError("Undefined frame fusion type : %s" % self.lfusion)
                self.per_step = self.lfusion == "reshape"
                self.head_name = "fc_convert" if self.lfusion == "state" else "output_fc"
                self.bi = bool(s.lstm_bidirectional)
                self.HO = 2 * self.H if self.bi else self.H       # width of the LSTM's output and of the head's input
                if self.bi:
                    check_blstm(self.H, "pipeline [%s]: lstm_bidirectional" % s.name)
                    if self.state_src is not None:
                        raise VltfError("pipeline [%s]: a bidirectional LSTM takes no state input ([%s]): the reference hands ONE vector to "
                                        "every cell as c = h, and which of the two directions it would initialise is not defined" %
                                        (s.name, self.state_src.ref))
                # fusion attn: learned attention pooling (engine.check_attn); None for every other fusion
                self.attn_dim = check_attn(lf, s.attn_dim, "lstm", self.HO, what="pipeline [%s]: attn_dim" % s.name)
                # fusion vlad: NetVLAD pooling (engine.check_vlad); None for every other fusion.  HW: the head's input width, K x HO
                self.vlad_k = check_vlad(lf, s.vlad_clusters, "lstm", self.HO, what="pipeline [%s]: vlad_clusters" % s.name)
                self.HW = (self.vlad_k or 1) * self.HO
                # rnn_cell mhsa: (heads, positions) of the self-attention layers (engine.check_mhsa); None for every other cell
                self.sa = check_mhsa(s.rnn_cell, self.H, self.fpc, s.sa_heads, s.sa_positions, self.lfusion,
                                     what="pipeline [%s]: rnn_cell" % s.name, sa_block=s.sa_block, sa_ffn_dim=s.sa_ffn_dim,
                                     sa_attn_dropout=s.sa_attn_dropout, sa_dropout=s.sa_dropout, sa_drop_path=s.sa_drop_path)
                # sa_attn_dropout / sa_dropout / sa_drop_path (engine.SaDrop), salted by the node index as the head's dropout is
                self.sa_drop = sa_drop_of(s, self.L, 1 + index) if self.sa else None
                # sa_block encoder: the feed-forward width of the blocks (engine.check_sa_block); None for the plain layer
                self.sa_ffn = check_sa_block(s.rnn_cell, self.H, s.sa_block, s.sa_ffn_dim)
                # rnn_cell tcn: (k, dilations, causal) of the convolution stack (engine.check_tcn); None for every other cell
                tc = check_tcn(s.rnn_cell, self.H, self.L, s.tcn_kernel, s.tcn_dilation, s.tcn_causal, self.lfusion,
                               what="pipeline [%s]: rnn_cell" % s.name)
                self.tc = (tc[0], tcn_dilations(tc[1], self.L), tc[2]) if tc else None
                if self.HW != C and self.head_name == "fc_convert" and self.rep_fc:
                    raise VltfError("Variable %sfc_convert_w already exists (representation fc and LSTM fusion state)" % self.scope)
                rows = rows if self.per_step else rows // self.fpc
            if s.lstm_bidirectional and self.cls != "lstm":
                raise VltfError("pipeline [%s]: lstm_bidirectional needs classifier lstm, not [%s]" % (s.name, self.cls))
            if self.cls != "lstm":
                self.sa = check_mhsa(s.rnn_cell, sa_heads=s.sa_heads, sa_positions=s.sa_positions, sa_block=s.sa_block,
                                     sa_ffn_dim=s.sa_ffn_dim, sa_attn_dropout=s.sa_attn_dropout, sa_dropout=s.sa_dropout,
                                     sa_drop_path=s.sa_drop_path)                                         # the keys without the cell: refused
                self.sa_ffn = self.sa_drop = None
                self.tc = check_tcn(s.rnn_cell, tcn_kernel=s.tcn_kernel, tcn_dilation=s.tcn_dilation, tcn_causal=s.tcn_causal)
            self.late = ftype == "late" and self.fpc > 1 and fmethod != "reshape"
            if self.late:
                if self.cls == "lstm" or rows % self.fpc:
                    raise VltfError("pipeline [%s]: late fusion needs one row per frame" % s.name)
                self.pre_late_rows = rows
                rows //= self.fpc
            self.out_dim, self.fpc_out, self.max_rows = C, 1, rows                        # model.py:153

    @staticmethod
    def _check_aux_rows(a, b):
        ratio = int(a.cpv / b.cpv)
        if ratio < 1 or b.max_rows * ratio * a.fpc != a.max_rows:
            raise VltfError("the vector input has %d rows per batch but the sequence has %d clips at clips-per-video ratio %d" %
                            (b.max_rows, a.max_rows // a.fpc, ratio))

    # ---- variables ---------------------------------------------------------------------------------------------------------------------
    def head_specs(self):
        """[(name, shape)] of everything but the tower, in backward order."""
        sc, C, specs = self.scope, self.g.num_classes, []
        if self.cls == "fc" and self.cls_fc:
            specs += [(sc + "fc_convert_w", (self.feat_dim, C)), (sc + "fc_convert_b", (C,))]
        if self.cls == "lstm":
            H, HO = self.H, self.HO
            if self.HW != C:
                specs += [(sc + self.head_name + "_w", (self.HW, C)), (sc + self.head_name + "_b", (C,))]
            if self.attn_dim:
                specs += attn_specs(HO, self.attn_dim, sc)
            if self.vlad_k:
                specs += vlad_specs(HO, self.vlad_k, sc)
            dims = [self.feat_dim] + [HO] * (self.L - 1)
            if self.sa_ffn:
                specs += encoder_specs(self.L, self.feat_dim, H, self.sa_ffn, self.sa[0], self.fpc, sc, self.sa[1], backward=True)
            if self.tc:
                specs += tcn_specs(self.L, self.feat_dim, H, self.tc[0], sc, backward=True)
            for l in reversed(range(0 if self.sa_ffn or self.tc else self.L)):
                if self.bi:
                    specs += [(n, (dims[l] + H, 4 * H) if n.endswith("kernel") else (4 * H,)) for n in blstm_names(l, sc)]
                    continue
                if self.is_gru:
                    specs += gru_specs(l, dims[l], H, sc)
                    continue
                if self.sa:
                    specs += mhsa_specs(l, dims[l], H, self.sa[0], self.fpc, sc, self.sa[1])
                    continue
                pre = sc + "rnn/multi_rnn_cell/cell_%d/basic_lstm_cell/" % l
                specs += [(pre + "kernel", (dims[l] + H, 4 * H)), (pre + "bias", (4 * H,))]
            if self.state_src is not None and self.state_src.dim != H:
                specs += [(sc + "input_state_fc_w", (self.state_src.dim, H)), (sc + "input_state_fc_b", (H,))]
        if self.rep_fc:
            specs += [(sc + "fc_convert_w", (self.x_dim, self.feat_dim)), (sc + "fc_convert_b", (self.feat_dim,))]
        return specs

    def tower_specs(self):
        return [(self.scope + n, s) for n, s in param_specs(self.tower_cfg)] if self.spec.representation == "dcnn" else []

    # ---- buffers ---------------------------------------------------------------------------------------------------------------------------
    def allocate(self, flat_w, flat_g, off):
        """Views of the flat parameter / gradient buffers and every activation buffer; returns the offset behind this pipeline."""
        g, dev, tr = self.g, self.g.dev, self.g.training

        def buf(*shape, dtype=torch.float32):
            return torch.empty(shape, dtype=dtype, device=dev)
        self.P, self.G = {}, {}
        self.head_off = off
        for name, shp in self.head_specs():
            n = int(np.prod(shp))
            self.P[name] = flat_w[off:off + n].view(shp)
            if tr:
                self.G[name] = flat_g[off:off + n].view(shp)
            off += n
        self.head_cnt = off - self.head_off
        if self.spec.representation == "dcnn":
            n1 = sum(int(np.prod(s)) for _, s in param_specs(self.tower_cfg))
            self.tower = LRCNEngine(self.tower_cfg, self.max_rows0 // self.fpc, str(dev), tr, dp=None,
                                    flat=(flat_w[off:off + n1], flat_g[off:off + n1] if tr else None))
            self.tower_off = off
            for n, _ in param_specs(self.tower_cfg):
                self.P[self.scope + n] = self.tower.P[n]
                if tr:
                    self.G[self.scope + n] = self.tower.G[n]
            if self.fusion:               # avg | maximum of several frame datasets: the other inputs' prepared frames (x0's layout)
                self.x0_others = [torch.zeros_like(self.tower.x0) for _ in self.srcs[1:]]
            off += n1
        R0, D0 = self.max_rows0, self.x_dim
        # is a gradient w.r.t. the stage-0 tensor wanted?  (a pipeline input other than the LSTM's state vector)
        self.primary_pipe = self.tower is None and any(x.kind == "pipe" for x in self.srcs if x is not self.state_src)
        # ... w.r.t. the classifier's input?  (not for a fully frozen tower: nobody would read it)
        self.wants_feat = (self.tower is not None and self.tower_trains) or self.rep_fc or self.primary_pipe
        if self.tower is None and self.fusion:
            self.xf = buf(R0, D0)
        if self.rep_fc:
            self.xrep = buf(R0, self.feat_dim)
            if tr and self.primary_pipe:
                self.dx0 = buf(R0, D0)
        if self.early:
            self.xearly = buf(R0 // self.fpc, self.feat_dim)
            if tr:
                self.dfeat_full = buf(R0, self.feat_dim)
        rows_cls = R0 // self.fpc if self.early else R0
        C = g.num_classes
        sw = 64 * max(1024, C, self.feat_dim, D0)
        if self.cls == "fc":
            self.cls_out = buf(rows_cls, C) if self.cls_fc else None
            if tr and self.cls_fc:
                self.dcls_in = buf(rows_cls, self.feat_dim)
        elif self.cls == "lstm":
            H, T, HO = self.H, self.fpc, self.HO
            B = R0 // T
            self.lstm, self.blstm, self.gru, self.mhsa = [], [], [], []  # per-layer buffers: unidirectional, bidirectional, GRU or self-attention layers
            if self.bi and ops.lstm_seq_bi_tag_span(1, 1, H) == 0:
                raise VltfError("pipeline [%s]: lstm_bidirectional: this device has too few compute units to hold both directions of "
                                "hidden size %d in one launch" % (self.spec.name, H))
            for l in range(self.L):
                if self.bi:
                    self.blstm.append(blstm_buffers(buf, R0, H, tr))
                    continue
                if self.is_gru:
                    self.gru.append(gru_buffers(buf, R0, H, tr))
                    continue
                if self.sa_ffn or self.tc:
                    continue
                if self.sa:
                    self.mhsa.append(mhsa_buffers(buf, R0, T, H, self.sa[0], self.sa[1], tr))
                    continue
                S = dict(gx=buf(R0, 4 * H), act=buf(R0, 4 * H), cseq=buf(R0, H), hseq=buf(R0, H), hprev=buf(R0, H))
                if tr:
                    S.update(dz=buf(R0, 4 * H), dout=buf(R0, H), dh0=buf(B, H), dc0=buf(B, H))
                self.lstm.append(S)
            self.lstm_ws = ops.lstm_seq_ws(B, T, H, dev) if H <= 1024 else None
            if self.lstm_ws is None:
                raise VltfError("GraphEngine: LSTM hidden size above 1024 is not built")
            self.seq_len_buf = torch.zeros(B, dtype=torch.int32, device=dev)     # per-clip lengths of a call that gives them
            r = R0 if self.per_step else B
            HW = self.HW
            self.fused = buf(r, HW) if not self.per_step else None
            self.dropped = buf(r, HW)
            self.drop_mask = buf(r, HW, dtype=torch.uint8)
            self.cls_out = buf(r, C) if HW != C else None
            self.attn = attn_buffers(buf, B, T, HO, self.attn_dim, tr) if self.attn_dim else None
            self.vlad = vlad_buffers(buf, B, T, HO, self.vlad_k, tr) if self.vlad_k else None
            if self.state_src is not None:
                sd = self.state_src.dim
                self.rep_state = buf(B, sd) if self.state_ratio > 1 else None
                self.state = buf(B, H) if sd != H else None
                if tr:
                    self.dstate = buf(B, H)
                    self.drep_state = buf(B, sd) if (sd != H and self.state_src.kind == "pipe") else None
            if tr:
                self.dpre, self.dfused = buf(r, HW), buf(r, HW)
                self.dxseq = buf(R0, self.feat_dim)
                if self.bi:
                    self.dx_bw = buf(R0, max(self.feat_dim, HO))      # the backward direction's share of a layer's input gradient
                    self.dlast = buf(B, HO)                           # fusion last / state: the fused gradient with its backward half zeroed
            sw = max(sw, 64 * 4 * H, 64 * H, 64 * (self.attn_dim or 0), 64 * (self.vlad_k or 0) * HO)
            if self.sa:
                # under seq_len the first layer reads its input through ops.live_rows: a padded frame's features reach no product
                self.xlive = buf(R0, self.feat_dim)
                sw = max(sw, 64 * self.sa[0] * (2 * T - 1))
            self.tcn, self.tconv = None, []
            if self.tc:
                # rnn_cell tcn: engine.tcn_buffers and its layers; the embedding's input goes through ops.live_rows under seq_len
                self.tcn = tcn_buffers(buf, R0, H, self.tc[0], self.L, tr)
                self.tconv = self.tcn["layers"]
                self.xlive = buf(R0, self.feat_dim)
            self.enc = None
            if self.sa_ffn:
                # sa_block encoder: engine.encoder_buffers; self.mhsa is its layers (the top layer's hseq / dout are the final norm's)
                self.enc = encoder_buffers(buf, R0, T, H, self.sa_ffn, self.sa[0], self.sa[1], self.L, tr, self.sa_drop if tr else None)
                self.mhsa = self.enc["layers"]
                sw = max(sw, 64 * self.sa_ffn)
        if self.late:
            self.late_out = buf(self.max_rows, C)
            if tr:
                self.dlate = buf(self.pre_late_rows, C)
        if tr and self.fusion in ("concat", "ibias") and self.tower is None:
            a, b = self.srcs
            self.daux = buf(b.max_rows * max(1, getattr(self, "ratio", 1)), b.dim)       # gradient of the replicated vector input
            self.dtmp = buf(b.max_rows * max(1, getattr(self, "ratio", 1)), b.dim)
            sw = max(sw, 64 * b.max_rows * b.dim)
        if self.fusion in ("concat", "ibias") and self.tower is None and getattr(self, "ratio", 1) > 1:
            self.rep_aux = buf(self.srcs[1].max_rows * self.ratio, self.srcs[1].dim)
        if self.state_src is not None:
            sw = max(sw, 64 * self.state_src.max_rows * self.state_src.dim)
        self.small_ws = buf(sw)
        if tr:
            self.dout = buf(self.max_rows, self.out_dim)       # d(loss) / d(output): the loss (last pipeline) or the consumers write it
            self.din = [buf(x.max_rows, x.dim) if x.kind == "pipe" else None for x in self.srcs]
        return off

    # ---- per-clip lengths ------------------------------------------------------------------------------------------------------------------
    seq_len = None          # device int32 [clips] for the current call, or None (every clip runs all fpc steps)

    def planned_rows(self, feeds):
        """Rows this pipeline will output for `feeds`, from the feeds' shapes alone (no launch): lets the engine check a length
        count before the first kernel."""
        x = self.srcs[0]
        if x.kind == "pipe":
            rows = x.ref.planned_rows(feeds)
        else:
            f = feeds[x.ref]
            rows = int((f["frames_u8"] if x.kind == "video" else f).shape[0])
        if self.fusion == "ibias" and self.tower is None:
            rows = rows // x.fpc * (x.fpc + 1)
        self._planned_rows0 = rows
        if self.early:
            rows //= self.fpc
        if self.cls == "lstm" and not self.per_step:
            rows //= self.fpc
        if self.late:
            rows //= self.fpc
        return rows

    def check_seq_len(self, lengths, feeds):
        """Host validation of one pipeline's lengths -> int32 numpy [clips].  Raises VltfError; launches nothing."""
        name = self.spec.name
        if self.cls != "lstm":
            raise VltfError("seq_len: pipeline [%s] has no LSTM classifier to give sequence lengths to" % name)
        if self.H > 1024:
            raise VltfError("seq_len: pipeline [%s] has hidden size %d; the one-launch recurrence that takes lengths holds <= 1024" %
                            (name, self.H))
        if self.fusion in ("concat", "ibias"):
            raise VltfError("seq_len: pipeline [%s] fuses its inputs by %s, which changes what a time step is; lengths are built for "
                            "pipelines without it (refused rather than guessed)" % (name, self.fusion))
        if self.state_src is not None and self.state_ratio > 1:
            raise VltfError("seq_len: pipeline [%s] replicates its state input at clips-per-video ratio %d; lengths are not built "
                            "for that (refused rather than guessed)" % (name, self.state_ratio))
        if torch.is_tensor(lengths):
            if lengths.device.type != "cpu":
                raise VltfError("seq_len: the lengths of pipeline [%s] must be host data (numpy / list / CPU tensor)" % name)
            lengths = lengths.numpy()
        a = np.asarray(lengths)
        if a.ndim != 1 or a.size == 0 or not np.issubdtype(a.dtype, np.integer):
            raise VltfError("seq_len: the lengths of pipeline [%s] must be a 1-d integer array" % name)
        self.planned_rows(feeds)
        clips = self._planned_rows0 // self.fpc
        if a.size != clips:
            raise VltfError("seq_len: pipeline [%s] has %d clips in this batch, %d lengths were given" % (name, clips, a.size))
        if a.min() < 1 or a.max() > self.fpc:
            raise VltfError("seq_len: the lengths of pipeline [%s] must lie in 1..%d (its steps per clip), got %d..%d" %
                            (name, self.fpc, a.min(), a.max()))
        return np.ascontiguousarray(a, np.int32)

    def _len_kw(self):
        """The keyword for the length-aware ops: passed only when this call was given lengths."""
        return {} if self.seq_len is None else {"seq_len": self.seq_len}

    # ---- forward ---------------------------------------------------------------------------------------------------------------------------
    def _src_tensor(self, x, feeds):
        if x.kind == "pipe":
            x.rows, x.tensor = x.ref.rows, x.ref.out
        else:
            t = feeds[x.ref]
            if x.kind == "vectors":
                if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != x.dim or t.shape[0] > x.max_rows or not t.is_contiguous():
                    raise VltfError("dataset [%s]: vectors must be contiguous float32 [rows <= %d, %d], got %s %s" %
                                    (x.ref, x.max_rows, x.dim, t.dtype, tuple(t.shape)))
                x.rows, x.tensor = t.shape[0], t
        return x

    def forward(self, feeds, train):
        g, s, P, sc, C = self.g, self.spec, self.P, self.scope, self.g.num_classes
        srcs = self.srcs
        # ---- stage 0 / 1 (dcnn): frames -> tower features
        if self.tower is not None:
            tw = self.tower
            seq = srcs if self.fusion else srcs[:1]
            if len(seq) > 1 and tw.c8:
                raise VltfError("input_fusion of frame datasets is built for the fp32 conv path only")
            n = b = None
            for i, x in enumerate(seq):        # each dataset's frames through input prep into x0; all but the last are set aside
                f = feeds[x.ref]
                ni, bi = tw.feed_u8(f["frames_u8"], f.get("mean_bgr"), f.get("crop_y"), f.get("crop_x"), f.get("mirror"), f.get("resize"),
                                     **({"crop_box": f["crop_box"]} if f.get("crop_box") is not None else {}))
                if n is not None and ni != n:
                    raise VltfError("pipeline [%s]: fused frame datasets gave %d and %d frames" % (s.name, n, ni))
                n, b = ni, bi
                if i + 1 < len(seq):
                    self.x0_others[i][:n].copy_(tw.x0[:n])
            if len(seq) > 1:                   # mean / maximum over the list (the zero halo stays zero under both)
                ops.fuse_n([t[:n] for t in self.x0_others] + [tw.x0[:n]], tw.x0[:n], self.fusion, count=tw.x0[:n].numel())
            tw.step_count = g._draw_index()        # (the tower's dropout seed; its own accumulate is 1)
            tw._forward(n, b, train)
            self._nb = (n, b)
            x, rows = tw.logits, n
            for xs in srcs[1:]:
                self._src_tensor(xs, feeds)
        else:
            for xs in srcs:
                self._src_tensor(xs, feeds)
            a = srcs[0]
            if self.fusion in ("avg", "maximum"):
                rows = a.rows
                if any(xs.rows != rows for xs in srcs):
                    raise VltfError("pipeline [%s]: fused inputs have %s rows" % (s.name, [xs.rows for xs in srcs]))
                ops.fuse_n([xs.tensor for xs in srcs], self.xf, self.fusion, count=rows * self.x_dim)
                x = self.xf
            elif self.fusion == "concat" and self.ratio == 1:
                b_ = srcs[1]
                rows = a.rows
                if b_.rows != rows:
                    raise VltfError("pipeline [%s]: concat of %d and %d rows" % (s.name, a.rows, b_.rows))
                ops.copy2d(a.tensor, self.xf, rows, a.dim, src_ld=a.dim, dst_ld=self.x_dim)
                ops.copy2d(b_.tensor, self.xf[:, a.dim:], rows, b_.dim, src_ld=b_.dim, dst_ld=self.x_dim)
                x = self.xf
            elif self.fusion in ("concat", "ibias"):
                b_ = srcs[1]
                T = a.fpc
                clips = a.rows // T
                aux = self._replicate(b_, self.ratio, clips, getattr(self, "rep_aux", None))
                if self.fusion == "concat":        # every clip's vector in front of each of its T sequence rows (vecfirst)
                    for t in range(T):
                        ops.copy2d(aux, self.xf[t:], clips, b_.dim, src_ld=b_.dim, dst_ld=T * self.x_dim)
                    ops.copy2d(a.tensor, self.xf[:, b_.dim:], a.rows, a.dim, src_ld=a.dim, dst_ld=self.x_dim)
                    rows = a.rows
                else:                              # the vector is time step 0 of every clip
                    Ts = T + 1
                    ops.copy2d(aux, self.xf, clips, a.dim, src_ld=a.dim, dst_ld=Ts * a.dim)
                    ops.copy2d(a.tensor, self.xf[1:], clips, T * a.dim, src_ld=T * a.dim, dst_ld=Ts * a.dim)
                    rows = clips * Ts
                x = self.xf
            else:
                x, rows = a.tensor, a.rows
        if rows % self.fpc:
            raise VltfError("pipeline [%s]: %d rows are not whole clips of %d" % (s.name, rows, self.fpc))
        self._x0, self._rows0 = x, rows
        # ---- stage 1: representation fc
        if self.rep_fc:
            ops.gemm(x, P[sc + "fc_convert_w"], self.xrep, rows, self.feat_dim, self.x_dim, bias=P[sc + "fc_convert_b"])
            x = self.xrep
        # ---- stage 2: early fusion
        if self.early:
            ops.temporal_fusion_fwd(x, self.xearly, rows // self.fpc, self.fpc, self.feat_dim, self.fmethod)
            x, rows = self.xearly, rows // self.fpc
        self._xcls, self._rows_cls = x, rows
        # ---- stage 3: classifier
        if self.cls == "fc":
            if self.cls_fc:
                ops.gemm(x, P[sc + "fc_convert_w"], self.cls_out, rows, C, self.feat_dim, bias=P[sc + "fc_convert_b"])
                x = self.cls_out
        elif self.cls == "lstm":
            x, rows = self._lstm_forward(x, rows, train)
        # ---- stage 4: late fusion
        if self.late:
            ops.temporal_fusion_fwd(x, self.late_out, rows // self.fpc, self.fpc, C, self.fmethod)
            self._pre_late_rows = rows
            x, rows = self.late_out, rows // self.fpc
        self.out, self.rows = x, rows
        return x

    def _replicate(self, src, ratio, want_rows, scratch):
        """replicate_auxilliary_tensor (tf_util.py:182-192): the WHOLE batch of vectors repeated `ratio` times in sequence."""
        if src.rows * ratio != want_rows:
            raise VltfError("pipeline [%s]: %d vectors x clips-per-video ratio %d do not pair up with %d clips" %
                            (self.spec.name, src.rows, ratio, want_rows))
        if ratio <= 1:
            return src.tensor
        ops.copy2d(src.tensor, scratch, ratio, src.rows * src.dim, src_ld=0, dst_ld=src.rows * src.dim)
        return scratch

    def _lstm_forward(self, x, rows, train):
        g, P, sc, C, H, T = self.g, self.P, self.scope, self.g.num_classes, self.H, self.fpc
        b = rows // T
        lk = self._len_kw()
        if lk and lk["seq_len"].numel() != b:
            raise VltfError("pipeline [%s]: %d lengths for %d clips" % (self.spec.name, lk["seq_len"].numel(), b))
        s0 = None
        if self.state_src is not None:                  # model.py:128-134, lstm.py:34-42,74-77
            st = self._replicate(self.state_src, self.state_ratio, b, self.rep_state)
            self._state_in = st
            s0 = st
            if self.state is not None:
                ops.gemm(st, P[sc + "input_state_fc_w"], self.state, b, H, self.state_src.dim, bias=P[sc + "input_state_fc_b"])
                s0 = self.state
        self._s0, self._b = s0, b
        xin, d = x, self.feat_dim
        HO, last = self.HO, "last" if self.lfusion == "state" else self.lfusion
        rk = lambda span: dict(ws=self.lstm_ws, **lk)
        if self.blstm:
            xin, d = blstm_forward(self.blstm, P, sc, xin, rows, b, T, d, H, g.ws, rk), HO
        if self.gru:
            xin, d = gru_forward(self.gru, P, sc, xin, rows, b, T, d, H, g.ws, rk), H
        # the dropouts of the self-attention model in a training forward: the counters are those of the global batch (clip0)
        self._sa_drop = None
        if train and self.sa and self.sa_drop is not None:
            rank = g.dp.rank if g.dp is not None else 0
            self._sa_drop = self.sa_drop.bind(rank * (self.max_rows0 // T), seed=dropout_seed(g._draw_index()))
        if self.mhsa or self.tcn:
            # Under seq_len the first product of a self-attention or convolution stack (the qkv projection, the embedding) reads its
            # input through ops.live_rows, because its weight gradient x^T dy reads every row of x: a padded frame's features reach no
            # product.  Above it no launch reads a dead row of what a launch wrote, and what a product leaves in a dead row of its
            # output (a bias) is read by nothing.
            if lk:
                ops.live_rows(xin, self.xlive, b, T, d, lk["seq_len"])
                xin = self.xlive
            self._xsa = xin
        if self.enc:
            xin, d = encoder_forward(self.enc, P, sc, xin, rows, b, T, d, H, self.sa_ffn, self.sa[0], self.sa[1], g.ws, lk,
                                     self._sa_drop), H
        elif self.mhsa:
            xin, d = mhsa_forward(self.mhsa, P, sc, xin, rows, b, T, d, H, self.sa[0], self.sa[1], g.ws, lk, self._sa_drop), H
        if self.tcn:
            xin, d = tcn_forward(self.tcn, P, sc, xin, rows, b, T, d, H, self.tc, g.ws, lk), H
        for l, S in enumerate(self.lstm):
            pre = sc + "rnn/multi_rnn_cell/cell_%d/basic_lstm_cell/" % l
            K = P[pre + "kernel"]
            ops.gemm(xin, K, S["gx"], rows, 4 * H, d, bias=P[pre + "bias"], ws=g.ws)
            ops.lstm_seq_fwd(S["gx"], K[d:], S["act"], S["cseq"], S["hseq"], S["hprev"], b, T, H, FORGET_BIAS, ws=self.lstm_ws, h0=s0, c0=s0,
                             **lk)
            xin, d = S["hseq"], H
        r = rows if self.per_step else b
        if self.per_step:
            v = xin                                                     # reshape fusion: every step's output (tf_util.py:26-27)
        elif self.attn is not None:
            attn_forward(self.attn, P, sc, xin, self.fused, rows, b, T, HO, self.attn_dim, lk)
            v = self.fused
        elif self.vlad is not None:
            vlad_forward(self.vlad, P, sc, xin, self.fused, rows, b, T, HO, self.vlad_k, lk)
            v = self.fused
        else:
            # with lengths `state` and `last` are h of step len - 1 (dynamic_rnn's final state), `avg` the mean over the live steps
            ops.temporal_fusion_fwd(xin, self.fused, b, T, HO, last, **lk)
            if self.bi and last == "last":
                # each direction's FINAL output: the forward half at step len - 1 (just fused), the backward half at step 0
                ops.copy2d(xin[:, H:], self.fused[:, H:], b, H, src_ld=T * HO, dst_ld=HO)
            v = self.fused
        self._dropout = train and g.dropout_keep_prob > 0 and self.lfusion != "state"       # lstm.py:80-93
        if self._dropout:
            ops.dropout_fwd(v[:r], self.dropped[:r], self.drop_mask[:r], g.dropout_keep_prob,
                            (g._draw_index() << 20) ^ (0x2545F4914F6CDD1D + 0x9E3779B9 * self.index))
            v = self.dropped
        self._v = v
        if self.HW != C:
            ops.gemm(v, P[sc + self.head_name + "_w"], self.cls_out, r, C, self.HW, bias=P[sc + self.head_name + "_b"])
            v = self.cls_out
        return v, r

    # ---- backward --------------------------------------------------------------------------------------------------------------------------
    def backward(self):
        """Consumes self.dout[:rows]; writes the gradients of this pipeline's variables and adds its input gradients into the producers'
        dout."""
        g, P, G, sc, C, sw = self.g, self.P, self.G, self.scope, self.g.num_classes, self.small_ws
        d, rows = self.dout, self.rows
        if self.late:
            ops.temporal_fusion_bwd(d, self.dlate, rows, self.fpc, C, self.fmethod)
            d, rows = self.dlate, self._pre_late_rows
        if self.cls == "fc":
            if self.cls_fc:
                ops.gemm(self._xcls, d, G[sc + "fc_convert_w"], self.feat_dim, C, rows, transa=True)
                ops.colsum(d, G[sc + "fc_convert_b"], sw, rows, C)
                if self.wants_feat:
                    ops.gemm(d, P[sc + "fc_convert_w"], self.dcls_in, rows, self.feat_dim, C, transb=True)
                d = self.dcls_in
        elif self.cls == "lstm":
            d, rows = self._lstm_backward(d)
        if self.wants_feat:
            if self.early:
                ops.temporal_fusion_bwd(d, self.dfeat_full, rows, self.fpc, self.feat_dim, self.fmethod)
                d, rows = self.dfeat_full, rows * self.fpc
            if self.rep_fc:
                ops.gemm(self._x0, d, G[sc + "fc_convert_w"], self.x_dim, self.feat_dim, rows, transa=True)
                ops.colsum(d, G[sc + "fc_convert_b"], sw, rows, self.feat_dim)
                if self.primary_pipe:
                    ops.gemm(d, P[sc + "fc_convert_w"], self.dx0, rows, self.x_dim, self.feat_dim, transb=True)
                    d = self.dx0
        # Every gradient of the head chunk is queued now -- the classifier's, its LSTM launches, AND the `representation: fc` variables
        # (fc_convert_w / _b belong to the same chunk, head_specs): only here may the chunk's all-reduce be issued.  Round 3 called this
        # before the representation-fc block: under data parallelism the exchange then read those two gradients before they were written.
        g._head_done(self)
        if self.wants_feat:
            if self.tower is not None:
                n, b = self._nb
                tw = self.tower
                tw.dlogits[:n].copy_(d[:n])       # d(features); the tower applies the encode layer's ReluGrad itself
                tw.dp = g._tower_dp(self)
                tw._backward(n, b)
                tw.dp = None
            elif self.primary_pipe:
                self._input_grads(d, rows)
        if self.state_src is not None and self.state_src.kind == "pipe":
            self._route(1, self._dstate_out)

    def _lstm_backward(self, d):
        g, P, G, sc, C, H, T, sw = self.g, self.P, self.G, self.scope, self.g.num_classes, self.H, self.fpc, self.small_ws
        b = self._b
        rows = b * T
        r = rows if self.per_step else b
        HO, last = self.HO, "last" if self.lfusion == "state" else self.lfusion
        if self.HW != C:
            ops.gemm(self._v, d, G[sc + self.head_name + "_w"], self.HW, C, r, transa=True)
            ops.colsum(d, G[sc + self.head_name + "_b"], sw, r, C)
            ops.gemm(d, P[sc + self.head_name + "_w"], self.dpre, r, self.HW, C, transb=True)
            d = self.dpre
        if self._dropout:
            ops.dropout_bwd(d[:r], self.drop_mask[:r], self.dfused[:r], g.dropout_keep_prob)
            d = self.dfused
        lk = self._len_kw()
        rk = lambda span: dict(ws=self.lstm_ws, **lk)
        param_grads = lambda launch: launch(g.ws, sw)
        top = (self.blstm or self.gru or self.mhsa or self.tconv or self.lstm)[-1]
        if self.per_step:
            top["dout"][:r].copy_(d[:r])
        elif self.bi and last == "last":
            # the forward half's gradient lands on step len - 1 (the fusion's own backward, on a copy whose backward half is zero), the
            # backward half's on step 0
            ops.fill(self.dlast[:b], 0.0)
            ops.copy2d(d, self.dlast, b, H, src_ld=HO, dst_ld=HO)
            ops.temporal_fusion_bwd(self.dlast, top["dout"], b, T, HO, last, **self._len_kw())
            ops.copy2d(d[:, H:], top["dout"][:, H:], b, H, src_ld=HO, dst_ld=T * HO)
        elif self.attn is not None:
            attn_backward(self.attn, P, G, sc, d, top["hseq"], top["dout"], rows, b, T, HO, self.attn_dim, lk, param_grads)
        elif self.vlad is not None:
            vlad_backward(self.vlad, P, G, sc, d, top["hseq"], self.fused, top["dout"], rows, b, T, HO, self.vlad_k, lk, param_grads)
        else:
            ops.temporal_fusion_bwd(d, top["dout"], b, T, HO, last, **self._len_kw())
        has_state = self._s0 is not None
        # the shared pairs of temporal.py: one stream here, every parameter gradient where the chain stands; each returns its first
        # layer's gradient and _feat_grad forms the input gradient from it where somebody reads it (wants_feat)
        D = self.feat_dim
        if self.blstm:
            blstm_backward(self.blstm, P, G, sc, self._xcls, rows, b, T, D, H, g.ws, rk, param_grads,
                           self.dxseq if self.wants_feat else None, self.dx_bw)
        if self.gru:
            dgx = gru_backward(self.gru, P, G, sc, self._xcls, rows, b, T, D, H, g.ws, rk, param_grads)
            self._feat_grad(dgx, P[gru_names(0, sc)[0]], rows, 3 * H)
        if self.enc:
            dx0 = encoder_backward(self.enc, P, G, sc, self._xsa, rows, b, T, D, H, self.sa_ffn, self.sa[0], self.sa[1], g.ws, lk,
                                   param_grads, self._sa_drop)
            embed_grads(G, encoder_var, sc, self._xsa, dx0, rows, D, H, param_grads)
            self._feat_grad(dx0, P[encoder_var(sc, None, "kernel")], rows, H)
        elif self.mhsa:
            dqkv = mhsa_backward(self.mhsa, P, G, sc, self._xsa, rows, b, T, D, H, self.sa[0], self.sa[1], g.ws, lk, param_grads,
                                 self._sa_drop)
            self._feat_grad(dqkv, P[mhsa_names(0, sc, self.sa[1])[0]], rows, 3 * H)
        if self.tcn:
            dx0 = tcn_backward(self.tcn, P, G, sc, rows, b, T, H, self.tc, lk, param_grads)
            embed_grads(G, tcn_var, sc, self._xsa, dx0, rows, D, H, param_grads)
            self._feat_grad(dx0, P[tcn_var(sc, None, "kernel")], rows, H)
        for l in reversed(range(len(self.lstm))):
            S = self.lstm[l]
            pre = sc + "rnn/multi_rnn_cell/cell_%d/basic_lstm_cell/" % l
            K = P[pre + "kernel"]
            din = self.feat_dim if l == 0 else H
            xin = self._xcls if l == 0 else self.lstm[l - 1]["hseq"]
            ops.lstm_seq_bwd(S["dout"], K[din:], S["act"], S["cseq"], S["dz"], b, T, H, ws=self.lstm_ws, c0=self._s0,
                             dh0=S["dh0"] if has_state else None, dc0=S["dc0"] if has_state else None, **self._len_kw())
            ops.gemm(xin, S["dz"], G[pre + "kernel"], din, 4 * H, rows, transa=True, ws=g.ws)
            ops.gemm(S["hprev"], S["dz"], G[pre + "kernel"][din:], H, 4 * H, rows, transa=True, ws=g.ws)
            ops.colsum(S["dz"], G[pre + "bias"], sw, rows, 4 * H)
            if has_state:                                               # c = h = state in EVERY layer: the gradients add up
                ops.eltwise2(S["dh0"], S["dc0"], S["dh0"], "add", count=b * H)
                if l == self.L - 1:
                    self.dstate[:b].copy_(S["dh0"][:b])
                else:
                    ops.eltwise2(self.dstate, S["dh0"], self.dstate, "add", count=b * H)
            if l > 0:
                ops.gemm(S["dz"], K, self.lstm[l - 1]["dout"], rows, H, 4 * H, transb=True, ldb=4 * H, ws=g.ws)
            else:
                self._feat_grad(S["dz"], K, rows, 4 * H)
        if has_state:
            ds, sd = self.dstate, self.state_src.dim
            to_pipe = self.state_src.kind == "pipe"
            if self.state is not None:                                  # input_state_fc (lstm.py:74-77)
                ops.gemm(self._state_in, self.dstate, G[sc + "input_state_fc_w"], sd, H, b, transa=True)
                ops.colsum(self.dstate, G[sc + "input_state_fc_b"], sw, b, H)
                if to_pipe:
                    ops.gemm(self.dstate, P[sc + "input_state_fc_w"], self.drep_state, b, sd, H, transb=True)
                    ds = self.drep_state
            if to_pipe:
                if self.state_ratio > 1:                                # the tiles of the replicated batch add up
                    ops.colsum(ds, self.din[1], sw, self.state_ratio, (b // self.state_ratio) * sd)
                    ds = self.din[1]
                self._dstate_out = ds
        return self.dxseq, rows

    def _feat_grad(self, dg, K, rows, W):
        """dxseq = dg K^T, the gradient of the classifier's input from its first layer's dg [rows, W], where somebody reads it."""
        if self.wants_feat:
            ops.gemm(dg, K, self.dxseq, rows, self.feat_dim, W, transb=True, ldb=W, ws=self.g.ws)

    def _input_grads(self, d, rows):
        """Gradient w.r.t. the fused stage-0 tensor -> the pipeline inputs' producers."""
        srcs = self.srcs
        a = srcs[0]
        if self.fusion in ("avg", "maximum"):
            dins = [self.din[i] if x.kind == "pipe" else None for i, x in enumerate(srcs)]
            ops.fuse_n_grad([x.tensor for x in srcs], d, dins, self.fusion, count=rows * self.x_dim)
            for i, x in enumerate(srcs):
                if x.kind == "pipe":
                    self._route(i, dins[i])
        elif self.fusion == "concat" and self.ratio == 1:
            b_ = srcs[1]
            if a.kind == "pipe":
                ops.copy2d(d, self.din[0], rows, a.dim, src_ld=self.x_dim, dst_ld=a.dim)
                self._route(0, self.din[0])
            if b_.kind == "pipe":
                ops.copy2d(d[:, a.dim:], self.din[1], rows, b_.dim, src_ld=self.x_dim, dst_ld=b_.dim)
                self._route(1, self.din[1])
        elif self.fusion in ("concat", "ibias"):
            b_ = srcs[1]
            T = a.fpc
            clips = a.rows // T
            if self.fusion == "concat":
                if b_.kind == "pipe":       # every sequence position of a clip carried a copy of its vector: sum the T column blocks
                    ops.copy2d(d, self.daux, clips, b_.dim, src_ld=T * self.x_dim, dst_ld=b_.dim)
                    for t in range(1, T):
                        ops.copy2d(d[t:], self.dtmp, clips, b_.dim, src_ld=T * self.x_dim, dst_ld=b_.dim)
                        ops.eltwise2(self.daux, self.dtmp, self.daux, "add", count=clips * b_.dim)
                if a.kind == "pipe":
                    ops.copy2d(d[:, b_.dim:], self.din[0], a.rows, a.dim, src_ld=self.x_dim, dst_ld=a.dim)
                    self._route(0, self.din[0])
            else:
                Ts = T + 1
                if b_.kind == "pipe":
                    ops.copy2d(d, self.daux, clips, a.dim, src_ld=Ts * a.dim, dst_ld=a.dim)
                if a.kind == "pipe":
                    ops.copy2d(d[1:], self.din[0], clips, T * a.dim, src_ld=Ts * a.dim, dst_ld=T * a.dim)
                    self._route(0, self.din[0])
            if b_.kind == "pipe":
                da = self.daux
                if self.ratio > 1:
                    ops.colsum(self.daux, self.din[1], self.small_ws, self.ratio, b_.rows * b_.dim)
                    da = self.din[1]
                self._route(1, da)
        elif a.kind == "pipe":
            self._route(0, d)

    def _route(self, i, d):
        """Adds (or, for the producer's only consumer edge, copies) d into the producer's dout."""
        x = self.srcs[i]
        prod = x.ref
        cnt = x.rows * x.dim
        if prod._dout_fresh:
            if d.data_ptr() != prod.dout.data_ptr():
                prod.dout.view(-1)[:cnt].copy_(d.reshape(-1)[:cnt])
            prod._dout_fresh = False
        else:
            ops.eltwise2(prod.dout, d, prod.dout, "add", count=cnt)


def init_params_for(specs, seed=0, stddev=0.05, well_scaled=False):
    """Reference initialisers for a variable list [(name, shape)] (alexnet.py:40-46, tf_util.py:44-45; BasicLSTMCell: glorot-uniform /
    zeros), drawn in list order from one generator."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, shp in specs:
        if name.endswith("conv_kernel") and len(shp) == 3:             # rnn_cell tcn: Keras' Conv1D fans, taps x in and taps x out
            lim = math.sqrt(6.0 / (shp[0] * shp[1] + shp[0] * shp[2]))
            out[name] = rng.uniform(-lim, lim, shp).astype(np.float32)
        elif name.endswith("kernel") or name.endswith("attention_pool/context") or name.endswith("netvlad/centers"):
            lim = math.sqrt(6.0 / (shp[0] + shp[1]))
            out[name] = rng.uniform(-lim, lim, shp).astype(np.float32)
        elif name.endswith("bias") or name.endswith("beta"):
            out[name] = np.zeros(shp, np.float32)
        elif name.endswith("gamma"):                                    # a layer norm's scale (sa_block encoder): ones
            out[name] = np.ones(shp, np.float32)
        elif len(shp) > 1:
            out[name] = _trunc_normal(rng, shp, math.sqrt(2.0 / int(np.prod(shp[:-1]))) if well_scaled else stddev)
        else:
            out[name] = np.full(shp, 0.1, np.float32)
    return out


def model_specs(pipelines, datasets, num_classes):
    """[(name, shape)] of a model's variables in flat-buffer order -- the host-side plan of GraphEngine without a device (fixture
    generators, checkpoint tools)."""
    eng = object.__new__(GraphEngine)
    eng.dev, eng.training, eng.dp = torch.device("cpu"), False, None
    eng._plan(pipelines, datasets, num_classes)
    return list(eng.specs)


class GraphEngine:
    def __init__(self, pipelines: List[PipelineSpec], datasets: dict, num_classes: int, device="cuda:0", training=True, dp=None,
                 optimizer="sgd", dropout_keep_prob=0.0, conv_math="f32", lr_mult=None, momentum=0.0, nesterov=False, weight_decay=0.0,
                 accumulate=1, fc_dropout_keep_prob=0.0, tensor_stats_interval=0, ema_decay=0.0, ema_warmup=False,
                 lars_eeta=0.0, lars_epsilon=0.0, label_smoothing=0.0, top_k=0,
                 lamb=False, lamb_epsilon=None, mixup_alpha=0.0, cutmix_alpha=0.0, class_weights=None, focal_gamma=0.0, erase_prob=0.0,
                 label_type="single"):
        """lr_mult: train.lr_mult, the learning-rate factor of the `modified` variables (engine.is_regular); a pipeline's train_from
        freezes the first layers of its tower (engine.tier_plan).  momentum, nesterov: tf.train.MomentumOptimizer's, optimizer sgd only
        (engine.check_momentum); 0 = plain SGD.  weight_decay: the L2 coefficient of every trained weight tensor of rank >= 2 of every
        pipeline (engine.decay_ranges); 0 = off.  accumulate: the most micro-batches one update may sum, train_step(micro=(i, k))
        (engine.check_accumulate, LRCNEngine.train_step_u8); 1 = off.  fc_dropout_keep_prob: dropout on relu(fc6) / relu(fc7) of every
        dcnn tower in a training forward (engine.check_fc_dropout), each tower under a salt of its own (1 + its node index: two towers
        draw different masks at one step; data-parallel ranks are not salted, as with the heads' dropout); 0 = off.
        tensor_stats_interval: per-variable gradient / weight statistics every N updates (engine.stat_segments over this engine's
        variable list, `<pipeline>/<tf name>` in a scoped model; LRCNEngine._stats_launch); None / 0 = off.  ema_decay, ema_warmup:
        tf.train.ExponentialMovingAverage's shadow of every variable of the model, averaged over the trained ranges after each update
        (engine.check_ema, engine.ema_rate, LRCNEngine._ema_launch); 0 = off.  lars_eeta, lars_epsilon: tf.contrib.opt.LARSOptimizer's
        trust ratio on the learning rate of every trained weight tensor of rank >= 2 of every pipeline (engine.check_lars,
        engine.lars_ranges, LRCNEngine._lars_setup); needs momentum > 0; 0 = off.  label_smoothing, top_k: the smoothed labels of
        tf.losses.softmax_cross_entropy and the top-k hit count, both in the loss launch of the last pipeline (engine.check_label_smoothing,
        engine.check_top_k, LRCNEngine._loss_setup); a forward-only engine ignores them; 0 = off.  lamb, lamb_epsilon: LAMB
        (tfa.optimizers.LAMB) in the place of the Adam update -- Adam's moments, a trust ratio |w| / |u| per trained weight tensor of rank
        >= 2 of every pipeline, weight_decay decoupled (engine.check_lamb, engine.lamb_ranges, LRCNEngine._lamb_setup); optimizer adam
        only; False = off.  mixup_alpha: refused when > 0 -- mixup pairs the clips of ONE dcnn pipeline (LRCNEngine).
        cutmix_alpha: refused when > 0 for the same reason.  class_weights, focal_gamma: num_classes weights inside the
        class sum of the loss and the focal loss's focusing parameter, in the loss launch of the last pipeline with its seq_len
        (engine.check_class_weights, engine.check_focal_gamma, LRCNEngine._loss_setup); a forward-only engine ignores
        them; None / 0 = off.  erase_prob: refused when > 0 -- random erasing draws one table per batch of ONE dcnn pipeline
        (LRCNEngine); per-tower tables are a follow-up.  label_type: "single" | "multiple" (engine.check_label_type):
        with multiple the loss launch of the last pipeline, with its seq_len, is ops.sigmoid_xent on multi-hot rows -- class_weights
        are its positive-term weights, top_k is refused (LRCNEngine._loss_setup)."""
        if check_erase(erase_prob).prob > 0.0:
            raise VltfError("erase_prob = %s is refused by GraphEngine: random erasing keeps one box table for the clips of one dcnn "
                            "pipeline; per-tower tables are a follow-up (use a single-pipeline model: LRCNEngine, NetConfig.erase_prob)"
                            % (erase_prob,))
        if check_cutmix(cutmix_alpha)[0] > 0.0:
            raise VltfError("cutmix_alpha = %s is refused by GraphEngine: frame towers, vector inputs, clips-per-video ratios and word-level "
                            "losses have no one clip to pair; CutMix runs on single-pipeline models (LRCNEngine, NetConfig.cutmix_alpha)"
                            % (cutmix_alpha,))
        if check_mixup(mixup_alpha)[0] > 0.0:
            raise VltfError("mixup_alpha = %s is refused by GraphEngine: frame towers, vector inputs, clips-per-video ratios and word-level "
                            "losses have no one clip to pair; mixup runs on single-pipeline models (LRCNEngine, NetConfig.mixup_alpha)"
                            % (mixup_alpha,))
        self._loss_opts = (check_label_smoothing(label_smoothing), check_top_k(top_k))
        self._loss_wf = (check_class_weights(class_weights, int(num_classes)), check_focal_gamma(focal_gamma))
        self._label_type = check_label_type(label_type)
        self.fc_dropout_keep_prob = check_fc_dropout(fc_dropout_keep_prob)
        self.accumulate = check_accumulate(accumulate)
        self.micro, self._mi = MicroSequence(self.accumulate), None
        self.momentum, self.nesterov = check_momentum(optimizer, momentum, nesterov)
        self.weight_decay = check_weight_decay(weight_decay)
        self.ema_decay, self.ema_warmup = check_ema(ema_decay, ema_warmup)
        self.lars_eeta, self.lars_epsilon = check_lars(optimizer, self.momentum, lars_eeta, lars_epsilon)
        self.lamb_on, self.lamb_epsilon = check_lamb(optimizer, lamb, lamb_epsilon)
        self.dev = torch.device(device)
        self._require_device()
        self.training, self.dp = training, dp
        self._plan(pipelines, datasets, num_classes, optimizer, dropout_keep_prob, conv_math, lr_mult)
        # (under LAMB the decay is decoupled: no regulariser launch, it enters through u alone)
        self.decay = decay_ranges(self.specs, self.plan, self.weight_decay) if self.weight_decay > 0.0 and training and not self.lamb_on else None
        self._allocate()
        self._stats_setup(tensor_stats_interval)
        self._lars_setup()
        self._lamb_setup()

    def _plan(self, pipelines, datasets, num_classes, optimizer="sgd", dropout_keep_prob=0.0, conv_math="f32", lr_mult=None):
        """The graph, its variable list and its training plan (self.nodes, self.specs, self.plan): host logic only, no device
        (model_specs uses it alone)."""
        if not pipelines:
            raise VltfError("no pipeline defined")
        self.num_classes, self.optimizer, self.dropout_keep_prob, self.conv_math = int(num_classes), optimizer, float(dropout_keep_prob or 0.0), conv_math
        self.datasets = datasets
        self.scoped = len(pipelines) > 1
        self.step_count = 0
        names = [p.name for p in pipelines]
        if len(set(names)) != len(names) or any(n in datasets for n in names):
            raise VltfError("pipeline names must be unique and differ from the dataset tags: %s" % names)
        # the last pipeline defines the logits (model.py:161); only what it depends on is ever evaluated
        needed, stack = set(), [pipelines[-1].name]
        by_name = {p.name: p for p in pipelines}
        while stack:
            n = stack.pop()
            if n in needed:
                continue
            needed.add(n)
            stack += [i for i in by_name[n].input if i in by_name]
        self.skipped = [p.name for p in pipelines if p.name not in needed]
        self.nodes, self.by_name = [], {}
        for spec in pipelines:
            if spec.name not in needed:
                continue
            srcs = []
            for src in spec.input:
                if src in self.by_name:
                    nd = self.by_name[src]
                    srcs.append(_Src("pipe", nd, nd.out_dim, nd.cpv_out, nd.fpc_out, nd.max_rows))
                elif src in by_name:
                    raise VltfError("Input identifier [%s] of pipeline [%s] is a pipeline that has not been declared yet." % (src, spec.name))
                elif src in datasets:
                    ds = datasets[src]
                    dim = ds.dim if ds.mode == "vectors" else ds.image_shape[-1]
                    srcs.append(_Src(ds.mode, src, dim, ds.cpv, ds.fpc, ds.max_clips * ds.fpc))
                else:
                    raise VltfError("Could not find a dataset with the tag %s, required by the pipeline %s" % (src, spec.name))
            node = PipeNode(self, spec, srcs, len(self.nodes))
            self.nodes.append(node)
            self.by_name[spec.name] = node
        self.last = self.nodes[-1]
        if self.last.out_dim != self.num_classes:
            raise VltfError("the last pipeline [%s] ends with %d-wide rows, the loss needs num_classes = %d (a classifier is missing)" %
                            (self.last.spec.name, self.last.out_dim, self.num_classes))
        # ---- one flat parameter / gradient buffer, last pipeline first
        order = list(reversed(self.nodes))
        self.specs = []
        for nd in order:
            self.specs += nd.head_specs() + nd.tower_specs()
        dup = {n for n, _ in self.specs if [m for m, _ in self.specs].count(n) > 1}
        if dup:
            raise VltfError("Variable %s already exists" % sorted(dup)[0])
        # ---- learning-rate tiers, frozen variables and the data-parallel chunks in the order backward completes them: per pipeline its
        # head, then its tower's own chunk list
        frozen, chunks, off = [], [], 0
        for nd in order:
            cnt = sum(int(np.prod(shp)) for _, shp in nd.head_specs())
            if cnt:
                chunks.append((off, cnt))
            off += cnt
            if nd.spec.representation == "dcnn":
                tp = finetune_plan(nd.tower_cfg)
                frozen += [nd.scope + n for n in tp.frozen]
                chunks += [(off + lo, c) for lo, c in tp.chunks]
                off += tp.total
        self.lr_mult = lr_mult
        self.plan = tier_plan(self.specs, frozen, lr_mult, chunks)
        if not self.plan.tiers:
            raise VltfError("the train_from settings leave this model nothing to train")
        if len(self.plan.tiers) > MAX_LR_TIERS:
            raise VltfError("this model needs %d learning-rate tiers (ranges of the flat parameter buffer with one factor, frozen ranges "
                            "between them); the update kernels take %d" % (len(self.plan.tiers), MAX_LR_TIERS))

    def _allocate(self):
        order = list(reversed(self.nodes))
        training, optimizer = self.training, self.optimizer
        total = sum(int(np.prod(s)) for _, s in self.specs)
        dev = self.dev
        self.w = torch.zeros(total, device=dev)
        self.g = torch.zeros(total, device=dev) if training else None
        self.ws = torch.empty((64 << 20) // 4, device=dev)            # split-k slabs of the heads' GEMMs
        off = 0
        self.P, self.G = {}, {}
        for nd in order:
            off = nd.allocate(self.w, self.g, off)
            self.P.update(nd.P)
            self.G.update(nd.G)
        assert off == total
        # data-parallel chunks in the order backward completes them: per pipeline its head, then the chunk list its tower issues
        # (= self.plan.chunks, which _plan derives from the configs alone)
        self.grad_chunks = []
        for nd in order:
            if nd.head_cnt:
                self.grad_chunks.append((nd.head_off, nd.head_cnt))
            if nd.tower is not None:
                self.grad_chunks += [(nd.tower_off + lo, cnt) for lo, cnt in nd.tower.grad_chunks]
        if optimizer == "adam" and training:
            self.adam_m, self.adam_v = torch.zeros(total, device=dev), torch.zeros(total, device=dev)
        self.mom = torch.zeros(total, device=dev) if self.momentum > 0.0 and training else None    # the momentum accumulator
        self.gacc = torch.empty(total, device=dev) if self.accumulate > 1 and training else None   # LRCNEngine.__init__: the running sum
        self.ema = torch.zeros(total, device=dev) if self.ema_decay > 0.0 and training else None   # LRCNEngine.__init__: the shadow weights
        rows = self.last.max_rows
        self._loss_setup(*self._loss_opts, rows, *self._loss_wf, num_classes=self.num_classes, label_type=self._label_type)
        self.ss = torch.zeros(1, device=dev)
        self.ss2 = None
        if self.decay is not None:                # L2 weight decay (LRCNEngine.__init__): {sum g'^2, regulariser}, self.ss its first word
            self.ss2 = torch.zeros(2, device=dev)
            self.ss = self.ss2[:1]
        self._skip = torch.zeros(1, dtype=torch.int32, device=dev)      # ops.step_guard: the optimizer launch's skip word
        self.small_ws = torch.empty(64 * 1024, device=dev)
        self._queued, self._pending_lstm = [], 0
        self.per_step = self.last.cls == "lstm" and self.last.per_step

    def _require_device(self):
        if self.dev.type != "cuda" or not torch.cuda.is_available():
            raise VltfError("GraphEngine needs a HIP device; there is no CPU fallback")
        torch.cuda.set_device(self.dev)

    def _sync(self):
        torch.cuda.synchronize(self.dev)

    # ---- parameters --------------------------------------------------------------------------------------------------------------------
    def load_params(self, params: dict):
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

    def init_params(self, seed=0, stddev=0.05, well_scaled=False):
        """Reference initialisers for every variable (alexnet.py:40-46, tf_util.py:44-45; BasicLSTMCell: glorot-uniform / zeros)."""
        return init_params_for(self.specs, seed, stddev, well_scaled)

    def get_params(self):
        self._sync()
        return {n: self.P[n].detach().cpu().numpy().copy() for n, _ in self.specs}

    def get_grads(self):
        self._sync()
        frozen = set(self.plan.frozen)
        return {n: self.G[n].detach().cpu().numpy().copy() for n, _ in self.specs if n not in frozen}

    OPT_PREFIX = LRCNEngine.OPT_PREFIX
    get_opt_state = LRCNEngine.get_opt_state
    load_opt_state = LRCNEngine.load_opt_state

    @property
    def cfg(self):
        """The optimizer-bearing view the checkpoint helpers of LRCNEngine read."""
        return self

    def check_status(self):
        try:
            ops.lstm_seq_check(*[nd.lstm_ws for nd in self.nodes if nd.cls == "lstm"])
        except VltfError:
            self.micro.reset()                # LRCNEngine.check_status: an accumulated update in progress is abandoned
            raise

    _draw_index = LRCNEngine._draw_index
    _acc_tiers = LRCNEngine._acc_tiers
    _ema_follow, _ema_launch, _ema_required, _flat_f32 = (LRCNEngine._ema_follow, LRCNEngine._ema_launch, LRCNEngine._ema_required,
                                                          LRCNEngine._flat_f32)
    get_ema_params, load_ema, use_ema_weights = LRCNEngine.get_ema_params, LRCNEngine.load_ema, LRCNEngine.use_ema_weights
    _stats_setup, _stats_due, _stats_launch, _stats_note = (LRCNEngine._stats_setup, LRCNEngine._stats_due, LRCNEngine._stats_launch,
                                                            LRCNEngine._stats_note)
    _stats_collect, _stats_result, tensor_stats = LRCNEngine._stats_collect, LRCNEngine._stats_result, LRCNEngine.tensor_stats
    _lars_setup, _lars_stats_launch, _lars_trust_launch = LRCNEngine._lars_setup, LRCNEngine._lars_stats_launch, LRCNEngine._lars_trust_launch
    _lars_named, lars_trust = LRCNEngine._lars_named, LRCNEngine.lars_trust
    _lamb_setup, _lamb_launch, _lamb_named, lamb_trust = (LRCNEngine._lamb_setup, LRCNEngine._lamb_launch, LRCNEngine._lamb_named,
                                                          LRCNEngine.lamb_trust)
    _loss_setup, _fetch_topk = LRCNEngine._loss_setup, LRCNEngine._fetch_topk

    def _xent_launch(self, logits, onehot, dlogits, grad_scale, **lengths):
        """LRCNEngine._xent_launch through this module's ops (lengths: seq_len and T of a loss masked by seq_len, or nothing)."""
        if self.multilabel:
            ops.sigmoid_xent(logits, onehot, dlogits, self.stats, grad_scale, self.loss_rows, self.label_smoothing, self.class_weights_dev,
                             self.focal_gamma, **lengths)
        elif self.xent_wf:
            ops.softmax_xent_wf(logits, onehot, dlogits, self.stats, grad_scale, self.loss_rows, self.label_smoothing, self.top_k,
                                self.class_weights_dev, self.focal_gamma, **lengths)
        elif self.xent_ls:
            ops.softmax_xent_ls(logits, onehot, dlogits, self.stats, grad_scale, self.loss_rows, self.label_smoothing, self.top_k, **lengths)
        else:
            ops.softmax_xent(logits, onehot, dlogits, self.stats, grad_scale, self.loss_rows, **lengths)

    def logits_host(self):
        self._sync()
        self.check_status()
        return self.last.out[:self.last.rows].detach().cpu().numpy().copy()

    def pipeline_output_host(self, name):
        self._sync()
        nd = self.by_name[name]
        return nd.out[:nd.rows].detach().cpu().numpy().copy()

    # ---- the two executor calls ------------------------------------------------------------------------------------------------------
    def _forward(self, feeds, train):
        ops.set_conv_math(self.conv_math)
        for nd in self.nodes:
            nd.forward(feeds, train)
        return self.last.rows

    def _set_seq_len(self, seq_len, feeds):
        """Validates the lengths of a call on the host (VltfError before anything is launched), copies them into the pipelines'
        device buffers and returns the live-row count of a masked loss (None: the loss is over all rows).  seq_len None: every
        pipeline runs all its steps, and no op is handed a length."""
        for nd in self.nodes:
            nd.seq_len = None
        if seq_len is None:
            return None
        if self.dp is not None and self.dp.world > 1:
            raise VltfError("seq_len under data parallelism is not built: the masked loss needs the live-row count of all ranks")
        if not isinstance(seq_len, dict):
            raise VltfError("seq_len must be a dict {pipeline name: lengths}")
        checked = {}
        for name, lengths in seq_len.items():
            if name not in self.by_name:
                raise VltfError("seq_len: [%s] is not a pipeline of this model (%s)" % (name, [nd.spec.name for nd in self.nodes]))
            checked[name] = self.by_name[name].check_seq_len(lengths, feeds)
        n_valid = None
        for name, a in checked.items():
            nd = self.by_name[name]
            nd.seq_len = nd.seq_len_buf[:a.size]
            nd.seq_len.copy_(torch.from_numpy(a))
            if nd is self.last and nd.per_step:
                n_valid = int(a.sum())
        return n_valid

    def forward(self, feeds, seq_len=None):
        """sess.run(model.logits, fdict).  feeds: {dataset tag: dict(frames_u8=, mean_bgr=, crop_y=, crop_x=, mirror=, resize=) for a
        frame dataset | float32 device tensor [rows, dim] for a vectors dataset}.  Returns a device view [rows, classes].
        seq_len: {pipeline name: host int32 lengths [clips of that pipeline]} (module docstring); under fusion `reshape` the rows of
        dead steps are still produced (the head applied to a zero vector)."""
        self._set_seq_len(seq_len, feeds)
        rows = self._forward(feeds, train=False)
        return self.last.out[:rows]

    def train_step(self, feeds, onehot, lr, clip_norm=0.0, fetch=True, global_rows=None, seq_len=None, micro=None):
        """sess.run([.., loss, .., optimizer], fdict): labels int32 one-hot [rows, classes] for the LAST pipeline's rows.
        seq_len as in forward; when the last pipeline has lengths and fusion `reshape`, loss and accuracy are means over the
        n_valid = sum(lengths) live rows (labels still hold every row) and the returned `rows` is n_valid.
        micro = (i, k): micro-step i of an update that sums k of them (LRCNEngine.train_step_u8); with a masked loss global_rows is then
        the live rows of the whole update (default n_valid * k)."""
        mi = self.micro.enter(micro)
        try:
            return self._train_step(feeds, onehot, lr, clip_norm, fetch, global_rows, seq_len, mi)
        except VltfError:
            self.micro.reset()
            raise
        finally:
            self._mi = None

    def _train_step(self, feeds, onehot, lr, clip_norm, fetch, global_rows, seq_len, mi):
        if not self.training:
            raise VltfError("engine was built with training=False")
        i, k = mi if mi is not None else (0, 1)
        n_valid = self._set_seq_len(seq_len, feeds)
        if n_valid is not None and global_rows is not None and k == 1:
            raise VltfError("global_rows is the data-parallel row count; a loss masked by seq_len takes its own live-row count")
        self._mi = mi
        rows = self._forward(feeds, train=True)
        if onehot.dtype != torch.int32 or tuple(onehot.shape) != (rows, self.num_classes):
            raise VltfError("labels must be int32 one-hot of shape (%d, %d)" % (rows, self.num_classes))
        world = self.dp.world if self.dp is not None else 1
        if i == 0:                                # loss_sum / correct sum on the device over the micro-steps of an update
            ops.fill(self.stats, 0.0)
        last = self.last
        if n_valid is not None:       # padded steps are kept out of the loss (non_padding_index, dataset_.py:327-383)
            self._xent_launch(last.out[:rows], onehot, last.dout, 1.0 / (global_rows or n_valid * k), seq_len=last.seq_len, T=last.fpc)
        else:
            self._xent_launch(last.out[:rows], onehot, last.dout, 1.0 / (global_rows or rows * world * k))
        # backward, last pipeline first.  RCCL chunks are held back while an LSTM backward launch is still to come: the cluster
        # form of the recurrence needs every CU and must not spin under an all-reduce kernel that holds some (vl_lstm_seq_status)
        self._pending_lstm = sum(1 for nd in self.nodes if nd.cls == "lstm")
        self._queued = []
        for nd in self.nodes:
            nd._dout_fresh = True
        for nd in reversed(self.nodes):
            nd.backward()
        self._flush()
        total_rows = self.micro.add_rows(mi, rows if n_valid is None else n_valid)
        if i < k - 1:                             # LRCNEngine._train: g joins the running sum, nothing else happens
            ops.grad_accumulate(self.gacc, self.g, ops.ACC_STORE if i == 0 else ops.ACC_ADD, self._acc_tiers())
            return self._fetch(total_rows, fetch, partial=True)
        if k > 1 and self.dp is None:             # (data parallel: _exchange added each chunk before it went out)
            ops.grad_accumulate(self.gacc, self.g, ops.ACC_FINAL, self._acc_tiers())
        return self._finish_step(total_rows, lr, clip_norm, fetch)

    def _exchange(self, off, cnt):
        """One chunk of the flat gradient goes out.  A non-final micro-step exchanges nothing; the final one of k > 1 first adds the
        running sum over the chunk, on the current stream (LRCNEngine._issue)."""
        mi = self._mi
        if mi is not None and mi[0] < mi[1] - 1:
            return
        if mi is not None and mi[1] > 1:
            ops.grad_accumulate(self.gacc, self.g, ops.ACC_FINAL, [(off, off + cnt, 1.0)])
        self.dp.reduce_async(self.g, off, cnt)

    def _reduce(self, off, cnt):
        if self.dp is None or cnt == 0:
            return
        if self._pending_lstm > 0:
            self._queued.append((off, cnt))
        else:
            self._exchange(off, cnt)

    def _flush(self):
        for off, cnt in self._queued:
            self._exchange(off, cnt)
        self._queued = []

    def _head_done(self, nd):
        """The head of a pipeline has queued all its backward launches (its LSTM's included): its chunk may go."""
        if nd.cls == "lstm":
            self._pending_lstm -= 1
        if self.dp is None:
            return
        if nd.head_cnt:
            self._queued.append((nd.head_off, nd.head_cnt))
        if self._pending_lstm == 0:
            self._flush()

    def _tower_dp(self, nd):
        return _TowerReduce(self, nd.tower_off) if self.dp is not None else None

    def train_step_empty(self, lr, clip_norm=0.0, fetch=True, micro=None):
        """This rank's shard of the global batch is empty: contribute zeros to the exchange, apply the same update as the others
        (as a micro-step: add nothing to the update's sum, LRCNEngine.train_step_empty)."""
        if self.dp is None:
            raise VltfError("train_step_empty is a data-parallel call")
        mi = self.micro.enter(micro)
        i, k = mi if mi is not None else (0, 1)
        if i == 0:
            ops.fill(self.stats, 0.0)
        total_rows = self.micro.add_rows(mi, 0)
        if i < k - 1:
            if i == 0:
                for lo, hi, _ in self.plan.tiers:
                    ops.fill(self.gacc[lo:hi], 0.0)
            return self._fetch(total_rows, fetch, partial=True)
        for lo, hi, _ in self.plan.tiers:
            ops.fill(self.g[lo:hi], 0.0)
        for lo, cnt in self.grad_chunks:
            if k > 1:
                ops.grad_accumulate(self.gacc, self.g, ops.ACC_FINAL, [(lo, lo + cnt, 1.0)])
            self.dp.reduce_async(self.g, lo, cnt)
        return self._finish_step(total_rows, lr, clip_norm, fetch)

    def _finish_step(self, rows, lr, clip_norm, fetch):
        if self.dp is not None:
            self.dp.wait()
        tiers = None if self.plan.full_range() else self.plan.tiers      # LRCNEngine._finish_step
        self._lars_stats_launch()
        if self.decay is not None:
            ops.l2_regularize(self.w, self.g, self.decay, self.ss2, self.small_ws)
        elif tiers is None:
            ops.sumsq(self.g, self.ss, self.small_ws)
        else:
            ops.sumsq_tiers(self.g, tiers, self.ss, self.small_ws)
        stats_step = self._stats_due()
        if stats_step:
            self._stats_launch(lr, clip_norm)
        self.step_count += 1
        skip = ops.step_guard(self._skip, *[nd.lstm_ws for nd in self.nodes if nd.cls == "lstm"])   # LRCNEngine._finish_step
        if self.lars is not None:
            self._lars_trust_launch(clip_norm, stats_step)
        if self.lamb is not None:                 # LRCNEngine._finish_step
            self._lamb_launch(lr, clip_norm, skip, stats_step, False)
        elif tiers is not None and self.optimizer == "adam":
            ops.adam_apply_tiers(self.w, self.g, self.adam_m, self.adam_v, tiers, lr, self.step_count, clip_norm, self.ss, 1.0, skip=skip)
        elif self.optimizer == "adam":
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
        self._sync()
        self.check_status()
        st = self.stats.cpu().numpy()
        if partial:
            return self._fetch_topk({"loss": float(st[0]) / max(rows, 1), "accuracy": float(st[1]) / max(rows, 1), "rows": rows,
                                     "loss_sum": float(st[0]), "correct": float(st[1])}, st, rows)
        out = {"loss": float(st[0]) / max(rows, 1), "accuracy": float(st[1]) / max(rows, 1),
               "grad_norm": math.sqrt(float(self.ss.item())), "rows": rows, "loss_sum": float(st[0]), "correct": float(st[1])}
        self._fetch_topk(out, st, rows)
        if self.ss2 is not None:
            out["reg_loss"] = float(self.ss2[1].item())
        return self._stats_result(out)


class _TowerReduce:
    """Lets a tower's backward issue its gradient chunks on the shared flat buffer (its own `g` is a slice of it)."""

    def __init__(self, graph, base):
        self.graph, self.base, self.world = graph, base, graph.dp.world

    def reduce_async(self, flat, offset, count):
        self.graph._reduce(self.base + offset, count)

    def wait(self):
        self.graph.dp.wait()
