"""Settings: the `run:` block of the reference's YAML (settings_.py:210-444; key list in SURVEY.md Appendix A)."""
import logging
import os
from shutil import copyfile

import yaml

from .defs_ import defs
from .feeder import Feeder
from .parse_opts import parse_seq
from .utils_ import CustomLogger, debug, error, get_datetime_str, info, warning


class Network:
    description = "Network representative class"


class TrainSettings:
    batch_size, epochs, epoch_index = 100, 15, 0
    optimizer, base_lr, lr_mult = defs.optim.sgd, 0.001, None
    lr_decay, clip_norm, dropout_keep_prob = None, 0, 0.5
    momentum, nesterov = 0.0, False
    weight_decay = 0.0
    accumulate = 1
    fc_dropout_keep_prob = 0.0
    ema_decay, ema_warmup = 0.0, False
    lars_eeta, lars_epsilon = 0.0, 0.0
    lamb, lamb_epsilon = False, None
    label_smoothing, top_k = 0.0, 0
    mixup_alpha, mixup_seed = 0.0, 0
    cutmix_alpha, cutmix_seed, cutmix_mode, cutmix_prob = 0.0, 0, None, None
    erase = (0.0, None, None, None, None, None, 0)     # erase_prob, _scale, _ratio, _frames, _mode, _std, _seed (NetConfig's fields)
    class_weights, focal_gamma = None, 0.0


class ValSettings:
    batch_size, logits_save_interval = 88, -1
    clip_fusion_type, clip_fusion_method = defs.fusion_type.late, defs.fusion_method.avg
    use_ema = False
    top_k = 0
    per_class = False


def balanced_class_weights(item_labels, num_classes):
    """`train: class_weights: balanced`: w_c = N / (C n_c), n_c the occurrences of class c among the labels of the item list (one list
    of labels per item, as Dataset.read_frames_metadata keeps them; a multi-label item counts once per label) and N their total --
    sklearn's compute_class_weight("balanced").  A class without an occurrence gets 1.0.  -> (weights, the absent classes)."""
    counts = [0] * num_classes
    for labels in item_labels:
        for l in labels:
            c = int(l)
            if not 0 <= c < num_classes:
                error("train.class_weights: balanced: the item list holds the label %s, outside the %d classes" % (l, num_classes))
            counts[c] += 1
    total = sum(counts)
    if total == 0:
        error("train.class_weights: balanced: the training item list holds no label")
    absent = [c for c, n in enumerate(counts) if n == 0]
    return [total / (num_classes * n) if n else 1.0 for n in counts], absent


def balanced_pos_weights(item_labels, num_classes):
    """`train: class_weights: balanced` under `network: label_type: multiple`: the positive-term weight q_c = (N - n_c) / n_c, N the
    number of items of the list and n_c the number of items that carry class c (a label repeated inside one item counts once) -- the
    negatives-to-positives ratio that torch documents for BCEWithLogitsLoss's pos_weight.  A class no item carries gets 1.0.
    -> (weights, the absent classes)."""
    counts, items = [0] * num_classes, 0
    for labels in item_labels:
        items += 1
        for c in sorted(set(int(l) for l in labels)):
            if not 0 <= c < num_classes:
                error("train.class_weights: balanced: the item list holds the label %s, outside the %d classes" % (c, num_classes))
            counts[c] += 1
    if items == 0 or sum(counts) == 0:
        error("train.class_weights: balanced: the training item list holds no label")
    absent = [c for c, n in enumerate(counts) if n == 0]
    return [(items - n) / n if n else 1.0 for n in counts], absent


class Settings:
    label_type = defs.label_type.single

    def __init__(self):
        self.run_id, self.resume_file, self.run_folder = "", None, None
        self.tensor_stats_interval = 0
        self.global_step = 0
        self.feeder = None
        self.pipelines, self.pipeline_names = {}, []
        self.train = self.val = None

    def should_resume(self):
        return bool(self.resume_file)

    def get_dropout(self):
        return self.train.dropout_keep_prob if self.phase == defs.phase.train else 0.0

    def get_fc_dropout(self):
        """train.fc_dropout_keep_prob (dropout on relu(fc6) / relu(fc7) of the dcnn towers); 0 = off, and outside the train phase."""
        return self.train.fc_dropout_keep_prob if self.phase == defs.phase.train else 0.0

    def get_ema(self):
        """(train.ema_decay, train.ema_warmup): the shadow weights of tf.train.ExponentialMovingAverage; (0, False) = off, and outside
        the train phase (validation reads a stored shadow through val.use_ema, it keeps none of its own)."""
        return (self.train.ema_decay, self.train.ema_warmup) if self.phase == defs.phase.train else (0.0, False)

    def get_lars(self):
        """(train.lars_eeta, train.lars_epsilon): tf.contrib.opt.LARSOptimizer's trust ratio on the momentum update; (0, 0) = off, and
        outside the train phase."""
        return (self.train.lars_eeta, self.train.lars_epsilon) if self.phase == defs.phase.train else (0.0, 0.0)

    def get_label_smoothing(self):
        """train.label_smoothing (tf.losses.softmax_cross_entropy's label_smoothing); 0 = off, and outside the train phase."""
        return self.train.label_smoothing if self.phase == defs.phase.train else 0.0

    def get_top_k(self):
        """train.top_k: the k of the top-k accuracy a training step also counts; 0 = off, and outside the train phase (validation ranks
        its fused logits on the host under val.top_k, Validation.get_topk_accuracy)."""
        return self.train.top_k if self.phase == defs.phase.train else 0

    def get_class_weights(self):
        """train.class_weights as the numbers the engine takes (a list, or the balanced weights of the training item list, formed by
        initialize once the datasets are read); None = off, and outside the train phase."""
        if self.phase != defs.phase.train or self.train.class_weights is None:
            return None
        if isinstance(self.train.class_weights, str):
            error("train.class_weights: balanced needs the training datasets, which are not read yet")
        return self.train.class_weights

    def get_focal_gamma(self):
        """train.focal_gamma (the focal loss's focusing parameter); 0 = off, and outside the train phase."""
        return self.train.focal_gamma if self.phase == defs.phase.train else 0.0

    def get_mixup(self):
        """(train.mixup_alpha, train.mixup_seed): mixup's Beta(alpha, alpha) and the key of its draws (engine.check_mixup,
        engine.mixup_lambda); (0, 0) = off, and outside the train phase (validation never blends)."""
        return (self.train.mixup_alpha, self.train.mixup_seed) if self.phase == defs.phase.train else (0.0, 0)

    def get_erase(self):
        """(train.erase_prob, erase_scale, erase_ratio, erase_frames, erase_mode, erase_std, erase_seed): random erasing's chance per
        clip, the ranges of its box, its fill and the key of its draws, checked and with the defaults filled in (engine.check_erase,
        engine.erase_row); (0, None, None, None, None, None, 0) = off, and outside the train phase (validation never erases)."""
        return self.train.erase if self.phase == defs.phase.train else TrainSettings.erase

    def get_cutmix(self):
        """(train.cutmix_alpha, train.cutmix_seed, train.cutmix_mode, train.cutmix_prob): CutMix / VideoMix's Beta(alpha, alpha), the key
        of its box draws, the axes the box spans and, with mixup on too, the chance that a batch is cut (engine.check_cutmix,
        engine.cutmix_box); (0, 0, None, None) = off, and outside the train phase (validation never cuts)."""
        t = self.train
        return (t.cutmix_alpha, t.cutmix_seed, t.cutmix_mode, t.cutmix_prob) if self.phase == defs.phase.train else (0.0, 0, None, None)

    def get_lamb(self):
        """(train.lamb, train.lamb_epsilon): LAMB in the place of the Adam update (engine.check_lamb; the epsilon is the checked one,
        TFA's 1e-6 when the key is absent); (False, None) = off, and outside the train phase."""
        on = self.phase == defs.phase.train and self.train.lamb
        return (True, self.train.lamb_epsilon) if on else (False, None)

    def get_tensor_stats_interval(self):
        """logging.tensor_stats_interval (per-variable gradient / weight statistics every N updates); 0 = off, and outside the train phase."""
        return self.tensor_stats_interval if self.phase == defs.phase.train else 0

    # ---- pipelines (settings_.py:134-208) ---------------------------------------------------------------
    def read_field(self, config, fieldname, validate=None, required=False, listify=False):
        self.pipeline_field_cache.append(fieldname)
        val = config.get(fieldname)
        if val is None:
            if required:
                error("No default value specified for missing field [%s]" % fieldname)
            return [None] if listify else None
        if validate is not None:
            if isinstance(validate, (list, tuple)):
                val = list(parse_seq(val))
                if len(validate) != len(val):
                    error("Field [%s] required %d entries, found: [%s]" % (fieldname, len(validate), str(val)))
                val = [defs.check(el, v) for el, v in zip(val, validate)]
            else:
                val = defs.check(val, validate)
        if listify and not isinstance(val, (list, tuple)):
            val = [val]
        return val

    def read_network(self, content):
        network = Network()
        self.pipeline_field_cache = []
        network.input = list(self.read_field(content, "input", listify=True))
        if any(x is None for x in network.input):
            error("<None> or undefined <input> tag in pipeline: %s" % content)
        for i, inp in enumerate(network.input):
            if inp not in self.pipelines:
                ok, tagname = defs.check(inp, defs.dataset_tag, do_boolean=True)
                if not ok:
                    error("Input identifier [%s] is not a dataset tag, but no such pipeline has been declared yet." % inp)
                network.input[i] = tagname
        network.representation = self.read_field(content, "representation", required=True, validate=defs.representation)
        network.frame_encoding_layer = None
        if network.representation == defs.representation.dcnn:
            network.frame_encoding_layer = self.read_field(content, "frame_encoding_layer", required=True)
        if network.representation == defs.representation.fc:
            network.fc_output_dim = self.read_field(content, "fc_output_dim", required=True)
        network.classifier = self.read_field(content, "classifier", validate=defs.classifier)
        network.lstm_params = None
        if network.classifier == defs.classifier.lstm:
            params = parse_seq(self.read_field(content, "lstm_params", required=True))
            network.lstm_params = [int(params[0]), int(params[1]), defs.check(params[2], defs.fusion_method)]
        network.lstm_bidirectional = self.read_lstm_bidirectional(content, network)
        network.rnn_cell = self.read_rnn_cell(content, network)
        network.attn_dim = self.read_attn_dim(content, network)
        network.vlad_clusters = self.read_vlad_clusters(content, network)
        network.sa_heads, network.sa_positions = self.read_self_attention(content, network)
        network.sa_block, network.sa_ffn_dim = self.read_sa_block(content, network)
        network.sa_attn_dropout, network.sa_dropout, network.sa_drop_path = self.read_sa_dropout(content, network)
        network.tcn_kernel, network.tcn_dilation, network.tcn_causal = self.read_temporal_conv(content, network)
        network.weights_file = self.read_field(content, "weights_file")
        network.frame_fusion = self.read_field(content, "frame_fusion", validate=(defs.fusion_type, defs.fusion_method))
        if network.frame_fusion and network.frame_fusion[1] == defs.fusion_method.attn:
            error("frame_fusion: attn is a fusion of the recurrent classifier (lstm_params), not a frame fusion")
        if network.frame_fusion and network.frame_fusion[1] == defs.fusion_method.vlad:
            error("frame_fusion: vlad is a fusion of the recurrent classifier (lstm_params), not a frame fusion")
        network.input_shape = self.read_field(content, "input_shape", listify=True)
        network.input_fusion = self.read_field(content, "input_fusion", validate=defs.fusion_method)
        if network.input_fusion == defs.fusion_method.attn:
            error("input_fusion: attn is a fusion of the recurrent classifier (lstm_params), not an input fusion")
        if network.input_fusion == defs.fusion_method.vlad:
            error("input_fusion: vlad is a fusion of the recurrent classifier (lstm_params), not an input fusion")
        network.train_from = self.read_train_from(content, network)
        unread = [x for x in content if x not in self.pipeline_field_cache]
        if unread:
            error("Undefined pipeline field(s):" + str(unread))
        return network

    def read_lstm_bidirectional(self, content, network):
        """`lstm_bidirectional: True` beside lstm_params (this project's extension of the pipeline schema): every LSTM layer gets a
        forward and a backward cell whose outputs are concatenated (tf.nn.bidirectional_dynamic_rnn).  Absent / None / False = off.
        Refused without the LSTM classifier and for a hidden size the one-launch recurrence cannot take."""
        v = self.read_field(content, "lstm_bidirectional")
        if v in (None, "None", False, "False"):
            return False
        if v not in (True, "True"):
            error("lstm_bidirectional must be True or False, got [%s]" % (v,))
        if network.classifier != defs.classifier.lstm:
            error("lstm_bidirectional needs classifier lstm, but the pipeline's classifier is [%s]" % network.classifier)
        from .engine import VltfError, check_blstm
        try:
            check_blstm(network.lstm_params[0])
        except VltfError as ex:
            error(str(ex))
        return True

    def read_rnn_cell(self, content, network):
        """`rnn_cell: gru` beside lstm_params (this project's extension of the pipeline schema): the layers of classifier lstm are
        reset-after GRU cells (engine.gru_names) of lstm_params' hidden size.  Absent / None / lstm = BasicLSTMCell.  Refused without the
        LSTM classifier, with lstm_bidirectional, with a second (state) input, above the hidden size the recurrence takes, and for any
        other value (engine.check_rnn_cell)."""
        v = self.read_field(content, "rnn_cell")
        if v in (None, "None"):
            return "lstm"
        from .engine import VltfError, check_rnn_cell
        lstm = network.classifier == defs.classifier.lstm
        state_input = lstm and len(network.input) > 1 and self.read_field(content, "input_fusion") in (None, "None")
        try:
            return check_rnn_cell(v, network.classifier, network.lstm_params[0] if lstm else 1, network.lstm_bidirectional, state_input)
        except VltfError as ex:
            error(str(ex))

    def read_attn_dim(self, content, network):
        """`attn_dim: <A>` beside lstm_params (this project's extension of the pipeline schema): the width of the scorer of fusion attn,
        learned attention pooling over the recurrent outputs (engine.attn_specs).  Absent / None = the recurrent output width.  Refused
        without fusion attn and unless an integer in 1..1024; fusion attn itself is refused without the recurrent classifier
        (engine.check_attn).  -> the width, or None for every other fusion."""
        v = self.read_field(content, "attn_dim")
        lstm = network.classifier == defs.classifier.lstm
        from .engine import VltfError, check_attn
        try:
            if not lstm:
                return check_attn(None, v, network.classifier)
            H = network.lstm_params[0] * (2 if network.lstm_bidirectional else 1)
            return check_attn(network.lstm_params[2], v, network.classifier, H)
        except VltfError as ex:
            error(str(ex))

    def read_self_attention(self, content, network):
        """`sa_heads: <n>` and `sa_positions: relative | none` beside `rnn_cell: mhsa` (this project's extension of the pipeline schema):
        the heads of the self-attention layers (must divide lstm_params' width; absent / None = 4 where 4 divides it, else 1) and their
        learned relative-position bias (absent / None = relative).  Refused without rnn_cell mhsa; the widths the launches take are
        checked against lstm_params here, the step count when the engine is built (engine.check_mhsa).  -> (heads, positions), or
        (None, None) for every other cell."""
        heads, positions = self.read_field(content, "sa_heads"), self.read_field(content, "sa_positions")
        from .engine import VltfError, check_mhsa
        lstm = network.classifier == defs.classifier.lstm
        try:
            sa = check_mhsa(network.rnn_cell, network.lstm_params[0] if lstm else 1, 1, heads, positions,
                            network.lstm_params[2] if lstm else "avg")
        except VltfError as ex:
            error(str(ex))
        return sa if sa else (None, None)

    def read_sa_block(self, content, network):
        """`sa_block: plain | encoder` and `sa_ffn_dim: <F>` beside `rnn_cell: mhsa` (this project's extension of the pipeline schema):
        `encoder` wraps every self-attention layer in the pre-LN Transformer encoder block (layer norm, residual, feed-forward block of
        width F; absent / None = 4 x lstm_params' width; 8..4096) behind an embedding and in front of a final norm
        (engine.encoder_specs); absent / None / plain = the bare layer.  Refused: either key without rnn_cell mhsa, sa_ffn_dim without
        sa_block encoder (engine.check_sa_block).  -> (block, F) as the engine takes them: (None, None) for the plain layer."""
        block, ffn = self.read_field(content, "sa_block"), self.read_field(content, "sa_ffn_dim")
        from .engine import VltfError, check_sa_block
        lstm = network.classifier == defs.classifier.lstm
        try:
            F = check_sa_block(network.rnn_cell, network.lstm_params[0] if lstm else 1, block, ffn)
        except VltfError as ex:
            error(str(ex))
        return ("encoder", F) if F else (None, None)

    def read_sa_dropout(self, content, network):
        """`sa_attn_dropout: p`, `sa_dropout: p` and `sa_drop_path: p` beside `rnn_cell: mhsa` (this project's extension of the pipeline
        schema): rates in [0, 1) of the dropout on the softmax weights, on the elements of the encoder block's two residual branches,
        and of stochastic depth over those branches (the linear rule 1 - p (l + 1) / L), in a training forward only (engine.SaDrop).
        Absent / None / 0 = off.  Refused by name: a key without rnn_cell mhsa, sa_dropout / sa_drop_path without sa_block encoder,
        bools, strings, NaN, values outside [0, 1) (engine.check_mhsa).  -> the three rates, None where off."""
        keys = ("sa_attn_dropout", "sa_dropout", "sa_drop_path")
        vals = [self.read_field(content, k) for k in keys]
        vals = [None if isinstance(v, str) and v == "None" else v for v in vals]
        from .engine import VltfError, check_mhsa, check_sa_rate
        lstm = network.classifier == defs.classifier.lstm
        try:
            check_mhsa(network.rnn_cell, network.lstm_params[0] if lstm else 1, 1, network.sa_heads, network.sa_positions,
                       network.lstm_params[2] if lstm else "avg", sa_block=network.sa_block, sa_ffn_dim=network.sa_ffn_dim,
                       sa_attn_dropout=vals[0], sa_dropout=vals[1], sa_drop_path=vals[2])
            rates = [check_sa_rate(k, v) for k, v in zip(keys, vals)]
        except VltfError as ex:
            error(str(ex))
        return tuple(r if r > 0 else None for r in rates)

    def read_temporal_conv(self, content, network):
        """`tcn_kernel: <k>`, `tcn_dilation: exponential | none` and `tcn_causal: True | False` beside `rnn_cell: tcn` (this project's
        extension of the pipeline schema): the layers of classifier lstm are dilated residual 1-D convolutions over the frames
        (engine.tcn_specs) of k taps (absent / None = 3; 1..9, odd unless causal), layer l dilated by 2^l (absent / None / exponential;
        at most 17 layers) or by 1 (none), centred (absent / None / False) or causal.  Refused by name: a key without rnn_cell tcn,
        fusion state, a width above 1024 (engine.check_tcn).  -> (k, dilation, causal) as the engine takes them, or (None, None, None)
        for every other cell."""
        k, dil, causal = (self.read_field(content, key) for key in ("tcn_kernel", "tcn_dilation", "tcn_causal"))
        causal = {"True": True, "False": False}.get(causal, causal) if isinstance(causal, str) else causal
        from .engine import VltfError, check_tcn
        lstm = network.classifier == defs.classifier.lstm
        try:
            tc = check_tcn(network.rnn_cell, network.lstm_params[0] if lstm else 1, network.lstm_params[1] if lstm else 1, k, dil, causal,
                           network.lstm_params[2] if lstm else "avg")
        except VltfError as ex:
            error(str(ex))
        return tc if tc else (None, None, None)

    def read_vlad_clusters(self, content, network):
        """`vlad_clusters: <K>` beside lstm_params (this project's extension of the pipeline schema): the number of centres of fusion
        vlad, NetVLAD pooling over the recurrent outputs (engine.vlad_specs).  Absent / None = 8.  Refused without fusion vlad, unless
        an integer in 2..64, and where K x the recurrent output width exceeds 16384; fusion vlad itself is refused without the recurrent
        classifier (engine.check_vlad).  -> K, or None for every other fusion."""
        v = self.read_field(content, "vlad_clusters")
        lstm = network.classifier == defs.classifier.lstm
        from .engine import VltfError, check_vlad
        try:
            if not lstm:
                return check_vlad(None, v, network.classifier)
            H = network.lstm_params[0] * (2 if network.lstm_bidirectional else 1)
            return check_vlad(network.lstm_params[2], v, network.classifier, H)
        except VltfError as ex:
            error(str(ex))

    def read_train_from(self, content, network):
        """`train_from: <layer>` (this project's extension of the pipeline schema): the first dcnn layer that trains -- every dcnn layer
        before it keeps its weights; `classifier` freezes the whole dcnn (engine.frozen_layers)."""
        layer = self.read_field(content, "train_from")
        if layer in (None, "None"):
            return None
        if network.representation != defs.representation.dcnn:
            error("train_from freezes dcnn layers, but the pipeline's representation is [%s]" % network.representation)
        from .engine import NetConfig, VltfError, frozen_layers
        try:
            frozen_layers(NetConfig(frame_encoding_layer=network.frame_encoding_layer, train_from=str(layer)))
        except VltfError as ex:
            error(str(ex))
        return str(layer)

    @staticmethod
    def read_tensor_stats_interval(lg):
        """`logging: tensor_stats_interval: N` (this project's extension of the logging block, next to the reference's print_tensors /
        tensorboard_folder): per-variable statistics every N updates (engine.stat_segments).  Absent / None / 0 = off; a quoted number
        is read as the number."""
        from .engine import VltfError, check_tensor_stats_interval
        n = lg.get("tensor_stats_interval")
        if isinstance(n, str) and n != "None":
            try:
                n = int(n)
            except ValueError:
                pass
        try:
            return check_tensor_stats_interval(None if n == "None" else n)
        except VltfError as ex:
            error("logging.tensor_stats_interval: %s" % ex)

    @staticmethod
    def read_top_k(obj, where):
        """`train: top_k: K` / `val: top_k: K` (this project's extension): absent / None / 0 = off; a quoted number is read as the number."""
        from .engine import VltfError, check_top_k
        k = obj.get("top_k")
        if isinstance(k, str) and k != "None":
            try:
                k = int(k)
            except ValueError:
                pass
        try:
            return check_top_k(None if k == "None" else k)
        except VltfError as ex:
            error("%s.top_k: %s" % (where, ex))

    def read_loss_weights(self, obj):
        """`train: class_weights: [w_0, ..]` | `balanced` and `train: focal_gamma: G` (this project's extension): absent /
        None = off; quoted numbers are read as numbers.  -> (a list of num_classes floats | "balanced" | None, gamma)."""
        from .engine import VltfError, check_class_weights, check_focal_gamma

        def number(v):
            if isinstance(v, str) and v != "None":      # a quoted number; nan / inf come as strings too
                try:
                    return float(v)
                except ValueError:
                    pass
            return v

        cw = obj.get("class_weights")
        if cw in (None, "None"):
            cw = None
        elif isinstance(cw, str) and cw.strip().lower() == "balanced":
            cw = "balanced"
        else:
            if isinstance(cw, str):                      # "1, 2.5, 1" / "[1, 2.5, 1]"
                cw = [x for x in cw.replace("[", " ").replace("]", " ").replace(",", " ").split()]
            try:
                w = check_class_weights([number(v) for v in cw] if isinstance(cw, (list, tuple)) else cw, self.num_classes)
                cw = [float(v) for v in w]
            except VltfError as ex:
                error("train.class_weights: %s" % ex)
        g = number(obj.get("focal_gamma"))
        try:
            return cw, check_focal_gamma(None if g == "None" else g)
        except VltfError as ex:
            error("train.focal_gamma: %s" % ex)

    @staticmethod
    def read_label_type(network):
        """`network: label_type: defs.label_type.multiple` (the reference's name for the case; a plain `multiple` / `single` is read
        too): absent / None = single.  multiple: multi-hot label rows under the sigmoid loss (engine.check_label_type)."""
        from .engine import VltfError, check_label_type
        v = network.get("label_type")
        if v in (None, "None"):
            return defs.label_type.single
        if isinstance(v, str) and v.startswith("defs."):
            return defs.check(v, defs.label_type)
        try:
            return check_label_type(v)
        except VltfError as ex:
            error("network.label_type: %s" % ex)

    def check_multilabel_options(self):
        """The options label_type multiple refuses: a top-k count (a multi-hot row has no one label to rank) and the per-class recall
        (it files an item under one class); validation reports AP per class and mAP instead (Validation.get_multilabel)."""
        if self.label_type != defs.label_type.multiple:
            return
        for where, s in (("train", self.train), ("val", self.val)):
            if s is not None and s.top_k > 0:
                error("%s.top_k: %d is refused with network.label_type multiple: a multi-hot row has no one label to rank" % (where, s.top_k))
        if self.val is not None and self.val.per_class:
            error("val.per_class is refused with network.label_type multiple: it files an item under one class; a multiple run writes "
                  "ap_per_class_<run_id> and map_<run_id>")

    def resolve_balanced_weights(self):
        """After the datasets are read: `class_weights: balanced` becomes the numbers, from the main training dataset's item list."""
        if not self.train or self.train.class_weights != "balanced":
            return
        main = [d for d in self.feeder.datasets.get(defs.phase.train, []) if d.tag == defs.dataset_tag.main]
        if not main:
            error("train.class_weights: balanced: there is no [%s] training dataset to count the labels of" % defs.dataset_tag.main)
        balanced = balanced_pos_weights if self.label_type == defs.label_type.multiple else balanced_class_weights
        weights, absent = balanced(main[0].labels, self.num_classes)
        if absent:
            warning("train.class_weights: balanced: no item of class(es) %s in [%s]: their weight is 1.0" % (absent, main[0].id))
        self.train.class_weights = weights

    # ---- run block (settings_.py:210-366) -------------------------------------------------------------------
    def read_config(self, config, init_file):
        self.resume_file = config.get("resume_file")
        self.run_folder = config["run_folder"]
        self.run_id = config.get("run_id") or ""
        self.phases = defs.check(config["phase"], defs.phase)
        if not isinstance(self.phases, list):
            self.phases = [self.phases]
        self.phase = self.phases[0]
        trainval = ("train" if defs.phase.train in self.phases else "") + ("val" if defs.phase.val in self.phases else "")
        trainval += "_resume" if self.should_resume() else "_scratch"
        self.run_id = "_".join([self.run_id or os.path.basename(init_file), trainval])
        os.makedirs(self.run_folder, exist_ok=True)       # (every rank of a data-parallel launch gets here at the same moment)
        lg = config["logging"]
        self.save_freq_per_epoch = lg["save_freq_per_epoch"]
        self.logging_level = lg["level"]
        self.tensorboard_folder = lg.get("tensorboard_folder", "tensorboard")
        self.print_tensors = lg.get("print_tensors", False)
        self.configure_logging()
        self.tensor_stats_interval = self.read_tensor_stats_interval(lg)

        for pipeline in config["network"]["pipelines"]:
            pname, content = list(pipeline.items())[0]
            debug("Reading network [%s]" % pname)
            self.pipelines[pname] = self.read_network(content)
            self.pipeline_names.append(pname)
        self.num_classes = int(config["network"]["num_classes"])
        self.label_type = self.read_label_type(config["network"])

        for phase in self.phases:
            obj = config[phase]
            if phase == defs.phase.train:
                t = self.train = TrainSettings()
                t.batch_size, t.epochs = int(obj["batch_size"]), int(obj["epochs"])
                t.optimizer = defs.check(obj["optimizer"], defs.optim)
                if t.optimizer not in (defs.optim.sgd, defs.optim.adam):        # train.py:171,208 (rmsprop is a name without an update)
                    error("Undefined optimizer %s" % t.optimizer)
                t.base_lr = float(obj["base_lr"])
                # two learning-rate tiers (train.py:152-197, whose own code is broken: SURVEY 2): the `modified` variables -- fc8, the
                # LSTM, the fc heads -- learn with base_lr * lr_mult, the pretrained dcnn with base_lr (engine.is_regular)
                t.lr_mult = float(obj["lr_mult"]) if obj.get("lr_mult") not in (None, "None") else None
                if t.lr_mult is not None and not (t.lr_mult > 0 and t.lr_mult != float("inf")):
                    error("lr_mult must be a finite number > 0, got [%s] (train_from holds layers fixed)" % obj["lr_mult"])
                # SGD with momentum (tf.train.MomentumOptimizer; the reference's `#momentum: 0.9`): absent / None = plain SGD
                from .engine import VltfError, check_momentum
                nesterov = obj.get("nesterov") if obj.get("nesterov") not in (None, "None") else False
                if not isinstance(nesterov, bool):
                    error("train.nesterov must be a boolean, got [%s]" % (nesterov,))
                try:
                    t.momentum, t.nesterov = check_momentum(
                        t.optimizer, float(obj["momentum"]) if obj.get("momentum") not in (None, "None") else 0.0, nesterov)
                except (VltfError, TypeError, ValueError) as ex:
                    error("train.momentum / train.nesterov: %s" % ex)
                # L2 weight decay of the trained weight tensors (engine.decay_ranges): absent / None = off
                from .engine import check_weight_decay
                wd = obj.get("weight_decay")
                if isinstance(wd, str) and wd != "None":         # YAML reads 5e-4 (no dot) and nan / inf as strings
                    try:
                        wd = float(wd)
                    except ValueError:
                        pass
                try:
                    t.weight_decay = check_weight_decay(None if wd == "None" else wd)
                except VltfError as ex:
                    error("train.weight_decay: %s" % ex)
                # gradient accumulation: `accumulate` consecutive batches of an epoch make one update (train.accumulate_groups); batch_size
                # stays what one call feeds.  absent / None = 1
                from .engine import check_accumulate
                try:
                    t.accumulate = check_accumulate(None if obj.get("accumulate") == "None" else obj.get("accumulate"))
                except VltfError as ex:
                    error("train.accumulate: %s" % ex)
                # dropout on the ReLU'd fc layers of the AlexNet towers (Caffe's drop6 / drop7; engine.check_fc_dropout): absent / None = off
                from .engine import check_fc_dropout
                fk = obj.get("fc_dropout_keep_prob")
                if isinstance(fk, str) and fk != "None":         # a quoted number; nan / inf come as strings too
                    try:
                        fk = float(fk)
                    except ValueError:
                        pass
                try:
                    t.fc_dropout_keep_prob = check_fc_dropout(None if fk == "None" else fk)
                except VltfError as ex:
                    error("train.fc_dropout_keep_prob: %s" % ex)
                # exponential moving average of the weights (tf.train.ExponentialMovingAverage; engine.check_ema): absent / None = off
                from .engine import check_ema
                ed = obj.get("ema_decay")
                if isinstance(ed, str) and ed != "None":         # a quoted number; nan / inf come as strings too
                    try:
                        ed = float(ed)
                    except ValueError:
                        pass
                try:
                    t.ema_decay, t.ema_warmup = check_ema(None if ed == "None" else ed,
                                                          None if obj.get("ema_warmup") == "None" else obj.get("ema_warmup"))
                except VltfError as ex:
                    error("train.ema_decay / train.ema_warmup: %s" % ex)
                # LARS, layer-wise adaptive learning rates on the momentum update (tf.contrib.opt.LARSOptimizer; engine.check_lars):
                # absent / None = off
                from .engine import check_lars
                lv = []
                for key in ("lars_eeta", "lars_epsilon"):
                    v = obj.get(key)
                    if isinstance(v, str) and v != "None":       # YAML reads 1e-3 (no dot) and nan / inf as strings
                        try:
                            v = float(v)
                        except ValueError:
                            pass
                    lv.append(None if v == "None" else v)
                try:
                    t.lars_eeta, t.lars_epsilon = check_lars(t.optimizer, t.momentum, lv[0], lv[1])
                except VltfError as ex:
                    error("train.lars_eeta / train.lars_epsilon: %s" % ex)
                # LAMB, layer-wise trust ratios and decoupled decay on the Adam update (tfa.optimizers.LAMB; engine.check_lamb):
                # absent / None = off
                from .engine import check_lamb
                le = obj.get("lamb_epsilon")
                if isinstance(le, str) and le != "None":         # YAML reads 1e-6 (no dot) and nan / inf as strings
                    try:
                        le = float(le)
                    except ValueError:
                        pass
                try:
                    t.lamb, eps = check_lamb(t.optimizer, None if obj.get("lamb") == "None" else obj.get("lamb"), None if le == "None" else le)
                    t.lamb_epsilon = eps if t.lamb else None
                except VltfError as ex:
                    error("train.lamb / train.lamb_epsilon: %s" % ex)
                # label smoothing of the loss (tf.losses.softmax_cross_entropy(label_smoothing=); engine.check_label_smoothing) and the top-k
                # accuracy counted in the same launch (engine.check_top_k): absent / None = off
                from .engine import check_label_smoothing
                ls = obj.get("label_smoothing")
                if isinstance(ls, str) and ls != "None":         # a quoted number; nan / inf come as strings too
                    try:
                        ls = float(ls)
                    except ValueError:
                        pass
                try:
                    t.label_smoothing = check_label_smoothing(None if ls == "None" else ls)
                except VltfError as ex:
                    error("train.label_smoothing: %s" % ex)
                t.top_k = self.read_top_k(obj, "train")
                # mixup (Zhang et al. 2018): clips and labels blended in pairs inside a rank's batch, the weight drawn from
                # Beta(mixup_alpha, mixup_alpha) under the key mixup_seed (engine.check_mixup, engine.mixup_lambda): absent / None = off
                from .engine import check_mixup
                mx = [obj.get("mixup_alpha"), obj.get("mixup_seed")]
                for i, conv in enumerate((float, int)):
                    if isinstance(mx[i], str) and mx[i] != "None":     # a quoted number; nan / inf come as strings too
                        try:
                            mx[i] = conv(mx[i])
                        except ValueError:
                            pass
                try:
                    t.mixup_alpha, t.mixup_seed = check_mixup(*(None if v == "None" else v for v in mx))
                except VltfError as ex:
                    error("train.mixup_alpha / train.mixup_seed: %s" % ex)
                # CutMix / VideoMix (Yun et al. 2019, 2020): one box swapped in pairs inside a rank's batch, the cut fraction drawn from
                # Beta(cutmix_alpha, cutmix_alpha) under the key cutmix_seed (engine.check_cutmix, engine.cutmix_box): absent / None = off
                from .engine import check_cutmix
                cm = [obj.get("cutmix_alpha"), obj.get("cutmix_seed"), obj.get("cutmix_mode"), obj.get("cutmix_prob")]
                for i, conv in enumerate((float, int, None, float)):
                    if conv is not None and isinstance(cm[i], str) and cm[i] != "None":      # a quoted number
                        try:
                            cm[i] = conv(cm[i])
                        except ValueError:
                            pass
                try:
                    a, sd, md, pr = check_cutmix(*(None if v == "None" else v for v in cm))
                    t.cutmix_alpha, t.cutmix_seed = a, sd
                    t.cutmix_mode, t.cutmix_prob = (md, pr) if a > 0.0 else (None, None)
                except VltfError as ex:
                    error("train.cutmix_alpha / train.cutmix_seed / train.cutmix_mode / train.cutmix_prob: %s" % ex)
                # random erasing (Zhong et al. 2017): every clip gets a box of its own, or none, filled with the mean colour or noise
                # (engine.check_erase, engine.erase_row): absent / None = off
                from .engine import check_erase
                names = ("erase_prob", "erase_scale", "erase_ratio", "erase_frames", "erase_mode", "erase_std", "erase_seed")
                er = [obj.get(k) for k in names]
                for i, conv in enumerate((float, None, None, None, None, float, int)):
                    if conv is not None and isinstance(er[i], str) and er[i] != "None":      # a quoted number
                        try:
                            er[i] = conv(er[i])
                        except ValueError:
                            pass
                try:
                    e = check_erase(*(None if v == "None" else v for v in er))
                    t.erase = tuple(e) if e.prob > 0.0 else TrainSettings.erase
                except VltfError as ex:
                    error("train.%s: %s" % (" / train.".join(names), ex))
                # class weights inside the loss's class sum and the focal loss (engine.check_class_weights, engine.check_focal_gamma;
                # `balanced` is resolved by initialize, from the training item list): absent / None = off
                t.class_weights, t.focal_gamma = self.read_loss_weights(obj)
                if obj.get("lr_decay") in (None, "None"):
                    t.lr_decay = None
                else:
                    d = parse_seq(obj["lr_decay"])
                    t.lr_decay = [defs.check(d[0], defs.decay), defs.check(d[1], defs.periodicity), int(d[2]), float(d[3])] + \
                        ([int(d[4])] if len(d) > 4 else [])
                t.clip_norm = int(obj["clip_norm"]) if obj.get("clip_norm") not in (None, "None") else 0
                t.dropout_keep_prob = float(obj["dropout_keep_prob"])
            if phase == defs.phase.val:
                v = self.val = ValSettings()
                v.batch_size = int(obj["batch_size"])
                v.logits_save_interval = int(obj["logits_save_interval"])
                cf = parse_seq(obj["clip_fusion"])
                v.clip_fusion_type, v.clip_fusion_method = defs.check(cf[0], defs.fusion_type), defs.check(cf[1], defs.fusion_method)
                if v.clip_fusion_method == defs.fusion_method.attn:
                    error("val.clip_fusion: attn is a fusion of the recurrent classifier (lstm_params), not a fusion of a video's clips")
                if v.clip_fusion_method == defs.fusion_method.vlad:
                    error("val.clip_fusion: vlad is a fusion of the recurrent classifier (lstm_params), not a fusion of a video's clips")
                # evaluate the averaged weights a training run with train.ema_decay stored beside its weights: absent / None = the weights
                ue = obj.get("use_ema") if obj.get("use_ema") not in (None, "None") else False
                if not isinstance(ue, bool):
                    error("val.use_ema must be a boolean, got [%s]" % (ue,))
                v.use_ema = ue
                # top-k accuracy of the fused per-video logits beside the top-1 one (Validation.get_topk_accuracy): absent / None = off
                v.top_k = self.read_top_k(obj, "val")
                # recall per class and the mean-class accuracy of the fused per-video logits (Validation.get_per_class): absent / None = off
                pc = obj.get("per_class") if obj.get("per_class") not in (None, "None") else False
                if not isinstance(pc, bool):
                    error("val.per_class must be a boolean, got [%s]" % (pc,))
                v.per_class = pc
        self.check_multilabel_options()

        self.feeder = Feeder(defs.input_mode.video, self.phases, (self.train, self.val), self.save_freq_per_epoch, self.run_folder,
                             self.should_resume())
        for dataid, dataobj in config["data"].items():
            dataset_phase = defs.check(dataobj["phase"], defs.phase)
            if dataset_phase not in self.phases:
                info("Omitting dataset [%s] due to its phase [%s]" % (dataid, dataset_phase))
                continue
            mean_image = parse_seq(dataobj["mean_image"]) if "mean_image" in dataobj else None
            batch_item = defs.check(dataobj["batch_item"], defs.batch_item) if "batch_item" in dataobj else defs.batch_item.default
            image_shape = parse_seq(dataobj["image_shape"]) if "image_shape" in dataobj else None
            imgproc = [defs.check(o, defs.imgproc) for o in (parse_seq(dataobj["imgproc"]) if "imgproc" in dataobj else [])]
            if defs.imgproc.sub_mean in imgproc and not mean_image:
                error("[%s] option requires a supplied mean image intensity." % defs.imgproc.sub_mean)
            raw_image_shape = parse_seq(dataobj["raw_image_shape"]) if "raw_image_shape" in dataobj else None
            ncrop = sum(o in imgproc for o in (defs.imgproc.rand_crop, defs.imgproc.center_crop, defs.imgproc.resize))
            if ncrop > 1:
                error("Need at most one image processing parameter. Imgproc params : %s" % imgproc)
            if mean_image is not None and defs.imgproc.sub_mean not in imgproc:
                imgproc.append(defs.imgproc.sub_mean)                      # settings_.py:341-342
            if self.val and (defs.imgproc.rand_crop in imgproc or defs.imgproc.rand_mirror in imgproc):
                error("Random cropping / mirroring is enabled in validation mode (the reference prompts; we fail).")
            crop_jitter = self.read_crop_jitter(dataid, dataobj, dataset_phase, imgproc)
            self.feeder.add_dataset(dataset_phase, dataid, dataobj["data_path"], mean_image, dataobj.get("prepend_folder"),
                                    image_shape, imgproc, raw_image_shape, defs.check(dataobj["data_format"], defs.data_format),
                                    dataobj.get("frame_format"), batch_item, self.num_classes,
                                    defs.check(dataobj["tag"], defs.dataset_tag), int(dataobj.get("read_tries", 1)),
                                    crop_jitter=crop_jitter)

    def read_crop_jitter(self, dataid, dataobj, dataset_phase, imgproc):
        """imgproc rand_resized_crop with its keys crop_scale / crop_ratio / crop_seed of one dataset ->
        dataset_.check_crop_jitter's (scale, ratio, seed), or None without the imgproc entry.  Every misuse is refused here."""
        from .dataset_ import check_crop_jitter
        name = defs.imgproc.rand_resized_crop
        keys = [k for k in ("crop_scale", "crop_ratio", "crop_seed") if dataobj.get(k) not in (None, "None")]
        if name not in imgproc:
            if keys:
                error("dataset [%s]: %s need imgproc [%s], which is not listed" % (dataid, keys, name))
            return None
        other = [o for o in (defs.imgproc.rand_crop, defs.imgproc.center_crop, defs.imgproc.resize) if o in imgproc]
        if other:
            error("dataset [%s]: imgproc [%s] resamples its own box to the network input and is refused together with %s" %
                  (dataid, name, other))
        if dataset_phase == defs.phase.val:
            error("dataset [%s]: imgproc [%s] on a validation dataset: a random validation crop is a mistake" % (dataid, name))
        # (a vectors dataset is known by its size file only: Dataset.initialize_imgproc refuses the entry there)
        vals = [dataobj.get(k) if dataobj.get(k) != "None" else None for k in ("crop_scale", "crop_ratio", "crop_seed")]
        try:
            return check_crop_jitter(*(parse_seq(v) if isinstance(v, str) else v for v in vals))
        except ValueError as ex:
            error("dataset [%s]: %s" % (dataid, ex))

    def configure_logging(self):
        self.timestamp = get_datetime_str()
        logfile = os.path.join(self.run_folder, "log_" + self.run_id + "_" + self.timestamp + ".log")
        if int(os.environ.get("RANK", "0")) > 0:      # data parallel: rank 0 owns the run's log file, the others log to the console
            logfile = None
        self.logger = CustomLogger()
        self.logger.configure_logging(logfile, self.logging_level)

    def initialize(self, init_file):
        """settings_.py:404-444 -> Feeder."""
        if not os.path.exists(init_file):
            raise Exception("Unable to read initialization file [%s]." % init_file)
        if init_file.endswith(".ini"):
            raise Exception(".ini files deprecated.")
        with open(init_file, "r") as f:
            config = yaml.safe_load(f)["run"]
        self.read_config(config, init_file)
        info("Initialized from configuration file: [%s]" % init_file)
        if os.path.abspath(os.path.dirname(init_file)) != os.path.abspath(self.run_folder):
            copyfile(init_file, os.path.join(self.run_folder, os.path.basename(init_file)))
        if self.train and self.val:
            error("Cannot specify simultaneous training and validation run, for now.")
        if not (self.train or self.val):
            error("Neither training nor validation is enabled.")
        self.tensorboard_folder = os.path.join(self.run_folder, self.tensorboard_folder, self.phase)
        self.feeder.set_phase(self.phase)
        self.feeder.initialize_datasets()
        self.resolve_balanced_weights()
        if self.should_resume():
            if self.train:
                info("Resuming training.")
                self.train.epoch_index, self.global_step = self.feeder.resume_snap(self.resume_file)
            if self.val:
                info("Evaluating trained network.")
        else:
            info("Starting training from scratch." if self.train else "Starting validation-only run with an untrained network.")
        info("Starting run on folder [%s]." % self.run_folder)
        return self.feeder
