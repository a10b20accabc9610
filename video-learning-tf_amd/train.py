"""Train: learning-rate table and the per-step call with the reference's surface (train.py:50-149, 199-222)."""
import json
import math
import os

import numpy as np
import torch

from .defs_ import defs
from .engine import ema_extra_bytes
from .utils_ import error, info, warning


def precompute_learning_rates(settings, num_batches):
    """train.py:50-109, including the schedule dump to <run_id>_lr_decay_schedule.txt.  Because idx advances by
    decay_freq per block, exp and staircase give the same piecewise-constant table."""
    base_lr, decay_params = settings.train.base_lr, settings.train.lr_decay
    total = num_batches * settings.train.epochs
    if decay_params is None:
        return [base_lr] * total
    offset = 0 if len(tuple(decay_params)) == 4 else decay_params[-1]
    strategy, scheme, freq, factor = tuple(decay_params[:4])
    if strategy not in (defs.decay.exp, defs.decay.staircase):
        error("Undefined decay strategy %s" % strategy)
    staircase = strategy == defs.decay.staircase
    if scheme == defs.periodicity.interval:
        period = freq
    elif scheme == defs.periodicity.drops:
        period = math.ceil(total / freq)
    else:
        error("Undefined decay scheme %s" % scheme)
    lrs, idx = [], 0
    while len(lrs) < total:
        fraction = idx // freq if staircase else idx / freq
        lrs.extend([base_lr * pow(factor, fraction)] * period)
        idx += freq
    lrs = lrs[:total]
    if offset:
        lrs = [base_lr] * offset + lrs[0:-offset]
    path = os.path.join(settings.run_folder, settings.run_id + "_lr_decay_schedule.txt")
    with open(path, "w") as f:
        k = 0
        for ep in range(settings.train.epochs):
            for b in range(num_batches):
                f.write("Epoch %d/%d, batch %d/%d, lr %2.8f\n" % (ep + 1, settings.train.epochs, b + 1, num_batches, lrs[k]))
                k += 1
    info("Dropping LR of %2.5f, mid / last lr is: %1.5f, %1.5f, total drops: %d" % (base_lr, lrs[len(lrs) // 2], lrs[-1], len(set(lrs))))
    return lrs


def accumulate_groups(num_batches, k, start_batch=0):
    """[(first, last)] batch indices of an epoch, inclusive: the groups of k consecutive batches that make one update each, from
    start_batch on.  Groups never span epochs, so the last one may be short.  start_batch must be where a group begins (checkpoints are
    written at group ends only, so a resume lands there); num_batches itself (a finished epoch) gives no group."""
    if k < 1 or num_batches < 0 or not (0 <= start_batch <= num_batches):
        raise ValueError("accumulate_groups(%r, %r, %r): need k >= 1 and 0 <= start_batch <= num_batches" % (num_batches, k, start_batch))
    if start_batch % k and start_batch != num_batches:
        raise ValueError("batch %d does not begin a group of %d batches: a run with accumulate %d resumes at a multiple of %d only" %
                         (start_batch, k, k, k))
    return [(first, min(first + k, num_batches) - 1) for first in range(start_batch, num_batches, k)]


def json_safe(v):
    """v with every non-finite float replaced by the string "nan" / "inf" / "-inf", so that json.dumps(.., allow_nan=False) takes it."""
    if isinstance(v, dict):
        return {k: json_safe(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [json_safe(x) for x in v]
    if isinstance(v, (float, np.floating)):
        v = float(v)
        return v if math.isfinite(v) else ("nan" if v != v else "inf" if v > 0 else "-inf")
    if isinstance(v, np.integer):
        return int(v)
    return v


def tensor_stats_lines(stats):
    """(info line, warning line or None) for one stats step: the variables with the largest and the smallest sgd_update_ratio, and
    the variables that hold NaN / Inf in their gradient or their weights."""
    rated = [(d["sgd_update_ratio"], n) for n, d in stats.items() if d["sgd_update_ratio"] is not None and math.isfinite(d["sgd_update_ratio"])]
    line = "Tensor statistics over %d variables: no update-to-weight ratio is defined" % len(stats)
    if rated:
        hi, lo = max(rated), min(rated)
        line = "Tensor statistics over %d variables: update / weight norm largest %.3e [%s], smallest %.3e [%s]" % (
            len(stats), hi[0], hi[1], lo[0], lo[1])
    bad = ["%s (gradient %d, weights %d)" % (n, d["grad_nonfinite"], d["weight_nonfinite"]) for n, d in stats.items()
           if d["grad_nonfinite"] > 0 or d["weight_nonfinite"] > 0]
    return line, ("Non-finite elements in: " + ", ".join(bad)) if bad else None


class TensorStatsLog:
    """<run_folder>/<run_id>_tensor_stats.jsonl: one strict-JSON line per stats step, appended (a resumed run goes on in the file it
    finds).  Rank 0 owns the file like the run's log; the other ranks write nothing."""

    def __init__(self, run_folder, run_id, rank=0):
        self.path = os.path.join(run_folder, run_id + "_tensor_stats.jsonl") if rank == 0 else None

    def write(self, global_step, update, lr, clip_norm, out):
        """out: the result of a stats step (it holds tensor_stats).  Returns the record, or None on a rank that does not write."""
        if self.path is None:
            return None
        from .engine import clip_scale_of
        rec = {"global_step": int(global_step), "update": int(update), "lr": float(lr),
               "clip_scale": clip_scale_of(out["grad_norm"] ** 2, clip_norm), "grad_norm": out["grad_norm"],
               "grads_norm_mean": out["grads_norm_mean"], "vars": out["tensor_stats"]}
        with open(self.path, "a") as f:
            f.write(json.dumps(json_safe(rec), allow_nan=False) + "\n")
        return rec


def dp_scalars(out):
    """The per-rank sums a data-parallel step adds over the ranks (dp.sum_scalars): loss sum, hits, rows -- and the top-k hits as a
    fourth only when the engine counts them (train.top_k), so that a run without them exchanges the vector it always did.  The
    exact-match rows of a multi-label run (label_type multiple, which refuses top_k) travel the same way, after them."""
    v = [out["loss_sum"], out["correct"], float(out["rows"])]
    if "topk_correct" in out:
        v.append(out["topk_correct"])
    if "subset_correct" in out:
        v.append(out["subset_correct"])
    return v


def dp_global(out, tot):
    """out with loss / accuracy (/ topk_accuracy / subset_accuracy) of the GLOBAL batch, from the summed dp_scalars vector."""
    g = dict(out, loss=float(tot[0] / max(tot[2], 1)), accuracy=float(tot[1] / max(tot[2], 1)))
    i = 3
    if "topk_correct" in out:
        g["topk_accuracy"] = float(tot[i] / max(tot[2], 1))
        i += 1
    if "subset_correct" in out:
        g["subset_accuracy"] = float(tot[i] / max(tot[2], 1))
    return g


class Train:
    """train.py:112-149: owns the LR table and global_step; run_step is the train sess.run.
    train.accumulate k > 1: the batches of an epoch go to the engine in groups (accumulate_groups) as the micro-steps of one update.
    global_step, the learning-rate table and the checkpoint names keep counting BATCHES; the update takes the lr of its last batch."""

    def __init__(self, settings, feeder, engine):
        self.engine = engine
        self.learning_rates = precompute_learning_rates(settings, feeder.get_num_batches())
        self.global_step = settings.global_step
        self.clip_norm = float(settings.train.clip_norm or 0)
        self.accumulate = int(getattr(settings.train, "accumulate", 1) or 1)
        self._group, self._group_clips = None, 0
        self.group_done = True                  # the last run_step closed an update: a checkpoint may be written
        # per-variable statistics (logging.tensor_stats_interval): intervals count UPDATES (the engine's step_count), the line carries the
        # workflow's global_step, which counts batches
        self.stats_log = None
        if getattr(engine, "tensor_stats_interval", 0) > 0:
            self.stats_log = TensorStatsLog(settings.run_folder, settings.run_id, int(os.environ.get("RANK", "0")))
        if getattr(engine, "ema", None) is not None:
            info("Averaging the trained weights: decay %s, warm-up %s (rate max(1 - decay, 9 / (10 + updates)) if on), +%.1f MB of device memory "
                 "for the shadow; validate it with val.use_ema" %
                 (engine.ema_decay, "on" if engine.ema_warmup else "off", ema_extra_bytes(engine.ema.numel()) / 1e6))
        if getattr(engine, "lars", None) is not None:
            info("LARS on the momentum update: eeta %s, epsilon %s; %d weight tensors get a trust ratio, the biases learn with the plain rate" %
                 (engine.lars_eeta, engine.lars_epsilon, len(engine.lars["segs"])))
        if getattr(engine, "lamb", None) is not None:
            info("LAMB on the Adam update: epsilon %s, decoupled weight decay %s; %d weight tensors get a trust ratio |w| / |u|, the biases "
                 "learn with the plain rate and no decay" % (engine.lamb_epsilon, engine.weight_decay, len(engine.lamb["segs"])))
        if getattr(engine, "xent_ls", False) and not getattr(engine, "multilabel", False):
            info("Loss: label smoothing %s (labels y (1 - eps) + eps / %d; the logged loss is the smoothed one), top-k accuracy %s" %
                 (engine.label_smoothing, settings.num_classes, ("k = %d" % engine.top_k) if engine.top_k > 0 else "off"))
        if getattr(engine, "multilabel", False):
            w = engine.class_weights
            info("Loss: label_type multiple -- sigmoid cross-entropy per class, the row loss the mean over the %d classes (gradients are "
                 "%d times smaller than a softmax row's); smoothing %s (labels t (1 - eps) + eps / 2), focal gamma %s, positive-term "
                 "weights %s; accuracy is hit@1, subset accuracy the rows predicted exactly" %
                 (settings.num_classes, settings.num_classes, engine.label_smoothing, engine.focal_gamma,
                  "off" if w is None else "min %g (class %d), max %g (class %d)" % (w.min(), int(w.argmin()), w.max(), int(w.argmax()))))
        elif getattr(engine, "xent_wf", False):
            w = engine.class_weights
            info("Loss: focal gamma %s, class weights %s; rows are normalised by their count, not by their weights, and the logged loss is "
                 "the weighted one" % (engine.focal_gamma, "off" if w is None else "min %g (class %d), max %g (class %d)" %
                                       (w.min(), int(w.argmin()), w.max(), int(w.argmax()))))

        if getattr(engine, "mix_lam", None) is not None:
            info("Mixup: alpha %s, seed %d (one Beta(alpha, alpha) weight per batch, folded to max(lam, 1 - lam)); clip i is blended with "
                 "clip B - 1 - i inside a rank's batch, and the logged loss is the one on the mixed labels" %
                 (engine.mixup_alpha, engine.mixup_seed))

        if getattr(engine, "cut_box", None) is not None:
            info("CutMix: alpha %s, seed %d, mode %s (one box per batch, at most half the clip); inside a rank's batch clip i and clip "
                 "B - 1 - i exchange the box, the label weight is 1 - volume / clip volume%s" %
                 (engine.cutmix_alpha, engine.cutmix_seed, engine.cutmix_mode,
                  ("; with mixup on a batch is cut with probability %s, else blended" % engine.cutmix_prob)
                  if engine.blend_lam is not None else ""))

        if getattr(engine, "erase", None) is not None:
            e = engine.erase
            info("Random erasing: prob %s, scale %s, ratio %s, frames %s, mode %s%s, seed %d; every clip of a batch draws a box of its own "
                 "(or none), overwritten after the feed and ahead of mixup / CutMix; the labels stay as they are" %
                 (e.prob, tuple(e.scale), tuple(e.ratio), tuple(e.frames), e.mode, "" if e.mode == "zero" else " (std %s)" % e.std, e.seed))

    def _stats_step(self, out, lr):
        """After a step: a stats step's result goes to the JSONL file and to the log."""
        if self.stats_log is None or "tensor_stats" not in out:
            return
        self.stats_log.write(self.global_step, self.engine.step_count - 1, lr, self.clip_norm, out)
        line, bad = tensor_stats_lines(out["tensor_stats"])
        info(line)
        if bad:
            warning(bad)

    def _micro(self, fdict):
        """-> (micro, clips of the whole group over all ranks) of the batch in fdict; (None, None) without accumulation.  The group's
        clips come from the dataset's batch list before its first step, so a short last batch inside a group still gives the exact
        mean over the group."""
        if self.accumulate == 1:
            return None, None
        d = fdict["dataset"]
        pos = fdict["batch_index"] - 1           # (the dataset's index has already moved past this batch)
        if self._group is None or not (self._group[0] <= pos <= self._group[1]):
            try:
                self._group = accumulate_groups(len(d.batches), self.accumulate, pos)[0]
            except (ValueError, IndexError) as ex:
                error("train.accumulate: %s" % ex)
            first, last = self._group
            self._group_clips = sum(d.clips_per_video[first * d.batch_size:(last + 1) * d.batch_size])
        first, last = self._group
        self.group_done = pos == last
        return (pos - first, last - first + 1), self._group_clips

    def run_step(self, fdict, others=None):
        """-> (loss, current_lr, global_step) like sess.run([.., loss, current_lr, global_step, optimizer]).
        others: {tag: batch} of the other datasets of a multi-pipeline model (fdict is the MAIN dataset's: the labels are its, train.py:117)."""
        if others is not None:
            return self.run_step_graph(fdict, others)
        if self.global_step >= len(self.learning_rates):
            error("global step %d exceeds the precomputed learning-rate table (%d)" % (self.global_step, len(self.learning_rates)))
        lr = float(self.learning_rates[self.global_step])
        dev = self.engine.dev
        eng, dpg = self.engine, self.engine.dp
        # data parallel: the loss is the mean over the GLOBAL batch, of which this rank holds a shard (possibly ragged or empty)
        per_clip = eng.cfg.classifier == "lstm" or eng.early or eng.late          # one logits row per clip
        grows = None
        if dpg is not None and fdict.get("global_clips") is not None:
            # per-frame head (classifier fc, no frame fusion): one logits row per frame -> global rows = global clips * fpc
            grows = fdict["global_clips"] * (1 if per_clip else eng.cfg.fpc)
        micro, group_clips = self._micro(fdict)
        kw = {}
        if micro is not None:                    # the loss is the mean over the rows of the whole update, on every one of its calls
            grows = group_clips * (1 if per_clip else eng.cfg.fpc)
            kw = dict(micro=micro)
        if len(fdict["labels"]) == 0:
            out = eng.train_step_empty(lr, self.clip_norm, **kw)
        elif "device" in fdict:          # uploaded ahead of time by the feeder's BatchPrefetcher: wait for the copy on the stream
            torch.cuda.current_stream(dev).wait_event(fdict["ready"])
            t = fdict["device"]
            if t.get("crop_box") is not None:    # imgproc rand_resized_crop: a box per frame in the place of the crop offsets
                kw["crop_box"] = t["crop_box"]
            out = eng.train_step_u8(t["frames_u8"], t["labels"], lr, self.clip_norm, fdict["mean_bgr"], t["crop_y"], t["crop_x"],
                                    t["mirror"], global_rows=grows, resize=fdict.get("resize"), **kw)
        else:
            up = lambda a: None if a is None else torch.from_numpy(a).to(dev)
            if fdict.get("crop_box") is not None:    # imgproc rand_resized_crop: a box per frame in the place of the crop offsets
                kw["crop_box"] = up(fdict["crop_box"])
            out = eng.train_step_u8(torch.from_numpy(fdict["frames_u8"]).to(dev, non_blocking=True),
                                    torch.from_numpy(fdict["labels"]).to(dev),
                                    lr, self.clip_norm, fdict["mean_bgr"], up(fdict["crop_y"]), up(fdict["crop_x"]),
                                    up(fdict["mirror"]), global_rows=grows, resize=fdict.get("resize"), **kw)
        if dpg is not None:              # log the global-batch loss, not the shard's
            tot = dpg.sum_scalars(torch.tensor(dp_scalars(out), device=dev, dtype=torch.float64))
            out = dp_global(out, tot.cpu().numpy())
        self.global_step += 1
        self.last = out
        self._stats_step(out, lr)
        return out["loss"], lr, self.global_step

    def run_step_graph(self, fdict, others):
        """Multi-pipeline model (vltf_amd.graph): one batch per dataset tag; a per-step model (the last pipeline an LSTM with
        fusion reshape) takes the main dataset's per-record targets, any other its per-clip ones."""
        from .defs_ import defs
        from .run_task import graph_feeds
        if self.global_step >= len(self.learning_rates):
            error("global step %d exceeds the precomputed learning-rate table (%d)" % (self.global_step, len(self.learning_rates)))
        lr = float(self.learning_rates[self.global_step])
        eng, dev = self.engine, self.engine.dev
        labels = fdict["record_labels"] if (eng.per_step and "record_labels" in fdict) else fdict["labels"]
        grows = None
        if eng.dp is not None and fdict.get("global_clips") is not None and len(fdict["labels"]):
            # rows of the GLOBAL batch: the main dataset's global clips times this model's logits rows per main clip
            grows = fdict["global_clips"] * len(labels) // len(fdict["labels"])
        micro, group_clips = self._micro(fdict)
        kw = {}
        if micro is not None:
            kw = dict(micro=micro)
            if len(fdict["labels"]):
                grows = group_clips * len(labels) // len(fdict["labels"])
        if len(labels) == 0:                 # this rank's shard of a short last batch is empty
            out = eng.train_step_empty(lr, self.clip_norm, **kw)
        else:
            fdicts = dict(others)
            fdicts[defs.dataset_tag.main] = fdict
            out = eng.train_step(graph_feeds(fdicts, sorted(fdicts), dev), torch.from_numpy(np.ascontiguousarray(labels)).to(dev), lr,
                                 self.clip_norm, global_rows=grows, **kw)
        if eng.dp is not None:
            tot = eng.dp.sum_scalars(torch.tensor(dp_scalars(out), device=dev, dtype=torch.float64))
            out = dp_global(out, tot.cpu().numpy())
        self.global_step += 1
        self.last = out
        self._stats_step(out, lr)
        return out["loss"], lr, self.global_step
