"""Validation: clip -> video logit fusion, accuracy, pickled logits with the reference's file names
(val.py:59-203).  Host numpy; the logits come from LRCNEngine.forward_u8."""
import os
import pickle

import numpy as np

from .defs_ import defs
from .utils_ import debug, error, info


def topk_hits(logits, labels, k):
    """Per row: the label t (first arg-max of the label row) is among the k largest logits, ties going to the lower index:
    #{c : z_c > z_t} + #{c < t : z_c == z_t} < k -- the rule of the training loss launch (vl_softmax_xent_ls), the same set as
    t in np.argsort(-z, kind="stable")[:k].  k = 1 is the arg-max comparison of get_chunk_accuracy."""
    logits = np.asarray(logits)
    t = np.argmax(labels, axis=1)
    zt = logits[np.arange(len(logits)), t][:, None]
    before = np.arange(logits.shape[1])[None, :] < t[:, None]
    rank = np.sum(logits > zt, axis=1) + np.sum((logits == zt) & before, axis=1)
    return rank < int(k)


def average_precision(scores, positives):
    """sklearn's average_precision_score for one class: sum_n (R_n - R_{n-1}) P_n over the distinct score thresholds in descending
    order -- the rows of a tied score enter together and form ONE threshold.  nan without a positive."""
    scores, pos = np.asarray(scores, np.float64), np.asarray(positives) > 0
    total = int(pos.sum())
    if total == 0:
        return float("nan")
    order = np.argsort(-scores, kind="stable")
    s, hit = scores[order], pos[order]
    last = np.flatnonzero(np.append(s[1:] != s[:-1], True))      # the last row of every run of equal scores
    tp = np.cumsum(hit)[last].astype(np.float64)
    precision, recall = tp / (last + 1.0), tp / total
    return float(np.sum(np.diff(np.append(0.0, recall)) * precision))


def _f1(tp, fp, fn):
    """2 tp / (2 tp + fp + fn); an empty denominator counts as 0."""
    den = 2.0 * tp + fp + fn
    return float(2.0 * tp / den) if den > 0 else 0.0


def hit1_rows(logits, labels):
    """Per row: the first arg-max of the logits is a class the row carries (the loss launch's hit@1; a row without labels never hits)."""
    logits, labels = np.asarray(logits), np.asarray(labels)
    return labels[np.arange(len(logits)), np.argmax(logits, axis=1)] > 0 if len(logits) else np.zeros(0, bool)


def multilabel_metrics(logits, labels):
    """The metrics of a multi-label run (network.label_type multiple) over ALL rows at once.  logits, labels: [N, C], a
    label > 0 is a positive; the prediction of class c is z_c > 0 (p > 0.5; z == 0 predicts negative, as in the loss launch).
    -> dict: ap [C] (average_precision per class, nan for a class without a positive), positives [C], map (the mean AP over the
    classes with a positive; nan when there is none), f1_micro (tp, fp, fn summed over every class), f1_macro (the mean F1 over the
    classes with a positive; an F1 with an empty denominator counts as 0), hit1 (hit1_rows' mean) and subset_accuracy (the rows
    predicted exactly)."""
    logits, pos = np.asarray(logits, np.float64), np.asarray(labels) > 0
    if logits.ndim != 2 or logits.shape != pos.shape:
        error("multilabel_metrics: logits %s and labels %s are not two [N, C] arrays of one shape" % (logits.shape, pos.shape))
    n, classes = logits.shape
    ap = np.array([average_precision(logits[:, c], pos[:, c]) for c in range(classes)], np.float64).reshape(classes)
    positives = pos.sum(axis=0).astype(np.int64)
    present = positives > 0
    pred = logits > 0
    tp, fp, fn = (pred & pos).sum(axis=0), (pred & ~pos).sum(axis=0), (~pred & pos).sum(axis=0)
    f1 = np.array([_f1(tp[c], fp[c], fn[c]) for c in range(classes)], np.float64).reshape(classes)
    return {"ap": ap, "positives": positives,
            "map": float(np.mean(ap[present])) if present.any() else float("nan"),
            "f1_micro": _f1(tp.sum(), fp.sum(), fn.sum()),
            "f1_macro": float(np.mean(f1[present])) if present.any() else 0.0,
            "hit1": float(np.mean(hit1_rows(logits, pos))) if n else 0.0,
            "subset_accuracy": float(np.mean(np.all(pred == pos, axis=1))) if n else 0.0}


class Validation:
    def __init__(self, settings):
        self.multilabel = getattr(settings, "label_type", defs.label_type.single) == defs.label_type.multiple
        self.item_logits = np.zeros([0, settings.num_classes], np.float32)
        self.item_labels = np.zeros([0, settings.num_classes], np.float32)
        self.save_counter = 0
        self.save_interval = settings.val.logits_save_interval
        self.run_folder, self.run_id, self.timestamp = settings.run_folder, settings.run_id, settings.timestamp

    def apply_clip_fusion(self, clips_logits, cpv, video_labels, clip_fusion):
        """val.py:158-167."""
        cur = clips_logits[0:cpv, :]
        if clip_fusion == defs.fusion_method.avg:
            video_logits = np.mean(cur, axis=0)
        elif clip_fusion == defs.fusion_method.last:
            video_logits = cur[-1, :]
        else:
            error("Undefined clip fusion [%s]" % clip_fusion)
        self.item_logits = np.vstack((self.item_logits, video_logits))
        self.item_labels = np.vstack((self.item_labels, video_labels[0, :]))

    def process_validation_logits(self, dataset, settings, logits, labels, batch_index=None):
        """val.py:59-113, video batch mode (the only working one in the reference).  batch_index: the dataset's batch index right
        after THIS batch was read (the reference reads dataset.batch_index here; with a read-ahead feeder that has moved on)."""
        maxvid = (dataset.batch_index if batch_index is None else batch_index) * dataset.batch_size
        for vidx in range(maxvid - dataset.batch_size, maxvid):
            if vidx >= dataset.num_items:
                break
            cpv = dataset.clips_per_video[vidx]
            self.apply_clip_fusion(logits, cpv, labels, settings.val.clip_fusion_method)
            logits, labels = logits[cpv:, :], labels[cpv:, :]
        if len(logits) or len(labels):
            error("Logits and/or labels non empty at the end of video item mode aggregation!")
        info("Incremental accuracy up to current batch: %2.3f" % np.mean(self.get_chunk_accuracy(self.item_logits, self.item_labels)))

    def add_items(self, logits, labels):
        """Logit rows that are items of their own (per-step logits of a `reshape`-fusion model: no clip -> video fusion)."""
        self.item_logits = np.vstack((self.item_logits, np.asarray(logits, np.float32)))
        self.item_labels = np.vstack((self.item_labels, np.asarray(labels, np.float32)))
        info("Incremental accuracy up to current batch: %2.3f" % np.mean(self.get_chunk_accuracy(self.item_logits, self.item_labels)))

    def save_validation_logits_chunk(self, save_all=False):
        """val.py:115-148: '<run_folder>/validation_logits_<run_id>_<ts>.total' or '.part_k'."""
        if self.save_interval is None or len(self.item_logits) == 0:
            return
        if self.save_interval <= 0:
            if save_all:
                path = os.path.join(self.run_folder, "validation_logits_%s_%s.total" % (self.run_id, self.timestamp))
                info("Saving all %d extracted validation logits to %s" % (len(self.item_logits), path))
                with open(path, "wb") as f:
                    pickle.dump(self.item_logits, f)
            return
        if len(self.item_logits) >= self.save_interval or save_all:
            path = os.path.join(self.run_folder, "validation_logits_%s_%s.part_%d" % (self.run_id, self.timestamp, self.save_counter))
            info("Saving a %d-sized chunk of validation logits to %s" % (len(self.item_logits), path))
            with open(path, "wb") as f:
                pickle.dump(self.item_logits, f)
            self.item_logits = np.zeros([0, self.item_logits.shape[-1]], np.float32)
            self.save_counter += 1

    def load_validation_logits_chunk(self, idx):
        path = os.path.join(self.run_folder, "validation_logits_%s_%s.part_%d" % (self.run_id, self.timestamp, idx))
        with open(path, "rb") as f:
            return pickle.load(f)          # a file this code wrote

    def get_accuracy(self):
        """val.py:174-197: mean of per-chunk accuracies."""
        accuracies, cur = [], 0
        for k in range(self.save_counter):
            logits = self.load_validation_logits_chunk(k)
            accuracies.append(self.get_chunk_accuracy(logits, self.item_labels[cur:cur + len(logits), :]))
            cur += len(logits)
        if len(self.item_logits) > 0:
            n = len(self.item_logits)
            accuracies.append(self.get_chunk_accuracy(self.item_logits, self.item_labels[cur:cur + n, :]))
        return float(np.mean(accuracies))

    def get_topk_accuracy(self, k):
        """get_accuracy with topk_hits(.., k) in place of the arg-max comparison: the same chunks, the same mean of per-chunk means."""
        accuracies, cur = [], 0
        for c in range(self.save_counter):
            logits = self.load_validation_logits_chunk(c)
            accuracies.append(np.mean(topk_hits(logits, self.item_labels[cur:cur + len(logits), :], k)))
            cur += len(logits)
        if len(self.item_logits) > 0:
            n = len(self.item_logits)
            accuracies.append(np.mean(topk_hits(self.item_logits, self.item_labels[cur:cur + n, :], k)))
        return float(np.mean(accuracies))

    def get_per_class(self):
        """val.per_class: -> (mean-class accuracy, hits [classes], items [classes]) over the fused per-video logits of every saved
        chunk and the rows still in memory.  An item counts under the first arg-max of its label row (the rule of topk_hits, so a
        multi-hot item has one class); hits and items are SUMMED over the chunks -- a chunk may hold no item of a class, so there is
        no mean of chunk means here.  A class's recall is hits / items; the mean-class accuracy is the mean recall over the classes
        that have at least one item."""
        classes = self.item_labels.shape[1]
        hits, items = np.zeros(classes, np.int64), np.zeros(classes, np.int64)
        chunks, cur = [], 0
        for c in range(self.save_counter):
            chunks.append(self.load_validation_logits_chunk(c))
        if len(self.item_logits) > 0:
            chunks.append(self.item_logits)
        for logits in chunks:
            t = np.argmax(self.item_labels[cur:cur + len(logits), :], axis=1)
            cur += len(logits)
            items += np.bincount(t, minlength=classes)
            hits += np.bincount(t[np.argmax(logits, axis=1) == t], minlength=classes)
        present = items > 0
        if not present.any():
            error("val.per_class: there are no validation items")
        return float(np.mean(hits[present] / items[present])), hits, items

    def report_per_class(self, write=True):
        """get_per_class logged -- the mean-class accuracy and the three classes of lowest recall -- and, with write, stored beside the
        accuracy file: accuracy_mean_class_<run_id> (the number) and accuracy_per_class_<run_id>, one line `class hits items recall`
        per class (a class without items has recall nan).  -> the mean-class accuracy."""
        mean_class, hits, items = self.get_per_class()
        recall = np.where(items > 0, hits / np.maximum(items, 1), np.nan)
        present = np.flatnonzero(items > 0)
        worst = present[np.argsort(recall[present], kind="stable")[:3]]
        info("Validation mean-class accuracy: %2.5f over %d of %d classes with items; lowest recall: %s" %
             (mean_class, len(present), len(items), ", ".join("class %d %d/%d" % (c, hits[c], items[c]) for c in worst)))
        if write:
            with open(os.path.join(self.run_folder, "accuracy_mean_class_" + self.run_id), "w") as f:
                f.write(str(mean_class))
            with open(os.path.join(self.run_folder, "accuracy_per_class_" + self.run_id), "w") as f:
                for c in range(len(items)):
                    f.write("%d %d %d %s\n" % (c, hits[c], items[c], repr(float(recall[c]))))
        return mean_class

    def get_multilabel(self):
        """multilabel_metrics over the fused per-video logits of every saved chunk and the rows still in memory, CONCATENATED as
        get_per_class walks them: AP ranks all items of a class against each other, so there is no mean of chunk means here."""
        chunks = [self.load_validation_logits_chunk(c) for c in range(self.save_counter)]
        if len(self.item_logits) > 0:
            chunks.append(self.item_logits)
        if not chunks:
            error("multilabel validation: there are no validation items")
        logits = np.concatenate(chunks)
        return multilabel_metrics(logits, self.item_labels[:len(logits), :])

    def report_multilabel(self, write=True):
        """get_multilabel logged and, with write, stored beside the accuracy file: map_<run_id>, f1_micro_<run_id>, f1_macro_<run_id>,
        subset_accuracy_<run_id> (a number each) and ap_per_class_<run_id>, one line `class positives ap` per class (a class
        without a positive has ap nan).  -> the metrics."""
        m = self.get_multilabel()
        present = np.flatnonzero(m["positives"] > 0)
        worst = present[np.argsort(m["ap"][present], kind="stable")[:3]]
        info("Validation mAP: %2.5f over %d of %d classes with positives, micro-F1 %2.5f, macro-F1 %2.5f, hit@1 %2.5f, subset accuracy "
             "%2.5f; lowest AP: %s" % (m["map"], len(present), len(m["ap"]), m["f1_micro"], m["f1_macro"], m["hit1"],
                                        m["subset_accuracy"], ", ".join("class %d %.4f" % (c, m["ap"][c]) for c in worst)))
        if write:
            for name in ("map", "f1_micro", "f1_macro", "subset_accuracy"):
                with open(os.path.join(self.run_folder, "%s_%s" % (name, self.run_id)), "w") as f:
                    f.write(str(m[name]))
            with open(os.path.join(self.run_folder, "ap_per_class_" + self.run_id), "w") as f:
                for c in range(len(m["ap"])):
                    f.write("%d %d %s\n" % (c, m["positives"][c], repr(float(m["ap"][c]))))
        return m

    def get_chunk_accuracy(self, logits, labels):
        if getattr(self, "multilabel", False):    # label_type multiple: hit@1 -- the arg-max of the logits is a class the item carries
            return np.mean(hit1_rows(logits, labels))
        return np.mean(np.equal(np.argmax(logits, axis=1), np.argmax(labels, axis=1)))
