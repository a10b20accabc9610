"""float64 reference of the multi-label loss launch (vl_sigmoid_xent, NetConfig.label_type "multiple"), the closed form, in
numpy, and a brute-force average precision.  Per element, z the logit, t the float label (the mixup blend of tests/mixup_ref.py's partner
rows, then the smoothing t (1 - eps) + eps / 2), q the positive-term weights (None: ones), g = gamma:

    log p = -(max(-z, 0) + sp),  log(1 - p) = -(max(z, 0) + sp),  sp = log1p(exp(-|z|))
    g == 0:  l = -(q t log p + (1 - t) log(1 - p)),                        dl/dz = p (q t + 1 - t) - q t
    g  > 0:  l = q t (1 - p)^g (-log p) + (1 - t) p^g (-log(1 - p)),       (1 - p)^g = exp(g log(1 - p)),  p^g = exp(g log p)
             dl/dz = q t (1 - p)^g (g p log p - (1 - p)) + (1 - t) p^g (p - g (1 - p) log(1 - p))

p = exp(log p) and 1 - p = exp(log(1 - p)): no subtraction from 1, no division, so z = +-120 is finite at every gamma.  The row loss is the
MEAN over the classes; dlogits = dl/dz / (live rows * C).  q, gamma, eps and lam are the float32 values the launch receives.  hit@1: the
first arg-max of the logits is a class with y > 0, the row's own labels; exact: (z > 0) == (y > 0) for every class."""
import contextlib

import numpy as np

from oracle import lrcn_oracle as O
from tests import mixup_ref as MX

F64 = np.float64


def weights32(q, classes):
    """The positive-term weights as float64 of their float32 values; None = ones."""
    return np.ones(classes, F64) if q is None else np.asarray(q, np.float32).astype(F64)


def targets(labels, lam=1.0, eps=0.0, rows_per_clip=1):
    """The float label matrix: lam y + (1 - lam) y_partner (MX.partner_rows), then t (1 - eps) + eps / 2."""
    y = np.asarray(labels, F64)
    l, e = MX.lam32(lam), float(np.float32(eps))
    t = y if l == 1.0 else l * y + (1.0 - l) * y[MX.partner_rows(len(y), rows_per_clip)]
    return t * (1.0 - e) + e / 2.0


def elem_terms(logits, target, q=None, gamma=0.0):
    """-> (l [rows, C], dl/dz [rows, C]) per element, unscaled."""
    z, t = np.asarray(logits, F64), np.asarray(target, F64)
    g = float(np.float32(gamma))
    qt, ut = weights32(q, z.shape[1])[None, :] * t, 1.0 - t
    sp = np.log1p(np.exp(-np.abs(z)))
    lp, lq = -(np.maximum(-z, 0.0) + sp), -(np.maximum(z, 0.0) + sp)
    p, np_ = np.exp(lp), np.exp(lq)
    if g == 0.0:
        return -(qt * lp + ut * lq), p * (qt + ut) - qt
    m1, m0 = np.exp(g * lq), np.exp(g * lp)
    return qt * m1 * -lp + ut * m0 * -lq, qt * m1 * (g * p * lp - np_) + ut * m0 * (p - g * np_ * lq)


def xent_mean(logits, target, q=None, gamma=0.0):
    """O.softmax_xent_mean's contract for the sigmoid loss on a float label matrix: (mean over the rows of the class-mean loss,
    its gradient = dl/dz / (rows * C))."""
    l, d = elem_terms(logits, target, q, gamma)
    return float(l.mean(axis=1).mean()), d / l.size


def hit1(logits, labels):
    z, y = np.asarray(logits), np.asarray(labels)
    return y[np.arange(len(z)), np.argmax(z, axis=1)] > 0


def exact(logits, labels):
    return np.all((np.asarray(logits) > 0) == (np.asarray(labels) > 0), axis=1)


def xent(logits, labels, q=None, gamma=0.0, eps=0.0, lam=1.0, rows_per_clip=1, live=None):
    """-> dict(row_losses (zeros in dead rows), loss_sum, loss (mean over the live rows), hits, exact, hit_rows, exact_rows, dlogits
    [rows, C] scaled by 1 / (live rows * C) with zeros in dead rows, rows).  live: the mask of a loss under seq_len (no mixing then)."""
    z, y = np.asarray(logits), np.asarray(labels)
    m = np.ones(len(z), bool) if live is None else np.asarray(live, bool)
    assert live is None or (MX.lam32(lam) == 1.0 and rows_per_clip == 1)
    t = targets(y, lam, eps, rows_per_clip)
    n = int(m.sum())
    rl, dl = np.zeros(len(z), F64), np.zeros(z.shape, F64)
    l, d = elem_terms(z[m], t[m], q, gamma)
    rl[m], dl[m] = l.mean(axis=1), d / (n * z.shape[1])
    hr, er = np.zeros(len(z), bool), np.zeros(len(z), bool)
    hr[m], er[m] = hit1(z[m], y[m]), exact(z[m], y[m])
    return dict(row_losses=rl, loss_sum=float(rl.sum()), loss=float(rl.sum()) / n, hits=float(hr.sum()), exact=float(er.sum()),
                hit_rows=hr, exact_rows=er, dlogits=dl, rows=n)


def average_precision_brute(scores, positives):
    """AP threshold by threshold over the distinct scores, descending: at threshold s the predictions are score >= s; sum of
    (R_n - R_{n-1}) P_n.  nan without a positive."""
    s, pos = np.asarray(scores, F64), np.asarray(positives) > 0
    total = int(pos.sum())
    if total == 0:
        return float("nan")
    ap, prev = 0.0, 0.0
    for thr in sorted(set(s.tolist()), reverse=True):
        pred = s >= thr
        tp = int((pred & pos).sum())
        ap += (tp / total - prev) * (tp / int(pred.sum()))
        prev = tp / total
    return ap


def metrics_brute(logits, labels):
    """val.multilabel_metrics by loops: ap per class, map, f1_micro, f1_macro, hit1, subset_accuracy."""
    z, pos = np.asarray(logits, F64), np.asarray(labels) > 0
    ap = np.array([average_precision_brute(z[:, c], pos[:, c]) for c in range(z.shape[1])])
    f1s, TP, FP, FN = [], 0, 0, 0
    for c in range(z.shape[1]):
        tp = int(((z[:, c] > 0) & pos[:, c]).sum())
        fp = int(((z[:, c] > 0) & ~pos[:, c]).sum())
        fn = int((~(z[:, c] > 0) & pos[:, c]).sum())
        TP, FP, FN = TP + tp, FP + fp, FN + fn
        if pos[:, c].any():
            f1s.append(2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0)
    present = pos.any(axis=0)
    return dict(ap=ap, map=float(np.mean(ap[present])), f1_micro=2 * TP / (2 * TP + FP + FN) if 2 * TP + FP + FN else 0.0,
                f1_macro=float(np.mean(f1s)), hit1=float(np.mean(hit1(z, pos))), subset_accuracy=float(np.mean(exact(z, pos))))


@contextlib.contextmanager
def oracle_loss(q=None, gamma=0.0):
    """Inside: the fp64 oracles (O.lrcn_train_step, the graph oracles of tests/seq_len_ref.py) take their loss and its dlogits from
    xent_mean on the float label matrix they are fed (targets(..)), so their backward runs on this file's dlogits.  The oracle is as it
    was after."""
    plain = O.softmax_xent_mean
    O.softmax_xent_mean = lambda logits, target, dtype=F64: xent_mean(logits, target, q, gamma)
    try:
        yield
    finally:
        O.softmax_xent_mean = plain
