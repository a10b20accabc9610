"""float64 reference of the class-weighted focal loss (vl_softmax_xent_wf, NetConfig.class_weights / focal_gamma), the
closed form, in numpy.  With p = softmax(z), y' the float label matrix (tests/mixup_ref.py::targets: the mixup blend, then
tests/label_smoothing_ref.py's smoothing), w the class weights (None: ones) and m_c = (1 - p_c)^gamma:

    loss = sum_c w_c y'_c m_c (-log p_c)
    a_c  = w_c y'_c (m_c - gamma (1 - p_c)^(gamma - 1) p_c log p_c),   A = sum_c a_c,   dz_j = (p_j A - a_j) * grad_scale

log p_c = z_c - lse, 1 - p_c = -expm1(log p_c); the second term of a_c is 0 where 1 - p_c == 0 (its limit), so a saturated row is finite
at every gamma, where autograd of the loss line gives NaN for 0 < gamma < 1.  gamma == 0: m = 1 exactly and no power is taken.  The
normaliser is the live-row count, never sum w.  w and gamma are the float32 values the launch receives.  Hits and top-k hits: LS's rules,
unweighted, against each row's own labels."""
import contextlib

import numpy as np

from oracle import lrcn_oracle as O
from tests import label_smoothing_ref as LS
from tests import mixup_ref as MX

F64 = np.float64


def weights32(w, classes):
    """The class weights as float64 of their float32 values; None = ones."""
    return np.ones(classes, F64) if w is None else np.asarray(w, np.float32).astype(F64)


def row_terms(logits, target, w=None, gamma=0.0):
    """-> (row losses [rows], d loss_r / d z [rows, C], p) for a float label matrix `target`, unscaled."""
    z, y = np.asarray(logits, F64), np.asarray(target, F64)
    g = float(np.float32(gamma))
    wy = weights32(w, z.shape[1])[None, :] * y
    mx = z.max(axis=1, keepdims=True)
    lse = np.log(np.exp(z - mx).sum(axis=1, keepdims=True)) + mx
    lp = z - lse
    p, q = np.exp(lp), -np.expm1(lp)
    if g == 0.0:
        m, second = np.ones_like(q), np.zeros_like(q)
    else:
        m = q ** g
        with np.errstate(divide="ignore", invalid="ignore"):
            second = np.where(q > 0, g * q ** (g - 1.0) * p * lp, 0.0)
    a = wy * (m - second)
    return (wy * m * -lp).sum(axis=1), p * a.sum(axis=1, keepdims=True) - a, p


def xent_mean(logits, target, w=None, gamma=0.0):
    """O.softmax_xent_mean's contract for the weighted focal loss: (mean row loss, dlogits / rows) on a float label matrix."""
    l, d, _ = row_terms(logits, target, w, gamma)
    return float(l.mean()), d / len(l)


def xent(logits, onehot, w=None, gamma=0.0, eps=0.0, k=0, lam=1.0, rows_per_clip=1, live=None):
    """-> dict(row_losses (zeros in dead rows), loss_sum, loss (mean over the live rows), hits, topk, dlogits [rows, C] scaled by
    1 / live rows with zeros in dead rows, rows).  lam / rows_per_clip: the partner rows of MX.partner_rows (lam 1: none is read);
    live: the mask of a loss under seq_len (no mixing then)."""
    z, oh = np.asarray(logits), np.asarray(onehot)
    m = np.ones(len(z), bool) if live is None else np.asarray(live, bool)
    assert live is None or (lam32(lam) == 1.0 and rows_per_clip == 1)
    y = MX.targets(oh, lam, eps, rows_per_clip)
    n = int(m.sum())
    rl, dl = np.zeros(len(z), F64), np.zeros(z.shape, F64)
    rl[m], d, _ = row_terms(z[m], y[m], w, gamma)
    dl[m] = d / n
    hits = float(np.sum(np.argmax(z[m], 1) == LS.target(oh[m])))
    topk = float(np.sum(LS.topk_hits(z[m], oh[m], k))) if k > 0 else 0.0
    return dict(row_losses=rl, loss_sum=float(rl.sum()), loss=float(rl.sum()) / n, hits=hits, topk=topk, dlogits=dl, rows=n)


def lam32(lam):
    return MX.lam32(lam)


@contextlib.contextmanager
def oracle_loss(w=None, gamma=0.0):
    """Inside: the fp64 oracles (O.lrcn_train_step, the graph oracles of tests/seq_len_ref.py) take their loss and its dlogits from
    xent_mean on the float label matrix they are fed, so their backward runs on this file's dlogits.  The oracle is as it was after."""
    plain = O.softmax_xent_mean
    O.softmax_xent_mean = lambda logits, onehot, dtype=F64: xent_mean(logits, onehot, w, gamma)
    try:
        yield
    finally:
        O.softmax_xent_mean = plain
