"""float64 reference of label smoothing and top-k accuracy (vl_softmax_xent_ls, NetConfig.label_smoothing / top_k), built on the
existing oracle: the smoothed labels y' = y (1 - eps) + eps / C are a float label matrix, and O.softmax_xent_mean, O.lrcn_train_step
and the graph oracles take any float label matrix.  eps is the float32 the launch receives.  The top-k rule is the stable argsort."""
import numpy as np

from oracle import lrcn_oracle as O

F64 = np.float64


def smooth(onehot, eps):
    """y' in float64 from the fp32-rounded eps; C is the row width."""
    y = np.asarray(onehot, F64)
    e = float(np.float32(eps))
    return y * (1.0 - e) + e / y.shape[1]


def target(onehot):
    """First arg-max of every label row."""
    return np.argmax(np.asarray(onehot), axis=1)


def topk_hits(logits, onehot, k):
    """Boolean per row: the target is among the first k of the stable descending sort of the row."""
    z, t = np.asarray(logits), target(onehot)
    return np.array([t[r] in np.argsort(-z[r], kind="stable")[:k] for r in range(len(z))], bool)


def rank(logits, onehot):
    """#{c : z_c > z_t} + #{c < t : z_c == z_t} per row: the rule the kernel and val.topk_hits are written in."""
    z, t = np.asarray(logits), target(onehot)
    out = np.zeros(len(z), np.int64)
    for r in range(len(z)):
        zt = z[r, t[r]]
        out[r] = int(np.sum(z[r] > zt)) + int(np.sum(z[r, :t[r]] == zt))
    return out


def xent(logits, onehot, eps, k, live=None):
    """-> dict(loss_sum, loss (mean over the live rows), hits, topk, dlogits [rows, C] scaled by 1 / live rows, zeros in dead rows)."""
    z = np.asarray(logits)
    m = np.ones(len(z), bool) if live is None else np.asarray(live, bool)
    loss, dl = O.softmax_xent_mean(z[m], smooth(np.asarray(onehot)[m], eps))
    full = np.zeros(z.shape, F64)
    full[m] = dl
    n = int(m.sum())
    hits = float(np.sum(np.argmax(z[m], 1) == target(np.asarray(onehot)[m])))
    topk = float(np.sum(topk_hits(z[m], np.asarray(onehot)[m], k))) if k > 0 else 0.0
    return dict(loss_sum=loss * n, loss=loss, hits=hits, topk=topk, dlogits=full, rows=n)
