"""float64 reference of mixup (vl_mixup_pairs, vl_softmax_xent_mix, NetConfig.mixup_alpha), built on tests/label_smoothing_ref.py: the
blend of clip i with clip B - 1 - i, the bf16 round-to-nearest-even of the packed path, and the loss on the mixed labels -- a float label
matrix, which O.softmax_xent_mean and O.lrcn_train_step take as they take the smoothed one.  lam is the float32 the launch receives;
1 - lam is formed in float64 (for lam in [0.5, 1] the float32 difference is exact)."""
import numpy as np

from oracle import lrcn_oracle as O
from tests import label_smoothing_ref as LS

F64 = np.float64


def lam32(lam):
    return float(np.float32(lam))


def partner_rows(rows, rows_per_clip=1):
    """Index of every row's partner: row r % rows_per_clip of clip clips - 1 - r // rows_per_clip."""
    assert rows % rows_per_clip == 0
    r = np.arange(rows)
    return (rows // rows_per_clip - 1 - r // rows_per_clip) * rows_per_clip + r % rows_per_clip


def blend(x, lam):
    """x [clips, ...] -> lam x_i + (1 - lam) x_{clips - 1 - i} in float64.  The middle clip of an odd count is its own partner; it comes
    back as it went in, also in this formula's rounding (lam x + (1 - lam) x), so it is copied."""
    x = np.asarray(x, F64)
    l = lam32(lam)
    out = l * x + (1.0 - l) * x[::-1]
    if len(x) % 2:
        out[len(x) // 2] = x[len(x) // 2]
    return out


def bf16_bits(x):
    """float -> the uint16 of the nearest bfloat16, ties to even (finite values)."""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff).astype(np.uint16)


def bf16_value(bits):
    """uint16 bfloat16 patterns -> float64."""
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(F64)


def bf16_round(x):
    """The nearest bfloat16 of float32(x) as float64 (the double rounding is what it is: callers compare within ulp bounds)."""
    return bf16_value(bf16_bits(x))


def bf16_ulp(x):
    """The spacing of bfloat16 (8 significant bits) at |x|: 2^(floor(log2 |x|) - 7); that of the smallest normal below it."""
    a = np.maximum(np.abs(np.asarray(x, F64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 7)


def mix_labels(onehot, lam, rows_per_clip=1):
    """y' = lam y_r + (1 - lam) y_partner(r) in float64."""
    y = np.asarray(onehot, F64)
    l = lam32(lam)
    return l * y + (1.0 - l) * y[partner_rows(len(y), rows_per_clip)]


def targets(onehot, lam, eps, rows_per_clip=1):
    """The float label matrix the loss is taken on: the mixed labels, then LS.smooth's y (1 - eps) + eps / C."""
    y = mix_labels(onehot, lam, rows_per_clip)
    e = float(np.float32(eps))
    return y * (1.0 - e) + e / y.shape[1]


def row_losses(logits, target):
    """sum_c target_c (lse - z_c) per row, float64."""
    z = np.asarray(logits, F64)
    m = z.max(axis=1, keepdims=True)
    lse = np.log(np.exp(z - m).sum(axis=1, keepdims=True)) + m
    return (np.asarray(target, F64) * (lse - z)).sum(axis=1)


def xent(logits, onehot, lam, eps, k, rows_per_clip=1):
    """-> dict(loss_sum, loss, hits, topk, dlogits scaled by 1 / rows).  Hits and top-k hits against each row's OWN label (LS's rules)."""
    z = np.asarray(logits)
    loss, dl = O.softmax_xent_mean(z, targets(onehot, lam, eps, rows_per_clip))
    hits = float(np.sum(np.argmax(z, 1) == LS.target(onehot)))
    topk = float(np.sum(LS.topk_hits(z, onehot, k))) if k > 0 else 0.0
    return dict(loss_sum=loss * len(z), loss=loss, hits=hits, topk=topk, dlogits=dl, rows=len(z))
