"""LAMB restated in numpy for the tests (You et al. 2019; tfa.optimizers.LAMB): the element rule step by step in float32,
the trust ratio in float64 and the range table of the update.  Nothing here imports the package: the engine's own functions are checked
AGAINST these.

Rounding.  mul, sqrt, add and div are single correctly rounded float32 operations here (numpy) as on the device, so those steps agree
bit for bit.  The fused multiply-adds are formed as float32(float64 product + addend): the product of two float32 values is exact in
float64, the sum is rounded to float64 and then to float32 -- a double rounding that can differ from the device's fmaf by one unit in
the last place of the result, and by nothing else."""
import numpy as np

f32 = np.float32
B1, B2 = f32(0.9), f32(0.999)
A1, A2 = f32(0.1), f32(0.001)
ULP = 2.0 ** -23                 # one unit in the last place of a normal float32, relative to its magnitude, at most


def fma_ref(a, b, c):
    """float32(a * b + c) with the product and the sum in float64 (tests/test_weight_decay_gpu.py::fma_ref)."""
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
            + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


def clip_scale_f32(clip_norm, sumsq, gscale=1.0):
    """tests/lars_ref.py::clip_scale_f32: the clip scale the update launches form, step for step in float32."""
    if not clip_norm or clip_norm <= 0.0:
        return f32(gscale)
    norm = f32(f32(gscale) * np.sqrt(f32(sumsq)))
    return f32(f32(f32(gscale) * f32(clip_norm)) / max(norm, f32(clip_norm)))


def corrections(t):
    """(c1, c2) of update t >= 1 as float32: 1 / (1 - 0.9^t), 1 / (1 - 0.999^t) in double, rounded once."""
    return f32(1.0 / (1.0 - 0.9 ** int(t))), f32(1.0 / (1.0 - 0.999 ** int(t)))


def moments(g, m, v, sc):
    """(m', v') in float32: gi = g * sc, m' = fma(0.9, m, 0.1 * gi), v' = fma(0.999, v, gi * (0.001 * gi)).  Each within one ulp of the
    device's (the fma)."""
    with np.errstate(all="ignore"):
        g, m, v = (np.asarray(x, np.float32) for x in (g, m, v))
        gi = g * f32(sc)
        return fma_ref(B1, m, A1 * gi), fma_ref(B2, v, gi * (A2 * gi))


def direction(w, m1, v1, c1, c2, eps, decay):
    """u in float32 from the moments of THIS update: r = (m' c1) / (sqrt(v' c2) + eps), u = fma(decay, w, r) where decay > 0, else r.
    Bit-exact for decay 0; within one ulp of the device's u for decay > 0."""
    with np.errstate(all="ignore"):
        w, m1, v1 = (np.asarray(x, np.float32) for x in (w, m1, v1))
        mh = m1 * f32(c1)
        vh = v1 * f32(c2)
        r = mh / (np.sqrt(vh) + f32(eps))
        return fma_ref(f32(decay), w, r) if float(decay) > 0.0 else r


def sumsq64(x):
    """Sum of squares in float64 of the finite elements, and the count of the others."""
    x = np.asarray(x, np.float32).astype(np.float64).ravel()
    fin = np.isfinite(x)
    return float(np.sum(np.where(fin, x, 0.0) ** 2)), int((~fin).sum())


def trust(w, u):
    """The trust ratio of one weight tensor in float64: |w| / |u|, or 1 where a norm is 0 or w or u hold a non-finite element (TF's
    where(w_norm > 0, where(g_norm > 0, ..., 1), 1))."""
    wq, wb = sumsq64(w)
    uq, ub = sumsq64(u)
    if wb or ub or not (wq > 0.0 and uq > 0.0):
        return 1.0
    return float(np.sqrt(wq) / np.sqrt(uq))


def rate(lr, mult, t):
    """The rate the element rule sees: float32(float32(lr * mult) * float32(trust))."""
    return f32(f32(f32(lr) * f32(mult)) * f32(t))


def apply(w, u, a):
    """w' = fma(-a, u, w) in float32 (within one ulp of the device's)."""
    with np.errstate(all="ignore"):
        return fma_ref(-f32(a), u, w)


def sumsq_tol(n, decay):
    """Relative bound on |device u_sumsq - sumsq64(direction(..))|.  Where decay > 0 every u may differ by one ulp, |du| <= ULP |u|, so
    |d(u^2)| <= (2 ULP + ULP^2) u^2 and the sums differ by at most that fraction; where decay is 0 the elements are bit-equal.  Both
    sides then add n non-negative float64 terms in some order: each within n 2^-53 of the exact sum."""
    return ((2.0 * ULP + ULP * ULP) if float(decay) > 0.0 else 0.0) + 2.0 * n * 2.0 ** -53


def trust_tol(n, decay):
    """Relative bound on |float32 device trust - trust(..)|.  The ratio is sqrt(wq) / sqrt(uq): half the relative error of each sum
    (w_sumsq: summation order only, 2 n 2^-53), two square roots and a division in float64 on either side (6 roundings of 2^-53), then
    the device rounds to float32 once (half an ulp, 2^-24 relative) and the reference is compared as a double."""
    return 0.5 * sumsq_tol(n, decay) + 0.5 * 2.0 * n * 2.0 ** -53 + 6 * 2.0 ** -53 + 2.0 ** -24


def ranges(specs, tiers, weight_decay=0.0):
    """(ranges, segments) of a LAMB update.  specs: [(name, shape)] in flat order; tiers: [(begin, end, lr_mult)], the trained ranges.
    ranges = [(begin, end, lr_mult, decay, trust_index)]: a variable inside a tier is listed, one outside every tier (frozen) is not;
    rank >= 2 gets weight_decay and the next trust index, rank 1 gets decay 0 and -1 and joins an adjacent -1 entry of the same
    factor.  segments = [(name, begin, end)] of the indexed variables."""
    out, segs, off = [], [], 0
    for name, shape in specs:
        n = int(np.prod(shape))
        inside = [m for lo, hi, m in tiers if lo <= off and off + n <= hi]
        if n and inside:
            m = float(inside[0])
            if len(shape) >= 2:
                out.append((off, off + n, m, float(weight_decay), len(segs)))
                segs.append((name, off, off + n))
            elif out and out[-1][4] == -1 and out[-1][1] == off and out[-1][2] == m:
                out[-1] = (out[-1][0], off + n, m, 0.0, -1)
            else:
                out.append((off, off + n, m, 0.0, -1))
        off += n
    return out, segs
