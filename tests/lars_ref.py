"""LARS restated in numpy for the tests (tf.contrib.opt.LARSOptimizer): the trust ratio in float64 and the range table of
the update.  Nothing here imports the package: the engine's own functions are checked AGAINST these."""
import numpy as np


def clip_scale_f32(clip_norm, sumsq, gscale=1.0):
    """The clip scale the update launches form, step for step in float32 as the device does (sqrt and division are correctly rounded
    there as here): gscale * clip_norm / max(gscale * sqrt(sumsq), clip_norm), or gscale without a clip."""
    f = np.float32
    if not clip_norm or clip_norm <= 0.0:
        return f(gscale)
    norm = f(f(gscale) * np.sqrt(f(sumsq)))
    return f(f(f(gscale) * f(clip_norm)) / max(norm, f(clip_norm)))


def trust(w, g, eeta, eps=0.0, decay=0.0, sc=1.0):
    """The trust ratio of one variable in float64.  w: its weights, g: its RAW gradient (before the regulariser), sc: the clip scale
    (a float32 value, clip_scale_f32), decay: the variable's L2 coefficient as the float32 the device holds.  1 where a norm is 0 or
    w or g hold a non-finite element (TF's where(w_norm > 0, where(g_norm > 0, ..., 1), 1))."""
    w, g = np.asarray(w, np.float64).ravel(), np.asarray(g, np.float64).ravel()
    if not (np.isfinite(w).all() and np.isfinite(g).all()):
        return 1.0
    wn = float(np.sqrt(np.sum(w * w)))
    gn = float(np.float64(np.float32(sc))) * float(np.sqrt(np.sum(g * g)))
    if not (wn > 0.0 and gn > 0.0):
        return 1.0
    return float(eeta) * wn / (gn + float(np.float32(decay)) * wn + float(eps))


def lr_k(lr, mult, t):
    """The rate the element rule sees: float32(float32(lr * mult) * float32(trust))."""
    f = np.float32
    return f(f(f(lr) * f(mult)) * f(t))


def ranges(specs, tiers, weight_decay=0.0):
    """(ranges, segments, decays) of a LARS update.  specs: [(name, shape)] in flat order; tiers: [(begin, end, lr_mult)], the trained
    ranges.  ranges = [(begin, end, lr_mult, trust_index)]: a variable inside a tier is listed, one outside every tier (frozen) is
    not; rank >= 2 gets the next trust index, rank 1 gets -1 and joins an adjacent -1 entry of the same factor.  segments = [(name,
    begin, end)] of the indexed variables, decays = their coefficient."""
    out, segs, decays, off = [], [], [], 0
    for name, shape in specs:
        n = int(np.prod(shape))
        inside = [m for lo, hi, m in tiers if lo <= off and off + n <= hi]
        if n and inside:
            m = float(inside[0])
            if len(shape) >= 2:
                out.append((off, off + n, m, len(segs)))
                segs.append((name, off, off + n))
                decays.append(float(weight_decay))
            elif out and out[-1][3] == -1 and out[-1][1] == off and out[-1][2] == m:
                out[-1] = (out[-1][0], off + n, m, -1)
            else:
                out.append((off, off + n, m, -1))
        off += n
    return out, segs, decays
