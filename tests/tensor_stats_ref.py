"""numpy restatement of the per-variable statistics (include/vltf.h: vl_tensor_stats; engine.tensor_stats_report), shared by
tests/test_tensor_stats.py (host) and tests/test_tensor_stats_gpu.py (device).  Per segment: the finite mask, math.fsum sums (exact
up to one rounding), min / max over the finite elements, the counts; the derived dict restates the engine's formulas."""
import collections
import math

import numpy as np

INF = float("inf")


def one_side(x):
    """Sums, extrema and counts of one float32 array as the launch defines them, plus sum|term| of both sums for the error bound."""
    x = np.asarray(x, np.float32).ravel()
    fin = np.isfinite(x)
    v = x[fin].astype(np.float64)
    sq = v * v                                  # exact: the product of two float32 values fits a float64
    return dict(sum=math.fsum(v), sumsq=math.fsum(sq), abs_sum=math.fsum(np.abs(v)), abs_sumsq=math.fsum(sq),
                min=float(v.min()) if v.size else INF, max=float(v.max()) if v.size else -INF,
                nonfinite=int((~fin).sum()), zero=int((x == 0.0).sum()), n=int(x.size))


def segment_rows(w, g, segments):
    """[(row of the weights, row of the gradient)] for segments [(begin, end)] or [(name, begin, end)] of the flat arrays."""
    return [(one_side(w[s[-2]:s[-1]]), one_side(g[s[-2]:s[-1]])) for s in segments]


def sum_bound(side, key):
    """The contract: a sum over a segment of N elements is within N 2^-53 sum|term| of the exact sum."""
    return side["n"] * 2.0 ** -53 * side["abs_" + key]


def check_row(got, want_w, want_g, msg=""):
    """got: one ops.STAT_DTYPE record.  Sums to the contract's bound, min / max by value, counts exactly, reserved 0."""
    for p, want in (("w", want_w), ("g", want_g)):
        for key in ("sum", "sumsq"):
            err, bound = abs(float(got["%s_%s" % (p, key)]) - want[key]), sum_bound(want, key)
            assert err <= bound, "%s %s_%s: |%r - %r| = %g > %g" % (msg, p, key, float(got["%s_%s" % (p, key)]), want[key], err, bound)
        assert float(got[p + "_min"]) == want["min"] and float(got[p + "_max"]) == want["max"], \
            (msg, p, float(got[p + "_min"]), want["min"], float(got[p + "_max"]), want["max"])
        assert int(got[p + "_nonfinite"]) == want["nonfinite"], (msg, p, int(got[p + "_nonfinite"]), want["nonfinite"])
    assert int(got["g_zero"]) == want_g["zero"], (msg, int(got["g_zero"]), want_g["zero"])
    assert int(got["reserved"]) == 0, msg


def clip_scale(sumsq, clip_norm):
    return clip_norm / max(math.sqrt(sumsq), clip_norm) if clip_norm and clip_norm > 0 else 1.0


def derived(names, rows, lr_mults, lr, clip_norm, sumsq):
    """({name: {...}}, grads_norm_mean) from segment_rows' output: the engine's keys by the issue's formulas."""
    sc = clip_scale(sumsq, clip_norm)
    out, norms = collections.OrderedDict(), []
    for name, (w, g), mult in zip(names, rows, lr_mults):
        d = {}
        for key, s in (("grad", g), ("weight", w)):
            fin = s["n"] - s["nonfinite"]
            mean = s["sum"] / fin if fin else float("nan")
            d[key + "_norm"] = math.sqrt(s["sumsq"])
            d[key + "_mean"] = mean
            d[key + "_std"] = math.sqrt(max(s["sumsq"] / fin - mean * mean, 0.0)) if fin else float("nan")
            d[key + "_min"], d[key + "_max"], d[key + "_nonfinite"] = s["min"], s["max"], s["nonfinite"]
        d["grad_zero_fraction"] = g["zero"] / g["n"]
        d["lr_mult"] = mult
        d["sgd_update_ratio"] = lr * mult * sc * d["grad_norm"] / d["weight_norm"] if d["weight_norm"] > 0 else None
        out[name] = d
        norms.append(sc * d["grad_norm"])
    return out, sum(norms) / len(norms)


def close_reports(got, want, counts, msg=""):
    """Two derived dicts: same variables in the same order; counts, min / max, lr_mult and None-ness equal.  counts: {name: elements}.
    With eps = n 2^-53, the contract's relative bound of a sum of one sign (sumsq; |sum| <= sum|x|): norms, ratios and means are held to
    4 eps of their scale (rms for a mean), and std = sqrt(sumsq / n - mean^2), a difference of two numbers each good to ~eps rms^2, to
    sqrt(4 eps) rms."""
    assert list(got) == list(want), (msg, list(got), list(want))
    for name in want:
        g, w = got[name], want[name]
        assert sorted(g) == sorted(w), (msg, name)
        for k, wv in w.items():
            gv = g[k]
            if wv is None or isinstance(wv, int):
                assert gv == wv, (msg, name, k, gv, wv)
            elif isinstance(wv, float) and math.isnan(wv):
                assert math.isnan(gv), (msg, name, k, gv)
            elif k.endswith("_min") or k.endswith("_max") or k == "lr_mult":
                assert gv == wv, (msg, name, k, gv, wv)
            elif k.endswith("_std") or k.endswith("_mean"):
                pre = k[:k.rindex("_")]
                eps = counts[name] * 2.0 ** -53
                rms = math.sqrt(w[pre + "_mean"] ** 2 + w[pre + "_std"] ** 2)
                tol = (math.sqrt(4 * eps) if k.endswith("_std") else 4 * eps) * rms + 1e-300
                assert abs(gv - wv) <= tol, (msg, name, k, gv, wv, tol)
            else:
                assert abs(gv - wv) <= 4 * counts[name] * 2.0 ** -53 * abs(wv) + 1e-300, (msg, name, k, gv, wv)
