#!/usr/bin/env python3
"""The bytes the flat-buffer update launches write, as one SHA-256 per case: for comparing two builds of the library.

Every entry point that walks ranges of the flat buffers -- vl_sumsq_tiers, vl_l2_regularize, vl_sgd_apply / _tiers / _st / _tiers_st,
vl_adam_apply / _tiers / _st / _tiers_st, vl_momentum_apply / _st, vl_grad_accumulate (modes 0, 1, 2), vl_ema_update / _st,
vl_lars_apply / _st, vl_lamb_apply / _st -- is launched over a fixed list of cases, the smallest at which a walk can go wrong:
  walk     one range of 1, 2, 3, 4, 5, 7, 8 or 1027 elements that begins 0, 1, 2 or 3 elements into the buffer: as a one-range table
           and, where the entry point has a form without a table (plain or NULL), as the whole buffer behind a base pointer of that phase
  table    three ranges with gaps and distinct lr_mult / decay / trust_index (a -1 among them, a decay of 0 next to a non-zero one), the
           base pointers of all arrays 0 or 1 element past a 16-byte boundary, or each array at a phase of its own (the all-scalar path)
  whole    the form without a table over 1027 elements, the same three sets of base pointers
  options  clip_norm {0, 0.5} with a sumsq word, gscale {1, 0.125}, nesterov {0, 1}, the skip word absent, 0 and 1 (with 1 nothing
           may change: checked here), each where the entry point has the argument
  large    4 * 4096 * 256 + 5 elements: the grids are capped at 4096 and 1024 workgroups of 256, so the interior's grid-stride loop
           takes a second pass
and every case of an entry point with an _st form runs through that form too, the step state written by vl_step_state_set, _set_ema and
_set_lamb.  vl_fc_dropout_fwd / _st and vl_relu_dropout_grad go through the same walk over a whole buffer and have those cases;
vl_lamb_moments and vl_tensor_stats (another walk) have one case each.

The inputs are fixed-seed N(0, 1) floats (Adam's and LAMB's v: their squares, a second moment is not negative).  Every array sits in a
backing buffer with room on both sides; a case's digest is over the raw bytes of the backing buffers of all its arrays in the order of the
rule, then of what else the launch defines: the `out` words, and of a partial-sum workspace (NaN beforehand) the `blocks` words of each sum.

The launches are deterministic, so two builds that compute the same thing write the same file:

    VLTF_HIP_LIB=/path/to/other/libvltf_hip.so python tools/update_bits.py --out a.json
    python tools/update_bits.py --out b.json && cmp a.json b.json

One process, one library (VLTF_HIP_LIB or the built one).  No CPU fallback.
usage: update_bits.py [--out FILE]"""
import argparse
import hashlib
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from vltf_amd import _ffi, ops

DEV = "cuda:0"
NAN = float("nan")
LENGTHS, OFFSETS = (1, 2, 3, 4, 5, 7, 8, 1027), (0, 1, 2, 3)
LARGE = 4 * 4096 * 256 + 5
GAPS, GAPS_N = [(3, 10), (17, 530), (535, 1090)], 1100
MULT, DECAY, TRUST_INDEX, TRUST = (0.5, 2.0, 1.0), (0.01, 0.0, 0.003), (1, -1, 0), (0.75, 1.5)
LR, MOMENTUM, RATE, EPS, STEP = 0.01, 0.9, 0.001, 1e-6, 6
KEEP, SEED, SALT = 0.5, 1234, 6
C1, C2 = 1.0 / (1.0 - 0.9 ** (STEP + 1)), 1.0 / (1.0 - 0.999 ** (STEP + 1))
PAD = 4


def grid_for(work, cap):
    """csrc/pointwise.hip: grid_for(work, 256, cap)"""
    return max(1, min((work + 255) // 256, cap))


def update_kw(o, *names):
    return {k: o[k] for k in ("clip_norm", "sumsq_t", "gscale", "skip") + names}


def tiers(t, shift=0):
    return [(b, e, MULT[(k + shift) % 3]) for k, (b, e) in enumerate(t)]


def lars_ranges(t):
    return [(b, e, MULT[k % 3], TRUST_INDEX[k % 3]) for k, (b, e) in enumerate(t)]


def lamb_ranges(t):
    return [(b, e, MULT[k % 3], DECAY[k % 3], TRUST_INDEX[k % 3]) for k, (b, e) in enumerate(t)]


def trust():
    return torch.tensor(TRUST, device=DEV)


# ---- the rules: launch(a, t, st, o) with a = {name: view}, t = [(begin, end)] or None, st = a step state or None, o = the options --------
def sumsq_tiers(a, t, st, o):
    out, ws = torch.full((1,), NAN, device=DEV), torch.full((1024,), NAN, device=DEV)
    ops.sumsq_tiers(a["g"], tiers(t), out, ws)
    return [ws[:grid_for(sum(e - b for b, e in t) // 4 + 1, 1024)], out]


def l2_regularize(shift):
    def launch(a, t, st, o):
        out, ws = torch.full((2,), NAN, device=DEV), torch.full((2048,), NAN, device=DEV)
        ops.l2_regularize(a["w"], a["g"], [(b, e, DECAY[(k + shift) % 3]) for k, (b, e) in enumerate(t)], out, ws)
        blocks = grid_for(sum(e - b for b, e in t) // 4 + 1, 1024)
        return [ws[:blocks], ws[1024:1024 + blocks], out]
    return launch


def sgd(a, t, st, o):
    kw = update_kw(o)
    if t is None and st is None: ops.sgd_apply(a["w"], a["g"], LR, **kw)
    elif t is None: ops.sgd_apply_st(a["w"], a["g"], st, **kw)
    elif st is None: ops.sgd_apply_tiers(a["w"], a["g"], tiers(t), LR, **kw)
    else: ops.sgd_apply_tiers_st(a["w"], a["g"], tiers(t), st, **kw)


def adam(a, t, st, o):
    kw, x = update_kw(o), (a["w"], a["g"], a["m"], a["v"])
    if t is None and st is None: ops.adam_apply(*x, LR, STEP + 1, **kw)
    elif t is None: ops.adam_apply_st(*x, st, **kw)
    elif st is None: ops.adam_apply_tiers(*x, tiers(t), LR, STEP + 1, **kw)
    else: ops.adam_apply_tiers_st(*x, tiers(t), st, **kw)


def momentum(a, t, st, o):
    kw = update_kw(o, "nesterov")
    kw["tiers"] = None if t is None else tiers(t)
    if st is None: ops.momentum_apply(a["w"], a["g"], a["a"], LR, MOMENTUM, **kw)
    else: ops.momentum_apply_st(a["w"], a["g"], a["a"], st, MOMENTUM, **kw)


def accumulate(mode):
    return lambda a, t, st, o: ops.grad_accumulate(a["acc"], a["g"], mode, None if t is None else tiers(t))


def ema(a, t, st, o):
    ranges = None if t is None else tiers(t)
    if st is None: ops.ema_update(a["s"], a["w"], RATE, skip=o["skip"], ranges=ranges)
    else: ops.ema_update_st(a["s"], a["w"], st, skip=o["skip"], ranges=ranges)


def lars(a, t, st, o):
    kw = update_kw(o, "nesterov")
    if st is None: ops.lars_apply(a["w"], a["g"], a["a"], lars_ranges(t), trust(), LR, MOMENTUM, **kw)
    else: ops.lars_apply_st(a["w"], a["g"], a["a"], lars_ranges(t), trust(), st, MOMENTUM, **kw)


def lamb(a, t, st, o):
    if st is None: ops.lamb_apply(a["w"], a["m"], a["v"], lamb_ranges(t), trust(), LR, C1, C2, EPS, skip=o["skip"])
    else: ops.lamb_apply_st(a["w"], a["m"], a["v"], lamb_ranges(t), trust(), st, EPS, skip=o["skip"])


def fc_dropout(a, t, st, o):
    if st is None: ops.fc_dropout_fwd(a["y"], KEEP, SEED, SALT)
    else: ops.fc_dropout_fwd_st(a["y"], KEEP, st, SALT)


def relu_dropout_grad(a, t, st, o):
    ops.relu_dropout_grad(a["d"], a["y"], KEEP)


def lamb_moments(a, t, st, o):
    ranges = lamb_ranges(t)
    rows = torch.zeros(len(TRUST) * ops.LAMB_ROW_BYTES, dtype=torch.uint8, device=DEV)
    tr = torch.full((len(TRUST),), NAN, device=DEV)
    ws = torch.zeros(ops.lamb_moments_ws_bytes(ranges), dtype=torch.uint8, device=DEV)
    ops.lamb_moments(a["w"], a["g"], a["m"], a["v"], ranges, rows, tr, ws, C1, C2, EPS, clip_norm=0.5, sumsq_t=o["sumsq_t"])
    return [rows, tr]


def tensor_stats(a, t, st, o):
    out = torch.zeros(len(t) * ops.STAT_ROW_BYTES, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(ops.tensor_stats_ws_bytes(t), dtype=torch.uint8, device=DEV)
    ops.tensor_stats(a["w"], a["g"], t, out, ws)
    return [out]


CLIP = ("clip_norm", "gscale", "skip")
TABLE, WHOLE = 1, 2
# name, arrays, launch, its forms (with a table, without one: plain or NULL), has an _st form, the options it takes
RULES = [
    ("sumsq_tiers", ("g",), sumsq_tiers, TABLE, False, ()),
    ("l2_regularize", ("w", "g"), l2_regularize(0), TABLE, False, ()),
    ("l2_regularize decay 0 first", ("w", "g"), l2_regularize(1), TABLE, False, ()),
    ("sgd", ("w", "g"), sgd, TABLE | WHOLE, True, CLIP),
    ("adam", ("w", "g", "m", "v"), adam, TABLE | WHOLE, True, CLIP),
    ("momentum", ("w", "g", "a"), momentum, TABLE | WHOLE, True, CLIP + ("nesterov",)),
    ("accumulate 0", ("acc", "g"), accumulate(0), TABLE | WHOLE, False, ()),
    ("accumulate 1", ("acc", "g"), accumulate(1), TABLE | WHOLE, False, ()),
    ("accumulate 2", ("acc", "g"), accumulate(2), TABLE | WHOLE, False, ()),
    ("ema", ("s", "w"), ema, TABLE | WHOLE, True, ("skip",)),
    ("lars", ("w", "g", "a"), lars, TABLE, True, CLIP + ("nesterov",)),
    ("lamb", ("w", "m", "v"), lamb, TABLE, True, ("skip",)),
    ("fc_dropout", ("y",), fc_dropout, WHOLE, True, ()),
    ("relu_dropout_grad", ("d", "y"), relu_dropout_grad, WHOLE, False, ()),
]
GUARDS = [("lamb_moments", ("w", "g", "m", "v"), lamb_moments), ("tensor_stats", ("w", "g"), tensor_stats)]
VALUES = {"clip_norm": (0.0, 0.5), "gscale": (1.0, 0.125), "nesterov": (False, True), "skip": (None, 0, 1)}
DEFAULTS = {"clip_norm": 0.0, "gscale": 1.0, "nesterov": False, "skip": None}
PHASES = (("phase 0", lambda j: 0), ("phase 1", lambda j: 1), ("phases apart", lambda j: j % 4))


def cases(forms, options):
    """(name, n, table, phase of array j, options) of every case of one rule"""
    whole = forms & WHOLE
    for length, off in itertools.product(LENGTHS, OFFSETS):
        if forms & TABLE:
            yield "walk %d at %d, table" % (length, off), off + length + 3, [(off, off + length)], PHASES[0][1], {}
        if whole:
            yield "walk %d at %d, whole" % (length, off), length, None, lambda j, off=off: off, {}
    for name, phase in PHASES:
        if forms & TABLE:
            yield "table, %s" % name, GAPS_N, GAPS, phase, {}
        if whole:
            yield "whole, %s" % name, 1027, None, phase, {}
    for values in itertools.product(*(VALUES[k] for k in options)):
        o = dict(zip(options, values))
        if o:
            yield "options %s" % " ".join("%s %s" % kv for kv in o.items()), GAPS_N, GAPS, PHASES[0][1], o
    yield "large", LARGE, None if whole else [(0, LARGE)], PHASES[0][1], {}
    if forms == TABLE | WHOLE:
        yield "large, table", LARGE, [(0, LARGE)], PHASES[0][1], {}


def run(name, arrays, launch, n, table, phase, opts, state):
    """one launch on fresh arrays -> the digest"""
    rng = np.random.default_rng(n)
    back, views = [], {}
    for j, k in enumerate(arrays):
        x = rng.standard_normal(n + 2 * PAD).astype(np.float32)
        back.append(torch.from_numpy(x * x if k == "v" else x).to(DEV))
        views[k] = back[-1][PAD + phase(j):PAD + phase(j) + n]
    o = dict(DEFAULTS, **opts)
    o["sumsq_t"] = torch.tensor([9.0], device=DEV)
    if o["skip"] is not None:
        o["skip"] = torch.tensor([o["skip"]], dtype=torch.int32, device=DEV)
    before = [b.clone() for b in back]
    extra = launch(views, table, state, o) or []
    if opts.get("skip") == 1 and not all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(before, back)):
        raise SystemExit("%s: the skip word holds 1 and the launch wrote" % name)
    h = hashlib.sha256()
    for t in back + extra:
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="the digests as JSON (default: standard output)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("update_bits.py needs a HIP device; there is no CPU fallback")
    state = ops.step_state(DEV)
    ops.step_state_set(state, STEP, LR, 0)
    ops.step_state_set_ema(state, RATE)
    ops.step_state_set_lamb(state, C1, C2)
    digests = {}
    for rule, arrays, launch, forms, has_st, options in RULES:
        for name, n, table, phase, opts in cases(forms, options):
            for st in (None, state) if has_st else (None,):
                full = "%s%s: %s" % (rule, "" if st is None else " st", name)
                digests[full] = run(full, arrays, launch, n, table, phase, opts, st)
    for rule, arrays, launch in GUARDS:
        digests["%s: table, phase 0" % rule] = run(rule, arrays, launch, GAPS_N, GAPS, PHASES[0][1], {}, None)
    h = hashlib.sha256()
    h.update(state.cpu().numpy().tobytes())
    digests["step state"] = h.hexdigest()
    text = json.dumps(digests, indent=1) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    print("%d cases, library %s" % (len(digests), _ffi.LIB_PATH), file=sys.stderr)


if __name__ == "__main__":
    main()
