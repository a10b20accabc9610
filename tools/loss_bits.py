#!/usr/bin/env python3
"""The bytes the loss launches write, as one SHA-256 per case: for comparing two builds of the library.

Every entry point (vl_softmax_xent, vl_softmax_xent_len, vl_softmax_xent_ls, vl_softmax_xent_mix, and vl_softmax_xent_wf where the
library has it) is launched over a fixed list of
cases: the shapes of tests/test_label_smoothing_gpu.py and the two that tools/bench_label_smoothing.py times, both launch forms,
lengths off and on, smoothing {0, 0.1}, top_k {0, 5}, rows_per_clip {1, 2} where it divides the batch, lam {1, 0.5, 0.8} as a host
argument and as a device word.  The inputs are those of case() of that test file; dlogits and the rows workspace hold NaN beforehand
and stats holds 1, 2, 3 (a sum that is left alone shows).  A case's digest is over the raw bytes of dlogits, stats and rows, in that order.
The vl_softmax_xent_wf cases (weights off / on, gamma {0, 2}, smoothing 0.1, top_k 5, lengths, a lambda) come after the last case of the last shape,
so the file of a build from before that entry point is the head of this one's, name for name.

The launches are deterministic, so two builds that compute the same thing write the same file:

    VLTF_HIP_LIB=/path/to/other/libvltf_hip.so python tools/loss_bits.py --out a.json
    python tools/loss_bits.py --out b.json && cmp a.json b.json

One process, one library (VLTF_HIP_LIB or the built one).  No CPU fallback.
usage: loss_bits.py [--out FILE]"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from oracle import lrcn_oracle as O
from vltf_amd import _ffi, ops

DEV = "cuda:0"
NAN = float("nan")
SHAPES = [(5, 7), (4, 64), (3, 65), (9, 101), (6, 1000), (64, 101), (1344, 1000)]
SMOOTHING, TOP_K, LAMS = (0.0, 0.1), (0, 5), (1.0, 0.5, 0.8)


def case(b, c):
    """tests/test_label_smoothing_gpu.py::case: logits 2 N(0, 1) and one-hot labels, every third row a hit"""
    rng = np.random.default_rng(b * c)
    z = (rng.standard_normal((b, c)) * 2).astype(np.float32)
    onehot = O.labels_to_one_hot([[l] for l in rng.integers(0, c, b)], c)
    for r in range(0, b, 3):
        onehot[r] = 0
        onehot[r, np.argmax(z[r])] = 1
    return z, onehot


def lengths(b, c):
    """(seq_len, T): T the smallest divisor of b above 1, lengths drawn from 0 .. T (an empty and a whole sequence can occur)"""
    T = next(t for t in range(2, b + 1) if b % t == 0)
    return np.random.default_rng(b * c + 1).integers(0, T + 1, b // T).astype(np.int32), T


def cases(b, c):
    """(name, function of (z, y, dlogits, stats, rows)) of every launch at b x c but for the form, which the caller varies"""
    lens, T = lengths(b, c)
    sl = torch.from_numpy(lens).to(DEV)
    yield "plain", lambda z, y, dz, st, ws: ops.softmax_xent(z, y, dz, st[:2], 1.0 / b, ws)
    yield "len", lambda z, y, dz, st, ws: ops.softmax_xent(z, y, dz, st[:2], 1.0 / b, ws, seq_len=sl, T=T)
    for eps in SMOOTHING:
        for k in TOP_K:
            for with_len in (False, True):
                yield ("ls eps %g k %d len %d" % (eps, k, with_len),
                       lambda z, y, dz, st, ws, eps=eps, k=k, kw=dict(seq_len=sl, T=T) if with_len else {}:
                       ops.softmax_xent_ls(z, y, dz, st, 1.0 / b, ws, eps, k, **kw))
            for rpc in (1, 2):
                if b % rpc:
                    continue
                for lam in LAMS:
                    for on_device in (False, True):
                        yield ("mix eps %g k %d rpc %d lam %g %s" % (eps, k, rpc, lam, "device" if on_device else "host"),
                               lambda z, y, dz, st, ws, eps=eps, k=k, rpc=rpc,
                               lam=torch.tensor([lam], device=DEV) if on_device else lam:
                               ops.softmax_xent_mix(z, y, dz, st, 1.0 / b, ws, rpc, eps, k, lam))


def wf_cases(b, c):
    """cases() for vl_softmax_xent_wf"""
    lens, T = lengths(b, c)
    sl = torch.from_numpy(lens).to(DEV)
    w = torch.from_numpy(np.random.default_rng(b * c + 2).uniform(0.25, 4.0, c).astype(np.float32)).to(DEV)
    for weights in (False, True):
        for gamma in (0.0, 2.0):
            for name, kw in (("plain", {}), ("len", dict(seq_len=sl, T=T)), ("lam 0.8", dict(lam=0.8))):
                yield ("wf weights %d gamma %g %s" % (weights, gamma, name),
                       lambda z, y, dz, st, ws, weights=weights, gamma=gamma, kw=kw:
                       ops.softmax_xent_wf(z, y, dz, st, 1.0 / b, ws, 0.1, 5, w if weights else None, gamma, **kw))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="the digests as JSON (default: standard output)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_bits.py needs a HIP device; there is no CPU fallback")
    digests = {}
    for b, c, cases_of in [s + (cases,) for s in SHAPES] + [s + (wf_cases,) for s in SHAPES]:
        z, onehot = case(b, c)
        zd, yd = torch.from_numpy(z).to(DEV), torch.from_numpy(np.ascontiguousarray(onehot)).to(DEV, torch.int32)
        for name, launch in cases_of(b, c):
            for form in ("one-workgroup", "rows"):
                dz = torch.full((b, c), NAN, device=DEV)
                stats = torch.tensor([1.0, 2.0, 3.0], device=DEV)
                ws = torch.full((3 * b,), NAN, device=DEV) if form == "rows" else None
                launch(zd, yd, dz, stats, ws)
                h = hashlib.sha256()
                for t in (dz, stats) + (() if ws is None else (ws,)):
                    h.update(t.cpu().numpy().tobytes())
                digests["%dx%d %s, %s" % (b, c, name, form)] = h.hexdigest()
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
