#!/usr/bin/env python3
"""The bytes the unidirectional LSTM recurrence launches write, as one SHA-256 per case: for comparing two builds of the library.

vl_lstm_seq_fwd / vl_lstm_seq_bwd, their _len forms and their replay-safe _st forms (called eagerly, tag origin 1) are launched over
tests/lstm_plan.CLUSTER (every group size, ragged groups, two and three launches, every gather class, T = 1, 2, 21) and over every
variant of tests/lstm_plan.VARIANTS on VARIANT_CASES (initial states, gradients of them, forget biases, no dout, lengths; the per-clip form
included).  The inputs are lstm_plan.inputs of the case, the backward launch reads the fp64 reference's act and cseq rounded to fp32, every
output holds NaN beforehand (dh0 / dc0 that are not asked for keep it: that shows).  A case's digest is over the raw bytes of act, cseq,
hseq, hprev, dz, dh0, dc0, in that order.

The launches are deterministic, so two builds that compute the same thing write the same file:

    VLTF_HIP_LIB=/path/to/other/libvltf_hip.so python tools/lstm_bits.py --out a.json
    python tools/lstm_bits.py --out b.json && cmp a.json b.json

One process, one library (VLTF_HIP_LIB or the built one).  No CPU fallback.
usage: lstm_bits.py [--out FILE]"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from tests import lstm_plan as P
from vltf_amd import _ffi, ops

DEV = "cuda:0"
OUT = (("act", 4), ("cseq", 1), ("hseq", 1), ("hprev", 1), ("dz", 4))


def put(a, dtype=torch.float32):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def digest(case, variant, form, cus):
    batch, T, H = P.resolve(case, cus)
    ref = P.reference(batch, T, H, variant)
    gx, kh, h0, c0, dout = (put(a) for a in ref.inp)
    lens = put(ref.lens, torch.int32)
    o = {k: torch.full((batch * T, w * H), float("nan"), device=DEV) for k, w in OUT}
    o.update(dh0=torch.full((batch, H), float("nan"), device=DEV), dc0=torch.full((batch, H), float("nan"), device=DEV))
    grads = dict(dh0=o["dh0"] if variant.grads in ("dh0", "both") else None, dc0=o["dc0"] if variant.grads in ("dc0", "both") else None)
    ws = ops.lstm_seq_ws(batch, T, H, DEV)
    fwd = (gx, kh, o["act"], o["cseq"], o["hseq"], o["hprev"], batch, T, H)
    bwd = (dout, kh, put(ref.act32), put(ref.cseq32), o["dz"], batch, T, H)
    if form == "st":
        state = ops.step_state(DEV)
        ops.step_state_set(state, 0, 0.0, 1)
        span = ops.lstm_seq_tag_span(batch, T, H)
        ops.lstm_seq_fwd_st(*fwd, forget_bias=variant.forget_bias, ws=ws, state=state, tag_offset=0, h0=h0, c0=c0)
        ops.lstm_seq_bwd_st(*bwd, ws=ws, state=state, tag_offset=span, c0=c0, **grads)
    else:
        ops.lstm_seq_fwd(*fwd, forget_bias=variant.forget_bias, ws=ws, h0=h0, c0=c0, seq_len=lens)
        ops.lstm_seq_bwd(*bwd, ws=ws, c0=c0, seq_len=lens, **grads)
    if ops.lstm_seq_timed_out(ws):
        raise SystemExit("lstm_bits: a launch of %s timed out" % (case,))
    h = hashlib.sha256()
    for k in ("act", "cseq", "hseq", "hprev", "dz", "dh0", "dc0"):
        h.update(o[k].cpu().numpy().tobytes())
    return h.hexdigest()


def unbind_what_an_older_build_lacks():
    """VLTF_HIP_LIB may name a build from before entry points this tree declares; none of those is used here, and the binding would
    refuse the library for them.  Names are looked up in the file's symbol strings: nothing is loaded twice."""
    if not os.environ.get("VLTF_HIP_LIB"):
        return
    with open(_ffi.LIB_PATH, "rb") as f:
        blob = f.read()
    for name in [n for n in _ffi.SIGNATURES if n.encode() + b"\0" not in blob]:
        del _ffi.SIGNATURES[name]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    unbind_what_an_older_build_lacks()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    with_lens = P.Variant(lens=True)
    jobs = [(c, P.PLAIN, "eager") for c in P.CLUSTER] + [(c, with_lens, "len") for c in P.CLUSTER] + \
           [(c, P.PLAIN, "st") for c in P.CLUSTER + P.ST_CASES] + \
           [(c, v, "len" if v.lens else "eager") for c in P.VARIANT_CASES for v in P.VARIANTS] + \
           [(c, v, "st") for c in P.VARIANT_CASES for v in P.VARIANTS if not v.lens]
    out = {}
    for case, variant, form in jobs:
        name = "%s %s %s" % (form, P.case_id(case), P.case_id(variant))
        out[name] = digest(case, variant, form, cus)
    text = json.dumps({"compute_units": cus, "cases": out}, indent=1, sort_keys=True) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    h = hashlib.sha256(text.encode()).hexdigest()
    print("lstm_bits: %d cases, digest of the file %s" % (len(out), h))


if __name__ == "__main__":
    main()
