#!/usr/bin/env python3
"""What NetVLAD pooling over time (fusion vlad) costs on one GPU, in ONE process, everything in alternation.

1. The launches alone, T = 16, HO = 256, K = 8 and 64, at 8 and 64 clips, HIP events on the launch stream (tools/bench_attn_pool.py's
   method):
     vlad_k8, vlad_k64   vl_netvlad_fwd / vl_netvlad_bwd;
     attn                vl_attn_pool_fwd / vl_attn_pool_bwd at the same clips, T and HO (A = 256).
   Recorded, not bounded: the work differs by the factor K.

2. The launches a step with fusion vlad (K = 8) ADDS to a step with fusion avg, each alone at the step's shape (clips x 16 rows): the
   projection s = hseq W + beta, the two kernels, the kernel gradient hseq^T ds, the two column sums (ds for the bias, dcp for the
   centres), dproj = ds W^T and the add of dproj onto dout.  Recorded beside them and NOT part of the bound: what the WIDER HEAD costs,
   the head's three products and its dropout pair at K HO = 2048 columns less the same five launches at HO = 256 columns
   (head_extra_us).  The products are called as the engines call them, without a workspace: fp32 whatever the step's conv_math, so
   ONE measurement serves both steps.

3. The step.  The train step at the benchmark geometry (64 clips x 16 frames of 227x227, AlexNet(fc6) -> LSTM(256) -> 101 classes, plain
   SGD, dropout 0.5), fp32 and the packed-bf16 conv path, with fusion avg and with fusion vlad (vlad_clusters 8), with the spread
   between rounds.

The one check, attn's: step(vlad) - step(avg) <= (sum of the added launches measured alone) + (spread between rounds of step(vlad): max
- min of that run's per-round means).  The spread of the avg run is recorded beside it and NOT added.  The tool exits 1 when the check
fails in fp32 or on the bf16 path.

Writes profiles/netvlad_step.json.  No CPU fallback.
usage: bench_netvlad.py [--clips 64] [--rounds 8] [--steps 5] [--warmup 3] [--batch 100] [--launch-rounds 10] [--no-step] [--out FILE]"""
import argparse
import dataclasses
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from vltf_amd import ops
from vltf_amd.engine import LRCNEngine, NetConfig, init_params

MEAN = np.array([99.197148, 105.293620, 109.503945], np.float32)
T, HO, A, C = 16, 256, 256, 101
K_STEP = 8
ORDER = ["avg", "vlad"]
ADDED = ["projection", "netvlad_fwd", "netvlad_bwd", "kernel_grad", "colsum_ds", "colsum_dcp", "dproj", "add"]
HEAD = ["head_fwd", "head_wgrad", "head_dgrad", "dropout_fwd", "dropout_bwd"]


def alternate(launchers, rounds, batch):
    """{name: us per call}: `batch` calls of each between two device events, the names in alternation, `rounds` times."""
    for fn in launchers.values():
        for _ in range(min(batch, 20)):
            fn()
    torch.cuda.synchronize()
    per_round = {name: [] for name in launchers}
    for _ in range(rounds):
        for name, fn in launchers.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(batch):
                fn()
            b.record()
            b.synchronize()
            per_round[name].append(a.elapsed_time(b) / batch * 1e3)
    return {name: {"us": round(sum(v) / rounds, 3), "us_by_round": [round(x, 3) for x in v],
                   "spread_us": round(max(v) - min(v), 3)} for name, v in per_round.items()}


class Vlad:
    """The operands of every launch of fusion vlad at `clips` clips and K centres."""

    def __init__(self, clips, K, dev):
        torch.manual_seed(clips * 100 + K)
        n = clips * T
        r = lambda *s, scale=1.0: torch.randn(*s, device=dev) * scale
        z = lambda *s: torch.zeros(*s, device=dev)
        self.clips, self.n, self.K = clips, n, K
        self.h, self.W, self.b, self.c = r(n, HO), r(HO, K, scale=HO ** -0.5), r(K, scale=0.1), r(K, HO, scale=0.5)
        self.s, self.a, self.r, self.y, self.dy = z(n, K), z(n, K), z(clips, K), z(clips, K * HO), r(clips, K * HO)
        self.ds, self.dh, self.dcp, self.dproj = z(n, K), z(n, HO), z(clips, K * HO), z(n, HO)
        self.gW, self.gb, self.gc = z(HO, K), z(K), z(K * HO)
        self.sws = torch.empty(64 * max(1024, K * HO), device=dev)
        ops.gemm(self.h, self.W, self.s, n, K, HO, bias=self.b)
        self.fwd()
        self.bwd()

    def fwd(self):
        ops.netvlad_fwd(self.s, self.c, self.h, self.a, self.r, self.y, self.clips, T, HO, self.K)

    def bwd(self):
        ops.netvlad_bwd(self.dy, self.h, self.a, self.r, self.y, self.c, self.ds, self.dh, self.dcp, self.clips, T, HO, self.K)

    def added(self):
        n, clips, K = self.n, self.clips, self.K
        return {"projection": lambda: ops.gemm(self.h, self.W, self.s, n, K, HO, bias=self.b),
                "netvlad_fwd": self.fwd, "netvlad_bwd": self.bwd,
                "kernel_grad": lambda: ops.gemm(self.h, self.ds, self.gW, HO, K, n, transa=True),
                "colsum_ds": lambda: ops.colsum(self.ds, self.gb, self.sws, n, K),
                "colsum_dcp": lambda: ops.colsum(self.dcp, self.gc, self.sws, clips, K * HO),
                "dproj": lambda: ops.gemm(self.ds, self.W, self.dproj, n, HO, K, transb=True),
                "add": lambda: ops.eltwise2(self.dh, self.dproj, self.dh, "add", n * HO)}


class Head:
    """The head's three products and its dropout pair at `width` input columns."""

    def __init__(self, clips, width, dev):
        torch.manual_seed(width)
        r = lambda *s, scale=1.0: torch.randn(*s, device=dev) * scale
        z = lambda *s: torch.zeros(*s, device=dev)
        self.clips, self.width = clips, width
        self.v, self.W, self.b, self.d = r(clips, width), r(width, C, scale=width ** -0.5), z(C), r(clips, C)
        self.logits, self.gW, self.dv, self.dropped, self.dfused = z(clips, C), z(width, C), z(clips, width), z(clips, width), z(clips, width)
        self.mask = torch.zeros(clips, width, dtype=torch.uint8, device=dev)

    def launches(self):
        b, w = self.clips, self.width
        return {"head_fwd": lambda: ops.gemm(self.dropped, self.W, self.logits, b, C, w, bias=self.b),
                "head_wgrad": lambda: ops.gemm(self.dropped, self.d, self.gW, w, C, b, transa=True),
                "head_dgrad": lambda: ops.gemm(self.d, self.W, self.dv, b, w, C, transb=True),
                "dropout_fwd": lambda: ops.dropout_fwd(self.v, self.dropped, self.mask, 0.5, 12345),
                "dropout_bwd": lambda: ops.dropout_bwd(self.dv, self.mask, self.dfused, 0.5)}


class Attn:
    def __init__(self, clips, dev):
        torch.manual_seed(clips)
        n = clips * T
        r = lambda *s, scale=1.0: torch.randn(*s, device=dev) * scale
        z = lambda *s: torch.zeros(*s, device=dev)
        self.clips = clips
        self.h, self.c, self.u = r(n, HO), r(A, scale=A ** -0.5), r(n, A)
        self.s, self.alpha, self.y, self.dy = z(n, A), z(clips, T), z(clips, HO), r(clips, HO)
        self.du, self.dh, self.dcp = z(n, A), z(n, HO), z(clips, A)
        self.fwd()

    def fwd(self):
        ops.attn_pool_fwd(self.u, self.c, self.h, self.s, self.alpha, self.y, self.clips, T, HO, A)

    def bwd(self):
        ops.attn_pool_bwd(self.dy, self.h, self.s, self.alpha, self.c, self.du, self.dh, self.dcp, self.clips, T, HO, A)


def launches_alone(clips, rounds, batch, dev):
    v8, v64, at = Vlad(clips, 8, dev), Vlad(clips, 64, dev), Attn(clips, dev)
    fwd = alternate({"vlad_k8": v8.fwd, "vlad_k64": v64.fwd, "attn": at.fwd}, rounds, batch)
    bwd = alternate({"vlad_k8": v8.bwd, "vlad_k64": v64.bwd, "attn": at.bwd}, rounds, batch)
    for v in (fwd, bwd):
        v["vlad_k8_over_attn"] = round(v["vlad_k8"]["us"] / v["attn"]["us"], 3)
        v["vlad_k64_over_attn"] = round(v["vlad_k64"]["us"] / v["attn"]["us"], 3)
    return {"forward": fwd, "backward": bwd}


def added_alone(clips, rounds, batch, dev):
    res = alternate(Vlad(clips, K_STEP, dev).added(), rounds, batch)
    wide, narrow = Head(clips, K_STEP * HO, dev).launches(), Head(clips, HO, dev).launches()
    both = {"%s_%s" % (k, tag): fn for k in HEAD for tag, fn in (("wide", wide[k]), ("narrow", narrow[k]))}
    res["head"] = alternate(both, rounds, batch)
    res["head_extra_us"] = round(sum(res["head"][k + "_wide"]["us"] - res["head"][k + "_narrow"]["us"] for k in HEAD), 3)
    res["sum_us"] = round(sum(res[k]["us"] for k in ADDED), 3)          # the bound counts the ADDED launches only; head_extra_us is recorded
    return res


def measure_step(conv_math, clips, fpc, rounds, steps, warmup, dev):
    base = NetConfig(image_shape=(227, 227, 3), num_classes=C, fpc=fpc, dropout_keep_prob=0.5, conv_math=conv_math)
    cfgs = {"avg": base, "vlad": dataclasses.replace(base, fusion="vlad", vlad_clusters=K_STEP)}
    engines = {}
    for name in ORDER:
        engines[name] = LRCNEngine(cfgs[name], max_clips=clips, device=dev)
        engines[name].load_params(init_params(cfgs[name], seed=2))
    rng = np.random.default_rng(0)
    frames = torch.from_numpy(rng.integers(0, 256, (clips * fpc, 227, 227, 3), dtype=np.uint8)).to(dev)
    onehot = torch.zeros((clips, C), dtype=torch.int32)
    onehot[torch.arange(clips), torch.from_numpy(rng.integers(0, C, clips))] = 1
    onehot = onehot.to(dev)

    def run(name, fetch=False):
        return engines[name].train_step_u8(frames, onehot, lr=1e-3, clip_norm=10.0, mean_bgr=MEAN, fetch=fetch)

    for name in ORDER:
        for _ in range(warmup):
            run(name)
    torch.cuda.synchronize()
    per_round = {name: [] for name in ORDER}
    for _ in range(rounds):                         # in alternation: a drift of the clocks hits both alike
        for name in ORDER:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                run(name)
            torch.cuda.synchronize()
            per_round[name].append((time.perf_counter() - t0) / steps * 1e3)
    out = {}
    for name in ORDER:
        ms = sum(per_round[name]) / rounds
        check = run(name, fetch=True)
        out[name] = {"ms_per_step": round(ms, 3), "clips_per_s": round(clips / ms * 1e3, 1), "timed_steps": rounds * steps,
                     "ms_per_step_by_round": [round(v, 3) for v in per_round[name]],
                     "spread_ms": round(max(per_round[name]) - min(per_round[name]), 3), "loss": round(check["loss"], 4),
                     "grad_norm": round(check["grad_norm"], 4)}
    out["vlad_minus_avg_ms"] = round(out["vlad"]["ms_per_step"] - out["avg"]["ms_per_step"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--fpc", type=int, default=T)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5, help="timed steps per round (rounds x steps >= 20)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=100, help="calls between two device events")
    ap.add_argument("--launch-rounds", type=int, default=10)
    ap.add_argument("--no-step", action="store_true", help="the launches alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "netvlad_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_netvlad.py needs a HIP device; there is no CPU fallback")
    if args.rounds * args.steps < 20:
        raise SystemExit("at least 20 timed steps each: rounds x steps = %d" % (args.rounds * args.steps))
    if args.fpc != T:
        raise SystemExit("the added launches are measured at T = %d: --fpc must be %d" % (T, T))
    dev = "cuda:0"
    result = {"workload": "launches: T = %d, HO = %d, K = 8 and 64 (attn: A = %d), 8 and 64 clips; step: AlexNet(fc6) -> LSTM(256) -> avg | "
                          "vlad(%d) -> 101 classes, %d clips x %d frames 227x227, one GPU, synthetic data" % (T, HO, A, K_STEP, args.clips, args.fpc),
              "device": torch.cuda.get_device_name(0), "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
              "check": "step(vlad) - step(avg) <= sum of the eight added launches alone + spread between rounds of the vlad step's run (max - "
                       "min of its per-round means; the avg run's spread and what the wider head costs, head_extra_us, are recorded, not "
                       "added), fp32 and bf16"}
    result["launches_alone"] = {"clips_%d" % c: launches_alone(c, args.launch_rounds, args.batch, dev) for c in (8, 64)}
    ok = True
    if not args.no_step:
        result["steps"], result["verdict"] = {}, {}
        # every launch measurement before the first engine exists
        added = result["added_launches_alone"] = added_alone(args.clips, args.launch_rounds, args.batch, dev)
        for m in ("f32", "bf16"):
            step = measure_step(m, args.clips, args.fpc, args.rounds, args.steps, args.warmup, dev)
            allowed = added["sum_us"] / 1e3 + step["vlad"]["spread_ms"]
            v = {"vlad_minus_avg_ms": step["vlad_minus_avg_ms"], "added_launches_ms": round(added["sum_us"] / 1e3, 4),
                 "head_extra_ms": round(added["head_extra_us"] / 1e3, 4), "spread_vlad_ms": step["vlad"]["spread_ms"], "spread_avg_ms": step["avg"]["spread_ms"], "allowed_ms": round(allowed, 3),
                 "within": step["vlad_minus_avg_ms"] <= allowed}
            ok = ok and v["within"]
            result["steps"][m], result["verdict"][m] = step, v
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    brief = {"us": {k: {d: {n: v[d][n]["us"] for n in ("vlad_k8", "vlad_k64", "attn")} for d in ("forward", "backward")}
                    for k, v in result["launches_alone"].items()}}
    if not args.no_step:
        brief["ms_per_step"] = {m: {k: result["steps"][m][k]["ms_per_step"] for k in ORDER} for m in result["steps"]}
        brief["added_us"] = dict({k: added[k]["us"] for k in ADDED}, head_extra=added["head_extra_us"])
        brief["verdict"] = result["verdict"]
    print(json.dumps(brief))
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
