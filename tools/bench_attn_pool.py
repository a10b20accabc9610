#!/usr/bin/env python3
"""What attention pooling over time (fusion attn) costs on one GPU, in ONE process, everything in alternation.

1. The launches alone, T = 16, HO = 256, A = 256, at 8 and 64 clips, HIP events on the launch stream (tools/bench_gru.py's method):
     attn  vl_attn_pool_fwd / vl_attn_pool_bwd;
     avg   vl_temporal_fusion_fwd / _bwd (method avg) at the same shape.
   Recorded, not bounded: attention does strictly more than avg (it reads h twice and writes s, alpha, du and dcp besides).

2. The launches a step with fusion attn ADDS to a step with fusion avg, each alone at the step's shape (clips x 16 rows): the projection
   u = hseq W + b, the two kernels, the kernel gradient hseq^T du, the two column sums (du for the bias, dcp for the context), dproj = du W^T and the
   add of dproj onto dout.  The three products are called as the engines call them, without a workspace: fp32 whatever the step's
   conv_math, so ONE measurement serves both steps.

3. The step.  The train step at the benchmark geometry (64 clips x 16 frames of 227x227, AlexNet(fc6) -> LSTM(256) -> 101 classes, plain
   SGD, dropout 0.5), fp32 and the packed-bf16 conv path, with fusion avg and with fusion attn (attn_dim 256), with the spread between
   rounds.

The one check, derived and not chosen: step(attn) - step(avg) <= (sum of the added launches measured alone) + (spread between rounds of
step(attn): max - min of that run's per-round means).  A step cannot cost more than the launches it adds, run one after the other.  The
spread of the avg run is recorded beside it and NOT added.  The tool exits 1 when the check fails in fp32 or on the bf16 path.

Writes profiles/attn_pool_step.json.  No CPU fallback.
usage: bench_attn_pool.py [--clips 64] [--rounds 8] [--steps 5] [--warmup 3] [--batch 100] [--launch-rounds 10] [--no-step] [--out FILE]"""
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
T, HO, A = 16, 256, 256
ORDER = ["avg", "attn"]
ADDED = ["projection", "attn_pool_fwd", "attn_pool_bwd", "kernel_grad", "colsum_du", "colsum_dcp", "dproj", "add"]


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


class Tensors:
    """The operands of every launch of fusion attn at `clips` clips."""

    def __init__(self, clips, dev):
        torch.manual_seed(clips)
        n = clips * T
        r = lambda *s, scale=1.0: torch.randn(*s, device=dev) * scale
        z = lambda *s: torch.zeros(*s, device=dev)
        self.clips, self.n = clips, n
        self.h, self.W, self.b, self.c = r(n, HO), r(HO, A, scale=HO ** -0.5), r(A, scale=0.1), r(A, scale=A ** -0.5)
        self.u, self.s, self.alpha, self.y, self.dy = z(n, A), z(n, A), z(clips, T), z(clips, HO), r(clips, HO)
        self.du, self.dh, self.dcp, self.dproj = z(n, A), z(n, HO), z(clips, A), z(n, HO)
        self.gW, self.gb, self.gc = z(HO, A), z(A), z(A)
        self.sws = torch.empty(64 * 1024, device=dev)
        ops.gemm(self.h, self.W, self.u, n, A, HO, bias=self.b)
        self.fwd()
        self.bwd()

    def fwd(self):
        ops.attn_pool_fwd(self.u, self.c, self.h, self.s, self.alpha, self.y, self.clips, T, HO, A)

    def bwd(self):
        ops.attn_pool_bwd(self.dy, self.h, self.s, self.alpha, self.c, self.du, self.dh, self.dcp, self.clips, T, HO, A)

    def added(self):
        n, clips = self.n, self.clips
        return {"projection": lambda: ops.gemm(self.h, self.W, self.u, n, A, HO, bias=self.b),
                "attn_pool_fwd": self.fwd, "attn_pool_bwd": self.bwd,
                "kernel_grad": lambda: ops.gemm(self.h, self.du, self.gW, HO, A, n, transa=True),
                "colsum_du": lambda: ops.colsum(self.du, self.gb, self.sws, n, A),
                "colsum_dcp": lambda: ops.colsum(self.dcp, self.gc, self.sws, clips, A),
                "dproj": lambda: ops.gemm(self.du, self.W, self.dproj, n, HO, A, transb=True),
                "add": lambda: ops.eltwise2(self.dh, self.dproj, self.dh, "add", n * HO)}


def launches_alone(clips, rounds, batch, dev):
    t = Tensors(clips, dev)
    yavg, dxavg = torch.zeros(clips, HO, device=dev), torch.zeros(t.n, HO, device=dev)
    fwd = alternate({"attn": t.fwd, "avg": lambda: ops.temporal_fusion_fwd(t.h, yavg, clips, T, HO, "avg")}, rounds, batch)
    bwd = alternate({"attn": t.bwd, "avg": lambda: ops.temporal_fusion_bwd(t.dy, dxavg, clips, T, HO, "avg")}, rounds, batch)
    for v in (fwd, bwd):
        v["attn_over_avg"] = round(v["attn"]["us"] / v["avg"]["us"], 3)
    return {"forward": fwd, "backward": bwd}


def added_alone(clips, rounds, batch, dev):
    res = alternate(Tensors(clips, dev).added(), rounds, batch)
    res["sum_us"] = round(sum(res[k]["us"] for k in ADDED), 3)
    return res


def measure_step(conv_math, clips, fpc, rounds, steps, warmup, dev):
    base = NetConfig(image_shape=(227, 227, 3), num_classes=101, fpc=fpc, dropout_keep_prob=0.5, conv_math=conv_math)
    cfgs = {"avg": base, "attn": dataclasses.replace(base, fusion="attn", attn_dim=A)}
    engines = {}
    for name in ORDER:
        engines[name] = LRCNEngine(cfgs[name], max_clips=clips, device=dev)
        engines[name].load_params(init_params(cfgs[name], seed=2))
    rng = np.random.default_rng(0)
    frames = torch.from_numpy(rng.integers(0, 256, (clips * fpc, 227, 227, 3), dtype=np.uint8)).to(dev)
    onehot = torch.zeros((clips, 101), dtype=torch.int32)
    onehot[torch.arange(clips), torch.from_numpy(rng.integers(0, 101, clips))] = 1
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
    out["attn_minus_avg_ms"] = round(out["attn"]["ms_per_step"] - out["avg"]["ms_per_step"], 3)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_pool_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_pool.py needs a HIP device; there is no CPU fallback")
    if args.rounds * args.steps < 20:
        raise SystemExit("at least 20 timed steps each: rounds x steps = %d" % (args.rounds * args.steps))
    if args.fpc != T:
        raise SystemExit("the added launches are measured at T = %d: --fpc must be %d" % (T, T))
    dev = "cuda:0"
    result = {"workload": "launches: T = %d, HO = %d, A = %d, 8 and 64 clips; step: AlexNet(fc6) -> LSTM(256) -> avg | attn(256) -> 101 classes, "
                          "%d clips x %d frames 227x227, one GPU, synthetic data" % (T, HO, A, args.clips, args.fpc),
              "device": torch.cuda.get_device_name(0), "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
              "check": "step(attn) - step(avg) <= sum of the added launches alone + spread between rounds of the attn step's run (max - min "
                       "of its per-round means; the avg run's spread is recorded, not added), fp32 and bf16"}
    result["launches_alone"] = {"clips_%d" % c: launches_alone(c, args.launch_rounds, args.batch, dev) for c in (8, 64)}
    ok = True
    if not args.no_step:
        result["steps"], result["verdict"] = {}, {}
        # every launch measurement before the first engine exists
        added = result["added_launches_alone"] = added_alone(args.clips, args.launch_rounds, args.batch, dev)
        for m in ("f32", "bf16"):
            step = measure_step(m, args.clips, args.fpc, args.rounds, args.steps, args.warmup, dev)
            allowed = added["sum_us"] / 1e3 + step["attn"]["spread_ms"]
            v = {"attn_minus_avg_ms": step["attn_minus_avg_ms"], "added_launches_ms": round(added["sum_us"] / 1e3, 4),
                 "spread_attn_ms": step["attn"]["spread_ms"], "spread_avg_ms": step["avg"]["spread_ms"], "allowed_ms": round(allowed, 3),
                 "within": step["attn_minus_avg_ms"] <= allowed}
            ok = ok and v["within"]
            result["steps"][m], result["verdict"][m] = step, v
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    brief = {"us": {k: {d: {n: v[d][n]["us"] for n in ("attn", "avg")} for d in ("forward", "backward")}
                    for k, v in result["launches_alone"].items()}}
    if not args.no_step:
        brief["ms_per_step"] = {m: {k: result["steps"][m][k]["ms_per_step"] for k in ORDER} for m in result["steps"]}
        brief["added_us"] = {k: added[k]["us"] for k in ADDED}
        brief["verdict"] = result["verdict"]
    print(json.dumps(brief))
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
