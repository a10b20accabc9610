#!/usr/bin/env python3
"""What the temporal-convolution launches cost on one GPU, in ONE process, everything in alternation (tools/bench_self_attention.py's
method).

1. The two launches alone against their sibling, vl_copy2d of a [rows, taps C] matrix: the copy moves the bytes cols is written with,
   and at least the bytes the backward reads.  HIP events on the launch stream, taps = 3:
     small   64 clips x 16 frames, C = 256, dilation 1 and 4: both sides sit at the launch floor; recorded, not bounded;
     large   1024 clips x 16 frames, C = 512, dilation 1: off the launch floor.  The bound is the project's 1.15 x a launch's sibling,
             forward and backward; the tool exits 1 on a miss there.

2. The step.  The train step at the benchmark geometry (64 clips x 16 frames of 227x227, AlexNet(fc6) -> classifier(256) -> 101 classes,
   plain SGD), fp32 and the packed-bf16 conv path, with the GRU, the plain self-attention layer and the convolution stack (two layers,
   three taps), with the spread between rounds, beside the sum of the added launches alone.  Recorded, not bounded.

Writes profiles/tcn_step.json.  No CPU fallback.
usage: bench_tcn.py [--clips 64] [--rounds 4] [--steps 5] [--warmup 3] [--batch 100] [--launch-rounds 10] [--no-step] [--out FILE]"""
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
T, H, LAYERS, TAPS, HEADS = 16, 256, 2, 3, 4
BOUND = 1.15
ORDER = ["gru", "mhsa", "tcn"]
SHAPES = {"small_d1": (64, 256, 1, False), "small_d4": (64, 256, 4, False), "large": (1024, 512, 1, True)}   # clips, C, dilation, bounded


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


def launches_alone(clips, C, dilation, rounds, batch, dev):
    torch.manual_seed(clips + dilation)
    n = clips * T
    x, cols, dcols, dres, dx = (torch.randn(n, w, device=dev) for w in (C, TAPS * C, TAPS * C, C, C))
    src, dst = torch.randn(n, TAPS * C, device=dev), torch.zeros(n, TAPS * C, device=dev)
    res = alternate({"cols_fwd": lambda: ops.tconv_cols_fwd(x, cols, clips, T, C, TAPS, dilation),
                     "cols_bwd": lambda: ops.tconv_cols_bwd(dcols, dres, dx, clips, T, C, TAPS, dilation),
                     "copy2d": lambda: ops.copy2d(src, dst, n, TAPS * C)}, rounds, batch)
    mib = n * TAPS * C * 4 / 2 ** 20
    res.update(rows=n, C=C, taps=TAPS, dilation=dilation, cols_MiB=round(mib, 2),
               fwd_over_copy=round(res["cols_fwd"]["us"] / res["copy2d"]["us"], 4),
               bwd_over_copy=round(res["cols_bwd"]["us"] / res["copy2d"]["us"], 4))
    return res


def measure_step(conv_math, clips, fpc, rounds, steps, warmup, dev):
    base = NetConfig(image_shape=(227, 227, 3), num_classes=101, fpc=fpc, dropout_keep_prob=0.5, conv_math=conv_math, lstm_layers=LAYERS)
    cfgs = {"gru": dataclasses.replace(base, rnn_cell="gru"), "mhsa": dataclasses.replace(base, rnn_cell="mhsa", sa_heads=HEADS),
            "tcn": dataclasses.replace(base, rnn_cell="tcn", tcn_kernel=TAPS)}
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
    for _ in range(rounds):                         # in alternation: a drift of the clocks hits all alike
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
    out["tcn_minus_gru_ms"] = round(out["tcn"]["ms_per_step"] - out["gru"]["ms_per_step"], 3)
    out["tcn_minus_mhsa_ms"] = round(out["tcn"]["ms_per_step"] - out["mhsa"]["ms_per_step"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--fpc", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5, help="timed steps per round (rounds x steps >= 20)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=100, help="calls between two device events")
    ap.add_argument("--launch-rounds", type=int, default=10)
    ap.add_argument("--no-step", action="store_true", help="the launches alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tcn_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tcn.py needs a HIP device; there is no CPU fallback")
    if args.rounds * args.steps < 20:
        raise SystemExit("at least 20 timed steps each: rounds x steps = %d" % (args.rounds * args.steps))
    dev = "cuda:0"
    result = {"workload": "launches: T = %d, taps = %d, 64 clips x C = 256 (dilation 1, 4) and 1024 clips x C = 512; step: AlexNet(fc6) -> "
                          "GRU(%d) | self-attention(%d, %d heads) | tcn(%d, k = %d), %d layers -> 101 classes, %d clips x %d frames 227x227, "
                          "one GPU, synthetic data" % (T, TAPS, H, H, HEADS, H, TAPS, LAYERS, args.clips, args.fpc),
              "device": torch.cuda.get_device_name(0), "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
              "check": "cols_fwd and cols_bwd <= %.2f x copy2d of [rows, taps C] at the large shape; the small shapes are recorded" % BOUND}
    launches = {k: launches_alone(c, C, d, args.launch_rounds, args.batch, dev) for k, (c, C, d, _) in SHAPES.items()}
    result["launches_alone"] = launches
    misses = [(k, d) for k, (_, _, _, bounded) in SHAPES.items() if bounded for d in ("fwd_over_copy", "bwd_over_copy")
              if launches[k][d] > BOUND]
    # what the model's L layers add per step: one forward and one backward launch each, at the small shape's cost
    added = LAYERS * sum(launches[k][d]["us"] for k, d in (("small_d1", "cols_fwd"), ("small_d1", "cols_bwd")))
    result["verdict"] = {"bound": BOUND, "within_bound_at_the_large_shape": not misses, "misses": ["%s %s" % m for m in misses],
                         "over_copy": {k: {d: v[d] for d in ("fwd_over_copy", "bwd_over_copy")} for k, v in launches.items()},
                         "added_launches_per_step_us": round(added, 3)}
    if not args.no_step:
        result["steps"] = {m: measure_step(m, args.clips, args.fpc, args.rounds, args.steps, args.warmup, dev) for m in ("f32", "bf16")}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    brief = {"us": {k: {n: v[n]["us"] for n in ("cols_fwd", "cols_bwd", "copy2d")} for k, v in launches.items()}, "verdict": result["verdict"]}
    if not args.no_step:
        brief["ms_per_step"] = {m: {k: result["steps"][m][k]["ms_per_step"] for k in ORDER} for m in result["steps"]}
    print(json.dumps(brief))
    if misses:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
