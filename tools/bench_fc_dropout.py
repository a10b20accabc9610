#!/usr/bin/env python3
"""What dropout on relu(fc6) costs (NetConfig.fc_dropout_keep_prob), on one GPU, in ONE process.

Launches alone, on the benchmark geometry's fc6 tensor (1024 frames x 4096 floats): vl_fc_dropout_fwd (reads and writes y: 8 bytes an
element, and draws), vl_relu_dropout_grad (reads d and y, writes d: 12) and vl_relu_grad at the same count (the same 12), device events
around each launch, in alternation.  The tool checks

    T(vl_fc_dropout_fwd) <= 1.15 x T(vl_relu_grad)   and   T(vl_relu_dropout_grad) <= 1.15 x T(vl_relu_grad)

(15 %: the margin this project gives one launch against a comparable one, tools/bench_weight_decay.py) and exits 1 otherwise.

Whole step at 64 clips x 16 frames of 227x227, AlexNet(fc6) -> LSTM(256) -> 101 classes: keep 0.5 against off, fp32 and
conv_math "bf16", timed in alternation.  The difference is recorded beside the spread between rounds and the sum of the added launches'
isolated times, not bounded.  Writes profiles/fc_dropout_step.json.  No CPU fallback.
usage: bench_fc_dropout.py [--clips 64] [--rounds 4] [--steps 5] [--warmup 3] [--keep 0.5] [--out profiles/fc_dropout_step.json]"""
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
from vltf_amd.engine import FC_DIM, LRCNEngine, NetConfig, dropout_seed, init_params

MEAN = np.array([99.197148, 105.293620, 109.503945], np.float32)
ORDER = ["f32", "f32+drop", "bf16", "bf16+drop"]
LAUNCHES = ["vl_fc_dropout_fwd", "vl_relu_dropout_grad", "vl_relu_grad"]
BOUND = 1.15


def launches_alone(frames, keep, reps, dev):
    """ms of each launch alone on [frames, 4096] tensors of their own.  y is a ReLU output (half zeros, half positive), d a gradient;
    before every timed launch the tensor it writes is restored from a copy (untimed), so that every repetition sees the same values."""
    rng = np.random.default_rng(1)
    y0 = torch.from_numpy(np.maximum(rng.standard_normal((frames, FC_DIM)), 0).astype(np.float32)).to(dev)
    d0 = torch.from_numpy(rng.standard_normal((frames, FC_DIM)).astype(np.float32)).to(dev)
    y, d = y0.clone(), d0.clone()

    def launch(name, rep):
        if name == "vl_fc_dropout_fwd":
            ops.fc_dropout_fwd(y, keep, dropout_seed(rep), 0)
        elif name == "vl_relu_dropout_grad":
            ops.relu_dropout_grad(d, y0, keep)
        else:
            ops.relu_grad(d, y0)

    for name in LAUNCHES:
        launch(name, 0)
    torch.cuda.synchronize()
    total = {name: 0.0 for name in LAUNCHES}
    for rep in range(reps):
        for name in LAUNCHES:
            (y if name == "vl_fc_dropout_fwd" else d).copy_(y0 if name == "vl_fc_dropout_fwd" else d0)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch(name, rep)
            b.record()
            b.synchronize()
            total[name] += a.elapsed_time(b)
    return {name: total[name] / reps for name in LAUNCHES}


def measure_steps(clips, fpc, rounds, steps, warmup, keep, dev):
    base = NetConfig(image_shape=(227, 227, 3), num_classes=101, fpc=fpc, dropout_keep_prob=0.5)
    cfgs = {"f32": base, "bf16": dataclasses.replace(base, conv_math="bf16")}
    for m in ("f32", "bf16"):
        cfgs[m + "+drop"] = dataclasses.replace(cfgs[m], fc_dropout_keep_prob=keep)
    params = init_params(base, seed=2)
    engines = {}
    for name in ORDER:
        engines[name] = LRCNEngine(cfgs[name], max_clips=clips, device=dev)
        engines[name].load_params(params)
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
    for _ in range(rounds):                         # in alternation: a drift of the box's clocks hits all four alike
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
                     "ms_per_step_by_round": [round(v, 3) for v in per_round[name]], "loss": round(check["loss"], 4),
                     "grad_norm": round(check["grad_norm"], 4)}
    spread = round(max(max(v) - min(v) for v in per_round.values()), 3)
    return out, spread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--fpc", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5, help="timed steps per round (rounds x steps >= 20)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--keep", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fc_dropout_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fc_dropout.py needs a HIP device; there is no CPU fallback")
    if args.rounds * args.steps < 20:
        raise SystemExit("at least 20 timed steps each: rounds x steps = %d" % (args.rounds * args.steps))
    if not 0.0 < args.keep < 1.0:
        raise SystemExit("--keep must lie in (0, 1): the tool compares a step that drops against one that does not")
    dev, frames = "cuda:0", args.clips * args.fpc
    result = {"workload": "AlexNet(fc6) -> LSTM(256) -> 101 classes, %d clips x %d frames 227x227, one GPU, synthetic data" %
                          (args.clips, args.fpc),
              "device": torch.cuda.get_device_name(0), "fc_dropout_keep_prob": args.keep,
              "bound": "T(vl_fc_dropout_fwd) and T(vl_relu_dropout_grad) <= %.2f x T(vl_relu_grad), each alone at %d x %d floats in this run" %
                       (BOUND, frames, FC_DIM)}
    reps = 10 * args.rounds * args.steps                          # ~0.01 ms each: ten times the steps' count steadies the mean
    alone = launches_alone(frames, args.keep, reps, dev)
    count = frames * FC_DIM
    nbytes = {"vl_fc_dropout_fwd": 8 * count, "vl_relu_dropout_grad": 12 * count, "vl_relu_grad": 12 * count}
    launches = {name: {"ms": round(alone[name], 4), "bytes": nbytes[name], "tb_per_s": round(nbytes[name] / alone[name] / 1e9, 3)}
                for name in LAUNCHES}
    steps, spread = measure_steps(args.clips, args.fpc, args.rounds, args.steps, args.warmup, args.keep, dev)
    fwd, grad = alone["vl_fc_dropout_fwd"] / alone["vl_relu_grad"], alone["vl_relu_dropout_grad"] / alone["vl_relu_grad"]
    # what the option adds to an fc6 step with everything trained: one forward launch, and one gradient launch where the LSTM's
    # input-gradient GEMM applied ReluGrad in its epilogue (fp32) or a vl_relu_grad launch ran (bf16 path: replaced, not added)
    added = {"f32": alone["vl_fc_dropout_fwd"] + alone["vl_relu_dropout_grad"],
             "bf16": alone["vl_fc_dropout_fwd"] + alone["vl_relu_dropout_grad"] - alone["vl_relu_grad"]}
    verdict = {"fc_dropout_fwd_over_relu_grad": round(fwd, 4), "relu_dropout_grad_over_relu_grad": round(grad, 4), "bound": BOUND,
               "within_bound": fwd <= BOUND and grad <= BOUND,
               "step_drop_minus_none_ms": {m: round(steps[m + "+drop"]["ms_per_step"] - steps[m]["ms_per_step"], 3) for m in ("f32", "bf16")},
               "added_launches_alone_ms": {m: round(v, 4) for m, v in added.items()}, "spread_ms": spread, "elements": count,
               "launches_timed_each": reps}
    result.update(steps)
    result["launches_alone"] = launches
    result["verdict"] = verdict
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"ms_per_step": {k: steps[k]["ms_per_step"] for k in ORDER}, "launches_alone_ms": {k: launches[k]["ms"] for k in LAUNCHES},
                      "verdict": verdict}))
    if not verdict["within_bound"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
