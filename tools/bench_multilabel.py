#!/usr/bin/env python3
"""What the multi-label loss costs on one GPU, in ONE process.

The launch alone.  vl_sigmoid_xent takes the place of vl_softmax_xent_ls in the train step of a `label_type: multiple` run.  In the
rows-workspace form (two kernels each), in alternation:

    vl_softmax_xent_ls   smoothing 0, top_k 0 -- the launch it replaces
    plain                vl_sigmoid_xent, gamma 0, no weights, no smoothing.  Held to the project's bound for a launch that takes
                         another's place, T(vl_sigmoid_xent) <= 1.15 x T(vl_softmax_xent_ls); the tool exits 1 when a shape misses it.
    weights              positive-term weights
    smoothing            eps 0.1
    mixed                lam 0.7 as a device word (the partner's label row is read)
    gamma                gamma 2: two more exponentials per element

The last four have no bound of their own; their ratios are recorded.  Shapes: 64 x 101 (the benchmark's loss: 64 clips, 101 classes)
and 1344 x 1000 (a per-step loss: 64 clips x 21 steps, 1000 classes), multi-hot labels at density 0.05.  The launches take a few
microseconds, so a batch of them is timed between two device events, over several rounds.

The step.  The train step at the benchmark geometry (64 clips x 16 frames of 227x227, AlexNet(fc6) -> LSTM(256) -> 101 classes, plain
SGD) with label_type single and multiple, in fp32 and on the packed-bf16 conv path, in alternation; the differences are recorded beside
the spread between rounds of the single step, not bounded.  Writes profiles/multilabel_step.json.  No CPU fallback.
usage: bench_multilabel.py [--clips 64] [--rounds 4] [--steps 5] [--warmup 3] [--batch 200] [--out profiles/multilabel_step.json]"""
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
ORDER = ["single", "multiple"]
MATHS = ["f32", "bf16"]
VARIANTS = ["vl_softmax_xent_ls", "plain", "weights", "smoothing", "mixed", "gamma"]
SHAPES = [(64, 101), (1344, 1000)]
BOUND = 1.15
EPS, GAMMA, LAM, DENSITY = 0.1, 2.0, 0.7, 0.05


def pos_weights(classes):
    """Weights as a long-tailed set yields them under `balanced`: (N - n_c) / n_c for counts falling off as 1 / (1 + c)."""
    counts = 1000.0 / (1.0 + np.arange(classes))
    return ((2000.0 - counts) / counts).astype(np.float32)


def launches_alone(rows, classes, rounds, batch, dev):
    """us per launch of vl_softmax_xent_ls and of the variants of vl_sigmoid_xent at rows x classes: `batch` launches between two
    device events, all in alternation, `rounds` times; the mean over the rounds and every round's figure."""
    rng = np.random.default_rng(rows)
    z = torch.from_numpy((rng.standard_normal((rows, classes)) * 2).astype(np.float32)).to(dev)
    onehot = torch.zeros((rows, classes), dtype=torch.int32)
    onehot[torch.arange(rows), torch.from_numpy(rng.integers(0, classes, rows))] = 1
    onehot = onehot.to(dev)
    multi = torch.from_numpy((rng.random((rows, classes)) < DENSITY).astype(np.int32)).to(dev)
    q = torch.from_numpy(pos_weights(classes)).to(dev)
    lam = torch.tensor([LAM], device=dev)
    dz = torch.empty_like(z)
    stats, ws = torch.zeros(3, device=dev), torch.zeros(3 * rows, device=dev)

    def launch(name):
        if name == "vl_softmax_xent_ls":
            ops.softmax_xent_ls(z, onehot, dz, stats, 1.0 / rows, ws, 0.0, 0)
        else:
            ops.sigmoid_xent(z, multi, dz, stats, 1.0 / rows, ws, EPS if name == "smoothing" else 0.0, q if name == "weights" else None,
                             GAMMA if name == "gamma" else 0.0, lam=lam if name == "mixed" else 1.0)

    for name in VARIANTS:
        for _ in range(batch):
            launch(name)
    torch.cuda.synchronize()
    per_round = {name: [] for name in VARIANTS}
    for _ in range(rounds):
        for name in VARIANTS:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(batch):
                launch(name)
            b.record()
            b.synchronize()
            per_round[name].append(a.elapsed_time(b) / batch * 1e3)
    out = {name: {"us": round(sum(v) / rounds, 3), "us_by_round": [round(x, 3) for x in v]} for name, v in per_round.items()}
    base = out["vl_softmax_xent_ls"]["us"]
    for name in VARIANTS[1:]:
        out[name]["ratio"] = round(out[name]["us"] / base, 4)
    out.update(within_bound=out["plain"]["us"] / base <= BOUND, launches_per_round=batch, rounds=rounds)
    return out


def measure_step(clips, fpc, rounds, steps, warmup, dev, math):
    base = NetConfig(image_shape=(227, 227, 3), num_classes=101, fpc=fpc, dropout_keep_prob=0.5, conv_math=math)
    cfgs = {"single": base, "multiple": dataclasses.replace(base, label_type="multiple")}
    params = init_params(base, seed=2)
    engines = {}
    for name in ORDER:
        engines[name] = LRCNEngine(cfgs[name], max_clips=clips, device=dev)
        engines[name].load_params(params)
    rng = np.random.default_rng(0)
    frames = torch.from_numpy(rng.integers(0, 256, (clips * fpc, 227, 227, 3), dtype=np.uint8)).to(dev)
    onehot = torch.zeros((clips, 101), dtype=torch.int32)
    onehot[torch.arange(clips), torch.from_numpy(rng.integers(0, 101, clips))] = 1
    multi = torch.from_numpy((rng.random((clips, 101)) < DENSITY).astype(np.int32))
    labels = {"single": onehot.to(dev), "multiple": torch.maximum(onehot, multi).to(dev)}

    def run(name, fetch=False):
        return engines[name].train_step_u8(frames, labels[name], lr=1e-3, clip_norm=10.0, mean_bgr=MEAN, fetch=fetch)

    for name in ORDER:
        for _ in range(warmup):
            run(name)
    torch.cuda.synchronize()
    per_round = {name: [] for name in ORDER}
    for _ in range(rounds):                         # in alternation: a drift of the box's clocks hits both alike
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
                     "grad_norm": round(check["grad_norm"], 4), "accuracy": check["accuracy"]}
    single = per_round["single"]
    out["multiple_minus_single_ms"] = round(out["multiple"]["ms_per_step"] - out["single"]["ms_per_step"], 3)
    out["spread_single_ms"] = round(max(single) - min(single), 3)
    out["inside_spread"] = abs(out["multiple_minus_single_ms"]) <= out["spread_single_ms"]
    del engines
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--fpc", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5, help="timed steps per round (rounds x steps >= 20)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=200, help="launches between two device events")
    ap.add_argument("--launch-rounds", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multilabel_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_multilabel.py needs a HIP device; there is no CPU fallback")
    if args.rounds * args.steps < 20:
        raise SystemExit("at least 20 timed steps each: rounds x steps = %d" % (args.rounds * args.steps))
    dev = "cuda:0"
    result = {"workload": "AlexNet(fc6) -> LSTM(256) -> 101 classes, %d clips x %d frames 227x227, one GPU, synthetic data" %
                          (args.clips, args.fpc),
              "device": torch.cuda.get_device_name(0), "label_density": DENSITY,
              "bound": "T(vl_sigmoid_xent, gamma 0, no weights, no smoothing) <= %.2f x T(vl_softmax_xent_ls), rows-workspace form, "
                       "alternating in this run; weights, smoothing, mixed labels and gamma 2 are recorded, not bounded" % BOUND}
    launches = {"%dx%d" % s: launches_alone(s[0], s[1], args.launch_rounds, args.batch, dev) for s in SHAPES}
    steps = {math: measure_step(args.clips, args.fpc, args.rounds, args.steps, args.warmup, dev, math) for math in MATHS}
    verdict = {"launch_ratios": {k: {n: v[n]["ratio"] for n in VARIANTS[1:]} for k, v in launches.items()}, "bound": BOUND,
               "within_bound": all(v["within_bound"] for v in launches.values()),
               "step_multiple_minus_single_ms": {m: steps[m]["multiple_minus_single_ms"] for m in MATHS},
               "step_spread_single_ms": {m: steps[m]["spread_single_ms"] for m in MATHS}}
    result["step"] = steps
    result["launches_alone"] = launches
    result["verdict"] = verdict
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"ms_per_step": {m: {k: steps[m][k]["ms_per_step"] for k in ORDER} for m in MATHS},
                      "launches_alone_us": {k: {n: v[n]["us"] for n in VARIANTS} for k, v in launches.items()}, "verdict": verdict}))
    if not verdict["within_bound"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
