#!/usr/bin/env python3
"""What label smoothing and the top-k count cost on one GPU, in ONE process.

The launch alone.  vl_softmax_xent_ls (smoothing 0.1, top_k 5) takes the place of vl_softmax_xent in the train step, so it is held to the
project's bound for a launch that takes another's place,

    T(vl_softmax_xent_ls) <= 1.15 x T(vl_softmax_xent)

at 64 x 101 (the benchmark's loss: 64 clips, 101 classes) and at 1344 x 1000 (a word-level loss: 64 clips x 21 words, vocabulary 1000),
both in the rows-workspace form (two kernels each).  The launches take a few microseconds, so a batch of them is timed between two device
events, the two entry points in alternation, over several rounds; the tool exits 1 when a shape misses the bound.

The step.  The train step at the benchmark geometry (64 clips x 16 frames of 227x227, AlexNet(fc6) -> LSTM(256) -> 101 classes, fp32,
plain SGD) without and with the two options, in alternation; the difference is recorded against the spread between rounds of the step
WITHOUT them, not bounded.  Writes profiles/label_smoothing_step.json.  No CPU fallback.
usage: bench_label_smoothing.py [--clips 64] [--rounds 4] [--steps 5] [--warmup 3] [--batch 200] [--out profiles/label_smoothing_step.json]"""
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
ORDER = ["plain", "label_smoothing+top_k"]
LAUNCHES = ["vl_softmax_xent", "vl_softmax_xent_ls"]
SHAPES = [(64, 101), (1344, 1000)]
BOUND = 1.15
EPS, TOPK = 0.1, 5


def launches_alone(rows, classes, rounds, batch, dev):
    """us per launch of each entry point at rows x classes: `batch` launches between two device events, the two in alternation,
    `rounds` times; the mean over the rounds and every round's figure."""
    rng = np.random.default_rng(rows)
    z = torch.from_numpy((rng.standard_normal((rows, classes)) * 2).astype(np.float32)).to(dev)
    y = torch.zeros((rows, classes), dtype=torch.int32)
    y[torch.arange(rows), torch.from_numpy(rng.integers(0, classes, rows))] = 1
    y = y.to(dev)
    dz = torch.empty_like(z)
    stats, ws = torch.zeros(3, device=dev), torch.zeros(3 * rows, device=dev)

    def launch(name):
        if name == "vl_softmax_xent":
            ops.softmax_xent(z, y, dz, stats[:2], 1.0 / rows, ws)
        else:
            ops.softmax_xent_ls(z, y, dz, stats, 1.0 / rows, ws, EPS, TOPK)

    for name in LAUNCHES:
        for _ in range(batch):
            launch(name)
    torch.cuda.synchronize()
    per_round = {name: [] for name in LAUNCHES}
    for _ in range(rounds):
        for name in LAUNCHES:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(batch):
                launch(name)
            b.record()
            b.synchronize()
            per_round[name].append(a.elapsed_time(b) / batch * 1e3)
    out = {name: {"us": round(sum(v) / rounds, 3), "us_by_round": [round(x, 3) for x in v]} for name, v in per_round.items()}
    ratio = out["vl_softmax_xent_ls"]["us"] / out["vl_softmax_xent"]["us"]
    out.update(ratio=round(ratio, 4), within_bound=ratio <= BOUND, launches_per_round=batch, rounds=rounds)
    return out


def measure_step(clips, fpc, rounds, steps, warmup, dev):
    base = NetConfig(image_shape=(227, 227, 3), num_classes=101, fpc=fpc, dropout_keep_prob=0.5)
    cfgs = {"plain": base, "label_smoothing+top_k": dataclasses.replace(base, label_smoothing=EPS, top_k=TOPK)}
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
        if "topk_accuracy" in check:
            out[name]["topk_accuracy"] = check["topk_accuracy"]
    plain = per_round["plain"]
    verdict = {"step_with_minus_without_ms": round(out["label_smoothing+top_k"]["ms_per_step"] - out["plain"]["ms_per_step"], 3),
               "spread_without_ms": round(max(plain) - min(plain), 3)}
    verdict["inside_spread"] = abs(verdict["step_with_minus_without_ms"]) <= verdict["spread_without_ms"]
    return out, verdict


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--fpc", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5, help="timed steps per round (rounds x steps >= 20)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=200, help="launches between two device events")
    ap.add_argument("--launch-rounds", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_smoothing_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_label_smoothing.py needs a HIP device; there is no CPU fallback")
    if args.rounds * args.steps < 20:
        raise SystemExit("at least 20 timed steps each: rounds x steps = %d" % (args.rounds * args.steps))
    dev = "cuda:0"
    result = {"workload": "AlexNet(fc6) -> LSTM(256) -> 101 classes, %d clips x %d frames 227x227, fp32, one GPU, synthetic data" %
                          (args.clips, args.fpc),
              "device": torch.cuda.get_device_name(0), "label_smoothing": EPS, "top_k": TOPK,
              "bound": "T(vl_softmax_xent_ls) <= %.2f x T(vl_softmax_xent), rows-workspace form, alternating in this run" % BOUND}
    launches = {"%dx%d" % s: launches_alone(s[0], s[1], args.launch_rounds, args.batch, dev) for s in SHAPES}
    steps, verdict = measure_step(args.clips, args.fpc, args.rounds, args.steps, args.warmup, dev)
    verdict["launch_ratios"] = {k: v["ratio"] for k, v in launches.items()}
    verdict["bound"] = BOUND
    verdict["within_bound"] = all(v["within_bound"] for v in launches.values())
    result.update(steps)
    result["launches_alone"] = launches
    result["verdict"] = verdict
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"ms_per_step": {k: steps[k]["ms_per_step"] for k in ORDER},
                      "launches_alone_us": {k: {n: v[n]["us"] for n in LAUNCHES} for k, v in launches.items()}, "verdict": verdict}))
    if not verdict["within_bound"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
