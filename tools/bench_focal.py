#!/usr/bin/env python3
"""What class weights and the focal loss cost on one GPU, in ONE process.

The launch alone.  vl_softmax_xent_wf takes the place of vl_softmax_xent_ls in the train step (both with smoothing 0.1 and top_k 5 here,
so the difference is the weights and the focusing alone).  Three variants are timed against it, in alternation:

    weights      class weights, gamma 0: one more load and one more reduction, no transcendental.  Held to the project's bound for a
                 launch that takes another's place, T(vl_softmax_xent_wf) <= 1.15 x T(vl_softmax_xent_ls); the tool exits 1 when a shape
                 misses it.
    gamma        gamma 2, no weights: a powf and an expm1f per element with a label weight, and a last pass over dlogits.
    weights+gamma

The gamma variants have no bound of their own; their ratios are recorded.  Shapes: 64 x 101 (the benchmark's loss: 64 clips, 101
classes) and 1344 x 1000 (a word-level loss: 64 clips x 21 words, vocabulary 1000), both in the rows-workspace form (two kernels each).
The launches take a few microseconds, so a batch of them is timed between two device events, over several rounds.

The step.  The train step at the benchmark geometry (64 clips x 16 frames of 227x227, AlexNet(fc6) -> LSTM(256) -> 101 classes, fp32,
plain SGD) without and with both options (balanced-style weights, gamma 2), in alternation; the difference is recorded beside the launch
delta at 64 x 101 and the spread between rounds of the step WITHOUT them, not bounded.  Writes profiles/focal_step.json.  No CPU fallback.
usage: bench_focal.py [--clips 64] [--rounds 4] [--steps 5] [--warmup 3] [--batch 200] [--out profiles/focal_step.json]"""
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
ORDER = ["plain", "class_weights+focal_gamma"]
VARIANTS = ["vl_softmax_xent_ls", "weights", "gamma", "weights+gamma"]
SHAPES = [(64, 101), (1344, 1000)]
BOUND = 1.15
EPS, TOPK, GAMMA = 0.1, 5, 2.0


def class_weights(classes):
    """Weights as a long-tailed set yields them under `balanced`: N / (C n_c) for counts falling off as 1 / (1 + c)."""
    counts = 1000.0 / (1.0 + np.arange(classes))
    return (counts.sum() / (classes * counts)).astype(np.float32)


def launches_alone(rows, classes, rounds, batch, dev):
    """us per launch of vl_softmax_xent_ls and of the three variants of vl_softmax_xent_wf at rows x classes: `batch` launches between
    two device events, the four in alternation, `rounds` times; the mean over the rounds and every round's figure."""
    rng = np.random.default_rng(rows)
    z = torch.from_numpy((rng.standard_normal((rows, classes)) * 2).astype(np.float32)).to(dev)
    y = torch.zeros((rows, classes), dtype=torch.int32)
    y[torch.arange(rows), torch.from_numpy(rng.integers(0, classes, rows))] = 1
    y = y.to(dev)
    w = torch.from_numpy(class_weights(classes)).to(dev)
    dz = torch.empty_like(z)
    stats, ws = torch.zeros(3, device=dev), torch.zeros(3 * rows, device=dev)

    def launch(name):
        if name == "vl_softmax_xent_ls":
            ops.softmax_xent_ls(z, y, dz, stats, 1.0 / rows, ws, EPS, TOPK)
        else:
            ops.softmax_xent_wf(z, y, dz, stats, 1.0 / rows, ws, EPS, TOPK, w if "weights" in name else None,
                                GAMMA if "gamma" in name else 0.0)

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
    out.update(within_bound=out["weights"]["us"] / base <= BOUND, launches_per_round=batch, rounds=rounds)
    return out


def measure_step(clips, fpc, rounds, steps, warmup, dev):
    base = NetConfig(image_shape=(227, 227, 3), num_classes=101, fpc=fpc, dropout_keep_prob=0.5)
    cfgs = {"plain": base,
            "class_weights+focal_gamma": dataclasses.replace(base, class_weights=class_weights(101).tolist(), focal_gamma=GAMMA)}
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
    plain = per_round["plain"]
    verdict = {"step_with_minus_without_ms": round(out["class_weights+focal_gamma"]["ms_per_step"] - out["plain"]["ms_per_step"], 3),
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "focal_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_focal.py needs a HIP device; there is no CPU fallback")
    if args.rounds * args.steps < 20:
        raise SystemExit("at least 20 timed steps each: rounds x steps = %d" % (args.rounds * args.steps))
    dev = "cuda:0"
    result = {"workload": "AlexNet(fc6) -> LSTM(256) -> 101 classes, %d clips x %d frames 227x227, fp32, one GPU, synthetic data" %
                          (args.clips, args.fpc),
              "device": torch.cuda.get_device_name(0), "label_smoothing": EPS, "top_k": TOPK, "focal_gamma": GAMMA,
              "bound": "T(vl_softmax_xent_wf, weights only) <= %.2f x T(vl_softmax_xent_ls), rows-workspace form, alternating in this run; "
                       "the gamma variants are recorded, not bounded" % BOUND}
    launches = {"%dx%d" % s: launches_alone(s[0], s[1], args.launch_rounds, args.batch, dev) for s in SHAPES}
    steps, verdict = measure_step(args.clips, args.fpc, args.rounds, args.steps, args.warmup, dev)
    verdict["launch_ratios"] = {k: {n: v[n]["ratio"] for n in VARIANTS[1:]} for k, v in launches.items()}
    at_step = launches["64x101"]                    # the step's own loss shape: plain there is vl_softmax_xent, at most the ls launch
    verdict["launch_delta_64x101_us"] = round(at_step["weights+gamma"]["us"] - at_step["vl_softmax_xent_ls"]["us"], 3)
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
                      "launches_alone_us": {k: {n: v[n]["us"] for n in VARIANTS} for k, v in launches.items()}, "verdict": verdict}))
    if not verdict["within_bound"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
