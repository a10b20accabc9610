#!/usr/bin/env python3
"""What the momentum accumulator costs at the benchmark geometry (64 clips x 16 frames of 227x227, AlexNet(fc6) -> LSTM(256) -> 101
classes, fp32) on one GPU, in ONE process: the train step with plain SGD, with momentum 0.9 and with Adam, timed in alternation so that
all three see the same box in the same state.  Per element the update moves 3 floats with plain SGD (reads w, g; writes w), 5 with
momentum (+ the accumulator, read and written) and 7 with Adam (+ m and v), so the tool checks

    T_momentum - T_sgd <= T_adam - T_sgd

and exits 1 otherwise.  The update is well under 1 % of the step, so the step times alone say little about it: the tool also times
the three update launches by themselves (device events around the launch on the engines' own buffers, in alternation) and records
their bytes per second; those figures are a record, not part of the verdict.  Writes profiles/momentum_step.json.  No CPU fallback.
usage: bench_momentum.py [--clips 64] [--rounds 4] [--steps 5] [--warmup 3] [--out profiles/momentum_step.json]"""
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
FLOATS = {"sgd": 3, "momentum": 5, "adam": 7}        # moved per element by the update launch
ORDER = ["sgd", "momentum", "adam"]


def update_alone(engines, reps, dev):
    """ms of the update launch alone, per rule: device events around `reps` launches, the rules in alternation.  lr 0: the weights
    stay (the accumulators move, which the engines, done with their timed steps, no longer need)."""
    def launch(name):
        e = engines[name]
        if name == "sgd":
            ops.sgd_apply(e.w, e.g, 0.0, 10.0, e.ss)
        elif name == "momentum":
            ops.momentum_apply(e.w, e.g, e.mom, 0.0, e.momentum, e.nesterov, 10.0, e.ss)
        else:
            ops.adam_apply(e.w, e.g, e.adam_m, e.adam_v, 0.0, 1, 10.0, e.ss)

    for name in ORDER:
        launch(name)
    torch.cuda.synchronize()
    total = {name: 0.0 for name in ORDER}
    for _ in range(reps):
        for name in ORDER:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch(name)
            b.record()
            b.synchronize()
            total[name] += a.elapsed_time(b)
    return {name: total[name] / reps for name in ORDER}


def measure(clips, fpc, rounds, steps, warmup, dev):
    base = NetConfig(image_shape=(227, 227, 3), num_classes=101, fpc=fpc, dropout_keep_prob=0.5)
    cfgs = {"sgd": base, "momentum": dataclasses.replace(base, momentum=0.9), "adam": dataclasses.replace(base, optimizer="adam")}
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
    for _ in range(rounds):                         # in alternation: a drift of the box's clocks hits all three alike
        for name in ORDER:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                run(name)
            torch.cuda.synchronize()
            per_round[name].append((time.perf_counter() - t0) / steps * 1e3)
    count = engines["sgd"].w.numel()
    out = {}
    for name in ORDER:
        ms = sum(per_round[name]) / rounds
        check = run(name, fetch=True)
        out[name] = {"ms_per_step": round(ms, 3), "clips_per_s": round(clips / ms * 1e3, 1), "timed_steps": rounds * steps,
                     "ms_per_step_by_round": [round(v, 3) for v in per_round[name]], "loss": round(check["loss"], 4),
                     "grad_norm": round(check["grad_norm"], 4), "update_floats_per_element": FLOATS[name],
                     "update_bytes": FLOATS[name] * 4 * count}
    alone = update_alone(engines, rounds * steps, dev)
    for name in ORDER:
        out[name].update(update_alone_ms=round(alone[name], 4), update_alone_tb_per_s=round(out[name]["update_bytes"] / alone[name] / 1e9, 3))
    t = {name: out[name]["ms_per_step"] for name in ORDER}
    verdict = {"momentum_minus_sgd_ms": round(t["momentum"] - t["sgd"], 3), "adam_minus_sgd_ms": round(t["adam"] - t["sgd"], 3),
               "spread_ms": round(max(max(v) - min(v) for v in per_round.values()), 3), "parameters": count}
    verdict["within_bound"] = verdict["momentum_minus_sgd_ms"] <= verdict["adam_minus_sgd_ms"]
    return out, verdict


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--fpc", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5, help="timed steps per round (rounds x steps >= 20)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "momentum_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_momentum.py needs a HIP device; there is no CPU fallback")
    if args.rounds * args.steps < 20:
        raise SystemExit("at least 20 timed steps each: rounds x steps = %d" % (args.rounds * args.steps))
    result = {"workload": "AlexNet(fc6) -> LSTM(256) -> 101 classes, %d clips x %d frames 227x227, fp32, one GPU, synthetic data" %
                          (args.clips, args.fpc),
              "device": torch.cuda.get_device_name(0), "bound": "T_momentum - T_sgd <= T_adam - T_sgd"}
    steps, verdict = measure(args.clips, args.fpc, args.rounds, args.steps, args.warmup, "cuda:0")
    result.update(steps)
    result["verdict"] = verdict
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"ms_per_step": {k: steps[k]["ms_per_step"] for k in ORDER}, "update_alone_ms": {k: steps[k]["update_alone_ms"] for k in ORDER},
                      "verdict": verdict}))
    if not verdict["within_bound"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
