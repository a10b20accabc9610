#!/usr/bin/env python3
"""What LAMB costs at the benchmark geometry (64 clips x 16 frames of 227x227, AlexNet(fc6) -> LSTM(256) -> 101 classes, fp32) on one
GPU, in ONE process.

Launches alone, on the 44.6 M floats of the LAMB engine's own buffers, device events around each launch.  Two comparisons, each against a
launch of no less traffic, the two launches of a pair alternating with each other and with nothing else (both walk the same buffers, so
each meets what the other left in the chip's last-level cache, the same state for both):

    vl_lamb_moments (6 floats per element)  against  vl_adam_apply     (7 floats)
    vl_lamb_apply   (4 floats per element)  against  vl_momentum_apply (5 floats)

The bound is the project's one for a launch of no more traffic than its reference, T <= 1.15 x T(reference launch), for both pairs; the
tool exits 1 above it.  Then the train step with optimizer adam, without and with lamb, timed in alternation so that both see the same
box in the same state: both times, their difference and the spread between rounds are a record, nothing is asserted about them.
Writes profiles/lamb_step.json.  No CPU fallback.
usage: bench_lamb.py [--clips 64] [--rounds 4] [--steps 5] [--warmup 3] [--out profiles/lamb_step.json]"""
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
from vltf_amd.engine import LRCNEngine, NetConfig, init_params, lamb_corrections

MEAN = np.array([99.197148, 105.293620, 109.503945], np.float32)
ORDER = ["adam", "lamb"]
PAIRS = [("adam_apply", "lamb_moments"), ("momentum_apply", "lamb_apply")]
LAUNCHES = [name for pair in PAIRS for name in pair]
FLOATS = {"adam_apply": 7, "lamb_moments": 6, "momentum_apply": 5, "lamb_apply": 4}
BOUND = 1.15
WD = 0.01


def launches_alone(e, reps):
    """ms of each launch alone on the LAMB engine's buffers, in alternation inside its pair.  lr 0: the weights stay (the moments move,
    which the engine, done with its timed steps, no longer needs); the momentum launch gets an accumulator of its own."""
    L = e.lamb
    accum = torch.zeros_like(e.w)
    c1, c2 = lamb_corrections(e.step_count)

    def launch(name):
        if name == "adam_apply":
            ops.adam_apply(e.w, e.g, e.adam_m, e.adam_v, 0.0, e.step_count + 1, 10.0, e.ss)
        elif name == "lamb_moments":
            ops.lamb_moments(e.w, e.g, e.adam_m, e.adam_v, L["ranges"], L["rows"], L["trust"], L["ws"], c1, c2, e.lamb_epsilon, 10.0, e.ss)
        elif name == "momentum_apply":
            ops.momentum_apply(e.w, e.g, accum, 0.0, 0.9, False, 10.0, e.ss)
        else:
            ops.lamb_apply(e.w, e.adam_m, e.adam_v, L["ranges"], L["trust"], 0.0, c1, c2, e.lamb_epsilon)

    for name in LAUNCHES:
        launch(name)
    torch.cuda.synchronize()
    total = {name: 0.0 for name in LAUNCHES}
    for pair in PAIRS:
        for _ in range(reps):
            for name in pair:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                launch(name)
                b.record()
                b.synchronize()
                total[name] += a.elapsed_time(b)
    return {name: total[name] / reps for name in LAUNCHES}


def measure(clips, fpc, rounds, steps, warmup, dev):
    base = NetConfig(image_shape=(227, 227, 3), num_classes=101, fpc=fpc, dropout_keep_prob=0.5, optimizer="adam")
    cfgs = {"adam": base, "lamb": dataclasses.replace(base, lamb=True, weight_decay=WD)}
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
        return engines[name].train_step_u8(frames, onehot, lr=1e-4, clip_norm=10.0, mean_bgr=MEAN, fetch=fetch)

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
                     "grad_norm": round(check["grad_norm"], 4)}
    e = engines["lamb"]
    trust = e.lamb_trust()
    out["lamb"]["trust_min_max"] = [min(trust.values()), max(trust.values())]
    count = e.w.numel()
    reps = 10 * rounds * steps
    alone = launches_alone(e, reps)
    out["launches_alone"] = {name: {"ms": round(alone[name], 4), "launches": reps, "bytes": FLOATS[name] * 4 * count,
                                    "tb_per_s": round(FLOATS[name] * 4 * count / alone[name] / 1e9, 3)} for name in LAUNCHES}
    t = {name: out[name]["ms_per_step"] for name in ORDER}
    r_m, r_a = alone["lamb_moments"] / alone["adam_apply"], alone["lamb_apply"] / alone["momentum_apply"]
    verdict = {"lamb_moments_over_adam_apply": round(r_m, 4), "lamb_apply_over_momentum_apply": round(r_a, 4), "bound": BOUND,
               "within_bound": r_m <= BOUND and r_a <= BOUND,
               "lamb_launches_over_adam_apply": round((alone["lamb_moments"] + alone["lamb_apply"]) / alone["adam_apply"], 4),
               "lamb_minus_adam_ms": round(t["lamb"] - t["adam"], 3),
               "added_launches_ms": round(alone["lamb_moments"] + alone["lamb_apply"] - alone["adam_apply"], 4),
               "spread_ms": round(max(max(v) - min(v) for v in per_round.values()), 3), "parameters": count,
               "trust_segments": len(e.lamb["segs"]), "ranges": len(e.lamb["ranges"])}
    return out, verdict


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--fpc", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5, help="timed steps per round (rounds x steps >= 20)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lamb_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lamb.py needs a HIP device; there is no CPU fallback")
    if args.rounds * args.steps < 20:
        raise SystemExit("at least 20 timed steps each: rounds x steps = %d" % (args.rounds * args.steps))
    result = {"workload": "AlexNet(fc6) -> LSTM(256) -> 101 classes, %d clips x %d frames 227x227, fp32, one GPU, synthetic data, "
                          "optimizer adam, lamb with weight_decay %g" % (args.clips, args.fpc, WD),
              "device": torch.cuda.get_device_name(0),
              "bound": "T_lamb_moments <= %.2f x T_adam_apply and T_lamb_apply <= %.2f x T_momentum_apply (launches alone)" % (BOUND, BOUND)}
    steps, verdict = measure(args.clips, args.fpc, args.rounds, args.steps, args.warmup, "cuda:0")
    result.update(steps)
    result["verdict"] = verdict
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"ms_per_step": {k: steps[k]["ms_per_step"] for k in ORDER},
                      "launches_alone_ms": {k: steps["launches_alone"][k]["ms"] for k in LAUNCHES}, "verdict": verdict}))
    if not verdict["within_bound"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
