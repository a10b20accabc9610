#!/usr/bin/env python3
"""What L2 weight decay costs at the benchmark geometry (64 clips x 16 frames of 227x227, AlexNet(fc6) -> LSTM(256) -> 101 classes,
fp32) on one GPU, in ONE process: the train step with plain SGD, momentum 0.9 and Adam, each without and with weight_decay 5e-4, timed
in alternation so that all six see the same box in the same state.  With decay the step's norm launch (vl_sumsq: one read of g) is
replaced by vl_l2_regularize, which over the weights reads w and g and writes g -- the traffic of vl_sgd_apply.  So the tool times the
three launches alone (device events around the launch on the engines' own buffers, in alternation) and checks

    T(vl_l2_regularize) <= 1.15 x T(vl_sgd_apply)

(15 %: the second-stage launch and the two block reductions the update does not have) and exits 1 otherwise.  The whole-step
difference between decay and none is recorded, not bounded: it is well under 1 % of the step and of the size of the spread between
rounds.  Writes profiles/weight_decay_step.json.  No CPU fallback.
usage: bench_weight_decay.py [--clips 64] [--rounds 4] [--steps 5] [--warmup 3] [--decay 0.0005] [--out profiles/weight_decay_step.json]"""
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
RULES = ["sgd", "momentum", "adam"]
ORDER = [r + s for r in RULES for s in ("", "+wd")]
LAUNCHES = ["vl_sumsq", "vl_l2_regularize", "vl_sgd_apply"]
BOUND = 1.15


def launches_alone(e, reps):
    """ms of each launch alone: device events around `reps` launches, in alternation, all three on the buffers (w, g, norm word,
    workspace) of the SGD engine with weight decay, which is done with its timed steps.  lr 0, so the weights stay; g grows by
    decay * w per vl_l2_regularize call, which changes no timing."""
    def launch(name):
        if name == "vl_sumsq":
            ops.sumsq(e.g, e.ss, e.small_ws)
        elif name == "vl_l2_regularize":
            ops.l2_regularize(e.w, e.g, e.decay, e.ss2, e.small_ws)
        else:
            ops.sgd_apply(e.w, e.g, 0.0, 10.0, e.ss)

    for name in LAUNCHES:
        launch(name)
    torch.cuda.synchronize()
    total = {name: 0.0 for name in LAUNCHES}
    for _ in range(reps):
        for name in LAUNCHES:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch(name)
            b.record()
            b.synchronize()
            total[name] += a.elapsed_time(b)
    return {name: total[name] / reps for name in LAUNCHES}


def measure(clips, fpc, rounds, steps, warmup, decay, dev):
    base = NetConfig(image_shape=(227, 227, 3), num_classes=101, fpc=fpc, dropout_keep_prob=0.5)
    rules = {"sgd": base, "momentum": dataclasses.replace(base, momentum=0.9), "adam": dataclasses.replace(base, optimizer="adam")}
    cfgs = {}
    for r in RULES:
        cfgs[r], cfgs[r + "+wd"] = rules[r], dataclasses.replace(rules[r], weight_decay=decay)
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
    for _ in range(rounds):                         # in alternation: a drift of the box's clocks hits all six alike
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
        if "reg_loss" in check:
            out[name]["reg_loss"] = round(check["reg_loss"], 4)
    plain, decayed = engines["sgd"], engines["sgd+wd"]
    count = plain.w.numel()
    weights = sum(hi - lo for lo, hi, c in decayed.decay if c > 0.0)
    alone = launches_alone(decayed, 10 * rounds * steps)        # ~0.1 ms each: ten times the steps' count steadies the mean
    nbytes = {"vl_sumsq": 4 * count, "vl_l2_regularize": 4 * (3 * weights + (count - weights)), "vl_sgd_apply": 12 * count}
    launches = {name: {"ms": round(alone[name], 4), "bytes": nbytes[name], "tb_per_s": round(nbytes[name] / alone[name] / 1e9, 3)}
                for name in LAUNCHES}
    ratio = alone["vl_l2_regularize"] / alone["vl_sgd_apply"]
    verdict = {"l2_regularize_over_sgd_apply": round(ratio, 4), "bound": BOUND, "within_bound": ratio <= BOUND,
               "l2_regularize_minus_sumsq_ms": round(alone["vl_l2_regularize"] - alone["vl_sumsq"], 4),
               "step_decay_minus_none_ms": {r: round(out[r + "+wd"]["ms_per_step"] - out[r]["ms_per_step"], 3) for r in RULES},
               "spread_ms": round(max(max(v) - min(v) for v in per_round.values()), 3), "parameters": count, "decayed_parameters": weights,
               "decay_ranges": len(decayed.decay), "launches_timed_each": 10 * rounds * steps}
    return out, launches, verdict


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--fpc", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5, help="timed steps per round (rounds x steps >= 20)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--decay", type=float, default=5e-4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weight_decay_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_weight_decay.py needs a HIP device; there is no CPU fallback")
    if args.rounds * args.steps < 20:
        raise SystemExit("at least 20 timed steps each: rounds x steps = %d" % (args.rounds * args.steps))
    if not args.decay > 0.0:
        raise SystemExit("--decay must be > 0: the tool compares a step with weight decay against one without")
    result = {"workload": "AlexNet(fc6) -> LSTM(256) -> 101 classes, %d clips x %d frames 227x227, fp32, one GPU, synthetic data" %
                          (args.clips, args.fpc),
              "device": torch.cuda.get_device_name(0), "weight_decay": args.decay,
              "bound": "T(vl_l2_regularize) <= %.2f x T(vl_sgd_apply), both alone on the same buffers in this run" % BOUND}
    steps, launches, verdict = measure(args.clips, args.fpc, args.rounds, args.steps, args.warmup, args.decay, "cuda:0")
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
