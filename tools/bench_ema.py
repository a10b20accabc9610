#!/usr/bin/env python3
"""What the exponential moving average of the weights costs at the benchmark geometry (64 clips x 16 frames of 227x227, AlexNet(fc6) ->
LSTM(256) -> 101 classes, fp32) on one GPU, in ONE process: the train step with plain SGD without and with ema_decay 0.999 (warm-up on),
timed in alternation so that both see the same box in the same state.  The added launch, vl_ema_update, reads w and reads and writes the
shadow: the three passes of vl_sgd_apply (reads w, g; writes w).  So the tool times the two launches alone (device events around the launch
on the engine's own buffers, in alternation) and checks

    T(vl_ema_update) <= 1.15 x T(vl_sgd_apply)

(the project's bound for a launch with the update's traffic) and exits 1 otherwise.  The whole-step difference is recorded against the
spread between rounds, not bounded: one 0.1 ms launch in a 33.7 ms step is of the size of that spread.  Writes profiles/ema_step.json.
No CPU fallback.
usage: bench_ema.py [--clips 64] [--rounds 4] [--steps 5] [--warmup 3] [--decay 0.999] [--out profiles/ema_step.json]"""
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
from vltf_amd.engine import LRCNEngine, NetConfig, ema_extra_bytes, ema_rate, init_params

MEAN = np.array([99.197148, 105.293620, 109.503945], np.float32)
ORDER = ["sgd", "sgd+ema"]
LAUNCHES = ["vl_sgd_apply", "vl_ema_update"]
BOUND = 1.15


def launches_alone(e, reps, rate):
    """ms of each launch alone: device events around `reps` launches, in alternation, both on the buffers of the engine with the
    average, which is done with its timed steps.  lr 0, so the weights stay; the shadow keeps moving towards them, which changes no
    timing."""
    def launch(name):
        if name == "vl_sgd_apply":
            ops.sgd_apply(e.w, e.g, 0.0, 10.0, e.ss)
        else:
            ops.ema_update(e.ema, e.w, rate)

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
    cfgs = {"sgd": base, "sgd+ema": dataclasses.replace(base, ema_decay=decay, ema_warmup=True)}
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
                     "grad_norm": round(check["grad_norm"], 4)}
    plain, averaged = engines["sgd"], engines["sgd+ema"]
    same = all(np.array_equal(a, b) for a, b in zip(plain.get_params().values(), averaged.get_params().values()))
    count = averaged.w.numel()
    lag = float((averaged.ema - averaged.w).abs().max().item())
    alone = launches_alone(averaged, 10 * rounds * steps, ema_rate(decay, False, 0))      # ~0.1 ms each: ten times the steps' count
    launches = {name: {"ms": round(alone[name], 4), "bytes": 12 * count, "tb_per_s": round(12 * count / alone[name] / 1e9, 3)}
                for name in LAUNCHES}
    ratio = alone["vl_ema_update"] / alone["vl_sgd_apply"]
    verdict = {"ema_update_over_sgd_apply": round(ratio, 4), "bound": BOUND, "within_bound": ratio <= BOUND,
               "step_ema_minus_none_ms": round(out["sgd+ema"]["ms_per_step"] - out["sgd"]["ms_per_step"], 3),
               "spread_ms": round(max(max(v) - min(v) for v in per_round.values()), 3), "parameters": count,
               "shadow_bytes": ema_extra_bytes(count), "weights_equal_the_run_without": same, "max_abs_shadow_minus_weights": lag,
               "launches_timed_each": 10 * rounds * steps}
    return out, launches, verdict


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--fpc", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5, help="timed steps per round (rounds x steps >= 20)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--decay", type=float, default=0.999)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ema.py needs a HIP device; there is no CPU fallback")
    if args.rounds * args.steps < 20:
        raise SystemExit("at least 20 timed steps each: rounds x steps = %d" % (args.rounds * args.steps))
    if not 0.0 < args.decay < 1.0:
        raise SystemExit("--decay must lie in (0, 1): the tool compares a step with the average against one without")
    result = {"workload": "AlexNet(fc6) -> LSTM(256) -> 101 classes, %d clips x %d frames 227x227, fp32, one GPU, synthetic data" %
                          (args.clips, args.fpc),
              "device": torch.cuda.get_device_name(0), "ema_decay": args.decay, "ema_warmup": True,
              "bound": "T(vl_ema_update) <= %.2f x T(vl_sgd_apply), both alone on the same buffers in this run" % BOUND}
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
