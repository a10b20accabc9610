#!/usr/bin/env python3
"""What the per-variable statistics cost at the benchmark geometry (64 clips x 16 frames of 227x227, AlexNet(fc6) -> LSTM(256) -> 101
classes, fp32) on one GPU, in ONE process.  vl_tensor_stats reads w and g once over the model's 44.6 M floats -- 8 bytes per element,
against the 12 of vl_l2_regularize over the weights -- and spends the difference on fp64 accumulation and 64-byte partial rows.  So the
tool times the launch alone against vl_sumsq and vl_l2_regularize (device events around each launch, in alternation, 200 launches each,
on the engine's own buffers with the model's real tables, decay 5e-4) and checks

    T(vl_tensor_stats) <= 1.15 x T(vl_l2_regularize)

and exits 1 otherwise.  The train step with the option off, at interval 1 and at interval 10 is timed in alternation too (20 steps
each); the differences are recorded next to the spread between rounds of one variant, not judged: a 0.1 ms launch in a 34 ms step is
inside that spread.  Writes profiles/tensor_stats_step.json.  No CPU fallback.
usage: bench_tensor_stats.py [--clips 64] [--rounds 4] [--steps 5] [--warmup 3] [--launches 200] [--out profiles/tensor_stats_step.json]"""
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
from vltf_amd.engine import LRCNEngine, NetConfig, decay_ranges, init_params

MEAN = np.array([99.197148, 105.293620, 109.503945], np.float32)
ORDER = ["off", "interval1", "interval10"]
INTERVAL = {"off": 0, "interval1": 1, "interval10": 10}
LAUNCHES = ["vl_sumsq", "vl_l2_regularize", "vl_tensor_stats"]
BOUND = 1.15
DECAY = 5e-4


def launches_alone(e, reps):
    """ms of each launch alone on the buffers of the interval-1 engine, which is done with its timed steps: device events around
    `reps` launches each, in alternation.  g grows by decay * w per vl_l2_regularize call, which changes no timing."""
    decay = decay_ranges(e.specs, e.plan, DECAY)
    ss2 = torch.zeros(2, device=e.dev)

    def launch(name):
        if name == "vl_sumsq":
            ops.sumsq(e.g, e.ss, e.small_ws)
        elif name == "vl_l2_regularize":
            ops.l2_regularize(e.w, e.g, decay, ss2, e.small_ws)
        else:
            ops.tensor_stats(e.w, e.g, e.stat_segs, e.stat_out, e.stat_ws)

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
    return {name: total[name] / reps for name in LAUNCHES}, decay


def measure(clips, fpc, rounds, steps, warmup, reps, dev):
    base = NetConfig(image_shape=(227, 227, 3), num_classes=101, fpc=fpc, dropout_keep_prob=0.5)
    params = init_params(base, seed=2)
    engines = {}
    for name in ORDER:
        engines[name] = LRCNEngine(dataclasses.replace(base, tensor_stats_interval=INTERVAL[name]), max_clips=clips, device=dev)
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
    out = {}
    for name in ORDER:
        ms = sum(per_round[name]) / rounds
        check = run(name, fetch=True)
        out[name] = {"ms_per_step": round(ms, 3), "clips_per_s": round(clips / ms * 1e3, 1), "timed_steps": rounds * steps,
                     "ms_per_step_by_round": [round(v, 3) for v in per_round[name]], "loss": round(check["loss"], 4),
                     "grad_norm": round(check["grad_norm"], 4)}
    e = engines["interval1"]
    stats = e.tensor_stats()
    count = e.w.numel()
    alone, decay = launches_alone(e, reps)
    weights = sum(hi - lo for lo, hi, c in decay if c > 0.0)
    chunks = ops.stat_chunk_plan(e.stat_segs)[1]
    nbytes = {"vl_sumsq": 4 * count, "vl_l2_regularize": 4 * (3 * weights + (count - weights)),
              "vl_tensor_stats": 8 * count + 2 * ops.STAT_ROW_BYTES * chunks}
    launches = {name: {"ms": round(alone[name], 4), "bytes": nbytes[name], "tb_per_s": round(nbytes[name] / alone[name] / 1e9, 3)}
                for name in LAUNCHES}
    ratio = alone["vl_tensor_stats"] / alone["vl_l2_regularize"]
    verdict = {"tensor_stats_over_l2_regularize": round(ratio, 4), "bound": BOUND, "within_bound": ratio <= BOUND,
               "tensor_stats_over_sumsq": round(alone["vl_tensor_stats"] / alone["vl_sumsq"], 4),
               "step_minus_off_ms": {n: round(out[n]["ms_per_step"] - out["off"]["ms_per_step"], 3) for n in ORDER[1:]},
               "spread_ms": round(max(max(v) - min(v) for v in per_round.values()), 3), "parameters": count, "segments": len(e.stat_segs),
               "chunks": chunks, "chunk_elements": ops.STAT_CHUNK, "workspace_bytes": e.stat_ws.numel(), "launches_timed_each": reps,
               "largest_sgd_update_ratio": max((d["sgd_update_ratio"], n) for n, d in stats.items() if d["sgd_update_ratio"] is not None),
               "smallest_sgd_update_ratio": min((d["sgd_update_ratio"], n) for n, d in stats.items() if d["sgd_update_ratio"] is not None)}
    return out, launches, verdict


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--fpc", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5, help="timed steps per round (rounds x steps >= 20)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200, help="timed launches of each kernel alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor_stats_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tensor_stats.py needs a HIP device; there is no CPU fallback")
    if args.rounds * args.steps < 20:
        raise SystemExit("at least 20 timed steps each: rounds x steps = %d" % (args.rounds * args.steps))
    result = {"workload": "AlexNet(fc6) -> LSTM(256) -> 101 classes, %d clips x %d frames 227x227, fp32, one GPU, synthetic data" %
                          (args.clips, args.fpc),
              "device": torch.cuda.get_device_name(0), "weight_decay_of_the_l2_launch": DECAY,
              "bound": "T(vl_tensor_stats) <= %.2f x T(vl_l2_regularize), both alone on the same buffers in this run" % BOUND}
    steps, launches, verdict = measure(args.clips, args.fpc, args.rounds, args.steps, args.warmup, args.launches, "cuda:0")
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
