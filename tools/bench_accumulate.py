#!/usr/bin/env python3
"""What gradient accumulation costs and buys at the benchmark's layer shapes (AlexNet(fc6) -> LSTM(256) -> 101 classes, 16-frame clips
of 227x227, fp32) on one GPU, in ONE process.  Four measurements:

  launch alone   vl_grad_accumulate in store, add and final mode on the engine's own 44.6 M-float buffers against vl_sgd_apply on the
                 same buffers, device events around each launch, in alternation.  add and final move 3 floats per element like the
                 update, so they are held to the bound tools/bench_weight_decay.py holds vl_l2_regularize to:
                     T(add), T(final) <= 1.15 x T(vl_sgd_apply)        and        T(store) <= T(add)   (store moves 2 floats)
                 The tool exits 1 otherwise.
  update         16 clips per call, accumulate 4: one update of 4 micro-steps against 4 plain steps of an engine of the same geometry,
                 in alternation, the plain variant twice (its own spread is the yardstick for the difference).  Recorded, not bounded.
  memory         torch.cuda.max_memory_allocated over building an engine and running two updates: 64 clips plain against 16 clips with
                 accumulate 4 -- the same 64 clips per update.
  not measured   data-parallel timing: one GPU per run.

Writes profiles/accumulate_step.json.  No CPU fallback.
usage: bench_accumulate.py [--clips 16] [--k 4] [--rounds 4] [--updates 5] [--warmup 2] [--out profiles/accumulate_step.json]"""
import argparse
import dataclasses
import gc
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
LAUNCHES = ["store", "add", "final", "vl_sgd_apply"]
ORDER = ["plain_a", "accumulate", "plain_b"]
BOUND = 1.15


def batch(clips, fpc, dev, seed=0):
    rng = np.random.default_rng(seed)
    frames = torch.from_numpy(rng.integers(0, 256, (clips * fpc, 227, 227, 3), dtype=np.uint8)).to(dev)
    onehot = torch.zeros((clips, 101), dtype=torch.int32)
    onehot[torch.arange(clips), torch.from_numpy(rng.integers(0, 101, clips))] = 1
    return frames, onehot.to(dev)


def update(e, data, k):
    """One optimizer update of k calls on an accumulating engine (k = 1 calls on a plain one), nothing fetched."""
    if e.accumulate == 1:
        e.train_step_u8(*data, lr=1e-3, clip_norm=10.0, mean_bgr=MEAN, fetch=False)
        return
    for i in range(k):
        e.train_step_u8(*data, lr=1e-3, clip_norm=10.0, mean_bgr=MEAN, fetch=False, micro=(i, k))


def memory(cfg, params, clips, k, fpc, dev):
    """Peak bytes torch allocated, above what was live before, over building the engine and two updates of clips x k clips."""
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    e = LRCNEngine(dataclasses.replace(cfg, accumulate=k), max_clips=clips, device=dev)
    e.load_params(params)
    data = batch(clips, fpc, dev)
    for _ in range(2):
        update(e, data, k)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del e, data
    gc.collect()
    torch.cuda.empty_cache()
    return peak


def launches_alone(e, reps):
    """ms of each launch alone on the accumulating engine's w, g and gacc (lr 0: the weights stay; what g and gacc hold changes no
    timing)."""
    tiers = e._acc_tiers()

    def launch(name):
        if name == "vl_sgd_apply":
            ops.sgd_apply(e.w, e.g, 0.0, 10.0, e.ss)
        else:
            ops.grad_accumulate(e.gacc, e.g, LAUNCHES.index(name), tiers)

    ops.fill(e.g, 0.0)
    for name in LAUNCHES:
        launch(name)
    torch.cuda.synchronize()
    times = {name: [] for name in LAUNCHES}
    for _ in range(reps):
        for name in LAUNCHES:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch(name)
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    return {name: {"mean": sum(v) / reps, "median": float(np.median(v)), "min": min(v)} for name, v in times.items()}


def measure(clips, k, fpc, rounds, updates, warmup, dev):
    cfg = NetConfig(image_shape=(227, 227, 3), num_classes=101, fpc=fpc, dropout_keep_prob=0.5)
    params = init_params(cfg, seed=2)
    mem = {"plain_%d_clips" % (clips * k): memory(cfg, params, clips * k, 1, fpc, dev),
           "accumulate_%d_x_%d_clips" % (k, clips): memory(cfg, params, clips, k, fpc, dev)}
    engines = {"plain_a": LRCNEngine(cfg, max_clips=clips, device=dev),
               "accumulate": LRCNEngine(dataclasses.replace(cfg, accumulate=k), max_clips=clips, device=dev)}
    engines["plain_b"] = engines["plain_a"]              # the same engine timed twice: its own spread
    for e in engines.values():
        e.load_params(params)
    data = batch(clips, fpc, dev)

    def run(name):
        e = engines[name]
        if e.accumulate == 1:
            for _ in range(k):
                update(e, data, 1)
        else:
            update(e, data, k)

    for name in ORDER:
        for _ in range(warmup):
            run(name)
    torch.cuda.synchronize()
    per_round = {name: [] for name in ORDER}
    for _ in range(rounds):                              # in alternation: a drift of the box's clocks hits all three alike
        for name in ORDER:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(updates):
                run(name)
            torch.cuda.synchronize()
            per_round[name].append((time.perf_counter() - t0) / updates * 1e3)
    out = {name: {"ms_per_%d_calls" % k: round(sum(v) / rounds, 3), "by_round": [round(x, 3) for x in v], "timed": rounds * updates}
           for name, v in per_round.items()}
    ms = {name: sum(v) / rounds for name, v in per_round.items()}
    plain = 0.5 * (ms["plain_a"] + ms["plain_b"])
    acc = engines["accumulate"]
    count = acc.w.numel()
    reps = 10 * rounds * updates
    alone = launches_alone(acc, reps)
    nbytes = {"store": 8 * count, "add": 12 * count, "final": 12 * count, "vl_sgd_apply": 12 * count}
    launches = {name: {"ms": round(alone[name]["mean"], 4), "ms_median": round(alone[name]["median"], 4), "ms_min": round(alone[name]["min"], 4),
                       "bytes": nbytes[name], "tb_per_s": round(nbytes[name] / alone[name]["mean"] / 1e9, 3)} for name in LAUNCHES}
    sgd = alone["vl_sgd_apply"]["mean"]
    ratios = {m: alone[m]["mean"] / sgd for m in ("store", "add", "final")}
    ok = ratios["add"] <= BOUND and ratios["final"] <= BOUND and alone["store"]["mean"] <= alone["add"]["mean"]
    verdict = {"add_over_sgd_apply": round(ratios["add"], 4), "final_over_sgd_apply": round(ratios["final"], 4),
               "store_over_sgd_apply": round(ratios["store"], 4), "store_over_add": round(alone["store"]["mean"] / alone["add"]["mean"], 4),
               "bound": BOUND, "within_bound": ok, "parameters": count, "launches_timed_each": reps,
               "update_accumulate_ms": round(ms["accumulate"], 3), "update_plain_ms": round(plain, 3),
               "update_accumulate_minus_plain_ms": round(ms["accumulate"] - plain, 3),
               "update_accumulate_over_plain": round(ms["accumulate"] / plain, 4),
               "plain_a_minus_plain_b_ms": round(ms["plain_a"] - ms["plain_b"], 3),
               "spread_ms": round(max(max(v) - min(v) for v in per_round.values()), 3),
               "memory_bytes": mem, "memory_ratio": round(list(mem.values())[1] / list(mem.values())[0], 4),
               "data_parallel_timing": "not measured: one GPU per run"}
    return out, launches, verdict


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=16, help="clips per call")
    ap.add_argument("--k", type=int, default=4, help="micro-steps per update")
    ap.add_argument("--fpc", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--updates", type=int, default=5, help="timed updates per round (rounds x updates >= 20)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accumulate_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_accumulate.py needs a HIP device; there is no CPU fallback")
    if args.rounds * args.updates < 20:
        raise SystemExit("at least 20 timed updates each: rounds x updates = %d" % (args.rounds * args.updates))
    if args.k < 2:
        raise SystemExit("--k must be >= 2: the tool compares an accumulated update against plain steps")
    result = {"workload": "AlexNet(fc6) -> LSTM(256) -> 101 classes, %d clips x %d frames 227x227 per call, %d calls per update, fp32, one "
                          "GPU, synthetic data" % (args.clips, args.fpc, args.k),
              "device": torch.cuda.get_device_name(0),
              "bound": "T(vl_grad_accumulate add), T(final) <= %.2f x T(vl_sgd_apply) and T(store) <= T(add), all alone on the same "
                       "buffers in this run" % BOUND}
    steps, launches, verdict = measure(args.clips, args.k, args.fpc, args.rounds, args.updates, args.warmup, "cuda:0")
    result.update(steps)
    result["launches_alone"] = launches
    result["verdict"] = verdict
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"launches_alone_ms": {n: launches[n]["ms"] for n in LAUNCHES}, "verdict": verdict}))
    if not verdict["within_bound"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
