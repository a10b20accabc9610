#!/usr/bin/env python3
"""What LARS costs at the benchmark geometry (64 clips x 16 frames of 227x227, AlexNet(fc6) -> LSTM(256) -> 101 classes, fp32) on one
GPU, in ONE process.

Launches alone, on the 44.6 M floats of the LARS engine's own buffers, device events around each launch.  vl_momentum_apply and
vl_lars_apply (the launch that takes its place) alternate with each other and with nothing else: both walk the same three buffers, so
each meets what the other left in the chip's last-level cache, the same state for both (behind the read-only statistics launch an
update launch would find w and g warmer than its rival does).  The LARS vl_tensor_stats launch and vl_lars_trust, which are not part
of the comparison, then alternate in a loop of their own.  The bound is the project's one for an update launch against the launch it replaces,

    T_lars_apply <= 1.15 x T_momentum_apply

and the tool exits 1 above it.  The stats launch is vl_tensor_stats as it stands and vl_lars_trust has no predecessor: both are
recorded, not bounded.  Then the train step with momentum 0.9, without and with LARS, timed in alternation so that both see the same box
in the same state: both times, their difference and the spread between rounds are a record, nothing is asserted about them.
Writes profiles/lars_step.json.  No CPU fallback.
usage: bench_lars.py [--clips 64] [--rounds 4] [--steps 5] [--warmup 3] [--out profiles/lars_step.json]"""
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
ORDER = ["momentum", "lars"]
LAUNCHES = ["momentum_apply", "lars_apply", "lars_tensor_stats", "lars_trust"]
BOUND = 1.15
EETA = 0.001


def launches_alone(e, reps):
    """ms of each launch alone on the LARS engine's buffers, in alternation.  lr 0: the weights stay (the accumulator moves, which the
    engine, done with its timed steps, no longer needs)."""
    L = e.lars

    def launch(name):
        if name == "momentum_apply":
            ops.momentum_apply(e.w, e.g, e.mom, 0.0, e.momentum, e.nesterov, 10.0, e.ss)
        elif name == "lars_apply":
            ops.lars_apply(e.w, e.g, e.mom, L["ranges"], L["trust"], 0.0, e.momentum, e.nesterov, 10.0, e.ss)
        elif name == "lars_tensor_stats":
            ops.tensor_stats(e.w, e.g, L["segs"], L["rows"], L["ws"])
        else:
            ops.lars_trust(L["rows"], L["decays"], L["trust"], e.lars_eeta, e.lars_epsilon, 10.0, e.ss)

    for name in LAUNCHES:
        launch(name)
    torch.cuda.synchronize()
    total = {name: 0.0 for name in LAUNCHES}
    for group in (LAUNCHES[:2], LAUNCHES[2:]):    # the two update launches against each other, then the two added launches
        for _ in range(reps):
            for name in group:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                launch(name)
                b.record()
                b.synchronize()
                total[name] += a.elapsed_time(b)
    return {name: total[name] / reps for name in LAUNCHES}


def measure(clips, fpc, rounds, steps, warmup, dev):
    base = NetConfig(image_shape=(227, 227, 3), num_classes=101, fpc=fpc, dropout_keep_prob=0.5, momentum=0.9)
    cfgs = {"momentum": base, "lars": dataclasses.replace(base, lars_eeta=EETA)}
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
    e = engines["lars"]
    trust = e.lars_trust()
    out["lars"]["trust_min_max"] = [min(trust.values()), max(trust.values())]
    count = e.w.numel()
    inside = sum(hi - lo for _, lo, hi in e.lars["segs"])
    alone = launches_alone(e, 10 * rounds * steps)
    bytes_of = {"momentum_apply": 5 * 4 * count, "lars_apply": 5 * 4 * count, "lars_tensor_stats": 2 * 4 * inside}
    out["launches_alone"] = {name: {"ms": round(alone[name], 4), "launches": 10 * rounds * steps} for name in LAUNCHES}
    for name, nbytes in bytes_of.items():
        out["launches_alone"][name].update(bytes=nbytes, tb_per_s=round(nbytes / alone[name] / 1e9, 3))
    t = {name: out[name]["ms_per_step"] for name in ORDER}
    ratio = alone["lars_apply"] / alone["momentum_apply"]
    verdict = {"lars_apply_over_momentum_apply": round(ratio, 4), "bound": BOUND, "within_bound": ratio <= BOUND,
               "lars_minus_momentum_ms": round(t["lars"] - t["momentum"], 3),
               "added_launches_ms": round(alone["lars_tensor_stats"] + alone["lars_trust"] + alone["lars_apply"] - alone["momentum_apply"], 4),
               "spread_ms": round(max(max(v) - min(v) for v in per_round.values()), 3), "parameters": count,
               "trust_segments": len(e.lars["segs"]), "ranges": len(e.lars["ranges"])}
    return out, verdict


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--fpc", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5, help="timed steps per round (rounds x steps >= 20)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lars_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lars.py needs a HIP device; there is no CPU fallback")
    if args.rounds * args.steps < 20:
        raise SystemExit("at least 20 timed steps each: rounds x steps = %d" % (args.rounds * args.steps))
    result = {"workload": "AlexNet(fc6) -> LSTM(256) -> 101 classes, %d clips x %d frames 227x227, fp32, one GPU, synthetic data, "
                          "momentum 0.9, lars_eeta %g" % (args.clips, args.fpc, EETA),
              "device": torch.cuda.get_device_name(0), "bound": "T_lars_apply <= %.2f x T_momentum_apply (launches alone)" % BOUND}
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
