#!/usr/bin/env python3
"""What fine-tuning saves at the benchmark geometry (64 clips x 16 frames of 227x227, AlexNet(fc6) -> LSTM(256) -> 101 classes) on one
GPU, in ONE process: the full train step, the forward pass alone, and the train step with the conv stack frozen (train_from fc6) and
with the whole dcnn frozen (train_from classifier), timed in alternation so that all four see the same box in the same state; fp32 and
the packed-bf16 conv path.  Writes profiles/finetune_step.json: ms per step and clips/s of each, the conv launches each step made
(LRCNEngine.set_probe labels) and the bytes of its data-parallel exchange plan, and checks the bounds

    train_from fc6:         T <= T_fwd + 0.15 (T_full - T_fwd)
    train_from classifier:  T <= T_fwd + 0.05 (T_full - T_fwd)

(what is left of the backward -- fc6's weight gradient, the LSTM's three products and its recurrence, norm and update -- is about 5 % /
1.5 % of the full backward by the per-launch figures of DESIGN 8; the bounds leave 3x for lost overlap and launch gaps).  Exits 1 when
a bound is missed; the recorded labels then show which launch should not be there.  There is no CPU fallback.
usage: bench_finetune.py [--clips 64] [--rounds 4] [--steps 5] [--warmup 3] [--out profiles/finetune_step.json]"""
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

from vltf_amd.engine import CONV_LAYERS, LRCNEngine, NetConfig, init_params

MEAN = np.array([99.197148, 105.293620, 109.503945], np.float32)
LABELS = [c[0] + k for c in CONV_LAYERS for k in (".fwd", ".dgrad", ".wgrad")]
BOUNDS = {"train_from_fc6": 0.15, "train_from_classifier": 0.05}


def measure(math, clips, fpc, rounds, steps, warmup, dev):
    base = NetConfig(image_shape=(227, 227, 3), num_classes=101, fpc=fpc, dropout_keep_prob=0.5, conv_math=math)
    cfgs = {"full": base, "train_from_fc6": dataclasses.replace(base, train_from="fc6"),
            "train_from_classifier": dataclasses.replace(base, train_from="classifier")}
    params = init_params(base, seed=2)
    engines = {}
    for name, cfg in cfgs.items():
        engines[name] = LRCNEngine(cfg, max_clips=clips, device=dev)
        engines[name].load_params(params)
    rng = np.random.default_rng(0)
    frames = torch.from_numpy(rng.integers(0, 256, (clips * fpc, 227, 227, 3), dtype=np.uint8)).to(dev)
    onehot = torch.zeros((clips, 101), dtype=torch.int32)
    onehot[torch.arange(clips), torch.from_numpy(rng.integers(0, 101, clips))] = 1
    onehot = onehot.to(dev)

    def run(name):
        if name == "forward":
            engines["full"].forward_u8(frames, mean_bgr=MEAN)
        else:
            engines[name].train_step_u8(frames, onehot, lr=1e-3, clip_norm=10.0, mean_bgr=MEAN, fetch=False)

    order = ["full", "forward", "train_from_fc6", "train_from_classifier"]
    for name in order:
        for _ in range(warmup):
            run(name)
    torch.cuda.synchronize()
    total = {name: 0.0 for name in order}
    for _ in range(rounds):                         # in alternation: a drift of the box's clocks hits all four alike
        for name in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                run(name)
            torch.cuda.synchronize()
            total[name] += time.perf_counter() - t0
    out = {}
    for name in order:
        ms = total[name] / (rounds * steps) * 1e3
        out[name] = {"ms_per_step": round(ms, 3), "clips_per_s": round(clips / ms * 1e3, 1), "timed_steps": rounds * steps}
        if name == "forward":
            continue
        eng = engines[name]
        eng.set_probe(LABELS)
        check = eng.train_step_u8(frames, onehot, lr=1e-3, clip_norm=10.0, mean_bgr=MEAN)
        out[name]["launched"] = [l for l, _ in eng.probe_times_ms()]
        eng.set_probe(None)
        out[name].update(exchange_bytes=eng.plan.trainable_bytes(), exchange_chunks=len(eng.plan.chunks), frozen=len(eng.plan.frozen),
                         tiers=[list(t) for t in eng.plan.tiers], loss=round(check["loss"], 4), grad_norm=round(check["grad_norm"], 4))
    t_full, t_fwd = out["full"]["ms_per_step"], out["forward"]["ms_per_step"]
    ok = True
    for name, frac in BOUNDS.items():
        bound = t_fwd + frac * (t_full - t_fwd)
        out[name].update(bound_ms=round(bound, 3), backward_left=round((out[name]["ms_per_step"] - t_fwd) / (t_full - t_fwd), 4),
                         within_bound=out[name]["ms_per_step"] <= bound)
        ok = ok and out[name]["within_bound"]
    return out, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--fpc", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5, help="timed steps per round (rounds x steps >= 20)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "finetune_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_finetune.py needs a HIP device; there is no CPU fallback")
    if args.rounds * args.steps < 20:
        raise SystemExit("at least 20 timed steps each: rounds x steps = %d" % (args.rounds * args.steps))
    dev = "cuda:0"
    result = {"workload": "AlexNet(fc6) -> LSTM(256) -> 101 classes, %d clips x %d frames 227x227, one GPU, synthetic data" % (args.clips, args.fpc),
              "device": torch.cuda.get_device_name(0), "bounds": BOUNDS}
    all_ok = True
    for math in ("f32", "bf16"):
        result[math], ok = measure(math, args.clips, args.fpc, args.rounds, args.steps, args.warmup, dev)
        all_ok = all_ok and ok
    result["within_bounds"] = all_ok
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({m: {k: (v["ms_per_step"], v.get("within_bound")) for k, v in result[m].items()} for m in ("f32", "bf16")}))
    if not all_ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
