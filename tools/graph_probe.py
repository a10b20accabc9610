#!/usr/bin/env python3
"""Is the train step launch-bound?  Times train_step_u8 eagerly and replayed (NetConfig(step_graph=True)) per configuration.
usage: graph_probe.py [--steps K] [--fetched F] [--reps R] [--out FILE.json] [CONFIG ...]      CONFIG = <f32|bf16>:<clips>x<frames>
(default: f32:64x16 f32:8x16 bf16:64x16 bf16:8x16 bf16:8x32).

An eager and a step_graph engine of the configuration live side by side (same parameters, same inputs); after the warm-up (the
graph engine's first step is eager, its second is captured) R rounds alternate the two, the order flipping every round.  Per round
and engine:
  * queued: K steps with fetch=False between two synchronisations -> device ms per step, and host ms to issue one step (the same K
    calls without the final synchronisation; the host can run ahead of the device here);
  * fetched: F steps with fetch=True, as run_task's loop runs them (each step synchronises and reads its loss) -> ms per step.
The replay's figures include the static-input copies, the mean's host-to-device copy and the step-state launch.  Reported: median,
min and max over the R rounds, and the one-time capture cost."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from vltf_amd.engine import LRCNEngine, NetConfig, init_params

MEAN = np.array([99.197148, 105.293620, 109.503945], np.float32)
DEFAULT = ("f32:64x16", "f32:8x16", "bf16:64x16", "bf16:8x16", "bf16:8x32")


def spread(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


def measure(math, clips, fpc, steps, fetched, reps, warmup=5):
    dev = "cuda:0"
    engines = {}
    for kind in ("eager", "replay"):
        cfg = NetConfig(image_shape=(227, 227, 3), num_classes=101, fpc=fpc, classifier="lstm", lstm_hidden=256, lstm_layers=1,
                        dropout_keep_prob=0.5, conv_math=math, step_graph=kind == "replay")
        engines[kind] = LRCNEngine(cfg, max_clips=clips, device=dev)
        engines[kind].load_params(init_params(cfg, seed=2))
    rng = np.random.default_rng(0)
    n = clips * fpc
    frames = torch.from_numpy(rng.integers(0, 256, (n, 240, 320, 3), dtype=np.uint8)).to(dev)
    cy = torch.full((n,), 6, dtype=torch.int32, device=dev)
    cx = torch.full((n,), 46, dtype=torch.int32, device=dev)
    mirror = torch.zeros(n, dtype=torch.uint8, device=dev)
    onehot = torch.zeros((clips, 101), dtype=torch.int32)
    onehot[torch.arange(clips), torch.from_numpy(rng.integers(0, 101, clips))] = 1
    onehot = onehot.to(dev)

    def step(eng, fetch):
        return eng.train_step_u8(frames, onehot, lr=1e-3, clip_norm=10.0, mean_bgr=MEAN, crop_y=cy, crop_x=cx, mirror=mirror, fetch=fetch)

    for eng in engines.values():
        for _ in range(warmup):
            step(eng, False)
    torch.cuda.synchronize()
    res = {k: dict(ms_per_step=[], host_issue_ms_per_step=[], fetched_ms_per_step=[]) for k in engines}
    last = {}
    for r in range(reps):
        for kind in (("eager", "replay") if r % 2 == 0 else ("replay", "eager")):
            eng = engines[kind]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step(eng, False)
            issue = (time.perf_counter() - t0) / steps * 1e3
            torch.cuda.synchronize()
            res[kind]["ms_per_step"].append((time.perf_counter() - t0) / steps * 1e3)
            res[kind]["host_issue_ms_per_step"].append(issue)
            t0 = time.perf_counter()
            for _ in range(fetched):
                last[kind] = step(eng, True)
            res[kind]["fetched_ms_per_step"].append((time.perf_counter() - t0) / fetched * 1e3)
    out = {k: {m: spread(v) for m, v in res[k].items()} for k in res}
    out["replay"]["capture_ms"] = round(engines["replay"].graph_capture_ms[0], 1)
    out["same_results"] = last["eager"] == last["replay"]
    for m in ("ms_per_step", "fetched_ms_per_step"):
        out["replay_over_eager_" + m] = round(out["replay"][m]["median"] / out["eager"][m]["median"], 4)
    del engines
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=list(DEFAULT))
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--fetched", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for c in args.configs:
        math, shape = c.split(":")
        clips, fpc = (int(v) for v in shape.split("x"))
        row = dict(config=c, conv_math=math, clips=clips, frames_per_clip=fpc, **measure(math, clips, fpc, args.steps, args.fetched, args.reps))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/graph_probe.py", steps=args.steps, fetched=args.fetched, reps=args.reps,
                           wgrad_stream=os.environ.get("VLTF_WGRAD_STREAM", ""), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
