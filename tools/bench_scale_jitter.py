#!/usr/bin/env python3
"""What the random resized crop costs on one GPU, in ONE process, everything in alternation.

1. The launches alone, at the step's own geometry (1024 frames of 240x320 -> 227x227, mirror flags and the mean given), in both
   layouts conv1 reads: vl_input_prep_u8 against vl_input_prep_u8_box over the engine's haloed, phase-split fp32 x0, and
   vl_input_prep_u8_s2d against vl_input_prep_u8_box_s2d over its packed space-to-depth bf16 input.  Three box sets: identity boxes
   (the crop kernel's own windows, 227x227 at the drawn offsets), full-frame boxes (240x320, the largest downscale) and boxes drawn at
   the default scale and ratio (one per clip of 16 frames).  The box kernel issues at most four source taps where the crop kernel
   issues one, and writes the same bytes:

       T(box launch) <= 4 x T(crop launch)          for every box set, in both layouts.

   The tool exits 1 when a ratio misses the bound.

2. The step.  The train step at that geometry (AlexNet(fc6) -> LSTM(256) -> 101 classes, plain SGD, 64 clips x 16 frames), fp32 and
   the packed-bf16 conv path, fed the same 240x320 frames with crop offsets (the step of before) and with drawn boxes, on ONE engine
   (the option is a keyword of the call).  Checked, and the tool exits 1 when it fails:

       T_with - T_without <= (t_box - t_crop, launches alone, drawn boxes) + 2 x the spread between the rounds of the step without.

Both sides of every check are recorded.  Writes profiles/scale_jitter_step.json.  No CPU fallback.
usage: bench_scale_jitter.py [--clips 64] [--rounds 4] [--steps 5] [--warmup 3] [--batch 100] [--out profiles/scale_jitter_step.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from vltf_amd import ops
from vltf_amd.dataset_ import CROP_RATIO, CROP_SCALE, resized_crop_boxes
from vltf_amd.engine import LRCNEngine, NetConfig, init_params

MEAN = np.array([99.197148, 105.293620, 109.503945], np.float32)
ORDER = ["crop", "box"]
BOUND = 4.0
RH, RW, H, W = 240, 320, 227, 227
SEED = 7


def alternate(launchers, rounds, batch):
    """{name: us per launch}: `batch` launches of each between two device events, the names in alternation, `rounds` times."""
    for fn in launchers.values():
        for _ in range(min(batch, 20)):
            fn()
    torch.cuda.synchronize()
    per_round = {name: [] for name in launchers}
    for _ in range(rounds):
        for name, fn in launchers.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(batch):
                fn()
            b.record()
            b.synchronize()
            per_round[name].append(a.elapsed_time(b) / batch * 1e3)
    return {name: {"us": round(sum(v) / rounds, 3), "us_by_round": [round(x, 3) for x in v]} for name, v in per_round.items()}


def box_sets(clips, fpc, cy, cx):
    n = clips * fpc
    drawn, _ = resized_crop_boxes(SEED, 0, clips, RH, RW, CROP_SCALE, CROP_RATIO, True)
    return {"identity": np.stack([cy, cx, np.full(n, H, np.int32), np.full(n, W, np.int32)], 1).astype(np.int32),
            "full_frame": np.tile(np.array([0, 0, RH, RW], np.int32), (n, 1)),
            "drawn": np.repeat(drawn, fpc, axis=0).astype(np.int32)}


def measure(conv_math, clips, fpc, rounds, steps, warmup, launch_rounds, batch, dev):
    cfg = NetConfig(image_shape=(H, W, 3), num_classes=101, fpc=fpc, dropout_keep_prob=0.5, conv_math=conv_math)
    eng = LRCNEngine(cfg, max_clips=clips, device=dev)
    eng.load_params(init_params(cfg, seed=2))
    n = clips * fpc
    rng = np.random.default_rng(0)
    frames = torch.from_numpy(rng.integers(0, 256, (n, RH, RW, 3), dtype=np.uint8)).to(dev)
    onehot = torch.zeros((clips, 101), dtype=torch.int32)
    onehot[torch.arange(clips), torch.from_numpy(rng.integers(0, 101, clips))] = 1
    onehot = onehot.to(dev)
    cy, cx = rng.integers(0, RH - H + 1, n).astype(np.int32), rng.integers(0, RW - W + 1, n).astype(np.int32)
    mirror = torch.from_numpy(np.repeat(rng.integers(0, 2, clips), fpc).astype(np.uint8)).to(dev)
    cyd, cxd = torch.from_numpy(cy).to(dev), torch.from_numpy(cx).to(dev)
    boxes = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in box_sets(clips, fpc, cy, cx).items()}
    mean = torch.from_numpy(MEAN).to(dev)

    # ---- the step, without and with the option, in alternation on the one engine
    def run(name, fetch=False):
        kw = dict(crop_y=cyd, crop_x=cxd) if name == "crop" else dict(crop_box=boxes["drawn"])
        return eng.train_step_u8(frames, onehot, lr=1e-3, clip_norm=10.0, mean_bgr=MEAN, mirror=mirror, fetch=fetch, **kw)

    for name in ORDER:
        for _ in range(warmup):
            run(name)
    torch.cuda.synchronize()
    per_round = {name: [] for name in ORDER}
    for _ in range(rounds):
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

    # ---- the launches alone, into the buffer the step feeds
    packed = bool(eng.c8)
    if packed:
        conv, xb = eng.layers[0]["conv"], eng.layers[0]["xb"][:n]
        crop_name, box_name = "vl_input_prep_u8_s2d", "vl_input_prep_u8_box_s2d"
        launchers = {crop_name: lambda: conv.input_prep_u8_s2d(frames, xb, cyd, cxd, mirror, mean)}
        for k, b in boxes.items():
            launchers["%s/%s" % (box_name, k)] = (lambda b=b: conv.input_prep_u8_box_s2d(frames, xb, b, mirror, mean))
        written = xb.numel() * xb.element_size()
    else:
        x0 = eng.x0[:n]
        crop_name, box_name = "vl_input_prep_u8", "vl_input_prep_u8_box"
        kw = dict(halo=eng.x0_halo, phase=eng.x0_phase, out_hw=(H, W))
        launchers = {crop_name: lambda: ops.input_prep_u8(frames, x0, cyd, cxd, mirror, mean, **kw)}
        for k, b in boxes.items():
            launchers["%s/%s" % (box_name, k)] = (lambda b=b: ops.input_prep_u8_box(frames, x0, b, mirror, mean, **kw))
        written = x0.numel() * x0.element_size()
    alone = alternate(launchers, launch_rounds, batch)
    for name in alone:
        alone[name]["bytes_written"] = written
        alone[name]["write_TB_per_s"] = round(written / alone[name]["us"] * 1e-6, 3)
    ratios = {k: round(alone["%s/%s" % (box_name, k)]["us"] / alone[crop_name]["us"], 4) for k in boxes}
    without = per_round["crop"]
    delta = out["box"]["ms_per_step"] - out["crop"]["ms_per_step"]
    launch_delta = (alone["%s/drawn" % box_name]["us"] - alone[crop_name]["us"]) * 1e-3
    spread = max(without) - min(without)
    verdict = {"crop_launch": crop_name, "box_launch": box_name, "launch_ratios_box_over_crop": ratios, "bound": BOUND,
               "within_bound": all(r <= BOUND for r in ratios.values()),
               "step_with_minus_without_ms": round(delta, 3), "launch_box_minus_crop_ms": round(launch_delta, 3),
               "spread_between_rounds_without_ms": round(spread, 3), "allowed_ms": round(launch_delta + 2 * spread, 3),
               "step_costs_no_more_than_its_launch": delta <= launch_delta + 2 * spread}
    out["launches_alone"] = alone
    out["verdict"] = verdict
    del eng
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--fpc", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5, help="timed steps per round (rounds x steps >= 20)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=100, help="launches between two device events")
    ap.add_argument("--launch-rounds", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scale_jitter_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scale_jitter.py needs a HIP device; there is no CPU fallback")
    if args.rounds * args.steps < 20:
        raise SystemExit("at least 20 timed steps each: rounds x steps = %d" % (args.rounds * args.steps))
    dev = "cuda:0"
    result = {"workload": "AlexNet(fc6) -> LSTM(256) -> 101 classes, %d clips x %d frames, %dx%d -> %dx%d, one GPU, synthetic data"
                          % (args.clips, args.fpc, RH, RW, H, W),
              "device": torch.cuda.get_device_name(0), "crop_scale": list(CROP_SCALE), "crop_ratio": list(CROP_RATIO), "crop_seed": SEED,
              "checks": "each box launch <= %.1f x its crop launch; step with - without <= launch box - crop + 2 x spread" % BOUND}
    steps = {}
    for math in ("f32", "bf16"):
        steps[math] = measure(math, args.clips, args.fpc, args.rounds, args.steps, args.warmup, args.launch_rounds, args.batch, dev)
    result["steps"] = steps
    ok = all(steps[m]["verdict"]["within_bound"] and steps[m]["verdict"]["step_costs_no_more_than_its_launch"] for m in steps)
    result["verdict"] = {"all_checks_hold": ok, "by_path": {m: steps[m]["verdict"] for m in steps}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"ms_per_step": {m: {k: steps[m][k]["ms_per_step"] for k in ORDER} for m in steps}, "verdict": result["verdict"]}))
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
