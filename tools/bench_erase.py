#!/usr/bin/env python3
"""What random erasing costs on one GPU, in ONE process, everything in alternation.

1. The launch alone, at the step's own geometry (64 clips x 16 frames of 227x227) and tools/bench_cutmix.py's box: every frame, the
   centred 160 x 160 square, in every clip's row of the table, read from the device.  vl_erase_boxes in each mode is timed against
   vl_cutmix_pairs over the same x0 and box, vl_erase_boxes_s2d against vl_cutmix_pairs_s2d over the same packed input.  The erase
   writes the box of every clip and reads nothing, the swap reads and writes it: at most half the bytes.  Modes zero and clip are
   held to the project's standing bound for a launch,

       T(vl_erase_boxes, zero | clip) <= 1.15 x T(vl_cutmix_pairs)      T(vl_erase_boxes_s2d, zero | clip) <= 1.15 x T(vl_cutmix_pairs_s2d).

   The tool exits 1 when a bounded mode misses in either layout.  Mode pixel hashes twice per element and may be bound by the vector
   ALU: its ratio is recorded, not bounded.

2. The step.  The train step at that geometry (AlexNet(fc6) -> LSTM(256) -> 101 classes, plain SGD), fp32 and the packed-bf16 conv
   path, without and with erasing (erase_prob 1, pixel mode, the default box ranges).  Recorded beside the spread between rounds of
   the step without; not bounded.  (The step also draws and writes clips x 8 ints before it starts: host work inside the difference.)

Writes profiles/erase_step.json.  No CPU fallback.
usage: bench_erase.py [--clips 64] [--rounds 4] [--steps 5] [--warmup 3] [--batch 200] [--out profiles/erase_step.json]"""
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
from vltf_amd.engine import ERASE_MODES, LRCNEngine, NetConfig, init_params

MEAN = np.array([99.197148, 105.293620, 109.503945], np.float32)
ORDER = ["plain", "erase"]
BOUND = 1.15
BOUNDED = ("zero", "clip")
PROB, MODE, STD, SEED = 1.0, "pixel", 57.63, 7
H = W = 227


def half_box(fpc):
    side = int(H * (0.5 ** 0.5))
    lo = (H - side) // 2
    return (0, fpc, lo, lo + side, lo, lo + side)


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


def measure_step(conv_math, clips, fpc, rounds, steps, warmup, launch_rounds, batch, dev):
    base = NetConfig(image_shape=(H, W, 3), num_classes=101, fpc=fpc, dropout_keep_prob=0.5, conv_math=conv_math)
    cfgs = {"plain": base, "erase": dataclasses.replace(base, erase_prob=PROB, erase_mode=MODE, erase_std=STD, erase_seed=SEED)}
    params = init_params(base, seed=2)
    engines = {}
    for name in ORDER:
        engines[name] = LRCNEngine(cfgs[name], max_clips=clips, device=dev)
        engines[name].load_params(params)
    rng = np.random.default_rng(0)
    frames = torch.from_numpy(rng.integers(0, 256, (clips * fpc, H, W, 3), dtype=np.uint8)).to(dev)
    onehot = torch.zeros((clips, 101), dtype=torch.int32)
    onehot[torch.arange(clips), torch.from_numpy(rng.integers(0, 101, clips))] = 1
    onehot = onehot.to(dev)

    def run(name, fetch=False):                     # erasing draws its own table per step (18 % of the frame on average, every clip)
        return engines[name].train_step_u8(frames, onehot, lr=1e-3, clip_norm=10.0, mean_bgr=MEAN, fetch=fetch)

    for name in ORDER:
        for _ in range(warmup):
            run(name)
    torch.cuda.synchronize()
    per_round = {name: [] for name in ORDER}
    for _ in range(rounds):                         # in alternation: a drift of the clocks hits both alike
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
                     "grad_norm": round(check["grad_norm"], 4), "accuracy": check["accuracy"]}
    # the launches alone, over the buffer the step erases: every clip's centred box in each mode, against the swap of that box
    eng = engines["erase"]
    n = clips * fpc
    packed = eng.c8 and eng._xb_fed
    buf = eng.layers[0]["xb"][:n] if packed else eng.x0[:n]
    box = half_box(fpc)
    box_dev = torch.tensor(box, dtype=torch.int32, device=dev)
    keys = rng.integers(-2 ** 31, 2 ** 31, (clips, 2))
    table = torch.from_numpy(np.concatenate([np.tile(np.array(box, np.int64), (clips, 1)), keys], axis=1).astype(np.int32)).to(dev)
    scale = ops.erase_scale(STD)
    if packed:
        conv = eng.layers[0]["conv"]
        cut_name, erase_name = "vl_cutmix_pairs_s2d", "vl_erase_boxes_s2d"
        cut = lambda: conv.cutmix_pairs_s2d(buf, clips, fpc, box_dev)
        erase = lambda mode: (lambda: conv.erase_boxes_s2d(buf, clips, fpc, table, mode, scale))
    else:
        cut_name, erase_name = "vl_cutmix_pairs", "vl_erase_boxes"
        cut = lambda: ops.cutmix_pairs(buf, clips, fpc, (H, W), eng.x0_halo, eng.x0_phase, box_dev)
        erase = lambda mode: (lambda: ops.erase_boxes(buf, clips, fpc, (H, W), eng.x0_halo, eng.x0_phase, table, mode, scale))
    launchers = {cut_name: cut}
    for mode, name in enumerate(ERASE_MODES):
        launchers["%s[%s]" % (erase_name, name)] = erase(mode)
    alone = alternate(launchers, launch_rounds, batch)
    vol = (box[1] - box[0]) * (box[3] - box[2]) * (box[5] - box[4])
    frac = vol / float(fpc * H * W)
    clip_bytes = (buf.numel() // clips) * buf.element_size()
    alone[cut_name]["bytes"] = int(2 * (clips // 2) * 2 * clip_bytes * frac)              # both partners, read and written
    for name in ERASE_MODES:
        alone["%s[%s]" % (erase_name, name)]["bytes"] = int(clips * clip_bytes * frac)    # every clip, written
    for v in alone.values():
        v["TB_per_s"] = round(v["bytes"] / v["us"] * 1e-6, 3)
    ratios = {name: round(alone["%s[%s]" % (erase_name, name)]["us"] / alone[cut_name]["us"], 4) for name in ERASE_MODES}
    plain = per_round["plain"]
    verdict = {"launch": erase_name, "against": cut_name, "launch_ratios": ratios, "bounded_modes": list(BOUNDED),
               "within_bound": all(ratios[name] <= BOUND for name in BOUNDED),
               "step_with_minus_without_ms": round(out["erase"]["ms_per_step"] - out["plain"]["ms_per_step"], 3),
               "spread_without_ms": round(max(plain) - min(plain), 3)}
    out["erased_buffer"] = {"dtype": str(buf.dtype).replace("torch.", ""), "elements": buf.numel(), "box": list(box),
                            "box_fraction_of_the_clip": round(frac, 4)}
    out["launches_alone_at_step_sizes"] = alone
    out["verdict"] = verdict
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--fpc", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5, help="timed steps per round (rounds x steps >= 20)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=200, help="launches between two device events")
    ap.add_argument("--launch-rounds", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "erase_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_erase.py needs a HIP device; there is no CPU fallback")
    if args.rounds * args.steps < 20:
        raise SystemExit("at least 20 timed steps each: rounds x steps = %d" % (args.rounds * args.steps))
    dev = "cuda:0"
    result = {"workload": "AlexNet(fc6) -> LSTM(256) -> 101 classes, %d clips x %d frames 227x227, one GPU, synthetic data" % (args.clips, args.fpc),
              "device": torch.cuda.get_device_name(0), "erase_prob": PROB, "erase_mode": MODE, "erase_std": STD, "erase_seed": SEED,
              "bound": "launch ratio of modes %s <= %.2f in both layouts, alternating in this run; mode pixel recorded" % (" and ".join(BOUNDED), BOUND)}
    steps = {}
    for math in ("f32", "bf16"):
        steps[math] = measure_step(math, args.clips, args.fpc, args.rounds, args.steps, args.warmup, args.launch_rounds, args.batch, dev)
    result["steps"] = steps
    verdict = {"launch_ratios": {steps[m]["verdict"]["launch"]: steps[m]["verdict"]["launch_ratios"] for m in steps},
               "bound": BOUND, "bounded_modes": list(BOUNDED), "within_bound": all(steps[m]["verdict"]["within_bound"] for m in steps),
               "step": {m: steps[m]["verdict"] for m in steps}}
    result["verdict"] = verdict
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"ms_per_step": {m: {k: steps[m][k]["ms_per_step"] for k in ORDER} for m in steps}, "verdict": verdict}))
    if not verdict["within_bound"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
