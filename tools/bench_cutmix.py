#!/usr/bin/env python3
"""What CutMix / VideoMix costs on one GPU, in ONE process, everything in alternation.

1. The launch alone, at the step's own geometry (64 clips x 16 frames of 227x227): the largest box a `spatial` draw gives -- every
   frame, the centred 160 x 160 square, int(227 sqrt(1 / 2)) a side, 49.7 % of the clip -- read from the device.  vl_cutmix_pairs is
   timed against vl_mixup_pairs over the same x0, vl_cutmix_pairs_s2d against vl_mixup_pairs (dtype 1) over the same packed input.
   The swap moves at most half the bytes of the blend, in row pieces; it is held to the project's standing bound for a launch,

       T(vl_cutmix_pairs) <= 1.15 x T(vl_mixup_pairs)          T(vl_cutmix_pairs_s2d) <= 1.15 x T(vl_mixup_pairs, packed bf16).

   The tool exits 1 when one of the two ratios misses the bound.

2. The step.  The train step at that geometry (AlexNet(fc6) -> LSTM(256) -> 101 classes, plain SGD), fp32 and the packed-bf16 conv
   path, without and with cutmix_alpha.  No number is fixed in advance: the difference is reported beside the added launches measured
   alone (the swap of the half box, the loss launch minus the one it replaces) and the spread between rounds of the step WITHOUT
   CutMix.  The expectation that is checked and recorded, not enforced: difference <= launches alone + spread.  (The step also writes
   six ints and one float to the device before it starts: host work, inside the difference and not inside the launches.)

Writes profiles/cutmix_step.json.  No CPU fallback.
usage: bench_cutmix.py [--clips 64] [--rounds 4] [--steps 5] [--warmup 3] [--batch 200] [--out profiles/cutmix_step.json]"""
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
from vltf_amd.engine import LRCNEngine, NetConfig, cutmix_lambda, init_params

MEAN = np.array([99.197148, 105.293620, 109.503945], np.float32)
ORDER = ["plain", "cutmix"]
BOUND = 1.15
ALPHA, SEED, MODE = 1.0, 7, "spatial"
H = W = 227
LAM = 0.7


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
    cfgs = {"plain": base, "cutmix": dataclasses.replace(base, cutmix_alpha=ALPHA, cutmix_seed=SEED, cutmix_mode=MODE)}
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

    def run(name, fetch=False):                     # CutMix draws its own box per step (a quarter of the clip on average at alpha 1)
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
    # the launches alone, over the buffer the step cuts: the swap of the half box against the blend, and the loss launch against the
    # one it replaces (the plain engine's: vl_softmax_xent)
    eng = engines["cutmix"]
    n = clips * fpc
    packed = eng.c8 and eng._xb_fed
    buf = eng.layers[0]["xb"][:n] if packed else eng.x0[:n]
    box = half_box(fpc)
    box_dev = torch.tensor(box, dtype=torch.int32, device=dev)
    lam = torch.tensor([LAM], device=dev)
    z, dz = torch.randn((clips, 101), device=dev), torch.empty((clips, 101), device=dev)
    st, ws = torch.zeros(3, device=dev), torch.zeros(3 * clips, device=dev)
    if packed:
        cut_name, conv = "vl_cutmix_pairs_s2d", eng.layers[0]["conv"]
        cut = lambda: conv.cutmix_pairs_s2d(buf, clips, fpc, box_dev)
    else:
        cut_name = "vl_cutmix_pairs"
        cut = lambda: ops.cutmix_pairs(buf, clips, fpc, (H, W), eng.x0_halo, eng.x0_phase, box_dev)
    alone = alternate({"vl_mixup_pairs": lambda: ops.mixup_pairs(buf, clips, lam), cut_name: cut,
                       "vl_softmax_xent": lambda: ops.softmax_xent(z, onehot, dz, st[:2], 1.0 / clips, ws),
                       "vl_softmax_xent_mix": lambda: ops.softmax_xent_mix(z, onehot, dz, st, 1.0 / clips, ws, 1, 0.0, 0, lam)},
                      launch_rounds, batch)
    pair_bytes = 2 * (clips // 2) * 2 * (buf.numel() // clips) * buf.element_size()       # both partners, read and written
    frac = 1.0 - cutmix_lambda(box, fpc, H, W)
    for name, nbytes in (("vl_mixup_pairs", pair_bytes), (cut_name, int(pair_bytes * frac))):
        alone[name]["bytes"] = nbytes
        alone[name]["TB_per_s"] = round(nbytes / alone[name]["us"] * 1e-6, 3)
    ratio = alone[cut_name]["us"] / alone["vl_mixup_pairs"]["us"]
    added = (alone[cut_name]["us"] + alone["vl_softmax_xent_mix"]["us"] - alone["vl_softmax_xent"]["us"]) * 1e-3
    plain = per_round["plain"]
    verdict = {"launch": cut_name, "launch_ratio_to_vl_mixup_pairs": round(ratio, 4), "within_bound": ratio <= BOUND,
               "step_with_minus_without_ms": round(out["cutmix"]["ms_per_step"] - out["plain"]["ms_per_step"], 3),
               "added_launches_alone_ms": round(added, 3), "spread_without_ms": round(max(plain) - min(plain), 3)}
    verdict["difference_within_launches_plus_spread"] = (verdict["step_with_minus_without_ms"]
                                                         <= verdict["added_launches_alone_ms"] + verdict["spread_without_ms"])
    out["cut_buffer"] = {"dtype": str(buf.dtype).replace("torch.", ""), "elements": buf.numel(), "box": list(box),
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cutmix_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cutmix.py needs a HIP device; there is no CPU fallback")
    if args.rounds * args.steps < 20:
        raise SystemExit("at least 20 timed steps each: rounds x steps = %d" % (args.rounds * args.steps))
    dev = "cuda:0"
    result = {"workload": "AlexNet(fc6) -> LSTM(256) -> 101 classes, %d clips x %d frames 227x227, one GPU, synthetic data" % (args.clips, args.fpc),
              "device": torch.cuda.get_device_name(0), "cutmix_alpha": ALPHA, "cutmix_seed": SEED, "cutmix_mode": MODE,
              "bound": "each launch ratio <= %.2f, alternating in this run" % BOUND}
    steps = {}
    for math in ("f32", "bf16"):
        steps[math] = measure_step(math, args.clips, args.fpc, args.rounds, args.steps, args.warmup, args.launch_rounds, args.batch, dev)
    result["steps"] = steps
    verdict = {"launch_ratios": {steps[m]["verdict"]["launch"]: steps[m]["verdict"]["launch_ratio_to_vl_mixup_pairs"] for m in steps},
               "bound": BOUND, "within_bound": all(steps[m]["verdict"]["within_bound"] for m in steps),
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
