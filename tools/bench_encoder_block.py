#!/usr/bin/env python3
"""What the encoder block (sa_block encoder) costs on one GPU, in ONE process, everything in alternation (tools/bench_self_attention.py's
method: HIP events on the launch stream around batches of calls, the variants taking turns, several rounds).

1. The launches alone, 64 clips x 16 frames, H = 256, F = 1024, four heads:
     ln_fwd     vl_add_layer_norm_fwd with the residual (x + r stored, then the norm)      against vl_mhsa_fwd of the same shape
     gelu_fwd   vl_gelu_fwd over rows x F                                                  against vl_mhsa_fwd
     ln_bwd     vl_layer_norm_bwd with dres and the per-clip partials                      against vl_mhsa_bwd
     gelu_bwd   vl_gelu_bwd over rows x F                                                  against vl_mhsa_bwd
   The check: each new launch takes at most 1.15 x its sibling (the project's usual bound; the sibling sits at the launch floor and
   the new launches move at most 8 MB).  The tool exits 1 when a launch misses it; the miss stands in the JSON as measured.

2. The step at the benchmark geometry (64 clips x 16 frames of 227x227, AlexNet(fc6) -> temporal model (256) -> 101 classes, plain SGD),
   fp32 and the packed-bf16 conv path: GRU / plain mhsa / encoder block (one layer, F = 1024).  Recorded, not bounded.

3. The loss at the default initialisation after the warm-up steps, plain mhsa against the encoder block, in the same run.  The tool
   exits 1 unless the block's loss is finite and below the plain model's (513 on the parent): the reason the block exists.

Writes profiles/encoder_block_step.json.  No CPU fallback.
usage: bench_encoder_block.py [--clips 64] [--rounds 4] [--steps 5] [--warmup 3] [--batch 100] [--launch-rounds 10] [--no-step] [--out FILE]"""
import argparse
import dataclasses
import json
import math
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
T, H, F, HEADS = 16, 256, 1024, 4
BOUND = 1.15
ORDER = ["gru", "mhsa", "encoder"]
SIBLING = {"ln_fwd": "mhsa_fwd", "gelu_fwd": "mhsa_fwd", "ln_bwd": "mhsa_bwd", "gelu_bwd": "mhsa_bwd"}


def alternate(launchers, rounds, batch):
    """{name: us per call}: `batch` calls of each between two device events, the names in alternation, `rounds` times."""
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
    return {name: {"us": round(sum(v) / rounds, 3), "us_by_round": [round(x, 3) for x in v],
                   "spread_us": round(max(v) - min(v), 3)} for name, v in per_round.items()}


def launches_alone(clips, rounds, batch, dev):
    torch.manual_seed(clips)
    n = clips * T
    r = lambda *s, scale=1.0: torch.randn(*s, device=dev) * scale
    z = lambda *s: torch.zeros(*s, device=dev)
    qkv, pos, P, ctx, dctx, dqkv, dposp = r(n, 3 * H), r(HEADS, 2 * T - 1), z(clips * HEADS, T * T), z(n, H), r(n, H), z(n, 3 * H), z(clips, HEADS * (2 * T - 1))
    x, res, s, y, gamma, beta, stats = r(n, H, scale=40.0), r(n, H), z(n, H), z(n, H), r(H, scale=0.3) + 1.0, r(H, scale=0.3), z(n, 2)
    dy, dres, dx, part = r(n, H), r(n, H), z(n, H), z(clips, 2 * H)
    u, f, df, du = r(n, F, scale=3.0), z(n, F), r(n, F), z(n, F)     # (du apart from df: in place, 1000 calls would compound gelu')
    ops.mhsa_fwd(qkv, pos, P, ctx, clips, T, H, HEADS)             # the backward launches read what the forward ones wrote
    ops.add_layer_norm_fwd(x, res, s, y, gamma, beta, stats, clips, T, H)
    t = alternate({"mhsa_fwd": lambda: ops.mhsa_fwd(qkv, pos, P, ctx, clips, T, H, HEADS),
                   "ln_fwd": lambda: ops.add_layer_norm_fwd(x, res, s, y, gamma, beta, stats, clips, T, H),
                   "gelu_fwd": lambda: ops.gelu_fwd(u, f, n * F),
                   "mhsa_bwd": lambda: ops.mhsa_bwd(dctx, qkv, P, dqkv, dposp, clips, T, H, HEADS),
                   "ln_bwd": lambda: ops.layer_norm_bwd(dy, s, gamma, stats, dres, dx, part, clips, T, H),
                   "gelu_bwd": lambda: ops.gelu_bwd(df, u, du, n * F)}, rounds, batch)
    bytes_moved = {"ln_fwd": 4 * (4 * n * H + 2 * H + 2 * n), "ln_bwd": 4 * (4 * n * H + H + 2 * n + 2 * clips * H), "gelu_fwd": 4 * 2 * n * F,
                   "gelu_bwd": 4 * 3 * n * F}
    for name, sib in SIBLING.items():
        t[name].update(sibling=sib, over_sibling=round(t[name]["us"] / t[sib]["us"], 4), bytes=bytes_moved[name],
                       within_bound=t[name]["us"] <= BOUND * t[sib]["us"])
    return t


def measure_step(conv_math, clips, fpc, rounds, steps, warmup, dev):
    base = NetConfig(image_shape=(227, 227, 3), num_classes=101, fpc=fpc, dropout_keep_prob=0.5, conv_math=conv_math)
    cfgs = {"gru": dataclasses.replace(base, rnn_cell="gru"), "mhsa": dataclasses.replace(base, rnn_cell="mhsa", sa_heads=HEADS),
            "encoder": dataclasses.replace(base, rnn_cell="mhsa", sa_heads=HEADS, sa_block="encoder", sa_ffn_dim=F)}
    engines = {}
    for name in ORDER:
        engines[name] = LRCNEngine(cfgs[name], max_clips=clips, device=dev)
        engines[name].load_params(init_params(cfgs[name], seed=2))     # the default initialisation: nothing rescaled
    rng = np.random.default_rng(0)
    frames = torch.from_numpy(rng.integers(0, 256, (clips * fpc, 227, 227, 3), dtype=np.uint8)).to(dev)
    onehot = torch.zeros((clips, 101), dtype=torch.int32)
    onehot[torch.arange(clips), torch.from_numpy(rng.integers(0, 101, clips))] = 1
    onehot = onehot.to(dev)

    def run(name, fetch=False):
        return engines[name].train_step_u8(frames, onehot, lr=1e-3, clip_norm=10.0, mean_bgr=MEAN, fetch=fetch)

    after_warmup = {}
    for name in ORDER:
        for _ in range(warmup):
            run(name)
        after_warmup[name] = run(name, fetch=True)["loss"]              # the loss of the step behind the warm-up steps
    torch.cuda.synchronize()
    per_round = {name: [] for name in ORDER}
    for _ in range(rounds):                         # in alternation: a drift of the clocks hits all alike
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
        out[name] = {"ms_per_step": round(ms, 3), "clips_per_s": round(clips / ms * 1e3, 1), "timed_steps": rounds * steps,
                     "ms_per_step_by_round": [round(v, 3) for v in per_round[name]],
                     "spread_ms": round(max(per_round[name]) - min(per_round[name]), 3),
                     "loss_after_warmup": after_warmup[name] if math.isfinite(after_warmup[name]) else str(after_warmup[name])}
    out["encoder_minus_mhsa_ms"] = round(out["encoder"]["ms_per_step"] - out["mhsa"]["ms_per_step"], 3)
    out["encoder_minus_gru_ms"] = round(out["encoder"]["ms_per_step"] - out["gru"]["ms_per_step"], 3)
    out["encoder_loss_finite_and_below_plain"] = bool(math.isfinite(after_warmup["encoder"]) and after_warmup["encoder"] < after_warmup["mhsa"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--fpc", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5, help="timed steps per round (rounds x steps >= 20)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=100, help="calls between two device events")
    ap.add_argument("--launch-rounds", type=int, default=10)
    ap.add_argument("--no-step", action="store_true", help="the launches alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encoder_block_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_encoder_block.py needs a HIP device; there is no CPU fallback")
    if args.rounds * args.steps < 20:
        raise SystemExit("at least 20 timed steps each: rounds x steps = %d" % (args.rounds * args.steps))
    dev = "cuda:0"
    result = {"workload": "launches: %d clips x %d frames, H = %d, F = %d, %d heads; step: AlexNet(fc6) -> GRU(256) | self-attention(256, %d heads) "
                          "| encoder block(256, F = %d, one layer) -> 101 classes, %d clips x %d frames 227x227, one GPU, synthetic data"
                          % (args.clips, T, H, F, HEADS, HEADS, F, args.clips, args.fpc),
              "device": torch.cuda.get_device_name(0), "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
              "check": "each new launch <= %.2f x vl_mhsa_fwd (forward launches) / vl_mhsa_bwd (backward launches) of the same shape; the "
                       "block's loss after the warm-up steps finite and below the plain model's" % BOUND,
              "not_measured": "data-parallel timing; hardware counters"}
    launches = launches_alone(args.clips, args.launch_rounds, args.batch, dev)
    result["launches_alone"] = launches
    ok = all(launches[n]["within_bound"] for n in SIBLING)
    result["verdict"] = {"every_launch_within_bound": ok, "over_sibling": {n: launches[n]["over_sibling"] for n in SIBLING}}
    if not args.no_step:
        result["steps"] = {m: measure_step(m, args.clips, args.fpc, args.rounds, args.steps, args.warmup, dev) for m in ("f32", "bf16")}
        loss_ok = all(v["encoder_loss_finite_and_below_plain"] for v in result["steps"].values())
        result["verdict"]["encoder_loss_finite_and_below_plain"] = loss_ok
        ok = ok and loss_ok
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    brief = {"us": {n: launches[n]["us"] for n in launches}, "verdict": result["verdict"]}
    if not args.no_step:
        brief["ms_per_step"] = {m: {k: result["steps"][m][k]["ms_per_step"] for k in ORDER} for m in result["steps"]}
        brief["loss_after_warmup"] = {m: {k: result["steps"][m][k]["loss_after_warmup"] for k in ORDER} for m in result["steps"]}
    print(json.dumps(brief))
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
