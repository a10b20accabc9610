#!/usr/bin/env python3
"""What the dropouts of the self-attention model (sa_attn_dropout, sa_dropout, sa_drop_path) cost on one GPU, in ONE
process, everything in alternation (tools/bench_encoder_block.py's method: HIP events on the launch stream around batches of calls, the
variants taking turns, several rounds).

1. The launches alone, 64 clips x 16 frames, H = 256, F = 1024, four heads, each drop launch against ITS OWN non-drop sibling:
     mhsa_drop_fwd   vl_mhsa_drop_fwd, keep 0.9                                     against vl_mhsa_fwd
     mhsa_drop_bwd   vl_mhsa_drop_bwd, keep 0.9                                     against vl_mhsa_bwd
     ln_drop_fwd     vl_add_layer_norm_drop_fwd, keep 0.9 and path keep 0.9         against vl_add_layer_norm_fwd with the residual
   The check: each takes at most 1.15 x its sibling (the project's usual bound).  The tool exits 1 when one misses it; the miss stands
   in the JSON as measured.
     branch_grad     vl_branch_drop_grad over rows x H                              beside vl_gelu_bwd of the same element count:
   recorded, not bounded.

2. The step at the benchmark geometry (64 clips x 16 frames of 227x227, AlexNet(fc6) -> encoder block (256, F = 1024, one layer) ->
   101 classes, plain SGD), fp32 and the packed-bf16 conv path: without the options and with all three at 0.1.  Recorded with the
   spread between rounds, not bounded.

Writes profiles/encoder_dropout_step.json.  No CPU fallback.
usage: bench_encoder_dropout.py [--clips 64] [--rounds 4] [--steps 5] [--warmup 3] [--batch 100] [--launch-rounds 10] [--no-step] [--out FILE]"""
import argparse
import dataclasses
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from bench_encoder_block import BOUND, F, H, HEADS, MEAN, T, alternate
from vltf_amd import ops
from vltf_amd.engine import LRCNEngine, NetConfig, init_params

ORDER = ["encoder", "encoder_drop"]
SIBLING = {"mhsa_drop_fwd": "mhsa_fwd", "mhsa_drop_bwd": "mhsa_bwd", "ln_drop_fwd": "ln_fwd"}
KEEP, RATE = 0.9, 0.1


def launches_alone(clips, rounds, batch, dev):
    torch.manual_seed(clips)
    n = clips * T
    r = lambda *s, scale=1.0: torch.randn(*s, device=dev) * scale
    z = lambda *s: torch.zeros(*s, device=dev)
    qkv, pos, P, ctx, dctx, dqkv, dposp = r(n, 3 * H), r(HEADS, 2 * T - 1), z(clips * HEADS, T * T), z(n, H), r(n, H), z(n, 3 * H), z(clips, HEADS * (2 * T - 1))
    x, res, s, y, gamma, beta, stats = r(n, H, scale=40.0), r(n, H), z(n, H), z(n, H), r(H, scale=0.3) + 1.0, r(H, scale=0.3), z(n, 2)
    ds, dr, u, df, du = r(n, H), z(n, H), r(n * H, scale=3.0), r(n * H), z(n * H)
    att = dict(keep=KEEP, salt=ops.sa_drop_salt(0, 0, "weights"), seed=12345)
    br = dict(keep=KEEP, keep_path=KEEP, salt_elem=ops.sa_drop_salt(0, 0, "attn_branch"), salt_path=ops.sa_drop_salt(0, 0, "path"), branch=0, seed=12345)
    ops.mhsa_fwd(qkv, pos, P, ctx, clips, T, H, HEADS)             # the backward launches read the P the forward wrote (undropped in both)
    t = alternate({"mhsa_fwd": lambda: ops.mhsa_fwd(qkv, pos, P, ctx, clips, T, H, HEADS),
                   "mhsa_drop_fwd": lambda: ops.mhsa_drop_fwd(qkv, pos, P, ctx, clips, T, H, HEADS, **att),
                   "mhsa_bwd": lambda: ops.mhsa_bwd(dctx, qkv, P, dqkv, dposp, clips, T, H, HEADS),
                   "mhsa_drop_bwd": lambda: ops.mhsa_drop_bwd(dctx, qkv, P, dqkv, dposp, clips, T, H, HEADS, **att),
                   "ln_fwd": lambda: ops.add_layer_norm_fwd(x, res, s, y, gamma, beta, stats, clips, T, H),
                   "ln_drop_fwd": lambda: ops.add_layer_norm_drop_fwd(x, res, s, y, gamma, beta, stats, clips, T, H, **br),
                   "gelu_bwd": lambda: ops.gelu_bwd(df, u, du, n * H),
                   "branch_grad": lambda: ops.branch_drop_grad(ds, dr, clips, T, H, **br)}, rounds, batch)
    for name, sib in SIBLING.items():
        t[name].update(sibling=sib, over_sibling=round(t[name]["us"] / t[sib]["us"], 4), within_bound=t[name]["us"] <= BOUND * t[sib]["us"])
    t["branch_grad"].update(beside="gelu_bwd", over_gelu_bwd=round(t["branch_grad"]["us"] / t["gelu_bwd"]["us"], 4), elements=n * H)
    return t


def measure_step(conv_math, clips, fpc, rounds, steps, warmup, dev):
    base = NetConfig(image_shape=(227, 227, 3), num_classes=101, fpc=fpc, dropout_keep_prob=0.5, conv_math=conv_math, rnn_cell="mhsa",
                     sa_heads=HEADS, sa_block="encoder", sa_ffn_dim=F)
    cfgs = {"encoder": base, "encoder_drop": dataclasses.replace(base, sa_attn_dropout=RATE, sa_dropout=RATE, sa_drop_path=RATE)}
    engines = {}
    for name in ORDER:
        engines[name] = LRCNEngine(cfgs[name], max_clips=clips, device=dev)
        engines[name].load_params(init_params(cfgs[name], seed=2))
    rng = np.random.default_rng(0)
    frames = torch.from_numpy(rng.integers(0, 256, (clips * fpc, 227, 227, 3), dtype=np.uint8)).to(dev)
    onehot = torch.zeros((clips, 101), dtype=torch.int32)
    onehot[torch.arange(clips), torch.from_numpy(rng.integers(0, 101, clips))] = 1
    onehot = onehot.to(dev)
    run = lambda name: engines[name].train_step_u8(frames, onehot, lr=1e-3, clip_norm=10.0, mean_bgr=MEAN, fetch=False)
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
        out[name] = {"ms_per_step": round(ms, 3), "clips_per_s": round(clips / ms * 1e3, 1), "timed_steps": rounds * steps,
                     "ms_per_step_by_round": [round(v, 3) for v in per_round[name]],
                     "spread_ms": round(max(per_round[name]) - min(per_round[name]), 3)}
    out["drop_minus_plain_ms"] = round(out["encoder_drop"]["ms_per_step"] - out["encoder"]["ms_per_step"], 3)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encoder_dropout_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_encoder_dropout.py needs a HIP device; there is no CPU fallback")
    if args.rounds * args.steps < 20:
        raise SystemExit("at least 20 timed steps each: rounds x steps = %d" % (args.rounds * args.steps))
    dev = "cuda:0"
    result = {"workload": "launches: %d clips x %d frames, H = %d, %d heads, keep %.1f; step: AlexNet(fc6) -> encoder block(256, F = %d, one "
                          "layer) -> 101 classes, %d clips x %d frames 227x227, one GPU, synthetic data, without the options and with "
                          "sa_attn_dropout = sa_dropout = sa_drop_path = %.1f" % (args.clips, T, H, HEADS, KEEP, F, args.clips, args.fpc, RATE),
              "device": torch.cuda.get_device_name(0), "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
              "check": "each drop launch <= %.2f x its own non-drop sibling; vl_branch_drop_grad beside vl_gelu_bwd of the same element "
                       "count and the step times are recorded, not bounded" % BOUND,
              "not_measured": "data-parallel timing; hardware counters"}
    launches = launches_alone(args.clips, args.launch_rounds, args.batch, dev)
    result["launches_alone"] = launches
    ok = all(launches[n]["within_bound"] for n in SIBLING)
    result["verdict"] = {"every_launch_within_bound": ok, "over_sibling": {n: launches[n]["over_sibling"] for n in SIBLING},
                         "branch_grad_over_gelu_bwd": launches["branch_grad"]["over_gelu_bwd"]}
    if not args.no_step:
        result["steps"] = {m: measure_step(m, args.clips, args.fpc, args.rounds, args.steps, args.warmup, dev) for m in ("f32", "bf16")}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    brief = {"us": {n: launches[n]["us"] for n in launches}, "verdict": result["verdict"]}
    if not args.no_step:
        brief["ms_per_step"] = {m: {k: result["steps"][m][k]["ms_per_step"] for k in ORDER} for m in result["steps"]}
        brief["spread_ms"] = {m: {k: result["steps"][m][k]["spread_ms"] for k in ORDER} for m in result["steps"]}
    print(json.dumps(brief))
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
