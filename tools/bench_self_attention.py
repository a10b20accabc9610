#!/usr/bin/env python3
"""What the self-attention launches cost on one GPU, in ONE process, everything in alternation (tools/bench_gru.py's method).

1. The launches alone, T = 16, H = 256, four heads, at 8 and 64 clips, HIP events on the launch stream, forward and backward:
     mhsa   one self-attention launch (vl_mhsa_fwd / _bwd): batch x heads workgroups, a T x T problem each;
     gru    one GRU recurrence launch (vl_gru_seq_fwd / _bwd) of the same shape: a chain of T dependent steps;
     attn   one attention-pooling launch (vl_attn_pool_fwd / _bwd), HO = A = 256: the sibling pattern, one workgroup per clip.
   The check: at both batch sizes T(mhsa) <= T(gru), forward and backward.  Self-attention has no chain of T dependent steps, so losing
   to one means the kernel is mis-built.  The tool exits 1 when one of the four comparisons fails.  Everything else is recorded.

2. The step.  The train step at the benchmark geometry (64 clips x 16 frames of 227x227, AlexNet(fc6) -> classifier(256) -> 101 classes,
   plain SGD), fp32 and the packed-bf16 conv path, with the GRU and with the self-attention classifier, with the spread between rounds.
   Recorded, not bounded.

Writes profiles/self_attention_step.json.  No CPU fallback.
usage: bench_self_attention.py [--clips 64] [--rounds 4] [--steps 5] [--warmup 3] [--batch 100] [--launch-rounds 10] [--no-step] [--out FILE]"""
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
T, H, HEADS = 16, 256, 4
ORDER = ["gru", "mhsa"]
NAMES = ("mhsa", "gru", "attn")


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
    # self-attention: qkv, position bias, P, ctx; the backward reads what the forward wrote
    qkv, pos, P, ctx, dctx, dqkv, dposp = r(n, 3 * H), r(HEADS, 2 * T - 1), z(clips * HEADS, T * T), z(n, H), r(n, H), z(n, 3 * H), z(clips, HEADS * (2 * T - 1))
    # GRU: gx, recurrent kernel and bias, gates, candidate term
    ws = ops.lstm_seq_ws(clips, T, H, dev)
    gx, gk, gb, ga, gc, gh, gp = r(n, 3 * H, scale=0.5), r(H, 3 * H, scale=0.05), r(3 * H, scale=0.1), z(n, 3 * H), z(n, H), z(n, H), z(n, H)
    dgx, dgh, gd = z(n, 3 * H), z(n, 3 * H), r(n, H)
    # attention pooling: u (s in place), context, h, alpha, y
    u, c, h, s, alpha, y, dy = r(n, H), r(H, scale=H ** -0.5), r(n, H), z(n, H), z(clips, T), z(clips, H), r(clips, H)
    du, dh, dcp = z(n, H), z(n, H), z(clips, H)
    fwd = alternate({"mhsa": lambda: ops.mhsa_fwd(qkv, pos, P, ctx, clips, T, H, HEADS),
                     "gru": lambda: ops.gru_seq_fwd(gx, gk, ga, gc, gh, gp, clips, T, H, ws=ws, rb=gb),
                     "attn": lambda: ops.attn_pool_fwd(u, c, h, s, alpha, y, clips, T, H, H)}, rounds, batch)
    bwd = alternate({"mhsa": lambda: ops.mhsa_bwd(dctx, qkv, P, dqkv, dposp, clips, T, H, HEADS),
                     "gru": lambda: ops.gru_seq_bwd(gd, gk, ga, gc, gp, dgx, dgh, clips, T, H, ws=ws),
                     "attn": lambda: ops.attn_pool_bwd(dy, h, s, alpha, c, du, dh, dcp, clips, T, H, H)}, rounds, batch)
    if ops.lstm_seq_timed_out(ws):
        raise SystemExit("bench_self_attention: a GRU launch timed out waiting for its peers; the numbers would mean nothing")
    res = {}
    for name, v in (("forward", fwd), ("backward", bwd)):
        v.update(mhsa_over_gru=round(v["mhsa"]["us"] / v["gru"]["us"], 4), mhsa_over_attn=round(v["mhsa"]["us"] / v["attn"]["us"], 4),
                 not_slower_than_gru=v["mhsa"]["us"] <= v["gru"]["us"])
        res[name] = v
    return res


def measure_step(conv_math, clips, fpc, rounds, steps, warmup, dev):
    base = NetConfig(image_shape=(227, 227, 3), num_classes=101, fpc=fpc, dropout_keep_prob=0.5, conv_math=conv_math)
    cfgs = {"gru": dataclasses.replace(base, rnn_cell="gru"), "mhsa": dataclasses.replace(base, rnn_cell="mhsa", sa_heads=HEADS)}
    engines = {}
    for name in ORDER:
        engines[name] = LRCNEngine(cfgs[name], max_clips=clips, device=dev)
        engines[name].load_params(init_params(cfgs[name], seed=2))
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
                     "ms_per_step_by_round": [round(v, 3) for v in per_round[name]],
                     "spread_ms": round(max(per_round[name]) - min(per_round[name]), 3), "loss": round(check["loss"], 4),
                     "grad_norm": round(check["grad_norm"], 4)}
    out["mhsa_minus_gru_ms"] = round(out["mhsa"]["ms_per_step"] - out["gru"]["ms_per_step"], 3)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "self_attention_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_self_attention.py needs a HIP device; there is no CPU fallback")
    if args.rounds * args.steps < 20:
        raise SystemExit("at least 20 timed steps each: rounds x steps = %d" % (args.rounds * args.steps))
    dev = "cuda:0"
    result = {"workload": "launches: T = %d, H = %d, %d heads, 8 and 64 clips; step: AlexNet(fc6) -> GRU(256) | self-attention(256, %d heads) -> "
                          "101 classes, %d clips x %d frames 227x227, one GPU, synthetic data" % (T, H, HEADS, HEADS, args.clips, args.fpc),
              "device": torch.cuda.get_device_name(0), "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
              "check": "mhsa <= gru (one launch each, the same shape), forward and backward, at 8 and at 64 clips"}
    launches = {"clips_%d" % c: launches_alone(c, args.launch_rounds, args.batch, dev) for c in (8, 64)}
    result["launches_alone"] = launches
    ok = all(v[d]["not_slower_than_gru"] for v in launches.values() for d in ("forward", "backward"))
    result["verdict"] = {"mhsa_not_slower_than_gru_everywhere": ok,
                         "mhsa_over_gru": {k: {d: v[d]["mhsa_over_gru"] for d in ("forward", "backward")} for k, v in launches.items()}}
    if not args.no_step:
        result["steps"] = {m: measure_step(m, args.clips, args.fpc, args.rounds, args.steps, args.warmup, dev) for m in ("f32", "bf16")}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    brief = {"us": {k: {d: {n: v[d][n]["us"] for n in NAMES} for d in ("forward", "backward")} for k, v in launches.items()},
             "verdict": result["verdict"]}
    if not args.no_step:
        brief["ms_per_step"] = {m: {k: result["steps"][m][k]["ms_per_step"] for k in ORDER} for m in result["steps"]}
    print(json.dumps(brief))
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
