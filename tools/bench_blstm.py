#!/usr/bin/env python3
"""What the bidirectional LSTM launch costs on one GPU, in ONE process, everything in alternation.

1. The launches alone, T = 16, H = 256, at 8 and 64 clips, HIP events on the launch stream (tools/lstm_probe.py's method), forward and
   backward:
     bi    one bidirectional launch (vl_lstm_seq_bi_fwd / _bwd): both directions of a layer;
     two   two unidirectional launches back to back on the stream: what a bidirectional layer would cost without the kernel;
     one   one unidirectional launch, for the record.
   The check: at both batch sizes T(bi) < T(two), forward and backward -- the chain of T dependent steps is paid once.  The tool exits 1
   when one of the four comparisons fails.  No other ratio is bounded; bi / one is recorded.

2. The step.  The train step at the benchmark geometry (64 clips x 16 frames of 227x227, AlexNet(fc6) -> LSTM(256) -> 101 classes, plain
   SGD), fp32 and the packed-bf16 conv path, with the unidirectional and with the bidirectional classifier, with the spread between
   rounds.  Nothing is bounded: a bidirectional layer has twice the LSTM weights and products.

Writes profiles/blstm_step.json.  No CPU fallback.
usage: bench_blstm.py [--clips 64] [--rounds 4] [--steps 5] [--warmup 3] [--batch 100] [--launch-rounds 10] [--no-step] [--out FILE]"""
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
T, H = 16, 256
ORDER = ["unidirectional", "bidirectional"]


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
    return {name: {"us": round(sum(v) / rounds, 3), "us_by_round": [round(x, 3) for x in v]} for name, v in per_round.items()}


def launches_alone(clips, rounds, batch, dev):
    torch.manual_seed(clips)
    n = clips * T
    r = lambda *s, scale=1.0: torch.randn(*s, device=dev) * scale
    z = lambda *s: torch.zeros(*s, device=dev)
    gx, kh = (r(n, 4 * H, scale=0.5), r(n, 4 * H, scale=0.5)), (r(H, 4 * H, scale=0.05), r(H, 4 * H, scale=0.05))
    act, dz, cseq, hprev = ((z(n, 4 * H), z(n, 4 * H)), (z(n, 4 * H), z(n, 4 * H)), (z(n, H), z(n, H)), (z(n, H), z(n, H)))
    out, dout = z(n, 2 * H), r(n, 2 * H)                              # the layer's [n][2H] output and its gradient, halves in place
    hseq, dhalf = (out[:, :H], out[:, H:]), (dout[:, :H], dout[:, H:])
    dense_h, dense_d = (z(n, H), z(n, H)), (r(n, H), r(n, H))        # the unidirectional launches take dense tensors
    ws = ops.lstm_seq_ws(clips, T, H, dev)

    def uni_fwd(d):
        ops.lstm_seq_fwd(gx[d], kh[d], act[d], cseq[d], dense_h[d], hprev[d], clips, T, H, ws=ws)

    def uni_bwd(d):
        ops.lstm_seq_bwd(dense_d[d], kh[d], act[d], cseq[d], dz[d], clips, T, H, ws=ws)

    fwd = alternate({"bi": lambda: ops.lstm_seq_bi_fwd(gx, kh, act, cseq, hseq, hprev, clips, T, H, ws=ws, hseq_ld=2 * H),
                     "two": lambda: (uni_fwd(0), uni_fwd(1)), "one": lambda: uni_fwd(0)}, rounds, batch)
    bwd = alternate({"bi": lambda: ops.lstm_seq_bi_bwd(dhalf, kh, act, cseq, dz, clips, T, H, ws=ws, dout_ld=2 * H),
                     "two": lambda: (uni_bwd(0), uni_bwd(1)), "one": lambda: uni_bwd(0)}, rounds, batch)
    if ops.lstm_seq_timed_out(ws):
        raise SystemExit("bench_blstm: a launch timed out waiting for its peers; the numbers would mean nothing")
    res = {}
    for name, v in (("forward", fwd), ("backward", bwd)):
        v.update(bi_over_two=round(v["bi"]["us"] / v["two"]["us"], 4), bi_over_one=round(v["bi"]["us"] / v["one"]["us"], 4),
                 bi_below_two=v["bi"]["us"] < v["two"]["us"])
        res[name] = v
    return res


def measure_step(conv_math, clips, fpc, rounds, steps, warmup, dev):
    base = NetConfig(image_shape=(227, 227, 3), num_classes=101, fpc=fpc, dropout_keep_prob=0.5, conv_math=conv_math)
    cfgs = {"unidirectional": base, "bidirectional": dataclasses.replace(base, lstm_bidirectional=True)}
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
    out["bidirectional_minus_unidirectional_ms"] = round(out["bidirectional"]["ms_per_step"] - out["unidirectional"]["ms_per_step"], 3)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blstm_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_blstm.py needs a HIP device; there is no CPU fallback")
    if args.rounds * args.steps < 20:
        raise SystemExit("at least 20 timed steps each: rounds x steps = %d" % (args.rounds * args.steps))
    dev = "cuda:0"
    result = {"workload": "launches: T = %d, H = %d, 8 and 64 clips; step: AlexNet(fc6) -> LSTM(256) -> 101 classes, %d clips x %d frames "
                          "227x227, one GPU, synthetic data" % (T, H, args.clips, args.fpc),
              "device": torch.cuda.get_device_name(0), "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
              "check": "bi < two (two unidirectional launches back to back), forward and backward, at 8 and at 64 clips"}
    launches = {"clips_%d" % c: launches_alone(c, args.launch_rounds, args.batch, dev) for c in (8, 64)}
    result["launches_alone"] = launches
    ok = all(v[d]["bi_below_two"] for v in launches.values() for d in ("forward", "backward"))
    result["verdict"] = {"bi_below_two_everywhere": ok,
                         "bi_over_two": {k: {d: v[d]["bi_over_two"] for d in ("forward", "backward")} for k, v in launches.items()},
                         "bi_over_one": {k: {d: v[d]["bi_over_one"] for d in ("forward", "backward")} for k, v in launches.items()}}
    if not args.no_step:
        result["steps"] = {m: measure_step(m, args.clips, args.fpc, args.rounds, args.steps, args.warmup, dev) for m in ("f32", "bf16")}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    brief = {"us": {k: {d: {n: v[d][n]["us"] for n in ("bi", "two", "one")} for d in ("forward", "backward")} for k, v in launches.items()},
             "verdict": result["verdict"]}
    if not args.no_step:
        brief["ms_per_step"] = {m: {k: result["steps"][m][k]["ms_per_step"] for k in ORDER} for m in result["steps"]}
    print(json.dumps(brief))
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
