#!/usr/bin/env python3
"""What mixup costs on one GPU, in ONE process, everything in alternation.

1. The blend alone.  vl_mixup_pairs (fp32) over 1.5 c floats reads and writes every one of them: 12 c bytes.  vl_sgd_apply over c floats
   reads w and g and writes w: 12 c bytes.  c = 44.6 M (the benchmark model's parameter count), so the two move the same bytes and the
   blend is held to the project's standing bound for a launch,

       T(vl_mixup_pairs, 1.5 c floats) <= 1.15 x T(vl_sgd_apply, c floats).

2. The loss launch alone.  vl_softmax_xent_mix takes the place of vl_softmax_xent_ls in the train step:

       T(vl_softmax_xent_mix) <= 1.15 x T(vl_softmax_xent_ls)

   at 64 x 101 (the benchmark's loss) and 1344 x 1000 (64 clips x 21 rows, 1000 classes), rows-workspace form, smoothing 0.1, top_k 5.

   The tool exits 1 when one of the three ratios misses the bound.

3. The step.  The train step at the benchmark geometry (64 clips x 16 frames of 227x227, AlexNet(fc6) -> LSTM(256) -> 101 classes, plain
   SGD), fp32 and the packed-bf16 conv path, without and with mixup_alpha.  No number is fixed in advance: the difference is reported
   beside the two added launches measured alone at the step's own sizes (the blend over the step's x0 / packed input, the loss launch
   minus the one it replaces) and the spread between rounds of the step WITHOUT mixup.  The expectation that is checked and recorded,
   not enforced: difference <= launches alone + spread.

Writes profiles/mixup_step.json.  No CPU fallback.
usage: bench_mixup.py [--clips 64] [--rounds 4] [--steps 5] [--warmup 3] [--batch 200] [--out profiles/mixup_step.json]"""
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
ORDER = ["plain", "mixup"]
SHAPES = [(64, 101), (1344, 1000)]
BOUND = 1.15
EPS, TOPK = 0.1, 5
ALPHA, SEED, LAM = 0.2, 7, 0.7
C = 44_600_000


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


def with_ratio(out, new, old, **more):
    ratio = out[new]["us"] / out[old]["us"]
    out.update(ratio=round(ratio, 4), within_bound=ratio <= BOUND, **more)
    return out


def blend_alone(rounds, batch, dev):
    """The blend over 1.5 c floats (two clips of 0.75 c) against the SGD update over c floats: 12 c bytes each."""
    elems = (C * 3 // 4) // 4 * 4
    x = torch.randn(2 * elems, device=dev)
    w, g = torch.randn(C, device=dev), torch.randn(C, device=dev)
    lam = torch.tensor([LAM], device=dev)
    out = alternate({"vl_sgd_apply": lambda: ops.sgd_apply(w, g, 1e-6, 0.0, None, 1.0),
                     "vl_mixup_pairs": lambda: ops.mixup_pairs(x, 2, lam)}, rounds, batch)
    for name, nbytes in (("vl_sgd_apply", 12 * C), ("vl_mixup_pairs", 8 * 2 * elems)):
        out[name]["bytes"] = nbytes
        out[name]["TB_per_s"] = round(nbytes / out[name]["us"] * 1e-6, 3)
    return with_ratio(out, "vl_mixup_pairs", "vl_sgd_apply", launches_per_round=batch, rounds=rounds, floats_blended=2 * elems, floats_updated=C)


def loss_alone(rows, classes, rpc, rounds, batch, dev):
    rng = np.random.default_rng(rows)
    z = torch.from_numpy((rng.standard_normal((rows, classes)) * 2).astype(np.float32)).to(dev)
    y = torch.zeros((rows, classes), dtype=torch.int32)
    y[torch.arange(rows), torch.from_numpy(rng.integers(0, classes, rows))] = 1
    y = y.to(dev)
    dz = torch.empty_like(z)
    stats, ws = torch.zeros(3, device=dev), torch.zeros(3 * rows, device=dev)
    lam = torch.tensor([LAM], device=dev)
    out = alternate({"vl_softmax_xent_ls": lambda: ops.softmax_xent_ls(z, y, dz, stats, 1.0 / rows, ws, EPS, TOPK),
                     "vl_softmax_xent_mix": lambda: ops.softmax_xent_mix(z, y, dz, stats, 1.0 / rows, ws, rpc, EPS, TOPK, lam)}, rounds, batch)
    return with_ratio(out, "vl_softmax_xent_mix", "vl_softmax_xent_ls", launches_per_round=batch, rounds=rounds, rows_per_clip=rpc)


def measure_step(conv_math, clips, fpc, rounds, steps, warmup, launch_rounds, batch, dev):
    base = NetConfig(image_shape=(227, 227, 3), num_classes=101, fpc=fpc, dropout_keep_prob=0.5, conv_math=conv_math)
    cfgs = {"plain": base, "mixup": dataclasses.replace(base, mixup_alpha=ALPHA, mixup_seed=SEED)}
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

    def run(name, fetch=False):                     # mixup draws its own weight per step (about 0.9 on average at alpha 0.2)
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
                     "grad_norm": round(check["grad_norm"], 4), "accuracy": check["accuracy"]}
    # the two added launches alone, at the step's own sizes: the blend over the buffer the step blends, and the loss launch against the
    # one it replaces (the plain engine's: vl_softmax_xent)
    eng = engines["mixup"]
    n = clips * fpc
    buf = eng.layers[0]["xb"][:n] if (eng.c8 and eng._xb_fed) else eng.x0[:n]
    lam = torch.tensor([LAM], device=dev)
    z, dz = torch.randn((clips, 101), device=dev), torch.empty((clips, 101), device=dev)
    st, ws = torch.zeros(3, device=dev), torch.zeros(3 * clips, device=dev)
    alone = alternate({"vl_mixup_pairs": lambda: ops.mixup_pairs(buf, clips, lam),
                       "vl_softmax_xent": lambda: ops.softmax_xent(z, onehot, dz, st[:2], 1.0 / clips, ws),
                       "vl_softmax_xent_mix": lambda: ops.softmax_xent_mix(z, onehot, dz, st, 1.0 / clips, ws, 1, 0.0, 0, lam)},
                      launch_rounds, batch)
    alone["vl_mixup_pairs"]["bytes"] = 2 * buf.numel() * buf.element_size() - (clips % 2) * 2 * (buf.numel() // clips) * buf.element_size()
    alone["vl_mixup_pairs"]["TB_per_s"] = round(alone["vl_mixup_pairs"]["bytes"] / alone["vl_mixup_pairs"]["us"] * 1e-6, 3)
    added = (alone["vl_mixup_pairs"]["us"] + alone["vl_softmax_xent_mix"]["us"] - alone["vl_softmax_xent"]["us"]) * 1e-3
    plain = per_round["plain"]
    verdict = {"step_with_minus_without_ms": round(out["mixup"]["ms_per_step"] - out["plain"]["ms_per_step"], 3),
               "added_launches_alone_ms": round(added, 3), "spread_without_ms": round(max(plain) - min(plain), 3)}
    verdict["difference_within_launches_plus_spread"] = (verdict["step_with_minus_without_ms"]
                                                         <= verdict["added_launches_alone_ms"] + verdict["spread_without_ms"])
    out["blended_buffer"] = {"dtype": str(buf.dtype).replace("torch.", ""), "elements": buf.numel()}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixup_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mixup.py needs a HIP device; there is no CPU fallback")
    if args.rounds * args.steps < 20:
        raise SystemExit("at least 20 timed steps each: rounds x steps = %d" % (args.rounds * args.steps))
    dev = "cuda:0"
    result = {"workload": "AlexNet(fc6) -> LSTM(256) -> 101 classes, %d clips x %d frames 227x227, one GPU, synthetic data" % (args.clips, args.fpc),
              "device": torch.cuda.get_device_name(0), "mixup_alpha": ALPHA, "mixup_seed": SEED, "lam_of_the_launches_alone": LAM,
              "bound": "each launch ratio <= %.2f, alternating in this run" % BOUND}
    launches = {"blend_%.1fM_floats" % (C * 1.5e-6): blend_alone(args.launch_rounds, max(args.batch // 10, 10), dev)}
    for rows, classes in SHAPES:
        launches["loss_%dx%d" % (rows, classes)] = loss_alone(rows, classes, 1 if rows == 64 else 21, args.launch_rounds, args.batch, dev)
    result["launches_alone"] = launches
    steps = {}
    for math in ("f32", "bf16"):
        steps[math] = measure_step(math, args.clips, args.fpc, args.rounds, args.steps, args.warmup, args.launch_rounds, args.batch, dev)
    result["steps"] = steps
    verdict = {"launch_ratios": {k: v["ratio"] for k, v in launches.items()}, "bound": BOUND,
               "within_bound": all(v["within_bound"] for v in launches.values()),
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
