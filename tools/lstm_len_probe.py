#!/usr/bin/env python3
"""Times the forward + backward LSTM recurrence with per-clip lengths at the decoder's shape of BASELINE config 4
([clips] x 21 word steps, hidden 256): the plain call, seq_len = T everywhere, uniform random lengths, all lengths 10.
usage: lstm_len_probe.py [clips] [plain|full|random|ten ...]
Prints device-event times per call (launch included).  For kernel times run ONE variant under the profiler, in a run of its own:
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/lstm_len_probe.py 64 random ; python tools/kstats.py <dir>
(profiles/lstm_seq_len.txt)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import vltf_amd.ops as ops

def timed(fn, reps=50):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3

T, H = 21, 256
dev = "cuda:0"
b = int(sys.argv[1]) if len(sys.argv) > 1 else 64
variants = sys.argv[2:] or ["plain", "full", "random", "ten"]
torch.manual_seed(0)
gx = torch.randn(b * T, 4 * H, device=dev) * 0.5
kh = torch.randn(H, 4 * H, device=dev) * 0.05
s0 = torch.randn(b, H, device=dev) * 0.5
act, dz = torch.zeros(b * T, 4 * H, device=dev), torch.zeros(b * T, 4 * H, device=dev)
cseq, hseq, hprev = (torch.zeros(b * T, H, device=dev) for _ in range(3))
dh0, dc0 = torch.zeros(b, H, device=dev), torch.zeros(b, H, device=dev)
dout = torch.randn(b * T, H, device=dev)
ws = ops.lstm_seq_ws(b, T, H, dev)
lengths = {"plain": None, "full": np.full(b, T), "random": np.random.default_rng(0).integers(1, T + 1, b), "ten": np.full(b, 10)}
for v in variants:
    kw = {} if lengths[v] is None else {"seq_len": torch.tensor(lengths[v], dtype=torch.int32, device=dev)}
    tf = timed(lambda: ops.lstm_seq_fwd(gx, kh, act, cseq, hseq, hprev, b, T, H, ws=ws, h0=s0, c0=s0, **kw))
    tb = timed(lambda: ops.lstm_seq_bwd(dout, kh, act, cseq, dz, b, T, H, ws=ws, c0=s0, dh0=dh0, dc0=dc0, **kw))
    if ops.lstm_seq_timed_out(ws):
        sys.exit("the recurrence timed out waiting for its peers: no number")
    live = b * T if lengths[v] is None else int(lengths[v].sum())
    print("clips %3d %-6s (%4d of %4d steps live): fwd %.1f us  bwd %.1f us  fwd + bwd %.1f us   [launch included]" %
          (b, v, live, b * T, tf, tb, tf + tb), flush=True)
