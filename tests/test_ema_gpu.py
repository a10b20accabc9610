"""Exponential moving average of the weights on the device (vl_ema_update, NetConfig.ema_decay): the rule of
tf.train.ExponentialMovingAverage written for rate = 1 - decay,
    s' = s + rate * (w - s)
-- against float64, through ranges bit for bit, under the skip word, with the rate read from the step state, in LRCNEngine (eager,
captured, with frozen layers, under accumulation), GraphEngine, one-rank RCCL and the checkpoint / validation of run_task.  Shapes and
tolerances are those of tests/test_momentum_gpu.py: 67x67x3 frames, 2 clips x 3 frames, hidden 8, 7 classes; against float64 rtol 1e-5 and
atol 1e-6 * max|want| (two fp32 roundings per element and update, each 6e-8 relative to a term no larger than a few max|want|, and the
recursion contracts an earlier error by 1 - rate)."""
import glob
import os
import pickle
import shutil
import socket

import numpy as np
import pytest
import torch
import yaml

from oracle import lrcn_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN = np.array([99.197148, 105.293620, 109.503945], np.float32)
DECAY = 0.9


def bits(t):
    return t.view(torch.int32)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def close(got, want, msg=""):
    want = np.asarray(want, np.float64)
    scale = float(np.abs(want).max()) or 1.0
    np.testing.assert_allclose(np.asarray(got, np.float64), want, rtol=1e-5, atol=1e-6 * scale, err_msg=msg)


def rule(s, w, rate):
    """One update in float64 with the float32 rate the launch got."""
    s = np.asarray(s, np.float64)
    return s + float(np.float32(rate)) * (np.asarray(w, np.float64) - s)


# ---- 1. the rule against float64 ---------------------------------------------------------------------------------------------------
N1 = 100003
_DATA1 = {}


def data1():
    """A shadow ~ N(0, 1) and four weight vectors ~ N(0, 1); made once, never written."""
    if not _DATA1:
        rng = np.random.default_rng(2)
        _DATA1["s"] = rng.standard_normal(N1).astype(np.float32)
        _DATA1["w"] = [rng.standard_normal(N1).astype(np.float32) for _ in range(4)]
    return _DATA1["s"], _DATA1["w"]


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
def test_rule_against_fp64(offset):
    """Fresh weights per call and the rates of n = 0, 5, 5000 at decay 0.999 with warm-up (0.9, 0.6, 9 / 5010: the warm-up branch of the
    maximum), then n = 20000 (past the cross-over at 8990: the branch 1 - decay), so both branches occur.  offset 1: views s[1:], w[1:] of
    16-byte aligned buffers -- three scalar head elements, then 16-byte accesses; the element before the views stays."""
    from vltf_amd import ops
    from vltf_amd.engine import ema_rate
    s0, ws = data1()
    o = offset
    sd = torch.full((N1 + o,), 7.0, device=DEV)
    wd = torch.full((N1 + o,), float("nan"), device=DEV)
    sd[o:] = torch.from_numpy(s0).to(DEV)
    sv, wv = sd[o:], wd[o:]
    ref = s0.astype(np.float64)
    rates = [ema_rate(0.999, True, n) for n in (0, 5, 5000, 20000)]
    assert rates[0] == float(np.float32(0.9)) and rates[2] == float(np.float32(9.0 / 5010.0)) and rates[3] == float(np.float32(1.0 - 0.999))
    for w, rate in zip(ws, rates):
        wv.copy_(torch.from_numpy(w).to(DEV))
        ops.ema_update(sv, wv, rate)
        ref = rule(ref, w, rate)
        close(host(sv), ref, "shadow at rate %g" % rate)
        assert np.array_equal(host(wv), w)                                   # the weights are read only
    if o:
        assert host(sd)[0] == 7.0 and np.isnan(host(wd)[0])                  # the element before the views


def test_rounding_order_is_the_documented_one():
    """d = fl(w - s); s' = fl(rate * d + s), one rounding each: float64 reproduces both (a product of two floats is exact in float64;
    the double rounding of the sum can differ from the fused one in the last bit, rarely)."""
    from vltf_amd import ops
    s0, ws = data1()
    rate = np.float32(0.3)
    sd, wd = torch.from_numpy(s0).to(DEV), torch.from_numpy(ws[0]).to(DEV)
    ops.ema_update(sd, wd, float(rate))
    d = (ws[0].astype(np.float64) - s0.astype(np.float64)).astype(np.float32)
    want = (np.float64(rate) * d.astype(np.float64) + s0.astype(np.float64)).astype(np.float32)
    got = host(sd)
    assert np.mean(got == want) > 0.999 and np.abs(got.astype(np.float64) - want).max() <= np.abs(want).max() * 2.0 ** -23


# ---- 2. ranges, bit for bit (COUNT and TIERS of tests/test_momentum_gpu.py, restated) -------------------------------------------------
COUNT = 4096 * 256 + 4099          # more elements than the grid has lanes (every lane loops), and a tail
# boundaries that are no multiple of 4, a range of one element, a gap of one element (4099) and a wide one
TIERS = [(5, 1000, 1.0), (1000, 4099, 0.25), (4100, 4101, 2.0), (9001, COUNT, 3.0)]
RATE = 0.0123


def kernel_data(seed=0):
    """shadow and w, both NaN outside the ranges (an element there must never be loaded or stored)."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    s, w = (torch.randn(COUNT, generator=gen) for _ in range(2))
    inside = torch.zeros(COUNT, dtype=torch.bool)
    for lo, hi, _ in TIERS:
        inside[lo:hi] = True
    s[~inside] = float("nan")
    w[~inside] = float("nan")
    return s.to(DEV), w.to(DEV), inside.to(DEV)


def state_block(rate, step=7, lr=0.5):
    from vltf_amd import ops
    st = ops.step_state(DEV)
    ops.step_state_set(st, step, lr, 1)
    ops.step_state_set_ema(st, rate)
    return st


@pytest.mark.parametrize("st", [False, True], ids=["eager", "st"])
def test_ema_update_ranges(st):
    from vltf_amd import ops
    s, w, inside = kernel_data()
    got = s.clone()
    if st:
        ops.ema_update_st(got, w, state_block(RATE), ranges=TIERS)
        eager = s.clone()
        ops.ema_update(eager, w, RATE, ranges=TIERS)
        assert torch.equal(bits(got), bits(eager))
    else:
        ops.ema_update(got, w, RATE, ranges=TIERS)
    assert torch.equal(bits(got)[~inside], bits(s)[~inside])                  # outside: the bits of before (NaN payloads included)
    assert bool(torch.isnan(got[~inside]).all())
    for lo, hi, _ in TIERS:                                                   # inside: the full-range call on the sub-range alone
        sub, wsub = s[lo:hi].clone(), w[lo:hi].clone()
        if st:
            ops.ema_update_st(sub, wsub, state_block(RATE))
        else:
            ops.ema_update(sub, wsub, RATE)
        assert torch.isfinite(sub).all() and not torch.equal(sub, s[lo:hi])
        assert torch.equal(bits(got[lo:hi]), bits(sub)), (lo, hi)
        assert torch.equal(bits(wsub), bits(w[lo:hi]))
    assert torch.equal(bits(w)[inside], bits(kernel_data()[1])[inside])       # w is read only


# ---- 3. skip word and argument checks ---------------------------------------------------------------------------------------------
def test_skip_word_and_argument_checks():
    from vltf_amd import ops
    from vltf_amd._ffi import VltfError
    s, w, inside = kernel_data(2)
    got = s.clone()
    skip = torch.ones(1, dtype=torch.int32, device=DEV)
    ops.ema_update(got, w, RATE, skip=skip, ranges=TIERS)
    ops.ema_update_st(got, w, state_block(RATE), skip=skip, ranges=TIERS)
    ops.ema_update(got[5:1000], w[5:1000], RATE, skip=skip)
    assert torch.equal(bits(got), bits(s))
    st = state_block(RATE)
    for rate in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        with pytest.raises(VltfError, match="rate"):
            ops.ema_update(got, w, rate, ranges=TIERS)
        with pytest.raises(VltfError, match="rate"):
            ops.step_state_set_ema(st, rate)
    with pytest.raises(VltfError):
        ops.ema_update(got, w[:-1], RATE)                                     # another size
    with pytest.raises(VltfError):
        ops.ema_update_st(got, w, None, ranges=TIERS)                         # no step state
    for table in ([(0, 10, 1.0), (9, 20, 1.0)], [(10, 20, 1.0), (5, 8, 1.0)], [(0, COUNT + 1, 1.0)], [], [(0, 10, 0.0)],
                  [(i, i + 1, 1.0) for i in range(17)]):
        with pytest.raises(VltfError):
            ops.ema_update(got, w, RATE, ranges=table)
        with pytest.raises(VltfError):
            ops.ema_update_st(got, w, st, ranges=table)
    torch.cuda.synchronize()
    assert torch.equal(bits(got), bits(s))
    skip.zero_()                                                              # the word cleared: the same call averages
    ops.ema_update(got, w, RATE, skip=skip, ranges=TIERS)
    assert not torch.equal(got[inside], s[inside]) and torch.equal(bits(got)[~inside], bits(s)[~inside])
    ops.ema_update(got, w, 1.0, ranges=TIERS)                                 # rate 1 (decay 0) is the upper end of what is allowed
    assert bool(torch.isfinite(got[inside]).all())


# ---- 4. the step-state form ---------------------------------------------------------------------------------------------------------
def test_step_state_setter_writes_one_field():
    from vltf_amd import ops
    st = ops.step_state(DEV)
    ops.step_state_set(st, 11, 0.25, 77)
    before = host(st).copy()
    assert before.size == 8 and before[5] == 0 and before[6] == 0 and before[7] == 0
    ops.step_state_set_ema(st, RATE)
    after = host(st).copy()
    want = before.copy()
    want[5] = np.float32(RATE).view(np.int32)
    assert np.array_equal(after, want)                                        # step, lr, tag origin, Adam's step size, reserved: as before
    ops.step_state_set(st, 12, 0.5, 78)                                       # the setters of before leave the rate alone
    ops.step_state_set_micro(st, 12, 25, 0.5, 78)
    again = host(st)
    assert again[5] == want[5] and again[6] == 0 and again[7] == 0 and not np.array_equal(again[:5], want[:5])
    s0, ws = data1()
    a, b = torch.from_numpy(s0).to(DEV), torch.from_numpy(s0).to(DEV)
    w = torch.from_numpy(ws[1]).to(DEV)
    ops.ema_update_st(a, w, st)
    ops.ema_update(b, w, RATE)
    assert torch.equal(bits(a), bits(b)) and not torch.equal(a, torch.from_numpy(s0).to(DEV))


# ---- 5. LRCNEngine ------------------------------------------------------------------------------------------------------------------
SHAPE, NCLS, FPC, B, HID = (67, 67, 3), 7, 3, 2, 8
LRS = (0.01, 0.02, 0.005)
CLIP = 0.5


def small_cfg(**kw):
    from vltf_amd.engine import NetConfig
    return NetConfig(image_shape=SHAPE, num_classes=NCLS, fpc=FPC, frame_encoding_layer="fc6", lstm_hidden=HID, **kw)


def small_batches(steps, seed=5):
    rng = np.random.default_rng(seed)
    p = O.init_params(rng, NCLS, "fc6", HID, 1, SHAPE, well_scaled=True)
    out = []
    for _ in range(steps):
        frames = torch.tensor(rng.integers(0, 256, (B * FPC,) + SHAPE, dtype=np.uint8), device=DEV)
        onehot = torch.tensor(O.labels_to_one_hot([[l] for l in rng.integers(0, NCLS, B)], NCLS), device=DEV)
        out.append((frames, onehot))
    return p, out


def flat_of(eng, params):
    return np.concatenate([np.asarray(params[n], np.float32).ravel() for n, _ in eng.specs])


def follow(eng, plain, step_fns, decay, warmup, frozen=()):
    """Runs the updates step_fns[i](engine) on both engines; after each the shadow is the float64 recursion over the fetched weights,
    the weights equal the option-off engine's bit for bit, and a frozen variable's shadow equals its weights bit for bit."""
    from vltf_amd.engine import ema_rate
    ref = flat_of(eng, eng.get_params()).astype(np.float64)
    assert np.array_equal(host(eng.ema), ref.astype(np.float32))              # before the first update: a copy of the weights
    offsets = {}
    off = 0
    for name, shp in eng.specs:
        offsets[name] = (off, int(np.prod(shp)))
        off += int(np.prod(shp))
    for i, fn in enumerate(step_fns):
        n = eng.step_count
        fn(eng)
        fn(plain)
        assert eng.step_count == n + 1
        after = eng.get_params()
        other = plain.get_params()
        for k in after:
            assert np.array_equal(after[k].view(np.int32), other[k].view(np.int32)), "weights differ from the option-off run: %s" % k
        w = flat_of(eng, after)
        new = rule(ref, w, ema_rate(decay, warmup, n))
        got = host(eng.ema)
        for k, (o, cnt) in offsets.items():
            if k in frozen:
                new[o:o + cnt] = ref[o:o + cnt]
                assert np.array_equal(got[o:o + cnt].view(np.int32), w[o:o + cnt].view(np.int32)), "frozen %s" % k
        ref = new
        close(got, ref, "shadow after update %d" % i)
        assert not np.array_equal(got, w)                                     # it lags behind the weights
        named = eng.get_ema_params()
        assert all(np.array_equal(named[k].ravel(), got[o:o + cnt]) and named[k].shape == after[k].shape for k, (o, cnt) in offsets.items())
    return ref


@pytest.mark.parametrize("warmup", [False, True], ids=["constant", "warmup"])
def test_engine_three_steps(warmup):
    from vltf_amd.engine import LRCNEngine
    p, batches = small_batches(3)
    eng = LRCNEngine(small_cfg(ema_decay=DECAY, ema_warmup=warmup), max_clips=B, device=DEV)
    plain = LRCNEngine(small_cfg(), max_clips=B, device=DEV)
    assert eng.ema is not None and eng.ema.numel() == eng.w.numel() and plain.ema is None
    eng.load_params(p)
    plain.load_params(p)
    steps = [lambda e, i=i, lr=lr: e.train_step_u8(*batches[i], lr=lr, clip_norm=CLIP, mean_bgr=MEAN) for i, lr in enumerate(LRS)]
    follow(eng, plain, steps, DECAY, warmup)
    assert eng.OPT_PREFIX + "ema" in eng.get_opt_state() and eng.OPT_PREFIX + "ema" not in plain.get_opt_state()


def test_engine_off_allocates_nothing_and_refusals():
    from vltf_amd._ffi import VltfError
    from vltf_amd.engine import LRCNEngine
    for kw in (dict(ema_decay=1.0), dict(ema_decay=-0.1), dict(ema_warmup=True), dict(ema_decay=float("nan"))):
        with pytest.raises(VltfError, match="ema"):
            LRCNEngine(small_cfg(**kw), max_clips=B, device=DEV)
    off = LRCNEngine(small_cfg(), max_clips=B, device=DEV)
    assert off.ema is None and off.load_opt_state(off.get_opt_state()) == []
    with pytest.raises(VltfError, match="averaged"):
        off.get_ema_params()
    with pytest.raises(VltfError, match="averaged"):
        off.load_ema(np.zeros(off.w.numel(), np.float32))
    infer = LRCNEngine(small_cfg(ema_decay=DECAY), max_clips=B, device=DEV, training=False)
    assert infer.ema is None
    flat = np.arange(infer.w.numel(), dtype=np.float32)
    infer.use_ema_weights(flat)
    assert np.array_equal(host(infer.w), flat)
    with pytest.raises(VltfError, match="shape"):
        infer.use_ema_weights(flat[:-1])
    on = LRCNEngine(small_cfg(ema_decay=DECAY), max_clips=B, device=DEV)
    with pytest.raises(VltfError, match="training=False"):
        on.use_ema_weights(flat)
    on.load_ema(flat)
    assert np.array_equal(host(on.ema), flat)


def test_engine_opt_state_round_trip():
    from vltf_amd._ffi import VltfError
    from vltf_amd.engine import LRCNEngine
    p, _ = small_batches(0)
    eng = LRCNEngine(small_cfg(ema_decay=DECAY), max_clips=B, device=DEV)
    eng.load_params(p)
    eng.ema.copy_(torch.arange(eng.ema.numel(), device=DEV) % 7)
    st = eng.get_opt_state()
    key = eng.OPT_PREFIX + "ema"
    assert st[key].shape == (eng.w.numel(),)
    other = LRCNEngine(small_cfg(ema_decay=DECAY), max_clips=B, device=DEV)
    other.load_params(p)
    assert other.load_opt_state(st) == [] and torch.equal(other.ema, eng.ema)
    bare = {k: v for k, v in st.items() if k != key}
    assert other.load_opt_state(bare) == [key] and torch.equal(bits(other.ema), bits(other.w))   # absent: a copy of the loaded weights
    with pytest.raises(VltfError, match="shape"):
        other.load_opt_state({**st, key: st[key][:-1]})


def test_engine_with_frozen_layers():
    """train_from fc6: the frozen variables' shadow equals their weights bit for bit, the rest follows the recursion."""
    from vltf_amd.engine import LRCNEngine
    p, batches = small_batches(2)
    eng = LRCNEngine(small_cfg(ema_decay=DECAY, train_from="fc6", lr_mult=4.0), max_clips=B, device=DEV)
    plain = LRCNEngine(small_cfg(train_from="fc6", lr_mult=4.0), max_clips=B, device=DEV)
    eng.load_params(p)
    plain.load_params(p)
    frozen = set(eng.plan.frozen)
    assert frozen == {"dcnn/conv%d%s" % (i, k) for i in range(1, 6) for k in "Wb"} and not eng.plan.full_range()
    steps = [lambda e, i=i, lr=lr: e.train_step_u8(*batches[i], lr=lr, clip_norm=CLIP, mean_bgr=MEAN) for i, lr in enumerate(LRS[:2])]
    follow(eng, plain, steps, DECAY, False, frozen)


def test_captured_step_equals_eager():
    """Step 1 is the warm-up, step 2 is captured and replayed, steps 3 and 4 are replays: three replays.  lr and the warm-up rate change
    every step (both come from the step state); weights and shadow are bit-equal to the eager engine's after each."""
    from tests.test_step_graph_gpu import batch, pair, same_state, train_both
    eager, graph = pair(B, fpc=FPC, hid=HID, ema_decay=DECAY, ema_warmup=True)
    rng = np.random.default_rng(11)
    start = host(eager.ema).copy()
    for step, lr in enumerate(LRS + (0.03,)):
        train_both((eager, graph), batch(rng, B, FPC), lr=lr)
        same_state(eager, graph)
        assert torch.equal(bits(eager.ema), bits(graph.ema))
    assert len(graph._graphs) == 1 and not np.array_equal(host(graph.ema), start)
    assert not torch.equal(graph.ema, graph.w)


def test_accumulated_update_averages_once():
    """accumulate 2: the shadow keeps its bits over the first micro-step and moves once per update, at the rate of the update count."""
    from vltf_amd.engine import LRCNEngine
    p, batches = small_batches(4)
    eng = LRCNEngine(small_cfg(ema_decay=DECAY, ema_warmup=True, accumulate=2), max_clips=B, device=DEV)
    plain = LRCNEngine(small_cfg(accumulate=2), max_clips=B, device=DEV)
    eng.load_params(p)
    plain.load_params(p)

    def update(u, lr):
        def fn(e):
            before = None if e.ema is None else host(e.ema).copy()
            e.train_step_u8(*batches[2 * u], lr=lr, clip_norm=CLIP, mean_bgr=MEAN, micro=(0, 2))
            if before is not None:
                assert np.array_equal(host(e.ema).view(np.int32), before.view(np.int32))          # not on the first micro-step
            e.train_step_u8(*batches[2 * u + 1], lr=lr, clip_norm=CLIP, mean_bgr=MEAN, micro=(1, 2))
        return fn

    follow(eng, plain, [update(0, LRS[0]), update(1, LRS[1])], DECAY, True)
    assert eng.step_count == 2


# ---- 6. GraphEngine -----------------------------------------------------------------------------------------------------------------
def test_graph_engine_two_steps():
    from tests import graph_cases as GC
    from tests.test_graph_gpu import device_feeds
    from vltf_amd._ffi import VltfError
    from vltf_amd.graph import GraphEngine
    case = GC.CASES["encdec_state"]()                   # two pipelines, one tower of 2-frame clips: the smallest of graph_cases
    pipes, ds = GC.specs_and_datasets(case)
    with pytest.raises(VltfError, match="ema"):
        GraphEngine(pipes, ds, case["V"], device=DEV, ema_warmup=True)
    plain = GraphEngine(pipes, ds, case["V"], device=DEV)
    assert plain.ema is None
    eng = GraphEngine(pipes, ds, case["V"], device=DEV, ema_decay=DECAY, ema_warmup=True)
    params = eng.init_params(seed=case["seed"], well_scaled=True)
    eng.load_params(params)
    plain.load_params(params)
    raw, feeds = GC.inputs(case)
    fd = device_feeds(raw)
    eng.forward(fd)
    rows = eng.logits_host().shape[0]
    onehot = torch.tensor(O.labels_to_one_hot([[l] for l in np.random.default_rng(0).integers(0, case["V"], rows)], case["V"]), device=DEV)
    steps = [lambda e, lr=lr: e.train_step(fd, onehot, lr=lr, clip_norm=CLIP) for lr in LRS[:2]]
    follow(eng, plain, steps, DECAY, True)
    assert eng.OPT_PREFIX + "ema" in eng.get_opt_state()


# ---- 7. one-rank RCCL ---------------------------------------------------------------------------------------------------------------
def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def dp_worker(port, q):
    os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from vltf_amd import dp
    from vltf_amd.engine import LRCNEngine, NetConfig
    dp.init_from_env(backend="nccl", force=True)
    shape, ncls, fpc, clips, hid = (67, 67, 3), 5, 2, 4, 6
    rng = np.random.default_rng(11)
    p = O.init_params(rng, ncls, "fc6", hid, 1, shape, well_scaled=True)
    frames = torch.tensor(rng.integers(0, 256, (clips * fpc,) + shape, dtype=np.uint8), device="cuda:0")
    onehot = torch.tensor(O.labels_to_one_hot([[l] for l in rng.integers(0, ncls, clips)], ncls), device="cuda:0")
    cfg = NetConfig(image_shape=shape, num_classes=ncls, fpc=fpc, lstm_hidden=hid, ema_decay=0.9, ema_warmup=True)
    eng = LRCNEngine(cfg, max_clips=clips, device="cuda:0", dp=dp.GradAllReduce(always=True))
    ref = LRCNEngine(cfg, max_clips=clips, device="cuda:0")
    eng.load_params(p)
    ref.load_params(p)
    start = ref.ema.clone()
    for lr in (0.05, 0.02):
        eng.train_step_u8(frames, onehot, lr=lr, clip_norm=0.5, mean_bgr=MEAN)
        ref.train_step_u8(frames, onehot, lr=lr, clip_norm=0.5, mean_bgr=MEAN)
    got, want = eng.get_params(), ref.get_params()
    torch.cuda.synchronize()
    q.put(dict(same=all(np.array_equal(got[k], want[k]) for k in want),
               ema_same=bool(torch.equal(eng.ema.view(torch.int32), ref.ema.view(torch.int32))),
               ema_moved=not bool(torch.equal(ref.ema, start)), ema_lags=not bool(torch.equal(ref.ema, ref.w))))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_one_rank_rccl_shadow_equals_single_process():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    pr = ctx.Process(target=dp_worker, args=(free_port(), q))
    pr.start()
    pr.join(300)
    assert pr.exitcode == 0, "rank exited with %s" % pr.exitcode
    r = q.get(timeout=10)
    assert r["same"] and r["ema_same"] and r["ema_moved"] and r["ema_lags"], r


# ---- 8. checkpoint and validation through run_task ----------------------------------------------------------------------------------
KEY = "__optimizer__/ema"


class Runs:
    """One folder: a dataset of 2 batches per epoch, the uninterrupted 2-epoch (4-update) training run with its two checkpoints."""

    def __init__(self, folder):
        from tests.test_host_workflow import make_dataset
        from tests.test_run_task_gpu import RAW
        self.folder = folder
        self.train_path, _, _ = make_dataset(folder, "train.txt", nvid=4, cpv=(1, 2, 1, 1), shape=RAW, seed=1)
        self.val_path, _, _ = make_dataset(folder, "val.txt", nvid=3, cpv=(2, 1, 2), shape=RAW, seed=2)

    def cfg(self, name, phase="train", run="runA", resume=None, train=None, val=None):
        from tests.test_run_task_gpu import write_cfg
        path = write_cfg(self.folder, name, self.train_path if phase == "train" else self.val_path, phase, epochs=2, det=True, run=run,
                         resume=resume)
        with open(path) as f:
            c = yaml.safe_load(f)
        c["run"]["train"].update(dict(ema_decay=DECAY, ema_warmup=True, base_lr=0.05), **(train or {}))
        c["run"]["val"].update(val or {})
        with open(path, "w") as f:
            yaml.safe_dump(c, f)
        return path

    def checkpoints(self, run="runA"):
        return sorted(glob.glob(os.path.join(self.folder, run, "checkpoints", "*.weights.npz")), key=os.path.getmtime)

    def logs(self, pattern, run="runA"):
        return "".join(open(f).read() for f in glob.glob(os.path.join(self.folder, run, pattern)))


def load_npz(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from vltf_amd import run_task
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("VLTF_PREFETCH", "0")
        mp.setenv("VLTF_CONV_MATH", "f32")
        mp.delenv("VLTF_STEP_GRAPH", raising=False)
        r = Runs(str(tmp_path_factory.mktemp("ema_runs")))
        run_task.main(r.cfg("a.yml"), seed=3)
        r.first, r.full = r.checkpoints()                                     # end of epoch 1 (2 updates), end of epoch 2 (4 updates)
        r.first_npz, r.full_npz = load_npz(r.first), load_npz(r.full)
        yield r


def test_resume_equals_uninterrupted(runs):
    """2 updates, save, resume for 2 more: weights and shadow equal those of the 4 uninterrupted updates bit for bit.  A weights-only
    checkpoint resumes with a warning and its shadow starts at the loaded weights."""
    from vltf_amd import run_task
    full, first = runs.full_npz, runs.first_npz
    assert int(first["__optimizer__/step_count"][0]) == 2 and int(full["__optimizer__/step_count"][0]) == 4
    assert KEY in first and KEY in full and first[KEY].dtype == np.float32
    wflat = np.concatenate([full[k].ravel() for k in full if not k.startswith("__optimizer__/")])
    assert full[KEY].shape == wflat.shape and not np.array_equal(np.sort(full[KEY]), np.sort(wflat))
    assert "Averaging the trained weights: decay 0.9, warm-up on" in runs.logs("log_e2e_train_scratch_*.log")
    base = runs.first[:-len(".weights.npz")]
    run_task.main(runs.cfg("b.yml", resume=base), seed=77)
    resumed = load_npz(runs.checkpoints()[-1])
    assert int(resumed["__optimizer__/step_count"][0]) == 4
    for k in full:
        np.testing.assert_array_equal(resumed[k].view(np.int32) if resumed[k].dtype == np.float32 else resumed[k],
                                      full[k].view(np.int32) if full[k].dtype == np.float32 else full[k], err_msg=k)
    # a weights-only checkpoint: a warning that names the key; the shadow starts at the weights, so it ends elsewhere
    folder = os.path.join(runs.folder, "runA", "checkpoints")
    bare = os.path.join(folder, "bare.graph-2")
    np.savez(bare + ".weights.npz", **{k: v for k, v in first.items() if not k.startswith("__optimizer__/")})
    shutil.copy(base + ".snap", bare + ".snap")
    from vltf_amd.engine import LRCNEngine, NetConfig
    from vltf_amd.feeder import Feeder
    from vltf_amd.defs_ import defs
    eng = LRCNEngine(NetConfig(image_shape=(67, 67, 3), num_classes=4, fpc=3, frame_encoding_layer="fc6", lstm_hidden=8, ema_decay=DECAY),
                     max_clips=4, device=DEV)
    fd = Feeder(defs.input_mode.video, [defs.phase.train], (None, None), 1, os.path.join(runs.folder, "runA"), True)
    fd.set_phase(defs.phase.train)
    fd.init_saveload(eng, bare)
    assert eng.step_count == 2 and torch.equal(bits(eng.ema), bits(eng.w))
    assert np.array_equal(host(eng.w), np.concatenate([first[n].ravel() for n, _ in eng.specs]))
    run_task.main(runs.cfg("c.yml", resume=bare), seed=77)
    log = runs.logs("log_e2e_train_resume_*.log")
    assert "no optimizer state" in log and KEY in log
    fresh = load_npz(runs.checkpoints()[-1])
    for k in full:                                                            # plain SGD: the weights need no state and end where they did
        if not k.startswith("__optimizer__/"):
            np.testing.assert_array_equal(fresh[k], full[k], err_msg=k)
    assert not np.array_equal(fresh[KEY], full[KEY])


def val_logits(runs, run):
    tot = glob.glob(os.path.join(runs.folder, run, "validation_logits_e2e_val_resume_*.total"))
    assert len(tot) == 1
    with open(tot[0], "rb") as f:
        return pickle.load(f)                                                 # written by this run


def test_validation_with_the_averaged_weights(runs):
    """use_ema True: the logits are, bit for bit, those of a validation run over a checkpoint whose weights are get_ema_params() of an
    engine restored from the original; False / absent: those of the raw weights.  The two differ.  A checkpoint without the key fails
    with a message that names the key and the file."""
    from vltf_amd import run_task
    from vltf_amd.engine import LRCNEngine, NetConfig
    last, stored = runs.full, runs.full_npz
    eng = LRCNEngine(NetConfig(image_shape=(67, 67, 3), num_classes=4, fpc=3, frame_encoding_layer="fc6", lstm_hidden=8, ema_decay=DECAY),
                     max_clips=4, device=DEV)
    eng.load_params({k: v for k, v in stored.items() if not k.startswith("__optimizer__/")})
    assert eng.load_opt_state({k: v for k, v in stored.items() if k.startswith("__optimizer__/")}) == []
    averaged = eng.get_ema_params()
    assert any(not np.array_equal(averaged[k], stored[k]) for k in averaged)
    for run, weights in (("valE", stored), ("valR", stored), ("valS", averaged), ("valN", {k: v for k, v in stored.items() if k != KEY})):
        folder = os.path.join(runs.folder, run, "checkpoints")
        os.makedirs(folder)
        np.savez(os.path.join(folder, "x.graph-4.weights.npz"), **weights)
        shutil.copy(last[:-len(".weights.npz")] + ".snap", os.path.join(folder, "x.graph-4.snap"))

    def validate(run, **val):
        base = os.path.join(runs.folder, run, "checkpoints", "x.graph-4")
        return run_task.main(runs.cfg("val_%s.yml" % run, phase="val", run=run, resume=base, val=val))

    validate("valE", use_ema=True)
    validate("valR", use_ema=False)
    validate("valS")                                                          # the averaged weights as a plain checkpoint, key absent
    ema, raw, swapped = val_logits(runs, "valE"), val_logits(runs, "valR"), val_logits(runs, "valS")
    assert ema.shape == (3, 4) and np.isfinite(ema).all()
    assert np.array_equal(ema.view(np.int32), swapped.view(np.int32))
    assert not np.array_equal(ema, raw) and np.abs(ema - raw).max() > 1e-4 * np.abs(raw).max()
    assert "Evaluating the averaged weights" in runs.logs("log_e2e_val_resume_*.log", "valE")
    assert "Evaluating the averaged weights" not in runs.logs("log_e2e_val_resume_*.log", "valR")
    with pytest.raises(Exception, match=r"x\.graph-4\.weights\.npz.*__optimizer__/ema|__optimizer__/ema.*x\.graph-4\.weights\.npz"):
        validate("valN", use_ema=True)
