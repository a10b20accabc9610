"""SGD with momentum / Nesterov on the device (vl_momentum_apply, NetConfig.momentum): the rule of tf.train.MomentumOptimizer --
    gi = g * clip scale;  a' = momentum * a + gi;  w' = w - lr * a'   (nesterov: w - lr * (gi + momentum * a'))
-- against float64, through learning-rate tiers bit for bit, under the skip word, in LRCNEngine (eager and captured, with frozen
layers), GraphEngine, one-rank RCCL and the checkpoint of run_task.  Small shapes: 67x67x3 frames, 2 clips x 3 frames, hidden 8, 7
classes.  Tolerance of every comparison with float64: the one of the two-step Adam check of tests/test_ops_gpu.py::test_optimizer,
rtol 1e-5 and atol 1e-6 * max|want| (three fp32 roundings per element and step, each 6e-8 relative to a term no larger than a few
max|want|)."""
import glob
import math
import os
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
MOM = 0.9


def f32(x):
    return float(np.float32(x))


def bits(t):
    return t.view(torch.int32)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def close(got, want, msg=""):
    want = np.asarray(want, np.float64)
    scale = float(np.abs(want).max()) or 1.0
    np.testing.assert_allclose(np.asarray(got, np.float64), want, rtol=1e-5, atol=1e-6 * scale, err_msg=msg)


def rule(w, a, g, lr, sc, nesterov, momentum=MOM):
    """One step in float64 -> (w', a')."""
    gi = np.asarray(g, np.float64) * sc
    a = momentum * np.asarray(a, np.float64) + gi
    return np.asarray(w, np.float64) - lr * ((gi + momentum * a) if nesterov else a), a


def clip_scale(clip, norm, gscale=1.0):
    return gscale * (clip / max(gscale * norm, clip) if clip > 0 else 1.0)


# ---- 1. the rule against float64 ---------------------------------------------------------------------------------------------------
N1 = 100003
_DATA1 = {}


def data1():
    """w ~ N(0, 1) and three gradients ~ 3 N(0, 1), as tests/test_ops_gpu.py::test_optimizer; made once, never written."""
    if not _DATA1:
        rng = np.random.default_rng(2)
        _DATA1["w"] = rng.standard_normal(N1).astype(np.float32)
        _DATA1["g"] = [(rng.standard_normal(N1) * 3).astype(np.float32) for _ in range(3)]
    return _DATA1["w"], _DATA1["g"]


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("clip,gscale", [(0.0, 1.0), (10.0, 1.0), (10.0, 0.125)])
@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
def test_rule_against_fp64(nesterov, clip, gscale, offset):
    """Three calls, a fresh gradient and another lr each: the accumulator holds gradients, not lr * gradients (the Caffe form, which
    the changing lr tells apart).  offset 1: views w[1:], g[1:], a[1:] of 16-byte aligned buffers -- three scalar head elements, then
    16-byte accesses."""
    from vltf_amd import ops
    w, gs = data1()
    o = offset
    wd = torch.zeros(N1 + o, device=DEV)
    ad = torch.zeros(N1 + o, device=DEV)
    gd = torch.zeros(N1 + o, device=DEV)
    wd[o:] = torch.from_numpy(w).to(DEV)
    wv, av, gv = wd[o:], ad[o:], gd[o:]
    ss, ws = torch.zeros(1, device=DEV), torch.empty(1024, device=DEV)
    wr, ar = w.astype(np.float64), np.zeros(N1)
    for g, lr in zip(gs, (0.01, 0.02, 0.005)):
        gv.copy_(torch.from_numpy(g).to(DEV))
        ops.sumsq(gv, ss, ws)
        ops.momentum_apply(wv, gv, av, lr, MOM, nesterov, clip, ss, gscale)
        norm = math.sqrt(float((g.astype(np.float64) ** 2).sum()))
        wr, ar = rule(wr, ar, g, lr, clip_scale(clip, norm, gscale), nesterov)
        close(host(wv), wr, "w")
        close(host(av), ar, "accumulator")
    if o:
        assert host(wd)[0] == 0.0 and host(ad)[0] == 0.0          # the element before the views


# ---- 2. tiers, bit for bit (COUNT, TIERS, LR and the NaN-outside g of tests/test_finetune_gpu.py, restated) -------------------------
COUNT = 4096 * 256 + 4099          # more elements than the grid has lanes (every lane loops), and a tail
# boundaries that are no multiple of 4, a tier of one element, a gap of one element (4099) and a wide one
TIERS = [(5, 1000, 1.0), (1000, 4099, 0.25), (4100, 4101, 2.0), (9001, COUNT, 3.0)]
LR = 0.0123


def kernel_data(seed=0):
    """w, g, a random accumulator; g is NaN outside the tiers (an element there must never be loaded)."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    w, g, a = (torch.randn(COUNT, generator=gen) for _ in range(3))
    inside = torch.zeros(COUNT, dtype=torch.bool)
    for lo, hi, _ in TIERS:
        inside[lo:hi] = True
    g[~inside] = float("nan")
    return [t.to(DEV) for t in (w, g, a)], inside.to(DEV)


def norm_word(g):
    from vltf_amd import ops
    ss, ws = torch.zeros(1, device=DEV), torch.empty(1024, device=DEV)
    ops.sumsq_tiers(g, TIERS, ss, ws)
    return ss


def state_block(step, lr):
    from vltf_amd import ops
    st = ops.step_state(DEV)
    ops.step_state_set(st, step, lr, 1)
    return st


@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
@pytest.mark.parametrize("clip", [0.0, 0.5])
@pytest.mark.parametrize("st", [False, True], ids=["eager", "st"])
def test_momentum_apply_tiers(st, clip, nesterov):
    """Inside a tier: w and the accumulator are, bit for bit, the full-range call on the cloned slice with lr' = fl32(lr * mult);
    outside every tier both keep their bits (and g, NaN there, is never loaded).  The step-state form equals the eager one."""
    from vltf_amd import ops
    (w, g, a), inside = kernel_data()
    ss = norm_word(g)
    gw, ga = w.clone(), a.clone()
    if st:
        ops.momentum_apply_st(gw, g, ga, state_block(7, LR), MOM, nesterov, clip, ss, tiers=TIERS)
        ew, ea = w.clone(), a.clone()
        ops.momentum_apply(ew, g, ea, LR, MOM, nesterov, clip, ss, tiers=TIERS)
        assert torch.equal(bits(gw), bits(ew)) and torch.equal(bits(ga), bits(ea))
    else:
        ops.momentum_apply(gw, g, ga, LR, MOM, nesterov, clip, ss, tiers=TIERS)
    assert torch.equal(bits(gw)[~inside], bits(w)[~inside]) and torch.equal(bits(ga)[~inside], bits(a)[~inside])
    for lo, hi, mult in TIERS:
        lr_k = f32(np.float32(LR) * np.float32(mult))
        ww, wa = w[lo:hi].clone(), a[lo:hi].clone()
        if st:
            ops.momentum_apply_st(ww, g[lo:hi].clone(), wa, state_block(7, lr_k), MOM, nesterov, clip, ss)
        else:
            ops.momentum_apply(ww, g[lo:hi].clone(), wa, lr_k, MOM, nesterov, clip, ss)
        assert torch.isfinite(ww).all() and torch.isfinite(wa).all()
        assert not torch.equal(ww, w[lo:hi]) and not torch.equal(wa, a[lo:hi])
        assert torch.equal(bits(gw[lo:hi]), bits(ww)) and torch.equal(bits(ga[lo:hi]), bits(wa)), (lo, hi, mult)
    if clip > 0:
        return
    # without clipping (scale exactly 1) the bits are the documented rounding order: a' = fma(m, a, g); w' = fma(-lr_k, a' | fma(m, a', g), w)
    lo, hi, mult = TIERS[1]
    w64, a64 = (host(t[lo:hi]).astype(np.float64) for t in (w, a))
    gi = host(g[lo:hi])
    a1 = (np.float64(np.float32(MOM)) * a64 + gi).astype(np.float32)                # (a product of two floats is exact in float64)
    u = (np.float64(np.float32(MOM)) * a1 + gi).astype(np.float32) if nesterov else a1
    w1 = (w64 - np.float64(np.float32(LR) * np.float32(mult)) * u).astype(np.float32)
    # float64 rounds once more before the float32 rounding: a double rounding can differ from the fused one in the last bit, rarely
    assert np.mean(host(ga[lo:hi]) == a1) > 0.999 and np.abs(host(ga[lo:hi]).astype(np.float64) - a1).max() <= np.abs(a1).max() * 2.0 ** -23
    assert np.mean(host(gw[lo:hi]) == w1) > 0.999 and np.abs(host(gw[lo:hi]).astype(np.float64) - w1).max() <= np.abs(w1).max() * 2.0 ** -23


# ---- 3. skip word and argument checks ---------------------------------------------------------------------------------------------
def test_skip_word_and_argument_checks():
    from vltf_amd import ops
    from vltf_amd._ffi import VltfError
    (w, g, a), inside = kernel_data(2)
    ss = norm_word(g)
    skip = torch.ones(1, dtype=torch.int32, device=DEV)
    gw, ga = w.clone(), a.clone()
    for nesterov in (False, True):
        ops.momentum_apply(gw, g, ga, LR, MOM, nesterov, 0.5, ss, skip=skip, tiers=TIERS)
        ops.momentum_apply_st(gw, g, ga, state_block(0, LR), MOM, nesterov, 0.5, ss, skip=skip, tiers=TIERS)
        ops.momentum_apply(gw[5:1000], g[5:1000], ga[5:1000], LR, MOM, nesterov, skip=skip)
    assert torch.equal(bits(gw), bits(w)) and torch.equal(bits(ga), bits(a))
    st = state_block(0, LR)
    for m in (0.0, 1.0, -0.5, 1.5, float("nan")):
        with pytest.raises(VltfError, match="momentum"):
            ops.momentum_apply(gw, g, ga, LR, m, tiers=TIERS)
        with pytest.raises(VltfError, match="momentum"):
            ops.momentum_apply_st(gw, g, ga, st, m, tiers=TIERS)
    with pytest.raises(VltfError):
        ops.momentum_apply(gw, g, None, LR, MOM, tiers=TIERS)                       # a null accumulator
    with pytest.raises(VltfError):
        ops.momentum_apply_st(gw, g, None, st, MOM, tiers=TIERS)
    with pytest.raises(VltfError):
        ops.momentum_apply(gw, g, ga[:-1], LR, MOM, tiers=TIERS)                    # an accumulator of another size
    with pytest.raises(VltfError):
        ops.momentum_apply_st(gw, g, ga, None, MOM, tiers=TIERS)                    # no step state
    for table in ([(0, 10, 1.0), (9, 20, 1.0)], [(10, 20, 1.0), (5, 8, 1.0)], [(0, COUNT + 1, 1.0)], [], [(0, 10, 0.0)],
                  [(i, i + 1, 1.0) for i in range(17)]):
        with pytest.raises(VltfError):
            ops.momentum_apply(gw, g, ga, LR, MOM, tiers=table)
        with pytest.raises(VltfError):
            ops.momentum_apply_st(gw, g, ga, st, MOM, tiers=table)
    torch.cuda.synchronize()
    assert torch.equal(bits(gw), bits(w)) and torch.equal(bits(ga), bits(a))
    skip.zero_()                                                                       # the word cleared: the same call updates
    ops.momentum_apply(gw, g, ga, LR, MOM, False, 0.5, ss, skip=skip, tiers=TIERS)
    assert not torch.equal(gw[inside], w[inside]) and not torch.equal(ga[inside], a[inside])


# ---- 4. LRCNEngine ------------------------------------------------------------------------------------------------------------------
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


def check_steps(eng, step_fn, lrs, nesterov, mult=None, frozen=(), acc0=None):
    """Runs step_fn(i, lr) per lr; after each, parameters and accumulator must be the rule in float64 applied to the parameters read
    before the step, with the engine's own gradients and norm (the gradient path is not under test).  mult: {name: lr factor}."""
    acc = {k: (np.zeros(n) if acc0 is None else acc0[off:off + n].astype(np.float64)) for k, (off, n) in eng.offsets.items()}
    for i, lr in enumerate(lrs):
        before = eng.get_params()
        out = step_fn(i, lr)
        g, after, mom = eng.get_grads(), eng.get_params(), host(eng.mom)
        assert math.isfinite(out["loss"])
        gn = math.sqrt(sum(float((v.astype(np.float64) ** 2).sum()) for v in g.values()))
        assert abs(out["grad_norm"] - gn) <= 1e-5 * gn
        sc = clip_scale(CLIP, out["grad_norm"])
        for k, (off, n) in eng.offsets.items():
            if k in frozen:
                assert np.array_equal(after[k], before[k]), k
                continue
            want_w, acc[k] = rule(before[k].ravel(), acc[k], g[k].ravel(), lr * (mult[k] if mult else 1.0), sc, nesterov)
            close(after[k].ravel(), want_w, "param %s step %d" % (k, i))
            close(mom[off:off + n], acc[k], "accumulator %s step %d" % (k, i))
        assert any(not np.array_equal(after[k], before[k]) for k in after)


@pytest.mark.parametrize("arith,nesterov", [("f32", False), ("f32", True), ("bf16", False)], ids=["f32", "f32-nesterov", "bf16"])
def test_engine_three_steps(arith, nesterov):
    from vltf_amd.engine import LRCNEngine
    p, batches = small_batches(3)
    eng = LRCNEngine(small_cfg(conv_math=arith, momentum=MOM, nesterov=nesterov), max_clips=B, device=DEV)
    eng.load_params(p)
    assert eng.mom is not None and eng.mom.numel() == eng.w.numel() and not bool(eng.mom.any())
    check_steps(eng, lambda i, lr: eng.train_step_u8(*batches[i], lr=lr, clip_norm=CLIP, mean_bgr=MEAN), LRS, nesterov)


def test_engine_refusals_and_plain_sgd_allocates_nothing():
    from vltf_amd._ffi import VltfError
    from vltf_amd.engine import LRCNEngine
    for kw, msg in ((dict(momentum=1.0), r"\[0, 1\)"), (dict(momentum=-0.1), r"\[0, 1\)"), (dict(nesterov=True), "nesterov"),
                    (dict(momentum=0.9, optimizer="adam"), "adam"), (dict(nesterov=True, optimizer="adam"), "nesterov|adam")):
        with pytest.raises(VltfError, match=msg):
            LRCNEngine(small_cfg(**kw), max_clips=B, device=DEV)
    assert LRCNEngine(small_cfg(), max_clips=B, device=DEV).mom is None
    assert LRCNEngine(small_cfg(momentum=MOM), max_clips=B, device=DEV, training=False).mom is None
    eng = LRCNEngine(small_cfg(), max_clips=B, device=DEV)
    assert not any(k.endswith("momentum") for k in eng.get_opt_state()) and eng.load_opt_state(eng.get_opt_state()) == []


def test_engine_opt_state_round_trip():
    from vltf_amd._ffi import VltfError
    from vltf_amd.engine import LRCNEngine
    eng = LRCNEngine(small_cfg(momentum=MOM), max_clips=B, device=DEV)
    eng.mom.copy_(torch.arange(eng.mom.numel(), device=DEV) % 7)
    st = eng.get_opt_state()
    key = eng.OPT_PREFIX + "momentum"
    assert key in st and st[key].shape == (eng.w.numel(),)
    other = LRCNEngine(small_cfg(momentum=MOM), max_clips=B, device=DEV)
    assert other.load_opt_state(st) == [] and torch.equal(other.mom, eng.mom)
    bare = {k: v for k, v in st.items() if k != key}
    assert other.load_opt_state(bare) == [key]                                  # reported: the caller warns, the accumulator stays
    with pytest.raises(VltfError, match="shape"):
        other.load_opt_state({**st, key: st[key][:-1]})


# ---- 5. captured equals eager -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
def test_captured_momentum_step_equals_eager(nesterov):
    """Step 1 is the warm-up, step 2 is captured and replayed, step 3 is a replay; lr changes every step (it comes from the step
    state).  Parameters and accumulator are bit-equal after each step."""
    from tests.test_step_graph_gpu import batch, pair, same_state, train_both
    eager, graph = pair(B, fpc=FPC, hid=HID, momentum=MOM, nesterov=nesterov)
    assert eager.plan.full_range()
    rng = np.random.default_rng(11)
    for step, lr in enumerate(LRS):
        train_both((eager, graph), batch(rng, B, FPC), lr=lr)
        same_state(eager, graph)
        assert torch.equal(bits(eager.mom), bits(graph.mom)) and bool(eager.mom.any())
    assert len(graph._graphs) == 1 and "__optimizer__/momentum" in graph.get_opt_state()


# ---- 6. with fine-tuning ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "captured"])
def test_momentum_with_finetuning(graph):
    """train_from fc6 and lr_mult 4: the accumulator's frozen ranges keep a sentinel, the trained ranges follow the rule with lr * mult
    (the tier changes lr only, never the accumulator)."""
    from vltf_amd.engine import LRCNEngine, is_regular
    p, batches = small_batches(2)
    eng = LRCNEngine(small_cfg(momentum=MOM, train_from="fc6", lr_mult=4.0, step_graph=graph), max_clips=B, device=DEV)
    eng.load_params(p)
    frozen = set(eng.plan.frozen)
    assert frozen == {"dcnn/conv%d%s" % (i, k) for i in range(1, 6) for k in "Wb"} and len(eng.plan.tiers) == 2
    for k in frozen:
        off, n = eng.offsets[k]
        eng.mom[off:off + n] = 0.25
        eng.G[k].fill_(float("nan"))
    mult = {k: (1.0 if is_regular(k) else 4.0) for k in p}
    assert sorted(set(mult.values())) == [1.0, 4.0]
    check_steps(eng, lambda i, lr: eng.train_step_u8(*batches[i], lr=lr, clip_norm=CLIP, mean_bgr=MEAN), LRS[:2], False, mult, frozen,
                acc0=host(eng.mom).copy())
    for k in frozen:
        off, n = eng.offsets[k]
        assert bool((eng.mom[off:off + n] == 0.25).all()), k
        assert bool(torch.isnan(eng.g[off:off + n]).all()), k


# ---- 7. GraphEngine -----------------------------------------------------------------------------------------------------------------
def test_graph_engine_two_steps():
    from tests import graph_cases as GC
    from tests.test_graph_gpu import device_feeds
    from vltf_amd._ffi import VltfError
    from vltf_amd.graph import GraphEngine
    case = GC.CASES["encdec_state"]()                   # two pipelines, one tower of 2-frame clips: the smallest of graph_cases
    pipes, ds = GC.specs_and_datasets(case)
    with pytest.raises(VltfError, match="adam"):
        GraphEngine(pipes, ds, case["V"], device=DEV, optimizer="adam", momentum=MOM)
    with pytest.raises(VltfError, match="nesterov"):
        GraphEngine(pipes, ds, case["V"], device=DEV, nesterov=True)
    assert GraphEngine(pipes, ds, case["V"], device=DEV).mom is None
    eng = GraphEngine(pipes, ds, case["V"], device=DEV, momentum=MOM, nesterov=True)
    eng.load_params(eng.init_params(seed=case["seed"], well_scaled=True))
    raw, feeds = GC.inputs(case)
    fd = device_feeds(raw)
    eng.forward(fd)
    rows = eng.logits_host().shape[0]
    onehot = torch.tensor(O.labels_to_one_hot([[l] for l in np.random.default_rng(0).integers(0, case["V"], rows)], case["V"]), device=DEV)
    eng.offsets, off = {}, 0                            # name -> (offset, count) of the flat buffers, for check_steps
    for name, shp in eng.specs:
        eng.offsets[name] = (off, int(np.prod(shp)))
        off += int(np.prod(shp))
    assert off == eng.mom.numel()
    check_steps(eng, lambda i, lr: eng.train_step(fd, onehot, lr=lr, clip_norm=CLIP), LRS[:2], True)
    assert eng.OPT_PREFIX + "momentum" in eng.get_opt_state()


# ---- 8. one-rank RCCL ---------------------------------------------------------------------------------------------------------------
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
    cfg = NetConfig(image_shape=shape, num_classes=ncls, fpc=fpc, lstm_hidden=hid, momentum=0.9)
    eng = LRCNEngine(cfg, max_clips=clips, device="cuda:0", dp=dp.GradAllReduce(always=True))
    ref = LRCNEngine(cfg, max_clips=clips, device="cuda:0")
    eng.load_params(p)
    ref.load_params(p)
    outs = []
    for lr in (0.05, 0.02):
        a = eng.train_step_u8(frames, onehot, lr=lr, clip_norm=0.5, mean_bgr=MEAN)
        b = ref.train_step_u8(frames, onehot, lr=lr, clip_norm=0.5, mean_bgr=MEAN)
        outs.append((a["loss"], b["loss"], a["grad_norm"], b["grad_norm"]))
    got, want = eng.get_params(), ref.get_params()
    torch.cuda.synchronize()
    q.put(dict(same=all(np.array_equal(got[k], want[k]) for k in want) and all(o[0] == o[1] and o[2] == o[3] for o in outs),
               moved=all(not np.array_equal(want[k], p[k]) for k in want),
               mom_same=bool(torch.equal(eng.mom.view(torch.int32), ref.mom.view(torch.int32))), mom_set=bool(eng.mom.any()), outs=outs))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_one_rank_rccl_momentum_step():
    """Two momentum steps under a one-rank process group equal the engine without data parallelism bit for bit, accumulator included
    (the update runs after the exchange, on the reduced gradient)."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    pr = ctx.Process(target=dp_worker, args=(free_port(), q))
    pr.start()
    pr.join(300)
    assert pr.exitcode == 0, "rank exited with %s" % pr.exitcode
    r = q.get(timeout=10)
    assert r["same"] and r["moved"] and r["mom_same"] and r["mom_set"], r


# ---- 9. resume equals uninterrupted ------------------------------------------------------------------------------------------------
def test_momentum_resume_equals_uninterrupted(tmp_path, monkeypatch):
    """The checkpoint keeps the accumulator (`__optimizer__/momentum`): a run resumed from the end-of-epoch-1 checkpoint ends with
    exactly the weights of the uninterrupted 2-epoch run; a weights-only file resumes with a warning and a zero accumulator."""
    monkeypatch.setenv("VLTF_PREFETCH", "0")
    monkeypatch.setenv("VLTF_CONV_MATH", "f32")
    from tests.test_host_workflow import make_dataset
    from tests.test_run_task_gpu import RAW, write_cfg
    from vltf_amd import run_task
    folder = str(tmp_path)
    train_path, _, _ = make_dataset(folder, "train.txt", shape=RAW, seed=1)

    def cfg(name, **kw):
        path = write_cfg(folder, name, train_path, "train", epochs=2, det=True, run="runA", **kw)
        with open(path) as f:
            c = yaml.safe_load(f)
        c["run"]["train"].update(momentum=0.9, base_lr=0.01)
        with open(path, "w") as f:
            yaml.safe_dump(c, f)
        return path

    def final_weights():
        ck = sorted(glob.glob(os.path.join(folder, "runA", "checkpoints", "*.weights.npz")), key=os.path.getmtime)
        with np.load(ck[-1], allow_pickle=False) as z:
            return ck, {k: z[k] for k in z.files}

    run_task.main(cfg("a.yml"), seed=3)
    ck, full = final_weights()
    assert len(ck) == 2 and int(full["__optimizer__/step_count"][0]) == 6
    assert "__optimizer__/momentum" in full and np.abs(full["__optimizer__/momentum"]).max() > 0
    first = ck[0][:-len(".weights.npz")]
    with np.load(first + ".weights.npz", allow_pickle=False) as z:
        assert np.abs(z["__optimizer__/momentum"]).max() > 0
    run_task.main(cfg("b.yml", resume=first), seed=77)
    _, resumed = final_weights()
    assert int(resumed["__optimizer__/step_count"][0]) == 6
    for k in full:
        np.testing.assert_array_equal(resumed[k], full[k], err_msg=k)
    # a weights-only checkpoint: a warning, a zero accumulator -- so the run ends elsewhere
    bare = os.path.join(folder, "runA", "checkpoints", "bare.graph-3")
    np.savez(bare + ".weights.npz", **{k: v for k, v in np.load(first + ".weights.npz").items() if not k.startswith("__optimizer__/")})
    shutil.copy(first + ".snap", bare + ".snap")
    run_task.main(cfg("c.yml", resume=bare), seed=77)
    log = "".join(open(f).read() for f in glob.glob(os.path.join(folder, "runA", "log_e2e_train_resume_*.log")))
    assert "no optimizer state" in log and "__optimizer__/momentum" in log
    _, fresh = final_weights()
    assert not np.array_equal(fresh["output_fc_w"], full["output_fc_w"])
