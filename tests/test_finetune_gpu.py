"""Fine-tuning on the device: the tiered norm / update kernels (vl_*_tiers), LRCNEngine and GraphEngine with learning-rate tiers and
frozen dcnn layers (NetConfig.lr_mult / train_from), their pruned backward, the captured step, the data-parallel exchange and the
workflow.  Small shapes: 67x67x3 frames, 2 clips x 3 frames, hidden 8, 7 classes (tests/test_engine_gpu.py::test_train_step_small)."""
import glob
import math
import os
import socket

import numpy as np
import pytest
import torch
import yaml

from oracle import lrcn_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN = np.array([99.197148, 105.293620, 109.503945], np.float32)

# ---- kernels -------------------------------------------------------------------------------------------------------------------
COUNT = 4096 * 256 + 4099          # more elements than the grid has lanes (every lane loops), and a tail
# boundaries that are no multiple of 4, a tier of one element, a gap of one element (4099) and a wide one
TIERS = [(5, 1000, 1.0), (1000, 4099, 0.25), (4100, 4101, 2.0), (9001, COUNT, 3.0)]
LR = 0.0123


def f32(x):
    return float(np.float32(x))


def bits(t):
    return t.view(torch.int32)


def kernel_data(seed=0):
    """w, g, Adam m, v; g is NaN outside the tiers (an element there must never be loaded)."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    w, g, m = (torch.randn(COUNT, generator=gen) for _ in range(3))
    v = torch.rand(COUNT, generator=gen)
    inside = torch.zeros(COUNT, dtype=torch.bool)
    for lo, hi, _ in TIERS:
        inside[lo:hi] = True
    g[~inside] = float("nan")
    return [t.to(DEV) for t in (w, g, m, v)], inside.to(DEV)


def norm_word(g):
    from vltf_amd import ops
    ss, ws = torch.zeros(1, device=DEV), torch.empty(1024, device=DEV)
    ops.sumsq_tiers(g, TIERS, ss, ws)
    return ss


def state_block(step, lr, adam_lr=None):
    """A step state written by vl_step_state_set; adam_lr overrides the step-size word (float at byte 16 of vl_step_state)."""
    from vltf_amd import ops
    st = ops.step_state(DEV)
    ops.step_state_set(st, step, lr, 1)
    if adam_lr is not None:
        st.view(torch.float32)[4] = adam_lr
    return st


def test_sumsq_tiers():
    from vltf_amd import ops
    (w, g, m, v), inside = kernel_data()
    a, b = norm_word(g), norm_word(g)
    want = float((g[inside].double() ** 2).sum())
    assert math.isfinite(a.item()) and bits(a).item() == bits(b).item()
    assert abs(a.item() - want) <= 1e-6 * want, (a.item(), want)
    # a base address that is not 16-byte aligned (a slice of a flat buffer): the same elements, scalar or 16-byte loads
    g2 = torch.full((COUNT + 3,), float("nan"), device=DEV)
    g2[3:] = g
    ss, ws = torch.zeros(1, device=DEV), torch.empty(1024, device=DEV)
    ops.sumsq_tiers(g2[3:], TIERS, ss, ws)
    assert abs(ss.item() - want) <= 1e-6 * want


@pytest.mark.parametrize("clip", [0.0, 0.5])
@pytest.mark.parametrize("st", [False, True], ids=["eager", "st"])
def test_sgd_apply_tiers(clip, st):
    """Inside a tier: bit for bit the plain entry point on that slice with lr' = fl32(lr * mult); outside: untouched."""
    from vltf_amd import ops
    (w, g, m, v), inside = kernel_data()
    ss = norm_word(g)
    got = w.clone()
    if st:
        ops.sgd_apply_tiers_st(got, g, TIERS, state_block(7, LR), clip, ss)
    else:
        ops.sgd_apply_tiers(got, g, TIERS, LR, clip, ss)
    assert torch.equal(bits(got)[~inside], bits(w)[~inside])
    for lo, hi, mult in TIERS:
        lr_k = f32(np.float32(LR) * np.float32(mult))
        want = w[lo:hi].clone()
        if st:
            ops.sgd_apply_st(want, g[lo:hi].clone(), state_block(7, lr_k), clip, ss)
        else:
            ops.sgd_apply(want, g[lo:hi].clone(), lr_k, clip, ss)
        assert torch.isfinite(want).all() and not torch.equal(want, w[lo:hi])
        assert torch.equal(bits(got[lo:hi]), bits(want)), (lo, hi, mult)


@pytest.mark.parametrize("clip", [0.0, 0.5])
@pytest.mark.parametrize("st", [False, True], ids=["eager", "st"])
def test_adam_apply_tiers(clip, st):
    """Adam's step size in a tier is fl32(adam_lr * mult), adam_lr being the bias-corrected step size the host computes from lr
    (vl_step_state_set / vl_adam_apply share that code): the same in the eager and the step-state form, so a captured step equals the
    eager one.  Reference of every tier: the plain step-state entry point on the slice, its state's step-size word holding that
    product.  Where mult is a power of two the product is exact and the tier also equals, bit for bit, the plain eager entry point on
    the slice with lr' = fl32(lr * mult); for other factors that call rounds lr' * sqrt(1 - b2^t) / (1 - b1^t) once where the tier
    rounds twice, so it is not a bitwise reference (the last tier's 3.0)."""
    from vltf_amd import ops
    (w, g, m, v), inside = kernel_data(1)
    ss = norm_word(g)
    step = 3
    adam_lr = float(state_block(step - 1, LR).view(torch.float32)[4].item())
    gw, gm, gv = w.clone(), m.clone(), v.clone()
    if st:
        ops.adam_apply_tiers_st(gw, g, gm, gv, TIERS, state_block(step - 1, LR), clip, ss)
    else:
        ops.adam_apply_tiers(gw, g, gm, gv, TIERS, LR, step, clip, ss)
    for t0, t1 in ((gw, w), (gm, m), (gv, v)):
        assert torch.equal(bits(t0)[~inside], bits(t1)[~inside])
    for lo, hi, mult in TIERS:
        refs = [lambda a, b, c, d, mult=mult: ops.adam_apply_st(a, b, c, d, state_block(step - 1, LR, f32(np.float32(adam_lr) * np.float32(mult))),
                                                                 clip, ss)]
        if math.log2(mult) == int(math.log2(mult)):
            refs.append(lambda a, b, c, d, mult=mult: ops.adam_apply(a, b, c, d, f32(np.float32(LR) * np.float32(mult)), step, clip, ss))
        for ref in refs:
            ww, wm, wv = w[lo:hi].clone(), m[lo:hi].clone(), v[lo:hi].clone()
            ref(ww, g[lo:hi].clone(), wm, wv)
            assert torch.isfinite(ww).all() and not torch.equal(ww, w[lo:hi])
            for a, b in ((gw, ww), (gm, wm), (gv, wv)):
                assert torch.equal(bits(a[lo:hi]), bits(b)), (lo, hi, mult)


def test_tiers_skip_word_and_table_checks():
    from vltf_amd import ops
    from vltf_amd._ffi import VltfError
    (w, g, m, v), inside = kernel_data(2)
    ss = norm_word(g)
    skip = torch.ones(1, dtype=torch.int32, device=DEV)
    gw, gm, gv = w.clone(), m.clone(), v.clone()
    ops.sgd_apply_tiers(gw, g, TIERS, LR, 0.5, ss, skip=skip)
    ops.sgd_apply_tiers_st(gw, g, TIERS, state_block(0, LR), 0.5, ss, skip=skip)
    ops.adam_apply_tiers(gw, g, gm, gv, TIERS, LR, 1, 0.5, ss, skip=skip)
    ops.adam_apply_tiers_st(gw, g, gm, gv, TIERS, state_block(0, LR), 0.5, ss, skip=skip)
    for a, b in ((gw, w), (gm, m), (gv, v)):
        assert torch.equal(bits(a), bits(b))
    bad = [[(10, 20, 1.0), (5, 8, 1.0)],                        # not sorted
           [(0, 10, 1.0), (9, 20, 1.0)],                        # overlap
           [(0, COUNT + 1, 1.0)],                               # beyond count
           [(5, 5, 1.0)],                                       # empty
           [(i, i + 1, 1.0) for i in range(17)],                # more than VL_MAX_LR_TIERS
           [], [(0, 10, 0.0)], [(0, 10, -1.0)], [(0, 10, float("nan"))], [(0, 10, float("inf"))]]
    ws = torch.empty(1024, device=DEV)
    for table in bad:
        with pytest.raises(VltfError):
            ops.sgd_apply_tiers(gw, g, table, LR)
        with pytest.raises(VltfError):
            ops.sumsq_tiers(g, table, ss, ws)
    assert torch.equal(bits(gw), bits(w))
    ops.sgd_apply_tiers(gw, g, [(i, i + 1, 1.0) for i in range(5, 21)], LR)           # 16 tiers are fine
    assert torch.equal(bits(gw[21:1000]), bits(w[21:1000])) and not torch.equal(gw[5:21], w[5:21])


# ---- LRCNEngine ----------------------------------------------------------------------------------------------------------------
SHAPE, NCLS, FPC, B, HID = (67, 67, 3), 7, 3, 2, 8
CONV_LABELS = ["conv%d.%s" % (i, k) for i in range(1, 6) for k in ("fwd", "wgrad", "dgrad")]
_CASE = {}


def engine_case(layer, math, opt):
    """Parameters, inputs, the oracle's step and the gradients of an UNFROZEN engine for one (encode layer, arithmetic, optimizer);
    computed once and shared by the cases that freeze different layers."""
    key = (layer, math, opt)
    if key not in _CASE:
        from vltf_amd.engine import LRCNEngine, NetConfig
        rng = np.random.default_rng(5)
        cfg = NetConfig(image_shape=SHAPE, num_classes=NCLS, fpc=FPC, frame_encoding_layer=layer, lstm_hidden=HID, conv_math=math, optimizer=opt)
        p = O.init_params(rng, NCLS, layer, HID, 1, SHAPE, well_scaled=True)
        frames = rng.integers(0, 256, (B * FPC,) + SHAPE, dtype=np.uint8)
        onehot = O.labels_to_one_hot([[l] for l in rng.integers(0, NCLS, B)], NCLS)
        okey = ("oracle", layer)
        if okey not in _CASE:
            _CASE[okey] = O.lrcn_train_step(p, frames.astype(np.float32) - MEAN, onehot, FPC, lr=0.0, clip_norm=0.5, final_layer=layer)
        eng = LRCNEngine(cfg, max_clips=B, device=DEV)
        eng.load_params(p)
        out = eng.train_step_u8(torch.tensor(frames, device=DEV), torch.tensor(onehot, device=DEV), lr=0.0, clip_norm=0.5, mean_bgr=MEAN)
        _CASE[key] = dict(cfg=cfg, p=p, frames=frames, onehot=onehot, oracle=_CASE[okey], grads=eng.get_grads(), loss=out["loss"])
    return _CASE[key]


ENGINE_CASES = [(dict(lr_mult=4.0), "fc6", m, "sgd") for m in ("f32", "bf16x3", "bf16")] + \
               [(dict(train_from=t), "fc6", m, "sgd") for t in ("conv3", "fc6", "classifier") for m in ("f32", "bf16x3", "bf16")] + \
               [(dict(train_from="fc7", lr_mult=2.5), "fc7", "f32", "sgd"), (dict(train_from="fc6", lr_mult=4.0), "fc6", "f32", "adam")]


@pytest.mark.parametrize("kw,layer,arith,opt", ENGINE_CASES,
                         ids=["-".join([str(v) for v in kw.values()] + [layer, m, o]) for kw, layer, m, o in ENGINE_CASES])
def test_engine_finetune_step(kw, layer, arith, opt):
    import dataclasses
    from vltf_amd.engine import LRCNEngine, dcnn_layers, frozen_layers, is_regular
    case = engine_case(layer, arith, opt)
    cfg = dataclasses.replace(case["cfg"], **kw)
    p, grads_ref = case["p"], case["grads"]
    _, loss, _, _, _, ograds = case["oracle"]
    eng = LRCNEngine(cfg, max_clips=B, device=DEV)
    eng.load_params(p)
    frozen = set(eng.plan.frozen)
    assert frozen == {"dcnn/%s%s" % (l, k) for l in frozen_layers(cfg) for k in "Wb"}
    trainable = [k for k in p if k not in frozen]
    # whatever a frozen layer would have computed or read is NaN: its range of g, its dy / dp buffers; its Adam slots a sentinel
    for k in frozen:
        eng.G[k].fill_(float("nan"))
    for L in eng.layers[:eng.first_conv]:
        L["dy"].fill_(float("nan"))
        if "dp" in L:
            L["dp"].fill_(float("nan"))
    if opt == "adam":
        eng.adam_m.fill_(0.0), eng.adam_v.fill_(0.0)
        for k in frozen:
            off, n = eng.offsets[k]
            eng.adam_m[off:off + n] = 0.25
            eng.adam_v[off:off + n] = 0.75
    eng.set_probe(CONV_LABELS)
    lr, clip = (1e-3 if opt == "adam" else 0.01), 0.5
    out = eng.train_step_u8(torch.tensor(case["frames"], device=DEV), torch.tensor(case["onehot"], device=DEV), lr=lr, clip_norm=clip, mean_bgr=MEAN)
    labels = [l for l, _ in eng.probe_times_ms()]
    # 1. the chain above the cut is untouched: trainable gradients are those of the unfrozen engine, bit for bit
    g = eng.get_grads()
    assert sorted(g) == sorted(trainable)
    for k in trainable:
        assert np.array_equal(g[k], grads_ref[k]), k
    # 2. frozen: parameters as loaded, their range of g never written; everything finite
    got = eng.get_params()
    for k in frozen:
        assert np.array_equal(got[k], p[k]), k
        off, n = eng.offsets[k]
        assert bool(torch.isnan(eng.g[off:off + n]).all()), k
        if opt == "adam":
            assert bool((eng.adam_m[off:off + n] == 0.25).all()) and bool((eng.adam_v[off:off + n] == 0.75).all()), k
    assert math_isfinite(out["loss"], out["grad_norm"]) and all(np.isfinite(v).all() for v in got.values())
    assert out["loss"] == case["loss"]
    # 3. one global norm over the trainable gradients; w - lr m clip g with m = lr_mult for the modified variables
    gn = math.sqrt(sum(float((ograds[k].astype(np.float64) ** 2).sum()) for k in trainable))
    mult = {k: (1.0 if is_regular(k) else (cfg.lr_mult or 1.0)) for k in trainable}
    if arith == "bf16":         # reduced precision by design: the bounds of test_plain_bf16_conv_mode_runs_close
        assert abs(out["loss"] - loss) < 1e-2 * max(1, abs(loss)) and abs(out["grad_norm"] - gn) < 5e-2 * gn
        gn_dev = math.sqrt(sum(float((g[k].astype(np.float64) ** 2).sum()) for k in trainable))
        assert abs(out["grad_norm"] - gn_dev) < 1e-5 * gn_dev
        for k in trainable:                         # the update itself, from the engine's own gradients
            want = p[k].astype(np.float64) - lr * mult[k] * clip / max(gn_dev, clip) * g[k]
            np.testing.assert_allclose(got[k], want, rtol=1e-4, atol=1e-5, err_msg="param " + k)
    elif opt == "adam":
        assert abs(out["grad_norm"] - gn) < 1e-3 * gn
        newp = O.adam_update({k: p[k] for k in trainable}, {k: ograds[k] for k in trainable}, {}, lr, clip)
        clipped, _ = O.clip_by_global_norm({k: ograds[k] for k in trainable}, clip)
        for k in trainable:        # Adam's step is ~lr * mult whatever the gradient's size: the bounds of test_adam_steps_match_oracle
            want = p[k].astype(np.float64) + mult[k] * (newp[k].astype(np.float64) - p[k])
            d = np.abs(got[k] - want)
            tiny = np.abs(clipped[k]) < 1e-5
            assert d[~tiny].max(initial=0) <= 0.02 * lr * mult[k] + 1e-6 and d.max() <= lr * mult[k] + 1e-6, k
    else:
        assert abs(out["loss"] - loss) < 1e-4 * max(1, abs(loss)) and abs(out["grad_norm"] - gn) < 1e-3 * gn
        for k in trainable:
            want = p[k].astype(np.float64) - lr * mult[k] * clip / max(gn, clip) * ograds[k]
            np.testing.assert_allclose(got[k], want, rtol=1e-4, atol=1e-5, err_msg="param " + k)
        if cfg.lr_mult:
            moved = got["output_fc_w"].astype(np.float64) - p["output_fc_w"]
            assert np.abs(moved).max() > 0
    # 4. only trainable layers get a weight gradient, and an input gradient is computed only above the cut
    k0 = min(len(frozen_layers(cfg)), 5)
    assert [l for l in labels if l.endswith(".fwd")] == ["conv%d.fwd" % i for i in range(1, 6)]
    assert sorted(l for l in labels if l.endswith(".wgrad")) == ["conv%d.wgrad" % (i + 1) for i in range(k0, 5)]
    assert sorted(l for l in labels if l.endswith(".dgrad")) == ["conv%d.dgrad" % (i + 1) for i in range(k0 + 1, 5)]
    if k0 == 5:
        assert getattr(eng, "_side", None) is None                       # the second stream was never forked
    assert dcnn_layers(cfg)[-1] == layer


def math_isfinite(*xs):
    return all(math.isfinite(x) for x in xs)


def test_engine_refusals():
    from vltf_amd._ffi import VltfError
    from vltf_amd.engine import LRCNEngine, NetConfig
    small = dict(image_shape=SHAPE, num_classes=NCLS, fpc=FPC, lstm_hidden=HID)
    with pytest.raises(VltfError, match="no such layer"):
        LRCNEngine(NetConfig(train_from="fc7", **small), max_clips=B, device=DEV)
    with pytest.raises(VltfError, match="nothing to train"):
        LRCNEngine(NetConfig(image_shape=SHAPE, num_classes=NCLS, fpc=FPC, frame_encoding_layer="fc8", classifier="fc",
                             train_from="classifier"), max_clips=B, device=DEV)
    with pytest.raises(VltfError, match="lr_mult"):
        LRCNEngine(NetConfig(lr_mult=0.0, **small), max_clips=B, device=DEV)


# ---- captured step -------------------------------------------------------------------------------------------------------------
def test_captured_frozen_step_equals_eager():
    """train_from fc6 with Adam and lr_mult: step 1 is the warm-up, step 2 is captured and replayed, steps 3-5 are replays; the tier
    table travels in the captured launch's arguments."""
    from tests.test_step_graph_gpu import batch, pair, same_state, train_both
    eager, graph = pair(2, opt="adam", train_from="fc6", lr_mult=3.0)
    assert not eager.plan.full_range() and len(eager.plan.tiers) == 2
    p0 = eager.get_params()
    rng = np.random.default_rng(11)
    for step in range(5):
        train_both((eager, graph), batch(rng, 2, 4), lr=0.01 * (0.7 ** step))
    assert len(graph._graphs) == 1
    same_state(eager, graph)
    p1 = graph.get_params()
    for k in p0:
        assert np.array_equal(p0[k], p1[k]) == (k in eager.plan.frozen), k


# ---- data parallelism: one-rank RCCL ---------------------------------------------------------------------------------------------
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
    results = []
    for train_from in ("conv4", "classifier"):
        cfg = NetConfig(image_shape=shape, num_classes=ncls, fpc=fpc, lstm_hidden=hid, train_from=train_from, lr_mult=2.0)
        gar = dp.GradAllReduce(always=True)
        issued = []
        inner = gar.reduce_async
        gar.reduce_async = lambda flat, off, cnt, inner=inner, issued=issued: (issued.append((off, cnt)), inner(flat, off, cnt))[1]
        eng = LRCNEngine(cfg, max_clips=clips, device="cuda:0", dp=gar)
        ref = LRCNEngine(cfg, max_clips=clips, device="cuda:0")
        eng.load_params(p)
        ref.load_params(p)
        for k in eng.plan.frozen:
            eng.G[k].fill_(float("nan"))
        outs = []
        for _ in range(2):
            a = eng.train_step_u8(frames, onehot, lr=0.05, clip_norm=0.5, mean_bgr=MEAN)
            b = ref.train_step_u8(frames, onehot, lr=0.05, clip_norm=0.5, mean_bgr=MEAN)
            outs.append((a["loss"], b["loss"], a["grad_norm"], b["grad_norm"]))
        got, want = eng.get_params(), ref.get_params()
        same = all(np.array_equal(got[k], want[k]) for k in want) and all(o[0] == o[1] and o[2] == o[3] for o in outs)
        moved = [k for k in want if not np.array_equal(want[k], p[k])]
        frozen = set(eng.plan.frozen)
        ranges = [(eng.offsets[k][0], sum(eng.offsets[k])) for k in frozen]
        inside = all(lo + cnt <= a or lo >= b for lo, cnt in issued for a, b in ranges)
        steps_ok = issued == list(eng.plan.chunks) * 2
        # an empty shard: zero gradients into the exchange over the trainable ranges only, the same update as everywhere
        del issued[:]
        before = eng.get_params()
        out = eng.train_step_empty(lr=0.05, clip_norm=0.5)
        after = eng.get_params()
        empty_ok = issued == list(eng.plan.chunks) and all(np.array_equal(before[k], after[k]) for k in before) and out["grad_norm"] == 0.0
        nan_kept = all(bool(torch.isnan(eng.g[eng.offsets[k][0]:sum(eng.offsets[k])]).all()) for k in frozen)
        results.append(dict(train_from=train_from, same=same, moved=sorted(moved), frozen=sorted(frozen), inside=inside, steps_ok=steps_ok,
                            empty_ok=empty_ok, nan_kept=nan_kept, chunks=list(eng.plan.chunks), issued=gar.issued, outs=outs,
                            trainable=sorted(k for k in want if k not in frozen)))
    q.put(results)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_one_rank_rccl_frozen_step():
    """The exchange is handed exactly the plan's chunks, in order, none touching a frozen range; the step equals the plain frozen
    engine's bit for bit (one rank: the sum is the identity); train_step_empty leaves frozen weights alone."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    pr = ctx.Process(target=dp_worker, args=(free_port(), q))
    pr.start()
    pr.join(300)
    assert pr.exitcode == 0, "rank exited with %s" % pr.exitcode
    for r in q.get(timeout=10):
        assert r["steps_ok"] and r["inside"] and r["same"] and r["empty_ok"] and r["nan_kept"], r
        assert r["moved"] == r["trainable"] and r["frozen"], r
        assert r["issued"] == 3 * len(r["chunks"]), r


# ---- GraphEngine ---------------------------------------------------------------------------------------------------------------
def test_two_stream_one_tower_frozen():
    from tests import graph_cases as GC
    from tests.test_graph_gpu import device_feeds
    from vltf_amd.engine import is_regular
    from vltf_amd.graph import GraphEngine
    case = GC.CASES["two_stream_avg"]()
    pipes, ds = GC.specs_and_datasets(case)
    raw, feeds = GC.inputs(case)
    ref = GraphEngine(pipes, ds, case["V"], device=DEV)
    p = ref.init_params(seed=case["seed"], well_scaled=True)
    ref.load_params(p)
    logits, onehot, loss, ograds, _ = GC.expect(case, p, feeds)
    fd, od = device_feeds(raw), torch.from_numpy(onehot).to(DEV)
    ref.train_step(fd, od, lr=0.0, clip_norm=0.5)
    gref = ref.get_grads()
    import dataclasses
    frozen_pipes = [dataclasses.replace(sp, train_from={"rgb": "classifier", "flow": "conv3"}.get(sp.name)) for sp in pipes]
    eng = GraphEngine(frozen_pipes, ds, case["V"], device=DEV, lr_mult=4.0)
    eng.load_params(p)
    for k in eng.plan.frozen:
        eng.G[k].fill_(float("nan"))
    rgb, flow = eng.by_name["rgb"].tower, eng.by_name["flow"].tower
    called = []
    rgb._backward = lambda n, b: called.append("rgb")
    for L in list(rgb.layers) + list(flow.layers[:2]):
        L["dy"].fill_(float("nan"))
        if "dp" in L:
            L["dp"].fill_(float("nan"))
    out = eng.train_step(fd, od, lr=0.01, clip_norm=0.5)
    assert called == [] and len(eng.plan.tiers) == 2 and not eng.plan.full_range()
    frozen = set(eng.plan.frozen)
    assert frozen == {k for k in p if k.startswith("rgb/")} | {"flow/dcnn/conv%d%s" % (i, k) for i in (1, 2) for k in "Wb"}
    g = eng.get_grads()
    assert sorted(g) == sorted(k for k in p if k not in frozen)
    for k in g:
        assert np.array_equal(g[k], gref[k]), k
    gn = math.sqrt(sum(float((ograds[k].astype(np.float64) ** 2).sum()) for k in g))
    assert abs(out["loss"] - loss) < 1e-4 * max(1, abs(loss)) and abs(out["grad_norm"] - gn) < 1e-3 * gn
    got = eng.get_params()
    for k in p:
        if k in frozen:
            assert np.array_equal(got[k], p[k]), k
        else:
            want = p[k].astype(np.float64) - 0.01 * (1.0 if is_regular(k) else 4.0) * 0.5 / max(gn, 0.5) * ograds[k]
            np.testing.assert_allclose(got[k], want, rtol=1e-4, atol=1e-5, err_msg="param " + k)
    assert all(np.isfinite(v).all() for v in got.values())


# ---- workflow ------------------------------------------------------------------------------------------------------------------
def test_run_task_finetune(tmp_path, monkeypatch):
    """`lr_mult: 10` and `train_from: fc6` through run_task: the conv variables of the written checkpoint are the initial ones, bit
    for bit, every other variable has moved, and the log names the two tiers."""
    monkeypatch.setenv("VLTF_PREFETCH", "0")
    monkeypatch.setenv("VLTF_CONV_MATH", "f32")
    from tests.test_host_workflow import make_dataset
    from tests.test_run_task_gpu import RAW, WANT, write_cfg
    from vltf_amd import run_task
    from vltf_amd.engine import NetConfig, init_params
    folder = str(tmp_path)
    train_path, _, _ = make_dataset(folder, "train.txt", shape=RAW, seed=1)
    path = write_cfg(folder, "train.yml", train_path, "train", epochs=1)
    with open(path) as f:
        cfg = yaml.safe_load(f)
    cfg["run"]["train"]["lr_mult"] = 10
    cfg["run"]["train"]["base_lr"] = 0.01              # large enough that three steps move even a bias of 0.1 by more than its ulp
    cfg["run"]["network"]["pipelines"][0]["lrcn"]["train_from"] = "fc6"
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    run_task.main(path, seed=3)
    run = os.path.join(folder, "run")
    ck = glob.glob(os.path.join(run, "checkpoints", "*.weights.npz"))
    assert len(ck) == 1
    with np.load(ck[0], allow_pickle=False) as z:
        saved = {k: z[k] for k in z.files}
    init = init_params(NetConfig(image_shape=WANT, num_classes=4, fpc=3, lstm_hidden=8), seed=3)
    assert set(init) <= set(saved)                                       # checkpoints keep every variable
    for k, v in init.items():
        if k.startswith("dcnn/conv"):
            assert np.array_equal(saved[k], v), k
        else:
            assert not np.array_equal(saved[k], v), k
    log = open(glob.glob(os.path.join(run, "log_e2e_train_scratch_*.log"))[0]).read()
    assert "Setting up two-tier training with a factor of 10.0" in log and "output_fc_w" in log.split("two-tier")[1].split("\n")[0]
    assert "dcnn/conv1W" in log.split("Frozen (train_from)")[1].split("\n")[0]
