"""Gradient accumulation on the device: vl_grad_accumulate bit for bit against numpy, vl_step_state_set_micro, and one update of k
micro-steps in LRCNEngine (against the fp64 oracle on the concatenated batch, every optimizer, weight decay, fine-tuning, captured,
the bf16 path, one-rank RCCL), GraphEngine and run_task.  Small shapes throughout: 67x67x3 frames, micro-batches of 2 clips x 3 frames,
hidden 8, 7 classes.  Tolerances against the oracle and between a k-step update and the plain step on the whole batch are those of
tests/test_engine_gpu.py::test_train_step_small, restated: loss 1e-4 * max(1, |loss|); gradients rtol 2e-3, atol 2e-4 * max|grad|;
parameters rtol 1e-4, atol 1e-5."""
import glob
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


def bits(t):
    return t.view(torch.int32)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def close_params(got, want, names=None):
    for k in (names or want):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-4, atol=1e-5, err_msg="param " + k)


def close_grads(got, want):
    for k in want:
        scale = np.abs(want[k]).max() + 1e-12
        np.testing.assert_allclose(got[k], want[k], rtol=2e-3, atol=2e-4 * scale, err_msg="grad " + k)


# ---- A. the kernel ------------------------------------------------------------------------------------------------------------------
COUNT = 4096 * 256 + 4099          # more elements than the grid has lanes (every lane loops), and a tail
# (tests/test_momentum_gpu.py's table, restated) boundaries that are no multiple of 4, a range of one element, a gap of one element
RANGES = [(5, 1000, 1.0), (1000, 4099, 0.25), (4100, 4101, 2.0), (9001, COUNT, 3.0)]
STORE, ADD, FINAL = 0, 1, 2


def ranged_pair(seed):
    """acc and g, random inside RANGES, NaN outside (an element there must be neither loaded nor stored), and the inside mask."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    acc, g = torch.randn(COUNT, generator=gen), torch.randn(COUNT, generator=gen)
    inside = torch.zeros(COUNT, dtype=torch.bool)
    for lo, hi, _ in RANGES:
        inside[lo:hi] = True
    acc[~inside] = float("nan")
    g[~inside] = float("nan")
    return acc, g, inside


@pytest.mark.parametrize("mode", [STORE, ADD, FINAL], ids=["store", "add", "final"])
def test_kernel_bitwise_against_numpy(mode):
    from vltf_amd import ops
    acc, g, inside = ranged_pair(mode)
    a_np, g_np, m = acc.numpy(), g.numpy(), inside.numpy()
    da, dg = acc.to(DEV), g.to(DEV)
    ops.grad_accumulate(da, dg, mode, RANGES)
    ga, gg = host(da), host(dg)
    want_a, want_g = a_np.copy(), g_np.copy()
    total = np.add(a_np[m], g_np[m], dtype=np.float32)
    if mode == STORE:
        want_a[m] = g_np[m]
    elif mode == ADD:
        want_a[m] = total
    else:
        want_g[m] = total
    assert np.isfinite(ga[m]).all() and np.isfinite(gg[m]).all()
    assert np.array_equal(ga.view(np.int32), want_a.view(np.int32))       # inside: exact; outside: acc keeps its (NaN) bits
    assert np.array_equal(gg.view(np.int32), want_g.view(np.int32))       # and so does g
    changed = ga if mode != FINAL else gg
    assert not np.array_equal(changed[m], (a_np if mode != FINAL else g_np)[m])


@pytest.mark.parametrize("oa,og", [(0, 0), (1, 1), (0, 1)], ids=["aligned", "offset1", "phases-disagree"])
@pytest.mark.parametrize("mode", [STORE, ADD, FINAL], ids=["store", "add", "final"])
def test_kernel_alignment_full_range(mode, oa, og):
    """n_ranges == 0 is the full range.  (1, 1): views one float into 16-byte aligned buffers, three scalar head elements; (0, 1): the
    16-byte phases of acc and g disagree, scalar loops only.  The element before each view is not touched."""
    from vltf_amd import ops
    n = 100003
    gen = torch.Generator(device="cpu").manual_seed(7)
    a_np, g_np = torch.randn(n, generator=gen).numpy(), torch.randn(n, generator=gen).numpy()
    da, dg = torch.full((n + 1,), 7.0, device=DEV), torch.full((n + 1,), 9.0, device=DEV)
    va, vg = da[oa:oa + n], dg[og:og + n]
    va.copy_(torch.from_numpy(a_np))
    vg.copy_(torch.from_numpy(g_np))
    ops.grad_accumulate(va, vg, mode)
    total = np.add(a_np, g_np, dtype=np.float32)
    want_a = g_np if mode == STORE else total if mode == ADD else a_np
    want_g = total if mode == FINAL else g_np
    assert np.array_equal(host(va).view(np.int32), want_a.view(np.int32)) and np.array_equal(host(vg).view(np.int32), want_g.view(np.int32))
    assert host(da)[0 if oa else n] == 7.0 and host(dg)[0 if og else n] == 9.0


def test_kernel_chunk_sub_range():
    """The data-parallel use: one range {lo, lo + cnt} with lo no multiple of 4, everything else NaN."""
    from vltf_amd import ops
    lo, cnt = 4099, 70001
    acc, g, _ = ranged_pair(3)
    acc, g = torch.nan_to_num(acc, nan=1.0), torch.nan_to_num(g, nan=2.0)
    acc[:lo], acc[lo + cnt:], g[:lo], g[lo + cnt:] = [float("nan")] * 4
    da, dg = acc.to(DEV), g.to(DEV)
    ops.grad_accumulate(da, dg, FINAL, [(lo, lo + cnt, 1.0)])
    want = g.numpy().copy()
    want[lo:lo + cnt] = np.add(acc.numpy()[lo:lo + cnt], g.numpy()[lo:lo + cnt], dtype=np.float32)
    assert np.array_equal(host(dg).view(np.int32), want.view(np.int32)) and np.isfinite(want[lo:lo + cnt]).all()
    assert np.array_equal(host(da).view(np.int32), acc.numpy().view(np.int32))


def test_kernel_summation_order():
    """store, add, final = ((g1 + g2) + g3) in fp32, bit for bit (magnitudes spread so that the order shows)."""
    from vltf_amd import ops
    gen = torch.Generator(device="cpu").manual_seed(5)
    g1, g2, g3 = (torch.randn(COUNT, generator=gen) * s for s in (1.0, 1e-4, 1e3))
    acc, g = torch.full((COUNT,), float("nan"), device=DEV), torch.empty(COUNT, device=DEV)
    for src, mode in ((g1, STORE), (g2, ADD), (g3, FINAL)):
        g.copy_(src)
        ops.grad_accumulate(acc, g, mode, [(0, COUNT, 1.0)])
    want = np.add(np.add(g1.numpy(), g2.numpy(), dtype=np.float32), g3.numpy(), dtype=np.float32)
    other = np.add(g1.numpy(), np.add(g2.numpy(), g3.numpy(), dtype=np.float32), dtype=np.float32)
    assert np.array_equal(host(g).view(np.int32), want.view(np.int32)) and not np.array_equal(want, other)
    assert np.array_equal(host(acc), np.add(g1.numpy(), g2.numpy(), dtype=np.float32))


def test_kernel_refusals():
    from vltf_amd import ops
    from vltf_amd._ffi import VltfError
    acc, g = torch.zeros(100, device=DEV), torch.ones(100, device=DEV)
    for mode in (-1, 3, 7):
        with pytest.raises(VltfError, match="mode"):
            ops.grad_accumulate(acc, g, mode)
    for table in ([(10, 20, 1.0), (5, 8, 1.0)], [(0, 10, 1.0), (9, 20, 1.0)], [(0, 101, 1.0)], [(5, 5, 1.0)], [],
                  [(i, i + 1, 1.0) for i in range(17)]):
        with pytest.raises(VltfError):
            ops.grad_accumulate(acc, g, ADD, table)
    with pytest.raises(VltfError):
        ops.grad_accumulate(acc[:0], g[:0], ADD)                                         # an empty tensor
    with pytest.raises(VltfError):
        ops.grad_accumulate(acc[:50], g, ADD)
    torch.cuda.synchronize()
    assert not bool(acc.any()) and bool((g == 1).all())


def test_step_state_set_micro():
    from vltf_amd import ops
    a, b = ops.step_state(DEV), ops.step_state(DEV)
    for u in (0, 7):
        ops.step_state_set(a, u, 0.0123, 5)
        ops.step_state_set_micro(b, u, u, 0.0123, 5)
        assert torch.equal(a, b) and bool(a.any())
    update, draw, lr = 3, 3 * 4 + 2, 0.0123
    ops.step_state_set_micro(b, update, draw, lr, 5)
    gen = torch.Generator(device="cpu").manual_seed(1)
    w, g, m = (torch.randn(5001, generator=gen).to(DEV) for _ in range(3))
    v = torch.rand(5001, generator=gen).to(DEV)
    w2, m2, v2 = w.clone(), m.clone(), v.clone()
    ops.adam_apply_st(w, g, m, v, b)                                                 # Adam's step size: the UPDATE count
    ops.adam_apply(w2, g, m2, v2, lr, update + 1)
    assert torch.equal(bits(w), bits(w2)) and torch.equal(bits(m), bits(m2)) and torch.equal(bits(v), bits(v2))
    x = torch.randn(4099, generator=gen).to(DEV)
    y, y2 = torch.empty_like(x), torch.empty_like(x)
    k, k2 = torch.empty(4099, dtype=torch.uint8, device=DEV), torch.empty(4099, dtype=torch.uint8, device=DEV)
    ops.dropout_fwd_st(x, y, k, 0.5, b)                                              # the dropout seed: the DRAW index
    ops.dropout_fwd(x, y2, k2, 0.5, (draw << 20) ^ 0x5DEECE66D)
    assert torch.equal(k, k2) and torch.equal(bits(y), bits(y2))
    ops.dropout_fwd(x, y2, k2, 0.5, (update << 20) ^ 0x5DEECE66D)
    assert not torch.equal(k, k2)


# ---- B. LRCNEngine ------------------------------------------------------------------------------------------------------------------
SHAPE, NCLS, FPC, B, HID = (67, 67, 3), 7, 3, 2, 8
LR, CLIP = 0.01, 0.5
_DATA = {}


def small_cfg(**kw):
    from vltf_amd.engine import NetConfig
    return NetConfig(image_shape=SHAPE, num_classes=NCLS, fpc=FPC, frame_encoding_layer="fc6", lstm_hidden=HID, **kw)


def data():
    """Parameters and 6 clips with labels, made once and never written: micro-batches are consecutive pairs of clips."""
    if not _DATA:
        rng = np.random.default_rng(5)
        _DATA["p"] = O.init_params(rng, NCLS, "fc6", HID, 1, SHAPE, well_scaled=True)
        _DATA["frames"] = rng.integers(0, 256, (6 * FPC,) + SHAPE, dtype=np.uint8)
        _DATA["onehot"] = O.labels_to_one_hot([[l] for l in rng.integers(0, NCLS, 6)], NCLS)
        _DATA["oracle"] = {}
    return _DATA["p"], _DATA["frames"], _DATA["onehot"]


def oracle_step(clips):
    """O.lrcn_train_step on the first `clips` clips (plain SGD, lr 0.01, clip_norm 0.5), computed once per clip count."""
    p, frames, onehot = data()
    if clips not in _DATA["oracle"]:
        x = frames[:clips * FPC].astype(np.float32) - MEAN
        _DATA["oracle"][clips] = O.lrcn_train_step(p, x, onehot[:clips], FPC, lr=LR, clip_norm=CLIP)
    return _DATA["oracle"][clips]


def dev_batch(c0, c1):
    _, frames, onehot = data()
    return torch.tensor(frames[c0 * FPC:c1 * FPC], device=DEV), torch.tensor(onehot[c0:c1], device=DEV)


def engine(max_clips=B, load=True, **kw):
    from vltf_amd.engine import LRCNEngine
    eng = LRCNEngine(small_cfg(**kw), max_clips=max_clips, device=DEV)
    if load:
        eng.load_params(data()[0])
    return eng


def update(eng, cuts, lr=LR, clip=CLIP, global_rows=None):
    """One accumulated update over the clip ranges `cuts`; returns every call's result."""
    k = len(cuts)
    return [eng.train_step_u8(*dev_batch(c0, c1), lr=lr, clip_norm=clip, mean_bgr=MEAN, global_rows=global_rows, micro=(i, k))
            for i, (c0, c1) in enumerate(cuts)]


@pytest.mark.parametrize("k", [2, 3])
def test_update_matches_oracle_on_the_concatenated_batch(k):
    newp, loss, gn, _, _, grads = oracle_step(2 * k)
    eng = engine(accumulate=3)
    before = eng.step_count
    outs = update(eng, [(2 * i, 2 * i + 2) for i in range(k)])
    for i, o in enumerate(outs[:-1]):
        assert "grad_norm" not in o and o["rows"] == 2 * (i + 1)
    out = outs[-1]
    assert eng.step_count == before + 1 and out["rows"] == 2 * k and not eng.micro.open()
    assert abs(out["loss"] - loss) < 1e-4 * max(1, abs(loss)) and abs(out["grad_norm"] - gn) < 1e-3 * gn
    close_grads(eng.get_grads(), grads)
    close_params(eng.get_params(), newp)


def test_unequal_micro_batches():
    """2 clips then 1 clip: global_rows = 3 on both calls gives the exact mean over the 3 clips."""
    newp, loss, gn, _, _, grads = oracle_step(3)
    eng = engine(accumulate=2)
    outs = update(eng, [(0, 2), (2, 3)], global_rows=3)
    assert outs[-1]["rows"] == 3 and abs(outs[-1]["loss"] - loss) < 1e-4 * max(1, abs(loss)) and abs(outs[-1]["grad_norm"] - gn) < 1e-3 * gn
    close_grads(eng.get_grads(), grads)
    close_params(eng.get_params(), newp)


@pytest.mark.parametrize("kw", [dict(momentum=0.9), dict(momentum=0.9, nesterov=True), dict(optimizer="adam")],
                         ids=["momentum", "nesterov", "adam"])
def test_other_optimizers_with_weight_decay(kw):
    """Two updates of 2 x 2 clips against two plain 4-clip steps of an engine of the same configuration.  lr: 0.01 for SGD's rules.
    Adam moves a weight by ~lr g / (|g| + eps') whatever the gradient's size, so where |g| is within ~30x of eps' = 3e-7 the fp32
    summation order of the two runs (1e-8 absolute in g) is worth several % of lr (tests/test_engine_gpu.py::test_adam_steps_match_
    oracle measured 3.4 %): lr = 1e-4 keeps that under the 1e-5 of the tolerance while every weight still moves by ~1e-4 per step."""
    lr = 1e-4 if kw.get("optimizer") == "adam" else LR
    acc, plain = engine(accumulate=2, weight_decay=0.05, **kw), engine(max_clips=4, weight_decay=0.05, **kw)
    p0 = plain.get_params()
    for cuts in ([(0, 2), (2, 4)], [(2, 4), (4, 6)]):
        out = update(acc, cuts, lr=lr)[-1]
        f, o = dev_batch(cuts[0][0], cuts[0][1])
        f2, o2 = dev_batch(cuts[1][0], cuts[1][1])
        want = plain.train_step_u8(torch.cat([f, f2]), torch.cat([o, o2]), lr=lr, clip_norm=CLIP, mean_bgr=MEAN)
        assert abs(out["loss"] - want["loss"]) < 1e-4 * max(1, abs(want["loss"]))
    got, ref = acc.get_params(), plain.get_params()
    close_params(got, ref)
    assert any(np.abs(ref[k] - p0[k]).max() > 1e-4 for k in ref)                         # (the comparison is of weights that moved)
    assert acc.step_count == plain.step_count == 2


def test_weight_decay_enters_once():
    """Plain SGD, decay > 0: reg_loss and the regularised norm are the plain 4-clip step's -- not k times the decay."""
    acc, plain = engine(accumulate=2, weight_decay=0.05), engine(max_clips=4, weight_decay=0.05)
    out = update(acc, [(0, 2), (2, 4)])[-1]
    f, o = dev_batch(0, 4)
    want = plain.train_step_u8(f, o, lr=LR, clip_norm=CLIP, mean_bgr=MEAN)
    assert want["reg_loss"] > 0
    np.testing.assert_allclose(out["reg_loss"], want["reg_loss"], rtol=1e-5)
    np.testing.assert_allclose(out["grad_norm"], want["grad_norm"], rtol=1e-5)
    close_params(acc.get_params(), plain.get_params())


def test_fine_tuning_leaves_frozen_ranges_alone():
    kw = dict(train_from="fc6", lr_mult=10.0)
    acc, plain = engine(accumulate=2, **kw), engine(max_clips=4, **kw)
    inside = torch.zeros(acc.plan.total, dtype=torch.bool, device=DEV)
    for lo, hi, _ in acc.plan.tiers:
        inside[lo:hi] = True
    assert not acc.plan.full_range() and bool((~inside).any())
    acc.g[~inside] = float("nan")
    acc.gacc[~inside] = float("nan")
    w0 = acc.w.clone()
    update(acc, [(0, 2), (2, 4)])
    f, o = dev_batch(0, 4)
    plain.train_step_u8(f, o, lr=LR, clip_norm=CLIP, mean_bgr=MEAN)
    assert bool(torch.isfinite(acc.w).all())
    assert torch.equal(bits(acc.w)[~inside], bits(w0)[~inside]) and not torch.equal(acc.w[inside], w0[inside])
    assert bool(torch.isnan(acc.g[~inside]).all()) and bool(torch.isnan(acc.gacc[~inside]).all())
    frozen = set(acc.plan.frozen)
    got, ref = acc.get_params(), plain.get_params()
    close_params(got, ref, [k for k in ref if k not in frozen])


def test_sequence_errors():
    from vltf_amd._ffi import VltfError
    eng = engine(accumulate=2)
    one = dev_batch(0, 2)

    def call(micro):
        return eng.train_step_u8(*one, lr=LR, clip_norm=CLIP, mean_bgr=MEAN, micro=micro)

    def group_works():
        before = eng.step_count
        call((0, 2))
        call((1, 2))
        assert eng.step_count == before + 1

    for first, bad in ((None, (1, 2)), ((0, 2), (0, 2)), ((0, 2), (1, 3)), (None, (0, 3))):
        if first is not None:
            call(first)
        before = eng.step_count
        with pytest.raises(VltfError):
            call(bad)
        assert eng.step_count == before
        group_works()
    call((0, 2))
    eng.forward_u8(one[0], MEAN)                                                     # a forward between micro-steps is allowed
    with pytest.raises(VltfError, match="update boundaries"):
        eng.get_opt_state()
    group_works()
    assert "__optimizer__/step_count" in eng.get_opt_state()
    with pytest.raises(VltfError):                                                   # a plain engine takes no group at all
        engine(load=False).train_step_u8(*one, lr=LR, micro=(0, 2))


@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_accumulate_one_is_bit_for_bit_the_plain_engine(opt):
    """accumulate=1 / micro=None, and the one-step group micro=(0, 1), against an engine built without the argument: dropout 0.5."""
    kw = dict(optimizer=opt, dropout_keep_prob=0.5)
    plain, one, single = engine(**kw), engine(accumulate=1, **kw), engine(accumulate=1, **kw)
    assert one.gacc is None
    for step in range(3):
        bt = dev_batch(2 * step, 2 * step + 2)
        outs = [e.train_step_u8(*bt, lr=LR, clip_norm=CLIP, mean_bgr=MEAN, **m) for e, m in
                ((plain, {}), (one, dict(micro=None)), (single, dict(micro=(0, 1))))]
        assert outs[0] == outs[1] == outs[2]
    assert torch.equal(bits(plain.w), bits(one.w)) and torch.equal(bits(plain.w), bits(single.w))
    assert torch.equal(plain.drop_mask, one.drop_mask) and plain.step_count == single.step_count == 3


@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_captured_update_equals_eager(opt):
    """step_graph, k = 2, dropout 0.5: four updates (warm-up, capture, two replays of each micro role) leave, bit for bit, the weights,
    g and optimizer slots of an eager engine fed the same sequence; the two micro-steps of one update draw different masks."""
    from tests.test_step_graph_gpu import batch, pair, same_state
    eager, graph = pair(2, opt=opt, fpc=FPC, hid=HID, accumulate=2)
    rng = np.random.default_rng(13)
    for upd in range(4):
        masks = []
        for i in range(2):
            bt = batch(rng, 2, FPC)
            outs = [e.train_step_u8(bt["frames_u8"], bt["onehot"], 0.01 * 0.7 ** upd, 5.0, MEAN, bt["crop_y"], bt["crop_x"], bt["mirror"],
                                    micro=(i, 2)) for e in (eager, graph)]
            assert outs[0] == outs[1], (upd, i, outs)
            assert torch.equal(eager.drop_mask, graph.drop_mask)
            masks.append(graph.drop_mask.clone())
        assert not torch.equal(masks[0], masks[1])
        assert torch.equal(bits(eager.g), bits(graph.g)) and torch.equal(bits(eager.gacc), bits(graph.gacc))
        same_state(eager, graph)
    assert len(graph._graphs) == 2 and eager.step_count == 4                             # one graph per micro role: first, last


def test_bf16_path_sums_its_micro_steps():
    """conv_math bf16 needs nothing of its own (g is fp32 there too): the update's g is gacc + g of its two micro-steps, read from a
    second engine that runs them as plain steps with lr 0 (its weights stay) and the same loss scale."""
    acc, probe = engine(accumulate=2, conv_math="bf16"), engine(conv_math="bf16")
    parts = []
    for c0, c1 in ((0, 2), (2, 4)):
        probe.train_step_u8(*dev_batch(c0, c1), lr=0.0, clip_norm=CLIP, mean_bgr=MEAN, global_rows=4)
        parts.append(host(probe.g).copy())
    assert torch.equal(bits(probe.w), bits(acc.w))
    out = update(acc, [(0, 2), (2, 4)])[-1]
    assert np.isfinite(out["loss"]) and out["grad_norm"] > 0
    want = np.add(parts[0], parts[1], dtype=np.float32)
    assert np.array_equal(host(acc.g).view(np.int32), want.view(np.int32))
    assert np.array_equal(host(acc.gacc).view(np.int32), parts[0].view(np.int32))


# ---- one-rank RCCL ------------------------------------------------------------------------------------------------------------------
def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def dp_worker(port, q):
    os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from vltf_amd import dp
    from vltf_amd.engine import LRCNEngine
    dp.init_from_env(backend="nccl", force=True)
    p = data()[0]
    gar = dp.GradAllReduce(always=True)
    calls = []
    reduce_async = gar.reduce_async

    def counting(flat, offset, count):
        calls.append((offset, count))
        return reduce_async(flat, offset, count)

    gar.reduce_async = counting
    cfg = small_cfg(accumulate=2)
    eng, ref = LRCNEngine(cfg, max_clips=B, device=DEV, dp=gar), LRCNEngine(cfg, max_clips=B, device=DEV)
    eng.load_params(p)
    ref.load_params(p)
    res = dict(chunks=len(eng.grad_chunks))
    eng.train_step_u8(*dev_batch(0, 2), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, micro=(0, 2))
    res["calls_first"] = len(calls)
    a = eng.train_step_u8(*dev_batch(2, 4), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, micro=(1, 2))
    res["calls_update"] = list(calls)
    b = update(ref, [(0, 2), (2, 4)])[-1]
    got, want = eng.get_params(), ref.get_params()
    res["same"] = all(np.array_equal(got[k], want[k]) for k in want) and a == b
    res["moved"] = all(not np.array_equal(want[k], p[k]) for k in want)
    # an empty shard as the final micro-step: the update is the first micro-step's gradient alone
    del calls[:]
    eng.load_params(p)
    eng.train_step_u8(*dev_batch(0, 2), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, global_rows=4, micro=(0, 2))
    e = eng.train_step_empty(LR, CLIP, micro=(1, 2))
    alone = LRCNEngine(small_cfg(), max_clips=B, device=DEV)
    alone.load_params(p)
    f = alone.train_step_u8(*dev_batch(0, 2), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, global_rows=4)
    got, want = eng.get_params(), alone.get_params()
    res["empty_same"] = all(np.array_equal(got[k], want[k]) for k in want) and e["grad_norm"] == f["grad_norm"] and e["rows"] == 2
    res["empty_calls"] = len(calls)
    torch.cuda.synchronize()
    q.put(res)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_one_rank_rccl_accumulated_update():
    """k = 2 under a one-rank process group equals the accumulated update without data parallelism bit for bit; the exchange runs once
    per update (len(grad_chunks) reduce_async calls, none during the non-final micro-step), each chunk's sum added right before it."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    pr = ctx.Process(target=dp_worker, args=(free_port(), q))
    pr.start()
    pr.join(300)
    assert pr.exitcode == 0, "rank exited with %s" % pr.exitcode
    r = q.get(timeout=10)
    assert r["calls_first"] == 0 and len(r["calls_update"]) == r["chunks"] >= 3, r
    assert r["same"] and r["moved"], r
    assert r["empty_same"] and r["empty_calls"] == r["chunks"], r


# ---- C. GraphEngine -----------------------------------------------------------------------------------------------------------------
def test_graph_engine_update_and_sequence_errors():
    """encdec_state (two pipelines, one tower of 2-frame clips, an LSTM head: the smallest of tests/graph_cases.py): k = 2 x its 2
    items against the plain step on the 4 items."""
    from tests import graph_cases as GC
    from tests.test_graph_gpu import device_feeds
    from vltf_amd._ffi import VltfError
    from vltf_amd.graph import GraphEngine
    case = GC.CASES["encdec_state"]()
    pipes, ds = GC.specs_and_datasets(case)
    pipes4, ds4 = GC.specs_and_datasets(case, items=4)
    acc = GraphEngine(pipes, ds, case["V"], device=DEV, accumulate=2)
    plain = GraphEngine(pipes4, ds4, case["V"], device=DEV)
    assert plain.gacc is None and acc.gacc.numel() == acc.w.numel()
    p = acc.init_params(seed=case["seed"], well_scaled=True)
    acc.load_params(p)
    plain.load_params(p)
    raw, _ = GC.inputs(case, items=4)
    halves = [device_feeds({t: v[:len(v) // 2] for t, v in raw.items()}), device_feeds({t: v[len(v) // 2:] for t, v in raw.items()})]
    rows = plain.forward(device_feeds(raw)).shape[0]
    onehot = torch.tensor(O.labels_to_one_hot([[l] for l in np.random.default_rng(0).integers(0, case["V"], rows)], case["V"]), device=DEV)
    want = plain.train_step(device_feeds(raw), onehot, lr=LR, clip_norm=CLIP)
    first = acc.train_step(halves[0], onehot[:rows // 2], lr=LR, clip_norm=CLIP, micro=(0, 2))
    out = acc.train_step(halves[1], onehot[rows // 2:], lr=LR, clip_norm=CLIP, micro=(1, 2))
    assert "grad_norm" not in first and first["rows"] == rows // 2 and out["rows"] == rows and acc.step_count == 1
    assert abs(out["loss"] - want["loss"]) < 1e-4 * max(1, abs(want["loss"])) and abs(out["grad_norm"] - want["grad_norm"]) < 1e-3 * want["grad_norm"]
    close_grads(acc.get_grads(), plain.get_grads())
    close_params(acc.get_params(), plain.get_params())
    assert any(not np.array_equal(v, p[k]) for k, v in acc.get_params().items())

    def call(micro):
        return acc.train_step(halves[0], onehot[:rows // 2], lr=LR, clip_norm=CLIP, micro=micro)

    for first, bad in ((None, (1, 2)), ((0, 2), (0, 2)), ((0, 2), (1, 3)), (None, (0, 3))):
        if first is not None:
            call(first)
        with pytest.raises(VltfError):
            call(bad)
        before = acc.step_count
        call((0, 2))
        call((1, 2))
        assert acc.step_count == before + 1
    call((0, 2))
    with pytest.raises(VltfError, match="update boundaries"):
        acc.get_opt_state()
    call((0, 2))
    call((1, 2))


# ---- D. run_task ---------------------------------------------------------------------------------------------------------------------
def test_run_task_accumulate(tmp_path, monkeypatch):
    """5 videos, batch_size 2, accumulate 2, 2 epochs: 3 batches per epoch = a group of two and a short group of one (a single video).
    The engine counts 4 updates, everything else counts 6 batches; the learning-rate schedule is the plain run's; a run resumed from the
    end-of-epoch-1 checkpoint (a group boundary) ends with exactly the weights of the uninterrupted one (deterministic imgproc, as
    tests/test_run_task_gpu.py::test_adam_resume_equals_uninterrupted)."""
    monkeypatch.setenv("VLTF_PREFETCH", "0")
    monkeypatch.setenv("VLTF_CONV_MATH", "f32")
    from tests.test_host_workflow import make_dataset
    from tests.test_run_task_gpu import RAW, write_cfg
    from vltf_amd import run_task
    folder = str(tmp_path)
    train_path, _, _ = make_dataset(folder, "train.txt", shape=RAW, seed=1)

    def cfg(name, run, accumulate, **kw):
        path = write_cfg(folder, name, train_path, "train", epochs=2, det=True, run=run, **kw)
        with open(path) as f:
            c = yaml.safe_load(f)
        c["run"]["train"].update(accumulate=accumulate, base_lr=0.01, momentum=0.9)
        with open(path, "w") as f:
            yaml.safe_dump(c, f)
        return path

    def final_weights(run):
        ck = sorted(glob.glob(os.path.join(folder, run, "checkpoints", "*.weights.npz")), key=os.path.getmtime)
        with np.load(ck[-1], allow_pickle=False) as z:
            return ck, {k: z[k] for k in z.files}

    run_task.main(cfg("a.yml", "runA", 2), seed=3)
    ck, full = final_weights("runA")
    assert len(ck) == 2 and int(full["__optimizer__/step_count"][0]) == 4                 # 2 groups per epoch
    assert ck[-1].split(".graph-")[0].endswith("_gs_6") and "_gs_3" in os.path.basename(ck[0])
    log = open(glob.glob(os.path.join(folder, "runA", "log_e2e_train_scratch_*.log"))[0]).read()
    assert "global step: 6" in log and log.count("Update ") == 4 and "Gradient accumulation: 2 batches of 2 videos" in log
    run_task.main(cfg("p.yml", "runP", 1), seed=3)
    _, plain = final_weights("runP")
    assert int(plain["__optimizer__/step_count"][0]) == 6
    sched = [open(os.path.join(folder, r, "e2e_train_scratch_lr_decay_schedule.txt"), "rb").read() for r in ("runA", "runP")]
    assert sched[0] == sched[1] and len(sched[0].splitlines()) == 6
    assert not np.array_equal(plain["output_fc_w"], full["output_fc_w"])
    first = ck[0][:-len(".weights.npz")]
    run_task.main(cfg("b.yml", "runA", 2, resume=first), seed=77)
    _, resumed = final_weights("runA")
    assert int(resumed["__optimizer__/step_count"][0]) == 4
    for k in full:
        np.testing.assert_array_equal(resumed[k], full[k], err_msg=k)
