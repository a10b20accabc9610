"""Per-variable gradient and weight statistics on the device (vl_tensor_stats; NetConfig.tensor_stats_interval,
GraphEngine(tensor_stats_interval=), logging.tensor_stats_interval): the segmented two-stage launch against the numpy restatement
tests/tensor_stats_ref.py, then through LRCNEngine (eager, captured, accumulated, frozen layers, the packed-bf16 path, one-rank
RCCL), GraphEngine and run_task.
Bounds.  Sums: the contract of include/vltf.h, |got - exact| <= N 2^-53 sum|term| per segment of N elements, the exact sum from
math.fsum.  Min / max by value, counts exactly.  Derived keys: tensor_stats_ref.close_reports, worked out from the same contract.
The launch's sum of g_sumsq over the variables against grad_norm^2 (an fp32 sum): 1e-5 relative.
Small shapes: the kernel on segments of 1, 3, 5, CHUNK - 1, CHUNK, CHUNK + 1 and 2 CHUNK + 5 elements (a single short chunk, a whole
one, a whole one and a one-element one, two and a short one) at offsets of every residue mod 4; the engines on 67x67x3 frames, 2
clips x 3 frames, hidden 8, 7 classes.  The launch's grid is the table's chunk count, uncapped, so there is no second pass to cover."""
import glob
import json
import math
import os
import re
import socket

import numpy as np
import pytest
import torch
import yaml

from oracle import lrcn_oracle as O
from tests import tensor_stats_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN = np.array([99.197148, 105.293620, 109.503945], np.float32)
NAN, INF = float("nan"), float("inf")
FLT_MAX = float(np.finfo(np.float32).max)


def chunk():
    from vltf_amd import ops
    return ops.STAT_CHUNK


# ---- the launch --------------------------------------------------------------------------------------------------------------------
_K = {}


def table():
    """Segments [(begin, end)]: the first begins at the odd offset 1, a one-element gap follows it, later gaps of 0 .. 3 elements put
    the begins on every residue mod 4; six elements follow the last segment."""
    C = chunk()
    lengths = [1, 3, 5, C - 1, C, C + 1, 2 * C + 5, 7, 4]
    gaps = [1, 1, 0, 2, 0, 3, 1, 0, 2]
    segs, off = [], 0
    for n, gap in zip(lengths, gaps):
        off += gap
        segs.append((off, off + n))
        off += n
    return segs, off + 6


def kernel_data():
    """Host w, g: normal values inside the segments, NaN in every gap and behind the last segment in both arrays; the special values
    of the module docstring planted by hand.  Made once, with the restatement's rows."""
    if not _K:
        C = chunk()
        segs, count = table()
        rng = np.random.default_rng(7)
        w = (rng.standard_normal(count) * 0.05).astype(np.float32)
        g = (rng.standard_normal(count) * 3.0).astype(np.float32)
        inside = np.zeros(count, bool)
        for lo, hi in segs:
            inside[lo:hi] = True
        w[~inside] = NAN
        g[~inside] = NAN
        lo = segs[2][0]                                   # 5 elements: nothing but denormals and zeros (a flush to zero would show)
        g[lo:lo + 5] = np.array([1e-45, -0.0, 0.0, 3e-40, -1e-42], np.float32)
        w[lo:lo + 5] = np.array([-0.0, 2e-45, -7e-41, 0.0, 1e-39], np.float32)
        lo = segs[5][0]                                   # CHUNK + 1 elements: non-finite values, one of them alone in the short chunk
        g[lo + 10], g[lo + 11], g[lo + C] = NAN, INF, -INF
        w[lo], w[lo + 77] = NAN, -INF
        lo = segs[6][0]                                   # 2 CHUNK + 5: -0, a denormal, FLT_MAX (its square is finite in fp64)
        g[lo + 5], g[lo + 6], g[lo + C + 3] = -0.0, 1e-41, FLT_MAX
        w[lo + 9], w[lo + 2 * C + 4] = -0.0, -FLT_MAX
        lo = segs[7][0]                                   # 7 elements, none finite
        g[lo:lo + 7] = np.array([NAN, INF, -INF, NAN, NAN, INF, -INF], np.float32)
        w[lo:lo + 7] = np.array([INF, INF, NAN, -INF, NAN, NAN, NAN], np.float32)
        _K.update(segs=segs, count=count, w=w, g=g, want=R.segment_rows(w, g, segs))
    return _K


def launch(w, g, segs):
    """One ops.tensor_stats call on garbage-filled out / ws -> (rows, the bytes of out)."""
    from vltf_amd import ops
    out = torch.full((len(segs) * ops.STAT_ROW_BYTES,), 0xAB, dtype=torch.uint8, device=DEV)
    ws = torch.full((ops.tensor_stats_ws_bytes(segs),), 0xCD, dtype=torch.uint8, device=DEV)
    ops.tensor_stats(w, g, segs, out, ws)
    torch.cuda.synchronize()
    return ops.stat_rows(out, len(segs)), out.cpu().numpy().tobytes()


def shifted(a, shift, pad=4):
    """The array on the device as a view `shift` floats behind a 16-byte boundary."""
    buf = torch.full((a.size + pad,), NAN, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[shift:shift + a.size]
    v.copy_(torch.from_numpy(a))
    return v


def first_result():
    if "rows" not in _K:
        k = kernel_data()
        _K["rows"], _K["bytes"] = launch(shifted(k["w"], 0), shifted(k["g"], 0), k["segs"])
    return _K["rows"], _K["bytes"]


def test_launch_against_the_restatement():
    k = kernel_data()
    rows, _ = first_result()
    for i, ((lo, hi), (ww, wg)) in enumerate(zip(k["segs"], k["want"])):
        R.check_row(rows[i], ww, wg, "segment %d [%d, %d)" % (i, lo, hi))
    # the planted values were seen for what they are
    assert int(rows[2]["g_zero"]) == 2 and float(rows[2]["g_sum"]) != 0.0 and float(rows[2]["w_min"]) < 0.0      # denormals kept
    assert (int(rows[5]["g_nonfinite"]), int(rows[5]["w_nonfinite"])) == (3, 2) and math.isfinite(float(rows[5]["g_sumsq"]))
    assert float(rows[6]["g_max"]) == FLT_MAX and float(rows[6]["w_min"]) == -FLT_MAX and float(rows[6]["g_sumsq"]) > 1e76
    assert (int(rows[7]["g_nonfinite"]), int(rows[7]["w_nonfinite"])) == (7, 7)
    assert (float(rows[7]["g_sum"]), float(rows[7]["g_sumsq"]), float(rows[7]["g_min"]), float(rows[7]["g_max"])) == (0.0, 0.0, INF, -INF)
    assert (float(rows[7]["w_min"]), float(rows[7]["w_max"])) == (INF, -INF)
    assert float(rows[0]["g_sum"]) == float(k["g"][1]) and float(rows[0]["w_sumsq"]) == float(k["w"][1]) ** 2    # one element: exact


@pytest.mark.parametrize("sw,sg", [(1, 1), (2, 2), (3, 3), (1, 0), (2, 3)], ids=["both+1", "both+2", "both+3", "w+1", "w+2,g+3"])
def test_alignment_changes_no_bit(sw, sg):
    """w and g moved off the 16-byte boundary together (the 16-byte loads begin elsewhere in every chunk) and against each other (the
    4-byte loads): the same bytes as the aligned call."""
    k = kernel_data()
    _, want = first_result()
    _, got = launch(shifted(k["w"], sw), shifted(k["g"], sg), k["segs"])
    assert got == want


def test_repeatable_and_fully_overwritten():
    k = kernel_data()
    rows, want = first_result()
    _, again = launch(shifted(k["w"], 0), shifted(k["g"], 0), k["segs"])          # other buffers, other garbage underneath
    assert again == want
    assert (rows["reserved"] == 0).all() and b"\xab" * 8 not in want


def test_sixty_five_segments_take_two_launches():
    from vltf_amd import ops
    C = chunk()
    segs, off = [], 2
    for i in range(65):
        n = C + 3 if i == 40 else i % 7 + 1
        segs.append(("v%d" % i, off, off + n))
        off += n + i % 3
    rng = np.random.default_rng(8)
    w, g = rng.standard_normal(off).astype(np.float32), rng.standard_normal(off).astype(np.float32)
    g[segs[64][1]] = NAN                                  # seen by the second launch
    assert ops.tensor_stats_ws_bytes(segs) == 64 * (63 + 2)
    rows, _ = launch(torch.from_numpy(w).to(DEV), torch.from_numpy(g).to(DEV), segs)
    for i, (ww, wg) in enumerate(R.segment_rows(w, g, segs)):
        R.check_row(rows[i], ww, wg, "segment %d" % i)
    assert int(rows[64]["g_nonfinite"]) == 1 and int(rows[63]["g_nonfinite"]) == 0


def test_a_segment_past_two_to_the_31():
    """Element indices are 64-bit: one segment of CHUNK + 1 elements beginning past 2^31 in buffers that large (nothing else in them
    is read, so nothing else is written here either)."""
    C = chunk()
    lo = 2 ** 31 + 3
    count = lo + C + 1 + 2
    rng = np.random.default_rng(9)
    w, g = rng.standard_normal(C + 1).astype(np.float32), rng.standard_normal(C + 1).astype(np.float32)
    wt, gt = torch.empty(count, device=DEV), torch.empty(count, device=DEV)
    wt[lo:lo + C + 1].copy_(torch.from_numpy(w))
    gt[lo:lo + C + 1].copy_(torch.from_numpy(g))
    wt[lo - 1], wt[lo + C + 1], gt[lo - 1], gt[lo + C + 1] = NAN, NAN, NAN, NAN
    rows, _ = launch(wt, gt, [(lo, lo + C + 1)])
    R.check_row(rows[0], R.one_side(w), R.one_side(g), "past 2^31")


def test_refusals():
    from vltf_amd import _ffi, ops
    from vltf_amd._ffi import VltfError
    w, g = torch.zeros(100, device=DEV), torch.zeros(100, device=DEV)
    out, ws = torch.zeros(64 * 70, dtype=torch.uint8, device=DEV), torch.zeros(64 * 70, dtype=torch.uint8, device=DEV)
    for bad, what in (([(10, 20), (0, 5)], "segment 1"), ([(0, 10), (9, 20)], "segment 1"), ([(0, 10), (10, 10)], "segment 1"),
                      ([(0, 10), (50, 101)], "segment 1"), ([(-1, 5)], "segment 0")):
        with pytest.raises(VltfError, match=what):
            ops.tensor_stats(w, g, bad, out, ws)
    with pytest.raises(VltfError, match="empty"):
        ops.tensor_stats(w, g, [], out, ws)
    with pytest.raises(VltfError, match="out needs"):
        ops.tensor_stats(w, g, [(0, 10), (20, 30)], out[:64], ws)
    with pytest.raises(VltfError, match="one element count"):
        ops.tensor_stats(w, g[:50], [(0, 10)], out, ws)
    with pytest.raises(VltfError, match="uint8"):
        ops.tensor_stats(w, g, [(0, 10)], torch.zeros(16, device=DEV), ws)
    # the C entry point itself: 0 and 65 segments, null pointers, a short workspace
    lib = _ffi.lib()
    seg = (_ffi.StatSegment * 65)()
    for i in range(65):
        seg[i].begin, seg[i].end = i, i + 1
    s = torch.cuda.current_stream().cuda_stream

    def call(wp, gp, n, outp, wsp, ws_bytes):
        rc = lib.vl_tensor_stats(wp, gp, 100, seg, n, outp, wsp, ws_bytes, s)
        return rc, lib.vl_last_error().decode()
    ptrs = (w.data_ptr(), g.data_ptr(), out.data_ptr(), ws.data_ptr())
    for n in (0, 65):
        rc, msg = call(ptrs[0], ptrs[1], n, ptrs[2], ptrs[3], ws.numel())
        assert rc != 0 and "1 .. 64 segments, got %d" % n in msg
    for k in range(4):
        p = list(ptrs)
        p[k] = None
        rc, msg = call(p[0], p[1], 2, p[2], p[3], ws.numel())
        assert rc != 0 and "bad argument" in msg
    rc, msg = call(ptrs[0], ptrs[1], 3, ptrs[2], ptrs[3], 2 * 64)
    assert rc != 0 and "workspace has 128 bytes, this table needs 192" in msg
    assert call(ptrs[0], ptrs[1], 3, ptrs[2], ptrs[3], 3 * 64)[0] == 0
    assert lib.vl_tensor_stats_ws_bytes(seg, 0) == 0 and lib.vl_tensor_stats_ws_bytes(seg, 65) == 0 and lib.vl_tensor_stats_ws_bytes(None, 1) == 0
    torch.cuda.synchronize()


# ---- LRCNEngine ----------------------------------------------------------------------------------------------------------------------
SHAPE, NCLS, FPC, B, HID = (67, 67, 3), 7, 3, 2, 8
LR, CLIP = 0.01, 0.5
KEYS = {"tensor_stats", "grads_norm_mean"}


def small_cfg(**kw):
    from vltf_amd.engine import NetConfig
    return NetConfig(image_shape=SHAPE, num_classes=NCLS, fpc=FPC, frame_encoding_layer="fc6", lstm_hidden=HID, **kw)


def small_batches(steps, seed=5, clips=B):
    rng = np.random.default_rng(seed)
    p = O.init_params(rng, NCLS, "fc6", HID, 1, SHAPE, well_scaled=True)
    out = []
    for _ in range(steps):
        frames = torch.tensor(rng.integers(0, 256, (clips * FPC,) + SHAPE, dtype=np.uint8), device=DEV)
        onehot = torch.tensor(O.labels_to_one_hot([[l] for l in rng.integers(0, NCLS, clips)], NCLS), device=DEV)
        out.append((frames, onehot))
    return p, out


def check_stats_step(eng, out, before, grads, lr, clip, msg=""):
    """A stats step's result against the restatement on the parameters fetched before the step and the gradient fetched after it."""
    assert KEYS <= set(out), (msg, sorted(out))
    names = [n for n, _, _ in eng.stat_segs]
    assert list(out["tensor_stats"]) == names and sorted(names) == sorted(grads)
    mults = [next(m for lo, hi, m in eng.plan.tiers if lo <= a and b <= hi) for _, a, b in eng.stat_segs]
    ss = float(eng.stat_ss.item())
    assert ss == float(eng.ss.item()) and math.sqrt(ss) == out["grad_norm"]
    want, mean = R.derived(names, [(R.one_side(before[n]), R.one_side(grads[n])) for n in names], mults, lr, clip, ss)
    counts = {n: b - a for n, a, b in eng.stat_segs}
    R.close_reports(out["tensor_stats"], want, counts, msg)
    assert abs(out["grads_norm_mean"] - mean) <= 4 * max(counts.values()) * 2.0 ** -53 * mean, (msg, out["grads_norm_mean"], mean)
    total = sum(d["grad_norm"] ** 2 for d in out["tensor_stats"].values())
    assert abs(total - out["grad_norm"] ** 2) <= 1e-5 * total, (msg, total, out["grad_norm"] ** 2)
    assert all(d["grad_nonfinite"] == 0 and d["weight_nonfinite"] == 0 for d in out["tensor_stats"].values())
    assert eng.tensor_stats() is out["tensor_stats"]


OPTS = {"sgd+clip": dict(), "momentum+decay": dict(momentum=0.9, weight_decay=0.05), "adam": dict(optimizer="adam"),
        "bf16": dict(conv_math="bf16")}


@pytest.mark.parametrize("opt", list(OPTS))
def test_engine_stats_equal_the_restatement_and_change_no_weight(opt):
    """Interval 1, three steps: every step's statistics are those of the weights the forward pass used and of the gradient the optimizer
    consumed (with weight decay g + decay w: get_grads hands out the regularised gradient), and the weights end bit-equal to an engine
    built without the option, whose results never carry the keys."""
    from vltf_amd.engine import LRCNEngine
    p, batches = small_batches(3)
    eng = LRCNEngine(small_cfg(tensor_stats_interval=1, **OPTS[opt]), max_clips=B, device=DEV)
    plain = LRCNEngine(small_cfg(**OPTS[opt]), max_clips=B, device=DEV)
    assert plain.stat_segs is None and not hasattr(plain, "stat_out") and plain.tensor_stats() is None
    assert len(eng.stat_segs) == 16 and eng.stat_out.numel() == 16 * 64 and eng.tensor_stats() is None
    eng.load_params(p)
    plain.load_params(p)
    for i, lr in enumerate((LR, 0.02, 0.005)):
        before = eng.get_params()
        out = eng.train_step_u8(*batches[i], lr=lr, clip_norm=CLIP, mean_bgr=MEAN)
        ref = plain.train_step_u8(*batches[i], lr=lr, clip_norm=CLIP, mean_bgr=MEAN)
        assert set(out) - set(ref) == KEYS and all(out[k] == ref[k] for k in ref)
        check_stats_step(eng, out, before, eng.get_grads(), lr, CLIP, "%s step %d" % (opt, i))
    if opt == "momentum+decay":                           # the regulariser shows in the weight tensors' statistics
        assert out["tensor_stats"]["dcnn/fc6W"]["grad_norm"] > 0.0
    got, want = eng.get_params(), plain.get_params()
    for k in want:
        assert np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), k
    assert out["grad_norm"] > CLIP                        # the clip bit: the ratios carry its scale (close_reports)
    with_lr = out["tensor_stats"]["dcnn/conv1W"]
    assert with_lr["sgd_update_ratio"] == pytest.approx(0.005 * CLIP / out["grad_norm"] * with_lr["grad_norm"] / with_lr["weight_norm"], rel=1e-12)


def test_interval_two_and_a_look_without_fetch():
    from vltf_amd._ffi import VltfError
    from vltf_amd.engine import LRCNEngine
    p, batches = small_batches(3)
    eng = LRCNEngine(small_cfg(tensor_stats_interval=2), max_clips=B, device=DEV)
    eng.load_params(p)
    outs = [eng.train_step_u8(*batches[i], lr=LR, clip_norm=CLIP, mean_bgr=MEAN) for i in range(2)]
    assert KEYS <= set(outs[0]) and not KEYS & set(outs[1])
    assert eng.tensor_stats() is outs[0]["tensor_stats"]                            # the most recent one
    before = eng.get_params()
    assert eng.train_step_u8(*batches[2], lr=0.02, clip_norm=CLIP, mean_bgr=MEAN, fetch=False) is None       # update 2: a stats step
    got = eng.tensor_stats()                                                          # synchronises and reads
    assert got is not outs[0]["tensor_stats"] and eng.tensor_stats() is got
    out = dict(tensor_stats=got, grads_norm_mean=eng._stats_last["grads_norm_mean"], grad_norm=math.sqrt(float(eng.ss.item())))
    check_stats_step(eng, out, before, eng.get_grads(), 0.02, CLIP, "fetch=False")
    for bad in (-1, 1.5, "2", True):
        with pytest.raises(VltfError, match="tensor_stats_interval"):
            LRCNEngine(small_cfg(tensor_stats_interval=bad), max_clips=B, device=DEV)
    with pytest.raises(VltfError, match="GraphEngine"):                             # a feature pipeline has no step of its own
        LRCNEngine(small_cfg(tensor_stats_interval=1, classifier="none"), max_clips=B, device=DEV)
    assert LRCNEngine(small_cfg(tensor_stats_interval=1), max_clips=B, device=DEV, training=False).stat_segs is None


def test_frozen_ranges_of_g_are_never_read():
    """train_from fc6, lr_mult 4: the conv stack is absent from the table; its range of g is filled with NaN and no statistic shows it."""
    from vltf_amd.engine import LRCNEngine
    p, batches = small_batches(1)
    eng = LRCNEngine(small_cfg(tensor_stats_interval=1, train_from="fc6", lr_mult=4.0), max_clips=B, device=DEV)
    eng.load_params(p)
    frozen = set(eng.plan.frozen)
    assert len(frozen) == 10 and [n for n, _, _ in eng.stat_segs] == [n for n, _ in eng.specs if n not in frozen]
    for k in frozen:
        eng.G[k].fill_(NAN)
    before = eng.get_params()
    out = eng.train_step_u8(*batches[0], lr=LR, clip_norm=CLIP, mean_bgr=MEAN)
    check_stats_step(eng, out, before, eng.get_grads(), LR, CLIP, "frozen")
    assert out["tensor_stats"]["output_fc_w"]["lr_mult"] == 4.0 and out["tensor_stats"]["dcnn/fc6W"]["lr_mult"] == 1.0
    for k in frozen:
        off, n = eng.offsets[k]
        assert bool(torch.isnan(eng.g[off:off + n]).all()), k


def test_accumulated_update_reports_the_summed_gradient():
    from vltf_amd.engine import LRCNEngine
    p, batches = small_batches(2, clips=1)
    eng = LRCNEngine(small_cfg(tensor_stats_interval=1, accumulate=2), max_clips=B, device=DEV)
    eng.load_params(p)
    before = eng.get_params()
    first = eng.train_step_u8(*batches[0], lr=LR, clip_norm=CLIP, mean_bgr=MEAN, micro=(0, 2))
    assert not KEYS & set(first) and eng.tensor_stats() is None
    g_first = eng.get_grads()
    out = eng.train_step_u8(*batches[1], lr=LR, clip_norm=CLIP, mean_bgr=MEAN, micro=(1, 2))
    grads = eng.get_grads()                               # the final micro-step leaves g = the sum of both
    check_stats_step(eng, out, before, grads, LR, CLIP, "accumulate 2")
    assert not np.array_equal(grads["dcnn/fc6W"], g_first["dcnn/fc6W"])


def test_captured_stats_steps_equal_eager_ones():
    """Interval 2 over six steps: updates 0, 2, 4 are stats steps.  Each of the two launch sequences warms up once and is captured
    once; every replayed result equals the eager engine's, the rows byte for byte, and the state stays that of a captured engine
    built without the option (its plain steps are the sequence of before)."""
    from tests.test_step_graph_gpu import batch, pair, same_state, train_both
    eager, graph = pair(B, fpc=FPC, hid=HID, tensor_stats_interval=2)
    _, off = pair(B, fpc=FPC, hid=HID)
    rng = np.random.default_rng(11)
    for step in range(6):
        bt = batch(rng, B, FPC)
        lr = 0.01 * (0.8 ** step)
        outs = train_both((eager, graph), bt, lr=lr)
        ref = off.train_step_u8(bt["frames_u8"], bt["onehot"], lr, 5.0, MEAN, bt["crop_y"], bt["crop_x"], bt["mirror"])
        assert (KEYS <= set(outs[0])) == (step % 2 == 0) and set(outs[0]) == set(outs[1])
        if step % 2 == 0:
            assert outs[0]["tensor_stats"] == outs[1]["tensor_stats"] and outs[0]["grads_norm_mean"] == outs[1]["grads_norm_mean"]
            assert torch.equal(eager.stat_out, graph.stat_out) and torch.equal(eager.stat_ss, graph.stat_ss)
            assert outs[1]["tensor_stats"]["dcnn/fc6W"]["sgd_update_ratio"] > 0.0
        assert all(ref[k] == outs[1][k] for k in ref)
    same_state(eager, graph)
    same_state(off, graph)
    assert len(graph._graphs) == 2 and len(off._graphs) == 1


# ---- one-rank RCCL -------------------------------------------------------------------------------------------------------------------
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
    cfg = NetConfig(image_shape=shape, num_classes=ncls, fpc=fpc, lstm_hidden=hid, tensor_stats_interval=1)
    eng = LRCNEngine(cfg, max_clips=clips, device="cuda:0", dp=dp.GradAllReduce(always=True))
    ref = LRCNEngine(cfg, max_clips=clips, device="cuda:0")
    eng.load_params(p)
    ref.load_params(p)
    same, keys = True, True
    for lr in (0.05, 0.02):
        a = eng.train_step_u8(frames, onehot, lr=lr, clip_norm=0.5, mean_bgr=MEAN)
        b = ref.train_step_u8(frames, onehot, lr=lr, clip_norm=0.5, mean_bgr=MEAN)
        keys = keys and "tensor_stats" in a and "grads_norm_mean" in a
        same = same and a["tensor_stats"] == b["tensor_stats"] and a["grads_norm_mean"] == b["grads_norm_mean"] and \
            bool(torch.equal(eng.stat_out, ref.stat_out))
    e = eng.train_step_empty(0.01, 0.5)                   # the same path: zero gradients, the same launch
    zero = all(d["grad_norm"] == 0.0 and d["grad_zero_fraction"] == 1.0 for d in e["tensor_stats"].values())
    got, want = eng.get_params(), ref.get_params()
    torch.cuda.synchronize()
    q.put(dict(same=same and all(np.array_equal(got[k], want[k]) for k in want), keys=keys, zero=zero))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_one_rank_rccl_equals_no_data_parallelism():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    pr = ctx.Process(target=dp_worker, args=(free_port(), q))
    pr.start()
    pr.join(300)
    assert pr.exitcode == 0, "rank exited with %s" % pr.exitcode
    r = q.get(timeout=10)
    assert r["same"] and r["keys"] and r["zero"], r


# ---- GraphEngine ---------------------------------------------------------------------------------------------------------------------
def test_graph_engine_names_carry_the_pipeline_scope():
    from tests import graph_cases as GC
    from tests.test_graph_gpu import device_feeds
    from vltf_amd._ffi import VltfError
    from vltf_amd.graph import GraphEngine
    case = GC.CASES["encdec_state"]()                     # two pipelines, one tower of 2-frame clips: the smallest of graph_cases
    pipes, ds = GC.specs_and_datasets(case)
    with pytest.raises(VltfError, match="tensor_stats_interval"):
        GraphEngine(pipes, ds, case["V"], device=DEV, tensor_stats_interval=-2)
    eng = GraphEngine(pipes, ds, case["V"], device=DEV, lr_mult=3.0, tensor_stats_interval=2)
    off = GraphEngine(pipes, ds, case["V"], device=DEV, lr_mult=3.0)
    assert off.stat_segs is None and off.tensor_stats() is None
    assert [n for n, _, _ in eng.stat_segs] == [n for n, _ in eng.specs]
    assert all(n.split("/")[0] in ("enc", "dec") for n, _, _ in eng.stat_segs) and "enc/dcnn/conv1W" in dict((n, 0) for n, _, _ in eng.stat_segs)
    p = eng.init_params(seed=case["seed"], well_scaled=True)
    raw, _ = GC.inputs(case)
    fd = device_feeds(raw)
    eng.load_params(p)
    off.load_params(p)
    eng.forward(fd)
    rows = eng.logits_host().shape[0]
    onehot = torch.tensor(O.labels_to_one_hot([[l] for l in np.random.default_rng(0).integers(0, case["V"], rows)], case["V"]), device=DEV)
    for i, lr in enumerate((LR, 0.02, 0.005)):
        before = eng.get_params()
        out = eng.train_step(fd, onehot, lr=lr, clip_norm=CLIP)
        ref = off.train_step(fd, onehot, lr=lr, clip_norm=CLIP)
        assert all(out[k] == ref[k] for k in ref)
        if i == 1:
            assert not KEYS & set(out)
        else:
            check_stats_step(eng, out, before, eng.get_grads(), lr, CLIP, "graph step %d" % i)
            assert out["tensor_stats"]["enc/dcnn/conv1W"]["lr_mult"] == 1.0 and out["tensor_stats"]["dec/output_fc_w"]["lr_mult"] == 3.0
    got, want = eng.get_params(), off.get_params()
    for k in want:
        assert np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), k


# ---- run_task ------------------------------------------------------------------------------------------------------------------------
def test_run_task_writes_one_line_per_update(tmp_path, monkeypatch):
    """`logging: tensor_stats_interval: 1`: six updates, six strict-JSON lines whose grad_norm is the log's, and the same final weights
    as the run without the key (there is no new state)."""
    monkeypatch.setenv("VLTF_PREFETCH", "0")
    monkeypatch.setenv("VLTF_CONV_MATH", "f32")
    from tests.test_host_workflow import make_dataset
    from tests.test_run_task_gpu import RAW, write_cfg
    from vltf_amd import run_task
    folder = str(tmp_path)
    train_path, _, _ = make_dataset(folder, "train.txt", shape=RAW, seed=1)

    def cfg(name, run, interval):
        path = write_cfg(folder, name, train_path, "train", epochs=2, det=True, run=run)
        with open(path) as f:
            c = yaml.safe_load(f)
        c["run"]["train"].update(base_lr=0.01)
        if interval is not None:
            c["run"]["logging"].update(tensor_stats_interval=interval)
        with open(path, "w") as f:
            yaml.safe_dump(c, f)
        return path

    def final_weights(run):
        ck = sorted(glob.glob(os.path.join(folder, run, "checkpoints", "*.weights.npz")), key=os.path.getmtime)
        with np.load(ck[-1], allow_pickle=False) as z:
            return {k: z[k] for k in z.files}

    run_task.main(cfg("a.yml", "runA", 1), seed=3)
    path = os.path.join(folder, "runA", "e2e_train_scratch_tensor_stats.jsonl")
    lines = open(path).read().splitlines()
    recs = [json.loads(l, parse_constant=lambda c: pytest.fail("non-strict JSON constant %s" % c)) for l in lines]
    assert [r["global_step"] for r in recs] == [1, 2, 3, 4, 5, 6] and [r["update"] for r in recs] == [0, 1, 2, 3, 4, 5]
    log = open(glob.glob(os.path.join(folder, "runA", "log_e2e_train_scratch_*.log"))[0]).read()
    logged = [(float(a), float(b)) for a, b in re.findall(r"gradient norm : (\S+), mean per variable : (\S+)", log)]
    assert len(logged) == 6 and log.count("Tensor statistics over 16 variables") == 6 and "Non-finite" not in log
    for r, (gn, mean) in zip(recs, logged):
        assert abs(r["grad_norm"] - gn) <= 1e-7 * gn and abs(r["grads_norm_mean"] - mean) <= 1e-7 * mean      # (%.8g in the log)
        assert len(r["vars"]) == 16 and r["clip_scale"] == pytest.approx(min(1.0, 5.0 / r["grad_norm"]), rel=1e-12)
        assert r["vars"]["dcnn/fc6W"]["sgd_update_ratio"] > 0.0
    run_task.main(cfg("plain.yml", "runB", None), seed=3)
    assert not glob.glob(os.path.join(folder, "runB", "*tensor_stats*"))
    full, plain = final_weights("runA"), final_weights("runB")
    assert sorted(full) == sorted(plain)
    for k in full:
        np.testing.assert_array_equal(full[k], plain[k], err_msg=k)
