"""L2 weight decay on the device (vl_l2_regularize, NetConfig.weight_decay, GraphEngine(weight_decay=)): the launch that takes the
global norm's place writes g <- g + decay * w in place and returns sum g'^2 and sum (decay / 2) w^2 -- against float64, through odd
range tables and alignments, in LRCNEngine (eager and captured, with frozen layers), GraphEngine, one-rank RCCL and run_task.
Small shapes: the kernel on 4096*256 + 4099 elements (every lane loops, and a tail), the engines on 67x67x3 frames, 2 clips x 3
frames, hidden 8, 7 classes.  Tolerances, all the project's: sums against float64 1e-6 relative (test_sumsq_tiers), grad_norm against
the fetched gradients 1e-5 relative (test_momentum_gpu.check_steps), parameters after an update rtol 1e-5 and atol 1e-6 * max|want|
(test_momentum_gpu.close); g' against float32(float64(decay) * w + g) one unit in the last place (the fma rounds once, the float64
route twice)."""
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
WD = 0.05                 # large enough that the decay moves fc6 visibly at these shapes
NAN = float("nan")


def bits(t):
    return t.view(torch.int32)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def close(got, want, msg=""):
    want = np.asarray(want, np.float64)
    scale = float(np.abs(want).max()) or 1.0
    np.testing.assert_allclose(np.asarray(got, np.float64), want, rtol=1e-5, atol=1e-6 * scale, err_msg=msg)


def fma_ref(decay, w, g):
    """float32(float64(float32 decay) * w + g): the product of two floats is exact in float64, so this rounds twice where fmaf rounds once."""
    return (np.float64(np.float32(decay)) * np.asarray(w, np.float64) + np.asarray(g, np.float64)).astype(np.float32)


def within_one_ulp(got, want, msg=""):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    ulp = np.maximum(np.spacing(np.abs(want)), np.spacing(np.abs(got))).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert np.isfinite(got).all() and (err <= ulp).all(), (msg, float((err / ulp).max()))


def clip_scale(clip, norm):
    return clip / max(norm, clip) if clip > 0 else 1.0


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------
COUNT = 4096 * 256 + 4099
# boundaries off multiples of 4, an entry of one element, a gap of one element (4099) and a wide one, decay / 0 entries side by side
RANGES = [(5, 1000, 0.01), (1000, 4099, 0.0), (4100, 4101, 0.5), (9001, 20000, 0.0), (20000, COUNT, 0.01)]
_K = {}


def kernel_data():
    """Host w, g (float32; NaN outside every entry, w NaN inside the decay-0 entries too) and the float64 expectations; made once."""
    if not _K:
        gen = torch.Generator(device="cpu").manual_seed(3)
        w, g = torch.randn(COUNT, generator=gen).numpy(), torch.randn(COUNT, generator=gen).numpy()
        decayed, summed = np.zeros(COUNT, bool), np.zeros(COUNT, bool)
        want_g, ss, rs = g.copy(), 0.0, 0.0
        for lo, hi, d in RANGES:
            summed[lo:hi] = True
            w64, g64 = w[lo:hi].astype(np.float64), g[lo:hi].astype(np.float64)
            if d > 0:
                decayed[lo:hi] = True
                want_g[lo:hi] = fma_ref(d, w[lo:hi], g[lo:hi])
                ss += float(((np.float64(np.float32(d)) * w64 + g64) ** 2).sum())
                rs += float((0.5 * np.float64(np.float32(d)) * w64 * w64).sum())
            else:
                ss += float((g64 * g64).sum())
        w[~decayed] = NAN
        g[~summed] = NAN
        _K.update(w=w, g=g, decayed=decayed, want_g=want_g, ss=ss, rs=rs, ss_plain=float((g[summed].astype(np.float64) ** 2).sum()))
    return _K


def run_kernel(w, g, ranges=RANGES):
    from vltf_amd import ops
    out, ws = torch.full((2,), NAN, device=DEV), torch.empty(2048, device=DEV)
    ops.l2_regularize(w, g, ranges, out, ws)
    return host(out).copy()


def first_result():
    """The aligned call's g' and sums, computed once and shared (tests 1 and 2)."""
    if "got_g" not in _K:
        k = kernel_data()
        w, g = torch.from_numpy(k["w"]).to(DEV), torch.from_numpy(k["g"]).to(DEV)
        assert w.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0
        _K["out"] = run_kernel(w, g)
        _K["got_g"] = host(g).copy()
    return _K["got_g"], _K["out"]


def check_sums(out, k, msg=""):
    assert np.isfinite(out).all(), (msg, out)
    assert abs(float(out[0]) - k["ss"]) <= 1e-6 * k["ss"], (msg, out[0], k["ss"])
    assert abs(float(out[1]) - k["rs"]) <= 1e-6 * k["rs"], (msg, out[1], k["rs"])


def test_kernel_against_fp64():
    k = kernel_data()
    got, out = first_result()
    d = k["decayed"]
    within_one_ulp(got[d], k["want_g"][d], "g'")
    assert np.mean(got[d] == k["want_g"][d]) > 0.99                                # (the two routes differ in the last bit rarely)
    assert np.array_equal(got[~d].view(np.int32), k["g"][~d].view(np.int32))       # decay-0 entries and gaps: g keeps its bits
    check_sums(out, k)
    w, g = torch.from_numpy(k["w"]).to(DEV), torch.from_numpy(k["g"]).to(DEV)      # a second call on fresh copies: the same words
    again = run_kernel(w, g)
    assert np.array_equal(again.view(np.int32), out.view(np.int32))
    assert np.array_equal(host(g).view(np.int32), got.view(np.int32))


@pytest.mark.parametrize("ow,og", [(3, 3), (1, 2)], ids=["phase3", "phases-disagree"])
def test_kernel_alignment(ow, og):
    """Views w[ow:], g[og:] of 16-byte aligned buffers: a shared phase that is not 0 (head / interior / tail move), and phases that
    disagree (the scalar path).  Every element's g' has the bits of the aligned call; the sums keep their tolerance."""
    k = kernel_data()
    want, _ = first_result()
    wb, gb = torch.full((COUNT + ow,), NAN, device=DEV), torch.full((COUNT + og,), NAN, device=DEV)
    assert wb.data_ptr() % 16 == 0 and gb.data_ptr() % 16 == 0
    wb[ow:] = torch.from_numpy(k["w"]).to(DEV)
    gb[og:] = torch.from_numpy(k["g"]).to(DEV)
    out = run_kernel(wb[ow:], gb[og:])
    assert np.array_equal(host(gb[og:]).view(np.int32), want.view(np.int32))
    assert bool(torch.isnan(gb[:og]).all())                                         # the elements before the view
    check_sums(out, k)


def test_kernel_all_zero_table():
    k = kernel_data()
    w, g = torch.from_numpy(k["w"]).to(DEV), torch.from_numpy(k["g"]).to(DEV)
    w.fill_(NAN)                                                                    # never loaded
    out = run_kernel(w, g, [(lo, hi, 0.0) for lo, hi, _ in RANGES])
    assert np.array_equal(host(g).view(np.int32), k["g"].view(np.int32))
    assert float(out[1]) == 0.0
    assert abs(float(out[0]) - k["ss_plain"]) <= 1e-6 * k["ss_plain"]


def test_kernel_refusals_change_nothing():
    from vltf_amd import ops
    from vltf_amd._ffi import VltfError
    k = kernel_data()
    w, g = torch.from_numpy(k["w"]).to(DEV), torch.from_numpy(k["g"]).to(DEV)
    out, ws = torch.full((2,), 7.0, device=DEV), torch.empty(2048, device=DEV)
    tables = {"empty": [], "unsorted": [(10, 20, 0.1), (5, 8, 0.1)], "overlap": [(0, 10, 0.1), (9, 20, 0.1)],
              "past count": [(0, COUNT + 1, 0.1)], "65 entries": [(i, i + 1, 0.1) for i in range(65)],
              "negative": [(0, 10, 0.1), (10, 20, -1.0)], "nan": [(0, 10, NAN)], "inf": [(0, 10, float("inf"))]}
    for name, table in tables.items():
        with pytest.raises(VltfError):
            ops.l2_regularize(w, g, table, out, ws)
    with pytest.raises(VltfError, match="range 1"):                                 # the message names the entry
        ops.l2_regularize(w, g, tables["negative"], out, ws)
    with pytest.raises(VltfError, match="2048"):
        ops.l2_regularize(w, g, RANGES, out, torch.empty(2047, device=DEV))
    with pytest.raises(VltfError, match="2 floats"):
        ops.l2_regularize(w, g, RANGES, out[:1], ws)
    with pytest.raises(VltfError):
        ops.l2_regularize(w, g.double(), RANGES, out, ws)
    assert np.array_equal(host(g).view(np.int32), k["g"].view(np.int32)) and host(out).tolist() == [7.0, 7.0]
    ops.l2_regularize(w, g, [(i, i + 1, 0.0) for i in range(5, 69)], out, ws)     # 64 entries are taken
    assert math.isfinite(float(host(out)[0]))


# ---- engines ------------------------------------------------------------------------------------------------------------------------
SHAPE, NCLS, FPC, B, HID = (67, 67, 3), 7, 3, 2, 8
LR, CLIP = 0.01, 0.5


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


class Rule:
    """The optimizer's rule in float64 on the (already regularised) gradient; state per variable, zero before the first step."""

    def __init__(self, kind, momentum=0.0):
        self.kind, self.momentum, self.state, self.t = kind, momentum, {}, 0

    def begin_step(self):
        self.t += 1

    def __call__(self, name, w, g, lr, sc):
        w, gi = np.asarray(w, np.float64), np.asarray(g, np.float64) * sc
        if self.kind == "adam":
            m, v = self.state.get(name, (0.0, 0.0))
            m, v = 0.9 * m + 0.1 * gi, 0.999 * v + 0.001 * gi * gi
            self.state[name] = (m, v)
            return w - lr * math.sqrt(1 - 0.999 ** self.t) / (1 - 0.9 ** self.t) * m / (np.sqrt(v) + 1e-8)
        if self.momentum > 0:
            a = self.momentum * self.state.get(name, 0.0) + gi
            self.state[name] = a
            return w - lr * a
        return w - lr * gi


def reg_ref(params, decay, skip=()):
    return 0.5 * decay * sum(float((v.astype(np.float64) ** 2).sum()) for k, v in params.items() if v.ndim >= 2 and k not in skip)


def check_own_step(out, before, g, after, rule, lr, decay, mult=None, frozen=(), msg=""):
    """One step of an engine with weight decay against what it fetched itself: reg_loss at the weights before the step, grad_norm of
    the regularised gradient, and the rule applied to that gradient with the clip scale of that norm."""
    want_reg = reg_ref(before, np.float64(np.float32(decay)), frozen)
    assert abs(out["reg_loss"] - want_reg) <= 1e-6 * want_reg, (msg, out["reg_loss"], want_reg)
    gn = math.sqrt(sum(float((v.astype(np.float64) ** 2).sum()) for v in g.values()))
    assert abs(out["grad_norm"] - gn) <= 1e-5 * gn, (msg, out["grad_norm"], gn)
    sc = clip_scale(CLIP, out["grad_norm"])
    rule.begin_step()
    for k in before:
        if k in frozen:
            assert np.array_equal(after[k].view(np.int32), before[k].view(np.int32)), k
            continue
        close(after[k].ravel(), rule(k, before[k].ravel(), g[k].ravel(), lr * (mult[k] if mult else 1.0), sc), "%s param %s" % (msg, k))


def differential(out_a, g_a, out_b, g_b, before, decay):
    """Engine B (decay) against its twin A (none) after the first step from the same parameters and batch."""
    assert out_b["loss"] == out_a["loss"] and out_b["loss_sum"] == out_a["loss_sum"] and math.isfinite(out_b["loss"])
    assert "reg_loss" not in out_a and sorted(set(out_b) - set(out_a)) == ["reg_loss"]
    for k, ga in g_a.items():
        if ga.ndim >= 2:
            within_one_ulp(g_b[k], fma_ref(decay, before[k], ga), k)
            assert not np.array_equal(g_b[k], ga), k
        else:
            assert np.array_equal(g_b[k].view(np.int32), ga.view(np.int32)), k


OPTS = {"sgd": dict(), "momentum": dict(momentum=0.9), "adam": dict(optimizer="adam")}


@pytest.mark.parametrize("opt,arith", [("sgd", "f32"), ("momentum", "f32"), ("adam", "f32"), ("momentum", "bf16")])
def test_engine_differential(opt, arith):
    from vltf_amd.engine import LRCNEngine
    p, batches = small_batches(1)
    a = LRCNEngine(small_cfg(conv_math=arith, **OPTS[opt]), max_clips=B, device=DEV)
    b = LRCNEngine(small_cfg(conv_math=arith, weight_decay=WD, **OPTS[opt]), max_clips=B, device=DEV)
    assert a.ss2 is None and a.decay is None and a.ss.numel() == 1                  # off: nothing new
    assert b.ss2.numel() == 2 and len(b.decay) == 16 and b.ss.data_ptr() == b.ss2.data_ptr()
    outs, grads, params = [], [], []
    for eng in (a, b):
        eng.load_params(p)
        outs.append(eng.train_step_u8(*batches[0], lr=LR, clip_norm=CLIP, mean_bgr=MEAN))
        grads.append(eng.get_grads())
        params.append(eng.get_params())
    p32 = {k: np.asarray(v, np.float32) for k, v in p.items()}
    differential(outs[0], grads[0], outs[1], grads[1], p32, WD)
    check_own_step(outs[1], p32, grads[1], params[1],
                   Rule("adam" if opt == "adam" else "sgd", OPTS[opt].get("momentum", 0.0)), LR, WD, msg=opt)
    assert not np.array_equal(params[0]["dcnn/fc6W"], params[1]["dcnn/fc6W"])
    assert outs[1]["grad_norm"] != outs[0]["grad_norm"]


def test_engine_refusals_and_off_allocates_nothing():
    from vltf_amd._ffi import VltfError
    from vltf_amd.engine import LRCNEngine
    for bad in (-0.1, NAN, float("inf"), "0.1"):
        with pytest.raises(VltfError, match="weight_decay"):
            LRCNEngine(small_cfg(weight_decay=bad), max_clips=B, device=DEV)
    with pytest.raises(VltfError, match="GraphEngine"):                             # a feature pipeline has no step of its own
        LRCNEngine(small_cfg(weight_decay=WD, classifier="none"), max_clips=B, device=DEV)
    for eng in (LRCNEngine(small_cfg(weight_decay=None), max_clips=B, device=DEV),
                LRCNEngine(small_cfg(weight_decay=WD), max_clips=B, device=DEV, training=False)):
        assert eng.ss2 is None and eng.decay is None


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "captured"])
def test_weight_decay_with_finetuning(graph):
    """train_from fc6 and lr_mult 4: the frozen conv stack is outside every entry -- its g (NaN) is never read or written, its weights
    keep their bits and stay out of the regulariser -- and the trained variables follow the rule with lr * mult on g + decay * w."""
    from vltf_amd.engine import LRCNEngine, is_regular
    p, batches = small_batches(2)
    eng = LRCNEngine(small_cfg(weight_decay=WD, train_from="fc6", lr_mult=4.0, step_graph=graph), max_clips=B, device=DEV)
    eng.load_params(p)
    frozen = set(eng.plan.frozen)
    assert frozen == {"dcnn/conv%d%s" % (i, k) for i in range(1, 6) for k in "Wb"} and len(eng.decay) == 6
    for k in frozen:
        eng.G[k].fill_(NAN)
    mult = {k: (1.0 if is_regular(k) else 4.0) for k in p}
    rule = Rule("sgd")
    for i, lr in enumerate((0.01, 0.02)):                   # (captured: step 1 is the eager warm-up, step 2 the capture and its replay)
        before = eng.get_params()
        out = eng.train_step_u8(*batches[i], lr=lr, clip_norm=CLIP, mean_bgr=MEAN)
        check_own_step(out, before, eng.get_grads(), eng.get_params(), rule, lr, WD, mult, frozen, "step %d" % i)
        assert reg_ref(before, WD) > 1.001 * out["reg_loss"]                        # the conv weights would have shown
    for k in frozen:
        off, n = eng.offsets[k]
        assert bool(torch.isnan(eng.g[off:off + n]).all()), k
    assert (len(eng._graphs) == 1) if graph else not eng.step_graph


def test_captured_step_equals_eager():
    """Step 1 is the warm-up, step 2 is captured and replayed, step 3 is a replay; lr changes every step.  The state is bit-equal
    after each step and the captured engine reports the same regulariser."""
    from tests.test_step_graph_gpu import batch, pair, same_state, train_both
    eager, graph = pair(B, fpc=FPC, hid=HID, weight_decay=WD)
    rng = np.random.default_rng(11)
    for lr in (0.01, 0.02, 0.005):
        outs = train_both((eager, graph), batch(rng, B, FPC), lr=lr)
        assert outs[0]["reg_loss"] == outs[1]["reg_loss"] > 0.0
        same_state(eager, graph)
        assert torch.equal(bits(eager.g), bits(graph.g))
    assert len(graph._graphs) == 1


def test_graph_engine_two_steps():
    from tests import graph_cases as GC
    from tests.test_graph_gpu import device_feeds
    from vltf_amd._ffi import VltfError
    from vltf_amd.graph import GraphEngine
    case = GC.CASES["encdec_state"]()                   # two pipelines, one tower of 2-frame clips: the smallest of graph_cases
    pipes, ds = GC.specs_and_datasets(case)
    with pytest.raises(VltfError, match="weight_decay"):
        GraphEngine(pipes, ds, case["V"], device=DEV, weight_decay=-0.01)
    a = GraphEngine(pipes, ds, case["V"], device=DEV, momentum=0.9)
    b = GraphEngine(pipes, ds, case["V"], device=DEV, momentum=0.9, weight_decay=WD)
    assert a.ss2 is None and a.decay is None and b.ss2.numel() == 2
    off = 0
    for _, shp in b.specs:                              # every variable lies in one entry, with its rank's coefficient
        n = int(np.prod(shp))
        assert [c for lo, hi, c in b.decay if lo <= off and off + n <= hi] == [WD if len(shp) >= 2 else 0.0]
        off += n
    assert b.decay[0][0] == 0 and b.decay[-1][1] == off and all(x[1] == y[0] for x, y in zip(b.decay, b.decay[1:]))
    p = b.init_params(seed=case["seed"], well_scaled=True)
    raw, _ = GC.inputs(case)
    fd = device_feeds(raw)
    a.load_params(p)
    b.load_params(p)
    a.forward(fd)
    rows = a.logits_host().shape[0]
    onehot = torch.tensor(O.labels_to_one_hot([[l] for l in np.random.default_rng(0).integers(0, case["V"], rows)], case["V"]), device=DEV)
    out_a = a.train_step(fd, onehot, lr=LR, clip_norm=CLIP)
    rule = Rule("sgd", 0.9)
    for i, lr in enumerate((LR, 0.02)):
        before = b.get_params()
        out_b = b.train_step(fd, onehot, lr=lr, clip_norm=CLIP)
        g_b, after = b.get_grads(), b.get_params()
        if i == 0:
            differential(out_a, a.get_grads(), out_b, g_b, before, WD)
            assert any(not np.array_equal(after[k], v) for k, v in a.get_params().items() if v.ndim >= 2)
        check_own_step(out_b, before, g_b, after, rule, lr, WD, msg="step %d" % i)


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
    from vltf_amd.engine import LRCNEngine, NetConfig
    dp.init_from_env(backend="nccl", force=True)
    shape, ncls, fpc, clips, hid = (67, 67, 3), 5, 2, 4, 6
    rng = np.random.default_rng(11)
    p = O.init_params(rng, ncls, "fc6", hid, 1, shape, well_scaled=True)
    frames = torch.tensor(rng.integers(0, 256, (clips * fpc,) + shape, dtype=np.uint8), device="cuda:0")
    onehot = torch.tensor(O.labels_to_one_hot([[l] for l in rng.integers(0, ncls, clips)], ncls), device="cuda:0")
    cfg = NetConfig(image_shape=shape, num_classes=ncls, fpc=fpc, lstm_hidden=hid, momentum=0.9, weight_decay=0.05)
    eng = LRCNEngine(cfg, max_clips=clips, device="cuda:0", dp=dp.GradAllReduce(always=True))
    ref = LRCNEngine(cfg, max_clips=clips, device="cuda:0")
    eng.load_params(p)
    ref.load_params(p)
    outs = []
    for lr in (0.05, 0.02):
        a = eng.train_step_u8(frames, onehot, lr=lr, clip_norm=0.5, mean_bgr=MEAN)
        b = ref.train_step_u8(frames, onehot, lr=lr, clip_norm=0.5, mean_bgr=MEAN)
        outs.append([(a[k], b[k]) for k in ("loss", "grad_norm", "reg_loss")])
    got, want = eng.get_params(), ref.get_params()
    torch.cuda.synchronize()
    q.put(dict(same=all(np.array_equal(got[k], want[k]) for k in want) and all(x == y for o in outs for x, y in o),
               moved=all(not np.array_equal(want[k], p[k]) for k in want), reg=all(o[2][0] > 0.0 for o in outs), outs=outs))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_one_rank_rccl_weight_decay_step():
    """Two steps with weight decay under a one-rank process group equal the engine without data parallelism bit for bit: the
    regulariser runs after the exchange on the reduced gradient and is not divided by the world size."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    pr = ctx.Process(target=dp_worker, args=(free_port(), q))
    pr.start()
    pr.join(300)
    assert pr.exitcode == 0, "rank exited with %s" % pr.exitcode
    r = q.get(timeout=10)
    assert r["same"] and r["moved"] and r["reg"], r


# ---- run_task -----------------------------------------------------------------------------------------------------------------------
def test_run_task_logs_trains_and_resumes(tmp_path, monkeypatch):
    """`weight_decay: 0.01` in the YAML: the log carries the regulariser, the run ends at other weights than the run without the
    key, and -- there being no new state -- a run resumed from the end-of-epoch-1 checkpoint ends exactly where the uninterrupted one does."""
    monkeypatch.setenv("VLTF_PREFETCH", "0")
    monkeypatch.setenv("VLTF_CONV_MATH", "f32")
    from tests.test_host_workflow import make_dataset
    from tests.test_run_task_gpu import RAW, write_cfg
    from vltf_amd import run_task
    folder = str(tmp_path)
    train_path, _, _ = make_dataset(folder, "train.txt", shape=RAW, seed=1)

    def cfg(name, run, decay, **kw):
        path = write_cfg(folder, name, train_path, "train", epochs=2, det=True, run=run, **kw)
        with open(path) as f:
            c = yaml.safe_load(f)
        c["run"]["train"].update(base_lr=0.01)
        if decay is not None:
            c["run"]["train"].update(weight_decay=decay)
        with open(path, "w") as f:
            yaml.safe_dump(c, f)
        return path

    def final_weights(run):
        ck = sorted(glob.glob(os.path.join(folder, run, "checkpoints", "*.weights.npz")), key=os.path.getmtime)
        with np.load(ck[-1], allow_pickle=False) as z:
            return ck, {k: z[k] for k in z.files}

    run_task.main(cfg("a.yml", "runA", 0.01), seed=3)
    ck, full = final_weights("runA")
    assert len(ck) == 2 and int(full["__optimizer__/step_count"][0]) == 6
    log = open(glob.glob(os.path.join(folder, "runA", "log_e2e_train_scratch_*.log"))[0]).read()
    assert log.count("L2 regulariser : ") == 6 and "batch loss/nats" in log
    regs = [float(x.split()[0]) for x in log.split("L2 regulariser : ")[1:]]
    assert all(r > 0.0 and math.isfinite(r) for r in regs)
    run_task.main(cfg("plain.yml", "runB", None), seed=3)
    _, plain = final_weights("runB")
    assert sorted(plain) == sorted(full)                                            # no new state in the checkpoint
    assert not np.array_equal(plain["dcnn/fc6W"], full["dcnn/fc6W"])
    assert "L2 regulariser" not in open(glob.glob(os.path.join(folder, "runB", "log_e2e_train_scratch_*.log"))[0]).read()
    first = ck[0][:-len(".weights.npz")]
    run_task.main(cfg("b.yml", "runA", 0.01, resume=first), seed=77)
    _, resumed = final_weights("runA")
    assert int(resumed["__optimizer__/step_count"][0]) == 6
    for k in full:
        np.testing.assert_array_equal(resumed[k], full[k], err_msg=k)
