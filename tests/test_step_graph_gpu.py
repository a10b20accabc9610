"""NetConfig.step_graph: train_step_u8 / forward_u8 captured once per input key and replayed.  The eager step is bitwise
reproducible, so every replayed result must EQUAL the eager engine's on the same inputs: loss sum, correct count,
grad norm and logits after every step, parameters and Adam's moments at the end -- with a new lr, new frames, labels and crop /
mirror every step (the baked-in scalars of a naive capture), dropout on (its seed follows the step count), the LSTM cluster form
(its exchange tags must move between replays)."""
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN = np.array([99.197148, 105.293620, 109.503945], np.float32)
RAW, SHAPE, NCLS = (80, 90, 3), (67, 67, 3), 7


def net(math="f32", opt="sgd", fpc=4, step_graph=False, shape=SHAPE, ncls=NCLS, hid=32, **kw):
    from vltf_amd.engine import NetConfig
    return NetConfig(image_shape=shape, num_classes=ncls, fpc=fpc, frame_encoding_layer="fc6", classifier="lstm", lstm_hidden=hid,
                     lstm_layers=1, fusion="avg", dropout_keep_prob=0.5, optimizer=opt, conv_math=math, step_graph=step_graph, **kw)


def pair(max_clips, seed=4, **kw):
    """(eager engine, step_graph engine) from the same parameters."""
    from vltf_amd.engine import LRCNEngine, init_params
    cfg_e, cfg_g = net(**kw), net(step_graph=True, **kw)
    params = init_params(cfg_e, seed=seed, well_scaled=True)
    out = []
    for cfg in (cfg_e, cfg_g):
        eng = LRCNEngine(cfg, max_clips=max_clips, device=DEV)
        eng.load_params(params)
        out.append(eng)
    return out


def batch(rng, clips, fpc, raw=RAW, shape=SHAPE, ncls=NCLS, crop_from=None):
    """New frames, labels and per-frame crop / mirror, as device tensors; crop_from: the (h, w) the crop is taken from (a resized frame)."""
    n = clips * fpc
    frames = torch.from_numpy(rng.integers(0, 256, (n,) + raw, dtype=np.uint8)).to(DEV)
    onehot = np.zeros((clips, ncls), np.int32)
    onehot[np.arange(clips), rng.integers(0, ncls, clips)] = 1
    ch, cw = crop_from or raw[:2]
    cy = torch.from_numpy(rng.integers(0, ch - shape[0] + 1, n).astype(np.int32)).to(DEV)
    cx = torch.from_numpy(rng.integers(0, cw - shape[1] + 1, n).astype(np.int32)).to(DEV)
    mir = torch.from_numpy(rng.integers(0, 2, n).astype(np.uint8)).to(DEV)
    return dict(frames_u8=frames, onehot=torch.from_numpy(onehot).to(DEV), crop_y=cy, crop_x=cx, mirror=mir)


def train_both(engines, bt, lr, clip_norm=5.0, resize=None):
    outs = [e.train_step_u8(bt["frames_u8"], bt["onehot"], lr, clip_norm, MEAN, bt["crop_y"], bt["crop_x"], bt["mirror"], resize=resize)
            for e in engines]
    logits = [e.logits_host() for e in engines]
    for k in ("loss_sum", "correct", "grad_norm", "rows"):
        assert outs[0][k] == outs[1][k], (k, outs[0][k], outs[1][k])
    assert np.array_equal(logits[0], logits[1]), np.abs(logits[0] - logits[1]).max()
    return outs


def same_state(a, b):
    pa, pb = a.get_params(), b.get_params()
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), k
    oa, ob = a.get_opt_state(), b.get_opt_state()
    assert sorted(oa) == sorted(ob)
    for k in oa:
        assert np.array_equal(oa[k], ob[k]), k
    assert a.step_count == b.step_count


@pytest.mark.parametrize("math", ["f32", "bf16"])
@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_replay_equals_eager_step_by_step(math, opt):
    """2 clips x 4 frames (8 frames: the bf16 path runs fc6 and the LSTM input projection on the packed-operand kernel too);
    step 1 is the warm-up, step 2 is captured and replayed, steps 3-5 are replays."""
    eager, graph = pair(2, math=math, opt=opt)
    rng = np.random.default_rng(11)
    for step in range(5):
        train_both((eager, graph), batch(rng, 2, 4), lr=0.01 * (0.7 ** step))
    assert len(graph._graphs) == 1 and graph.graph_tag_next > 1
    same_state(eager, graph)


def test_interleaved_forward_and_checkpoint_restore():
    """graph steps, an eager forward on other frames, more graph steps, then get_opt_state -> load_params + load_opt_state into a
    fresh step_graph engine and more steps: every result equals an all-eager run of the same sequence."""
    from vltf_amd.engine import LRCNEngine
    eager, graph = pair(2, opt="adam")
    rng = np.random.default_rng(12)
    for step in range(3):
        train_both((eager, graph), batch(rng, 2, 4), lr=0.02 / (step + 1))
    other = batch(rng, 2, 4)
    fw = [e.forward_u8(other["frames_u8"], MEAN, other["crop_y"], other["crop_x"], other["mirror"]).cpu().numpy() for e in (eager, graph)]
    assert np.array_equal(fw[0], fw[1])
    for step in range(2):
        train_both((eager, graph), batch(rng, 2, 4), lr=0.005 * (step + 1))
    same_state(eager, graph)
    fresh = []
    for e, sg in ((eager, False), (graph, True)):
        f = LRCNEngine(net(opt="adam", step_graph=sg), max_clips=2, device=DEV)
        f.load_params(e.get_params())
        assert f.load_opt_state(e.get_opt_state()) == []
        fresh.append(f)
    assert fresh[1].step_count == 5
    for step in range(3):
        train_both(fresh, batch(rng, 2, 4), lr=0.003 * (step + 1))
    same_state(*fresh)


def test_short_last_batch_gets_its_own_graph():
    """A short batch (fewer clips) in the middle of a graph run: its key's first call runs eagerly, its second is captured; the
    full-size graph goes on replaying around it."""
    eager, graph = pair(3, opt="adam")
    rng = np.random.default_rng(13)
    for step, clips in enumerate((3, 3, 2, 3, 2, 3, 2)):
        train_both((eager, graph), batch(rng, clips, 4), lr=0.01 + 0.001 * step)
    assert len(graph._graphs) == 2
    same_state(eager, graph)


def test_tag_wrap():
    """Across the wrap of the graph workspace's tags, the exchange words must be zeroed.  A 3-clip graph replays first at origin 1;
    a 2-clip graph then replays just below the limit (it rewrites only part of the words the 3-clip graph used); the next 3-clip
    replay no longer fits, so the words are zeroed and the tags start over at 1 -- the 3-clip graph's first replay's tags, which
    words the 2-clip graph never touched still hold.  Every step equals eager.  A stale tag that matches yields a wrong value only
    when a reader outruns the peer that rewrites the word, so equality alone need not catch a missing clear: the clear itself is
    checked directly at the end."""
    eager, graph = pair(3)
    rng = np.random.default_rng(14)
    for clips in (3, 3, 2, 2):                       # warm-up + capture of each key: the 3-clip graph's replay at origin 1
        train_both((eager, graph), batch(rng, clips, 4), lr=0.01)
    spans = {k[1] // 4: g["span"] for k, g in graph._graphs.items()}
    assert sorted(spans) == [2, 3] and spans[3] > 0 and spans[2] > 0
    graph.graph_tag_next = graph.GRAPH_TAG_LIMIT - spans[2] - 1
    for clips in (2, 3, 2, 3):                       # fits below the limit; wraps to 1; then above the wrap
        train_both((eager, graph), batch(rng, clips, 4), lr=0.01)
    assert graph.graph_tag_next == 1 + 2 * spans[3] + spans[2]
    same_state(eager, graph)
    # the wrap zeroes every exchange word: all of the workspace past its status block (the first 256 bytes, csrc/lstm_cluster.hip)
    words = graph.lstm_ws_graph.view(torch.int32)
    torch.cuda.synchronize()
    assert bool(words[64:].any())
    graph.graph_tag_next = graph.GRAPH_TAG_LIMIT
    assert graph._graph_tag_origin(spans[3]) == 1 and graph.graph_tag_next == 1 + spans[3]
    torch.cuda.synchronize()
    assert not bool(words[64:].any())


def test_resize_chain_short_batch_captured_first():
    """A two-pass resize (both axes change: the resizer needs an intermediate) under step_graph, a short batch's graph captured
    before the first full batch arrives: the full batch's eager warm-up grows the resizer's own intermediate, and the short
    graph must not have baked in the one it replaced.  Every step equals eager."""
    resize, mid = [((80, 90), (72, 84))], (72, 84)
    eager, graph = pair(3, opt="adam")
    rng = np.random.default_rng(17)
    for step, clips in enumerate((2, 2, 3, 3, 2, 3, 2, 3)):
        train_both((eager, graph), batch(rng, clips, 4, crop_from=mid), lr=0.01 + 0.001 * step, resize=resize)
    x = batch(rng, 2, 4, crop_from=mid)
    for _ in range(3):                               # the forward graph over the same resizer
        got = [e.forward_u8(x["frames_u8"], MEAN, x["crop_y"], x["crop_x"], x["mirror"], resize=resize).cpu().numpy() for e in (eager, graph)]
        assert np.array_equal(got[0], got[1])
    assert len(graph._graphs) == 3
    same_state(eager, graph)


def test_forward_replay_over_two_inputs():
    """Replays of one forward graph over alternating inputs: each returns that input's eager logits (a replay that reused its
    predecessor's LSTM tags would read the predecessor's h_t words and return its logits)."""
    eager, graph = pair(2)
    rng = np.random.default_rng(15)
    xs = [batch(rng, 2, 4) for _ in range(2)]
    for i in (0, 1, 0, 1, 1, 0):
        x = xs[i]
        got = [e.forward_u8(x["frames_u8"], MEAN, x["crop_y"], x["crop_x"], x["mirror"]).cpu().numpy() for e in (eager, graph)]
        assert np.array_equal(got[0], got[1]), i
    assert len(graph._graphs) == 1


def test_eager_lstm_call_refused_under_capture():
    """vl_lstm_seq_fwd bakes its tags into the launch: on a capturing stream it returns an error (host side, nothing launched)."""
    from vltf_amd import ops
    from vltf_amd._ffi import VltfError
    B, T, H = 2, 3, 16
    f = lambda *s: torch.zeros(s, device=DEV)
    gx, kh, act, cseq, hseq, hprev = f(B * T, 4 * H), f(H, 4 * H), f(B * T, 4 * H), f(B * T, H), f(B * T, H), f(B * T, H)
    ws = ops.lstm_seq_ws(B, T, H, DEV)
    g = torch.cuda.CUDAGraph()
    with pytest.raises(VltfError, match="captured"):
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            ops.lstm_seq_fwd(gx, kh, act, cseq, hseq, hprev, B, T, H, ws=ws)
    ops.lstm_seq_fwd(gx, kh, act, cseq, hseq, hprev, B, T, H, ws=ws)        # outside a capture: runs
    torch.cuda.synchronize()
    ops.lstm_seq_check(ws)


def test_refusals():
    from vltf_amd.engine import LRCNEngine
    from vltf_amd._ffi import VltfError
    with pytest.raises(VltfError, match="data parallelism"):
        LRCNEngine(net(step_graph=True), max_clips=2, device=DEV, dp=object())
    eng = LRCNEngine(net(step_graph=True), max_clips=2, device=DEV)
    with pytest.raises(VltfError, match="probe"):
        eng.set_probe(["conv1.fwd"])


def test_run_task_refusals(tmp_path, monkeypatch):
    """VLTF_STEP_GRAPH=1 with --gpus 2 is refused before any rank starts; with a two-pipeline model (GraphEngine) it is refused too."""
    from tests.test_run_task_graph_gpu import CPV, V, make_dataset, write_two_stream_cfg
    from tests.test_run_task_gpu import write_cfg
    from vltf_amd import run_task
    folder = str(tmp_path)
    monkeypatch.setenv("VLTF_STEP_GRAPH", "1")
    monkeypatch.setattr(run_task.dpmod, "self_launch", lambda n: pytest.fail("a rank was started"))
    train_path, _, _ = make_dataset(folder, "train.txt", shape=RAW, seed=1)
    with pytest.raises(Exception, match="VLTF_STEP_GRAPH=1 is refused with --gpus 2"):
        run_task.cli([write_cfg(folder, "train.yml", train_path, "train"), "--gpus", "2"])
    rpath, _, _ = make_dataset(folder, "rgb.txt", nvid=5, cpv=CPV, shape=RAW, classes=V, seed=7)
    fpath, _, _ = make_dataset(folder, "flow.txt", nvid=5, cpv=CPV, shape=RAW, classes=V, seed=8)
    with pytest.raises(Exception, match="GraphEngine"):
        run_task.main(write_two_stream_cfg(folder, "ts.yml", rpath, fpath, "train"), seed=3)


@pytest.mark.parametrize("math", ["f32", "bf16"])
def test_run_task_with_step_graph_equals_eager(tmp_path, monkeypatch, math):
    """Two epochs of the workflow (lr decay, Adam, batches uploaded ahead by the feeder's thread while the step is captured) with
    VLTF_STEP_GRAPH=1 and 0: the final checkpoints hold the same arrays.  Center crops (det): random crops come from an unseeded
    generator, as in the reference."""
    from tests.test_host_workflow import make_dataset
    from tests.test_run_task_gpu import write_cfg
    from vltf_amd import run_task
    monkeypatch.setenv("VLTF_CONV_MATH", math)
    folder = str(tmp_path)
    train_path, _, _ = make_dataset(folder, "train.txt", shape=RAW, seed=1)
    final = {}
    for sg in ("0", "1"):
        monkeypatch.setenv("VLTF_STEP_GRAPH", sg)
        run_task.main(write_cfg(folder, "train%s.yml" % sg, train_path, "train", epochs=2, optimizer="adam", det=True,
                                     run="run" + sg), seed=3)
        ck = sorted(glob.glob(os.path.join(folder, "run" + sg, "checkpoints", "*.weights.npz")), key=os.path.getmtime)
        with np.load(ck[-1], allow_pickle=False) as z:
            final[sg] = {k: z[k] for k in z.files}
    assert sorted(final["0"]) == sorted(final["1"])
    for k in final["0"]:
        assert np.array_equal(final["0"][k], final["1"][k]), k


@pytest.mark.parametrize("math,fpc", [("f32", 16), ("bf16", 32)])
def test_full_geometry(math, fpc):
    """8 clips at 227 x 227 (fp32 x 16 frames; the bf16 path x 32 frames = BASELINE config 5's per-rank job), hidden 256, 101
    classes: the warm-up step and 3 replays equal eager."""
    eager, graph = pair(8, math=math, fpc=fpc, shape=(227, 227, 3), ncls=101, hid=256)
    rng = np.random.default_rng(16)
    for step in range(4):
        train_both((eager, graph), batch(rng, 8, fpc, raw=(240, 320, 3), shape=(227, 227, 3), ncls=101), lr=1e-3 * (step + 1),
                   clip_norm=10.0)
    same_state(eager, graph)
