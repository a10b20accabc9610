"""Dropout on relu(fc6) / relu(fc7) of the AlexNet tower on the device (NetConfig.fc_dropout_keep_prob).

The mask is a function of (seed, salt, element) with a numpy restatement (tests/fc_dropout_ref.py): the launches must equal it
EXACTLY, so nothing here is statistical.  The engines are held against a torch fp64 model with the restated masks behind relu(fc6) /
relu(fc7), at the shapes and tolerances of tests/test_engine_gpu.py::test_train_step_small -- and, so that no parity check passes
with the option silently off, every engine test also looks at the zero pattern the step left in f6."""
import numpy as np
import pytest
import torch

from oracle import lrcn_oracle as O
from oracle import torch_cpu as TC
from tests import fc_dropout_ref as R
from tests import graph_cases as GC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN = np.array([99.197148, 105.293620, 109.503945], np.float32)
KEEP = 0.5


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def positive(rng, count):
    """ReLU-active values: a kept element is never 0, so the zeros of the output are the mask's."""
    return (np.abs(rng.standard_normal(count)) + 0.1).astype(np.float32)


def check_forward(got, x, mask, keep):
    assert np.array_equal(got == 0, ~mask)                                       # zeros exactly where dropped
    np.testing.assert_allclose(got[mask], x[mask] / np.float32(keep), rtol=1e-6, atol=0)        # one division's rounding


# ---- A. the launches against the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [0.25, 0.5, 0.9])
@pytest.mark.parametrize("count", [1, 3, 4, 5, 1023, 3 * 4096 + 1])
def test_forward_equals_the_restatement(count, keep):
    from vltf_amd import ops
    from vltf_amd.engine import dropout_seed
    rng = np.random.default_rng(count)
    x = positive(rng, count)
    y = torch.from_numpy(x).to(DEV)
    seed, salt = dropout_seed(7), 3
    ops.fc_dropout_fwd(y, keep, seed, salt)
    check_forward(host(y), x, R.keep_mask(seed, salt, count, keep), keep)


@pytest.mark.parametrize("keep", [0.25, 0.5, 0.9])
def test_forward_on_a_view_one_float_past_an_aligned_base(keep):
    """The element index is relative to the pointer given, whatever its alignment; nothing outside the view is touched."""
    from vltf_amd import ops
    from vltf_amd.engine import dropout_seed
    rng = np.random.default_rng(3)
    x = positive(rng, 16)
    base = torch.from_numpy(x).to(DEV)
    assert base.data_ptr() % 16 == 0
    view = base[1:10]
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    ops.fc_dropout_fwd(view, keep, dropout_seed(2), 1)
    got = host(base)
    check_forward(got[1:10], x[1:10], R.keep_mask(dropout_seed(2), 1, 9, keep), keep)
    assert np.array_equal(got[:1], x[:1]) and np.array_equal(got[10:], x[10:])


def test_forward_past_one_pass_of_the_grid():
    """ops.FC_DROPOUT_GRID_SPAN = 4 elements a lane x 256 lanes x the launch's grid cap of 4096 work-groups: what one pass of the
    grid-stride loop covers.  5 more elements: the first lanes take a second pass and one element is left for the scalar tail."""
    from vltf_amd import ops
    from vltf_amd.engine import dropout_seed
    count = ops.FC_DROPOUT_GRID_SPAN + 5
    assert count == 4 * 256 * 4096 + 5
    x = positive(np.random.default_rng(1), count)
    y = torch.from_numpy(x).to(DEV)
    ops.fc_dropout_fwd(y, 0.5, dropout_seed(0), 0)
    check_forward(host(y), x, R.keep_mask(dropout_seed(0), 0, count, 0.5), 0.5)


@pytest.mark.parametrize("step", [0, 1, 2 ** 20 + 3])
def test_state_form_equals_the_eager_call_with_the_engine_seed(step):
    from vltf_amd import ops
    from vltf_amd.engine import dropout_seed
    count = 4099
    x = positive(np.random.default_rng(8), count)
    eager, again, st = (torch.from_numpy(x).to(DEV) for _ in range(3))
    state = ops.step_state(DEV)
    ops.step_state_set(state, step, 0.01, 1)
    ops.fc_dropout_fwd_st(st, 0.5, state, 5)
    ops.fc_dropout_fwd(eager, 0.5, dropout_seed(step), 5)
    ops.fc_dropout_fwd(again, 0.5, dropout_seed(step), 5)
    assert torch.equal(eager.view(torch.int32), st.view(torch.int32))
    assert torch.equal(eager.view(torch.int32), again.view(torch.int32))          # the same arguments: the same bits
    check_forward(host(st), x, R.keep_mask(dropout_seed(step), 5, count, 0.5), 0.5)


@pytest.mark.parametrize("od,oy", [(0, 0), (1, 1), (1, 2)], ids=["aligned", "offset1", "phases-disagree"])
@pytest.mark.parametrize("count", [5, 4099])
def test_gradient_against_numpy(count, od, oy):
    from vltf_amd import ops
    rng = np.random.default_rng(count + od)
    y = np.maximum(rng.standard_normal(count + oy), 0).astype(np.float32)          # zeros and positives
    d = rng.standard_normal(count + od).astype(np.float32)
    y[oy], y[oy + 1] = 0.0, 1.5
    yd, dd = torch.from_numpy(y).to(DEV), torch.from_numpy(d).to(DEV)
    ops.relu_dropout_grad(dd[od:], yd[oy:], 0.25)
    got = host(dd)
    want = np.where(y[oy:] > 0, d[od:] / np.float32(0.25), np.float32(0))
    assert np.array_equal(got[od:] == 0, want == 0)
    np.testing.assert_allclose(got[od:], want, rtol=1e-6, atol=0)
    assert np.array_equal(got[:od], d[:od])


def test_bad_arguments_are_refused():
    from vltf_amd import ops
    from vltf_amd._ffi import VltfError
    y, d = torch.ones(8, device=DEV), torch.ones(8, device=DEV)
    state = ops.step_state(DEV)
    for keep in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(VltfError, match="vl_fc_dropout_fwd: bad argument"):
            ops.fc_dropout_fwd(y, keep, 1, 0)
        with pytest.raises(VltfError, match="vl_fc_dropout_fwd_st: bad argument"):
            ops.fc_dropout_fwd_st(y, keep, state, 0)
        with pytest.raises(VltfError, match="vl_relu_dropout_grad: bad argument"):
            ops.relu_dropout_grad(d, y, keep)
    with pytest.raises(VltfError):
        ops.fc_dropout_fwd(y[:0], 0.5, 1, 0)
    assert torch.equal(y, torch.ones(8, device=DEV)) and torch.equal(d, torch.ones(8, device=DEV))


# ---- B. LRCNEngine against the masked fp64 model ----------------------------------------------------------------------------------
SHAPE, NCLS, FPC, B = (67, 67, 3), 7, 3, 2
N = B * FPC
LR, CLIP = 0.01, 0.5
CASES = {
    "fc6-lstm-avg": dict(frame_encoding_layer="fc6", lstm_hidden=8, lstm_layers=1, fusion="avg"),
    "fc7-lstm2-last": dict(frame_encoding_layer="fc7", lstm_hidden=12, lstm_layers=2, fusion="last"),
    "fc8-lstm-avg": dict(frame_encoding_layer="fc8", lstm_hidden=7, lstm_layers=1, fusion="avg"),
    "fc7-fc-early-avg": dict(frame_encoding_layer="fc7", classifier="fc", frame_fusion=("early", "avg")),
    "fc6-fc-none": dict(frame_encoding_layer="fc6", classifier="fc", frame_fusion=None),
}
# train_from fc7: fc6 (and the conv stack) frozen under a trained fc7
OTHER_CASES = {"fc7-lstm-avg-frozen": dict(frame_encoding_layer="fc7", lstm_hidden=8, lstm_layers=1, fusion="avg", train_from="fc7")}
_DATA, _REF = {}, {}


def config(name, **kw):
    from vltf_amd.engine import NetConfig
    return NetConfig(image_shape=SHAPE, num_classes=NCLS, fpc=FPC, dropout_keep_prob=0, **{**CASES.get(name, OTHER_CASES.get(name)), **kw})


def data(name):
    """Parameters, frames and labels of a case, made once and never written."""
    if name not in _DATA:
        cfg = config(name)
        rng = np.random.default_rng(5)
        p = O.init_params(rng, NCLS, cfg.frame_encoding_layer, cfg.lstm_hidden, cfg.lstm_layers, SHAPE, classifier=cfg.classifier,
                          well_scaled=True, fusion=cfg.fusion)
        frames = rng.integers(0, 256, (N,) + SHAPE, dtype=np.uint8)
        rows = N if (cfg.classifier == "fc" and not cfg.frame_fusion) else B
        onehot = O.labels_to_one_hot([[l] for l in rng.integers(0, NCLS, rows)], NCLS)
        _DATA[name] = (p, frames, onehot)
    return _DATA[name]


def masks_at(cfg, draw):
    return {l: R.engine_mask(cfg, l, draw, N, KEEP) for l in ("fc6", "fc7")}


def reference(name, draw=0, params=None, frozen=()):
    """The masked fp64 step of a case at a draw index: (new params, loss, grad norm, logits, grads); computed once per key when it
    starts from the case's own parameters."""
    key = (name, draw, tuple(frozen))
    if params is None and key in _REF:
        return _REF[key]
    p, frames, onehot = data(name)
    cfg = config(name, fc_dropout_keep_prob=KEEP)
    x = torch.from_numpy(frames.astype(np.float32) - MEAN).double()
    masks = masks_at(cfg, draw)
    out = R.sgd_step(params or p, lambda q: R.masked_logits(
        q, x, FPC, KEEP, masks, final_layer=cfg.frame_encoding_layer, lstm_layers=cfg.lstm_layers, fusion=cfg.fusion,
        classifier=cfg.classifier, frame_fusion=cfg.frame_fusion, num_classes=NCLS), onehot, LR, CLIP, frozen)
    if params is None:
        _REF[key] = out
    return out


def engine(name, **kw):
    from vltf_amd.engine import LRCNEngine
    eng = LRCNEngine(config(name, **kw), max_clips=B, device=DEV)
    eng.load_params(data(name)[0])
    return eng


def step(eng, name, **kw):
    _, frames, onehot = data(name)
    return eng.train_step_u8(torch.tensor(frames, device=DEV), torch.tensor(onehot, device=DEV), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, **kw)


def follows(f, mask):
    """The zero pattern of a dropped ReLU output: 0 wherever the mask drops, and alive somewhere it keeps."""
    f = host(f)
    return not f[~mask].any() and f[mask].any()


def close_step(eng, out, ref, names=None):
    """Loss, norm, gradients and updated parameters at the tolerances of test_train_step_small."""
    newp, loss, gn, _, grads = ref
    assert abs(out["loss"] - loss) < 1e-4 * max(1, abs(loss)), (out["loss"], loss)
    assert abs(out["grad_norm"] - gn) < 1e-3 * gn, (out["grad_norm"], gn)
    g = eng.get_grads()
    assert set(g) == set(grads)
    for k in grads:
        scale = np.abs(grads[k]).max() + 1e-12
        np.testing.assert_allclose(g[k], grads[k], rtol=2e-3, atol=2e-4 * scale, err_msg="grad " + k)
    got = eng.get_params()
    for k in newp:
        np.testing.assert_allclose(got[k], newp[k], rtol=1e-4, atol=1e-5, err_msg="param " + k)


@pytest.mark.parametrize("name", sorted(CASES))
def test_engine_step_matches_the_masked_model(name):
    eng, plain = engine(name, fc_dropout_keep_prob=KEEP), engine(name)
    fd = torch.tensor(data(name)[1], device=DEV)
    fwd = eng.forward_u8(fd, MEAN).clone()
    assert torch.equal(fwd.view(torch.int32), plain.forward_u8(fd, MEAN).view(torch.int32))        # validation never drops
    out = step(eng, name)
    masks = masks_at(eng.cfg, 0)
    assert follows(eng.f6[:N], masks["fc6"])
    if eng.f7 is not None:
        assert follows(eng.f7[:N], masks["fc7"]) and not np.array_equal(masks["fc6"], masks["fc7"])
    np.testing.assert_allclose(eng.logits_host(), reference(name)[3], rtol=1e-3, atol=1e-3)
    close_step(eng, out, reference(name))
    plain.load_params(eng.get_params())
    assert torch.equal(eng.forward_u8(fd, MEAN).view(torch.int32), plain.forward_u8(fd, MEAN).view(torch.int32))


def test_keep_one_launches_nothing_and_is_the_plain_step():
    name = "fc6-lstm-avg"
    one, plain = engine(name, fc_dropout_keep_prob=1.0), engine(name)
    assert step(one, name) == step(plain, name)
    assert torch.equal(one.w.view(torch.int32), plain.w.view(torch.int32)) and torch.equal(one.f6.view(torch.int32), plain.f6.view(torch.int32))


def test_second_step_draws_a_new_mask():
    name = "fc6-lstm-avg"
    eng = engine(name, fc_dropout_keep_prob=KEEP)
    step(eng, name)
    first = host(eng.f6[:N]).copy()
    out = step(eng, name)
    m0, m1 = R.engine_mask(eng.cfg, "fc6", 0, N), R.engine_mask(eng.cfg, "fc6", 1, N)
    assert follows(eng.f6[:N], m1) and not follows(eng.f6[:N], m0)
    assert host(eng.f6[:N])[m1 & ~m0].any() and first[m0 & ~m1].any()
    close_step(eng, out, reference(name, draw=1, params=reference(name)[0]))


def test_frozen_fc6_still_drops():
    """train_from fc7: fc6 is frozen and still dropped in a training forward (as Caffe does); fc7's gradients are computed on the
    dropped f6, nothing below fc7 moves."""
    name = "fc7-lstm-avg-frozen"
    eng = engine(name, fc_dropout_keep_prob=KEEP)
    frozen = sorted(eng.plan.frozen)
    assert "dcnn/fc6W" in frozen and "dcnn/conv1W" in frozen and "dcnn/fc7W" not in frozen
    before = {k: eng.P[k].clone() for k in frozen}
    out = step(eng, name)
    masks = masks_at(eng.cfg, 0)
    assert follows(eng.f6[:N], masks["fc6"]) and follows(eng.f7[:N], masks["fc7"])
    close_step(eng, out, reference(name, frozen=frozen))
    for k in frozen:
        assert torch.equal(before[k].view(torch.int32), eng.P[k].view(torch.int32)), k


def test_packed_bf16_path():
    """conv_math bf16: the pattern, and loss / grad norm against the masked model at the bounds of test_plain_bf16_conv_mode_runs_close."""
    name = "fc6-lstm-avg"
    eng = engine(name, fc_dropout_keep_prob=KEEP, conv_math="bf16")
    out = step(eng, name)
    assert follows(eng.f6[:N], R.engine_mask(eng.cfg, "fc6", 0, N))
    _, loss, gn, _, _ = reference(name)
    print("bf16 path: loss %.6f (masked model %.6f), grad norm %.6f (%.6f)" % (out["loss"], loss, out["grad_norm"], gn))
    assert abs(out["loss"] - loss) < 1e-2 * max(1, abs(loss)) and abs(out["grad_norm"] - gn) < 5e-2 * gn


# ---- C. captured steps and accumulation: bitwise the eager engine, fresh masks on every replay ------------------------------------
@pytest.mark.parametrize("math", ["f32", "bf16"])
def test_captured_step_equals_eager_and_redraws(math):
    """step_graph with both dropouts at 0.5, 2 clips x 4 frames (8 frames: the bf16 path's packed-operand fc6): warm-up, capture, two
    replays.  Every step leaves the eager engine's f6 and results, bit for bit; the two replays' zero patterns are those of draw
    indices 2 and 3."""
    from tests.test_step_graph_gpu import batch, pair, same_state, train_both
    eager, graph = pair(2, math=math, fc_dropout_keep_prob=KEEP)
    rng = np.random.default_rng(21)
    patterns = []
    for i in range(4):
        train_both((eager, graph), batch(rng, 2, 4), lr=0.01 * 0.7 ** i)
        assert torch.equal(eager.f6.view(torch.int32), graph.f6.view(torch.int32))
        assert follows(graph.f6[:8], R.engine_mask(graph.cfg, "fc6", i, 8))
        patterns.append(host(graph.f6[:8]) != 0)
    assert len(graph._graphs) == 1
    assert not np.array_equal(patterns[2], patterns[3])
    same_state(eager, graph)


def test_accumulated_update_draws_per_micro_step():
    """accumulate 2, eager and captured (fp32): micro-step i of update u drops by draw index 2 u + i; the engines end bitwise equal."""
    from tests.test_step_graph_gpu import batch, pair, same_state
    eager, graph = pair(2, fpc=FPC, hid=8, accumulate=2, fc_dropout_keep_prob=KEEP)
    rng = np.random.default_rng(13)
    for upd in range(4):
        for i in range(2):
            bt = batch(rng, 2, FPC)
            outs = [e.train_step_u8(bt["frames_u8"], bt["onehot"], 0.01 * 0.7 ** upd, 5.0, MEAN, bt["crop_y"], bt["crop_x"], bt["mirror"],
                                    micro=(i, 2)) for e in (eager, graph)]
            assert outs[0] == outs[1], (upd, i, outs)
            mask = R.engine_mask(graph.cfg, "fc6", 2 * upd + i, N)
            assert follows(eager.f6[:N], mask) and follows(graph.f6[:N], mask)
            assert torch.equal(eager.f6.view(torch.int32), graph.f6.view(torch.int32))
        assert torch.equal(eager.g.view(torch.int32), graph.g.view(torch.int32))
        same_state(eager, graph)
    assert len(graph._graphs) == 2 and eager.step_count == 4


# ---- D. GraphEngine: each tower under its own salt -------------------------------------------------------------------------------------
def test_graph_engine_two_towers(monkeypatch):
    from vltf_amd.graph import GraphEngine
    case = GC.CASES["two_stream_avg"]()
    pipes, ds = GC.specs_and_datasets(case)
    eng = GraphEngine(pipes, ds, case["V"], device=DEV, fc_dropout_keep_prob=KEEP)
    p = eng.init_params(seed=case["seed"], well_scaled=True)
    eng.load_params(p)
    raw, feeds = GC.inputs(case)
    rows = case["items"]
    n = rows * case["data"]["main"]["fpc"]
    onehot = O.labels_to_one_hot([[l] for l in np.random.default_rng(0).integers(0, case["V"], rows)], case["V"])
    towers = {nd.scope: nd for nd in eng.nodes if nd.tower is not None}
    assert sorted(towers) == ["flow/", "rgb/"]
    masks = {sc: {"fc6": R.engine_mask(nd.tower_cfg, "fc6", 0, n, KEEP)} for sc, nd in towers.items()}
    assert not np.array_equal(masks["rgb/"]["fc6"], masks["flow/"]["fc6"])

    def masked(q, scope, frames, final_layer):
        return R.masked_dcnn_features(q, scope, frames, final_layer, KEEP, masks[scope])
    monkeypatch.setattr(TC, "dcnn_features", masked)
    dsets = {t: dict(cpv=d["cpv"], fpc=d["fpc"]) for t, d in case["data"].items()}
    tfeeds = {t: torch.from_numpy(v).double() for t, v in feeds.items()}
    newp, loss, gn, logits, grads = R.sgd_step(p, lambda q: TC.model_logits(q, case["pipes"], dsets, tfeeds, case["V"]), onehot, 0.01, 0.5)

    fd = {t: dict(frames_u8=torch.from_numpy(v).to(DEV), mean_bgr=GC.MEAN) for t, v in raw.items()}
    out = eng.train_step(fd, torch.from_numpy(onehot).to(DEV), lr=0.01, clip_norm=0.5)
    for sc, nd in towers.items():
        assert follows(nd.tower.f6[:n], masks[sc]["fc6"]), sc
    assert not follows(towers["rgb/"].tower.f6[:n], masks["flow/"]["fc6"])
    np.testing.assert_allclose(eng.logits_host(), logits, rtol=1e-3, atol=1e-3)
    assert abs(out["loss"] - loss) < 1e-4 * max(1, abs(loss))
    assert abs(out["grad_norm"] - gn) < 1e-3 * gn
    g = eng.get_grads()
    assert set(g) == set(p)
    for k in p:
        scale = np.abs(grads[k]).max() + 1e-12
        np.testing.assert_allclose(g[k], grads[k], rtol=2e-3, atol=2e-4 * scale, err_msg="grad " + k)
    got = eng.get_params()
    for k in p:
        np.testing.assert_allclose(got[k], newp[k], rtol=1e-4, atol=1e-5, err_msg="param " + k)


# ---- E. run_task: the YAML key reaches the engine, eager and captured ------------------------------------------------------------
def test_run_task_with_the_key(tmp_path, monkeypatch):
    """5 videos, batch_size 2, 2 epochs (6 steps), deterministic imgproc: the run with train.fc_dropout_keep_prob ends with other weights
    than the run without it, and the same run under VLTF_STEP_GRAPH=1 (whose full batches are replayed) with exactly its weights."""
    import glob
    import os

    import yaml
    monkeypatch.setenv("VLTF_PREFETCH", "0")
    monkeypatch.setenv("VLTF_CONV_MATH", "f32")
    from tests.test_host_workflow import make_dataset
    from tests.test_run_task_gpu import RAW, write_cfg
    from vltf_amd import run_task
    folder = str(tmp_path)
    train_path, _, _ = make_dataset(folder, "train.txt", shape=RAW, seed=1)

    def final_weights(name, run, keep, graph):
        path = write_cfg(folder, name, train_path, "train", epochs=2, det=True, run=run)
        with open(path) as f:
            c = yaml.safe_load(f)
        c["run"]["train"].update(base_lr=0.01)
        if keep is not None:
            c["run"]["train"].update(fc_dropout_keep_prob=keep)
        with open(path, "w") as f:
            yaml.safe_dump(c, f)
        monkeypatch.setenv("VLTF_STEP_GRAPH", "1" if graph else "0")
        run_task.main(path, seed=3)
        ck = sorted(glob.glob(os.path.join(folder, run, "checkpoints", "*.weights.npz")), key=os.path.getmtime)
        with np.load(ck[-1], allow_pickle=False) as z:
            return {k: z[k] for k in z.files}

    plain = final_weights("p.yml", "runP", None, False)
    drop = final_weights("d.yml", "runD", KEEP, False)
    captured = final_weights("g.yml", "runG", KEEP, True)
    assert int(drop["__optimizer__/step_count"][0]) == 6
    assert not np.array_equal(plain["dcnn/fc6W"], drop["dcnn/fc6W"]) and not np.array_equal(plain["output_fc_w"], drop["output_fc_w"])
    assert sorted(captured) == sorted(drop)
    for k in drop:
        np.testing.assert_array_equal(captured[k], drop[k], err_msg=k)
