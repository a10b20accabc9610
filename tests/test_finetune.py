"""Fine-tuning on the host: the `lr_mult` / `train_from` settings and the plan they give -- the learning-rate tiers of the flat
parameter buffer, the frozen variables and the chunks of the data-parallel exchange.  No GPU: no engine is constructed."""
import numpy as np
import pytest
import yaml

from tests.test_host_workflow import config, make_dataset
from vltf_amd import settings_
from vltf_amd._ffi import VltfError

TOTAL, HEAD_END, FC6_END = 44570341, 4483429, 42236261       # the default model: all, head + LSTM, .. + fc6 (conv5..conv1 follow)


def _settings(tmp_path, train=None, pipeline=None):
    folder = str(tmp_path)
    data_path, _, _ = make_dataset(folder, "train.txt")
    path = config(folder, data_path)
    with open(path) as f:
        cfg = yaml.safe_load(f)
    cfg["run"]["train"].update(train or {})
    cfg["run"]["network"]["pipelines"][0]["lrcn"].update(pipeline or {})
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    s = settings_.Settings()
    s.initialize(path)
    return s


# ---- settings ------------------------------------------------------------------------------------------------------------------
def test_settings_lr_mult_parses(tmp_path):
    s = _settings(tmp_path, train={"lr_mult": 10})
    assert s.train.lr_mult == 10.0 and isinstance(s.train.lr_mult, float)
    assert s.pipelines["lrcn"].train_from is None


@pytest.mark.parametrize("bad", [0, -2.5, "nan"])
def test_settings_lr_mult_refused(tmp_path, bad):
    with pytest.raises(Exception, match="lr_mult"):
        _settings(tmp_path, train={"lr_mult": bad})


def test_settings_train_from_parses(tmp_path):
    s = _settings(tmp_path, pipeline={"train_from": "fc6"})
    assert s.pipelines["lrcn"].train_from == "fc6" and s.train.lr_mult is None


@pytest.mark.parametrize("pipeline,msg", [
    ({"train_from": "conv6"}, "not one of"),                                   # no such layer anywhere
    ({"train_from": "fc7"}, "no such layer"),                                            # frame_encoding_layer fc6: the tower ends there
    ({"train_from": "fc6", "representation": "defs.representation.nop"}, "representation"),
])
def test_settings_train_from_refused(tmp_path, pipeline, msg):
    with pytest.raises(Exception, match=msg):
        _settings(tmp_path, pipeline=pipeline)


# ---- the plan of the default model ---------------------------------------------------------------------------------------------
def parent_chunks(cfg):
    """The exchange chunks as LRCNEngine computed them before there was a plan, restated from param_specs."""
    from vltf_amd.engine import FC_DIM, param_specs
    specs = param_specs(cfg)
    offsets, off = {}, 0
    for name, shp in specs:
        offsets[name] = (off, int(np.prod(shp)))
        off += int(np.prod(shp))
    total = off
    first_conv = offsets["dcnn/conv5W"][0]
    f6o, _ = offsets["dcnn/fc6W"]
    rows6 = specs[[n for n, _ in specs].index("dcnn/fc6W")][1][0]
    nch = max(1, min(4, rows6 // 128))
    edges = [(-(-rows6 * i // nch) + 127) // 128 * 128 if 0 < i < nch else (0 if i == 0 else rows6) for i in range(nch + 1)]
    blocks = [(edges[i], edges[i + 1]) for i in range(nch) if edges[i + 1] > edges[i]]
    chunks = [(0, f6o)] if f6o > 0 else []
    for bi, (r0, r1) in enumerate(blocks):
        lo, hi = f6o + r0 * FC_DIM, f6o + r1 * FC_DIM
        if bi == len(blocks) - 1:
            hi = first_conv
        chunks.append((lo, hi - lo))
    conv_lo = offsets["dcnn/conv2W"][0]
    chunks.append((first_conv, conv_lo - first_conv))
    chunks.append((conv_lo, total - conv_lo))
    return chunks


def check_cover(plan):
    """The chunks are disjoint, lie inside trainable ranges and cover them."""
    spans = []
    for lo, hi, _ in plan.tiers:                    # trainable ranges = the tiers with touching neighbours joined
        if spans and spans[-1][1] == lo:
            spans[-1] = (spans[-1][0], hi)
        else:
            spans.append((lo, hi))
    covered = []
    for lo, cnt in plan.chunks:
        assert cnt > 0 and any(a <= lo and lo + cnt <= b for a, b in spans), (lo, cnt)
        covered.append((lo, lo + cnt))
    covered.sort()
    assert all(covered[i][1] <= covered[i + 1][0] for i in range(len(covered) - 1))
    assert sum(b - a for a, b in covered) == sum(b - a for a, b in spans)
    assert all(plan.tiers[i][1] <= plan.tiers[i + 1][0] for i in range(len(plan.tiers) - 1))


CONV_VARS = {"dcnn/conv%d%s" % (i, k) for i in range(1, 6) for k in "Wb"}


def test_plan_lr_mult():
    from vltf_amd.engine import NetConfig, finetune_plan
    plan = finetune_plan(NetConfig(lr_mult=4))
    assert plan.tiers == [(0, HEAD_END, 4.0), (HEAD_END, TOTAL, 1.0)] and plan.frozen == [] and not plan.full_range()
    assert plan.chunks == parent_chunks(NetConfig())
    check_cover(plan)


def test_plan_train_from_fc6():
    from vltf_amd.engine import NetConfig, finetune_plan
    plan = finetune_plan(NetConfig(train_from="fc6"))
    assert plan.tiers == [(0, FC6_END, 1.0)] and set(plan.frozen) == CONV_VARS and len(plan.frozen) == 10
    assert plan.chunks == parent_chunks(NetConfig())[:5]                 # today's boundaries wherever the range still exists
    assert plan.trainable_bytes() == 4 * FC6_END
    check_cover(plan)
    plan = finetune_plan(NetConfig(train_from="fc6", lr_mult=4))
    assert plan.tiers == [(0, HEAD_END, 4.0), (HEAD_END, FC6_END, 1.0)]
    check_cover(plan)


def test_plan_train_from_conv3_cuts_a_chunk():
    from vltf_amd.engine import NetConfig, finetune_plan
    plan = finetune_plan(NetConfig(train_from="conv3"))
    base = parent_chunks(NetConfig())
    assert set(plan.frozen) == {"dcnn/conv1W", "dcnn/conv1b", "dcnn/conv2W", "dcnn/conv2b"}
    assert plan.chunks == base[:6] and plan.tiers == [(0, base[6][0], 1.0)]
    check_cover(plan)
    plan = finetune_plan(NetConfig(train_from="conv5"))                  # the conv5..conv3 chunk survives in part
    assert plan.chunks[:5] == base[:5] and len(plan.chunks) == 6 and plan.chunks[5][0] == base[5][0] and plan.chunks[5][1] < base[5][1]
    check_cover(plan)


@pytest.mark.parametrize("m", [None, 0.5])
def test_plan_classifier(m):
    from vltf_amd.engine import NetConfig, finetune_plan
    plan = finetune_plan(NetConfig(train_from="classifier", lr_mult=m))
    assert plan.tiers == [(0, HEAD_END, 1.0 if m is None else m)]
    assert plan.chunks == [(0, HEAD_END)] and plan.trainable_bytes() == 4 * HEAD_END
    assert set(plan.frozen) == CONV_VARS | {"dcnn/fc6W", "dcnn/fc6b"}
    check_cover(plan)


@pytest.mark.parametrize("kw", [dict(), dict(lr_mult=1.0), dict(frame_encoding_layer="fc8", classifier="fc", num_classes=11),
                                dict(frame_encoding_layer="fc7", lstm_layers=2, image_shape=(67, 67, 3))])
def test_plan_nothing_set_is_the_parent(kw):
    from vltf_amd.engine import NetConfig, finetune_plan, param_specs
    cfg = NetConfig(**kw)
    plan = finetune_plan(cfg)
    total = sum(int(np.prod(s)) for _, s in param_specs(cfg))
    assert plan.tiers == [(0, total, 1.0)] and plan.full_range() and plan.frozen == [] and plan.total == total
    assert plan.chunks == parent_chunks(cfg)
    check_cover(plan)


def test_plan_tiers_with_fc8():
    """fc8 is re-initialised (alexnet.py:273,280): it learns with the modified variables although it is a dcnn layer."""
    from vltf_amd.engine import NetConfig, finetune_plan, is_regular, param_specs
    cfg = NetConfig(frame_encoding_layer="fc8", lr_mult=3, train_from="fc7")
    plan = finetune_plan(cfg)
    specs = param_specs(cfg)
    sizes = {n: int(np.prod(s)) for n, s in specs}
    head = sum(sizes[n] for n, _ in specs if not is_regular(n))
    assert [n for n, _ in specs if not is_regular(n)][-2:] == ["dcnn/fc8W", "dcnn/fc8b"]
    fc7 = sizes["dcnn/fc7W"] + sizes["dcnn/fc7b"]
    assert plan.tiers == [(0, head, 3.0), (head, head + fc7, 1.0)]
    assert set(plan.frozen) == CONV_VARS | {"dcnn/fc6W", "dcnn/fc6b"}
    check_cover(plan)
    assert is_regular("rgb/dcnn/conv1W") and not is_regular("rgb/dcnn/fc8b") and not is_regular("dcnn/output_fc_w")
    assert not is_regular("rnn/multi_rnn_cell/cell_0/basic_lstm_cell/kernel") and not is_regular("fuse/fc_convert_w")


def test_plan_refusals():
    from vltf_amd.engine import NetConfig, finetune_plan
    with pytest.raises(VltfError, match="no such layer"):
        finetune_plan(NetConfig(train_from="fc7"))                       # frame_encoding_layer fc6
    with pytest.raises(VltfError, match="train_from"):
        finetune_plan(NetConfig(train_from="pool5"))
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(VltfError, match="lr_mult"):
            finetune_plan(NetConfig(lr_mult=bad))


# ---- GraphEngine's plan (the host path graph.model_specs uses) -----------------------------------------------------------------
def graph_plan(pipes, data, V, lr_mult=None):
    import torch
    from vltf_amd.graph import DatasetInfo, GraphEngine, PipelineSpec
    eng = object.__new__(GraphEngine)
    eng.dev, eng.training, eng.dp = torch.device("cpu"), False, None
    ds = {t: DatasetInfo("video", 3, 1, 2, image_shape=(67, 67, 3)) for t in data}
    eng._plan([PipelineSpec(name=n, **kw) for n, kw in pipes], ds, V, lr_mult=lr_mult)
    return eng


def test_graph_plan_two_towers():
    pipes = [("rgb", dict(input=["main"], representation="dcnn", frame_encoding_layer="fc6", train_from="classifier")),
             ("flow", dict(input=["aux"], representation="dcnn", frame_encoding_layer="fc7", train_from="conv3")),
             ("fuse", dict(input=["rgb", "flow"], input_fusion="avg", representation="nop", classifier="lstm", lstm_params=(6, 1, "avg")))]
    eng = graph_plan(pipes, ["main", "aux"], 7, lr_mult=2.0)
    plan, specs = eng.plan, eng.specs
    off, offs = 0, {}
    for n, s in specs:
        offs[n] = (off, off + int(np.prod(s)))
        off += int(np.prod(s))
    rgb = [n for n, _ in specs if n.startswith("rgb/")]
    assert set(plan.frozen) == set(rgb) | {"flow/dcnn/conv1W", "flow/dcnn/conv1b", "flow/dcnn/conv2W", "flow/dcnn/conv2b"}
    # flat order: fuse's head, flow's tower (fc7, fc6, conv5..conv1), rgb's tower
    assert plan.tiers == [(0, offs["flow/dcnn/fc7W"][0], 2.0), (offs["flow/dcnn/fc7W"][0], offs["flow/dcnn/conv2W"][0], 1.0)]
    assert plan.chunks[0] == (0, offs["flow/dcnn/fc7W"][0]) and sum(plan.chunks[-1]) == offs["flow/dcnn/conv2W"][0]
    check_cover(plan)
    assert not eng.by_name["rgb"].tower_trains and eng.by_name["flow"].tower_trains
    unfrozen = graph_plan([(n, {k: v for k, v in kw.items() if k != "train_from"}) for n, kw in pipes], ["main", "aux"], 7)
    assert unfrozen.plan.full_range() and unfrozen.plan.frozen == [] and unfrozen.specs == specs
    check_cover(unfrozen.plan)


def test_graph_plan_refusals():
    tower = dict(input=["main"], representation="dcnn", frame_encoding_layer="fc8")
    # nine towers, each [fc8: lr_mult] [fc7 .. : 1] -> 18 tiers and the head's
    pipes = [("t%d" % i, dict(tower)) for i in range(9)]
    pipes.append(("out", dict(input=["t%d" % i for i in range(9)], input_fusion="avg", representation="nop", classifier="fc")))
    with pytest.raises(VltfError, match="tiers"):
        graph_plan(pipes, ["main"], 7, lr_mult=2.0)
    assert len(graph_plan(pipes, ["main"], 7).plan.tiers) == 1
    with pytest.raises(VltfError, match="train_from"):
        graph_plan([("a", dict(input=["main"], representation="dcnn", frame_encoding_layer="fc6", classifier=None)),
                    ("b", dict(input=["a"], representation="nop", classifier="fc", train_from="fc6"))], ["main"], 7)
    with pytest.raises(VltfError, match="nothing to train"):
        graph_plan([("a", dict(input=["main"], representation="dcnn", frame_encoding_layer="fc8", classifier="fc",
                               train_from="classifier"))], ["main"], 7)


def test_tier_table_abi():
    """The ctypes view of vl_lr_tier has the header's layout (two int64, a float, padded to 24 bytes) and its limit."""
    import ctypes
    import os
    import re
    from vltf_amd import _ffi
    assert ctypes.sizeof(_ffi.LrTier) == 24 and _ffi.LrTier.lr_mult.offset == 16
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vltf.h")).read()
    assert int(re.search(r"#define VL_MAX_LR_TIERS (\d+)", src).group(1)) == _ffi.MAX_LR_TIERS == 16
    for name in ("vl_sgd_apply_tiers", "vl_adam_apply_tiers", "vl_sgd_apply_tiers_st", "vl_adam_apply_tiers_st", "vl_sumsq_tiers"):
        assert name in _ffi.SIGNATURES


def test_graph_frozen_tower_on_the_cpu_double(monkeypatch):
    """GraphEngine's host logic with one tower frozen whole, on the torch-CPU stand-in of the kernels (tests/cpu_double.py) with the
    tiered norm / update restated here: the frozen tower's backward is never called, the gradient it would be handed is not computed,
    its range of g is never written, and the step is the oracle's restricted to the trainable variables, the head at lr * lr_mult."""
    import dataclasses
    import math
    import torch
    from tests import graph_cases as GC
    from tests.cpu_double import CpuOps, install
    from vltf_amd import graph
    from vltf_amd.engine import is_regular
    Engine = install(monkeypatch)

    class TierOps(CpuOps):
        @staticmethod
        def sumsq_tiers(g, tiers, out, ws):
            out[0] = sum(float((g[lo:hi].double() ** 2).sum()) for lo, hi, _ in tiers)

        @staticmethod
        def sgd_apply_tiers(w, g, tiers, lr, clip_norm=0.0, sumsq_t=None, gscale=1.0, skip=None):
            for lo, hi, m in tiers:
                CpuOps.sgd_apply(w[lo:hi], g[lo:hi], lr * m, clip_norm, sumsq_t, gscale, skip)

    monkeypatch.setattr(graph, "ops", TierOps)
    case = GC.CASES["two_stream_avg"]()
    pipes, ds = GC.specs_and_datasets(case)
    pipes = [dataclasses.replace(sp, train_from="classifier" if sp.name == "rgb" else None) for sp in pipes]
    eng = Engine(pipes, ds, case["V"], device="cpu", lr_mult=4.0)
    p = eng.init_params(seed=case["seed"], well_scaled=True)
    eng.load_params(p)
    raw, feeds = GC.inputs(case)
    logits, onehot, loss, grads, _ = GC.expect(case, p, feeds)
    frozen = set(eng.plan.frozen)
    assert frozen == {k for k in p if k.startswith("rgb/")} and len(eng.plan.tiers) == 2
    for k in frozen:
        eng.G[k].fill_(float("nan"))
    rgb = eng.by_name["rgb"]
    assert not rgb.wants_feat and eng.by_name["flow"].wants_feat
    rgb.tower._backward = lambda n, b: pytest.fail("the frozen tower's backward was called")
    dev_feeds = {t: dict(frames_u8=torch.from_numpy(v), mean_bgr=GC.MEAN) for t, v in raw.items()}
    out = eng.train_step(dev_feeds, torch.from_numpy(onehot), lr=0.01, clip_norm=0.5)
    trainable = [k for k in p if k not in frozen]
    gn = math.sqrt(sum(float((grads[k].astype(np.float64) ** 2).sum()) for k in trainable))
    assert abs(out["loss"] - loss) < 1e-4 * max(1, abs(loss)) and abs(out["grad_norm"] - gn) < 1e-3 * gn
    g = eng.get_grads()
    assert sorted(g) == sorted(trainable)
    for k in trainable:
        np.testing.assert_allclose(g[k], grads[k], rtol=2e-3, atol=2e-4 * (np.abs(grads[k]).max() + 1e-12), err_msg="grad " + k)
    newp = eng.get_params()
    for k in p:
        if k in frozen:
            assert np.array_equal(newp[k], p[k]) and bool(torch.isnan(eng.G[k]).all()), k
        else:
            want = p[k].astype(np.float64) - 0.01 * (1.0 if is_regular(k) else 4.0) * 0.5 / max(gn, 0.5) * grads[k]
            np.testing.assert_allclose(newp[k], want, rtol=1e-4, atol=1e-5, err_msg="param " + k)
