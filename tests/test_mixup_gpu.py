"""Mixup on the device (vl_mixup_pairs, vl_softmax_xent_mix, NetConfig.mixup_alpha): the in-place blend against the float64 reference
of tests/mixup_ref.py in fp32 and packed bf16, the mixed-label loss launch in both launch forms, lam = 1 bit for bit the input and
vl_softmax_xent_ls, the device-read weight, whole steps of LRCNEngine (eager, per-frame head, odd clip count, captured, replayed with
another weight, accumulated, the bf16 conv path) against the oracle fed the host-blended frames and mixed labels, and run_task on the
example.

Tolerances.  The fp32 blend is four roundings (1 - lam, two products, one sum), each at most 2^-24 of max(|a|, |b|): the bound is
8 * 2^-24 * max(|a|, |b|), a margin of two.  The bf16 blend adds the final rounding: half a bf16 ulp of the larger of result and exact
value.  The loss launch: the bounds tests/test_label_smoothing_gpu.py holds vl_softmax_xent_ls to (loss 1e-5 * max(1, |loss|), dlogits
rtol 1e-4 with atol 1e-6 of the largest element, hit counts exact).  Whole steps against the fp64 oracle: those it restates from
tests/test_engine_gpu.py::test_train_step_small (loss 1e-4 * max(1, |loss|), gradient norm 1e-3 relative, parameters rtol 1e-4 and atol
1e-5, logits rtol 1e-3 and atol 1e-3)."""
import glob
import os
import re

import numpy as np
import pytest
import torch
import yaml

from oracle import lrcn_oracle as O
from tests import label_smoothing_ref as LS
from tests import mixup_ref as MX
from tests.test_label_smoothing_gpu import B, CLIP, FPC, LR, MEAN, SHAPE, SHAPES, bits, case, data, dev_batch, small_cfg
from tests.test_ops_gpu import close, dev, host

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAMS = (1.0, 0.5, 0.7310586)
EPS32 = 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    import vltf_amd.ops as ops_
    return ops_


_CLIPS = {}


def clips_f32(clips, elems):
    """[clips, elems] N(0, 64), pixel-minus-mean sized; made once per shape, never written."""
    if (clips, elems) not in _CLIPS:
        _CLIPS[(clips, elems)] = (np.random.default_rng(clips * 100003 + elems).standard_normal((clips, elems)) * 64).astype(np.float32)
    return _CLIPS[(clips, elems)]


def pair_scale(x):
    """max(|a|, |b|) per element of every pair."""
    return np.maximum(np.abs(x), np.abs(x[::-1])).astype(np.float64)


# ---- 1. the blend, fp32 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("elems", [3, 256, 257, 5003, 70003])
@pytest.mark.parametrize("clips", [1, 2, 3, 4, 5])
def test_mixup_pairs_f32(ops, clips, elems):
    x = clips_f32(clips, elems)
    n = clips * elems
    for lam in LAMS:
        buf = torch.full((n + 64,), NAN, device=DEV)                    # a NaN canary behind the clips
        buf[:n] = dev(x).view(-1)
        ops.mixup_pairs(buf[:n], clips, lam)
        got = host(buf)
        assert np.isnan(got[n:]).all(), "the canary behind clips * clip_elems was written"
        got = got[:n].reshape(clips, elems)
        want = MX.blend(x, lam)
        err = np.abs(got.astype(np.float64) - want)
        bound = 8 * EPS32 * pair_scale(x)
        print("clips %d elems %d lam %g: worst error / bound %.3f" % (clips, elems, lam, float((err / np.maximum(bound, 1e-300)).max())))
        assert (err <= bound).all()
        if lam == 1.0 or clips == 1:
            assert np.array_equal(got.view(np.int32), x.view(np.int32))                   # every bit of the input
        else:
            assert not np.array_equal(got[0], x[0])
        if clips % 2:
            assert np.array_equal(got[clips // 2].view(np.int32), x[clips // 2].view(np.int32))      # the middle clip: untouched
        # the weight read from the device: the bytes of the host-argument launch
        buf2 = torch.full((n + 64,), NAN, device=DEV)
        buf2[:n] = dev(x).view(-1)
        ops.mixup_pairs(buf2[:n], clips, torch.tensor([lam], device=DEV))
        assert torch.equal(bits(buf2[:n]), bits(buf[:n])) and bool(torch.isnan(buf2[n:]).all())


def test_mixup_pairs_misaligned_base(ops):
    """A base 4 bytes past a 16-byte boundary with whole-vector clips: no pair is aligned, every one goes element by element."""
    clips, elems = 4, 256
    x = clips_f32(clips, elems)
    buf = torch.full((clips * elems + 8,), NAN, device=DEV)
    buf[1:1 + clips * elems] = dev(x).view(-1)
    ops.mixup_pairs(buf[1:1 + clips * elems], clips, 0.7310586)
    got = host(buf)
    assert np.isnan(got[0]) and np.isnan(got[1 + clips * elems:]).all()
    aligned = dev(x).view(-1).clone()
    ops.mixup_pairs(aligned, clips, 0.7310586)
    assert np.array_equal(got[1:1 + clips * elems].view(np.int32), host(aligned).view(np.int32))     # the same bits as the 16-byte loop


def test_mixup_pairs_refusals_launch_nothing(ops):
    from vltf_amd import _ffi
    from vltf_amd._ffi import VltfError
    x = clips_f32(4, 256)
    xd = dev(x).view(-1)
    st = torch.cuda.current_stream().cuda_stream
    for args, msg in (((None, 0, 4, 256, 0.5, None), "x is null"), ((xd.data_ptr(), 0, -1, 256, 0.5, None), "clips must be >= 0"),
                      ((xd.data_ptr(), 0, 4, 0, 0.5, None), "clip_elems must be > 0"), ((xd.data_ptr(), 2, 4, 256, 0.5, None), "dtype must be 0"),
                      ((xd.data_ptr(), 1, 4, 12, 0.5, None), "no multiple of 8"), ((xd.data_ptr(), 0, 4, 256, -0.25, None), "lam must lie"),
                      ((xd.data_ptr(), 0, 4, 256, 1.25, None), "lam must lie"), ((xd.data_ptr(), 0, 4, 256, NAN, None), "lam must lie"),
                      ((xd.data_ptr(), 0, 4, 256, float("inf"), None), "lam must lie")):
        with pytest.raises(VltfError, match=msg):
            _ffi.call("vl_mixup_pairs", *args, st)
    with pytest.raises(VltfError, match="float32 or bfloat16"):
        ops.mixup_pairs(xd.to(torch.float16), 4, 0.5)
    with pytest.raises(VltfError, match="equal clips"):
        ops.mixup_pairs(xd, 3, 0.5)
    with pytest.raises(VltfError, match="one float32"):
        ops.mixup_pairs(xd, 4, torch.zeros(2, device=DEV))
    ops.mixup_pairs(xd, 1, 0.5)                                                           # one clip: nothing to pair, nothing launched
    assert np.array_equal(host(xd).view(np.int32), x.reshape(-1).view(np.int32))


# ---- 2. the blend, packed bf16 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("elems", [8, 264, 70008])
@pytest.mark.parametrize("clips", [2, 3, 5])
def test_mixup_pairs_bf16(ops, clips, elems):
    xb = torch.from_numpy(clips_f32(clips, elems)).to(torch.bfloat16)
    x = xb.to(torch.float64).numpy()
    n = clips * elems
    for lam in LAMS:
        buf = torch.full((n + 64,), NAN, dtype=torch.bfloat16, device=DEV)
        buf[:n] = xb.to(DEV).view(-1)
        ops.mixup_pairs(buf[:n], clips, lam)
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[n:]).all())
        got = buf[:n].to(torch.float64).cpu().numpy().reshape(clips, elems)
        want = MX.blend(x, lam)
        err = np.abs(got - want)
        bound = 0.5 * MX.bf16_ulp(np.maximum(np.abs(got), np.abs(want))) + 8 * EPS32 * pair_scale(x)
        print("clips %d elems %d lam %g: worst error / bound %.3f" % (clips, elems, lam, float((err / bound).max())))
        assert (err <= bound).all()
        if lam == 1.0:
            assert torch.equal(buf[:n].view(torch.int16).cpu(), xb.view(-1).view(torch.int16))
        if clips % 2:
            assert np.array_equal(got[clips // 2], x[clips // 2])
        buf2 = torch.full((n + 64,), NAN, dtype=torch.bfloat16, device=DEV)
        buf2[:n] = xb.to(DEV).view(-1)
        ops.mixup_pairs(buf2[:n], clips, torch.tensor([lam], device=DEV))
        assert torch.equal(buf2[:n].view(torch.int16), buf[:n].view(torch.int16))


def test_mixup_pairs_bf16_refuses_a_clip_that_is_not_whole_blocks(ops):
    from vltf_amd._ffi import VltfError
    x = torch.ones(24, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(VltfError, match="clip_elems 12 is no multiple of 8"):
        ops.mixup_pairs(x, 2, 0.5)
    torch.cuda.synchronize()
    assert bool((x == 1).all())


# ---- 3. the loss launch -----------------------------------------------------------------------------------------------------------------------
def launch(ops, z, onehot, eps, k, rows_ws, rpc, lam):
    """-> (stats[3], dlogits, rows workspace or None) of one ops.softmax_xent_mix; every output buffer holds NaN beforehand but stats."""
    n, c = z.shape
    dl = torch.full((n, c), NAN, device=DEV)
    stats = torch.zeros(3, device=DEV)
    rows = torch.full((3 * n,), NAN, device=DEV) if rows_ws else None
    ops.softmax_xent_mix(dev(z), dev(onehot, torch.int32), dl, stats, 1.0 / n, rows, rpc, eps, k, lam)
    return stats, dl, rows


XENT_CASES = [(b, c, 1) for b, c in SHAPES] + [(4, 64, 2), (6, 1000, 2)]       # (6, 1000, 2): three clips, the middle one its own partner


@pytest.mark.parametrize("b,c,rpc", XENT_CASES)
def test_softmax_xent_mix(ops, b, c, rpc):
    z, onehot = case(b, c)
    for eps in (0.0, 0.1):
        for k in (0, 5):
            for lam in (1.0, 0.5, 0.8):
                want = MX.xent(z, onehot, lam, eps, k, rpc)
                res = {}
                for rows_ws in (False, True):
                    stats, dl, rows = launch(ops, z, onehot, eps, k, rows_ws, rpc, lam)
                    st = host(stats)
                    print("b %d c %d rpc %d eps %g k %d lam %g rows %s: loss %.8f want %.8f, hits %g / %g, top-k %g / %g" %
                          (b, c, rpc, eps, k, lam, rows_ws, st[0] / b, want["loss"], st[1], want["hits"], st[2], want["topk"]))
                    assert abs(st[0] / b - want["loss"]) < 1e-5 * max(1.0, abs(want["loss"]))
                    assert want["hits"] > 0 and st[1] == want["hits"] and st[2] == want["topk"]
                    close(host(dl), want["dlogits"], rtol=1e-4, atol_rel=1e-6, msg="dlogits eps %g k %d lam %g" % (eps, k, lam))
                    if rows_ws:
                        rw = host(rows).reshape(3, b)
                        assert np.isfinite(rw).all()
                        assert np.array_equal(rw[1], (np.argmax(z, 1) == np.argmax(onehot, 1)).astype(np.float32))
                        assert np.array_equal(rw[2], LS.topk_hits(z, onehot, k).astype(np.float32) if k else np.zeros(b, np.float32))
                    res[rows_ws] = (stats, dl, host(rows)[:b].copy() if rows_ws else None)
                # the two launch forms agree bit for bit in everything a row yields: dlogits, the row losses' hit counts.  Their loss
                # SUMS add the same row losses in the two fixed orders of vl_softmax_xent_ls (four wave sums | 256 strided sums and a
                # tree), which lam = 1 must reproduce per form (below): each is held to the float64 loss above, not to the other's bits
                # (on an MI355X 18 of this file's 84 pairs of sums differ in the last bits).
                assert torch.equal(bits(res[False][1]), bits(res[True][1]))
                assert torch.equal(bits(res[False][0][1:]), bits(res[True][0][1:]))
                # The row losses themselves agree bit for bit: those of the rows form, added on the host in the one-workgroup form's
                # order (wave w adds rows w, w + 4, ..; then ((w0 + w1) + w2) + w3), give its sum to the last bit.
                waves = [np.float32(0)] * 4
                for r, v in enumerate(res[True][2]):
                    waves[r % 4] = np.float32(waves[r % 4] + v)
                resum = np.float32(np.float32(np.float32(waves[0] + waves[1]) + waves[2]) + waves[3])
                assert resum.view(np.int32) == host(res[False][0])[:1].view(np.int32)[0]
                print("    loss sums of the two forms: %s" % ("equal bits" if torch.equal(bits(res[False][0][:1]), bits(res[True][0][:1]))
                                                              else "differ in the order of the sum only"))
                # the weight read from the device: the bytes of the host-argument launch
                n = b
                for rows_ws in (False, True):
                    dl2, st2 = torch.full((n, c), NAN, device=DEV), torch.zeros(3, device=DEV)
                    rows2 = torch.full((3 * n,), NAN, device=DEV) if rows_ws else None
                    ops.softmax_xent_mix(dev(z), dev(onehot, torch.int32), dl2, st2, 1.0 / n, rows2, rpc, eps, k,
                                         torch.tensor([lam], device=DEV))
                    assert torch.equal(bits(dl2), bits(res[rows_ws][1])) and torch.equal(bits(st2), bits(res[rows_ws][0]))
                # lam = 1: the bytes of vl_softmax_xent_ls
                if lam == 1.0:
                    for rows_ws in (False, True):
                        dl1, st1 = torch.full((n, c), NAN, device=DEV), torch.zeros(3, device=DEV)
                        rows1 = torch.full((3 * n,), NAN, device=DEV) if rows_ws else None
                        ops.softmax_xent_ls(dev(z), dev(onehot, torch.int32), dl1, st1, 1.0 / n, rows1, eps, k)
                        assert torch.equal(bits(dl1), bits(res[rows_ws][1])) and torch.equal(bits(st1), bits(res[rows_ws][0]))


def test_softmax_xent_mix_host_checks(ops):
    from vltf_amd._ffi import VltfError
    z, onehot = case(4, 64)
    zd, yd = dev(z), dev(onehot, torch.int32)
    dl, stats, rows = torch.empty_like(zd), torch.zeros(3, device=DEV), torch.zeros(12, device=DEV)
    with pytest.raises(VltfError, match="int32"):
        ops.softmax_xent_mix(zd, yd.float(), dl, stats, 0.25, rows, 1, 0.1, 2, 0.5)
    with pytest.raises(VltfError, match="3\\*batch"):
        ops.softmax_xent_mix(zd, yd, dl, stats, 0.25, rows[:8], 1, 0.1, 2, 0.5)
    with pytest.raises(VltfError, match="3 floats"):
        ops.softmax_xent_mix(zd, yd, dl, stats[:2], 0.25, rows, 1, 0.1, 2, 0.5)
    with pytest.raises(VltfError, match="logits' shape"):
        ops.softmax_xent_mix(zd, yd[:2], dl, stats, 0.25, rows, 1, 0.1, 2, 0.5)
    for rpc, eps, k, lam in ((3, 0.1, 2, 0.5), (0, 0.1, 2, 0.5), (1, -0.1, 2, 0.5), (1, 1.0, 2, 0.5), (1, 0.1, -1, 0.5), (1, 0.1, 2, -0.5),
                             (1, 0.1, 2, 1.5), (1, 0.1, 2, NAN)):
        with pytest.raises(VltfError, match="whole clips|smoothing|top_k|lam must lie"):
            ops.softmax_xent_mix(zd, yd, dl, stats, 0.25, rows, rpc, eps, k, lam)
    torch.cuda.synchronize()
    assert not bool(stats.any())                                               # nothing was launched


# ---- 4. engine steps (the geometry of tests/test_momentum_gpu.py, through tests/test_label_smoothing_gpu.py) ------------------------------------
LAM = 0.7
_ORACLE = {}


def oracle_step(clips, lam, eps=0.0):
    """O.lrcn_train_step fed the frames of the first `clips` clips blended on the host and their mixed labels; once per case."""
    p, frames, onehot = data()
    if (clips, lam, eps) not in _ORACLE:
        x = (frames[:clips * FPC].astype(np.float32) - MEAN).reshape((clips, FPC) + SHAPE)
        _ORACLE[(clips, lam, eps)] = O.lrcn_train_step(p, MX.blend(x, lam).reshape((clips * FPC,) + SHAPE), MX.targets(onehot[:clips], lam, eps),
                                                       FPC, lr=LR, clip_norm=CLIP)
    return _ORACLE[(clips, lam, eps)]


def check_step(out, eng, want, onehot):
    newp, loss, gn = want[0], want[1], want[2]
    print("loss %.8f want %.8f, grad norm %.8f want %.8f, accuracy %g" % (out["loss"], loss, out["grad_norm"], gn, out["accuracy"]))
    np.testing.assert_allclose(eng.logits_host(), want[4], rtol=1e-3, atol=1e-3)
    assert abs(out["loss"] - loss) < 1e-4 * max(1, abs(loss)) and abs(out["grad_norm"] - gn) < 1e-3 * gn
    assert out["accuracy"] == O.accuracy(eng.logits_host(), onehot)                  # against the clips' OWN labels
    got = eng.get_params()
    for k in newp:
        np.testing.assert_allclose(got[k], newp[k], rtol=1e-4, atol=1e-5, err_msg="param " + k)


def same_bits(a, b):
    pa, pb = a.get_params(), b.get_params()
    return all(np.array_equal(pa[k].view(np.int32), pb[k].view(np.int32)) for k in pa)


def test_engine_eager_step():
    from vltf_amd.engine import LRCNEngine
    p, _, onehot = data()
    assert not np.array_equal(onehot[0], onehot[1])                                   # the pair's labels differ: the mixed row has two entries
    eng = LRCNEngine(small_cfg(mixup_alpha=0.2, mixup_seed=7), max_clips=B, device=DEV)
    eng.load_params(p)
    assert eng.mix_lam is not None and eng.mix_lam.numel() == 1 and eng.stats.numel() == 3 and eng.loss_rows.numel() == 3 * B
    out = eng.train_step_u8(*dev_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, mix_lambda=LAM)
    assert eng.mix_lambda_last == LAM and float(eng.mix_lam) == np.float32(LAM)
    check_step(out, eng, oracle_step(B, LAM), onehot[:B])
    unmixed = oracle_step(B, 1.0)
    assert abs(out["loss"] - unmixed[1]) > 1e-3 * abs(unmixed[1])                     # and it is not the unmixed step
    # the override is folded: 0.3 is 0.7 with the partners swapped
    again = LRCNEngine(small_cfg(mixup_alpha=0.2, mixup_seed=7), max_clips=B, device=DEV)
    again.load_params(p)
    out2 = again.train_step_u8(*dev_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, mix_lambda=0.3)
    assert again.mix_lambda_last == LAM and out2 == out and same_bits(again, eng)
    # a forward-only engine ignores the option, and forward never blends
    infer = LRCNEngine(small_cfg(mixup_alpha=0.2, mixup_seed=7), max_clips=B, device=DEV, training=False)
    assert infer.mix_lam is None and infer.mixup_alpha == 0.0 and infer.stats.numel() == 2


def test_engine_with_label_smoothing_and_an_odd_clip_count():
    """Three clips: the middle one is its own partner and trains on its own label, smoothed; top-k hits ride along."""
    from vltf_amd.engine import LRCNEngine
    p, _, onehot = data()
    eng = LRCNEngine(small_cfg(mixup_alpha=1.0, label_smoothing=0.1, top_k=2), max_clips=3, device=DEV)
    eng.load_params(p)
    out = eng.train_step_u8(*dev_batch(0, 3), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, mix_lambda=LAM)
    check_step(out, eng, oracle_step(3, LAM, 0.1), onehot[:3])
    assert out["topk_correct"] == float(LS.topk_hits(eng.logits_host(), onehot[:3], 2).sum())


def test_engine_per_frame_fc_head():
    """classifier fc without frame fusion: one logits row per FRAME; a frame's partner is the same frame of the mirrored clip."""
    from vltf_amd.engine import LRCNEngine
    ncls = 11
    rng = np.random.default_rng(12)
    cfg = small_cfg(num_classes=ncls, classifier="fc", frame_fusion=None, mixup_alpha=0.2)
    p = O.init_params(rng, ncls, "fc6", cfg.lstm_hidden, 1, SHAPE, classifier="fc", well_scaled=True)
    frames = rng.integers(0, 256, (B * FPC,) + SHAPE, dtype=np.uint8)
    onehot = O.labels_to_one_hot([[l] for l in rng.integers(0, ncls, B * FPC)], ncls)
    x = (frames.astype(np.float32) - MEAN).reshape((B, FPC) + SHAPE)
    want = O.lrcn_train_step(p, MX.blend(x, LAM).reshape((B * FPC,) + SHAPE), MX.targets(onehot, LAM, 0.0, FPC), FPC, lr=LR, clip_norm=CLIP,
                             classifier="fc", frame_fusion=None)
    eng = LRCNEngine(cfg, max_clips=B, device=DEV)
    eng.load_params(p)
    assert eng.rows_out == B * FPC and eng.loss_rows.numel() == 3 * B * FPC
    out = eng.train_step_u8(torch.tensor(frames, device=DEV), torch.tensor(onehot, device=DEV), lr=LR, clip_norm=CLIP, mean_bgr=MEAN,
                            mix_lambda=LAM)
    assert out["rows"] == B * FPC
    check_step(out, eng, want, onehot)


def test_mixup_off_is_the_engine_of_before(monkeypatch):
    """mixup_alpha 0 / None, given or not: no device word, no blend launch, the loss launch, keys and bytes of a plain engine -- loss,
    logits and parameters after two steps."""
    import vltf_amd.ops as ops_
    from vltf_amd._ffi import VltfError
    from vltf_amd.engine import LRCNEngine
    monkeypatch.setattr(ops_, "mixup_pairs", lambda *a, **k: pytest.fail("mixup_pairs was launched"))
    monkeypatch.setattr(ops_, "softmax_xent_mix", lambda *a, **k: pytest.fail("softmax_xent_mix was launched"))
    p, _, _ = data()
    res = []
    for kw in (dict(mixup_alpha=0.0, mixup_seed=0), dict(mixup_alpha=None, mixup_seed=None), dict()):
        eng = LRCNEngine(small_cfg(**kw), max_clips=B, device=DEV)
        eng.load_params(p)
        assert eng.mix_lam is None and eng.stats.numel() == 2 and eng.loss_rows.numel() == 2 * B
        outs = [eng.train_step_u8(*dev_batch(c0, c0 + B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN) for c0 in (0, 2)]
        res.append((outs, eng.logits_host().copy(), eng.get_params()))
        with pytest.raises(VltfError, match="mix_lambda is given, but mixup is off"):
            eng.train_step_u8(*dev_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, mix_lambda=0.7)
        with pytest.raises(VltfError, match="mix_lambda is given, but mixup is off"):
            eng.train_step_f32(torch.zeros((B * FPC,) + SHAPE, device=DEV), dev_batch(0, B)[1], lr=LR, mix_lambda=0.7)
        assert eng.step_count == 2
    for outs, logits, params in res[:2]:
        assert outs == res[2][0] and np.array_equal(logits.view(np.int32), res[2][1].view(np.int32))
        for k in params:
            assert np.array_equal(params[k].view(np.int32), res[2][2][k].view(np.int32)), k


def test_engine_refusals():
    from vltf_amd._ffi import VltfError
    from vltf_amd.engine import LRCNEngine
    for kw in (dict(mixup_alpha=-0.1), dict(mixup_alpha=NAN), dict(mixup_alpha=True), dict(mixup_alpha="0.2"), dict(mixup_seed=7),
               dict(mixup_alpha=0.2, mixup_seed=-1), dict(mixup_alpha=0.2, mixup_seed=1.5)):
        with pytest.raises(VltfError, match="mixup_alpha|mixup_seed"):
            LRCNEngine(small_cfg(**kw), max_clips=B, device=DEV)
    eng = LRCNEngine(small_cfg(mixup_alpha=0.2), max_clips=B, device=DEV)
    eng.load_params(data()[0])
    for bad in (-0.1, 1.5, NAN, True, "0.7"):
        with pytest.raises(VltfError, match="mix_lambda"):
            eng.train_step_u8(*dev_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, mix_lambda=bad)
    assert eng.step_count == 0


def step_keys_equal(a, b):
    return set(a) == set(b) and all(a[k] == b[k] for k in ("loss_sum", "correct", "grad_norm", "rows", "loss"))


def test_captured_step_equals_eager():
    """Step 1 is the warm-up, step 2 is captured and replayed, step 3 is a replay, each with a weight of its own: the replays pick up the
    weight the host wrote before them and are bit-equal to the eager engine in the sums, the norm and every parameter."""
    from vltf_amd.engine import LRCNEngine
    p, _, onehot = data()
    eager = LRCNEngine(small_cfg(mixup_alpha=0.2), max_clips=B, device=DEV)
    graph = LRCNEngine(small_cfg(mixup_alpha=0.2, step_graph=True), max_clips=B, device=DEV)
    eager.load_params(p)
    graph.load_params(p)
    for step, (c0, lam) in enumerate(((0, LAM), (2, 0.9), (0, 0.55))):
        outs = [e.train_step_u8(*dev_batch(c0, c0 + B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, mix_lambda=lam) for e in (eager, graph)]
        assert step_keys_equal(*outs), (step, outs)
        assert same_bits(eager, graph), step
        assert np.array_equal(eager.logits_host().view(np.int32), graph.logits_host().view(np.int32))
        if step == 0:
            check_step(outs[1], graph, oracle_step(B, LAM), onehot[:B])
    assert len(graph._graphs) == 1                                                    # one graph: the weight is no part of the key


def test_a_replay_reads_the_weight_written_before_it():
    """Three engines, the same two steps; the third step is a replay on the captured engine with lam2: it is the eager lam2 step bit
    for bit, and it is not the eager lam1 step."""
    from vltf_amd.engine import LRCNEngine
    p, _, _ = data()
    lam1, lam2 = 0.9, 0.6
    graph = LRCNEngine(small_cfg(mixup_alpha=0.2, step_graph=True), max_clips=B, device=DEV)
    eager1, eager2 = (LRCNEngine(small_cfg(mixup_alpha=0.2), max_clips=B, device=DEV) for _ in range(2))
    for e in (graph, eager1, eager2):
        e.load_params(p)
        for c0 in (0, 2):
            e.train_step_u8(*dev_batch(c0, c0 + B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, mix_lambda=lam1)
    assert len(graph._graphs) == 1 and same_bits(graph, eager1) and same_bits(graph, eager2)
    og = graph.train_step_u8(*dev_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, mix_lambda=lam2)
    o1 = eager1.train_step_u8(*dev_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, mix_lambda=lam1)
    o2 = eager2.train_step_u8(*dev_batch(0, B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, mix_lambda=lam2)
    assert len(graph._graphs) == 1
    assert step_keys_equal(og, o2) and same_bits(graph, eager2)
    assert og["loss_sum"] != o1["loss_sum"] and not same_bits(graph, eager1)


def test_accumulated_update_draws_a_weight_per_micro_step():
    """accumulate 2, three updates, captured (warm-up, capture, replay of each micro-step's role): every micro-step draws
    mixup_lambda(alpha, seed, step_count * 2 + i).  Bit for bit the eager engine given those weights through mix_lambda."""
    from vltf_amd.engine import LRCNEngine, mixup_lambda
    p, _, _ = data()
    alpha, seed = 0.4, 11
    drawn = LRCNEngine(small_cfg(mixup_alpha=alpha, mixup_seed=seed, accumulate=2, step_graph=True), max_clips=B, device=DEV)
    given = LRCNEngine(small_cfg(mixup_alpha=alpha, mixup_seed=seed, accumulate=2), max_clips=B, device=DEV)
    drawn.load_params(p)
    given.load_params(p)
    seen = []
    for update in range(3):
        for i, c0 in enumerate((0, 2)):
            lam = mixup_lambda(alpha, seed, update * 2 + i)
            a = drawn.train_step_u8(*dev_batch(c0, c0 + B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, micro=(i, 2))
            b = given.train_step_u8(*dev_batch(c0, c0 + B), lr=LR, clip_norm=CLIP, mean_bgr=MEAN, micro=(i, 2), mix_lambda=lam)
            assert drawn.mix_lambda_last == lam == given.mix_lambda_last and 0.5 <= lam < 1.0
            assert a["loss_sum"] == b["loss_sum"] and a["correct"] == b["correct"] and a["rows"] == b["rows"], (update, i)
            seen.append(lam)
        assert a["grad_norm"] == b["grad_norm"] and same_bits(drawn, given), update
    assert len(set(seen)) == 6 and drawn.step_count == 3


def test_bf16_conv_path_blends_the_packed_input():
    """conv_math bf16: feed_u8 writes conv1's packed space-to-depth input directly; the blend runs over it (dtype 1).  After a feed with
    mixing it is the reference blend of the one fed without, within the bf16 bound; the halo and padding zeros stay zero; one full
    step is finite."""
    from vltf_amd.engine import LRCNEngine
    p, _, _ = data()
    eng = LRCNEngine(small_cfg(mixup_alpha=0.2, conv_math="bf16"), max_clips=B, device=DEV)
    eng.load_params(p)
    frames, onehot = dev_batch(0, B)
    n, b = eng.feed_u8(frames, MEAN)
    assert eng.c8 and eng._xb_fed and (n, b) == (B * FPC, B)
    xb = eng.layers[0]["xb"][:n]
    assert xb.dtype == torch.bfloat16 and (xb.numel() // b) % 8 == 0
    before = xb.to(torch.float64).cpu().numpy().reshape(b, -1)
    eng._mix_write(LAM, None)
    eng._mix_launch(n, b)
    torch.cuda.synchronize()
    got = xb.to(torch.float64).cpu().numpy().reshape(b, -1)
    want = MX.blend(before, LAM)
    err = np.abs(got - want)
    bound = 0.5 * MX.bf16_ulp(np.maximum(np.abs(got), np.abs(want))) + 8 * EPS32 * pair_scale(before)
    print("worst error / bound %.3f, zeros %d of %d" % (float((err / bound).max()), int((before == 0).all(axis=0).sum()), before.shape[1]))
    assert (err <= bound).all() and not np.array_equal(got, before)
    assert not got[:, (before == 0).all(axis=0)].any()                              # zeros of both partners (halo, padding) blend to zero
    out = eng.train_step_u8(frames, onehot, lr=LR, clip_norm=CLIP, mean_bgr=MEAN, mix_lambda=LAM)
    assert np.isfinite(out["loss"]) and np.isfinite(out["grad_norm"]) and out["grad_norm"] > 0 and np.isfinite(eng.logits_host()).all()
    assert all(np.isfinite(v).all() for v in eng.get_params().values())


# ---- 5. run_task on the example -----------------------------------------------------------------------------------------------------------------
def test_run_task_on_the_example(tmp_path, monkeypatch):
    """examples/lrcn_mixup.yml shrunk: the synthetic dataset and the small network of tests/test_run_task_gpu.py, one epoch, with the
    example's own mixup keys.  The info line is there, the losses are finite, and a second run with the same seed logs the same losses."""
    from tests.test_host_workflow import make_dataset
    from tests.test_run_task_gpu import RAW, write_cfg
    from vltf_amd import run_task
    monkeypatch.setenv("VLTF_PREFETCH", "0")
    monkeypatch.setenv("VLTF_CONV_MATH", "f32")
    monkeypatch.delenv("VLTF_STEP_GRAPH", raising=False)
    with open(os.path.join(ROOT, "examples", "lrcn_mixup.yml")) as f:
        example = yaml.safe_load(f)["run"]
    assert example["train"]["mixup_alpha"] == 0.2 and example["train"]["mixup_seed"] == 7
    folder = str(tmp_path)
    train_path, _, _ = make_dataset(folder, "train.txt", nvid=4, cpv=(1, 2, 1, 1), shape=RAW, seed=1)
    losses = []
    for run in ("run_a", "run_b"):
        out = write_cfg(folder, run + ".yml", train_path, "train", epochs=1, det=True, run=run)
        with open(out) as f:
            c = yaml.safe_load(f)
        c["run"]["train"].update(mixup_alpha=example["train"]["mixup_alpha"], mixup_seed=example["train"]["mixup_seed"])
        with open(out, "w") as f:
            yaml.safe_dump(c, f)
        run_task.main(out, seed=3)
        log = open(glob.glob(os.path.join(folder, run, "log_e2e_train_scratch_*.log"))[0]).read()
        assert "Mixup: alpha 0.2, seed 7" in log and "inside a rank's batch" in log
        found = [float(v) for v in re.findall(r"batch loss/nats : ([-+0-9.eE]+|nan|inf) /", log)]
        assert len(found) >= 2 and np.isfinite(found).all(), found
        losses.append(found)
    assert losses[0] == losses[1]
