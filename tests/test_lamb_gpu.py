"""LAMB on the device (vl_lamb_moments, vl_lamb_apply, NetConfig.lamb): the moments bit for bit against vl_adam_apply, the fp64 rows
against vl_tensor_stats and tests/lamb_ref.py, the update against the reference, slicing, the skip word and the refusals, LRCNEngine
(fp32 and the bf16 path, captured, with frozen layers, under accumulation), GraphEngine, one-rank RCCL and the checkpoint of run_task.
Small shapes: a flat buffer of 35 K floats; 67x67x3 frames, 2 clips x 3 frames, hidden 8, 7 classes.

Bounds (tests/lamb_ref.py states the rounding model: mul, sqrt, add, div agree bit for bit, an fma within one ulp).
- m', v': bit-equal to vl_adam_apply's at the ops level; within one ulp of lamb_ref.moments where the reference forms them (the fma).
- u is formed by the reference from the DEVICE's m', v' (checked as above), so u is bit-equal where decay is 0 and within one ulp of
  the device's where decay > 0 (the fma that adds decay * w).
- rows.u_sumsq: lamb_ref.sumsq_tol(n, decay) relative = (2 ULP + ULP^2 where decay > 0, else 0) + 2 n 2^-53: one ulp per element of u
  changes u^2 by at most (2 ULP + ULP^2) u^2, and each side's float64 sum of n non-negative terms is within n 2^-53 of exact.
- trust: lamb_ref.trust_tol(n, decay) relative = half of each sum's bound, six float64 roundings (two square roots and a division on
  either side) and the device's one rounding to float32 (2^-24), the reference being compared as a double.
- w': |w' - reference| <= ulp(reference) + a ulp(u) where decay > 0, ulp(reference) where it is 0; `a` is formed from the device's own
  trust value, so it is the device's `a` bit for bit."""
import glob
import math
import os
import socket

import numpy as np
import pytest
import torch
import yaml

from oracle import lrcn_oracle as O
from tests import lamb_ref
from tests.test_momentum_gpu import B, CLIP, DEV, MEAN, bits, host, small_batches, small_cfg, state_block

pytestmark = pytest.mark.gpu
WD = 0.01
EPS = 1e-6
LRS = (0.02, 0.05, 0.01)
LR = 0.0123

# ---- the flat buffer of the kernel tests ------------------------------------------------------------------------------------------------
CHUNK = 16384                      # VL_STAT_CHUNK (asserted below)
# (begin, length, lr_mult, trust index): two chunks; 3 elements; 1 element; all-zero w; a NaN in g; a bias range (index -1); one chunk and
# a part, beginning at an odd element.  NaN-filled gaps before the first, between some, and behind the last.
_LAYOUT = [(3, CHUNK + 5, 1.0, 0), (CHUNK + 9, 3, 0.25, 1), (CHUNK + 12, 1, 2.0, 2), (CHUNK + 15, 7, 3.0, 3), (CHUNK + 22, 5, 1.0, 4),
           (CHUNK + 31, 1029, 0.5, -1), (CHUNK + 1061, CHUNK + 1023, 4.0, 5)]
COUNT = 2 * CHUNK + 2090
TWO_CHUNKS, ZERO_W, NAN_G, BIAS = 0, 3, 4, 5
N_TRUST = 6
_BUF = {}


def table(decay):
    return [(lo, lo + n, mult, decay if ti >= 0 else 0.0, ti) for lo, n, mult, ti in _LAYOUT]


def flat_data():
    """w, g, m, v on the host, made once, never written: N(0, 1) weights, 3 N(0, 1) gradients, moments of that size, NaN outside the
    ranges."""
    if not _BUF:
        r = table(0.0)
        assert r[-1][1] < COUNT and all(a[1] <= b[0] for a, b in zip(r, r[1:])) and r[0][0] > 0
        assert any(a[1] < b[0] for a, b in zip(r, r[1:])) and any(a[1] == b[0] for a, b in zip(r, r[1:]))
        rng = np.random.default_rng(7)
        w = rng.standard_normal(COUNT).astype(np.float32)
        g = (3 * rng.standard_normal(COUNT)).astype(np.float32)
        m = (0.3 * rng.standard_normal(COUNT)).astype(np.float32)
        v = (0.09 * rng.standard_normal(COUNT) ** 2).astype(np.float32)
        inside = np.zeros(COUNT, bool)
        for lo, hi, _, _, _ in r:
            inside[lo:hi] = True
        for t in (w, g, m, v):
            t[~inside] = np.nan
        w[r[ZERO_W][0]:r[ZERO_W][1]] = 0.0
        g[r[NAN_G][0] + 2] = np.nan
        _BUF.update(w=w, g=g, m=m, v=v, inside=inside)
    return _BUF["w"], _BUF["g"], _BUF["m"], _BUF["v"], _BUF["inside"]


def on_device(x, offset):
    """x as a view that begins `offset` floats behind a 16-byte aligned address."""
    base = torch.zeros(x.size + offset, device=DEV)
    assert base.data_ptr() % 16 == 0
    v = base[offset:]
    v.copy_(torch.from_numpy(x).to(DEV))
    return v


def norm_word(g, ranges):
    """The global sum of squares over the ranges without the NaN one: a finite norm."""
    from vltf_amd import ops
    ss, sws = torch.zeros(1, device=DEV), torch.empty(1024, device=DEV)
    ops.sumsq_tiers(g, [(r[0], r[1], 1.0) for k, r in enumerate(ranges) if k != NAN_G], ss, sws)
    return ss


def lamb_state(step, lr, c1, c2):
    from vltf_amd import ops
    st = state_block(step, lr)
    ops.step_state_set_lamb(st, c1, c2)
    return st


def lamb_buffers(ranges, n_trust=N_TRUST):
    from vltf_amd import ops
    rows = torch.full(((n_trust + 1) * ops.LAMB_ROW_BYTES,), 0xAB, dtype=torch.uint8, device=DEV)
    trust = torch.full((n_trust + 1,), -7.0, device=DEV)
    ws = torch.empty(ops.lamb_moments_ws_bytes(ranges), dtype=torch.uint8, device=DEV)
    return rows, trust[:n_trust], trust, ws


def ulp(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


def check_range_update(w0, u, got_w, lr, mult, t, decay, what):
    """w' against the reference: one ulp of the reference, plus a ulp(u) where decay > 0 (module docstring)."""
    a = lamb_ref.rate(lr, mult, t)
    want = lamb_ref.apply(w0, u, a)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got_w), fin), what
    bound = ulp(want[fin]) + (float(a) * ulp(u[fin]) if decay > 0 else 0.0)
    err = np.abs(got_w[fin].astype(np.float64) - want[fin].astype(np.float64))
    print("%s: max |w' - reference| / bound = %.3g" % (what, float((err / bound).max()) if err.size else 0.0))
    assert (err <= bound).all(), what
    return a


# ---- 1. the two launches against vl_adam_apply, vl_tensor_stats and the reference ---------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("st", [False, True], ids=["eager", "st"])
@pytest.mark.parametrize("decay", [0.0, 0.05], ids=["nodecay", "decay"])
@pytest.mark.parametrize("clip", [0.0, 1.0], ids=["noclip", "clip"])
def test_moments_rows_trust_and_update(clip, decay, st, offset):
    from vltf_amd import ops
    assert ops.STAT_CHUNK == CHUNK
    w, g, m, v, inside = flat_data()
    ranges = table(decay)
    t = 3
    c1, c2 = (float(c) for c in lamb_ref.corrections(t))
    wd, gd, md, vd = (on_device(x, offset) for x in (w, g, m, v))
    ss = norm_word(gd, ranges)
    sc = lamb_ref.clip_scale_f32(clip, float(host(ss)[0]))
    if clip > 0:
        assert float(sc) < 0.5                                                  # the clip bites
    rows, trust, trust_all, ws = lamb_buffers(ranges)
    state = lamb_state(t - 1, LR, c1, c2)
    if st:
        ops.lamb_moments_st(wd, gd, md, vd, ranges, rows, trust, ws, state, EPS, clip, ss)
    else:
        ops.lamb_moments(wd, gd, md, vd, ranges, rows, trust, ws, c1, c2, EPS, clip, ss)
    ins = torch.from_numpy(inside).to(DEV)
    # w and g are never written; m and v keep their bits (NaN) outside every range
    assert torch.equal(bits(wd), bits(on_device(w, offset))) and torch.equal(bits(gd), bits(on_device(g, offset)))
    assert torch.equal(bits(md)[~ins], bits(on_device(m, offset))[~ins]) and torch.equal(bits(vd)[~ins], bits(on_device(v, offset))[~ins])
    # m', v': what vl_adam_apply leaves from the same inputs, sumsq and gscale
    aw, am, av = (on_device(x, offset) for x in (w, m, v))
    ops.adam_apply_tiers(aw, gd, am, av, [(r[0], r[1], 1.0) for r in ranges], LR, t, clip, ss, 1.0)
    assert torch.equal(bits(md), bits(am)) and torch.equal(bits(vd), bits(av))
    m1, v1 = host(md), host(vd)
    # rows.w_sumsq: vl_tensor_stats's bits for the same segments
    idx = [r for r in ranges if r[4] >= 0]
    segs = [(r[0], r[1]) for r in idx]
    srows = torch.empty(len(segs) * ops.STAT_ROW_BYTES, dtype=torch.uint8, device=DEV)
    ops.tensor_stats(wd, gd, segs, srows, torch.empty(ops.tensor_stats_ws_bytes(segs), dtype=torch.uint8, device=DEV))
    want_rows = ops.stat_rows(srows, len(segs))
    got_rows = ops.lamb_rows(rows, N_TRUST)
    assert np.array_equal(got_rows["w_sumsq"].view(np.int64), want_rows["w_sumsq"].view(np.int64))
    assert (got_rows["reserved"] == 0).all()
    assert bytes(host(rows)[N_TRUST * ops.LAMB_ROW_BYTES:]) == b"\xab" * ops.LAMB_ROW_BYTES          # n rows written, not one more
    tr = host(trust_all)
    assert tr[N_TRUST] == -7.0
    # rows.u_sumsq, nonfinite and trust against the reference
    us = {}
    for k, (lo, hi, mult, d, ti) in enumerate(ranges):
        us[k] = u = lamb_ref.direction(w[lo:hi], m1[lo:hi], v1[lo:hi], c1, c2, EPS, d)
        if ti < 0:
            continue
        n = hi - lo
        uq, ub = lamb_ref.sumsq64(u)
        want_t = lamb_ref.trust(w[lo:hi], u)
        print("range %d [%d, %d): u_sumsq %.17g (reference %.17g), nonfinite %d, trust %.9g (reference %.17g)" %
              (k, lo, hi, got_rows["u_sumsq"][ti], uq, got_rows["nonfinite"][ti], tr[ti], want_t))
        assert abs(got_rows["u_sumsq"][ti] - uq) <= lamb_ref.sumsq_tol(n, d) * uq, k
        if k == NAN_G:
            assert got_rows["nonfinite"][ti] > 0 and ub > 0 and want_t == 1.0 and tr[ti] == 1.0
        elif k == ZERO_W:
            assert got_rows["nonfinite"][ti] == 0 and got_rows["w_sumsq"][ti] == 0.0 and want_t == 1.0 and tr[ti] == 1.0
        else:
            assert got_rows["nonfinite"][ti] == 0 and want_t != 1.0
            assert abs(float(tr[ti]) - want_t) <= lamb_ref.trust_tol(n, d) * want_t, (k, tr[ti], want_t)
    # the update
    if st:
        ops.lamb_apply_st(wd, md, vd, ranges, trust, state, EPS)
    else:
        ops.lamb_apply(wd, md, vd, ranges, trust, LR, c1, c2, EPS)
    w1 = host(wd)
    assert torch.equal(bits(md), bits(am)) and torch.equal(bits(vd), bits(av))                   # m and v are read-only here
    assert torch.equal(bits(wd)[~ins], bits(on_device(w, offset))[~ins])
    for k, (lo, hi, mult, d, ti) in enumerate(ranges):
        check_range_update(w[lo:hi], us[k], w1[lo:hi], LR, mult, 1.0 if ti < 0 else tr[ti], d, "range %d" % k)
        if k == NAN_G:
            assert np.isnan(w1[lo + 2]) and np.isfinite(np.delete(w1[lo:hi], 2)).all()            # the NaN travels as under Adam
        else:
            assert not np.array_equal(w1[lo:hi], w[lo:hi]), k
    # the trust does something: range 6 moved by another amount than with trust 1
    lo, hi, mult, d, ti = ranges[6]
    assert tr[ti] != 1.0
    pw = on_device(w, offset)
    ops.lamb_apply(pw, md, vd, [(lo, hi, mult, d, -1)], None, LR, c1, c2, EPS)
    assert not torch.equal(pw[lo:hi], wd[lo:hi])


def test_eager_and_st_forms_agree_bit_for_bit():
    from vltf_amd import ops
    w, g, m, v, _ = flat_data()
    ranges = table(0.05)
    c1, c2 = (float(c) for c in lamb_ref.corrections(5))
    outs = []
    for st in (False, True):
        wd, gd, md, vd = (on_device(x, 1) for x in (w, g, m, v))
        ss = norm_word(gd, ranges)
        rows, trust, _, ws = lamb_buffers(ranges)
        if st:
            state = lamb_state(4, LR, c1, c2)
            ops.lamb_moments_st(wd, gd, md, vd, ranges, rows, trust, ws, state, EPS, 1.0, ss)
            ops.lamb_apply_st(wd, md, vd, ranges, trust, state, EPS)
        else:
            ops.lamb_moments(wd, gd, md, vd, ranges, rows, trust, ws, c1, c2, EPS, 1.0, ss)
            ops.lamb_apply(wd, md, vd, ranges, trust, LR, c1, c2, EPS)
        outs.append((wd, md, vd, trust, rows))
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.uint8) if a.dtype == torch.uint8 else bits(a), b.view(torch.uint8) if b.dtype == torch.uint8 else bits(b))


def test_step_state_set_lamb_writes_two_words_and_no_other_setter_touches_them():
    from vltf_amd import ops
    st = ops.step_state(DEV)
    ops.step_state_set(st, 7, 0.5, 3)
    ops.step_state_set_ema(st, 0.25)
    before = host(st).copy()
    assert before[6] == 0 and before[7] == 0
    ops.step_state_set_lamb(st, 10.0, 1000.0)
    after = host(st).copy()
    assert np.array_equal(after[:6], before[:6])
    assert after[6:8].view(np.float32).tolist() == [10.0, 1000.0]                # bytes 24 and 28
    ops.step_state_set(st, 8, 0.125, 4)
    ops.step_state_set_micro(st, 9, 11, 0.0625, 5)
    ops.step_state_set_ema(st, 0.5)
    assert host(st)[6:8].view(np.float32).tolist() == [10.0, 1000.0]


# ---- 2. more ranges than one launch takes --------------------------------------------------------------------------------------------------
def test_more_ranges_than_one_launch_takes():
    """70 ranges of 3 elements with one-element gaps: two launches each, all indexing the one rows / trust pair; bit for bit what 70
    single-range calls give, and the reference's trust."""
    from vltf_amd import ops
    n = 70
    gen = torch.Generator(device="cpu").manual_seed(1)
    w, g, m = (torch.randn(4 * n, generator=gen) for _ in range(3))
    v = torch.rand(4 * n, generator=gen)
    ranges = [(4 * i, 4 * i + 3, 1.0 + 0.01 * i, 0.001 * i, i) for i in range(n)]
    c1, c2 = (float(c) for c in lamb_ref.corrections(2))
    gw, gg, gm, gv = (t.to(DEV) for t in (w, g, m, v))
    rows, trust, _, ws = lamb_buffers(ranges, n)
    assert ws.numel() == 64 * ops.LAMB_ROW_BYTES                                # the largest slice
    ops.lamb_moments(gw, gg, gm, gv, ranges, rows, trust, ws, c1, c2, EPS)
    ops.lamb_apply(gw, gm, gv, ranges, trust, LR, c1, c2, EPS)
    ow, om, ov = (t.to(DEV) for t in (w, m, v))
    orows, otrust, _, ows = lamb_buffers(ranges, n)
    for r in ranges:
        ops.lamb_moments(ow, gg, om, ov, [r], orows, otrust, ows, c1, c2, EPS)
    for r in ranges:
        ops.lamb_apply(ow, om, ov, [r], otrust, LR, c1, c2, EPS)
    assert torch.equal(bits(gw), bits(ow)) and torch.equal(bits(gm), bits(om)) and torch.equal(bits(gv), bits(ov))
    assert torch.equal(bits(trust), bits(otrust)) and torch.equal(rows, orows)
    tr, m1, v1 = host(trust), host(gm), host(gv)
    wn = w.numpy()
    for lo, hi, _, d, i in ranges:
        u = lamb_ref.direction(wn[lo:hi], m1[lo:hi], v1[lo:hi], c1, c2, EPS, d)
        want = lamb_ref.trust(wn[lo:hi], u)
        assert abs(float(tr[i]) - want) <= lamb_ref.trust_tol(3, d) * want, i
        assert torch.equal(bits(gw[hi:hi + 1]), bits(w[hi:hi + 1].to(DEV)))         # the one-element gaps


# ---- 3. skip word and argument checks -----------------------------------------------------------------------------------------------------
def test_skip_word_and_argument_checks():
    from vltf_amd import _ffi, ops
    from vltf_amd._ffi import VltfError
    w, g, m, v, inside = flat_data()
    ranges = table(0.05)
    c1, c2 = (float(c) for c in lamb_ref.corrections(1))
    wd, gd, md, vd = (on_device(x, 0) for x in (w, g, m, v))
    ss = norm_word(gd, ranges)
    rows, trust, _, ws = lamb_buffers(ranges)
    skip = torch.ones(1, dtype=torch.int32, device=DEV)
    gw, gm, gv = wd.clone(), md.clone(), vd.clone()
    st = lamb_state(0, LR, c1, c2)
    ops.lamb_moments(gw, gd, gm, gv, ranges, rows, trust, ws, c1, c2, EPS, 1.0, ss, skip=skip)
    ops.lamb_moments_st(gw, gd, gm, gv, ranges, rows, trust, ws, st, EPS, 1.0, ss, skip=skip)
    ops.lamb_apply(gw, gm, gv, ranges, trust, LR, c1, c2, EPS, skip=skip)
    ops.lamb_apply_st(gw, gm, gv, ranges, trust, st, EPS, skip=skip)

    def untouched():
        torch.cuda.synchronize()
        return torch.equal(bits(gw), bits(wd)) and torch.equal(bits(gm), bits(md)) and torch.equal(bits(gv), bits(vd))

    assert untouched() and bool((trust == -7.0).all())
    # ---- every refusal launches nothing
    for eps in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(VltfError, match="eps"):
            ops.lamb_moments(gw, gd, gm, gv, ranges, rows, trust, ws, c1, c2, eps)
        with pytest.raises(VltfError, match="eps"):
            ops.lamb_moments_st(gw, gd, gm, gv, ranges, rows, trust, ws, st, eps)
        with pytest.raises(VltfError, match="eps"):
            ops.lamb_apply(gw, gm, gv, ranges, trust, LR, c1, c2, eps)
        with pytest.raises(VltfError, match="eps"):
            ops.lamb_apply_st(gw, gm, gv, ranges, trust, st, eps)
    for c in (0.5, float("nan"), float("inf")):
        with pytest.raises(VltfError, match="c1"):
            ops.lamb_moments(gw, gd, gm, gv, ranges, rows, trust, ws, c, c2, EPS)
        with pytest.raises(VltfError, match="c2"):
            ops.lamb_apply(gw, gm, gv, ranges, trust, LR, c1, c, EPS)
        with pytest.raises(VltfError, match="c1"):
            ops.step_state_set_lamb(st, c, c2)
    with pytest.raises(VltfError):
        ops.lamb_moments(gw, gd, gm[:-1], gv, ranges, rows, trust, ws, c1, c2, EPS)            # a moment of another size
    with pytest.raises(VltfError):
        ops.lamb_moments(gw, gd, None, gv, ranges, rows, trust, ws, c1, c2, EPS)               # a null moment
    with pytest.raises(VltfError):
        ops.lamb_apply(gw, gm, gv[:-1], ranges, trust, LR, c1, c2, EPS)
    with pytest.raises(VltfError):
        ops.lamb_moments_st(gw, gd, gm, gv, ranges, rows, trust, ws, None, EPS)                # no step state
    with pytest.raises(VltfError):
        ops.lamb_apply_st(gw, gm, gv, ranges, trust, None, EPS)
    with pytest.raises(VltfError):
        ops.lamb_moments(gw, gd, gm, gv, ranges, None, None, ws, c1, c2, EPS)                  # indices, and no table to index
    with pytest.raises(VltfError):
        ops.lamb_apply(gw, gm, gv, ranges, None, LR, c1, c2, EPS)
    with pytest.raises(VltfError, match="rows"):
        ops.lamb_moments(gw, gd, gm, gv, ranges, rows[:N_TRUST * ops.LAMB_ROW_BYTES - 1], trust, ws, c1, c2, EPS)
    with pytest.raises(VltfError, match="ws"):
        ops.lamb_moments(gw, gd, gm, gv, ranges, rows, trust, ws[:-1], c1, c2, EPS)            # a workspace too small
    with pytest.raises(VltfError, match="ws"):
        ops.lamb_moments(gw, gd, gm, gv, ranges, rows, trust, None, c1, c2, EPS)
    for tb in ([(0, 10, 1.0, 0.0, 0), (9, 20, 1.0, 0.0, 1)], [(10, 20, 1.0, 0.0, 0), (5, 8, 1.0, 0.0, 1)], [(0, COUNT + 1, 1.0, 0.0, 0)], [],
               [(0, 10, 0.0, 0.0, 0)], [(0, 10, 1.0, -1.0, 0)], [(0, 10, 1.0, float("nan"), 0)], [(0, 10, 1.0, 0.0, N_TRUST)],
               [(0, 10, 1.0, 0.0, -2)], [(0, 10, 1.0, 0.0, 2 ** 20)]):
        big = torch.empty(4096, dtype=torch.uint8, device=DEV)
        with pytest.raises(VltfError):
            ops.lamb_moments(gw, gd, gm, gv, tb, rows, trust, big, c1, c2, EPS)
        with pytest.raises(VltfError):
            ops.lamb_moments_st(gw, gd, gm, gv, tb, rows, trust, big, st, EPS)
        with pytest.raises(VltfError):
            ops.lamb_apply(gw, gm, gv, tb, trust, LR, c1, c2, EPS)
        with pytest.raises(VltfError):
            ops.lamb_apply_st(gw, gm, gv, tb, trust, st, EPS)
    arr = (_ffi.LambRange * 65)()                                                  # 65 entries in ONE call (ops would cut them in two)
    for i in range(65):
        arr[i].begin, arr[i].end, arr[i].lr_mult, arr[i].decay, arr[i].trust_index = i, i + 1, 1.0, 0.0, -1
    big = torch.empty(65 * ops.LAMB_ROW_BYTES, dtype=torch.uint8, device=DEV)
    with pytest.raises(VltfError, match="ranges"):
        _ffi.call("vl_lamb_moments", gw.data_ptr(), gd.data_ptr(), gm.data_ptr(), gv.data_ptr(), COUNT, c1, c2, EPS, 0.0, None, 1.0, None,
                  arr, 65, rows.data_ptr(), trust.data_ptr(), N_TRUST, big.data_ptr(), big.numel(), ops.stream())
    with pytest.raises(VltfError, match="ranges"):
        _ffi.call("vl_lamb_apply", gw.data_ptr(), gm.data_ptr(), gv.data_ptr(), COUNT, LR, c1, c2, EPS, None, arr, 65, trust.data_ptr(),
                  N_TRUST, ops.stream())
    assert untouched() and bool((trust == -7.0).all())
    assert bytes(host(rows)) == b"\xab" * rows.numel()
    # ---- the word cleared: the same calls update
    skip.zero_()
    ops.lamb_moments(gw, gd, gm, gv, ranges, rows, trust, ws, c1, c2, EPS, 1.0, ss, skip=skip)
    ops.lamb_apply(gw, gm, gv, ranges, trust, LR, c1, c2, EPS, skip=skip)
    ins = torch.from_numpy(inside).to(DEV)
    live = ins.clone()
    live[ranges[NAN_G][0]:ranges[NAN_G][1]] = False
    assert not torch.equal(gw[live], wd[live]) and not torch.equal(gm[live], md[live]) and not torch.equal(gv[live], vd[live])
    assert bool((trust != -7.0).all())


# ---- 4. LRCNEngine -------------------------------------------------------------------------------------------------------------------------
def offsets_of(eng):
    out, off = {}, 0
    for name, shp in eng.specs:
        out[name] = (off, int(np.prod(shp)))
        off += int(np.prod(shp))
    return out


def check_lamb_steps(eng, step_fn, lrs, decay=0.0, mult=None, frozen=(), eps=EPS, bites=True, first_update=1):
    """Runs step_fn(i, lr) per lr.  After each step the reference is fed the engine's own pre-step w, m, v, its own get_grads() (the raw
    gradient: the launches never write g) and its own norm word:
    - m', v' are within one ulp of lamb_ref.moments (the fma);
    - u is formed from the engine's m', v' (just checked), so the ops-level bounds of the module docstring hold for lamb_trust() and w';
    - biases (rank 1) have trust exactly 1 and no decay; frozen variables are absent and keep their bits."""
    offs = offsets_of(eng)
    shapes = dict(eng.specs)
    for i, lr in enumerate(lrs):
        before, m0, v0 = eng.get_params(), host(eng.adam_m).copy(), host(eng.adam_v).copy()
        out = step_fn(i, lr)
        g, after, m1, v1, got = eng.get_grads(), eng.get_params(), host(eng.adam_m), host(eng.adam_v), eng.lamb_trust()
        assert math.isfinite(out["loss"]) and "reg_loss" not in out                # decoupled: no regulariser term anywhere
        sumsq = float(host(eng.ss)[0])
        raw = sum(float(np.sum(g[k].astype(np.float64) ** 2)) for k in g)
        assert abs(sumsq - raw) <= 1e-5 * raw and out["grad_norm"] == math.sqrt(sumsq)          # the norm of the RAW gradient
        sc = lamb_ref.clip_scale_f32(CLIP, sumsq)
        assert float(sc) < 1.0 or not bites                                     # the clip bites
        c1, c2 = lamb_ref.corrections(first_update + i)
        assert set(got) == set(offs) - set(frozen) and list(got) == [k for k, _ in eng.specs if k not in frozen]
        for k, (off, n) in offs.items():
            if k in frozen:
                assert np.array_equal(after[k], before[k]), k
                continue
            w0 = before[k].ravel()
            rm, rv = lamb_ref.moments(g[k].ravel(), m0[off:off + n], v0[off:off + n], sc)
            mk, vk = m1[off:off + n], v1[off:off + n]
            assert (np.abs(mk.astype(np.float64) - rm) <= ulp(rm)).all() and (np.abs(vk.astype(np.float64) - rv) <= ulp(rv)).all(), (i, k)
            d = decay if len(shapes[k]) >= 2 else 0.0
            u = lamb_ref.direction(w0, mk, vk, c1, c2, eps, d)
            if len(shapes[k]) >= 2:
                want = lamb_ref.trust(w0, u)
                tol = lamb_ref.trust_tol(n, d)
                print("step %d %s: trust %.9g, reference %.17g, bound %.3g" % (i, k, got[k], want, tol))
                assert want != 1.0 and abs(got[k] - want) <= tol * want, (i, k, got[k], want, tol)
            else:
                assert got[k] == 1.0, k
            check_range_update(w0, u, after[k].ravel(), lr, mult[k] if mult else 1.0, got[k], d, "step %d %s" % (i, k))
            assert not np.array_equal(after[k], before[k]), k


def lamb_cfg(**kw):
    return small_cfg(optimizer="adam", lamb=True, **kw)


@pytest.mark.parametrize("arith", ["f32", "bf16"])
def test_engine_three_steps(arith):
    """Weight decay on, a clip that bites, another lr every step."""
    from vltf_amd.engine import LRCNEngine
    p, batches = small_batches(3)
    eng = LRCNEngine(lamb_cfg(conv_math=arith, weight_decay=WD), max_clips=B, device=DEV)
    eng.load_params(p)
    assert eng.decay is None and eng.ss2 is None                                 # no regulariser launch under LAMB
    assert all(v == 1.0 for v in eng.lamb_trust().values())                      # before the first update
    check_lamb_steps(eng, lambda i, lr: eng.train_step_u8(*batches[i], lr=lr, clip_norm=CLIP, mean_bgr=MEAN), LRS, decay=WD)
    assert sorted(eng.get_opt_state()) == ["__optimizer__/adam_m", "__optimizer__/adam_v", "__optimizer__/step_count"]


def test_weight_decay_is_decoupled_and_lamb_is_not_adam():
    """One step from the same weights: with and without weight_decay the gradient handed out is the same bits (g was not regularised)
    and so are the moments, the weights differ; a plain Adam engine moves the weights differently and leaves the same moments."""
    from vltf_amd.engine import LRCNEngine
    p, batches = small_batches(1)
    engs = {}
    for name, cfg in (("wd", lamb_cfg(weight_decay=WD)), ("plain", lamb_cfg()), ("adam", small_cfg(optimizer="adam"))):
        e = engs[name] = LRCNEngine(cfg, max_clips=B, device=DEV)
        e.load_params(p)
        e.train_step_u8(*batches[0], lr=0.02, clip_norm=CLIP, mean_bgr=MEAN)
    ga, gb = engs["wd"].get_grads(), engs["plain"].get_grads()
    pa, pb, pc = (engs[k].get_params() for k in ("wd", "plain", "adam"))
    assert all(np.array_equal(ga[k], gb[k]) for k in ga)
    assert torch.equal(bits(engs["wd"].ss), bits(engs["plain"].ss))
    for a in ("wd", "adam"):
        assert torch.equal(bits(engs[a].adam_m), bits(engs["plain"].adam_m)) and torch.equal(bits(engs[a].adam_v), bits(engs["plain"].adam_v))
    shapes = dict(engs["wd"].specs)
    for k in pa:
        assert np.array_equal(pa[k], pb[k]) == (len(shapes[k]) < 2), k            # the biases carry no decay
        assert not np.array_equal(pb[k], pc[k]), k


def test_engine_refusals_checkpoints_and_off_allocates_nothing():
    from vltf_amd._ffi import VltfError
    from vltf_amd.engine import LRCNEngine
    for kw, msg in ((dict(lamb=True), "adam"), (dict(lamb=True, momentum=0.9), "adam"), (dict(optimizer="adam", lamb=1), "lamb"),
                    (dict(optimizer="adam", lamb=True, lamb_epsilon=0.0), "lamb_epsilon"),
                    (dict(optimizer="adam", lamb=True, lamb_epsilon=float("nan")), "lamb_epsilon"),
                    (dict(optimizer="adam", lamb_epsilon=1e-6), "lamb"), (dict(optimizer="adam", lamb=True, lars_eeta=0.02), "adam")):
        with pytest.raises(VltfError, match=msg):
            LRCNEngine(small_cfg(**kw), max_clips=B, device=DEV)
    off = LRCNEngine(small_cfg(optimizer="adam", weight_decay=WD), max_clips=B, device=DEV)
    assert off.lamb is None and off.decay is not None                            # off: Adam keeps the coupled L2
    with pytest.raises(VltfError, match="lamb"):
        off.lamb_trust()
    assert LRCNEngine(lamb_cfg(), max_clips=B, device=DEV, training=False).lamb is None
    on = LRCNEngine(lamb_cfg(lamb_epsilon=1e-5), max_clips=B, device=DEV)
    assert on.lamb_epsilon == 1e-5 and LRCNEngine(lamb_cfg(), max_clips=B, device=DEV).lamb_epsilon == 1e-6
    # an Adam checkpoint loads into a LAMB run and the other way round
    p, batches = small_batches(1)
    for src, dst in ((off, on), (on, off)):
        src.load_params(p)
        src.train_step_u8(*batches[0], lr=0.02, clip_norm=CLIP, mean_bgr=MEAN)
        state = src.get_opt_state()
        assert sorted(state) == ["__optimizer__/adam_m", "__optimizer__/adam_v", "__optimizer__/step_count"]
        assert dst.load_opt_state(state) == [] and dst.step_count == src.step_count
        assert torch.equal(bits(dst.adam_m), bits(src.adam_m)) and torch.equal(bits(dst.adam_v), bits(src.adam_v))


def test_stats_step_carries_the_trust_ratios():
    from vltf_amd.engine import LRCNEngine
    p, batches = small_batches(2)
    eng = LRCNEngine(lamb_cfg(weight_decay=WD, tensor_stats_interval=2), max_clips=B, device=DEV)
    eng.load_params(p)
    out = eng.train_step_u8(*batches[0], lr=0.02, clip_norm=CLIP, mean_bgr=MEAN)
    first = eng.lamb_trust()
    assert {n: d["lamb_trust"] for n, d in out["tensor_stats"].items()} == first and any(v != 1.0 for v in first.values())
    out = eng.train_step_u8(*batches[1], lr=0.02, clip_norm=CLIP, mean_bgr=MEAN)     # not a stats step: the report stays the first one's
    assert "tensor_stats" not in out and eng.lamb_trust() != first
    assert {n: d["lamb_trust"] for n, d in eng.tensor_stats().items()} == first
    plain = LRCNEngine(small_cfg(optimizer="adam", tensor_stats_interval=1), max_clips=B, device=DEV)
    plain.load_params(p)
    out = plain.train_step_u8(*batches[0], lr=0.02, clip_norm=CLIP, mean_bgr=MEAN)
    assert not any("lamb_trust" in d for d in out["tensor_stats"].values())


# ---- 5. composition ------------------------------------------------------------------------------------------------------------------------
def test_captured_lamb_step_equals_eager():
    """Step 1 is the warm-up, step 2 is captured and replayed, step 3 is a replay; lr changes every step.  Parameters, moments and the
    trust table are bit-equal after each step, and the graph's key needed nothing new."""
    from tests.test_step_graph_gpu import batch, pair, same_state, train_both
    eager, graph = pair(B, fpc=3, hid=8, opt="adam", lamb=True, weight_decay=WD)
    rng = np.random.default_rng(11)
    for step, lr in enumerate(LRS):
        train_both((eager, graph), batch(rng, B, 3), lr=lr, clip_norm=CLIP)
        same_state(eager, graph)
        assert torch.equal(bits(eager.adam_m), bits(graph.adam_m)) and bool(eager.adam_m.any())
        assert torch.equal(bits(eager.lamb["trust"]), bits(graph.lamb["trust"])) and torch.equal(eager.lamb["rows"], graph.lamb["rows"])
        assert eager.lamb_trust() == graph.lamb_trust() and any(v != 1.0 for v in graph.lamb_trust().values())
    assert len(graph._graphs) == 1


def test_lamb_with_frozen_layers():
    """train_from fc6, lr_mult 4: frozen variables keep their bits, their gradient range (NaN) is never read, their moments stay, and
    they are absent from lamb_trust(); the trained ones follow the rule with lr * mult * trust."""
    from vltf_amd.engine import LRCNEngine, is_regular
    p, batches = small_batches(2)
    eng = LRCNEngine(lamb_cfg(train_from="fc6", lr_mult=4.0, weight_decay=WD), max_clips=B, device=DEV)
    eng.load_params(p)
    frozen = set(eng.plan.frozen)
    assert frozen == {"dcnn/conv%d%s" % (i, k) for i in range(1, 6) for k in "Wb"}
    for k in frozen:
        off, n = eng.offsets[k]
        eng.adam_m[off:off + n] = 0.25
        eng.adam_v[off:off + n] = float("nan")
        eng.G[k].fill_(float("nan"))
    assert not any(n in frozen for n, _, _ in eng.lamb["segs"]) and not frozen & set(eng.lamb_trust())
    mult = {k: (1.0 if is_regular(k) else 4.0) for k in p}
    assert sorted(set(mult.values())) == [1.0, 4.0]
    check_lamb_steps(eng, lambda i, lr: eng.train_step_u8(*batches[i], lr=lr, clip_norm=CLIP, mean_bgr=MEAN), LRS[:2], decay=WD, mult=mult,
                     frozen=frozen)
    for k in frozen:
        off, n = eng.offsets[k]
        assert bool((eng.adam_m[off:off + n] == 0.25).all()) and bool(torch.isnan(eng.adam_v[off:off + n]).all()), k
        assert bool(torch.isnan(eng.g[off:off + n]).all()), k


def test_accumulated_update_is_the_update_of_the_summed_gradient():
    """accumulate 2: the first micro-step launches nothing new -- the weights, the moments and the trust table keep their bits -- and
    the update after the second equals, bit for bit, lamb_moments -> lamb_apply run here on copies of the weights and the moments of
    before with the summed gradient (g still holds it: the launches never write g)."""
    from vltf_amd import ops
    from vltf_amd.engine import LRCNEngine, lamb_corrections
    p, batches = small_batches(4)
    eng = LRCNEngine(lamb_cfg(weight_decay=WD, accumulate=2), max_clips=B, device=DEV)
    eng.load_params(p)
    for u, lr in enumerate(LRS[:2]):
        w0, m0, v0, t0 = eng.w.clone(), eng.adam_m.clone(), eng.adam_v.clone(), eng.lamb["trust"].clone()
        eng.train_step_u8(*batches[2 * u], lr=lr, clip_norm=CLIP, mean_bgr=MEAN, micro=(0, 2))
        torch.cuda.synchronize()
        assert torch.equal(bits(eng.w), bits(w0)) and torch.equal(bits(eng.adam_m), bits(m0)) and torch.equal(bits(eng.adam_v), bits(v0))
        assert torch.equal(bits(eng.lamb["trust"]), bits(t0)) and eng.step_count == u
        eng.train_step_u8(*batches[2 * u + 1], lr=lr, clip_norm=CLIP, mean_bgr=MEAN, micro=(1, 2))
        L = eng.lamb
        n = len(L["segs"])
        rows = torch.zeros(n * ops.LAMB_ROW_BYTES, dtype=torch.uint8, device=DEV)
        trust = torch.zeros(n, device=DEV)
        c1, c2 = lamb_corrections(u)
        ops.lamb_moments(w0, eng.g, m0, v0, L["ranges"], rows, trust, torch.empty_like(L["ws"]), c1, c2, EPS, CLIP, eng.ss, 1.0)
        ops.lamb_apply(w0, m0, v0, L["ranges"], trust, lr, c1, c2, EPS)
        assert torch.equal(bits(trust), bits(L["trust"])) and bool((trust != 1.0).all()) and torch.equal(rows, L["rows"])
        assert torch.equal(bits(eng.w), bits(w0)) and torch.equal(bits(eng.adam_m), bits(m0)) and torch.equal(bits(eng.adam_v), bits(v0))
        assert eng.step_count == u + 1


def test_graph_engine_two_steps():
    from tests import graph_cases as GC
    from tests.test_graph_gpu import device_feeds
    from vltf_amd._ffi import VltfError
    from vltf_amd.graph import GraphEngine
    case = GC.CASES["encdec_state"]()                   # two pipelines, one tower of 2-frame clips: the smallest of graph_cases
    pipes, ds = GC.specs_and_datasets(case)
    with pytest.raises(VltfError, match="adam"):
        GraphEngine(pipes, ds, case["V"], device=DEV, lamb=True)
    with pytest.raises(VltfError, match="lamb"):
        GraphEngine(pipes, ds, case["V"], device=DEV, optimizer="adam", lamb_epsilon=1e-6)
    with pytest.raises(VltfError, match="adam"):
        GraphEngine(pipes, ds, case["V"], device=DEV, optimizer="adam", lamb=True, lars_eeta=0.02)
    assert GraphEngine(pipes, ds, case["V"], device=DEV, optimizer="adam").lamb is None
    eng = GraphEngine(pipes, ds, case["V"], device=DEV, optimizer="adam", weight_decay=WD, lamb=True)
    assert eng.decay is None and eng.lamb_epsilon == 1e-6
    eng.load_params(eng.init_params(seed=case["seed"], well_scaled=True))
    raw, feeds = GC.inputs(case)
    fd = device_feeds(raw)
    eng.forward(fd)
    rows = eng.logits_host().shape[0]
    onehot = torch.tensor(O.labels_to_one_hot([[l] for l in np.random.default_rng(0).integers(0, case["V"], rows)], case["V"]), device=DEV)
    check_lamb_steps(eng, lambda i, lr: eng.train_step(fd, onehot, lr=lr, clip_norm=CLIP), LRS[:2], decay=WD, bites=False)
    assert sorted(eng.get_opt_state()) == ["__optimizer__/adam_m", "__optimizer__/adam_v", "__optimizer__/step_count"]


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
    cfg = NetConfig(image_shape=shape, num_classes=ncls, fpc=fpc, lstm_hidden=hid, optimizer="adam", weight_decay=0.01, lamb=True)
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
    ta, tb = eng.lamb_trust(), ref.lamb_trust()
    torch.cuda.synchronize()
    q.put(dict(same=all(np.array_equal(got[k], want[k]) for k in want) and all(o[0] == o[1] and o[2] == o[3] for o in outs),
               moved=all(not np.array_equal(want[k], p[k]) for k in want),
               m_same=bool(torch.equal(eng.adam_m.view(torch.int32), ref.adam_m.view(torch.int32))), m_set=bool(eng.adam_m.any()),
               v_same=bool(torch.equal(eng.adam_v.view(torch.int32), ref.adam_v.view(torch.int32))),
               trust_same=ta == tb, trust_set=any(v != 1.0 for v in ta.values()), outs=outs))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_one_rank_rccl_lamb_step():
    """Two LAMB steps under a one-rank process group equal the engine without data parallelism bit for bit, moments and trust table
    included (the launches run after the exchange, on the reduced gradient)."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    pr = ctx.Process(target=dp_worker, args=(free_port(), q))
    pr.start()
    pr.join(300)
    assert pr.exitcode == 0, "rank exited with %s" % pr.exitcode
    r = q.get(timeout=10)
    assert r["same"] and r["moved"] and r["m_same"] and r["m_set"] and r["v_same"] and r["trust_same"] and r["trust_set"], r


def test_lamb_resume_equals_uninterrupted(tmp_path, monkeypatch):
    """A run resumed from the end-of-epoch-1 checkpoint (weights + __optimizer__/adam_m, adam_v, step_count, as an Adam run's) ends with
    exactly the weights of the uninterrupted 2-epoch run -- and with other weights than the same run with plain Adam.  The interruption
    is after update 3 of 6: run_task writes checkpoints at epoch ends, and an epoch of this dataset is 3 batches."""
    monkeypatch.setenv("VLTF_PREFETCH", "0")
    monkeypatch.setenv("VLTF_CONV_MATH", "f32")
    from tests.test_host_workflow import make_dataset
    from tests.test_run_task_gpu import RAW, write_cfg
    from vltf_amd import run_task
    folder = str(tmp_path)
    train_path, _, _ = make_dataset(folder, "train.txt", shape=RAW, seed=1)

    def cfg(name, run, lamb=True, **kw):
        path = write_cfg(folder, name, train_path, "train", epochs=2, optimizer="adam", det=True, run=run, **kw)
        with open(path) as f:
            c = yaml.safe_load(f)
        c["run"]["train"].update(base_lr=0.01, weight_decay=0.01)
        if lamb:
            c["run"]["train"].update(lamb=True, lamb_epsilon=1e-6)
        with open(path, "w") as f:
            yaml.safe_dump(c, f)
        return path

    def final_weights(run):
        ck = sorted(glob.glob(os.path.join(folder, run, "checkpoints", "*.weights.npz")), key=os.path.getmtime)
        with np.load(ck[-1], allow_pickle=False) as z:
            return ck, {k: z[k] for k in z.files}

    run_task.main(cfg("a.yml", "runA"), seed=3)
    ck, full = final_weights("runA")
    assert len(ck) == 2 and int(full["__optimizer__/step_count"][0]) == 6
    assert sorted(k for k in full if k.startswith("__optimizer__/")) == ["__optimizer__/adam_m", "__optimizer__/adam_v",
                                                                        "__optimizer__/step_count"]
    first = ck[0][:-len(".weights.npz")]
    run_task.main(cfg("b.yml", "runA", resume=first), seed=77)
    _, resumed = final_weights("runA")
    assert int(resumed["__optimizer__/step_count"][0]) == 6
    for k in full:
        np.testing.assert_array_equal(resumed[k], full[k], err_msg=k)
    run_task.main(cfg("c.yml", "runC", lamb=False), seed=3)
    _, plain = final_weights("runC")
    assert not np.array_equal(plain["output_fc_w"], full["output_fc_w"])
