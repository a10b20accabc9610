"""LARS on the device (vl_lars_trust, vl_lars_apply, NetConfig.lars_eeta): the trust ratios of a vl_tensor_stats launch against
tests/lars_ref.py in float64, the update bit for bit against vl_momentum_apply with the rate formed on the host, the skip word and the
refusals, LRCNEngine (fp32 and the bf16 path, captured, with frozen layers, under accumulation), GraphEngine, one-rank RCCL and the
checkpoint of run_task.  Small shapes: a flat buffer of 70 K floats; 67x67x3 frames, 2 clips x 3 frames, hidden 8, 7 classes.

TRUST_TOL = 2^-22 relative: the device forms the ratio in double from fp64 sums of positive terms that are within N 2^-53 of exact
(negligible at these N), so its double and the reference's agree to ~1e-12, and two doubles that close round to floats at most one ulp
(2^-23 relative) apart; the reference is compared as a double, which adds the half ulp of the float it is compared with."""
import glob
import math
import os
import socket

import numpy as np
import pytest
import torch
import yaml

from oracle import lrcn_oracle as O
from tests import lars_ref
from tests.test_momentum_gpu import (B, CLIP, DEV, MEAN, MOM, bits, close, host, rule, small_batches, small_cfg, state_block)

pytestmark = pytest.mark.gpu
TRUST_TOL = 2.0 ** -22
EETA = 0.02
WD = 0.01
LRS = (0.5, 1.0, 0.25)

# ---- the flat buffer of the kernel tests ------------------------------------------------------------------------------------------------
COUNT = 70001
CHUNK = 16384                      # VL_STAT_CHUNK (asserted below)
# (begin, length): lengths 1, 3, 4, 5, 1023, 1025, CHUNK, CHUNK + 1; NaN-filled gaps before the first, between some, and behind the last
_LAYOUT = [(2, 1), (3, 3), (7, 4), (11, 5), (23, 1023), (1046, 1025), (7071, CHUNK), (23458, CHUNK + 1)]
SEGS = [(lo, lo + n) for lo, n in _LAYOUT]
ZERO_W, ZERO_G, NAN_G = 2, 4, 3    # the segment with all-zero w (length 4), all-zero g (length 1023), one NaN in g (length 5)
MULTS = [1.0, 0.25, 2.0, 3.0, 1.0, 0.5, 4.0, 1.0]
_BUF = {}


def flat_data():
    """w, g, accumulator on the host, made once, never written: N(0, 1) weights, 3 N(0, 1) gradients, NaN outside the segments."""
    if not _BUF:
        assert [hi - lo for lo, hi in SEGS] == [1, 3, 4, 5, 1023, 1025, CHUNK, CHUNK + 1] and SEGS[-1][1] < COUNT
        assert all(a[1] <= b[0] for a, b in zip(SEGS, SEGS[1:])) and any(a[1] < b[0] for a, b in zip(SEGS, SEGS[1:]))
        rng = np.random.default_rng(7)
        w = rng.standard_normal(COUNT).astype(np.float32)
        g = (3 * rng.standard_normal(COUNT)).astype(np.float32)
        a = rng.standard_normal(COUNT).astype(np.float32)
        inside = np.zeros(COUNT, bool)
        for lo, hi in SEGS:
            inside[lo:hi] = True
        for t in (w, g, a):
            t[~inside] = np.nan
        w[SEGS[ZERO_W][0]:SEGS[ZERO_W][1]] = 0.0
        g[SEGS[ZERO_G][0]:SEGS[ZERO_G][1]] = 0.0
        g[SEGS[NAN_G][0] + 2] = np.nan
        _BUF.update(w=w, g=g, a=a, inside=inside)
    return _BUF["w"], _BUF["g"], _BUF["a"], _BUF["inside"]


def on_device(x, offset):
    """x as a view that begins `offset` floats behind a 16-byte aligned address."""
    base = torch.zeros(x.size + offset, device=DEV)
    assert base.data_ptr() % 16 == 0
    v = base[offset:]
    v.copy_(torch.from_numpy(x).to(DEV))
    return v


def device_trust(w, g, decays, clip, gscale, eeta=EETA, eps=0.0):
    """tensor_stats over SEGS, the global sum of squares over SEGS, lars_trust -> (trust tensor, rows tensor, the sumsq word)."""
    from vltf_amd import ops
    assert ops.STAT_CHUNK == CHUNK
    n = len(SEGS)
    rows = torch.empty(n * ops.STAT_ROW_BYTES, dtype=torch.uint8, device=DEV)
    ws = torch.empty(ops.tensor_stats_ws_bytes(SEGS), dtype=torch.uint8, device=DEV)
    ops.tensor_stats(w, g, SEGS, rows, ws)
    ss, sws = torch.zeros(1, device=DEV), torch.empty(1024, device=DEV)
    live = [(lo, hi, 1.0) for k, (lo, hi) in enumerate(SEGS) if k != NAN_G]          # a finite norm: the NaN segment is left out of it
    ops.sumsq_tiers(g, live, ss, sws)
    trust = torch.full((n + 1,), float("nan"), device=DEV)
    trust[n] = -7.0
    rows_before = rows.clone()
    ops.lars_trust(rows, decays, trust, eeta, eps, clip, ss, gscale)
    assert torch.equal(rows, rows_before)                                          # read-only on the rows
    return trust, rows, ss


# ---- 1. trust values ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("decay", [0.0, 0.05], ids=["nodecay", "decay"])
@pytest.mark.parametrize("clip", [0.0, 1.0], ids=["noclip", "clip"])
@pytest.mark.parametrize("gscale", [1.0, 0.125])
def test_trust_values(gscale, clip, decay, offset):
    w, g, _, _ = flat_data()
    wd, gd = on_device(w, offset), on_device(g, offset)
    decays = [decay] * len(SEGS)
    trust, rows, ss = device_trust(wd, gd, decays, clip, gscale, eps=1e-6)
    got = host(trust)
    assert got[len(SEGS)] == -7.0                                               # n entries written, not one more
    sumsq = float(host(ss)[0])
    sc = lars_ref.clip_scale_f32(clip, sumsq, gscale)
    if clip > 0:
        assert float(sc) < 0.5 * gscale                                         # the clip bites
    for k, (lo, hi) in enumerate(SEGS):
        want = lars_ref.trust(w[lo:hi], g[lo:hi], EETA, 1e-6, decay, sc)
        print("segment %d [%d, %d): trust %.9g, reference %.17g" % (k, lo, hi, got[k], want))
        if k in (ZERO_W, ZERO_G, NAN_G):
            assert want == 1.0 and got[k] == 1.0, k
        else:
            assert want != 1.0 and abs(float(got[k]) - want) <= TRUST_TOL * want, (k, got[k], want)


def test_trust_more_segments_than_one_launch_takes():
    """70 one-element segments: two launches over consecutive slices of the rows, of the decays and of the trust table."""
    from vltf_amd import ops
    n = 70
    rng = np.random.default_rng(3)
    w, g = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    wd, gd = torch.from_numpy(w).to(DEV), torch.from_numpy(g).to(DEV)
    segs = [(i, i + 1) for i in range(n)]
    rows = torch.empty(n * ops.STAT_ROW_BYTES, dtype=torch.uint8, device=DEV)
    ops.tensor_stats(wd, gd, segs, rows, torch.empty(ops.tensor_stats_ws_bytes(segs), dtype=torch.uint8, device=DEV))
    decays = [0.001 * i for i in range(n)]
    trust = torch.zeros(n, device=DEV)
    ops.lars_trust(rows, decays, trust, EETA)
    got = host(trust)
    for i in range(n):
        want = lars_ref.trust(w[i:i + 1], g[i:i + 1], EETA, 0.0, decays[i])
        assert abs(float(got[i]) - want) <= TRUST_TOL * want, i


# ---- 2. the update, bit for bit ------------------------------------------------------------------------------------------------------------
LR = 0.0123
# every segment a range; two of them with trust 1 by index -1 (the others read the device table)
RANGES = [(lo, hi, MULTS[k], -1 if k in (1, 5) else k) for k, (lo, hi) in enumerate(SEGS)]


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("st", [False, True], ids=["eager", "st"])
@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
def test_update_equals_momentum_apply_with_the_host_rate(nesterov, st, offset):
    """For every range, w and the accumulator are what vl_momentum_apply gives on copies of the buffers through the single tier
    {begin, end, 1.0} with lr = float32(float32(lr * mult) * trust_k), trust_k the device's own table read back; the NaN gaps keep
    their bits in w and in the accumulator (and g, NaN there, is never loaded)."""
    from vltf_amd import ops
    w, g, a, inside = flat_data()
    wd, gd, ad = on_device(w, offset), on_device(g, offset), on_device(a, offset)
    clip = 1.0
    trust, _, ss = device_trust(wd, gd, [0.05] * len(SEGS), clip, 1.0)
    tr = host(trust)
    gw, ga = on_device(w, offset), on_device(a, offset)                          # (clone() would realign: fresh views at the offset)
    if st:
        ops.lars_apply_st(gw, gd, ga, RANGES, trust, state_block(7, LR), MOM, nesterov, clip, ss)
    else:
        ops.lars_apply(gw, gd, ga, RANGES, trust, LR, MOM, nesterov, clip, ss)
    ins = torch.from_numpy(inside).to(DEV)
    assert torch.equal(bits(gw)[~ins], bits(wd)[~ins]) and torch.equal(bits(ga)[~ins], bits(ad)[~ins])
    assert bool(torch.isnan(gw[~ins]).all()) and bool(torch.isnan(ga[~ins]).all())
    for k, (lo, hi, mult, ti) in enumerate(RANGES):
        t = 1.0 if ti < 0 else tr[ti]
        lr_k = float(lars_ref.lr_k(LR, mult, t))
        ww, wa = on_device(w, offset), on_device(a, offset)
        if st:
            ops.momentum_apply_st(ww, gd, wa, state_block(7, lr_k), MOM, nesterov, clip, ss, tiers=[(lo, hi, 1.0)])
        else:
            ops.momentum_apply(ww, gd, wa, lr_k, MOM, nesterov, clip, ss, tiers=[(lo, hi, 1.0)])
        assert torch.equal(bits(gw[lo:hi]), bits(ww[lo:hi])) and torch.equal(bits(ga[lo:hi]), bits(wa[lo:hi])), (k, lo, hi, mult, ti)
        if k != NAN_G:
            assert bool(torch.isfinite(gw[lo:hi]).all()) and not torch.equal(gw[lo:hi], wd[lo:hi]), k
    # the table does something: a weight range moved by another amount than it would with trust 1
    k = 6
    lo, hi = SEGS[k]
    assert tr[k] != 1.0 and 0.0 < tr[k] < 1.0
    pw, pa = on_device(w, offset), on_device(a, offset)
    ops.momentum_apply(pw, gd, pa, LR, MOM, nesterov, clip, ss, tiers=[(lo, hi, MULTS[k])])
    assert torch.equal(bits(pa[lo:hi]), bits(ga[lo:hi])) and not torch.equal(pw[lo:hi], gw[lo:hi])      # the accumulator never sees the rate


def test_update_more_ranges_than_one_launch_takes():
    """70 ranges: two launches, both indexing the one trust table."""
    from vltf_amd import ops
    n = 70
    gen = torch.Generator(device="cpu").manual_seed(1)
    w, g, a = (torch.randn(4 * n, generator=gen).to(DEV) for _ in range(3))
    trust = (torch.rand(n, generator=gen) + 0.5).to(DEV)
    ranges = [(4 * i, 4 * i + 3, 1.0, i) for i in range(n)]
    gw, ga = w.clone(), a.clone()
    ops.lars_apply(gw, g, ga, ranges, trust, LR, MOM)
    tr = host(trust)
    for lo, hi, _, i in ranges:
        ww, wa = w.clone(), a.clone()
        ops.momentum_apply(ww, g, wa, float(lars_ref.lr_k(LR, 1.0, tr[i])), MOM, tiers=[(lo, hi, 1.0)])
        assert torch.equal(bits(gw[lo:hi]), bits(ww[lo:hi])) and torch.equal(bits(ga[lo:hi]), bits(wa[lo:hi])), i
        assert torch.equal(bits(gw[hi:hi + 1]), bits(w[hi:hi + 1]))                 # the one-element gaps


# ---- 3. skip word and argument checks -----------------------------------------------------------------------------------------------------
def test_skip_word_and_argument_checks():
    from vltf_amd import _ffi, ops
    from vltf_amd._ffi import VltfError
    w, g, a, inside = flat_data()
    wd, gd, ad = on_device(w, 0), on_device(g, 0), on_device(a, 0)
    trust, rows, ss = device_trust(wd, gd, [0.0] * len(SEGS), 1.0, 1.0)
    trust = trust[:len(SEGS)].clone()
    skip = torch.ones(1, dtype=torch.int32, device=DEV)
    gw, ga = wd.clone(), ad.clone()
    st = state_block(0, LR)
    for nesterov in (False, True):
        ops.lars_apply(gw, gd, ga, RANGES, trust, LR, MOM, nesterov, 1.0, ss, skip=skip)
        ops.lars_apply_st(gw, gd, ga, RANGES, trust, st, MOM, nesterov, 1.0, ss, skip=skip)
    assert torch.equal(bits(gw), bits(wd)) and torch.equal(bits(ga), bits(ad))
    # ---- lars_trust
    n = len(SEGS)
    out = torch.zeros(n, device=DEV)
    for eeta, eps in ((0.0, 0.0), (-1.0, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (EETA, -1.0), (EETA, float("nan")), (EETA, float("inf"))):
        with pytest.raises(VltfError):
            ops.lars_trust(rows, [0.0] * n, out, eeta, eps)
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(VltfError, match="decay"):
            ops.lars_trust(rows, [0.0] * (n - 1) + [bad], out, EETA)
    with pytest.raises(VltfError):
        ops.lars_trust(rows, [], out, EETA)                                        # no segment
    with pytest.raises(VltfError):
        ops.lars_trust(None, [0.0] * n, out, EETA)                                 # null rows
    with pytest.raises(VltfError):
        ops.lars_trust(rows, [0.0] * n, out[:n - 1], EETA)                         # a trust table too small
    with pytest.raises(VltfError):
        ops.lars_trust(rows, [0.0] * (n + 1), torch.zeros(n + 1, device=DEV), EETA)    # more segments than rows
    for n_segs in (0, 65):                                                         # the entry point itself: 1 .. 64 per launch
        with pytest.raises(VltfError, match="segments"):
            _ffi.call("vl_lars_trust", rows.data_ptr(), n_segs, EETA, 0.0, (_ffi.f32 * 65)(), 0.0, None, 1.0, out.data_ptr(), ops.stream())
    assert not bool(out.any())                                                     # a refused call launched nothing
    # ---- lars_apply
    for m in (0.0, 1.0, -0.5, 1.5, float("nan")):
        with pytest.raises(VltfError, match="momentum"):
            ops.lars_apply(gw, gd, ga, RANGES, trust, LR, m)
        with pytest.raises(VltfError, match="momentum"):
            ops.lars_apply_st(gw, gd, ga, RANGES, trust, st, m)
    with pytest.raises(VltfError):
        ops.lars_apply(gw, gd, None, RANGES, trust, LR, MOM)                       # a null accumulator
    with pytest.raises(VltfError):
        ops.lars_apply(gw, gd, ga[:-1], RANGES, trust, LR, MOM)                    # an accumulator of another size
    with pytest.raises(VltfError):
        ops.lars_apply_st(gw, gd, ga, RANGES, trust, None, MOM)                    # no step state
    with pytest.raises(VltfError):
        ops.lars_apply(gw, gd, ga, RANGES, None, LR, MOM)                          # indices, and no table to index
    for table in ([(0, 10, 1.0, 0), (9, 20, 1.0, 1)], [(10, 20, 1.0, 0), (5, 8, 1.0, 1)], [(0, COUNT + 1, 1.0, 0)], [], [(0, 10, 0.0, 0)],
                  [(0, 10, 1.0, n)], [(0, 10, 1.0, -2)], [(0, 10, 1.0, 2 ** 20)]):
        with pytest.raises(VltfError):
            ops.lars_apply(gw, gd, ga, table, trust, LR, MOM)
        with pytest.raises(VltfError):
            ops.lars_apply_st(gw, gd, ga, table, trust, st, MOM)
    arr = (_ffi.LarsRange * 65)()                                                  # 65 entries in ONE call (ops would cut them in two)
    for i in range(65):
        arr[i].begin, arr[i].end, arr[i].lr_mult, arr[i].trust_index = i, i + 1, 1.0, -1
    with pytest.raises(VltfError, match="ranges"):
        _ffi.call("vl_lars_apply", gw.data_ptr(), gd.data_ptr(), ga.data_ptr(), COUNT, LR, MOM, 0, 0.0, None, 1.0, None, arr, 65,
                  trust.data_ptr(), n, ops.stream())
    with pytest.raises(VltfError, match="ranges"):
        _ffi.call("vl_lars_apply_st", gw.data_ptr(), gd.data_ptr(), ga.data_ptr(), COUNT, st.data_ptr(), MOM, 0, 0.0, None, 1.0, None, arr, 65,
                  trust.data_ptr(), n, ops.stream())
    torch.cuda.synchronize()
    assert torch.equal(bits(gw), bits(wd)) and torch.equal(bits(ga), bits(ad))
    skip.zero_()                                                                   # the word cleared: the same call updates
    ops.lars_apply(gw, gd, ga, RANGES, trust, LR, MOM, False, 1.0, ss, skip=skip)
    ins = torch.from_numpy(inside).to(DEV)
    live = ins.clone()
    live[SEGS[NAN_G][0]:SEGS[NAN_G][1]] = False
    assert not torch.equal(gw[live], wd[live]) and not torch.equal(ga[live], ad[live])


# ---- 4. LRCNEngine -------------------------------------------------------------------------------------------------------------------------
def offsets_of(eng):
    out, off = {}, 0
    for name, shp in eng.specs:
        out[name] = (off, int(np.prod(shp)))
        off += int(np.prod(shp))
    return out


def check_lars_steps(eng, step_fn, lrs, nesterov, decay=0.0, mult=None, frozen=(), eeta=EETA, eps=0.0, bites=True):
    """Runs step_fn(i, lr) per lr.  After each step:
    - eng.lars_trust() matches lars_ref.trust of the parameters read BEFORE the step and the engine's own RAW gradient.  The engine hands
      out the regularised gradient g' = fl(g + decay w) (one fp32 fma: |g' - (g + decay w)| <= 2^-24 |g'| per element), so the raw
      gradient recovered on the host in float64, g' - decay w, is off by at most 2^-24 |g'| in norm, i.e. 2^-24 |g'| / |g| relative to
      the raw norm; the ratio's relative sensitivity to that norm is gn / (gn + decay wn + eps) <= 1.  Bound per variable:
      TRUST_TOL + 2^-24 |g'| / |g|  (TRUST_TOL alone without weight decay).  The clip scale is formed from the device's own norm word.
    - biases (rank 1) have trust exactly 1; frozen variables are absent and keep their bits.
    - parameters and accumulator follow the float64 momentum rule with lr * mult * reference trust, to the tolerance of
      tests/test_momentum_gpu.py::check_steps (`close`)."""
    offs = offsets_of(eng)
    shapes = dict(eng.specs)
    acc = {k: np.zeros(n) for k, (off, n) in offs.items()}
    d32 = float(np.float32(decay))
    for i, lr in enumerate(lrs):
        before = eng.get_params()
        out = step_fn(i, lr)
        g, after, mom, got = eng.get_grads(), eng.get_params(), host(eng.mom), eng.lars_trust()
        assert math.isfinite(out["loss"])
        sc = lars_ref.clip_scale_f32(CLIP, float(host(eng.ss)[0]))
        assert float(sc) < 1.0 or not bites                                     # the clip bites
        assert set(got) == set(offs) - set(frozen) and list(got) == [k for k, _ in eng.specs if k not in frozen]
        for k, (off, n) in offs.items():
            if k in frozen:
                assert np.array_equal(after[k], before[k]), k
                continue
            w0, gk = before[k].ravel().astype(np.float64), g[k].ravel().astype(np.float64)
            if len(shapes[k]) >= 2:
                raw = gk - d32 * w0 if decay else gk
                want = lars_ref.trust(w0, raw, eeta, eps, decay, sc)
                tol = TRUST_TOL + (2.0 ** -24 * np.linalg.norm(gk) / np.linalg.norm(raw) if decay else 0.0)
                print("step %d %s: trust %.9g, reference %.17g, bound %.3g" % (i, k, got[k], want, tol))
                assert want != 1.0 and abs(got[k] - want) <= tol * want, (i, k, got[k], want, tol)
            else:
                want = 1.0
                assert got[k] == 1.0, k
            m = mult[k] if mult else 1.0
            want_w, acc[k] = rule(w0, acc[k], gk, lr * m * want, float(sc), nesterov)
            close(after[k].ravel(), want_w, "param %s step %d" % (k, i))
            close(mom[off:off + n], acc[k], "accumulator %s step %d" % (k, i))
            assert not np.array_equal(after[k], before[k]), k


@pytest.mark.parametrize("arith,nesterov", [("f32", False), ("f32", True), ("bf16", False)], ids=["f32", "f32-nesterov", "bf16"])
def test_engine_three_steps(arith, nesterov):
    """Weight decay on, a clip that bites, another lr every step."""
    from vltf_amd.engine import LRCNEngine
    p, batches = small_batches(3)
    eng = LRCNEngine(small_cfg(conv_math=arith, momentum=MOM, nesterov=nesterov, weight_decay=WD, lars_eeta=EETA, lars_epsilon=1e-9),
                     max_clips=B, device=DEV)
    eng.load_params(p)
    assert all(v == 1.0 for v in eng.lars_trust().values())                      # before the first update
    check_lars_steps(eng, lambda i, lr: eng.train_step_u8(*batches[i], lr=lr, clip_norm=CLIP, mean_bgr=MEAN), LRS, nesterov, decay=WD,
                     eps=1e-9)
    assert sorted(eng.get_opt_state()) == ["__optimizer__/momentum", "__optimizer__/step_count"]      # no state of its own


def test_engine_refusals_and_off_allocates_nothing():
    from vltf_amd._ffi import VltfError
    from vltf_amd.engine import LRCNEngine
    for kw, msg in ((dict(lars_eeta=EETA), "momentum"), (dict(lars_eeta=EETA, optimizer="adam"), "adam"),
                    (dict(momentum=MOM, lars_eeta=-1.0), "lars_eeta"), (dict(momentum=MOM, lars_eeta=float("nan")), "lars_eeta"),
                    (dict(momentum=MOM, lars_eeta=EETA, lars_epsilon=-1.0), "lars_epsilon"),
                    (dict(momentum=MOM, lars_eeta=EETA, lars_epsilon=float("inf")), "lars_epsilon")):
        with pytest.raises(VltfError, match=msg):
            LRCNEngine(small_cfg(**kw), max_clips=B, device=DEV)
    off = LRCNEngine(small_cfg(momentum=MOM), max_clips=B, device=DEV)
    assert off.lars is None
    with pytest.raises(VltfError, match="lars_eeta"):
        off.lars_trust()
    assert LRCNEngine(small_cfg(momentum=MOM, lars_eeta=EETA), max_clips=B, device=DEV, training=False).lars is None


def test_stats_step_carries_the_trust_ratios():
    from vltf_amd.engine import LRCNEngine
    p, batches = small_batches(2)
    eng = LRCNEngine(small_cfg(momentum=MOM, weight_decay=WD, lars_eeta=EETA, tensor_stats_interval=2), max_clips=B, device=DEV)
    eng.load_params(p)
    out = eng.train_step_u8(*batches[0], lr=0.5, clip_norm=CLIP, mean_bgr=MEAN)
    first = eng.lars_trust()
    assert {n: d["lars_trust"] for n, d in out["tensor_stats"].items()} == first and any(v != 1.0 for v in first.values())
    out = eng.train_step_u8(*batches[1], lr=0.5, clip_norm=CLIP, mean_bgr=MEAN)      # not a stats step: the report stays the first one's
    assert "tensor_stats" not in out and eng.lars_trust() != first
    assert {n: d["lars_trust"] for n, d in eng.tensor_stats().items()} == first
    plain = LRCNEngine(small_cfg(momentum=MOM, tensor_stats_interval=1), max_clips=B, device=DEV)
    plain.load_params(p)
    out = plain.train_step_u8(*batches[0], lr=0.5, clip_norm=CLIP, mean_bgr=MEAN)
    assert not any("lars_trust" in d for d in out["tensor_stats"].values())


# ---- 5. composition ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
def test_captured_lars_step_equals_eager(nesterov):
    """Step 1 is the warm-up, step 2 is captured and replayed, step 3 is a replay; lr changes every step.  Parameters, accumulator
    and the trust table are bit-equal after each step, and the graph's key needed nothing new."""
    from tests.test_step_graph_gpu import batch, pair, same_state, train_both
    eager, graph = pair(B, fpc=3, hid=8, momentum=MOM, nesterov=nesterov, weight_decay=WD, lars_eeta=EETA)
    rng = np.random.default_rng(11)
    for step, lr in enumerate(LRS):
        train_both((eager, graph), batch(rng, B, 3), lr=lr, clip_norm=CLIP)
        same_state(eager, graph)
        assert torch.equal(bits(eager.mom), bits(graph.mom)) and bool(eager.mom.any())
        assert torch.equal(bits(eager.lars["trust"]), bits(graph.lars["trust"]))
        assert eager.lars_trust() == graph.lars_trust() and any(v != 1.0 for v in graph.lars_trust().values())
    assert len(graph._graphs) == 1
    plain = pair(B, fpc=3, hid=8, momentum=MOM, nesterov=nesterov, weight_decay=WD)[0]        # and LARS changes the weights
    rng = np.random.default_rng(11)
    for lr in LRS:
        plain.train_step_u8(**batch(rng, B, 3), lr=lr, clip_norm=CLIP, mean_bgr=MEAN)
    pa, pb = plain.get_params(), eager.get_params()
    assert any(not np.array_equal(pa[k], pb[k]) for k in pa)


def test_lars_with_frozen_layers():
    """train_from fc6, lr_mult 4: frozen variables keep their bits, their gradient range (NaN) is never read, and they are absent from
    lars_trust(); the trained ones follow the rule with lr * mult * trust."""
    from vltf_amd.engine import LRCNEngine, is_regular
    p, batches = small_batches(2)
    eng = LRCNEngine(small_cfg(momentum=MOM, train_from="fc6", lr_mult=4.0, weight_decay=WD, lars_eeta=EETA), max_clips=B, device=DEV)
    eng.load_params(p)
    frozen = set(eng.plan.frozen)
    assert frozen == {"dcnn/conv%d%s" % (i, k) for i in range(1, 6) for k in "Wb"}
    for k in frozen:
        off, n = eng.offsets[k]
        eng.mom[off:off + n] = 0.25
        eng.G[k].fill_(float("nan"))
    assert not any(n in frozen for n, _, _ in eng.lars["segs"]) and not frozen & set(eng.lars_trust())
    mult = {k: (1.0 if is_regular(k) else 4.0) for k in p}
    assert sorted(set(mult.values())) == [1.0, 4.0]
    mom0 = host(eng.mom).copy()                       # check_lars_steps starts the trained accumulators at zero
    assert all(not mom0[off:off + n].any() for k, (off, n) in eng.offsets.items() if k not in frozen)
    check_lars_steps(eng, lambda i, lr: eng.train_step_u8(*batches[i], lr=lr, clip_norm=CLIP, mean_bgr=MEAN), LRS[:2], False, decay=WD,
                     mult=mult, frozen=frozen)
    for k in frozen:
        off, n = eng.offsets[k]
        assert bool((eng.mom[off:off + n] == 0.25).all()), k
        assert bool(torch.isnan(eng.g[off:off + n]).all()), k


def test_accumulated_update_is_the_update_of_the_summed_gradient():
    """accumulate 2, no weight decay (so g still holds the raw sum after the update): the first micro-step launches nothing new -- the
    weights, the accumulator and the trust table keep their bits -- and the update after the second equals, bit for bit, tensor_stats
    -> lars_trust -> lars_apply run here on copies of the weights and the accumulator of before with the summed gradient."""
    from vltf_amd import ops
    from vltf_amd.engine import LRCNEngine
    p, batches = small_batches(4)
    eng = LRCNEngine(small_cfg(momentum=MOM, lars_eeta=EETA, accumulate=2), max_clips=B, device=DEV)
    eng.load_params(p)
    for u, lr in enumerate(LRS[:2]):
        w0, a0, t0 = eng.w.clone(), eng.mom.clone(), eng.lars["trust"].clone()
        eng.train_step_u8(*batches[2 * u], lr=lr, clip_norm=CLIP, mean_bgr=MEAN, micro=(0, 2))
        torch.cuda.synchronize()
        assert torch.equal(bits(eng.w), bits(w0)) and torch.equal(bits(eng.mom), bits(a0)) and torch.equal(bits(eng.lars["trust"]), bits(t0))
        assert eng.step_count == u
        eng.train_step_u8(*batches[2 * u + 1], lr=lr, clip_norm=CLIP, mean_bgr=MEAN, micro=(1, 2))
        L = eng.lars
        n = len(L["segs"])
        rows = torch.empty(n * ops.STAT_ROW_BYTES, dtype=torch.uint8, device=DEV)
        ops.tensor_stats(w0, eng.g, L["segs"], rows, torch.empty(ops.tensor_stats_ws_bytes(L["segs"]), dtype=torch.uint8, device=DEV))
        trust = torch.zeros(n, device=DEV)
        ops.lars_trust(rows, L["decays"], trust, EETA, 0.0, CLIP, eng.ss, 1.0)
        ops.lars_apply(w0, eng.g, a0, L["ranges"], trust, lr, MOM, False, CLIP, eng.ss, 1.0)
        assert torch.equal(bits(trust), bits(L["trust"])) and bool((trust != 1.0).all())
        assert torch.equal(bits(eng.w), bits(w0)) and torch.equal(bits(eng.mom), bits(a0))
        assert eng.step_count == u + 1


def test_graph_engine_two_steps():
    from tests import graph_cases as GC
    from tests.test_graph_gpu import device_feeds
    from vltf_amd._ffi import VltfError
    from vltf_amd.graph import GraphEngine
    case = GC.CASES["encdec_state"]()                   # two pipelines, one tower of 2-frame clips: the smallest of graph_cases
    pipes, ds = GC.specs_and_datasets(case)
    with pytest.raises(VltfError, match="adam"):
        GraphEngine(pipes, ds, case["V"], device=DEV, optimizer="adam", lars_eeta=EETA)
    with pytest.raises(VltfError, match="momentum"):
        GraphEngine(pipes, ds, case["V"], device=DEV, lars_eeta=EETA)
    assert GraphEngine(pipes, ds, case["V"], device=DEV, momentum=MOM).lars is None
    eng = GraphEngine(pipes, ds, case["V"], device=DEV, momentum=MOM, nesterov=True, weight_decay=WD, lars_eeta=EETA)
    eng.load_params(eng.init_params(seed=case["seed"], well_scaled=True))
    raw, feeds = GC.inputs(case)
    fd = device_feeds(raw)
    eng.forward(fd)
    rows = eng.logits_host().shape[0]
    onehot = torch.tensor(O.labels_to_one_hot([[l] for l in np.random.default_rng(0).integers(0, case["V"], rows)], case["V"]), device=DEV)
    check_lars_steps(eng, lambda i, lr: eng.train_step(fd, onehot, lr=lr, clip_norm=CLIP), LRS[:2], True, decay=WD, bites=False)
    assert sorted(eng.get_opt_state()) == ["__optimizer__/momentum", "__optimizer__/step_count"]


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
    cfg = NetConfig(image_shape=shape, num_classes=ncls, fpc=fpc, lstm_hidden=hid, momentum=0.9, weight_decay=0.01, lars_eeta=0.02)
    eng = LRCNEngine(cfg, max_clips=clips, device="cuda:0", dp=dp.GradAllReduce(always=True))
    ref = LRCNEngine(cfg, max_clips=clips, device="cuda:0")
    eng.load_params(p)
    ref.load_params(p)
    outs = []
    for lr in (0.5, 0.2):
        a = eng.train_step_u8(frames, onehot, lr=lr, clip_norm=0.5, mean_bgr=MEAN)
        b = ref.train_step_u8(frames, onehot, lr=lr, clip_norm=0.5, mean_bgr=MEAN)
        outs.append((a["loss"], b["loss"], a["grad_norm"], b["grad_norm"]))
    got, want = eng.get_params(), ref.get_params()
    ta, tb = eng.lars_trust(), ref.lars_trust()
    torch.cuda.synchronize()
    q.put(dict(same=all(np.array_equal(got[k], want[k]) for k in want) and all(o[0] == o[1] and o[2] == o[3] for o in outs),
               moved=all(not np.array_equal(want[k], p[k]) for k in want),
               mom_same=bool(torch.equal(eng.mom.view(torch.int32), ref.mom.view(torch.int32))), mom_set=bool(eng.mom.any()),
               trust_same=ta == tb, trust_set=any(v != 1.0 for v in ta.values()), outs=outs))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_one_rank_rccl_lars_step():
    """Two LARS steps under a one-rank process group equal the engine without data parallelism bit for bit, accumulator and trust
    table included (the norms are taken after the exchange, of the reduced gradient)."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    pr = ctx.Process(target=dp_worker, args=(free_port(), q))
    pr.start()
    pr.join(300)
    assert pr.exitcode == 0, "rank exited with %s" % pr.exitcode
    r = q.get(timeout=10)
    assert r["same"] and r["moved"] and r["mom_same"] and r["mom_set"] and r["trust_same"] and r["trust_set"], r


def test_lars_resume_equals_uninterrupted(tmp_path, monkeypatch):
    """LARS keeps no state: a run resumed from the end-of-epoch-1 checkpoint (weights + __optimizer__/momentum, nothing new) ends with
    exactly the weights of the uninterrupted 2-epoch run -- and with other weights than the same run without LARS.  The interruption
    is after update 3 of 6, not after update 2: run_task writes checkpoints at epoch ends, and an epoch of this dataset is 3 batches."""
    monkeypatch.setenv("VLTF_PREFETCH", "0")
    monkeypatch.setenv("VLTF_CONV_MATH", "f32")
    from tests.test_host_workflow import make_dataset
    from tests.test_run_task_gpu import RAW, write_cfg
    from vltf_amd import run_task
    folder = str(tmp_path)
    train_path, _, _ = make_dataset(folder, "train.txt", shape=RAW, seed=1)

    def cfg(name, run, lars=True, **kw):
        path = write_cfg(folder, name, train_path, "train", epochs=2, det=True, run=run, **kw)
        with open(path) as f:
            c = yaml.safe_load(f)
        c["run"]["train"].update(momentum=0.9, base_lr=0.05, weight_decay=0.001)
        if lars:
            c["run"]["train"].update(lars_eeta=0.02, lars_epsilon=0.0)
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
    assert sorted(k for k in full if k.startswith("__optimizer__/")) == ["__optimizer__/momentum", "__optimizer__/step_count"]
    first = ck[0][:-len(".weights.npz")]
    run_task.main(cfg("b.yml", "runA", resume=first), seed=77)
    _, resumed = final_weights("runA")
    assert int(resumed["__optimizer__/step_count"][0]) == 6
    for k in full:
        np.testing.assert_array_equal(resumed[k], full[k], err_msg=k)
    run_task.main(cfg("c.yml", "runC", lars=False), seed=3)
    _, plain = final_weights("runC")
    assert not np.array_equal(plain["output_fc_w"], full["output_fc_w"])
