"""The CPU half of tests/test_pool_geometry_gpu.py (no GPU needed).  Coverage: at 256 and at 64 compute units the case lists of
tests/pool_plan.py reach every launcher branch they are there for, by the restated launch arithmetic.  Discrimination: the very check
functions of the GPU half run here against a numpy float32 stand-in with the `ops` signatures (the oracle evaluated in float32, cut
into bands and channel ranges as the plan says) and pass -- which also shows that float32 arithmetic stays inside every tolerance
and the arg-max near-tie cap on each chosen input -- and fail for each defect the harness is there to catch."""
import numpy as np
import pytest
import torch

from oracle import lrcn_oracle as O
from tests import pool_plan as P
from tests import test_pool_geometry_gpu as G
from tests.test_ops_gpu import nchw, nhwc

CUS = (256, 64)
F32 = np.float32


# ---- coverage -----------------------------------------------------------------------------------------------------------------------
def plb(case, cus):
    return P.plb_plan(case.n, case.c, case.h, case.w, case.ph, case.dh, cus, case.beta, case.ranges)


def plb_c8(case, cus):
    return P.plb_c8_plan(case.n, case.c, case.h, case.w, case.ph, case.dh, cus, case.ranges)


def lpf(case, cus, c8=False):
    case = P.resolve(case, cus)
    return P.lpf_plan(case.n, case.c, case.h, case.w, case.ph, cus, c8, case.ranges)


@pytest.mark.parametrize("cus", CUS)
def test_pool_lrn_bwd_cases_reach_their_branches(cus):
    assert all(plb(c, cus).form == "chunked" for c in P.PLB_CHUNKED)
    assert plb(P.Plb(2, 16, 5, 63, 0, 0), cus).grid == (1, 1, 2)
    assert plb(P.Plb(2, 21, 7, 120, 1, 2), cus).grid == (2, 2, 2) and 21 % 16 == 5            # two 512-pixel bands, ragged second block
    by_beta = [c for c in P.PLB_CHUNKED if c.beta != 0.75]
    assert {c.beta for c in by_beta} == {0.5, 1.0} and all(plb(c._replace(beta=0.75), cus).form == "stream" for c in by_beta)
    (s5, c5), (s16, c16) = P.PLB_BOUNDARY
    mow = [P.stream_rows(c.w)[1] * P.pool_out(c.w) for c in (s5, c5, s16, c16)]
    assert mow == [150, 155, 140, 145] and 5 * 153 <= 768 < 5 * 154 and 16 * 144 <= 2304 < 16 * 145
    assert plb(s5, cus)[:3] == ("stream", 5, 3) and plb(s16, cus)[:3] == ("stream", 16, 9)
    assert plb(c5, cus).form == plb(c16, cus).form == "chunked" and (s5.c, c5.c, s16.c, c16.c) == (16, 16, 7, 7)
    assert plb(s5._replace(c=17), cus).form == "chunked"                                    # 150 > 144: only the 5-channel chunks take it
    assert plb(P.PLB_REFUSED, cus).form == "refuse" and plb(P.PLB_REFUSED._replace(w=300), cus).form == "chunked"
    assert P.PLB_REFUSED._replace(w=300) in P.PLB_CHUNKED
    plans = {c: plb(c, cus) for c in P.PLB_STREAM + P.PLB_FORCED}
    assert all(p.form == "stream" for p in plans.values()) and {p.chk for p in plans.values()} == {5, 16}
    assert {c.n for c in P.PLB_STREAM} >= {9, 17} and {plans[c].grid[1] for c in P.PLB_STREAM} >= {16, 24}      # images padded to 8
    assert {c.c for c in P.PLB_STREAM} >= {1, 2, 4} and {c.relu for c in P.PLB_STREAM} == {True, False}
    assert {(c.relu, c.alpha, c.bias) for c in P.PLB_STREAM} >= {(True, 1e-4, 2.0), (False, 1e-4, 2.0)}
    assert [(c.c, c.ranges, plans[c].nz, plans[c].cper) for c in P.PLB_FORCED] == \
        [(7, 2, 2, 4), (7, 3, 2, 4), (7, 4, 2, 4), (21, 2, 2, 11), (21, 3, 3, 7), (21, 4, 4, 6)]   # c = 7: the loop lowers 3 and 4 to 2
    assert all(c in P.PLB_ALL for pair in P.PLB_BOUNDARY for c in pair)


@pytest.mark.parametrize("cus", CUS)
def test_the_20_channel_stream_instantiation_is_unreachable(cus):
    for c in range(16, 400, 20):
        for w in range(3, 700):
            assert P.plb_plan(2, c, 5, w, 0, 0, cus).chk != 20


@pytest.mark.parametrize("cus", CUS)
def test_packed_pool_lrn_bwd_cases_reach_their_branches(cus):
    plans = {c: plb_c8(c, cus) for c in P.PLB_C8}
    assert all(p[:3] == ("stream", 8, 5) for p in plans.values())
    assert {c.c for c in P.PLB_C8} == {20, 33} and {(c.c, c.packed) for c in P.PLB_C8} == {(c, p) for c in (20, 33) for p in (False, True)}
    assert {c.relu for c in P.PLB_C8} == {True, False} and {c.n % 8 for c in P.PLB_C8} >= {1, 2}
    forced = [(c.c, c.ranges, plans[c].nz, plans[c].cper) for c in P.PLB_C8 if c.ranges]
    assert forced == [(20, 2, 2, 16), (20, 3, 3, 8), (20, 4, 3, 8), (33, 2, 2, 24), (33, 3, 3, 16), (33, 4, 3, 16)]    # 4 lowered to 3
    ok, no = P.PLB_C8_GATE
    assert 8 * P.stream_rows(ok.w)[1] * P.pool_out(ok.w) == 1280 and plb_c8(ok, cus).form == "stream" and ok in P.PLB_C8
    assert 8 * P.stream_rows(no.w)[1] * P.pool_out(no.w) == 1312 and plb_c8(no, cus).form == "refuse"


@pytest.mark.parametrize("cus", CUS)
def test_lrn_pool_fwd_cases_reach_their_branches(cus):
    n = P.N(cus)
    assert n == 2 * cus and P.resolve(P.LPF[0], cus).n == n and P.resolve(P.LPF[2], cus).n == n + 1
    assert all(P.lpf_plan(b, c, h, w, ph, cus).prb == 1                                          # what test_ops_gpu runs: one row per band
               for b, h, w, c, ph in [(2, 9, 11, 7, 0), (3, 13, 13, 20, 1), (2, 57, 57, 96, 2), (2, 28, 28, 256, 1), (1, 31, 64, 5, 0), (2, 13, 13, 41, 1)])
    whole, two, odd, outs, wide = (lpf(c, cus) for c in P.LPF[:5])
    assert (whole.bands, whole.prb, whole.last) == (1, 6, 6) and whole.grid[1] == n             # one band holding the whole plane
    assert (two.bands, two.prb, two.last) == (2, 6, 5)                                          # several rows per band, ragged last band
    assert (odd.bands, odd.prb) == (1, 11) and (n + 1) % 8 == 1 and odd.grid[1] == n + 8
    assert outs.by == "outputs" and two.by == odd.by == wide.by == "pixels"
    assert (wide.form, wide.threads, wide.bands) == ("fused", 512, 1) and lpf(P.LPF_REFUSED, cus).form == "refuse"
    assert (P.LPF[4].w, P.LPF_REFUSED.w) == (341, 342)
    assert {c.c for c in P.LPF} >= {1, 2, 4} and any((c.alpha, c.bias) == (1e-4, 2.0) for c in P.LPF)
    ranged = [c for c in P.LPF if c.ranges]
    assert [(lpf(c, cus).nz, lpf(c, cus).cper) for c in ranged] == [(2, 24)]
    assert {(c.c, c.packed) for c in P.LPF_C8} == {(c, p) for c in (20, 33) for p in (False, True)}
    big = [c for c in P.LPF_C8 if c.n == "N"]
    assert len(big) == 1 and big[0].packed and lpf(big[0], cus, True)[1:4] == (6, 1, 6)
    assert [lpf(c, cus, True).nz for c in P.LPF_C8 if c.ranges] == [3]


def test_lrn_cases():
    assert {c.c for c in P.LRN} == {1, 2, 4, 37} and {c.beta for c in P.LRN} == {0.75, 0.5, 1.0}
    assert {(c.n, c.h, c.w) for c in P.LRN} == {(3, 7, 13), (3, 11, 13)}
    assert 3 * 7 * 13 == 273 > 256 > 2 * 7 * 13                  # two workgroups; image boundaries inside the first
    assert 11 * 13 < 256 < 2 * 11 * 13 < 3 * 11 * 13 < 512       # an image boundary inside the second workgroup
    assert {(c.beta, c.alpha, c.bias) for c in P.LRN} >= {(0.75, 1e-4, 2.0), (0.5, 1e-4, 2.0)}


@pytest.mark.parametrize("cus", CUS)
def test_maxpool_cases_reach_their_branches(cus):
    assert {(c.k, c.s) for c in P.POOL_RUNTIME} == set(P.POOL_KS) == {(2, 2), (3, 1), (3, 3), (2, 3), (5, 2), (15, 1)}
    for c in P.POOL_RUNTIME:
        assert P.maxpool_fwd_plan(*c[:6])[:3] == ("generic", "runtime", 1)
        assert P.maxpool_bwd_plan(*c[:7], cus)[:3] == ("generic", "runtime", 1)
    assert {(c.hwc, c.yh > 0, c.dh > 0) for c in P.POOL_RUNTIME} == {(False, True, True), (True, False, True)}
    assert P.maxpool_fwd_plan(*P.POOL_REFUSED[:6]).form == "refuse" and P.POOL_REFUSED.k == 16
    assert [(c.c, P.pool_out(c.h), P.pool_out(c.w)) for c in P.POOL_DIV1] == [(1, 1, 1), (1, 2, 1), (1, 1, 1)] and {c.w for c in P.POOL_DIV1} == {3, 4}
    s = P.POOL_STRIDE
    assert (s.k, s.s) == (3, 2) and P.maxpool_fwd_plan(*s[:6])[1:3] == ("3/2", 2) and P.maxpool_bwd_plan(*s[:7], cus)[:3] == ("generic", "3/2", 5)
    for c in P.POOL_CB64:
        r = P.resolve(c, cus)
        assert r.n == 2 * cus and P.maxpool_bwd_plan(*r[:7], cus) == ("hwc", "3/2", 1, 64) and r.c % 64 == 6
        assert P.maxpool_bwd_plan(3, *r[1:7], cus).cb == 16 and P.maxpool_bwd_plan(r.n - 1, *r[1:7], cus).cb == 16
    assert {(c.dh, c.mask) for c in P.POOL_CB64} == {(0, False), (1, True)}
    lds, gen = P.POOL_LDS_GATE
    assert P.pool_out(lds.h) * P.pool_out(lds.w) == 95 and P.maxpool_bwd_plan(*lds[:7], cus)[::3] == ("hwc", 16)
    assert P.pool_out(gen.h) * P.pool_out(gen.w) == 96 and P.maxpool_bwd_plan(*gen[:7], cus)[:2] == ("generic", "3/2")


def test_the_wide_pool_reference_is_the_oracle():
    x = P.activations(2, 9, 11, 3)
    for got, want in zip(P.max_pool(x, 3, 2), O.max_pool_valid(x)):
        assert np.array_equal(got, want)
    assert int(P.pool_reference(2, 5, 17, 19, 15, 1).arg.max()) > 127


# ---- the stand-in -------------------------------------------------------------------------------------------------------------------
def pool(x, k, s, last=False):
    """First (last: the defect) maximum of each window in scan order, NHWC."""
    n, h, w, c = x.shape
    oh, ow = P.pool_out(h, k, s), P.pool_out(w, k, s)
    y, arg = np.full((n, oh, ow, c), -np.inf, x.dtype), np.zeros((n, oh, ow, c), np.uint8)
    for i in range(k):
        for j in range(k):
            v = x[:, i:i + (oh - 1) * s + 1:s, j:j + (ow - 1) * s + 1:s, :]
            upd = v >= y if last else v > y
            y, arg = np.where(upd, v, y), np.where(upd, np.uint8(i * k + j), arg)
    return y, arg


def inner(t, halo):
    return t if halo == 0 else t[:, :, halo:-halo, halo:-halo]


def unpack(x, c):
    """fp32 NCHW or bf16 c8 without a halo -> NHWC float32."""
    if x.dtype == torch.bfloat16:
        a = x.float().numpy()
        n, cb, h, w, _ = a.shape
        return np.ascontiguousarray(a.transpose(0, 2, 3, 1, 4).reshape(n, h, w, cb * 8)[..., :c])
    return nhwc(x.numpy())


DEFECTS = ("band row dropped", "seam", "last maximum", "unwritten", "halo column", "halo row", "guard", "pad channel", "default alpha")


class StandIn:
    """The operators' contracts in numpy float32 on CPU tensors -- and, on request, one defect."""

    def __init__(self, defect=None, cus=64):
        assert defect is None or defect in DEFECTS
        self.defect, self.cus, self.ranges = defect, cus, 0
        self.pool_out = P.pool_out

    def pool_lrn_bwd_test_ranges(self, ranges=0):
        self.ranges = ranges

    # -- output side: store, then the defects that are about WHERE things are written
    def store(self, out, value_nchw, halo, rows=None):
        dst = inner(out, halo)
        value = torch.from_numpy(np.ascontiguousarray(value_nchw)).to(out.dtype)
        if rows is None:
            dst.copy_(value)
        else:
            dst[:, :, rows] = value[:, :, rows]
        if self.defect == "unwritten":
            dst[-1, -1, -1, -1] = 255 if out.dtype == torch.uint8 else float("nan")
        self.stray(out, halo)

    def store_c8(self, out, value_nhwc, halo):
        n, h, w, c = value_nhwc.shape
        cb = (c + 7) // 8
        full = np.zeros((n, h, w, cb * 8), F32)
        full[..., :c] = value_nhwc
        dst = out[:, :, halo:halo + h, halo:halo + w]
        dst.copy_(torch.from_numpy(np.ascontiguousarray(full.reshape(n, h, w, cb, 8).transpose(0, 3, 1, 2, 4))).bfloat16())
        if self.defect == "unwritten":
            dst[-1, -1, -1, -1, (c - 1) % 8] = float("nan")
        if self.defect == "pad channel" and c % 8:
            dst[0, -1, 0, 0, 7] = 1.0
        self.stray(out, halo)

    def stray(self, out, halo):
        if self.defect == "halo column" and halo:
            out[0, 0, halo, 0] = 1
        if self.defect == "halo row" and halo:
            out[0, 0, 0, halo] = 0
        if self.defect == "guard":
            out.as_strided((1,), (1,), out.storage_offset() - 1).zero_()

    # -- arithmetic
    def lrn_ranged(self, x, ranges, alpha, bias):
        """LRN of each channel range from the channels it may read: two beyond each end -- none with the seam defect."""
        c, l = x.shape[-1], np.empty_like(x)
        for r0, r1 in ranges:
            lo, hi = (r0, r1) if self.defect == "seam" else (max(r0 - 2, 0), min(r1 + 2, c))
            l[..., r0:r1] = O.lrn(x[..., lo:hi], alpha=alpha, bias=bias, dtype=F32)[0][..., r0 - lo:r1 - lo]
        return l

    def lrn_grad(self, x, dy, alpha, beta, bias):
        g = O.lrn_grad(x, dy, alpha=alpha, beta=beta, bias=bias, dtype=F32)
        if self.defect == "default alpha":                     # the second term scaled as if alpha were 2e-5
            u = dy * O.lrn(x, alpha=alpha, beta=beta, bias=bias, dtype=F32)[1] ** F32(-beta)
            g = u - (u - g) * F32(2e-5 / alpha)
        return g

    def lrn_grad_ranged(self, x, dl, ranges, alpha, beta, bias):
        c, g = x.shape[-1], np.empty_like(x)
        for r0, r1 in ranges:
            lo, hi = (r0, r1) if self.defect == "seam" else (max(r0 - 4, 0), min(r1 + 4, c))
            g[..., r0:r1] = self.lrn_grad(x[..., lo:hi], dl[..., lo:hi], alpha, beta, bias)[..., r0 - lo:r1 - lo]
        return g

    # -- operators
    def lrn_fwd(self, x, y, radius=2, alpha=2e-5, beta=0.75, bias=1.0):
        self.store(y, nchw(O.lrn(nhwc(x.numpy()), alpha=alpha, beta=beta, bias=bias, dtype=F32)[0]), 0)

    def lrn_bwd(self, x, dy, dx, radius=2, alpha=2e-5, beta=0.75, bias=1.0, relu_fused=False, dx_halo=0):
        xa = nhwc(x.numpy())
        g = self.lrn_grad(xa, nhwc(dy.numpy()), alpha, beta, bias)
        self.store(dx, nchw(g * (xa > 0) if relu_fused else g), dx_halo)

    def maxpool_fwd(self, x, y, argmax, k=3, s=2, hwc=False, y_halo=0):
        n, c, h, w = x.shape
        if P.maxpool_fwd_plan(n, c, h, w, k, s).form == "refuse":
            raise RuntimeError("vl_maxpool_fwd: bad argument")
        v, a = pool(nhwc(x.numpy()), k, s, self.defect == "last maximum")
        if hwc:
            y.copy_(torch.from_numpy(v))
            argmax.copy_(torch.from_numpy(a))
        else:
            self.store(y, nchw(v), y_halo)
            self.store(argmax, nchw(a), y_halo)

    def maxpool_bwd(self, dy, argmax, dx, relu_mask=None, k=3, s=2, hwc=False, dy_halo=0, dx_halo=0):
        n, c = dx.shape[:2]
        shape = (n, dx.shape[2] - 2 * dx_halo, dx.shape[3] - 2 * dx_halo, c)
        d, a = (dy.numpy(), argmax.numpy()) if hwc else (nhwc(inner(dy, dy_halo).numpy()), nhwc(inner(argmax, dy_halo).numpy()))
        g = O.max_pool_valid_grad(shape, a, d, k, s)
        if relu_mask is not None:
            g = g * (nhwc(relu_mask.numpy()) > 0)
        self.store(dx, nchw(g), dx_halo)

    def fused_forward(self, x, p_halo, alpha, bias, c8):
        n, h, w, c = x.shape
        plan = P.lpf_plan(n, c, h, w, p_halo, self.cus, c8, self.ranges)
        if plan.form == "refuse":
            raise RuntimeError("vl_lrn_pool_fwd: plane too wide (%d) for one band of pooled rows" % w)
        v, a = pool(self.lrn_ranged(x, P.ranges_of(c, plan.nz, plan.cper), alpha, bias), 3, 2, self.defect == "last maximum")
        rows = None
        if self.defect == "band row dropped":                  # band 0 stops one pooled row early
            rows = [r for r in range(v.shape[1]) if r != plan.prb - 1]
        return v, a, rows

    def lrn_pool_fwd(self, x, p, argmax, p_halo=0, radius=2, alpha=2e-5, beta=0.75, bias=1.0):
        v, a, rows = self.fused_forward(nhwc(x.numpy()), p_halo, alpha, bias, False)
        self.store(p, nchw(v), p_halo, rows)
        self.store(argmax, nchw(a), p_halo, rows)

    def lrn_pool_fwd_c8(self, x, pb, argmax, p_halo=0, radius=2, alpha=2e-5, beta=0.75, bias=1.0, channels=None):
        v, a, _ = self.fused_forward(unpack(x, channels), p_halo, alpha, bias, True)
        self.store_c8(pb, v, p_halo)
        self.store(argmax, nchw(a), p_halo)

    def fused_backward(self, x, dp, argmax, p_halo, plan, alpha, beta, bias, relu):
        dl = O.max_pool_valid_grad(x.shape, nhwc(inner(argmax, p_halo).numpy()), nhwc(inner(dp, p_halo).numpy()))
        g = self.lrn_grad_ranged(x, dl, P.ranges_of(x.shape[-1], plan.nz, plan.cper), alpha, beta, bias)
        return g * (x > 0) if relu else g

    def pool_lrn_bwd(self, x, dp, argmax, dx, p_halo=0, dx_halo=0, radius=2, alpha=2e-5, beta=0.75, bias=1.0, relu_fused=True):
        n, c, h, w = x.shape
        plan = P.plb_plan(n, c, h, w, p_halo, dx_halo, self.cus, beta, self.ranges)
        if plan.form == "refuse":
            raise RuntimeError("vl_pool_lrn_bwd: pooled plane too wide (%d) for the LDS staging" % P.pool_out(w))
        self.store(dx, nchw(self.fused_backward(nhwc(x.numpy()), dp, argmax, p_halo, plan, alpha, beta, bias, relu_fused)), dx_halo)

    def pool_lrn_bwd_c8(self, x, dp, argmax, dxb, p_halo=0, dxb_halo=0, radius=2, alpha=2e-5, beta=0.75, bias=1.0, relu_fused=True):
        xa = unpack(x, dp.shape[1])
        n, h, w, c = xa.shape
        plan = P.plb_c8_plan(n, c, h, w, p_halo, dxb_halo, self.cus, self.ranges)
        if plan.form == "refuse":
            raise RuntimeError("vl_pool_lrn_bwd_c8: plane too large for the channel-stream form")
        self.store_c8(dxb, self.fused_backward(xa, dp, argmax, p_halo, plan, alpha, beta, bias, relu_fused), dxb_halo)


# ---- discrimination -----------------------------------------------------------------------------------------------------------------
CPU_CUS = 64


def jobs():
    """(check, case[, refusal]) of everything the GPU half runs but the 17 M-element grid-stride case (its branch is arithmetic above)."""
    r = lambda c: P.resolve(c, CPU_CUS)
    out = [(G.check_pool_lrn_bwd, c) for c in P.PLB_ALL] + [(G.check_pool_lrn_bwd, P.PLB_REFUSED, "pooled plane too wide")]
    out += [(G.check_pool_lrn_bwd_c8, c) for c in P.PLB_C8] + [(G.check_pool_lrn_bwd_c8, P.PLB_C8_GATE[1], "plane too large")]
    out += [(G.check_lrn_pool_fwd, r(c)) for c in P.LPF] + [(G.check_lrn_pool_fwd, P.LPF_REFUSED, "plane too wide")]
    out += [(G.check_lrn_pool_fwd_c8, r(c)) for c in P.LPF_C8] + [(G.check_lrn, c) for c in P.LRN] + [(G.check_maxpool, r(c)) for c in P.POOL_SMALL]
    return out


@pytest.mark.parametrize("job", jobs(), ids=lambda j: j[0].__name__[6:] + "-" + P.case_id(j[1]))
def test_a_correct_stand_in_passes(job):
    """Float32 arithmetic is inside every tolerance, and inside the arg-max near-tie cap, on each chosen input."""
    check, case = job[:2]
    check(StandIn(cus=CPU_CUS), case, "cpu", *job[2:])


BIG = P.resolve(P.LPF[0], CPU_CUS)                               # 128 x 8 x 6 x 6 pooled outputs: ~0.2 % of the windows are all zero
CAUGHT = [
    ("band row dropped", G.check_lrn_pool_fwd, P.resolve(P.LPF[1], CPU_CUS), "not written"),
    ("seam", G.check_pool_lrn_bwd, P.PLB_FORCED[-1], "Not equal to tolerance"),
    ("seam", G.check_pool_lrn_bwd_c8, P.PLB_C8[-1], "pool_lrn_bwd_c8"),
    ("seam", G.check_lrn_pool_fwd, P.LPF[-1], "Not equal to tolerance"),
    ("seam", G.check_lrn_pool_fwd_c8, P.LPF_C8[-1], "lrn_pool_fwd_c8"),
    ("last maximum", G.check_maxpool, P.POOL_RUNTIME[0], "arg-max"),
    ("last maximum", G.check_maxpool, P.POOL_LDS_GATE[0], "arg-max"),
    ("last maximum", G.check_lrn_pool_fwd, BIG, "lrn_pool_fwd"),
    ("unwritten", G.check_pool_lrn_bwd, P.PLB_CHUNKED[0], "not written"),
    ("unwritten", G.check_pool_lrn_bwd_c8, P.PLB_C8[1], "not written"),
    ("unwritten", G.check_lrn_pool_fwd, P.LPF[3], "not written"),
    ("unwritten", G.check_lrn_pool_fwd_c8, P.LPF_C8[1], "not written"),
    ("unwritten", G.check_lrn, P.LRN[0], "not written"),
    ("unwritten", G.check_maxpool, P.POOL_RUNTIME[0], "forward"),
    ("halo column", G.check_pool_lrn_bwd, P.PLB_CHUNKED[1], "halo column not zero"),
    ("halo column", G.check_lrn_pool_fwd, P.LPF[3], "halo column not zero"),
    ("halo column", G.check_lrn, P.LRN[0], "halo column not zero"),
    ("halo column", G.check_maxpool, P.POOL_RUNTIME[0], "halo column not zero"),
    ("halo column", G.check_pool_lrn_bwd_c8, P.PLB_C8[0], "halo of the packed tensor not zero"),
    ("halo column", G.check_lrn_pool_fwd_c8, P.LPF_C8[0], "halo of the packed tensor not zero"),
    ("halo row", G.check_pool_lrn_bwd, P.PLB_CHUNKED[1], "halo row written"),
    ("halo row", G.check_lrn_pool_fwd, P.LPF[3], "halo row written"),
    ("halo row", G.check_lrn, P.LRN[0], "halo row written"),
    ("halo row", G.check_maxpool, P.POOL_RUNTIME[1], "halo row written"),
    ("guard", G.check_pool_lrn_bwd, P.PLB_CHUNKED[0], "guard around the tensor written"),
    ("guard", G.check_pool_lrn_bwd_c8, P.PLB_C8[0], "guard around the tensor written"),
    ("guard", G.check_lrn_pool_fwd, P.LPF[4], "guard around the tensor written"),
    ("guard", G.check_lrn_pool_fwd_c8, P.LPF_C8[0], "guard around the tensor written"),
    ("guard", G.check_lrn, P.LRN[0], "guard around the tensor written"),
    ("guard", G.check_maxpool, P.POOL_DIV1[0], "guard around the tensor written"),
    ("pad channel", G.check_pool_lrn_bwd_c8, P.PLB_C8[0], "pad channel of the last 8-channel block not zero"),
    ("pad channel", G.check_lrn_pool_fwd_c8, P.LPF_C8[1], "pad channel of the last 8-channel block not zero"),
    ("default alpha", G.check_pool_lrn_bwd, P.PLB_STREAM[2], "Not equal to tolerance"),
    ("default alpha", G.check_lrn, P.LRN[-1], "Not equal to tolerance"),
]


def test_every_listed_defect_is_tried():
    assert {d for d, _, _, _ in CAUGHT} == set(DEFECTS)


@pytest.mark.parametrize("defect,check,case,message", CAUGHT, ids=lambda v: v if isinstance(v, str) else getattr(v, "__name__", None) or P.case_id(v))
def test_each_defect_is_caught(defect, check, case, message):
    check(StandIn(cus=CPU_CUS), case, "cpu")                     # the same case passes without the defect
    with pytest.raises(AssertionError, match=message):
        check(StandIn(defect, CPU_CUS), case, "cpu")
