"""The pooling / LRN family of csrc/pointwise.hip against the fp64 oracle on every launcher branch: vl_pool_lrn_bwd's chunked fall-back,
both stream instantiations at their staging limits and its refusal; vl_lrn_pool_fwd's bands of several pooled rows, ragged last band,
whole-plane band, thread count set by the outputs, widest plane and refusal; image counts that are no multiple of 8; alpha / beta /
bias other than the defaults; 1, 2 and 4 channels; vl_lrn_fwd / _bwd with an image boundary inside the second workgroup; the runtime
max-pool instantiations, the grid-stride loop, divisor 1, the hwc backward with 64-channel blocks and its LDS gate; the packed
outputs with a ragged last 8-channel block.  The cases, their inputs, fp64 references and the restated launch arithmetic are in
tests/pool_plan.py; tests/test_pool_geometry.py (CPU) shows that the lists reach those branches and runs the check functions below
against a float32 stand-in with and without defects.

Tolerances: fp32 results `close(rtol=1e-5, atol_rel=1e-6)` (what the fused tests of test_ops_gpu hold); max-pool forward bit-exact;
the fused forward's arg-max by the near-tie rule of test_lrn_pool_fwd_fused; packed outputs within 2^-7 |want| per element of the
bf16 rounding of the fp64 oracle (test_pool_lrn_bwd_packed_output's bound), pad channels and halo exactly zero.

Every output is a view into a larger allocation (Guarded): sentinels before and behind it and in its halo rows must still be there
afterwards, the halo columns of interior rows hold zeros before and after, the interior starts as NaN (arg-max: 255).  Pooled
gradients and arg-max maps handed IN carry NaN / 255 in their halo: nothing may read it."""
import numpy as np
import pytest
import torch

from tests import pool_plan as P
from tests.test_ops_gpu import close, dev, host, nchw, near_tie_argmax, nhwc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL, SENT8, GUARD = 12345.0, 0xA5, 64


@pytest.fixture(scope="module")
def ops():
    import vltf_amd.ops as ops_
    return ops_


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def put(a, device, dtype=torch.float32):
    return dev(a, dtype) if device == DEV else torch.tensor(np.ascontiguousarray(a), dtype=dtype)


def get(t):
    return host(t) if t.is_cuda else t.detach().numpy()


def haloed(a_nchw, halo, blank, device, dtype=torch.float32):
    """A pool-output tensor handed to a kernel: the values inside, `blank` (NaN / 255: never to be read) in the halo."""
    n, c, h, w = a_nchw.shape
    full = np.full((n, c, h + 2 * halo, w + 2 * halo), blank, a_nchw.dtype)
    full[:, :, halo:halo + h, halo:halo + w] = a_nchw
    return put(full, device, dtype)


def c8_shape(n, c, h, w, halo):
    return (n, (c + 7) // 8, h + 2 * halo, w + 2 * halo, 8)


def pack_c8(a_nhwc, device):
    """NHWC fp32 (bf16-representable values) -> bf16 [n][c / 8][h][w][8] without a halo, zeros beyond c."""
    n, h, w, c = a_nhwc.shape
    cb = (c + 7) // 8
    full = np.zeros((n, h, w, cb * 8), np.float32)
    full[..., :c] = a_nhwc
    return put(full.reshape(n, h, w, cb, 8).transpose(0, 3, 1, 2, 4), device).bfloat16().contiguous()


class Guarded:
    """An output inside a larger allocation.  NCHW with a halo: sentinel halo rows, zero halo columns (fp32; sentinel for the arg-max
    map, whose halo columns are unspecified), blank interior (NaN / 255).  c8 (channels given): zeros, blank interior channels < c."""

    def __init__(self, shape, device, dtype=torch.float32, halo=0, channels=None):
        self.shape, self.halo, self.c, self.u8 = tuple(shape), halo, channels, dtype == torch.uint8
        numel = int(np.prod(shape))
        self.flat = torch.full((numel + 2 * GUARD,), SENT8 if self.u8 else SENTINEL, dtype=dtype, device=device)
        self.sent = SENT8 if self.u8 else float(self.flat[0].float())
        self.t = self.flat[GUARD:GUARD + numel].view(self.shape)
        blank = 255 if self.u8 else float("nan")
        if channels is not None:
            self.t.zero_()
            inner = self.t[:, :, halo:shape[2] - halo, halo:shape[3] - halo]
            inner.fill_(blank)
            if channels % 8:
                inner[:, -1, :, :, channels % 8:] = 0
        elif halo:
            rows = self.t[:, :, halo:-halo]
            if not self.u8:
                rows.zero_()
            rows[:, :, :, halo:-halo].fill_(blank)
        else:
            self.t.fill_(blank)
        self.init = self.flat.clone()

    def untouched(self):
        return torch.equal(self.flat.view(torch.uint8), self.init.view(torch.uint8))

    def settle(self, what, cols="zero"):
        """Everything around the interior is as it must be; returns the interior (c8: as NHWC fp32 of the first c channels)."""
        a = get(self.flat if self.u8 else self.flat.float())
        assert (a[:GUARD] == self.sent).all() and (a[-GUARD:] == self.sent).all(), what + ": guard around the tensor written"
        t, halo = a[GUARD:-GUARD].reshape(self.shape), self.halo
        if self.c is not None:
            n, cb, hp, wp, _ = self.shape
            full = t.transpose(0, 2, 3, 1, 4).reshape(n, hp, wp, cb * 8).copy()
            inside = full[:, halo:hp - halo, halo:wp - halo]
            inner = inside[..., :self.c].copy()
            assert not inside[..., self.c:].any(), what + ": pad channel of the last 8-channel block not zero"
            inside[...] = 0
            assert not full.any(), what + ": halo of the packed tensor not zero"
            return inner
        if halo:
            assert (t[:, :, :halo] == self.sent).all() and (t[:, :, -halo:] == self.sent).all(), what + ": halo row written"
            rows = t[:, :, halo:-halo]
            if cols == "zero":
                assert not rows[..., :halo].any() and not rows[..., -halo:].any(), what + ": halo column not zero"
            return rows[..., halo:-halo]
        return t


def written(got, what):
    assert np.isfinite(got).all(), what + ": interior element not written (or not finite)"
    return got


def refused(call, outs, match, what):
    """An error return and no launch: every output is bit for bit what it was."""
    with pytest.raises(Exception, match=match):
        call()
    if outs[0].flat.is_cuda:
        torch.cuda.synchronize()
    assert all(o.untouched() for o in outs), what + ": refused, yet an output was written"


def packed_close(got, want, what):
    """Against the bf16 rounding of the fp64 oracle: every element within 2^-7 |want| (one bf16 ulp), and not all zero."""
    want = P.O.bf16_round(np.asarray(want, np.float64).astype(np.float32)).astype(np.float64)
    err = np.abs(written(got, what).astype(np.float64) - want)
    bad = err > 2.0 ** -7 * np.abs(want) + 1e-30
    assert not bad.any(), (what, int(bad.sum()), float(err[bad].max()), float(np.abs(want[bad]).min()))
    assert np.abs(got).max() > 0, what


def argmax_rule(got_arg, ref, what):
    """test_lrn_pool_fwd_fused's near-tie rule against the fp64 oracle; 255 (the blank) is an unwritten element."""
    near_tie_argmax(got_arg, ref.arg, ref.l, what)


class forced_ranges:
    def __init__(self, ops, ranges):
        self.ops, self.ranges = ops, ranges

    def __enter__(self):
        self.ops.pool_lrn_bwd_test_ranges(self.ranges)

    def __exit__(self, *exc):
        self.ops.pool_lrn_bwd_test_ranges(0)


# ---- the checks (tests/test_pool_geometry.py runs them on the CPU against a stand-in) ---------------------------------------------------
def plb_operands(ref, ph, device):
    return haloed(nchw(ref.dy), ph, np.nan, device), haloed(nchw(ref.arg), ph, 255, device, torch.uint8)


def check_pool_lrn_bwd(ops, case, device=DEV, refuse=None):
    n, c, h, w, ph, dh = case[:6]
    what = "pool_lrn_bwd " + P.case_id(case)
    ref = P.plb_reference(n, c, h, w, case.relu, case.alpha, case.beta, case.bias)
    dp, ap = plb_operands(ref, ph, device)
    dx = Guarded((n, c, h + 2 * dh, w + 2 * dh), device, halo=dh)

    def call():
        with forced_ranges(ops, case.ranges):
            ops.pool_lrn_bwd(put(nchw(ref.x), device), dp, ap, dx.t, p_halo=ph, dx_halo=dh, alpha=case.alpha, beta=case.beta, bias=case.bias,
                             relu_fused=case.relu)
    if refuse:
        return refused(call, [dx], refuse, what)
    call()
    close(written(nhwc(dx.settle(what)), what), ref.want, rtol=1e-5, atol_rel=1e-6, msg=what)


def check_pool_lrn_bwd_c8(ops, case, device=DEV, refuse=None):
    n, c, h, w, ph, dh = case[:6]
    what = "pool_lrn_bwd_c8 " + P.case_id(case)
    ref = P.plb_reference(n, c, h, w, case.relu, bf16=case.packed)
    dp, ap = plb_operands(ref, ph, device)
    x = pack_c8(ref.x, device) if case.packed else put(nchw(ref.x), device)
    dxb = Guarded(c8_shape(n, c, h, w, dh), device, torch.bfloat16, halo=dh, channels=c)

    def call():
        with forced_ranges(ops, case.ranges):
            ops.pool_lrn_bwd_c8(x, dp, ap, dxb.t, p_halo=ph, dxb_halo=dh, relu_fused=case.relu)
    if refuse:
        return refused(call, [dxb], refuse, what)
    call()
    packed_close(dxb.settle(what), ref.want, what)


def check_lrn_pool_fwd(ops, case, device=DEV, refuse=None):
    n, c, h, w, ph = case[:5]
    what = "lrn_pool_fwd " + P.case_id(case)
    ref = P.lpf_reference(n, c, h, w, case.alpha, case.bias)
    oh, ow = P.pool_out(h), P.pool_out(w)
    p = Guarded((n, c, oh + 2 * ph, ow + 2 * ph), device, halo=ph)
    ap = Guarded(p.shape, device, torch.uint8, halo=ph)

    def call():
        with forced_ranges(ops, case.ranges):
            ops.lrn_pool_fwd(put(nchw(ref.x), device), p.t, ap.t, p_halo=ph, alpha=case.alpha, bias=case.bias)
    if refuse:
        return refused(call, [p, ap], refuse, what)
    call()
    close(written(nhwc(p.settle(what)), what), ref.y, rtol=1e-5, atol_rel=1e-6, msg=what)
    argmax_rule(nhwc(ap.settle(what, cols="any")), ref, what)


def check_lrn_pool_fwd_c8(ops, case, device=DEV):
    n, c, h, w, ph = case[:5]
    what = "lrn_pool_fwd_c8 " + P.case_id(case)
    ref = P.lpf_reference(n, c, h, w, bf16=case.packed)
    oh, ow = P.pool_out(h), P.pool_out(w)
    x = pack_c8(ref.x, device) if case.packed else put(nchw(ref.x), device)
    pb = Guarded(c8_shape(n, c, oh, ow, ph), device, torch.bfloat16, halo=ph, channels=c)
    ap = Guarded((n, c, oh + 2 * ph, ow + 2 * ph), device, torch.uint8, halo=ph)
    with forced_ranges(ops, case.ranges):
        ops.lrn_pool_fwd_c8(x, pb.t, ap.t, p_halo=ph, channels=c)
    packed_close(pb.settle(what), ref.y, what)
    argmax_rule(nhwc(ap.settle(what, cols="any")), ref, what)


def check_lrn(ops, case, device=DEV):
    n, h, w, c, alpha, beta, bias = case
    what = "lrn " + P.case_id(case)
    ref = P.lrn_reference(*case)
    x, dy = put(nchw(ref.x), device), put(nchw(ref.dy), device)
    y = Guarded((n, c, h, w), device)
    ops.lrn_fwd(x, y.t, alpha=alpha, beta=beta, bias=bias)
    close(written(nhwc(y.settle(what)), what), ref.y, rtol=1e-5, atol_rel=1e-6, msg=what + " forward")
    for relu, halo in ((False, 0), (True, 0), (False, 2), (True, 1)):
        tag = "%s backward relu=%d halo=%d" % (what, relu, halo)
        dx = Guarded((n, c, h + 2 * halo, w + 2 * halo), device, halo=halo)
        ops.lrn_bwd(x, dy, dx.t, alpha=alpha, beta=beta, bias=bias, relu_fused=relu, dx_halo=halo)
        close(written(nhwc(dx.settle(tag)), tag), ref.dx * (ref.x > 0) if relu else ref.dx, rtol=1e-5, atol_rel=1e-6, msg=tag)


def check_maxpool(ops, case, device=DEV):
    n, c, h, w, k, s, hwc, yh, dh, mask = case
    what = "maxpool " + P.case_id(case)
    ref = P.pool_reference(n, c, h, w, k, s)
    oh, ow = P.pool_out(h, k, s), P.pool_out(w, k, s)
    x = put(nchw(ref.x), device)
    shape = (n, oh, ow, c) if hwc else (n, c, oh + 2 * yh, ow + 2 * yh)
    y, a = Guarded(shape, device, halo=yh), Guarded(shape, device, torch.uint8, halo=yh)
    ops.maxpool_fwd(x, y.t, a.t, k=k, s=s, hwc=hwc, y_halo=yh)
    gy, ga = y.settle(what), a.settle(what, cols="any")
    np.testing.assert_array_equal(gy if hwc else nhwc(gy), ref.y, err_msg=what + " forward")
    np.testing.assert_array_equal(ga if hwc else nhwc(ga), ref.arg, err_msg=what + " arg-max")
    dyd = put(ref.dy, device) if hwc else haloed(nchw(ref.dy), yh, np.nan, device)
    ad = put(ref.arg, device, torch.uint8) if hwc else haloed(nchw(ref.arg), yh, 255, device, torch.uint8)
    dx = Guarded((n, c, h + 2 * dh, w + 2 * dh), device, halo=dh)
    ops.maxpool_bwd(dyd, ad, dx.t, relu_mask=x if mask else None, k=k, s=s, hwc=hwc, dy_halo=yh, dx_halo=dh)
    close(written(nhwc(dx.settle(what)), what), ref.dx * (ref.x > 0) if mask else ref.dx, rtol=1e-5, atol_rel=1e-6, msg=what + " backward")


# ---- vl_pool_lrn_bwd ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.PLB_ALL, ids=P.case_id)
def test_pool_lrn_bwd(ops, case):
    """The chunked fall-back (planes past the stream form's staging, beta 0.5 and 1.0 through powf, two 512-pixel bands, a ragged
    second 16-channel block), both stream instantiations at the last width they take, 9 and 17 images, relu_fused both ways,
    alpha 1e-4 / bias 2, 1 / 2 / 4 channels, forced channel ranges that the launcher lowers."""
    check_pool_lrn_bwd(ops, case)


def test_pool_lrn_bwd_refuses_a_plane_too_wide_for_its_staging(ops):
    check_pool_lrn_bwd(ops, P.PLB_REFUSED, refuse="pooled plane too wide")


@pytest.mark.parametrize("case", P.PLB_C8, ids=P.case_id)
def test_pool_lrn_bwd_packed(ops, case):
    """20 and 33 channels (a ragged last 8-channel block), fp32 and packed input, forced ranges in units of 8, the widest plane."""
    check_pool_lrn_bwd_c8(ops, case)


def test_pool_lrn_bwd_packed_refuses_past_its_gate(ops):
    check_pool_lrn_bwd_c8(ops, P.PLB_C8_GATE[1], refuse="plane too large for the channel-stream form")


# ---- vl_lrn_pool_fwd ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.LPF, ids=P.case_id)
def test_lrn_pool_fwd(ops, case):
    """N = 2 x CUs images: one band holding the whole plane, two bands of 6 and 5 pooled rows, N + 1 images; threads set by the
    outputs; the widest plane; 1 / 2 / 4 channels; alpha 1e-4 / bias 2; two channel ranges."""
    check_lrn_pool_fwd(ops, P.resolve(case, cus()))


def test_lrn_pool_fwd_refuses_a_plane_wider_than_one_band(ops):
    check_lrn_pool_fwd(ops, P.LPF_REFUSED, refuse="plane too wide")


@pytest.mark.parametrize("case", P.LPF_C8, ids=P.case_id)
def test_lrn_pool_fwd_packed(ops, case):
    check_lrn_pool_fwd_c8(ops, P.resolve(case, cus()))


# ---- vl_lrn_fwd / vl_lrn_bwd ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.LRN, ids=P.case_id)
def test_lrn(ops, case):
    """273 and 429 positions: two workgroups along the positions, image boundaries inside the first and inside the second.  beta 0.5
    and 1.0 take powf."""
    check_lrn(ops, case)


# ---- vl_maxpool_fwd / vl_maxpool_bwd ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.POOL_SMALL, ids=P.case_id)
def test_maxpool(ops, case):
    """The runtime-k,s instantiations (NCHW with halos, and hwc through the generic backward), divisor 1, the hwc backward with
    64-channel blocks (ragged second block of 6) and either side of its LDS gate."""
    check_maxpool(ops, P.resolve(case, cus()))


def test_maxpool_grid_stride(ops):
    """More outputs (forward) and inputs (backward) than one pass of 16384 x 256 threads covers."""
    check_maxpool(ops, P.POOL_STRIDE)


def test_maxpool_refuses_a_window_of_256(ops):
    n, c, h, w, k, s = P.POOL_REFUSED[:6]
    oh, ow = P.pool_out(h, k, s), P.pool_out(w, k, s)
    y, a = Guarded((n, c, oh, ow), DEV), Guarded((n, c, oh, ow), DEV, torch.uint8)
    x = put(nchw(P.activations(n, h, w, c)), DEV)
    refused(lambda: ops.maxpool_fwd(x, y.t, a.t, k=k, s=s), [y, a], "bad argument", "maxpool k=16")
