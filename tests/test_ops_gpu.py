"""Per-op parity: every HIP entry point (through the C-ABI) against the CPU oracle on the same
seeded inputs.  Oracle works NHWC/HWIO (the reference's layouts); the device works NCHW/HWIO.
Tolerances are ours (parity unpinned): fp32 fma-chain error ~1e-7 * sum|a*b|."""
import math

import numpy as np
import pytest
import torch

from oracle import lrcn_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    import vltf_amd.ops as ops_
    return ops_


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def nchw(a):
    return np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2)))


def nhwc(a):
    return np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))


def close(got, want, rtol=3e-5, atol_rel=3e-5, msg=""):
    want = np.asarray(want, np.float64)
    scale = float(np.abs(want).max()) or 1.0
    np.testing.assert_allclose(np.asarray(got, np.float64), want, rtol=rtol, atol=atol_rel * scale, err_msg=msg)


# ---- GEMM ------------------------------------------------------------------------------------------
@pytest.fixture
def conv_math(ops, request):
    ops.set_conv_math(request.param)
    assert ops.conv_math() == request.param
    yield request.param
    ops.set_conv_math("f32")


@pytest.mark.parametrize("ta", [False, True])
@pytest.mark.parametrize("tb", [False, True])
@pytest.mark.parametrize("m,n,k", [(70, 150, 37), (130, 260, 100), (8, 1024, 256), (256, 128, 512), (1, 5, 3)])
def test_gemm(ops, ta, tb, m, n, k):
    rng = np.random.default_rng(m * 1000 + n + k)
    a = rng.standard_normal((m, k)).astype(np.float32)
    b = rng.standard_normal((k, n)).astype(np.float32)
    bias = rng.standard_normal(n).astype(np.float32)
    mask = rng.standard_normal((m, n)).astype(np.float32)
    ad = dev(a.T if ta else a)
    bd = dev(b.T if tb else b)
    c = torch.full((m, n), 7.0, device=DEV)
    ops.gemm(ad, bd, c, m, n, k, transa=ta, transb=tb)
    close(host(c), a.astype(np.float64) @ b)
    ops.gemm(ad, bd, c, m, n, k, transa=ta, transb=tb, bias=dev(bias), relu=True, relu_mask=dev(mask))
    want = np.maximum(a.astype(np.float64) @ b + bias, 0) * (mask > 0)
    close(host(c), want)


@pytest.mark.parametrize("conv_math", ["bf16x3", "bf16x6", "bf16"], indirect=True)
@pytest.mark.parametrize("ta,tb", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("m,n,k", [(130, 300, 200), (256, 512, 4096), (1024, 384, 130)])
def test_gemm_split_products(ops, conv_math, ta, tb, m, n, k):
    """vl_gemm under vl_set_conv_math with the workspace of vl_gemm_split_ws_bytes: both operands pre-split into images, the
    MFMA loop VALU-free.  Ragged m / n / k (zero-padded images), split-K (the 256 x 512 x 4096 case), leading dimensions,
    bias + ReLU + mask.  bf16x3 / bf16x6 at the fp32 tolerance, plain bf16 at 1e-2 relative L2."""
    rng = np.random.default_rng(m + n + k)
    a = rng.standard_normal((m, k)).astype(np.float32)
    b = rng.standard_normal((k, n)).astype(np.float32)
    bias = rng.standard_normal(n).astype(np.float32)
    mask = rng.standard_normal((m, n)).astype(np.float32)
    ap = np.pad(a.T if ta else a, ((0, 0), (0, 3)))              # lda / ldb / ldc larger than the row
    bp = np.pad(b.T if tb else b, ((0, 0), (0, 5)))
    ws = torch.empty(ops.gemm_split_ws_bytes(m, n, k) // 4 + 1, device=DEV)
    c = torch.zeros((m, n + 2), device=DEV)
    ops.gemm(dev(ap), dev(bp), c, m, n, k, transa=ta, transb=tb, lda=ap.shape[1], ldb=bp.shape[1], ldc=n + 2, ws=ws)
    want = a.astype(np.float64) @ b
    got = host(c)
    err = np.linalg.norm(got[:, :n] - want) / np.linalg.norm(want)
    if conv_math == "bf16":
        assert 1e-4 < err < 1e-2, err
    else:
        close(got[:, :n], want)
        assert err < 2e-5
    assert np.all(got[:, n:] == 0)
    ops.gemm(dev(ap), dev(bp), c, m, n, k, transa=ta, transb=tb, lda=ap.shape[1], ldb=bp.shape[1], ldc=n + 2, bias=dev(bias), relu=True,
             relu_mask=dev(np.pad(mask, ((0, 0), (0, 2)))), ws=ws)
    want2 = np.maximum(want + bias, 0) * (mask > 0)
    got2 = host(c)[:, :n]
    if conv_math == "bf16":
        assert np.linalg.norm(got2 - want2) / np.linalg.norm(want2) < 1e-2
    else:
        close(got2, want2)


@pytest.mark.parametrize("m,n,k,ws_mb", [(130, 300, 200, 4), (1000, 384, 130, 16), (256, 512, 4096, 16), (9216, 4096, 128, 64), (4352, 1024, 1024, 64)])
def test_gemm_reduction_major_operands_at_the_step_sizes(ops, m, n, k, ws_mb):
    """vl_gemm transa = 1 (x^T dy: the fc / LSTM weight gradients) with leading dimensions, split reduction through the workspace,
    bias + ReLU + mask, up to fc6's weight gradient on an 8-clip shard (9216 x 4096 x 128) and the benchmark's LSTM kernel gradient
    (4352 x 1024 x 1024)."""
    rng = np.random.default_rng(m + n + k)
    at = rng.standard_normal((k, m + 3)).astype(np.float32)            # A stored [k][m], lda = m + 3
    b = rng.standard_normal((k, n + 5)).astype(np.float32)             # ldb = n + 5
    bias = rng.standard_normal(n).astype(np.float32)
    ws = torch.empty(ws_mb << 18, device=DEV)
    c = torch.zeros((m, n + 2), device=DEV)
    atd, bd = dev(at), dev(b)
    ops.gemm(atd, bd, c, m, n, k, transa=True, lda=m + 3, ldb=n + 5, ldc=n + 2, ws=ws)
    want = (torch.from_numpy(at[:, :m]).double().t() @ torch.from_numpy(b[:, :n]).double()).numpy()
    got = host(c)
    close(got[:, :n], want)
    assert np.all(got[:, n:] == 0)                                      # padding untouched
    mask = rng.standard_normal((m, n + 2)).astype(np.float32)
    ops.gemm(atd, bd, c, m, n, k, transa=True, lda=m + 3, ldb=n + 5, ldc=n + 2, bias=dev(bias), relu=True, relu_mask=dev(mask), ws=ws)
    close(host(c)[:, :n], np.maximum(want + bias, 0) * (mask[:, :n] > 0))


def test_gemm_ld_and_splitk(ops):
    rng = np.random.default_rng(7)
    m, n, k = 64, 200, 2048
    a = rng.standard_normal((m, k + 5)).astype(np.float32)     # lda = k + 5
    b = rng.standard_normal((k, n + 3)).astype(np.float32)     # ldb = n + 3
    bias = rng.standard_normal(n).astype(np.float32)
    c = torch.zeros((m, n + 9), device=DEV)                    # ldc = n + 9
    ws = torch.empty(16 * m * n, device=DEV)
    ops.gemm(dev(a), dev(b), c, m, n, k, lda=k + 5, ldb=n + 3, ldc=n + 9, bias=dev(bias), relu=True, ws=ws)
    want = np.maximum(a[:, :k].astype(np.float64) @ b[:, :n] + bias, 0)
    got = host(c)
    close(got[:, :n], want)
    assert np.all(got[:, n:] == 0)                             # padding untouched


# ---- convolution -----------------------------------------------------------------------------------
CONV_CASES = [
    # n, h, w, cin, cout, k, stride, groups
    (2, 23, 23, 3, 8, 11, 4, 1),
    (3, 24, 20, 3, 8, 11, 4, 1),        # asymmetric SAME padding
    (2, 9, 9, 6, 8, 5, 1, 2),
    (2, 7, 6, 8, 6, 3, 1, 2),
    (1, 227, 227, 3, 96, 11, 4, 1),     # conv1
    (2, 28, 28, 96, 256, 5, 1, 2),      # conv2
    (3, 13, 13, 256, 384, 3, 1, 1),     # conv3
    (3, 13, 13, 384, 384, 3, 1, 2),     # conv4
    (3, 13, 13, 384, 256, 3, 1, 2),     # conv5
    (1, 10, 7, 40, 100, 3, 1, 1),       # ragged everything: 100 / 40 channels, K = 360 / 900 (tail stages), one partial pixel tile
    (2, 6, 5, 40, 96, 1, 1, 1),         # 1x1: K = 40 -> fewer reduction stages than the split-product kernel's ring has slots
]


def pad_nchw(a_nchw, halo):
    return np.pad(a_nchw, ((0, 0), (0, 0), (halo, halo), (halo, halo)))


def interior(t, halo):
    return t if halo == 0 else t[:, :, halo:-halo, halo:-halo]


@pytest.mark.parametrize("conv_math,padded", [("f32", False), ("f32", True), ("bf16x3", True), ("bf16x6", True)], indirect=["conv_math"])
@pytest.mark.parametrize("n,h,w,cin,cout,k,s,g", CONV_CASES)
def test_conv_fwd_bwd(ops, conv_math, padded, n, h, w, cin, cout, k, s, g):
    """padded=False: dense NCHW, bounds-tested gather.  padded=True: every tensor carries a zero halo
    (x/dy: the SAME padding -> test-free gather; y/dx: an arbitrary halo of 1) as the engine lays them out.
    conv_math="bf16x3" / "bf16x6": the opt-in split-bf16 products of vl_set_conv_math (padded layout, >= 40 output channels per
    group: conv1 phase-split, conv2-5 forward and dgrad, every wgrad) against the SAME oracle at the SAME tolerances."""
    rng = np.random.default_rng(h * 100 + cin)
    x = rng.standard_normal((n, h, w, cin)).astype(np.float32)
    wt = (rng.standard_normal((k, k, cin // g, cout)) / math.sqrt(k * k * cin / g)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    conv = ops.Conv(cin, h, w, cout, k, k, s, g)
    oh, _, _ = O.same_pad(h, k, s)
    ow, _, _ = O.same_pad(w, k, s)
    assert (conv.oh, conv.ow) == (oh, ow)
    xh = conv.same_pad() if padded else 0
    yh = 1 if padded else 0
    dyh = (k - 1) if padded else 0          # >= K-1-pad on every side
    dxh = 2 if padded else 0
    conv.set_halo(xh, yh, dyh, dxh)
    xd, wd, bd = dev(pad_nchw(nchw(x), xh)), dev(wt), dev(b)
    y = torch.zeros((n, cout, oh + 2 * yh, ow + 2 * yh), device=DEV)
    conv.fwd(xd, wd, bd, y, relu=False)
    z = O.grouped_conv(x, wt, b, s, g)
    close(nhwc(host(interior(y, yh))), z, msg="conv fwd")
    if yh:
        yy = host(y)
        assert np.all(yy[:, :, 0, :] == 0) and np.all(yy[:, :, :, -1] == 0)      # halo untouched
    conv.fwd(xd, wd, bd, y, relu=True)
    close(nhwc(host(interior(y, yh))), np.maximum(z, 0), msg="conv fwd+relu")

    dy = rng.standard_normal(z.shape).astype(np.float32)
    dxo, dwo, dbo = O.grouped_conv_grad(x, wt, dy, s, g, need_dx=(s == 1))
    dyd = dev(pad_nchw(nchw(dy), dyh))
    dw = torch.empty_like(wd)
    ws = torch.empty(max(conv.wgrad_ws_bytes(n) // 4, 1), device=DEV)
    conv.wgrad(xd, dyd, dw, ws)
    close(host(dw), dwo, msg="conv wgrad")
    db = torch.empty(cout, device=DEV)
    ops.bias_grad_nchw(dyd, db, torch.empty(64 * cout, device=DEV))       # halo zeros add nothing
    close(host(db), dbo, msg="bias grad")
    # the bias row rides in a spare row of the last 128-row tile of K = k*k*cin/g: not when K % 128 == 0 (conv3)
    fused = (padded or conv.same_pad() == 0) and (k * k * (cin // g)) % 128 != 0      # a 1x1 conv needs no halo to be "padded"
    assert conv.fuses_bias() == fused
    if fused:                                                             # bias gradient fused into the wgrad pass
        db2 = torch.full((cout,), 7.0, device=DEV)
        dw.zero_()
        conv.wgrad(xd, dyd, dw, ws, db=db2)
        close(host(dw), dwo, msg="conv wgrad (with fused bias grad)")
        close(host(db2), dbo, msg="fused bias grad")
    else:
        with pytest.raises(Exception):
            conv.wgrad(xd, dyd, dw, ws, db=db)
    if padded and s > 1:
        # the same conv with x stored column-phase-split (what the engine feeds conv1): identical results
        ph = conv.set_x_phase_split(True)
        assert ph == s
        xp = pad_nchw(nchw(x), xh)
        wq = -(-xp.shape[3] // ph)
        xp = np.pad(xp, ((0, 0), (0, 0), (0, 0), (0, wq * ph - xp.shape[3])))
        xps = dev(np.ascontiguousarray(xp.reshape(n, cin, xp.shape[2], wq, ph).transpose(0, 1, 4, 2, 3)).reshape(n, cin * ph, xp.shape[2], wq))
        assert tuple(xps.shape) == conv.x_shape(n)
        y2 = torch.zeros_like(y)
        conv.fwd(xps, wd, bd, y2, relu=True)
        if conv_math == "f32":
            assert torch.equal(y2, y)
        else:                                     # the phase-split layout runs the split-product kernel, the plain one fp32
            close(nhwc(host(interior(y2, yh))), np.maximum(z, 0), msg="conv fwd+relu (phase-split x, bf16x3)")
        dw2, db3 = torch.empty_like(wd), torch.empty(cout, device=DEV)
        conv.wgrad(xps, dyd, dw2, ws, db=db3 if conv.fuses_bias() else None)
        close(host(dw2), dwo, msg="conv wgrad (phase-split x)")
        with pytest.raises(Exception):
            conv.fwd(xd, wd, bd, y2, relu=True)                      # the plain layout no longer matches the descriptor
        conv.set_x_phase_split(False)
    if s == 1:
        wtt = torch.empty(wd.numel(), device=DEV)
        conv.wt_transpose(wd, wtt)
        dx = torch.zeros((n, cin, h + 2 * dxh, w + 2 * dxh), device=DEV)
        conv.dgrad(dyd, wtt, dx)
        close(nhwc(host(interior(dx, dxh))), dxo, msg="conv dgrad")
        mask = rng.standard_normal(x.shape).astype(np.float32)
        conv.dgrad(dyd, wtt, dx, relu_mask=dev(pad_nchw(nchw(mask), xh)))
        close(nhwc(host(interior(dx, dxh))), dxo * (mask > 0), msg="conv dgrad+mask")
        if dxh:
            assert np.all(host(dx)[:, :, :dxh, :] == 0)
    else:
        with pytest.raises(Exception):
            conv.dgrad(dyd, wd, torch.empty_like(xd))



def test_conv_forward_with_its_last_round_split_off_equals_the_two_half_batches(ops):
    """conv2's geometry at one rank's 128-frame shard: 1568 workgroups = 6.1 rounds of the chip, so the launcher runs 125 frames on
    128-wide tiles and the trailing 3 on 48-wide ones (dispatch_conv's tail split).  An output frame does not depend on the batch
    it was computed in (same reduction order per output in every tile width): the 128-frame call must equal two 64-frame calls,
    which are not split (and run on 48-wide tiles), bit for bit."""
    rng = np.random.default_rng(28)
    n, h, w, cin, cout, k, g = 128, 28, 28, 96, 256, 5, 2
    conv = ops.Conv(cin, h, w, cout, k, k, 1, g)
    conv.set_halo(conv.same_pad(), 1, k - 1, 2)
    xh = conv.same_pad()
    x = torch.zeros((n, cin, h + 2 * xh, w + 2 * xh), device=DEV)
    x[:, :, xh:-xh, xh:-xh] = torch.from_numpy(rng.standard_normal((n, cin, h, w)).astype(np.float32)).to(DEV)
    wt = dev((rng.standard_normal((k, k, cin // g, cout)) * 0.03).astype(np.float32))
    b = dev(rng.standard_normal(cout).astype(np.float32))
    y = torch.zeros((n, cout, h + 2, w + 2), device=DEV)
    conv.fwd(x, wt, b, y, relu=True)
    yy = torch.zeros_like(y)
    for lo in (0, 64):
        conv.fwd(x[lo:lo + 64], wt, b, yy[lo:lo + 64], relu=True)
    assert torch.equal(y, yy)
    assert float(y[125:].abs().max()) > 0 and float(y[:, :, 0].abs().max()) == 0       # the trailing frames were written; halo untouched
    # one frame against the oracle (the split's second launch: frame 126)
    z = O.grouped_conv(nhwc(host(x[126:127, :, xh:-xh, xh:-xh])), host(wt), host(b), 1, g)
    close(nhwc(host(y[126:127, :, 1:-1, 1:-1])), np.maximum(z, 0), msg="frame 126")


@pytest.mark.parametrize("conv_math", ["bf16"], indirect=True)
@pytest.mark.parametrize("n,h,w,cin,cout,k,s,g", [(2, 28, 28, 96, 256, 5, 1, 2), (3, 13, 13, 256, 384, 3, 1, 1)])
def test_conv_plain_bf16_mode(ops, conv_math, n, h, w, cin, cout, k, s, g):
    """vl_set_conv_math(1): plain bf16 products with fp32 accumulation (BASELINE config 5's reduced-precision conv path).
    Outside the fp32 tolerances by design: each contraction must land within 6e-3 relative L2 of the oracle (bf16 rounding of
    both operands: ~2.3e-3 measured) and NOT within 1e-4 (i.e. the mode really is in force)."""
    rng = np.random.default_rng(7)
    x = rng.standard_normal((n, h, w, cin)).astype(np.float32)
    wt = (rng.standard_normal((k, k, cin // g, cout)) / math.sqrt(k * k * cin / g)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    dy = rng.standard_normal((n, h, w, cout)).astype(np.float32)
    conv = ops.Conv(cin, h, w, cout, k, k, s, g)
    pad = conv.same_pad()
    conv.set_halo(pad, 0, k - 1, 0)
    xd, wd, dyd = dev(pad_nchw(nchw(x), pad)), dev(wt), dev(pad_nchw(nchw(dy), k - 1))
    y = torch.empty((n, cout, h, w), device=DEV)
    conv.fwd(xd, wd, dev(b), y, relu=False)
    dxo, dwo, _ = O.grouped_conv_grad(x, wt, dy, s, g, need_dx=True)
    wtt = torch.empty(wd.numel(), device=DEV)
    conv.wt_transpose(wd, wtt)
    dx = torch.empty((n, cin, h, w), device=DEV)
    conv.dgrad(dyd, wtt, dx)
    dw = torch.empty_like(wd)
    conv.wgrad(xd, dyd, dw, torch.empty(max(conv.wgrad_ws_bytes(n) // 4, 1), device=DEV))
    for name, got, want in (("fwd", nhwc(host(y)), O.grouped_conv(x, wt, b, s, g)), ("dgrad", nhwc(host(dx)), dxo), ("wgrad", host(dw), dwo)):
        err = np.linalg.norm(got - want) / np.linalg.norm(want)
        assert 1e-4 < err < 6e-3, (name, err)


# ---- LRN / pool ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w,c", [(2, 5, 4, 11), (2, 9, 7, 96), (1, 6, 6, 256), (3, 3, 3, 33)])
def test_lrn(ops, n, h, w, c):
    rng = np.random.default_rng(c)
    x = np.maximum(rng.standard_normal((n, h, w, c)) * 40, 0).astype(np.float32)     # relu outputs, large to exercise the scale
    dy = rng.standard_normal(x.shape).astype(np.float32)
    xd = dev(nchw(x))
    y = torch.empty_like(xd)
    ops.lrn_fwd(xd, y)
    want, _ = O.lrn(x)
    close(nhwc(host(y)), want, rtol=2e-6, atol_rel=1e-7, msg="lrn fwd")
    dx = torch.empty_like(xd)
    ops.lrn_bwd(xd, dev(nchw(dy)), dx)
    g = O.lrn_grad(x, dy)
    close(nhwc(host(dx)), g, rtol=1e-5, atol_rel=1e-6, msg="lrn bwd")
    ops.lrn_bwd(xd, dev(nchw(dy)), dx, relu_fused=True)
    close(nhwc(host(dx)), g * (x > 0), rtol=1e-5, atol_rel=1e-6, msg="lrn bwd + relu grad")
    dxp = torch.zeros((n, c, h + 4, w + 4), device=DEV)
    ops.lrn_bwd(xd, dev(nchw(dy)), dxp, dx_halo=2)
    close(nhwc(host(dxp[:, :, 2:-2, 2:-2])), g, rtol=1e-5, atol_rel=1e-6, msg="lrn bwd into a haloed dx")
    assert float(dxp[:, :, :2].abs().max()) == 0 and float(dxp[:, :, :, -2:].abs().max()) == 0


@pytest.mark.parametrize("hwc", [False, True])
@pytest.mark.parametrize("n,h,w,c", [(2, 9, 11, 3), (2, 13, 13, 16), (1, 57, 57, 5), (2, 28, 28, 7), (3, 13, 13, 256), (2, 13, 13, 70)])
def test_maxpool(ops, hwc, n, h, w, c):
    rng = np.random.default_rng(h + c)
    x = np.maximum(rng.standard_normal((n, h, w, c)), 0).astype(np.float32)           # ties at 0 like post-ReLU data
    y, arg = O.max_pool_valid(x)
    oh, ow = y.shape[1], y.shape[2]
    xd = dev(nchw(x))
    yd = torch.empty((n, oh, ow, c) if hwc else (n, c, oh, ow), device=DEV)
    ad = torch.empty(yd.shape, dtype=torch.uint8, device=DEV)
    ops.maxpool_fwd(xd, yd, ad, hwc=hwc)
    got = host(yd) if hwc else nhwc(host(yd))
    np.testing.assert_array_equal(got, y)
    ga = host(ad) if hwc else nhwc(host(ad))
    np.testing.assert_array_equal(ga, arg)
    dy = rng.standard_normal(y.shape).astype(np.float32)
    dyd = dev(dy if hwc else nchw(dy))
    dx = torch.full(xd.shape, 9.0, device=DEV)
    ops.maxpool_bwd(dyd, ad, dx, hwc=hwc)
    want = O.max_pool_valid_grad(x.shape, arg, dy.astype(np.float64))
    close(nhwc(host(dx)), want, rtol=1e-6, atol_rel=1e-7)
    ops.maxpool_bwd(dyd, ad, dx, relu_mask=xd, hwc=hwc)
    close(nhwc(host(dx)), want * (x > 0), rtol=1e-6, atol_rel=1e-7)
    if hwc:         # pool5 as the engine runs it: (h, w, c)-flat pooled tensors, dx = conv5's dy with a halo
        dxh = torch.zeros((n, c, h + 2, w + 2), device=DEV)
        ops.maxpool_bwd(dyd, ad, dxh, relu_mask=xd, hwc=True, dx_halo=1)
        close(nhwc(host(dxh[:, :, 1:-1, 1:-1])), want * (x > 0), rtol=1e-6, atol_rel=1e-7)
        assert float(dxh[:, :, 0].abs().max()) == 0 and float(dxh[:, :, :, -1].abs().max()) == 0
    if not hwc:     # haloed pool output (feeds a conv) and haloed dx (is a conv's dy)
        yp = torch.zeros((n, c, oh + 4, ow + 4), device=DEV)
        ap = torch.zeros(yp.shape, dtype=torch.uint8, device=DEV)
        ops.maxpool_fwd(xd, yp, ap, y_halo=2)
        np.testing.assert_array_equal(nhwc(host(yp[:, :, 2:-2, 2:-2])), y)
        assert float(yp[:, :, :2].abs().max()) == 0
        dyp = torch.zeros_like(yp)
        dyp[:, :, 2:-2, 2:-2] = dev(nchw(dy))
        dxp = torch.zeros((n, c, h + 2, w + 2), device=DEV)
        ops.maxpool_bwd(dyp, ap, dxp, dy_halo=2, dx_halo=1)
        close(nhwc(host(dxp[:, :, 1:-1, 1:-1])), want, rtol=1e-6, atol_rel=1e-7)
        assert float(dxp[:, :, 0].abs().max()) == 0


@pytest.mark.parametrize("n,h,w,c,ph,dh", [(2, 9, 11, 7, 0, 0), (2, 13, 13, 40, 1, 2), (1, 57, 57, 20, 2, 0), (3, 28, 28, 33, 1, 2)])
def test_pool_lrn_bwd_fused(ops, n, h, w, c, ph, dh):
    """Fused kernel == maxpool_bwd followed by lrn_bwd(+ReluGrad) of the oracle."""
    rng = np.random.default_rng(h * c)
    x = np.maximum(rng.standard_normal((n, h, w, c)) * 30, 0).astype(np.float32)
    l, _ = O.lrn(x)
    y, arg = O.max_pool_valid(l)
    oh, ow = y.shape[1], y.shape[2]
    dy = rng.standard_normal(y.shape).astype(np.float32)
    dl = O.max_pool_valid_grad(x.shape, arg, dy.astype(np.float64))
    want = O.lrn_grad(x, dl) * (x > 0)
    dp = torch.zeros((n, c, oh + 2 * ph, ow + 2 * ph), device=DEV)
    ap = torch.zeros(dp.shape, dtype=torch.uint8, device=DEV)
    interior(dp, ph).copy_(dev(nchw(dy)))
    interior(ap, ph).copy_(dev(nchw(arg), torch.uint8))
    dx = torch.zeros((n, c, h + 2 * dh, w + 2 * dh), device=DEV)
    ops.pool_lrn_bwd(dev(nchw(x)), dp, ap, dx, p_halo=ph, dx_halo=dh)
    close(nhwc(host(interior(dx, dh))), want, rtol=1e-5, atol_rel=1e-6)
    if dh:
        assert float(dx[:, :, :dh].abs().max()) == 0


def test_pool_lrn_bwd_is_bitwise_stable_beside_a_split_bf16_weight_gradient(ops):
    """Round 3's open defect in isolation (tools/plb_race_probe.py): conv2's pool / LRN backward on the main stream while conv3's
    split-bf16 weight gradient (v_cvt_pk / v_pk_add + bf16 MFMAs) runs on a second stream must give, bit for bit, what it gives alone.
    With hipcc's SLP-vectorised code (two `v_pk_add_f32 ... op_sel:[0,1]` in the kernel) about 1200 of 51 M elements differed per launch,
    all in lanes 48..63; the build now has no such instruction (tests/test_isa_lint.py)."""
    n = 128
    torch.manual_seed(0)
    y2 = torch.relu(torch.randn(n, 256, 28, 28, device=DEV) * 70.0).contiguous()
    p2 = torch.zeros(n, 256, 15, 15, device=DEV)
    arg2 = torch.zeros(n, 256, 15, 15, device=DEV, dtype=torch.uint8)
    ops.lrn_pool_fwd(y2, p2, arg2, p_halo=1)
    dp2 = torch.zeros_like(p2)
    dp2[:, :, 1:-1, 1:-1] = torch.randn(n, 256, 13, 13, device=DEV) * 1e-6
    dy2 = torch.zeros(n, 256, 32, 32, device=DEV)
    conv3 = ops.Conv(256, 13, 13, 384, 3, 3, 1, 1)
    conv3.set_halo(1, 1, 1, 1)
    dy3 = torch.zeros(n, 384, 15, 15, device=DEV)
    dy3[:, :, 1:-1, 1:-1] = torch.randn(n, 384, 13, 13, device=DEV) * 1e-3
    dw3, db3 = torch.zeros(3, 3, 256, 384, device=DEV), torch.zeros(384, device=DEV)
    side = torch.cuda.Stream()
    try:
        ops.set_conv_math("bf16x3")
        ws = torch.zeros(conv3.wgrad_ws_bytes(n) // 4 + 64, device=DEV)
        ops.pool_lrn_bwd(y2, dp2, arg2, dy2, p_halo=1, dx_halo=2)
        torch.cuda.synchronize()
        ref = dy2.clone()
        for _ in range(12):
            dy2.zero_()
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                conv3.wgrad(p2, dy3, dw3, ws, db3 if conv3.fuses_bias() else None)
            ops.pool_lrn_bwd(y2, dp2, arg2, dy2, p_halo=1, dx_halo=2)
            torch.cuda.synchronize()
            assert int((dy2 != ref).sum()) == 0
    finally:
        ops.set_conv_math("f32")


@pytest.mark.parametrize("ranges", ["1", "2", "3", "4", ""])
@pytest.mark.parametrize("n,h,w,c,ph,dh", [(2, 55, 55, 96, 2, 0), (3, 27, 27, 256, 1, 2), (2, 13, 13, 33, 1, 1)])
def test_pool_lrn_bwd_channel_ranges(ops, request, ranges, n, h, w, c, ph, dh):
    """The channel-stream backward split into 1..4 channel ranges per (band, image) (grid z; the test hook vl_pool_lrn_bwd_test_ranges forces the count, 0 =
    the dispatcher's choice): every range restarts the LRN windows 4 channels early and must reproduce the oracle at its seams --
    AlexNet's two LRN layers (5-channel chunks) and a ragged channel count (16-channel chunks)."""
    ops.pool_lrn_bwd_test_ranges(int(ranges or 0))
    request.addfinalizer(lambda: ops.pool_lrn_bwd_test_ranges(0))
    rng = np.random.default_rng(h * c + 1)
    x = np.maximum(rng.standard_normal((n, h, w, c)) * 30, 0).astype(np.float32)
    l, _ = O.lrn(x)
    y, arg = O.max_pool_valid(l)
    oh, ow = y.shape[1], y.shape[2]
    dy = rng.standard_normal(y.shape).astype(np.float32)
    want = O.lrn_grad(x, O.max_pool_valid_grad(x.shape, arg, dy.astype(np.float64))) * (x > 0)
    dp = torch.zeros((n, c, oh + 2 * ph, ow + 2 * ph), device=DEV)
    ap = torch.zeros(dp.shape, dtype=torch.uint8, device=DEV)
    interior(dp, ph).copy_(dev(nchw(dy)))
    interior(ap, ph).copy_(dev(nchw(arg), torch.uint8))
    dx = torch.full((n, c, h + 2 * dh, w + 2 * dh), float("nan"), device=DEV)
    if dh:
        dx[:, :, :dh] = 0; dx[:, :, -dh:] = 0; dx[:, :, :, :dh] = 0; dx[:, :, :, -dh:] = 0
    ops.pool_lrn_bwd(dev(nchw(x)), dp, ap, dx, p_halo=ph, dx_halo=dh)
    close(nhwc(host(interior(dx, dh))), want, rtol=1e-5, atol_rel=1e-6)          # every interior element written (no NaN left)


def near_tie_argmax(got_arg, arg, l, what=""):
    """The fused forward's arg-max (NHWC) against the fp64 oracle's `arg` of the fp64 LRN output `l`: window-local index of the first
    maximum; where the two differ, the two candidates must be a near-tie of the LRN output (the fused kernel rounds the LRN sums in a
    slightly different order than any other kernel), and fewer than 1e-3 of the outputs may differ."""
    got_arg = got_arg.astype(np.int64)
    assert got_arg.min() >= 0 and got_arg.max() <= 8, what + ": arg-max outside 0..8"
    n, oh, ow, c = got_arg.shape
    oi, oj = np.meshgrid(np.arange(oh), np.arange(ow), indexing="ij")
    def window_value(a):                                   # l at the window position a (NHWC)
        ii, jj = 2 * oi[None, :, :, None] + a // 3, 2 * oj[None, :, :, None] + a % 3
        return l[np.arange(n)[:, None, None, None], ii, jj, np.arange(c)[None, None, None, :]]
    diff = np.abs(window_value(got_arg) - window_value(arg.astype(np.int64)))
    share = float((got_arg != arg).mean())
    assert share < 1e-3 and diff.max() <= 1e-5 * np.abs(l).max(), (what, share, float(diff.max()))


@pytest.mark.parametrize("ranges", [0, 2, 3, 4])
@pytest.mark.parametrize("n,h,w,c,ph", [(2, 9, 11, 7, 0), (3, 13, 13, 20, 1), (2, 57, 57, 96, 2), (2, 28, 28, 256, 1), (1, 31, 64, 5, 0), (2, 13, 13, 41, 1)])
def test_lrn_pool_fwd_fused(ops, request, n, h, w, c, ph, ranges):
    """Fused kernel == lrn followed by max_pool_valid of the oracle (values and first-maximum arg-max), halo untouched.  `ranges`: the
    channel walk cut into that many ranges (grid z; 0 = the launcher's choice, which splits these few-image launches by itself): every
    range restarts the LRN window two channels early and must reproduce the oracle at its seams."""
    ops.pool_lrn_bwd_test_ranges(ranges)
    request.addfinalizer(lambda: ops.pool_lrn_bwd_test_ranges(0))
    rng = np.random.default_rng(h * c + w)
    x = np.maximum(rng.standard_normal((n, h, w, c)) * 30, 0).astype(np.float32)
    l, _ = O.lrn(x)
    y, arg = O.max_pool_valid(l)
    oh, ow = y.shape[1], y.shape[2]
    p = torch.full((n, c, oh + 2 * ph, ow + 2 * ph), 5.0, device=DEV)
    ap = torch.full(p.shape, 77, dtype=torch.uint8, device=DEV)
    ops.lrn_pool_fwd(dev(nchw(x)), p, ap, p_halo=ph)
    close(nhwc(host(interior(p, ph))), y, rtol=1e-5, atol_rel=1e-6)
    near_tie_argmax(nhwc(host(interior(ap, ph))), arg, l)
    if ph:      # halo ROWS untouched; the halo columns of interior rows are stored with the row: 0.0 in p, unspecified in the arg-max map
        assert float((p[:, :, :ph] - 5.0).abs().max()) == 0 and float((p[:, :, -ph:] - 5.0).abs().max()) == 0
        assert int(ap[:, :, :ph].min()) == 77 and int(ap[:, :, -ph:].min()) == 77
        assert float(p[:, :, ph:-ph, :ph].abs().max()) == 0 and float(p[:, :, ph:-ph, -ph:].abs().max()) == 0


def test_colsum(ops):
    rng = np.random.default_rng(0)
    a = rng.standard_normal((100, 300)).astype(np.float32)
    out = torch.empty(300, device=DEV)
    ops.colsum(dev(a), out, torch.empty(64 * 300, device=DEV), 100, 300)
    close(host(out), a.astype(np.float64).sum(0))


# ---- input prep ------------------------------------------------------------------------------------
def test_input_prep(ops):
    rng = np.random.default_rng(3)
    n, rh, rw, oh, ow = 5, 24, 32, 17, 19
    src = rng.integers(0, 256, (n, rh, rw, 3), dtype=np.uint8)
    cy = rng.integers(0, rh - oh + 1, n).astype(np.int32)
    cx = rng.integers(0, rw - ow + 1, n).astype(np.int32)
    mir = rng.integers(0, 2, n).astype(np.uint8)
    mean = np.array([99.197148, 105.293620, 109.503945], np.float32)
    dst = torch.empty((n, 3, oh, ow), device=DEV)
    ops.input_prep_u8(dev(src, torch.uint8), dst, dev(cy, torch.int32), dev(cx, torch.int32), dev(mir, torch.uint8), dev(mean))
    # halo 4 + column-phase-split destination (conv1's input layout): same values at [c][iw % 4][ih][iw // 4]
    halo, ph = 4, 4
    shp = ops.phase_split_shape(n, 3, oh, ow, halo, ph)
    dps = torch.zeros(shp, device=DEV)
    ops.input_prep_u8(dev(src, torch.uint8), dps, dev(cy, torch.int32), dev(cx, torch.int32), dev(mir, torch.uint8), dev(mean),
                      halo=halo, phase=ph, out_hw=(oh, ow))
    back = host(dps).reshape(n, 3, ph, oh + 2 * halo, shp[3]).transpose(0, 1, 3, 4, 2).reshape(n, 3, oh + 2 * halo, shp[3] * ph)
    assert np.array_equal(back[:, :, halo:halo + oh, halo:halo + ow], host(dst))
    assert np.all(back[:, :, :halo] == 0) and np.all(back[:, :, :, :halo] == 0) and np.all(back[:, :, :, halo + ow:] == 0)
    want = np.stack([O.process_image(src[i], (oh, ow, 3), (cy[i], cx[i]), mean, bool(mir[i])) for i in range(n)])
    np.testing.assert_array_equal(nhwc(host(dst)), want)          # bit exact: u8 -> f32 minus f32
    ops.input_prep_u8(dev(src, torch.uint8)[:, :oh, :ow].contiguous(), dst)
    np.testing.assert_array_equal(nhwc(host(dst)), src[:, :oh, :ow].astype(np.float32))
    dsth = torch.zeros((n, 3, oh + 8, ow + 8), device=DEV)
    ops.input_prep_u8(dev(src, torch.uint8), dsth, dev(cy, torch.int32), dev(cx, torch.int32), dev(mir, torch.uint8), dev(mean), halo=4)
    np.testing.assert_array_equal(nhwc(host(dsth[:, :, 4:-4, 4:-4])), want)
    assert float(dsth[:, :, :4].abs().max()) == 0 and float(dsth[:, :, :, -4:].abs().max()) == 0
    # layout converters
    x = rng.standard_normal((2, 5, 7, 3)).astype(np.float32)
    t = torch.empty((2, 3, 5, 7), device=DEV)
    ops.nhwc_to_nchw(dev(x), t)
    np.testing.assert_array_equal(host(t), nchw(x))
    th = torch.zeros((2, 3, 9, 11), device=DEV)
    ops.nhwc_to_nchw(dev(x), th, halo=2)
    np.testing.assert_array_equal(host(th[:, :, 2:-2, 2:-2]), nchw(x))
    back = torch.empty((2, 5, 7, 3), device=DEV)
    ops.nchw_to_nhwc(t, back)
    np.testing.assert_array_equal(host(back), x)


# ---- LSTM step / fusion / dropout -------------------------------------------------------------------
def test_lstm_steps_match_layer(ops):
    """Drives the step kernels + vl_gemm exactly as the host does and compares with the oracle layer."""
    rng = np.random.default_rng(11)
    b, T, d, H = 5, 4, 24, 16
    x = rng.standard_normal((b, T, d)).astype(np.float32)
    kern = (rng.standard_normal((d + H, 4 * H)) * 0.3).astype(np.float32)
    bias = (rng.standard_normal(4 * H) * 0.1).astype(np.float32)
    out, (c_last, h_last), cache = O.lstm_layer_forward(x, kern, bias)
    xd, kd, bd = dev(x.reshape(b * T, d)), dev(kern), dev(bias)
    gx = torch.empty((b * T, 4 * H), device=DEV)
    ops.gemm(xd, kd, gx, b * T, 4 * H, d, bias=bd)
    gh = torch.empty((b, 4 * H), device=DEV)
    act = torch.empty((b * T, 4 * H), device=DEV)
    cseq = torch.empty((b * T, H), device=DEV)
    hseq = torch.empty((b * T, H), device=DEV)
    hprev = torch.empty((b * T, H), device=DEV)
    kh = kd[d:]
    for t in range(T):
        if t > 0:
            ops.gemm(hseq[t - 1:], kh, gh, b, 4 * H, H, lda=T * H)
        ops.lstm_step_fwd(gx, gh if t > 0 else None, act, cseq, hseq, hprev, b, T, t, H)
    close(host(hseq).reshape(b, T, H), out, rtol=1e-5, atol_rel=1e-6, msg="lstm outputs")
    close(host(cseq).reshape(b, T, H)[:, -1], c_last, rtol=1e-5, atol_rel=1e-6)
    hp = np.concatenate([np.zeros((b, 1, H)), out[:, :-1]], axis=1)
    close(host(hprev).reshape(b, T, H), hp, rtol=1e-5, atol_rel=1e-6)

    dout = rng.standard_normal(out.shape).astype(np.float32)
    dxo, dko, dbo, _, _ = O.lstm_layer_backward(kern, cache, dout)
    dd = dev(dout.reshape(b * T, H))
    dz = torch.empty((b * T, 4 * H), device=DEV)
    dc = torch.zeros((b, H), device=DEV)
    dh = torch.empty((b, H), device=DEV)
    for t in reversed(range(T)):
        ops.lstm_step_bwd(dd, dh if t < T - 1 else None, act, cseq, dc, dz, b, T, t, H)
        if t > 0:
            ops.gemm(dz[t:], kh, dh, b, H, 4 * H, transb=True, lda=T * 4 * H)
    dk = torch.empty_like(kd)
    ops.gemm(xd, dz, dk, d, 4 * H, b * T, transa=True)
    ops.gemm(hprev, dz, dk[d:], H, 4 * H, b * T, transa=True)
    dbias = torch.empty(4 * H, device=DEV)
    ops.colsum(dz, dbias, torch.empty(64 * 4 * H, device=DEV), b * T, 4 * H)
    dx = torch.empty((b * T, d), device=DEV)
    ops.gemm(dz, kd, dx, b * T, d, 4 * H, transb=True)
    close(host(dk), dko, rtol=1e-4, atol_rel=1e-5, msg="lstm dkernel")
    close(host(dbias), dbo, rtol=1e-4, atol_rel=1e-5, msg="lstm dbias")
    close(host(dx).reshape(b, T, d), dxo, rtol=1e-4, atol_rel=1e-5, msg="lstm dx")


@pytest.mark.parametrize("b,T,d,H", [(5, 4, 24, 16), (3, 6, 40, 256), (9, 3, 12, 300), (2, 2, 8, 7),
                                     # the benchmark's LSTM (fc6 encode 4096 -> 256 hidden) at both clip lengths and at the
                                     # 8-clip shard of the 8-GPU strong-scaling run as well as the 64-clip batch
                                     (8, 16, 4096, 256), (64, 16, 4096, 256), (8, 32, 4096, 256), (64, 32, 4096, 256),
                                     (1, 16, 64, 256), (130, 5, 32, 128), (20, 7, 24, 512), (3, 4, 16, 600), (11, 21, 50, 100)])
@pytest.mark.parametrize("init", [False, True])
def test_lstm_persistent_kernels(ops, b, T, d, H, init):
    """vl_lstm_seq_fwd / _bwd (one launch per direction for all steps) against the oracle layer: the weight-stationary cluster
    form (H <= 512; groups of 1, 3, 4 and 8 clips) and the per-clip form (H = 600).  Every case here is ONE launch per direction: the
    130-clip case has H = 128, 8 workgroups per group, so a launch of a 256-CU device holds 256 clips.  The cases of several launches,
    of every group size and of ragged groups are in tests/test_lstm_geometry_gpu.py (lists MULTI, FULL, RAGGED of tests/lstm_plan.py).
    init: a non-zero initial state c0 = h0 (lstm.py:34-42) and the gradients w.r.t. it."""
    if init and d >= 1024 and b > 8:
        pytest.skip("initial state is covered at the other sizes")
    rng = np.random.default_rng(b * H)
    x = rng.standard_normal((b, T, d)).astype(np.float32)
    kern = (rng.standard_normal((d + H, 4 * H)) * (0.5 / math.sqrt(H))).astype(np.float32)
    bias = (rng.standard_normal(4 * H) * 0.1).astype(np.float32)
    s0 = (rng.standard_normal((b, H)) * 0.5).astype(np.float32) if init else None
    out, (c_last, _), cache = O.lstm_layer_forward(x, kern, bias, h0=s0, c0=s0)
    xd, kd = dev(x.reshape(b * T, d)), dev(kern)
    s0d = dev(s0) if init else None
    gx = torch.empty((b * T, 4 * H), device=DEV)
    ops.gemm(xd, kd, gx, b * T, 4 * H, d, bias=dev(bias))
    act, cseq = torch.empty((b * T, 4 * H), device=DEV), torch.empty((b * T, H), device=DEV)
    hseq, hprev = torch.empty((b * T, H), device=DEV), torch.empty((b * T, H), device=DEV)
    ws = ops.lstm_seq_ws(b, T, H, DEV)
    ws[64:].fill_(float("nan"))                                  # scratch contents before the call are irrelevant (the first 256 bytes
                                                                 # hold the sticky status word: zeroed once at allocation)
    ops.lstm_seq_fwd(gx, kd[d:], act, cseq, hseq, hprev, b, T, H, ws=ws, h0=s0d, c0=s0d)
    assert not ops.lstm_seq_timed_out(ws)
    # a 4096-term fp32 pre-activation of size ~2 carries ~5e-6 of rounding (measured 5.5e-6 .. 8.1e-6 on |h| <= 1): the per-op
    # bound of DESIGN section 2 (3e-5 of the largest element) applies there; the small cases stay at 1e-6
    tol = dict(rtol=3e-5, atol_rel=3e-5) if d >= 1024 else dict(rtol=1e-5, atol_rel=1e-6)
    close(host(hseq).reshape(b, T, H), out, msg="outputs", **tol)
    close(host(cseq).reshape(b, T, H)[:, -1], c_last, **tol)
    first = np.zeros((b, 1, H)) if s0 is None else s0[:, None, :]
    close(host(hprev).reshape(b, T, H), np.concatenate([first, out[:, :-1]], axis=1), **tol)
    dout = rng.standard_normal(out.shape).astype(np.float32)
    dxo, dko, dbo, dh0o, dc0o = O.lstm_layer_backward(kern, cache, dout)
    dz = torch.empty((b * T, 4 * H), device=DEV)
    dh0, dc0 = (torch.empty((b, H), device=DEV), torch.empty((b, H), device=DEV)) if init else (None, None)
    ops.lstm_seq_bwd(dev(dout.reshape(b * T, H)), kd[d:], act, cseq, dz, b, T, H, ws=ws, c0=s0d, dh0=dh0, dc0=dc0)
    assert not ops.lstm_seq_timed_out(ws)
    dk = torch.empty_like(kd)
    ops.gemm(xd, dz, dk, d, 4 * H, b * T, transa=True)
    ops.gemm(hprev, dz, dk[d:], H, 4 * H, b * T, transa=True)
    dx = torch.empty((b * T, d), device=DEV)
    ops.gemm(dz, kd, dx, b * T, d, 4 * H, transb=True)
    close(host(dk), dko, rtol=1e-4, atol_rel=1e-5, msg="dkernel")
    close(host(dx).reshape(b, T, d), dxo, rtol=1e-4, atol_rel=1e-5, msg="dx")
    if init:
        close(host(dh0), dh0o, rtol=1e-4, atol_rel=1e-5, msg="dh0")
        close(host(dc0), dc0o, rtol=1e-4, atol_rel=1e-5, msg="dc0")


def test_lstm_cluster_is_deterministic_and_reentrant(ops):
    """Two calls on the same workspace give bitwise identical results (the reduce-scatter of the backward sums partials in
    workgroup order; stale exchange words of the first call must not satisfy the second)."""
    rng = np.random.default_rng(3)
    b, T, H = 24, 9, 256
    gx = dev((rng.standard_normal((b * T, 4 * H)) * 1.5).astype(np.float32))
    kh = dev((rng.standard_normal((H, 4 * H)) * 0.05).astype(np.float32))
    dout = dev(rng.standard_normal((b * T, H)).astype(np.float32))
    ws = ops.lstm_seq_ws(b, T, H, DEV)
    res = []
    for _ in range(2):
        act, cseq = torch.zeros((b * T, 4 * H), device=DEV), torch.zeros((b * T, H), device=DEV)
        hseq, hprev, dz = torch.zeros((b * T, H), device=DEV), torch.zeros((b * T, H), device=DEV), torch.zeros((b * T, 4 * H), device=DEV)
        ops.lstm_seq_fwd(gx, kh, act, cseq, hseq, hprev, b, T, H, ws=ws)
        ops.lstm_seq_bwd(dout, kh, act, cseq, dz, b, T, H, ws=ws)
        assert not ops.lstm_seq_timed_out(ws)
        res.append((host(hseq), host(dz)))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert np.abs(res[0][1]).max() > 0


def test_lstm_cluster_calls_of_different_lengths_share_a_workspace(ops):
    """The exchange words are never cleared between launches (round 4): their tags are unique per launch.  A long call, then a short
    one with another batch on the same workspace, then the long one again -- every call must equal its run on a fresh workspace,
    bitwise (a stale word of an earlier call that satisfied a later one would change the values)."""
    H = 256

    def run(b, T, ws, seed):
        r = np.random.default_rng(seed)
        gx = dev((r.standard_normal((b * T, 4 * H)) * 1.5).astype(np.float32))
        kh = dev((r.standard_normal((H, 4 * H)) * 0.05).astype(np.float32))
        dout = dev(r.standard_normal((b * T, H)).astype(np.float32))
        act, cseq = torch.zeros((b * T, 4 * H), device=DEV), torch.zeros((b * T, H), device=DEV)
        hseq, hprev, dz = torch.zeros((b * T, H), device=DEV), torch.zeros((b * T, H), device=DEV), torch.zeros((b * T, 4 * H), device=DEV)
        ops.lstm_seq_fwd(gx, kh, act, cseq, hseq, hprev, b, T, H, ws=ws)
        ops.lstm_seq_bwd(dout, kh, act, cseq, dz, b, T, H, ws=ws)
        assert not ops.lstm_seq_timed_out(ws)
        return host(hseq), host(dz)

    shared = ops.lstm_seq_ws(64, 16, H, DEV)
    for b, T, seed in ((64, 16, 1), (5, 3, 2), (64, 16, 1), (17, 7, 3), (5, 3, 2)):
        got = run(b, T, shared, seed)
        want = run(b, T, ops.lstm_seq_ws(64, 16, H, DEV), seed)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (b, T)


def test_lstm_cluster_timeout_is_sticky_until_read(ops):
    """A workgroup that never hears from a peer gives up after the spin limit and raises the status word (wrong results, no
    hang).  The word is sticky: a later healthy launch on the same workspace does not clear it; reading it does.
    Forced with the library's test hooks: workgroup 0 publishes nothing, 64 polls instead of 2^18."""
    rng = np.random.default_rng(4)
    b, T, H = 8, 6, 256
    gx = dev((rng.standard_normal((b * T, 4 * H)) * 1.5).astype(np.float32))
    kh = dev((rng.standard_normal((H, 4 * H)) * 0.05).astype(np.float32))
    dout = dev(rng.standard_normal((b * T, H)).astype(np.float32))
    ws = ops.lstm_seq_ws(b, T, H, DEV)
    act, cseq = torch.zeros((b * T, 4 * H), device=DEV), torch.zeros((b * T, H), device=DEV)
    hseq, hprev, dz = torch.zeros((b * T, H), device=DEV), torch.zeros((b * T, H), device=DEV), torch.zeros((b * T, 4 * H), device=DEV)
    try:
        ops.lstm_seq_test_hooks(spin_limit=64, mute_workgroup=0)
        ops.lstm_seq_fwd(gx, kh, act, cseq, hseq, hprev, b, T, H, ws=ws)
        torch.cuda.synchronize()
    finally:
        ops.lstm_seq_test_hooks()
    ops.lstm_seq_bwd(dout, kh, act, cseq, dz, b, T, H, ws=ws)        # healthy launch: must not erase the forward's flag
    assert ops.lstm_seq_timed_out(ws)
    assert not ops.lstm_seq_timed_out(ws)                            # the read reset it
    ops.lstm_seq_fwd(gx, kh, act, cseq, hseq, hprev, b, T, H, ws=ws)
    ops.lstm_seq_bwd(dout, kh, act, cseq, dz, b, T, H, ws=ws)
    assert not ops.lstm_seq_timed_out(ws)
    try:
        ops.lstm_seq_test_hooks(spin_limit=64, mute_workgroup=3)
        ops.lstm_seq_bwd(dout, kh, act, cseq, dz, b, T, H, ws=ws)
        torch.cuda.synchronize()
    finally:
        ops.lstm_seq_test_hooks()
    with pytest.raises(Exception, match="timed out"):
        ops.lstm_seq_check(ws)


@pytest.mark.parametrize("method", ["avg", "last"])
def test_temporal_fusion(ops, method):
    rng = np.random.default_rng(5)
    b, T, H = 3, 5, 7
    x = rng.standard_normal((b, T, H)).astype(np.float32)
    y = torch.empty((b, H), device=DEV)
    ops.temporal_fusion_fwd(dev(x), y, b, T, H, method)
    close(host(y), O.temporal_fusion(x.astype(np.float64), method), rtol=1e-6, atol_rel=1e-7)
    dy = rng.standard_normal((b, H)).astype(np.float32)
    dx = torch.empty((b, T, H), device=DEV)
    ops.temporal_fusion_bwd(dev(dy), dx, b, T, H, method)
    close(host(dx), O.temporal_fusion_grad(x.shape, method, dy.astype(np.float64)), rtol=1e-6, atol_rel=1e-7)


def test_dropout(ops):
    n, keep = 1 << 16, 0.5
    x = torch.ones(n, device=DEV)
    y = torch.empty(n, device=DEV)
    m = torch.empty(n, dtype=torch.uint8, device=DEV)
    ops.dropout_fwd(x, y, m, keep, 1234)
    yh, mh = host(y), host(m)
    assert set(np.unique(yh)) <= {0.0, 2.0} and np.array_equal(yh > 0, mh > 0)
    assert abs(mh.mean() - keep) < 0.01
    y2 = torch.empty(n, device=DEV)
    ops.dropout_fwd(x, y2, m, keep, 1234)
    assert np.array_equal(host(y2), yh)                         # counter based: same seed, same mask
    ops.dropout_fwd(x, y2, torch.empty_like(m), keep, 99)
    assert not np.array_equal(host(y2), yh)
    dx = torch.empty(n, device=DEV)
    ops.dropout_bwd(x, m, dx, keep)
    assert np.array_equal(host(dx), yh)


# ---- loss / optimizer --------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_ws", [False, True])
@pytest.mark.parametrize("b,c", [(6, 9), (64, 101), (9, 200), (1344, 1000)])
def test_softmax_xent(ops, b, c, rows_ws):
    """rows_ws: one wave per row over the chip + fixed-order sum (the engines' path) vs one workgroup walking the batch."""
    rng = np.random.default_rng(b)
    z = (rng.standard_normal((b, c)) * 5).astype(np.float32)
    lab = rng.integers(0, c, b)
    z[0, lab[0]] = 50.0                                         # at least one correct prediction
    onehot = O.labels_to_one_hot([[l] for l in lab], c)
    loss, dz = O.softmax_xent_mean(z, onehot)
    stats = torch.zeros(2, device=DEV)
    dl = torch.empty((b, c), device=DEV)
    rows = torch.full((2 * b,), float("nan"), device=DEV) if rows_ws else None
    ops.softmax_xent(dev(z), dev(onehot, torch.int32), dl, stats, 1.0 / b, rows)
    s = host(stats)
    assert abs(s[0] / b - loss) < 1e-5 * max(1.0, abs(loss))
    if rows_ws:                                                 # the workspace holds the per-row terms; twice gives the same bits
        r = host(rows)
        assert abs(r[:b].astype(np.float64).sum() / b - loss) < 1e-5 * max(1.0, abs(loss))
        stats2 = torch.zeros(2, device=DEV)
        ops.softmax_xent(dev(z), dev(onehot, torch.int32), dl, stats2, 1.0 / b, rows)
        assert host(stats2).tobytes() == s.tobytes()
    assert s[1] == round(O.accuracy(z, onehot) * b)
    close(host(dl), dz, rtol=1e-4, atol_rel=1e-6)


def test_optimizer(ops):
    rng = np.random.default_rng(2)
    n = 100003
    w = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * 3).astype(np.float32)
    ss = torch.zeros(1, device=DEV)
    ws = torch.empty(1024, device=DEV)
    gd = dev(g)
    ops.sumsq(gd[:50000], ss, ws)
    ops.sumsq(gd[50000:], ss, ws, accumulate=True)
    want_ss = float((g.astype(np.float64) ** 2).sum())
    assert abs(host(ss)[0] - want_ss) / want_ss < 1e-6
    for clip, gscale in [(10.0, 1.0), (1e9, 1.0), (0.0, 1.0), (10.0, 0.125)]:
        wd = dev(w)
        ops.sgd_apply(wd, gd, 0.01, clip, ss, gscale)
        norm = gscale * math.sqrt(want_ss)
        scale = gscale * (clip / max(norm, clip) if clip > 0 else 1.0)
        close(host(wd), w - 0.01 * scale * g.astype(np.float64), rtol=1e-6, atol_rel=1e-7)
    # Adam, two steps, TF formulation (train.py:205-206)
    wd, m, v = dev(w), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    wr, mr, vr = w.astype(np.float64), np.zeros(n), np.zeros(n)
    for step in (1, 2):
        ops.adam_apply(wd, gd, m, v, 0.001, step)
        mr = 0.9 * mr + 0.1 * g
        vr = 0.999 * vr + 0.001 * g.astype(np.float64) ** 2
        lr_t = 0.001 * math.sqrt(1 - 0.999 ** step) / (1 - 0.9 ** step)
        wr = wr - lr_t * mr / (np.sqrt(vr) + 1e-8)
    close(host(wd), wr, rtol=1e-5, atol_rel=1e-6)
    f = torch.empty(1000, device=DEV)
    ops.fill(f, 0.1)
    assert np.all(host(f) == np.float32(0.1))
