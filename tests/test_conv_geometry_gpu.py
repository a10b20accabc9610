"""Conv kernels against the oracle OUTSIDE AlexNet's geometry: what vl_conv_create accepts (kh and kw apart, any stride, any group
count) and the table builders carry (four independent paddings), not only the five layers of the other conv tests.

  - asymmetric SAME padding at stride 1 (even kernels: pad before (k-1)//2 < pad after k//2): the dgrad rule "pad dy by k-1-pad
    before", the bwd_padded test, the x_halo - pad shifts of the packed-bf16 tap tables, the ring kernels' 16-byte fetches;
  - kh != kw (k_to_row, the weight transpose and the tables are all that tell the two apart);
  - strides 2 and 3 (the phase-split x layout at phase 2 / 3, a kernel smaller than the stride, a strided 1x1);
  - more than two groups, channels per group that are no multiple of 16 (natural reduction order inside a grouped launch);
  - planes smaller than the kernel (taps wholly in the halo; the "row of padding only" exit of the row-class builder);
  - the many-frames branches of dispatch_conv no AlexNet layer selects (test_many_frames).

The oracle is oracle/lrcn_oracle.py (fp64 numpy; tests/test_oracle.py pins it at these geometries against torch-CPU), the tolerance
test_ops_gpu's `close` (DESIGN 2's per-op bound) for fp32, bf16x3, bf16x6 and the packed path on bf16-rounded operands; the in-loop bf16
mode keeps test_conv_plain_bf16_mode's band.  Every bitwise claim is exact equality.  Outputs are filled with a sentinel before each
call: every interior element must have been written and no halo element touched.

The CPU tests at the end (not marked gpu) show that the cases discriminate: a kernel that swapped the paddings, swapped kh and kw or
used the forward padding in dgrad would miss the oracle by far more than `close` allows."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import lrcn_oracle as O

DEV = "cuda:0"
SENTINEL = 12345.0

# ---- the cases: n, h, w, cin, cout, kh, kw, stride, groups ----------------------------------------------------------------------
EVEN = [(2, 9, 8, 16, 40, 2, 2, 1, 1), (3, 13, 11, 32, 48, 4, 4, 1, 2), (2, 10, 10, 24, 100, 6, 6, 1, 1)]
NONSQUARE = [(2, 10, 7, 16, 40, 3, 5, 1, 1), (2, 10, 7, 32, 96, 5, 3, 1, 2), (2, 5, 9, 16, 24, 1, 7, 1, 1), (2, 9, 5, 16, 24, 7, 1, 1, 1),
             (2, 12, 9, 12, 20, 2, 3, 1, 1)]
STRIDED = [(2, 11, 13, 6, 9, 3, 3, 2, 3), (2, 31, 29, 3, 64, 7, 7, 2, 1), (2, 23, 20, 3, 32, 5, 5, 3, 1), (2, 13, 12, 3, 8, 6, 6, 2, 1),
           (2, 12, 12, 8, 16, 1, 1, 2, 1), (2, 14, 14, 8, 16, 2, 2, 3, 1)]       # the last two: kernel smaller than the stride
GROUPED = [(2, 9, 9, 48, 48, 3, 3, 1, 3), (2, 9, 9, 64, 128, 3, 3, 1, 4), (2, 9, 9, 24, 24, 3, 3, 1, 24)]
SMALL_PLANE = [(3, 3, 3, 16, 32, 5, 5, 1, 2), (3, 2, 2, 16, 16, 3, 3, 1, 1), (3, 1, 1, 32, 48, 3, 3, 1, 1), (2, 4, 3, 16, 16, 5, 5, 1, 1),
               (2, 2, 9, 16, 16, 5, 3, 1, 1)]
FP32_CASES = EVEN + NONSQUARE + STRIDED + GROUPED + SMALL_PLANE

# ragged OW with an asymmetric left pad: the ring kernels fetch four output columns as 16 bytes, rows enumerated ceil4(OW) wide
RING_EXTRA = [(2, 9, 10, 48, 48, 4, 4, 1, 1), (2, 7, 13, 96, 128, 2, 3, 1, 1)]


def ring_width(c):
    """dispatch_conv: under vl_set_conv_math the contraction with c output channels per group runs launch_conv_ring<64> / <128>."""
    return 40 <= c <= 64 or c >= 96


# forward (cout / groups) or dgrad (cin / groups, stride 1) takes a ring kernel
SPLIT_CASES = [c for c in FP32_CASES if ring_width(c[4] // c[8]) or (c[7] == 1 and ring_width(c[3] // c[8]))] + RING_EXTRA

C8_CASES = [(3, 13, 11, 32, 48, 4, 4, 1, 2), (2, 9, 8, 16, 40, 2, 2, 1, 1), (2, 10, 7, 32, 96, 5, 3, 1, 2), (2, 10, 7, 16, 40, 3, 5, 1, 1),
            (2, 9, 9, 64, 128, 3, 3, 1, 4), (3, 2, 2, 16, 16, 3, 3, 1, 1), (3, 1, 1, 32, 48, 3, 3, 1, 1), (4, 3, 3, 16, 32, 5, 5, 1, 2)]
C8_STRIDED = (2, 11, 13, 8, 16, 3, 3, 2, 1)

# h, w, cin, cout, kh, kw, groups (stride 1, padded layout; the frame count comes from the device: many_frames)
MANY = [(64, 64, 128, 512, 3, 3, 8),      # forward 64 channels per group: launch_conv<64,1,4,true>; dgrad 16: dma48
        (64, 64, 128, 128, 4, 4, 8),      # 16 both ways: dma48 with four asymmetric row classes
        (64, 64, 64, 384, 3, 5, 4),       # forward 96: dma96, non-square; dgrad 16
        (32, 32, 128, 1024, 5, 5, 8)]     # forward 128: dma128, five classes at a non-AlexNet plane; dgrad 16


def case_id(c):
    return "-".join(str(v) for v in c)


@pytest.fixture(scope="module")
def ops():
    import vltf_amd.ops as ops_
    return ops_


@pytest.fixture
def conv_math(ops, request):
    ops.set_conv_math(request.param)
    assert ops.conv_math() == request.param
    yield request.param
    ops.set_conv_math("f32")


@pytest.fixture
def hook(ops):
    yield ops.conv_set_row_classes
    ops.conv_set_row_classes(True)


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def nchw(a):
    return np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2)))


def nhwc(a):
    return np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))


def close(got, want, rtol=3e-5, atol_rel=3e-5, msg=""):     # test_ops_gpu.close
    want = np.asarray(want, np.float64)
    scale = float(np.abs(want).max()) or 1.0
    np.testing.assert_allclose(np.asarray(got, np.float64), want, rtol=rtol, atol=atol_rel * scale, err_msg=msg)


def pad_nchw(a_nchw, halo):
    return np.pad(a_nchw, ((0, 0), (0, 0), (halo, halo), (halo, halo)))


def interior(t, halo):
    return t if halo == 0 else t[:, :, halo:-halo, halo:-halo]


def written(out, halo, what):
    """The sentinel-filled output after a call, on the host: every interior element written, no halo element touched."""
    a = host(out)
    assert not (interior(a, halo) == SENTINEL).any(), "%s: interior not fully written" % what
    if halo:
        frame = a.copy()
        interior(frame, halo)[...] = SENTINEL
        assert np.all(frame == SENTINEL), "%s: halo touched" % what
    return a


def conv_inputs(rng, n, h, w, cin, cout, kh, kw, g):
    x = rng.standard_normal((n, h, w, cin)).astype(np.float32)
    wt = (rng.standard_normal((kh, kw, cin // g, cout)) / math.sqrt(kh * kw * cin / g)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    return x, wt, b


def phase_split(xp, ph):
    """Padded NCHW -> the column-phase-split layout of vl_conv_set_x_phase_split."""
    n, c, hp, wp = xp.shape
    wq = -(-wp // ph)
    xp = np.pad(xp, ((0, 0), (0, 0), (0, 0), (0, wq * ph - wp)))
    return np.ascontiguousarray(xp.reshape(n, c, hp, wq, ph).transpose(0, 1, 4, 2, 3)).reshape(n, c * ph, hp, wq)


def check(mode, in_mode, got, want, msg):
    """fp32 / bf16x3 / bf16x6: `close`.  bf16, where the contraction runs in that arithmetic: test_conv_plain_bf16_mode's band."""
    if mode == "bf16" and in_mode:
        err = np.linalg.norm(np.asarray(got, np.float64) - want) / np.linalg.norm(want)
        print("%s: relative L2 %.3e" % (msg, err))
        assert 1e-4 < err < 6e-3, (msg, err)
    else:
        close(got, want, msg=msg)


def run_conv_case(ops, mode, padded, n, h, w, cin, cout, kh, kw, s, g):
    """test_ops_gpu.test_conv_fwd_bwd's protocol with kh and kw apart and sentinel-filled outputs."""
    rng = np.random.default_rng(h * 100 + cin)
    x, wt, b = conv_inputs(rng, n, h, w, cin, cout, kh, kw, g)
    conv = ops.Conv(cin, h, w, cout, kh, kw, s, g)
    oh, _, _ = O.same_pad(h, kh, s)
    ow, _, _ = O.same_pad(w, kw, s)
    assert (conv.oh, conv.ow) == (oh, ow)
    xh = conv.same_pad() if padded else 0          # the largest of the four sides
    yh = 1 if padded else 0
    dyh = (max(kh, kw) - 1) if padded else 0       # >= k-1-pad and >= pad on every side
    dxh = 2 if padded else 0
    conv.set_halo(xh, yh, dyh, dxh)
    is_padded = padded or conv.same_pad() == 0     # a layer without padding needs no halo to be "padded"
    # the contractions that run in the arithmetic of `mode` (include/vltf.h: vl_set_conv_math; dispatch_conv)
    fwd_ring = padded and s == 1 and ring_width(cout // g)
    dgrad_ring = padded and ring_width(cin // g)
    xd, wd, bd = dev(pad_nchw(nchw(x), xh)), dev(wt), dev(b)
    y = torch.full((n, cout, oh + 2 * yh, ow + 2 * yh), SENTINEL, device=DEV)
    conv.fwd(xd, wd, bd, y, relu=False)
    z = O.grouped_conv(x, wt, b, s, g)
    check(mode, fwd_ring, nhwc(interior(written(y, yh, "fwd"), yh)), z, "conv fwd")
    y.fill_(SENTINEL)
    conv.fwd(xd, wd, bd, y, relu=True)
    yrelu = written(y, yh, "fwd+relu")
    check(mode, fwd_ring, nhwc(interior(yrelu, yh)), np.maximum(z, 0), "conv fwd+relu")

    dy = rng.standard_normal(z.shape).astype(np.float32)
    dxo, dwo, dbo = O.grouped_conv_grad(x, wt, dy, s, g, need_dx=(s == 1))
    dyd = dev(pad_nchw(nchw(dy), dyh))
    dw = torch.full(conv.w_shape, SENTINEL, device=DEV)
    ws = torch.empty(max(conv.wgrad_ws_bytes(n) // 4, 1), device=DEV)
    conv.wgrad(xd, dyd, dw, ws)
    assert not bool((dw == SENTINEL).any())
    check(mode, is_padded, host(dw), dwo, "conv wgrad")
    db = torch.full((cout,), SENTINEL, device=DEV)
    ops.bias_grad_nchw(dyd, db, torch.empty(64 * cout, device=DEV))       # halo zeros add nothing
    close(host(db), dbo, msg="bias grad")
    # the bias row rides in a spare row of the last 128-row tile of K = kh*kw*cin/g
    fused = is_padded and (kh * kw * (cin // g)) % 128 != 0
    assert conv.fuses_bias() == fused
    if fused:
        db2 = torch.full((cout,), SENTINEL, device=DEV)
        dw.fill_(SENTINEL)
        conv.wgrad(xd, dyd, dw, ws, db=db2)
        check(mode, is_padded, host(dw), dwo, "conv wgrad (with fused bias grad)")
        check(mode, is_padded, host(db2), dbo, "fused bias grad")          # a row of the same contraction: dy in the mode's arithmetic
    else:
        with pytest.raises(Exception):
            conv.wgrad(xd, dyd, dw, ws, db=db)
    if padded and s > 1:
        # the same conv with x stored column-phase-split: identical results (fp32); under a split mode this layout runs the ring kernel
        ph = conv.set_x_phase_split(True)
        assert ph == s
        xps = dev(phase_split(pad_nchw(nchw(x), xh), ph))
        assert tuple(xps.shape) == conv.x_shape(n)
        y2 = torch.full_like(y, SENTINEL)
        conv.fwd(xps, wd, bd, y2, relu=True)
        y2h = written(y2, yh, "fwd (phase-split x)")
        if mode == "f32":
            assert np.array_equal(y2h, yrelu), "phase-split x: not bitwise the plain layout"
        else:
            check(mode, ring_width(cout // g), nhwc(interior(y2h, yh)), np.maximum(z, 0), "conv fwd+relu (phase-split x)")
        dw2, db3 = torch.full(conv.w_shape, SENTINEL, device=DEV), torch.empty(cout, device=DEV)
        conv.wgrad(xps, dyd, dw2, ws, db=db3 if conv.fuses_bias() else None)
        check(mode, True, host(dw2), dwo, "conv wgrad (phase-split x)")
        with pytest.raises(Exception):
            conv.fwd(xd, wd, bd, y2, relu=True)                      # the plain layout no longer matches the descriptor
        conv.set_x_phase_split(False)
    if s == 1:
        wtt = torch.empty(wd.numel(), device=DEV)
        conv.wt_transpose(wd, wtt)
        want_wtt = np.concatenate([wt[::-1, ::-1, :, i * (cout // g):(i + 1) * (cout // g)].transpose(0, 1, 3, 2) for i in range(g)], axis=3)
        assert np.array_equal(host(wtt).reshape(want_wtt.shape), want_wtt), "wt_transpose"
        dx = torch.full((n, cin, h + 2 * dxh, w + 2 * dxh), SENTINEL, device=DEV)
        conv.dgrad(dyd, wtt, dx)
        check(mode, dgrad_ring, nhwc(interior(written(dx, dxh, "dgrad"), dxh)), dxo, "conv dgrad")
        mask = rng.standard_normal(x.shape).astype(np.float32)
        dx.fill_(SENTINEL)
        conv.dgrad(dyd, wtt, dx, relu_mask=dev(pad_nchw(nchw(mask), xh)))
        check(mode, dgrad_ring, nhwc(interior(written(dx, dxh, "dgrad+mask"), dxh)), dxo * (mask > 0), "conv dgrad+mask")
    else:
        dx = torch.full((n, cin, h + 2 * dxh, w + 2 * dxh), SENTINEL, device=DEV)
        with pytest.raises(Exception, match="stride-1"):
            conv.dgrad(dyd, wd, dx)
        assert bool((dx == SENTINEL).all()), "a refused dgrad wrote its output"


# ---- fp32 kernels at few frames ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("case", FP32_CASES, ids=case_id)
def test_conv_fp32(ops, case, padded):
    """padded=False: dense NCHW, bounds-tested gather.  padded=True: x carries the largest SAME padding as its halo, y 1, dy
    max(kh,kw)-1, dx 2 (the LDS-DMA kernels of dispatch_conv's few-frames branch)."""
    assert ops.conv_math() == "f32"
    run_conv_case(ops, "f32", padded, *case)


# ---- split-bf16 modes and the in-loop bf16 mode -----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("conv_math", ["bf16x3", "bf16x6", "bf16"], indirect=True)
@pytest.mark.parametrize("case", SPLIT_CASES, ids=case_id)
def test_conv_split_modes(ops, conv_math, case):
    """The ring kernels (40..64 or >= 96 output channels per group in forward or dgrad; a strided layer through its phase-split x)
    and every wgrad, padded layout, against the SAME oracle: bf16x3 / bf16x6 at `close`; bf16 at 1e-4 < relative L2 < 6e-3 for the
    contractions that run in that mode (the others keep fp32 arithmetic and `close`)."""
    run_conv_case(ops, conv_math, True, *case)


# ---- the packed-bf16 path -----------------------------------------------------------------------------------------------------------
def bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy()


def to_c8(a_nhwc, halo):
    """NHWC fp32 (values already bf16-representable) -> device bf16 [n][cb][h + 2 halo][w + 2 halo][8]."""
    n, h, w, c = a_nhwc.shape
    cb = (c + 7) // 8
    full = np.zeros((n, h + 2 * halo, w + 2 * halo, cb * 8), np.float32)
    full[:, halo:halo + h, halo:halo + w, :c] = a_nhwc
    t = torch.from_numpy(np.ascontiguousarray(full.reshape(n, h + 2 * halo, w + 2 * halo, cb, 8).transpose(0, 3, 1, 2, 4)))
    return t.to(DEV).bfloat16().contiguous()


def from_c8(t, c, halo):
    """device c8 -> host NHWC fp32 interior, + the halo / channel-padding values (must be zero)."""
    torch.cuda.synchronize()
    a = t.float().cpu().numpy()                                   # [n][cb][hp][wp][8]
    n, cb, hp, wp, _ = a.shape
    full = a.transpose(0, 2, 3, 1, 4).reshape(n, hp, wp, cb * 8)
    inner = full[:, halo:hp - halo, halo:wp - halo, :c]
    outside = full.copy()
    outside[:, halo:hp - halo, halo:wp - halo, :c] = 0
    return np.ascontiguousarray(inner), outside


@pytest.mark.gpu
@pytest.mark.parametrize("case", C8_CASES, ids=case_id)
def test_conv_c8(ops, case):
    """test_conv_c8_gpu.test_conv_c8_fwd_dgrad_wgrad's protocol (operands rounded to bf16 first, the oracle on the rounded operands,
    `close` at the fp32 tolerance) with x_halo = dy_halo = the largest SAME padding."""
    n, h, w, cin, cout, kh, kw, s, g = case
    rng = np.random.default_rng(h * 100 + cin)
    x = bf16_round(np.maximum(rng.standard_normal((n, h, w, cin)), 0))             # post-ReLU-like input (zeros included)
    wt = (rng.standard_normal((kh, kw, cin // g, cout)) / math.sqrt(kh * kw * cin / g)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    dy = bf16_round(rng.standard_normal((n, h, w, cout)))
    wr = bf16_round(wt)
    conv = ops.Conv(cin, h, w, cout, kh, kw, 1, g)
    pad = conv.same_pad()
    conv.set_halo(pad, 1, pad, 2)                                                  # x / dy: the SAME padding; y: 1; dx: 2
    xb, dyb = to_c8(x, pad), to_c8(dy, pad)
    wd, bd = torch.from_numpy(wt).to(DEV), torch.from_numpy(b).to(DEV)
    wb = torch.zeros(conv.c8_w_bytes(False), dtype=torch.uint8, device=DEV)
    wbt = torch.zeros(conv.c8_w_bytes(True), dtype=torch.uint8, device=DEV)
    conv.c8_pack_w(wd, wb, False)
    conv.c8_pack_w(wd, wbt, True)

    # forward: fp32 NCHW and c8 outputs of the same launch
    z = O.grouped_conv(x, wr, b, 1, g)
    y = torch.full((n, cout, h + 2, w + 2), SENTINEL, device=DEV)
    yb = torch.zeros(ops.c8_shape(n, cout, h, w, 1), dtype=torch.bfloat16, device=DEV)
    conv.c8_fwd(xb, wb, bd, y=y, yb=yb, relu=False)
    yh = written(y, 1, "c8 fwd")
    close(nhwc(yh[:, :, 1:-1, 1:-1]), z, msg="c8 fwd (fp32 out)")
    inner, outside = from_c8(yb, cout, 1)
    assert np.array_equal(inner, bf16_round(nhwc(yh[:, :, 1:-1, 1:-1]))), "c8 output = bf16 rounding of the fp32 output"
    assert not outside.any()
    y.fill_(SENTINEL)
    conv.c8_fwd(xb, wb, bd, y=y, relu=True)
    close(nhwc(written(y, 1, "c8 fwd + relu")[:, :, 1:-1, 1:-1]), np.maximum(z, 0), msg="c8 fwd + relu")
    conv.set_halo(pad, 0, pad, 2)                                                  # dense y: the LDS-staged 16-byte store path
    yd = torch.full((n, cout, h, w), SENTINEL, device=DEV)
    conv.c8_fwd(xb, wb, bd, y=yd, relu=False)
    close(nhwc(written(yd, 0, "c8 fwd (dense)")), z, msg="c8 fwd (dense fp32 out)")
    conv.set_halo(pad, 1, pad, 2)

    dxo, dwo, _ = O.grouped_conv_grad(x, wr, dy, 1, g, need_dx=True)
    dx = torch.full((n, cin, h + 4, w + 4), SENTINEL, device=DEV)
    dxb = torch.zeros(ops.c8_shape(n, cin, h, w, 2), dtype=torch.bfloat16, device=DEV)
    conv.c8_dgrad(dyb, wbt, dx=dx, dxb=dxb)
    dxh = written(dx, 2, "c8 dgrad")
    close(nhwc(dxh[:, :, 2:-2, 2:-2]), dxo, msg="c8 dgrad")
    inner, outside = from_c8(dxb, cin, 2)
    assert np.array_equal(inner, bf16_round(nhwc(dxh[:, :, 2:-2, 2:-2]))) and not outside.any()
    mask = rng.standard_normal(x.shape).astype(np.float32)
    dx.fill_(SENTINEL)
    conv.c8_dgrad(dyb, wbt, dx=dx, relu_mask=torch.from_numpy(pad_nchw(nchw(mask), 2)).to(DEV))
    close(nhwc(written(dx, 2, "c8 dgrad + mask")[:, :, 2:-2, 2:-2]), dxo * (mask > 0), msg="c8 dgrad + mask")
    dx.fill_(SENTINEL)
    conv.c8_dgrad(dyb, wbt, dx=dx, relu_mask_c8=xb)                                # ReluGrad from the layer's own packed input
    close(nhwc(written(dx, 2, "c8 dgrad + packed mask")[:, :, 2:-2, 2:-2]), dxo * (x > 0), msg="c8 dgrad + packed mask")
    # wgrad (twice: bitwise reproducible)
    dw = torch.full(conv.w_shape, SENTINEL, device=DEV)
    ws = torch.empty(max(conv.c8_wgrad_ws_bytes(n) // 4, 1), device=DEV)
    conv.c8_wgrad(xb, dyb, dw, ws)
    assert not bool((dw == SENTINEL).any())
    close(host(dw), dwo, msg="c8 wgrad")
    dw2 = torch.full(conv.w_shape, SENTINEL, device=DEV)
    conv.c8_wgrad(xb, dyb, dw2, ws)
    assert torch.equal(dw, dw2)


@pytest.mark.gpu
def test_conv_c8_strided_forward(ops):
    """vl_conv_c8_fwd has no stride check of its own: a strided layer must either agree with the oracle or be refused (and then
    leave its output alone)."""
    from vltf_amd._ffi import VltfError
    n, h, w, cin, cout, kh, kw, s, g = C8_STRIDED
    rng = np.random.default_rng(h * 100 + cin)
    x = bf16_round(rng.standard_normal((n, h, w, cin)))
    wt = (rng.standard_normal((kh, kw, cin // g, cout)) / math.sqrt(kh * kw * cin / g)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    conv = ops.Conv(cin, h, w, cout, kh, kw, s, g)
    pad = conv.same_pad()
    conv.set_halo(pad, 1, pad, 2)
    wd = torch.from_numpy(wt).to(DEV)
    wb = torch.zeros(conv.c8_w_bytes(False), dtype=torch.uint8, device=DEV)
    conv.c8_pack_w(wd, wb, False)
    y = torch.full((n, cout, conv.oh + 2, conv.ow + 2), SENTINEL, device=DEV)
    try:
        conv.c8_fwd(to_c8(x, pad), wb, torch.from_numpy(b).to(DEV), y=y, relu=False)
    except VltfError as e:
        print("c8 strided forward refused: %s" % e)
        assert bool((y == SENTINEL).all()), "a refused c8 forward wrote its output"
        return
    print("c8 strided forward ran")
    z = O.grouped_conv(x, bf16_round(wt), b, s, g)
    close(nhwc(written(y, 1, "c8 strided fwd")[:, :, 1:-1, 1:-1]), z, msg="c8 strided fwd")


# ---- the many-frames branches ---------------------------------------------------------------------------------------------------------
def many_frames(h, w, cog, g, cus):
    """Smallest frame count with ceil(n h w / 128) * ceil(cog / 128) * g >= 1.1 * 8 * cus (dispatch_conv's `few` is false, 10 % to spare)."""
    px = -(-int(1.1 * 8 * cus * 1000) // (1000 * -(-cog // 128) * g))
    return -(-px * 128 // (h * w))


def sample_frames(n):
    return sorted({0, n // 2, n - 1})


def on_and_off(hook, run, out, halo):
    """run() with the row-class hook off and on into the sentinel-filled `out`: interior written, halo untouched, the two results
    equal bit for bit; returns the hook-on result on the host."""
    res = []
    for on in (False, True):
        hook(on)
        out.fill_(SENTINEL)
        run()
        res.append(written(out, halo, "row classes %s" % ("on" if on else "off")))
    assert np.array_equal(res[1], res[0]), "row classes on != off"
    return res[1]


@pytest.mark.gpu
@pytest.mark.parametrize("case", MANY, ids=case_id)
def test_many_frames(ops, hook, case):
    """dispatch_conv leaves its few-frames branch (which only launches the LDS-DMA kernels in the flat pixel order) when
        ceil(M / 128) * ceil(Cog / 128) * groups >= 8 * CUs        M = frames * OH * OW, Cog = output channels per group of the launch
    The frame count is computed from the device's CU count so that this holds with 10 % to spare for forward (Cog = cout / g) and
    dgrad (Cog = cin / g) alike: with 8 groups that is 9 frames of 64x64 on 256 CUs.  Forward and dgrad: hook on == hook off bit for
    bit, first / middle / last frame against the oracle; wgrad once against the oracle's dw over ALL frames."""
    h, w, cin, cout, kh, kw, g = case
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = max(many_frames(h, w, cout // g, g, cus), many_frames(h, w, cin // g, g, cus))
    for cog in (cout // g, cin // g):
        assert -(-n * h * w // 128) * -(-cog // 128) * g >= 8 * cus            # not `few`
    print("many frames: %d CUs, n = %d for %s" % (cus, n, (h, w, cin, cout, kh, kw, g)))
    gen = torch.Generator(device=DEV)
    gen.manual_seed(h * 7 + cout)
    conv = ops.Conv(cin, h, w, cout, kh, kw, 1, g)
    xh, yh, dyh, dxh = conv.same_pad(), 1, max(kh, kw) - 1, 2
    conv.set_halo(xh, yh, dyh, dxh)

    def haloed(c, halo):
        t = torch.zeros((n, c, h + 2 * halo, w + 2 * halo), device=DEV)
        interior(t, halo).copy_(torch.randn((n, c, h, w), device=DEV, generator=gen))
        return t
    x, dy, mask = haloed(cin, xh), haloed(cout, dyh), haloed(cin, xh)
    wt = torch.randn((kh, kw, cin // g, cout), device=DEV, generator=gen) / math.sqrt(kh * kw * cin / g)
    b = torch.randn(cout, device=DEV, generator=gen)
    frames = sample_frames(n)
    xs, dys, ms = (nhwc(host(interior(t, hl)[frames])) for t, hl in ((x, xh), (dy, dyh), (mask, xh)))
    wh, bh = host(wt), host(b)

    y = torch.empty((n, cout, h + 2 * yh, w + 2 * yh), device=DEV)
    z = O.grouped_conv(xs, wh, bh, 1, g)
    for relu in (False, True):
        got = on_and_off(hook, lambda: conv.fwd(x, wt, b, y, relu=relu), y, yh)
        close(nhwc(interior(got, yh)[frames]), np.maximum(z, 0) if relu else z, msg="fwd relu=%s" % relu)
    del y

    wtt = torch.empty(wt.numel(), device=DEV)
    conv.wt_transpose(wt, wtt)
    dx = torch.empty((n, cin, h + 2 * dxh, w + 2 * dxh), device=DEV)
    dxo, _, _ = O.grouped_conv_grad(xs, wh, dys, 1, g, need_dx=True)
    for m in (None, mask):
        got = on_and_off(hook, lambda: conv.dgrad(dy, wtt, dx, relu_mask=m), dx, dxh)
        close(nhwc(interior(got, dxh)[frames]), dxo if m is None else dxo * (ms > 0), msg="dgrad mask=%s" % (m is not None))
    del dx

    dw = torch.full(conv.w_shape, SENTINEL, device=DEV)
    db = torch.full((cout,), SENTINEL, device=DEV) if conv.fuses_bias() else None
    conv.wgrad(x, dy, dw, torch.empty(max(conv.wgrad_ws_bytes(n) // 4, 1), device=DEV), db=db)
    assert not bool((dw == SENTINEL).any())
    _, dwo, dbo = O.grouped_conv_grad(nhwc(host(interior(x, xh))), wh, nhwc(host(interior(dy, dyh))), 1, g, need_dx=False)
    close(host(dw), dwo, msg="wgrad over all %d frames" % n)
    if db is not None:
        close(host(db), dbo, msg="fused bias grad over all %d frames" % n)


# ---- the cases discriminate (CPU) --------------------------------------------------------------------------------------------------------
def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def conv_pads(x, wt, s, g, pads):
    """Grouped conv of NHWC x with HWIO wt under explicit paddings (top, bottom, left, right), torch fp64."""
    pt, pb, pl, pr = pads
    return F.conv2d(F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb)), wt.permute(3, 2, 0, 1), stride=s, groups=g).permute(0, 2, 3, 1)


def conv_all(x, wt, dy, s, g, pads):
    """y, dx, dw of conv_pads (no bias) by autograd."""
    xt, wtt = t64(x).requires_grad_(), t64(wt).requires_grad_()
    y = conv_pads(xt, wtt, s, g, pads)
    y.backward(t64(dy))
    return y.detach().numpy(), xt.grad.numpy(), wtt.grad.numpy()


def dgrad_as_conv(dy, wt, g, before):
    """Stride-1 dx as the kernels compute it: dy padded by `before` = (rows, columns) ahead and the rest of k-1 behind, convolved with
    the flipped kernel, channel roles swapped per group."""
    kh, kw, cig, cout = wt.shape
    cog = cout // g
    wf = t64(wt[::-1, ::-1])
    wd = torch.cat([wf[:, :, :, i * cog:(i + 1) * cog].permute(2, 3, 0, 1) for i in range(g)], 0)      # [cin][cog][kh][kw]
    dyp = F.pad(t64(dy).permute(0, 3, 1, 2), (before[1], kw - 1 - before[1], before[0], kh - 1 - before[0]))
    return F.conv2d(dyp, wd, groups=g).permute(0, 2, 3, 1).numpy()


DISCRIMINATING = sorted({c for c in FP32_CASES + RING_EXTRA + C8_CASES + [C8_STRIDED] + [(1, h, w, ci, co, kh, kw, 1, g) for h, w, ci, co, kh, kw, g in MANY]
                         if c[5] != c[6] or O.same_pad(c[1], c[5], c[7])[1] != O.same_pad(c[1], c[5], c[7])[2]
                         or O.same_pad(c[2], c[6], c[7])[1] != O.same_pad(c[2], c[6], c[7])[2]})


@pytest.mark.parametrize("case", DISCRIMINATING, ids=case_id)
def test_cases_discriminate(case):
    """Every asymmetric or non-square case of this file (the many-frames ones at one frame: frames are independent): each wrong
    oracle that is a different computation at that geometry differs from the right one by at least 100x the `close` tolerance, i.e.
    3e-3 of the largest element, in y, dx and dw.  The wrong oracles:
      - pads swapped (top <-> bottom, left <-> right): where the SAME padding is asymmetric;
      - kernel transposed (the HWIO buffer read with kh and kw exchanged) where kh != kw, the kernel flipped where it is square;
      - dgrad with the forward padding ahead of dy instead of k-1-pad: stride 1 with an asymmetric padding (k-1-pad == pad otherwise).
    A non-square kernel with odd sides has symmetric paddings: there the transposed kernel is the one wrong oracle that applies."""
    n, h, w, cin, cout, kh, kw, s, g = case
    rng = np.random.default_rng(h * 100 + cin)
    x, wt, _ = conv_inputs(rng, n, h, w, cin, cout, kh, kw, g)
    (oh, pt, pb), (ow, pl, pr) = O.same_pad(h, kh, s), O.same_pad(w, kw, s)
    dy = rng.standard_normal((n, oh, ow, cout)).astype(np.float32)
    right = conv_all(x, wt, dy, s, g, (pt, pb, pl, pr))
    dxo, dwo, _ = O.grouped_conv_grad(x, wt, dy, s, g)
    for got, want in zip(right, (O.grouped_conv(x, wt, np.zeros(cout), s, g), dxo, dwo)):       # the restatement IS the oracle
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-9)

    def far(wrong, what):
        for name, a, b in zip(("y", "dx", "dw"), wrong, right):
            if a is not None:
                diff, bound = float(np.abs(a - b).max()), 100 * 3e-5 * float(np.abs(b).max())
                assert diff >= bound, "%s: %s within %.2e of the right oracle (bound %.2e)" % (what, name, diff, bound)

    applied = 0
    if pt != pb or pl != pr:
        far(conv_all(x, wt, dy, s, g, (pb, pt, pr, pl)), "pads swapped")
        applied += 1
    if kh != kw:
        # the same buffer read as [kw][kh][ci][co]: a kw x kh kernel with its own SAME paddings
        wsw = wt.reshape(kw, kh, cin // g, cout)
        ys, dxs, dws = conv_all(x, wsw, dy, s, g, O.same_pad(h, kw, s)[1:] + O.same_pad(w, kh, s)[1:])
        far((ys, dxs, dws.reshape(wt.shape)), "kh and kw exchanged")
    else:
        yf, dxf, dwf = conv_all(x, wt[::-1, ::-1], dy, s, g, (pt, pb, pl, pr))
        far((yf, dxf, dwf[::-1, ::-1]) if kh > 1 else (None, None, None), "kernel flipped")
    applied += 1 if (kh != kw or kh > 1) else 0
    if s == 1:
        np.testing.assert_allclose(dgrad_as_conv(dy, wt, g, (kh - 1 - pt, kw - 1 - pl)), dxo, rtol=1e-9, atol=1e-9)
        if (pt, pl) != (kh - 1 - pt, kw - 1 - pl):
            far((None, dgrad_as_conv(dy, wt, g, (pt, pl)), None), "dgrad with the forward padding")
            applied += 1
    assert applied > 0
