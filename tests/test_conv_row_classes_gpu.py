"""Row-class pixel order of the fp32 conv forward / input-gradient launches (vl_conv_set_row_classes, include/vltf.h): a launch with
many frames enumerates its output pixels by row class and leaves out the kernel rows that read nothing but the SAME-padding halo.
The terms left out are w * (+0) added to a sum that starts at +0, and the order of the other terms is unchanged, so the results must
be those of the flat order (hook off) BIT FOR BIT; the hook-on results are also held to the oracle at test_ops_gpu's `close` tolerance.

Frame counts 3 .. 130 stay below dispatch_conv's many-frames threshold on a 256-CU device (both runs are then the flat order: the hook
must change nothing there either); 600 and 1024 run the class order, 600 with partial last tiles in every class segment (1024 frames
fill every segment exactly).  The oracle is the CPU one, so at more than a few frames it checks the first, the middle and the last
frame: an output frame does not depend on the batch it is computed in."""
import math

import numpy as np
import pytest
import torch

from oracle import lrcn_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 12345.0

LAYERS = {  # h, w, cin, cout, k, groups
    "conv3": (13, 13, 256, 384, 3, 1),      # 256 -> 384 channels per group
    "conv4": (13, 13, 384, 384, 3, 2),      # 192 -> 192
    "conv5": (13, 13, 384, 256, 3, 2),      # 192 -> 128
    "conv2": (28, 28, 96, 256, 5, 2),       # 48 -> 128, five row classes
}
FRAMES = [3, 37, 128, 130, 600, 1024]


@pytest.fixture(scope="module")
def ops():
    import vltf_amd.ops as ops_
    return ops_


@pytest.fixture
def hook(ops):
    yield ops.conv_set_row_classes
    ops.conv_set_row_classes(True)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def nhwc(a):
    return np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))


def close(got, want, rtol=3e-5, atol_rel=3e-5, msg=""):     # test_ops_gpu.close
    want = np.asarray(want, np.float64)
    scale = float(np.abs(want).max()) or 1.0
    np.testing.assert_allclose(np.asarray(got, np.float64), want, rtol=rtol, atol=atol_rel * scale, err_msg=msg)


def interior(t, halo):
    return t if halo == 0 else t[:, :, halo:-halo, halo:-halo]


def haloed(gen, n, c, h, w, halo):
    t = torch.zeros((n, c, h + 2 * halo, w + 2 * halo), device=DEV)
    interior(t, halo).copy_(torch.randn((n, c, h, w), device=DEV, generator=gen))
    return t


def on_and_off(hook, run, out, halo):
    """run() with the hook off and on into the sentinel-filled `out`: both results on the host, after checking that the "on" run wrote
    every interior element and that the two are equal bit for bit (the halo, which neither may touch, included)."""
    res = []
    for on in (False, True):
        hook(on)
        out.fill_(SENTINEL)
        run()
        assert not bool((interior(out, halo) == SENTINEL).any()), "interior not fully written (hook %s)" % on
        res.append(host(out))
    assert np.array_equal(res[1], res[0])
    if halo:
        assert np.all(res[1][:, :, 0, :] == SENTINEL) and np.all(res[1][:, :, :, -1] == SENTINEL)
    return res[1]


def sample_frames(n):
    return sorted({0, n // 2, n - 1})


@pytest.mark.parametrize("out_halo", [0, 1])
@pytest.mark.parametrize("n", FRAMES)
@pytest.mark.parametrize("layer", list(LAYERS))
def test_forward_is_bitwise_the_flat_order(ops, hook, layer, n, out_halo):
    h, w, cin, cout, k, g = LAYERS[layer]
    gen = torch.Generator(device=DEV)
    gen.manual_seed(n * 7 + h)
    conv = ops.Conv(cin, h, w, cout, k, k, 1, g)
    xh = conv.same_pad()
    conv.set_halo(xh, out_halo, xh, out_halo)
    x = haloed(gen, n, cin, h, w, xh)
    wt = torch.randn((k, k, cin // g, cout), device=DEV, generator=gen) / math.sqrt(k * k * cin / g)
    b = torch.randn(cout, device=DEV, generator=gen)
    y = torch.empty((n, cout, h + 2 * out_halo, w + 2 * out_halo), device=DEV)
    frames = sample_frames(n)
    xs, ws, bs = nhwc(host(interior(x, xh)[frames])), host(wt), host(b)
    for bias, relu in ((None, False), (b, False), (b, True)):
        got = on_and_off(hook, lambda: conv.fwd(x, wt, bias, y, relu=relu), y, out_halo)
        z = O.grouped_conv(xs, ws, bs if bias is not None else np.zeros_like(bs), 1, g)
        if relu:
            z = np.maximum(z, 0)
        close(nhwc(interior(got, out_halo)[frames]), z, msg="%s fwd n=%d bias=%s relu=%s" % (layer, n, bias is not None, relu))


@pytest.mark.parametrize("out_halo", [0, 2])
@pytest.mark.parametrize("n", FRAMES)
@pytest.mark.parametrize("layer", list(LAYERS))
def test_dgrad_is_bitwise_the_flat_order(ops, hook, layer, n, out_halo):
    h, w, cin, cout, k, g = LAYERS[layer]
    gen = torch.Generator(device=DEV)
    gen.manual_seed(n * 11 + h)
    conv = ops.Conv(cin, h, w, cout, k, k, 1, g)
    xh = conv.same_pad()
    conv.set_halo(xh, 0, xh, out_halo)
    dy = haloed(gen, n, cout, h, w, xh)
    mask = haloed(gen, n, cin, h, w, xh)
    wt = torch.randn((k, k, cin // g, cout), device=DEV, generator=gen) / math.sqrt(k * k * cin / g)
    wtt = torch.empty(wt.numel(), device=DEV)
    conv.wt_transpose(wt, wtt)
    dx = torch.empty((n, cin, h + 2 * out_halo, w + 2 * out_halo), device=DEV)
    frames = sample_frames(n)
    dys, ms, ws = nhwc(host(interior(dy, xh)[frames])), nhwc(host(interior(mask, xh)[frames])), host(wt)
    dxo, _, _ = O.grouped_conv_grad(np.zeros((len(frames), h, w, cin), np.float32), ws, dys, 1, g, need_dx=True)
    for m in (None, mask):
        got = on_and_off(hook, lambda: conv.dgrad(dy, wtt, dx, relu_mask=m), dx, out_halo)
        want = dxo if m is None else dxo * (ms > 0)
        close(nhwc(interior(got, out_halo)[frames]), want, msg="%s dgrad n=%d mask=%s" % (layer, n, m is not None))
