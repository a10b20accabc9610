"""Stage depth of the 16x16-MFMA LDS-DMA conv kernel (conv_dma16_kernel<TA, SR, OCC>; vl_conv_set_stage_depth, include/vltf.h): 16-row
stages with three workgroups per CU against 32-row stages with two.  The depth moves barriers, never the order in which products enter
an accumulator, so every case compares forced depth 16 with forced depth 32 BIT FOR BIT (torch.equal on the whole output buffer, halo
included, both pre-filled with a sentinel), holds the depth-16 result to the fp64 oracle at test_ops_gpu's `close` (3e-5), and asserts
through vl_conv_last_launch that the launch really ran the kernel under test at the tile height the case is about.

How a case reaches a tile height (dispatch_conv):
  few frames  the width with the smallest ceil(workgroups / CUs) * rows, ties to the wider: three frames always run 48-row tiles
              (TA = 3: 48 channels, and 40 for the `co < Cog` guards), and a frame count from `frames_for`, derived from the device's
              CU count through `few_plan` (the dispatcher's rule restated), runs 96-row tiles (TA = 6: 96, 192 = two channel tiles,
              100 = a second tile of 4 channels); a larger count splits the last round off as a second, 48-row launch;
  many frames 96-row tiles for 96 / 192 channels per group, 48-row tiles for 48 / 144; frame count from the CU count as in
              test_conv_geometry_gpu.many_frames.

Reduction lengths K = 9, 16, 18, 32, 33, 48, 144 and conv1's 363 (11x11x3 at stride 4, phase-split x): one, two, three and more
16-row stages, odd and even counts, a prefetch of a stage that does not exist, last stages of 1..4 live k4-steps, and for depth 32
the half-filled last stage.  The CPU test at the end holds the LDS arithmetic of both forms."""
import math
import os
import re

import numpy as np
import pytest
import torch

from oracle import lrcn_oracle as O

DEV = "cuda:0"
SENTINEL = 12345.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (128, 96, 48)


def cdiv(a, b):
    return -(-a // b)


# ---- dispatch_conv's few-frames rule, restated -----------------------------------------------------------------------------------------
def few_plan(n, ohw, cog, g, cus):
    """None when the launch is not `few`; else the tile heights of its launches: (height,) or (first, second) for a tail split."""
    px = cdiv(n * ohw, 128)
    if px * cdiv(cog, 128) * g >= 8 * cus:
        return None

    def pick(pxt):
        best, load = 0, None
        for i, wd in enumerate(WIDTHS):
            l = cdiv(pxt * cdiv(cog, wd) * g, cus) * wd
            if load is None or l < load:
                best, load = i, l
        return best, load
    best, best_load = pick(px)
    wpp = cdiv(cog, WIDTHS[best]) * g
    rounds = px * wpp // cus
    if rounds >= 6:
        n_a = (rounds * cus // wpp) * 128 // ohw
        n_b = n - n_a
        if n_a > 0 and n_b > 0:
            wb, load_b = pick(cdiv(n_b * ohw, 128))
            load_a = cdiv(cdiv(n_a * ohw, 128) * wpp, cus) * WIDTHS[best]
            if (load_a + max(load_b, 64) + 16) * 100 <= best_load * 95:
                return WIDTHS[best], WIDTHS[wb]
    return (WIDTHS[best],)


def frames_for(ohw, cog, g, cus, want, split=False):
    """Smallest frame count >= 2 whose few-frames plan is one launch of `want`-row tiles (split: a tail split that ends in one)."""
    for n in range(2, 2000):
        plan = few_plan(n, ohw, cog, g, cus)
        if plan is None:
            break
        if len(plan) == (2 if split else 1) and plan[-1] == want:
            return n
    raise AssertionError("no frame count gives %d-row tiles for %d channels x %d groups on %d CUs" % (want, cog, g, cus))


def many_frames(ohw, cog, g, cus):
    """test_conv_geometry_gpu.many_frames: `few` is false with 10 % to spare."""
    px = cdiv(int(1.1 * 8 * cus * 1000), 1000 * cdiv(cog, 128) * g)
    return cdiv(px * 128, ohw)


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    import vltf_amd.ops as ops_
    return ops_


@pytest.fixture
def hooks(ops):
    yield ops
    ops.conv_set_stage_depth(0)
    ops.conv_set_row_classes(True)


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def close(got, want, msg=""):     # test_ops_gpu.close
    want = np.asarray(want, np.float64)
    scale = float(np.abs(want).max()) or 1.0
    np.testing.assert_allclose(np.asarray(got, np.float64), want, rtol=3e-5, atol=3e-5 * scale, err_msg=msg)


def interior(t, halo):
    return t if halo == 0 else t[:, :, halo:-halo, halo:-halo]


def nhwc(t):
    return np.ascontiguousarray(t.detach().cpu().numpy().transpose(0, 2, 3, 1))


def haloed(gen, n, c, h, w, halo):
    t = torch.zeros((n, c, h + 2 * halo, w + 2 * halo), device=DEV)
    interior(t, halo).copy_(torch.randn((n, c, h, w), device=DEV, generator=gen))
    return t


def phase_split(xp, ph):
    """Padded NCHW -> the column-phase-split layout of vl_conv_set_x_phase_split (test_conv_geometry_gpu.phase_split, on the device)."""
    n, c, hp, wp = xp.shape
    wq = cdiv(wp, ph)
    xp = torch.nn.functional.pad(xp, (0, wq * ph - wp))
    return xp.reshape(n, c, hp, wq, ph).permute(0, 1, 4, 2, 3).reshape(n, c * ph, hp, wq).contiguous()


def both_depths(ops, launch, shape, halo, tile, what):
    """launch(out) at forced depth 32, at 16 and at 16 again, each into a fresh sentinel-filled buffer: the form that ran is the 16x16
    kernel at `tile` rows and that depth, interior written and halo untouched, all three equal bit for bit.  Returns the depth-16 result."""
    res = []
    for depth in (32, 16, 16):
        ops.conv_set_stage_depth(depth)
        out = torch.full(shape, SENTINEL, device=DEV)
        launch(out)
        assert ops.conv_last_launch() == tile * 100 + depth, "%s: ran form %d, not %d-row tiles at depth %d" % (
            what, ops.conv_last_launch(), tile, depth)
        assert not bool((interior(out, halo) == SENTINEL).any()), "%s depth %d: interior not fully written" % (what, depth)
        if halo:
            frame = out.clone()
            interior(frame, halo).fill_(SENTINEL)
            assert bool((frame == SENTINEL).all()), "%s depth %d: halo touched" % (what, depth)
        res.append(out)
    ops.conv_set_stage_depth(0)
    assert torch.equal(res[1], res[0]), "%s: depth 16 != depth 32" % what
    assert torch.equal(res[2], res[1]), "%s: depth 16 twice differs" % what
    return res[1]


def sample(n):
    return sorted({0, n // 2, n - 1})


def make_layer(ops, gen, n, h, w, cin, cout, kh, kw, s, g, y_halo, dx_halo=0):
    conv = ops.Conv(cin, h, w, cout, kh, kw, s, g)
    xh, dyh = conv.same_pad(), max(kh, kw) - 1
    conv.set_halo(xh, y_halo, dyh if s == 1 else 0, dx_halo)
    x = haloed(gen, n, cin, h, w, xh)
    wt = torch.randn((kh, kw, cin // g, cout), device=DEV, generator=gen) / math.sqrt(kh * kw * cin / g)
    b = torch.randn(cout, device=DEV, generator=gen)
    return conv, x, wt, b, xh, dyh


def run_forward(ops, n, h, w, cin, cout, kh, kw, s, g, tile, phase=False):
    """Forward of one layer at n frames: dense y (the wide 16-byte store path: 13x13 and 9x9 planes are odd, so 4-pixel runs straddle
    frames, and n * OH * OW is no multiple of 128) with bias and ReLU, and haloed y (per-accumulator stores) without either."""
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1000 * kh + 10 * cin + cout)
    conv, x, wt, b, xh, _ = make_layer(ops, gen, n, h, w, cin, cout, kh, kw, s, g, 0)
    oh, ow = conv.oh, conv.ow
    assert (n * oh * ow) % 128 != 0 and (oh * ow) % 4 != 0
    xs = nhwc(interior(x, xh)[sample(n)])
    xd = x
    if phase:
        assert conv.set_x_phase_split(True) == s
        xd = phase_split(x, s)
        assert tuple(xd.shape) == conv.x_shape(n)
    z = O.grouped_conv(xs, wt.cpu().numpy(), b.cpu().numpy(), s, g)
    got = both_depths(ops, lambda y: conv.fwd(xd, wt, b, y, relu=True), (n, cout, oh, ow), 0, tile, "fwd dense")
    close(nhwc(got[sample(n)]), np.maximum(z, 0), "fwd dense + bias + relu")
    conv.set_halo(xh, 1, conv.dy_halo, 0)
    got = both_depths(ops, lambda y: conv.fwd(xd, wt, None, y, relu=False), (n, cout, oh + 2, ow + 2), 1, tile, "fwd haloed")
    close(nhwc(interior(got, 1)[sample(n)]), z - b.cpu().numpy(), "fwd haloed, no bias, no relu")


def run_dgrad(ops, n, h, w, cin, cout, kh, kw, g, tile):
    """Input gradient (the kernel with cin / g output channels and K = kh kw cout / g): haloed dx with and without the ReluGrad mask."""
    gen = torch.Generator(device=DEV)
    gen.manual_seed(2000 * kh + 10 * cin + cout)
    dxh = 2
    conv, x, wt, _, xh, dyh = make_layer(ops, gen, n, h, w, cin, cout, kh, kw, 1, g, 0, dxh)
    dy = haloed(gen, n, cout, h, w, dyh)
    mask = haloed(gen, n, cin, h, w, xh)
    wtt = torch.empty(wt.numel(), device=DEV)
    conv.wt_transpose(wt, wtt)
    fr = sample(n)
    dxo, _, _ = O.grouped_conv_grad(nhwc(interior(x, xh)[fr]), wt.cpu().numpy(), nhwc(interior(dy, dyh)[fr]), 1, g, need_dx=True)
    shape = (n, cin, h + 2 * dxh, w + 2 * dxh)
    got = both_depths(ops, lambda dx: conv.dgrad(dy, wtt, dx), shape, dxh, tile, "dgrad")
    close(nhwc(interior(got, dxh)[fr]), dxo, "dgrad")
    got = both_depths(ops, lambda dx: conv.dgrad(dy, wtt, dx, relu_mask=mask), shape, dxh, tile, "dgrad + mask")
    close(nhwc(interior(got, dxh)[fr]), dxo * (nhwc(interior(mask, xh)[fr]) > 0), "dgrad + mask")


# ---- reduction length x tile height, few frames ----------------------------------------------------------------------------------------
# K: (h, w, channels per group of the reduction, kh, kw)
K_GEOM = {9: (13, 13, 1, 3, 3), 16: (13, 11, 1, 4, 4), 18: (13, 13, 2, 3, 3), 32: (13, 11, 2, 4, 4), 33: (13, 13, 1, 3, 11),
          48: (13, 11, 3, 4, 4), 144: (13, 13, 16, 3, 3)}
# output channels per group -> tile height of the launch: 48 / 40 at three frames, 96 / 192 / 100 at frames_for(...)
HEIGHTS = {48: 48, 40: 48, 96: 96, 192: 96, 100: 96}


@pytest.mark.gpu
@pytest.mark.parametrize("cog", sorted(HEIGHTS))
@pytest.mark.parametrize("k", sorted(K_GEOM))
def test_forward_reduction_lengths(hooks, cus, k, cog):
    h, w, cig, kh, kw = K_GEOM[k]
    assert kh * kw * cig == k
    g, tile = 2, HEIGHTS[cog]
    n = 3 if tile == 48 else frames_for(h * w, cog, g, cus, 96)
    assert few_plan(n, h * w, cog, g, cus) == (tile,)
    run_forward(hooks, n, h, w, cig * g, cog * g, kh, kw, 1, g, tile)


@pytest.mark.gpu
@pytest.mark.parametrize("cout", [96, 48])
def test_forward_conv1_tail(hooks, cus, cout):
    """K = 363 = 22 blocks + 11 rows: 11x11x3 at stride 4 on a 35x35 image (9x9 outputs), x column-phase-split as the engine stores it."""
    tile = 96 if cout == 96 else 48
    n = 3 if tile == 48 else frames_for(81, cout, 1, cus, 96)
    assert few_plan(n, 81, cout, 1, cus) == (tile,)
    run_forward(hooks, n, 35, 35, 3, cout, 11, 11, 4, 1, tile, phase=True)


@pytest.mark.gpu
@pytest.mark.parametrize("cig", sorted(HEIGHTS))
@pytest.mark.parametrize("cog", [1, 2, 16])
def test_dgrad_mask(hooks, cus, cog, cig):
    """3x3 dgrad: K = 9, 18 and 144 at every tile height, haloed output, with and without the fused ReluGrad mask."""
    g, tile = 2, HEIGHTS[cig]
    n = 3 if tile == 48 else frames_for(169, cig, g, cus, 96)
    assert few_plan(n, 169, cig, g, cus) == (tile,)
    run_dgrad(hooks, n, 13, 13, cig * g, cog * g, 3, 3, g, tile)


@pytest.mark.gpu
def test_few_frames_tail_split(hooks, cus):
    """A frame count below the many-frames threshold whose last, mostly empty round is split off as a second launch (flat pixel order;
    100 channels x 2 groups on 13x13: 128-row tiles, then the last frames as 48-row tiles of the kernel under test, three channel tiles
    of which the last holds 4 channels).  vl_conv_last_launch reports the second launch."""
    n = frames_for(169, 100, 2, cus, 48, split=True)
    plan = few_plan(n, 169, 100, 2, cus)
    print("tail split: %d frames, tile heights %s" % (n, plan))
    hooks.conv_set_row_classes(False)
    run_forward(hooks, n, 13, 13, 32, 200, 3, 3, 1, 2, 48)


# ---- many frames: row classes on and off -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("classes", [True, False], ids=["classes", "flat"])
@pytest.mark.parametrize("cog,tile", [(192, 96), (144, 48)])
def test_many_frames_forward(hooks, cus, cog, tile, classes):
    n = many_frames(169, cog, 2, cus)
    assert few_plan(n, 169, cog, 2, cus) is None
    hooks.conv_set_row_classes(classes)
    run_forward(hooks, n, 13, 13, 32, 2 * cog, 3, 3, 1, 2, tile)


@pytest.mark.gpu
@pytest.mark.parametrize("classes", [True, False], ids=["classes", "flat"])
def test_many_frames_dgrad(hooks, cus, classes):
    n = many_frames(169, 192, 2, cus)
    assert few_plan(n, 169, 192, 2, cus) is None
    hooks.conv_set_row_classes(classes)
    run_dgrad(hooks, n, 13, 13, 384, 32, 3, 3, 2, 96)


# ---- the LDS arithmetic of both forms (CPU) -------------------------------------------------------------------------------------------------
CU_LDS = 163840


def lds_bytes(bm, sr):
    """conv16_lds_bytes: two stage buffers of sr rows x (weight row of roundup(bm, 64) + 16 floats | 128 + 16 pixels), or the [bm][132]
    staging tile of the wide-store epilogue, whichever is larger."""
    stage = 2 * sr * (cdiv(bm, 64) * 64 + 16 + 144) * 4
    staging = bm * (128 + 4) * 4
    return stage, staging, max(stage, staging)


def test_lds_arithmetic_keeps_three_workgroups_resident():
    assert lds_bytes(96, 32) == (73728, 50688, 73728) and lds_bytes(96, 16) == (36864, 50688, 50688)
    assert lds_bytes(48, 32) == (57344, 25344, 57344) and lds_bytes(48, 16) == (28672, 25344, 28672)
    assert CU_LDS // lds_bytes(96, 32)[2] == 2 and CU_LDS // lds_bytes(48, 32)[2] == 2
    assert CU_LDS // lds_bytes(96, 16)[2] == 3 and CU_LDS // lds_bytes(48, 16)[2] >= 3
    # the table beside the launcher (csrc/mfma_gemm.hip, above conv16_stage_bytes) says the same, row for row ...
    src = open(os.path.join(ROOT, "video-learning-tf_amd", "csrc", "mfma_gemm.hip")).read()
    rows = re.findall(r"^//\s+(48|96)\s+(16|32)\s+([\d,]+)\s+([\d,]+)\s+([\d,]+)\s+(\d)", src, flags=re.M)
    assert len(rows) == 4, rows
    for bm, sr, stage, staging, alloc, fit in rows:
        want = lds_bytes(int(bm), int(sr))
        assert tuple(int(v.replace(",", "")) for v in (stage, staging, alloc)) == want, (bm, sr)
        assert int(fit) == CU_LDS // want[2], (bm, sr)
    # ... and the launcher computes its allocation by these formulas and asserts the residency at compile time
    assert "(size_t)2 * SR * ((BM + 63) / 64 * 64 + 16 + 144) * sizeof(float)" in src
    assert "(size_t)BM * (128 + 4) * sizeof(float)" in src
    assert "3 * conv16_lds_bytes(96, 16) <= 163840 && 3 * conv16_lds_bytes(48, 16) <= 163840" in src
    # the kernel's row strides: SA = roundup(BM, 64) + 16 and SB = 144 are both 16 mod 32 (conflict-free fragment reads)
    for bm in (48, 96):
        assert (cdiv(bm, 64) * 64 + 16) % 32 == 16 and 144 % 32 == 16
