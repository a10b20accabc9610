"""Conv weight gradient across frame counts: vl_conv_wgrad (csrc/mfma_gemm.hip) in fp32, split-bf16 and in-loop bf16 arithmetic, and the
packed vl_conv_c8_wgrad (csrc/conv_c8.hip), against a float64 weight / bias gradient over the WHOLE batch (the gradient sums over
frames, so a sampled reference would not do).  test_ops_gpu holds these kernels to the oracle at 1-3 frames, where a split of
wgrad_dma_kernel's pixel range is one or two 64-pixel tiles long; the frame counts here are the smallest at which the launch changes
character on a 256-CU device: splits that get no tile, odd and even tile counts per split (the tile loop is unrolled by two over
two LDS buffers), 32 and more tiles per split, other split counts, a last tile that ends inside the batch -- and, for the packed
kernel, many slabs that start in the middle of an image.  test_the_frame_counts_cover_the_launch_shapes derives the split count from
the public workspace query and fails, naming the clause, when a change of the heuristic leaves one of these shapes uncovered.

The reference is torch's CPU convolution backward in double on explicitly padded input (cross-checked against the numpy oracle, which
pins the asymmetric SAME padding).  It is computed once per (layer, frame count) and shared by every arithmetic mode.  The tolerance is
test_ops_gpu's `close`, unchanged: an fp32 CPU gradient stays below 0.15 of that bound against float64 at every size here, the kernels
below 0.17 (profiles/conv_wgrad_frames.txt has both, per case), while dropping the batch's last 64-pixel tile (float64, on the CPU) puts 99 % of dw's
elements outside it, by a factor of 500 and more, at the largest frame counts used here.

Every call runs with dw, db and the workspace filled with NaN (the workspace is otherwise torch.empty: a slab that is read but never
written may happen to hold zeros) and with a sentinel pattern behind the size the workspace query declares.  Each check prints its
worst |got - want| / bound as a `WGF` line before it asserts (pytest -s shows them)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import lrcn_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = ["f32", "bf16x3", "bf16x6"]

LAYERS = {  # h, w, cin, cout, k, stride, groups
    "conv1": (227, 227, 3, 96, 11, 4, 1),
    "conv2": (28, 28, 96, 256, 5, 1, 2),
    "conv3": (13, 13, 256, 384, 3, 1, 1),
    "conv4": (13, 13, 384, 384, 3, 1, 2),
    "conv5": (13, 13, 384, 256, 3, 1, 2),
    # ragged layers, 10 x 7 planes
    "k639": (10, 7, 71, 64, 3, 1, 1),        # K = 639, K % 128 == 127: the fused bias row is the last row of the last tile
    "k513": (10, 7, 114, 256, 3, 1, 2),      # 57 channels per group: K = 513, K % 128 == 1
    "co129": (10, 7, 40, 129, 3, 1, 1),      # 96-wide tiles, the second with 33 live channels
    "co40": (10, 7, 48, 80, 3, 1, 2),        # 40 output channels per group
}
STACK = ["conv2", "conv3", "conv4", "conv5"]
RAGGED = ["k639", "k513", "co129", "co40"]
FRAMES = [5, 16, 37, 130, 257]
CONV1_FRAMES = [1, 5, 16, 37]
RAGGED_FRAMES = [5, 37]
C8_FRAMES = [16, 37, 130, 257]

# layouts: "k-1" = x with the SAME halo, dy with a halo of k - 1 (test_ops_gpu's padded layout); "same" = dy with the SAME halo (what
# the engine allocates); "plain" / "phase" = conv1 as the engine runs it (dy dense), x plain or column-phase-split; "dense" = no halo
# anywhere: the bounds-checked launch_wgrad (32-pixel tiles, its own split rule)
CASES = [(l, n, "k-1") for l in STACK for n in FRAMES] + [(l, 130, "same") for l in STACK] + \
        [("conv1", n, lay) for n in CONV1_FRAMES for lay in ("plain", "phase")] + \
        [(l, n, "k-1") for l in RAGGED for n in RAGGED_FRAMES] + \
        [(l, 37, "dense") for l in ["conv1"] + STACK]
BF16_CASES = [(l, n, "k-1") for l in STACK for n in (37, 130)] + [("conv1", 37, "plain"), ("conv1", 37, "phase")] + \
             [(l, 37, "k-1") for l in RAGGED]


@pytest.fixture(scope="module")
def ops():
    import vltf_amd.ops as ops_
    return ops_


@pytest.fixture
def conv_math(ops):
    yield ops.set_conv_math
    ops.set_conv_math("f32")


def close(got, want, rtol=3e-5, atol_rel=3e-5, msg=""):     # test_ops_gpu.close
    want = np.asarray(want, np.float64)
    scale = float(np.abs(want).max()) or 1.0
    np.testing.assert_allclose(np.asarray(got, np.float64), want, rtol=rtol, atol=atol_rel * scale, err_msg=msg)


def bound_ratio(got, want, rtol=3e-5, atol_rel=3e-5):
    """Worst |got - want| / (close's bound), for the record: the assertion is close()."""
    want = np.asarray(want, np.float64)
    scale = float(np.abs(want).max()) or 1.0
    return float(np.max(np.abs(np.asarray(got, np.float64) - want) / (atol_rel * scale + rtol * np.abs(want))))


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def haloed(t, halo):
    """The dense [n, c, h, w] tensor as the interior of a zero halo."""
    return t.contiguous() if halo == 0 else F.pad(t, (halo, halo, halo, halo)).contiguous()


def phase_split(xp, ph):
    """Padded NCHW -> the column-phase-split layout of vl_conv_set_x_phase_split: [n, c * ph, hp, ceil(wp / ph)]."""
    n, c, hp, wp = xp.shape
    wq = -(-wp // ph)
    xp = F.pad(xp, (0, wq * ph - wp))
    return xp.reshape(n, c, hp, wq, ph).permute(0, 1, 4, 2, 3).reshape(n, c * ph, hp, wq).contiguous()


def to_c8(t):
    """NCHW fp32 (any halo already in place, values bf16-representable) -> bf16 [n][c / 8][hp][wp][8]."""
    n, c, hp, wp = t.shape
    return t.reshape(n, c // 8, 8, hp, wp).permute(0, 1, 3, 4, 2).contiguous().bfloat16()


def reference_grads(x, dy, k, s, g):
    """float64 dw (HWIO) and db of the SAME convolution from host NCHW float32 tensors: torch's CPU backward on explicitly padded x."""
    n, cin, h, w = x.shape
    cout = dy.shape[1]
    _, pt, pb = O.same_pad(h, k, s)
    _, pl, pr = O.same_pad(w, k, s)
    xp = F.pad(x.double(), (pl, pr, pt, pb))
    dyd = dy.double()
    dw = torch.nn.grad.conv2d_weight(xp, (cout, cin // g, k, k), dyd, stride=s, padding=0, groups=g)      # OIHW
    return dw.permute(2, 3, 1, 0).contiguous().numpy(), dyd.sum(dim=(0, 2, 3)).numpy()


@functools.lru_cache(maxsize=2)
def case_data(layer, n, packed=False):
    """Seeded device inputs of one (layer, frame count) and their float64 reference; packed: bf16-representable values, x post-ReLU-like."""
    h, w, cin, cout, k, s, g = LAYERS[layer]
    oh, ow = -(-h // s), -(-w // s)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(n * 13 + h + cin + (1000 if packed else 0))
    x = torch.randn((n, cin, h, w), device=DEV, generator=gen)
    dy = torch.randn((n, cout, oh, ow), device=DEV, generator=gen)
    if packed:
        x, dy = x.clamp_(min=0).bfloat16().float(), dy.bfloat16().float()
    torch.cuda.synchronize()
    dw, db = reference_grads(x.cpu(), dy.cpu(), k, s, g)
    return x, dy, dw, db


def nan_ws(nbytes, slack=0, extra=1024):
    """Workspace of nbytes (rounded up to floats) + `slack` floats, all NaN, with `extra` sentinel floats behind: (tensor, floats, sentinel)."""
    nf = max((nbytes + 3) // 4, 1)
    ws = torch.full((nf + slack + extra,), float("nan"), device=DEV)
    sentinel = torch.arange(extra, device=DEV, dtype=torch.float32) * 0.5 + 12345.0
    ws[nf + slack:] = sentinel
    return ws, nf, sentinel


def ws_untouched_behind(ws, nf, sentinel):
    """Nothing written behind the first nf floats: the slack still NaN, the sentinel intact."""
    tail = ws[nf:]
    slack = tail.numel() - sentinel.numel()
    return bool(torch.isnan(tail[:slack]).all()) and torch.equal(tail[slack:], sentinel)


def split_shape(conv, n, K, cout, tile=64):
    """(splits, tiles per split, empty splits) from the public workspace query."""
    splits = max(conv.wgrad_ws_bytes(n) // ((K + 1) * cout * 4), 1)
    rtiles = -(-n * conv.oh * conv.ow // tile)
    per = -(-rtiles // splits)
    return splits, per, (splits * per - rtiles) // per


def make_layer(ops, layer, n, layout):
    """Descriptor in `layout` and the device operands (x, dy) laid out for it."""
    h, w, cin, cout, k, s, g = LAYERS[layer]
    x, dy, dwo, dbo = case_data(layer, n)
    conv = ops.Conv(cin, h, w, cout, k, k, s, g)
    pad = conv.same_pad()
    xh, dyh = {"k-1": (pad, k - 1), "same": (pad, pad), "plain": (pad, 0), "phase": (pad, 0), "dense": (0, 0)}[layout]
    conv.set_halo(xh, 0, dyh, 0)
    xd = haloed(x, xh)
    if layout == "phase":
        ph = conv.set_x_phase_split(True)
        assert ph == s
        xd = phase_split(xd, ph)
    assert tuple(xd.shape) == conv.x_shape(n)
    return conv, xd, haloed(dy, dyh), dwo, dbo


def run_wgrad(conv, xd, dyd, n, with_db, exact_ws):
    """One vl_conv_wgrad call into NaN-filled dw / db / workspace; the sentinel behind the declared workspace size must survive.
    exact_ws: hand over exactly wgrad_ws_bytes(n); otherwise a larger workspace, whose surplus must stay as it was."""
    need = conv.wgrad_ws_bytes(n)
    slack = 0 if exact_ws else 4096
    ws, nf, sentinel = nan_ws(need, slack)
    dw = torch.full(conv.w_shape, float("nan"), device=DEV)
    db = torch.full((conv.cout,), 7.0, device=DEV) if with_db else None
    conv.wgrad(xd, dyd, dw, ws[:nf + slack], db=db)
    torch.cuda.synchronize()
    assert ws_untouched_behind(ws, nf, sentinel), "vl_conv_wgrad wrote behind the workspace it asked for"
    assert not bool(torch.isnan(dw).any()), "NaN left in dw: an element not written, or a workspace slab read but not written"
    return dw, db


@pytest.mark.parametrize("layer,n,layout,mode", [c + (m,) for c in CASES for m in MODES])
def test_wgrad_against_the_full_batch_reference(ops, conv_math, layer, n, layout, mode):
    h, w, cin, cout, k, s, g = LAYERS[layer]
    conv, xd, dyd, dwo, dbo = make_layer(ops, layer, n, layout)
    K = k * k * (cin // g)
    splits, per, empty = split_shape(conv, n, K, cout, 32 if layout == "dense" else 64)
    tag = "WGF %s n=%d %s %s splits=%d per=%d empty=%d" % (layer, n, layout, mode, splits, per, empty)
    conv_math(mode)
    dw, _ = run_wgrad(conv, xd, dyd, n, False, exact_ws=True)
    print("%s dw=%.4f" % (tag, bound_ratio(host(dw), dwo)))
    close(host(dw), dwo, msg=tag + " dw")
    # run to run: bit for bit (README), the second time inside a larger workspace
    dw2, _ = run_wgrad(conv, xd, dyd, n, False, exact_ws=False)
    assert torch.equal(dw, dw2), tag + ": a second identical call gave other bits"

    fused = layout != "dense" and K % 128 != 0
    assert conv.fuses_bias() == fused
    if fused:
        dw3, db = run_wgrad(conv, xd, dyd, n, True, exact_ws=True)
        assert torch.equal(dw3, dw), tag + ": dw changes with the fused bias gradient"
        print("%s db_fused=%.4f" % (tag, bound_ratio(host(db), dbo)))
        close(host(db), dbo, msg=tag + " fused db")
        dw4, db2 = run_wgrad(conv, xd, dyd, n, True, exact_ws=False)
        assert torch.equal(dw4, dw) and torch.equal(db2, db), tag + ": a second identical call gave other bits (fused bias)"
    else:
        from vltf_amd._ffi import VltfError
        with pytest.raises(VltfError):
            run_wgrad(conv, xd, dyd, n, True, exact_ws=True)

    dbs = []
    for _ in range(2):
        bws, nf, sentinel = nan_ws(64 * cout * 4)
        db = torch.full((cout,), float("nan"), device=DEV)
        ops.bias_grad_nchw(dyd, db, bws[:nf])
        torch.cuda.synchronize()
        assert ws_untouched_behind(bws, nf, sentinel)
        dbs.append(db)
    print("%s db_nchw=%.4f" % (tag, bound_ratio(host(dbs[0]), dbo)))
    close(host(dbs[0]), dbo, msg=tag + " bias_grad_nchw")
    assert torch.equal(dbs[0], dbs[1])

    if layout == "phase" and mode == "f32":
        # the phase-split layout changes addresses only (same kernel, same pixel and tile order): the plain layout's bits
        convp, xp, dyp, _, _ = make_layer(ops, layer, n, "plain")
        dwp, _ = run_wgrad(convp, xp, dyp, n, False, exact_ws=True)
        assert torch.equal(dwp, dw), tag + ": phase-split and plain x give different bits"


@pytest.mark.parametrize("layer,n,layout", BF16_CASES)
def test_wgrad_in_loop_bf16(ops, conv_math, layer, n, layout):
    """vl_set_conv_math("bf16"): test_conv_plain_bf16_mode's band (inside 6e-3 relative L2 of the reference, NOT inside 1e-4)."""
    conv, xd, dyd, dwo, _ = make_layer(ops, layer, n, layout)
    conv_math("bf16")
    dw, _ = run_wgrad(conv, xd, dyd, n, False, exact_ws=True)
    err = float(np.linalg.norm(host(dw) - dwo) / np.linalg.norm(dwo))
    print("WGF %s n=%d %s bf16 relL2=%.3e" % (layer, n, layout, err))
    assert 1e-4 < err < 6e-3, (layer, n, layout, err)
    dw2, _ = run_wgrad(conv, xd, dyd, n, False, exact_ws=False)
    assert torch.equal(dw, dw2)


@pytest.mark.parametrize("layer,n", [(l, n) for l in STACK for n in C8_FRAMES])
def test_packed_wgrad_against_the_full_batch_reference(ops, layer, n):
    """vl_conv_c8_wgrad / vl_bias_grad_c8 on bf16-representable operands: the products are exact, so the float64 reference of the
    rounded inputs applies at the fp32 tolerance."""
    h, w, cin, cout, k, s, g = LAYERS[layer]
    x, dy, dwo, dbo = case_data(layer, n, True)
    conv = ops.Conv(cin, h, w, cout, k, k, s, g)
    pad = conv.same_pad()
    conv.set_halo(pad, 0, pad, 0)
    xb, dyb = to_c8(haloed(x, pad)), to_c8(haloed(dy, pad))
    need = conv.c8_wgrad_ws_bytes(n)
    tag = "WGF %s n=%d c8 ws_bytes=%d" % (layer, n, need)
    dws = []
    for slack in (0, 4096):
        ws, nf, sentinel = nan_ws(need, slack)
        dw = torch.full(conv.w_shape, float("nan"), device=DEV)
        conv.c8_wgrad(xb, dyb, dw, ws[:nf + slack])
        torch.cuda.synchronize()
        assert ws_untouched_behind(ws, nf, sentinel), "vl_conv_c8_wgrad wrote behind the workspace it asked for"
        assert not bool(torch.isnan(dw).any()), "NaN left in dw"
        dws.append(dw)
    print("%s dw=%.4f" % (tag, bound_ratio(host(dws[0]), dwo)))
    close(host(dws[0]), dwo, msg=tag + " dw")
    assert torch.equal(dws[0], dws[1]), tag + ": a second identical call gave other bits"
    dbs = []
    for _ in range(2):
        bws, nf, sentinel = nan_ws(64 * 8 * ((cout + 7) // 8) * 4)
        db = torch.full((cout,), float("nan"), device=DEV)
        ops.bias_grad_c8(dyb, db, bws[:nf], cout, pad)
        torch.cuda.synchronize()
        assert ws_untouched_behind(bws, nf, sentinel)
        dbs.append(db)
    print("%s db=%.4f" % (tag, bound_ratio(host(dbs[0]), dbo)))
    close(host(dbs[0]), dbo, msg=tag + " bias_grad_c8")
    assert torch.equal(dbs[0], dbs[1])


def test_the_frame_counts_cover_the_launch_shapes(ops):
    """On a 256-CU device FRAMES must give every conv2-conv5 launch of wgrad_dma_kernel: a split without tiles, an odd and an even
    tile count per split past the pipeline's fill, 32 or more tiles per split, and a batch that ends inside a 64-pixel tile.  The
    split count comes from the workspace query: when the heuristic changes, adjust FRAMES, not the clauses."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != 256:
        pytest.skip("the frame counts are chosen for wgrad_splits() on 256 CUs, this device has %d" % cus)
    missing = []
    for layer in STACK:
        h, w, cin, cout, k, s, g = LAYERS[layer]
        conv = ops.Conv(cin, h, w, cout, k, k, s, g)
        conv.set_halo(conv.same_pad(), 0, k - 1, 0)
        shapes = [split_shape(conv, n, k * k * (cin // g), cout) for n in FRAMES]
        clauses = {
            "a split without tiles": any(empty >= 1 for _, _, empty in shapes),
            "odd tiles per split >= 3": any(per >= 3 and per % 2 == 1 for _, per, _ in shapes),
            "even tiles per split >= 4": any(per >= 4 and per % 2 == 0 for _, per, _ in shapes),
            "tiles per split >= 32": any(per >= 32 for _, per, _ in shapes),
            "a partial last pixel tile": any(n * conv.oh * conv.ow % 64 != 0 for n in FRAMES),
        }
        missing += ["%s: %s (splits, per, empty = %s)" % (layer, name, shapes) for name, ok in clauses.items() if not ok]
    assert not missing, "FRAMES no longer covers: " + "; ".join(missing)


@pytest.mark.parametrize("n,h,w,cin,cout,k,s,g", [(3, 24, 20, 3, 8, 11, 4, 1),       # asymmetric SAME padding, strided
                                                  (3, 67, 67, 3, 96, 11, 4, 1),      # conv1's geometry on a small image
                                                  (3, 13, 13, 384, 384, 3, 1, 2),    # conv4: groups
                                                  (3, 10, 7, 48, 80, 3, 1, 2)])
def test_the_reference_is_the_oracle(n, h, w, cin, cout, k, s, g):
    """reference_grads (torch, explicit padding, OIHW -> HWIO) == oracle.lrcn_oracle.grouped_conv_grad, both float64."""
    rng = np.random.default_rng(h * 100 + cin)
    x = rng.standard_normal((n, h, w, cin)).astype(np.float32)
    dy = rng.standard_normal((n, -(-h // s), -(-w // s), cout)).astype(np.float32)
    wt = np.zeros((k, k, cin // g, cout), np.float32)
    _, dwo, dbo = O.grouped_conv_grad(x, wt, dy, s, g, need_dx=False)
    dw, db = reference_grads(torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(dy).permute(0, 3, 1, 2), k, s, g)
    np.testing.assert_allclose(dw, dwo, rtol=1e-12, atol=1e-12 * float(np.abs(dwo).max()))
    np.testing.assert_allclose(db, dbo, rtol=1e-12, atol=1e-12 * float(np.abs(dbo).max()))
