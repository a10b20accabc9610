"""Everything between the TFRecord bytes and conv1 against the restatements of tests/feed_ref.py, bit for bit and on every launch
branch: vl_input_prep_u8 (the crop feed), vl_input_prep_u8_s2d (both kernels) and vl_s2d_c8_from_x0 (the packed feed),
vl_nhwc_to_nchw and vl_nchw_to_nhwc.  tests/test_feed_geometry.py (CPU) shows that the two references agree and that the case lists
tell wrong feeds apart.

No tolerance anywhere: every operation here is a copy, a u8 -> f32 conversion minus an f32 mean, or that rounded to bf16 (nearest even),
so the reference equals the kernel in every bit.

The harness.  fp32 outputs are views into one sentinel-filled allocation per test, placed by test_gemm_geometry_gpu's Layout: 1, 2 or 3
floats past a 16-byte boundary, guard floats on both sides.  The allocation is downloaded once; the expected elements are compared as
uint32 patterns, "written 0.0" is the pattern 0x00000000, and everything a call must not touch -- halo rows, the floats between and
around the tensors -- must still be the sentinel.  Every call runs twice into two views that must hold the same bits.  The packed bf16
outputs are written with 16-byte stores, so their views begin ON a 16-byte boundary of an allocation filled with a 16-bit sentinel,
64 elements of it between and around them; the feed writes every slot of such a buffer, so there the whole buffer is compared."""
import numpy as np
import pytest
import torch

from tests import feed_ref as F
from tests.test_cutmix_gpu import special_words, x0_index
from tests.test_gemm_geometry_gpu import DEV, SENTINEL, Layout, cus
from tests.test_reductions_gpu import intact, take

pytestmark = pytest.mark.gpu

SENT_BITS = int(np.float32(SENTINEL).view(np.uint32))
SENT16 = 0x5A5A                                                # as bf16 a finite number no feed produces


@pytest.fixture(scope="module")
def ops():
    import vltf_amd.ops as ops_
    return ops_


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def sentinel_pool(floats):
    out = torch.full((floats,), SENTINEL, device=DEV)
    assert out.data_ptr() % 16 == 0
    return out


def first_difference(got, want, what):
    bad = np.flatnonzero(got != want)
    return "%s: %d of %d words differ, the first at %d: %#010x, expected %#010x" % (what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


# ---- 1. vl_input_prep_u8 --------------------------------------------------------------------------------------------------------------------
def feed_call(ops, case, src, dst):
    ops.input_prep_u8(src, dst, dev(case["cy"]), dev(case["cx"]), dev(case["mir"]), dev(case["mean"]), halo=case["halo"], phase=case["phase"],
                      out_hw=(case["oh"], case["ow"]))


def run_crop(ops, cases):
    """Each case twice into the sentinel pool; pixels = reference bits, the other columns of the interior rows 0x00000000, halo rows and
    surroundings the sentinel."""
    lay, recs = Layout(), []
    for c in cases:
        shape = ops.phase_split_shape(c["src"].shape[0], 3, c["oh"], c["ow"], c["halo"], c["phase"])
        recs.append((c, shape, int(np.prod(shape)), [lay.place(int(np.prod(shape))) for _ in range(2)]))
    out = sentinel_pool(lay.total())
    for c, shape, count, offs in recs:
        src = dev(c["src"])
        for o in offs:
            feed_call(ops, c, src, out[o:o + count].view(shape))
    got = out.cpu().numpy()
    for c, shape, count, offs in recs:
        val, written = F.crop_want(c)
        assert val.shape == shape, c["name"]
        want = F.expected_bits(val, written, SENTINEL)
        a, b = (take(got, o, count).view(np.uint32) for o in offs)
        assert np.array_equal(a, b), c["name"] + ": two calls, two results"
        assert np.array_equal(a, want), first_difference(a, want, c["name"])
        if c["halo"]:
            assert (want == SENT_BITS).any() and (want == 0).any(), c["name"]           # the case has both kinds of non-pixel
    intact(got, "vl_input_prep_u8")


@pytest.mark.parametrize("halo,phase", F.CROP_LAYOUTS)
def test_crop_feed(ops, halo, phase):
    """(oh, ow) = (17, 19), (1, 1), (9, 14), (8, 13) from (oh + 3) x (ow + 5) frames: six frames at the four crop corners and two
    random offsets, mirror alternating; at (0, 1) and (2, 4) also without a mean, with crop_y = crop_x = None under a mirror, and
    with no room to crop (raw frame = output frame)."""
    cases = F.crop_cases(halo, phase)
    assert {(c["oh"], c["ow"]) for c in cases} == set(F.CROP_SIZES)
    run_crop(ops, cases)


@pytest.mark.parametrize("rh,rw,oh,ow,halo,phase,bx", [(20, 22, 17, 19, 0, 1, 1), (42, 33, 40, 30, 2, 4, 2)])
def test_crop_feed_both_grids(ops, rh, rw, oh, ow, halo, phase, bx):
    """The launcher takes bx = ceil(per_img / 1024) workgroups per image, the kernel's loop turning up to four times, unless
    bx * n < 8 * CUs: then ceil(per_img / 256), one element per thread.  n = ceil(8 * CUs / bx) is the first batch on the loop side,
    n - 1 the last on the other; per_img > 256 * bx, so the loop does turn.  Both against the reference, and the frames they share
    bit for bit against each other.  The second call of each is compared on the device."""
    ncu = cus()
    per_img = oh * phase * -(-(ow + 2 * halo) // phase)
    n = -(-8 * ncu // bx)
    assert -(-per_img // 1024) == bx and per_img > 256 * bx and bx * n >= 8 * ncu > bx * (n - 1) and n <= 65535
    rng = np.random.default_rng(ncu + bx)
    case = dict(name="grid", src=F.u8_frames(bx, n, rh, rw), cy=rng.integers(0, rh - oh + 1, n).astype(np.int32),
                cx=rng.integers(0, rw - ow + 1, n).astype(np.int32), mir=rng.integers(0, 2, n).astype(np.uint8), mean=F.MEAN, oh=oh, ow=ow,
                halo=halo, phase=phase)
    shape = ops.phase_split_shape(n, 3, oh, ow, halo, phase)
    per = int(np.prod(shape[1:]))
    lay = Layout()
    o_loop, o_flat = lay.place(n * per), lay.place((n - 1) * per)
    src = dev(case["src"])
    pools = []
    for _ in range(2):
        out = sentinel_pool(lay.total())
        feed_call(ops, case, src, out[o_loop:o_loop + n * per].view(shape))
        feed_call(ops, case, src[:n - 1], out[o_flat:o_flat + (n - 1) * per].view((n - 1,) + shape[1:]))
        pools.append(out)
    assert torch.equal(pools[0].view(torch.int32), pools[1].view(torch.int32)), "two calls, two results"
    got = pools[0].cpu().numpy()
    want = F.expected_bits(*F.crop_want(case), SENTINEL)
    loop, flat = take(got, o_loop, n * per).view(np.uint32), take(got, o_flat, (n - 1) * per).view(np.uint32)
    assert np.array_equal(loop, want), first_difference(loop, want, "loop branch, n = %d" % n)
    assert np.array_equal(flat, want[:(n - 1) * per]), first_difference(flat, want[:(n - 1) * per], "one element per thread, n = %d" % (n - 1))
    assert np.array_equal(loop[:(n - 1) * per], flat)
    intact(got, "vl_input_prep_u8")


def test_crop_feed_batch_limit(ops):
    """An image per blockIdx.y: 65535 frames (2 x 2 -> 1 x 1) run and are right, 65536 are refused and nothing is launched."""
    from vltf_amd._ffi import VltfError
    n = 65535
    rng = np.random.default_rng(65535)
    src = F.u8_frames(9, n + 1, 2, 2)
    cy, cx, mir = rng.integers(0, 2, n + 1).astype(np.int32), rng.integers(0, 2, n + 1).astype(np.int32), rng.integers(0, 2, n + 1).astype(np.uint8)
    case = dict(name="65535 frames", src=src[:n], cy=cy[:n], cx=cx[:n], mir=mir[:n], mean=F.MEAN, oh=1, ow=1, halo=0, phase=1)
    run_crop(ops, [case])
    lay = Layout()
    o = lay.place(3 * (n + 1))
    out = sentinel_pool(lay.total())
    with pytest.raises(VltfError, match="exceeds the grid limit"):
        ops.input_prep_u8(dev(src), out[o:o + 3 * (n + 1)].view(n + 1, 3, 1, 1), dev(cy), dev(cx), dev(mir), dev(F.MEAN))
    intact(out.cpu().numpy(), "a refused vl_input_prep_u8")


# ---- 2. the packed feed ----------------------------------------------------------------------------------------------------------------------
class Layout16:
    """Offsets, in 16-bit elements, of views that begin on a 16-byte boundary with at least 64 elements between and around them."""

    def __init__(self):
        self.size = 0

    def place(self, count):
        off = (self.size + 64 + 7) // 8 * 8
        self.size = off + count
        return off

    def total(self):
        return self.size + 64


def s2d_conv(ops, desc, phase_split=False):
    cin, h, w, k, s = desc
    conv = ops.Conv(cin, h, w, 8, k, k, s, 1)
    conv.set_halo(conv.same_pad(), 0, 0, 0)
    if phase_split:
        assert conv.set_x_phase_split(True) == s
    oh, ow, pt, pl = F.same_geometry(h, w, k, s)
    assert (conv.oh, conv.ow) == (oh, ow)
    return conv, ops.c8_shape(1, cin * s * s, oh, ow, (-(-k // s) - 1) // 2)[1:]


def run_packed(ops, jobs):
    """jobs: [(name, shape of the packed buffer, expected int16 image, launch(xb))], each launched twice; the WHOLE buffer is compared."""
    lay, recs = Layout16(), []
    for name, shape, want, launch in jobs:
        assert tuple(want.shape) == tuple(shape), name
        recs.append((name, shape, want, launch, [lay.place(want.size) for _ in range(2)]))
    out = torch.full((lay.total(),), SENT16, dtype=torch.int16, device=DEV)
    assert out.data_ptr() % 16 == 0
    for name, shape, want, launch, offs in recs:
        for o in offs:
            launch(out[o:o + want.size].view(torch.bfloat16).view(shape))
    got = out.cpu().numpy()
    for name, shape, want, launch, offs in recs:
        a, b = (got[o:o + want.size].copy() for o in offs)
        for o in offs:
            got[o:o + want.size] = SENT16
        assert np.array_equal(a, b), name + ": two calls, two results"
        w16 = want.reshape(-1)
        assert np.array_equal(a, w16), first_difference(a.view(np.uint16), w16.view(np.uint16), name)
    assert (got == SENT16).all(), "written outside a packed buffer"


def feed_job(ops, case):
    conv, per = s2d_conv(ops, case["desc"])
    src, cy, cx, mir, mean = dev(case["src"]), dev(case["cy"]), dev(case["cx"]), dev(case["mir"]), dev(case["mean"])
    return (case["name"], (case["src"].shape[0],) + tuple(per), F.packed_want(case),
            lambda xb: conv.input_prep_u8_s2d(src, xb, cy, cx, mir, mean))


def test_packed_feed_generic_kernel(ops):
    """Any cin and stride: (2, 9, 10, 5, 2), (3, 9, 10, 5, 2) and (4, 11, 8, 9, 3) -- the last chunk of the latter two half used, its
    upper slots +0 -- four frames of (h + 3) x (w + 5), crops at two corners and two random offsets, mirror alternating; and once with
    a mean that puts u8 - mean exactly between two bf16 values.  (1, 7, 7, 3, 2) is not run: ceil(3 / 2) is even and the host
    check refuses it, launching nothing."""
    from vltf_amd._ffi import VltfError
    cases = [F.packed_case(d) for d in F.GENERIC] + [F.packed_case(F.GENERIC[1], tie=True)]
    assert F.is_bf16_tie(F.feed_frames(cases[-1]["src"], cases[-1]["cy"], cases[-1]["cx"], cases[-1]["mir"], cases[-1]["mean"], 9, 10)).any()
    run_packed(ops, [feed_job(ops, c) for c in cases])
    cin, h, w, k, s = F.REFUSED
    conv = ops.Conv(cin, h, w, 8, k, k, s, 1)
    conv.set_halo(conv.same_pad(), 0, 0, 0)
    shape = ops.c8_shape(1, cin * s * s, conv.oh, conv.ow, 0)
    xb = torch.full((int(np.prod(shape)),), SENT16, dtype=torch.int16, device=DEV)
    with pytest.raises(VltfError, match="must be odd"):
        conv.input_prep_u8_s2d(dev(F.u8_frames(1, 1, h, w, cin)), xb.view(torch.bfloat16).view(shape))
    assert bool((xb == SENT16).all())


def test_packed_feed_three_channels_stride_4(ops):
    """k = 11, s = 4, cin = 3 over h in {17 .. 20} x w in {20 .. 23}: pl = 3, 5, 4, 4, so the 12-byte load of a column quad starts at
    three residues of 4 and the quads at both edges are cut by the frame, wholly outside it, or inside (asserted on the inputs).
    Frame 0 uncropped and unmirrored, frame 1 at the bottom-right corner and mirrored (the reversed quad), frame 2 random and
    mirrored.  Once with the mean of the bf16 ties."""
    residues, classes = set(), set()
    for cin, h, w, k, s in F.C3S4_SWEEP:
        oh, ow, pt, pl = F.same_geometry(h, w, k, s)
        residues.add(-pl % 4)
        classes |= F.c3s4_classes(w, pl, F.packed_dims(cin, k, s, oh, ow)[2])
    assert len(residues) > 1 and classes == {"interior", "left, cut", "left, outside", "right, cut", "right, outside"}
    tie = F.packed_case(F.S2D_ALONE[0], tie=True)
    assert F.is_bf16_tie(F.feed_frames(tie["src"], tie["cy"], tie["cx"], tie["mir"], tie["mean"], 19, 23)).any()
    cases = [F.packed_case(d) for d in F.C3S4_SWEEP] + [tie]
    for c in cases:
        assert c["mir"].tolist() == [0, 1, 1] and (c["cy"][0], c["cx"][0]) == (0, 0) and (c["cy"][1], c["cx"][1]) == (3, 5)
    run_packed(ops, [feed_job(ops, c) for c in cases])


def test_packed_feed_alexnet_frame(ops):
    """227 x 227 out of 240 x 320, two frames: the workload's own geometry, pt = pl = 4."""
    case = F.packed_case(F.C3S4_FULL)
    assert case["src"].shape == (2, 240, 320, 3) and F.same_geometry(227, 227, 11, 4) == (57, 57, 4, 4)
    run_packed(ops, [feed_job(ops, case)])


@pytest.mark.parametrize("desc", F.S2D_ALONE)
def test_s2d_from_x0_alone(ops, desc):
    """vl_s2d_c8_from_x0 from a host-built x0 -- once plain with its halo, once column-phase-split -- of random fp32 with exact bf16
    ties and zeros of both signs: both give the reference's bits, hence each other's."""
    cin, h, w, k, s = desc
    oh, ow, pt, pl = F.same_geometry(h, w, k, s)
    img = F.s2d_alone_frames(desc)
    assert F.is_bf16_tie(img).any() and (img < 0).any()
    want = F.pack_s2d(img, cin, h, w, k, s, pt, pl, oh, ow)
    jobs = []
    for split in (False, True):
        conv, per = s2d_conv(ops, desc, split)
        x0 = dev(F.x0_layout(img, conv.x_halo, s if split else 1))
        assert tuple(x0.shape) == tuple(conv.x_shape(2))
        jobs.append(("%s %s" % (desc, "phase split" if split else "plain"), (2,) + tuple(per), want,
                     lambda xb, conv=conv, x0=x0: conv.s2d_c8_from_x0(x0, xb)))
    run_packed(ops, jobs)


# ---- 3. layout converters ----------------------------------------------------------------------------------------------------------------------
NHWC_SHAPES = [(2, 5, 7, 3), (1, 1, 1, 1), (3, 4, 9, 5)]
NHWC_LAYOUTS = [(0, 1), (2, 1), (0, 4), (3, 4), (1, 3)]
BIG = (2, 64, 130, 130)                                        # 2 163 200 elements > 8192 * 256: the grid-stride loops turn


def x0_index_c(n, h, w, c, halo, phase):
    """tests/test_cutmix_gpu.py's x0_index for c channels: [n, h, w, c] -> flat index of plane ch * phase + (x + halo) % phase, row
    y + halo, column (x + halo) // phase."""
    hp, wq = h + 2 * halo, -(-(w + 2 * halo) // phase)
    f, y, x, ch = np.meshgrid(np.arange(n), np.arange(h), np.arange(w), np.arange(c), indexing="ij")
    return ((f * c * phase + ch * phase + (x + halo) % phase) * hp + y + halo) * wq + (x + halo) // phase


def words(shape, seed):
    """float32 tensor on the device holding special_words' patterns, and those patterns."""
    u = special_words(int(np.prod(shape)), seed).reshape(shape)
    return torch.from_numpy(u.view(np.int32)).to(DEV).view(torch.float32), u


def test_x0_index_for_c_channels_is_x0_index():
    assert np.array_equal(x0_index_c(4, 5, 7, 3, 2, 4), x0_index(2, 2, 5, 7, 2, 4))


@pytest.mark.parametrize("halo,phase", NHWC_LAYOUTS)
def test_nhwc_to_nchw(ops, halo, phase):
    """A copy: NaN payloads, -0.0 and denormals arrive as they left.  Pixels where the layout formula puts them; EVERYTHING else still
    the sentinel, the halo and phase-padding columns of the interior rows included: the kernel writes pixels only (include/vltf.h)."""
    lay, recs = Layout(), []
    for i, (n, h, w, c) in enumerate(NHWC_SHAPES):
        shape = ops.phase_split_shape(n, c, h, w, halo, phase)
        src, u = words((n, h, w, c), 11 * i + halo + phase)
        recs.append((n, h, w, c, shape, int(np.prod(shape)), src, u, [lay.place(int(np.prod(shape))) for _ in range(2)]))
    out = sentinel_pool(lay.total())
    for n, h, w, c, shape, count, src, u, offs in recs:
        for o in offs:
            ops.nhwc_to_nchw(src, out[o:o + count].view(shape), halo=halo, phase=phase)
    got = out.cpu().numpy()
    for n, h, w, c, shape, count, src, u, offs in recs:
        idx = x0_index_c(n, h, w, c, halo, phase)
        assert len(np.unique(idx)) == idx.size and idx.max() < count
        want = np.full(count, SENT_BITS, np.uint32)
        want[idx] = u
        a, b = (take(got, o, count).view(np.uint32) for o in offs)
        assert np.array_equal(a, b), "two calls, two results"
        assert np.array_equal(a, want), first_difference(a, want, "nhwc_to_nchw %s halo %d phase %d" % ((n, h, w, c), halo, phase))
    intact(got, "vl_nhwc_to_nchw")


def test_nchw_to_nhwc(ops):
    """Bit for bit the numpy transpose, and back through vl_nhwc_to_nchw (halo 0) to the source bits."""
    lay, recs = Layout(), []
    for i, (n, h, w, c) in enumerate(NHWC_SHAPES):
        src, u = words((n, c, h, w), 40 + i)
        recs.append((n, h, w, c, src, u, [lay.place(u.size) for _ in range(2)], lay.place(u.size)))
    out = sentinel_pool(lay.total())
    for n, h, w, c, src, u, offs, back in recs:
        for o in offs:
            ops.nchw_to_nhwc(src, out[o:o + u.size].view(n, h, w, c))
        ops.nhwc_to_nchw(out[offs[0]:offs[0] + u.size].view(n, h, w, c), out[back:back + u.size].view(n, c, h, w))
    got = out.cpu().numpy()
    for n, h, w, c, src, u, offs, back in recs:
        want = np.ascontiguousarray(u.transpose(0, 2, 3, 1)).reshape(-1)
        a, b = (take(got, o, u.size).view(np.uint32) for o in offs)
        assert np.array_equal(a, b) and np.array_equal(a, want), first_difference(a, want, "nchw_to_nhwc %s" % ((n, h, w, c),))
        assert np.array_equal(take(got, back, u.size).view(np.uint32), u.reshape(-1)), "round trip"
    intact(got, "vl_nchw_to_nhwc")


def test_layout_converters_past_one_grid(ops):
    """(2, 64, 130, 130): more elements than the 8192 x 256 threads of the capped grid, so the grid-stride loop of both kernels takes
    a second turn (for 65 536 of them).  vl_nhwc_to_nchw into halo 1, phase 4; vl_nchw_to_nhwc of the same element count (its
    n * hw * c is formed in 64 bits: hw is an int64).  The second call of each is compared on the device."""
    n, h, w, c = BIG
    total = n * h * w * c
    assert 8192 * 256 < total < 2 * 8192 * 256
    halo, phase = 1, 4
    shape = ops.phase_split_shape(n, c, h, w, halo, phase)
    count = int(np.prod(shape))
    src, u = words((n, h, w, c), 77)
    lay = Layout()
    o_split, o_nhwc = lay.place(count), lay.place(total)
    pools = []
    for _ in range(2):
        out = sentinel_pool(lay.total())
        ops.nhwc_to_nchw(src, out[o_split:o_split + count].view(shape), halo=halo, phase=phase)
        ops.nchw_to_nhwc(src.view(n, h, w, c), out[o_nhwc:o_nhwc + total].view(n, w, c, h))   # the same words read as [n][c' = h][h' = w][w' = c]
        pools.append(out)
    assert torch.equal(pools[0].view(torch.int32), pools[1].view(torch.int32)), "two calls, two results"
    got = pools[0].cpu().numpy()
    want = np.full(count, SENT_BITS, np.uint32)
    want[x0_index_c(n, h, w, c, halo, phase)] = u
    a = take(got, o_split, count).view(np.uint32)
    assert np.array_equal(a, want), first_difference(a, want, "nhwc_to_nchw %s" % (BIG,))
    b = take(got, o_nhwc, total).view(np.uint32)
    want = np.ascontiguousarray(u.transpose(0, 2, 3, 1)).reshape(-1)
    assert np.array_equal(b, want), first_difference(b, want, "nchw_to_nhwc %s" % ((n, w, c, h),))
    intact(got, "the layout converters")
