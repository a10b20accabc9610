"""The launch arithmetic of the pooling / LRN family of csrc/pointwise.hip restated in plain Python for the tests: vl_pool_lrn_bwd
(channel-stream 5/3 and 16/9, the LDS-staged chunked fall-back, refuse), plb_channel_ranges with its forced-count loop,
vl_pool_lrn_bwd_c8's gate, launch_lrn_pool_fwd (band search, balancing, threads, channel ranges, refuse), vl_maxpool_fwd / _bwd -- and
the case lists, seeded inputs and fp64 references (oracle/lrcn_oracle.py) that tests/test_pool_geometry.py (CPU) and
tests/test_pool_geometry_gpu.py share.  Nothing here imports the package: the kernels are checked AGAINST these.  Every plan is a
function of the shape and the CU count; N(cus) = 2 x CUs is the batch at which launch_lrn_pool_fwd wants ONE band per image.

The 20-channel instantiation pool_lrn_bwd_stream_kernel<20, 11> cannot be reached in the product build: it is tried after <5, 3> on
the same channel counts ((c + 4) % 20 == 0 implies (c + 4) % 5 == 0), so it would need 5 m ow > 768 (m ow >= 154) and 20 m ow <= 2816
(m ow <= 140) at once, and the switches that skip <5, 3> (VL_POOL_LRN_BWD_R1, VL_POOL_LRN_CHK16) are compiled out of that build.
plb_plan therefore never answers chunk 20 (tests/test_pool_geometry.py sweeps it); the code is left alone.

Inputs are post-ReLU data scaled by 30 as in tests/test_ops_gpu.py: half of the values are exact zeros, so ties at 0 are exact."""
import collections
import functools

import numpy as np

from oracle import lrcn_oracle as O


def ceil_div(a, b):
    return -(-a // b)


def pool_out(h, k=3, s=2):
    return (h - k) // s + 1


def N(cus):
    """The batch of the many-image cases: launch_lrn_pool_fwd's want = ceil(2 CUs / n) is 1, vl_maxpool_bwd's hwc form takes CB = 64."""
    return 2 * cus


# ---- launchers ----------------------------------------------------------------------------------------------------------------------
def plb_channel_ranges(workgroups, c, unit, lead, cus, forced=0):
    """plb_channel_ranges: (ranges, channels per range).  forced 1..4: vl_pool_lrn_bwd_test_ranges, lowered until no range is empty
    or shorter than the lead-in."""
    slots, best, best_cost, cper = 8 * cus, 1, 0, c
    for sp in range(1, 5):
        per = ceil_div(ceil_div(c, sp), unit) * unit
        if sp > 1 and (per * (sp - 1) >= c or per < lead):
            continue
        cost = ceil_div(workgroups * sp, slots) * (per + 12)
        if sp == 1 or cost < best_cost:
            best, best_cost, cper = sp, cost, per
    if 1 <= forced <= 4:
        best = forced
        cper = ceil_div(ceil_div(c, best), unit) * unit
        while best > 1 and (cper * (best - 1) >= c or cper < lead):
            best -= 1
            cper = ceil_div(ceil_div(c, best), unit) * unit
    return best, cper


def ranges_of(c, nz, cper):
    """[(R0, R1)] of the output channels of each grid-z slice."""
    return [(z * cper, min(c, (z + 1) * cper)) for z in range(nz)]


def stream_rows(w):
    """(input rows a 256-pixel band can touch, pooled rows staged for it)."""
    rows = (255 + w - 1) // w + 1
    return rows, rows // 2 + 2


PlbPlan = collections.namedtuple("PlbPlan", "form chk nst grid nz cper")
# form   "stream": pool_lrn_bwd_stream_kernel<chk, nst>; "chunked": pool_lrn_bwd_kernel<16, 2, 512>; "refuse": an error, no launch
# grid   stream: (256-pixel bands over the halo-layout rows, images padded to 8, nz); chunked: (512-pixel bands, 16-channel blocks, n)


def plb_plan(n, c, h, w, p_halo, dx_halo, cus, beta=0.75, forced=0):
    """What vl_pool_lrn_bwd launches."""
    oh, ow = pool_out(h), pool_out(w)
    owp = ow + 2 * p_halo
    pplane, origin = (oh + 2 * p_halo) * owp, p_halo * owp + p_halo
    if n > 65528:
        return PlbPlan("refuse", 0, 0, None, 0, 0)
    m = stream_rows(w)[1]
    fits32 = (c + 24) * h * w * 4 < 2 ** 31 and (c + 24) * (h + 2 * dx_halo) * (w + 2 * dx_halo) * 4 < 2 ** 31 and \
        (c * pplane - origin) * 4 < 2 ** 31 and pplane < 2 ** 24
    ok = beta == 0.75 and fits32
    bands = ceil_div(h * (w + 2 * dx_halo), 256)
    nz, cper = plb_channel_ranges(bands * n, c, 1, 4, cus, forced)
    grid = (bands, ceil_div(n, 8) * 8, nz)
    if ok and (c + 4) % 5 == 0 and 5 * m * ow <= 3 * 256:
        return PlbPlan("stream", 5, 3, grid, nz, cper)
    if ok and (c + 4) % 20 == 0 and 20 * m * ow <= 11 * 256:
        return PlbPlan("stream", 20, 11, grid, nz, cper)
    if ok and 16 * m * ow <= 9 * 256:
        return PlbPlan("stream", 16, 9, grid, nz, cper)
    max_prow = ((512 + w - 1) // w + 1) // 2 + 3
    lds = (20 * max_prow * ow * 5 + 15) & ~15
    if lds > 64 * 1024:
        return PlbPlan("refuse", 0, 0, None, 0, 0)
    return PlbPlan("chunked", 16, 0, (ceil_div(h * w, 512), ceil_div(c, 16), n), 1, c)


def plb_c8_plan(n, c, h, w, p_halo, dxb_halo, cus, forced=0):
    """What vl_pool_lrn_bwd_c8 launches: <8, 5> or nothing (8 m ow <= 1280 staging slots)."""
    oh, ow = pool_out(h), pool_out(w)
    owp = ow + 2 * p_halo
    pplane, origin = (oh + 2 * p_halo) * owp, p_halo * owp + p_halo
    m = stream_rows(w)[1]
    fits32 = (c + 24) * h * w * 4 < 2 ** 31 and (ceil_div(c, 8) + 3) * (h + 2 * dxb_halo) * (w + 2 * dxb_halo) * 16 < 2 ** 31 and \
        (c * pplane - origin) * 4 < 2 ** 31 and pplane < 2 ** 24
    if n > 65528 or not fits32 or 8 * m * ow > 5 * 256:
        return PlbPlan("refuse", 0, 0, None, 0, 0)
    bands = ceil_div(h * w, 256)
    nz, cper = plb_channel_ranges(bands * n, c, 8, 8, cus, forced)
    return PlbPlan("stream", 8, 5, (bands, ceil_div(n, 8) * 8, nz), nz, cper)


LpfPlan = collections.namedtuple("LpfPlan", "form prb bands last threads by grid nz cper")
# prb    pooled rows per band after balancing; bands of them, the last one holds `last` rows (ragged when last < prb)
# by     "outputs" when the pooled outputs of a chunk, not the band's pixels, set the thread count


def lpf_plan(n, c, h, w, p_halo, cus, c8=False, forced=0):
    """launch_lrn_pool_fwd<2, 2, 1>: 2-channel chunks, 2 pixels and 1 pooled output per thread."""
    CHK, PPT, NSL = 2, 2, 1
    oh, ow = pool_out(h), pool_out(w)
    row_w = ow if c8 else ow + 2 * p_halo

    def need(cand):
        return ceil_div((2 * cand + 1) * w, PPT), ceil_div(CHK * cand * row_w, NSL)

    prb = 0
    for cand in range(oh, 0, -1):
        t = ceil_div(max(need(cand)), 64) * 64
        if t <= 512 and 2 * (CHK * (2 * cand + 1) * w + 1) * 4 <= 64 * 1024:
            prb = cand
            break
    if not prb or n > 65528:
        return LpfPlan("refuse", 0, 0, 0, 0, "", None, 0, 0)
    bands = ceil_div(oh, prb)
    want = ceil_div(2 * cus, n)
    if bands < want:
        bands = min(want, oh)
    prb = ceil_div(oh, bands)
    bands = ceil_div(oh, prb)
    px, out = need(prb)
    threads = ceil_div(max(px, out), 64) * 64
    nz, cper = 1, c
    wantz = min(ceil_div(8 * cus, bands * n), 8, max(c // 32, 1))
    if forced >= 1:
        wantz = forced
    if wantz > 1:
        cper = ceil_div(ceil_div(c, wantz), 8) * 8
        nz = ceil_div(c, cper)
    return LpfPlan("fused", prb, bands, oh - (bands - 1) * prb, threads, "outputs" if out > px else "pixels", (bands, ceil_div(n, 8) * 8, nz), nz, cper)


GRID_CAP = 16384 * 256                                         # elements one pass of the element-per-thread max-pool kernels covers
PoolPlan = collections.namedtuple("PoolPlan", "form inst iters cb")
# form   "generic": maxpool_fwd_kernel / maxpool_bwd_kernel; "hwc": maxpool_bwd_hwc_k3s2_kernel<cb>; "refuse"
# inst   "3/2": K, S compile-time; "runtime": the <0, 0> instantiation; iters: trips of the grid-stride loop of the busiest thread


def maxpool_fwd_plan(n, c, h, w, k, s):
    if not (h >= k and w >= k and k * k <= 255):
        return PoolPlan("refuse", "", 0, 0)
    total = n * c * pool_out(h, k, s) * pool_out(w, k, s)
    if total >= 2 ** 31:
        return PoolPlan("refuse", "", 0, 0)
    return PoolPlan("generic", "3/2" if (k, s) == (3, 2) else "runtime", ceil_div(total, min(ceil_div(total, 256), 16384) * 256), 0)


def maxpool_bwd_plan(n, c, h, w, k, s, hwc, cus):
    oh, ow, total = pool_out(h, k, s), pool_out(w, k, s), n * c * h * w
    if not (h >= k and w >= k) or total >= 2 ** 31:
        return PoolPlan("refuse", "", 0, 0)
    if (k, s) == (3, 2) and hwc and n <= 65535 and 64 * (oh * ow + 1) * 8 <= 48 * 1024:
        return PoolPlan("hwc", "3/2", 1, 64 if ceil_div(c, 64) * n >= 4 * cus else 16)
    return PoolPlan("generic", "3/2" if (k, s) == (3, 2) else "runtime", ceil_div(total, min(ceil_div(total, 256), 16384) * 256), 0)


# ---- cases --------------------------------------------------------------------------------------------------------------------------
# n may be an int or "N" / "N+1" (resolved with the CU count by `resolve`)
Plb = collections.namedtuple("Plb", "n c h w ph dh relu alpha beta bias ranges", defaults=(True, 2e-5, 0.75, 1.0, 0))
PlbC8 = collections.namedtuple("PlbC8", "n c h w ph dh relu packed ranges", defaults=(True, False, 0))
Lpf = collections.namedtuple("Lpf", "n c h w ph alpha bias ranges", defaults=(2e-5, 1.0, 0))
LpfC8 = collections.namedtuple("LpfC8", "n c h w ph packed ranges", defaults=(False, 0))
Lrn = collections.namedtuple("Lrn", "n h w c alpha beta bias", defaults=(2e-5, 0.75, 1.0))
Pool = collections.namedtuple("Pool", "n c h w k s hwc yh dh mask", defaults=(3, 2, False, 0, 0, False))

PLB_CHUNKED = [Plb(2, 16, 5, 63, 0, 0), Plb(2, 21, 7, 120, 1, 2), Plb(2, 7, 9, 11, 0, 1, beta=0.5), Plb(2, 4, 9, 11, 1, 1, relu=False, beta=1.0),
               Plb(1, 7, 5, 300, 0, 0)]
PLB_BOUNDARY = [(Plb(2, 16, 5, 61, 0, 0), Plb(2, 16, 5, 63, 0, 0)), (Plb(2, 7, 5, 57, 0, 0), Plb(2, 7, 5, 59, 0, 0))]       # (streams, chunked)
PLB_REFUSED = Plb(1, 7, 5, 700, 0, 0)
PLB_STREAM = [Plb(9, 7, 9, 11, 0, 1), Plb(17, 16, 9, 11, 1, 0, relu=False), Plb(3, 16, 13, 13, 1, 2, alpha=1e-4, bias=2.0),
              Plb(3, 7, 13, 13, 1, 1, relu=False, alpha=1e-4, bias=2.0), Plb(2, 1, 9, 11, 0, 1), Plb(2, 2, 9, 11, 1, 0), Plb(2, 4, 9, 11, 0, 0, relu=False)]
PLB_FORCED = [Plb(2, c, 9, 11, 1, 1, ranges=r) for c in (7, 21) for r in (2, 3, 4)]        # c = 7: 3 and 4 ranges are lowered to 2
PLB_ALL = PLB_CHUNKED + [c for pair in PLB_BOUNDARY for c in pair if c not in PLB_CHUNKED] + PLB_STREAM + PLB_FORCED

PLB_C8 = [PlbC8(2, 20, 9, 11, 1, 1), PlbC8(9, 33, 9, 11, 1, 2, relu=False), PlbC8(2, 20, 9, 11, 0, 1, packed=True), PlbC8(2, 33, 13, 13, 1, 1, packed=True),
          PlbC8(1, 20, 5, 81, 0, 0)] + [PlbC8(2, c, 9, 11, 1, 1, ranges=r) for c in (20, 33) for r in (2, 3, 4)]
PLB_C8_GATE = (PlbC8(1, 20, 5, 81, 0, 0), PlbC8(1, 20, 5, 83, 0, 0))                      # (accepted, refused)

LPF = [Lpf("N", 8, 13, 13, 1), Lpf("N", 3, 23, 61, 1), Lpf("N+1", 3, 23, 7, 0), Lpf(2, 6, 13, 5, 2), Lpf(1, 5, 3, 341, 0),
       Lpf(2, 1, 9, 11, 1), Lpf(2, 2, 9, 11, 0), Lpf(2, 4, 9, 11, 2), Lpf(3, 7, 13, 13, 1, alpha=1e-4, bias=2.0), Lpf(9, 40, 9, 11, 1, ranges=2)]
LPF_REFUSED = Lpf(1, 5, 3, 342, 0)
LPF_C8 = [LpfC8(2, 20, 9, 11, 1), LpfC8(2, 33, 9, 11, 2), LpfC8(2, 20, 9, 11, 0, packed=True), LpfC8(3, 33, 13, 13, 1, packed=True),
          LpfC8("N", 20, 13, 13, 1, packed=True), LpfC8(2, 33, 9, 11, 1, ranges=3)]

# 3 x 7 x 13 = 273 positions: two workgroups, both image boundaries inside the first; 3 x 11 x 13 = 429: the second one holds a boundary
LRN = [Lrn(3, 7, 13, c, beta=b) for c in (1, 2, 4, 37) for b in (0.75, 0.5, 1.0)] + [Lrn(3, 11, 13, 4), Lrn(3, 11, 13, 37, beta=0.5)] + \
      [Lrn(3, 7, 13, c, alpha=1e-4, beta=b, bias=2.0) for c, b in ((4, 0.75), (37, 0.75), (37, 0.5))]

POOL_KS = [(2, 2), (3, 1), (3, 3), (2, 3), (5, 2), (15, 1)]
POOL_RUNTIME = [Pool(2, 5, 17, 19, k, s, hwc, yh, dh, mask) for k, s in POOL_KS for hwc, yh, dh, mask in ((False, 2, 1, False), (True, 0, 1, True))]
POOL_REFUSED = Pool(1, 1, 17, 19, 16, 1)
POOL_DIV1 = [Pool(2, 1, 3, 3), Pool(2, 1, 5, 4, yh=1, dh=1), Pool(1, 1, 3, 4, hwc=True, mask=True)]
POOL_STRIDE = Pool(2, 32, 515, 515)
POOL_CB64 = [Pool("N", 70, 7, 7, hwc=True, dh=dh, mask=mask) for dh, mask in ((0, False), (1, True))]
POOL_LDS_GATE = (Pool(2, 5, 11, 39, hwc=True, dh=1, mask=True), Pool(2, 5, 17, 25, hwc=True, dh=1, mask=True))               # (LDS form, generic)
POOL_SMALL = POOL_RUNTIME + POOL_DIV1 + POOL_CB64 + list(POOL_LDS_GATE)


def resolve(case, cus):
    """The case with its batch size as a number."""
    n = case.n
    return case._replace(n={"N": N(cus), "N+1": N(cus) + 1}.get(n, n))


def case_id(c):
    return "-".join("%g" % v if isinstance(v, float) else str(int(v) if isinstance(v, bool) else v) for v in c)


# ---- inputs and references ----------------------------------------------------------------------------------------------------------
def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def activations(n, h, w, c, bf16=False):
    """The LRN / pool input, NHWC fp32: post-ReLU, scaled by 30; bf16: rounded to bf16-representable values (a packed conv output)."""
    x = np.maximum(np.random.default_rng([n, h, w, c]).standard_normal((n, h, w, c)) * 30, 0).astype(np.float32)
    return frozen(O.bf16_round(x).astype(np.float32) if bf16 else x)


@functools.lru_cache(maxsize=None)
def gradient(shape):
    return frozen(np.random.default_rng(list(shape) + [1]).standard_normal(shape).astype(np.float32))


def max_pool(x, k, s):
    """oracle.max_pool_valid with an arg-max wide enough for k = 15 (window-local index of the FIRST maximum, up to 224)."""
    n, h, w, c = x.shape
    oh, ow = pool_out(h, k, s), pool_out(w, k, s)
    y = np.full((n, oh, ow, c), -np.inf, dtype=x.dtype)
    arg = np.zeros((n, oh, ow, c), dtype=np.int16)
    for i in range(k):
        for j in range(k):
            v = x[:, i:i + (oh - 1) * s + 1:s, j:j + (ow - 1) * s + 1:s, :]
            upd = v > y
            y = np.where(upd, v, y)
            arg = np.where(upd, np.int16(i * k + j), arg)
    return y, arg


LpfRef = collections.namedtuple("LpfRef", "x l y arg")


@functools.lru_cache(maxsize=None)
def lpf_reference(n, c, h, w, alpha=2e-5, bias=1.0, bf16=False):
    """fp64: the LRN output l, its 3x3/2 max-pool y and the first-maximum arg-max of the activations of this shape."""
    x = activations(n, h, w, c, bf16)
    l, _ = O.lrn(x, alpha=alpha, bias=bias)
    y, arg = O.max_pool_valid(l)
    return LpfRef(x, *frozen(l, y, arg.astype(np.uint8)))


PlbRef = collections.namedtuple("PlbRef", "x dy arg want")


@functools.lru_cache(maxsize=None)
def plb_reference(n, c, h, w, relu=True, alpha=2e-5, beta=0.75, bias=1.0, bf16=False):
    """fp64: d/dx of max_pool(lrn(x)) for a seeded pooled gradient dy, routed through the fp64 arg-max, (+ ReluGrad)."""
    x = activations(n, h, w, c, bf16)
    l, _ = O.lrn(x, alpha=alpha, beta=beta, bias=bias)
    y, arg = O.max_pool_valid(l)
    dy = gradient(y.shape)
    want = O.lrn_grad(x, O.max_pool_valid_grad(x.shape, arg, dy.astype(np.float64)), alpha=alpha, beta=beta, bias=bias)
    if relu:
        want = want * (x > 0)
    return PlbRef(x, dy, *frozen(arg.astype(np.uint8), want))


LrnRef = collections.namedtuple("LrnRef", "x dy y dx")


@functools.lru_cache(maxsize=None)
def lrn_reference(n, h, w, c, alpha=2e-5, beta=0.75, bias=1.0):
    x = activations(n, h, w, c)
    dy = gradient(x.shape)
    return LrnRef(x, dy, *frozen(O.lrn(x, alpha=alpha, beta=beta, bias=bias)[0], O.lrn_grad(x, dy, alpha=alpha, beta=beta, bias=bias)))


PoolRef = collections.namedtuple("PoolRef", "x y arg dy dx")


@functools.lru_cache(maxsize=4)
def pool_reference(n, c, h, w, k, s):
    """Max-pool of the activations (unscaled ties at 0 are as exact), arg-max, a seeded dy and the routed gradient in fp64."""
    x = activations(n, h, w, c)
    y, arg = max_pool(x, k, s)
    dy = gradient(y.shape)
    return PoolRef(x, *frozen(y, arg.astype(np.uint8), dy, O.max_pool_valid_grad(x.shape, arg, dy.astype(np.float64), k, s)))
