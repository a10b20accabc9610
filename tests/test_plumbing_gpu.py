"""The small kernels that glue multi-input pipelines together and the LSTM dropout (csrc/pointwise.hip), each on its own, past one
workgroup and into its grid-stride loop, bit for bit: vl_copy2d, vl_eltwise2, vl_max2_grad, vl_fuse_n, vl_fuse_n_grad, vl_relu_grad,
vl_fill, vl_dropout_fwd, vl_dropout_fwd_st, vl_dropout_bwd.

Every operation here is a copy, a max, a compare, or one or two correctly rounded fp32 operations in a fixed order (hipcc divides fp32
correctly rounded unless told otherwise, and csrc/build.sh does not tell it), so numpy's float32 arithmetic gives the expected BITS and no
tolerance appears, except in the cross-checks against the oracle that tests/test_composed_gpu.py::test_tensor_list_ops already makes, at its
tolerances (the oracle averages in numpy's own order).  The dropout draw is tests/feed_ref.py's dropout_mask.

Launch branches: all these kernels run grid_for(count, 256, 4096) workgroups of 256 threads, so 1 .. 256 elements are one workgroup, 257
is the second, and from 4096 * 256 = 1 048 576 elements on the loop turns: 1 048 577 gives exactly one thread a second element.

The harness: inputs are views into a NaN-filled allocation, outputs views into a sentinel-filled one, all 1, 2 or 3 floats past a 16-byte
boundary (test_gemm_geometry_gpu's Layout); tensors are TAIL floats longer than the count passed, so the tail as well as the surroundings
must still hold the sentinel.  Every set of calls runs twice into two such allocations that must agree in every bit (compared on the
device); one of them is downloaded, once, and the expected elements are compared as uint32 patterns."""
import numpy as np
import pytest
import torch

from oracle import lrcn_oracle as O
from tests import feed_ref as F
from tests.test_cutmix_gpu import special_words
from tests.test_gemm_geometry_gpu import DEV, SENTINEL, Layout
from tests.test_reductions_gpu import intact, take

pytestmark = pytest.mark.gpu

TAIL = 43
COUNTS = [1, 255, 256, 257, 1_048_577]
SENT_BITS = int(np.float32(SENTINEL).view(np.uint32))
MASK_SENTINEL = 0xA5
ZERO = np.float32(0)


@pytest.fixture(scope="module")
def ops():
    import vltf_amd.ops as ops_
    return ops_


class Pool:
    """Named views of one flat float32 allocation."""

    def __init__(self):
        self.lay, self.items = Layout(), {}

    def add(self, key, floats):
        self.items[key] = (self.lay.place(floats), floats)
        return key

    def host(self, fill):
        return np.full(self.lay.total(), fill, np.float32)

    def put(self, flat, key, values):
        o, c = self.items[key]
        v = np.ascontiguousarray(values).reshape(-1)
        flat[o:o + v.size] = v.view(np.float32)

    def view(self, t, key, floats=None):
        o, c = self.items[key]
        return t[o:o + (c if floats is None else floats)]

    def take(self, got, key, floats=None):
        o, c = self.items[key]
        return take(got, o, c if floats is None else floats).view(np.uint32)


def upload(flat):
    t = torch.from_numpy(flat.view(np.int32)).to(DEV).view(torch.float32)
    assert t.data_ptr() % 16 == 0
    return t


def twice(pool, launch, prefill=None):
    """launch(t) into two sentinel-filled copies of the pool (prefill: host image of in-place operands); the same bits in both;
    -> the first, downloaded."""
    host = pool.host(SENTINEL) if prefill is None else prefill
    ts = [upload(host.copy()) for _ in range(2)]
    for t in ts:
        launch(t)
    assert torch.equal(ts[0].view(torch.int32), ts[1].view(torch.int32)), "two calls, two results"
    return ts[0].cpu().numpy()


def same(got, want, what):
    want = np.ascontiguousarray(want).reshape(-1).view(np.uint32)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError("%s: %d of %d words differ, the first at %d: %#010x, expected %#010x" % (what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]]))


def ulps_against_fp64(got_bits, num, den):
    """Largest distance, in units of the float32 spacing at the exact quotient, between float32 results and num / den in fp64."""
    exact = num.astype(np.float64) / np.float64(den)
    got = got_bits.view(np.float32).astype(np.float64)
    fin = np.isfinite(exact) & (exact != 0)
    return float(np.max(np.abs(got[fin] - exact[fin]) / np.spacing(np.abs(exact[fin]).astype(np.float32)).astype(np.float64), initial=0.0))


def quotient(got, num, den, what):
    """got = float32(num) / float32(den), correctly rounded: numpy's float32 quotient in every bit.  A difference is reported with its
    size against the fp64 quotient."""
    want = (num / np.float32(den)).astype(np.float32)
    if not np.array_equal(got, want.reshape(-1).view(np.uint32)):
        raise AssertionError("%s: fp32 division is not correctly rounded here: up to %.2f ulp from the fp64 quotient"
                             % (what, ulps_against_fp64(got, num.reshape(-1), den)))


# ---- 1. vl_copy2d --------------------------------------------------------------------------------------------------------------------------
COPIES = [(1, 1, 1, 1), (6, 5, 5, 8), (3, 30, 0, 30), (7, 1000, 1003, 1001), (1025, 1030, 1031, 1033)]      # rows, cols, src_ld, dst_ld


def test_copy2d(ops):
    """Row strides above and equal to the width, src_ld = 0 (one row repeated), and 1025 x 1030 > 4096 * 256 elements, where the loop turns.
    NaN payloads, -0.0 and infinities arrive as they left; the dst_ld - cols floats behind every row keep the sentinel."""
    assert COPIES[-1][0] * COPIES[-1][1] > 4096 * 256
    pin, pout = Pool(), Pool()
    for i, (rows, cols, sld, dld) in enumerate(COPIES):
        pin.add(i, (rows - 1) * sld + cols)
        pout.add(i, (rows - 1) * dld + cols)
    src = pin.host(np.nan)
    words = {}
    for i, (rows, cols, sld, dld) in enumerate(COPIES):
        words[i] = special_words((rows - 1) * sld + cols, 3 + i)
        pin.put(src, i, words[i])
    srcd = upload(src)

    def launch(t):
        for i, (rows, cols, sld, dld) in enumerate(COPIES):
            ops.copy2d(pin.view(srcd, i), pout.view(t, i), rows, cols, src_ld=sld, dst_ld=dld)
    got = twice(pout, launch)
    for i, (rows, cols, sld, dld) in enumerate(COPIES):
        want = np.full((rows - 1) * dld + cols, SENT_BITS, np.uint32)
        for r in range(rows):
            want[r * dld:r * dld + cols] = words[i][r * sld:r * sld + cols]
        same(pout.take(got, i), want, "copy2d %s" % (COPIES[i],))
    intact(got, "vl_copy2d")
    # what the kernel is used for: replicate_auxilliary_tensor is a src_ld = 0 copy
    a = words[2].view(np.float32)[:30].reshape(6, 5)
    rep = O.replicate_auxilliary_tensor(a, 3)
    want = np.concatenate([words[2][:30]] * 3)
    assert np.array_equal(rep.reshape(-1).view(np.uint32), want)


# ---- 2. vl_eltwise2 and vl_max2_grad ------------------------------------------------------------------------------------------------------------
def pair(count, seed):
    """Two random normal vectors and a gradient: every fifth element an exact tie, infinities of both signs in either input and in
    both (never opposite ones in one slot: inf - inf is a NaN whose payload is not ours to define); no NaN, no zero."""
    rng = np.random.default_rng(seed)
    a, b, d = (rng.standard_normal(count).astype(np.float32) for _ in range(3))
    i = np.arange(count)
    b[i % 5 == 0] = a[i % 5 == 0]
    for r, (va, vb) in {3: (np.inf, None), 7: (-np.inf, None), 11: (None, np.inf), 13: (None, -np.inf), 17: (np.inf, np.inf),
                        19: (-np.inf, -np.inf)}.items():
        if va is not None:
            a[i % 97 == r] = va
        if vb is not None:
            b[i % 97 == r] = vb
    assert not np.isnan(a + b).any() and (a != 0).all() and (b != 0).all()
    return a, b, d


@pytest.mark.parametrize("count", COUNTS)
def test_eltwise2_and_max2_grad(ops, count):
    a, b, d = pair(count, count)
    if count > 100:
        assert (a == b).any() and np.isinf(a).any() and np.isinf(b).any() and (np.isinf(a) & (a == b)).any()
    pin, pout = Pool(), Pool()
    for k in "abd":
        pin.add(k, count + TAIL)
    for k in ("add", "avg", "maximum", "da", "db"):
        pout.add(k, count + TAIL)
    src = pin.host(np.nan)
    for k, v in zip("abd", (a, b, d)):
        pin.put(src, k, v)
    srcd = upload(src)
    ad, bd, dd = (pin.view(srcd, k) for k in "abd")

    def launch(t):
        for op in ("add", "avg", "maximum"):
            ops.eltwise2(ad, bd, pout.view(t, op), op, count=count)
        ops.max2_grad(ad, bd, dd, pout.view(t, "da"), pout.view(t, "db"), count=count)
    got = twice(pout, launch)
    res = {k: pout.take(got, k, count) for k in ("add", "avg", "maximum", "da", "db")}
    intact(got, "vl_eltwise2 / vl_max2_grad at count %d of %d" % (count, count + TAIL))       # the tails too
    half = np.float32(0.5)
    same(res["add"], a + b, "add")
    same(res["avg"], (a + b) * half, "avg")
    same(res["maximum"], np.maximum(a, b), "maximum")
    same(res["da"], np.where(a > b, d, np.where(a == b, half * d, ZERO)), "max2_grad da")
    same(res["db"], np.where(b > a, d, np.where(a == b, half * d, ZERO)), "max2_grad db")
    # the oracle, as test_tensor_list_ops holds it
    for method in ("avg", "maximum"):
        want, _, _, _, cache = O.tensor_list_fusion([a, b], method, [1, 1], [1, 1], [1, 1])
        np.testing.assert_allclose(res[method].view(np.float32), want, rtol=1e-6)
    wa, wb = O.tensor_list_fusion_grad(cache, d)
    np.testing.assert_array_equal(res["da"].view(np.float32), wa)
    np.testing.assert_array_equal(res["db"].view(np.float32), wb)


# ---- 3. vl_fuse_n and vl_fuse_n_grad -------------------------------------------------------------------------------------------------------------
def fuse_inputs(n, count, seed):
    """n random normal vectors and a gradient.  Planted: 2-, 3- and 8-way ties AT the maximum (as many as n allows), ties below it, +inf
    in one input, +inf in two, -inf in one."""
    rng = np.random.default_rng(seed)
    xs = [rng.standard_normal(count).astype(np.float32) for _ in range(n)]
    d = rng.standard_normal(count).astype(np.float32)
    i = np.arange(count)
    for ways, every in ((2, 7), (3, 11), (8, 13)):
        sel = i % every == 0
        top = (np.maximum.reduce(xs) + np.float32(1))[sel]
        for j in range(min(ways, n)):
            xs[(every + j) % n][sel] = top                                  # not always the leading inputs
    if n >= 2:
        xs[1][i % 17 == 1] = xs[0][i % 17 == 1]                             # a tie wherever it falls
        xs[n - 1][i % 101 == 2] = np.inf
        xs[0][i % 101 == 2] = np.inf
    xs[n // 2][i % 101 == 1] = np.inf
    xs[0][i % 101 == 3] = -np.inf
    return xs, d


def fuse_want(xs, d, method):
    n = len(xs)
    if method == "avg":
        acc = xs[0].copy()
        for x in xs[1:]:
            acc = acc + x                                                   # float32, left to right in list order
        return acc, np.float32(n), [d] * n, [np.float32(n)] * n
    m = np.maximum.reduce(xs)
    hits = sum((x == m).astype(np.int32) for x in xs)
    return m, None, [np.where(x == m, d, ZERO) for x in xs], hits.astype(np.float32)


@pytest.mark.parametrize("count", [257, 1_048_577])
@pytest.mark.parametrize("method", ["avg", "maximum"])
def test_fuse_n_and_its_gradient(ops, method, count):
    """Lists of 1 to 8 tensors.  avg: the float32 sum left to right in list order, divided by float32(n); its gradient d / float32(n),
    once with the inputs given and once with a list of None (the header: ins may be null for the mean).  maximum: the maximum, and
    d / float32(hits) to every input equal to it.  The gradient once into every slot and once with every other slot None, which must
    cost the other slots nothing."""
    hits_seen = set()
    for n in range(1, 9):
        xs, d = fuse_inputs(n, count, 100 * n + count % 100)
        pin, pout = Pool(), Pool()
        for j in range(n):
            pin.add(j, count + TAIL)
        pin.add("d", count + TAIL)
        pout.add("out", count + TAIL)
        for j in range(n):
            pout.add(("all", j), count + TAIL)
            if j % 2 == 0:
                pout.add(("alt", j), count + TAIL)
        src = pin.host(np.nan)
        for j in range(n):
            pin.put(src, j, xs[j])
        pin.put(src, "d", d)
        srcd = upload(src)
        ins, dd = [pin.view(srcd, j) for j in range(n)], pin.view(srcd, "d")

        def launch(t):
            ops.fuse_n(ins, pout.view(t, "out"), method, count=count)
            ops.fuse_n_grad(ins, dd, [pout.view(t, ("all", j)) for j in range(n)], method, count=count)
            ops.fuse_n_grad([None] * n if method == "avg" else ins, dd, [pout.view(t, ("alt", j)) if j % 2 == 0 else None for j in range(n)],
                            method, count=count)
        got = twice(pout, launch)
        out = pout.take(got, "out", count)
        grads = {k: pout.take(got, k, count) for k in pout.items if k != "out"}
        intact(got, "vl_fuse_n / vl_fuse_n_grad, %d inputs" % n)
        what = "%s of %d, count %d" % (method, n, count)
        value, div, num, den = fuse_want(xs, d, method)
        if method == "avg":
            quotient(out, value, div, what)
            for k, g in grads.items():
                quotient(g, d, div, "%s: gradient %s" % (what, k))
        else:
            same(out, value, what)
            hits_seen |= set(np.unique(den).astype(int).tolist())
            for k, g in grads.items():
                want = (num[k[1]] / den).astype(np.float32)
                if not np.array_equal(g, want.view(np.uint32)):
                    raise AssertionError("%s: gradient %s differs from float32(d) / float32(hits): up to %.2f ulp from the fp64 quotient"
                                         % (what, k, ulps_against_fp64(g, num[k[1]], den)))
        if count == 257:                                                    # the oracle, at its own precision
            want, _, _, _, cache = O.tensor_list_fusion(xs, method, [1] * n, [1] * n, [1] * n)
            np.testing.assert_allclose(out.view(np.float32), want, rtol=1e-6)
            for j, w in enumerate(O.tensor_list_fusion_grad(cache, d)):
                np.testing.assert_allclose(grads[("all", j)].view(np.float32), w, rtol=1e-6)
    if method == "maximum":
        assert hits_seen >= {1, 2, 3, 8}, hits_seen


# ---- 4. vl_relu_grad and vl_fill -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 257, 1_048_577])
def test_relu_grad(ops, count):
    """d = y > 0 ? d : 0 in place: +0.0, -0.0, NaN and negatives (-inf too) give +0.0; the smallest positive normal and +inf let d
    through with every bit (NaN payloads, -0.0); the TAIL elements behind `count` keep what they held."""
    rng = np.random.default_rng(count)
    y = rng.standard_normal(count + TAIL).astype(np.float32)
    special = np.array([0x00000000, 0x80000000, 0x00800000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00001, 0x7f800001], np.uint32).view(np.float32)
    y[rng.integers(0, count + TAIL, (count + TAIL) // 2)] = special[rng.integers(0, special.size, (count + TAIL) // 2)]
    y[0] = special[2 if count == 1 else 0]
    d = special_words(count + TAIL, count + 1)
    pin, pout = Pool(), Pool()
    pin.add("y", count + TAIL)
    pout.add("d", count + TAIL)
    src = pin.host(np.nan)
    pin.put(src, "y", y)
    srcd = upload(src)
    start = pout.host(SENTINEL)
    pout.put(start, "d", d)
    got = twice(pout, lambda t: ops.relu_grad(pout.view(t, "d"), pin.view(srcd, "y"), count=count), prefill=start)
    want = d.copy()
    want[:count] = np.where(y[:count] > 0, d[:count], np.uint32(0))
    if count > 1:
        for s in special:
            assert (y[:count].view(np.uint32) == s.view(np.uint32)).any()
        assert (want[:count] == 0).any() and (want[:count] == d[:count]).any()
    same(pout.take(got, "d"), want, "relu_grad, count %d of %d" % (count, count + TAIL))
    intact(got, "vl_relu_grad")


def test_fill(ops):
    value = np.array([0xc2f6e979], np.uint32).view(np.float32)[0]            # -123.456..., no byte repeated
    counts = [1, 257, 1_048_577]
    pout = Pool()
    for c in counts:
        pout.add(c, c)
    got = twice(pout, lambda t: [ops.fill(pout.view(t, c), float(value)) for c in counts])
    for c in counts:
        same(pout.take(got, c), np.full(c, value, np.float32), "fill %d" % c)
    intact(got, "vl_fill")


# ---- 5. the LSTM dropout --------------------------------------------------------------------------------------------------------------------------
SEEDS = [0, 1234, 2 ** 63 + 5, 2 ** 64 - 1]
DROP_COUNTS = [1, 257, 1_048_577]
_X = {}


def normals(count):
    if count not in _X:
        _X[count] = np.random.default_rng(count).standard_normal(count).astype(np.float32)
    return _X[count]


class MaskPool:
    """uint8 views at odd offsets of one allocation filled with MASK_SENTINEL."""

    def __init__(self):
        self.size, self.items = 0, {}

    def add(self, key, count):
        off = (self.size + 16) // 2 * 2 + 1
        self.items[key] = (off, count)
        self.size = off + count

    def alloc(self):
        return torch.full((self.size + 16,), MASK_SENTINEL, dtype=torch.uint8, device=DEV)

    def view(self, t, key):
        o, c = self.items[key]
        return t[o:o + c]

    def take(self, got, key):
        o, c = self.items[key]
        v = got[o:o + c].copy()
        got[o:o + c] = MASK_SENTINEL
        return v


def dropped(x, kept, keep, what, got):
    """got = kept ? x / keep : +0.0, bit for bit."""
    want = np.where(kept, (x / np.float32(keep)).astype(np.float32), ZERO)
    if not np.array_equal(got, want.view(np.uint32)):
        if np.array_equal(got == 0, want.view(np.uint32) == 0):
            raise AssertionError("%s: the kept values are not float32(x) / float32(keep): up to %.2f ulp from the fp64 quotient"
                                 % (what, ulps_against_fp64(got[kept], x[kept], np.float32(keep))))
        same(got, want, what)


@pytest.mark.parametrize("keep", [0.5, 0.9, 1.0])
def test_dropout_fwd_is_the_documented_draw(ops, keep):
    """The mask is dropout_mask(seed, element) in every byte, for seeds that use the top bit and all 64, at one element, in the second
    workgroup and where the loop turns; y = x / keep where kept, else +0.0, x random normal (0.9 is not a power of two: the quotient
    rounds); keep = 1 keeps everything and y has x's bits.  Sentinels behind y and the mask."""
    pin, pout, pm = Pool(), Pool(), MaskPool()
    for c in DROP_COUNTS:
        pin.add(c, c)
        for s in SEEDS:
            pout.add((c, s), c)
            pm.add((c, s), c)
    src = pin.host(np.nan)
    for c in DROP_COUNTS:
        pin.put(src, c, normals(c))
    srcd = upload(src)
    masks = [pm.alloc() for _ in range(2)]

    def launch(t):
        m = masks[1] if launch.calls else masks[0]
        launch.calls += 1
        for c in DROP_COUNTS:
            for s in SEEDS:
                ops.dropout_fwd(pin.view(srcd, c), pout.view(t, (c, s)), pm.view(m, (c, s)), keep, s)
    launch.calls = 0
    got = twice(pout, launch)
    assert torch.equal(masks[0], masks[1]), "two calls, two masks"
    gm = masks[0].cpu().numpy()
    seen = set()
    for c in DROP_COUNTS:
        for s in SEEDS:
            kept = F.dropout_mask(s, c, keep)
            m = pm.take(gm, (c, s))
            assert np.array_equal(m, kept.astype(np.uint8)), "mask, count %d seed %d keep %g: %d bytes differ" % (c, s, keep, (m != kept).sum())
            y = pout.take(got, (c, s))
            dropped(normals(c), kept, keep, "y, count %d seed %d keep %g" % (c, s, keep), y)
            if keep == 1.0:
                assert kept.all() and np.array_equal(y, normals(c).view(np.uint32))
            elif c > 1:
                assert kept.any() and not kept.all()
                seen.add(kept[:257].tobytes())
    assert keep == 1.0 or len(seen) == len(SEEDS)                              # four seeds, four masks
    assert (gm == MASK_SENTINEL).all(), "written outside a mask"
    intact(got, "vl_dropout_fwd")


def test_dropout_element_index_counts_from_the_pointer(ops):
    """Views one float (one byte) into 16-byte aligned buffers get the mask of the aligned call: element e is e from the pointer given."""
    count, keep, seed = 70001, 0.5, 1234
    x = torch.from_numpy(normals(count)).to(DEV)
    xs = torch.zeros(count + 1, device=DEV)
    xs[1:] = x
    y0, y1 = torch.zeros(count, device=DEV), torch.zeros(count + 1, device=DEV)
    m0, m1 = torch.zeros(count, dtype=torch.uint8, device=DEV), torch.zeros(count + 1, dtype=torch.uint8, device=DEV)
    assert all(t.data_ptr() % 16 == 0 for t in (x, xs, y0, y1, m0, m1))
    ops.dropout_fwd(x, y0, m0, keep, seed)
    ops.dropout_fwd(xs[1:], y1[1:], m1[1:], keep, seed)
    assert torch.equal(m0, m1[1:]) and torch.equal(y0.view(torch.int32), y1[1:].view(torch.int32))
    assert np.array_equal(m0.cpu().numpy(), F.dropout_mask(seed, count, keep).astype(np.uint8))
    assert int(m1[0]) == 0 and float(y1[0]) == 0


@pytest.mark.parametrize("step", [0, 1, 2 ** 31, 2 ** 44 + 3])
def test_dropout_fwd_st_forms_its_seed_from_the_step(ops, step):
    """seed = ((step << 20) ^ 0x5DEECE66D) mod 2^64, read from the step state; at 2^44 + 3 the shift wraps.  Against vl_dropout_fwd with
    that seed and against the reference draw."""
    keep = 0.9
    state = ops.step_state(DEV)
    ops.step_state_set_micro(state, 0, step, 0.01, 0)                          # the count the dropout reads = the draw step
    pin, pout, pm = Pool(), Pool(), MaskPool()
    counts = [257, 70001]
    for c in counts:
        pin.add(c, c)
        for k in ("st", "eager"):
            pout.add((c, k), c)
            pm.add((c, k), c)
    src = pin.host(np.nan)
    for c in counts:
        pin.put(src, c, normals(c))
    srcd = upload(src)
    masks = [pm.alloc() for _ in range(2)]

    def launch(t):
        m = masks[1] if launch.calls else masks[0]
        launch.calls += 1
        for c in counts:
            ops.dropout_fwd_st(pin.view(srcd, c), pout.view(t, (c, "st")), pm.view(m, (c, "st")), keep, state)
            ops.dropout_fwd(pin.view(srcd, c), pout.view(t, (c, "eager")), pm.view(m, (c, "eager")), keep, F.st_seed(step))
    launch.calls = 0
    got = twice(pout, launch)
    assert torch.equal(masks[0], masks[1])
    gm = masks[0].cpu().numpy()
    for c in counts:
        kept = F.dropout_mask(F.st_seed(step), c, keep)
        st, eager = pm.take(gm, (c, "st")), pm.take(gm, (c, "eager"))
        assert np.array_equal(st, eager) and np.array_equal(st, kept.astype(np.uint8)), "step %d, count %d" % (step, c)
        yst, yeager = pout.take(got, (c, "st")), pout.take(got, (c, "eager"))
        assert np.array_equal(yst, yeager)
        dropped(normals(c), kept, keep, "step %d, count %d" % (step, c), yst)
    assert (gm == MASK_SENTINEL).all()
    intact(got, "vl_dropout_fwd_st")


@pytest.mark.parametrize("keep", [0.5, 0.9])
def test_dropout_bwd(ops, keep):
    """dx = mask != 0 ? dy / keep : +0.0 for a hand-made mask with bytes other than 0 and 1."""
    pin, pout = Pool(), Pool()
    for c in DROP_COUNTS:
        pin.add(c, c)
        pout.add(c, c)
    src = pin.host(np.nan)
    for c in DROP_COUNTS:
        pin.put(src, c, normals(c))
    srcd = upload(src)
    values = np.array([0, 1, 0, 2, 255, 0, 128, 1, 0, 0, 77], np.uint8)
    hm = {c: values[(np.arange(c) * 7 + c) % values.size] for c in DROP_COUNTS}
    dm = {c: torch.from_numpy(np.concatenate([[9], hm[c]]).astype(np.uint8)).to(DEV)[1:] for c in DROP_COUNTS}      # an odd address
    got = twice(pout, lambda t: [ops.dropout_bwd(pin.view(srcd, c), dm[c], pout.view(t, c), keep) for c in DROP_COUNTS])
    for c in DROP_COUNTS:
        if c > 1:
            assert set(np.unique(hm[c]).tolist()) == set(values.tolist())
        dropped(normals(c), hm[c] != 0, keep, "dropout_bwd, count %d keep %g" % (c, keep), pout.take(got, c))
    intact(got, "vl_dropout_bwd")
