"""vl_pack_kc8 + vl_gemm_kc8 (wgrad_c8_kernel<4,2,2> on reduction-major operands) on every launch branch and with hostile
surroundings: the direct and the reduced form, every split shape of gemm_kc8_plan, the three fetch branches of a stage, the three-slot
pipeline at 1, 2, 3 and 4+ stages, partial tiles on both sides, both passes of the slab sum, both thread orders of the pack.  The cases,
their inputs, the references and the restated launch arithmetic are in tests/kc8_plan.py; tests/test_kc8_geometry.py (CPU) shows that the
lists reach those branches, that the cases discriminate and that this harness notices what it is there to notice.

References: the fp64 product of the bf16-exact operands (+ bias) (ReLU).  Integer inputs must come out EQUAL (every partial sum is an
integer below 2^24: fp32 accumulation is exact in any order); Gaussian inputs within test_conv_c8_gpu.close (rtol = atol_rel = 3e-5,
the packed path's bound).  The pack is compared bit for bit with torch's CPU rounding.

The harness (run): ONE allocation per test.  Its bf16 part holds the kc8 operands as 16-byte-aligned views, NaN in between -- a fetch
past k, past the last 8-row block or past the operand poisons its sum.  Its fp32 part holds the outputs, each 1, 2 or 3 floats past a
16-byte boundary, NaN inside (an element the kernel does not store stays non-finite) and a finite sentinel around, and the biases.  The
workspace is exactly vl_gemm_kc8_ws_bytes long -- asserted equal to the restated plan -- NaN before every call (a slab element read
without having been written shows), with a sentinel guard behind it; a direct call leaves it all NaN and runs a second time without
one.  Every call runs twice into two outputs that must agree bit for bit.  One upload and one download per test."""
import numpy as np
import pytest
import torch

from tests import kc8_plan as P
from tests.test_conv_c8_gpu import close

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 12345.0
SENTINEL_BF16 = 0x4640                                          # 12288 in bf16
NAN_BF16 = 0x7FC0
GUARD = 4096                                                    # floats behind the workspace
RTOL = ATOL_REL = 3e-5
WORST = {}                                                      # test -> worst error / bound seen in this process


@pytest.fixture(scope="module")
def ops():
    import vltf_amd.ops as ops_
    yield ops_
    print("\nkc8 geometry, worst error / bound:", " ".join("%s %.3f" % kv for kv in sorted(WORST.items())))


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- the comparison -----------------------------------------------------------------------------------------------------------------
def agree(kind, got, want, what, tag=None):
    """"int": exact equality; "gauss": close() at the path's bound, the worst error / bound kept in WORST[tag]."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    if kind == "int":
        bad = np.argwhere(got != want)
        assert not len(bad), "%s: %d of %d elements differ from the exact result, first at %s: %r != %r" % (
            what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
        return
    scale = float(np.abs(want).max()) or 1.0
    ratio = float((np.abs(got - want) / (ATOL_REL * scale + RTOL * np.abs(want))).max())
    if tag is not None:
        WORST[tag] = max(WORST.get(tag, 0.0), ratio)
    close(got, want, rtol=RTOL, atol_rel=ATOL_REL, msg="%s (worst error / bound %.3g)" % (what, ratio))


# ---- the allocation -----------------------------------------------------------------------------------------------------------------
class Arena:
    """One host image, uploaded once: bf16 views at multiples of 8 elements (16 bytes), at least 8 NaN elements apart; behind them
    fp32 views 1, 2 or 3 floats past a 16-byte boundary, at least 8 sentinel floats apart."""

    def __init__(self, bf16_fill=NAN_BF16):
        self.bf16_fill, self.h, self.f, self.nh, self.nf, self.count = bf16_fill, [], [], 8, 8, 0

    def bf16(self, bits):
        """bits: uint16 image of the view, or a length to leave at the fill."""
        n = bits if isinstance(bits, int) else bits.size
        off = (self.nh + 7) // 8 * 8
        self.nh = off + n + 8
        if not isinstance(bits, int):
            self.h.append((off, np.ascontiguousarray(bits, np.uint16).reshape(-1)))
        return off

    def f32(self, values):
        """values: float32 image of the view (inputs), or a length to fill with NaN (outputs)."""
        n = values if isinstance(values, int) else values.size
        self.count += 1
        off = (self.nf + 8 + 3) // 4 * 4 + 1 + self.count % 3
        self.nf = off + n
        self.f.append((off, np.full(n, np.nan, np.float32) if isinstance(values, int) else np.ascontiguousarray(values, np.float32).reshape(-1)))
        return off

    def upload(self, dev):
        """-> (bf16 view, fp32 view) of one device allocation; keeps the host image."""
        words = (self.nh + 8 + 7) // 8 * 4                       # fp32 words under the bf16 part: a multiple of 4, so 16-byte aligned
        host = np.full(words + self.nf + 8, SENTINEL, np.float32)
        half = host[:words].view(np.uint16)
        half[:] = self.bf16_fill
        for off, bits in self.h:
            half[off:off + bits.size] = bits
        for off, vals in self.f:
            host[words + off:words + off + vals.size].view(np.uint32)[:] = vals.view(np.uint32)
        self.host, self.words = host, words
        self.flat = torch.from_numpy(host.copy()).to(dev)
        assert self.flat.data_ptr() % 16 == 0
        return self.flat[:words].view(torch.bfloat16), self.flat[words:]

    def download(self):
        """-> (uint16 image of the bf16 part, fp32 part) as they are now."""
        got = self.flat.cpu().numpy()
        return got[:self.words].view(np.uint16), got[self.words:]

    def expected(self):
        return self.host[:self.words].view(np.uint16), self.host[self.words:]


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32 if a.dtype == np.float32 else a.dtype), b.view(np.uint32 if b.dtype == np.float32 else b.dtype))


def settle(arena, outputs, packed=(), what="output"):
    """After the calls: download once, cut the output windows out (fp32 `outputs`, bf16 `packed`: [(offset, length)]) and require
    everything else -- operands, biases, sentinels, NaN padding -- to be bit for bit what was uploaded.  -> ([fp32 window], [bf16 window])."""
    half, flt = arena.download()
    half0, flt0 = arena.expected()
    wins, halves = [], []
    for off, n in outputs:
        wins.append(flt[off:off + n].copy())
        flt[off:off + n].view(np.uint32)[:] = flt0[off:off + n].view(np.uint32)
    for off, n in packed:
        halves.append(half[off:off + n].copy())
        half[off:off + n] = half0[off:off + n]
    assert same_bits(flt, flt0), what + " written outside its window"
    assert np.array_equal(half, half0), "an operand was written, or a pack wrote outside its destination"
    return wins, halves


# ---- the GEMM harness ---------------------------------------------------------------------------------------------------------------
def run(ops, jobs, kind, dev=DEV, ncus=None):
    """jobs: [Case].  Runs each twice and checks everything that does not depend on the arithmetic.  -> [(case, plan, c [m][n], label)].
    dev, ncus: tests/test_kc8_geometry.py runs the harness itself on the CPU against a stand-in with known defects."""
    ncus = ncus or cus()
    arena, recs = Arena(), []
    for case in jobs:
        m, n, k = case[:3]
        a, b, bias = P.operands(m, n, k, kind)
        recs.append(dict(case=case, plan=P.plan_of(case, ncus), a=arena.bf16(P.to_kc8(a)), b=arena.bf16(P.to_kc8(b)),
                         bias=arena.f32(bias) if case.bias else None, c=[arena.f32(m * n) for _ in range(2)]))
    half, flt = arena.upload(dev)
    wsbuf = torch.empty(max(r["plan"].ws_bytes for r in recs) // 4 + GUARD, device=dev)
    assert wsbuf.data_ptr() % 16 == 0
    flags, labels = [], []
    for r in recs:
        case, plan = r["case"], r["plan"]
        m, n, k = case[:3]
        what = P.case_id(case)
        assert ops.gemm_kc8_ws_bytes(m, n, k) == plan.ws_bytes, "%s: vl_gemm_kc8_ws_bytes is not what the restated plan says" % what
        w = plan.ws_bytes // 4
        ws, guard = wsbuf[:w], wsbuf[w:w + GUARD]
        av = half[r["a"]:r["a"] + m * k].view(ops.kc8_shape(k, m))
        bv = half[r["b"]:r["b"] + n * k].view(ops.kc8_shape(k, n))
        assert av.data_ptr() % 16 == 0 and bv.data_ptr() % 16 == 0
        for i, off in enumerate(r["c"]):
            assert flt[off:].data_ptr() % 16 in (4, 8, 12)
            guard.fill_(SENTINEL)
            ws.fill_(float("nan"))
            ops.gemm_kc8(av, bv, flt[off:], m, n, k, bias=flt[r["bias"]:r["bias"] + n] if case.bias else None, relu=case.relu,
                         ws=None if plan.direct and i == 1 else ws)      # a direct call needs no workspace: the second goes without
            flags.append((guard != SENTINEL).any())
            labels.append("%s call %d: guard behind the workspace written" % (what, i))
            if plan.direct:
                flags.append((ws == ws).any())                   # anything but NaN
                labels.append("%s call %d: direct, yet the workspace was written" % (what, i))
    bad = torch.stack(flags).cpu().numpy()
    wins, _ = settle(arena, [(off, r["case"].m * r["case"].n) for r in recs for off in r["c"]])
    assert not bad.any(), [l for l, f in zip(labels, bad) if f]
    res = []
    for i, r in enumerate(recs):
        what = "%s (%s)" % (P.branch(r["case"], ncus), kind)
        c0, c1 = wins[2 * i], wins[2 * i + 1]
        assert np.isfinite(c0).all() and np.isfinite(c1).all(), what + ": non-finite output (an element not stored, padding or stale workspace read)"
        assert c0.tobytes() == c1.tobytes(), what + ": two calls, two results"
        res.append((r["case"], r["plan"], c0.reshape(r["case"].m, r["case"].n), what))
    return res


def check(res, kind, tag=None):
    for case, _, got, what in res:
        agree(kind, got, P.want_of(case, kind), what, tag)


# ---- 1. the GEMM cases --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("name", ["DIRECT", "REDUCED", "SPLIT", "MANY_TILES"])
def test_gemm_cases(ops, name, kind):
    """Every case of a list, integer inputs (exact) and Gaussian inputs (the path's bound), through the harness."""
    res = run(ops, P.cases(cus())[name], kind)
    direct = {p.direct for _, p, _, _ in res}
    assert direct == ({True} if name in ("DIRECT", "MANY_TILES") else {False})
    check(res, kind, name)


def test_lists_reach_their_branches_on_this_device(ops):
    from tests.test_kc8_geometry import assert_coverage
    assert_coverage(cus())


# ---- 2. the products as the engine packs them ---------------------------------------------------------------------------------------
def run_engine(ops, frames, kind, dev=DEV, ncus=None):
    """The six products of engine_products(frames) from fp32 matrices through pack_kc8 and gemm_kc8, and the fc6 weight gradient of the
    row-block shape in one call and block by block.  -> ([(product, c)], whole, blockwise)."""
    ncus = ncus or cus()
    mats = P.engine_matrices(frames, kind)
    arena = Arena()
    src = {name: arena.f32(m) for name, m in mats.items()}
    prods = P.engine_products(frames)
    pk = {}
    for pr in prods:
        for opnd in (pr.a, pr.b):
            pk.setdefault(opnd, arena.bf16(P.ceil_div(opnd[2], 8) * 8 * opnd[1]))
    outs = [arena.f32(pr.m * pr.n) for pr in prods]
    # the row-block form: x [frames][384], d [frames][128] -> dW [384][128]
    M, N = P.ROW_BLOCK_M, P.ROW_BLOCK_N
    xa, xb, _ = P.operands(M, N, frames, kind)                   # [frames][M], [frames][N]
    rb_src = (arena.f32(xa), arena.f32(xb))
    rb_pk = (arena.bf16(M * frames), arena.bf16(N * frames))
    rb_out = (arena.f32(M * N), arena.f32(M * N))
    half, flt = arena.upload(dev)
    shapes = [(pr.m, pr.n, pr.k) for pr in prods] + [(M, N, frames)] + [(r1 - r0, N, frames) for r0, r1 in P.ROW_BLOCKS]
    wsbuf = torch.empty(max(P.plan(*s, ncus).ws_bytes for s in shapes) // 4 + GUARD, device=dev)
    flags = []

    def view(off, positions, channels):
        return half[off:off + P.ceil_div(channels, 8) * 8 * positions].view(ops.kc8_shape(positions, channels))

    def gemm(a, b, c, m, n, k, bias=None, relu=False):
        w = P.plan(m, n, k, ncus).ws_bytes // 4
        assert ops.gemm_kc8_ws_bytes(m, n, k) == 4 * w
        wsbuf[:w].fill_(float("nan"))
        wsbuf[w:w + GUARD].fill_(SENTINEL)
        ops.gemm_kc8(a, b, c, m, n, k, bias=bias, relu=relu, ws=wsbuf[:w])
        flags.append((wsbuf[w:w + GUARD] != SENTINEL).any())

    for name, pos, ch, ps, cs in pk:
        ops.pack_kc8(flt[src[name]:src[name] + mats[name].size], view(pk[(name, pos, ch, ps, cs)], pos, ch), pos, ch, ps, cs)
    for pr, out in zip(prods, outs):
        bias = flt[src[pr.bias]:src[pr.bias] + pr.n] if pr.bias else None
        gemm(view(pk[pr.a], pr.k, pr.m), view(pk[pr.b], pr.k, pr.n), flt[out:], pr.m, pr.n, pr.k, bias, pr.relu)
    a, b = view(rb_pk[0], frames, M), view(rb_pk[1], frames, N)
    ops.pack_kc8(flt[rb_src[0]:rb_src[0] + xa.size], a, frames, M, M, 1)
    ops.pack_kc8(flt[rb_src[1]:rb_src[1] + xb.size], b, frames, N, N, 1)
    gemm(a, b, flt[rb_out[0]:], M, N, frames)
    for r0, r1 in P.ROW_BLOCKS:
        gemm(a[r0 // 8:r1 // 8], b, flt[rb_out[1] + r0 * N:], r1 - r0, N, frames)
    bad = torch.stack(flags).cpu().numpy()
    packed = [(o, P.ceil_div(key[2], 8) * 8 * key[1]) for key, o in pk.items()] + [(rb_pk[0], M * frames), (rb_pk[1], N * frames)]
    wins, _ = settle(arena, [(o, pr.m * pr.n) for pr, o in zip(prods, outs)] + [(o, M * N) for o in rb_out], packed)
    assert not bad.any(), "guard behind the workspace written"
    assert all(np.isfinite(w).all() for w in wins), "non-finite output"
    got = [(pr, w.reshape(pr.m, pr.n)) for pr, w in zip(prods, wins)]
    return got, wins[-2].reshape(M, N), wins[-1].reshape(M, N)


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("frames", P.ENGINE_FRAMES)
def test_engine_products(ops, frames, kind):
    """fc6's and the first LSTM layer's three products each, operands packed with the engine's own strides (six orientations), the two
    weight gradients with k = frames (the per-lane fetch); the DP row-block loop (a direct block and a reduced one) must give what the
    one-call form gives."""
    ncus = cus()
    plans = [P.plan(r1 - r0, P.ROW_BLOCK_N, frames, ncus) for r0, r1 in P.ROW_BLOCKS]
    assert [p.direct for p in plans] == [True, False]
    got, whole, blockwise = run_engine(ops, frames, kind)
    mats = P.engine_matrices(frames, kind)
    for pr, c in got:
        agree(kind, c, P.engine_want(pr, mats), "%s at %d frames (%s)" % (pr.name, frames, kind), "ENGINE")
    want = P.reference(P.ROW_BLOCK_M, P.ROW_BLOCK_N, frames, kind)
    agree(kind, whole, want, "row-block shape in one call at %d frames (%s)" % (frames, kind), "ENGINE")
    agree(kind, blockwise, want, "row-block shape block by block at %d frames (%s)" % (frames, kind), "ENGINE")
    agree(kind, blockwise, whole, "row-block shape, block by block against one call, at %d frames (%s)" % (frames, kind))
    if kind == "int":
        assert whole.tobytes() == blockwise.tobytes()


# ---- 3. the pack --------------------------------------------------------------------------------------------------------------------
def run_pack(ops, jobs, dev=DEV):
    """Each case packed into a destination with a bf16 sentinel before, behind and all through it.  -> [(case, image [CB][P][8])]."""
    arena = Arena(bf16_fill=SENTINEL_BF16)
    recs = []
    for case in jobs:
        _, src = P.pack_source(case)
        recs.append((case, arena.f32(src), arena.bf16(P.ceil_div(case.C, 8) * 8 * case.P)))
    half, flt = arena.upload(dev)
    for case, s, d in recs:
        dst = half[d:d + P.ceil_div(case.C, 8) * 8 * case.P].view(ops.kc8_shape(case.P, case.C))
        assert dst.data_ptr() % 16 == 0
        ops.pack_kc8(flt[s:s + P.pack_src_len(case)], dst, case.P, case.C, case.ps, case.cs)
    _, halves = settle(arena, [], [(d, P.ceil_div(case.C, 8) * 8 * case.P) for case, _, d in recs], what="the source was")
    return [(case, h.reshape(-1, case.P, 8)) for (case, _, _), h in zip(recs, halves)]


def check_pack(res):
    for case, got in res:
        mat, _ = P.pack_source(case)
        want = P.to_kc8(mat)
        nan = (want & 0x7FFF) > 0x7F80
        what = "%s (%s order, %d threads)" % (P.pack_id(case), P.pack_order(case.cs), P.pack_threads(case.P, case.C, case.cs))
        assert got.shape == want.shape, what
        assert np.array_equal((got & 0x7FFF) > 0x7F80, nan), what + ": NaN in other places than the reference"
        bad = np.argwhere((got != want) & ~nan)
        assert not len(bad), "%s: %d elements differ, first at [block, position, lane] %s: %#06x != %#06x" % (
            what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("name", ["PACK_ROWS", "PACK_TRANSPOSE", "PACK_STRIDED"])
def test_pack_cases(ops, name):
    """Both thread orders, every P % 4 (the break of the four-positions-per-thread order), channels around one and two blocks (+0 in the
    pad channels), thread counts that are and are not multiples of 256, sources with both strides above 1; ties, overflow to inf,
    zeros of both signs, infinities and NaN among the values.  The WHOLE destination bit for bit, sentinels around it."""
    check_pack(run_pack(ops, getattr(P, name)))


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------
def test_a_workspace_one_float_short_is_refused_and_c_untouched(ops):
    from vltf_amd._ffi import VltfError
    case = P.SPLIT[0]
    m, n, k = case[:3]
    a, b, _ = P.operands(m, n, k, "int")
    arena = Arena()
    oa, ob, oc = arena.bf16(P.to_kc8(a)), arena.bf16(P.to_kc8(b)), arena.f32(m * n)
    half, flt = arena.upload(DEV)
    w = ops.gemm_kc8_ws_bytes(m, n, k) // 4
    ws = torch.full((w + GUARD,), SENTINEL, device=DEV)
    with pytest.raises(VltfError, match="workspace too small"):
        ops.gemm_kc8(half[oa:oa + m * k].view(ops.kc8_shape(k, m)), half[ob:ob + n * k].view(ops.kc8_shape(k, n)), flt[oc:], m, n, k, ws=ws[:w - 1])
    with pytest.raises(VltfError, match="workspace too small"):
        ops.gemm_kc8(half[oa:oa + m * k].view(ops.kc8_shape(k, m)), half[ob:ob + n * k].view(ops.kc8_shape(k, n)), flt[oc:], m, n, k, ws=None)
    torch.cuda.synchronize()
    assert bool((ws == SENTINEL).all()), "a refused call wrote the workspace"
    half_now, flt_now = arena.download()
    half0, flt0 = arena.expected()
    assert same_bits(flt_now, flt0) and np.array_equal(half_now, half0), "a refused call wrote c"
