"""vl_gemm OUTSIDE the workload's shapes and with hostile surroundings: both tile heights at their edges, the 16-element
reduction tile at its edges, every loader pairing, fp32 split-K with an empty trailing split, a capped and a refused workspace, both
slab reductions, and the split-image path at the edges of its gate.  The cases, their inputs and the restated dispatch arithmetic are in
tests/gemm_plan.py; tests/test_gemm_geometry.py (CPU) shows that the lists reach those branches and that the cases discriminate.

The reference everywhere is the fp64 product of the same fp32 inputs, the tolerance test_ops_gpu's `close` (DESIGN 2's per-op bound)
for fp32, bf16x3 and bf16x6; plain bf16 keeps the band of test_gemm_split_products.  Every bitwise claim is exact equality.

The harness (run): every operand, bias, mask and output is a view into one allocation per test, 1, 2 or 3 floats past a 16-byte
boundary, leading dimensions larger than the rows.  Around the inputs the allocation is NaN -- a loader that reads past k, m or n and
counts on a zero to hide it poisons its sum -- around the outputs a finite sentinel that must still be there afterwards.  The workspace
is NaN before every call (a slab or an image element that is read without having been written shows) and is followed by a sentinel
guard; a call that must not split leaves it all NaN.  Every call runs twice into two outputs that must agree bit for bit.  One upload
and one download per test."""
import numpy as np
import pytest
import torch

from tests import gemm_plan as P
from tests.test_ops_gpu import close

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 12345.0
GUARD = 4096                                                   # floats behind the workspace
TRANSPOSES = [(False, False), (True, False), (False, True), (True, True)]


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


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


class Layout:
    """Offsets of views in one flat allocation: each begins 1, 2 or 3 floats past a 16-byte boundary, at least 8 floats behind the
    one before, and 8 floats remain behind the last."""

    def __init__(self):
        self.size = self.count = 0

    def place(self, floats):
        self.count += 1
        off = (self.size + 8 + 3) // 4 * 4 + 1 + self.count % 3
        self.size = off + floats
        return off

    def total(self):
        return self.size + 8


def window(flat, off, rows, width, ld):
    return flat[off:off + rows * ld].reshape(rows, ld)[:, :width]


def run(ops, jobs, math="f32", dev=DEV, ncus=None):
    """jobs: [(case, transa, transb)].  Runs each plain and with bias + ReLU + mask, twice each, and checks everything that does not
    depend on the arithmetic.  Returns [(case, plan, plain, fused, label)]: the m x n windows of the first plain and the first fused call.
    dev, ncus: tests/test_gemm_geometry.py runs the harness itself on the CPU against a stand-in with known defects."""
    ncus = ncus or cus()
    lay_in, lay_out, recs = Layout(), Layout(), []
    for i, (case, ta, tb) in enumerate(jobs):
        m, n, k, _ = case
        ra, wa = (k, m) if ta else (m, k)
        rb, wb = (n, k) if tb else (k, n)
        lda, ldb, ldc = wa + 1 + i % 4, wb + 2 + i % 3, n + 1 + i % 5
        recs.append(dict(case=case, ta=ta, tb=tb, lda=lda, ldb=ldb, ldc=ldc, a=lay_in.place(ra * lda), b=lay_in.place(rb * ldb),
                         bias=lay_in.place(n), mask=lay_in.place(m * ldc), c=[lay_out.place(m * ldc) for _ in range(4)]))
    src = np.full(lay_in.total(), np.nan, np.float32)
    for r in recs:
        m, n, k, _ = r["case"]
        a, b, bias, mask = P.operands(m, n, k)
        at, bt = (a.T if r["ta"] else a), (b.T if r["tb"] else b)
        window(src, r["a"], at.shape[0], at.shape[1], r["lda"])[...] = at
        window(src, r["b"], bt.shape[0], bt.shape[1], r["ldb"])[...] = bt
        src[r["bias"]:r["bias"] + n] = bias
        window(src, r["mask"], m, n, r["ldc"])[...] = mask      # indexed with ldc, as the kernel does
    pool = torch.tensor(src, device=dev)
    out = torch.full((lay_out.total(),), SENTINEL, device=dev)
    nws = {c: P.ws_floats(c, ncus) for c, _, _ in jobs}
    wsbuf = torch.empty(max(nws.values()) + GUARD, device=dev)
    assert pool.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0 and wsbuf.data_ptr() % 16 == 0
    flags, labels = [], []
    for r in recs:
        case, w = r["case"], nws[r["case"]]
        m, n, k, _ = case
        if case.ws.startswith("image"):                        # the library's own figure, which the restatement must match
            assert ops.gemm_split_ws_bytes(m, n, k) == P.gemm_split_ws_bytes(m, n, k, ncus)
        r["plan"] = plan = P.plan_of(case, ncus, math)
        ws, guard = (wsbuf[:w] if w else None), wsbuf[w:w + GUARD]
        for i, fused in enumerate((False, False, True, True)):
            guard.fill_(SENTINEL)
            if w:
                ws.fill_(float("nan"))
            ops.gemm(pool[r["a"]:], pool[r["b"]:], out[r["c"][i]:], m, n, k, transa=r["ta"], transb=r["tb"], lda=r["lda"], ldb=r["ldb"],
                     ldc=r["ldc"], bias=pool[r["bias"]:] if fused else None, relu=fused, relu_mask=pool[r["mask"]:] if fused else None, ws=ws)
            flags.append((guard != SENTINEL).any())
            labels.append("%s ta=%d tb=%d call %d: guard behind the workspace written" % (P.case_id(case), r["ta"], r["tb"], i))
            if w and plan.path == "f32" and plan.splits == 1:
                flags.append((ws == ws).any())                  # anything but NaN
                labels.append("%s ta=%d tb=%d call %d: unsplit, yet the workspace was written" % (P.case_id(case), r["ta"], r["tb"], i))
    bad = torch.stack(flags).cpu().numpy()
    got = out.cpu().numpy()
    assert not bad.any(), [l for l, f in zip(labels, bad) if f]
    res = []
    for r in recs:
        m, n, k, _ = r["case"]
        what = "%s ta=%d tb=%d" % (P.case_id(r["case"]), r["ta"], r["tb"])
        wins = [window(got, off, m, n, r["ldc"]).copy() for off in r["c"]]
        for off in r["c"]:
            window(got, off, m, n, r["ldc"])[...] = SENTINEL
        assert all(np.isfinite(w).all() for w in wins), what + ": non-finite output (padding or stale workspace read)"
        assert wins[0].tobytes() == wins[1].tobytes() and wins[2].tobytes() == wins[3].tobytes(), what + ": two calls, two results"
        res.append((r["case"], r["plan"], wins[0], wins[2], what))
    assert np.array_equal(got.view(np.uint32), np.full(got.shape, SENTINEL, np.float32).view(np.uint32)), "output written outside an m x n window"
    return res


def rel_l2(got, want):
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


def check(res, bf16_band=False, fp32=False):
    """close for plain and fused; bf16_band: the image path in plain bf16 (1e-4 < relative L2 < 1e-2, fused < 1e-2); fp32: < 2e-5 too."""
    for case, plan, plain, fused, what in res:
        want = P.reference(*case[:3])
        wantf = P.epilogue(want, *case[:3])
        err = rel_l2(plain, want)
        if bf16_band:
            assert plan.path == "image" and 1e-4 < err < 1e-2, (what, err)
            assert rel_l2(fused, wantf) < 1e-2, what
        else:
            close(plain, want, msg=what)
            close(fused, wantf, msg=what + " bias + ReLU + mask")
            if fp32:
                assert err < 2e-5, (what, err)


# ---- 1. tile edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ta,tb", TRANSPOSES)
def test_tile_edges(ops, ta, tb):
    """<64,1,4> up to m = 64 and <128,2,2> beyond, n around one and two 128-column tiles, k around one and two 16-element reduction
    tiles (DenseXK's masked last tile, DenseKX's shortened last resource), no workspace: all m x n at k = 17 and 100, all k at three
    (m, n).  With NaN behind every row and every operand, an over-read is a NaN in the window."""
    res = run(ops, [(c, ta, tb) for c in P.TILE_EDGES])
    assert {p.bm for _, p, _, _, _ in res} == {64, 128} and all(p.splits == 1 for _, p, _, _, _ in res)
    check(res)


# ---- 2. fp32 split-K ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ta,tb", TRANSPOSES)
def test_split_k_with_the_workspace_as_given(ops, ta, tb):
    """The empty 18th split on both tile heights (its slab must be stored as zeros: the workspace was NaN), 16 and 17 splits through
    the four-way reduction, three splits because the workspace holds three slabs (one-way reduction), no split because it holds
    less than one or because k < 256 -- the workspace still all NaN afterwards."""
    res = run(ops, [(c, ta, tb) for c in P.SPLIT_K])
    plans = {c: p for c, p, _, _, _ in res}
    assert all(plans[c].splits == 18 and plans[c].empty == 1 for c in P.EMPTY_SPLIT)
    assert [(plans[c].splits, plans[c].ways) for c in P.FOUR_WAY] == [(16, 4), (17, 4)]
    assert all((plans[c].splits, plans[c].ways) == (3, 1) for c in P.CAPPED) and all(plans[c].splits == 1 for c in P.UNSPLIT)
    check(res)


# ---- 3. the split-image path ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conv_math", ["bf16x3", "bf16x6", "bf16"], indirect=True)
def test_split_image_path(ops, conv_math):
    """gemm_split_image_kernel + gemm_split_kernel with exactly the workspace vl_gemm_split_ws_bytes asks for: m, n, k of exactly 128,
    one above, a single partial 256-column tile (n = 200, 255), a ninth stage of one element (k = 129), split-K of 2, 7 and 8 --
    every transpose pair, i.e. both branches of the image kernel (k contiguous, rows contiguous) for both operands.  (130, 300, 200)
    with the exact byte count: the gate opens (in bf16 the band says so) and the guard behind the workspace stays."""
    res = run(ops, [(c, ta, tb) for c in P.IMAGE + P.GATE_OPEN for ta, tb in TRANSPOSES], conv_math)
    assert all(p.path == "image" for _, p, _, _, _ in res) and {p.splits for _, p, _, _, _ in res} >= {1, 2, 7, 8}
    check(res, bf16_band=conv_math == "bf16")


@pytest.mark.parametrize("conv_math", ["bf16x3", "bf16x6", "bf16"], indirect=True)
def test_split_image_gate_refuses(ops, conv_math):
    """One of m, n, k at 127, a workspace one float short, no workspace: fp32 arithmetic (relative L2 < 2e-5; in bf16 mode the image
    path would sit at ~3e-3), and the short workspace untouched."""
    res = run(ops, [(c, ta, tb) for c in P.GATE_SHAPE + P.GATE_WS for ta, tb in TRANSPOSES], conv_math)
    assert all(p.path == "f32" for _, p, _, _, _ in res)
    check(res, fp32=True)
