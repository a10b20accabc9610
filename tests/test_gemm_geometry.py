"""The CPU half of tests/test_gemm_geometry_gpu.py and tests/test_reductions_gpu.py (no GPU needed): the restated dispatch arithmetic of
tests/gemm_plan.py reaches every branch the case lists are there for, at 256 and at 64 compute units, and the cases discriminate -- a
product that lost its last reduction element, its last row, its last column or the last non-empty split misses `close`
(tests/test_ops_gpu.py, the tolerance the GPU half applies) on the very inputs the GPU half uploads.  Last, the GPU harness itself runs
here against a CPU stand-in: correct, it passes; with an over-read, an unstored slab or a stray write, it says so."""
import numpy as np
import pytest

from tests import gemm_plan as P
from tests.test_ops_gpu import close

CUS = (256, 64)


# ---- coverage -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cus", CUS)
def test_tile_edges_take_both_tile_heights_and_never_split(cus):
    plans = {c: P.plan_of(c, cus) for c in P.TILE_EDGES}
    assert all(p.path == "f32" and p.splits == 1 and p.empty == 0 and p.ways == 0 for p in plans.values())
    assert {c.m for c, p in plans.items() if p.bm == 64} == {1, 63, 64} and {c.m for c, p in plans.items() if p.bm == 128} == {65, 127, 128, 129, 257}
    assert {(c.m, c.n) for c in P.TILE_EDGES if c.k in (17, 100)} == {(m, n) for m in P.EDGE_M for n in P.EDGE_N}
    for mn in ((1, 1), (65, 129), (129, 257)):
        assert {c.k for c in P.TILE_EDGES if (c.m, c.n) == mn} == set(P.EDGE_K)
    # the masked last tile of DenseXK / the shortened last resource of DenseKX: k that is no multiple of 16, below and above one tile
    assert {c.k % P.BR for c in P.TILE_EDGES} >= {0, 1, 2, 15} and {P.ceil_div(c.k, P.BR) for c in P.TILE_EDGES} >= {1, 2, 3, 7}


@pytest.mark.parametrize("cus", CUS)
def test_split_k_cases_reach_their_branches(cus):
    for c in P.EMPTY_SPLIT:                                     # 289 tiles, 18 splits of 17: the 18th is empty; both tile heights
        assert P.plan_of(c, cus)[1:] == (64 if c.m <= 64 else 128, 18, 17, 1, 4)
    assert {P.plan_of(c, cus).bm for c in P.EMPTY_SPLIT} == {64, 128}
    assert len(P.split_ranges(*P.EMPTY_SPLIT[0][:3], P.plan_of(P.EMPTY_SPLIT[0], cus))) == 17
    p16, p17 = (P.plan_of(c, cus) for c in P.FOUR_WAY)
    assert (p16.splits, p16.per, p16.empty, p16.ways) == (16, 16, 0, 4)
    assert (p17.splits, p17.per, p17.empty, p17.ways) == (17, 17, 0, 4) and p17.splits % 4 != 0     # the last of 17 splits holds 3 of 275 tiles
    assert P.split_ranges(8, 1024, 4400, p17)[-1] == (16 * 17 * 16, 4400)
    for c in P.CAPPED:                                          # wanted 8 (k / 256), the workspace holds 3: one-way reduction
        assert P.plan_of(c, cus)[1:] == (64 if c.m <= 64 else 128, 3, 43, 0, 1)
        assert P.gemm_plan(c.m, c.n, c.k, 4 * 32 * c.m * c.n, cus).splits == 8
    for c in P.UNSPLIT:                                         # splits == 1 WITH a workspace: capped to nothing, and k < 256
        assert P.plan_of(c, cus)[1:] == (128, 1, P.ceil_div(c.k, 16), 0, 0) and P.ws_floats(c, cus) > 0
    assert P.gemm_plan(70, 200, 2048, 4 * 70 * 200, cus).splits == 1 and P.gemm_plan(70, 200, 2048, 8 * 70 * 200, cus).splits == 2


@pytest.mark.parametrize("math", ["bf16x3", "bf16x6", "bf16"])
@pytest.mark.parametrize("cus", CUS)
def test_image_cases_and_the_gate(cus, math):
    plans = [P.plan_of(c, cus, math) for c in P.IMAGE]
    assert all(p.path == "image" and p.empty == 0 for p in plans)
    assert [p.splits for p in plans][:4] == [1, 1, 1, 2] and plans[4].splits == 7 and plans[5].splits == 8     # one split, and more than one
    assert {p.ways for p in plans} == {0, 1}
    assert P.ceil_div(129, 16) == 9 and P.ceil_div(255, 256) == 1 and 129 <= 200 <= 255                        # ninth stage; one partial tile
    for c in P.GATE_SHAPE + P.GATE_WS:
        assert P.plan_of(c, cus, math).path == "f32", c
    assert P.plan_of(P.GATE_OPEN[0], cus, math).path == "image"
    for c in P.IMAGE + P.GATE_OPEN:                             # the workspace asked for holds the slabs of either split count
        m, n, k, _ = c
        images = P.ceil_div(k, 16) * 8 * (3 if math == "bf16x6" else 2) * (P.ceil_div(m, 128) * 128 + P.ceil_div(n, 256) * 256) * 4
        p = P.plan_of(c, cus, math)
        assert images + (p.splits * m * n * 4 if p.splits > 1 else 0) <= P.gemm_split_ws_bytes(m, n, k, cus)
    assert all(P.plan_of(c, cus, "f32").path == "f32" for c in P.IMAGE)


def test_reduction_plans():
    for m, want in P.COLSUM_SLICES.items():
        assert P.colsum_plan(m) == want
    assert [P.colsum_plan(m)[0] for m in P.COLSUM_M] == [1] * 9 + [2, 4, 64, 64, 64]
    assert all(s * per >= m > (s - 1) * per for m in P.COLSUM_M for s, per in [P.colsum_plan(m)])
    assert tuple(P.bias_grad_plan(n, hw)[0] for n, _, hw in P.BIAS_GRAD) == P.BIAS_GRAD_SLICES
    pers = [P.bias_grad_plan(n, hw)[1] for n, _, hw in P.BIAS_GRAD]
    assert pers == [3, 7, 13, 35, 1, 3, 3]                     # short passes of 3, 7, 5 (after 8), 3 (after 32), 1, 3 (the last slice: 1), 3
    assert 64 * 32 * 600 > 4096 * 256 >= 5 * 16 * 300          # temporal_fusion_bwd: the third case enters the grid-stride loop


# ---- discrimination -----------------------------------------------------------------------------------------------------------------
def misses(wrong, want):
    try:
        close(wrong, want)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("case", sorted(set(P.ALL_CASES)), ids=P.case_id)
def test_cases_discriminate(case):
    """Each wrong reference misses `close`, for the plain product and after bias + ReLU + mask.  The last non-empty split is taken from
    the plan at either CU count and, for the image cases, either split count (a case that does not split loses its whole sum)."""
    m, n, k, _ = case
    a, b, _, _ = P.operands(m, n, k)
    a, b = a.astype(np.float64), b.astype(np.float64)
    want = P.reference(m, n, k)
    assert np.array_equal(want, a @ b)
    wrong = {"last reduction element dropped": a[:, :k - 1] @ b[:k - 1], "row m-1 dropped": want.copy(), "column n-1 dropped": want.copy()}
    wrong["row m-1 dropped"][m - 1] = 0
    wrong["column n-1 dropped"][:, n - 1] = 0
    maths = ("bf16x3", "bf16x6") if case.ws.startswith("image") else ("f32",)
    for cus in CUS:
        for math in maths:
            plan = P.plan_of(case, cus, math)
            k0, k1 = P.split_ranges(m, n, k, plan)[-1]
            assert k0 < k1 == k
            wrong["last split of %d left out (%s, %d CUs)" % (plan.splits, math, cus)] = want - a[:, k0:k1] @ b[k0:k1]
    for what, w in wrong.items():
        assert misses(w, want), what
        if min(m, n) > 1:                                       # (a lone row or column may be masked out whole: nothing to see there)
            assert misses(P.epilogue(w, m, n, k), P.epilogue(want, m, n, k)), what + ", bias + ReLU + mask"


# ---- the harness notices (CPU) ------------------------------------------------------------------------------------------------------
class StandIn:
    """vl_gemm's contract in torch on the CPU, split-K through the workspace as the plan says (a slab per split, the empty ones zeros,
    then their sum) -- and, on request, one of the defects the GPU harness is there to catch."""

    def __init__(self, defect=None, cus=256):
        self.defect, self.cus = defect, cus

    def gemm(self, a, b, c, m, n, k, transa=False, transb=False, lda=None, ldb=None, ldc=None, bias=None, relu=False, relu_mask=None, ws=None):
        kk = k + 1 if self.defect == "reads one past k" else k
        A = a.as_strided((kk, m), (lda, 1)).T if transa else a.as_strided((m, kk), (lda, 1))
        B = b.as_strided((n, kk), (ldb, 1)).T if transb else b.as_strided((kk, n), (ldb, 1))
        A, B = A.double(), B.double()
        plan = P.gemm_plan(m, n, k, 0 if ws is None else 4 * ws.numel(), self.cus)
        if plan.splits > 1:
            slabs = ws[:plan.splits * m * n].view(plan.splits, m, n)
            ranges = P.split_ranges(m, n, k, plan)
            for z in range(plan.splits):
                if z < len(ranges):
                    slabs[z] = (A[:, ranges[z][0]:ranges[z][1]] @ B[ranges[z][0]:ranges[z][1]]).float()
                elif self.defect != "empty split not stored":
                    slabs[z] = 0
            r = slabs.double().sum(0)
        else:
            r = A[:, :kk] @ B[:kk]
            if ws is not None and self.defect == "writes an unused workspace":
                ws[0] = 0
        if bias is not None:
            r = r + bias[:n].double()
        if relu:
            r = r.clamp(min=0)
        if relu_mask is not None:
            r = r * (relu_mask.as_strided((m, n), (ldc, 1)) > 0)
        c.as_strided((m, n), (ldc, 1)).copy_(r.float())
        if self.defect == "writes behind row m-1":
            c[(m - 1) * ldc + n] = 0
        if ws is not None and self.defect == "writes behind the workspace":
            ws.as_strided((1,), (1,), ws.storage_offset() + ws.numel()).zero_()


HARNESS_JOBS = [(P.Case(65, 129, 17, "none"), False, False), (P.Case(65, 129, 17, "none"), True, True), (P.EMPTY_SPLIT[0], False, True),
                (P.UNSPLIT[0], True, False)]


@pytest.mark.parametrize("defect,message", [(None, None), ("reads one past k", "non-finite output"), ("empty split not stored", "non-finite output"),
                                            ("writes an unused workspace", "unsplit, yet the workspace was written"),
                                            ("writes behind row m-1", "outside an m x n window"),
                                            ("writes behind the workspace", "guard behind the workspace written")])
def test_harness_notices(defect, message):
    """The harness of tests/test_gemm_geometry_gpu.py on the CPU: a correct stand-in passes it, and each defect is reported as what it
    is -- the NaN padding turns an over-read and an unstored slab into a non-finite window, the sentinels show both stray writes."""
    from tests.test_gemm_geometry_gpu import check, run
    if defect is None:
        check(run(StandIn(), HARNESS_JOBS, dev="cpu", ncus=256), fp32=True)
        return
    with pytest.raises(AssertionError, match=message):
        run(StandIn(defect), HARNESS_JOBS, dev="cpu", ncus=256)
