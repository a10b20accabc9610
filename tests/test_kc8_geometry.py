"""The CPU half of tests/test_kc8_geometry_gpu.py (no GPU needed): the launch arithmetic restated in tests/kc8_plan.py reaches every
branch the case lists are named for, at 256 and at 64 compute units; the references are right (naive loops, torch's own rounding); the
cases discriminate -- a product that lost its last reduction element, its last slab, its last 8-row or 8-column block, that counted a
slab twice, added the bias per slab or applied ReLU before the slab sum fails the comparison the GPU half applies, on the very inputs
it uploads; the GPU harness itself runs here against a stand-in and names each defect it is there to catch; and the two entry points
refuse what they cannot run before they ask for a device."""
import numpy as np
import pytest
import torch

from tests import kc8_plan as P
from tests.test_kc8_geometry_gpu import agree, check, check_pack, run, run_engine, run_pack

CUS = (256, 64)


# ---- coverage -----------------------------------------------------------------------------------------------------------------------
def assert_coverage(cus):
    """Every list reaches the branch it is named for on a device of `cus` compute units (the GPU half calls this with its own)."""
    lists = P.cases(cus)
    plans = {c: P.plan_of(c, cus) for cs in lists.values() for c in cs}
    # DIRECT: one slab, stored straight into c; tiny / whole / tail fetches and every pipeline depth on one tile; 2 x 2 tiles
    assert all(plans[c].direct and plans[c].slabs == 1 and (plans[c].rows_p, plans[c].co_p) == (c.m, c.n) for c in lists["DIRECT"])
    one = [plans[P.Case(256, 128, k, False, False)].slab[0] for k in P.DIRECT_K]
    assert [(s.stages, s.tail, s.tiny) for s in one] == [(1, 1, True), (1, 8, True), (1, 31, True), (1, 0, False), (2, 8, False), (3, 0, False),
                                                         (4, 0, False), (15, 0, False)]
    assert plans[P.DIRECT[-1]][:3] == (2, 2, 4)
    assert P.plan(256, 128, 480, 10 ** 6).slabs == 1 and P.plan(256, 128, 512, cus).slabs == 2        # 480: the largest k that never splits
    # REDUCED: one slab through the workspace; each of the four conditions of `direct` fails alone
    assert all(not plans[c].direct and plans[c].slabs == 1 for c in lists["REDUCED"])
    for c in P.EPILOGUE:
        assert P.plan(c.m, c.n, c.k, cus).direct and not plans[c].direct
    assert P.plan(128, 128, 64, cus).direct is False and P.plan(256, 8, 32, cus).direct is False     # m % 256, n % 128 alone
    assert P.plan(256, 128, 512, cus).direct is False                                                  # slabs alone
    p = plans[P.Case(264, 136, 70, False, False)]
    assert (p.ta, p.tb, p.rows_p, p.co_p) == (2, 2, 512, 256) and p.slab[0][2:] == (3, 6, False)      # one tap / one block in the second tiles
    assert {c.m % 256 for c in P.PARTIAL} >= {8, 128, 248} and {c.n % 128 for c in P.PARTIAL} >= {8, 120}
    assert plans[P.Case(8, 8, 5, False, False)].slab[0][2:] == (1, 5, True) and plans[P.Case(8, 128, 31, False, False)].slab[0].tiny
    assert plans[P.Case(248, 120, 33, False, False)].slab[0][2:] == (2, 1, False)
    # SPLIT
    sp = {P.case_id(c): plans[c] for c in lists["SPLIT"]}
    assert all(not p.direct and p.slabs > 1 for p in sp.values())
    p = sp["256x128x511"]
    assert (p.slabs, p.slab_len) == (2, 256) and p.slab[-1][2:] == (8, 31, False) and p.slab[0][2:] == (8, 0, False)
    p = sp["256x128x512"]
    assert (p.slabs, p.slab_len) == (2, 256) and all(s[2:] == (8, 0, False) for s in p.slab)
    p = sp["256x128x520"]
    assert (p.slabs, p.slab_len) == (2, 288) and p.slab[-1][2:] == (8, 8, False) and p.slab[-1].k1 - p.slab[-1].k0 == 7 * 32 + 8
    assert all(sp[i].slabs == 8 and sp[i].s == 8 for i in ("256x128x2048+bias", "256x128x2048+relu", "256x128x2048+bias+relu"))
    p = sp["264x136x2592"]
    assert (p.s, p.slabs, p.slab_len) == (10, 9, 288) and p.slabs < p.s                               # fewer slabs than asked for
    p = plans[P.CU_CAPPED]
    assert p.tiles == 16 and p.want == cus // 8 and p.s == min(p.want, p.stages // 8) and p.stages // 8 == 33
    if cus == 256:
        assert (p.s, p.per, p.slabs, p.slab[-1].tail) == (32, 9, 30, 5) and p.s < p.stages // 8       # capped by the CU term
    if cus == 64:
        assert (p.s, p.slabs) == (8, 8)
    # MANY_TILES: more tiles than two per CU, so no split although k >= 512
    c, = lists["MANY_TILES"]
    p = plans[c]
    assert p.tiles == 2 * cus + 1 and p.ta >= p.tb and p.want == 0 and p.s == 1 and p.slabs == 1 and p.direct and c.k == 512
    assert all(P.plan(256 * ta, 128 * tb, 512, cus).tiles <= 2 * cus or ta * tb >= p.tiles for ta in range(1, 64) for tb in range(1, 64))
    if cus == 256:
        assert (c.m, c.n) == (6912, 2432)
    # together
    every = list(plans.values())
    assert set().union(*(P.fetches(p) for p in every)) == {"whole", "tail", "tiny"}
    assert set().union(*(P.depths(p) for p in every)) == {1, 2, 3, 4}
    slabs = {p.slabs for p in every}
    assert slabs >= {1, 2, 8, 9}                                 # sum_slabs_c8: below 8, exactly 8, 8 + 1
    if cus >= 256:
        assert any(s >= 16 and s % 8 for s in slabs)             # two passes of eight and a remainder
    for cond in ("slabs", "bias", "relu", "m", "n"):
        assert {True, False} <= {direct_without(c, cus, cond) for c in plans}, cond


def direct_without(case, cus, cond):
    """Is the case direct once the named condition of the rule is the only one left to decide it?"""
    p = P.plan_of(case, cus)
    conds = dict(slabs=p.slabs == 1, bias=not case.bias, relu=not case.relu, m=case.m % 256 == 0, n=case.n % 128 == 0)
    others = all(v for name, v in conds.items() if name != cond)
    return conds[cond] if others else None


@pytest.mark.parametrize("cus", CUS)
def test_lists_reach_their_branches(cus):
    assert_coverage(cus)


def test_plan_matches_the_figures_of_the_issue_at_256():
    """The workspace is slabs x padded tile area; the direct rule does not change it."""
    assert P.plan(256, 128, 2048, 256).ws_bytes == 8 * 256 * 128 * 4 == P.plan(256, 128, 2048, 256, True, True).ws_bytes
    assert P.plan(264, 136, 70, 256).ws_bytes == 512 * 256 * 4 and P.plan(256, 128, 40, 256).ws_bytes == 256 * 128 * 4
    assert P.plan(8, 8, 5, 256).ws_bytes == 256 * 128 * 4


def test_engine_and_row_block_shapes():
    for cus in CUS:
        for frames in P.ENGINE_FRAMES:
            prods = P.engine_products(frames)
            assert [(p.m, p.n, p.k) for p in prods] == [(frames, 136, 72), (72, 136, frames), (frames, 72, 136), (frames, 64, 40),
                                                        (40, 64, frames), (frames, 40, 64)]
            assert all(p.m % 8 == 0 and p.n % 8 == 0 for p in prods)
            orient = {(o[3] == 1, o[4] == 1) for p in prods for o in (p.a, p.b)}
            assert orient == {(True, False), (False, True)}      # both pack orders
            assert len({(p.a[0], p.a[3] == 1) for p in prods} | {(p.b[0], p.b[3] == 1) for p in prods}) >= 6
            for p in prods:
                pl = P.plan(p.m, p.n, p.k, cus, bool(p.bias), p.relu)
                assert pl.slabs == 1 and not pl.direct
                if p.k == frames:
                    assert pl.slab[0].tiny                       # the weight gradients: k = frames < 32
            blocks = [P.plan(r1 - r0, P.ROW_BLOCK_N, frames, cus) for r0, r1 in P.ROW_BLOCKS]
            assert [b.direct for b in blocks] == [True, False] and all(r0 % 128 == 0 and r1 % 128 == 0 for r0, r1 in P.ROW_BLOCKS)
            assert P.ROW_BLOCKS[0][0] == 0 and P.ROW_BLOCKS[-1][1] == P.ROW_BLOCK_M and P.ROW_BLOCKS[0][1] == P.ROW_BLOCKS[1][0]


def test_pack_cases_reach_both_orders():
    rows = [c for c in P.PACK if P.pack_order(c.cs) == "cb"]
    cols = [c for c in P.PACK if P.pack_order(c.cs) == "pos"]
    assert {c.P % 4 for c in rows} == {0, 1, 2, 3} and {c.P for c in rows} >= {1, 3, 4, 5, 1023} and {c.C for c in rows} >= {1, 7, 8, 9, 20}
    assert any(c.ps > c.C for c in rows)                         # a leading dimension larger than C
    assert {c.P for c in cols if c.ps == 1} >= {1, 255, 257} and any(c.ps > 1 and c.cs > 1 for c in cols)
    for group in (rows, cols):
        threads = [P.pack_threads(c.P, c.C, c.cs) for c in group]
        assert any(t > 256 and t % 256 for t in threads) and any(t < 256 for t in threads)      # a short last block; a lone short block
        assert any(c.C % 8 for c in group) and any(c.C % 8 == 0 for c in group)      # pad channels, and none
    assert any(P.pack_threads(c.P, c.C, c.cs) % 256 == 0 for c in rows)
    assert P.pack_threads(1023, 20, 1) == 768 and P.pack_threads(1025, 20, 1) == 771 and P.pack_threads(257, 20, 257) == 771
    assert all(len(P.SPECIALS) <= c.P * c.C or c.P * c.C < 64 for c in P.PACK)
    assert any(c.P * c.C >= len(P.SPECIALS) for c in rows) and any(c.P * c.C >= len(P.SPECIALS) for c in cols)


# ---- the references are right -------------------------------------------------------------------------------------------------------
def test_integer_sums_are_exact_in_fp32():
    """|operand| <= 8 and |bias| <= 64: every partial sum of every case is an integer of magnitude <= 64 k + 64 < 2^24."""
    for cus in CUS:
        for cs in P.cases(cus).values():
            for c in cs:
                assert P.INT_MAX_ABS ** 2 * c.k + P.INT_MAX_ABS ** 2 < 2 ** 24
                if c.m * c.k <= 1 << 22:
                    a, b, bias = P.operands(c.m, c.n, c.k, "int")
                    assert max(np.abs(a).max(), np.abs(b).max()) <= P.INT_MAX_ABS and np.abs(bias).max() <= P.INT_MAX_ABS ** 2
                    assert np.array_equal(a, np.round(a)) and np.array_equal(P.bf16_round(a), a) and np.array_equal(P.bf16_round(b), b)
    assert 64 * 8453 + 64 < 2 ** 24
    for frames in P.ENGINE_FRAMES:
        for name, mat in P.engine_matrices(frames, "int").items():
            assert np.array_equal(P.bf16_round(mat), mat) or mat.ndim == 1


@pytest.mark.parametrize("kind", P.KINDS)
def test_references_equal_naive_loops(kind):
    for case in (P.Case(8, 8, 5, True, True), P.Case(16, 8, 33, True, False)):
        a, b, bias = P.operands(case.m, case.n, case.k, kind)
        assert np.array_equal(P.bf16_round(a), a) and np.array_equal(P.bf16_round(b), b)              # what the kernel multiplies
        loops = P.product_loops(a, b, bias, case.relu)
        want = P.want_of(case, kind)
        if kind == "int":
            assert np.array_equal(want, loops)
        else:
            np.testing.assert_allclose(want, loops, rtol=1e-13, atol=1e-13)
    mats = P.engine_matrices(8, kind)
    pr = P.engine_products(8)[0]                                 # fc6 forward: c[frame][j] = relu(sum_f x[frame][f] W[f][j] + b[j])
    want = np.maximum(P.bf16_round(mats["x"]).astype(np.float64) @ P.bf16_round(mats["W"]).astype(np.float64) + mats["fc6b"], 0)
    np.testing.assert_allclose(P.engine_want(pr, mats), want, rtol=1e-13, atol=1e-13)
    pr = P.engine_products(8)[2]                                 # fc6 input gradient: d W^T
    want = P.bf16_round(mats["d"]).astype(np.float64) @ P.bf16_round(mats["W"]).astype(np.float64).T
    np.testing.assert_allclose(P.engine_want(pr, mats), want, rtol=1e-13, atol=1e-13)


def test_pack_reference_is_torchs_rounding():
    assert np.array_equal(P.bf16_bits(P.SPECIALS.view(np.float32))[:-1], P.SPECIALS_BF16[:-1])        # by hand == torch; NaN stays NaN
    assert (P.bf16_bits(P.SPECIALS.view(np.float32))[-1] & 0x7FFF) > 0x7F80
    for case in (P.Pack(5, 9, 12, 1), P.Pack(3, 20, 1, 3), P.Pack(37, 20, 2, 80)):
        mat, src = P.pack_source(case)
        assert np.array_equal(P.gather(src, case.P, case.C, case.ps, case.cs).view(np.uint32), mat.view(np.uint32))
        img = P.to_kc8(mat)
        assert img.shape == (P.ceil_div(case.C, 8), case.P, 8) and np.array_equal(img, P.to_kc8_loops(mat))
        back = torch.from_numpy(img.view(np.int16)).view(torch.bfloat16).float().numpy()               # [CB][P][8] -> [P][CB * 8]
        back = back.transpose(1, 0, 2).reshape(case.P, -1)
        want = torch.from_numpy(mat.copy()).bfloat16().float().numpy()
        assert np.array_equal(back[:, :case.C], want, equal_nan=True) and not back[:, case.C:].any()
        assert not np.signbit(back[:, case.C:]).any()            # +0 in the pad channels
    present = set(np.concatenate([P.pack_source(c)[0].reshape(-1).view(np.uint32) for c in P.PACK if c.P * c.C >= 64]).tolist())
    assert present >= set(P.SPECIALS.tolist())


# ---- discrimination -----------------------------------------------------------------------------------------------------------------
def fails(kind, wrong, want):
    try:
        agree(kind, wrong.astype(np.float32), want, "defect")
    except AssertionError:
        return True
    return False


def defects(case, kind, cus):
    """{defect: what a kernel with that defect would return} on the case's own inputs."""
    m, n, k = case[:3]
    a, b, bias = P.operands(m, n, k, kind)
    bias = bias if case.bias else None
    plan, prod = P.plan_of(case, cus), P.reference(m, n, k, kind)
    epi = lambda x: P.epilogue(x, bias, case.relu)
    last = plan.slab[-1]
    tail = P.product(a, b, last.k0, last.k1)
    out = {"last reduction element dropped": epi(prod - np.outer(a[k - 1].astype(np.float64), b[k - 1].astype(np.float64))),
           "last slab of %d dropped" % plan.slabs: epi(prod - tail), "last slab of %d counted twice" % plan.slabs: epi(prod + tail)}
    rows, cols = prod.copy(), prod.copy()
    rows[m - 8:] = 0
    cols[:, n - 8:] = 0
    out["last 8-row block dropped"], out["last 8-column block dropped"] = epi(rows), epi(cols)
    if plan.slabs > 1 and case.bias:
        out["bias added per slab"] = P.epilogue(prod, bias * plan.slabs, case.relu)
    if plan.slabs > 1 and case.relu:
        early = sum(np.maximum(P.product(a, b, s.k0, s.k1), 0) for s in plan.slab)
        out["ReLU before the slab sum"] = epi(early)
    return out


def all_cases(cus):
    return [c for cs in P.cases(cus).values() for c in cs]


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("case", sorted(set(all_cases(256) + all_cases(64))), ids=P.case_id)
def test_cases_discriminate(case, kind):
    want = P.want_of(case, kind)
    assert not fails(kind, want, want)
    seen = set()
    for cus in CUS:
        if case not in all_cases(cus):
            continue
        for what, wrong in defects(case, kind, cus).items():
            assert fails(kind, wrong, want), "%s at %d CUs goes unnoticed" % (what, cus)
            seen.add(what)
    assert len(seen) >= 5


def test_every_defect_is_shown_by_some_case():
    names = set()
    for c in P.SPLIT:
        names |= set(defects(c, "int", 256)) if c.m * c.n * c.k < 1 << 27 else set()
    assert {"bias added per slab", "ReLU before the slab sum"} <= names


@pytest.mark.parametrize("kind", P.KINDS)
def test_engine_cases_discriminate(kind):
    """The weight gradients (k = frames) lose a frame, the others their last reduction element; the row-block form loses its second block."""
    for frames in P.ENGINE_FRAMES:
        mats = P.engine_matrices(frames, kind)
        for pr in P.engine_products(frames):
            want = P.engine_want(pr, mats)
            short = pr._replace(a=pr.a[:1] + (pr.k - 1,) + pr.a[2:], b=pr.b[:1] + (pr.k - 1,) + pr.b[2:], k=pr.k - 1)
            assert fails(kind, P.engine_want(short, mats), want), pr.name
        want = P.reference(P.ROW_BLOCK_M, P.ROW_BLOCK_N, frames, kind)
        wrong = want.copy()
        wrong[P.ROW_BLOCKS[1][0]:] = 0
        assert fails(kind, wrong, want)


# ---- the harness notices (CPU) ------------------------------------------------------------------------------------------------------
class StandIn:
    """The contracts of pack_kc8 and gemm_kc8 in torch on the CPU, the product through the workspace as the plan says (padded slab images,
    then their sum in slab order) -- and, on request, one of the defects the GPU harness is there to catch."""

    def __init__(self, defect=None, cus=256):
        self.defect, self.cus = defect, cus

    @staticmethod
    def kc8_shape(positions, channels):
        return ((channels + 7) // 8, positions, 8)

    def gemm_kc8_ws_bytes(self, m, n, k):
        return P.plan(m, n, k, self.cus).ws_bytes + (4 if self.defect == "asks for another workspace" else 0)

    def pack_kc8(self, src, dst, positions, channels, pos_stride, ch_stride):
        assert dst.data_ptr() % 16 == 0 and tuple(dst.shape) == self.kc8_shape(positions, channels)
        mat = src.as_strided((positions, channels), (pos_stride, ch_stride))
        full = torch.zeros(positions, dst.shape[0] * 8)
        full[:, :channels] = mat
        dst.copy_(full.view(positions, -1, 8).permute(1, 0, 2).bfloat16())
        if self.defect == "pack leaves the pad channels":
            dst[-1, :, 7] = 1.0
        if self.defect == "pack writes behind its destination":
            dst.as_strided((1,), (1,), dst.storage_offset() + dst.numel()).zero_()

    def gemm_kc8(self, a, b, c, m, n, k, bias=None, relu=False, ws=None):
        assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
        A = a.permute(1, 0, 2).reshape(k, m).double()
        B = b.permute(1, 0, 2).reshape(k, n).double()
        plan = P.plan(m, n, k, self.cus, bias is not None, relu)
        if plan.direct:
            r = A.T @ B
            if ws is not None and self.defect == "direct call writes the workspace":
                ws[0] = 0
        else:
            assert ws is not None and ws.numel() * 4 >= plan.ws_bytes
            slabs = ws[:plan.slabs * plan.rows_p * plan.co_p].view(plan.slabs, plan.rows_p, plan.co_p)
            for z, s in enumerate(plan.slab):
                slabs[z] = 0
                slabs[z, :m, :n] = (A[s.k0:s.k1].T @ B[s.k0:s.k1]).float()
            if self.defect == "slab element not stored":
                slabs[plan.slabs - 1, m - 1, n - 1] = float("nan")
            r = slabs[:, :m, :n].double().sum(0)
            if bias is not None:
                r = r + bias[:n].double()
            if relu:
                r = r.clamp(min=0)
        flat = r.float().reshape(-1)
        if self.defect == "c element not stored":
            c[:m * n - 1].copy_(flat[:-1])
        else:
            c[:m * n].copy_(flat)
        if self.defect == "writes behind c":
            c[m * n] = 0
        if ws is not None and self.defect == "writes behind the workspace":
            ws.as_strided((1,), (1,), ws.storage_offset() + ws.numel()).zero_()


HARNESS_JOBS = [P.Case(256, 128, 40, False, False), P.Case(264, 136, 70, False, False), P.Case(256, 128, 511, False, False),
                P.Case(256, 128, 64, True, True), P.Case(8, 8, 5, False, False)]


@pytest.mark.parametrize("kind", P.KINDS)
def test_harness_passes_a_correct_stand_in(kind):
    check(run(StandIn(), HARNESS_JOBS, kind, dev="cpu", ncus=256), kind)
    check(run(StandIn(cus=64), HARNESS_JOBS, kind, dev="cpu", ncus=64), kind)


@pytest.mark.parametrize("defect,message", [("c element not stored", "non-finite output"), ("writes behind c", "written outside its window"),
                                            ("slab element not stored", "non-finite output"),
                                            ("writes behind the workspace", "guard behind the workspace written"),
                                            ("direct call writes the workspace", "direct, yet the workspace was written"),
                                            ("asks for another workspace", "not what the restated plan says")])
def test_harness_notices(defect, message):
    with pytest.raises(AssertionError, match=message):
        run(StandIn(defect), HARNESS_JOBS, "int", dev="cpu", ncus=256)


def test_harness_notices_a_plan_for_another_device():
    """A library that plans for 64 CUs where the harness expects 256 asks for another workspace in the split case."""
    with pytest.raises(AssertionError, match="not what the restated plan says"):
        run(StandIn(cus=64), [P.CU_CAPPED], "int", dev="cpu", ncus=256)


@pytest.mark.parametrize("kind", P.KINDS)
def test_engine_harness_on_the_stand_in(kind):
    got, whole, blockwise = run_engine(StandIn(), 8, kind, dev="cpu", ncus=256)
    mats = P.engine_matrices(8, kind)
    for pr, c in got:
        agree(kind, c, P.engine_want(pr, mats), pr.name)
    want = P.reference(P.ROW_BLOCK_M, P.ROW_BLOCK_N, 8, kind)
    agree(kind, whole, want, "whole")
    agree(kind, blockwise, want, "blockwise")
    with pytest.raises(AssertionError, match="outside its destination"):
        run_engine(StandIn("pack writes behind its destination"), 8, kind, dev="cpu", ncus=256)


def test_pack_harness_on_the_stand_in():
    jobs = [P.Pack(5, 9, 12, 1), P.Pack(257, 20, 1, 257), P.Pack(37, 20, 2, 80), P.Pack(4, 8, 8, 1)]
    check_pack(run_pack(StandIn(), jobs, dev="cpu"))
    with pytest.raises(AssertionError, match="elements differ"):
        check_pack(run_pack(StandIn("pack leaves the pad channels"), jobs, dev="cpu"))
    with pytest.raises(AssertionError, match="outside its destination"):
        run_pack(StandIn("pack writes behind its destination"), jobs, dev="cpu")


# ---- refusals that need no device ---------------------------------------------------------------------------------------------------
def test_ffi_refusals_need_no_device():
    """Both entry points validate before they plan (the plan asks the device for its CU count) and before they launch: null pointers,
    sizes, m or n no multiple of 8, the 32-bit-offset bound, and a kc8 address that is no multiple of 16.  Nothing runs."""
    from vltf_amd import _ffi
    p, i32, i64, sz = _ffi.p, _ffi.i32, _ffi.i64, _ffi.sz
    assert _ffi.SIGNATURES["vl_pack_kc8"] == (i32, [p, p, i64, i32, i64, i64, p])
    assert _ffi.SIGNATURES["vl_gemm_kc8"] == (i32, [p, p, p, i32, i32, i32, p, i32, p, sz, p])
    lib = _ffi.lib()
    fake = 4096                                  # a non-null, aligned address: validation fails before anything dereferences it
    ok = dict(src=fake, dst=fake, P=4, C=8, ps=8, cs=1)
    for over, msg in [(dict(src=None), b"bad argument"), (dict(dst=None), b"bad argument"), (dict(P=0), b"bad argument"), (dict(P=-1), b"bad argument"),
                      (dict(C=0), b"bad argument"), (dict(dst=fake + 2), b"16-byte aligned"), (dict(dst=fake + 8), b"16-byte aligned")]:
        a = dict(ok, **over)
        assert lib.vl_pack_kc8(a["src"], a["dst"], a["P"], a["C"], a["ps"], a["cs"], None) != 0, over
        err = lib.vl_last_error()
        assert b"vl_pack_kc8" in err and msg in err, (over, err)
    ok = dict(a=fake, b=fake, c=fake, m=8, n=8, k=8)
    for over, msg in [(dict(a=None), b"bad argument"), (dict(b=None), b"bad argument"), (dict(c=None), b"bad argument"), (dict(m=0), b"bad argument"),
                      (dict(n=-8), b"bad argument"), (dict(k=0), b"bad argument"), (dict(m=12), b"multiples of 8"), (dict(n=4), b"multiples of 8"),
                      (dict(m=8, n=1 << 20, k=1 << 15), b"32-bit offsets"), (dict(m=1 << 21, n=8, k=1 << 14), b"32-bit offsets"),
                      (dict(a=fake + 2), b"16-byte aligned"), (dict(b=fake + 8), b"16-byte aligned"), (dict(a=fake + 4, b=fake + 4), b"16-byte aligned")]:
        a = dict(ok, **over)
        assert lib.vl_gemm_kc8(a["a"], a["b"], a["c"], a["m"], a["n"], a["k"], None, 0, fake, 1 << 30, None) != 0, over
        err = lib.vl_last_error()
        assert b"vl_gemm_kc8" in err and msg in err, (over, err)
    assert lib.vl_gemm_kc8_ws_bytes(0, 8, 8) == 0 and lib.vl_gemm_kc8_ws_bytes(8, -8, 8) == 0 and lib.vl_gemm_kc8_ws_bytes(8, 8, 0) == 0
