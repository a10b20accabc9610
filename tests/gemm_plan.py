"""The dispatch arithmetic of the dense side restated in plain Python for the tests: vl_gemm, gemm_split_splits,
vl_gemm_split_ws_bytes and launch_reduce_slabs of csrc/mfma_gemm.hip, vl_colsum and vl_bias_grad_nchw of csrc/pointwise.hip -- and the
case lists, inputs and fp64 references that tests/test_gemm_geometry.py (CPU) and tests/test_gemm_geometry_gpu.py share.  Nothing here
imports the package: the kernels are checked AGAINST these."""
import collections
import functools

import numpy as np

BR = 16                 # reduction tile of the fp32 GEMM instances = k per stage of the split-image kernel
CONV_MATH = {"f32": 0, "bf16": 1, "bf16x3": 3, "bf16x6": 6}


def ceil_div(a, b):
    return -(-a // b)


# ---- launchers ----------------------------------------------------------------------------------------------------------------------
def gemm_split_splits(m, n, k, slots):
    """gemm_split_splits: split-K of the split-image GEMM (128 x 256 tiles), each split >= 8 stages deep, none empty."""
    nstages, tiles = ceil_div(k, BR), ceil_div(m, 128) * ceil_div(n, 256)
    splits = 1
    if tiles < slots:
        splits = min(ceil_div(slots, tiles), 8)
        if splits > nstages // 8:
            splits = max(nstages // 8, 1)
    return ceil_div(nstages, ceil_div(nstages, splits))


def gemm_split_ws_bytes(m, n, k, cus):
    """vl_gemm_split_ws_bytes: operand images of three planes, the slabs of the two-workgroups-per-CU split count, 4096 spare."""
    st, mp, np_ = ceil_div(k, BR), ceil_div(m, 128) * 128, ceil_div(n, 256) * 256
    splits = gemm_split_splits(m, n, k, 2 * cus)
    return st * 24 * (mp + np_) * 4 + (splits * m * n * 4 if splits > 1 else 0) + 4096


def reduce_ways(count, splits):
    """launch_reduce_slabs: 4 = a workgroup per 64 elements, its four waves a quarter of the slabs each; 1 = a thread per element."""
    return 4 if splits >= 16 and count * 4 <= splits * 65536 else 1


Plan = collections.namedtuple("Plan", "path bm splits per empty ways")
# path   "f32": mfma_contract<64,1,4> / <128,2,2> on 16-element reduction tiles; "image": gemm_split_kernel on 16-element stages
# bm     tile height of the fp32 instance (the image kernel's tiles are 128 x 256)
# splits grid.z; per = reduction tiles (stages) per split; empty = trailing splits that own no tile and must store zeros
# ways   the slab reduction behind splits > 1 (0 when there is none)


def gemm_plan(m, n, k, ws_bytes, cus, math="f32"):
    """What vl_gemm launches for an m x n x k product with a workspace of ws_bytes (0: none) on a device of `cus` compute units."""
    code = CONV_MATH[math]
    if code != 0 and min(m, n, k) >= 128 and ws_bytes > 0 and ws_bytes >= gemm_split_ws_bytes(m, n, k, cus):
        splits = gemm_split_splits(m, n, k, cus * (1 if code == 6 else 2))
        return Plan("image", 128, splits, ceil_div(ceil_div(k, BR), splits), 0, reduce_ways(m * n, splits) if splits > 1 else 0)
    bm = 64 if m <= 64 else 128
    tiles, want, splits = ceil_div(m, bm) * ceil_div(n, 128), 3 * cus, 1
    if ws_bytes > 0 and tiles < want:
        splits = min(ceil_div(want, tiles), max(k // 256, 1), ws_bytes // (m * n * 4))
        splits = max(splits, 1)
    rtiles = ceil_div(k, BR)
    per = ceil_div(rtiles, splits)
    return Plan("f32", bm, splits, per, splits - ceil_div(rtiles, per), reduce_ways(m * n, splits) if splits > 1 else 0)


def split_ranges(m, n, k, plan):
    """[(k0, k1)] of the plan's NON-EMPTY splits, in reduction elements."""
    rtiles = ceil_div(k, BR)
    return [(z * plan.per * BR, min(k, (z + 1) * plan.per * BR)) for z in range(plan.splits) if z * plan.per < rtiles]


def colsum_plan(m):
    """vl_colsum: (row slices, rows per slice); more than one slice goes through the workspace and sum_partials_kernel."""
    per = ceil_div(m, min(ceil_div(m, 256), 64))
    return ceil_div(m, per), per


def bias_grad_plan(n, hw):
    """vl_bias_grad_nchw: (image slices, images per slice); a slice walks its images 8 per pass."""
    want = (n * hw + 8191) // 8192
    s = 1 if want < 1 else 64 if want > 64 else n if want > n else want
    per = ceil_div(n, s)
    return ceil_div(n, per), per


# ---- GEMM cases ---------------------------------------------------------------------------------------------------------------------
# ws: "none" | "ample" (32 slabs) | "3mn" | "mn-1" (floats) | "image" (vl_gemm_split_ws_bytes) | "image-1" (one float short)
Case = collections.namedtuple("Case", "m n k ws")

EDGE_M = (1, 63, 64, 65, 127, 128, 129, 257)
EDGE_N = (1, 127, 128, 129, 257)
EDGE_K = (1, 2, 15, 16, 17, 31, 32, 33, 100)
TILE_EDGES = ([Case(m, n, k, "none") for k in (17, 100) for m in EDGE_M for n in EDGE_N]
              + [Case(m, n, k, "none") for m, n in ((1, 1), (65, 129), (129, 257)) for k in EDGE_K if k not in (17, 100)])

EMPTY_SPLIT = [Case(8, 128, 4624, "ample"), Case(200, 129, 4624, "ample")]       # 18 splits of 17 tiles over 289: the 18th owns none
FOUR_WAY = [Case(8, 1024, 4096, "ample"), Case(8, 1024, 4400, "ample")]          # 16 and 17 splits
CAPPED = [Case(70, 200, 2048, "3mn"), Case(64, 200, 2048, "3mn")]                # the workspace holds three slabs: both tile heights
UNSPLIT = [Case(70, 200, 2048, "mn-1"), Case(129, 257, 200, "ample")]            # less than one slab; k < 256
SPLIT_K = EMPTY_SPLIT + FOUR_WAY + CAPPED + UNSPLIT

IMAGE = [Case(*s, "image") for s in ((128, 128, 128), (129, 129, 129), (130, 200, 144), (128, 255, 256), (300, 257, 1000), (129, 300, 4624))]
GATE_SHAPE = [Case(127, 300, 200, "image"), Case(300, 127, 200, "image"), Case(300, 200, 127, "image")]      # one side below 128
GATE_WS = [Case(130, 300, 200, "image-1"), Case(130, 300, 200, "none")]
GATE_OPEN = [Case(130, 300, 200, "image")]
ALL_CASES = TILE_EDGES + SPLIT_K + IMAGE + GATE_SHAPE + GATE_WS + GATE_OPEN


def ws_floats(case, cus):
    m, n, k, ws = case
    return {"none": 0, "ample": 32 * m * n, "3mn": 3 * m * n, "mn-1": m * n - 1, "image": gemm_split_ws_bytes(m, n, k, cus) // 4,
            "image-1": gemm_split_ws_bytes(m, n, k, cus) // 4 - 1}[ws]


def plan_of(case, cus, math="f32"):
    return gemm_plan(case.m, case.n, case.k, 4 * ws_floats(case, cus), cus, math)


def case_id(c):
    return "-".join(str(v) for v in c)


@functools.lru_cache(maxsize=None)
def operands(m, n, k):
    """a [m][k], b [k][n], bias [n], mask [m][n] of a shape: fp32, read-only, the same for every test and transpose."""
    rng = np.random.default_rng([m, n, k])
    out = (rng.standard_normal((m, k)).astype(np.float32), rng.standard_normal((k, n)).astype(np.float32),
           rng.standard_normal(n).astype(np.float32), rng.standard_normal((m, n)).astype(np.float32))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(m, n, k):
    """The fp64 product of the fp32 operands."""
    a, b, _, _ = operands(m, n, k)
    want = a.astype(np.float64) @ b.astype(np.float64)
    want.setflags(write=False)
    return want


def epilogue(want, m, n, k):
    """bias + ReLU + mask on a product, as EpiRowMajor and reduce_slabs_kernel apply them."""
    _, _, bias, mask = operands(m, n, k)
    return np.maximum(want + bias, 0) * (mask > 0)


# ---- reduction cases ----------------------------------------------------------------------------------------------------------------
COLSUM_M = (1, 7, 8, 9, 31, 32, 33, 255, 256, 257, 1000, 16384, 16385, 20000)
COLSUM_N = (1, 31, 32, 33, 300)
COLSUM_PAD = (0, 3)                                            # lda - n
COLSUM_SLICES = {257: (2, 129), 16384: (64, 256), 16385: (64, 257)}
BIAS_GRAD = [(5, 3, 3249), (19, 5, 1000), (37, 4, 500), (70, 2, 225), (2, 3, 9000), (130, 2, 4096), (3, 7, 169)]       # n, c, hw
BIAS_GRAD_SLICES = (2, 3, 3, 2, 2, 44, 1)
TRANSPOSE = [(1, 1), (1, 40), (31, 33), (32, 32), (33, 65), (300, 7)]                                              # rows, cols
TRANSPOSE_PAD = (0, 5)
FUSION = [(1, 1, 1), (5, 16, 300), (64, 32, 600), (3, 1, 257)]                                                     # b, T, H
