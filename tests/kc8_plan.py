"""The launch arithmetic of the packed-bf16 dense product restated in plain Python for the tests: gemm_kc8_plan,
vl_gemm_kc8_ws_bytes, the `direct` rule of vl_gemm_kc8, the stages wgrad_c8_kernel<4,2,2> walks per slab and the thread order of
vl_pack_kc8 (csrc/conv_c8.hip) -- and the case lists, inputs and references that tests/test_kc8_geometry.py (CPU) and
tests/test_kc8_geometry_gpu.py share.  Nothing here imports the package: the kernels are checked AGAINST these."""
import collections
import functools

import numpy as np

KP = 32                 # reduction positions per pipeline stage
TILE_M, TILE_N = 256, 128
INT_MAX_ABS = 8         # integer inputs: operands uniform in [-8, 8], bias in [-64, 64]


def ceil_div(a, b):
    return -(-a // b)


# ---- launcher -----------------------------------------------------------------------------------------------------------------------
Slab = collections.namedtuple("Slab", "k0 k1 stages tail tiny")
# k0, k1  the slab's reduction range; stages = 32-position stages the workgroup walks (the depth the three-slot pipeline sees)
# tail    positions in its last stage when that stage is short (0: every stage whole); tiny = the short stage decodes per lane (k < 32)

Plan = collections.namedtuple("Plan", "ta tb tiles stages want s per slab_len slabs direct rows_p co_p ws_bytes slab")
# ta, tb  tiles of 256 rows / 128 columns; stages = ceil(k / 32); want = 2 CUs / tiles, s = the split count asked for (>= 1)
# per     stages per slab; slabs = grid.z <= s; direct = the kernel stores into c itself (no workspace, no reduction)
# rows_p, co_p  pitch of what the kernel stores; ws_bytes = vl_gemm_kc8_ws_bytes (the same with and without bias / ReLU); slab = [Slab]


def plan(m, n, k, cus, bias=False, relu=False):
    """What vl_gemm_kc8 launches for c[m][n] = sum_k a[k][m] b[k][n] on a device of `cus` compute units."""
    ta, tb = ceil_div(m // 8, 32), ceil_div(n, TILE_N)
    tiles, stages = ta * tb, ceil_div(k, KP)
    want = (2 * cus) // tiles
    s = max(min(want, stages // 8), 1)
    per = ceil_div(stages, s)
    slab_len = KP * per
    slabs = ceil_div(k, slab_len)
    direct = slabs == 1 and not bias and not relu and m % TILE_M == 0 and n % TILE_N == 0
    slab = []
    for z in range(slabs):
        k0, k1 = z * slab_len, min(k, (z + 1) * slab_len)
        slab.append(Slab(k0, k1, ceil_div(k1 - k0, KP), (k1 - k0) % KP, k < KP))
    return Plan(ta, tb, tiles, stages, want, s, per, slab_len, slabs, direct, m if direct else ta * TILE_M, n if direct else tb * TILE_N,
                slabs * ta * TILE_M * tb * TILE_N * 4, slab)


def fetches(p):
    """The branches of issue() the plan's stages take: "whole", "tail" (a short stage at k >= 32), "tiny" (k < 32)."""
    out = set()
    for s in p.slab:
        if s.stages > (1 if s.tail else 0):
            out.add("whole")
        if s.tail:
            out.add("tiny" if s.tiny else "tail")
    return out


def depths(p):
    """Stages per slab as the three-slot pipeline sees them: 1, 2, 3 or 4 (= four or more)."""
    return {min(s.stages, 4) for s in p.slab}


def pack_order(ch_stride):
    """vl_pack_kc8: "cb" = channel blocks fastest, four positions per thread (ch_stride == 1); "pos" = positions fastest, one each."""
    return "cb" if ch_stride == 1 else "pos"


def pack_threads(positions, channels, ch_stride):
    cb = ceil_div(channels, 8)
    return ceil_div(positions, 4) * cb if ch_stride == 1 else positions * cb


# ---- GEMM cases ---------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "m n k bias relu")


def _c(m, n, k, bias=False, relu=False):
    return Case(m, n, k, bias, relu)


DIRECT_K = (1, 8, 31, 32, 40, 96, 128, 480)    # tiny; tiny; tiny; one whole stage; tail of 8; depth 3; depth 4; 15 stages: never splits
DIRECT = [_c(256, 128, k) for k in DIRECT_K] + [_c(512, 256, 96)]
EPILOGUE = [_c(256, 128, 64, True, False), _c(256, 128, 64, False, True), _c(256, 128, 64, True, True)]     # each alone forces the reduction
PARTIAL = [_c(8, 8, 5), _c(264, 136, 70), _c(248, 120, 33), _c(128, 128, 64), _c(8, 128, 31), _c(256, 8, 32)]
REDUCED = EPILOGUE + PARTIAL
CU_CAPPED = _c(1024, 512, 8453)
SPLIT = [_c(256, 128, 511), _c(256, 128, 512), _c(256, 128, 520), _c(256, 128, 2048, True, False), _c(264, 136, 2592), CU_CAPPED,
         _c(256, 128, 2048, False, True), _c(256, 128, 2048, True, True)]       # (the last two: ReLU behind a slab sum)


def many_tiles(cus):
    """The smallest tile count above 2 CUs (2 CUs + 1) in its most nearly square factorisation, the larger factor on the rows
    (6912 x 2432 at 256 CUs), at k = 512: one slab and direct, although one tile would split the same k in two."""
    t = 2 * cus + 1
    f = max(d for d in range(1, int(t ** 0.5) + 1) if t % d == 0)
    return _c(TILE_M * (t // f), TILE_N * f, 512)


def cases(cus):
    return {"DIRECT": DIRECT, "REDUCED": REDUCED, "SPLIT": SPLIT, "MANY_TILES": [many_tiles(cus)]}


def plan_of(case, cus):
    return plan(case.m, case.n, case.k, cus, case.bias, case.relu)


def case_id(c):
    return "%dx%dx%d%s%s" % (c.m, c.n, c.k, "+bias" if c.bias else "", "+relu" if c.relu else "")


def branch(case, cus):
    """One line on what a case reaches, for the summary and for failure messages."""
    p = plan_of(case, cus)
    return "%s: %dx%d tiles, want %d, s %d, %d slab(s) of %d, stages %s, tails %s, %s, %s" % (
        case_id(case), p.ta, p.tb, p.want, p.s, p.slabs, p.slab_len, sorted({s.stages for s in p.slab}), sorted({s.tail for s in p.slab}),
        "+".join(sorted(fetches(p))), "direct" if p.direct else "reduced")


# ---- ENGINE cases -------------------------------------------------------------------------------------------------------------------
# The six products as engine.py packs them, in terms of row-major fp32 matrices: x [frames][F] (pool5), W [F][FC] (fc6W), d [frames][FC]
# (dfc6), xin [frames][D], K [D][4H], dz [frames][4H].  An operand is (matrix, positions, channels, pos_stride, ch_stride).
ENGINE_FRAMES = (8, 16)
F, FC, D, H4 = 72, 136, 40, 64
Product = collections.namedtuple("Product", "name a b m n k bias relu")


def engine_products(frames):
    n = frames
    return [Product("fc6 forward", ("x", F, n, 1, F), ("W", F, FC, FC, 1), n, FC, F, "fc6b", True),
            Product("fc6 weight gradient", ("x", n, F, F, 1), ("d", n, FC, FC, 1), F, FC, n, None, False),
            Product("fc6 input gradient", ("d", FC, n, 1, FC), ("W", FC, F, 1, FC), n, F, FC, None, False),
            Product("lstm input projection", ("xin", D, n, 1, D), ("K", D, H4, H4, 1), n, H4, D, "lstmb", False),
            Product("lstm kernel gradient", ("xin", n, D, D, 1), ("dz", n, H4, H4, 1), D, H4, n, None, False),
            Product("lstm input gradient", ("dz", H4, n, 1, H4), ("K", H4, D, 1, H4), n, D, H4, None, False)]


def engine_shapes(frames):
    return {"x": (frames, F), "W": (F, FC), "d": (frames, FC), "xin": (frames, D), "K": (D, H4), "dz": (frames, H4), "fc6b": (FC,),
            "lstmb": (H4,)}


ROW_BLOCK_M, ROW_BLOCK_N = 384, 128            # the DP row-block loop: a[r0 // 8:r1 // 8] and c[r0:r1], k = frames
ROW_BLOCKS = ((0, 256), (256, 384))            # (edges at multiples of 128) the first block is direct, the second is not


# ---- PACK cases ---------------------------------------------------------------------------------------------------------------------
Pack = collections.namedtuple("Pack", "P C ps cs")
PACK_P, PACK_C = (1, 3, 4, 5, 6, 1023, 1025), (1, 7, 8, 9, 20)
PACK_ROWS = [Pack(p, c, c, 1) for p in PACK_P for c in PACK_C] + [Pack(p, c, c + 3, 1) for p, c in ((1, 1), (5, 9), (1023, 20), (1025, 7))]
PACK_TRANSPOSE = [Pack(p, c, 1, max(p, 6)) for p in (1, 255, 257) for c in (1, 8, 20)] + [Pack(257, 9, 1, 262)]
PACK_STRIDED = [Pack(37, 20, 2, 80), Pack(257, 9, 3, 800)]
PACK = PACK_ROWS + PACK_TRANSPOSE + PACK_STRIDED

# fp32 bit patterns: ties to even in both directions and their neighbours, both signs; the largest finite fp32 (rounds to inf); zeros,
# infinities, NaN.  No subnormals: the flush mode is not the project's to set.
SPECIALS = np.array([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000, 0xBF808001, 0xBF807FFF, 0x7F7FFFFF, 0xFF7FFFFF,
                     0x7F7F8000, 0x7F7F7FFF, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000], np.uint32)
SPECIALS_BF16 = np.array([0x3F80, 0x3F82, 0x3F81, 0x3F80, 0xBF80, 0xBF82, 0xBF81, 0xBF80, 0x7F80, 0xFF80, 0x7F80, 0x7F7F, 0x0000, 0x8000, 0x7F80,
                          0xFF80, 0x7FC0], np.uint16)          # by hand; test_kc8_geometry.py proves them against torch


def pack_id(c):
    return "P%d-C%d-ps%d-cs%d" % c


def pack_src_len(c):
    return (c.P - 1) * c.ps + (c.C - 1) * c.cs + 1


@functools.lru_cache(maxsize=None)
def pack_source(case):
    """(matrix [P][C], src): Gaussians with the specials at seeded places, scattered into a source of the case's strides that is NaN
    wherever the pack has no business reading."""
    rng = np.random.default_rng(list(case))
    mat = rng.standard_normal((case.P, case.C)).astype(np.float32)
    where = rng.permutation(mat.size)[:len(SPECIALS)]
    mat.reshape(-1).view(np.uint32)[where] = SPECIALS[:len(where)]
    src = np.full(pack_src_len(case), np.nan, np.float32)
    idx = np.arange(case.P)[:, None] * case.ps + np.arange(case.C)[None, :] * case.cs
    assert len(np.unique(idx)) == idx.size                       # the strides of a case never alias
    src.view(np.uint32)[idx] = mat.view(np.uint32)
    for a in (mat, src):
        a.setflags(write=False)
    return mat, src


# ---- bf16 on the host ---------------------------------------------------------------------------------------------------------------
def bf16_bits(x):
    """Round-to-nearest-even bf16 bit patterns of an fp32 array, as torch's CPU .bfloat16() gives them."""
    import torch
    t = torch.from_numpy(np.array(x, np.float32)).bfloat16()      # (a copy: the inputs are read-only)
    return t.view(torch.int16).numpy().view(np.uint16)


def bf16_round(x):
    return (bf16_bits(x).astype(np.uint32) << 16).view(np.float32)


def to_kc8(mat):
    """kc8 image [ceil(C / 8)][P][8] (bf16 bit patterns) of a matrix [P][C]: +0 in the pad channels."""
    p, c = mat.shape
    cb = ceil_div(c, 8)
    full = np.zeros((p, cb * 8), np.uint16)
    full[:, :c] = bf16_bits(mat)
    return np.ascontiguousarray(full.reshape(p, cb, 8).transpose(1, 0, 2))


def to_kc8_loops(mat):
    """The same by the definition, element by element (small matrices only)."""
    p, c = mat.shape
    out = np.zeros((ceil_div(c, 8), p, 8), np.uint16)
    bits = bf16_bits(mat)
    for pos in range(p):
        for ch in range(c):
            out[ch // 8][pos][ch % 8] = bits[pos][ch]
    return out


# ---- GEMM inputs and references -------------------------------------------------------------------------------------------------------
KINDS = ("int", "gauss")


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def operands(m, n, k, kind):
    """a [k][m], b [k][n], bias [n] of a shape: fp32 values that bf16 holds exactly, read-only, the same for every test.
    "int": uniform integers in [-8, 8], integer bias in [-64, 64]; "gauss": standard normals rounded to bf16 (the bias stays fp32)."""
    rng = np.random.default_rng([m, n, k, KINDS.index(kind)])
    if kind == "int":
        a, b = (rng.integers(-INT_MAX_ABS, INT_MAX_ABS + 1, (k, w)).astype(np.float32) for w in (m, n))
        bias = rng.integers(-INT_MAX_ABS ** 2, INT_MAX_ABS ** 2 + 1, n).astype(np.float32)
    else:
        a, b = (bf16_round(rng.standard_normal((k, w)).astype(np.float32)) for w in (m, n))
        bias = rng.standard_normal(n).astype(np.float32)
    return _freeze(a, b, bias)


def product(a, b, k0=0, k1=None):
    """fp64 a[k0:k1]^T b[k0:k1]."""
    return a[k0:k1].astype(np.float64).T @ b[k0:k1].astype(np.float64)


@functools.lru_cache(maxsize=None)
def reference(m, n, k, kind):
    """The fp64 product of the bf16-exact operands, before bias and ReLU."""
    a, b, _ = operands(m, n, k, kind)
    want, = _freeze(product(a, b))
    return want


def epilogue(prod, bias, relu):
    out = prod if bias is None else prod + bias.astype(np.float64)
    return np.maximum(out, 0) if relu else out


def want_of(case, kind):
    bias = operands(case.m, case.n, case.k, kind)[2] if case.bias else None
    return epilogue(reference(case.m, case.n, case.k, kind), bias, case.relu)


def product_loops(a, b, bias, relu):
    """c = a^T b (+ bias) (ReLU) by the definition, in Python floats (doubles), for the proof of the references."""
    k, m = a.shape
    n = b.shape[1]
    out = np.zeros((m, n))
    for i in range(m):
        for j in range(n):
            s = 0.0
            for kk in range(k):
                s += float(a[kk][i]) * float(b[kk][j])
            if bias is not None:
                s += float(bias[j])
            out[i][j] = max(s, 0.0) if relu else s
    return out


@functools.lru_cache(maxsize=None)
def engine_matrices(frames, kind):
    """The fp32 matrices of engine_shapes: integers, or Gaussians NOT yet rounded (the pack rounds them)."""
    rng = np.random.default_rng([frames, 77, KINDS.index(kind)])
    out = {}
    for name, shape in engine_shapes(frames).items():
        bias = len(shape) == 1
        if kind == "int":
            lim = INT_MAX_ABS ** 2 if bias else INT_MAX_ABS
            out[name] = rng.integers(-lim, lim + 1, shape).astype(np.float32)
        else:
            out[name] = rng.standard_normal(shape).astype(np.float32)
        out[name].setflags(write=False)
    return out


def gather(mat, positions, channels, ps, cs):
    """[positions][channels] of a row-major matrix through the strides vl_pack_kc8 is given."""
    flat = mat.reshape(-1)
    return flat[np.arange(positions)[:, None] * ps + np.arange(channels)[None, :] * cs]


def engine_want(prod, mats):
    """fp64 reference of an engine product: the gathered operands rounded to bf16, multiplied, plus bias, ReLU."""
    a = bf16_round(gather(mats[prod.a[0]], *prod.a[1:]))
    b = bf16_round(gather(mats[prod.b[0]], *prod.b[1:]))
    return epilogue(product(a, b), mats[prod.bias] if prod.bias else None, prod.relu)
