"""The small kernels behind every bias gradient and fusion (csrc/pointwise.hip), each on its own and past its one-launch branch:
vl_colsum and vl_bias_grad_nchw through the workspace and sum_partials_kernel, vl_transpose, vl_temporal_fusion_* over more than one
workgroup and into the grid-stride loop of the backward.  Slice counts are those of tests/gemm_plan.py (pinned in
tests/test_gemm_geometry.py).  The harness is test_gemm_geometry_gpu's: inputs are views into one NaN-filled allocation per test (NaN in
the padding columns, behind the last row, between tensors), outputs views into a sentinel-filled one that must be intact around them,
the workspace NaN before every call with a sentinel guard behind it, every call twice with identical bits.  Sums against fp64 with
test_ops_gpu's `close`; the transpose bit for bit; the fusion against the oracle at test_temporal_fusion's tolerances."""
import numpy as np
import pytest
import torch

from oracle import lrcn_oracle as O
from tests import gemm_plan as P
from tests.test_gemm_geometry_gpu import DEV, GUARD, SENTINEL, Layout, window
from tests.test_ops_gpu import close

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    import vltf_amd.ops as ops_
    return ops_


def intact(got, what):
    assert np.array_equal(got.view(np.uint32), np.full(got.shape, SENTINEL, np.float32).view(np.uint32)), what + ": written outside its output"


def take(got, off, count):
    """The `count` floats at `off` of a downloaded output allocation; the place is reset to the sentinel for intact()."""
    v = got[off:off + count].copy()
    got[off:off + count] = SENTINEL
    return v


class Flags:
    """Device-side verdicts collected during a test and read once at its end."""

    def __init__(self):
        self.flags, self.labels = [], []

    def add(self, flag, label):
        self.flags.append(flag)
        self.labels.append(label)

    def check(self):
        bad = torch.stack(self.flags).cpu().numpy()
        assert not bad.any(), [l for l, f in zip(self.labels, bad) if f]


def poisoned_ws(floats):
    """(workspace of `floats`, guard behind it, arm()): arm() makes the workspace NaN and the guard the sentinel."""
    buf = torch.empty(floats + GUARD, device=DEV)
    ws, guard = buf[:floats], buf[floats:]

    def arm():
        ws.fill_(NAN)
        guard.fill_(SENTINEL)
    return ws, guard, arm


@pytest.mark.parametrize("pad", P.COLSUM_PAD)
def test_colsum(ops, pad):
    """lda = n + pad.  One matrix of 20000 rows per n; m runs downwards and the rows from m on are turned to NaN on the device before
    the call, so every call has NaN behind its last row and in its padding columns.  Up to 256 rows: one launch, the workspace stays
    NaN.  Beyond: 2 slices of 129 rows at m = 257, 64 slices of 256 and of 257 rows at m = 16384 and 16385."""
    rng = np.random.default_rng(pad)
    rows = max(P.COLSUM_M)
    lay_in, lay_out = Layout(), Layout()
    mats = {n: lay_in.place(rows * (n + pad)) for n in P.COLSUM_N}
    outs = {(n, m): (lay_out.place(n), lay_out.place(n)) for n in P.COLSUM_N for m in P.COLSUM_M}
    src = np.full(lay_in.total(), np.nan, np.float32)
    for n, off in mats.items():
        window(src, off, rows, n, n + pad)[...] = rng.standard_normal((rows, n), dtype=np.float32)
    pool = torch.tensor(src, device=DEV)
    out = torch.full((lay_out.total(),), SENTINEL, device=DEV)
    flags = Flags()
    for n, off in mats.items():
        lda = n + pad
        ws, guard, arm = poisoned_ws(64 * n)
        above = rows
        for m in sorted(P.COLSUM_M, reverse=True):
            pool[off + m * lda:off + above * lda].fill_(NAN)
            above = m
            for o in outs[n, m]:
                arm()
                ops.colsum(pool[off:], out[o:], ws, m, n, lda=lda)
                flags.add((guard != SENTINEL).any(), "n=%d m=%d: guard behind 64*n floats written" % (n, m))
                if P.colsum_plan(m)[0] == 1:
                    flags.add((ws == ws).any(), "n=%d m=%d: one slice, yet the workspace was written" % (n, m))
    got = out.cpu().numpy()
    flags.check()
    for n, off in mats.items():
        a = window(src, off, rows, n, n + pad).astype(np.float64)
        for m in P.COLSUM_M:
            first, second = (take(got, o, n) for o in outs[n, m])
            assert first.tobytes() == second.tobytes(), (n, m)
            close(first, a[:m].sum(0), msg="colsum m=%d n=%d lda=%d" % (m, n, n + pad))
    intact(got, "colsum")


def test_bias_grad_nchw(ops):
    """2, 3, 3, 2, 2, 44 and 1 image slices; a slice walks 8 images per pass: 3, 7, 8 + 5, 4 x 8 + 3, 1, 3 (and 1 in the last), 3."""
    rng = np.random.default_rng(1)
    lay_in, lay_out = Layout(), Layout()
    recs = [(n, c, hw, lay_in.place(n * c * hw), (lay_out.place(c), lay_out.place(c))) for n, c, hw in P.BIAS_GRAD]
    src = np.full(lay_in.total(), np.nan, np.float32)
    for n, c, hw, off, _ in recs:
        src[off:off + n * c * hw] = rng.standard_normal(n * c * hw, dtype=np.float32)
    pool = torch.tensor(src, device=DEV)
    out = torch.full((lay_out.total(),), SENTINEL, device=DEV)
    flags = Flags()
    for n, c, hw, off, dbs in recs:
        ws, guard, arm = poisoned_ws(64 * c)
        for o in dbs:
            arm()
            ops.bias_grad_nchw(pool[off:off + n * c * hw].view(n, c, hw), out[o:o + c], ws)
            flags.add((guard != SENTINEL).any(), "%s: guard behind 64*c floats written" % ((n, c, hw),))
            if P.bias_grad_plan(n, hw)[0] == 1:
                flags.add((ws == ws).any(), "%s: one slice, yet the workspace was written" % ((n, c, hw),))
    got = out.cpu().numpy()
    flags.check()
    for n, c, hw, off, dbs in recs:
        first, second = (take(got, o, c) for o in dbs)
        assert first.tobytes() == second.tobytes(), (n, c, hw)
        close(first, src[off:off + n * c * hw].reshape(n, c, hw).astype(np.float64).sum((0, 2)), msg="bias_grad_nchw %s" % ((n, c, hw),))
    intact(got, "bias_grad_nchw")


def test_transpose(ops):
    """One element, one row, one tile exactly, ragged tiles either way, a tall strip; ld = cols and cols + 5.  Bit for bit."""
    rng = np.random.default_rng(2)
    lay_in, lay_out = Layout(), Layout()
    recs = [(r, c, c + pad, lay_in.place(r * (c + pad)), lay_out.place(r * c)) for r, c in P.TRANSPOSE for pad in P.TRANSPOSE_PAD]
    src = np.full(lay_in.total(), np.nan, np.float32)
    for r, c, ld, off, _ in recs:
        window(src, off, r, c, ld)[...] = rng.standard_normal((r, c), dtype=np.float32)
    pool = torch.tensor(src, device=DEV)
    out = torch.full((lay_out.total(),), SENTINEL, device=DEV)
    for r, c, ld, off, o in recs:
        ops.transpose(pool[off:], out[o:], r, c, ld=ld)
    got = out.cpu().numpy()
    for r, c, ld, off, o in recs:
        assert np.array_equal(take(got, o, r * c).reshape(c, r), window(src, off, r, c, ld).T), (r, c, ld)
    intact(got, "transpose")


@pytest.mark.parametrize("method", ["avg", "last"])
def test_temporal_fusion(ops, method):
    """One element, several workgroups, a backward of 64 x 32 x 600 > 4096 x 256 elements (the grid-stride loop), and T = 1.  dx holds
    NaN before the call: every element must be written."""
    rng = np.random.default_rng(5)
    lay_in, lay_out = Layout(), Layout()
    recs = [(b, T, H, lay_in.place(b * T * H), lay_in.place(b * H), lay_out.place(b * H), lay_out.place(b * T * H)) for b, T, H in P.FUSION]
    src = np.full(lay_in.total(), np.nan, np.float32)
    for b, T, H, x, dy, _, _ in recs:
        src[x:x + b * T * H] = rng.standard_normal(b * T * H, dtype=np.float32)
        src[dy:dy + b * H] = rng.standard_normal(b * H, dtype=np.float32)
    pool = torch.tensor(src, device=DEV)
    out = torch.full((lay_out.total(),), SENTINEL, device=DEV)
    for b, T, H, x, dy, y, dx in recs:
        out[dx:dx + b * T * H].fill_(NAN)
        ops.temporal_fusion_fwd(pool[x:], out[y:], b, T, H, method)
        ops.temporal_fusion_bwd(pool[dy:], out[dx:], b, T, H, method)
    got = out.cpu().numpy()
    for b, T, H, x, dy, y, dx in recs:
        xs, dys = src[x:x + b * T * H].reshape(b, T, H).astype(np.float64), src[dy:dy + b * H].reshape(b, H).astype(np.float64)
        close(take(got, y, b * H).reshape(b, H), O.temporal_fusion(xs, method), rtol=1e-6, atol_rel=1e-7, msg="fwd %s" % ((b, T, H),))
        close(take(got, dx, b * T * H).reshape(b, T, H), O.temporal_fusion_grad(xs.shape, method, dys), rtol=1e-6, atol_rel=1e-7,
              msg="bwd %s" % ((b, T, H),))
    intact(got, "temporal_fusion")
