"""The drop launches of the self-attention model (vl_mhsa_drop_fwd / _bwd, vl_add_layer_norm_drop_fwd, vl_branch_drop_grad and their _st
forms) against the fp64 reference of tests/encoder_dropout_ref.py, their bitwise identities, and the engines that run
sa_attn_dropout / sa_dropout / sa_drop_path on them.

Attention cases (of mhsa_ref.CASES): a single key (dropping it gives a zero row), dh = 8 with three heads, dh = 50 with an odd T, a key
on every lane, and T = 64 with dh = 128 (the LDS maximum); each with and without lengths (NaN in the dead rows), at keep 0.5 and 0.9,
positions on and off; the backward FROM the reference's undropped P rounded to fp32.  Add-and-norm and branch gradient: over
encoder_block_ref.LN_CASES at both SCALES, elements only / path only / both (keeps of 0.5: the factors reach 4), with and without
lengths: `sum` and the branch gradient are BIT FOR BIT the fp32 restatement (that is the mask-equality test: no GPU test is
statistical), y and stats against fp64.

Tolerance: class act (3e-5, 3e-5) of tests/test_lstm_geometry_gpu.TOL on every output (stats per column), as
tests/test_encoder_dropout.py::test_float32_decides_the_class_of_the_gpu_tests decides on these very inputs: the plain float32
restatement stays below 0.02 of it (the factors scale value and error alike).  The engine cases run at the tolerances of
tests/test_encoder_block_gpu.py / tests/test_self_attention_gpu.py."""
import os

import numpy as np
import pytest
import torch

from tests import encoder_block_ref as E
from tests import encoder_dropout_ref as D
from tests import lstm_plan as LP
from tests import mhsa_ref as M
from tests.test_encoder_dropout import ATTN_CASES, CLIP0, KEEPS, LN_OPTIONS, SALT_E, SALT_P, SALT_W, SEED, attn_reference, ln_reference
from tests.test_lstm_geometry_gpu import DEV, Guarded, put, same_bits, within
from tests.test_self_attention_gpu import MEAN, shapes

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
STEP = 5                                                             # SEED = seed_of(5): the _st forms get a state of this step


@pytest.fixture(scope="module")
def ops():
    import vltf_amd.ops as ops_
    return ops_


def state_of(ops, step):
    st = ops.step_state(DEV)
    ops.step_state_set(st, step, 0.01, 0)
    return st


def nan_dead(a, T, lens):
    return a if lens is None else M.with_nan_in_dead_rows(a, T, lens)


def run_attn(ops, case, inp, lens, P32, keep, positions=True, what="", clip0=CLIP0, seed=SEED, state=None, plain=False):
    """mhsa_drop_fwd on the inputs, mhsa_drop_bwd on the P given, NaN in the dead rows; the memory checks; -> {output: array}.
    plain: the launches without dropout."""
    batch, T, H, heads = case
    qkv, dctx = put(nan_dead(inp.qkv, T, lens), DEV), put(nan_dead(inp.dctx, T, lens), DEV)
    pos = put(inp.pos, DEV) if positions else None
    L = put(lens, DEV, torch.int32)
    o = {k: Guarded(shp, DEV) for k, shp in shapes(case, positions).items()}
    dposp = o["dposp"].t if positions else None
    if plain:
        ops.mhsa_fwd(qkv, pos, o["P"].t, o["ctx"].t, batch, T, H, heads, seq_len=L)
        ops.mhsa_bwd(dctx, qkv, put(P32, DEV), o["dqkv"].t, dposp, batch, T, H, heads, seq_len=L)
    else:
        kw = dict(keep=float(keep), salt=SALT_W, clip0=clip0, seq_len=L, **(dict(state=state) if state is not None else dict(seed=seed)))
        ops.mhsa_drop_fwd(qkv, pos, o["P"].t, o["ctx"].t, batch, T, H, heads, **kw)
        ops.mhsa_drop_bwd(dctx, qkv, put(P32, DEV), o["dqkv"].t, dposp, batch, T, H, heads, **kw)
    return {k: g.settle(what + " " + k) for k, g in o.items()}


def run_ln(ops, case, inp, lens, keep, keep_path, what="", branch=1, clip0=CLIP0, seed=SEED, state=None, plain=False, shift=0):
    """add_layer_norm_drop_fwd on x, r and branch_drop_grad on dy, NaN in the dead rows; -> {sum, y, stats, dr}.  plain: the launch
    without dropout (and dr = the live rows of dy).  shift: r, dy and dr sit that many floats off a 16-byte boundary."""
    clips, T, W = case
    x, r, dy = (put(nan_dead(a, T, lens), DEV) for a in (inp.x, inp.r, inp.dy))
    gamma, beta = put(inp.gamma, DEV), put(inp.beta, DEV)
    L = put(lens, DEV, torch.int32)
    rows = clips * T
    o = dict(sum=Guarded((rows, W), DEV), y=Guarded((rows, W), DEV), stats=Guarded((rows, 2), DEV))
    big = torch.full((rows * W + 2 * 64 + shift,), 12345.0, device=DEV)
    dr = big[64 + shift:64 + shift + rows * W].view(rows, W)
    dr.fill_(float("nan"))
    if shift:
        off = lambda t: torch.cat([torch.zeros(shift, device=DEV), t.reshape(-1)])[shift:].view(rows, W)
        r, dy = off(r), off(dy)
        assert r.data_ptr() % 16 == 4 * shift == dr.data_ptr() % 16 == dy.data_ptr() % 16
    if plain:
        ops.add_layer_norm_fwd(x, r, o["sum"].t, o["y"].t, gamma, beta, o["stats"].t, clips, T, W, seq_len=L)
        if L is None:
            dr.copy_(dy)
        else:
            ops.live_rows(dy, dr, clips, T, W, L)
    else:
        kw = dict(keep=float(keep), keep_path=float(keep_path), salt_elem=SALT_E, salt_path=SALT_P, branch=branch, clip0=clip0, seq_len=L,
                  **(dict(state=state) if state is not None else dict(seed=seed)))
        ops.add_layer_norm_drop_fwd(x, r, o["sum"].t, o["y"].t, gamma, beta, o["stats"].t, clips, T, W, **kw)
        ops.branch_drop_grad(dy, dr, clips, T, W, **kw)
    out = {k: g.settle(what + " " + k) for k, g in o.items()}
    flat = big.cpu().numpy()
    assert (flat[:64 + shift] == 12345.0).all() and (flat[64 + shift + rows * W:] == 12345.0).all(), what + ": guard around dr written"
    out["dr"] = flat[64 + shift:64 + shift + rows * W].reshape(rows, W)
    assert np.isfinite(out["dr"]).all(), what + ": element of dr not written"
    return out


# ---- 1. the launches against the reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("case", ATTN_CASES, ids=M.case_id)
def test_dropped_attention_against_the_reference(ops, case, keep, lens):
    batch, T, H, heads = case
    for positions in (True, False):
        what = "mhsa drop %s keep %s %s %s" % (M.case_id(case), keep, "lens" if lens else "full", "pos" if positions else "no pos")
        ref = attn_reference(case, keep, lens, positions)
        got = run_attn(ops, case, ref["inp"], ref["lens"], ref["P32"], keep, positions, what)
        want = dict(ref["fwd"]._asdict(), **ref["bwd"]._asdict())
        for name in got:
            within("act", got[name], want[name], what + " " + name)
        live = M.live_mask(ref["lens"], batch, T)
        sums = got["P"].astype(F64).sum(axis=3)                                  # P is stored undropped: its live rows sum to 1
        np.testing.assert_allclose(sums, np.broadcast_to(live[:, None, :], sums.shape).astype(F64), rtol=0, atol=2e-6)
        if lens:
            dead = ~live.reshape(-1)
            for name in ("ctx", "dqkv"):
                assert not got[name][dead].any(), "%s: dead row of %s not zero" % (what, name)
    if T == 1:                                                                   # a single key: dropping it gives a zero row of ctx
        Fw = D.weight_factor(SEED, SALT_W, batch, heads, T, 0.5, CLIP0)
        ctx = run_attn(ops, case, ref["inp"], None, ref["P32"], 0.5, what="single key")["ctx"]
        v = ref["inp"].qkv[:, 2 * H:]
        assert np.array_equal(ctx, (v * F32(Fw.reshape(-1)[0])).astype(F32))


@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
@pytest.mark.parametrize("scale", E.SCALES, ids=lambda k: "k%d" % k)
@pytest.mark.parametrize("case", E.LN_CASES, ids=E.case_id)
def test_dropped_add_norm_and_branch_gradient(ops, case, scale, lens):
    """sum and the branch gradient bit for bit the fp32 restatement (mask equality); y and stats against fp64 at class act."""
    clips, T, W = case
    for option in sorted(LN_OPTIONS):
        what = "add norm drop %s k%d %s %s" % (E.case_id(case), scale, "lens" if lens else "full", option)
        ref = ln_reference(case, scale, lens, option)
        got = run_ln(ops, case, ref["inp"], ref["lens"], ref["keep"], ref["keep_path"], what)
        same_bits(dict(sum=got["sum"], dr=got["dr"]), dict(sum=ref["sum32"], dr=ref["dr32"]), what)
        fwd = ref["fwd"]
        within("act", got["y"], fwd.y, what + " y")
        within("act", got["sum"], fwd.sum, what + " sum")
        within("act", got["stats"][:, 0], fwd.stats[:, 0], what + " mean")
        within("act", got["stats"][:, 1], fwd.stats[:, 1], what + " rstd")
        if lens and clips > 1:
            dead = ~M.live_mask(ref["lens"], clips, T).reshape(-1)
            assert dead.any() and all(not got[k][dead].any() for k in ("sum", "y", "stats", "dr")), what + ": dead row not zero"
    other = ln_reference(case, scale, lens, "all", branch=0)                     # the other branch of the layer draws its own path
    got0 = run_ln(ops, case, other["inp"], other["lens"], 0.5, 0.5, "branch 0", branch=0)
    same_bits(dict(sum=got0["sum"], dr=got0["dr"]), dict(sum=other["sum32"], dr=other["dr32"]), "branch 0")


# ---- 2. bitwise identities ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
def test_keep_one_is_the_existing_launch(ops, lens):
    for case in ((3, 2, 24, 3), (2, 21, 250, 5), (5, 16, 256, 4)):
        ref = M.reference(case, 1, lens)
        same_bits(run_attn(ops, case, ref.inp, ref.lens, ref.P32, 1.0, what="mhsa drop, keep 1"),
                  run_attn(ops, case, ref.inp, ref.lens, ref.P32, 1.0, what="mhsa", plain=True), "mhsa %s: keep 1" % (case,))
    for case in ((21, 5, 250), (16, 4, 256), (7, 4, 72), (2, 64, 1024)):
        ref = E.ln_reference(case, 40, lens)
        same_bits(run_ln(ops, case, ref.inp, ref.lens, 1.0, 1.0, "add norm drop, keeps 1"),
                  run_ln(ops, case, ref.inp, ref.lens, 1.0, 1.0, "add norm", plain=True), "add norm %s: keeps 1" % (case,))


def test_seed_form_is_the_st_form_and_runs_repeat(ops):
    st = state_of(ops, STEP)
    case = (3, 7, 96, 3)
    ref = M.reference(case, 1, True)
    a = run_attn(ops, case, ref.inp, ref.lens, ref.P32, 0.5, what="mhsa drop")
    same_bits(run_attn(ops, case, ref.inp, ref.lens, ref.P32, 0.5, what="mhsa drop again"), a, "mhsa drop: a second run")
    same_bits(run_attn(ops, case, ref.inp, ref.lens, ref.P32, 0.5, what="mhsa drop st", state=st), a, "mhsa drop: _st form")
    b = run_attn(ops, case, ref.inp, ref.lens, ref.P32, 0.5, what="mhsa drop next", state=state_of(ops, STEP + 1))
    assert not np.array_equal(a["ctx"], b["ctx"]) and np.array_equal(a["P"], b["P"])           # another step: other masks, the same P
    for lncase in ((5, 6, 256), (5, 6, 65)):
        lref = E.ln_reference(lncase, 40, True)
        c = run_ln(ops, lncase, lref.inp, lref.lens, 0.5, 0.5, "add norm drop")
        same_bits(run_ln(ops, lncase, lref.inp, lref.lens, 0.5, 0.5, "add norm drop again"), c, "add norm drop: a second run")
        same_bits(run_ln(ops, lncase, lref.inp, lref.lens, 0.5, 0.5, "add norm drop st", state=st), c, "add norm drop: _st form")
        d = run_ln(ops, lncase, lref.inp, lref.lens, 0.5, 0.5, "add norm drop next", state=state_of(ops, STEP + 1))
        assert not np.array_equal(c["sum"], d["sum"]) and not np.array_equal(c["dr"], d["dr"])


def test_the_bits_do_not_depend_on_the_alignment_of_a_pointer(ops):
    for case in ((3, 5, 72), (3, 5, 65), (2, 3, 1024)):
        ref = E.ln_reference(case, 40, True)
        same_bits(run_ln(ops, case, ref.inp, ref.lens, 0.5, 0.5, "off by 4 bytes", shift=1), run_ln(ops, case, ref.inp, ref.lens, 0.5, 0.5, "aligned"),
                  "add norm drop %s: r, ds and dr off a 16-byte boundary" % (case,))
        same_bits(run_ln(ops, case, ref.inp, ref.lens, 0.5, 0.5, "off by 12 bytes", shift=3), run_ln(ops, case, ref.inp, ref.lens, 0.5, 0.5, "aligned"),
                  "add norm drop %s: off by 12 bytes" % (case,))


@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
def test_clips_two_and_three_alone_with_clip0_two_are_those_clips_in_the_batch(ops, lens):
    """The counters are those of the global batch: what a rank that holds clips [2, 4) draws is what one launch over [0, 4) draws for
    them (the two-rank step rests on this)."""
    case = batch, T, H, heads = (4, 7, 96, 3)
    ref = M.reference(case, 1, lens)
    whole = run_attn(ops, case, ref.inp, ref.lens, ref.P32, 0.5, what="mhsa drop 0..4", clip0=0)
    rows, clip = slice(2 * T, 4 * T), slice(2, 4)
    part_in = M.Inputs(ref.inp.qkv[rows], ref.inp.pos, ref.inp.dctx[rows])
    part = run_attn(ops, (2, T, H, heads), part_in, None if ref.lens is None else ref.lens[clip], ref.P32[clip], 0.5, what="mhsa drop 2..4", clip0=2)
    same_bits(part, {k: v[clip] if v.shape[0] == batch else v[rows] for k, v in whole.items()}, "mhsa drop: clips 2..4 with clip0 2")
    moved = run_attn(ops, (2, T, H, heads), part_in, None if ref.lens is None else ref.lens[clip], ref.P32[clip], 0.5, what="clip0 0", clip0=0)
    assert not np.array_equal(moved["ctx"], part["ctx"])
    for lncase in ((4, 6, 256), (4, 6, 65)):
        clips, T2, W = lncase
        lref = E.ln_reference(lncase, 40, lens)
        whole = run_ln(ops, lncase, lref.inp, lref.lens, 0.5, 0.5, "add norm drop 0..4", clip0=0)
        rows = slice(2 * T2, 4 * T2)
        one = lref.inp._replace(x=lref.inp.x[rows], r=lref.inp.r[rows], dy=lref.inp.dy[rows], dres=lref.inp.dres[rows])
        part = run_ln(ops, (2, T2, W), one, None if lref.lens is None else lref.lens[2:4], 0.5, 0.5, "add norm drop 2..4", clip0=2)
        same_bits(part, {k: v[rows] for k, v in whole.items()}, "add norm drop %s: clips 2..4 with clip0 2" % (lncase,))


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ops):
    """keep outside (0, 1], NaN, null pointers, clip0 out of range: through ops (which refuses first) and straight through the C entry
    points, seed and _st forms; nothing is launched."""
    from vltf_amd import _ffi
    batch, T, H, heads, W = 2, 3, 16, 2, 16
    z = lambda *shape: torch.zeros(shape, device=DEV)
    qkv, x, gam, st = z(batch * T, 3 * H), z(batch * T, W), z(W), state_of(ops, 1)
    o = dict(P=Guarded((batch, heads, T, T), DEV), ctx=Guarded((batch * T, H), DEV), dqkv=Guarded((batch * T, 3 * H), DEV),
             sum=Guarded((batch * T, W), DEV), y=Guarded((batch * T, W), DEV), stats=Guarded((batch * T, 2), DEV), dr=Guarded((batch * T, W), DEV))
    p = lambda t: None if t is None else t.data_ptr()
    s = ops.stream

    def c_calls(keep=0.5, keep_path=0.5, clip0=0, qkv_=qkv, x_=x, state=st, branch=0):
        for sfx, sd in (("", 7), ("_st", p(state))):
            yield lambda: _ffi.call("vl_mhsa_drop_fwd" + sfx, p(qkv_), None, None, p(o["P"].t), p(o["ctx"].t), batch, T, H, heads, keep, sd, 1, clip0, s())
            yield lambda: _ffi.call("vl_mhsa_drop_bwd" + sfx, p(x_), p(qkv_), p(o["P"].t), None, p(o["dqkv"].t), None, batch, T, H, heads, keep, sd,
                                    1, clip0, s())
            yield lambda: _ffi.call("vl_add_layer_norm_drop_fwd" + sfx, p(x_), p(x_), p(o["sum"].t), p(o["y"].t), p(gam), p(gam), p(o["stats"].t),
                                    batch, T, W, 1e-5, None, keep, keep_path, sd, 1, 3, branch, clip0, s())
            yield lambda: _ffi.call("vl_branch_drop_grad" + sfx, p(x_), p(o["dr"].t), batch, T, W, None, keep, keep_path, sd, 1, 3, branch, clip0, s())
    n = 0
    for kw, match in ((dict(keep=0.0), "keep"), (dict(keep=-0.25), "keep"), (dict(keep=1.5), "keep"), (dict(keep=float("nan")), "keep"),
                      (dict(clip0=-1), "clip0"), (dict(clip0=1 << 31), "clip0"), (dict(qkv_=None, x_=None), "null pointer")):
        for call in c_calls(**kw):
            with pytest.raises(Exception, match=match):
                call()
            n += 1
    for kw, match in ((dict(keep_path=0.0), "keep_path"), (dict(keep_path=float("nan")), "keep_path"), (dict(keep_path=1.25), "keep_path"),
                      (dict(branch=2), "branch")):
        for call in list(c_calls(**kw))[2:4] + list(c_calls(**kw))[6:8]:
            with pytest.raises(Exception, match=match):
                call()
            n += 1
    for call in list(c_calls(state=None))[4:]:
        with pytest.raises(Exception, match="null pointer"):
            call()
        n += 1
    assert n == 7 * 8 + 4 * 4 + 4
    for keep in (0.0, 1.0001, float("nan"), True, "0.5"):                           # ops refuses first
        with pytest.raises(Exception, match="must lie in"):
            ops.mhsa_drop_fwd(qkv, None, o["P"].t, o["ctx"].t, batch, T, H, heads, keep, 1, seed=7)
        with pytest.raises(Exception, match="must lie in"):
            ops.branch_drop_grad(x, o["dr"].t, batch, T, W, 0.5, keep, 1, 3, 0, seed=7)
    with pytest.raises(Exception, match="one of the two"):
        ops.mhsa_drop_bwd(x, qkv, o["P"].t, o["dqkv"].t, None, batch, T, H, heads, 0.5, 1)
    with pytest.raises(Exception, match="one of the two"):
        ops.add_layer_norm_drop_fwd(x, x, o["sum"].t, o["y"].t, gam, gam, o["stats"].t, batch, T, W, 0.5, 0.5, 1, 3, 0, seed=7, state=st)
    with pytest.raises(Exception, match="elements"):
        ops.branch_drop_grad(x, z(batch * T * W - 1), batch, T, W, 0.5, 0.5, 1, 3, 0, seed=7)
    with pytest.raises(Exception, match="clip0"):
        ops.mhsa_drop_fwd(qkv, None, o["P"].t, o["ctx"].t, batch, T, H, heads, 0.5, 1, clip0=-2, seed=7)
    torch.cuda.synchronize()
    assert all(g.untouched() for g in o.values()), "refused, yet an output was written"
    for call in c_calls():                                                          # (the arguments are good otherwise)
        call()
    torch.cuda.synchronize()
    assert not any(g.untouched() for g in o.values())


# ---- 4. LRCNEngine -----------------------------------------------------------------------------------------------------------------------
SHAPE, NCLS, FPC, CLIPS = (67, 67, 3), 7, 3, 2                                  # the geometry of tests/test_encoder_block_gpu.py
RATES = dict(sa_attn_dropout=0.3, sa_dropout=0.25, sa_drop_path=0.3)


def lrcn_case(H, heads, layers, F, fusion, block, seed):
    from vltf_amd.engine import NetConfig
    rng = np.random.default_rng(seed)
    rates = RATES if block == "encoder" else dict(sa_attn_dropout=0.3)
    kw = dict(image_shape=SHAPE, num_classes=NCLS, fpc=FPC, frame_encoding_layer="fc6", lstm_hidden=H, lstm_layers=layers, fusion=fusion,
              rnn_cell="mhsa", sa_heads=heads)
    if block == "encoder":
        kw.update(sa_block="encoder", sa_ffn_dim=F)
        p = E.init_params(rng, NCLS, "fc6", H, layers, SHAPE, heads, FPC, F)
    else:
        p = M.init_params(rng, NCLS, "fc6", H, layers, SHAPE, heads, FPC)
    frames = M.varied_frames(rng, CLIPS, FPC, SHAPE)
    onehot = np.eye(NCLS, dtype=np.int32)[rng.integers(0, NCLS, CLIPS)]
    if block != "encoder":
        M.tame_first_layer(p, frames.astype(np.float32) - MEAN, "fc6")
    return NetConfig(**kw), NetConfig(**kw, **rates), p, frames, onehot, rates


@pytest.mark.parametrize("H,heads,layers,F,fusion,block,seed", [(16, 2, 1, 32, "avg", "encoder", 7), (8, 1, 2, 8, "last", "encoder", 6),
                                                                 (16, 2, 1, None, "avg", "plain", 6)])
def test_lrcn_engine_train_step_against_the_reference(H, heads, layers, F, fusion, block, seed):
    """Two consecutive steps with every applicable option on against encoder_dropout_ref.model_train_step with the masks of draw index
    0 and 1, at the tolerances of tests/test_encoder_block_gpu.py (tests/test_self_attention_gpu.py for the plain model: the same
    figures).  The second step holds only with the masks of ITS seed; a forward-only call afterwards is the model without dropout, bit
    for bit; self_attention_weights() stays the undropped P."""
    from vltf_amd.engine import LRCNEngine, param_specs
    cfg0, cfg, p, frames, onehot, rates = lrcn_case(H, heads, layers, F, fusion, block, seed)
    assert param_specs(cfg) == param_specs(cfg0)
    eng = LRCNEngine(cfg, max_clips=CLIPS, device=DEV)
    eng.load_params(p)
    x = frames.astype(np.float32) - MEAN
    fd, ld = torch.tensor(frames, device=DEV), torch.tensor(onehot, device=DEV)
    losses = []
    for step in range(2):
        dr = D.drop(rates.get("sa_attn_dropout"), rates.get("sa_dropout"), rates.get("sa_drop_path"), seed=D.seed_of(step), layers=layers)
        newp, loss, gn, logits, grads, P = D.model_train_step(p, x, onehot, FPC, 0.01, 0.5, "fc6", H, layers, heads, fusion, dr, block)
        out = eng.train_step_u8(fd, ld, lr=0.01, clip_norm=0.5, mean_bgr=MEAN)
        np.testing.assert_allclose(eng.logits_host(), logits, rtol=1e-3, atol=1e-3)
        assert abs(out["loss"] - loss) < 1e-4 * max(1, abs(loss)), (step, out["loss"], loss)
        assert abs(out["grad_norm"] - gn) < 1e-3 * gn
        got_P = eng.self_attention_weights().cpu().numpy()
        np.testing.assert_allclose(got_P, P, rtol=1e-3, atol=1e-3)
        np.testing.assert_allclose(got_P.astype(F64).sum(axis=3), 1.0, rtol=0, atol=1e-6)      # undropped: rows sum to 1
        g = eng.get_grads()
        for k in p:
            scale = np.abs(grads[k]).max() + 1e-12
            np.testing.assert_allclose(g[k], grads[k], rtol=2e-3, atol=2e-4 * scale, err_msg="step %d grad %s" % (step, k))
        got = eng.get_params()
        for k in p:
            np.testing.assert_allclose(got[k], newp[k], rtol=1e-4, atol=1e-5, err_msg="step %d param %s" % (step, k))
        if step == 1:                                                            # the masks of step 0 on the same parameters: another loss
            stale = D.model_train_step(p, x, onehot, FPC, 0.01, 0.5, "fc6", H, layers, heads, fusion, dr._replace(seed=D.seed_of(0)), block)[1]
            assert abs(stale - loss) > 1e-3 * max(1, abs(loss)), "the two steps' masks give the same loss: the test cannot tell them apart"
        losses.append(loss)
        p = got                                                                  # the next step starts from what the device holds
    clean = LRCNEngine(cfg0, max_clips=CLIPS, device=DEV, training=False)
    clean.load_params(p)
    assert torch.equal(eng.forward_u8(fd, MEAN), clean.forward_u8(fd, MEAN)), "a forward-only call dropped something"
    assert torch.equal(eng.self_attention_weights(), clean.self_attention_weights())


@pytest.mark.parametrize("block", ("encoder", "plain"))
def test_rates_of_zero_are_the_engine_without_the_keys(block):
    from vltf_amd.engine import LRCNEngine, NetConfig
    cfg0, _, p, frames, onehot, rates = lrcn_case(16, 2, 2 if block == "encoder" else 1, 32, "avg", block, 6)
    zero = NetConfig(**dict(vars(cfg0), **{k: 0.0 for k in rates}))
    fd, ld = torch.tensor(frames, device=DEV), torch.tensor(onehot, device=DEV)
    res = []
    for cfg in (cfg0, zero):
        eng = LRCNEngine(cfg, max_clips=CLIPS, device=DEV)
        eng.load_params(p)
        assert eng.sa_drop is None and all("do" not in S for S in eng.mhsa)
        outs = [eng.train_step_u8(fd, ld, lr=0.01, clip_norm=0.5, mean_bgr=MEAN) for _ in range(2)]
        res.append((outs, eng.logits_host(), eng.get_params()))
    for a, b in zip(res[0][0], res[1][0]):
        assert (a["loss"], a["grad_norm"]) == (b["loss"], b["grad_norm"])
    assert np.array_equal(res[0][1], res[1][1])
    for k in res[0][2]:
        assert np.array_equal(res[0][2][k], res[1][2][k]), k


def test_lrcn_engine_captured_step_is_the_eager_step():
    """step_graph with the three options (and the head's dropout): the warm-up step, the captured one and three replays equal the eager
    engine's bit for bit -- the _st forms draw each replay's masks from the step state, as the eager launches do from the seed."""
    from vltf_amd.engine import LRCNEngine, NetConfig, init_params
    kw = dict(image_shape=SHAPE, num_classes=NCLS, fpc=FPC, frame_encoding_layer="fc6", lstm_hidden=16, lstm_layers=2, fusion="avg",
              rnn_cell="mhsa", sa_heads=2, sa_block="encoder", sa_ffn_dim=24, dropout_keep_prob=0.5, **RATES)
    params = init_params(NetConfig(**kw), seed=4, well_scaled=True)
    rng = np.random.default_rng(11)
    engines = []
    for sg in (False, True):
        e = LRCNEngine(NetConfig(step_graph=sg, **kw), max_clips=CLIPS, device=DEV)
        e.load_params(params)
        engines.append(e)
    frames = torch.from_numpy(rng.integers(0, 256, (CLIPS * FPC,) + SHAPE, dtype=np.uint8)).to(DEV)
    onehot = torch.from_numpy(np.eye(NCLS, dtype=np.int32)[rng.integers(0, NCLS, CLIPS)]).to(DEV)
    seen = []
    for step in range(5):                                                        # the SAME batch every step: only the masks change
        outs = [e.train_step_u8(frames, onehot, 0.0, 5.0, MEAN) for e in engines]
        for k in ("loss_sum", "correct", "grad_norm", "rows"):
            assert outs[0][k] == outs[1][k], (step, k, outs[0][k], outs[1][k])
        assert np.array_equal(engines[0].logits_host(), engines[1].logits_host()), step
        assert torch.equal(engines[0].self_attention_weights(), engines[1].self_attention_weights()), step
        seen.append(outs[1]["loss_sum"])
    assert len(engines[1]._graphs) == 1
    assert len(set(seen)) == 5, "lr 0 and one batch, yet a replay repeated a loss: it did not draw fresh masks"
    pa, pb = engines[0].get_params(), engines[1].get_params()
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), k


# ---- 5. GraphEngine ------------------------------------------------------------------------------------------------------------------------
G_DIM, G_H, G_HEADS, G_F, G_C, G_CLIPS = 10, 16, 2, 24, 5, 4


def graph_engine(T, layers=2, fusion="avg", seed=3):
    from vltf_amd.graph import DatasetInfo, GraphEngine, PipelineSpec, init_params_for, model_specs
    pipes = [PipelineSpec("net", ["main"], "nop", classifier="lstm", lstm_params=(G_H, layers, fusion), rnn_cell="mhsa", sa_heads=G_HEADS,
                          sa_block="encoder", sa_ffn_dim=G_F, **RATES)]
    ds = {"main": DatasetInfo("vectors", T, 1, G_CLIPS, dim=G_DIM)}
    eng = GraphEngine(pipes, ds, G_C, device=DEV)
    p = init_params_for(model_specs(pipes, ds, G_C), seed=seed, well_scaled=True)
    for k in p:
        if k.endswith(("bias", "beta", "gamma")):
            p[k] = (p[k] + 0.1 * np.random.default_rng(len(k)).standard_normal(p[k].shape)).astype(np.float32)
    eng.load_params(p)
    return eng, p


def test_graph_engine_with_lengths_against_the_reference_and_padding_is_inert():
    """A vector-input pipeline with lengths and the three options: the step against the reference with the masks of node salt 1 (1 + the
    node's index) and draw index 0; NaN in the padded frames changes no bit."""
    from oracle import lrcn_oracle as O
    from tests import gru_ref
    T, lens = 5, np.array([5, 2, 1, 4])
    x = (np.random.default_rng(8).standard_normal((G_CLIPS * T, G_DIM))).astype(np.float32)
    onehot = np.eye(G_C, dtype=np.int32)[np.random.default_rng(9).integers(0, G_C, G_CLIPS)]
    res = []
    for fill in (None, "nan"):
        eng, p = graph_engine(T)
        fed = x.copy()
        if fill:
            fed[~M.live_mask(lens, G_CLIPS, T).reshape(-1)] = np.nan
        out = eng.train_step({"main": torch.from_numpy(fed).to(DEV)}, torch.from_numpy(onehot).to(DEV), lr=0.01, clip_norm=0.0, seq_len={"net": lens})
        res.append((out["loss"], eng.get_grads(), eng.get_params()))
    dr = D.drop(RATES["sa_attn_dropout"], RATES["sa_dropout"], RATES["sa_drop_path"], seed=D.seed_of(0), node=1, layers=2)
    outr, cache = D.stack_forward(x, p, T, 2, G_HEADS, dr, lens)
    fused = gru_ref.fuse(outr, T, G_H, "avg", lens)
    want = fused @ p["output_fc_w"].astype(F64) + p["output_fc_b"]
    loss, d = O.softmax_xent_mean(want, onehot, F64)
    grads = {"output_fc_w": fused.T @ d, "output_fc_b": d.sum(0)}
    grads.update(D.stack_backward(gru_ref.fuse_backward(d @ p["output_fc_w"].astype(F64).T, T, G_H, "avg", lens), cache)[1])
    plain_loss = O.softmax_xent_mean(gru_ref.fuse(E.stack_forward(x, p, T, 2, G_HEADS, lens)[0], T, G_H, "avg", lens)
                                     @ p["output_fc_w"].astype(F64) + p["output_fc_b"], onehot, F64)[0]
    assert abs(plain_loss - loss) > 1e-3                                         # (the options matter to this loss)
    got_loss, g, _ = res[0]
    assert abs(got_loss - loss) < 1e-4 * max(1, abs(loss)), (got_loss, loss)
    assert set(g) == set(grads)
    for k in grads:
        scale = np.abs(grads[k]).max() + 1e-12
        np.testing.assert_allclose(g[k], grads[k], rtol=2e-3, atol=2e-4 * scale, err_msg="grad " + k)
    assert res[0][0] == res[1][0] and np.isfinite(res[1][0])
    for k in res[0][2]:
        assert np.isfinite(res[1][2][k]).all() and np.array_equal(res[0][2][k], res[1][2][k]), "parameter %s moved with the padding" % k


# ---- 6. two ranks ------------------------------------------------------------------------------------------------------------------------
def dp_worker(rank, world, port, q):
    """tests/test_encoder_block_gpu.dp_worker with the three options on (that worker builds its config inside, so it cannot be reused as
    it stands): both ranks on cuda:0 over gloo, each on its half of the clips, against one engine on all of them.  Rank 1 draws with
    clip0 = 2: the masks of the global batch's clips 2 and 3."""
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from vltf_amd import dp
    from vltf_amd.engine import LRCNEngine, NetConfig
    r, w, _ = dp.init_from_env(backend="gloo")
    assert (r, w) == (rank, world)
    shape, ncls, fpc, clips, hid, heads, ffn = (67, 67, 3), 5, 2, 4, 16, 2, 32
    cfg = NetConfig(image_shape=shape, num_classes=ncls, fpc=fpc, lstm_hidden=hid, fusion="avg", rnn_cell="mhsa", sa_heads=heads,
                    sa_block="encoder", sa_ffn_dim=ffn, **RATES)
    rng = np.random.default_rng(11)                                  # identical on every rank
    p = E.init_params(rng, ncls, "fc6", hid, 1, shape, heads, fpc, ffn)
    frames = M.varied_frames(rng, clips, fpc, shape)
    onehot = np.eye(ncls, dtype=np.int32)[rng.integers(0, ncls, clips)]
    CLIP = 1e4                                                       # above the global norm: the updates stay at lr x gradient
    lo, hi = dp.shard_range(clips, rank, world)
    gar = dp.GradAllReduce()
    eng = LRCNEngine(cfg, max_clips=hi - lo, device="cuda:0", dp=gar)
    eng.load_params(p)
    gar.broadcast_params(eng.w)
    out = eng.train_step_u8(torch.tensor(frames[lo * fpc:hi * fpc], device="cuda:0"), torch.tensor(onehot[lo:hi], device="cuda:0"),
                            lr=0.05, clip_norm=CLIP, mean_bgr=MEAN)
    got = eng.get_params()
    if rank == 0:
        ref = LRCNEngine(cfg, max_clips=clips, device="cuda:0")       # one engine, all the clips
        ref.load_params(p)
        want_out = ref.train_step_u8(torch.tensor(frames, device="cuda:0"), torch.tensor(onehot, device="cuda:0"), lr=0.05,
                                     clip_norm=CLIP, mean_bgr=MEAN)
        want = ref.get_params()
        err = {k: float(np.abs(got[k] - want[k]).max() / (np.abs(want[k] - p[k]).max() + 1e-12)) for k in want}
        q.put(("ok", max(err.values()), abs(out["grad_norm"] - want_out["grad_norm"]) / want_out["grad_norm"]))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_rank_step_equals_one_rank():
    """tests/test_encoder_block_gpu.test_two_rank_step_equals_one_rank with sa_attn_dropout, sa_dropout and sa_drop_path on, at its
    tolerance: the global counters make a clip's masks the same on whichever rank holds it."""
    import torch.multiprocessing as mp
    from tests.test_self_attention_gpu import free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    for pr in procs:
        pr.join(300)
        assert pr.exitcode == 0, "rank exited with %s" % pr.exitcode
    tag, worst, gn_err = q.get(timeout=10)
    assert tag == "ok"
    assert worst < 1e-3 and gn_err < 1e-5, (worst, gn_err)


# ---- 7. run_task.py on examples/lrcn_encoder_dropout.yml ---------------------------------------------------------------------------------
def test_run_task_on_the_example_trains_validates_and_resumes(tmp_path, monkeypatch):
    """examples/lrcn_encoder_dropout.yml pointed at the synthetic dataset, in the pattern of the encoder block's test: two epochs of
    three steps with a checkpoint each, a validation of the last, and a second training run that resumes from the first checkpoint and
    ends with exactly the weights of the uninterrupted run -- the resumed run continues the mask sequence."""
    import glob
    import yaml
    from tests.test_host_workflow import make_dataset
    from tests.test_run_task_gpu import RAW, WANT
    from vltf_amd import run_task
    monkeypatch.setenv("VLTF_PREFETCH", "0")
    monkeypatch.setenv("VLTF_CONV_MATH", "f32")
    folder = str(tmp_path)
    train_path, _, _ = make_dataset(folder, "train.txt", shape=RAW, seed=1)
    val_path, _, _ = make_dataset(folder, "val.txt", nvid=3, cpv=(2, 1, 2), shape=RAW, seed=2)
    run = os.path.join(folder, "run")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def cfg(name, data_path, phase, resume=None):
        with open(os.path.join(root, "examples", "lrcn_encoder_dropout.yml")) as f:
            c = yaml.safe_load(f)
        r = c["run"]
        r.update(resume_file=resume, run_folder=run, phase="defs.phase.%s" % phase)
        d = r["data"].pop("train_set")
        d.update(data_path=data_path, phase="defs.phase.%s" % phase, raw_image_shape=str(RAW), image_shape=str(WANT),
                 imgproc=["defs.imgproc.center_crop", "defs.imgproc.sub_mean"])
        r["data"]["d"] = d
        r["network"]["num_classes"] = 4
        pipe = r["network"]["pipelines"][0]["lrcn"]
        assert (pipe["sa_block"], pipe["sa_attn_dropout"], pipe["sa_dropout"], pipe["sa_drop_path"]) == ("encoder", 0.1, 0.1, 0.1)
        pipe["lstm_params"] = [16, 2, "defs.fusion_method.avg"]
        pipe.update(sa_heads=2, sa_ffn_dim=32, sa_attn_dropout=0.3, sa_dropout=0.3, sa_drop_path=0.3)
        r["train"].update(batch_size=2, epochs=2, base_lr=1e-2, lr_decay=["defs.decay.exp", "defs.periodicity.interval", 2, 0.9], clip_norm=5)
        r["val"]["batch_size"] = 2
        path = os.path.join(folder, name)
        with open(path, "w") as f:
            yaml.safe_dump(c, f)
        return path

    def checkpoints():
        return sorted(glob.glob(os.path.join(run, "checkpoints", "*.weights.npz")), key=os.path.getmtime)

    run_task.main(cfg("train.yml", train_path, "train"), seed=3)
    ck = checkpoints()
    assert len(ck) == 2
    with np.load(ck[-1], allow_pickle=False) as z:
        full = {k: z[k] for k in z.files}
    names = E.param_names(2)
    shapes_ = E.param_shapes(2, 4096, 16, 32, 2, 3)
    assert all(n in full and full[n].shape == shapes_[n] for n in names)          # no new variables: the block's own, nothing else
    assert not [k for k in full if "drop" in k or "mask" in k]
    acc = run_task.main(cfg("val.yml", val_path, "val", resume="latest"))
    assert 0.0 <= acc <= 1.0
    first = ck[0][:-len(".weights.npz")]
    run_task.main(cfg("resume.yml", train_path, "train", resume=first), seed=5)
    with np.load(checkpoints()[-1], allow_pickle=False) as z:
        resumed = {k: z[k] for k in z.files}
    assert set(resumed) == set(full)
    for k in full:
        assert np.array_equal(resumed[k], full[k]), "resumed run differs in " + k
