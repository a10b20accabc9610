"""rnn_cell tcn on the GPU: vl_tconv_cols_fwd / _bwd against tests/tcn_ref.py (bit for bit: the forward only copies and stores zeros,
the backward adds in a stated order), their contracts (dead rows, a clip alone, alignment, refusals), and the convolution stack in
LRCNEngine (train step, conv_math, captured step) and GraphEngine (seq_len)."""
import numpy as np
import pytest
import torch

from tests import lstm_plan as LP
from tests import tcn_ref as R
from tests.test_lstm_geometry_gpu import DEV, Guarded, put, same_bits, within

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import vltf_amd.ops as ops_
    return ops_


def run_tconv(ops, case, inp, lens, dres=True, what=""):
    """Both launches into Guarded outputs (NaN in the dead rows of every input under lens); the memory checks; -> {cols, dx}."""
    batch, T, C, taps, dilation, causal = case
    nan = (lambda a: a) if lens is None else (lambda a: R.with_nan_in_dead_rows(a, T, lens))
    x, dcols = put(nan(inp.x), DEV), put(nan(inp.dcols), DEV)
    res = put(nan(inp.dres), DEV) if dres else None
    L = put(lens, DEV, torch.int32)
    o = dict(cols=Guarded((batch * T, taps * C), DEV), dx=Guarded((batch * T, C), DEV))
    ops.tconv_cols_fwd(x, o["cols"].t, batch, T, C, taps, dilation, causal, seq_len=L)
    ops.tconv_cols_bwd(dcols, res, o["dx"].t, batch, T, C, taps, dilation, causal, seq_len=L)
    return {k: g.settle(what + " " + k) for k, g in o.items()}


# ---- 1. the launches against the reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_tconv_cols_against_the_reference(ops, case, lens):
    batch, T, C, taps, dilation, causal = case
    ref = R.reference(case, lens)
    for dres in (True, False):
        what = "tconv %s %s %s" % (R.case_id(case), "lens" if lens else "full", "dres" if dres else "no dres")
        got = run_tconv(ops, case, ref.inp, ref.lens, dres, what)
        want32, want64 = (ref.dx32, ref.dx) if dres else (ref.dx32_nores, ref.dx_nores)
        same_bits(dict(cols=got["cols"]), dict(cols=ref.cols), what + ": cols against the reference")
        same_bits(dict(dx=got["dx"]), dict(dx=want32), what + ": dx against the fp32 ascending-order restatement")
        within("act", got["dx"], want64, what + " dx")
        if lens:
            dead = ~R.live_mask(ref.lens, batch, T).reshape(-1)
            assert batch == 1 or (dead.any() and not dead.all())
            for name in ("cols", "dx"):
                assert not got[name][dead].view(np.int32).any(), "%s: dead row of %s not +0.0" % (what, name)


# ---- 2. bit for bit ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", (False, True), ids=("full", "lens"))
def test_repeatable_and_a_clip_alone_equals_the_clip_in_a_batch(ops, lens):
    case = batch, T, C, taps, dilation, causal = (5, 16, 256, 3, 4, 0)
    ref = R.reference(case, lens)
    whole = run_tconv(ops, case, ref.inp, ref.lens, what="tconv")
    same_bits(run_tconv(ops, case, ref.inp, ref.lens, what="tconv again"), whole, "tconv: a second run")
    for b in range(batch):
        rows = slice(b * T, (b + 1) * T)
        one = R.Inputs(*(a[rows] for a in ref.inp))
        alone = run_tconv(ops, (1,) + case[1:], one, None if ref.lens is None else ref.lens[b:b + 1], what="tconv clip %d alone" % b)
        same_bits(alone, {k: v[rows] for k, v in whole.items()}, "tconv: clip %d alone against the batch of %d" % (b, batch))


# ---- 3. degenerate cases -----------------------------------------------------------------------------------------------------------------
def test_one_tap_is_the_copy_of_the_live_rows(ops):
    case = batch, T, C, taps, dilation, causal = (2, 6, 3, 1, 1, 0)
    for lens in (None, LP.lengths(batch, T)):
        inp = R.inputs(case)
        got = run_tconv(ops, case, inp, lens, what="tconv one tap")
        live = R.live_mask(lens, batch, T).reshape(-1)
        assert np.array_equal(got["cols"][live], inp.x[live]) and not got["cols"][~live].any()
        assert np.array_equal(got["dx"][live], (inp.dres + inp.dcols)[live]) and not got["dx"][~live].any()


def test_a_dilation_of_t_or_more_leaves_the_zero_offset_tap_alone(ops):
    for case in ((2, 16, 256, 3, 16, 0), (2, 16, 256, 3, 65536, 0), (3, 5, 24, 4, 5, 1)):
        batch, T, C, taps, dilation, causal = case
        inp = R.inputs(case)
        got = run_tconv(ops, case, inp, None, what="tconv " + R.case_id(case))
        j0 = taps - 1 if causal else (taps - 1) // 2
        cols = got["cols"].reshape(batch * T, taps, C)
        assert np.array_equal(cols[:, j0], inp.x)
        assert not np.delete(cols, j0, axis=1).any()
        assert np.array_equal(got["dx"], inp.dres + inp.dcols.reshape(batch * T, taps, C)[:, j0])


def test_causal_taps_read_no_later_step(ops):
    case = batch, T, C, taps, dilation, causal = (4, 7, 96, 4, 2, 1)
    inp = R.inputs(case)
    base = run_tconv(ops, case, inp, None, what="tconv causal")["cols"].reshape(batch, T, -1)
    for s in (0, 3, T - 1):
        x = inp.x.copy().reshape(batch, T, C)
        x[:, s] += 1.0
        got = run_tconv(ops, case, R.Inputs(x.reshape(batch * T, C), inp.dcols, inp.dres), None, what="tconv causal")["cols"].reshape(batch, T, -1)
        assert np.array_equal(got[:, :s], base[:, :s]) and not np.array_equal(got[:, s], base[:, s])


@pytest.mark.parametrize("case", [(5, 16, 256, 3, 4, 0), (2, 9, 7, 9, 1, 1)], ids=R.case_id)
def test_a_view_one_float_off_alignment_gives_the_aligned_result(ops, case):
    """Every pointer in turn (and all of them) starts one float behind a 16-byte boundary: the scalar path, the same bits."""
    batch, T, C, taps, dilation, causal = case
    ref = R.reference(case, True)
    L = put(ref.lens, DEV, torch.int32)

    def off(a, shift):
        flat = torch.zeros(a.size + 4, device=DEV)
        v = flat[shift:shift + a.size].view(a.shape)
        v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        assert v.data_ptr() % 16 == 4 * shift
        return v

    for shifts in ((1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 1), (1, 1, 1, 1, 1)):
        x, dcols, dres = (off(R.with_nan_in_dead_rows(a, T, ref.lens), s) for a, s in zip(ref.inp, shifts))
        cols = off(np.full((batch * T, taps * C), np.nan, np.float32), shifts[3])
        dx = off(np.full((batch * T, C), np.nan, np.float32), shifts[4])
        ops.tconv_cols_fwd(x, cols, batch, T, C, taps, dilation, causal, seq_len=L)
        ops.tconv_cols_bwd(dcols, dres, dx, batch, T, C, taps, dilation, causal, seq_len=L)
        got = dict(cols=cols.cpu().numpy(), dx=dx.cpu().numpy())
        same_bits(got, dict(cols=ref.cols, dx=ref.dx32), "tconv %s at offsets %s" % (R.case_id(case), shifts))


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ops):
    """Every limit through ops (which refuses first) and straight through the C entry points; tensors smaller than the launch; null
    pointers.  Every buffer is large enough for every shape tried.  Nothing is written; then one good call writes."""
    from vltf_amd import _ffi
    o = dict(cols=Guarded((2 * 16, 10 * 1028), DEV), dx=Guarded((2 * 16, 1028), DEV))
    f = lambda *shape: torch.zeros(shape, device=DEV)
    x, dcols, dres = f(2 * 16, 1028), f(2 * 16, 10 * 1028), f(2 * 16, 1028)
    good = dict(batch=2, T=16, C=256, taps=3, dilation=1, causal=0)
    fwd = lambda x_=x, cols_=o["cols"].t, **kw: ops.tconv_cols_fwd(x_, cols_, **dict(good, **kw))
    bwd = lambda dcols_=dcols, dres_=dres, dx_=o["dx"].t, **kw: ops.tconv_cols_bwd(dcols_, dres_, dx_, **dict(good, **kw))
    cases = ((dict(batch=0), "must be positive"), (dict(T=0), "must be positive"), (dict(C=0), "must be positive"),
             (dict(taps=0), "taps 0 must lie in 1..9"), (dict(taps=10, causal=1), "taps 10 must lie in 1..9"), (dict(taps=11), "must lie in 1..9"),
             (dict(taps=4), "must be odd unless causal"), (dict(dilation=0), "dilation 0 must lie in 1..65536"),
             (dict(dilation=65537), "dilation 65537 must lie in 1..65536"), (dict(C=1028), "C 1028 exceeds 1024"))
    for call in (fwd, bwd):
        for kw, match in cases:
            with pytest.raises(Exception, match=match):
                call(**kw)
    for call, kw in ((fwd, dict(x_=f(2 * 16, 255))), (fwd, dict(cols_=f(2 * 16 * 3, 255))), (bwd, dict(dcols_=f(2 * 16 * 3 - 1, 256))),
                     (bwd, dict(dres_=f(2 * 16 - 1, 256))), (bwd, dict(dx_=f(2 * 16, 255)))):
        with pytest.raises(Exception, match="elements"):         # tensors smaller than the launch would read or write
            call(**kw)
    for call, kw in ((fwd, dict(x_=None)), (fwd, dict(cols_=None)), (bwd, dict(dcols_=None)), (bwd, dict(dx_=None))):
        with pytest.raises(Exception, match="null pointer"):
            call(**kw)
    # the C entry points refuse on their own
    p = lambda t: t.data_ptr()
    for kw, match in cases:
        a = [dict(good, **kw)[k] for k in ("batch", "T", "C", "taps", "dilation", "causal")]
        with pytest.raises(Exception, match=match):
            _ffi.call("vl_tconv_cols_fwd", p(x), None, p(o["cols"].t), *a, ops.stream())
        with pytest.raises(Exception, match=match):
            _ffi.call("vl_tconv_cols_bwd", p(dcols), p(dres), None, p(o["dx"].t), *a, ops.stream())
    a = [good[k] for k in ("batch", "T", "C", "taps", "dilation", "causal")]
    for args in ((None, None, p(o["cols"].t)), (p(x), None, None)):
        with pytest.raises(Exception, match="null pointer"):
            _ffi.call("vl_tconv_cols_fwd", *args, *a, ops.stream())
    for args in ((None, p(dres), None, p(o["dx"].t)), (p(dcols), p(dres), None, None)):
        with pytest.raises(Exception, match="null pointer"):
            _ffi.call("vl_tconv_cols_bwd", *args, *a, ops.stream())
    torch.cuda.synchronize()
    assert all(g.untouched() for g in o.values()), "tconv: refused, yet an output was written"
    fwd()                                                           # (the arguments are good otherwise)
    torch.cuda.synchronize()
    assert o["dx"].untouched() and not o["cols"].untouched()
    bwd(dres_=None)                                                 # (dres alone may be missing)
    torch.cuda.synchronize()
    assert not o["dx"].untouched()


# ---- 5. LRCNEngine -----------------------------------------------------------------------------------------------------------------------
MEAN = np.array([99.197148, 105.293620, 109.503945], np.float32)
SHAPE, NCLS, FPC, CLIPS, ATTN, VLAD_K = (67, 67, 3), 7, 3, 2, 5, 4           # the smoke() geometry of tests/test_gru_gpu.py
SEED = 6                                                                     # (tcn_ref.model_train_step asserts the ReLU margin under it)
ENGINE_CASES = [(16, 1, 3, "avg", False, "exponential"), (8, 2, 3, "last", True, "exponential"), (16, 2, 5, "attn", False, "none"),
                (16, 1, 3, "vlad", False, "exponential"), (128, 1, 3, "avg", False, "exponential")]


def engine_cfg(H, layers, k, fusion, causal, mode, fpc=FPC, **kw):
    from vltf_amd.engine import NetConfig
    return NetConfig(image_shape=SHAPE, num_classes=NCLS, fpc=fpc, frame_encoding_layer="fc6", lstm_hidden=H, lstm_layers=layers,
                     fusion=fusion, attn_dim=ATTN if fusion == "attn" else None, vlad_clusters=VLAD_K if fusion == "vlad" else None,
                     rnn_cell="tcn", tcn_kernel=k, tcn_dilation=mode, tcn_causal=causal, **kw)


def engine_problem(H, layers, k, fusion):
    """Parameters, frames and labels of an engine case from SEED, the embedding tamed on the reference's features."""
    rng = np.random.default_rng(SEED)
    p = R.init_params(rng, NCLS, "fc6", H, layers, SHAPE, k, fusion, ATTN, VLAD_K)
    frames = rng.integers(0, 256, (CLIPS * FPC,) + SHAPE, dtype=np.uint8)
    onehot = np.eye(NCLS, dtype=np.int32)[rng.integers(0, NCLS, CLIPS)]
    R.tame_embedding(p, frames.astype(np.float32) - MEAN, "fc6")
    return p, frames, onehot


@pytest.mark.parametrize("H,layers,k,fusion,causal,mode", ENGINE_CASES)
def test_lrcn_engine_train_step_against_the_reference(H, layers, k, fusion, causal, mode):
    """Logits, loss, gradient norm, every gradient and the clipped SGD step against tcn_ref.model_train_step at the bounds of
    tests/test_attn_pool_gpu.test_lrcn_engine_train_step_against_the_reference; a gradient reaches every temporal_conv variable."""
    from vltf_amd.engine import LRCNEngine, param_specs
    cfg = engine_cfg(H, layers, k, fusion, causal, mode)
    eng = LRCNEngine(cfg, max_clips=CLIPS, device=DEV)
    p, frames, onehot = engine_problem(H, layers, k, fusion)
    assert {n: tuple(s) for n, s in param_specs(cfg)} == {n: v.shape for n, v in p.items()}
    eng.load_params(p)
    newp, loss, gn, logits, grads = R.model_train_step(p, frames.astype(np.float32) - MEAN, onehot, FPC, 0.01, 0.5, "fc6", H, layers, fusion,
                                                       mode, causal)
    fd = torch.tensor(frames, device=DEV)
    got_fwd = eng.forward_u8(fd, MEAN).cpu().numpy()
    assert got_fwd.shape == logits.shape
    np.testing.assert_allclose(got_fwd, logits, rtol=1e-3, atol=1e-3)
    out = eng.train_step_u8(fd, torch.tensor(onehot, device=DEV), lr=0.01, clip_norm=0.5, mean_bgr=MEAN)
    assert abs(out["loss"] - loss) < 1e-4 * max(1, abs(loss))
    assert abs(out["grad_norm"] - gn) < 1e-3 * gn
    g = eng.get_grads()
    assert set(g) == set(p) and set(R.param_names(layers)) <= set(g)
    for n in p:
        scale = np.abs(grads[n]).max() + 1e-12
        np.testing.assert_allclose(g[n], grads[n], rtol=2e-3, atol=2e-4 * scale, err_msg="grad " + n)
        assert scale > 1e-9, "no gradient reached " + n
    got = eng.get_params()
    for n in p:
        np.testing.assert_allclose(got[n], newp[n], rtol=1e-4, atol=1e-5, err_msg="param " + n)


def tame_on_device(eng, p, frames):
    """tcn_ref.tame_embedding with the rms of the features the DEVICE computes (one forward); loads p into the engine."""
    eng.load_params(p)
    eng.forward_u8(frames, MEAN)
    rms = float(eng.feat[:frames.shape[0]].double().square().mean().sqrt())
    name = R.var_name(None, "kernel")
    p[name] = (p[name] / rms).astype(np.float32)
    eng.load_params(p)


# ---- 6. the block's products are fp32 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", ("f32", "bf16x3", "bf16"))
def test_the_blocks_products_are_fp32_under_every_conv_math(math):
    """8 clips x 16 frames, H = 128, three taps: the block's products have 128 rows and columns and a depth of 128 or 384, the sizes from
    which ops.gemm WITH a workspace follows conv_math into split-bf16 arithmetic.  They are called without one: each is compared with
    the fp64 product of the operands THE DEVICE holds, at class act (3e-5, 3e-5) -- an fp32 product of that depth is well inside it, a
    single-plane bf16 product (2^-9 per factor) two orders outside.  The taps between them are held to the reference bit for bit."""
    from vltf_amd.engine import LRCNEngine, init_params
    clips, fpc, H, k = 8, 16, 128, 3
    n = clips * fpc
    cfg = engine_cfg(H, 1, k, "avg", False, "exponential", fpc=fpc, conv_math=math)
    p = init_params(cfg, seed=3, well_scaled=True)
    r = np.random.default_rng(5)
    for v in ("conv_bias", "out_bias"):
        p[R.var_name(0, v)] = (0.1 * r.standard_normal(H)).astype(np.float32)
    eng = LRCNEngine(cfg, max_clips=clips, device=DEV)
    rng = np.random.default_rng(12)
    frames = torch.from_numpy(rng.integers(0, 256, (n,) + SHAPE, dtype=np.uint8)).to(DEV)
    onehot = torch.from_numpy(np.eye(NCLS, dtype=np.int32)[rng.integers(0, NCLS, clips)]).to(DEV)
    tame_on_device(eng, p, frames)
    out = eng.train_step_u8(frames, onehot, lr=0.01, clip_norm=0.0, mean_bgr=MEAN)
    assert np.isfinite(out["loss"]) and out["rows"] == clips
    host = lambda t: t.detach().cpu().numpy().astype(np.float64)
    S = eng.tcn["layers"][0]
    x0, dx0 = host(eng.tcn["x0"][:n]), host(eng.tcn["dx0"][:n])
    cols, z, m, hseq, dy, dz, dcols = (host(S[key][:n]) for key in ("cols", "z", "m", "hseq", "dout", "dz", "dcols"))
    W1, b1, W2, b2 = (p[R.var_name(0, v)].astype(np.float64) for v in R.VARS)
    W1 = W1.reshape(k * H, H)
    assert 0.1 < np.abs(x0).mean() < 10 and np.abs(dy).max() > 0 and 0.05 < (z > 0).mean() < 0.95
    what = "tcn products under conv_math %s: " % math
    assert np.array_equal(cols, R.cols_fwd(x0, None, clips, fpc, H, k, 1, False)), what + "cols"
    within("act", z, np.maximum(cols @ W1 + b1, 0.0), what + "z = relu(cols W1 + b1)")
    within("act", m, z @ W2 + b2, what + "m = z W2 + b2")
    assert np.array_equal(hseq.astype(np.float32), (x0.astype(np.float32) + m.astype(np.float32))), what + "hseq = x + m"
    within("act", host(eng.G[R.var_name(0, "out_kernel")]), z.T @ dy, what + "G[out_kernel] = z^T dy")
    within("act", host(eng.G[R.var_name(0, "out_bias")]), dy.sum(axis=0), what + "G[out_bias]")
    within("act", dz, (dy @ W2.T) * (z > 0), what + "dz = relu_grad(dy W2^T, z)")
    within("act", host(eng.G[R.var_name(0, "conv_kernel")]).reshape(k * H, H), cols.T @ dz, what + "G[conv_kernel] = cols^T dz")
    within("act", host(eng.G[R.var_name(0, "conv_bias")]), dz.sum(axis=0), what + "G[conv_bias]")
    within("act", dcols, dz @ W1.T, what + "dcols = dz W1^T")
    want = R.cols_bwd(dcols.astype(np.float32), dy.astype(np.float32), None, clips, fpc, H, k, 1, False, dtype=np.float32)
    assert np.array_equal(dx0.astype(np.float32), want), what + "dx0"


# ---- 7. the captured step ----------------------------------------------------------------------------------------------------------------
def test_lrcn_engine_captured_step_is_the_eager_step():
    """step_graph with dropout behind the fusion and two layers: the warm-up step, the captured one and three replays equal the eager
    engine's bit for bit -- the two launches take no host-varying argument and replay as they are.  One graph is held."""
    from vltf_amd.engine import LRCNEngine, init_params
    engines = []
    kw = dict(dropout_keep_prob=0.5)
    params = init_params(engine_cfg(16, 2, 3, "avg", False, "exponential", **kw), seed=4, well_scaled=True)
    rng = np.random.default_rng(11)
    some = torch.from_numpy(rng.integers(0, 256, (CLIPS * FPC,) + SHAPE, dtype=np.uint8)).to(DEV)
    for sg in (False, True):
        e = LRCNEngine(engine_cfg(16, 2, 3, "avg", False, "exponential", step_graph=sg, **kw), max_clips=CLIPS, device=DEV)
        if not sg:
            tame_on_device(e, params, some)                                  # (changes params: activations of order 1)
        e.load_params(params)
        engines.append(e)
    for step in range(5):
        frames = torch.from_numpy(rng.integers(0, 256, (CLIPS * FPC,) + SHAPE, dtype=np.uint8)).to(DEV)
        onehot = torch.from_numpy(np.eye(NCLS, dtype=np.int32)[rng.integers(0, NCLS, CLIPS)]).to(DEV)
        outs = [e.train_step_u8(frames, onehot, 0.01 * 0.7 ** step, 5.0, MEAN) for e in engines]
        for key in ("loss_sum", "correct", "grad_norm", "rows"):
            assert outs[0][key] == outs[1][key], (step, key, outs[0][key], outs[1][key])
        assert np.array_equal(engines[0].logits_host(), engines[1].logits_host()), step
        assert torch.equal(engines[0].tconv[-1]["hseq"], engines[1].tconv[-1]["hseq"]), step
    assert len(engines[1]._graphs) == 1
    pa, pb = engines[0].get_params(), engines[1].get_params()
    for n in pa:
        assert np.array_equal(pa[n], pb[n]), n
    name = R.var_name(1, "conv_kernel")
    assert not np.array_equal(pa[name], params[name])                        # the second layer's convolution trains


# ---- 8. GraphEngine: a vector-input pipeline with lengths ------------------------------------------------------------------------------
G_DIM, G_H, G_C, G_CLIPS, G_LAYERS = 10, 16, 5, 4, 2


def graph_engine(T, fusion="avg", seed=3, params=None):
    from vltf_amd.graph import DatasetInfo, GraphEngine, PipelineSpec, init_params_for, model_specs
    pipes = [PipelineSpec("net", ["main"], "nop", classifier="lstm", lstm_params=(G_H, G_LAYERS, fusion), rnn_cell="tcn")]
    ds = {"main": DatasetInfo("vectors", T, 1, G_CLIPS, dim=G_DIM)}
    eng = GraphEngine(pipes, ds, G_C, device=DEV)
    p = params
    if p is None:
        p = init_params_for(model_specs(pipes, ds, G_C), seed=seed, well_scaled=True)
        for n in p:                                                 # biases that are not zero
            if n.endswith("bias"):
                p[n] = (0.1 * np.random.default_rng(len(n)).standard_normal(p[n].shape)).astype(np.float32)
    eng.load_params(p)
    return eng, p


@pytest.mark.parametrize("fusion", ("avg", "last"))
def test_graph_engine_with_lengths_against_the_reference(fusion):
    """seq_len and NaN in the padded steps' features: logits and every gradient equal tcn_ref with lengths."""
    from oracle import lrcn_oracle as O
    T, lens = 5, np.array([5, 2, 1, 4])
    eng, p = graph_engine(T, fusion)
    x = (np.random.default_rng(8).standard_normal((G_CLIPS * T, G_DIM))).astype(np.float32)
    onehot = np.eye(G_C, dtype=np.int32)[np.random.default_rng(9).integers(0, G_C, G_CLIPS)]
    fd = {"main": torch.from_numpy(R.with_nan_in_dead_rows(x, T, lens)).to(DEV)}
    got = eng.forward(fd, seq_len={"net": lens}).cpu().numpy()
    out, caches = R.stack_forward(x, p, T, G_LAYERS, lens=lens)
    assert R.relu_margin(caches) > R.RELU_BAND
    want, loss, dout, grads = R.head_step(p, out, onehot, T, G_H, fusion, lens, softmax_xent=lambda lg, oh: O.softmax_xent_mean(lg, oh, np.float64))
    np.testing.assert_allclose(got, want, rtol=1e-3, atol=1e-3)
    grads.update(R.stack_backward(dout, caches)[1])
    res = eng.train_step(fd, torch.from_numpy(onehot).to(DEV), lr=0.01, clip_norm=0.0, seq_len={"net": lens})
    assert abs(res["loss"] - loss) < 1e-4 * max(1, abs(loss))
    g = eng.get_grads()
    assert set(g) == set(grads)
    for n in grads:
        scale = np.abs(grads[n]).max() + 1e-12
        np.testing.assert_allclose(g[n], grads[n], rtol=2e-3, atol=2e-4 * scale, err_msg="grad " + n)
        assert scale > 1e-9, "no gradient reached " + n
        assert np.isfinite(g[n]).all()


def test_graph_engine_uniform_length_is_the_shorter_model():
    """Clips of length 3 in a 5-step batch (NaN in the padding) give what they give in a 3-step model, at class act: logits and every
    gradient."""
    T, L = 5, 3
    x = (np.random.default_rng(8).standard_normal((G_CLIPS, T, G_DIM))).astype(np.float32)
    onehot = torch.from_numpy(np.eye(G_C, dtype=np.int32)[np.random.default_rng(9).integers(0, G_C, G_CLIPS)]).to(DEV)
    _, p = graph_engine(T)
    res = []
    for steps, kw in ((T, dict(seq_len={"net": [L] * G_CLIPS})), (L, {})):
        eng, _ = graph_engine(steps, params=p)
        fed = np.ascontiguousarray(x[:, :steps])
        fed[:, L:] = np.nan
        fd = {"main": torch.from_numpy(fed.reshape(-1, G_DIM)).to(DEV)}
        logits = eng.forward(fd, **kw).cpu().numpy()
        out = eng.train_step(fd, onehot, lr=0.01, clip_norm=0.0, **kw)
        res.append((logits, out, eng.get_grads()))
    within("act", res[0][0], res[1][0], "tcn: logits of the padded batch against the shorter model")
    assert res[0][1]["rows"] == res[1][1]["rows"] == G_CLIPS
    assert abs(res[0][1]["loss"] - res[1][1]["loss"]) < 1e-5 * max(1, abs(res[1][1]["loss"]))
    for n in res[0][2]:
        within("act", res[0][2][n], res[1][2][n], "tcn: gradient %s of the padded batch against the shorter model" % n)


# ---- 9. run_task.py on examples/lrcn_tcn.yml -------------------------------------------------------------------------------------------
def test_run_task_on_the_example_trains(tmp_path, monkeypatch):
    """examples/lrcn_tcn.yml pointed at the synthetic dataset (its shapes, four classes, two 16-wide layers, batches of 2, deterministic
    image processing): two epochs of three steps with a checkpoint each; the checkpoint holds the temporal_conv variables under their
    names and shapes, and every one of them left its initial value."""
    import glob
    import os
    import yaml
    from tests.test_host_workflow import make_dataset
    from tests.test_run_task_gpu import RAW, WANT
    from vltf_amd import run_task
    monkeypatch.setenv("VLTF_PREFETCH", "0")
    monkeypatch.setenv("VLTF_CONV_MATH", "f32")
    folder = str(tmp_path)
    train_path, _, _ = make_dataset(folder, "train.txt", shape=RAW, seed=1)
    run = os.path.join(folder, "run")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "examples", "lrcn_tcn.yml")) as f:
        c = yaml.safe_load(f)
    r = c["run"]
    r.update(resume_file=None, run_folder=run, phase="defs.phase.train")
    d = r["data"].pop("train_set")
    d.update(data_path=train_path, phase="defs.phase.train", raw_image_shape=str(RAW), image_shape=str(WANT),
             imgproc=["defs.imgproc.center_crop", "defs.imgproc.sub_mean"])
    r["data"]["d"] = d
    r["network"]["num_classes"] = 4
    pipe = r["network"]["pipelines"][0]["lrcn"]
    assert (pipe["rnn_cell"], pipe["tcn_kernel"], pipe["tcn_dilation"], pipe["tcn_causal"]) == ("tcn", 3, "exponential", False)
    pipe["lstm_params"] = [16, 2, "defs.fusion_method.avg"]
    r["train"].update(batch_size=2, epochs=2, base_lr=1e-2, lr_decay=["defs.decay.exp", "defs.periodicity.interval", 2, 0.9], clip_norm=5)
    path = os.path.join(folder, "train.yml")
    with open(path, "w") as f:
        yaml.safe_dump(c, f)
    run_task.main(path, seed=3)                                                            # 5 videos, batch 2: three steps an epoch
    ck = sorted(glob.glob(os.path.join(run, "checkpoints", "*.weights.npz")), key=os.path.getmtime)
    assert len(ck) == 2
    with np.load(ck[-1], allow_pickle=False) as z:
        full = {k: z[k] for k in z.files}
    names = R.param_names(2)
    assert all(n in full for n in names) and full["output_fc_w"].shape == (16, 4)
    assert [full[n].shape for n in names] == R.param_shapes(2, 4096, 16, 3)
    assert all(full[n].any() and np.isfinite(full[n]).all() for n in names)               # the biases left their zeros
    log = open(glob.glob(os.path.join(run, "log_lrcn_tcn_train_scratch_*.log"))[0]).read()
    assert "global step: 6" in log
