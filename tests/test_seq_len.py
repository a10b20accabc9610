"""Per-clip sequence lengths (tf.nn.dynamic_rnn's sequence_length), the parts that need no GPU:
  * the reference of the length tests (tests/seq_len_ref.py: the existing oracle applied clip by clip to the live prefix) against an
    INDEPENDENT statement of the semantics -- a torch-CPU float64 cell loop over all T steps with torch.where(t < len, new, old)
    state copy-through and zeroed outputs, gradients by autograd;
  * its engine-level assembly against O.model_forward / O.model_backward at full length;
  * GraphEngine's host validation of `seq_len` on the torch-CPU stand-in of the kernels (tests/cpu_double.py): every refusal is a
    VltfError raised before any op is called, and a call without seq_len passes no new keyword to the ops.
The kernels are tests/test_seq_len_gpu.py's business."""
import numpy as np
import pytest
import torch

from oracle import lrcn_oracle as O
from tests import graph_cases as GC
from tests import seq_len_ref as R
from tests.cpu_double import install

torch.set_num_threads(4)


def rel_close(got, want, tol=1e-9, msg=""):
    want = np.asarray(want, np.float64)
    scale = float(np.abs(want).max()) or 1.0
    err = float(np.abs(np.asarray(got, np.float64) - want).max()) / scale
    assert err <= tol, "%s: relative error %.3e" % (msg, err)


def masked_lstm_autograd(x, kernel, bias, lens, s0, dout):
    """dynamic_rnn with sequence_length, stated directly: all T steps for all clips, the state copied through where t >= len."""
    b, T, d = x.shape
    H = kernel.shape[1] // 4
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    kt = torch.tensor(kernel, dtype=torch.float64, requires_grad=True)
    bt = torch.tensor(bias, dtype=torch.float64, requires_grad=True)
    ln = torch.tensor(np.asarray(lens))[:, None]
    if s0 is None:
        h0 = c0 = None
        h, c = torch.zeros(b, H, dtype=torch.float64), torch.zeros(b, H, dtype=torch.float64)
    else:
        h0 = torch.tensor(s0, dtype=torch.float64, requires_grad=True)
        c0 = torch.tensor(s0, dtype=torch.float64, requires_grad=True)
        h, c = h0, c0
    outs = []
    for t in range(T):
        z = torch.cat([xt[:, t], h], 1) @ kt + bt
        i, j, f, o = z.chunk(4, 1)
        cn = c * torch.sigmoid(f + O.FORGET_BIAS) + torch.sigmoid(i) * torch.tanh(j)
        hn = torch.tanh(cn) * torch.sigmoid(o)
        alive = t < ln
        c = torch.where(alive, cn, c)
        h = torch.where(alive, hn, h)
        outs.append(torch.where(alive, hn, torch.zeros_like(hn)))
    out = torch.stack(outs, 1)
    (out * torch.tensor(dout, dtype=torch.float64)).sum().backward()
    g = dict(out=out.detach().numpy(), c_last=c.detach().numpy(), h_last=h.detach().numpy(), dx=xt.grad.numpy(), dk=kt.grad.numpy(),
             db=bt.grad.numpy())
    if s0 is not None:
        g.update(dh0=h0.grad.numpy(), dc0=c0.grad.numpy())
    return g


@pytest.mark.parametrize("init", [False, True])
@pytest.mark.parametrize("b,T,d,H", [(6, 5, 7, 4), (9, 8, 3, 11)])
def test_prefix_oracle_equals_masked_dynamic_rnn(b, T, d, H, init):
    rng = np.random.default_rng(b * 100 + T)
    x = rng.standard_normal((b, T, d))
    kernel = rng.standard_normal((d + H, 4 * H)) * 0.4
    bias = rng.standard_normal(4 * H) * 0.1
    s0 = rng.standard_normal((b, H)) * 0.5 if init else None
    lens = rng.integers(1, T + 1, b)
    lens[0], lens[1] = 1, T
    dout = rng.standard_normal((b, T, H))
    got = R.lstm_layer(x, kernel, bias, lens, s0=s0, dout=dout)
    want = masked_lstm_autograd(x, kernel, bias, lens, s0, dout)
    for k in ("out", "c_last", "h_last", "dx", "dk", "db") + (("dh0", "dc0") if init else ()):
        rel_close(got[k], want[k], msg=k)
    dead = ~R.live_rows(lens, T)
    assert dead.any() and not got["out"].reshape(b * T, H)[dead].any() and not got["dx"].reshape(b * T, d)[dead].any()
    # the carried state in the dead rows is the final state
    assert np.array_equal(got["c"][:, -1], got["c_last"])


def test_prefix_fusion_and_loss_pieces():
    rng = np.random.default_rng(5)
    b, T, H, C = 5, 4, 3, 6
    x, lens = rng.standard_normal((b, T, H)), np.array([1, 4, 2, 3, 4])
    d = rng.standard_normal((b, H))
    for method in ("avg", "last"):
        y, g = R.fusion(x, lens, method, d)
        xt = torch.tensor(x, requires_grad=True)
        yt = torch.stack([xt[i, :L].mean(0) if method == "avg" else xt[i, L - 1] for i, L in enumerate(lens)])
        (yt * torch.tensor(d)).sum().backward()
        rel_close(y, yt.detach().numpy(), msg=method)
        rel_close(g, xt.grad.numpy(), msg=method + " grad")
    logits = rng.standard_normal((b * T, C))
    onehot = O.labels_to_one_hot([[l] for l in rng.integers(0, C, b * T)], C)
    loss_sum, hits, dl, loss = R.xent(logits, onehot, lens, T)
    m = R.live_rows(lens, T)
    zt = torch.tensor(logits, requires_grad=True)
    lt = -(torch.log_softmax(zt, 1) * torch.tensor(onehot, dtype=torch.float64)).sum(1)[torch.tensor(m)].mean()
    lt.backward()
    assert m.sum() == lens.sum() and abs(loss - float(lt.detach())) < 1e-12 and abs(loss_sum - loss * lens.sum()) < 1e-9
    rel_close(dl, zt.grad.numpy(), msg="dlogits")
    assert not dl[~m].any() and 0 <= hits <= m.sum()


@pytest.mark.parametrize("make", [lambda: GC.encdec(), lambda: GC.encdec(None, 1, "avg"), lambda: R.single_lstm_case(3)])
def test_item_by_item_assembly_equals_the_model_oracle_at_full_length(make):
    """tests/seq_len_ref.model_with_lengths with every length = fpc is O.model_forward / O.model_backward."""
    from vltf_amd.graph import init_params_for, model_specs
    case = make()
    items = 2
    pipes, ds = GC.specs_and_datasets(case, items)
    p = init_params_for(model_specs(pipes, ds, case["V"]), seed=case["seed"], well_scaled=True)
    _, feeds = GC.inputs(case, items)
    logits, onehot, loss, grads, _ = GC.expect(case, p, feeds)
    full = {n: [case["data"][s["input"][0]]["fpc"]] * items for n, s in case["pipes"]}
    for lens in (full, {}):
        got_logits, mask, got_loss, got_grads, n = R.model_with_lengths(p, case, feeds, lens, onehot, items)
        assert mask.all() and n == logits.shape[0]
        rel_close(got_logits, logits, msg="logits")
        assert abs(got_loss - loss) < 1e-9 * max(1, abs(loss))
        for k in p:
            rel_close(got_grads[k], grads[k], tol=1e-8, msg="grad " + k)


# ---- GraphEngine: host validation -------------------------------------------------------------------------------------------------------
class _NoOps:
    """Stands in for graph.ops once the engine is built: any op the engine reaches for is a failure of `validate before launch`."""

    def __getattr__(self, name):
        raise AssertionError("ops.%s was reached before the lengths were refused" % name)


def _engine(monkeypatch, case, items=None, dp=None):
    Engine = install(monkeypatch)
    pipes, ds = GC.specs_and_datasets(case, items)
    eng = Engine(pipes, ds, case["V"], device="cpu", dp=dp)
    eng.load_params(eng.init_params(seed=case["seed"], well_scaled=True))
    raw, _ = GC.inputs(case, items)
    feeds = {t: (dict(frames_u8=torch.from_numpy(v), mean_bgr=GC.MEAN) if v.dtype == np.uint8 else torch.from_numpy(v)) for t, v in raw.items()}
    return eng, feeds


def _refused(monkeypatch, eng, feeds, seq_len, match):
    from vltf_amd import graph
    from vltf_amd._ffi import VltfError
    rows = eng.last.max_rows
    onehot = torch.zeros((rows, eng.num_classes), dtype=torch.int32)
    with monkeypatch.context() as m:
        m.setattr(graph, "ops", _NoOps())
        with pytest.raises(VltfError, match=match):
            eng.forward(feeds, seq_len=seq_len)
        with pytest.raises(VltfError, match=match):
            eng.train_step(feeds, onehot, lr=0.01, seq_len=seq_len)


def test_lengths_are_validated_on_the_host_before_any_launch(monkeypatch):
    eng, feeds = _engine(monkeypatch, GC.encdec())                       # enc: 2 clips x 2 frames; dec: 2 clips x 4 word steps
    _refused(monkeypatch, eng, feeds, {"nope": [1, 2]}, "not a pipeline")
    _refused(monkeypatch, eng, feeds, {"dec": [1, 2, 3]}, "2 clips in this batch, 3 lengths")
    _refused(monkeypatch, eng, feeds, {"dec": [0, 4]}, r"1\.\.4")
    _refused(monkeypatch, eng, feeds, {"dec": [1, 5]}, r"1\.\.4")
    _refused(monkeypatch, eng, feeds, {"enc": [1, 3]}, r"1\.\.2")
    _refused(monkeypatch, eng, feeds, {"dec": np.array([1.0, 2.0])}, "integer")
    _refused(monkeypatch, eng, feeds, [1, 2], "dict")
    monkeypatch.setattr(eng.by_name["dec"], "H", 2048)
    _refused(monkeypatch, eng, feeds, {"dec": [1, 2]}, "1024")


def test_lengths_are_refused_where_they_are_not_built(monkeypatch):
    eng, feeds = _engine(monkeypatch, GC.two_stream("avg"))
    _refused(monkeypatch, eng, feeds, {"rgb": [1, 2]}, "no LSTM classifier")
    eng, feeds = _engine(monkeypatch, GC.encdec("concat", 2))
    _refused(monkeypatch, eng, feeds, {"dec": [1, 2, 3, 4]}, "concat")
    eng, feeds = _engine(monkeypatch, GC.encdec("ibias", 1))
    _refused(monkeypatch, eng, feeds, {"dec": [1, 2]}, "ibias")
    eng, feeds = _engine(monkeypatch, GC.encdec(None, 2, "avg"))
    _refused(monkeypatch, eng, feeds, {"dec": [1, 2, 3, 4]}, "ratio 2")

    class _TwoRanks:
        world = 2

        def reduce_async(self, flat, off, cnt):
            pass

        def wait(self):
            pass

    eng, feeds = _engine(monkeypatch, GC.encdec(), dp=_TwoRanks())
    _refused(monkeypatch, eng, feeds, {"dec": [1, 2]}, "data parallelism")


def test_a_call_without_lengths_passes_no_new_keyword(monkeypatch):
    """tests/cpu_double.CpuOps has the signatures of the ops before lengths existed: forward and train_step without seq_len (and
    with seq_len=None) must still run on it."""
    eng, feeds = _engine(monkeypatch, GC.encdec())
    a = eng.forward(feeds).numpy().copy()
    b = eng.forward(feeds, seq_len=None).numpy().copy()
    assert np.array_equal(a, b)
    onehot = torch.from_numpy(O.labels_to_one_hot([[1]] * a.shape[0], eng.num_classes))
    out = eng.train_step(feeds, onehot, lr=0.01, clip_norm=0.5, seq_len=None)
    assert out["rows"] == a.shape[0] and np.isfinite(out["loss"])
    assert all(nd.seq_len is None for nd in eng.nodes)
