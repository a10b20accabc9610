"""The calling convention of vltf_amd.temporal's function pairs, without a GPU: the bidirectional LSTM, the GRU, plain self-attention,
attention pooling and NetVLAD, each forward and backward, on small CPU tensors with temporal.ops replaced by a recorder.  What both
engines rely on: a launch writes into G exactly where param_grads runs it; the length keyword reaches every launch that
takes lengths and only with lengths; rk is asked once per recurrence launch, for that launch's tag span; the bidirectional stack
launches no input gradient of its bottom layer where nobody reads one.  Every recorded call must also bind to the signature of the
real vltf_amd.ops function.  What the launches compute is the business of the per-model GPU tests."""
import inspect

import pytest
import torch

from vltf_amd import ops as real_ops
from vltf_amd import temporal as TM

B, T, D, H, LAYERS, HEADS = 3, 4, 5, 8, 2, 2
ROWS = B * T
RECURRENCES = {"lstm_seq_bi_fwd": "lstm_seq_bi_tag_span", "lstm_seq_bi_bwd": "lstm_seq_bi_tag_span", "gru_seq_fwd": "gru_seq_tag_span",
               "gru_seq_bwd": "gru_seq_tag_span"}
SPANS = {"lstm_seq_bi_tag_span": lambda b, t, h: 1000 + b * t * h, "gru_seq_tag_span": lambda b, t, h: 2000 + b * t * h}
HOST = ("sa_drop_salt", "SA_DROP_SITES")                         # host helpers of ops that launch nothing: passed through


def tensors_of(x):
    if torch.is_tensor(x):
        return [x]
    return [t for e in x for t in tensors_of(e)] if isinstance(x, (tuple, list)) else []


class Recorder:
    """Stands in for vltf_amd.ops: notes every launch as (name, args, kwargs, inside param_grads?) and launches nothing."""

    def __init__(self):
        self.calls, self.inside = [], 0

    def __getattr__(self, name):
        if name in HOST:
            return getattr(real_ops, name)
        if name in SPANS:
            return SPANS[name]

        def launch(*args, **kw):
            inspect.signature(getattr(real_ops, name)).bind(*args, **kw)          # TypeError: not a call the real function takes
            self.calls.append((name, args, kw, self.inside > 0))
        return launch

    def param_grads(self, launch):
        self.inside += 1
        launch(self.ws_side, self.sws_side)
        self.inside -= 1

    ws_side, sws_side = torch.zeros(4), torch.zeros(4)


def takes_lengths(name):
    return "seq_len" in inspect.signature(getattr(real_ops, name)).parameters


def flat_views(specs):
    """{name: view} over ONE flat buffer, as the engines keep P and G"""
    flat = torch.zeros(sum(int(torch.Size(s).numel()) for _, s in specs))
    out, o = {}, 0
    for name, shape in specs:
        n = int(torch.Size(shape).numel())
        out[name] = flat[o:o + n].view(shape)
        o += n
    return flat, out


def aliases(x, flat):
    return any(t.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr() for t in tensors_of(x))


def touches(call, flat):
    return any(aliases(a, flat) for a in list(call[1]) + list(call[2].values()))


buf = lambda *shape: torch.zeros(*shape)


def blstm_specs(scope):
    return [(n, s) for l in range(LAYERS) for n, s in zip(TM.blstm_names(l, scope), 2 * (((D if l == 0 else 2 * H) + H, 4 * H), (4 * H,)))]


class Model:
    """One model kind: its variables, buffers and the two calls, given (rec, scope, lk, drop, dx)."""

    def __init__(self, kind, scope, drop=None):
        self.kind, self.scope, self.drop = kind, scope, drop
        self.x0, self.ws, self.lstm_ws = buf(ROWS, D), buf(16), buf(16)
        if kind == "blstm":
            specs = blstm_specs(scope)
            self.layers = [TM.blstm_buffers(buf, ROWS, H, True) for _ in range(LAYERS)]
            self.dx, self.dx_bw = buf(ROWS, D), buf(ROWS, max(D, 2 * H))
        elif kind == "gru":
            specs = [s for l in range(LAYERS) for s in TM.gru_specs(l, D if l == 0 else H, H, scope)]
            self.layers = [TM.gru_buffers(buf, ROWS, H, True) for _ in range(LAYERS)]
        elif kind in ("mhsa", "mhsa nopos"):
            self.positions = "none" if kind == "mhsa nopos" else "relative"
            specs = [s for l in range(LAYERS) for s in TM.mhsa_specs(l, D if l == 0 else H, H, HEADS, T, scope, self.positions)]
            self.layers = [TM.mhsa_buffers(buf, ROWS, T, H, HEADS, self.positions, True) for _ in range(LAYERS)]
        elif kind == "attn":
            specs, self.S = TM.attn_specs(H, 6, scope), TM.attn_buffers(buf, B, T, H, 6, True)
        elif kind == "vlad":
            specs, self.S = TM.vlad_specs(H, 3, scope), TM.vlad_buffers(buf, B, T, H, 3, True)
        if kind in ("attn", "vlad"):
            self.hseq, self.dout, self.d = buf(ROWS, H), buf(ROWS, H), buf(B, 3 * H)
            self.fused = buf(B, 3 * H)
        self.pflat, self.P = flat_views(specs)
        self.gflat, self.G = flat_views(specs)

    def run(self, rec, lk, dx_given=True):
        """forward then backward -> the rk spans asked for"""
        asked = []

        def rk(span):
            asked.append(span)
            return dict(ws=self.lstm_ws, tag_offset=len(asked), **lk)

        k, P, G, sc, pg = self.kind, self.P, self.G, self.scope, rec.param_grads
        if k == "blstm":
            out = TM.blstm_forward(self.layers, P, sc, self.x0, ROWS, B, T, D, H, self.ws, rk)
            assert out is self.layers[-1]["hseq"]
            assert TM.blstm_backward(self.layers, P, G, sc, self.x0, ROWS, B, T, D, H, self.ws, rk, pg, self.dx if dx_given else None,
                                     self.dx_bw) is None
        elif k == "gru":
            assert TM.gru_forward(self.layers, P, sc, self.x0, ROWS, B, T, D, H, self.ws, rk) is self.layers[-1]["hseq"]
            assert TM.gru_backward(self.layers, P, G, sc, self.x0, ROWS, B, T, D, H, self.ws, rk, pg) is self.layers[0]["dgx"]
        elif k in ("mhsa", "mhsa nopos"):
            out = TM.mhsa_forward(self.layers, P, sc, self.x0, ROWS, B, T, D, H, HEADS, self.positions, self.ws, lk, self.drop)
            assert out is self.layers[-1]["hseq"]
            assert TM.mhsa_backward(self.layers, P, G, sc, self.x0, ROWS, B, T, D, H, HEADS, self.positions, self.ws, lk, pg,
                                    self.drop) is self.layers[0]["dqkv"]
        elif k == "attn":
            TM.attn_forward(self.S, P, sc, self.hseq, self.fused, ROWS, B, T, H, 6, lk)
            TM.attn_backward(self.S, P, G, sc, self.d, self.hseq, self.dout, ROWS, B, T, H, 6, lk, pg)
        elif k == "vlad":
            TM.vlad_forward(self.S, P, sc, self.hseq, self.fused, ROWS, B, T, H, 3, lk)
            TM.vlad_backward(self.S, P, G, sc, self.d, self.hseq, self.fused, self.dout, ROWS, B, T, H, 3, lk, pg)
        return asked


KINDS = ("blstm", "gru", "mhsa", "mhsa nopos", "mhsa drop", "attn", "vlad")


def recorded(monkeypatch, kind, scope, lk, dx_given=True):
    rec = Recorder()
    monkeypatch.setattr(TM, "ops", rec)
    drop = TM.SaDrop.plan(0.3, None, None, LAYERS).bind(0, seed=5) if kind == "mhsa drop" else None
    m = Model("mhsa" if kind == "mhsa drop" else kind, scope, drop)
    asked = m.run(rec, lk, dx_given)
    assert rec.calls and rec.inside == 0
    return rec, m, asked


@pytest.mark.parametrize("scope", ("", "net/"))
@pytest.mark.parametrize("kind", KINDS)
def test_gradients_are_written_inside_param_grads_and_nowhere_else(monkeypatch, kind, scope):
    rec, m, _ = recorded(monkeypatch, kind, scope, {})
    inside = [c for c in rec.calls if c[3]]
    assert inside, "no parameter gradient was launched"
    for c in rec.calls:
        assert touches(c, m.gflat) == c[3], (c[0], c[3])
    for name, args, kw, _ in inside:                                 # on the scratch param_grads handed over, not on the chain's
        scratch = [t for a in list(args) + list(kw.values()) for t in tensors_of(a)
                   if t.untyped_storage().data_ptr() == m.ws.untyped_storage().data_ptr()]
        assert not scratch, name
        assert name != "colsum" or args[2] is rec.sws_side
        assert "ws" not in kw or kw["ws"] is rec.ws_side
    written = {n for n, g in m.G.items() if any(c[3] and any(t.data_ptr() == g.data_ptr() for a in c[1] for t in tensors_of(a)) for c in rec.calls)}
    assert written == set(m.G), set(m.G) - written                   # every variable of the model got its gradient launch


@pytest.mark.parametrize("kind", KINDS)
def test_lengths_reach_every_launch_that_takes_them_and_only_with_lengths(monkeypatch, kind):
    rec, _, _ = recorded(monkeypatch, kind, "", {})
    assert all("seq_len" not in kw for _, _, kw, _ in rec.calls)
    lens = torch.tensor([4, 2, 1], dtype=torch.int32)
    with_len, _, _ = recorded(monkeypatch, kind, "", {"seq_len": lens})
    assert [c[0] for c in with_len.calls] == [c[0] for c in rec.calls]            # lengths change no launch sequence
    took = [name for name, _, kw, _ in with_len.calls if takes_lengths(name)]
    assert took, "the model has no launch that takes lengths"
    for name, _, kw, _ in with_len.calls:
        if takes_lengths(name):
            assert kw.get("seq_len") is lens, name
        else:
            assert "seq_len" not in kw, name


@pytest.mark.parametrize("kind", ("blstm", "gru"))
def test_rk_is_asked_once_per_recurrence_launch_for_its_tag_span(monkeypatch, kind):
    rec, m, asked = recorded(monkeypatch, kind, "", {})
    launches = [(name, kw) for name, _, kw, _ in rec.calls if name in RECURRENCES]
    assert len(launches) == 2 * LAYERS == len(asked)
    assert asked == [SPANS[RECURRENCES[name]](B, T, H) for name, _ in launches]
    assert [kw["tag_offset"] for _, kw in launches] == list(range(1, len(asked) + 1))    # each launch got the answer to its own question
    assert all(kw["ws"] is m.lstm_ws for _, kw in launches)
    for other in ("mhsa", "attn", "vlad"):
        assert recorded(monkeypatch, other, "", {})[2] == []


def test_blstm_without_dx_launches_no_input_gradient_of_the_bottom_layer(monkeypatch):
    rec, m, _ = recorded(monkeypatch, "blstm", "", {})
    bare, m2, _ = recorded(monkeypatch, "blstm", "", {}, dx_given=False)
    sig = lambda calls: [(c[0], [a for a in c[1] if not tensors_of(a)], sorted(c[2])) for c in calls]
    n = len(rec.calls)                                               # the last launches: a product into dx, one into dx_bw, their add
    assert [c[0] for c in rec.calls[-3:]] == ["gemm", "gemm", "eltwise2"]
    assert [i for i, c in enumerate(rec.calls) if touches(c, m.dx)] == [n - 3, n - 1]
    assert sig(bare.calls) == sig(rec.calls[:-3])
    assert not any(touches(c, m2.dx) for c in bare.calls)
    # the layer above still hands its input gradient down: the bottom layer's dout is written in both
    assert any(c[0] == "eltwise2" and c[1][2] is m2.layers[0]["dout"] for c in bare.calls)
