"""TEST INFRASTRUCTURE: the reference for per-clip sequence lengths = the EXISTING oracle (oracle.lrcn_oracle) applied clip by clip
to the live prefix.  A clip of length L in a T-step batch must give what the same clip gives in an L-step model, so nothing here
knows about masking: every function cuts clip b to its first lens[b] steps, runs the unchanged oracle on that one-item batch, and
puts the pieces back (outputs of dead steps zero, states carried, weight gradients summed over clips).

Engine level (`model_with_lengths`): one item at a time through the oracle's own pieces -- alexnet_forward / alexnet_backward for a
`representation: dcnn`, lstm_classifier_forward / lstm_classifier_backward for the `classifier: lstm` -- chained as
oracle.model_forward chains them for the pipeline kinds the length tests use (dcnn | nop representation into an LSTM classifier,
optionally with an earlier pipeline's output as its state).  It is not O.model_forward itself only because that repeats the
reference's guard "The LSTM classifier requires an fpc greater than 1" (model.py:121), which a clip of length 1 inside a longer
batch is not subject to; tests/test_seq_len.py pins this assembly to O.model_forward / O.model_backward at full length."""
import numpy as np

from oracle import lrcn_oracle as O

F64 = np.float64


def lstm_layer(x, kernel, bias, lens, s0=None, dout=None):
    """One LSTM layer over x [B, T, D] with lengths lens [B]; s0: initial state (c = h) or None; dout [B, T, H] or None.
    -> dict(out [B,T,H] (dead steps 0), c [B,T,H] and hprev [B,T,H] (dead steps: the carried state), c_last, h_last [B,H],
            and with dout: dx [B,T,D] (dead steps 0), dk, db, dh0, dc0)."""
    b, T, d = x.shape
    H = kernel.shape[1] // 4
    r = dict(out=np.zeros((b, T, H), F64), c=np.zeros((b, T, H), F64), hprev=np.zeros((b, T, H), F64),
             c_last=np.zeros((b, H), F64), h_last=np.zeros((b, H), F64))
    if dout is not None:
        r.update(dx=np.zeros((b, T, d), F64), dk=np.zeros(kernel.shape, F64), db=np.zeros(4 * H, F64), dh0=np.zeros((b, H), F64),
                 dc0=np.zeros((b, H), F64))
    for i in range(b):
        L = int(lens[i])
        st = None if s0 is None else s0[i:i + 1]
        out, (c, h), cache = O.lstm_layer_forward(x[i:i + 1, :L], kernel, bias, h0=st, c0=st)
        first = np.zeros((1, H), F64) if st is None else st.astype(F64)
        r["out"][i, :L] = out[0]
        r["c"][i, :L] = np.stack([v[0] for v in cache["cs"]])
        r["c"][i, L:] = c[0]
        r["hprev"][i, :L] = np.concatenate([first, out[0, :L - 1]], axis=0)
        r["hprev"][i, L:] = h[0]
        r["c_last"][i], r["h_last"][i] = c[0], h[0]
        if dout is not None:
            dx, dk, db, dh0, dc0 = O.lstm_layer_backward(kernel, cache, dout[i:i + 1, :L])
            r["dx"][i, :L] = dx[0]
            r["dk"] += dk
            r["db"] += db
            r["dh0"][i], r["dc0"][i] = dh0[0], dc0[0]
    return r


def fusion(x, lens, method, d=None):
    """O.temporal_fusion of every clip's live prefix; with d [B, H] also its gradient [B, T, H] (dead steps 0)."""
    b, T, H = x.shape
    y = np.stack([O.temporal_fusion(x[i:i + 1, :int(lens[i])], method)[0] for i in range(b)])
    if d is None:
        return y
    g = np.zeros((b, T, H), F64)
    for i in range(b):
        L = int(lens[i])
        g[i, :L] = O.temporal_fusion_grad((1, L, H), method, d[i:i + 1].astype(F64))[0]
    return y, g


def live_rows(lens, T):
    """Boolean [B * T]: row b T + t is live iff t < lens[b]."""
    return (np.arange(T)[None, :] < np.asarray(lens)[:, None]).reshape(-1)


def xent(logits, onehot, lens, T):
    """O.softmax_xent_mean over the live rows -> (sum of their losses, hits among them, dlogits [rows, C] with zeros in dead rows,
    mean loss)."""
    m = live_rows(lens, T)
    loss, dl = O.softmax_xent_mean(logits[m], onehot[m])
    full = np.zeros(logits.shape, F64)
    full[m] = dl
    hits = float(np.sum(np.argmax(logits[m], 1) == np.argmax(onehot[m], 1)))
    return loss * int(m.sum()), hits, full, loss


# ---- engine level -------------------------------------------------------------------------------------------------------------------
def _pipe_item(p, scope, spec, x, T, state, V):
    """One pipeline on ONE item whose sequence has T steps: x = T frames (dcnn) or T vectors (nop); state [1, S] or None."""
    c = {"scope": scope, "spec": spec}
    if spec["representation"] == "dcnn":
        pd = O._sub(p, scope)
        feat, c["cnn"] = O.alexnet_forward(pd, x, spec["frame_encoding_layer"], F64, True)
    else:
        assert spec["representation"] == "nop" and spec.get("input_fusion") is None
        feat = x.astype(F64)
    hidden, layers, lfusion = spec["lstm_params"][:3]
    logits, c["lstm"] = O.lstm_classifier_forward(p, scope, feat, T, layers, lfusion, V, state=state)
    return logits, c


def _pipe_item_backward(p, c, dout):
    g, d, dstate = O.lstm_classifier_backward(p, c["lstm"], dout)
    if "cnn" in c:
        scope = c["scope"]
        gc = O.alexnet_backward(O._sub(p, scope), c["cnn"], d, c["spec"]["frame_encoding_layer"], F64)
        g.update({scope + k: v for k, v in gc.items()})
    return g, dstate


def model_with_lengths(p, case, feeds, lens, onehot=None, items=None):
    """The model of tests.graph_cases `case` with lengths lens = {pipeline: [items]} (a pipeline not named runs all its steps),
    item by item on the live prefixes.
    -> (logits of the live rows in batch order, live-row mask over the engine's logits rows, and with onehot [engine rows, V]:
        loss, gradients {name: array}, n rows the loss is a mean over)."""
    pipes, V = case["pipes"], case["V"]
    items = items or case["items"]
    scoped = len(pipes) > 1
    last_name, last = pipes[-1]
    per_step = last["lstm_params"][2] == "reshape"
    T_last = case["data"][last["input"][0]]["fpc"]
    L_last = np.asarray(lens.get(last_name, [T_last] * items))
    mask = live_rows(L_last, T_last) if per_step else np.ones(items, bool)
    n_rows = int(mask.sum())
    out_logits, caches = [], []
    for i in range(items):
        outs, cs = {}, {}
        for name, spec in pipes:
            tag = spec["input"][0]
            T = case["data"][tag]["fpc"]
            assert case["data"][tag]["cpv"] == 1
            L = int(lens[name][i]) if name in lens else T
            x = feeds[tag][i * T:i * T + L]
            state = outs[spec["input"][1]] if len(spec["input"]) > 1 else None
            outs[name], cs[name] = _pipe_item(p, name + "/" if scoped else "", spec, x, L, state, V)
        out_logits.append(outs[last_name])
        caches.append(cs)
    logits = np.concatenate(out_logits, axis=0)
    if onehot is None:
        return logits, mask
    loss, dlogits = O.softmax_xent_mean(logits, onehot[mask])          # mean over the n_rows live rows
    grads = {k: np.zeros(v.shape, F64) for k, v in p.items()}
    r0 = 0
    for i in range(items):
        n = out_logits[i].shape[0]
        dout = {last_name: dlogits[r0:r0 + n]}
        r0 += n
        for name, spec in reversed(pipes):
            if name not in dout:
                continue
            g, dstate = _pipe_item_backward(p, caches[i][name], dout[name])
            for k, v in g.items():
                grads[k] += v
            if len(spec["input"]) > 1 and dstate is not None:
                src = spec["input"][1]
                dout[src] = dout[src] + dstate if src in dout else dstate
    return logits, mask, loss, grads, n_rows


def single_lstm_case(fpc=6, fusion="last"):
    """One `dcnn -> lstm [6, 2, fusion]` pipeline (two layers) over clips of `fpc` frames."""
    return dict(pipes=[("net", dict(input=["main"], representation="dcnn", frame_encoding_layer="fc6", classifier="lstm",
                                    lstm_params=[6, 2, fusion]))],
                data={"main": dict(mode="video", fpc=fpc, cpv=1)}, V=7, items=5, seed=33)
