#!/usr/bin/env python3
"""What two train steps of every temporal model and pooling over time compute, as one SHA-256 per case: for comparing two checkouts.

The temporal models (bidirectional LSTM, GRU, self-attention plain and as the encoder block, the dilated convolutions) and the poolings
(avg, attn, vlad) run through both engines.  Only the public engine API is used (LRCNEngine, GraphEngine, init_params,
init_params_for), so this file runs unmodified in a checkout from before vltf_amd/temporal.py existed.  A case is two train steps
from fixed seeds; its digest is over the raw bytes of the logits, of every gradient and of every parameter (both in flat-buffer order)
after each step.

LRCNEngine, the smoke geometry of the model tests (67 x 67 x 3 images, 3 frames per clip, 2 clips, 7 classes, two layers; H = 8, 16
for self-attention, whose heads are 8 wide at least), each case eager and with step_graph:
  cell {blstm, gru, mhsa, mhsa without positions, mhsa with sa_attn_dropout, encoder, tcn} x fusion {avg, attn, vlad}, where the
  engine admits the pair (a refused pair is left out: both checkouts refuse the same ones, or the files differ);
  per cell one case with the tower frozen (train_from classifier: nobody reads the gradient of the features);
  gru with fusion reshape, blstm with fusion last, gru on conv_math bf16.
GraphEngine:
  the same cells on a vector-input `nop` pipeline (T = 5, 4 clips, dim 10; H = 6, 16 for self-attention and the convolutions as
  in their tests) x fusion {avg, attn, vlad}, without lengths and with the lengths [5, 2, 1, 4] -- the input takes no gradient;
  per cell a two-pipeline model, a dcnn tower whose fc6 features feed the temporal pipeline -- the input takes one.

The launches are deterministic, so two checkouts that compute the same thing write the same file:

    (cd /path/to/other/checkout && python tools/temporal_bits.py --out a.json)
    python tools/temporal_bits.py --out b.json && cmp a.json b.json

No CPU fallback.
usage: temporal_bits.py [--out FILE]"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from vltf_amd._ffi import VltfError
from vltf_amd.engine import LRCNEngine, NetConfig, init_params
from vltf_amd.graph import DatasetInfo, GraphEngine, PipelineSpec, init_params_for

DEV = "cuda:0"
SHAPE, NCLS, FPC, CLIPS, LAYERS = (67, 67, 3), 7, 3, 2, 2
MEAN = np.array([99.197148, 105.293620, 109.503945], np.float32)
G_T, G_CLIPS, G_DIM, G_C, G_LENS = 5, 4, 10, 5, [5, 2, 1, 4]
FUSIONS = ("avg", "attn", "vlad")
STEPS = 2

# cell name -> (the keys of NetConfig / PipelineSpec, H of LRCNEngine, H of the vector pipeline)
CELLS = {
    "blstm": (dict(lstm_bidirectional=True), 8, 6),
    "gru": (dict(rnn_cell="gru"), 8, 6),
    "mhsa": (dict(rnn_cell="mhsa", sa_heads=2), 16, 16),
    "mhsa nopos": (dict(rnn_cell="mhsa", sa_heads=2, sa_positions="none"), 16, 16),
    "mhsa attn-drop": (dict(rnn_cell="mhsa", sa_heads=2, sa_attn_dropout=0.3), 16, 16),
    "encoder": (dict(rnn_cell="mhsa", sa_heads=2, sa_block="encoder", sa_ffn_dim=24), 16, 16),
    "tcn": (dict(rnn_cell="tcn"), 8, 16),
}


class Refused(Exception):
    """the engine does not admit the case (raised by its constructor, before a launch)"""


def admitted(make):
    try:
        return make()
    except VltfError as e:
        raise Refused(str(e))


def digest_step(h, eng):
    h.update(eng.logits_host().tobytes())
    for table in (eng.get_grads(), eng.get_params()):
        for name, _ in eng.specs:
            if name in table:
                h.update(np.ascontiguousarray(table[name]).tobytes())


def nonzero_biases(p):
    """biases that are not zero: a bias gradient on the wrong bias would show"""
    for k in sorted(p):
        if k.endswith("bias") or k.endswith("beta"):
            p[k] = (0.1 * np.random.default_rng(len(k)).standard_normal(p[k].shape)).astype(np.float32)
    return p


def lrcn_case(H, fusion, step_graph, **keys):
    cfg = NetConfig(image_shape=SHAPE, num_classes=NCLS, fpc=FPC, frame_encoding_layer="fc6", classifier="lstm", lstm_hidden=H,
                    lstm_layers=LAYERS, fusion=fusion, step_graph=step_graph, **keys)
    eng = admitted(lambda: LRCNEngine(cfg, max_clips=CLIPS, device=DEV))
    eng.load_params(nonzero_biases(init_params(cfg, seed=4, well_scaled=True)))
    rng = np.random.default_rng(11)
    h = hashlib.sha256()
    for step in range(STEPS):
        frames = torch.from_numpy(rng.integers(0, 256, (CLIPS * FPC,) + SHAPE, dtype=np.uint8)).to(DEV)
        rows = CLIPS * FPC if fusion == "reshape" else CLIPS
        onehot = torch.from_numpy(np.eye(NCLS, dtype=np.int32)[rng.integers(0, NCLS, rows)]).to(DEV)
        eng.train_step_u8(frames, onehot, 0.01 * 0.7 ** step, 5.0, MEAN)
        digest_step(h, eng)
    return h.hexdigest()


def graph_run(eng, feeds_of, rows, seq_len=None):
    eng.load_params(nonzero_biases(init_params_for(eng.specs, seed=3, well_scaled=True)))
    rng = np.random.default_rng(8)
    h = hashlib.sha256()
    for step in range(STEPS):
        feeds = feeds_of(rng)
        onehot = torch.from_numpy(np.eye(G_C, dtype=np.int32)[rng.integers(0, G_C, rows)]).to(DEV)
        eng.train_step(feeds, onehot, 0.01 * 0.7 ** step, 5.0, **({"seq_len": seq_len} if seq_len else {}))
        digest_step(h, eng)
    return h.hexdigest()


def vector_case(H, fusion, lens, **keys):
    pipes = [PipelineSpec("net", ["main"], "nop", classifier="lstm", lstm_params=(H, LAYERS, fusion), **keys)]
    eng = admitted(lambda: GraphEngine(pipes, {"main": DatasetInfo("vectors", G_T, 1, G_CLIPS, dim=G_DIM)}, G_C, device=DEV))
    feeds_of = lambda rng: {"main": torch.from_numpy(rng.standard_normal((G_CLIPS * G_T, G_DIM)).astype(np.float32)).to(DEV)}
    return graph_run(eng, feeds_of, G_CLIPS, {"net": lens} if lens else None)


def tower_case(H, fusion, **keys):
    pipes = [PipelineSpec("feat", ["main"], "dcnn", frame_encoding_layer="fc6", classifier=None),
             PipelineSpec("net", ["feat"], "nop", classifier="lstm", lstm_params=(H, LAYERS, fusion), **keys)]
    eng = admitted(lambda: GraphEngine(pipes, {"main": DatasetInfo("video", FPC, 1, CLIPS, image_shape=SHAPE)}, G_C, device=DEV))
    feeds_of = lambda rng: {"main": dict(mean_bgr=MEAN, frames_u8=torch.from_numpy(
        rng.integers(0, 256, (CLIPS * FPC,) + SHAPE, dtype=np.uint8)).to(DEV))}
    return graph_run(eng, feeds_of, CLIPS)


def cases():
    """(name, function) of every case, in the file's order"""
    for cell, (keys, H, _) in CELLS.items():
        for fusion in FUSIONS:
            for sg in (False, True):
                yield "lrcn %s, %s, %s" % (cell, fusion, "captured" if sg else "eager"), lambda H=H, fusion=fusion, sg=sg, keys=keys: \
                    lrcn_case(H, fusion, sg, **keys)
        for sg in (False, True):
            yield "lrcn %s, avg, frozen tower, %s" % (cell, "captured" if sg else "eager"), lambda H=H, sg=sg, keys=keys: \
                lrcn_case(H, "avg", sg, train_from="classifier", **keys)
    for sg in (False, True):
        form = "captured" if sg else "eager"
        yield "lrcn gru, reshape, " + form, lambda sg=sg: lrcn_case(8, "reshape", sg, rnn_cell="gru")
        yield "lrcn blstm, last, " + form, lambda sg=sg: lrcn_case(8, "last", sg, lstm_bidirectional=True)
        yield "lrcn gru, avg, conv_math bf16, " + form, lambda sg=sg: lrcn_case(8, "avg", sg, rnn_cell="gru", conv_math="bf16")
    for cell, (keys, _, H) in CELLS.items():
        for fusion in FUSIONS:
            for lens in (None, G_LENS):
                yield "graph vectors %s, %s, %s" % (cell, fusion, "lengths" if lens else "no lengths"), \
                    lambda H=H, fusion=fusion, lens=lens, keys=keys: vector_case(H, fusion, lens, **keys)
        yield "graph tower %s, avg" % cell, lambda H=H, keys=keys: tower_case(H, "avg", **keys)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="the digests as JSON (default: standard output)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("temporal_bits.py needs a HIP device; there is no CPU fallback")
    t0 = time.time()
    digests, refused = {}, []
    for name, run in cases():
        try:
            digests[name] = run()
        except Refused as e:
            refused.append("%s: %s" % (name, str(e)[:100]))
    text = json.dumps(digests, indent=1) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    print("%d cases in %.1f s, %d refused" % (len(digests), time.time() - t0, len(refused)), file=sys.stderr)
    for r in refused:
        print("refused " + r, file=sys.stderr)


if __name__ == "__main__":
    main()
