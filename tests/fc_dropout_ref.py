"""Restatements for the fc6 / fc7 dropout tests (no tests here).

keep_mask: the mask definition of vl_fc_dropout_fwd (include/vltf.h) in numpy uint64 arithmetic with a float32 compare --
the device must equal it exactly.  masked_step: the model with those masks behind relu(fc6) / relu(fc7) in torch fp64 on the CPU,
built from the pieces of oracle.torch_cpu; autograd gives the gradients, the clipped-SGD update is spelled out."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import lrcn_oracle as O
from oracle import torch_cpu as TC

FC_DIM = 4096
_M64 = (1 << 64) - 1


def _splitmix64_int(z):
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def splitmix64(z):
    """The generator of csrc/pointwise.hip on a uint64 array (arithmetic mod 2^64)."""
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def keep_mask(seed, salt, count, keep):
    """bool[count]: element e (counted from the pointer the launch gets) is kept."""
    s = np.uint64((int(seed) & _M64) ^ _splitmix64_int((0xFC00 + int(salt)) & _M64))
    h = splitmix64(s ^ splitmix64(np.arange(count, dtype=np.uint64)))
    uni = (h >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)       # 24 bits: exact in float32
    return uni < np.float32(keep)


def engine_mask(cfg, layer, draw_index, n, keep=None):
    """bool[n, 4096]: what an engine of this config keeps of `layer` ("fc6" | "fc7") over n frames at this draw index."""
    from vltf_amd.engine import dropout_seed, fc_dropout_salt
    keep = cfg.fc_dropout_keep_prob if keep is None else keep
    return keep_mask(dropout_seed(draw_index), fc_dropout_salt(cfg, layer), n * FC_DIM, keep).reshape(n, FC_DIM)


def masked_dcnn_features(p, scope, frames, final_layer, keep, masks):
    """oracle.torch_cpu.dcnn_features with y = relu(z) * mask / keep behind fc6 and fc7; masks: {"fc6" | "fc7": bool[n, 4096]}."""
    a = frames
    for name, kh, kw, co, s, g in O.ALEXNET_CONVS:
        a = torch.relu(TC.conv_same(a, p[scope + "dcnn/%sW" % name], s, g) + p[scope + "dcnn/%sb" % name])
        if name in ("conv1", "conv2"):
            a = F.local_response_norm(a.permute(0, 3, 1, 2), 5, alpha=1e-4, beta=0.75, k=1.0).permute(0, 2, 3, 1)
        if name in ("conv1", "conv2", "conv5"):
            a = F.max_pool2d(a.permute(0, 3, 1, 2), 3, 2).permute(0, 2, 3, 1)
    drop = lambda v, layer: v * torch.from_numpy(masks[layer]).to(v.dtype) / keep
    a = drop(torch.relu(a.reshape(a.shape[0], -1) @ p[scope + "dcnn/fc6W"] + p[scope + "dcnn/fc6b"]), "fc6")
    if final_layer != "fc6":
        a = drop(torch.relu(a @ p[scope + "dcnn/fc7W"] + p[scope + "dcnn/fc7b"]), "fc7")
    if final_layer not in ("fc6", "fc7"):
        a = a @ p[scope + "dcnn/fc8W"] + p[scope + "dcnn/fc8b"]
    return a


def masked_logits(p, frames, fpc, keep, masks, final_layer="fc6", lstm_layers=1, fusion="avg", classifier="lstm", frame_fusion=None,
                  num_classes=None):
    """oracle.torch_cpu.lrcn_logits over the masked tower, from that module's pieces."""
    v = masked_dcnn_features(p, "", frames, final_layer, keep, masks)
    if classifier == "fc":
        early = bool(frame_fusion) and frame_fusion[0] == "early" and fpc > 1
        late = bool(frame_fusion) and frame_fusion[0] == "late" and fpc > 1
        if early:
            v = TC._fuse_time(v, fpc, frame_fusion[1])
        v = TC._fc(p, "fc_convert", v, num_classes)
        return TC._fuse_time(v, fpc, frame_fusion[1]) if late else v
    return TC.lstm_classifier(p, "", v, fpc, lstm_layers, fusion, num_classes)


def sgd_step(params, logits_fn, onehot, lr, clip_norm, frozen=()):
    """One clipped-SGD step in fp64.  params: {name: float32 array}; logits_fn(p: {name: fp64 leaf tensor}) -> logits.
    Returns (new params, loss, global grad norm, logits, grads) as numpy; names in `frozen` get no gradient and stay."""
    p = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=k not in frozen) for k, v in params.items()}
    logits = logits_fn(p)
    loss = F.cross_entropy(logits, torch.from_numpy(np.argmax(onehot, 1)))
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for k, v in p.items() if k not in frozen}
    gn = float(np.sqrt(sum((g ** 2).sum() for g in grads.values())))
    scale = clip_norm / max(gn, clip_norm) if clip_norm > 0 else 1.0
    newp = {k: (v.detach().numpy() - lr * scale * grads[k]) if k in grads else v.detach().numpy() for k, v in p.items()}
    return newp, float(loss.detach()), gn, logits.detach().numpy(), grads
