"""bench.py's plain run: one headline line and nothing else measured, and --dump-outputs writes what its LAST TIMED step computed --
the same warm-up + timed steps replayed here on the same inputs (frames default_rng(0), labels default_rng(1000), init_params seed 2,
dropout keep 0.5) give bitwise the same loss, accuracy, gradient norm, logits and parameters (the engine is reproducible run to run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIPS, STEPS, WARMUP = 8, 2, 1


def test_plain_run_dumps_its_last_timed_step(tmp_path):
    import bench
    from vltf_amd.engine import LRCNEngine, NetConfig, init_params
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["VLTF_NO_PRETOUCH"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--clips-per-gpu", str(CLIPS), "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--dump-outputs", str(tmp_path / "out")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.split("\n") if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == STEPS and d["warmup"] == WARMUP and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "clips/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["metric"].startswith("clips/sec")
    assert not {"roofline", "forward_only", "oracle_check", "bf16x3", "bf16x6", "bf16", "check", "cpu_baseline"} & set(d)
    files = sorted(os.listdir(tmp_path / "out"))
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in files}
    assert all(f.endswith(".npy") for f in files) and all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20

    cfg = NetConfig(image_shape=(227, 227, 3), num_classes=101, fpc=16, frame_encoding_layer="fc6", classifier="lstm", lstm_hidden=256,
                    lstm_layers=1, fusion="avg", dropout_keep_prob=0.5)
    eng = LRCNEngine(cfg, max_clips=CLIPS, device="cuda:0")
    eng.load_params(init_params(cfg, seed=2))
    frames = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (CLIPS * 16, 227, 227, 3), dtype=np.uint8)).to("cuda:0")
    onehot = torch.zeros((CLIPS, 101), dtype=torch.int32)
    onehot[torch.arange(CLIPS), torch.from_numpy(np.random.default_rng(1000).integers(0, 101, CLIPS))] = 1
    onehot = onehot.to("cuda:0")
    for i in range(WARMUP + STEPS):
        out = eng.train_step_u8(frames, onehot, lr=1e-3, clip_norm=10.0, mean_bgr=bench.MEAN_BGR, fetch=i == WARMUP + STEPS - 1)
    want = bench.step_outputs(eng)
    assert sorted(want) == sorted(got)
    assert (got["loss"], got["accuracy"], got["grad_norm"]) == (out["loss"], out["accuracy"], out["grad_norm"])
    np.testing.assert_array_equal(got["logits"], eng.logits_host())
    params = eng.get_params()
    np.testing.assert_array_equal(got["param_dcnn_conv1W"], params["dcnn/conv1W"])
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
