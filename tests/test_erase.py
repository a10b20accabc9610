"""Random erasing on the host: check_erase, the draws of erase_row against an independent restatement (tests/erase_ref.py) and their
properties, the caller's box check, the moments of the reference noise, the YAML keys with their refusals and the getter outside the
train phase, the C-ABI rows and the entry points' argument checks, the example, and the refusals of GraphEngine and run_task ahead of
any device call.  No GPU: nothing is launched.

Noise moments.  noise is a centred sum of four uniform 16-bit fields times std / 37837.227...: over n = 3 * 3 * 67 * 67 = 40401
elements the mean of a perfect generator has a standard error of std / sqrt(n) = 0.005 std and the standard deviation one of about
std / sqrt(2 n) = 0.0035 std; the bounds are 0.05 std and 2 %, ten and six standard errors."""
import os

import numpy as np
import pytest
import yaml

from tests import erase_ref as ER
from tests.test_ema import _val_settings
from tests.test_finetune import _settings
from vltf_amd._ffi import VltfError
from vltf_amd.engine import ERASE_MODES, EraseConfig, NetConfig, check_erase, check_erase_boxes, erase_config, erase_row, erase_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("erase_prob", "erase_scale", "erase_ratio", "erase_frames", "erase_mode", "erase_std", "erase_seed")
OFF = (0.0, None, None, None, None, None, 0)
DEFAULT = EraseConfig(0.0, (0.02, 0.33), (0.3, 3.3), (1.0, 1.0), "zero", 57.63, 0)
GEOMS = ((3, 67, 67), (16, 227, 227))
COMBOS = [(seed, draw, clip) for seed in (0, 7) for draw in (0, 1, 5) for clip in range(8)]


# ---- check_erase ----------------------------------------------------------------------------------------------------------------------
def test_check_erase_accepts_and_off_is_the_default():
    assert check_erase() == DEFAULT and check_erase(None, None, None, None, None, None, None) == DEFAULT and check_erase(0, seed=0) == DEFAULT
    assert check_erase(0.25) == DEFAULT._replace(prob=0.25)
    e = check_erase(1, [0.1, 0.2], (1, 2), (0.5, 1), "pixel", 10, 2 ** 64 - 1)
    assert e == EraseConfig(1.0, (0.1, 0.2), (1.0, 2.0), (0.5, 1.0), "pixel", 10.0, 2 ** 64 - 1)
    assert isinstance(e.prob, float) and isinstance(e.std, float) and isinstance(e.seed, int) and isinstance(e.scale[0], float)
    assert check_erase(np.float32(0.5), np.array([0.1, 0.1]), std=np.float64(0.0), seed=np.int64(3), mode="clip").seed == 3
    assert check_erase(0.5, seed=5.0).seed == 5
    cfg = NetConfig()
    assert cfg.erase_prob == 0 and tuple(getattr(cfg, k) for k in KEYS) == OFF
    assert erase_config(cfg) == DEFAULT and erase_config(NetConfig(erase_prob=0.5, erase_mode="clip")).mode == "clip"
    assert ERASE_MODES == ("zero", "clip", "pixel") == ER.MODES


@pytest.mark.parametrize("kw,name", [
    (dict(prob=-0.1), "erase_prob"), (dict(prob=1.5), "erase_prob"), (dict(prob=float("nan")), "erase_prob"), (dict(prob=True), "erase_prob"),
    (dict(prob="0.5"), "erase_prob"), (dict(prob=[0.5]), "erase_prob"),
    (dict(prob=0.5, scale=(0.0, 0.3)), "erase_scale"), (dict(prob=0.5, scale=(0.4, 0.3)), "erase_scale"),
    (dict(prob=0.5, scale=(0.1, 1.5)), "erase_scale"), (dict(prob=0.5, scale=0.3), "erase_scale"), (dict(prob=0.5, scale=(0.1, 0.2, 0.3)), "erase_scale"),
    (dict(prob=0.5, scale=("0.1", 0.3)), "erase_scale"), (dict(prob=0.5, scale=(True, 1)), "erase_scale"), (dict(prob=0.5, scale="ab"), "erase_scale"),
    (dict(prob=0.5, scale=(0.1, float("nan"))), "erase_scale"),
    (dict(prob=0.5, ratio=(0.0, 2.0)), "erase_ratio"), (dict(prob=0.5, ratio=(3.0, 2.0)), "erase_ratio"), (dict(prob=0.5, ratio=(-1, 2.0)), "erase_ratio"),
    (dict(prob=0.5, ratio=(1.0, float("inf"))), "erase_ratio"),
    (dict(prob=0.5, frames=(0.5, 1.5)), "erase_frames"), (dict(prob=0.5, frames=(0, 1)), "erase_frames"), (dict(prob=0.5, frames=(1, 0.5)), "erase_frames"),
    (dict(prob=0.5, mode="noise"), "erase_mode"), (dict(prob=0.5, mode=2), "erase_mode"),
    (dict(prob=0.5, std=-1.0), "erase_std"), (dict(prob=0.5, std=float("inf")), "erase_std"), (dict(prob=0.5, std=float("nan")), "erase_std"),
    (dict(prob=0.5, std="57"), "erase_std"), (dict(prob=0.5, std=False), "erase_std"),
    (dict(prob=0.5, seed=-1), "erase_seed"), (dict(prob=0.5, seed=2 ** 64), "erase_seed"), (dict(prob=0.5, seed=1.5), "erase_seed"),
    (dict(prob=0.5, seed="7"), "erase_seed"), (dict(prob=0.5, seed=True), "erase_seed"),
    (dict(scale=(0.1, 0.2)), "erase_scale is given without erase_prob"), (dict(prob=0, ratio=(1, 2)), "erase_ratio is given without erase_prob"),
    (dict(frames=(1, 1)), "erase_frames is given without erase_prob"), (dict(prob=0.0, mode="zero"), "erase_mode is given without erase_prob"),
    (dict(std=57.63), "erase_std is given without erase_prob"), (dict(prob=None, seed=7), "erase_seed is given without erase_prob")])
def test_check_erase_refuses(kw, name):
    with pytest.raises(VltfError, match=name):
        check_erase(**kw)


def test_check_erase_boxes():
    assert check_erase_boxes([(0, 3, 0, 9, 0, 11), (0, 0, 0, 0, 0, 0)], 2, 3, 9, 11) == [(0, 3, 0, 9, 0, 11), (0, 0, 0, 0, 0, 0)]   # no half-volume rule
    assert check_erase_boxes(np.array([[1, 2, 3, 4, 5, 6]]), 1, 3, 9, 11) == [(1, 2, 3, 4, 5, 6)]
    for bad, msg in (([(0, 3, 0, 9, 0, 11)], "must be 2 boxes"), (None, "must be 2 boxes"), ((0, 3, 0, 9, 0, 11), "must be 2 boxes"),
                     ([(0, 3, 0, 9, 0), (0,) * 6], "box 0 must be six whole numbers"), ([(0,) * 6, (0, 1.5, 0, 1, 0, 1)], "box 1 must be six"),
                     ([(0,) * 6, (0, 4, 0, 1, 0, 1)], "box 1: the t range .* leaves"), ([(0, 3, -1, 1, 0, 1), (0,) * 6], "box 0: the y range .* leaves"),
                     ([(0, 3, 0, 1, 0, 12), (0,) * 6], "the x range .* leaves"), ([(2, 1, 0, 1, 0, 1), (0,) * 6], "is reversed")):
        with pytest.raises(VltfError, match=msg):
            check_erase_boxes(bad, 2, 3, 9, 11)


# ---- erase_row ------------------------------------------------------------------------------------------------------------------------
def _ref_row(e, draw, clip, fpc, h, w):
    return ER.erase_row(e.prob, e.scale, e.ratio, e.frames, e.seed, draw, clip, fpc, h, w)


@pytest.mark.parametrize("fpc,h,w", GEOMS)
def test_erase_row_agrees_with_the_reference_and_is_pure(fpc, h, w):
    assert len(COMBOS) == 48 and len({c[:2] for c in COMBOS}) * 8 == 48
    erased = 0
    for kw in (dict(prob=0.5), dict(prob=1.0, frames=(0.3, 1.0), scale=(0.02, 0.9), ratio=(0.1, 8.0))):
        rows = set()
        for seed, draw, clip in COMBOS:
            e = check_erase(seed=seed or None, **kw)
            row = erase_row(e, draw, clip, fpc, h, w)
            assert row == _ref_row(e, draw, clip, fpc, h, w), (seed, draw, clip)
            assert row == erase_row(e, draw, clip, fpc, h, w) and len(row) == 8 and all(isinstance(v, int) for v in row)
            assert row == erase_row(NetConfig(erase_prob=e.prob, erase_scale=e.scale, erase_ratio=e.ratio, erase_frames=e.frames,
                                              erase_seed=e.seed), draw, clip, fpc, h, w)
            t0, t1, y0, y1, x0, x1 = row[:6]
            assert all(-2 ** 31 <= v < 2 ** 31 for v in row[6:])
            if row[:6] != (0,) * 6:
                erased += 1
                assert 0 <= t0 < t1 <= fpc and 0 <= y0 < y1 <= h and 0 <= x0 < x1 <= w and y1 - y0 < h and x1 - x0 < w
                if "frames" not in kw:
                    assert (t0, t1) == (0, fpc)                                           # frames (1, 1): every frame
            rows.add(row)
        assert len(rows) == len(COMBOS)                                                   # the keys alone tell any two apart
    assert erased > len(COMBOS)                                                           # both settings erased, the second one always


@pytest.mark.parametrize("fpc,h,w", GEOMS)
def test_erase_row_at_the_ends_of_prob(fpc, h, w):
    side = int(round(np.sqrt(0.1 * h * w)))
    for seed, draw, clip in COMBOS:
        off = erase_row(check_erase(0.0), draw, clip, fpc, h, w)
        assert off[:6] == (0,) * 6
        e = check_erase(1.0, (0.1, 0.1), (1, 1), seed=seed or None)
        t0, t1, y0, y1, x0, x1, lo, hi = erase_row(e, draw, clip, fpc, h, w)
        assert (t0, t1, y1 - y0, x1 - x0) == (0, fpc, side, side) and 0 <= y0 <= h - side and 0 <= x0 <= w - side
        assert (lo, hi) == erase_row(e._replace(prob=0.5), draw, clip, fpc, h, w)[6:]     # the key does not depend on the rest
        if seed == 0:
            assert (lo, hi) == off[6:]


def test_two_ranks_share_a_batch_of_eight():
    e = check_erase(0.7, seed=7, mode="pixel")
    whole = erase_table(e, 5, 0, 8, 3, 67, 67)
    assert whole.dtype == np.int32 and whole.shape == (8, 8)
    assert [tuple(r) for r in whole] == [erase_row(e, 5, i, 3, 67, 67) for i in range(8)]
    r0, r1 = erase_table(e, 5, 0, 4, 3, 67, 67), erase_table(e, 5, 1, 4, 3, 67, 67)
    assert np.array_equal(r0, whole[:4]) and np.array_equal(r1, whole[4:]) and not np.array_equal(r0, r1)
    assert np.array_equal(erase_table(e, 5, 1, 4, 3, 67, 67, clips=2), whole[4:6])         # a short last batch keeps its clips' rows
    given = erase_table(e, 5, 1, 4, 3, 67, 67, boxes=[(0, 1, 2, 3, 4, 5)] * 4)
    assert np.array_equal(given[:, 6:], whole[4:, 6:]) and (given[:, :6] == (0, 1, 2, 3, 4, 5)).all()
    assert not np.array_equal(erase_table(e, 4, 0, 8, 3, 67, 67), whole)                  # another micro-step, another table


# ---- the reference noise --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [7, 0, 2 ** 63 + 5])
def test_reference_noise_moments(key):
    std = 57.63
    scale = ER.scale_of(std)
    v = ER.fill((3, 67, 67, 3), key, 2, scale)
    assert v.dtype == np.float32 and v.shape == (3, 67, 67, 3)
    mean, dev = float(v.astype(np.float64).mean()), float(v.astype(np.float64).std())
    print("key %d: mean / std %.4f, std ratio %.4f" % (key, mean / std, dev / std))
    assert abs(mean) <= 0.05 * std and abs(dev / std - 1.0) <= 0.02
    assert (np.abs(v) <= np.float32(131070) * scale).all()
    assert len(np.unique(v)) > 10000                                                      # a value per element, not per row
    per_clip = ER.fill((3, 67, 67, 3), key, 1, scale)
    assert (per_clip == per_clip[0, 0, 0]).all() and len(set(per_clip[0, 0, 0].tolist())) == 3
    assert not ER.fill((3, 67, 67, 3), key, 0, scale).any()


def test_reference_pieces():
    assert int(ER.splitmix64(0)) == 0xE220A8397B1DCDAF and int(ER.splitmix64(1)) == 0x910A2DEC89025CC1   # the published first outputs
    assert ER.key_of((0, 0, 0, 0, 0, 0, -1, 1)) == (1 << 32) | 0xFFFFFFFF and ER.key_words((1 << 32) | 0xFFFFFFFF) == (-1, 1)
    assert ER.clamp((-5, 99, -1, 6, 3, 400, 1, 2), 3, 9, 11) == (0, 3, 0, 6, 3, 11) and ER.clamp((0, 3, 7, 2, 0, 11), 3, 9, 11) == (0,) * 6
    # round to nearest even: 1 + 2^-8 is a tie and goes to the even 1.0, 1 + 3 * 2^-8 goes up to 1 + 2^-6
    got = ER.bf16_bits(np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -0.0, 0.0, 1.0 + 2.0 ** -8 + 2.0 ** -20], np.float32))
    assert got.tolist() == [0x3F80, 0x3F80, 0x3F82, 0x8000, 0x0000, 0x3F81]
    x = np.arange(2 * 3 * 4 * 5 * 3, dtype=np.float32).reshape(2, 3, 4, 5, 3) + 1
    table = np.array([[1, 3, 1, 3, 2, 5, 9, 0], [0, 3, 0, 4, 0, 0, 9, 0]], np.int32)
    y = ER.erase(x, table, 0, ER.scale_of(1.0))
    assert not y[0, 1:3, 1:3, 2:5].any() and np.count_nonzero(y == 0) == 2 * 2 * 3 * 3 and np.array_equal(y[1], x[1])


# ---- YAML -------------------------------------------------------------------------------------------------------------------------------
def test_settings_keys_parse(tmp_path):
    from vltf_amd import run_task
    train = dict(erase_prob=0.25, erase_scale=[0.05, 0.2], erase_ratio=[0.5, 2.0], erase_frames=[0.5, 1.0], erase_mode="pixel", erase_std=30,
                 erase_seed=7)
    s = _settings(tmp_path, train=train)
    assert s.get_erase() == (0.25, (0.05, 0.2), (0.5, 2.0), (0.5, 1.0), "pixel", 30.0, 7)
    s = _settings(tmp_path, train={"erase_prob": "2.5e-1", "erase_std": "30", "erase_seed": "7"})       # quoted numbers
    assert s.get_erase() == (0.25, (0.02, 0.33), (0.3, 3.3), (1.0, 1.0), "zero", 30.0, 7)
    assert _settings(tmp_path, train={"erase_prob": 1}).get_erase() == tuple(DEFAULT._replace(prob=1.0))


def test_net_config_carries_the_keys(tmp_path):
    from tests.test_scale_jitter import _settings as data_settings
    from vltf_amd import run_task
    s, feeder = data_settings(tmp_path)
    dataset = feeder.get_dataset_by_tag("main")[0]
    assert tuple(getattr(run_task.net_config(s, dataset)[0], k) for k in KEYS) == OFF
    s.train.erase = tuple(check_erase(0.25, mode="clip", seed=7))
    cfg = run_task.net_config(s, dataset)[0]
    assert tuple(getattr(cfg, k) for k in KEYS) == (0.25, (0.02, 0.33), (0.3, 3.3), (1.0, 1.0), "clip", 57.63, 7)
    assert erase_config(cfg) == check_erase(0.25, mode="clip", seed=7)


@pytest.mark.parametrize("train", [{}, dict.fromkeys(KEYS), dict.fromkeys(KEYS, "None"), {"erase_prob": 0, "erase_seed": 0}, {"erase_prob": "None"}],
                         ids=["absent", "null", "None-strings", "zeros", "None-prob"])
def test_settings_absent_keys_mean_off(tmp_path, train):
    assert _settings(tmp_path, train=train).get_erase() == OFF


@pytest.mark.parametrize("train,name", [
    ({"erase_prob": -0.5}, "erase_prob"), ({"erase_prob": 2}, "erase_prob"), ({"erase_prob": "often"}, "erase_prob"), ({"erase_prob": True}, "erase_prob"),
    ({"erase_prob": 0.5, "erase_scale": [0.3, 0.1]}, "erase_scale"), ({"erase_prob": 0.5, "erase_scale": [0.1, 1.5]}, "erase_scale"),
    ({"erase_prob": 0.5, "erase_scale": 0.3}, "erase_scale"), ({"erase_prob": 0.5, "erase_ratio": [0, 2]}, "erase_ratio"),
    ({"erase_prob": 0.5, "erase_frames": [0.5, 2]}, "erase_frames"), ({"erase_prob": 0.5, "erase_mode": "noise"}, "erase_mode"),
    ({"erase_prob": 0.5, "erase_std": -3}, "erase_std"), ({"erase_prob": 0.5, "erase_std": "loud"}, "erase_std"),
    ({"erase_prob": 0.5, "erase_seed": -1}, "erase_seed"), ({"erase_prob": 0.5, "erase_seed": 1.5}, "erase_seed"),
    ({"erase_mode": "pixel"}, "erase_mode is given without erase_prob"), ({"erase_prob": "None", "erase_seed": 7}, "erase_seed is given without")])
def test_settings_refusals(tmp_path, train, name):
    with pytest.raises(Exception, match="train.erase_prob / .*%s" % name):
        _settings(tmp_path, train=train)


def test_settings_outside_the_train_phase_is_off(tmp_path):
    s = _val_settings(tmp_path, train={"erase_prob": 0.5, "erase_mode": "pixel", "erase_seed": 7})
    assert s.get_erase() == OFF


def test_example_yaml_is_the_cutmix_one_with_the_erase_keys(tmp_path):
    here = os.path.join(ROOT, "examples")
    with open(os.path.join(here, "lrcn_erase.yml")) as f:
        er = yaml.safe_load(f)
    with open(os.path.join(here, "lrcn_cutmix.yml")) as f:
        base = yaml.safe_load(f)
    t = er["run"]["train"]
    got = {k: t.pop(k) for k in KEYS}
    assert got == dict(erase_prob=0.25, erase_scale=[0.02, 0.33], erase_ratio=[0.3, 3.3], erase_frames=[1.0, 1.0], erase_mode="pixel",
                       erase_std=57.63, erase_seed=7)
    for cfg in (er, base):
        cfg["run"].pop("run_folder", None), cfg["run"].pop("run_id", None)
    assert er == base                                                                    # mixup and CutMix stay on: the example runs all three
    s = _settings(tmp_path, train=got)
    assert s.get_erase() == (0.25, (0.02, 0.33), (0.3, 3.3), (1.0, 1.0), "pixel", 57.63, 7)


# ---- C-ABI ------------------------------------------------------------------------------------------------------------------------------
def test_ffi_rows_and_ops_names():
    from tests.test_mixup import _header_arg_count
    from vltf_amd import _ffi
    import vltf_amd.ops as ops
    p, i32, f32 = _ffi.p, _ffi.i32, _ffi.f32
    assert _ffi.SIGNATURES["vl_erase_boxes"] == (i32, [p, i32, i32, i32, i32, i32, i32, p, i32, f32, p])
    assert _ffi.SIGNATURES["vl_erase_boxes_s2d"] == (i32, [p, p, i32, i32, p, i32, f32, p])
    for name in ("vl_erase_boxes", "vl_erase_boxes_s2d"):
        assert len(_ffi.SIGNATURES[name][1]) == _header_arg_count(name), name
    assert callable(ops.erase_boxes) and callable(ops.Conv.erase_boxes_s2d)
    assert ops.erase_scale(57.63) == float(ER.scale_of(57.63)) and ops.ERASE_SUM_STD == ER.SUM_STD == np.sqrt(4 * (65536.0 ** 2 - 1) / 12)


def test_host_refusals_need_no_device():
    """Both launches validate before they launch, each refusal with a message of its own.  Nothing runs."""
    from vltf_amd import _ffi
    lib = _ffi.lib()
    fake = 4096                                  # a non-null, aligned address: validation fails before anything dereferences it
    ok = dict(x=fake, clips=2, fpc=3, h=9, w=11, halo=2, phase=4, table=fake, mode=2, scale=1.0)
    for change, msg in ((dict(x=None), b"x0 is null"), (dict(table=None), b"table_dev is null"), (dict(clips=-1), b"clips must be >= 0"),
                        (dict(fpc=0), b"fpc must lie in"), (dict(fpc=65536), b"fpc must lie in"), (dict(h=0), b"bad frame size"),
                        (dict(w=-11), b"bad frame size"), (dict(halo=-1), b"halo must be >= 0"), (dict(phase=0), b"phase must be >= 1"),
                        (dict(mode=3), b"mode must be 0"), (dict(mode=-1), b"mode must be 0"), (dict(scale=float("nan")), b"scale must be finite"),
                        (dict(scale=float("inf")), b"scale must be finite"), (dict(x=fake + 2), b"not 4-byte aligned")):
        a = dict(ok, **change)
        assert lib.vl_erase_boxes(a["x"], a["clips"], a["fpc"], a["h"], a["w"], a["halo"], a["phase"], a["table"], a["mode"], a["scale"],
                                  None) != 0, change
        err = lib.vl_last_error()
        assert b"vl_erase_boxes" in err and msg in err, (change, err)
    assert lib.vl_erase_boxes(fake, 0, 3, 9, 11, 2, 4, fake, 2, 1.0, None) == 0            # no clips: accepted, the addresses are never touched
    for args, msg in (((None, None, 2, 3, fake, 0, 1.0), b"xb is null"), ((None, fake, 2, 3, None, 0, 1.0), b"table_dev is null"),
                      ((None, fake, -1, 3, fake, 0, 1.0), b"clips must be >= 0"), ((None, fake, 2, 0, fake, 0, 1.0), b"fpc must lie in"),
                      ((None, fake, 2, 3, fake, 0, 1.0), b"vl_erase_boxes_s2d: a strided, ungrouped, square layer")):
        assert lib.vl_erase_boxes_s2d(*args, None) != 0 and msg in lib.vl_last_error(), args


# ---- GraphEngine / ComposedEngine / run_task: refused before any device call ----------------------------------------------------------------
class _NoOps:
    def __getattr__(self, name):
        raise AssertionError("ops.%s was reached before random erasing was refused" % name)


def test_graph_engine_and_composed_engine_refuse_erasing(monkeypatch):
    from tests import graph_cases as GC
    from vltf_amd import composed, graph
    case = GC.encdec()
    pipes, ds = GC.specs_and_datasets(case, None)
    monkeypatch.setattr(graph, "ops", _NoOps())
    monkeypatch.setattr(graph.torch, "zeros", lambda *a, **k: pytest.fail("a buffer was allocated"))
    with pytest.raises(VltfError, match="erase_prob = 0.25 is refused by GraphEngine.*per-tower tables are a follow-up"):
        graph.GraphEngine(pipes, ds, case["V"], device="cuda:0", erase_prob=0.25)
    with pytest.raises(VltfError, match="erase_prob"):
        graph.GraphEngine(pipes, ds, case["V"], device="cuda:0", erase_prob=-1.0)
    enc = NetConfig(image_shape=(67, 67, 3), num_classes=7, fpc=3, lstm_hidden=8, erase_prob=0.5)
    with pytest.raises(VltfError, match="erase_prob = 0.5 is refused by GraphEngine.*per-tower tables are a follow-up"):
        composed.ComposedEngine(enc, composed.HeadConfig(in_dim=5, fpc=4, num_classes=9, lstm_hidden=8), max_clips=2)


def test_run_task_refuses_erasing_on_a_multi_pipeline_model(tmp_path, monkeypatch):
    from tests import test_run_task_graph_gpu as TS
    from vltf_amd import graph, run_task
    folder = str(tmp_path)
    rpath, _, _ = TS.make_dataset(folder, "rgb.txt", nvid=5, cpv=TS.CPV, shape=TS.RAW, classes=TS.V, seed=7)
    fpath, _, _ = TS.make_dataset(folder, "flow.txt", nvid=5, cpv=TS.CPV, shape=TS.RAW, classes=TS.V, seed=8)
    path = TS.write_two_stream_cfg(folder, "ts.yml", rpath, fpath, "train")
    with open(path) as f:
        cfg = yaml.safe_load(f)
    cfg["run"]["train"].update(erase_prob=0.25, erase_seed=7)
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    monkeypatch.setattr(graph, "GraphEngine", lambda *a, **k: pytest.fail("an engine was built"))
    monkeypatch.setattr(run_task, "LRCNEngine", lambda *a, **k: pytest.fail("an engine was built"))
    monkeypatch.setattr(run_task, "graph_config", lambda *a, **k: pytest.fail("the graph was configured"))
    with pytest.raises(Exception, match="train.erase_prob is refused for this model.*single-pipeline"):
        run_task.main(path, seed=3)
