"""CutMix / VideoMix on the host: check_cutmix, the draws of cutmix_box and their properties, the label weight of hand-computed boxes,
the caller's box check, the YAML keys with their refusals and the getter outside the train phase, the host reference
(tests/cutmix_ref.py), the C-ABI rows and the entry points' argument checks, the example, and the refusals of GraphEngine and
run_task ahead of any device call.  No GPU: nothing is launched."""
import os

import numpy as np
import pytest
import yaml

from tests import cutmix_ref as CM
from tests.test_ema import _val_settings
from tests.test_finetune import _settings
from vltf_amd._ffi import VltfError
from vltf_amd.engine import (CUTMIX_MODES, NetConfig, check_cut_box, check_cutmix, cutmix_box, cutmix_lambda, fold_lambda,
                             mixup_lambda)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR = "train.cutmix_alpha / train.cutmix_seed / train.cutmix_mode / train.cutmix_prob"


# ---- check_cutmix -------------------------------------------------------------------------------------------------------------------
def test_check_cutmix_accepts():
    off = (0.0, 0, "spatial", 0.5)
    assert check_cutmix(None) == off and check_cutmix(None, None, None, None) == off and check_cutmix(0, 0) == off
    assert check_cutmix(1.0) == (1.0, 0, "spatial", 0.5)
    assert check_cutmix(0.5, 7, "cuboid", 0.25) == (0.5, 7, "cuboid", 0.25)
    assert check_cutmix(np.float32(0.5), np.int64(3), "temporal", 1) == (0.5, 3, "temporal", 1.0)
    assert check_cutmix(2, 5.0, None, 0) == (2.0, 5, "spatial", 0.0) and check_cutmix(1.0, 2 ** 64 - 1)[1] == 2 ** 64 - 1
    a, s, m, p = check_cutmix(1, 2.0, "spatial", 1)
    assert isinstance(a, float) and isinstance(s, int) and isinstance(m, str) and isinstance(p, float)
    cfg = NetConfig()
    assert (cfg.cutmix_alpha, cfg.cutmix_seed, cfg.cutmix_mode, cfg.cutmix_prob) == (0.0, 0, None, None)
    assert CUTMIX_MODES == ("spatial", "temporal", "cuboid")


@pytest.mark.parametrize("bad", [-0.1, float("nan"), float("inf"), True, False, "1.0", b"1.0", [1.0], np.bool_(True)])
def test_check_cutmix_refuses_alpha(bad):
    with pytest.raises(VltfError, match="cutmix_alpha") as ex:
        check_cutmix(bad)
    assert repr(bad) in str(ex.value)


@pytest.mark.parametrize("bad", [-1, 2.5, float("nan"), float("inf"), True, "7", b"7", [7], 2 ** 64])
def test_check_cutmix_refuses_seed(bad):
    with pytest.raises(VltfError, match="cutmix_seed") as ex:
        check_cutmix(1.0, bad)
    assert repr(bad) in str(ex.value)


@pytest.mark.parametrize("bad", ["box", "Spatial", "", 1, True, b"spatial", ["spatial"]])
def test_check_cutmix_refuses_mode(bad):
    with pytest.raises(VltfError, match="cutmix_mode must be one of spatial \\| temporal \\| cuboid"):
        check_cutmix(1.0, 0, bad)


@pytest.mark.parametrize("bad", [-0.1, 1.1, float("nan"), float("inf"), True, "0.5", b"0.5", [0.5]])
def test_check_cutmix_refuses_prob(bad):
    with pytest.raises(VltfError, match="cutmix_prob"):
        check_cutmix(1.0, 0, None, bad)


@pytest.mark.parametrize("alpha", [None, 0, 0.0])
def test_check_cutmix_refuses_options_without_alpha(alpha):
    with pytest.raises(VltfError, match="cutmix_seed is given without cutmix_alpha"):
        check_cutmix(alpha, 7)
    with pytest.raises(VltfError, match="cutmix_mode is given without cutmix_alpha"):
        check_cutmix(alpha, None, "cuboid")
    with pytest.raises(VltfError, match="cutmix_prob is given without cutmix_alpha"):
        check_cutmix(alpha, None, None, 0.5)


# ---- the draws --------------------------------------------------------------------------------------------------------------------------
def test_cutmix_box_is_a_pure_function_of_its_arguments():
    draws = [cutmix_box(1.0, 7, "cuboid", i, 16, 227, 227) for i in range(64)]
    assert draws == [cutmix_box(1.0, 7, "cuboid", i, 16, 227, 227) for i in range(64)]
    assert len(set(draws)) == 64
    other = [cutmix_box(1.0, 8, "cuboid", i, 16, 227, 227) for i in range(64)]
    assert all(a != b for a, b in zip(draws, other))
    assert cutmix_box(1.0, 7, "cuboid", 5, 16, 227, 227) != cutmix_box(0.4, 7, "cuboid", 5, 16, 227, 227)
    assert cutmix_box(1.0, 7, None, 5, 16, 227, 227) == cutmix_box(1.0, 7, "spatial", 5, 16, 227, 227)
    assert cutmix_box(1.0, 7, "spatial", 2 ** 40, 16, 227, 227) == cutmix_box(1.0, 7, "spatial", 2 ** 40, 16, 227, 227)
    assert cutmix_box(0.0, 0, None, 3, 16, 227, 227) == ((0, 0, 0, 0, 0, 0), 1.0)        # off: nothing is cut
    assert cutmix_box(None, None, None, 3, 16, 227, 227) == ((0, 0, 0, 0, 0, 0), 1.0)
    with pytest.raises(VltfError, match="cutmix_alpha"):
        cutmix_box(-1.0, 0, None, 0, 16, 227, 227)
    for b in draws:
        assert all(isinstance(v, int) for v in b[0]) and isinstance(b[1], float)


@pytest.mark.parametrize("mode", CUTMIX_MODES)
@pytest.mark.parametrize("geom", [(16, 227, 227), (3, 9, 11)], ids=["16x227x227", "3x9x11"])
def test_cutmix_box_properties(mode, geom):
    """10 000 draw indices: every box lies inside its bounds, is at most half the clip, lam lies in [0.5, 1] and is 1 exactly when the
    box is empty; the axes a mode does not cut are whole."""
    fpc, h, w = geom
    empty = 0
    for i in range(10000):
        (t0, t1, y0, y1, x0, x1), u = cutmix_box(1.0, 11, mode, i, fpc, h, w)
        assert 0 <= t0 <= t1 <= fpc and 0 <= y0 <= y1 <= h and 0 <= x0 <= x1 <= w
        assert 0.0 <= u < 1.0
        vol = (t1 - t0) * (y1 - y0) * (x1 - x0)
        assert 2 * vol <= fpc * h * w
        lam = cutmix_lambda((t0, t1, y0, y1, x0, x1), fpc, h, w)
        assert 0.5 <= lam <= 1.0
        assert (lam == 1.0) == (vol == 0)
        assert lam == CM.lam((t0, t1, y0, y1, x0, x1), fpc, h, w)
        empty += vol == 0
        if mode == "spatial":
            assert (t0, t1) == (0, fpc)
        if mode == "temporal":
            assert (y0, y1, x0, x1) == (0, h, 0, w)
        check_cut_box((t0, t1, y0, y1, x0, x1), fpc, h, w)                               # what the draw gives, the override takes
    assert empty < 10000                                                                 # (something is cut)


def test_cutmix_box_follows_the_stated_stream():
    """The generator's order: Beta, the three centres over fpc, h, w, then u -- whatever the mode, so u and the centres are shared by
    the modes, and u is what mixup's presence cannot move (it is drawn from cutmix's own key)."""
    fpc, h, w = 16, 32, 40
    for i in range(50):
        rng = np.random.Generator(np.random.Philox(key=np.array([5, i], np.uint64)))
        lam0 = fold_lambda(float(rng.beta(0.7, 0.7)))
        ct, cy, cx = (int(rng.integers(n)) for n in (fpc, h, w))
        u = float(rng.random())
        r = np.sqrt(1.0 - lam0)
        bh, bw = int(h * r), int(w * r)
        want = (0, fpc, min(max(cy - bh // 2, 0), h), min(max(cy - bh // 2 + bh, 0), h), min(max(cx - bw // 2, 0), w),
                min(max(cx - bw // 2 + bw, 0), w))
        assert cutmix_box(0.7, 5, "spatial", i, fpc, h, w) == (want, u)
        bt = int(fpc * (1.0 - lam0))
        want_t = (min(max(ct - bt // 2, 0), fpc), min(max(ct - bt // 2 + bt, 0), fpc), 0, h, 0, w)
        assert cutmix_box(0.7, 5, "temporal", i, fpc, h, w) == (want_t, u)
        r3 = float(np.cbrt(1.0 - lam0))
        e = (int(fpc * r3), int(h * r3), int(w * r3))
        want_c = []
        for c, b, n in zip((ct, cy, cx), e, (fpc, h, w)):
            want_c += [min(max(c - b // 2, 0), n), min(max(c - b // 2 + b, 0), n)]
        assert cutmix_box(0.7, 5, "cuboid", i, fpc, h, w) == (tuple(want_c), u)
    # u is the LAST draw: a generator that stops before it gives another number
    rng = np.random.Generator(np.random.Philox(key=np.array([5, 0], np.uint64)))
    rng.beta(0.7, 0.7)
    assert float(rng.random()) != cutmix_box(0.7, 5, "spatial", 0, fpc, h, w)[1]
    # mixup's draw is a stream of its own: the box of a run does not move when mixup is on, nor mixup's weight when cutmix is
    assert mixup_lambda(0.2, 5, 3) == mixup_lambda(0.2, 5, 3)
    assert cutmix_box(0.7, 5, "spatial", 3, fpc, h, w) == cutmix_box(0.7, 5, "spatial", 3, fpc, h, w)


def test_lambda_of_hand_computed_boxes():
    assert cutmix_lambda((0, 0, 0, 0, 0, 0), 3, 9, 11) == 1.0
    assert cutmix_lambda((0, 3, 4, 4, 0, 11), 3, 9, 11) == 1.0                           # an empty axis empties the box
    assert cutmix_lambda((0, 3, 1, 6, 3, 10), 3, 9, 11) == float(np.float32(1.0 - 105 / 297))
    assert cutmix_lambda((1, 2, 0, 9, 0, 11), 3, 9, 11) == float(np.float32(2.0 / 3.0))
    assert cutmix_lambda((0, 8, 0, 227, 0, 227), 16, 227, 227) == 0.5
    assert cutmix_lambda((0, 1, 0, 1, 0, 1), 16, 227, 227) == float(np.float32(1.0 - 1.0 / (16 * 227 * 227)))
    assert cutmix_lambda((0, 1, 0, 1, 0, 1), 16, 227, 227) < 1.0                          # one pixel is not nothing in float32
    for box in ((0, 3, 1, 6, 3, 10), (1, 2, 0, 9, 0, 11)):
        assert CM.lam(box, 3, 9, 11) == cutmix_lambda(box, 3, 9, 11)


def test_check_cut_box():
    assert check_cut_box((0, 3, 1, 6, 3, 10), 3, 9, 11) == (0, 3, 1, 6, 3, 10)
    assert check_cut_box([np.int64(1), 2, 0.0, 9, 0, 11], 3, 9, 11) == (1, 2, 0, 9, 0, 11)
    assert check_cut_box((0, 0, 0, 0, 0, 0), 3, 9, 11) == (0, 0, 0, 0, 0, 0)
    for bad in ((0, 3, 1, 6, 3), None, 5, "012345", (0, 3, 1, 6, 3, 10.5), (0, 3, 1, 6, 3, True), (0, 3, 1, 6, 3, "10")):
        with pytest.raises(VltfError, match="cut_box must be six whole numbers"):
            check_cut_box(bad, 3, 9, 11)
    for bad in ((0, 4, 0, 1, 0, 1), (-1, 1, 0, 1, 0, 1), (0, 1, 0, 10, 0, 1), (0, 1, 0, 1, 0, 12), (0, 1, 0, 1, 12, 13)):
        with pytest.raises(VltfError, match="leaves the frame"):
            check_cut_box(bad, 3, 9, 11)
    for bad in ((2, 1, 0, 1, 0, 1), (0, 1, 5, 4, 0, 1), (0, 1, 0, 1, 11, 3)):
        with pytest.raises(VltfError, match="is reversed"):
            check_cut_box(bad, 3, 9, 11)
    with pytest.raises(VltfError, match="above half the clip"):
        check_cut_box((0, 3, 0, 9, 0, 6), 3, 9, 11)
    assert check_cut_box((0, 8, 0, 227, 0, 227), 16, 227, 227)                           # exactly half is allowed


# ---- the host reference -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clips", [1, 2, 3, 4, 5])
def test_reference_swap(clips):
    rng = np.random.default_rng(clips)
    x = rng.integers(0, 255, (clips, 3, 9, 11, 3)).astype(np.uint8)
    box = (0, 3, 1, 6, 3, 10)
    y = CM.swap(x, box)
    assert np.array_equal(CM.swap(y, box), x)                                            # an involution
    assert np.array_equal(y[:, :, 1:6, 3:10], x[::-1, :, 1:6, 3:10])                     # inside: the partner's
    mask = np.ones(x.shape, bool)
    mask[:, :, 1:6, 3:10] = False
    assert np.array_equal(y[mask], x[mask])                                              # outside: untouched
    if clips % 2:
        assert np.array_equal(y[clips // 2], x[clips // 2])
    assert np.array_equal(CM.swap(x, (0, 0, 0, 0, 0, 0)), x) and np.array_equal(CM.swap(x, (2, 1, 0, 9, 0, 11)), x)
    assert np.array_equal(CM.swap(x, (0, 3, 0, 9, 0, 11)), x[::-1])
    assert np.array_equal(CM.swap(x, (-5, 99, -1, 6, 3, 400)), CM.swap(x, (0, 3, 0, 6, 3, 11)))   # clamped, as the device does
    assert CM.clamp((-5, 99, -1, 6, 3, 400), 3, 9, 11) == (0, 3, 0, 6, 3, 11) and CM.clamp((0, 3, 7, 2, 0, 11), 3, 9, 11) == (0,) * 6
    f = x.reshape((clips * 3, 9, 11, 3))
    assert np.array_equal(CM.swap_frames(f, clips, box), y.reshape(f.shape))


# ---- YAML -------------------------------------------------------------------------------------------------------------------------------
def test_settings_keys_parse(tmp_path):
    s = _settings(tmp_path, train={"cutmix_alpha": 1.0, "cutmix_seed": 7, "cutmix_mode": "cuboid", "cutmix_prob": 0.25})
    assert s.get_cutmix() == (1.0, 7, "cuboid", 0.25)
    assert isinstance(s.train.cutmix_alpha, float) and isinstance(s.train.cutmix_seed, int)
    s = _settings(tmp_path, train={"cutmix_alpha": "1e0", "cutmix_seed": "7", "cutmix_prob": "2.5e-1"})     # quoted numbers
    assert s.get_cutmix() == (1.0, 7, "spatial", 0.25)
    assert _settings(tmp_path, train={"cutmix_alpha": 1}).get_cutmix() == (1.0, 0, "spatial", 0.5)
    assert NetConfig(cutmix_alpha=1.0, cutmix_mode="temporal").cutmix_mode == "temporal"


@pytest.mark.parametrize("train", [{}, {"cutmix_alpha": None, "cutmix_seed": None, "cutmix_mode": None, "cutmix_prob": None},
                                   {"cutmix_alpha": "None", "cutmix_seed": "None", "cutmix_mode": "None", "cutmix_prob": "None"},
                                   {"cutmix_alpha": 0, "cutmix_seed": 0}, {"cutmix_alpha": "None"}],
                         ids=["absent", "null", "None-strings", "zeros", "None-alpha"])
def test_settings_absent_keys_mean_off(tmp_path, train):
    s = _settings(tmp_path, train=train)
    assert s.get_cutmix() == (0.0, 0, None, None)
    assert s.get_mixup() == (0.0, 0)


@pytest.mark.parametrize("train", [{"cutmix_alpha": -1.0}, {"cutmix_alpha": "nan"}, {"cutmix_alpha": "much"}, {"cutmix_alpha": True},
                                   {"cutmix_seed": 7}, {"cutmix_mode": "cuboid"}, {"cutmix_prob": 0.5},
                                   {"cutmix_alpha": "None", "cutmix_seed": 7}, {"cutmix_alpha": 1.0, "cutmix_seed": -1},
                                   {"cutmix_alpha": 1.0, "cutmix_seed": 1.5}, {"cutmix_alpha": 1.0, "cutmix_seed": "seven"},
                                   {"cutmix_alpha": 1.0, "cutmix_mode": "box"}, {"cutmix_alpha": 1.0, "cutmix_mode": 3},
                                   {"cutmix_alpha": 1.0, "cutmix_prob": 1.5}, {"cutmix_alpha": 1.0, "cutmix_prob": "often"},
                                   {"cutmix_alpha": 1.0, "cutmix_prob": True}])
def test_settings_refusals(tmp_path, train):
    with pytest.raises(Exception, match=ERR):
        _settings(tmp_path, train=train)


def test_settings_outside_the_train_phase_is_off(tmp_path):
    s = _val_settings(tmp_path, train={"cutmix_alpha": 1.0, "cutmix_seed": 7, "cutmix_mode": "cuboid", "cutmix_prob": 0.25})
    assert s.get_cutmix() == (0.0, 0, None, None)


def test_example_yaml_is_the_mixup_one_with_the_cutmix_keys(tmp_path):
    here = os.path.join(ROOT, "examples")
    with open(os.path.join(here, "lrcn_cutmix.yml")) as f:
        cut = yaml.safe_load(f)
    with open(os.path.join(here, "lrcn_mixup.yml")) as f:
        base = yaml.safe_load(f)
    t = cut["run"]["train"]
    got = (t.pop("cutmix_alpha"), t.pop("cutmix_seed"), t.pop("cutmix_mode"), t.pop("cutmix_prob"))
    assert got == (1.0, 7, "cuboid", 0.5)
    for cfg in (cut, base):
        cfg["run"].pop("run_folder", None), cfg["run"].pop("run_id", None)
    assert cut == base                                                                   # mixup stays on: the example runs both
    s = _settings(tmp_path, train={"cutmix_alpha": 1.0, "cutmix_seed": 7, "cutmix_mode": "cuboid", "cutmix_prob": 0.5,
                                   "mixup_alpha": 0.2, "mixup_seed": 7})
    assert s.get_cutmix() == got and s.get_mixup() == (0.2, 7)


# ---- C-ABI ------------------------------------------------------------------------------------------------------------------------------
def test_ffi_rows_and_ops_names():
    from tests.test_mixup import _header_arg_count
    from vltf_amd import _ffi
    import vltf_amd.ops as ops
    p, i32 = _ffi.p, _ffi.i32
    assert _ffi.SIGNATURES["vl_cutmix_pairs"] == (i32, [p, i32, i32, i32, i32, i32, i32, p, p, p])
    assert _ffi.SIGNATURES["vl_cutmix_pairs_s2d"] == (i32, [p, p, i32, i32, p, p, p])
    for name in ("vl_cutmix_pairs", "vl_cutmix_pairs_s2d"):
        assert len(_ffi.SIGNATURES[name][1]) == _header_arg_count(name), name
    assert _ffi.SIGNATURES["vl_mixup_pairs"] == (i32, [p, i32, i32, _ffi.i64, _ffi.f32, p, p])                  # as it was
    assert callable(ops.cutmix_pairs) and callable(ops.Conv.cutmix_pairs_s2d)


def _box(*v):
    import ctypes
    return (ctypes.c_int32 * 6)(*v)


def test_host_refusals_of_the_fp32_launch_need_no_device():
    """vl_cutmix_pairs validates before it launches, each refusal with a message of its own.  Nothing runs."""
    from vltf_amd import _ffi
    lib = _ffi.lib()
    fake = 4096                                  # a non-null, aligned address: validation fails before anything dereferences it
    ok = dict(x=fake, clips=2, fpc=3, h=9, w=11, halo=2, phase=4, box=_box(0, 3, 1, 6, 3, 10), dev=None)
    for change, msg in ((dict(x=None), b"x0 is null"), (dict(box=None), b"both box pointers are null"),
                        (dict(clips=-1), b"clips must be >= 0"), (dict(fpc=0), b"fpc must lie in"), (dict(fpc=-3), b"fpc must lie in"),
                        (dict(h=0), b"bad frame size"), (dict(w=-11), b"bad frame size"), (dict(halo=-1), b"halo must be >= 0"),
                        (dict(phase=0), b"phase must be >= 1"),
                        (dict(box=_box(0, 4, 1, 6, 3, 10)), b"t range [0, 4) leaves [0, 3]"),
                        (dict(box=_box(-1, 3, 1, 6, 3, 10)), b"t range [-1, 3) leaves"),
                        (dict(box=_box(0, 3, 1, 10, 3, 10)), b"y range [1, 10) leaves [0, 9]"),
                        (dict(box=_box(0, 3, 1, 6, 3, 12)), b"x range [3, 12) leaves [0, 11]"),
                        (dict(box=_box(2, 1, 1, 6, 3, 10)), b"t range [2, 1) is reversed"),
                        (dict(box=_box(0, 3, 6, 1, 3, 10)), b"y range [6, 1) is reversed"),
                        (dict(box=_box(0, 3, 1, 6, 10, 3)), b"x range [10, 3) is reversed")):
        a = dict(ok, **change)
        assert lib.vl_cutmix_pairs(a["x"], a["clips"], a["fpc"], a["h"], a["w"], a["halo"], a["phase"], a["box"], a["dev"], None) != 0, change
        err = lib.vl_last_error()
        assert b"vl_cutmix_pairs" in err and msg in err, (change, err)
    # nothing to pair, nothing to cut: accepted, and nothing is launched (the address is never touched)
    for change in (dict(clips=0), dict(clips=1), dict(box=_box(0, 0, 0, 0, 0, 0)), dict(box=_box(0, 3, 4, 4, 0, 11))):
        a = dict(ok, **change)
        assert lib.vl_cutmix_pairs(a["x"], a["clips"], a["fpc"], a["h"], a["w"], a["halo"], a["phase"], a["box"], None, None) == 0, change


def test_host_refusals_of_the_packed_launch_need_no_device():
    from vltf_amd import _ffi
    lib = _ffi.lib()
    fake = 4096
    box = _box(0, 1, 0, 1, 0, 1)
    assert lib.vl_cutmix_pairs_s2d(None, None, 2, 3, box, None, None) != 0 and b"xb is null" in lib.vl_last_error()
    assert lib.vl_cutmix_pairs_s2d(None, fake, 2, 3, None, None, None) != 0 and b"both box pointers are null" in lib.vl_last_error()
    assert lib.vl_cutmix_pairs_s2d(None, fake, -1, 3, box, None, None) != 0 and b"clips must be >= 0" in lib.vl_last_error()
    assert lib.vl_cutmix_pairs_s2d(None, fake, 2, 0, box, None, None) != 0 and b"fpc must lie in" in lib.vl_last_error()
    assert lib.vl_cutmix_pairs_s2d(None, fake, 2, 3, box, None, None) != 0                # a null descriptor: s2d_check's refusal
    assert b"vl_cutmix_pairs_s2d: a strided, ungrouped, square layer" in lib.vl_last_error()


def test_ops_wrappers_refuse_a_malformed_box():
    import vltf_amd.ops as ops
    for bad in ((0, 1, 0, 1, 0), None, 7, (0, 1, 0, 1, 0, 1.5), "012345", (0, 1, 0, 1, 0, 2 ** 40)):
        with pytest.raises(VltfError, match="the box is six whole numbers"):
            ops._cut_box(bad, "cutmix_pairs")
    host, dev, keep = ops._cut_box((0, 3, 1, 6, 3, 10), "cutmix_pairs")
    assert dev is None and list(keep) == [0, 3, 1, 6, 3, 10]


# ---- GraphEngine / run_task: refused before any device call ---------------------------------------------------------------------------------
class _NoOps:
    def __getattr__(self, name):
        raise AssertionError("ops.%s was reached before CutMix was refused" % name)


def test_graph_engine_refuses_cutmix(monkeypatch):
    from tests import graph_cases as GC
    from vltf_amd import graph
    case = GC.encdec()
    pipes, ds = GC.specs_and_datasets(case, None)
    monkeypatch.setattr(graph, "ops", _NoOps())
    monkeypatch.setattr(graph.torch, "zeros", lambda *a, **k: pytest.fail("a buffer was allocated"))
    with pytest.raises(VltfError, match="cutmix_alpha = 1.0 is refused by GraphEngine.*single-pipeline"):
        graph.GraphEngine(pipes, ds, case["V"], device="cuda:0", cutmix_alpha=1.0)
    with pytest.raises(VltfError, match="cutmix_alpha"):
        graph.GraphEngine(pipes, ds, case["V"], device="cuda:0", cutmix_alpha=-1.0)


def test_run_task_refuses_cutmix_on_a_multi_pipeline_model(tmp_path, monkeypatch):
    from tests import test_run_task_graph_gpu as TS
    from vltf_amd import graph, run_task
    folder = str(tmp_path)
    rpath, _, _ = TS.make_dataset(folder, "rgb.txt", nvid=5, cpv=TS.CPV, shape=TS.RAW, classes=TS.V, seed=7)
    fpath, _, _ = TS.make_dataset(folder, "flow.txt", nvid=5, cpv=TS.CPV, shape=TS.RAW, classes=TS.V, seed=8)
    path = TS.write_two_stream_cfg(folder, "ts.yml", rpath, fpath, "train")
    with open(path) as f:
        cfg = yaml.safe_load(f)
    cfg["run"]["train"].update(cutmix_alpha=1.0, cutmix_seed=7)
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    monkeypatch.setattr(graph, "GraphEngine", lambda *a, **k: pytest.fail("an engine was built"))
    monkeypatch.setattr(run_task, "LRCNEngine", lambda *a, **k: pytest.fail("an engine was built"))
    monkeypatch.setattr(run_task, "graph_config", lambda *a, **k: pytest.fail("the graph was configured"))
    with pytest.raises(Exception, match="train.cutmix_alpha is refused for this model.*single-pipeline"):
        run_task.main(path, seed=3)
