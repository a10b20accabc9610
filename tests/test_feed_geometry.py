"""The references of tests/feed_ref.py on the case lists of tests/test_feed_geometry_gpu.py, on the CPU: that the two references agree
with each other (packed_feed = crop_feed pushed through the space-to-depth map of tests/test_cutmix_gpu.py), that the case lists tell
every deliberately wrong variant from the reference (a case list that cannot is too weak to judge a kernel), that the three-channel
stride-4 sweep reaches both sides of that kernel's `interior` test at both edges and more than one alignment, and what the dropout draw
is made of."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import feed_ref as F
from tests.fc_dropout_ref import keep_mask
from tests.test_cutmix_gpu import s2d_index, x0_index

SENTINEL = 12345.0


def all_crop_cases():
    return [c for halo, phase in F.CROP_LAYOUTS for c in F.crop_cases(halo, phase)]


def test_crop_sizes_fill_the_last_column_group_and_leave_it_ragged():
    split = [((ow + 2 * halo) % phase == 0) for halo, phase in F.CROP_LAYOUTS if phase > 1 for _, ow in F.CROP_SIZES]
    assert any(split) and not all(split)
    assert (1, 1) in F.CROP_SIZES and any(h == 0 for h, _ in F.CROP_LAYOUTS)


def test_crop_feed_places_pixels_where_x0_index_says():
    """crop_feed's placement (written there by planes, rows and columns) against the flat-index map the CutMix tests use."""
    for case in all_crop_cases():
        val, written = F.crop_want(case)
        n, oh, ow, halo, phase = case["src"].shape[0], case["oh"], case["ow"], case["halo"], case["phase"]
        idx = x0_index(n, 1, oh, ow, halo, phase)
        assert len(np.unique(idx)) == idx.size, case["name"]
        frames = F.feed_frames(case["src"], case["cy"], case["cx"], case["mir"], case["mean"], oh, ow)
        assert np.array_equal(val.reshape(-1)[idx].view(np.uint32), frames.view(np.uint32)), case["name"]
        rest = np.ones(val.size, bool)
        rest[idx.reshape(-1)] = False
        assert not val.reshape(-1)[rest].view(np.uint32).any(), case["name"]              # every other element: +0.0 ...
        rows = np.zeros(val.shape, bool)
        rows[:, :, halo:halo + oh] = True
        assert np.array_equal(written, rows), case["name"]                               # ... written in the interior rows alone
        want = F.expected_bits(val, written, SENTINEL)
        assert (want == np.float32(SENTINEL).view(np.uint32)).sum() == n * 3 * phase * 2 * halo * val.shape[3], case["name"]


def test_packed_feed_is_crop_feed_through_the_s2d_map():
    for case in F.packed_cases() + [F.packed_case(F.C3S4_FULL)]:
        cin, h, w, k, s = case["desc"]
        oh, ow, pt, pl = F.same_geometry(h, w, k, s)
        n = case["src"].shape[0]
        got = F.packed_want(case)
        assert got.shape == (n,) + F.packed_dims(cin, k, s, oh, ow) + (8,) and got.dtype == np.int16, case["name"]
        if cin == 3:                                                                      # the crop reference knows three channels
            val, _ = F.crop_feed(case["src"], case["cy"], case["cx"], case["mir"], case["mean"], h, w, 0, 1)
            frames = val.reshape(n, 3, h, w).transpose(0, 2, 3, 1)
        else:
            frames = F.feed_frames(case["src"], case["cy"], case["cx"], case["mir"], case["mean"], h, w)
        idx = s2d_index(n, 1, cin, h, w, k, s, SimpleNamespace(oh=oh, ow=ow))
        assert len(np.unique(idx)) == idx.size and idx.max() < got.size, case["name"]
        want = np.zeros(got.size, np.int16)                                               # +0 in every slot no pixel maps to
        want[idx] = F.bf16_bits(frames)
        assert np.array_equal(got.reshape(-1), want), case["name"]


def test_bf16_rounding_of_the_reference():
    v = np.array([128.5, 129.5, -128.5, -129.5, 1.0, 0.0, -0.0, 1.00390625, 1.01171875], np.float32)
    #             tie -> even (128), tie -> even (130), the same negated, exact, zeros, tie at 1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6
    want = np.array([0x4300, 0x4302, 0xc300, 0xc302, 0x3f80, 0x0000, 0x8000, 0x3f80, 0x3f82], np.uint16)
    assert np.array_equal(F.bf16_bits(v).view(np.uint16), want)
    assert F.is_bf16_tie(v).tolist() == [True, True, True, True, False, False, False, True, True]
    for case in (F.packed_case(F.GENERIC[1], tie=True), F.packed_case(F.S2D_ALONE[0], tie=True)):
        cin, h, w, k, s = case["desc"]
        assert F.is_bf16_tie(F.feed_frames(case["src"], case["cy"], case["cx"], case["mir"], case["mean"], h, w)).any(), case["name"]
    for desc in F.S2D_ALONE:
        assert F.is_bf16_tie(F.s2d_alone_frames(desc)).mean() > 0.1


@pytest.mark.parametrize("wrong", F.WRONG_CROP)
def test_crop_cases_tell_a_wrong_feed_apart(wrong):
    told = [c["name"] for c in all_crop_cases()
            if not np.array_equal(F.expected_bits(*F.crop_want(c), SENTINEL), F.expected_bits(*F.crop_want(c, wrong), SENTINEL))]
    print("%s: told apart by %d cases, the first: %s" % (wrong, len(told), told[:1]))
    assert told, "no case of the list tells '%s' from the reference: the list is too weak" % wrong


@pytest.mark.parametrize("wrong", F.WRONG_PACKED)
def test_packed_cases_tell_a_wrong_feed_apart(wrong):
    told = [c["name"] for c in F.packed_cases() if not np.array_equal(F.packed_want(c), F.packed_want(c, wrong))]
    print("%s: told apart by %d cases, the first: %s" % (wrong, len(told), told[:1]))
    assert told, "no case of the list tells '%s' from the reference: the list is too weak" % wrong
    if wrong in ("py and px swapped", "pt and pl swapped", "truncation"):                 # both kernels must meet a case that tells
        assert any(n.startswith("(3, 1") or n.startswith("(3, 2") for n in told) and any(n.startswith(("(2,", "(3, 9", "(4,")) for n in told), told


def test_s2d_alone_cases_tell_wrong_maps_apart():
    for desc in F.S2D_ALONE:
        cin, h, w, k, s = desc
        oh, ow, pt, pl = F.same_geometry(h, w, k, s)
        img = F.s2d_alone_frames(desc)
        want = F.pack_s2d(img, cin, h, w, k, s, pt, pl, oh, ow)
        for wrong in ("py and px swapped", "truncation"):
            assert not np.array_equal(want, F.pack_s2d(img, cin, h, w, k, s, pt, pl, oh, ow, wrong)), (desc, wrong)
    desc = F.S2D_ALONE[1]                                                                  # pt = 2, pl = 1
    cin, h, w, k, s = desc
    oh, ow, pt, pl = F.same_geometry(h, w, k, s)
    assert pt != pl
    img = F.s2d_alone_frames(desc)
    assert not np.array_equal(F.pack_s2d(img, cin, h, w, k, s, pt, pl, oh, ow), F.pack_s2d(img, cin, h, w, k, s, pt, pl, oh, ow, "pt and pl swapped"))


def test_the_stride_4_sweep_reaches_both_paths_at_both_edges():
    """A condition on the INPUTS of the three-channel stride-4 kernel: (4 S - pl) mod 4 in more than one residue over the sweep, and
    column quads inside, cut by and wholly outside the frame at the left and at the right."""
    residues, classes = set(), set()
    for cin, h, w, k, s in F.C3S4_SWEEP:
        oh, ow, pt, pl = F.same_geometry(h, w, k, s)
        residues.add(-pl % 4)
        classes |= F.c3s4_classes(w, pl, F.packed_dims(cin, k, s, oh, ow)[2])
    assert len(residues) > 1, residues
    assert classes == {"interior", "left, cut", "left, outside", "right, cut", "right, outside"}, classes
    assert {F.same_geometry(h, w, 11, 4)[2:] for _, h, w, _, _ in F.C3S4_SWEEP} >= {(5, 3), (3, 5), (4, 4)}    # pt != pl both ways


def test_generic_descriptors_and_the_refused_one():
    for cin, h, w, k, s in F.GENERIC + F.C3S4_SWEEP + [F.C3S4_FULL]:
        assert -(-k // s) % 2 == 1
    cin, h, w, k, s = F.REFUSED
    assert -(-k // s) % 2 == 0
    assert (F.GENERIC[1][0] * F.GENERIC[1][4] ** 2) % 8 == 4 and (F.GENERIC[2][0] * F.GENERIC[2][4] ** 2) % 8 == 4   # half-used last chunks


def test_dropout_mask_restatement():
    """The draw of (seed, element) alone: another seed, another mask; element e does not depend on the count; keep = 1 keeps all; the
    rate is the keep probability; it is NOT vl_fc_dropout_fwd's salted draw; the _st seed wraps past 64 bits."""
    m = F.dropout_mask(1234, 100000, 0.5)
    assert abs(m.mean() - 0.5) < 0.01 and abs(F.dropout_mask(1234, 100000, 0.9).mean() - 0.9) < 0.01
    assert F.dropout_mask(1234, 4096, 1.0).all()
    assert np.array_equal(m[:257], F.dropout_mask(1234, 257, 0.5))
    assert not np.array_equal(m, F.dropout_mask(1235, 100000, 0.5)) and not np.array_equal(m[1:], m[:-1])
    assert not np.array_equal(m, keep_mask(1234, 0, 100000, 0.5))
    assert np.array_equal(F.dropout_mask(2 ** 64 + 7, 1000, 0.5), F.dropout_mask(7, 1000, 0.5))
    assert F.st_seed(0) == 0x5DEECE66D and F.st_seed(1) == (1 << 20) ^ 0x5DEECE66D
    assert F.st_seed(2 ** 44 + 3) == (3 << 20) ^ 0x5DEECE66D and F.st_seed(2 ** 31) == (1 << 51) ^ 0x5DEECE66D
    assert len({F.st_seed(s) for s in (0, 1, 2 ** 31, 2 ** 43 + 3)}) == 4
