"""What the cases of tests/result3d_cases.py claim to exercise, pinned on the CPU against the oracle alone, before
tests/test_gpu_result3d.py runs them through result3d_nms_kernel.  The first claim is a condition, not a measurement, and it is the one
that lets the GPU test demand equality: no pair of a class judged against the oracle has an fp64 IoU within KNIFE of a threshold the
case runs at.  The host-side split of the packed result buffer (consumers.split_packed_result) is checked here too: it needs no GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nms_bev_cases as nc  # noqa: E402
import result3d_cases as rc  # noqa: E402
from test_rotated_overlap_cases_cpu import KNIFE, NMS_THRS  # noqa: E402


def test_thresholds_and_caps_are_the_modules():
    from monorun_amd import consumers
    assert set(rc.THRS) == set(NMS_THRS) | {0.01}
    assert (rc.MAX_N, rc.MAX_C) == (consumers.RESULT3D_MAX_N, consumers.RESULT3D_MAX_CLASSES) == (512, 16)


@pytest.mark.parametrize('name', rc.NAMES)
def test_no_pair_of_an_oracle_judged_class_is_near_a_threshold(name):
    c = rc.case(name)
    N = len(c['labels'])
    assert N <= rc.MAX_N and c['C'] <= rc.MAX_C and c['thrs'] == rc.THRS
    for key, shape in (('dimensions', (N, 3)), ('yaw', (N, 1)), ('t_vec', (N, 3)), ('scores', (N,)), ('det_bboxes', (N, 5))):
        assert c[key].dtype == np.float32 and c[key].shape == shape and c[key].flags['C_CONTIGUOUS'], key
    assert c['labels'].dtype == np.int64
    margins = rc.knife_margins(name)
    judged = [i for i, (r, _) in enumerate(rc.class_rows(name)) if i not in c['hand'] and len(r) > 1]
    assert sorted(margins) == judged
    for i, m in margins.items():
        assert m >= KNIFE, (name, i, m)
    print(f'{name}: {len(judged)} oracle-judged classes, closest pair to a threshold {min(margins.values(), default=np.inf):.3e}')


@pytest.mark.parametrize('name', rc.NAMES)
def test_kept_counts_are_pinned(name):
    c = rc.case(name)
    for thr in c['thrs']:
        want = rc.expected(name, thr)
        assert [len(k) for k in want] == rc.KEPT[name][thr], (name, thr)
        for (r, _), k in zip(rc.class_rows(name), want):
            assert k.dtype == np.int64 and len(set(k.tolist())) == len(k) and (len(k) == 0 or (0 <= k.min() and k.max() < len(r)))
            assert len(r) < 8 or c['hand'] or 1 < len(k) < len(r)                  # from 8 members on, boxes both go and stay


def test_sized_cases_hold_the_sizes_they_name():
    want = {0, 1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 512}
    seen, classes = set(), set()
    for name, (C, sizes, outsiders) in rc.SIZED.items():
        c = rc.case(name)
        assert c['C'] == C == len(sizes) and c['sizes'] == sizes
        assert [int((c['labels'] == i).sum()) for i in range(C)] == list(sizes)
        assert int((c['labels'] == -1).sum()) == (outsiders + 1) // 2 and int((c['labels'] == C).sum()) == outsiders // 2
        assert len(c['labels']) == sum(sizes) + outsiders
        seen |= set(sizes)
        classes.add(C)
    assert want <= seen and classes == {1, 3, 16}
    assert rc.case('c1_all_512')['sizes'] == (512,) and len(rc.case('c1_all_512')['labels']) == 512
    assert sum(o > 0 for _, _, o in rc.SIZED.values()) >= 3                        # rows labelled -1 and C


def test_labels_are_interleaved_and_keep_each_class_in_order():
    """a compaction that is not stable, or that takes rows rather than earlier members as the local index, gives other indices"""
    for name in ('c16_small', 'c3_256_1_240', 'special_scores'):
        c = rc.case(name)
        lab = c['labels']
        assert (np.diff(lab) != 0).sum() > len(lab) // 3                            # neighbours mostly differ in class
        for i, (r, rows) in enumerate(rc.class_rows(name)):
            assert np.all(np.diff(rows) > 0) and np.array_equal(r[:, 7], c['scores'][rows], equal_nan=True)
            if len(rows) > 2:
                assert rows[-1] - rows[0] > len(rows)                               # spread: local index != row - first row


def test_scores_have_ties_zeros_nans_and_infinities():
    c = rc.case('c16_small')
    for i, (r, _) in enumerate(rc.class_rows('c16_small')):
        if len(r) >= 8:
            s = r[:, 7]
            assert (s == 0).sum() >= 2 and len(np.unique(s)) < len(s)               # failed solves tie at 0
    s = rc.case('special_scores')
    per = [r[:, 7] for r, _ in rc.class_rows('special_scores')]
    assert [len(p) for p in per] == [3, 5, 33, 100, 64, 37, 20, 0]
    assert all(np.isnan(p).any() for p in per[:6]) and np.isnan(per[5]).all() and np.isinf(per[6]).all() and np.isposinf(per[3]).sum() == 2
    for thr in s['thrs']:
        k = rc.expected('special_scores', thr)
        assert k[0].tolist() == [0, 2] and k[1].tolist() == [0, 2, 3] and k[7].shape == (0,)
    assert c['thrs'] == rc.THRS


def test_special_boxes_survive_the_rows(orc):
    """the degenerate boxes stay degenerate when a row carries them as [x, z, l, w]: NaN coordinates, zero areas, negative sizes"""
    (r0, _), (r1, _), (r2, _) = rc.class_rows('special_boxes')
    b0, b1, b2 = rc.rebuilt(r0), rc.rebuilt(r1), rc.rebuilt(r2)
    assert np.isnan(b0[1]).any() and np.isnan(b0[3]).any() and np.isfinite(b0[[0, 2, 4]]).all() and np.array_equal(b0[0], b0[4])
    assert (np.abs((b1[:, 2] - b1[:, 0]) * (b1[:, 3] - b1[:, 1])) == 0).sum() == 6
    assert np.all(b2[0:6, 2] < b2[0:6, 0]) and np.all(b2[6:12, 3] < b2[6:12, 1]) and np.all(r2[12:18, 0] < 0) and np.all(r2[12:18, 2] < 0)
    c = rc.case('special_boxes')
    assert c['hand'] == {0: [0, 1, 2, 3], 1: [0, 1, 2, 3, 4, 5, 6, 7]}
    for thr in c['thrs']:
        fin = [0, 2, 4]                                 # class 0 without its NaN boxes, class 1 whole: the oracle agrees with the hand
        assert [fin[i] for i in orc.nms_bev(b0[fin], r0[fin, 7], thr)] == [0, 2]
        assert np.array_equal(orc.nms_bev(b1, r1[:, 7], thr), rc.expected('special_boxes', thr)[1])
        k = rc.expected('special_boxes', thr)[2]
        assert np.array_equal(k, orc.nms_bev(nc.sorted_coords(b2), r2[:, 7], thr)) and 1 < len(k) < len(r2)


def test_rebuilt_boxes_are_within_an_ulp_of_the_builders():
    b, s = rc._class_group('c1_257', 0, 257, rc.TRIES['c1_257'].get(0, 0))
    r, _ = rc.class_rows('c1_257')[0]
    assert np.array_equal(r[:, 7], s)
    assert np.abs(rc.rebuilt(r)[:, :4] - b[:, :4]).max() <= 2 * np.spacing(np.float32(80.0))


# ------------------------------------------------------------------------------- the packed buffer's host side
def _hand_buffer(C, n, kept):
    """a packed buffer written by hand: class c keeps kept[c] = [(local, row), ...]; its 3-D row k is 100 c + k + [0 .. 7] / 10"""
    from monorun_amd.consumers import result_3d_layout
    layout, size = result_3d_layout(C, n)
    buf = np.zeros(size, np.uint8)
    f = {name: buf[off:off + int(np.prod(shape)) * dt.itemsize].view(dt).reshape(shape) for name, (off, dt, shape) in layout.items()}
    f['out3d'][:], f['out2d'][:], f['keep_local'][:], f['keep_row'][:] = np.nan, np.nan, -1, -1
    for c, ks in enumerate(kept):
        f['num_keep'][c], f['num_in_class'][c] = len(ks), len(ks) + 1
        for k, (local, row) in enumerate(ks):
            f['out3d'][c, k] = 100 * c + k + np.arange(8) / 10
            f['out2d'][c, k] = -(100 * c + k + np.arange(5) / 10)
            f['keep_local'][c, k], f['keep_row'][c, k] = local, row
    return buf, layout, size


def test_layout_of_the_packed_buffer():
    from monorun_amd.consumers import result_3d_layout
    layout, size = result_3d_layout(3, 5)
    assert layout['keep_local'][0] == 0 and layout['keep_row'][0] == 120 and layout['out3d'][0] == 240 and layout['out3d'][0] % 16 == 0
    assert layout['out2d'][0] == 240 + 480 and layout['num_keep'][0] == 720 + 300 and layout['num_in_class'][0] == 1032 and size == 1044
    for C, n in ((1, 1), (16, 512), (3, 7), (0, 0), (2, 0)):
        layout, size = result_3d_layout(C, n)
        assert size == C * n * (8 + 8 + 32 + 20) + 8 * C
        assert layout['out3d'][0] % 16 == 0 and layout['keep_row'][0] % 8 == 0 and all(off % 4 == 0 for off, _, _ in layout.values())


def test_split_of_a_hand_written_buffer():
    from monorun_amd.consumers import split_packed_result
    kept = [[(2, 7), (0, 1)], [], [(0, 3)], [(1, 4), (3, 6), (0, 0)]]
    buf, _, _ = _hand_buffer(4, 8, kept)
    b3, inds, b2, rows = split_packed_result(buf, 4, 8)
    assert len(b3) == len(inds) == len(b2) == len(rows) == 4
    for c, ks in enumerate(kept):
        assert b3[c].shape == (len(ks), 8) and b3[c].dtype == np.float32 and b2[c].shape == (len(ks), 5) and b2[c].dtype == np.float32
        assert inds[c].dtype == np.int64 and rows[c].dtype == np.int64
        assert inds[c].tolist() == [l for l, _ in ks] and rows[c].tolist() == [r for _, r in ks]
        for k in range(len(ks)):
            assert np.array_equal(b3[c][k], (100 * c + k + np.arange(8) / 10).astype(np.float32))
            assert np.array_equal(b2[c][k], (-(100 * c + k + np.arange(5) / 10)).astype(np.float32))
    assert b3[1].shape == (0, 8) and b2[1].shape == (0, 5) and inds[1].shape == (0,)              # a class with no members
    before = buf.copy()
    b3[0][:] = 0                                                                                 # copies: the buffer is not aliased
    assert np.array_equal(buf, before)
    b3, inds, b2, rows = split_packed_result(_hand_buffer(3, 0, [[], [], []])[0], 3, 0)          # no detections at all
    assert [a.shape for a in b3] == [(0, 8)] * 3 and [a.shape for a in b2] == [(0, 5)] * 3 and all(i.dtype == np.int64 for i in inds)
    with pytest.raises(AssertionError):
        split_packed_result(buf[:-1], 4, 8)
