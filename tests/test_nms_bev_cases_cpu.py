"""What the cases of tests/nms_bev_cases.py claim to exercise, pinned on the CPU against the oracle alone, before
tests/test_gpu_nms_bev.py runs them through nms_bev_kernel.  The first claim is the one that lets the GPU test demand equality: no pair
of a group judged against the oracle has an fp64 IoU within KNIFE of a threshold the group runs at."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nms_bev_cases as nc  # noqa: E402
from test_rotated_overlap_cases_cpu import KNIFE, NMS_THRS  # noqa: E402


def _inside_limits(c):
    for g, s in zip(c['groups'], c['scores']):
        assert g.dtype == np.float32 and s.dtype == np.float32 and g.shape == (len(s), 5)
        ctr = 0.5 * (g[:, 0:2] + g[:, 2:4])
        assert np.all(np.abs(ctr[np.isfinite(ctr)]) <= 80.0)


@pytest.mark.parametrize('name', nc.NAMES)
def test_no_pair_of_an_oracle_judged_group_is_near_a_threshold(name):
    c = nc.case(name)
    _inside_limits(c)
    assert c['thrs'] == NMS_THRS
    worst, pairs = np.inf, 0
    for i in nc.oracle_judged(name):
        ious = nc.pair_ious(c['groups'][i])
        m = nc.knife_margin(ious, c['thrs'])
        assert m >= KNIFE, (name, i, m)
        worst, pairs = min(worst, m), pairs + len(ious)
    print(f'{name}: {pairs} near pairs in {len(nc.oracle_judged(name))} oracle-judged groups, closest to a threshold {worst:.3e}')


def test_near_pairs_are_all_the_pairs_that_intersect(orc):
    """the shortcut of the knife-edge check and of oracle.nms_bev: a pair it leaves out has IoU exactly 0"""
    b = nc.case('every_n')['groups'][59]
    near = set(nc.near_pairs(b))
    assert 0 < len(near) < len(b) * (len(b) - 1) // 2
    for i in range(len(b)):
        for j in range(i + 1, len(b)):
            if (i, j) not in near:
                assert orc.rotated_iou_bev(b[i], b[j]) == 0.0 and orc.rotated_iou_bev(b[j], b[i]) == 0.0


def test_every_n_suppresses_at_every_size_and_has_ties():
    c = nc.case('every_n')
    assert [len(g) for g in c['groups']] == list(range(1, nc.EVERY_N + 1)) and sum(len(g) for g in c['groups']) == 8515
    for thr in NMS_THRS:
        want = nc.expected('every_n', thr)
        for g, k in zip(c['groups'], want):
            n = len(g)
            assert len(k) == len(set(k.tolist())) and (n < 8 or 1 < len(k) < n), (thr, n, len(k))
        print(f'every_n thr {thr}: {sum(len(k) for k in want)} of 8515 kept')
    grid = (np.arange(1, 20) * np.float32(0.05)).astype(np.float32)
    tied = [len(np.unique(s)) < len(s) for s in c['scores']]
    for s in c['scores']:
        assert np.isin(s, grid).sum() >= (len(s) + 1) // 2           # half of the boxes on the 0.05 grid (19 levels)
    print(f'every_n: ties in {sum(tied)} of {len(tied)} groups, none in sizes {[i + 1 for i, t in enumerate(tied) if not t]}')
    assert all(tied[2:])                                             # every size from 3 on has two boxes of one score


def test_boundaries_use_the_mask_words(orc):
    c = nc.case('boundaries')
    assert tuple(len(g) for g in c['groups']) == nc.BOUNDARY_SIZES == (0, 255, 0, 256, 0, 257, 0, 511, 0, 512, 0)
    b, s = c['groups'][9], c['scores'][9]
    order = orc.nms_order_rule(s)
    place = np.empty(512, int)
    place[order] = np.arange(512)
    ious = nc.pair_ious(b)
    for thr in NMS_THRS:
        want = nc.expected('boundaries', thr)
        assert [len(k) for k, n in zip(want, nc.BOUNDARY_SIZES) if n == 0] == [0] * 6
        assert all(1 < len(k) < n for k, n in zip(want, nc.BOUNDARY_SIZES) if n)
        kept = set(want[9].tolist())
        sup, vic = set(), set()                       # mask words (sorted place / 32) with a kept box that suppresses / a suppressed box
        crossing = 0
        for (i, j), v in ious.items():
            if v > thr:
                hi, lo = (i, j) if place[i] < place[j] else (j, i)
                if hi in kept and lo not in kept:
                    sup.add(place[hi] // 32)
                    vic.add(place[lo] // 32)
                    crossing += place[hi] // 32 != place[lo] // 32
        print(f'boundaries thr {thr}: 512 group keeps {len(kept)}; words that suppress {len(sup)}, are suppressed {len(vic)}, both {len(sup & vic)}; '
              f'{crossing} suppressions cross a word')
        assert len(sup & vic) >= 12 and crossing >= 16


def test_chains_keep_the_box_only_a_removed_box_covers(orc):
    c = nc.case('chains')
    assert [t[4] for t in c['triples']] == list(nc.CHAIN_PLACES) == [31, 32, 63, 64, 65, 480]
    for gi, (g, s, (a, b, cc, pa, pb, pc)) in enumerate(zip(c['groups'], c['scores'], c['triples'])):
        order = orc.nms_order_rule(s)
        assert (order[pa], order[pb], order[pc]) == (a, b, cc) and pa < pb < pc and len(np.unique(s)) == len(s)
        iab, ibc, iac = orc.rotated_iou_bev(g[a], g[b]), orc.rotated_iou_bev(g[b], g[cc]), orc.rotated_iou_bev(g[a], g[cc])
        assert abs(iab - 3.6 / 12.4) < 1e-5 and abs(ibc - 3.6 / 12.4) < 1e-5 and iac == 0.0
        ious = nc.pair_ious(g)
        assert {k for k, v in ious.items() if v > 0} == {tuple(sorted((a, b))), tuple(sorted((b, cc)))}      # the fillers overlap nothing
        for thr in NMS_THRS:
            assert min(iab, ibc) > thr + KNIFE
            want = nc.expected('chains', thr)[gi]
            assert want.tolist() == [i for i in order if i != b] and np.array_equal(want, orc.nms_bev(g, s, thr))
    assert [len(g) for g in c['groups']] == [40, 41, 72, 73, 74, 512]


def test_special_scores_groups(orc):
    c = nc.case('special_scores')
    assert [len(g) for g in c['groups']] == [3, 5, 33, 100, 64, 37, 20]
    for thr in NMS_THRS:
        want = [k.tolist() for k in nc.expected('special_scores', thr)]
        assert want[0] == [0, 2] and want[1] == [0, 2, 3]             # 1 under 0 goes; 2 stays, last; of the twins 3 and 4 the lower stays
        for g, s, k in zip(c['groups'][:5], c['scores'][:5], want[:5]):
            nan = set(np.nonzero(np.isnan(s))[0].tolist())
            assert 1 not in k and 2 in k and (len(g) < 5 or (3 in k and 4 not in k))
            tail = [i for i in k if i in nan]
            assert k[len(k) - len(tail):] == tail == sorted(tail) and tail[0] == 2         # the NaN-scored survivors come last, by index
            if len(g) > 8:
                assert np.isposinf(s).sum() == 2 and np.isneginf(s).sum() == 2 and len(nan) == 5
                assert np.isposinf(s[k[0]]) and 1 < len(k) < len(g)
        assert np.isnan(c['scores'][5]).all() and want[5] == sorted(want[5]) and want[5][0] == 0 and 1 < len(want[5]) < 37
        assert np.isinf(c['scores'][6]).all() and 1 < len(want[6]) < 20
        hi = [i for i in want[6] if c['scores'][6][i] > 0]
        assert want[6][:len(hi)] == hi == sorted(hi) and want[6][len(hi):] == sorted(want[6][len(hi):])


def test_special_boxes_expectations(orc):
    c = nc.case('special_boxes')
    g0, g1, g2 = c['groups']
    assert np.isnan(g0[1]).sum() == 1 and np.isnan(g0[3]).sum() == 1 and np.isfinite(g0[[0, 2, 4]]).all() and np.array_equal(g0[0], g0[4])
    area = np.abs((g1[:, 2] - g1[:, 0]) * (g1[:, 3] - g1[:, 1]))
    assert (area == 0).sum() == 6 and np.array_equal(g1[0], g1[2]) and np.array_equal(g1[4], g1[5]) and np.array_equal(g1[3], g1[6])
    for i in range(len(g1)):                                        # a zero-area box has IoU 0 with everything, itself included
        for j in range(len(g1)):
            if i != j and (area[i] == 0 or area[j] == 0):
                assert orc.rotated_iou_bev(g1[i], g1[j]) == 0.0, (i, j)
    for thr in NMS_THRS:
        assert np.array_equal(orc.nms_bev(g1, c['scores'][1], thr), nc.expected('special_boxes', thr)[1])
        fin = [0, 2, 4]                                             # group 0 without its NaN boxes: the oracle agrees with the hand-written rest
        assert [fin[i] for i in orc.nms_bev(g0[fin], c['scores'][0][fin], thr)] == [0, 2]
    lo, hi = c['swapped']
    assert lo == 2 and np.all(g2[0:6, 2] < g2[0:6, 0]) and np.all(g2[6:12, 3] < g2[6:12, 1]) and np.all((g2[12:18, 2] < g2[12:18, 0]) & (g2[12:18, 3] < g2[12:18, 1]))
    assert np.all(g2[18:, 2] > g2[18:, 0]) and np.all(g2[18:, 3] > g2[18:, 1])
    srt = nc.sorted_coords(g2)
    over = 0
    for i in range(hi):                                             # the oracle's IoU of a swapped box is that of the same rectangle, sorted
        for j in range(len(g2)):
            if i != j:
                v, w = orc.rotated_iou_bev(g2[i], g2[j]), orc.rotated_iou_bev(srt[i], srt[j])
                assert abs(v - w) <= 1e-12 and abs(orc.rotated_iou_bev(g2[j], g2[i]) - w) <= 1e-12
                over += v > 0.25
    assert over >= 6
    for thr in NMS_THRS:
        k = nc.expected('special_boxes', thr)[2]
        assert np.array_equal(k, orc.nms_bev(srt, c['scores'][2], thr)) and 1 < len(k) < len(g2)
        assert set(range(hi)) - set(k.tolist()) and set(range(hi)) & set(k.tolist())       # swapped boxes both go and stay


# ------------------------------------------------------------------------------- the two older GPU tests' groups
def test_older_gpu_tests_groups_have_no_knife_edge():
    """test_consumers.py::test_gpu_nms_matches_oracle and test_gpu_rotated_overlap_edges.py::
    test_nms_group_sizes_at_word_and_padding_boundaries assert plain equality with the oracle; this is what entitles them to."""
    from test_consumers import nms_oracle_groups
    from test_gpu_rotated_overlap_edges import nms_boundary_groups
    for name, (groups, _) in (('test_consumers', nms_oracle_groups()), ('rotated_overlap_edges', nms_boundary_groups())):
        m = min(nc.knife_margin(nc.pair_ious(g), NMS_THRS) for g in groups)
        print(f'{name}: closest pair to a threshold {m:.3e}')
        assert m >= KNIFE, (name, m)
