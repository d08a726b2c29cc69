"""The order in which nms_bev_kernel visits a group's boxes (csrc/nms_order.inc), checked without a GPU: the oracle library compiles the
kernel's own comparator and padded bitonic network from that include and runs them on the host (orc_nms_order), and the result has to
equal the written rule (oracle.nms_order_rule, plain Python) for every group size the kernel accepts.

The comparator this replaces let padding entries pass NaN scores: with one NaN in a group whose size is no power of two the kernel
loaded a box from index 0x7fffffff.  That no padding index can appear among the first n places is what this file pins, and what makes
the NaN-score cases of tests/test_gpu_nms_bev.py safe to run."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_consumers import _rand_boxes  # noqa: E402

PAD = 0x7fffffff
NMAX = 512                                         # kNmsMax


def score_classes(n, rng):
    """the six score vectors of one size"""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    distinct = rng.permutation(n).astype(np.float32) / np.float32(n)
    levels = rng.integers(0, 5, n).astype(np.float32) * np.float32(0.25)
    equal = np.full(n, 0.5, np.float32)
    few = rng.uniform(0, 1, n).astype(np.float32)
    few[[0, n - 1]] = nan                          # first and last place
    few[rng.integers(0, n, 1 + n // 50)] = nan     # and random ones
    all_nan = np.full(n, nan, np.float32)
    mixed = rng.choice(np.array([inf, -inf, nan, 0.0, 0.5, 0.5, -1.0, 3.0e38, -3.0e38], np.float32), n)
    return dict(distinct=distinct, levels=levels, equal=equal, few_nan=few, all_nan=all_nan, inf_ties_nan=mixed)


def test_rule_on_written_examples(orc):
    """the rule itself, by hand"""
    nan, inf = float('nan'), float('inf')
    assert orc.nms_order_rule([0.5, nan, 0.3]) == [0, 2, 1]
    assert orc.nms_order_rule([nan, nan, 0.3, 0.1, 0.3]) == [2, 4, 3, 0, 1]
    assert orc.nms_order_rule([-inf, 0.0, inf, nan, -inf, inf]) == [2, 5, 1, 0, 4, 3]
    assert orc.nms_order_rule([nan] * 4) == [0, 1, 2, 3]
    assert orc.nms_order_rule([]) == []
    # the two groups whose order the earlier comparator got wrong (a padding index among the first n places)
    assert orc.nms_order([0.5, nan, 0.3]).tolist() == [0, 2, 1]
    assert orc.nms_order([nan, nan, 0.3, 0.1, 0.3]).tolist() == [2, 4, 3, 0, 1]


def test_shared_network_equals_the_rule_for_every_group_size(orc):
    rng = np.random.default_rng(20)
    checked = 0
    for n in range(1, NMAX + 1):
        for name, s in score_classes(n, rng).items():
            got = orc.nms_order(s)
            assert PAD not in got, (n, name)
            assert np.array_equal(np.sort(got), np.arange(n)), (n, name)
            assert got.tolist() == orc.nms_order_rule(s), (n, name)
            checked += 1
    assert checked == 6 * NMAX


def test_score_classes_hold_what_they_claim():
    rng = np.random.default_rng(21)
    for n in (1, 2, 3, 33, 100, 512):
        c = score_classes(n, rng)
        assert len(np.unique(c['distinct'])) == n and len(np.unique(c['equal'])) == 1 and np.isnan(c['all_nan']).all()
        assert np.isnan(c['few_nan'][0]) and np.isnan(c['few_nan'][-1])
        if n >= 33:
            assert len(np.unique(c['levels'])) == 5 and not np.isnan(c['few_nan']).all()
            m = c['inf_ties_nan']
            assert np.isposinf(m).sum() > 1 and np.isneginf(m).sum() > 1 and np.isnan(m).sum() > 1 and (m == 0.5).sum() > 1


def test_oracle_nms_orders_nan_scores_last(orc):
    """oracle.nms_bev takes its order from the rule: far-apart boxes are all kept, in that order"""
    n = 7
    boxes = np.array([[10.0 * i, 0, 10.0 * i + 2, 1, 0.3] for i in range(n)], np.float32)
    s = np.array([0.2, np.nan, np.inf, 0.2, -np.inf, np.nan, 0.9], np.float32)
    assert orc.nms_bev(boxes, s, 0.25).tolist() == [2, 6, 0, 3, 4, 1, 5]
    boxes[5] = boxes[1]                                             # two identical NaN-scored boxes: the lower index survives
    assert orc.nms_bev(boxes, s, 0.25).tolist() == [2, 6, 0, 3, 4, 1]
    boxes[1] = boxes[5] = boxes[4]                                  # under a -inf-scored box: both go
    assert orc.nms_bev(boxes, s, 0.25).tolist() == [2, 6, 0, 3, 4]


@pytest.mark.parametrize('thr', [0.01, 0.25])
def test_oracle_nms_near_pair_shortcut_changes_nothing(orc, thr):
    """oracle.nms_bev clips only pairs close enough to intersect; the result equals the all-pairs loop"""
    rng = np.random.default_rng(22)
    b = _rand_boxes(rng, 80, spread=8.0)
    s = rng.uniform(0, 1, 80).astype(np.float32)
    order = orc.nms_order_rule(s)
    keep, dead = [], set()
    for ii, i in enumerate(order):
        if i in dead:
            continue
        keep.append(i)
        dead |= {j for j in order[ii + 1:] if orc.rotated_iou_bev(b[i], b[j]) > thr}
    assert orc.nms_bev(b, s, thr).tolist() == keep and 1 < len(keep) < 80
