"""Consumer of G23 (tests/golden/make_golden_detector_train_mmdet.py): mmdet 2.x's own ``MaxIoUAssigner.assign``, ``bbox2delta``,
``AnchorHead.get_targets`` under a fixed sampling and the two heads' ``loss`` dictionaries, recorded where mmdet exists.  mmdet does not
import in this repository's image, so the fixture is absent and the tests SKIP BY NAME, saying which command records it; the generator has
not been run.  With the fixture present they turn "pinned against the stated definition" into a measured statement.

Bars: the assignment exact (the recorded cases are tie-free: tests/test_assign_cpu.py asserts their margins); max_overlaps and the deltas
within DELTA_C 2^-23 magnitudes of the float64 rule's terms; the losses within 1e-5 relative (sums of a few thousand fp32 terms)."""
import os

import numpy as np
import pytest
import torch

from tests import detector_train_ref as ref
from tests.test_assign_cpu import DELTA_C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
NAME = 'g23_detector_train_mmdet.npz'


def _load():
    f = os.path.join(GOLDEN, NAME)
    if not os.path.exists(f):
        pytest.skip(f'{NAME} is absent: it can only be recorded where mmdet 2.x imports — python tests/golden/make_golden_detector_train_mmdet.py')
    return dict(np.load(f, allow_pickle=False))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def test_assignment_and_deltas_equal_mmdet():
    from monorun_amd import assigners as A
    g23 = _load()
    for seed in ref.MARGIN_SEEDS:
        b, g = ref.margin_case(seed)
        labels = np.arange(len(g)) % 3
        for t, thr in enumerate(ref.THRESHOLDS):
            got = A.MaxIoUAssigner(**thr).assign(_t(b), _t(g), None, _t(labels))
            assert np.array_equal(got.gt_inds.numpy(), g23[f'assign_{seed}_{t}_gt_inds'])
            assert np.array_equal(got.labels.numpy(), g23[f'assign_{seed}_{t}_labels'])
            assert np.abs(got.max_overlaps.numpy() - g23[f'assign_{seed}_{t}_max_overlaps']).max() <= 16 * 2.0 ** -23      # eight roundings each side
    p, g = ref.delta_cases()
    for key, stds in (('deltas_unit', (1, 1, 1, 1)), ('deltas_rcnn', ref.RCNN_STDS)):
        want, terms = ref.bbox2delta(p, g, stds=stds, dtype=np.float64), ref.delta_bound_terms(p, g, stds=stds)
        assert (np.abs(g23[key] - want) <= DELTA_C * 2.0 ** -23 * terms).all()                       # mmdet's own fp32 within the bound
        assert (np.abs(A.bbox2delta(_t(p), _t(g), stds=stds).numpy() - g23[key]) <= 2 * DELTA_C * 2.0 ** -23 * terms).all()


def test_rpn_targets_and_both_losses_equal_mmdet():
    from tests.test_assign_cpu import make_bbox_head, make_rpn
    g23 = _load()
    head = make_rpn()
    _, gts = ref.margin_case(ref.MARGIN_SEEDS[0])
    gts = [_t(gts[:4]), _t(gts[4:])]
    metas = [dict(img_shape=(48, 80, 3), pad_shape=(48, 80, 3), scale_factor=1.0)] * 2
    keys = _t(np.tile(np.arange(945, dtype=np.float32) / 1024.0, (2, 1)))                           # keys that grow with the index: the fixed sampling
    head.assigner.ignore_iof_thr = -1.0
    anchors, flags = head.get_anchors([(12, 20), (6, 10), (3, 5)], metas, 'cpu')
    labels, label_weights, bbox_targets, bbox_weights, num_pos, num_neg = head.get_targets(anchors, flags, gts, metas, keys=keys)
    assert np.array_equal(labels.numpy(), g23['rpn_labels']) and np.array_equal(label_weights.numpy(), g23['rpn_label_weights'])
    assert np.array_equal(bbox_weights.numpy(), g23['rpn_bbox_weights']) and [int(num_pos), int(num_neg)] == g23['rpn_num_total'].tolist()
    assert np.abs(bbox_targets.numpy() - g23['rpn_bbox_targets']).max() <= 1e-5
    losses = head.loss([_t(g23[f'rpn_cls{l}']) for l in range(3)], [_t(g23[f'rpn_reg{l}']) for l in range(3)], gts, metas, keys=keys)
    for l in range(3):
        assert abs(float(losses['loss_rpn_cls'][l]) - g23['rpn_loss_cls'][l]) <= 1e-5 * g23['rpn_loss_cls'][l]
        assert abs(float(losses['loss_rpn_bbox'][l]) - g23['rpn_loss_bbox'][l]) <= 1e-5 * g23['rpn_loss_bbox'][l] + 1e-8
    box = make_bbox_head()
    got = box.loss(_t(g23['box_cls_score']), _t(g23['box_bbox_pred']), None, _t(g23['box_labels']), _t(g23['box_label_weights']),
                   _t(g23['box_bbox_targets']), _t(g23['box_bbox_weights']))
    want = g23['box_losses']
    assert abs(float(got['loss_cls']) - want[0]) <= 1e-5 * want[0] and abs(float(got['acc']) - want[1]) <= 1e-4
    assert abs(float(got['loss_bbox']) - want[2]) <= 1e-5 * want[2]
