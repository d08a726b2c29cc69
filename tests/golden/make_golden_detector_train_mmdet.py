#!/usr/bin/env python3
"""G23: the 2-D detector's training targets and losses as mmdet 2.x computes them.  Runs only where
mmdet imports — not in this repository's image; the fixture is therefore ABSENT until somebody records it there, and
tests/test_detector_train_mmdet_golden.py skips by name meanwhile.  It has not been run where it was written.

    python tests/golden/make_golden_detector_train_mmdet.py      # writes tests/golden/g23_detector_train_mmdet.npz

Recorded, on the tie-free cases only (the margin seeds of tests/detector_train_ref.py, whose float64 overlaps keep 1e-5 from every
threshold and from each other, so no ``==`` and no argmax depends on an implementation's rounding): ``MaxIoUAssigner.assign`` under both
threshold sets, ``bbox2delta`` on the delta cases, ``AnchorHead.get_targets`` of an ``RPNHead`` under a FIXED sampling (a sampler that
takes the lowest-index positives and negatives: mmdet's ``randperm`` stream is not what this library draws from) and the ``loss``
dictionaries of ``RPNHead`` and ``Shared2FCBBoxHead`` on recorded head outputs.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import detector_train_ref as ref  # noqa: E402


def main():
    from mmcv import ConfigDict
    from mmdet.core import build_assigner
    from mmdet.core.bbox.coder.delta_xywh_bbox_coder import bbox2delta
    from mmdet.core.bbox.samplers import BaseSampler, SamplingResult
    from mmdet.core.bbox.builder import BBOX_SAMPLERS
    from mmdet.models.dense_heads import RPNHead
    from mmdet.models.roi_heads.bbox_heads import Shared2FCBBoxHead

    @BBOX_SAMPLERS.register_module(force=True)
    class FirstSampler(BaseSampler):
        """the lowest-index positives and negatives: RandomSampler's counts with keys that grow with the index"""

        def _sample_pos(self, assign_result, num_expected, **kwargs):
            return torch.nonzero(assign_result.gt_inds > 0, as_tuple=False).squeeze(1)[:num_expected]

        def _sample_neg(self, assign_result, num_expected, **kwargs):
            return torch.nonzero(assign_result.gt_inds == 0, as_tuple=False).squeeze(1)[:num_expected]

    out = {}
    for seed in ref.MARGIN_SEEDS:
        b, g = ref.margin_case(seed)
        labels = torch.arange(len(g)) % 3
        for t, thr in enumerate(ref.THRESHOLDS):
            res = build_assigner(dict(type='MaxIoUAssigner', match_low_quality=True, ignore_iof_thr=-1, **thr)).assign(
                torch.from_numpy(b), torch.from_numpy(g), None, labels)
            out[f'assign_{seed}_{t}_gt_inds'], out[f'assign_{seed}_{t}_max_overlaps'] = res.gt_inds.numpy(), res.max_overlaps.numpy()
            out[f'assign_{seed}_{t}_labels'] = res.labels.numpy()
    p, g = ref.delta_cases()
    out['deltas_unit'] = bbox2delta(torch.from_numpy(p), torch.from_numpy(g)).numpy()
    out['deltas_rcnn'] = bbox2delta(torch.from_numpy(p), torch.from_numpy(g), (0., 0., 0., 0.), ref.RCNN_STDS).numpy()

    # the RPN on a 48 x 80 image: targets under the fixed sampling and the loss dictionary on recorded outputs
    b, gts = ref.margin_case(ref.MARGIN_SEEDS[0])
    gts = [torch.from_numpy(gts[:4]), torch.from_numpy(gts[4:])]
    train_cfg = ConfigDict(assigner=dict(type='MaxIoUAssigner', match_low_quality=True, ignore_iof_thr=-1, **ref.THRESHOLDS[0]),
                           sampler=dict(type='FirstSampler', num=64, pos_fraction=0.5, neg_pos_ub=-1, add_gt_as_proposals=False),
                           allowed_border=-1, pos_weight=-1, debug=False)
    torch.manual_seed(0)
    head = RPNHead(8, feat_channels=8, anchor_generator=dict(type='AnchorGenerator', scales=[8], ratios=[0.5, 1.0, 2.0], strides=[4, 8, 16]),
                   loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
                   loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0), train_cfg=train_cfg)
    metas = [dict(img_shape=(48, 80, 3), pad_shape=(48, 80, 3), scale_factor=1.0)] * 2
    gen = torch.Generator().manual_seed(3)
    cls = [torch.randn(2, 3, 48 // s, 80 // s, generator=gen) for s in (4, 8, 16)]
    reg = [0.3 * torch.randn(2, 12, 48 // s, 80 // s, generator=gen) for s in (4, 8, 16)]
    sizes = [c.shape[-2:] for c in cls]
    anchor_list, valid_flag_list = head.get_anchors(sizes, metas, device='cpu')
    targets = head.get_targets(anchor_list, valid_flag_list, gts, metas)
    for name, per_level in zip(('labels', 'label_weights', 'bbox_targets', 'bbox_weights'), targets[:4]):
        out['rpn_' + name] = torch.cat([t.reshape(2, -1, *t.shape[2:]) for t in per_level], dim=1).numpy()
    out['rpn_num_total'] = np.array(targets[4:6])
    losses = head.loss(cls, reg, gts, metas)
    for l in range(3):
        out[f'rpn_cls{l}'], out[f'rpn_reg{l}'] = cls[l].numpy(), reg[l].numpy()
    out['rpn_loss_cls'] = np.array([float(v) for v in losses['loss_rpn_cls']])
    out['rpn_loss_bbox'] = np.array([float(v) for v in losses['loss_rpn_bbox']])

    # the box head's loss on recorded targets
    box = Shared2FCBBoxHead(in_channels=8, fc_out_channels=16, roi_feat_size=7, num_classes=3,
                            loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0),
                            loss_bbox=dict(type='SmoothL1Loss', beta=1.0, loss_weight=1.0))
    R = 40
    out['box_cls_score'], out['box_bbox_pred'] = torch.randn(R, 4, generator=gen).numpy(), torch.randn(R, 12, generator=gen).numpy()
    out['box_labels'] = np.concatenate((np.arange(10) % 3, np.full(R - 10, 3))).astype(np.int64)
    out['box_label_weights'] = np.ones(R, dtype=np.float32)
    out['box_bbox_targets'] = np.concatenate((torch.randn(10, 4, generator=gen).numpy(), np.zeros((R - 10, 4), dtype=np.float32)))
    out['box_bbox_weights'] = np.concatenate((np.ones((10, 4), dtype=np.float32), np.zeros((R - 10, 4), dtype=np.float32)))
    t = lambda k: torch.from_numpy(out[k])
    got = box.loss(t('box_cls_score'), t('box_bbox_pred'), None, t('box_labels'), t('box_label_weights'), t('box_bbox_targets'), t('box_bbox_weights'))
    out['box_losses'] = np.array([float(got['loss_cls']), float(got['acc']), float(got['loss_bbox'])])
    path = os.path.join(HERE, 'g23_detector_train_mmdet.npz')
    np.savez_compressed(path, **out)
    print('G23:', os.path.getsize(path) // 1024, 'KiB')


if __name__ == '__main__':
    main()
