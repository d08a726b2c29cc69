#!/usr/bin/env python3
"""G22: the proposal stage as the real packages compute it: ``mmcv.ops.batched_nms`` and mmdet's ``RPNHead.get_bboxes`` (INTEGRATION.md
§8).  Runs only where mmcv's compiled NMS op, mmdet and a device they support exist — not in this repository's image, where neither
imports; the fixture is therefore ABSENT until somebody records it there, and tests/test_proposals_mmcv_golden.py skips by name
meanwhile.  It has not been run where it was written.

    python tests/golden/make_golden_proposals_mmcv.py      # writes tests/golden/g22_proposals_mmcv.npz

Recorded: for every clustered set of 600 of tests/proposals_ref (the cases whose float64 IoUs keep 1e-5 from the threshold, so mmcv's
coordinate-offset trick cannot flip a decision), with strictly decreasing scores (no ties: mmcv leaves those to an unstable sort) and
labels i % 3, ``batched_nms``'s dets and keep, class-aware and class-agnostic; and ``RPNHead.get_bboxes`` on the end-to-end case of
proposals_ref (its margins are asserted by tests/test_proposals_cpu.py).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import proposals_ref as ref  # noqa: E402


def nms_inputs(case):
    """the boxes of a one-group case in rank order, strictly decreasing scores, labels i % 3"""
    n = len(case['boxes'])
    return case['boxes'], (1.0 - np.arange(n) / 1024.0).astype(np.float32), (np.arange(n) % 3).astype(np.int64)


def main():
    from mmcv.ops import batched_nms
    from mmdet.models.dense_heads import RPNHead
    dev = torch.device('cuda')
    out = {}
    cases = {c['name']: c for c in ref.nms_cases()}
    for name in ref.MARGIN_CASES:
        boxes, scores, idxs = (torch.from_numpy(a).to(dev) for a in nms_inputs(cases[name]))
        for tag, agnostic in (('aware', False), ('agnostic', True)):
            dets, keep = batched_nms(boxes, scores, idxs, dict(type='nms', iou_threshold=cases[name]['thr']), class_agnostic=agnostic)
            out[f'{name}_{tag}_dets'], out[f'{name}_{tag}_keep'] = dets.cpu().numpy(), keep.cpu().numpy()
    c = ref.e2e_case()
    cfg = dict(nms_across_levels=False, nms_pre=ref.E2E_NMS_PRE, nms_post=ref.E2E_NMS_POST, max_num=ref.E2E_NMS_POST, nms_thr=ref.E2E_THR,
               min_bbox_size=ref.E2E_MIN_SIZE)
    head = RPNHead(8, feat_channels=8, anchor_generator=dict(type='AnchorGenerator', scales=[2], ratios=[0.4, 0.7, 1.0], strides=list(ref.STRIDES)),
                   bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=list(ref.MEANS), target_stds=list(ref.STDS)), test_cfg=cfg).to(dev)
    metas = [dict(img_shape=(int(h), int(w), 3), scale_factor=1.0) for h, w in ref.IMG_SHAPES]
    from mmcv import ConfigDict
    props = head.get_bboxes([torch.from_numpy(x).to(dev) for x in c['cls']], [torch.from_numpy(x).to(dev) for x in c['reg']], metas, ConfigDict(cfg))
    for n, p in enumerate(props):
        out[f'rpn_image{n}'] = p.cpu().numpy()
    path = os.path.join(HERE, 'g22_proposals_mmcv.npz')
    np.savez_compressed(path, **out)
    print('G22:', os.path.getsize(path) // 1024, 'KiB')


if __name__ == '__main__':
    main()
