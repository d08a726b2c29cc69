"""The proposal stage against the real mmcv.ops.batched_nms and mmdet's RPNHead.get_bboxes (G22,
tests/golden/make_golden_proposals_mmcv.py).  Neither package exists in this image, so the fixture is absent here and the test SKIPS BY
NAME, saying which command records it."""
import os

import numpy as np
import pytest
import torch

from tests import proposals_ref as ref

G22 = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g22_proposals_mmcv.npz')


def test_g22_mmcv_nms_and_mmdet_rpn_against_this_project():
    if not os.path.exists(G22):
        pytest.skip('g22_proposals_mmcv.npz is absent: it can only be recorded where mmcv.ops.nms (a CUDA extension), mmdet and their device '
                    'exist — python tests/golden/make_golden_proposals_mmcv.py')
    from monorun_amd.proposals import batched_nms
    from tests.golden.make_golden_proposals_mmcv import nms_inputs
    from tests.test_proposals_cpu import head, metas
    g = np.load(G22)
    cases = {c['name']: c for c in ref.nms_cases()}
    for name in ref.MARGIN_CASES:
        boxes, scores, idxs = (torch.from_numpy(a) for a in nms_inputs(cases[name]))
        for tag, agnostic in (('aware', False), ('agnostic', True)):
            dets, keep = batched_nms(boxes, scores, idxs, dict(type='nms', iou_threshold=cases[name]['thr']), class_agnostic=agnostic)
            assert np.array_equal(keep.numpy(), g[f'{name}_{tag}_keep']) and np.array_equal(dets.numpy(), g[f'{name}_{tag}_dets'])
    c = ref.e2e_case()
    got = head().get_bboxes([torch.from_numpy(x) for x in c['cls']], [torch.from_numpy(x) for x in c['reg']], metas())
    for n, p in enumerate(got):
        want = g[f'rpn_image{n}']
        assert p.shape == want.shape                                    # the case keeps 5e-3 from the threshold: the same kept set
        assert np.allclose(p.numpy(), want, rtol=1e-5, atol=1e-4)       # mmdet's decode runs torch's exp in another order
