"""The training step's assembly without a GPU: ``positives_torch`` against the numpy rule of tests/roi_train_ref.py, the C
entry point's argument checks and the loader's row, the literal ``forward_train`` of the RoI head and of the detector on the host (the
3-D stage up to the projection loss: the PnP runs on the GPU only), and ``_parse_losses``."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import roi_train_ref as tr
from monorun_amd import roi_train as RT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ('three-images', 'one-image', 'empty', 'agnostic', 'many')


def bits_equal(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if want.dtype == np.float32:
        return got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ the positive stage
@pytest.mark.parametrize('name', CASES)
def test_positives_torch_equals_the_numpy_rule_bitwise(name):
    case = tr.positives_case(name)
    want = tr.positives_numpy(case)
    got = RT.positives_torch(*tr.case_call(case, 'cpu'))
    assert got.counts == list(case['counts']) and len(got) == sum(case['counts'])
    for k in RT.FIELDS:
        assert bits_equal(getattr(got, k).numpy(), want[k]), (name, k)
    assert [len(v) for v in got.per_image('pos_bboxes')] == list(case['counts'])
    # off the GPU the public entry runs the restatement
    args = tr.case_call(case, 'cpu')
    assert not RT.hip_ok(args[0], args[1], args[2], args[4], args[5], args[8], args[12])
    again = RT.positives(*args)
    assert all(torch.equal(getattr(again, k), getattr(got, k)) for k in RT.FIELDS)


def test_cases_reach_what_they_are_built_for():
    case = tr.positives_case('three-images')
    want = tr.positives_numpy(case)
    assert case['counts'] == [0, 6, 0] and len(case['gt3d'][2]) == 0 and len(case['gt3d'][0]) == 2
    assert (case['pos_inds'][1, :2] == [0, 1]).all()                             # prepended ground truths among the positives
    assert len(set(want['pos_gt_labels'].tolist())) >= 2
    h, w = case['shapes'][1][:2]
    b = want['pos_bboxes']
    assert b[0].tolist() == [0, 0, w, h]                                         # the clip, then all four borders
    assert b[1, 2] - b[1, 0] < 1 and b[1, 3] - b[1, 1] < 1                       # the clip from below: 16 / 1000 of the size
    assert b[2, 0] == 0 and b[2, 1] == 0 and b[3, 2] == w and b[3, 3] == h
    clip = np.float32(abs(np.log(tr.WH_RATIO_CLIP)))
    p = case['bboxes'][1, 0]
    assert np.float32(p[2] - p[0]) * np.exp(clip) > w                             # without the image clamp the box would leave the image
    assert want['flip'].tolist() == [1] * 6 and (want['img_shapes'] == [h, w]).all() and (want['pos_img'] == 1).all()
    many = tr.positives_case('many')
    assert sum(many['counts']) > 2 * 64 and len(set(tr.positives_numpy(many)['flip'].tolist())) == 2


# ------------------------------------------------------------------------------------------------ the loader's row and the argument checks
_PINNED = ('mr_roi_train_positives',)


def test_loader_binds_the_roi_train_header():
    from monorun_amd import _lib
    key = 'roi_train'
    assert key in _lib.LATER_HEADERS and key in _lib.all_header_keys() and key not in _lib.header_keys()
    assert _lib.exported_symbols(key) == _lib.LATER_HEADERS[key][1] == _PINNED
    assert _lib.header_path(key) == os.path.join(ROOT, 'include', 'monorun_roi_train.h')
    assert [n for n, _, _ in _lib.header_prototypes(_lib.header_path(key))] == list(_PINNED)
    for other in _lib.all_header_keys():
        if other != key:
            assert not set(_PINNED) & set(_lib.exported_symbols(other)), other
    lib, raw = _lib.load(), ctypes.CDLL(_lib.SO)
    assert hasattr(raw, _PINNED[0]) and lib.mr_roi_train_positives.restype is ctypes.c_int
    names = _lib.arg_names('mr_roi_train_positives')
    assert names[:5] == ('bboxes', 'gt_inds', 'labels', 'pos_inds', 'pos_offsets') and names[-1] == 'dim_targets' and 'stream' not in names
    assert len(lib.mr_roi_train_positives.argtypes) == len(names) + 1 == 38
    src = open(_lib.header_path(key)).read()
    for cap in ('MR_ROI_TRAIN_MAX_IMAGES MR_ASSIGN_MAX_IMAGES', 'MR_ROI_TRAIN_MAX_GT MR_ASSIGN_MAX_GT', 'MR_ROI_TRAIN_MAX_CLASSES MR_BBOX_MAX_CLASSES'):
        assert re.search(r'#define\s+' + cap.replace(' ', r'\s+'), src), cap
    hip = open(os.path.join(ROOT, 'monorun_amd', 'csrc', 'monorun_pnp.hip')).read()
    assert '#include "monorun_roi_train.h"' in hip and '#include "roi_train_kernel.inc"' in hip and '#include "roi_train_abi.inc"' in hip


def test_argument_checks_without_a_gpu():
    """every check comes before any HIP call: the codes of monorun_pnp.h (-1 bad argument, -2 unsupported); no positives: no launch"""
    from monorun_amd import _lib
    lib = _lib.load()
    BAD, UNSUPPORTED = -1, -2
    one, f4 = ctypes.c_void_p(16), (ctypes.c_float * 4)(1, 1, 1, 1)      # never dereferenced: every call below is rejected before a launch
    pointers = ('bboxes', 'gt_inds', 'labels', 'pos_inds', 'pos_offsets', 'bbox_pred', 'bbox_row_offsets', 'gt_bboxes_3d', 'gt_offsets',
                'cam_intrinsic', 'img_shape', 'flip', 'dim_means', 'dim_stds', 'pos_rois', 'pos_bboxes', 'pos_gt_labels', 'pos_assigned_gt_inds',
                'pos_img', 'pos_img_long', 'pos_bboxes_3d', 'pos_cam_intrinsic', 'pos_img_shapes', 'pos_flip', 'dim_targets')
    base = dict({p: one for p in pointers}, n_images=2, n_boxes=10, num=8, n_pos=5, n_rows=12, num_classes=3, reg_class_agnostic=0, n_gt=4,
                max_gt=3, means=f4, stds=f4, wh_ratio_clip=16 / 1000)

    def call(**over):
        return lib.mr_roi_train_positives(*_lib.pack('mr_roi_train_positives', dict(base, **over)), None)

    for name in ('n_images', 'n_boxes', 'num', 'n_pos', 'n_rows', 'n_gt', 'max_gt'):
        assert call(**{name: -1}) == BAD, name
    assert call(num_classes=0) == BAD and call(means=None) == BAD and call(stds=None) == BAD
    assert call(wh_ratio_clip=0.0) == BAD and call(wh_ratio_clip=-1.0) == BAD and call(wh_ratio_clip=float('nan')) == BAD
    assert call(n_pos=17) == BAD                                         # more positives than n_images * num
    for name in pointers:
        assert call(**{name: None}) == BAD, name
    assert call(max_gt=257) == UNSUPPORTED and call(n_images=65536) == UNSUPPORTED and call(num_classes=17) == UNSUPPORTED
    assert call(n_images=65535, n_boxes=1 << 16) == UNSUPPORTED and call(n_rows=1 << 28) == UNSUPPORTED
    assert call(n_pos=0, **{p: None for p in pointers}) == 0              # K = 0: nothing is launched, nothing is read
    with pytest.raises(TypeError):
        _lib.pack('mr_roi_train_positives', dict(base), no_such_argument=1)


# ------------------------------------------------------------------------------------------------ the heads
def test_roi_head_builds_its_assigners_and_samplers_from_train_cfg():
    from monorun_amd import assigners as A
    from tests import roi_head_ref as rr
    head = tr.build_roi_head(pose=False)
    assert isinstance(head.bbox_assigner, A.MaxIoUAssigner) and isinstance(head.bbox_sampler, A.RandomSampler) and head.bbox_sampler.num == 32
    assert head.bbox_refined_assigner is None and head.bbox_refined_sampler is None
    refined = tr.build_roi_head(pose=False, refined=True)
    assert isinstance(refined.bbox_refined_assigner, A.MaxIoUAssigner) and refined.bbox_refined_sampler.num == 16
    from monorun_amd.roi_head import MonoRUnRoIHead
    cfg = tr.roi_head_cfg()
    cfg.pop('type')
    partial = MonoRUnRoIHead(**cfg, train_cfg=dict(dense_size=28, iou3d_sampler=tr.TRAIN_CFG['rcnn']['iou3d_sampler']))
    assert partial.bbox_assigner is None and partial.bbox_sampler is None and partial.score_head.iou3d_sampler is not None
    assert head.train_decode_reason() is None
    bare = rr.build_roi_head()
    assert bare.bbox_assigner is None and bare.bbox_sampler is None
    with pytest.raises(NotImplementedError, match='train_cfg'):         # an inference head does not train, as before
        bare.forward_train([torch.zeros(1, 16, 4, 4)], [dict()], [torch.zeros(0, 4)], [torch.zeros(0, 4)], [torch.zeros(0)])
    with pytest.raises(NotImplementedError, match='train_cfg'):
        rr.build_detector()(torch.zeros(1, 3, 32, 32), [dict()], return_loss=True)


@pytest.mark.parametrize('refined', [False, True])
def test_literal_forward_train_runs_on_the_host(refined):
    """fails on the parent commit: forward_train raised NotImplementedError"""
    head = tr.build_roi_head(pose=False, refined=refined)
    inputs = tr.batch_inputs('cpu', n_images=2, n_proposals=(12, 9))
    assert head.train_fast_path_reason(inputs['x']) == 'the feature maps are not CUDA fp32'
    with pytest.raises(RuntimeError, match='not CUDA fp32'):
        head.forward_train(**inputs, path='fast')
    losses = head.forward_train(**inputs, generator=torch.Generator().manual_seed(2))
    assert head.last_train_path == 'literal'
    assert set(losses) == {'loss_cls', 'acc', 'loss_bbox', 'loss_dim', 'loss_noc', 'loss_proj'}
    total = sum(v for k, v in losses.items() if 'loss' in k)
    assert torch.isfinite(total)
    total.backward()
    for part in (head.bbox_head, head.global_head, head.noc_head):
        grads = [p.grad for p in part.parameters() if p.grad is not None]
        assert grads and all(torch.isfinite(g).all() for g in grads) and sum(float(g.abs().sum()) for g in grads) > 0, type(part).__name__


def test_literal_forward_train_without_positives_on_the_host():
    head = tr.build_roi_head(pose=False)
    inputs = tr.batch_inputs('cpu', n_images=2, n_proposals=(6, 5), empty=True)
    losses = head.forward_train(**inputs, generator=torch.Generator().manual_seed(2))
    assert all(torch.isfinite(v).all() for v in losses.values())
    assert float(losses['loss_dim']) == 0 and float(losses['loss_noc']) == 0 and float(losses['loss_bbox']) == 0
    sum(v for k, v in losses.items() if 'loss' in k).sum().backward()


def test_detector_forward_with_return_loss_runs_on_the_host():
    """fails on the parent commit: forward(return_loss=True) raised NotImplementedError"""
    det = tr.build_detector(pose=False)
    inputs = tr.batch_inputs('cpu', n_images=2, n_proposals=(4, 4))
    g = torch.Generator().manual_seed(4)
    img = torch.randn(2, 3, tr.IMG_H, tr.IMG_W, generator=g)
    data = dict(img=img, **{k: v for k, v in inputs.items() if k not in ('x', 'proposal_list')})
    losses = det(**data, return_loss=True)
    assert {'loss_rpn_cls', 'loss_rpn_bbox', 'loss_cls', 'acc', 'loss_bbox', 'loss_dim', 'loss_noc', 'loss_proj'} == set(losses)
    assert isinstance(losses['loss_rpn_cls'], list) and len(losses['loss_rpn_cls']) == 5
    out = det.train_step(data)
    assert set(out) == {'loss', 'log_vars', 'num_samples'} and out['num_samples'] == 2 and torch.isfinite(out['loss'])
    assert set(out['log_vars']) == set(losses) | {'loss'} and all(isinstance(v, float) for v in out['log_vars'].values())


def test_parse_losses_sums_the_loss_keys_and_the_lists():
    from monorun_amd.detector import MonoRUnDetector
    losses = dict(loss_a=torch.tensor([1.0, 3.0]), loss_list=[torch.tensor(0.5), torch.tensor([1.0, 2.0])], acc=torch.tensor([80.0]),
                  mean_iou=torch.tensor(0.25))
    loss, log_vars = MonoRUnDetector._parse_losses(losses)
    assert float(loss) == 2.0 + (0.5 + 1.5) and list(log_vars) == ['loss_a', 'loss_list', 'acc', 'mean_iou', 'loss']
    assert log_vars == dict(loss_a=2.0, loss_list=2.0, acc=80.0, mean_iou=0.25, loss=4.0)
    with pytest.raises(TypeError, match='acc'):
        MonoRUnDetector._parse_losses(dict(acc=1.0))
