"""``MonoRUnRoIHead`` and ``MonoRUnDetector`` without a GPU: they build from a reference-shaped config dict (tests/roi_head_ref.py, at
reduced widths), their ``state_dict`` keys are the prefixed sub-modules', a round trip loads with ``strict=True``, an unknown type is a
``KeyError``, the training entry points say what they are, and the host-side split of the packed result buffer gives the reference's
per-class lists."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import roi_head_ref as rr  # noqa: E402

ROI_PARTS = ('bbox_head', 'noc_head', 'global_head', 'projection_head', 'pose_head', 'score_head')


def test_roi_head_builds_from_the_config_and_its_keys_are_the_sub_modules():
    from monorun_amd import MonoRUnRoIHead
    head = rr.build_roi_head()
    assert isinstance(head, MonoRUnRoIHead)
    assert head.with_bbox and head.with_noc and head.with_reg and head.with_projection and head.with_pose and head.with_score
    want = set()
    for part in ROI_PARTS:
        sub = getattr(head, part).state_dict()
        assert sub or part == 'projection_head' or part == 'pose_head', part
        want |= {f'{part}.{k}' for k in sub}
    assert set(head.state_dict()) == want and not list(head.bbox_roi_extractor.state_dict()) and not list(head.noc_roi_extractor.state_dict())
    assert 'pose_head.cov_calib_logscale' in want and any(k.startswith('projection_head.loss_proj.') for k in want)
    other = rr.build_roi_head(seed=5)
    assert any(not torch.equal(a, b) for a, b in zip(head.state_dict().values(), other.state_dict().values()))
    other.load_state_dict(head.state_dict(), strict=True)
    assert all(torch.equal(a, b) for a, b in zip(head.state_dict().values(), other.state_dict().values()))
    assert head.test_cfg['nms_3d_thr'] == 0.01 and head.new_version


def test_detector_builds_from_the_config_with_the_checkpoint_prefixes(tmp_path):
    from monorun_amd import MonoRUnDetector
    det = rr.build_detector()
    assert isinstance(det, MonoRUnDetector) and det.with_neck and det.with_rpn and det.with_bbox
    want = set()
    for part in ('backbone', 'neck', 'rpn_head', 'roi_head'):
        want |= {f'{part}.{k}' for k in getattr(det, part).state_dict()}
    assert set(det.state_dict()) == want and {k.split('.')[0] for k in want} == {'backbone', 'neck', 'rpn_head', 'roi_head'}
    assert det.rpn_head.test_cfg == rr.TEST_CFG['rpn'] and det.roi_head.test_cfg == rr.TEST_CFG['rcnn']
    path = tmp_path / 'ckpt.pth'
    torch.save(dict(state_dict=det.state_dict(), meta={}), path)
    other = rr.build_detector(seed=3)
    other.load_state_dict(torch.load(path, map_location='cpu')['state_dict'], strict=True)
    assert all(torch.equal(a, b) for a, b in zip(det.state_dict().values(), other.state_dict().values()))
    x = det.extract_feat(torch.randn(1, 3, rr.IMG_H, rr.IMG_W, generator=torch.Generator().manual_seed(0)))
    assert [tuple(f.shape[1:]) for f in x] == [(16, 48, 160), (16, 24, 80), (16, 12, 40), (16, 6, 20), (16, 3, 10), (16, 2, 5)]
    # pretrained: a local file loads into the backbone; a URL raises and nothing is fetched
    torch.save(det.backbone.state_dict(), tmp_path / 'backbone.pth')
    again = MonoRUnDetector(**rr.model_cfg(), test_cfg=rr.TEST_CFG, pretrained=str(tmp_path / 'backbone.pth'))
    assert all(torch.equal(a, b) for a, b in zip(det.backbone.state_dict().values(), again.backbone.state_dict().values()))
    with pytest.raises(ValueError):
        MonoRUnDetector(**rr.model_cfg(), test_cfg=rr.TEST_CFG, pretrained='torchvision://resnet18')


def test_built_modules_are_taken_as_they_are():
    from monorun_amd import MonoRUnRoIHead
    from monorun_amd.roi_head import build
    head = rr.build_roi_head()
    same = MonoRUnRoIHead(bbox_roi_extractor=head.bbox_roi_extractor, bbox_head=head.bbox_head, noc_roi_extractor=head.noc_roi_extractor,
                          noc_head=head.noc_head, global_head=head.global_head, projection_head=head.projection_head, pose_head=head.pose_head,
                          score_head=head.score_head, test_cfg=head.test_cfg)
    assert same.bbox_head is head.bbox_head and same.score_head is head.score_head and set(same.state_dict()) == set(head.state_dict())
    assert build(None) is None and build(head.noc_head) is head.noc_head


def test_an_unknown_type_is_a_key_error_naming_it():
    from monorun_amd import MonoRUnDetector, MonoRUnRoIHead
    from monorun_amd.roi_head import build
    with pytest.raises(KeyError, match='DoubleHeadRoIExtractor'):
        build(dict(type='DoubleHeadRoIExtractor', out_channels=16))
    cfg = rr.roi_head_cfg()
    cfg.pop('type')
    cfg['score_head'] = dict(type='ConvScoreHead')
    with pytest.raises(KeyError, match='ConvScoreHead'):
        MonoRUnRoIHead(**cfg)
    model = rr.model_cfg()
    model['neck'] = dict(type='PAFPN', in_channels=[8, 16, 32, 64], out_channels=16, num_outs=5)
    with pytest.raises(KeyError, match='PAFPN'):
        MonoRUnDetector(**model)
    model = rr.model_cfg()
    model['roi_head']['type'] = 'StandardRoIHead'
    with pytest.raises(KeyError, match='StandardRoIHead'):
        MonoRUnDetector(**model)


def test_training_and_augmented_entry_points_are_not_implemented():
    head, det = rr.build_roi_head(), rr.build_detector()
    with pytest.raises(NotImplementedError, match='follow-up'):
        head.forward_train([], [], [], [], [])
    for fn in (head.aug_test, head.forward_dummy):
        with pytest.raises(NotImplementedError):
            fn(None, None)
    with pytest.raises(NotImplementedError):
        det(torch.zeros(1, 3, 32, 32), [dict()], return_loss=True)
    with pytest.raises(NotImplementedError):
        det.forward_test([torch.zeros(1, 3, 32, 32)] * 2, [[dict()]] * 2)
    with pytest.raises(TypeError):
        det.forward_test(torch.zeros(1, 3, 32, 32), [dict()])


def test_packed_result_splits_into_the_reference_lists():
    """what simple_test's fast path hands back: a packed buffer written by hand here — class 0 keeps two members, class 1 has none,
    class 2 keeps one — split into the reference's per-class lists (the layout itself: tests/test_result3d_cases_cpu.py)"""
    from monorun_amd.consumers import result_3d_layout, split_packed_result
    C, n = 3, 4
    layout, size = result_3d_layout(C, n)
    buf = np.zeros(size, np.uint8)
    f = {k: buf[off:off + int(np.prod(shape)) * dt.itemsize].view(dt).reshape(shape) for k, (off, dt, shape) in layout.items()}
    f['out3d'][:], f['out2d'][:], f['keep_local'][:], f['keep_row'][:] = np.nan, np.nan, -1, -1
    f['num_keep'][:], f['num_in_class'][:] = [2, 0, 1], [3, 0, 1]
    f['out3d'][0, :2] = [[3.9, 1.5, 1.6, 1.0, 1.6, 20.0, 0.1, 0.9], [3.8, 1.4, 1.7, -4.0, 1.5, 31.0, -1.2, 0.4]]
    f['out2d'][0, :2] = [[10, 20, 110, 90, 0.95], [300, 40, 360, 80, 0.7]]
    f['keep_local'][0, :2], f['keep_row'][0, :2] = [2, 0], [3, 0]
    f['out3d'][2, 0], f['out2d'][2, 0], f['keep_local'][2, 0], f['keep_row'][2, 0] = np.arange(8), np.arange(5), 0, 2
    b3, inds, b2, rows = split_packed_result(buf, C, n)
    assert [a.shape for a in b3] == [(2, 8), (0, 8), (1, 8)] and [a.shape for a in b2] == [(2, 5), (0, 5), (1, 5)]
    assert all(a.dtype == np.float32 for a in b3 + b2) and all(i.dtype == np.int64 for i in inds + rows)
    assert inds[0].tolist() == [2, 0] and rows[0].tolist() == [3, 0] and inds[1].shape == (0,) and inds[2].tolist() == [0] and rows[2].tolist() == [2]
    assert np.array_equal(b3[0], f['out3d'][0, :2]) and np.array_equal(b2[0], f['out2d'][0, :2]) and b3[2][0].tolist() == list(range(8))
    empty = split_packed_result(np.zeros(result_3d_layout(C, 0)[1], np.uint8), C, 0)          # no detections: C arrays of (0, 8) / (0, 5)
    assert [a.shape for a in empty[0]] == [(0, 8)] * 3 and [a.shape for a in empty[2]] == [(0, 5)] * 3 and all(i.dtype == np.int64 for i in empty[1])


def test_literal_path_is_chosen_off_the_gpu_and_says_why():
    head = rr.build_roi_head()
    x = [torch.zeros(1, 16, 4, 4)]
    reg = dict(distance_pred=None)
    assert head.fast_path_reason(x, reg, 10) == 'the feature maps are not CUDA fp32'
    assert np.isfinite(head._decode_kw(None)['ref_length']) and head._decode_kw(None)['num_classes'] == 3
    kw = head._decode_kw(None)
    assert abs(kw['ref_length'] * kw['ref_focal_y'] * kw['target_std'] - head.projection_head.proj_error_coder.scaling_denomitor) < 1e-9
