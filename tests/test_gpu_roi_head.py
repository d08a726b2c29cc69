"""``MonoRUnRoIHead.simple_test`` and ``MonoRUnDetector.simple_test`` on the MI355X, on a tiny seeded model (tests/roi_head_ref.py):

  * the fast path equals ``roi_head_ref.simple_test_ref`` — the same public building blocks, then the OLD result tail — bit for bit,
    over ``rescale``, ``mult_2d_score``, ``calib_scoring``, ``cov_correction``, ``flip``, the empty branch and a ``pnp.initialiser='k0'`` head;
  * the fast path against the literal path of the same head, within exactly the bars tests/test_gpu_decode_and_head.py applies between
    ``pose_from_head`` and the literal chain (quoted below with their lines);
  * the detector equals ``roi_head.simple_test(neck(backbone(img)), rpn_head.simple_test_rpn(...), ...)`` bit for bit.

The Monte-Carlo global head draws its masks from torch's generator, which every run seeds alike."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import roi_head_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
MASK_SEED = 1234
# tests/test_gpu_decode_and_head.py, pose_from_head against the literal chain:
T_ABS = 1e-4            # :143  translation within 1e-4
YAW_ABS = 1e-4          # :145  rotation within 1e-4
COV_REL = 1e-4          # :147  calibrated covariance within 1e-4 of its largest entry


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def same_results(a, b):
    assert set(a) == set(b), (sorted(a), sorted(b))
    for key in a:
        assert len(a[key]) == len(b[key]) == rr.NUM_CLASSES, key
        for c, (p, q) in enumerate(zip(a[key], b[key])):
            assert bits_equal(p, q), (key, c, np.shape(p), np.shape(q))


def run(head, fn, inputs, **kw):
    torch.manual_seed(MASK_SEED)
    with torch.no_grad():
        return fn(inputs['x'], inputs['proposal_list'], inputs['img_metas'], coord_2d=inputs['coord_2d'], cam_intrinsic=inputs['cam_intrinsic'], **kw)


def cfg_with(**kw):
    return dict(copy.deepcopy(rr.TEST_CFG['rcnn']), **kw)


VARIANTS = {
    'plain': dict(),
    'rescale': dict(rescale=True),
    'no_mult_2d_score': dict(cfg=dict(mult_2d_score=False)),
    'no_calib_scoring': dict(cfg=dict(calib_scoring=False)),
    'no_cov_correction': dict(cfg=dict(cov_correction=False)),
    'flip': dict(flip=True),
    'debug': dict(cfg=dict(debug=True)),
    'k0': dict(pnp=dict(type='PnPUncert', z_min=0.5, epnp_istd_thres=0.6, inlier_opt_only=True, forward_exact_hessian=False, initialiser='k0')),
    'fc_extractor': dict(mc=False),
}


@pytest.mark.parametrize('name', list(VARIANTS))
def test_fast_path_equals_the_restatement_with_the_old_tail(name):
    v = VARIANTS[name]
    head = rr.build_roi_head(test_cfg=cfg_with(**v.get('cfg', {})), pnp=v.get('pnp'), mc=v.get('mc', True)).to(DEV)
    inputs = rr.image_inputs(DEV, flip=v.get('flip', False))
    got = run(head, head.simple_test, inputs, rescale=v.get('rescale', False))
    assert head.last_path == 'fast'
    (want,), labels = run(head, lambda *a, **k: rr.simple_test_ref(head, *a, **k), inputs, rescale=v.get('rescale', False))
    assert isinstance(got, list) and len(got) == 1
    same_results(got[0], want)
    per_class = [int((labels == c).sum()) for c in range(rr.NUM_CLASSES)]
    kept = [len(b) for b in got[0]['bbox_3d_results']]
    print(f'{name}: detections per class {per_class}, kept after the 3-D NMS {kept}')
    assert sum(k >= 2 for k in per_class) >= 2, per_class                  # at least two detections in at least two classes
    assert all(b.dtype == np.float32 and b.shape[1] == 8 for b in got[0]['bbox_3d_results']) and all(b.shape[1] == 5 for b in got[0]['bbox_results'])
    assert [len(b) for b in got[0]['bbox_results']] == kept and sum(kept) >= 2
    if name == 'debug':
        assert [len(m) for m in got[0]['oc_maps']] == kept and got[0]['oc_maps'][0].shape[1:] == (3, 28, 28) and got[0]['std_maps'][0].shape[1:] == (2, 28, 28)
        assert got[0]['pose_covs'][0].shape[1:] == (4, 4) and got[0]['latent_vecs'][0].shape[1:] == (16,)
    if name == 'rescale':                                                   # the 2-D boxes are in the original image's pixels: twice the testing scale's
        plain = run(head, head.simple_test, inputs)[0]
        assert max(float(b[:, :4].max()) for b in got[0]['bbox_results'] if len(b)) > max(float(b[:, :4].max()) for b in plain['bbox_results'] if len(b))


def test_empty_detection_branch():
    head = rr.build_roi_head(test_cfg=cfg_with(score_thr=2.0, debug=True)).to(DEV)
    inputs = rr.image_inputs(DEV)
    got = run(head, head.simple_test, inputs)[0]
    (want,), _ = run(head, lambda *a, **k: rr.simple_test_ref(head, *a, **k), inputs)
    assert head.last_path == 'empty'
    for key in ('bbox_results', 'bbox_3d_results'):
        assert all(bits_equal(p, q) for p, q in zip(got[key], want[key]))
    assert [b.shape for b in got['bbox_3d_results']] == [(0, 8)] * 3 and [b.shape for b in got['bbox_results']] == [(0, 5)] * 3
    assert got['oc_maps'][0].shape == (0, 3, 0, 0) and got['std_maps'][0].shape == (0, 2, 0, 0) and got['pose_covs'][0].shape == (0, 4, 4)
    assert got['latent_vecs'][0].shape == (0, 16) and len(got['oc_maps']) == 3


def test_forced_paths():
    head = rr.build_roi_head().to(DEV)
    inputs = rr.image_inputs(DEV)
    run(head, head.simple_test, inputs, path='literal')
    assert head.last_path == 'literal'
    head.projection_head.train_std_of_encoded_error = False
    run(head, head.simple_test, inputs)
    assert head.last_path == 'literal'                                      # the switch is not silent: the path is recorded and the reason named
    with pytest.raises(RuntimeError, match='train_std_of_encoded_error'):
        run(head, head.simple_test, inputs, path='fast')


def test_fast_path_against_the_literal_path():
    """The two paths of one head on one image, with the debug maps.  The 2-D stage is shared, so the detections are the same rows; the
    poses agree within the bars quoted above.  Each figure is printed before it is judged.  The NOC head's output is the canned,
    geometrically consistent one of roi_head_ref.with_canned_noc_head: the bars are stated for well-posed problems, and a random
    trunk's are not (measured on this model with its random trunk: translation 1.5e-1, yaw 3.4e-2 on objects whose posterior deviation
    is metres to kilometres, 2e-6 and below on the others; the maps the two paths hand the solver differ by 6e-7 in the weights only)."""
    head = rr.build_roi_head(test_cfg=cfg_with(debug=True, nms_3d_thr=1.0)).to(DEV)      # thr 1: the NMS drops nothing, every detection is compared
    inputs = rr.image_inputs(DEV)
    rr.with_canned_noc_head(head, inputs, MASK_SEED)
    fast = run(head, head.simple_test, inputs, path='fast')[0]
    lit = run(head, head.simple_test, inputs, path='literal')[0]
    worst = dict(t=0.0, yaw=0.0, cov=0.0)
    for c in range(rr.NUM_CLASSES):
        f2, l2 = fast['bbox_results'][c], lit['bbox_results'][c]
        assert f2.shape == l2.shape, (c, f2.shape, l2.shape)
        # pair the rows by their 2-D box (unique per detection), whatever order the 3-D scores put them in
        fo, lo = np.lexsort(f2.T), np.lexsort(l2.T)
        assert bits_equal(f2[fo], l2[lo]), c
        f3, l3 = fast['bbox_3d_results'][c][fo], lit['bbox_3d_results'][c][lo]
        fc, lc = fast['pose_covs'][c][fo], lit['pose_covs'][c][lo]
        ok = (f3[:, 7] > 0) & (l3[:, 7] > 0)                                 # solved in both (score 0 marks a failed solve)
        assert np.array_equal(f3[:, 7] > 0, l3[:, 7] > 0), c
        if ok.any():
            worst['t'] = max(worst['t'], float(np.abs(f3[ok, 3:6] - l3[ok, 3:6]).max()))
            worst['yaw'] = max(worst['yaw'], float(np.abs(np.angle(np.exp(1j * (f3[ok, 6] - l3[ok, 6])))).max()))
            worst['cov'] = max(worst['cov'], float((np.abs(fc - lc)[ok] / np.abs(lc)[ok].max((1, 2), keepdims=True)).max()))
    solved = sum(int((b[:, 7] > 0).sum()) for b in fast['bbox_3d_results'])
    total = sum(len(b) for b in fast['bbox_3d_results'])
    print(f'fast against literal: {solved} of {total} detections solved')
    assert solved >= 2 and 2 * solved >= total
    print(f'fast against literal: translation {worst["t"]:.3e} (bar {T_ABS}), yaw {worst["yaw"]:.3e} (bar {YAW_ABS}), '
          f'calibrated covariance {worst["cov"]:.3e} of its largest entry (bar {COV_REL})')
    assert worst['t'] <= T_ABS and worst['yaw'] <= YAW_ABS and worst['cov'] <= COV_REL, worst


def test_detector_equals_its_parts():
    det = rr.build_detector().to(DEV)
    inputs = rr.image_inputs(DEV)
    img = torch.randn(1, 3, rr.IMG_H, rr.IMG_W, generator=torch.Generator().manual_seed(7)).to(DEV)
    kw = dict(coord_2d=inputs['coord_2d'], cam_intrinsic=inputs['cam_intrinsic'])
    with torch.no_grad():
        torch.manual_seed(MASK_SEED)
        got = det.simple_test(img, inputs['img_metas'], **kw)
        torch.manual_seed(MASK_SEED)
        x = det.neck(det.backbone(img))
        want = det.roi_head.simple_test(x, det.rpn_head.simple_test_rpn(x, inputs['img_metas']), inputs['img_metas'], **kw)
        torch.manual_seed(MASK_SEED)
        through = det(img=[img], img_metas=[inputs['img_metas']], return_loss=False, **kw)
    same_results(got[0], want[0])
    same_results(through[0], want[0])
    assert det.roi_head.last_path == 'fast' and sum(len(b) for b in got[0]['bbox_3d_results']) >= 2
