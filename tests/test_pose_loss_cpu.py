"""CPU side of the pose head's training interface: fixture G14 against the evaluator oracle's rotated intersection and
a numpy restatement of the 3-D composition, both height rules, ``losses.KLLossMV`` and ``UncertPropPnPOptimizer.loss`` against the
reference's own loss, the head's construction and ``state_dict``, and the C entry point's argument checks.  No GPU needed: where
``loss()`` needs the 3-D IoU, the kernel is replaced by the same restatement."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iou3d_ref  # noqa: E402
from oracle import kitti_eval as ke  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g14_pose_loss.npz')
BEV = [0, 2, 3, 5, 6]                   # z_axis = 1


@pytest.fixture(scope='module')
def g14():
    return dict(np.load(GOLDEN))


def oracle_rinc(boxes, qboxes):
    return np.array([ke.rotated_overlap(boxes[i, BEV], qboxes[i, BEV], 2) for i in range(len(boxes))], np.float32)


def test_g14_rinc_matches_the_oracle_intersection(g14):
    b, q, rinc, co = g14['boxes'], g14['qboxes'], g14['rinc'], g14['coincident']
    mine = oracle_rinc(b, q)
    area = np.maximum(1.0, np.minimum(b[:, 3] * b[:, 5], q[:, 3] * q[:, 5]))
    assert co.sum() == 32 and (rinc[~co] > 0).sum() > 200 and (rinc[~co] == 0).sum() >= 32
    err = np.abs(mine - rinc) / area
    assert err[~co].max() < 2e-5, err[~co].max()
    # identical boxes: the oracle gives the box's area, the numba intersection is degenerate on coincident edges
    np.testing.assert_allclose(mine[co], (b[:, 3] * b[:, 5])[co], rtol=1e-6)


def test_composition_restatement_reproduces_both_reference_rules(g14):
    b, q, rinc, crit, zc, raises = (g14[k] for k in ('boxes', 'qboxes', 'rinc', 'criterion', 'z_center', 'ref_raises'))
    ok = ~raises
    assert set(crit[ok]) == {-1, 0, 1} and set(crit[raises]) == {2} and set(zc) == {1.0, 0.5}
    torch_rule = iou3d_ref.compose(b, q, rinc, crit, zc, rule='reference')
    numpy_rule = iou3d_ref.compose(b, q, rinc, crit, zc, rule='geometric')
    assert np.array_equal(torch_rule[ok], g14['iou_torch'][ok])
    assert np.array_equal(numpy_rule[ok], g14['iou_numpy'][ok])
    # the rules differ on the vertically offset pairs (slots 14..25 of every group of 40), in both directions
    slot = np.arange(len(b)) % 40
    off = ok & (slot >= 14) & (slot < 26) & (rinc > 0)
    assert (torch_rule[off] != numpy_rule[off]).all()
    assert (torch_rule[off] > numpy_rule[off]).all()          # the torch rule ignores part of the vertical misalignment
    # touching boxes (slots 26, 27): no geometric overlap, up to the rounding of the fp32 box edges
    touch = (slot >= 26) & (slot < 28)
    assert numpy_rule[touch].max() < 1e-5 and (numpy_rule[touch] == 0).sum() >= 8
    # criterion 2 (the reference raises there): the intersection volume, clamped to [0, 1]
    assert ((torch_rule[raises] >= 0) & (torch_rule[raises] <= 1)).all() and (torch_rule[raises] > 0).sum() > 20


def _fixture_loss_inputs(g14):
    T = lambda k: torch.from_numpy(np.ascontiguousarray(g14[k]))
    return (T('loss_ret_val'), T('loss_yaw_pred'), T('loss_t_vec_pred'), T('loss_pose_cov'), T('loss_dims_pred'), T('loss_pos_bboxes_3d'))


def test_kl_loss_mv_matches_the_reference_loss_and_gradient(g14):
    from monorun_amd.losses import KLLossMV
    ret, yaw, t, cov, _, gt = _fixture_loss_inputs(g14)
    cov = cov.clone().requires_grad_(True)
    v = ret
    yd = ((yaw[v] - gt[v, 6:7]) + np.pi) % (2 * np.pi) - np.pi
    d = torch.cat([yd, t[v] - gt[v, 3:6]], 1)
    c = cov[v]
    loss = KLLossMV(loss_weight=0.01)(d, 0, inv_cov=torch.inverse(c + torch.eye(4)))
    loss.backward()
    assert abs(loss.item() - float(g14['loss_calib'])) <= 1e-6 * max(1.0, abs(float(g14['loss_calib'])))
    np.testing.assert_allclose(cov.grad.numpy(), g14['loss_calib_grad_pose_cov'], rtol=0, atol=1e-6)
    assert (cov.grad[~ret] == 0).all() and (cov.grad[ret] != 0).any()


def test_kl_loss_mv_reductions_and_non_finite_logdet():
    from monorun_amd.losses import KLLossMV, kl_loss_mv
    g = torch.Generator().manual_seed(3)
    a = torch.randn(5, 4, 4, generator=g, dtype=torch.float64)
    inv = a @ a.transpose(1, 2) + torch.eye(4, dtype=torch.float64)
    inv[2] = torch.zeros(4, 4)                                          # logdet = -inf -> 0
    d = torch.randn(5, 4, generator=g, dtype=torch.float64)
    el = kl_loss_mv(d, 0, inv)
    assert el.shape == (5, 1) and el[2, 0] == 0
    want = 0.5 * (torch.einsum('bi,bij,bj->b', d, inv, d) - torch.logdet(inv))
    keep = torch.arange(5) != 2
    torch.testing.assert_close(el[keep, 0], want[keep])
    torch.testing.assert_close(kl_loss_mv(d + 1, torch.ones(5, 4, dtype=torch.float64), inv), el)
    w = torch.rand(5, 1, generator=g, dtype=torch.float64)
    m = KLLossMV(loss_weight=0.5)
    torch.testing.assert_close(m(d, 0, inv_cov=inv), 0.5 * el.mean())
    torch.testing.assert_close(m(d, 0, inv_cov=inv, reduction_override='sum'), 0.5 * el.sum())
    torch.testing.assert_close(m(d, 0, inv_cov=inv, reduction_override='none'), 0.5 * el)
    torch.testing.assert_close(m(d, 0, inv_cov=inv, weight=w, avg_factor=3.0), 0.5 * (el * w).sum() / 3.0)
    with pytest.raises(ValueError):
        m(d, 0, inv_cov=inv, avg_factor=3.0, reduction_override='sum')


def _cpu_iou(boxes, qboxes, criterion=-1, z_axis=1, z_center=1.0, height_rule='reference'):
    b, q = boxes.detach().numpy(), qboxes.detach().numpy()
    iou = iou3d_ref.compose(b, q, oracle_rinc(b, q), criterion, z_center, z_axis, height_rule)
    return torch.from_numpy(iou)[:, None]


def test_head_loss_matches_the_reference_loss(g14, monkeypatch):
    from monorun_amd import pose_head
    monkeypatch.setattr(pose_head, 'bbox3d_overlaps_aligned', _cpu_iou)
    ret, yaw, t, cov, dims, gt = _fixture_loss_inputs(g14)
    cov = cov.clone().requires_grad_(True)
    head = pose_head.UncertPropPnPOptimizer(loss_calib=dict(type='KLLossMV', loss_weight=0.01))
    yt, tt = head.get_targets(gt)
    assert torch.equal(yt, gt[:, 6:7]) and torch.equal(tt, gt[:, 3:6])
    loss, ious = head.loss(ret, yaw, t, cov, dims, yt, tt, gt)
    assert set(loss) == {'mean_iou', 'loss_calib'} and ious.shape == (24, 1) and not ious.requires_grad
    assert (ious[~ret] == 0).all()
    np.testing.assert_allclose(ious.numpy(), g14['loss_ious'], rtol=0, atol=2e-5)
    assert abs(loss['mean_iou'].item() - float(g14['loss_mean_iou'])) < 2e-5
    assert abs(loss['loss_calib'].item() - float(g14['loss_calib'])) <= 1e-6
    loss['loss_calib'].backward()
    np.testing.assert_allclose(cov.grad.numpy(), g14['loss_calib_grad_pose_cov'], rtol=0, atol=1e-6)


def test_head_loss_with_no_valid_object_and_unknown_loss_types(monkeypatch):
    from monorun_amd import pose_head
    monkeypatch.setattr(pose_head, 'bbox3d_overlaps_aligned', _cpu_iou)
    head = pose_head.UncertPropPnPOptimizer(loss_rot=dict(type='NoSuchLoss'), loss_trans=dict(type='NoSuchLoss'),
                                            loss_calib=dict(type='KLLossMV', loss_weight=0.01))
    n = 3
    gt = torch.tensor([[3.9, 1.5, 1.6, 1.0, 1.6, 20.0, 0.3]]).repeat(n, 1)
    yaw = torch.full((n, 1), 0.2, requires_grad=True)
    t = gt[:, 3:6].clone().requires_grad_(True)
    cov = (torch.eye(4) * 0.1).repeat(n, 1, 1).requires_grad_(True)
    loss, ious = head.loss(torch.zeros(n, dtype=torch.bool), yaw, t, cov, gt[:, :3], gt[:, 6:7], gt[:, 3:6], gt)
    assert (ious == 0).all() and loss['mean_iou'] == 0
    for k in ('loss_rot', 'loss_trans', 'loss_calib'):
        assert loss[k].item() == 0 and loss[k].requires_grad
    sum(loss[k] for k in ('loss_rot', 'loss_trans', 'loss_calib')).backward()
    assert (cov.grad == 0).all() and (t.grad == 0).all()
    with pytest.raises(RuntimeError, match='NoSuchLoss'):
        head.loss(torch.ones(n, dtype=torch.bool), yaw, t, cov, gt[:, :3], gt[:, 6:7], gt[:, 3:6], gt)


def test_head_construction_and_state_dict_unchanged():
    from monorun_amd.losses import KLLossMV, UnbuiltLoss
    from monorun_amd.pose_head import UncertPropPnPOptimizer
    try:
        import mmdet  # noqa: F401
        has_mmdet = True
    except ImportError:
        has_mmdet = False
    plain = UncertPropPnPOptimizer()
    assert plain.loss_rot is None and plain.loss_trans is None and plain.loss_calib is None
    assert list(plain.state_dict().keys()) == ['cov_calib_logscale']
    head = UncertPropPnPOptimizer(loss_calib=dict(type='KLLossMV', loss_weight=0.01), loss_rot=dict(type='SmoothL1Loss'))
    assert list(head.state_dict().keys()) == ['cov_calib_logscale']
    head.load_state_dict(plain.state_dict())
    if not has_mmdet:
        assert isinstance(head.loss_calib, KLLossMV) and head.loss_calib.loss_weight == 0.01
        assert isinstance(head.loss_rot, UnbuiltLoss)
    # LossUpdaterHook: rsetattr(model, 'roi_head.pose_head.loss_calib', build_loss(cfg))
    plain.loss_calib = KLLossMV(loss_weight=0.02)
    assert plain.loss_calib.loss_weight == 0.02 and list(plain.state_dict().keys()) == ['cov_calib_logscale']


def test_iou_op_argument_checks_and_exported_symbol():
    from monorun_amd import _lib
    from monorun_amd.iou3d import bbox3d_overlaps_aligned
    assert 'mr_bbox3d_overlaps_aligned' in _lib.exported_symbols('pnp')
    lib = _lib.load()
    f = lib.mr_bbox3d_overlaps_aligned
    args = lambda n=4, stride=7, crit=-1, z=1, flags=0: (None, stride, None, 7, n, crit, z, 1.0, flags, None, None, None)
    assert f(*args(n=0)) == 0
    for bad in (dict(n=-1), dict(crit=3), dict(crit=-2), dict(z=3), dict(z=-1), dict(stride=6), dict(flags=2), dict()):
        assert f(*args(**bad)) == -1, bad                       # dict(): n = 4 with NULL pointers
    x = torch.zeros(2, 7)
    for kw in (dict(criterion=5), dict(z_axis=3), dict(height_rule='max')):
        with pytest.raises(ValueError):
            bbox3d_overlaps_aligned(x, x, **kw)
    with pytest.raises(ValueError):
        bbox3d_overlaps_aligned(x, torch.zeros(3, 7))
