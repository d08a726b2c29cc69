"""The aligned 3-D IoU kernel (``mr_bbox3d_overlaps_aligned``) and the pose head's training interface on the MI355X:
the kernel against fixture G14 and against the fp32 composition restatement (tests/iou3d_ref.py) applied to its own BEV areas, edge
cases, ``loss()`` against the reference's loss, and one full training step of the pose head."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iou3d_ref  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g14_pose_loss.npz')


def _dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def g14():
    return dict(np.load(GOLDEN))


def _random_pairs(n, seed):
    rng = np.random.default_rng(seed)
    b = np.stack([rng.uniform(-10, 10, n), rng.uniform(0.5, 2.5, n), rng.uniform(5, 50, n), rng.uniform(3.0, 4.8, n),
                  rng.uniform(1.3, 1.9, n), rng.uniform(1.4, 1.9, n), rng.uniform(-np.pi, np.pi, n)], 1).astype(np.float32)
    q = (b + np.concatenate([rng.normal(0, 0.8, (n, 3)), rng.normal(0, 0.3, (n, 3)), rng.normal(0, 0.4, (n, 1))], 1)).astype(np.float32)
    q[:, 3:6] = np.abs(q[:, 3:6])
    return b, q


def test_kernel_against_g14(g14):
    from monorun_amd.iou3d import bbox3d_overlaps_aligned
    b, q, crit, zc, co, raises = (g14[k] for k in ('boxes', 'qboxes', 'criterion', 'z_center', 'coincident', 'ref_raises'))
    tb, tq = torch.from_numpy(b).to(_dev()), torch.from_numpy(q).to(_dev())
    area = np.maximum(1.0, np.minimum(b[:, 3] * b[:, 5], q[:, 3] * q[:, 5]))
    checked = 0
    for c in (-1, 0, 1, 2):
        for z in (1.0, 0.5):
            sel = np.nonzero((crit == c) & (zc == z))[0]
            for rule, key in (('reference', 'iou_torch'), ('geometric', 'iou_numpy')):
                iou, rinc = bbox3d_overlaps_aligned(tb[sel], tq[sel], criterion=c, z_center=z, height_rule=rule, return_rinc=True)
                iou, rinc = iou.cpu().numpy()[:, 0], rinc.cpu().numpy()
                assert iou.dtype == np.float32 and iou.shape == (len(sel),)
                # BEV stage against the numba device function, away from coincident edges (identical boxes: the geometric area)
                far = ~co[sel]
                assert (np.abs(rinc - g14['rinc'][sel]) / area[sel])[far].max() < 2e-5
                np.testing.assert_allclose(rinc[~far], (b[:, 3] * b[:, 5])[sel][~far], rtol=1e-6)
                # the composition: bit-exact against the fp32 restatement fed the kernel's own BEV areas
                want = iou3d_ref.compose(b[sel], q[sel], rinc, c, z, rule=rule)
                assert np.array_equal(iou, want), (c, z, rule, np.abs(iou - want).max())
                # the final IoU against the reference's (criterion 2 raises in the reference)
                ok = far & ~raises[sel]
                if ok.any():
                    assert np.abs(iou - g14[key][sel])[ok].max() < 2e-5, (c, z, rule)
                    checked += int(ok.sum())
    assert checked == 2 * 6 * 36


def test_edge_cases():
    from monorun_amd.iou3d import bbox3d_overlaps_aligned, bbox3d_overlaps_aligned_torch
    dev = _dev()
    e = torch.zeros(0, 7, device=dev)
    out = bbox3d_overlaps_aligned(e, e)
    assert out.shape == (0, 1) and out.device.type == 'cuda'
    b, q = _random_pairs(100000, 7)
    tb, tq = torch.from_numpy(b).to(dev), torch.from_numpy(q).to(dev)
    iou, rinc = bbox3d_overlaps_aligned(tb, tq, return_rinc=True)
    assert iou.shape == (100000, 1)
    iou_np, rinc_np = iou.cpu().numpy()[:, 0], rinc.cpu().numpy()
    assert np.array_equal(iou_np, iou3d_ref.compose(b, q, rinc_np, -1, 1.0))
    assert (iou_np > 0).mean() > 0.5 and ((iou_np >= 0) & (iou_np <= 1)).all()
    # the last block of more than one: its pairs against the oracle's intersection
    from oracle import kitti_eval as ke
    bev = [0, 2, 3, 5, 6]
    for i in (0, 1, 255, 256, 99999):
        ref = ke.rotated_overlap(b[i, bev], q[i, bev], 2)
        assert abs(rinc_np[i] - ref) <= 2e-5 * max(1.0, ref)
    # N = 1
    one = bbox3d_overlaps_aligned(tb[99999:], tq[99999:])
    assert one.shape == (1, 1) and one.item() == iou_np[99999]
    # two calls are bit-identical
    assert torch.equal(bbox3d_overlaps_aligned(tb, tq), iou)
    # strided rows: the permuted view of the training layout, and rows of a wider tensor, read in place
    lhw = torch.cat([tb[:, 3:6], tb[:, 0:3], tb[:, 6:7]], 1)
    wide = torch.cat([tb, torch.full((100000, 3), 7.0, device=dev)], 1)[:, :7]
    assert wide.stride() == (10, 1)
    assert torch.equal(bbox3d_overlaps_aligned(lhw[:, [3, 4, 5, 0, 1, 2, 6]], tq), iou)
    assert torch.equal(bbox3d_overlaps_aligned(wide, tq), iou)
    assert torch.equal(bbox3d_overlaps_aligned(tb, torch.cat([tq, tq], 1)[:, 7:]), iou)
    # host inputs are staged through the GPU; the result comes back to the host; other float dtypes are computed in fp32
    host = bbox3d_overlaps_aligned(torch.from_numpy(b[:1000]), torch.from_numpy(q[:1000]))
    assert host.device.type == 'cpu' and torch.equal(host, iou[:1000].cpu())
    assert torch.equal(bbox3d_overlaps_aligned(tb[:1000].double(), tq[:1000].double()), iou[:1000])
    # the reference's symbol returns (N,)
    assert torch.equal(bbox3d_overlaps_aligned_torch(tb[:10], tq[:10]), iou[:10, 0])
    # other z axes: the same boxes with the height axis moved
    for z in (0, 2):
        perm = {0: [1, 0, 2, 4, 3, 5, 6], 2: [0, 2, 1, 3, 5, 4, 6]}[z]
        iz, rz = bbox3d_overlaps_aligned(tb[:, perm], tq[:, perm], z_axis=z, z_center=0.5, return_rinc=True)
        assert torch.equal(rz, rinc)
        assert np.array_equal(iz.cpu().numpy()[:, 0], iou3d_ref.compose(b[:, perm], q[:, perm], rinc_np, -1, 0.5, z_axis=z))


def _fixture_loss_inputs(g14, dev):
    T = lambda k: torch.from_numpy(np.ascontiguousarray(g14[k])).to(dev)
    return (T('loss_ret_val'), T('loss_yaw_pred'), T('loss_t_vec_pred'), T('loss_pose_cov'), T('loss_dims_pred'), T('loss_pos_bboxes_3d'))


def test_loss_against_the_reference(g14):
    from monorun_amd.pose_head import UncertPropPnPOptimizer
    dev = _dev()
    ret, yaw, t, cov, dims, gt = _fixture_loss_inputs(g14, dev)
    cov = cov.clone().requires_grad_(True)
    head = UncertPropPnPOptimizer(loss_calib=dict(type='KLLossMV', loss_weight=0.01)).to(dev)
    yt, tt = head.get_targets(gt)
    loss, ious = head.loss(ret, yaw, t, cov, dims, yt, tt, gt)
    assert ious.shape == (24, 1) and ious.device.type == 'cuda' and not ious.requires_grad
    assert (ious[~ret] == 0).all() and (ious[ret] > 0).all()
    np.testing.assert_allclose(ious.cpu().numpy(), g14['loss_ious'], rtol=0, atol=2e-5)
    assert abs(loss['mean_iou'].item() - float(g14['loss_mean_iou'])) < 2e-5
    assert abs(loss['loss_calib'].item() - float(g14['loss_calib'])) <= 1e-5 * max(1.0, abs(float(g14['loss_calib'])))
    loss['loss_calib'].backward()
    np.testing.assert_allclose(cov.grad.cpu().numpy(), g14['loss_calib_grad_pose_cov'], rtol=1e-4, atol=1e-6)
    # no valid object: zero losses that still carry a graph
    cov2 = cov.detach().clone().requires_grad_(True)
    loss0, ious0 = head.loss(torch.zeros_like(ret), yaw, t, cov2, dims, yt, tt, gt)
    assert (ious0 == 0).all() and loss0['mean_iou'].item() == 0 and loss0['loss_calib'].item() == 0
    loss0['loss_calib'].backward()
    assert (cov2.grad == 0).all()
    # no object at all
    e = gt[:0]
    loss_e, ious_e = head.loss(ret[:0], yaw[:0], t[:0], cov[:0].detach(), dims[:0], e[:, 6:7], e[:, 3:6], e)
    assert ious_e.shape == (0, 1) and loss_e['mean_iou'].item() == 0 and loss_e['loss_calib'].item() == 0


class _Recorder(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.calls = []

    def forward(self, pred, target, **kw):
        self.calls.append((pred, target, kw))
        return (pred if isinstance(target, int) else pred - target).abs().mean()


def test_full_training_step_on_the_gpu():
    from monorun_amd import synthetic as syn
    from monorun_amd.losses import KLLossMV
    from monorun_amd.pose_head import UncertPropPnPOptimizer
    B = 64
    b = syn.make_batch(B=B, seed=31)
    dev = _dev()
    c2d, ls, c3d = (torch.from_numpy(b[k]).to(dev) for k in ('coords_2d', 'logstd', 'coords_3d'))
    K = torch.from_numpy(np.asarray(b['K'], np.float32)).to(dev)
    img = torch.from_numpy(np.asarray(b['img_shape'], np.float32)).to(dev)
    gt = torch.from_numpy(np.concatenate([b['dims'], b['gt_t'], b['gt_yaw'][:, None]], 1).astype(np.float32)).to(dev)
    dims = gt[:, :3]
    cfg = dict(type='PnPUncert', z_min=0.5, epnp_istd_thres=0.6, inlier_opt_only=True, forward_exact_hessian=False, differentiable=True)
    head = UncertPropPnPOptimizer(pnp=cfg, loss_calib=dict(type='KLLossMV', loss_weight=0.01)).to(dev)
    head.loss_rot, head.loss_trans = _Recorder(), _Recorder()
    leaves = [a.clone().requires_grad_(True) for a in (c2d, ls, c3d)]
    ret, yaw, t, cov, cov_calib = head(*leaves, K, img)
    yt, tt = head.get_targets(gt)
    loss, ious = head.loss(ret, yaw, t, cov_calib, dims, yt, tt, gt)
    assert set(loss) == {'mean_iou', 'loss_rot', 'loss_trans', 'loss_calib'}
    v = ret.bool()
    assert int(v.sum()) >= B // 2
    assert ((ious >= 0) & (ious <= 1)).all() and (ious[~v] == 0).all()
    assert float(ious[v].median()) > 0.5 and float(loss['mean_iou']) > 0.4
    # the reference's arguments: loss_rot(|| (cos, sin) difference ||, -1), loss_trans(t_vec, trans_targets)
    (p_rot, t_rot, kw_rot), = head.loss_rot.calls
    want = torch.norm(torch.cat([torch.cos(yaw[v]), torch.sin(yaw[v])], 1) - torch.cat([torch.cos(yt[v]), torch.sin(yt[v])], 1),
                      dim=1, p=2, keepdim=True)
    assert t_rot == -1 and kw_rot == {} and p_rot.shape == (int(v.sum()), 1) and torch.equal(p_rot, want)
    (p_tr, t_tr, kw_tr), = head.loss_trans.calls
    assert kw_tr == {} and torch.equal(p_tr, t[v]) and torch.equal(t_tr, tt[v])
    total = loss['loss_rot'] + loss['loss_trans'] + loss['loss_calib']
    total.backward()
    for g in [x.grad for x in leaves] + [head.cov_calib_logscale.grad]:
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    # LossUpdaterHook replaces loss_calib after construction: the new module is the one used
    head.loss_calib = KLLossMV(loss_weight=0.02)
    with torch.no_grad():
        out2 = head(*[x.detach() for x in leaves], K, img)
    assert all(torch.equal(x, y) for x, y in zip(out2, (ret, yaw, t, cov, cov_calib)))
    loss2, _ = head.loss(out2[0], out2[1], out2[2], out2[4], dims, yt, tt, gt)
    assert abs(loss2['loss_calib'].item() - 2 * loss['loss_calib'].item()) <= 1e-6 * abs(loss['loss_calib'].item())
    print(f"training step: {int(v.sum())}/{B} valid, median IoU {float(ious[v].median()):.3f}, mean_iou {float(loss['mean_iou']):.3f}, "
          f"loss_calib {loss['loss_calib'].item():.4f}")
