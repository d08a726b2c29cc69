"""The NOC head's training kernels on the MI355X: the projection bit for bit against tests/projection_ref.py and to
the reference's values (G15), the two-launch loss and its buffer, the gradients against G15 and an fp64 autograd of the reference
formula, torch's rules at ties, NaN, shapes and dtypes, determinism, the HIP path against the torch restatement, and one training
step of the NOC head through the differentiable PnP."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import projection_ref  # noqa: E402
from oracle import oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g15_projection_loss.npz')
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def g15():
    return dict(np.load(GOLDEN))


def _group(g, k, h, w, dev=DEV):
    T = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).to(dev)
    return dict(c3d=T(g[k + '_coords_3d']), ls=T(g[k + '_proj_logstd']), pose=T(g[k + '_pose']), K=T(g[k + '_cam_intrinsic']),
                img=T(g[k + '_img_shapes']), roi=T(orc.roi_grid(g[k + '_rois'], h, w)), dist=T(g[k + '_distances']))


def _random_group(n, h, w, seed, dev=DEV):
    rng = np.random.default_rng(seed)
    t = np.stack([rng.uniform(-12, 12, n), rng.uniform(1, 2, n), rng.uniform(3, 45, n)], 1)
    pose = np.concatenate([t, rng.uniform(-np.pi, np.pi, (n, 1))], 1).astype(np.float32)
    K = np.tile(np.array([[721.5, 0, 609.6], [0, 721.5, 172.9], [0, 0, 1]], np.float32), (n, 1, 1))
    img = np.tile(np.array([[375.0, 1242.0]], np.float32), (n, 1))
    c3d = rng.normal(0, 1.0, (n, 3, h, w)).astype(np.float32)
    c3d[:, 2] -= np.float32(0.5) * t[:, 2, None, None].astype(np.float32) * (rng.random((n, 1, 1)) < 0.1)   # some points behind z_min
    ls = rng.normal(-0.2, 1.0, (n, 2, h, w)).astype(np.float32)
    ls[rng.random((n, 2, h, w)) < 0.005] = -10.0
    proj = projection_ref.project(c3d, pose, K, img)
    noise = rng.normal(0, 8, proj.shape)
    noise += np.where(noise < 0, -0.05, 0.05)           # |proj - roi| >= 0.05 px: away from the kink of |x|, where fp32 and fp64 may disagree
    roi = (proj + noise).astype(np.float32)
    dist = np.linalg.norm(t, axis=1, keepdims=True).astype(np.float32)
    T = lambda a: torch.from_numpy(a).to(dev)
    return dict(c3d=T(c3d), ls=T(ls), pose=T(pose), K=T(K), img=T(img), roi=T(roi), dist=T(dist))


def _step(head, d, grads=True, c3d=None, ls=None):
    c3d = (d['c3d'] if c3d is None else c3d).detach().clone().requires_grad_(grads)
    ls = (d['ls'] if ls is None else ls).detach().clone().requires_grad_(grads)
    proj = head(c3d, d['pose'], d['K'], d['img'])
    loss = head.loss(proj, ls, d['roi'], d['dist'])['loss_proj']
    if grads:
        loss.backward()
    return proj.detach(), loss.detach(), (c3d.grad, ls.grad)


def _grad_ok(mine, ref):
    mine, ref = np.asarray(mine, np.float64), np.asarray(ref, np.float64)
    assert mine.shape == ref.shape
    err, scale = np.abs(mine - ref).max(), np.abs(ref).max()
    assert err <= 1e-4 * scale, (err, scale)


def _head():
    from monorun_amd.projection_head import UncertProjectionHead
    return UncertProjectionHead().to(DEV)


def test_projection_is_bitwise_the_fp32_restatement_and_matches_g15(g15):
    head = _head()
    for k, h, w in (('A', 28, 28), ('B', 7, 9)):
        d = _group(g15, k, h, w)
        with torch.no_grad():
            out = head(d['c3d'], d['pose'], d['K'], d['img']).cpu().numpy()
        want = projection_ref.project(g15[k + '_coords_3d'].astype(np.float32), g15[k + '_pose'], g15[k + '_cam_intrinsic'], g15[k + '_img_shapes'])
        assert np.array_equal(out, want), (k, np.abs(out - want).max())
        ref = g15[k + '_coords_2d_proj']
        assert (np.abs(out - ref) / np.maximum(np.abs(ref), 1000)).max() <= 1e-6


def _loss_tol(raw, c, loss_weight=1.0):
    return 1e-5 * float(np.abs(raw).astype(np.float64).sum() / raw.size) * loss_weight / float(c)


def test_loss_buffer_and_gradients_against_g15(g15):
    head = _head()
    A, B = _group(g15, 'A', 28, 28), _group(g15, 'B', 7, 9)
    results = []
    for d, grads in ((A, True), (B, True), (A, False)):
        before = float(head.loss_proj.mean_inv_std)
        proj, loss, g = _step(head, d, grads)
        err = ((proj - d['roi']) * (d['dist'][..., None, None] / head.proj_error_coder.scaling_denomitor)).cpu().numpy()
        want, buf, c, raw = projection_ref.robust_kl(err, d['ls'].cpu().numpy(), before)
        results.append((loss, float(head.loss_proj.mean_inv_std), g, raw, c))
        assert abs(float(loss) - float(want)) <= _loss_tol(raw, c)
        assert abs(float(head.loss_proj.mean_inv_std) - float(buf)) <= 1e-6 * abs(float(buf))
    for i, (loss, buf, _, raw, c) in enumerate(results):
        assert abs(float(loss) - float(g15['train_losses'][i])) <= _loss_tol(raw, c)
        assert abs(buf - float(g15['train_buffers'][i])) <= 1e-6 * float(g15['train_buffers'][i])
    for (_, _, (gc, gl), _, _), k in zip(results[:2], 'AB'):
        _grad_ok(gc.cpu().numpy(), g15[k + '_grad_coords_3d'])
        _grad_ok(gl.cpu().numpy(), g15[k + '_grad_proj_logstd'])
    head.eval()
    b = head.loss_proj.mean_inv_std.clone()
    _, le, _ = _step(head, A, grads=False)
    assert torch.equal(head.loss_proj.mean_inv_std, b)
    assert abs(float(le) - float(g15['eval_loss'])) <= _loss_tol(results[2][3], results[2][4])


def _fp64_reference(d, buf, momentum=0.1, z_min=0.5, border=200, sd=1.6 * 722 * 0.15, delta=1.414, eps=1e-4):
    """the reference's formulas in fp64 torch autograd on the CPU"""
    c3d = d['c3d'].double().cpu().requires_grad_(True)
    ls = d['ls'].double().cpu().requires_grad_(True)
    pose, K, img = d['pose'].double().cpu(), d['K'].double().cpu(), d['img'].double().cpu()
    n, _, h, w = c3d.shape
    s, c = torch.sin(pose[:, 3]), torch.cos(pose[:, 3])
    R = torch.zeros(n, 3, 3, dtype=torch.float64)
    R[:, 0, 0], R[:, 0, 2], R[:, 1, 1], R[:, 2, 0], R[:, 2, 2] = c, s, 1, -s, c
    proj = ((K @ R) @ c3d.reshape(n, 3, -1) + K @ pose[:, :3, None]).reshape(n, 3, h, w)
    uv = (proj[:, :2] / proj[:, 2:].clamp(min=z_min)).clamp(min=-border)
    uv = torch.min(uv, img[:, [1, 0], None, None] + border)
    err = (uv - d['roi'].double().cpu()) * (d['dist'].double().cpu()[..., None, None] / sd)
    inv = torch.exp(-ls).clamp(max=1 / eps)
    dw = err.abs() * inv
    el = torch.where(dw < delta, 0.5 * dw ** 2, delta * (dw - 0.5 * delta)) + ls
    m = buf * (1 - momentum) + momentum * float(inv.detach().mean())
    loss = el.mean() / max(m, 1e-6)
    loss.backward()
    return c3d.grad.numpy(), ls.grad.numpy()


def test_gradients_against_fp64_autograd_at_fresh_inputs():
    head = _head()
    for n, h, w, seed in ((384, 28, 28, 1), (5, 7, 9, 2), (16, 56, 56, 3)):
        d = _random_group(n, h, w, seed)
        before = float(head.loss_proj.mean_inv_std)
        _, _, (gc, gl) = _step(head, d)
        rc, rl = _fp64_reference(d, before)
        _grad_ok(gc.cpu().numpy(), rc)
        _grad_ok(gl.cpu().numpy(), rl)


def test_hip_path_against_the_torch_restatement_on_the_gpu():
    from monorun_amd.projection_head import UncertProjectionHead, uncert_projection
    from monorun_amd.losses import robust_kl_loss
    d = _random_group(384, 28, 28, 11)
    head = _head()
    proj, loss, (gc, gl) = _step(head, d)
    # torch: the same formulas as autograd ops on the same GPU tensors
    c3d = d['c3d'].clone().requires_grad_(True)
    ls = d['ls'].clone().requires_grad_(True)
    tp = uncert_projection(c3d, d['pose'], d['K'], d['img'])
    buf = torch.ones((), device=DEV)
    err = head.proj_error_coder.encode(tp - d['roi'], d['dist'])
    tl = robust_kl_loss(err, 0, logstd=ls, momentum=0.1, mean_inv_std=buf).mean()
    tl.backward()
    assert (proj - tp.detach()).abs().max().item() <= 1e-6 * max(1000.0, tp.abs().max().item())
    tl = tl.detach()
    assert abs(float(loss) - float(tl)) <= 1e-5 * abs(float(tl)) and abs(float(buf) - float(head.loss_proj.mean_inv_std)) <= 1e-6 * float(buf)
    _grad_ok(gc.cpu().numpy(), c3d.grad.cpu().numpy())
    _grad_ok(gl.cpu().numpy(), ls.grad.cpu().numpy())
    # the dispatch rule: a leading pose dimension, a weight, avg_factor or 'none' run the torch path and still agree
    p2 = UncertProjectionHead().to(DEV)(d['c3d'], d['pose'][None], d['K'], d['img'])
    assert p2.shape == (1, 384, 2, 28, 28) and (p2[0] - proj).abs().max().item() <= 1e-6 * max(1000.0, proj.abs().max().item())
    from monorun_amd.losses import RobustKLLoss
    m = RobustKLLoss(momentum=0.1).to(DEV)
    e = err.detach()
    mean_hip = m(e, 0, logstd=d['ls'])
    m.mean_inv_std.fill_(1.0)
    mean_w = m(e, 0, logstd=d['ls'], weight=torch.ones_like(e))
    m.mean_inv_std.fill_(1.0)
    none = m(e, 0, logstd=d['ls'], reduction_override='none')
    assert none.shape == e.shape
    assert abs(float(mean_hip) - float(mean_w)) <= 1e-5 * abs(float(mean_w)) and abs(float(none.mean()) - float(mean_w)) <= 1e-5 * abs(float(mean_w))


def test_ties_follow_torch_rules():
    """z == z_min, u == -border, u == W + border (half to each side of torch.min), dw == delta (the linear branch), pred == 0."""
    head = _head()
    K = torch.eye(3, device=DEV).expand(4, 3, 3).contiguous()
    pose = torch.tensor([[0.0, 0.0, 0.25, 0.0], [0.0, 0.0, 0.5, 0.0], [0.0, 0.0, 0.5, 0.0], [0.0, 0.0, 0.5, 0.0]], device=DEV)
    img = torch.tensor([[375.0, 1242.0]] * 4, device=DEV)
    c3d = torch.zeros(4, 3, 1, 2, device=DEV)
    c3d[0, 0], c3d[0, 2] = 1.0, 0.25                      # z == 0.5 == z_min (object 0)
    c3d[1, 0], c3d[1, 2] = -200.0, 0.5                    # u == -200 at z == 1
    c3d[2, 0], c3d[2, 2] = 1442.0, 0.5                    # u == W + 200
    c3d[3, 0], c3d[3, 2] = 10.0, 0.5                      # interior
    c3d.requires_grad_(True)
    out = head(c3d, pose, K, img)
    assert out[0, 0, 0, 0].item() == 2.0 and out[1, 0, 0, 0].item() == -200.0 and out[2, 0, 0, 0].item() == 1442.0
    g = torch.randn(4, 2, 1, 2, device=DEV)
    out.backward(g)
    from monorun_amd.projection_head import uncert_projection
    c2 = c3d.detach().clone().requires_grad_(True)
    uncert_projection(c2, pose, K, img).backward(g)
    torch.testing.assert_close(c3d.grad, c2.grad, rtol=1e-6, atol=1e-7)
    assert c3d.grad[0, 2, 0, 0].item() != 0                       # the clamp at z_min passes the gradient at its bound
    assert c3d.grad[1, 0, 0, 0].item() == g[1, 0, 0, 0].item()    # clamp(min=-border) passes at its bound
    assert c3d.grad[2, 0, 0, 0].item() == g[2, 0, 0, 0].item() / 2      # torch.min: half to each side
    # the loss: dw == delta (logstd 0, inv exactly 1) takes the linear branch; pred == 0 gets no gradient from |pred|
    from monorun_amd.losses import RobustKLLoss, robust_kl_loss
    pred = torch.tensor([float(np.float32(1.414)), -float(np.float32(1.414)), 0.0, 0.3], device=DEV).reshape(1, 4).requires_grad_(True)
    ls = torch.zeros(1, 4, device=DEV, requires_grad=True)
    m = RobustKLLoss(momentum=0.1).to(DEV)
    m(pred, 0, logstd=ls).backward()
    p2, l2 = pred.detach().clone().requires_grad_(True), ls.detach().clone().requires_grad_(True)
    robust_kl_loss(p2, 0, logstd=l2, momentum=0.1, mean_inv_std=torch.ones((), device=DEV)).mean().backward()
    torch.testing.assert_close(pred.grad, p2.grad, rtol=1e-6, atol=0)
    torch.testing.assert_close(ls.grad, l2.grad, rtol=1e-6, atol=1e-7)
    c = float(m.mean_inv_std)
    assert abs(pred.grad[0, 0].item() - float(np.float32(1.414)) / 4 / c) <= 1e-6 and pred.grad[0, 2].item() == 0.0
    assert pred.grad[0, 1].item() == -pred.grad[0, 0].item()


def test_nan_logstd_gives_nan_loss_and_buffer():
    from monorun_amd.losses import RobustKLLoss
    m = RobustKLLoss(momentum=0.1).to(DEV)
    x = torch.randn(2, 2, 28, 28, device=DEV)
    ls = torch.randn(2, 2, 28, 28, device=DEV)
    ls[1, 0, 3, 3] = float('nan')
    assert torch.isnan(m(x, 0, logstd=ls)) and torch.isnan(m.mean_inv_std)


def test_shapes_dtypes_and_strides():
    from monorun_amd.projection_head import UncertProjectionHead
    head = UncertProjectionHead().to(DEV)
    # n = 0: no launch, a zero loss with a graph, the buffer untouched
    e = _random_group(0, 28, 28, 0)
    proj, loss, (gc, gl) = _step(head, e)
    assert proj.shape == (0, 2, 28, 28) and loss.item() == 0 and gc.shape == (0, 3, 28, 28)
    assert float(head.loss_proj.mean_inv_std) == 1.0
    for n, h, w in ((1, 28, 28), (384, 28, 28), (4096, 28, 28), (7, 56, 56), (3, 7, 9)):
        d = _random_group(n, h, w, n + h)
        with torch.no_grad():
            out = head(d['c3d'], d['pose'], d['K'], d['img'])
        want = projection_ref.project(d['c3d'].cpu().numpy(), d['pose'].cpu().numpy(), d['K'].cpu().numpy(), d['img'].cpu().numpy())
        assert np.array_equal(out.cpu().numpy(), want), (n, h, w)
    # the pos_bboxes_3d[:, 3:7] slice as pose, read in place; non-contiguous coordinates; fp16 / fp64 inputs
    d = _random_group(384, 28, 28, 5)
    with torch.no_grad():
        ref = head(d['c3d'], d['pose'], d['K'], d['img'])
    boxes = torch.cat([torch.ones(384, 3, device=DEV), d['pose']], 1)
    assert boxes[:, 3:7].stride() == (7, 1)
    perm = d['c3d'].permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not perm.is_contiguous()
    with torch.no_grad():
        assert torch.equal(head(perm, boxes[:, 3:7], d['K'], d['img']), ref)
        assert torch.equal(head(d['c3d'].double(), d['pose'].double(), d['K'].double(), d['img'].double()), ref.double())
        assert head(d['c3d'].half(), d['pose'], d['K'], d['img']).dtype == torch.float16
    # gradients come back in the input's dtype; fp16 / fp64 logstd in the loss
    for dt in (torch.float16, torch.float64):
        c3d = d['c3d'].to(dt).requires_grad_(True)
        ls = d['ls'].to(dt).requires_grad_(True)
        proj = head(c3d, d['pose'], d['K'], d['img'])
        loss = head.loss(proj.float(), ls, d['roi'], d['dist'])['loss_proj']
        loss.backward()
        assert c3d.grad.dtype == dt and ls.grad.dtype == dt and torch.isfinite(c3d.grad.float()).all()
    # coords_2d_roi that requires grad gets -grad of the encoded error through torch
    roi = d['roi'].clone().requires_grad_(True)
    proj = head(d['c3d'].clone().requires_grad_(True), d['pose'], d['K'], d['img'])
    head.loss(proj, d['ls'], roi, d['dist'])['loss_proj'].backward()
    assert roi.grad is not None and float(roi.grad.abs().max()) > 0


def test_determinism():
    d = _random_group(4096, 28, 28, 21)
    outs = []
    for _ in range(2):
        head = _head()
        proj, loss, (gc, gl) = _step(head, d)
        outs.append((proj, loss, head.loss_proj.mean_inv_std.clone(), gc, gl))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_training_step_of_the_noc_head():
    """A synthetic batch: a leaf NOC prediction decoded in torch to coords_3d, loss_proj with the ground-truth poses and the
    roi_align_avg grid, the training decode_logstd into the differentiable PnP, loss_proj + loss_calib backpropagated."""
    from monorun_amd import synthetic as syn
    from monorun_amd.pose_head import UncertPropPnPOptimizer
    from monorun_amd.projection_head import UncertProjectionHead
    B = 64
    b = syn.make_batch(B=B, seed=41)
    dev = DEV
    c3d_true = torch.from_numpy(b['coords_3d']).to(dev)
    dims = torch.from_numpy(np.asarray(b['dims'], np.float32)).to(dev)
    noc = (c3d_true / dims[:, :, None, None]).clone().requires_grad_(True)          # the NOC head's output (leaf)
    ls_enc = torch.from_numpy(b['logstd']).to(dev).clone().requires_grad_(True)     # proj_logstd (leaf)
    coords_3d = noc * dims[:, :, None, None]                                         # the training decode, in torch
    K1 = torch.from_numpy(np.asarray(b['K'], np.float32)).to(dev)                   # (1, 3, 3), shared by the batch
    img1 = torch.from_numpy(np.asarray(b['img_shape'], np.float32)).to(dev)         # (1, 2) [H, W]
    K, img = K1.expand(B, 3, 3).contiguous(), img1.expand(B, 2).contiguous()
    gt = torch.from_numpy(np.concatenate([b['dims'], b['gt_t'], b['gt_yaw'][:, None]], 1).astype(np.float32)).to(dev)
    rois = torch.from_numpy(np.concatenate([np.zeros((B, 1)), b['rois']], 1).astype(np.float32)).to(dev)
    from monorun_amd.pose_head import roi_align_avg
    coord_map = torch.stack(torch.meshgrid(torch.arange(syn.IMG_W, device=dev, dtype=torch.float32),
                                           torch.arange(syn.IMG_H, device=dev, dtype=torch.float32), indexing='xy'), 0)[None]
    roi_grid = roi_align_avg(coord_map, rois, (28, 28))
    head = UncertProjectionHead().to(dev)
    dist = torch.norm(gt[:, 3:6], dim=1, keepdim=True)
    proj = head(coords_3d, gt[:, 3:7], K, img)
    loss_proj = head.loss(proj, ls_enc, roi_grid, dist)['loss_proj']
    ls_px = head.proj_error_coder.decode_logstd(ls_enc, None, dist)
    cfg = dict(type='PnPUncert', z_min=0.5, epnp_istd_thres=0.6, inlier_opt_only=True, forward_exact_hessian=False, differentiable=True)
    pose_head = UncertPropPnPOptimizer(pnp=cfg, loss_calib=dict(type='KLLossMV', loss_weight=0.01)).to(dev)
    ret, yaw, t, cov, cov_calib = pose_head(roi_grid, ls_px, coords_3d, K1, img1)
    yt, tt = pose_head.get_targets(gt)
    losses, _ = pose_head.loss(ret, yaw, t, cov_calib, dims, yt, tt, gt)
    (loss_proj + losses['loss_calib']).backward()
    for g in (noc.grad, ls_enc.grad):
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    assert int(ret.sum()) >= B // 2
    # the buffer moved by the momentum rule from 1
    inv = torch.exp(-ls_enc.detach()).clamp(max=1e4)
    want = 0.9 + 0.1 * float(inv.double().mean())
    assert abs(float(head.loss_proj.mean_inv_std) - want) <= 1e-5 * want
