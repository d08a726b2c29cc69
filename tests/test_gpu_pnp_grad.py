"""The backward of ``pnp_uncert`` on the MI355X (``mr_pnp_uncert_backward_batched``): gradients against the fp64
autodiff reference (tests/pnp_grad_ref.py) evaluated at the GPU's own pose / mask / valid / covariance, unchanged forward outputs,
zero gradients where the contract says so, determinism, and training through the pose head."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_grad_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

# per object: |g - g_ref| <= TOL * max|g_ref| over the object's gradients of one tensor.  Both sides evaluate the same fp64 quantities
# at the same (f32) pose, covariance and input values; what is left is fp64 round-off amplified by cond(H_F), the f32 rounding of the
# kernel's outputs (6e-8) and rows that sit exactly on a clip boundary (different operation order).
TOL = 1e-4


def _dev():
    return torch.device('cuda:0')


def _inputs(B, hw=28, seed=3, dtype=torch.float32):
    from monorun_amd import synthetic as syn
    b = syn.make_batch(B=B, hw=hw, seed=seed)
    x2d, istd, x3d, K, ur, vr, thr = syn.pnp_boundary(b, planar=True)

    def dv(a, dt=torch.float32):
        t = torch.from_numpy(np.asarray(a))
        d = torch.empty_strided(t.shape, t.stride(), dtype=dt, device=_dev())
        d.copy_(t)
        return d
    return dv(x2d, dtype), dv(istd, dtype), dv(x3d, dtype), dv(K), dv(ur), dv(vr), dv(thr)


def _losses(B, seed=0):
    g = torch.Generator().manual_seed(seed)
    gp = torch.randn(B, 4, generator=g, dtype=torch.float64).to(_dev())
    gc = torch.randn(B, 4, 4, generator=g, dtype=torch.float64).to(_dev())
    return gp, gc


def _close(g, r, tol=TOL):
    """per-object relative error, max over the batch"""
    g, r = g.detach().double().flatten(1), r.detach().double().flatten(1)
    scale = r.abs().amax(1).clamp(min=1e-300)
    return float(((g - r).abs().amax(1) / scale).max()) if g.numel() else 0.0


def _check(valid, pose, cov, mask, x, K, ur, vr, lm_all, gp, gc, which):
    """backward through the device function for one loss ('pose' | 'cov' | 'both') at the forward's f32 pose / cov against the reference"""
    from monorun_amd.ops.least_squares.pnp_uncert import pnp_uncert_backward_device
    ret = valid.bool()
    gpose = gp if which in ('pose', 'both') else None
    C, G = (cov, gc) if which in ('cov', 'both') else (None, None)
    got = pnp_uncert_backward_device(*x, K, ur, vr, pose, mask.to(torch.uint8), ret.to(torch.uint8), gpose, C, G, lm_all_points=lm_all,
                                     with_status=True)
    want = ref.pnp_grad_ref(*x, K, ur, vr, 0.5, pose, mask, ret, lm_all, gpose, C, G)
    assert torch.equal(got[3], want[3]), 'status differs from the reference'
    errs = [_close(a, b) for a, b in zip(got[:3], want[:3])]
    assert max(errs) <= TOL, (which, errs)
    assert all(bool(torch.isfinite(a).all()) for a in got[:3])
    return got


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.float64])
@pytest.mark.parametrize('initialiser,inlier_opt_only', [('epnp', True), ('epnp', False), ('k0', True), ('k0', False)])
def test_gradients_match_reference(initialiser, inlier_opt_only, dtype):
    from monorun_amd.ops import pnp_uncert
    B = 37
    x2d, istd, x3d, K, ur, vr, thr = _inputs(B, dtype=dtype)
    leaves = [a.clone().requires_grad_(True) for a in (x2d, istd, x3d)]
    out = pnp_uncert(*leaves, K, ur, vr, z_min=0.5, epnp_istd_thres=0.6, epnp_ransac_thres=thr, inlier_opt_only=inlier_opt_only,
                     initialiser=initialiser, differentiable=True)
    assert out[0].sum() >= 30
    gp, gc = (g.to(dtype).double() for g in _losses(B))          # output gradients as autograd hands them over (in the output dtype)
    # the f32 pose and covariance the kernels produced (r_vec / t_vec / pose_cov are their casts to the input dtype)
    _, _, _, pose, mask, valid, cov = out[1].grad_fn.saved_tensors
    for which in ('pose', 'cov', 'both'):
        got = _check(valid, pose, cov, mask, (x2d, istd, x3d), K, ur, vr, not inlier_opt_only, gp, gc, which)
        # the autograd path hands back exactly the device gradients, in the source dtype
        L = 0
        if which in ('pose', 'both'):
            L = L + (out[1] * gp[:, :1].to(dtype)).sum() + (out[2] * gp[:, 1:].to(dtype)).sum()
        if which in ('cov', 'both'):
            L = L + (out[3] * gc.to(dtype)).sum()
        ga = torch.autograd.grad(L, leaves, retain_graph=True)
        for a, d, leaf in zip(ga, got[:3], leaves):
            assert a.dtype == leaf.dtype and a.device == leaf.device
            assert torch.equal(a, d.to(dtype)), which


@pytest.mark.parametrize('B,hw,initialiser', [(1, 28, 'k0'), (1024, 28, 'epnp'), (64, 56, 'k0')])
def test_gradients_match_reference_sizes(B, hw, initialiser):
    from monorun_amd.ops import pnp_uncert
    x2d, istd, x3d, K, ur, vr, thr = _inputs(B, hw=hw, seed=11)
    with torch.no_grad():
        out = pnp_uncert(x2d, istd, x3d, K, ur, vr, z_min=0.5, epnp_istd_thres=0.6, epnp_ransac_thres=thr, inlier_opt_only=True,
                         initialiser=initialiser)
    gp, gc = _losses(B, seed=1)
    _check(out[0], torch.cat([out[1], out[2]], 1), out[3], out[4], (x2d, istd, x3d), K, ur, vr, False, gp, gc, 'both')


@pytest.mark.parametrize('initialiser', ['epnp', 'k0'])
def test_forward_unchanged_and_cpu_inputs(initialiser):
    from monorun_amd.ops import pnp_uncert
    x2d, istd, x3d, K, ur, vr, thr = _inputs(64, seed=5)
    kw = dict(z_min=0.5, epnp_istd_thres=0.6, epnp_ransac_thres=thr, inlier_opt_only=True, initialiser=initialiser, cov_symeig_rule=True)
    base = pnp_uncert(x2d, istd, x3d, K, ur, vr, **kw)
    leaves = [a.clone().requires_grad_(True) for a in (x2d, istd, x3d)]
    diff = pnp_uncert(*leaves, K, ur, vr, differentiable=True, **kw)
    assert all(torch.equal(a, b) for a, b in zip(base, diff))
    assert diff[1].requires_grad and diff[2].requires_grad and diff[3].requires_grad and not diff[0].requires_grad
    # host inputs: staged through the GPU; the gradients come back on the host, equal to the device run's
    host = [a.detach().cpu().requires_grad_(True) for a in (x2d, istd, x3d)]
    hout = pnp_uncert(*host, K, ur, vr, differentiable=True, **kw)
    L = lambda o: o[1].sum() + (o[2] * torch.arange(3, device=o[2].device)).sum() + o[3].sum()
    gd = torch.autograd.grad(L(diff), leaves)
    gh = torch.autograd.grad(L(hout), host)
    for a, b in zip(gd, gh):
        assert b.device.type == 'cpu' and torch.equal(a.cpu(), b)


def test_zero_gradients_status_and_determinism():
    from monorun_amd.ops import pnp_uncert
    from monorun_amd.ops.least_squares.pnp_uncert import pnp_uncert_backward_device
    B = 48
    x2d, istd, x3d, K, ur, vr, thr = _inputs(B, seed=9)
    with torch.no_grad():
        ret, yaw, t, cov, mask = pnp_uncert(x2d, istd, x3d, K, ur, vr, z_min=0.5, epnp_istd_thres=0.6, epnp_ransac_thres=thr,
                                            inlier_opt_only=True, initialiser='k0')
    pose = torch.cat([yaw, t], 1)
    valid = ret.clone()
    valid[::5] = False                                   # objects the forward did not solve
    pose[1::5, 3] = 1.0                                  # close to the camera: part of the points behind z_min
    pose[2::5, 1] += 12.0                                # at the border: u rows clipped
    gp, gc = _losses(B, seed=2)
    got = _check(valid, pose, cov, mask, (x2d, istd, x3d), K, ur, vr, False, gp, gc, 'both')
    g2, gw, g3, st = got
    assert torch.equal(st[::5], torch.ones_like(st[::5]))
    for g in (g2, gw, g3):
        assert torch.equal(g[::5], torch.zeros_like(g[::5]))
    # z-clipped points: no row of theirs is in either set -> all seven gradients zero
    from torch.func import vmap
    _, z = vmap(ref._proj)(pose.double(), x3d.double(), K.double().expand(B, 3, 3))
    zc = z < 0.5
    assert int(zc[1::5].sum()) > 0
    for g in (g2, gw, g3):
        assert torch.equal(g[zc], torch.zeros_like(g[zc]))
    # determinism: no atomics -> a second call is bit-identical, here at B = 1024
    x2d, istd, x3d, K, ur, vr, thr = _inputs(1024, seed=4)
    with torch.no_grad():
        ret, yaw, t, cov, mask = pnp_uncert(x2d, istd, x3d, K, ur, vr, z_min=0.5, epnp_istd_thres=0.6, epnp_ransac_thres=thr,
                                            inlier_opt_only=True, initialiser='k0')
    gp, gc = _losses(1024, seed=3)
    args = (x2d, istd, x3d, K, ur, vr, torch.cat([yaw, t], 1), mask.to(torch.uint8), ret.to(torch.uint8), gp, cov, gc)
    a = pnp_uncert_backward_device(*args, with_status=True)
    b = pnp_uncert_backward_device(*args, with_status=True)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def _kl(ret, yaw, t, cov_calib, gt):
    """KL-style loss of the pose head's outputs: Gaussian negative log-likelihood of a target pose under (pose, calibrated cov)"""
    d = (torch.cat([yaw, t], 1) - gt)[ret]
    c = cov_calib[ret]
    return 0.5 * (torch.linalg.solve(c, d[..., None])[..., 0] * d).sum() + 0.5 * torch.logdet(c).sum()


def test_training_through_the_pose_head():
    from monorun_amd import synthetic as syn
    from monorun_amd.ops import pnp_uncert
    from monorun_amd.pose_head import UncertPropPnPOptimizer, _planar_view
    B = 32
    b = syn.make_batch(B=B, seed=21)
    dev = _dev()
    c2d, ls, c3d = (torch.from_numpy(b[k]).to(dev) for k in ('coords_2d', 'logstd', 'coords_3d'))
    K = torch.from_numpy(np.asarray(b['K'], np.float32)).to(dev)
    img = torch.from_numpy(np.asarray(b['img_shape'], np.float32)).to(dev)
    cfg = dict(type='PnPUncert', z_min=0.5, epnp_istd_thres=0.6, inlier_opt_only=True, forward_exact_hessian=False, differentiable=True)
    head = UncertPropPnPOptimizer(pnp=cfg).to(dev)
    leaves = [a.clone().requires_grad_(True) for a in (c2d, ls, c3d)]
    ret, yaw, t, cov, cov_calib = head(*leaves, K, img)
    gt = torch.cat([yaw, t], 1).detach() + 0.05
    L = _kl(ret, yaw, t, cov_calib, gt)
    g_head = torch.autograd.grad(L, leaves + [head.cov_calib_logscale])
    assert all(bool(torch.isfinite(g).all()) for g in g_head) and float(g_head[0].abs().max()) > 0
    # the same computation through the functional op
    f = [a.clone().requires_grad_(True) for a in (c2d, ls, c3d)]
    istd = torch.exp(-f[1]) / head.std_scale
    ur, vr = head._ranges(f[0], img)
    thr = head.epnp_ransac_thres_ratio * (f[0][:, 1, -1, 0] - f[0][:, 1, 0, 0])
    o = pnp_uncert(_planar_view(f[0]), _planar_view(istd), _planar_view(f[2]), K, ur, vr, z_min=0.5, epnp_istd_thres=0.6,
                   epnp_ransac_thres=thr, inlier_opt_only=True, differentiable=True)
    g_fun = torch.autograd.grad(_kl(o[0], o[1], o[2], head._calibrate(o[3]), gt), f)
    for a, c in zip(g_head[:3], g_fun):
        assert torch.equal(a, c)
    # coord_istd_normalize=True: the normalisation stays in torch and autograd carries the gradient through it
    from monorun_amd.ops import PnPUncert
    m = PnPUncert(inlier_opt_only=True, coord_istd_normalize=True, differentiable=True)
    x2d, istd0, x3d, K2, ur2, vr2, thr2 = _inputs(B, seed=23)
    w = istd0.clone().requires_grad_(True)
    out = m(x2d, w, x3d, K2, ur2, vr2, thr2)
    gc = _losses(B, seed=4)[1].float()
    gw = torch.autograd.grad((out[3] * gc).sum() + out[2].sum(), w)[0]
    wn = (istd0 / istd0.mean(dim=(1, 2), keepdim=True).clamp(min=m.eps)).detach().requires_grad_(True)
    out2 = pnp_uncert(x2d, wn, x3d, K2, ur2, vr2, epnp_istd_thres=m.epnp_istd_thres, epnp_ransac_thres=thr2, inlier_opt_only=True,
                      differentiable=True)
    assert all(torch.equal(a, c) for a, c in zip(out, out2))
    gn = torch.autograd.grad((out2[3] * gc).sum() + out2[2].sum(), wn)[0]
    w2 = istd0.clone().requires_grad_(True)
    manual = torch.autograd.grad(w2 / w2.mean(dim=(1, 2), keepdim=True).clamp(min=m.eps), w2, gn)[0]
    torch.testing.assert_close(gw, manual, rtol=1e-5, atol=1e-6 * float(manual.abs().max()))
