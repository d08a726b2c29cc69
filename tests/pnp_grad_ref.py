"""Independent fp64 torch reference for the backward of the 4-DoF ``pnp_uncert``.

The weighted residual r(theta, x) is built from the formulas of the reference's ``forward_proj`` (jacobian.py:4-45: yaw rotation about
y, K (R X + t), division by depth), with the masks (z clip, per-axis uv clip, inlier mask) evaluated once at the given pose and then
frozen.  J = dr/dtheta, F = J^T r, H_F = dF/dtheta and phi = <W, J^T J> all come from torch.func autodiff, not from the kernel's closed
forms; then g = dL/dpose + dphi/dtheta, v = H_F^-1 g and grad_x = d(phi - v^T F)/dx.  Used by the CPU finite-difference test and as
the yardstick of the GPU kernel.
"""
import torch
from torch.func import grad, jacfwd, vmap


def _proj(theta, x3d, K, keep=None):
    """pi (P,2) and depth z (P,) of one object: forward_proj's arithmetic without the clamps.  keep (P,) bool: points whose depth is
    used; the others divide by 1 (their rows are masked: no inf / NaN reaches autodiff through them)."""
    c, s = torch.cos(theta[0]), torch.sin(theta[0])
    X, Y, Z = x3d[:, 0], x3d[:, 1], x3d[:, 2]
    q = torch.stack([c * X + s * Z + theta[1], Y + theta[2], -s * X + c * Z + theta[3]], dim=1)
    uvz = q @ K.T
    z = uvz[:, 2] if keep is None else torch.where(keep, uvz[:, 2], torch.ones_like(uvz[:, 2]))
    return uvz[:, :2] / z[:, None], z


def row_masks(x2d, x3d, K, ur, vr, z_min, pose, inlier, lm_all):
    """(m_lm, m_cov) (B,P,2) fp64 0/1: the rows of S_LM and S_cov at `pose` (the zero_mask of jacobian.py:52-58)."""
    with torch.no_grad():
        pi, z = vmap(_proj)(pose, x3d, K)
        lb = torch.stack([ur[:, 0], vr[:, 0]], 1)[:, None]
        ub = torch.stack([ur[:, 1], vr[:, 1]], 1)[:, None]
        keep = (z >= z_min)[..., None] & (pi >= lb) & (pi <= ub)
        m_cov = (keep & inlier[..., None]).to(torch.float64)
        m_lm = keep.to(torch.float64) if lm_all else m_cov
    return m_lm, m_cov


def resid(theta, x2d, istd, x3d, K, m):
    pi, _ = _proj(theta, x3d, K, m.sum(1) > 0)
    return m * istd * (pi - x2d)


def _jac(theta, x2d, istd, x3d, K, m):
    return jacfwd(resid, argnums=0)(theta, x2d, istd, x3d, K, m)          # (P,2,4)


def _F(theta, x2d, istd, x3d, K, m):
    J = _jac(theta, x2d, istd, x3d, K, m)
    return torch.einsum('pkj,pk->j', J, resid(theta, x2d, istd, x3d, K, m))


def _phi(theta, x2d, istd, x3d, K, m, W):
    J = _jac(theta, x2d, istd, x3d, K, m)
    return (W * torch.einsum('pki,pkj->ij', J, J)).sum()


def _lagr(x2d, istd, x3d, theta, K, m_lm, m_cov, W, v):
    return _phi(theta, x2d, istd, x3d, K, m_cov, W) - (v * _F(theta, x2d, istd, x3d, K, m_lm)).sum()


def stationarity(theta, x2d, istd, x3d, K, m):
    """F (B,4) and H_F (B,4,4) of every object (used by the Newton re-solve of the finite-difference test)."""
    return vmap(_F)(theta, x2d, istd, x3d, K, m), vmap(jacfwd(_F, argnums=0))(theta, x2d, istd, x3d, K, m)


def jtj(theta, x2d, istd, x3d, K, m):
    J = vmap(_jac)(theta, x2d, istd, x3d, K, m)
    return torch.einsum('bpki,bpkj->bij', J, J)


def pnp_grad_ref(x2d, istd, x3d, K, ur, vr, z_min, pose, inlier, valid, lm_all, grad_pose, cov=None, grad_cov=None):
    """Gradients (grad_x2d (B,P,2), grad_istd (B,P,2), grad_x3d (B,P,3)) fp64 and status (B,) (0 ok, 1 not valid, 2 singular H_F).

    All tensors any device; everything is promoted to fp64.  K (B|1,3,3), ur / vr (B|1,2), pose (B,4) [yaw, t], inlier (B,P) bool,
    valid (B,) bool, grad_pose (B,4) or None, cov / grad_cov (B,4,4) or None."""
    d = dict(dtype=torch.float64, device=x2d.device)
    B, P = x2d.shape[:2]
    x2d, istd, x3d = x2d.to(**d), istd.to(**d), x3d.to(**d)
    K = K.to(**d).reshape(-1, 3, 3).expand(B, 3, 3)
    ur, vr = ur.to(**d).reshape(-1, 2).expand(B, 2), vr.to(**d).reshape(-1, 2).expand(B, 2)
    pose = pose.to(**d).reshape(B, 4)
    inlier = inlier.to(device=x2d.device, dtype=torch.bool)
    valid = valid.to(device=x2d.device, dtype=torch.bool)
    m_lm, m_cov = row_masks(x2d, x3d, K, ur, vr, z_min, pose, inlier, lm_all)
    gp = grad_pose.to(**d).reshape(B, 4) if grad_pose is not None else torch.zeros(B, 4, **d)
    if cov is not None:
        C = cov.to(**d).reshape(B, 4, 4)
        G = grad_cov.to(**d).reshape(B, 4, 4)
        W = -C @ (0.5 * (G + G.transpose(1, 2))) @ C
        W = 0.5 * (W + W.transpose(1, 2))
    else:
        W = torch.zeros(B, 4, 4, **d)
    H = vmap(jacfwd(_F, argnums=0))(pose, x2d, istd, x3d, K, m_lm)
    g = gp + vmap(grad(_phi, argnums=0))(pose, x2d, istd, x3d, K, m_cov, W)
    Hs = torch.where(valid[:, None, None], H, torch.eye(4, **d).expand(B, 4, 4))
    v, info = torch.linalg.solve_ex(Hs, g)
    ok = valid & (info == 0) & torch.isfinite(v).all(1) & torch.isfinite(H).all((1, 2))
    v = torch.where(ok[:, None], v, torch.zeros_like(v))
    gx2d, gistd, gx3d = vmap(grad(_lagr, argnums=(0, 1, 2)))(x2d, istd, x3d, pose, K, m_lm, m_cov, W, v)
    z = lambda t: torch.where(ok[:, None, None], t, torch.zeros_like(t))
    status = torch.where(valid, torch.where(ok, 0, 2), 1).to(torch.uint8)
    return z(gx2d), z(gistd), z(gx3d), status
