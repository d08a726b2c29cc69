"""Adversarial correspondence sets for the PnP boundary (numpy only: shared by the CPU tests, the `-m gpu` tests and tests/sweeps/gpu_epnp_fuzz.py).

make_case(mode, rng) -> [x2d (B,P,2), istd (B,P,2), x3d (B,P,3), K, u_range, v_range, ransac_thr] float32, a random half of the objects of a
synthetic batch damaged in the way `mode` names; the other half stays ordinary."""
import numpy as np

from monorun_amd import synthetic as syn

MODES = ('coincident', 'nan', 'zero_weights', 'overflow', 'planar', 'garbage', 'zero_threshold', 'inf', 'collinear', 'one_point')


def make_case(mode, rng, B=None, hw=None, planar_layout=None):
    """mode: one of MODES or its index.  B / hw / planar_layout (channel-planar strided views, as the pipeline hands them over) are drawn
    from rng when None."""
    if not isinstance(mode, str):
        mode = MODES[int(mode) % len(MODES)]
    B = int(rng.choice([1, 3, 64, 200])) if B is None else int(B)
    hw = int(rng.choice([3, 4, 8, 10, 28])) if hw is None else int(hw)
    b = syn.make_batch(B=B, hw=hw, seed=int(rng.integers(1 << 30)))
    planar_layout = bool(rng.integers(2)) if planar_layout is None else bool(planar_layout)
    x2d, istd, x3d, K, ur, vr, thr = [np.array(a, copy=True) for a in syn.pnp_boundary(b, planar=planar_layout)]
    P = x2d.shape[1]
    sel = rng.uniform(size=B) < 0.5
    if mode == 'coincident': x3d[sel] = 0.0                                   # all points coincide
    elif mode == 'nan': x2d[sel, rng.integers(P)] = np.nan                    # NaN correspondences
    elif mode == 'zero_weights': istd[sel] = 0.0
    elif mode == 'overflow': x3d[sel] *= 1e20
    elif mode == 'planar': x3d[sel, :, 1] = 0.0                               # planar object (rank-2 covariance: one control point collapses)
    elif mode == 'garbage': x3d[sel] = rng.normal(0, 1, x3d[sel].shape).astype(np.float32)
    elif mode == 'zero_threshold': thr[sel] = 0.0
    elif mode == 'inf': x2d[sel] = np.inf
    elif mode == 'collinear': x3d[sel, :, 0] = 0.0; x3d[sel, :, 1] = 0.0      # collinear object
    elif mode == 'one_point': x3d[sel] = x3d[sel][:, :1]                      # every point the same 3-D point, different pixels
    else: raise ValueError(mode)
    return [x2d, istd, x3d, K, ur, vr, thr]


def make_tree_sensitive(rng, B, P):
    """Objects whose covariance Hessian is singular to rounding at the LM's pose, so that its Cholesky factorisation — the `valid` flag —
    depends on the summation tree, i.e. on the waves per object of the launch (csrc/pnp_kernel_body.inc stage 4).  Four points lie on a
    vertical line of the object (same x, z): for them a yaw step is a translation, J^T J has rank 3.  They carry weights around 1; the other
    P - 4 points carry weights of 1e-10 ... 1e-8, which makes the smallest pivot comparable to the rounding of the sums.  Fewer than five
    istd candidates: the initialiser runs on all points, which are exact projections of the object at its ground-truth pose, so RANSAC
    and the LM end normally.  Returns [x2d, istd, x3d, K, u_range, v_range, ransac_thr] float32, (B,P,C) contiguous."""
    b = syn.make_batch(B=B, hw=4, seed=int(rng.integers(1 << 30)))
    _, _, _, K, ur, vr, thr = [np.array(a, copy=True) for a in syn.pnp_boundary(b, planar=False)]
    dims = b['dims']
    X = rng.uniform(-0.5, 0.5, (B, P, 3)) * dims[:, None, :]
    X[..., 1] = -rng.uniform(0, 1, (B, P)) * dims[:, None, 1]
    line = np.zeros((B, P), bool)
    for i in range(B):
        line[i, rng.choice(P, 4, replace=False)] = True
    X[..., 0] = np.where(line, X[:, :1, 0], X[..., 0])
    X[..., 2] = np.where(line, X[:, :1, 2], X[..., 2])
    X = X.astype(np.float32)
    cam = syn._to_cam(X.astype(np.float64), b['gt_yaw'], b['gt_t'])
    Kd = K.reshape(3, 3).astype(np.float64)
    x2d = np.stack([Kd[0, 0] * cam[..., 0] / cam[..., 2] + Kd[0, 2], Kd[1, 1] * cam[..., 1] / cam[..., 2] + Kd[1, 2]], -1).astype(np.float32)
    eps = 10.0 ** rng.uniform(-10, -8, (B, 1, 1))
    istd = np.where(line[..., None], rng.uniform(0.5, 2, (B, P, 2)), eps * rng.uniform(0.5, 2, (B, P, 2))).astype(np.float32)
    return [x2d, istd, X, K, ur, vr, thr]
