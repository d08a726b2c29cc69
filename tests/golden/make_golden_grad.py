#!/usr/bin/env python3
"""G13: the reference's point-wise Jacobians (monorun/ops/least_squares/jacobian.py:101-138, ``get_jacobians``), the quantities the
backward of ``pnp_uncert`` is built from: jac_pw_c3d = dr/dX, jac_ew_istd = dr/distd, plus the pose Jacobians jac_t_vec / jac_yaw,
with the reference's zero rows (z clip, per-axis uv clip, outliers).

Runs only in the authoring container (needs the reference tree, read-only; loaded by file path, nothing of it is copied).  The
fixture is data: seeded inputs and what the reference's own function returned for them.

    python tests/golden/make_golden_grad.py         # rewrites tests/golden/g13_pointwise_jacobians.npz
"""
import importlib.util
import os
import sys

import numpy as np
import torch

REF = '/root/reference/monorun'
OUT = os.path.dirname(os.path.abspath(__file__))


def _load(modname, relpath):
    spec = importlib.util.spec_from_file_location(modname, os.path.join(REF, relpath))
    m = importlib.util.module_from_spec(spec)
    sys.modules[modname] = m
    spec.loader.exec_module(m)
    return m


def main():
    jac = _load('refls_jacobian', 'ops/least_squares/jacobian.py')
    rng = np.random.default_rng(1313)
    B, P = 8, 64
    K1 = np.array([[707.0912, 0.0, 601.8873], [0.0, 707.0912, 183.1104], [0.0, 0.0, 1.0]])
    dims = np.array([3.89, 1.53, 1.62])
    yaw = rng.uniform(-np.pi, np.pi, (B, 1))
    t = np.stack([rng.uniform(-8, 8, B), rng.uniform(1, 2, B), rng.uniform(6, 40, B)], 1)
    x3d = (rng.uniform(-0.5, 0.5, (B, P, 3)) + np.array([0.0, -0.5, 0.0])) * dims
    c, s = np.cos(yaw[:, 0]), np.sin(yaw[:, 0])
    R = np.zeros((B, 3, 3)); R[:, 0, 0] = c; R[:, 0, 2] = s; R[:, 1, 1] = 1; R[:, 2, 0] = -s; R[:, 2, 2] = c
    uvz = np.einsum('ij,bpj->bpi', K1, np.einsum('bij,bpj->bpi', R, x3d) + t[:, None])
    x2d = uvz[..., :2] / uvz[..., 2:] + rng.normal(0, 1.5, (B, P, 2))
    istd = np.exp(-rng.normal(np.log(2.0), 0.5, (B, P, 2))) / 10.0
    mask = rng.random((B, P)) > 0.25
    t[1, 2] = 1.2                        # object 1: close to the camera -> some points behind z_min (both rows zero)
    t[2] = [11.5, 1.5, 10.0]             # object 2: at the right border -> u beyond u_max for part of the points (u row zero)
    t[3] = [0.0, 6.2, 10.0]              # object 3: at the lower border -> v beyond v_max for part of the points (v row zero)
    mask[4] = True                       # object 4: every point an inlier
    K = np.repeat(K1[None], B, 0)
    K[6, 0, 1] = 3.0                     # object 6: skewed camera
    u_range = np.repeat(np.array([[-200.0, 1442.0]]), B, 0)
    v_range = np.repeat(np.array([[-200.0, 575.0]]), B, 0)
    u_range[7] = [550.0, 700.0]          # object 7: tight ranges -> many clipped rows
    v_range[7] = [150.0, 220.0]
    z_min = 0.5

    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.float64)
    with torch.no_grad():
        jt, jy, jpw, jew = jac.get_jacobians(T(x2d), T(istd), T(x3d), T(K), T(u_range), T(v_range), z_min, T(yaw), T(t),
                                             torch.from_numpy(mask))
    out = dict(x2d=x2d, istd=istd, x3d=x3d, K=K, u_range=u_range, v_range=v_range, yaw=yaw, t=t, mask=mask, z_min=np.float64(z_min),
               jac_t_vec=jt.numpy(), jac_yaw=jy.numpy(), jac_pw_c3d=jpw.numpy(), jac_ew_istd=jew.numpy())
    zero_rows = (jpw.abs().sum(3) == 0).numpy()
    print('zero rows per object:', zero_rows.sum((1, 2)))
    np.savez_compressed(os.path.join(OUT, 'g13_pointwise_jacobians.npz'), **out)
    print('wrote g13_pointwise_jacobians.npz', {k: v.shape for k, v in out.items() if hasattr(v, 'shape')})


if __name__ == '__main__':
    main()
