"""A numpy restatement of the covariance stage's summation tree (csrc/pnp_kernel_body.inc stage 4, block_sum_packed<WPO, 10>), independent
of the oracle's C (orc_cov_hessian_spec / orc_tree_sum): thread q % (64 waves) accumulates the q-th inlier, each wave's 64 partials combine
by the butterfly with strides 32, 16, 1, 2, 4, 8, the waves' totals add up in wave order."""
from fractions import Fraction

import numpy as np

STRIDES = (32, 16, 1, 2, 4, 8)


def tree64(p, strides=STRIDES):
    """(64, ...) -> (...): the in-wave butterfly."""
    p = np.array(p, np.float64, copy=True)
    lane = np.arange(64)
    for s in strides:
        p = p + p[lane ^ s]
    return p[0]


def tree_sum(part, waves, strides=STRIDES):
    """(64 waves, n) per-thread partials -> (n,) totals."""
    part = np.asarray(part, np.float64)
    assert part.shape[0] == 64 * waves
    acc = tree64(part[:64], strides)
    for w in range(1, waves):
        acc = acc + tree64(part[64 * w:64 * (w + 1)], strides)
    return acc


def fma(a, b, c):
    """Correctly rounded a * b + c (exact rational arithmetic; float(Fraction) rounds to nearest)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def cov_partials(K, z_min, u_range, v_range, sn, cs, t, x3d, istd, inlier, waves):
    """Per-thread partials (64 waves, 10) of J^T J's upper triangle as stage 4 forms them: no contraction, one IEEE division per point,
    acc = fma(Ju_i, Ju_j, fma(Jv_i, Jv_j, acc)).  sn, cs: the specified sin / cos of the float32 yaw."""
    K = np.asarray(K, np.float64).reshape(9)
    tx, ty, tz = (float(v) for v in np.asarray(t, np.float64).reshape(3))
    kr, kt = [0.0] * 9, [0.0] * 3
    for r in range(3):
        kr[3 * r + 0] = K[3 * r + 0] * cs - K[3 * r + 2] * sn
        kr[3 * r + 1] = K[3 * r + 1]
        kr[3 * r + 2] = K[3 * r + 0] * sn + K[3 * r + 2] * cs
        kt[r] = K[3 * r + 0] * tx + K[3 * r + 1] * ty + K[3 * r + 2] * tz
    m1 = (K[0] * (-sn) + K[2] * (-cs), K[0] * cs + K[2] * (-sn), K[3] * (-sn) + K[5] * (-cs), K[3] * cs + K[5] * (-sn))
    ur, vr = [float(v) for v in np.ravel(u_range)], [float(v) for v in np.ravel(v_range)]
    part = np.zeros((64 * waves, 10))
    q = 0
    for i in range(x3d.shape[0]):
        if inlier is not None and not inlier[i]:
            continue
        X, Y, Z = (float(v) for v in x3d[i])
        un = ((kr[0] * X + kr[1] * Y) + kr[2] * Z) + kt[0]
        vn = ((kr[3] * X + kr[4] * Y) + kr[5] * Z) + kt[1]
        z = ((kr[6] * X + kr[7] * Y) + kr[8] * Z) + kt[2]
        zclip = z < z_min
        z = z_min if zclip else z
        iz = 1.0 / z
        uv = [un * iz, vn * iz]
        cl = [uv[0] < ur[0] or uv[0] > ur[1], uv[1] < vr[0] or uv[1] > vr[1]]
        uv = [max(ur[0], min(ur[1], uv[0])), max(vr[0], min(vr[1], uv[1]))]
        J = [0.0] * 8
        for r in range(2):
            if zclip or cl[r]:
                continue
            w = float(istd[i, r]) * iz
            J[4 * r + 0] = w * ((m1[2 * r] + uv[r] * cs) * X + (m1[2 * r + 1] + uv[r] * sn) * Z)
            J[4 * r + 1] = w * K[3 * r + 0]
            J[4 * r + 2] = w * K[3 * r + 1]
            J[4 * r + 3] = w * (K[3 * r + 2] - uv[r])
        acc = part[q % (64 * waves)]
        k = 0
        for a in range(4):
            for b in range(a, 4):
                acc[k] = fma(J[a], J[b], fma(J[4 + a], J[4 + b], float(acc[k])))
                k += 1
        q += 1
    return part


def cov_hessian(K, z_min, u_range, v_range, sn, cs, t, x3d, istd, inlier, waves):
    """(4, 4) J^T J as stage 4 specifies it for `waves` waves per object."""
    tot = tree_sum(cov_partials(K, z_min, u_range, v_range, sn, cs, t, x3d, istd, inlier, waves), waves)
    H = np.zeros((4, 4))
    k = 0
    for a in range(4):
        for b in range(a, 4):
            H[a, b] = H[b, a] = tot[k]
            k += 1
    return H
