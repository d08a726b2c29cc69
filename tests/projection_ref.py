"""numpy restatements of the NOC head's training kernels, for the tests.

``project``: the projection in float32 in the kernel's operation order — sin / cos of yaw in float64 rounded to float32, P_R = K @ R
and P_t = K @ t, every three-term dot product summed left to right, IEEE division, clamps and min that propagate NaN — so the
kernel's output must equal it bit for bit.

``robust_kl``: the loss with the specified exp (oracle.spec_expf), the per-element values in float32 and the sums in float64, the
buffer update in torch's float32 steps.  The kernel's sums run in another order, so the loss agrees to rounding, not bitwise.
"""
import numpy as np

from oracle import oracle as orc

f32 = np.float32


def project(coords_3d, pose, cam_intrinsic, img_shapes, z_min=0.5, allowed_border=200):
    c3d = np.asarray(coords_3d, f32)
    pose, K, img = np.asarray(pose, f32), np.asarray(cam_intrinsic, f32), np.asarray(img_shapes, f32)
    yaw = pose[:, 3].astype(np.float64)
    s, c = np.sin(yaw).astype(f32), np.cos(yaw).astype(f32)
    z, o = np.zeros_like(c), np.ones_like(c)
    R = np.stack([c, z, s, z, o, z, -s, z, c], 1).reshape(-1, 3, 3)
    with np.errstate(all='ignore'):
        PR = np.empty_like(R)
        Pt = np.empty((len(pose), 3), f32)
        for i in range(3):
            for j in range(3):
                PR[:, i, j] = K[:, i, 0] * R[:, 0, j] + K[:, i, 1] * R[:, 1, j] + K[:, i, 2] * R[:, 2, j]
            Pt[:, i] = K[:, i, 0] * pose[:, 0] + K[:, i, 1] * pose[:, 1] + K[:, i, 2] * pose[:, 2]
        X, Y, Z = c3d[:, 0], c3d[:, 1], c3d[:, 2]
        e = lambda a: a[:, None, None]
        p = [e(PR[:, i, 0]) * X + e(PR[:, i, 1]) * Y + e(PR[:, i, 2]) * Z + e(Pt[:, i]) for i in range(3)]
        zc = np.where(p[2] < f32(z_min), f32(z_min), p[2])
        out = np.empty((len(pose), 2) + c3d.shape[2:], f32)
        for ch, hi in ((0, img[:, 1] + f32(allowed_border)), (1, img[:, 0] + f32(allowed_border))):
            uv = p[ch] / zc
            uv = np.where(uv < f32(-allowed_border), f32(-allowed_border), uv)
            out[:, ch] = np.where(np.isnan(uv) | (uv < e(hi)), uv, e(hi))
    return out


def robust_kl(pred, logstd, buf, target=0, delta=1.414, eps=1e-4, momentum=0.1, training=True, reduction='mean', loss_weight=1.0):
    """-> (loss, new buffer, c, raw (float32 per element)) as the two-launch forward computes them."""
    x, ls = np.asarray(pred, f32), np.asarray(logstd, f32)
    with np.errstate(all='ignore'):
        e = orc.spec_expf(-ls)
        inv = np.where(e > f32(1 / eps), f32(1 / eps), e)
        diff = x if target == -1 else np.abs(x)
        dw = diff * inv
        raw = np.where(dw < f32(delta), f32(0.5) * (dw * dw), f32(delta) * (dw - f32(0.5 * delta))) + ls
    m = f32(buf)
    if training:
        avg = f32(inv.astype(np.float64).sum() / inv.size)
        m = f32(m * f32(1 - momentum))
        m = f32(m + f32(momentum) * avg)
    c = m if not m < f32(1e-6) else f32(1e-6)
    s = raw.astype(np.float64).sum() / np.float64(c)
    if reduction == 'mean':
        s = s / raw.size
    return f32(f32(loss_weight) * f32(s)), m, c, raw
