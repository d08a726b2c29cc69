"""numpy fp64 reference of the global head's Monte-Carlo eval forward on given dropout masks, and the magnitude
network ``Abs`` behind the tests' bound B.  The reference is the reference module's own sequence (repeat, dropout2d as a channel
mask, FC, relu, dropout, FC, relu, dropout, FC, var_mean / mean over the samples), not the factored form the kernels evaluate."""
import numpy as np

U24 = 2.0 ** -24


def params_of(head):
    """{state_dict key: fp64 array} of an FCExtractor"""
    return {k: v.detach().cpu().double().numpy() for k, v in head.state_dict().items()}


def mc_forward_ref(params, x, masks, p2d, p, absolute=False):
    """x (n, C, rh, rw); masks = keep0 (S, n, C), keep1 (S, n, F), keep2 (S, n, F) bool; p2d, p the dropout rates.
    -> dict(samples (S, n, J), mean (n, J), var (n, J) unbiased two-pass, reg_fc_out (n, F), h1, h2 (S, n, F)), all fp64.
    ``absolute``: the same network on |x|, |W|, |b| (every product and sum non-negative): the Abs of the bound B; its relu is
    the identity."""
    f = (lambda a: np.abs(np.asarray(a, np.float64))) if absolute else (lambda a: np.asarray(a, np.float64))
    keep0, keep1, keep2 = (np.asarray(m).astype(bool) for m in masks)
    S, n, C = keep0.shape
    x = f(x).reshape(n, C, -1)
    q0, q1 = 1.0 / (1.0 - p2d), 1.0 / (1.0 - p)
    w1, b1, w2, b2 = f(params['fcs.0.weight']), f(params['fcs.0.bias']), f(params['fcs.1.weight']), f(params['fcs.1.bias'])
    wr, br = f(params['fc_reg.weight']), f(params['fc_reg.bias'])
    with np.errstate(invalid='ignore'):
        xs = (x[None] * (keep0[..., None] * q0)).reshape(S * n, -1)               # sample row s * n + i
        relu = lambda v: np.where(v < 0, 0.0, v)                                  # keeps NaN, as torch's
        h1 = relu(xs @ w1.T + b1) * (keep1.reshape(S * n, -1) * q1)
        h2 = relu(h1 @ w2.T + b2) * (keep2.reshape(S * n, -1) * q1)
        y = (h2 @ wr.T + br).reshape(S, n, -1)
        mean = y.mean(0)
        var = ((y - mean) ** 2).sum(0) / (S - 1)
    h2 = h2.reshape(S, n, -1)
    return dict(samples=y, mean=mean, var=var, reg_fc_out=h2.mean(0), h1=h1.reshape(S, n, -1), h2=h2)


def bound(params, x, masks, p2d, p):
    """B per element of ``samples`` and of ``reg_fc_out``: 2 (A + C + 2F + 16) 2^-24 Abs, the running-error bound of fp32 sums in any
    order through the three layers (relu is 1-Lipschitz; the 16 covers the bias adds, the scales and the roundings)."""
    a = mc_forward_ref(params, x, masks, p2d, p, absolute=True)
    C = np.asarray(masks[0]).shape[2]
    A = int(np.prod(np.asarray(x).shape[2:]))
    F = params['fcs.1.weight'].shape[0]
    g = 2.0 * (A + C + 2 * F + 16) * U24
    return dict(samples=g * a['samples'], reg_fc_out=g * a['reg_fc_out'])


def stats_of_samples(samples):
    """fp64 mean and two-pass unbiased variance over axis 0 of the (fp32) samples a kernel returned"""
    y = np.asarray(samples, np.float64)
    mean = y.mean(0)
    return mean, ((y - mean) ** 2).sum(0) / (y.shape[0] - 1)


def ulp32(v):
    """the spacing of fp32 at |v| (of the smallest normal below it)"""
    return np.spacing(np.maximum(np.abs(np.asarray(v, np.float64)), 2.0 ** -126).astype(np.float32)).astype(np.float64)
