"""Reference of the fused score-head launch for the tests: the formula of ``mr_score_head_forward`` (include/monorun_heads.h) in numpy
float64, and the magnitude bound its parity tolerance is derived from.

``score_head_ref`` returns, per row, the exact logit z and A, the same network evaluated on absolute values — |parameters|, |inputs|,
(|x| + |mean|) * |scale| + |shift| for the norm, + |reg_fc_out|, and no ReLU.  Every fp32 product and sum the kernel forms is
bounded by the matching partial of A, so a sum of fp32 terms in ANY order carries an error of at most (number of operations) * 2^-24
of it (the standard running-error bound); ReLU is 1-Lipschitz and passes the error through.  ``tolerance`` is

    2 * (17 + c1 + c2 + 16) * 2^-24 * A

— 17, c1 and c2 are the lengths of the three sums, 16 counts the remaining roundings (the gather's subtraction and scale, the fp32
scale itself, biases, the skip connection, the final partial sums), and the factor 2 covers the second-order terms.

The scale of the norm is part of the formula as an fp32 value (it is computed once, in fp32, when the parameters are packed), so it is
formed here in numpy float32 before everything moves to float64.
"""
import numpy as np


def params_of(head):
    """The parameters of a monorun_amd MLPScoreHead in the fused configuration, as float32 numpy arrays."""
    g = lambda t: t.detach().cpu().numpy().astype(np.float32)
    p = dict(W1=g(head.pose_fcs[0].weight), b1=g(head.pose_fcs[0].bias), W2=g(head.fused_fcs[0].weight), b2=g(head.fused_fcs[0].bias),
             w3=g(head.fc_out.weight).reshape(-1), b3=g(head.fc_out.bias).reshape(()))
    if head.use_pose_norm:
        n = head.pose_norm
        p.update(mean=g(n.running_mean), var=g(n.running_var), eps=n.eps, weight=g(n.weight), bias=g(n.bias))
    return p


def inputs_x(yaw, t_vec, pose_cov, dimensions):
    r, c = np.tril_indices(4)                     # row-major over the lower triangle: torch.tril_indices(4, 4) order
    return np.concatenate([yaw.reshape(-1, 1), t_vec, pose_cov.reshape(-1, 4, 4)[:, r, c], dimensions], axis=1)


def score_head_ref(p, reg_fc_out, yaw, t_vec, pose_cov, dimensions):
    """(z, A): (n,) float64 each."""
    f64 = lambda a: np.asarray(a, np.float64)
    x = f64(inputs_x(yaw, t_vec, pose_cov, dimensions))
    if 'mean' in p:
        scale = f64(np.float32(p['weight']) / np.sqrt(np.float32(p['var']) + np.float32(p['eps'])))
        mean, shift = f64(p['mean']), f64(p['bias'])
    else:
        scale, mean, shift = np.ones(17), np.zeros(17), np.zeros(17)
    W1, b1, W2, b2, w3, b3 = (f64(p[k]) for k in ('W1', 'b1', 'W2', 'b2', 'w3', 'b3'))
    with np.errstate(all='ignore'):
        xn = (x - mean) * scale + shift
        h1 = np.maximum(xn @ W1.T + b1, 0) + f64(reg_fc_out)
        h2 = np.maximum(h1 @ W2.T + b2, 0)
        z = h2 @ w3 + b3
        xa = (np.abs(x) + np.abs(mean)) * np.abs(scale) + np.abs(shift)
        h1a = xa @ np.abs(W1).T + np.abs(b1) + np.abs(f64(reg_fc_out))
        h2a = h1a @ np.abs(W2).T + np.abs(b2)
        A = h2a @ np.abs(w3) + np.abs(b3)
    return z, A


def tolerance(A, c1, c2):
    return 2.0 * (17 + c1 + c2 + 16) * 2.0 ** -24 * A
