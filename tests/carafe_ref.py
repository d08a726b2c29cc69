"""The CARAFE op of DESIGN.md §17 in numpy fp64, straight from its definition, with the analytic gradients and, alongside every
number, the sum of the absolute values of the terms it is a sum of (its conditioning term): the unit of the tests' error bound.

    l_t            = m[n, (g k^2 + t) s^2 + (ph % s) s + pw % s, ph // s, pw // s]           t = iy k + ix, g = c // (C / G)
    w_t            = softmax_t(l_t)
    out[n,c,ph,pw] = sum_t x[n, c, ph // s + iy - r, pw // s + ix - r] w_t                   r = (k - 1) / 2, zero outside the map

    grad_x[n,c,y,x]      = sum over (ph, pw, t) whose tap t reads (y, x) of grad_out[n,c,ph,pw] w_t
    gw_t[n,g,ph,pw]      = sum_{c in g} grad_out[n,c,ph,pw] x[n, c, window t]
    grad_l_t             = w_t (gw_t - sum_u w_u gw_u),          grad_m = grad_l at l's place in m

The bound: |got - ref| <= C_BOUND * 2^-23 * (that element's sum of absolute terms).
"""
import numpy as np

# The constant of the bound.  Measured on the CPU: carafe_pack_torch evaluated in fp32 on the inputs of SHAPES (make_inputs: seed 1717,
# logits at scale 3, features at scale 1 with exact zeros), its error against this module over the unit 2^-23 * (sum of absolute terms);
# the largest ratio over all shapes is 5.36 for the forward, 2.87 for grad_x and 10.02 for grad_m (tests/test_carafe_cpu.py prints them).
# C_MEASURED is the largest of the three; the margin of 4 covers the kernel's other summation order and exp (a few ulps per term each,
# DESIGN.md section 14's margin).
C_MEASURED = 10.02
C_BOUND = 4 * C_MEASURED
EPS32 = 2.0 ** -23

CHUNK = 32          # monorun_amd.carafe.CHUNK: channels the kernels stage at a time
# (N, C, H, W, k, G, s): each the smallest shape that exercises one way the kernel can be wrong
SHAPES = [
    (1, 1, 1, 1, 5, 1, 2),              # every tap but the centre is out of bounds
    (2, 6, 2, 3, 5, 1, 2),              # the window is larger than the map, H != W
    (3, 6, 3, 5, 3, 2, 2),              # groups
    (3, 6, 3, 5, 5, 3, 1),              # groups, s = 1
    (2, CHUNK + 3, 5, 4, 5, 1, 2),      # a ragged last channel chunk
    (2, 8, 3, 3, 7, 1, 4),              # the largest kernel and scale
    (2, 256, 14, 14, 5, 1, 2),          # the workload's tile
]


def make_inputs(shape, seed=1717):
    """Seeded (x, m, grad_out) in fp32: logits at scale 3 (a peaked but finite softmax), features at scale 1 with some exact zeros."""
    N, C, H, W, k, G, s = shape
    rng = np.random.default_rng([seed, *shape])
    x = rng.normal(0, 1, (N, C, H, W)).astype(np.float32)
    x[rng.random(x.shape) < 0.1] = 0.0
    m = rng.normal(0, 3, (N, G * k * k * s * s, H, W)).astype(np.float32)
    go = rng.normal(0, 1, (N, C, H * s, W * s)).astype(np.float32)
    return x, m, go


def shuffled_logits(m, k, G, s):
    """pixel_shuffle(m, s) as (N, G, k^2, H s, W s)"""
    N, _, H, W = m.shape
    l = m.reshape(N, G * k * k, s, s, H, W).transpose(0, 1, 4, 2, 5, 3)
    return l.reshape(N, G, k * k, H * s, W * s)


def unshuffle(gl, k, G, s):
    """the inverse: (N, G, k^2, H s, W s) -> m's layout (N, G k^2 s^2, H, W)"""
    N, _, _, HO, WO = gl.shape
    H, W = HO // s, WO // s
    g = gl.reshape(N, G * k * k, H, s, W, s).transpose(0, 1, 3, 5, 2, 4)
    return g.reshape(N, G * k * k * s * s, H, W)


def softmax(l, axis):
    e = np.exp(l - l.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def windows(x, k, s):
    """xw[n, c, t, ph, pw] = x[n, c, ph // s + iy - r, pw // s + ix - r], zero outside the map"""
    N, C, H, W = x.shape
    r = (k - 1) // 2
    xp = np.zeros((N, C, H + k - 1, W + k - 1), x.dtype)
    xp[:, :, r:r + H, r:r + W] = x
    xw = np.empty((N, C, k * k, H * s, W * s), x.dtype)
    for t in range(k * k):
        iy, ix = divmod(t, k)
        xw[:, :, t] = np.repeat(np.repeat(xp[:, :, iy:iy + H, ix:ix + W], s, axis=2), s, axis=3)
    return xw


def forward(x, m, k, G, s):
    """(out, sum_t |w_t x_t|) in fp64"""
    x, m = np.asarray(x, np.float64), np.asarray(m, np.float64)
    N, C, H, W = x.shape
    w = np.repeat(softmax(shuffled_logits(m, k, G, s), 2), C // G, axis=1)          # (N, C, k^2, HO, WO)
    terms = windows(x, k, s) * w
    return terms.sum(2), np.abs(terms).sum(2)


def backward(x, m, go, k, G, s):
    """(grad_x, its sum of absolute terms, grad_m, its sum of absolute terms) in fp64.  grad_m's terms are those of the softmax backward
    as it is stated and computed, w_t gw_t - sum_u w_t w_u gw_u: the products w_t grad_out[c] x[c, window t] and
    w_t w_u grad_out[c] x[c, window u] over c and u.  (Folding the u = t term into w_t (1 - w_t) first would make the unit vanish where
    the softmax is peaked, w_t -> 1, while gw_t and the dot product are each rounded before they cancel.)"""
    x, m, go = (np.asarray(a, np.float64) for a in (x, m, go))
    N, C, H, W = x.shape
    Cg, r = C // G, (k - 1) // 2
    w = softmax(shuffled_logits(m, k, G, s), 2)                                      # (N, G, k^2, HO, WO)
    wc = np.repeat(w, Cg, axis=1)                                                    # (N, C, k^2, HO, WO)
    # grad_x: each output pixel's term go * w_t lands on its window's source pixel; summed at source resolution over the s^2 sub-positions
    gx = np.zeros((N, C, H + k - 1, W + k - 1))
    gxa = np.zeros_like(gx)
    for t in range(k * k):
        iy, ix = divmod(t, k)
        p = (go * wc[:, :, t]).reshape(N, C, H, s, W, s)
        gx[:, :, iy:iy + H, ix:ix + W] += p.sum((3, 5))
        gxa[:, :, iy:iy + H, ix:ix + W] += np.abs(p).sum((3, 5))
    gx, gxa = gx[:, :, r:r + H, r:r + W], gxa[:, :, r:r + H, r:r + W]
    # grad_w and the softmax backward
    prod = (windows(x, k, s) * go[:, :, None]).reshape(N, G, Cg, k * k, H * s, W * s)
    gw, gwa = prod.sum(2), np.abs(prod).sum(2)                                       # (N, G, k^2, HO, WO)
    gl = w * (gw - (w * gw).sum(2, keepdims=True))
    gla = w * (gwa + (w * gwa).sum(2, keepdims=True))                                # |w_t gw_t| + sum_u |w_t w_u gw_u|, term by term
    return gx, gxa, unshuffle(gl, k, G, s), unshuffle(gla, k, G, s)


def ratio(got, ref, unit):
    """the largest |got - ref| / (2^-23 unit) over the elements; an element with unit 0 must be exact"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    assert np.all(err[unit == 0] == 0), 'an element that is a sum of zeros is not zero'
    return float((err[unit > 0] / (EPS32 * unit[unit > 0])).max()) if (unit > 0).any() else 0.0
