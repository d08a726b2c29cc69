"""The backbone's fused batch norm (include/monorun_backbone.h) restated in numpy fp32, forward and backward, in exactly the
orders the header states: every operation a float32 one rounded on its own, the two per-channel sums in the header's three steps.  Shared
by tests/test_resnet_cpu.py and tests/test_gpu_resnet.py; results are cached per case and must not be modified."""
import functools

import numpy as np

f32 = np.float32
THREADS, CHUNK, FINAL_THREADS = 256, 4096, 64          # MR_BN_THREADS, MR_BN_CHUNK, MR_BN_FINAL_THREADS


def chain_depth(n_images, hw):
    """D of the header: the longest chain of additions of a per-channel sum"""
    partials = n_images * (-(-hw // CHUNK))
    return (2 + 4 * (CHUNK // (4 * THREADS))) + 6 + 4 + -(-partials // FINAL_THREADS) + 6


def per_channel(v):
    return v.reshape(1, -1, 1, 1)


def istd_of(var, eps):
    return (f32(1) / np.sqrt(var + f32(eps))).astype(f32)


def forward(x, mean, var, weight=None, bias=None, eps=1e-5, r=None, relu=True):
    assert x.dtype == f32 and mean.dtype == f32 and var.dtype == f32
    u = (x - per_channel(mean)) * per_channel(istd_of(var, eps))
    if weight is not None:
        u = u * per_channel(weight)
    if bias is not None:
        u = u + per_channel(bias)
    if r is not None:
        u = u + r
    if relu:
        u = np.where(u <= 0, f32(0), u)
    assert u.dtype == f32
    return u


def butterfly(a):
    """a[..., i] = a[..., i] + a[..., i ^ d] for d = 32 .. 1 over the last axis of 64"""
    idx = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        a = a + a[..., idx ^ d]
    return a


def chunk_partial(terms, f0):
    """steps 1 and 2 of the header on the fp32 terms of one chunk whose first element has the index f0 in the tensor"""
    n = terms.size
    head = min((4 - f0 % 4) % 4, n)
    groups = (n - head) // 4
    acc = np.zeros(THREADS, f32)
    acc[:head] = acc[:head] + terms[:head]
    body = terms[head:head + 4 * groups].reshape(groups, 4)
    for first in range(0, groups, THREADS):
        rows = body[first:first + THREADS]
        for i in range(4):
            acc[:rows.shape[0]] = acc[:rows.shape[0]] + rows[:, i]
    tail = terms[head + 4 * groups:]
    acc[:tail.size] = acc[:tail.size] + tail
    waves = butterfly(acc.reshape(THREADS // 64, 64))[:, 0]
    total = f32(0)
    for w in waves:
        total = f32(total + w)
    return total


def channel_sums(terms):
    """the header's order on terms (N, C, H, W) fp32 -> (C,) fp32"""
    N, C, H, W = terms.shape
    hw = H * W
    flat = terms.reshape(N, C, hw)
    cpp = -(-hw // CHUNK)
    out = np.zeros(C, f32)
    for c in range(C):
        parts = np.array([chunk_partial(flat[n, c, k * CHUNK:(k + 1) * CHUNK], (n * C + c) * hw + k * CHUNK)
                          for n in range(N) for k in range(cpp)], f32)
        acc = np.zeros(FINAL_THREADS, f32)
        for first in range(0, parts.size, FINAL_THREADS):
            row = parts[first:first + FINAL_THREADS]
            acc[:row.size] = acc[:row.size] + row
        out[c] = butterfly(acc)[0]
    return out


def backward(g, y, x, mean, var, weight=None, eps=1e-5, relu=True, sums=True):
    """(grad_x, grad_r, grad_weight, grad_bias, the fp32 terms of grad_weight); the sums in the header's order (None without `sums`)"""
    gm = np.where(y <= 0, f32(0), g) if relu else g
    istd = istd_of(var, eps)
    k = istd * weight if weight is not None else istd
    gx = gm * per_channel(k)
    xhat = (x - per_channel(mean)) * per_channel(istd)
    terms = gm * xhat
    assert gx.dtype == f32 and terms.dtype == f32
    return gx, gm, (channel_sums(terms) if sums else None), (channel_sums(gm) if sums else None), terms


def maxpool(y):
    """max_pool2d(y, 3, 2, 1) in the header's visit order: dy outer, dx inner, padding skipped, m = (v > m || v != v) ? v : m from -inf"""
    N, C, H, W = y.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    m = np.full((N, C, Ho, Wo), -np.inf, f32)
    oy, ox = np.arange(Ho)[:, None], np.arange(Wo)[None, :]
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            iy, ix = 2 * oy + dy, 2 * ox + dx
            ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
            v = y[:, :, np.clip(iy, 0, H - 1), np.clip(ix, 0, W - 1)]
            with np.errstate(invalid='ignore'):
                m = np.where(ok & ((v > m) | (v != v)), v, m)
    return m


# the shapes of the GPU tests: (N, C, H, W).  Planes 1 x 1, 1 x 3, 5 x 7, 16 x 16 and an odd one of more than two chunks; C in {1, 3, 70}.
PLANES = [(1, 1), (1, 3), (5, 7), (16, 16), (91, 93)]
SHAPES = [(n, c) + p for p in PLANES for n, c in ((1, 1), (2, 3), (1, 70))] + [(2, 70, 5, 7), (2, 1, 91, 93)]
SHAPES.remove((1, 70, 91, 93))          # 70 channels of the large plane add nothing the other two do not show


@functools.lru_cache(maxsize=None)
def case(shape, exact=False, residual=True, relu=True, affine=True, seed=0):
    """inputs, the definition's outputs and gradients on one shape.  exact: integers in [-8, 8], var in {0.25, 1, 4}, eps = 0 — istd is a
    power of two and every order of every operation is exact"""
    N, C, H, W = shape
    rng = np.random.default_rng([seed, N, C, H, W, int(exact)])
    if exact:
        integers = lambda s: rng.integers(-8, 9, s).astype(f32)
        x, g, r = integers(shape), integers(shape), integers(shape)
        mean, weight, bias = integers(C), integers(C), integers(C)
        var, eps = rng.choice(np.array([0.25, 1.0, 4.0], f32), C), 0.0
    else:
        normal = lambda s: rng.standard_normal(s).astype(f32)
        x, g, r = normal(shape) * f32(2) + f32(0.5), normal(shape), normal(shape)
        mean, weight, bias = normal(C), normal(C) + f32(1), normal(C)
        var, eps = (rng.random(C).astype(f32) + f32(0.1)) * f32(3), 1e-5
    c = dict(shape=shape, x=x, g=g, r=r if residual else None, mean=mean, var=var, weight=weight if affine else None,
             bias=bias if affine else None, eps=eps, relu=relu)
    c['y'] = forward(x, mean, var, c['weight'], c['bias'], eps, c['r'], relu)
    c['gx'], c['gr'], c['gw'], c['gb'], c['terms'] = backward(g, c['y'], x, mean, var, c['weight'], eps, relu)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def stem_case(shape, exact=False, seed=1):
    c = dict(case(shape, exact, False, True, True, seed))
    c['p'] = maxpool(c['y'])
    c['p'].setflags(write=False)
    return c
