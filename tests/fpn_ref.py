"""The feature pyramid's top-down pathway (include/monorun_fpn.h) restated in numpy fp32, forward and backward, in exactly
the orders the header states: every operation a float32 one rounded on its own.  Shared by tests/test_fpn_cpu.py and
tests/test_gpu_fpn.py; results are cached per case and must not be modified."""
import functools

import numpy as np

f32 = np.float32

# the pyramids of the GPU tests: [(H_l, W_l)], finest first.  The last one is outside the header's rule (7 > 2 * 3).
PYRAMIDS = {
    'pow2': [(8, 8), (4, 4), (2, 2), (1, 1)],
    'ceil_odd': [(13, 7), (7, 4), (4, 2), (2, 1)],
    'wide': [(12, 70), (6, 35), (3, 18), (2, 9)],
    'one_level': [(3, 1)],
    'two_levels': [(5, 9), (3, 5)],
    'tall_six': [(40, 3), (20, 2), (10, 1), (5, 1), (3, 1), (2, 1)],
    'outside_rule': [(7, 5), (3, 2), (3, 2), (1, 1)],
}
SHAPES = [(n, c) for n in (1, 2) for c in (1, 5, 40)]       # (N, C): C is no multiple of any channel chunk


def in_rule(sizes):
    return all(b <= a <= 2 * b for s, t in zip(sizes[:-1], sizes[1:]) for a, b in zip(s, t))


def nearest_index(n_out, n_in):
    """iy of the header for every y < n_out: the pixel of the coarser level (n_in of them) that y reads"""
    r = f32(n_in) / f32(n_out)
    i = np.floor(np.arange(n_out, dtype=f32) * r).astype(np.int64)
    return np.minimum(i, n_in - 1)


def bilinear_taps(n_in):
    """i0, i1, l0, l1 of the x2 rule along an axis of n_in pixels"""
    Y = np.arange(2 * n_in, dtype=f32)
    src = np.maximum((Y + f32(0.5)) * f32(0.5) - f32(0.5), f32(0))
    i0 = src.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(f32)
    return i0, i1, f32(1) - l1, l1


def forward(lats, lower_scale):
    """(m, low): the merged maps (m[L-1] is lats[L-1]) and the x2 map or None"""
    assert lower_scale in (0, 2) and all(t.dtype == f32 for t in lats)
    m = [None] * len(lats)
    m[-1] = lats[-1]
    for l in range(len(lats) - 2, -1, -1):
        iy = nearest_index(lats[l].shape[2], lats[l + 1].shape[2])
        ix = nearest_index(lats[l].shape[3], lats[l + 1].shape[3])
        m[l] = lats[l] + m[l + 1][:, :, iy[:, None], ix[None, :]]
    low = None
    if lower_scale:
        i0y, i1y, l0y, l1y = bilinear_taps(m[0].shape[2])
        i0x, i1x, l0x, l1x = bilinear_taps(m[0].shape[3])
        a, b = m[0][:, :, i0y[:, None], i0x[None, :]], m[0][:, :, i0y[:, None], i1x[None, :]]
        c, d = m[0][:, :, i1y[:, None], i0x[None, :]], m[0][:, :, i1y[:, None], i1x[None, :]]
        low = l0y[:, None] * (l0x * a + l1x * b) + l1y[:, None] * (l0x * c + l1x * d)
        assert low.dtype == f32
    return m, low


def _read_weight(n_in, Y, y):
    """the weight with which row Y of low reads row y: the sum of the forward's l0 / l1 whose tap is y (0 for a Y outside the map)"""
    i0, i1, l0, l1 = bilinear_taps(n_in)
    ok = (Y >= 0) & (Y < 2 * n_in)
    Yc = np.clip(Y, 0, 2 * n_in - 1)
    w = np.where(i0[Yc] == y, l0[Yc], f32(0)) + np.where(i1[Yc] == y, l1[Yc], f32(0))
    return np.where(ok, w, f32(0)).astype(f32), Yc


def bilinear_transpose(g_low, H, W):
    """B of the header: per pixel of m[0] the terms (wy wx) g over the low pixels that read it with a weight that is not zero, Y outer, X
    inner, ascending, into an accumulator that starts at 0.  Candidates: 2y - 2 .. 2y + 3 (wider than any reader)."""
    acc = np.zeros(g_low.shape[:2] + (H, W), dtype=f32)
    ys, xs = np.arange(H), np.arange(W)
    for j in range(-2, 4):
        wy, Yc = _read_weight(H, 2 * ys + j, ys)
        for i in range(-2, 4):
            wx, Xc = _read_weight(W, 2 * xs + i, xs)
            w = wy[:, None] * wx[None, :]
            term = w * g_low[:, :, Yc[:, None], Xc[None, :]]
            acc = np.where(w != 0, acc + term, acc)
    assert acc.dtype == f32
    return acc


def children_sum(G, H, W):
    """S of the header: per pixel of a level (H, W) the row-major running sum from 0 of G (the finer level) over its children"""
    iy, ix = nearest_index(G.shape[2], H), nearest_index(G.shape[3], W)
    rows = [np.nonzero(iy == p)[0] for p in range(H)]
    cols = [np.nonzero(ix == p)[0] for p in range(W)]
    for group in rows + cols:
        assert len(group) == 0 or np.array_equal(group, np.arange(group[0], group[0] + len(group))), 'the children are contiguous'
    S = np.zeros(G.shape[:2] + (H, W), dtype=f32)
    for a in range(max(len(r) for r in rows)):
        py = np.array([p for p in range(H) if len(rows[p]) > a], dtype=np.int64)
        cy = np.array([rows[p][a] for p in py], dtype=np.int64)
        for b in range(max(len(c) for c in cols)):
            px = np.array([p for p in range(W) if len(cols[p]) > b], dtype=np.int64)
            cx = np.array([cols[p][b] for p in px], dtype=np.int64)
            S[:, :, py[:, None], px[None, :]] += G[:, :, cy[:, None], cx[None, :]]
    return S


def backward(sizes, shape, lower_scale, g_m, g_low):
    """grad_lat of the header from g_m (a list with None for a missing gradient) and g_low (or None)"""
    N, C = shape
    G = []
    for l, (H, W) in enumerate(sizes):
        g = g_m[l] if g_m[l] is not None else np.zeros((N, C, H, W), dtype=f32)
        if l == 0:
            if lower_scale:
                gl = g_low if g_low is not None else np.zeros((N, C, 2 * H, 2 * W), dtype=f32)
                g = g + bilinear_transpose(gl, H, W)
        else:
            g = g + children_sum(G[l - 1], H, W)
        assert g.dtype == f32
        G.append(g)
    return G


def make_inputs(name, shape, integer=False, seed=0):
    """laterals, gradients to every merged level and to low, fp32: normal, or integers in [-64, 64] (every result is then exact)"""
    sizes = PYRAMIDS[name]
    rng = np.random.RandomState(seed + 17 * len(sizes) + shape[1])

    def draw(h, w):
        if integer:
            return rng.randint(-64, 65, size=shape + (h, w)).astype(f32)
        return (rng.standard_normal(shape + (h, w)) * 3).astype(f32)
    lats = [draw(h, w) for h, w in sizes]
    g_m = [draw(h, w) for h, w in sizes]
    g_low = draw(2 * sizes[0][0], 2 * sizes[0][1])
    return lats, g_m, g_low


@functools.lru_cache(maxsize=None)
def case(name, shape, lower_scale, integer=False):
    """everything of one case, computed once: dict(lats, g_m, g_low, m, low, grads)"""
    sizes = PYRAMIDS[name]
    lats, g_m, g_low = make_inputs(name, shape, integer)
    m, low = forward(lats, lower_scale)
    grads = backward(sizes, shape, lower_scale, g_m, g_low if lower_scale else None)
    out = dict(sizes=sizes, lats=lats, g_m=g_m, g_low=g_low if lower_scale else None, m=m, low=low, grads=grads)
    for v in out.values():
        for t in (v if isinstance(v, list) else [v]):
            if isinstance(t, np.ndarray):
                t.setflags(write=False)
    return out
