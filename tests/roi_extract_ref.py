"""The multi-level RoI extraction of DESIGN.md §18 in numpy, straight from its definition, with the analytic gradient to the maps and,
alongside every number, the sum of the absolute values of the terms it is a sum of: the unit of the tests' error bound.

The GEOMETRY is part of the definition and is fp32 (every operation rounded as the kernels round it): the level rule, the degenerate
rule, the sample coordinates and the bilinear weights ly, lx, hy = 1 - ly, hx = 1 - lx.  Given those fp32 numbers, the pooling is exact
arithmetic, evaluated here in fp64:

    out[k, c, ph, pw]        = sum over the bin's samples (iy, ix), not dead, of
                               (hy hx F[y_lo, x_lo] + hy lx F[y_lo, x_hi] + ly hx F[y_hi, x_lo] + ly lx F[y_hi, x_hi]) / count
    grad_feats[l][n, c, y, x] = sum over the RoIs k of level l and image n, their bins and samples whose tap reads (y, x) of
                               weight grad_out[k, c, ph, pw] / count

with F = feats[level_k][image_k, c].  Weights and the dead rule are separable (dead = dead_y or dead_x), so per RoI the sums are two small
matrices: Ay (oh, H) and Ax (ow, W), out = Ay F Ax^T / count.

The bound: |got - ref| <= C_BOUND * 2^-23 * (that element's sum of absolute terms).
"""
import numpy as np

# The constant of the bound.  Measured on the CPU: roi_extract_torch evaluated in fp32 on CASES, its error against this module over the
# unit 2^-23 * (sum of absolute terms); the largest ratio over all cases is 1.65 for the forward and 1.70 for grad_feats
# (tests/test_roi_extract_cpu.py prints and checks them).  C_MEASURED is the larger; the margin of 4 covers the kernels' other summation
# order (DESIGN.md section 14's margin).
C_MEASURED = 1.70
C_BOUND = 4 * C_MEASURED
EPS32 = 2.0 ** -23
f32 = np.float32

IMAGE = (48, 80)                                   # H, W in pixels
STRIDES = (2, 4, 8, 16, 32)                        # maps of 24x40, 12x20, 6x10, 3x5, 2x3
FINEST = 8.0                                       # level 0 below a scale of 16 px, 1 below 32, 2 below 64, 3 below 128, else 4
N_IMAGES = 2


def level_sizes(L):
    return [(-(-IMAGE[0] // s), -(-IMAGE[1] // s)) for s in STRIDES[:L]]


# [image, x1, y1, x2, y2]; the comments give the level at L = 5
_ROIS = [
    (0, 20.3, 10.7, 44.9, 30.1),            # interior, level 1; a sub-pixel bin at 7x7 and 14x14 (a grid of 1)
    (0, -0.4, -0.6, 11.0, 9.0),             # crosses the top and left border by less than a pixel of level 0: clamped taps
    (1, 69.0, 38.5, 81.0, 49.2),            # ... the bottom and right border
    (0, -12.0, -10.0, 6.0, 8.0),            # crosses the top and left border by more than a pixel of level 1: dead samples
    (1, 60.0, 30.0, 100.0, 70.0),           # ... the bottom and right border, level 2
    (0, 200.0, 200.0, 240.0, 240.0),        # fully outside the map, level 2: zeros
    (1, 30.0, 20.0, 30.0, 20.0),            # zero area: no sample aligned (count = max(0, 1)), one per bin unaligned
    (1, 30.0, 2.0, 34.0, 46.0),             # tall, level 0: a grid of 4 in y at 7x7, 2 at 14x14
    (0, 1.0, 20.0, 79.0, 23.0),             # wide, level 0: a grid of 6 in x at 7x7, 3 at 14x14
    (0, 8.0, 8.0, 24.0, 24.0),              # a scale of exactly finest 2^1: level 1
    (0, 0.0, -10.0, 64.0, 54.0),            # exactly finest 2^3: level 3
    (0, 20.3, 10.7, 44.9, 30.1),            # identical to the first
    (0, 24.0, 14.0, 47.0, 33.0),            # overlaps it on level 1
    (1, -40.0, -30.0, 60.0, 50.0),          # level 3 (scale 89), mostly outside the 3x5 map
    (0, 40.0, -236.0, 40.4, 284.0),         # level 0, 260 map pixels tall: 14 x 19 samples in y, more than the forward's LDS table holds
    (1, -220.0, 20.0, 300.0, 20.25),        # level 0, 260 map pixels wide: 7 x 38 (14 x 19) samples in x, more than the table holds
    # ordinary proposals inside the image, levels 0 to 3
    (0, 5.0, 5.0, 17.0, 15.0),
    (0, 50.0, 30.0, 62.0, 41.0),
    (0, 10.0, 20.0, 30.0, 44.0),
    (0, 40.0, 5.0, 70.0, 25.0),
    (0, 2.0, 3.0, 50.0, 40.0),
    (0, 30.0, 8.0, 78.0, 46.0),
    (0, -5.0, -5.0, 75.0, 50.0),
    (0, 20.0, 10.0, 60.0, 28.0),
    (1, 12.0, 6.0, 40.0, 30.0),
    (1, 55.0, 12.0, 66.0, 24.0),
    # degenerate, one of each kind: zeros out, no gradient
    (0, float('nan'), 1.0, 5.0, 5.0),
    (1, 0.0, 0.0, float('inf'), 10.0),
    (2, 10.0, 10.0, 30.0, 30.0),            # image index outside [0, N)
    (-1, 10.0, 10.0, 30.0, 30.0),
    (float('nan'), 10.0, 10.0, 30.0, 30.0),
    (0, -1e4, -1e4, 1e4, 1e4),              # a sample grid beyond the map's size + 2 (at sampling_ratio 0)
    (1, -1e30, -1e30, 1e30, 1e30),          # its area overflows: the level rule sees inf
]
_LEVEL4 = (1, -150.0, -150.0, 250.0, 200.0)        # level 4 (scale 374): a grid of 2 on the 2x3 map


def _rows(rois, seed):
    """the rows in mixed level and image order"""
    r = np.asarray(rois, dtype=f32).reshape(-1, 5)
    return r[np.random.default_rng(seed).permutation(r.shape[0])]


def _case(name, C, L, size, sampling_ratio, aligned, rois):
    return dict(name=name, C=C, L=L, size=size, sampling_ratio=sampling_ratio, aligned=aligned, rois=rois)


# the main list leaves level 4 without a RoI; 'one_image' leaves image 1 without one and uses level 4
CASES = [
    _case('c5_L5_7x7', 5, 5, (7, 7), 0, True, _rows(_ROIS, 1)),
    _case('c33_L5_14x14', 33, 5, (14, 14), 0, True, _rows(_ROIS, 2)),
    _case('c1_L2_2x3', 1, 2, (2, 3), 0, True, _rows(_ROIS, 3)),
    _case('c5_L1_7x7_sr2', 5, 1, (7, 7), 2, True, _rows(_ROIS, 4)),
    _case('c5_L5_7x7_unaligned', 5, 5, (7, 7), 0, False, _rows(_ROIS, 5)),
    _case('c33_L2_14x14_sr2_unaligned', 33, 2, (14, 14), 2, False, _rows(_ROIS, 6)),
    _case('c5_L5_7x7_one_image', 5, 5, (7, 7), 0, True, _rows([r for r in _ROIS + [_LEVEL4] if r[0] != 1] + [(0,) + _LEVEL4[1:]], 7)),
    _case('c5_L5_7x7_no_rois', 5, 5, (7, 7), 0, True, np.zeros((0, 5), f32)),
]
IDS = [c['name'] for c in CASES]


def make_inputs(case, seed=1818):
    """Seeded (feats, grad_out) in fp32: maps at scale 1 with some exact zeros"""
    rng = np.random.default_rng([seed, CASES.index(case) if case in CASES else 99])
    feats = []
    for H, W in level_sizes(case['L']):
        x = rng.normal(0, 1, (N_IMAGES, case['C'], H, W)).astype(f32)
        x[rng.random(x.shape) < 0.1] = 0.0
        feats.append(x)
    go = rng.normal(0, 1, (case['rois'].shape[0], case['C']) + tuple(case['size'])).astype(f32)
    return feats, go


def roi_levels(rois, L, finest=FINEST):
    """rule 1 in fp32: the number of i in 1 .. L-1 with v >= 2^i (a NaN v: none)"""
    r = np.asarray(rois, f32)
    with np.errstate(all='ignore'):
        v = np.sqrt((r[:, 3] - r[:, 1]) * (r[:, 4] - r[:, 2])) / f32(finest) + f32(1e-6)
        return sum((v >= f32(2.0 ** i)).astype(np.int64) for i in range(1, L)) if L > 1 else np.zeros(r.shape[0], np.int64)


def _geom(roi, stride, size, sampling_ratio, aligned):
    """the per-RoI terms in fp32: (sw, sh, rw, rh) on the level's map"""
    scale = f32(1.0) / f32(stride)
    off = f32(0.5 if aligned else 0.0)
    with np.errstate(all='ignore'):
        x1, y1, x2, y2 = (f32(v) * scale for v in roi[1:])
        sw, sh = f32(x1 - off), f32(y1 - off)
        rw, rh = f32(f32(x2 - off) - sw), f32(f32(y2 - off) - sh)
    if not aligned:
        rw, rh = max(rw, f32(1.0)), max(rh, f32(1.0))
    return sw, sh, rw, rh


def roi_valid(roi, level_hw, stride, n_images, size, sampling_ratio, aligned):
    """rule 3: False for a degenerate RoI"""
    if not np.all(np.isfinite(roi)) or not (roi[0] > -1.0 and roi[0] < n_images):
        return False
    if sampling_ratio <= 0:
        _, _, rw, rh = _geom(roi, stride, size, sampling_ratio, aligned)
        with np.errstate(all='ignore'):
            if np.ceil(f32(rh / f32(size[0]))) > f32(level_hw[0] + 2) or np.ceil(f32(rw / f32(size[1]))) > f32(level_hw[1] + 2):
                return False
    return True


def _axis_matrix(start, extent, n_bins, n_map, sampling_ratio):
    """A (n_bins, n_map) fp64: the weight each bin's samples give to each map row / column; and the grid.  fp32 geometry."""
    b = f32(extent / f32(n_bins))
    g = int(sampling_ratio) if sampling_ratio > 0 else int(np.ceil(b))
    A = np.zeros((n_bins, n_map))
    for p in range(n_bins):
        for i in range(g):
            v = f32(f32(start + f32(f32(p) * b)) + f32(f32(f32(f32(i) + f32(0.5)) * b) / f32(g)))
            if v < f32(-1.0) or v > f32(n_map):
                continue
            if v <= 0:
                v = f32(0.0)
            lo = int(v)
            if lo >= n_map - 1:
                hi = lo = n_map - 1
                v = f32(lo)
            else:
                hi = lo + 1
            l = f32(v - f32(lo))
            h = f32(f32(1.0) - l)
            A[p, lo] += float(h)
            A[p, hi] += float(l)
    return A, g


def extract(case, feats, go=None):
    """(out, its sums of absolute terms, [grad_feats], [their sums of absolute terms]) in fp64; the gradients when go is given"""
    rois, L, size, sr, aligned = case['rois'], case['L'], case['size'], case['sampling_ratio'], case['aligned']
    sizes = level_sizes(L)
    K, C = rois.shape[0], case['C']
    f64 = [np.asarray(f, np.float64) for f in feats]
    out, outa = np.zeros((K, C) + tuple(size)), np.zeros((K, C) + tuple(size))
    grads, gradsa = [np.zeros(f.shape) for f in f64], [np.zeros(f.shape) for f in f64]
    levels = roi_levels(rois, L)
    for k in range(K):
        l = int(levels[k])
        if not roi_valid(rois[k], sizes[l], STRIDES[l], N_IMAGES, size, sr, aligned):
            continue
        n = int(rois[k, 0])
        sw, sh, rw, rh = _geom(rois[k], STRIDES[l], size, sr, aligned)
        Ay, gh = _axis_matrix(sh, rh, size[0], sizes[l][0], sr)
        Ax, gw = _axis_matrix(sw, rw, size[1], sizes[l][1], sr)
        count = float(max(gh * gw, 1))
        out[k] = np.einsum('py,cyx,qx->cpq', Ay, f64[l][n], Ax) / count
        outa[k] = np.einsum('py,cyx,qx->cpq', Ay, np.abs(f64[l][n]), Ax) / count
        if go is not None:
            g = np.asarray(go[k], np.float64)
            grads[l][n] += np.einsum('py,cpq,qx->cyx', Ay, g, Ax) / count
            gradsa[l][n] += np.einsum('py,cpq,qx->cyx', Ay, np.abs(g), Ax) / count
    return out, outa, grads, gradsa


def ratio(got, ref, unit):
    """the largest |got - ref| / (2^-23 unit) over the elements; an element with unit 0 must be exact"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    assert np.all(err[unit == 0] == 0), 'an element that is a sum of zeros is not zero'
    return float((err[unit > 0] / (EPS32 * unit[unit > 0])).max()) if (unit > 0).any() else 0.0
