"""Pairs of BEV boxes with known intersection areas for the one rotated-rectangle routine of the library (edge_inside_area_t,
csrc/kitti_eval_kernel.inc) and its three consumers: the KITTI evaluator's overlaps, the aligned 3-D IoU and the rotated-BEV NMS
(tests/test_rotated_overlap_cases_cpu.py, tests/test_gpu_rotated_overlap_edges.py).  numpy only.

A box is [cx, cy, dx, dy, angle] in the evaluator's convention (oracle.kitti_eval._corners).  Every value is exact in float32, and
so are cx -+ dx/2 and cy -+ dy/2 (centres on a 1/16 grid, sizes on a 1/8 grid), so that the evaluator's rows, the 3-D IoU's rows and
the NMS's [x1, y1, x2, y2, angle] rows all describe the same rectangles bit for bit (but for the classes of ``TURNED``, whose centres
are turned off the grid).

``classes()`` -> {name: Case}; a Case holds ``a``, ``b`` (SIZE, 5) float32, ``area`` (SIZE,) float64 — the expected intersection: the
closed form where ``closed`` is set, oracle.kitti_eval.rotated_intersection in fp64 elsewhere — and ``kind``:
  'identical'  a and b are the same bits: the intersection is the box, the IoU is 1
  'touching'   the interiors are disjoint and the boundaries meet on exact coordinates: the intersection is exactly 0
  'loose'      touching pairs turned by a common angle: the corners coincide no longer bit for bit, so the area is only known to be
               at most LOOSE * min(area a, area b)
  'general'    everything else.
Every class exists in both argument orders (``<name>`` and ``<name>_swapped``): the routine treats its first box's boundary as
closed and its second's as open, so it is not symmetric in its arguments.  Cases are cached: treat them as read-only."""
import collections
import functools
import zlib

import numpy as np

from oracle import kitti_eval as ke

SIZE = 64
LOOSE = 1e-5
Case = collections.namedtuple('Case', 'a b area closed kind')
PI = float(np.float32(np.pi))
HALF_PI = float(np.float32(np.pi / 2))


def _boxes(rng, n, spread=20.0):
    """Random boxes: centres on a 1/16 grid in +-spread, sizes on a 1/8 grid in [0.5, 4.5], any angle."""
    c = np.round(rng.uniform(-spread, spread, (n, 2)) * 16) / 16
    d = np.round(rng.uniform(0.5, 4.5, (n, 2)) * 8) / 8
    return np.concatenate([c, d, rng.uniform(-np.pi, np.pi, (n, 1))], 1).astype(np.float32).astype(np.float64)


def _near(rng, a, shift=1.5):
    """For each box of a, a box of its own size class close to it: random nearby pairs."""
    b = _boxes(rng, len(a))
    b[:, :2] = a[:, :2] + np.round(rng.uniform(-shift, shift, (len(a), 2)) * 16) / 16
    return b


def _ints(rng, n, lo, hi):
    return rng.integers(lo, hi + 1, n).astype(np.float64)


def _axis_pairs(rng, what):
    """Axis-aligned pairs on small integers (angle 0).  Returns a, b, closed-form area."""
    n = SIZE
    k, m = _ints(rng, n, -6, 6), _ints(rng, n, -6, 6)
    w, h = 2 * _ints(rng, n, 1, 3), _ints(rng, n, 1, 4)            # a: even width, any height; half sizes on the 1/2 grid
    z = np.zeros(n)
    a = np.stack([k, m, w, h, z], 1)
    vertical = rng.integers(0, 2, n).astype(bool)                    # the neighbour sits above instead of to the right
    if what == 'edge_full':                                          # b shares a whole edge of a: same length of that side
        w2, h2 = 2 * _ints(rng, n, 1, 3), _ints(rng, n, 1, 4)
        b = np.where(vertical[:, None], np.stack([k, m + h / 2 + h2 / 2, w, h2, z], 1), np.stack([k + w / 2 + w2 / 2, m, w2, h, z], 1))
        area = z
    elif what == 'edge_part':                                        # b is shifted along the shared line by half of that side
        b = np.where(vertical[:, None], np.stack([k + w / 2, m + h, w, h, z], 1), np.stack([k + w, m + h / 2, w, h, z], 1))
        area = z
    elif what == 'corner':                                           # one common corner
        sx, sy = rng.choice([-1.0, 1.0], n), rng.choice([-1.0, 1.0], n)
        w2, h2 = 2 * _ints(rng, n, 1, 3), _ints(rng, n, 1, 4)
        b = np.stack([k + sx * (w + w2) / 2, m + sy * (h + h2) / 2, w2, h2, z], 1)
        area = z
    elif what == 'inside_one_edge':                                  # b inside a, its right edge on a's right edge
        a[:, 2:4] = np.stack([w + 4, h + 2], 1)
        b = np.stack([k + (w + 4) / 2 - w / 4, m, w / 2, h, z], 1)
        area = w / 2 * h
    elif what == 'inside_two_edges':                                 # b inside a with a common corner
        sx, sy = rng.choice([-1.0, 1.0], n), rng.choice([-1.0, 1.0], n)
        a[:, 2:4] = np.stack([w + 2, h + 1], 1)
        b = np.stack([k + sx * ((w + 2) / 2 - w / 4), m + sy * ((h + 1) / 2 - h / 4), w / 2, h / 2, z], 1)
        area = w * h / 4
    elif what == 'half_overlap':                                     # the same box shifted by half of one side
        b = np.where(vertical[:, None], np.stack([k, m + h / 2, w, h, z], 1), np.stack([k + w / 2, m, w, h, z], 1))
        area = w * h / 2
    else:
        raise ValueError(what)
    return a, b, area


def _turn(box, theta):
    """The boxes turned about the origin by theta in the convention of the corners (x' = c x + s y, y' = -s x + c y)."""
    c, s = np.cos(theta), np.sin(theta)
    out = box.copy()
    out[:, 0], out[:, 1] = c * box[:, 0] + s * box[:, 1], -s * box[:, 0] + c * box[:, 1]
    out[:, 4] = box[:, 4] + theta
    return out.astype(np.float32).astype(np.float64)


def _make(name, rng):
    """(a, b, closed-form area or None, kind) of one class."""
    n = SIZE
    if name == 'identical_random':
        a = _boxes(rng, n)
        return a, a.copy(), a[:, 2] * a[:, 3], 'identical'
    if name == 'identical_axis':
        a = _boxes(rng, n)
        a[:, 4] = np.array([0.0, HALF_PI, PI, -HALF_PI])[np.arange(n) % 4]
        return a, a.copy(), a[:, 2] * a[:, 3], 'identical'
    if name == 'angle_plus_pi':
        a = _boxes(rng, n)
        a[:, 4] = np.float32(a[:, 4] / 2)                            # |angle| <= pi/2: angle + pi stays of its size
        b = a.copy()
        b[:, 4] = np.float32(a[:, 4] + np.pi)
        return a, b, None, 'general'
    if name == 'swapped_dims_half_pi':
        a = _boxes(rng, n)
        b = a[:, [0, 1, 3, 2, 4]].copy()
        b[:, 4] = np.float32(a[:, 4] + np.pi / 2)
        return a, b, None, 'general'
    if name in ('touch_edge_full', 'touch_edge_part', 'touch_corner'):
        a, b, area = _axis_pairs(rng, name[len('touch_'):])
        return a, b, area, 'touching'
    if name == 'touch_rotated':
        parts = [_axis_pairs(rng, w) for w in ('edge_full', 'edge_part', 'corner')]
        pick = np.arange(n) % 3
        a = np.stack([parts[pick[i]][0][i] for i in range(n)])
        b = np.stack([parts[pick[i]][1][i] for i in range(n)])
        theta = rng.uniform(-np.pi, np.pi, n)
        return _turn(a, theta), _turn(b, theta), None, 'loose'
    if name in ('inside_one_edge', 'inside_two_edges', 'half_overlap'):
        a, b, area = _axis_pairs(rng, name)
        return a, b, area, 'general'
    if name == 'inside_rotated':                                     # shared edges that coincide to float32 rounding only
        parts = [_axis_pairs(rng, w) for w in ('inside_one_edge', 'inside_two_edges')]
        a = np.stack([parts[i % 2][0][i] for i in range(n)])
        b = np.stack([parts[i % 2][1][i] for i in range(n)])
        theta = rng.uniform(-np.pi, np.pi, n)
        return _turn(a, theta), _turn(b, theta), None, 'general'
    if name == 'concentric_shared_lines':                            # same centre, angle and one size: two edges of each box lie on
        a = _boxes(rng, n)                                           # the lines of the other's, to the rounding of the corners only
        b = _boxes(rng, n)
        b[:, :2], b[:, 4] = a[:, :2], a[:, 4]
        k = 2 + np.arange(n) % 2
        b[np.arange(n), k] = a[np.arange(n), k]
        b[np.arange(n), 5 - k] = a[np.arange(n), 5 - k] + rng.choice([-1.0, 1.0], n) * np.round(rng.uniform(0.125, 0.4, n) * 8) / 8
        return a, b, np.minimum(a[:, 2], b[:, 2]) * np.minimum(a[:, 3], b[:, 3]), 'general'
    if name == 'concentric':
        a = _boxes(rng, n)
        b = _boxes(rng, n)
        b[:, :2] = a[:, :2]
        same = np.arange(n) % 2 == 0                                 # even pairs: the same angle, so the overlap is a rectangle
        b[same, 4] = a[same, 4]
        area = np.where(same, np.minimum(a[:, 2], b[:, 2]) * np.minimum(a[:, 3], b[:, 3]), np.nan)
        return a, b, area, 'general'
    if name in ('angle_1e-4', 'angle_1e-7'):
        a = _boxes(rng, n)
        b = a.copy()
        b[:, 4] = np.float32(a[:, 4] + float(name[len('angle_'):]))
        return a, b, None, 'general'
    if name == 'zero_dim':
        a = _boxes(rng, n)
        b = _near(rng, a, 1.0)
        b[np.arange(n), 2 + np.arange(n) % 2] = 0.0
        return a, b, np.zeros(n), 'general'
    if name == 'negative_dim':                                       # area -b.dx*b.dy <= 4.5 against a's >= 9: no union near 0
        a = _boxes(rng, n)
        a[:, 2:4] = np.round(rng.uniform(3.0, 4.5, (n, 2)) * 8) / 8
        b = _near(rng, a, 1.0)
        b[:, 2:4] = np.round(rng.uniform(0.5, 2.0, (n, 2)) * 8) / 8
        b[np.arange(n), 2 + np.arange(n) % 2] *= -1
        return a, b, None, 'general'
    if name == 'far_centres':
        a = _boxes(rng, n)
        b = _near(rng, a)
        off = rng.choice([-1.0, 1.0], (n, 2)) * _ints(rng, 2 * n, 900, 1100).reshape(n, 2)
        a[:, :2] += off
        b[:, :2] += off
        return a, b, None, 'general'
    if name == 'disjoint':
        a = _boxes(rng, n)
        b = _boxes(rng, n)
        phi = rng.uniform(0, 2 * np.pi, n)                           # centres 7 apart at least; the diagonals reach 3.2 each at most
        b[:, :2] = a[:, :2] + np.round(np.stack([np.cos(phi), np.sin(phi)], 1) * rng.uniform(7, 12, (n, 1)) * 16) / 16
        return a, b, np.zeros(n), 'general'
    if name == 'random_nearby':
        a = _boxes(rng, n)
        return a, _near(rng, a), None, 'general'
    raise ValueError(name)


BASE = ('identical_random', 'identical_axis', 'angle_plus_pi', 'swapped_dims_half_pi', 'touch_edge_full', 'touch_edge_part', 'touch_corner',
        'touch_rotated', 'inside_one_edge', 'inside_two_edges', 'inside_rotated', 'half_overlap', 'concentric', 'concentric_shared_lines', 'angle_1e-4', 'angle_1e-7', 'zero_dim',
        'negative_dim', 'far_centres', 'disjoint', 'random_nearby')
TURNED = ('touch_rotated', 'inside_rotated')        # centres off the grid: the NMS's x1 ... y2 are rounded, its rectangles move by an ulp
NAMES = tuple(n + s for n in BASE for s in ('', '_swapped'))


@functools.lru_cache(maxsize=None)
def classes(seed=0):
    out = {}
    for name in BASE:
        a, b, area, kind = _make(name, np.random.default_rng([seed, zlib.crc32(name.encode())]))       # a class keeps its pairs when others are added
        a32, b32 = a.astype(np.float32), b.astype(np.float32)
        assert np.array_equal(a32, a) and np.array_equal(b32, b), name                      # exact in float32 ...
        for x in (a32, b32) if name not in TURNED else ():                                  # ... and so are the NMS's x1, y1, x2, y2
            lo, hi = x[:, :2] - x[:, 2:4] / 2, x[:, :2] + x[:, 2:4] / 2
            assert np.array_equal(lo.astype(np.float64), x[:, :2].astype(np.float64) - x[:, 2:4].astype(np.float64) / 2), name
            assert np.array_equal(hi.astype(np.float64), x[:, :2].astype(np.float64) + x[:, 2:4].astype(np.float64) / 2), name
        orc = np.array([ke.rotated_intersection(a[i], b[i]) for i in range(SIZE)])
        closed = np.zeros(SIZE, bool) if area is None else ~np.isnan(area)
        want = np.where(closed, np.zeros(SIZE) if area is None else np.nan_to_num(area), orc)
        for arr in (a32, b32, want, closed):
            arr.setflags(write=False)
        out[name] = Case(a32, b32, want, closed, kind)
        out[name + '_swapped'] = Case(b32, a32, want, closed, kind)
    return out


def oracle_area(case):
    """oracle.kitti_eval.rotated_intersection of every pair of a case, fp64, in the case's argument order."""
    return np.array([ke.rotated_intersection(case.a[i].astype(np.float64), case.b[i].astype(np.float64)) for i in range(len(case.a))])


def box_area(x):
    return np.abs(x[:, 2].astype(np.float64) * x[:, 3].astype(np.float64))


def expected_iou(case):
    """IoU of the rectangles from the fp64 area, with the NMS's union: |area a| + |area b| - intersection, at least 1e-8."""
    return case.area / np.maximum(box_area(case.a) + box_area(case.b) - case.area, 1e-8)


def xyxyr(x):
    """[cx, cy, dx, dy, angle] -> the NMS's [x1, y1, x2, y2, angle], float32 (exact)."""
    return np.concatenate([x[:, :2] - x[:, 2:4] / 2, x[:, :2] + x[:, 2:4] / 2, x[:, 4:5]], 1).astype(np.float32)


def rows7(x, y=1.5, h=1.5):
    """-> the 3-D IoU's rows [x, y, z, l, h, w, ry] with one height and one bottom for all: BEV plane (x, z), sizes (l, w)."""
    n = len(x)
    return np.stack([x[:, 0], np.full(n, y, np.float32), x[:, 1], x[:, 2], np.full(n, h, np.float32), x[:, 3], x[:, 4]], 1).astype(np.float32)


def annos(x, y=1.5, h=1.5, score=None):
    """-> one KITTI annotation dict per box (an image each): the box as a 'Car' with bottom y and height h."""
    out = []
    for i in range(len(x)):
        out.append(dict(name=np.array(['Car']), truncated=np.zeros(1, np.float32), occluded=np.zeros(1, np.float32), alpha=np.zeros(1, np.float32),
                        bbox=np.array([[100.0, 100.0, 200.0, 200.0]], np.float32), dimensions=np.array([[x[i, 2], h, x[i, 3]]], np.float32),
                        location=np.array([[x[i, 0], y, x[i, 1]]], np.float32), rotation_y=np.array([x[i, 4]], np.float32),
                        score=np.full(1, 0.5 if score is None else score[i], np.float32)))
    return out
