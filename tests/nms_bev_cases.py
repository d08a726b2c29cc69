"""Named, seeded cases for the rotated-BEV NMS (nms_bev_kernel): what tests/test_gpu_nms_bev.py runs on the MI355X and what
tests/test_nms_bev_cases_cpu.py pins about them on the CPU first.

A case is a dict: groups (list of (n, 5) float32 [x1, y1, x2, y2, ry]), scores (list of (n,) float32), thrs (the thresholds it runs at),
want (None: the expectation is oracle.nms_bev's; else {thr: list of kept-index lists}, written by hand), and what the builder knows
about it (case-specific keys).  All boxes are float32, centres within +-80 m, sizes as test_consumers._rand_boxes makes them (special_boxes
adds degenerate ones on purpose).

A case judged against the oracle has NO pair whose fp64 IoU lies within KNIFE of a threshold it runs at (the CPU test asserts it), so
the kernel's fp32 IoU and the oracle's fp64 IoU decide every pair alike and the GPU test asserts equality, index for index.  The seeds
below were found by a search for that condition (SEARCH at the bottom of this file restates it: python tests/nms_bev_cases.py)."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(1, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from test_consumers import _rand_boxes  # noqa: E402
from test_rotated_overlap_cases_cpu import KNIFE, NMS_THRS  # noqa: E402

NAMES = ('every_n', 'boundaries', 'chains', 'special_scores', 'special_boxes')
EVERY_N = 130
BOUNDARY_SIZES = (0, 255, 0, 256, 0, 257, 0, 511, 0, 512, 0)
CHAIN_PLACES = (31, 32, 63, 64, 65, 480)
NAN, INF = np.float32(np.nan), np.float32(np.inf)


def _oracle():
    from oracle import oracle
    return oracle


# ------------------------------------------------------------------------------- pair IoUs -----
def near_pairs(boxes):
    """(i, j), i < j, of every pair close enough to intersect: centre distance at most the sum of the half-diagonals.  Every other
    pair has IoU exactly 0, in fp64 and in the kernel."""
    b = np.asarray(boxes, np.float64)
    c, r = 0.5 * (b[:, 0:2] + b[:, 2:4]), 0.5 * np.hypot(b[:, 2] - b[:, 0], b[:, 3] - b[:, 1])
    d = np.hypot(c[:, None, 0] - c[None, :, 0], c[:, None, 1] - c[None, :, 1])
    i, j = np.nonzero(np.triu(d <= (r[:, None] + r[None, :]) * (1 + 1e-9) + 1e-9, 1))
    return list(zip(i.tolist(), j.tolist()))


def pair_ious(boxes):
    """{(i, j): fp64 IoU} of the near pairs, in the argument order the NMS never depends on (symmetry: test_consumers.py)"""
    orc = _oracle()
    return {(i, j): orc.rotated_iou_bev(boxes[i], boxes[j]) for i, j in near_pairs(boxes)}


def knife_margin(ious, thrs):
    """the smallest | IoU - thr | over the pairs and thresholds (inf without pairs)"""
    v = np.array(list(ious.values()), np.float64)
    return min((float(np.abs(v - t).min()) for t in thrs), default=np.inf) if len(v) else np.inf


def knife_free(boxes, thrs=NMS_THRS):
    return knife_margin(pair_ious(boxes), thrs) >= KNIFE


# ------------------------------------------------------------------------------- builders ------
def _grid_scores(rng, n):
    """uniform scores; half of the boxes on a 0.05 grid, so that there are ties"""
    s = rng.uniform(0, 1, n).astype(np.float32)
    on = rng.permutation(n)[:(n + 1) // 2]
    s[on] = (rng.integers(1, 20, len(on)) * np.float32(0.05)).astype(np.float32)
    if len(on) > 1:
        s[on[1]] = s[on[0]]                                          # a tie at every size from 3 on
    return s


def _dense(seed, n, factor=1.25):
    """n boxes in a square of side 2 factor sqrt(n): at 1.25, one box to 6 m^2, so neighbours overlap and far ones do not"""
    rng = np.random.default_rng(seed)
    return _rand_boxes(rng, n, spread=min(80.0, max(1.5, factor * np.sqrt(n)))), _grid_scores(rng, n)


def _seeded(base, n, k, factor=1.25):
    return _dense(base + 1000 * k + n, n, factor)


# k-th try of the search that first left no pair within KNIFE of a threshold, per group size (0: the first try)
EVERY_N_TRIES = {8: 1, 12: 1, 15: 1, 40: 1, 49: 1, 56: 2, 64: 2, 70: 1, 79: 1, 88: 1, 90: 3, 99: 1, 107: 2, 112: 2, 113: 1, 124: 3, 126: 2, 129: 2}
BOUNDARY_TRIES = {255: 10, 257: 1, 511: 1, 512: 7}
BOUNDARY_FACTOR = {512: 1.05}      # the full group a little denser: suppression down to the late mask words at thr 0.25 too


def every_n():
    """groups of every size 1 .. 130 in one launch, dense enough that boxes are suppressed at every size from 8 on"""
    gs = [_seeded(50000, n, EVERY_N_TRIES.get(n, 0)) for n in range(1, EVERY_N + 1)]
    return dict(groups=[g for g, _ in gs], scores=[s for _, s in gs], thrs=NMS_THRS, want=None)


def boundaries():
    """the sizes around the sort's padding and the 256-thread trips, with empty groups between them and at both ends"""
    gs = [_seeded(70000, n, BOUNDARY_TRIES.get(n, 0), BOUNDARY_FACTOR.get(n, 1.25)) if n else (np.zeros((0, 5), np.float32), np.zeros(0, np.float32)) for n in BOUNDARY_SIZES]
    return dict(groups=[g for g, _ in gs], scores=[s for _, s in gs], thrs=NMS_THRS, want=None)


CHAIN_ANGLE, CHAIN_STEP = 0.3, 2.2


def _xyxyr(cx, cy, l, w, ry):
    return np.array([cx - l / 2, cy - w / 2, cx + l / 2, cy + w / 2, ry], np.float32)


def chain_triple(cx, cy):
    """A, B, C: 4 x 2 boxes at one angle, each CHAIN_STEP further along their long axis (direction (cos, -sin) in the corner convention
    x' = dx cos + dy sin, y' = -dx sin + dy cos).  Neighbours overlap by 1.8 x 2 (IoU 3.6 / 12.4 = 0.29), A and C are 0.4 apart."""
    ux, uy = np.cos(CHAIN_ANGLE) * CHAIN_STEP, -np.sin(CHAIN_ANGLE) * CHAIN_STEP
    return [_xyxyr(cx + k * ux, cy + k * uy, 4.0, 2.0, CHAIN_ANGLE) for k in (-1, 0, 1)]


def _fillers(rng, n):
    """n boxes on a 23 x 23 grid of 6.5 m cells (half-diagonals reach 2.47), the 3 x 3 cells round the origin left free"""
    cells = [(i, j) for i in range(-11, 12) for j in range(-11, 12) if max(abs(i), abs(j)) > 1]
    assert n <= len(cells)
    b = _rand_boxes(rng, n, spread=0.0)
    pick = rng.permutation(len(cells))[:n]
    for k, p in enumerate(pick):
        b[k, [0, 2]] += np.float32(6.5 * cells[p][0])
        b[k, [1, 3]] += np.float32(6.5 * cells[p][1])
    return b


def chains():
    """One group per place p of CHAIN_PLACES: a triple A > B > C in score with IoU(A, B) > thr, IoU(B, C) > thr, IoU(A, C) = 0 among
    fillers that overlap nothing; B sits at sorted place p, A before it, C after it.  B goes, and C, which only B covers, stays."""
    rng = np.random.default_rng(81)
    groups, scores, want, places = [], [], [], []
    for p in CHAIN_PLACES:
        n = 512 if p == 480 else p + 9
        pa, pc = p // 3, n - 2                                       # sorted places of A and C
        order = rng.permutation(n)                                   # order[place] = index into the group
        s = np.zeros(n, np.float32)
        s[order] = np.linspace(0.95, 0.05, n).astype(np.float32)    # distinct scores, descending along the places
        b = np.zeros((n, 5), np.float32)
        rest = np.ones(n, bool)
        rest[order[[pa, p, pc]]] = False
        b[order[[pa, p, pc]]] = chain_triple(0.0, 0.0)
        b[rest] = _fillers(rng, n - 3)
        groups.append(b)
        scores.append(s)
        want.append([int(i) for k, i in enumerate(order) if k != p])
        places.append((int(order[pa]), int(order[p]), int(order[pc]), pa, p, pc))
    return dict(groups=groups, scores=scores, thrs=NMS_THRS, want={t: want for t in NMS_THRS}, triples=places)


SPECIAL_SCORE_SIZES = (3, 5, 33, 100, 64)
SPECIAL_SCORE_TRIES = {'all_nan': 1}


def _special_score_group(n, k):
    """box 0 (finite score) covers box 1 (NaN score); box 2 (NaN) is far from everything; from n = 5 on boxes 3 and 4 (both NaN) are
    identical and far from the rest; the other boxes are a dense random crowd with +-inf among their scores"""
    rng = np.random.default_rng(90000 + 1000 * k + n)
    b, s = _dense(90500 + 1000 * k + n, n)
    b[0] = _xyxyr(-60.0, -60.0, 4.0, 2.0, 0.4)
    b[1] = _xyxyr(-59.5, -60.0, 4.0, 2.0, 0.4)
    b[2] = _xyxyr(60.0, -60.0, 3.0, 1.5, -1.0)
    s[0], s[1], s[2] = 0.5, NAN, NAN
    if n >= 5:
        b[3] = b[4] = _xyxyr(60.0, 60.0, 2.5, 1.0, 2.0)
        s[3] = s[4] = NAN
    if n > 8:
        rest = 5 + rng.permutation(n - 5)
        s[rest[0]], s[rest[1]], s[rest[2]], s[rest[3]] = INF, INF, -INF, -INF
        s[rest[4]] = NAN                                             # one NaN inside the crowd
    return b, s


def special_scores():
    """NaN and infinite scores.  Group sizes 3, 5, 33 and 100 (no power of two: the sort pads) and 64, then a crowd of 37 whose
    scores are all NaN, then one of 20 with only +-inf scores."""
    gs = [_special_score_group(n, SPECIAL_SCORE_TRIES.get(n, 0)) for n in SPECIAL_SCORE_SIZES]
    b, s = _seeded(95000, 37, SPECIAL_SCORE_TRIES.get('all_nan', 0))
    gs.append((b, np.full(37, NAN, np.float32)))
    b, s = _seeded(96000, 20, SPECIAL_SCORE_TRIES.get('inf', 0))
    gs.append((b, np.where(np.arange(20) % 3 == 0, INF, -INF).astype(np.float32)))
    return dict(groups=[g for g, _ in gs], scores=[s for _, s in gs], thrs=NMS_THRS, want=None)


def special_boxes():
    """Degenerate boxes, expectation by hand (group 0, 1) or geometric (group 2: a box with swapped coordinates is the same rectangle).

    group 0: a box with a NaN coordinate between finite ones, at the same place as box 0: kept at its score's place, suppresses nothing
             and is suppressed by nothing (every IoU with it is 0 over the 1e-8 floor).
    group 1: zero-width, zero-height and zero-area boxes on top of an ordinary one and of each other: IoU 0, all kept.
    group 2: boxes with x2 < x1, y2 < y1 or both over ordinary boxes."""
    a = _xyxyr(10.0, 5.0, 4.0, 2.0, 0.5)
    far = _xyxyr(-30.0, 20.0, 3.0, 1.0, -0.7)
    g0 = np.stack([a, a, far, a, a]).astype(np.float32)
    g0[1, 0] = NAN                                                   # x1
    g0[3, 4] = NAN                                                   # the angle
    s0 = np.array([0.9, 0.8, 0.7, 0.6, 0.5], np.float32)
    want0 = [0, 1, 2, 3]                                             # 4 is 0 again: suppressed by 0; the NaN boxes 1 and 3 stay
    zw = _xyxyr(10.0, 5.0, 0.0, 2.0, 0.5)                            # zero width, inside a
    zh = _xyxyr(10.0, 5.0, 4.0, 0.0, 0.5)                            # zero height
    pt = _xyxyr(10.0, 5.0, 0.0, 0.0, 0.5)                            # a point
    g1 = np.stack([zw, a, zw, zh, pt, pt, zh, far]).astype(np.float32)
    s1 = np.array([0.9, 0.8, 0.7, 0.6, 0.5, 0.5, 0.4, 0.3], np.float32)
    want1 = [0, 1, 2, 3, 4, 5, 6, 7]
    rng = np.random.default_rng(97)
    g2 = _rand_boxes(rng, 24, spread=4.0)
    s2 = _grid_scores(rng, 24)
    g2[0:6, [0, 2]] = g2[0:6, [2, 0]]                                # x2 < x1
    g2[6:12, [1, 3]] = g2[6:12, [3, 1]]                              # y2 < y1
    g2[12:18] = g2[12:18][:, [2, 3, 0, 1, 4]]                        # both
    return dict(groups=[g0, g1, g2], scores=[s0, s1, s2], thrs=NMS_THRS, want={t: [want0, want1, None] for t in NMS_THRS},
                swapped=(2, 18))


BUILDERS = dict(every_n=every_n, boundaries=boundaries, chains=chains, special_scores=special_scores, special_boxes=special_boxes)


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


def sorted_coords(b):
    """the same rectangles with x1 <= x2 and y1 <= y2"""
    b = np.array(b, np.float32)
    return np.stack([np.minimum(b[:, 0], b[:, 2]), np.minimum(b[:, 1], b[:, 3]), np.maximum(b[:, 0], b[:, 2]), np.maximum(b[:, 1], b[:, 3]),
                     b[:, 4]], 1)


@functools.lru_cache(maxsize=None)
def expected(name, thr):
    """kept indices per group: the hand-written ones where the case has them, oracle.nms_bev's elsewhere.  Computed once per run."""
    c, orc = case(name), _oracle()
    hand = c['want'][thr] if c['want'] is not None else [None] * len(c['groups'])
    return [np.array(h, np.int64) if h is not None else orc.nms_bev(g, s, thr) for g, s, h in zip(c['groups'], c['scores'], hand)]


def oracle_judged(name):
    """indices of the groups whose expectation is the oracle's"""
    c = case(name)
    return [i for i in range(len(c['groups'])) if c['want'] is None or c['want'][c['thrs'][0]][i] is None]


# ------------------------------------------------------------------------------- the seed search
def _search(make, ok, tries=200):
    for k in range(tries):
        if ok(*make(k)):
            return k
    raise RuntimeError('no seed found')


def SEARCH():
    """prints the tables above: per group, the first try that leaves no pair within KNIFE of a threshold (and, for every_n, has
    1 < kept < n from n = 8 on at both thresholds)"""
    orc = _oracle()

    def fine(b, s, need_kept=False):
        if not knife_free(b):
            return False
        return not need_kept or all(1 < len(orc.nms_bev(b, s, t)) < len(b) for t in NMS_THRS)
    print('EVERY_N_TRIES =', {n: k for n in range(1, EVERY_N + 1) if (k := _search(lambda k: _seeded(50000, n, k), lambda b, s: fine(b, s, n >= 8)))})
    print('BOUNDARY_TRIES =', {n: k for n in BOUNDARY_SIZES if n and (k := _search(lambda k: _seeded(70000, n, k, BOUNDARY_FACTOR.get(n, 1.25)), fine))},
          '(512: the first of these that also has 12 mask words which both suppress and are suppressed, tests/test_nms_bev_cases_cpu.py)')
    sp = {n: k for n in SPECIAL_SCORE_SIZES if (k := _search(lambda k: _special_score_group(n, k), fine))}
    for key, base, n in (('all_nan', 95000, 37), ('inf', 96000, 20)):
        if (k := _search(lambda k: _seeded(base, n, k), fine)):
            sp[key] = k
    print('SPECIAL_SCORE_TRIES =', sp)


if __name__ == '__main__':
    SEARCH()
