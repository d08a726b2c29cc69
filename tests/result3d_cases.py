"""Named, seeded cases for the one-launch result tail (result3d_nms_kernel, monorun_amd.consumers.result_3d_nms): what
tests/test_gpu_result3d.py runs on the MI355X and what tests/test_result3d_cases_cpu.py pins about them on the CPU first.

A case is a dict of the kernel's inputs as numpy arrays — dimensions (N, 3), yaw (N, 1), t_vec (N, 3), scores (N,), det_bboxes (N, 5)
float32, labels (N,) int64 — with C (num_classes), thrs, sizes (members per class) and hand ({class: kept local indices} where the
expectation is written by hand, as tests/nms_bev_cases.py does for its degenerate boxes).  The classes' BEV boxes come from the
builders of tests/nms_bev_cases.py and tests/test_consumers._rand_boxes; a row carries them as [x, z, l, w, ry], so the box the NMS
sees is the one consumers.xywhr2xyxyr REBUILDS from the row in float32, within an ulp of the builder's.

The expectation is consumers.get_bbox_3d_result on the host plus oracle.nms_bev in fp64 on the rebuilt boxes.  A class judged against
the oracle has NO pair whose fp64 IoU lies within KNIFE of a threshold it runs at (the CPU test asserts it), so the kernel's fp32 IoU and
the oracle's decide every pair alike and the GPU test asserts equality, index for index.  The tries below were found by a search for
that condition (SEARCH at the bottom restates it: python tests/result3d_cases.py)."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(1, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nms_bev_cases as nc  # noqa: E402
from test_rotated_overlap_cases_cpu import KNIFE, NMS_THRS  # noqa: E402

THRS = tuple(sorted(set(NMS_THRS) | {0.01}))
MAX_N, MAX_C = 512, 16                       # MR_RESULT3D_MAX_N, MR_RESULT3D_MAX_CLASSES

# name: (C, members per class, rows that belong to no class)
SIZED = {
    'c16_small': (16, (0, 1, 2, 31, 32, 33, 63, 64, 65, 0, 1, 2, 0, 5, 0, 0), 10),
    'c3_255_0_257': (3, (255, 0, 257), 0),
    'c3_256_1_240': (3, (256, 1, 240), 15),
    'c1_257': (1, (257,), 3),
    'c1_all_512': (1, (512,), 0),
}
NAMES = tuple(SIZED) + ('special_scores', 'special_boxes')
BASE = {name: 110000 + 10000 * i for i, name in enumerate(SIZED)}
FACTOR = {512: 1.05}                         # the full class a little denser, as nms_bev_cases does
# per case, {class: the first try of the search that leaves no pair of the rebuilt boxes within KNIFE of a threshold} (0: the first try)
TRIES = {
    'c16_small': {4: 1, 7: 1},
    'c3_255_0_257': {0: 1},
    'c3_256_1_240': {0: 2},
    'c1_257': {},
    'c1_all_512': {0: 3},
}
SPECIAL_SCORE_TRIES = {}                     # group of nms_bev_cases.special_scores -> try, where its own try does not survive the rebuild
# kept per class at each threshold, pinned: a case cannot silently degenerate to "everything kept"
KEPT = {
    'c16_small': {0.01: [0, 1, 2, 20, 14, 14, 32, 34, 28, 0, 1, 2, 0, 2, 0, 0], 0.25: [0, 1, 2, 28, 27, 26, 55, 55, 56, 0, 1, 2, 0, 5, 0, 0]},
    'c3_255_0_257': {0.01: [119, 0, 121], 0.25: [211, 0, 223]},
    'c3_256_1_240': {0.01: [122, 1, 112], 0.25: [228, 1, 207]},
    'c1_257': {0.01: [124], 0.25: [221]},
    'c1_all_512': {0.01: [202], 0.25: [427]},
    'special_scores': {0.01: [2, 3, 19, 51, 33, 17, 9, 0], 0.25: [2, 3, 26, 87, 53, 30, 17, 0]},
    'special_boxes': {0.01: [4, 8, 10], 0.25: [4, 8, 15]},
}


def _oracle():
    from oracle import oracle
    return oracle


def rows_of(boxes, scores, rng):
    """(n, 8) [l, h, w, x, y, z, ry, score] rows whose BEV box is `boxes` ([x1, y1, x2, y2, ry]) up to the rounding of the rebuild"""
    b = np.asarray(boxes, np.float32)
    r = np.zeros((len(b), 8), np.float32)
    r[:, 0], r[:, 2] = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]                              # l, w
    r[:, 1], r[:, 4] = rng.uniform(1.2, 2.0, len(b)), rng.uniform(0.8, 1.8, len(b))      # h, y
    r[:, 3], r[:, 5] = (b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2                  # x, z
    r[:, 6], r[:, 7] = b[:, 4], scores
    return r


def rebuilt(rows):
    """the [x1, y1, x2, y2, ry] boxes of (n, 8) rows, in the rows' float32: what consumers.xywhr2xyxyr gives the NMS"""
    return _oracle().xywhr2xyxyr(np.asarray(rows, np.float32)[:, [3, 5, 0, 2, 6]])


def _class_group(name, c, n, k):
    b, s = nc._seeded(BASE[name] + 100 * c, n, k, FACTOR.get(n, 1.25))
    if n >= 8:
        s[np.random.default_rng(BASE[name] + c).permutation(n)[:max(2, n // 10)]] = 0.0          # failed solves: score 0, tied
    return b, s


def _assemble(C, groups, outsiders, seed, hand=None):
    """rows of the classes' (boxes, scores), interleaved by a seeded permutation that keeps each class's order, plus `outsiders` rows
    labelled -1 and C alternately"""
    rng = np.random.default_rng(seed)
    rows = [rows_of(b, s, rng) for b, s in groups]
    out_b, out_s = nc._dense(seed + 1, outsiders, 1.25) if outsiders else (np.zeros((0, 5), np.float32), np.zeros(0, np.float32))
    rows.append(rows_of(out_b, out_s, rng))
    block_labels = [np.full(len(r), c, np.int64) for c, r in enumerate(rows[:-1])] + [np.where(np.arange(outsiders) % 2 == 0, -1, C).astype(np.int64)]
    blocks = rng.permutation(np.concatenate([np.full(len(r), g) for g, r in enumerate(rows)]))      # row p takes the next row of block blocks[p]
    out, final, taken = np.zeros((len(blocks), 8), np.float32), np.zeros(len(blocks), np.int64), [0] * len(rows)
    for p, g in enumerate(blocks):
        out[p], final[p] = rows[g][taken[g]], block_labels[g][taken[g]]
        taken[g] += 1
    N = len(final)
    assert N <= MAX_N and C <= MAX_C
    det = np.concatenate([rng.uniform(0, 300, (N, 2)), rng.uniform(300, 600, (N, 2)), rng.uniform(0, 1, (N, 1))], 1).astype(np.float32)
    return dict(C=C, dimensions=np.ascontiguousarray(out[:, 0:3]), yaw=np.ascontiguousarray(out[:, 6:7]), t_vec=np.ascontiguousarray(out[:, 3:6]),
                scores=np.ascontiguousarray(out[:, 7]), labels=final, det_bboxes=det, thrs=THRS, sizes=tuple(len(b) for b, _ in groups),
                hand=hand or {})


def _sized(name):
    C, sizes, outsiders = SIZED[name]
    groups = [_class_group(name, c, n, TRIES[name].get(c, 0)) if n else (np.zeros((0, 5), np.float32), np.zeros(0, np.float32))
              for c, n in enumerate(sizes)]
    return _assemble(C, groups, outsiders, BASE[name] + 7)


def _special_scores():
    """the NaN- and infinite-score groups of nms_bev_cases.special_scores as seven classes, and an empty eighth"""
    groups = []
    for g, n in enumerate(nc.SPECIAL_SCORE_SIZES):
        groups.append(nc._special_score_group(n, SPECIAL_SCORE_TRIES.get(g, nc.SPECIAL_SCORE_TRIES.get(n, 0))))
    b, _ = nc._seeded(95000, 37, SPECIAL_SCORE_TRIES.get(5, nc.SPECIAL_SCORE_TRIES.get('all_nan', 0)))
    groups.append((b, np.full(37, nc.NAN, np.float32)))
    b, _ = nc._seeded(96000, 20, SPECIAL_SCORE_TRIES.get(6, nc.SPECIAL_SCORE_TRIES.get('inf', 0)))
    groups.append((b, np.where(np.arange(20) % 3 == 0, nc.INF, -nc.INF).astype(np.float32)))
    groups.append((np.zeros((0, 5), np.float32), np.zeros(0, np.float32)))
    return _assemble(8, groups, 4, 170007)


def _special_boxes():
    """nms_bev_cases.special_boxes' three groups as classes: NaN coordinates, zero-area boxes (both by hand) and swapped coordinates"""
    c = nc.case('special_boxes')
    want = c['want'][NMS_THRS[0]]
    assert all(c['want'][t][:2] == want[:2] for t in NMS_THRS)
    return _assemble(3, list(zip(c['groups'], c['scores'])), 2, 180007, hand={0: want[0], 1: want[1]})


@functools.lru_cache(maxsize=None)
def case(name):
    return _sized(name) if name in SIZED else dict(special_scores=_special_scores, special_boxes=_special_boxes)[name]()


@functools.lru_cache(maxsize=None)
def class_rows(name):
    """per class (rows (n_c, 8), the members' rows in the inputs (n_c,)): consumers.get_bbox_3d_result on the host"""
    import torch
    from monorun_amd.consumers import get_bbox_3d_result
    c = case(name)
    res = get_bbox_3d_result(*(torch.from_numpy(c[k]) for k in ('dimensions', 'yaw', 't_vec', 'scores', 'labels')), c['C'], to_np=True)
    return [(r, np.nonzero(c['labels'] == i)[0]) for i, r in enumerate(res)]


@functools.lru_cache(maxsize=None)
def expected(name, thr):
    """kept local indices per class: the hand-written ones where the case has them, oracle.nms_bev's on the rebuilt boxes elsewhere.
    Computed once per run."""
    c, orc = case(name), _oracle()
    return [np.array(c['hand'][i], np.int64) if i in c['hand'] else orc.nms_bev(rebuilt(r), r[:, 7], thr).astype(np.int64).reshape(-1)
            for i, (r, _) in enumerate(class_rows(name))]


def knife_margins(name):
    """per oracle-judged class, the smallest | IoU - thr | over its near pairs and the case's thresholds"""
    c = case(name)
    return {i: nc.knife_margin(nc.pair_ious(rebuilt(r)), c['thrs']) for i, (r, _) in enumerate(class_rows(name)) if i not in c['hand'] and len(r) > 1}


# ------------------------------------------------------------------------------- the seed search
def SEARCH():
    """prints TRIES and KEPT: per class, the first try whose rebuilt boxes leave no pair within KNIFE of a threshold and, from 8 members
    on, keep more than one box and fewer than all at every threshold"""
    orc = _oracle()
    rng = np.random.default_rng(0)

    def fine(b, s):
        r = rows_of(b, s, rng)
        if nc.knife_margin(nc.pair_ious(rebuilt(r)), THRS) < KNIFE:
            return False
        return len(b) < 8 or all(1 < len(orc.nms_bev(rebuilt(r), s, t)) < len(b) for t in THRS)
    tries = {name: {c: k for c, n in enumerate(SIZED[name][1]) if n and (k := nc._search(lambda k: _class_group(name, c, n, k), fine))} for name in SIZED}
    print('TRIES =', tries)
    for name in ('special_scores', 'special_boxes'):
        print(name, 'margins', knife_margins(name))
    TRIES.update(tries)
    case.cache_clear(), class_rows.cache_clear(), expected.cache_clear()
    print('KEPT =', {name: {t: [len(k) for k in expected(name, t)] for t in THRS} for name in NAMES})


if __name__ == '__main__':
    SEARCH()
