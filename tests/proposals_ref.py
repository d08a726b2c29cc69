"""The proposal stage's definitions in numpy (no torch op takes part): the NMS rule with every operation in float32
(``nms_ref32``) and in float64 (``nms_ref64``), mmdet's delta2bbox in float64 from fp32 inputs (``decode_ref64``), the selection and merge
rules of ``RPNHeadMod.get_bboxes``, mmcv's batched_nms and mmdet's multiclass_nms stated on top of them, and the case tables with fixed
seeds that the CPU and the GPU tests share."""
import functools
import math

import numpy as np

F32 = np.float32
WH_RATIO_CLIP = 16 / 1000
EPS = 2.0 ** -23
# error / (2^-23 · magnitude) of the fp32 torch restatement of the decode on DECODE_CASES, measured on the CPU (tests/test_proposals_cpu.py
# recomputes them); the tests allow 4 x: another exp and another order of the same operations
C_BOX_MEASURED = 2.02
C_SCORE_MEASURED = 0.88
C_BOX, C_SCORE = 4 * C_BOX_MEASURED, 4 * C_SCORE_MEASURED


# ------------------------------------------------------------------------------------------------ NMS
def iou_matrix(boxes, dtype):
    """iou[j, i] of the rule, every operation in ``dtype``."""
    b = np.asarray(boxes).astype(dtype)
    with np.errstate(all='ignore'):
        x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
        zero = dtype(0)
        iw = np.maximum(np.minimum(x2[:, None], x2[None, :]) - np.maximum(x1[:, None], x1[None, :]), zero)
        ih = np.maximum(np.minimum(y2[:, None], y2[None, :]) - np.maximum(y1[:, None], y1[None, :]), zero)
        inter = iw * ih
        area = (x2 - x1) * (y2 - y1)
        return inter / ((area[:, None] + area[None, :]) - inter)


def _greedy(over, valid):
    n = over.shape[0]
    removed = ~np.asarray(valid, dtype=bool) if valid is not None else np.zeros(n, dtype=bool)
    removed = removed.copy()
    keep = np.zeros(n, dtype=bool)
    for i in range(n):
        if not removed[i]:
            keep[i] = True
            removed[i + 1:] |= over[i, i + 1:]
    return keep


def _grouped(boxes, valid, sizes, thr, dtype):
    keep = np.zeros(len(boxes), dtype=bool)
    first = 0
    for n in sizes:
        sl = slice(first, first + n)
        if n:
            keep[sl] = _greedy(iou_matrix(boxes[sl], dtype) > dtype(thr), None if valid is None else valid[sl])
        first += n
    return keep


def nms_ref32(boxes, valid, sizes, thr):
    """The definition: keep (T,) bool; boxes in rank order inside each group, every operation of the IoU in float32."""
    return _grouped(boxes, valid, sizes, thr, np.float32)


def nms_ref64(boxes, valid, sizes, thr):
    """The same rule in float64 (the fp32 threshold, as the kernel receives it)."""
    return _grouped(boxes, valid, sizes, float(F32(thr)), np.float64)


def nms_margin64(boxes, sizes, thr):
    """The smallest |iou - thr| over the pairs of each group in float64 (NaN IoUs apart); inf without pairs."""
    best, first = np.inf, 0
    for n in sizes:
        if n > 1:
            d = np.abs(iou_matrix(boxes[first:first + n], np.float64) - float(F32(thr)))[np.triu_indices(n, 1)]
            d = d[~np.isnan(d)]
            if d.size:
                best = min(best, float(d.min()))
        first += n
    return best


def clustered(seed, n=600, width=1248.0, height=384.0):
    """n fp32 boxes in clusters of near-duplicates, as an RPN level holds them."""
    rng = np.random.RandomState(seed)
    k = max(n // 12, 1)
    centre = rng.uniform([0, 0], [width, height], size=(k, 2))
    size = rng.uniform(16, 120, size=(k, 2))
    c = rng.randint(0, k, size=n)
    ctr = centre[c] + rng.normal(0, 0.12, size=(n, 2)) * size[c]
    wh = size[c] * np.exp(rng.normal(0, 0.15, size=(n, 2)))
    return np.concatenate([ctr - wh / 2, ctr + wh / 2], axis=1).astype(F32)


def _grid(n, step=20.0, side=10.0, cols=64):
    """n disjoint boxes"""
    i = np.arange(n)
    x, y = (i % cols) * step, (i // cols) * step
    return np.stack([x, y, x + side, y + side], axis=1).astype(F32)


def _chain(n):
    """box i overlaps i - 1 and i + 1 only (iou 1/6)"""
    x = np.arange(n) * 10.0
    return np.stack([x, np.zeros(n), x + 14.0, np.full(n, 10.0)], axis=1).astype(F32)


def _far(n, pairs):
    """disjoint boxes, except that box v is a copy of box s for (s, v) in pairs"""
    b = _grid(n)
    for s, v in pairs:
        b[v] = b[s]
    return b


def _special(rng):
    """NaN coordinates, zero-area boxes and infinite ones among duplicates of a plain box"""
    plain = [10.0, 10.0, 50.0, 40.0]
    rows = [plain, [np.nan, 10, 50, 40], plain, [20, 20, 20, 35], [20, 20, 20, 35], [12, 12, 12, 12], [12, 12, 12, 12], plain,
            [10, 10, np.inf, 40], [-np.inf, 10, 50, 40], [10, np.nan, 50, np.nan], [11, 11, 49, 39], [30, 5, 30, 60], [0, 0, 0, 0], plain]
    return np.asarray(rows, dtype=F32)


@functools.lru_cache(maxsize=None)
def nms_cases():
    """[dict(name, boxes (T, 4) fp32 in rank order inside each group, valid (T,) uint8 or None, sizes, thr)]"""
    rng = np.random.RandomState(11)
    cases = []

    def add(name, parts, thr, valid=None):
        boxes = np.concatenate([p.reshape(-1, 4) for p in parts]).astype(F32) if parts else np.zeros((0, 4), F32)
        cases.append(dict(name=name, boxes=boxes, valid=valid, sizes=tuple(len(p) for p in parts), thr=thr))

    empty = np.zeros((0, 4), F32)
    add('chain_129_65_2', [_chain(129), _chain(65), _chain(2)], 0.1)
    add('identical_65_1_64', [np.tile(_grid(1), (65, 1)), _grid(1), np.tile(_grid(3)[2:], (64, 1))], 0.5)
    add('disjoint_63_0_1025', [_grid(63), empty, _grid(1025)], 0.0)
    add('far_4096', [_far(4096, [(0, 64), (0, 4095), (3, 4096 - 64 + 3), (31, 4032), (63, 64 + 63), (64, 129), (100, 4000)])], 0.5)
    add('far_1025_129', [_far(1025, [(0, 1024), (1, 65), (63, 960), (64, 128)]), _far(129, [(0, 128), (5, 64), (64, 65)])], 0.75)
    add('special_values', [_special(rng), empty, _special(rng)[::-1].copy()], 0.5)
    for thr in (0.0, 0.75, 1.0):
        add(f'mixed_thr{thr}', [clustered(20, 65), empty, clustered(21, 129), clustered(22, 1), clustered(23, 2), clustered(24, 63),
                                clustered(25, 64), np.tile(_grid(1), (5, 1)), clustered(26, 1025)], thr)
    mixed = cases[-2]
    valid = (rng.uniform(size=len(mixed['boxes'])) < 0.6).astype(np.uint8)
    cases.append(dict(mixed, name='mixed_valid_flags', valid=valid))
    ident = np.tile(_grid(1), (130, 1))
    v = np.ones(130, np.uint8)
    v[0::2] = 0                                                         # an invalid box must not suppress: the first valid one survives
    cases.append(dict(name='identical_valid_interleaved', boxes=ident, valid=v, sizes=(65, 65), thr=0.5))
    v2 = np.zeros(130, np.uint8)
    cases.append(dict(name='none_valid', boxes=ident, valid=v2, sizes=(65, 65), thr=0.5))
    for seed in (0, 1, 3):              # sets whose float64 IoUs all lie farther than 1e-5 from both thresholds (seed 2 holds one at 3e-6)
        for thr in (0.7, 0.75):
            add(f'clustered600_seed{seed}_thr{thr}', [clustered(seed)], thr)
    add('clustered_4096', [clustered(7, 4096)], 0.75)
    add('no_boxes', [empty, empty], 0.5)
    return cases


NMS_IDS = [c['name'] for c in nms_cases()]
MARGIN_CASES = [n for n in NMS_IDS if n.startswith('clustered600')]        # the cases that claim a 1e-5 margin in float64


def scored(case, seed=3):
    """A case as the Python entries take it: the boxes shuffled, with scores that give the case's rank order back (equal scores inside a
    group in runs of three: the tie rule decides) and a label per group.  -> boxes, scores, idxs."""
    rng = np.random.RandomState(seed)
    T = len(case['boxes'])
    scores, idxs = np.zeros(T, F32), np.zeros(T, np.int64)
    first = 0
    for g, n in enumerate(case['sizes']):
        scores[first:first + n] = (1000.0 - (np.arange(n) // 3)) / 1024.0
        idxs[first:first + n] = (g * 7) % 11 + 11 * (g // 11)
        first += n
    # a shuffle that keeps the order of equal scores inside a group: position p holds original perm[p], ties go to the lower input index
    perm = rng.permutation(T)
    for lab in np.unique(idxs):
        for s in np.unique(scores[idxs == lab]):
            where = np.nonzero((scores[perm] == s) & (idxs[perm] == lab))[0]
            perm[where] = np.sort(perm[where])
    return case['boxes'][perm], scores[perm], idxs[perm]


def batched_nms_ref(boxes, scores, idxs, thr):
    """mmcv's batched_nms on unshifted coordinates: keep (k,) int64 in score-descending order, ties to the lower input index."""
    n = len(boxes)
    kept = np.zeros(n, dtype=bool)
    for lab in np.unique(idxs):
        members = np.nonzero(idxs == lab)[0]
        order = members[np.argsort(-scores[members].astype(np.float64), kind='stable')]
        kept[order] = nms_ref32(boxes[order], None, (len(order),), thr)
    order = np.argsort(-scores.astype(np.float64), kind='stable')
    return order[kept[order]]


def multiclass_nms_ref(multi_bboxes, multi_scores, score_thr, thr, max_num=-1, score_factors=None):
    """mmdet's multiclass_nms -> dets (k, 5) fp32, labels (k,)"""
    K, C = multi_scores.shape[0], multi_scores.shape[1] - 1
    bb = multi_bboxes.reshape(K, -1, 4) if multi_bboxes.shape[1] > 4 else np.broadcast_to(multi_bboxes[:, None], (K, C, 4))
    scores = multi_scores[:, :C]
    mask = scores > F32(score_thr)
    if score_factors is not None:
        scores = (scores * score_factors[:, None]).astype(F32)
    boxes, sc, labels = bb[mask], scores[mask], np.nonzero(mask)[1]
    if len(boxes) == 0:
        return np.zeros((0, 5), F32), np.zeros(0, np.int64)
    keep = batched_nms_ref(boxes.astype(F32), sc, labels, thr)
    if max_num > 0:
        keep = keep[:max_num]
    return np.concatenate([boxes[keep], sc[keep, None]], axis=1).astype(F32), labels[keep]


# ------------------------------------------------------------------------------------------------ decode, selection, merge
def select_ref(cls_scores, nms_pre):
    """index (N, P) int64 and the per-level counts: per level the highest logits of the (N, H W A) view, ties to the lower anchor index"""
    index, counts = [], []
    for c in cls_scores:
        N = c.shape[0]
        logits = np.transpose(c, (0, 2, 3, 1)).reshape(N, -1)
        k = min(nms_pre, logits.shape[1]) if nms_pre > 0 else logits.shape[1]
        index.append(np.argsort(-logits.astype(np.float64), axis=1, kind='stable')[:, :k])
        counts.append(k)
    return np.concatenate(index, axis=1).astype(np.int64), counts


def decode_ref64(cls_scores, bbox_preds, index, counts, img_shape, base_anchors, strides, means, stds, wh_ratio_clip=WH_RATIO_CLIP,
                 min_bbox_size=0):
    """delta2bbox in float64 from the fp32 inputs -> boxes (N, P, 4), score (N, P), logit (N, P) (the fp32 value), valid (N, P) bool,
    mag (N, P, 4): the magnitude |px| + |pw dx| + gw / 2 (y alike) that the tolerance of a coordinate is stated in."""
    N = index.shape[0]
    max_ratio = float(F32(abs(math.log(wh_ratio_clip))))
    out = []
    first = 0
    for l, (c, r, k) in enumerate(zip(cls_scores, bbox_preds, counts)):
        A, H, W = c.shape[1:]
        t = index[:, first:first + k]
        first += k
        a, cell = t % A, t // A
        y, x = cell // W, cell % W
        n = np.arange(N)[:, None]
        logit = c[n, a, y, x]
        d = np.stack([r[n, 4 * a + j, y, x] for j in range(4)], axis=-1).astype(np.float64)
        d = d * np.asarray(stds, F32).astype(np.float64) + np.asarray(means, F32).astype(np.float64)
        base = np.asarray(base_anchors[l], F32).astype(np.float64)[a]
        shift = np.stack([x, y, x, y], axis=-1).astype(np.float64) * float(strides[l])
        out.append((logit, d, base + shift))
    logit = np.concatenate([o[0] for o in out], axis=1)
    d = np.concatenate([o[1] for o in out], axis=1)
    an = np.concatenate([o[2] for o in out], axis=1)
    dw, dh = np.clip(d[..., 2], -max_ratio, max_ratio), np.clip(d[..., 3], -max_ratio, max_ratio)
    px, py = (an[..., 0] + an[..., 2]) * 0.5, (an[..., 1] + an[..., 3]) * 0.5
    pw, ph = an[..., 2] - an[..., 0], an[..., 3] - an[..., 1]
    gw, gh = pw * np.exp(dw), ph * np.exp(dh)
    gx, gy = px + pw * d[..., 0], py + ph * d[..., 1]
    shape = np.asarray(img_shape, F32).astype(np.float64)
    img_h, img_w = shape[:, 0:1], shape[:, 1:2]
    x1, x2 = np.clip(gx - gw * 0.5, 0, img_w), np.clip(gx + gw * 0.5, 0, img_w)
    y1, y2 = np.clip(gy - gh * 0.5, 0, img_h), np.clip(gy + gh * 0.5, 0, img_h)
    boxes = np.stack([x1, y1, x2, y2], axis=-1)
    mx, my = np.abs(px) + np.abs(pw * d[..., 0]) + gw * 0.5, np.abs(py) + np.abs(ph * d[..., 1]) + gh * 0.5
    mag = np.stack([mx, my, mx, my], axis=-1)
    score = 1.0 / (1.0 + np.exp(-logit.astype(np.float64)))
    valid = np.ones(logit.shape, dtype=bool)
    if min_bbox_size > 0:
        valid = ~((x2 - x1 < min_bbox_size) | (y2 - y1 < min_bbox_size))
    return boxes, score, logit, valid, mag


def merge_ref(boxes, score, logit, keep, nms_post):
    """per image the kept candidates by logit descending (ties to the position), the first nms_post -> [(k_n, 5)] in boxes' dtype"""
    out = []
    for n in range(logit.shape[0]):
        order = np.argsort(-logit[n].astype(np.float64), kind='stable')
        order = order[np.asarray(keep[n], dtype=bool)[order]][:nms_post]
        out.append(np.concatenate([boxes[n][order], score[n][order, None]], axis=1))
    return out


STRIDES = (4, 8, 16)
MAPS = ((12, 20), (6, 10), (3, 5))          # a 48 x 80 image
N_IMAGES, N_ANCHORS = 2, 3
IMG_SHAPES = ((48.0, 80.0), (41.0, 67.0))
MEANS, STDS = (0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0, 1.0)


def base_anchors64(scales, ratios, strides):
    """mmdet's base anchors in float64: per level (len(ratios) len(scales), 4), ratio-major"""
    out = []
    for s in strides:
        rows = []
        for r in ratios:
            for sc in scales:
                h_r = math.sqrt(r)
                w, h = s * (1 / h_r) * sc, s * h_r * sc
                rows.append([-w / 2, -h / 2, w / 2, h / 2])
        out.append(np.asarray(rows, dtype=np.float64))
    return out


def base_anchors32():
    return [b.astype(F32) for b in base_anchors64([2], [0.4, 0.7, 1.0], STRIDES)]


def head_outputs(seed, scale_wh=1.0):
    """cls_scores, bbox_preds of the three levels as fp32 NCHW arrays; some deltas beyond both sides of the wh clamp, some shifts that push
    boxes over all four borders"""
    rng = np.random.RandomState(seed)
    cls, reg = [], []
    for h, w in MAPS:
        cls.append(rng.normal(0, 2.0, size=(N_IMAGES, N_ANCHORS, h, w)).astype(F32))
        r = rng.normal(0, 0.5, size=(N_IMAGES, 4 * N_ANCHORS, h, w))
        r[:, 2::4] *= scale_wh
        r[:, 3::4] *= scale_wh
        reg.append(r.astype(F32))
    return cls, reg


def decode_case(min_bbox_size):
    """the decode test's inputs: deltas on both sides of the clamp (|dw| up to ~ 9 > 4.135) and boxes beyond every border"""
    cls, reg = head_outputs(5, scale_wh=6.0)
    reg[0][0, 0, 0, 0], reg[0][0, 1, 0, 0] = -3.0, -3.0            # over the left and the top border
    reg[0][1, 0, -1, -1], reg[0][1, 1, -1, -1] = 3.0, 3.0          # over the right and the bottom border
    index, counts = select_ref(cls, 0)
    return dict(cls=cls, reg=reg, index=index, counts=counts, img_shape=np.asarray(IMG_SHAPES, F32), base=base_anchors32(),
                min_bbox_size=min_bbox_size)


DECODE_CASES = {'min0': 0.0, 'min8': 8.0}
E2E_SEED, E2E_THR, E2E_NMS_PRE, E2E_NMS_POST, E2E_MIN_SIZE = 36, 0.6, 40, 50, 4.0


def e2e_case(seed=E2E_SEED):
    """the independent end-to-end case: head outputs for get_bboxes with nms_pre E2E_NMS_PRE, nms_thr E2E_THR"""
    cls, reg = head_outputs(seed, scale_wh=0.6)
    return dict(cls=cls, reg=reg, img_shape=np.asarray(IMG_SHAPES, F32), base=base_anchors32())
