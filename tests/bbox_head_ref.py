"""The 2-D detection head's get_bboxes defined in numpy, no torch op taking part: the softmax with every operation in
float32 (``softmax_ref32``) and in float64 (``softmax_ref64``), delta2bbox per class with the clamp and the rescale (``decode_ref32`` /
``decode_ref64``), the validity flag, the ranks (``rank_ref``), the per-image selection (``select_ref``) and the whole stage on top of
tests/proposals_ref.py's NMS rule (``detect_ref32`` / ``detect_ref64``); and the case tables with fixed seeds that the CPU and the GPU tests
share."""
import functools
import math

import numpy as np

from tests.proposals_ref import EPS, F32, WH_RATIO_CLIP, clustered, iou_matrix, nms_ref32, nms_ref64

# error of the fp32 torch restatement against the float64 definition over RANK_CASES, measured on the CPU (tests/test_bbox_head_cpu.py
# recomputes them): a coordinate in units of 2^-23 (|px| + |pw dx| + gw / 2) / scale_factor beyond half an ulp of the quotient, a score in
# units of 2^-23 score.  The GPU tests allow 4 x: another exp and another order of the same operations.
C_BOX_MEASURED = 1.09
C_SCORE_MEASURED = 5.64
C_BOX, C_SCORE = 4 * C_BOX_MEASURED, 4 * C_SCORE_MEASURED

MEANS, STDS = (0.0, 0.0, 0.0, 0.0), (0.1, 0.1, 0.2, 0.2)
IMG_SHAPES = ((384.0, 1248.0), (370.0, 1224.0), (375.0, 1242.0))
SCALES = ((1.5, 1.25, 1.5, 1.25), (0.8, 0.8, 0.8, 0.8), (2.0, 1.7, 2.0, 1.7))       # non-uniform 4-vectors


# ------------------------------------------------------------------------------------------------ the rule
def _softmax(x, dtype):
    x = np.asarray(x, F32).astype(dtype)
    with np.errstate(all='ignore'):
        e = np.exp(x - x.max(axis=1, keepdims=True))
        s = e[:, 0]
        for j in range(1, e.shape[1]):
            s = s + e[:, j]
        return e / s[:, None]


def softmax_ref32(cls_score):
    """scores (R, C + 1): m = max_j x_j, e_j = exp(x_j - m), s = e_0 + e_1 + ... in index order, e / s; every operation in float32"""
    return _softmax(cls_score, np.float32)


def softmax_ref64(cls_score):
    """the same in float64 from the fp32 logits"""
    return _softmax(cls_score, np.float64)


def per_row(table, counts):
    return np.repeat(np.asarray(table, F32), counts, axis=0)


def _decode(rois, bbox_pred, counts, img_shapes, scales, means, stds, dtype, wh_ratio_clip=WH_RATIO_CLIP):
    """boxes (R, G, 4), G = bbox_pred's groups of four, and the magnitudes the tolerance of a coordinate is stated in"""
    R = len(rois)
    max_ratio = dtype(F32(abs(math.log(wh_ratio_clip))))
    with np.errstate(all='ignore'):
        d = np.asarray(bbox_pred, F32).astype(dtype).reshape(R, np.shape(bbox_pred)[1] // 4, 4) * np.asarray(stds, F32).astype(dtype) + np.asarray(means, F32).astype(dtype)
        dw, dh = np.clip(d[..., 2], -max_ratio, max_ratio), np.clip(d[..., 3], -max_ratio, max_ratio)
        r = np.asarray(rois, F32).astype(dtype)[:, None, 1:5]
        half = dtype(0.5)
        px, py = (r[..., 0] + r[..., 2]) * half, (r[..., 1] + r[..., 3]) * half
        pw, ph = r[..., 2] - r[..., 0], r[..., 3] - r[..., 1]
        gw, gh = pw * np.exp(dw), ph * np.exp(dh)
        gx, gy = px + pw * d[..., 0], py + ph * d[..., 1]
        shape = per_row(img_shapes, counts).astype(dtype)
        zero, img_h, img_w = dtype(0), shape[:, 0:1], shape[:, 1:2]
        x1, x2 = np.minimum(np.maximum(gx - gw * half, zero), img_w), np.minimum(np.maximum(gx + gw * half, zero), img_w)
        y1, y2 = np.minimum(np.maximum(gy - gh * half, zero), img_h), np.minimum(np.maximum(gy + gh * half, zero), img_h)
        boxes = np.stack([x1, y1, x2, y2], axis=-1)
        mx, my = np.abs(px) + np.abs(pw * d[..., 0]) + gw * half, np.abs(py) + np.abs(ph * d[..., 1]) + gh * half
        mag = np.stack([mx, my, mx, my], axis=-1)
        if scales is not None:
            f = per_row(scales, counts).astype(dtype)[:, None, :]
            boxes, mag = boxes / f, mag / f
    return boxes, mag


def decode_ref32(rois, bbox_pred, counts, img_shapes, scales, means=MEANS, stds=STDS):
    """§19's delta2bbox of rois[:, 1:5] and each group of four deltas, the clamp to the image and the division by the image's
    scale_factor (None: no rescale), every operation in float32 -> boxes (R, G, 4)"""
    return _decode(rois, bbox_pred, counts, img_shapes, scales, means, stds, np.float32)[0]


def decode_ref64(rois, bbox_pred, counts, img_shapes, scales, means=MEANS, stds=STDS):
    """the same in float64 from the fp32 inputs -> boxes (R, G, 4), mag (R, G, 4): (|px| + |pw dx| + gw / 2) / scale_factor (y alike)"""
    return _decode(rois, bbox_pred, counts, img_shapes, scales, means, stds, np.float64)


def valid_ref(score, rois, score_thr):
    """(R, C) bool: score > score_thr (the fp32 threshold; NaN compares false) and the RoI's four coordinates finite"""
    with np.errstate(invalid='ignore'):
        return (score > score.dtype.type(F32(score_thr))) & np.isfinite(np.asarray(rois)[:, 1:5]).all(axis=1)[:, None]


def rank_ref(score):
    """the ranks of one group: indices (K,) by score descending, NaN after every number, ties to the lower index"""
    s = np.asarray(score, dtype=np.float64)
    nan = np.isnan(s)
    return np.lexsort((np.arange(len(s)), np.where(nan, 0.0, -s), nan))


def groups_ref(boxes, score, valid, counts):
    """(R, C, 4) boxes, (R, C) scores and flags -> the groups' layout, group (n, c) image-major in rank order: boxes (T, 4), score (T,),
    order (T,) int32, valid (T,) bool"""
    C = score.shape[1]
    ob, os_, oo, ov = [np.zeros((0, 4), boxes.dtype)], [np.zeros(0, score.dtype)], [np.zeros(0, np.int32)], [np.zeros(0, bool)]
    first = 0
    for k in counts:
        for c in range(C):
            o = rank_ref(score[first:first + k, c])
            ob.append(boxes[first:first + k, c][o]); os_.append(score[first:first + k, c][o]); oo.append(o.astype(np.int32))
            ov.append(valid[first:first + k, c][o])
        first += k
    return np.concatenate(ob), np.concatenate(os_), np.concatenate(oo), np.concatenate(ov)


def group_sizes(counts, C):
    return tuple(k for k in counts for _ in range(C))


def select_ref(boxes, score, order, keep, counts, C, max_num):
    """per image the kept candidates of the groups' layout by score descending, ties to the lower candidate order C + c, the first max_num
    (all when max_num <= 0) -> [(dets (k, 5) in boxes' dtype, labels (k,) int64)]"""
    out, first = [], 0
    for k in counts:
        sl = slice(first, first + C * k)
        first += C * k
        cls = np.repeat(np.arange(C), k)
        cand = order[sl].astype(np.int64) * C + cls
        kept = np.nonzero(np.asarray(keep[sl], dtype=bool))[0]
        kept = kept[np.lexsort((cand[kept], -score[sl][kept].astype(np.float64)))]
        if max_num > 0:
            kept = kept[:max_num]
        out.append((np.concatenate([boxes[sl][kept], score[sl][kept, None].astype(boxes.dtype)], axis=1), cls[kept].astype(np.int64)))
    return out


def _detect(c, iou_thr, max_num, dtype, scores=None, boxes=None):
    C = c['C']
    score = (softmax_ref32 if dtype is np.float32 else softmax_ref64)(c['cls'])[:, :C] if scores is None else scores
    if boxes is None:
        boxes = _decode(c['rois'], c['reg'], c['counts'], c['img_shapes'], c['scales'], c['means'], c['stds'], dtype)[0]
    if boxes.shape[1] == 1:
        boxes = np.broadcast_to(boxes, (len(boxes), C, 4))
    valid = valid_ref(score, c['rois'], c['score_thr'])
    gb, gs, go, gv = groups_ref(boxes, score, valid, c['counts'])
    keep = (nms_ref32 if dtype is np.float32 else nms_ref64)(gb, gv, group_sizes(c['counts'], C), iou_thr)
    return dict(boxes=gb, score=gs, order=go, valid=gv, keep=keep, dets=select_ref(gb, gs, go, keep, c['counts'], C, max_num))


def detect_ref32(case, iou_thr, max_num, scores=None, boxes=None):
    """the whole rule in float32 on a case (a dict of make_case): the groups' layout (boxes, score, order, valid, keep) and per image
    (dets, labels).  ``scores`` (R, C) / ``boxes`` (R, C or 1, 4): take these instead of computing them (everything after them is exact)."""
    return _detect(case, iou_thr, max_num, np.float32, scores, boxes)


def detect_ref64(case, iou_thr, max_num):
    """the whole rule in float64 from the fp32 inputs"""
    return _detect(case, iou_thr, max_num, np.float64)


# ------------------------------------------------------------------------------------------------ cases
def make_case(seed, counts, C, agnostic, rescale, special=False, score_thr=0.05, extremes=True, logit_scale=2.0):
    """head outputs and RoIs of len(counts) images: RoIs in clusters inside the image (a few pushed over each border by their deltas),
    logits N(0, logit_scale), deltas N(0, 1) (x std 0.1 / 0.2), some beyond both sides of the wh clamp; ``special``: equal logits across
    rows, NaN and +-inf logits, NaN-row and infinite RoIs"""
    rng = np.random.RandomState(seed)
    R, N = int(sum(counts)), len(counts)
    rois = np.zeros((R, 5), F32)
    first = 0
    for n, k in enumerate(counts):
        h, w = IMG_SHAPES[n]
        if k:
            b = clustered(seed * 7 + n, k, w, h)
            b[:, 0::2] = np.clip(b[:, 0::2], 0, w)
            b[:, 1::2] = np.clip(b[:, 1::2], 0, h)
            b[:, 2:] = np.maximum(b[:, 2:], b[:, :2] + 4)
            rois[first:first + k, 0], rois[first:first + k, 1:] = n, b
        first += k
    cls = rng.normal(0, logit_scale, size=(R, C + 1)).astype(F32)
    reg = rng.normal(0, 1.0, size=(R, 4 if agnostic else 4 * C)).astype(F32)
    G = reg.shape[1] // 4
    for i in range(R if extremes else 0):               # every 11th row: beyond the clamp of dw / dh, every 13th: over a border
        g = i % G
        if i % 11 == 0:
            reg[i, 4 * g + 2], reg[i, 4 * g + 3] = (30.0, -30.0) if i % 2 else (-30.0, 30.0)
        if i % 13 == 0:
            reg[i, 4 * g + 0], reg[i, 4 * g + 1] = ((-1) ** (i // 13)) * 60.0, ((-1) ** (i // 26)) * 60.0
    if special:
        assert R >= 120
        for i in (7, 20, 100):
            cls[i] = cls[3]                             # equal logits across rows: ties
        cls[40, 0], cls[41, C], cls[42] = np.nan, np.nan, np.nan
        cls[50, 0], cls[51, 0], cls[52, C], cls[53] = np.inf, -np.inf, -np.inf, -np.inf
        cls[54, 0], cls[54, C] = np.inf, np.inf
        rois[60, 1:], rois[61, 1:], rois[62, 3], rois[63, 1] = np.nan, np.nan, np.inf, -np.inf
        cls[60], cls[62] = 0.0, 0.0
        cls[60, 0], cls[62, 0] = 5.0, 5.0               # a high score on a NaN row and on an infinite one
    return dict(rois=rois, cls=cls, reg=reg, counts=tuple(int(k) for k in counts), C=C, agnostic=bool(agnostic),
                img_shapes=np.asarray(IMG_SHAPES[:N], F32), scales=np.asarray(SCALES[:N], F32) if rescale else None, means=MEANS, stds=STDS,
                score_thr=score_thr)


# name -> (seed, counts, C, agnostic, rescale, special): the row counts at which a padded sorting network and the 64-wide tiles can go
# wrong, C 1 and 3, class-agnostic and not, one and three images with unequal counts and an empty image in the middle
RANK_TABLE = {
    'k0': (1, (0,), 3, False, False, False),
    'k1_c1_agnostic': (2, (1,), 1, True, False, False),
    'k2_c3': (3, (2,), 3, False, True, False),
    'k63_c1': (4, (63,), 1, False, False, False),
    'k64_c3_agnostic': (5, (64,), 3, True, True, False),
    'k65_c3': (6, (65,), 3, False, False, False),
    'k129_c1_agnostic': (7, (129,), 1, True, True, False),
    'k1000_c3': (8, (1000,), 3, False, False, False),
    'k1025_c3_agnostic': (9, (1025,), 3, True, False, False),
    'k4096_c3': (10, (4096,), 3, False, True, False),
    'n3_65_0_129_c3': (11, (65, 0, 129), 3, False, True, False),
    'n3_1000_0_2_c1': (12, (1000, 0, 2), 1, False, False, False),
    'n3_1_4096_64_c3_agnostic': (13, (1, 4096, 64), 3, True, True, False),
    'special_c3': (14, (130,), 3, False, True, True),
    'special_n3_c1_agnostic': (15, (2, 0, 150), 1, True, False, True),
}
RANK_IDS = list(RANK_TABLE)


@functools.lru_cache(maxsize=None)
def rank_case(name):
    seed, counts, C, agnostic, rescale, special = RANK_TABLE[name]
    return make_case(seed, counts, C, agnostic, rescale, special)


@functools.lru_cache(maxsize=None)
def rank_reference(name):
    """the float64 definition on a rank case, computed once and shared: score (R, C), boxes (R, G, 4), mag (R, G, 4)"""
    c = rank_case(name)
    boxes, mag = decode_ref64(c['rois'], c['reg'], c['counts'], c['img_shapes'], c['scales'])
    score = softmax_ref64(c['cls'])[:, :c['C']]
    for a in (boxes, mag, score):
        a.setflags(write=False)
    return score, boxes, mag


def ratios(name, score32, boxes32):
    """(box ratio, score ratio) of fp32 results (score (R, C), boxes (R, G, 4)) against the float64 definition on a rank case, in the units
    C_BOX / C_SCORE are stated in; asserts what is exact: the NaN pattern of the scores and zeros where the definition has zeros.  Boxes are
    compared on the rows whose RoI is finite."""
    c = rank_case(name)
    s64, b64, mag = rank_reference(name)
    if len(s64) == 0:
        return 0.0, 0.0
    s32, b32 = np.asarray(score32).astype(np.float64), np.asarray(boxes32).astype(np.float64)
    assert np.array_equal(np.isnan(s32), np.isnan(s64)), 'the NaN scores are those of the definition'
    num = ~np.isnan(s64)
    assert ((s32 == 0) == (s64 < 1e-44))[num].all()
    pos = num & (s64 >= 1e-37)                           # normal numbers
    rs = float((np.abs(s32 - s64)[pos] / (EPS * s64[pos])).max()) if pos.any() else 0.0
    rows = np.isfinite(c['rois'][:, 1:5]).all(axis=1)
    err = np.abs(b32 - b64)[rows] - 0.5 * EPS * np.abs(b64[rows])
    rb = float(np.maximum(err / (EPS * mag[rows]), 0).max()) if rows.any() else 0.0
    return rb, rs


# the independent case: no pair of valid candidates of a group with a float64 IoU within 5e-3 of the threshold, no valid score within
# relative 1e-5 of score_thr or of another candidate's of the same image (tests/test_bbox_head_cpu.py asserts both on the float64 definition)
E2E_SEED, E2E_COUNTS, E2E_C, E2E_SCORE_THR, E2E_IOU_THR, E2E_MAX_NUM = 35, (36, 25), 3, 0.25, 0.5, 15


@functools.lru_cache(maxsize=None)
def e2e_case(seed=E2E_SEED):
    return make_case(1000 + seed, E2E_COUNTS, E2E_C, False, True, score_thr=E2E_SCORE_THR, extremes=False, logit_scale=1.5)


def e2e_margins(case, iou_thr):
    """on the float64 definition: (smallest |iou - thr| over the pairs of valid candidates of each group, smallest relative distance of a
    valid score to score_thr, smallest relative distance of two candidates' scores of an image where one is valid, smallest side)"""
    d = detect_ref64(case, iou_thr, 0)
    C, thr = case['C'], float(F32(iou_thr))
    iou_m, thr_m, pair_m, side = np.inf, np.inf, np.inf, np.inf
    first = 0
    for k in case['counts']:
        image = slice(first, first + C * k)
        for c in range(C):
            g = slice(first + c * k, first + (c + 1) * k)
            b = d['boxes'][g][d['valid'][g]]
            if len(b) > 1:
                iou = iou_matrix(b, np.float64)[np.triu_indices(len(b), 1)]
                iou_m = min(iou_m, float(np.abs(iou - thr).min()))
            if len(b):
                side = min(side, float(np.minimum(b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]).min()))
        s, v = d['score'][image], d['valid'][image]
        t = float(F32(case['score_thr']))
        thr_m = min(thr_m, float((np.abs(s - t) / t).min()))
        o = np.argsort(s)
        gap = np.diff(s[o]) / s[o][1:]
        near = v[o][1:] | v[o][:-1]
        if near.any():
            pair_m = min(pair_m, float(gap[near].min()))
        first += C * k
    return iou_m, thr_m, pair_m, side


def ungroup(counts, C, order, *arrays):
    """arrays in the groups' layout (T, ...) back to RoI order: (R, C, ...) each, by the ranks ``order`` (T,)"""
    out = [np.zeros((int(sum(counts)), C) + a.shape[1:], a.dtype) for a in arrays]
    first, row = 0, 0
    for k in counts:
        for c in range(C):
            o = order[first:first + k]
            for dst, a in zip(out, arrays):
                dst[row + o, c] = a[first:first + k]
            first += k
        row += k
    return out
