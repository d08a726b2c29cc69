"""The 2-D detector's training rule restated in numpy, no torch op in a definition: mmdet 2.x's ``bbox_overlaps``,
``MaxIoUAssigner.assign`` (``gt_max_assign_all=True``, ``ignore_wrt_candidates=True``), ``bbox2delta`` and ``RandomSampler`` by keys, in the
dtype asked for — float32 is the rule the kernels and ``assign_torch`` are exact against, float64 what the margins are measured with.
Shared by the CPU and the GPU tests, with the case builders."""
import numpy as np

EPS = 1e-6


def pmax(a, b):
    """torch's max: a NaN operand is the result"""
    return np.where((a >= b) | (a != a), a, b)


def pmin(a, b):
    return np.where((a <= b) | (a != a), a, b)


def overlaps(b1, b2, mode='iou', dtype=np.float32):
    """(m, 4), (n, 4) -> (m, n): iou, or iof over the area of b1's boxes; every operation in `dtype`"""
    a, b = np.asarray(b1, dtype=dtype)[:, None, :], np.asarray(b2, dtype=dtype)[None, :, :]
    zero, eps = dtype(0), dtype(EPS)
    with np.errstate(all='ignore'):
        area_a = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
        area_b = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
        w = pmax(pmin(a[..., 2], b[..., 2]) - pmax(a[..., 0], b[..., 0]), zero)
        h = pmax(pmin(a[..., 3], b[..., 3]) - pmax(a[..., 1], b[..., 1]), zero)
        inter = w * h
        union = pmax((area_a + area_b) - inter, eps) if mode == 'iou' else pmax(area_a + np.zeros_like(inter), eps)
        out = inter / union
    assert out.dtype == dtype
    return out


def bbox2delta(box, gt, means=(0, 0, 0, 0), stds=(1, 1, 1, 1), dtype=np.float32):
    p, g = np.asarray(box, dtype=dtype), np.asarray(gt, dtype=dtype)
    half = dtype(0.5)
    with np.errstate(all='ignore'):
        px, py, pw, ph = (p[..., 0] + p[..., 2]) * half, (p[..., 1] + p[..., 3]) * half, p[..., 2] - p[..., 0], p[..., 3] - p[..., 1]
        gx, gy, gw, gh = (g[..., 0] + g[..., 2]) * half, (g[..., 1] + g[..., 3]) * half, g[..., 2] - g[..., 0], g[..., 3] - g[..., 1]
        d = np.stack(((gx - px) / pw, (gy - py) / ph, np.log(gw / pw), np.log(gh / ph)), axis=-1)
        return ((d - np.asarray(means, dtype=dtype)) / np.asarray(stds, dtype=dtype)).astype(dtype)


def delta_bound_terms(box, gt, means=(0, 0, 0, 0), stds=(1, 1, 1, 1)):
    """per coordinate the sum of the magnitudes of the terms of the fp64 delta: (|gx| + |px|) / pw, |log(gw / pw)| + 1, each + |mean|, / std"""
    p, g = np.asarray(box, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    pw, ph, gw, gh = p[..., 2] - p[..., 0], p[..., 3] - p[..., 1], g[..., 2] - g[..., 0], g[..., 3] - g[..., 1]
    t = np.stack(((np.abs(g[..., 0]) + np.abs(g[..., 2]) + np.abs(p[..., 0]) + np.abs(p[..., 2])) / pw,
                  (np.abs(g[..., 1]) + np.abs(g[..., 3]) + np.abs(p[..., 1]) + np.abs(p[..., 3])) / ph,
                  np.abs(np.log(gw / pw)) + 1.0, np.abs(np.log(gh / ph)) + 1.0), axis=-1)
    return (t + np.abs(np.asarray(means, dtype=np.float64))) / np.asarray(stds, dtype=np.float64)


def assign(boxes, gts, labels=None, ignore=None, present=None, pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.0, ignore_iof_thr=-1.0,
           match_low_quality=True, means=(0, 0, 0, 0), stds=(1, 1, 1, 1), dtype=np.float32):
    """one image: boxes (B, >= 4), gts (G, 4) -> dict(gt_ind, label, max_overlap, argmax, ignored, gt_max, deltas)"""
    boxes = np.asarray(boxes, dtype=dtype)[:, :4]
    gts = np.asarray(gts, dtype=dtype).reshape(-1, 4)
    B, G = len(boxes), len(gts)
    here = np.ones(B, dtype=bool) if present is None else np.asarray(present, dtype=bool)
    boxes = np.where(here[:, None], boxes, dtype(0))
    out = dict(gt_ind=np.where(here, 0, -1).astype(np.int64), label=np.full(B, -1, dtype=np.int64), max_overlap=np.zeros(B, dtype=dtype),
               argmax=np.zeros(B, dtype=np.int64), ignored=np.zeros(B, dtype=bool), gt_max=np.zeros(0, dtype=dtype),
               deltas=np.zeros((B, 4), dtype=dtype))
    if G == 0:
        return out
    ov = overlaps(gts, boxes, dtype=dtype)
    ignored = np.zeros(B, dtype=bool)
    if ignore_iof_thr > 0 and ignore is not None and len(ignore) > 0:
        iof = overlaps(boxes, ignore, mode='iof', dtype=dtype)
        worst = np.full(B, -1, dtype=dtype)
        for i in range(iof.shape[1]):
            worst = np.where(iof[:, i] > worst, iof[:, i], worst)
        ignored = here & (worst > dtype(ignore_iof_thr))
        ov = np.where(ignored[None, :], dtype(-1), ov)
    best, arg = np.full(B, -1, dtype=dtype), np.zeros(B, dtype=np.int64)
    gt_max = np.full(G, -1, dtype=dtype)
    for i in range(G):
        up = ov[i] > best
        best, arg = np.where(up, ov[i], best), np.where(up, i, arg)
        row = ov[i][here]
        row = row[row > dtype(-1)]
        if len(row):
            gt_max[i] = row.max()
    ind = np.full(B, -1, dtype=np.int64)
    ind[(best >= 0) & (best < dtype(neg_iou_thr))] = 0
    pos = best >= dtype(pos_iou_thr)
    ind[pos] = arg[pos] + 1
    if match_low_quality:
        for i in range(G):
            if gt_max[i] >= dtype(min_pos_iou):
                ind[(ov[i] == gt_max[i]) & here] = i + 1
    ind[~here] = -1
    pos = ind > 0
    lab = np.zeros(G, dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64)
    out.update(gt_ind=ind, max_overlap=np.where(here, best, dtype(0)), argmax=np.where(here, arg, 0), ignored=ignored, gt_max=gt_max)
    out['label'][pos] = lab[ind[pos] - 1]
    out['deltas'][pos] = bbox2delta(boxes[pos], gts[ind[pos] - 1], means, stds, dtype=dtype)
    return out


def sample(gt_ind, keys, num, pos_fraction, neg_pos_ub=-1):
    """RandomSampler by keys on one image's (already prepended) gt_ind -> (pos_inds, neg_inds) ascending"""
    gt_ind, keys = np.asarray(gt_ind), np.asarray(keys)
    pos, neg = np.nonzero(gt_ind > 0)[0], np.nonzero(gt_ind == 0)[0]
    n_pos = min(len(pos), int(num * pos_fraction))
    n_neg = min(len(neg), num - n_pos)
    if neg_pos_ub >= 0:
        n_neg = min(n_neg, int(max(1, n_pos) * neg_pos_ub))
    take = lambda idx, k: np.sort(idx[np.argsort(keys[idx], kind='stable')[:k]])
    return take(pos, n_pos), take(neg, n_neg)


# ------------------------------------------------------------------------------------------------ case builders
def rb(r, n):
    """the issue's random boxes"""
    cx, cy, w, h = r.uniform(0, 80, n), r.uniform(0, 48, n), r.uniform(4, 60, n), r.uniform(4, 40, n)
    return np.stack((cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2), axis=-1).astype(np.float32)


def anchors_48x80():
    """the 945 anchors of a 48 x 80 image at strides 4 / 8 / 16, scale 8, ratios 0.5 / 1 / 2, in mmdet's order, fp32 operation for operation"""
    f = np.float32
    out = []
    for s in (4, 8, 16):
        h_r = np.sqrt(np.array([0.5, 1.0, 2.0], dtype=f))
        w_r = f(1) / h_r
        w, h = f(s) * w_r * f(8), f(s) * h_r * f(8)
        base = np.stack((f(-0.5) * w, f(-0.5) * h, f(0.5) * w, f(0.5) * h), axis=-1)
        H, W = 48 // s, 80 // s
        xx, yy = np.tile(np.arange(W, dtype=f) * f(s), H), np.repeat(np.arange(H, dtype=f) * f(s), W)
        shifts = np.stack((xx, yy, xx, yy), axis=-1)
        out.append((shifts[:, None, :] + base[None, :, :]).reshape(-1, 4))
    return np.concatenate(out).astype(f)


THRESHOLDS = (dict(pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3), dict(pos_iou_thr=0.6, neg_iou_thr=0.6, min_pos_iou=0.6))


def exact_cases():
    """[(name, boxes (B, 4 or 5), gts, labels, ignore, present, rule kwargs)]: the issue's exactness cases, one image each"""
    r = np.random.default_rng(2100)
    cases = []
    add = lambda name, boxes, gts, ignore=None, present=None, **kw: cases.append(
        (name, np.asarray(boxes, dtype=np.float32), np.asarray(gts, dtype=np.float32).reshape(-1, 4),
         r.integers(0, 3, len(gts)).astype(np.int64), None if ignore is None else np.asarray(ignore, dtype=np.float32), present,
         dict(THRESHOLDS[0], **kw)))
    for B in (0, 1, 63, 64, 65, 255, 256, 257):
        add(f'B{B}', rb(r, B), rb(r, 3))
    for G in (0, 1, 2, 63, 64, 65, 256):
        add(f'G{G}', rb(r, 130), rb(r, G))
    anchors = anchors_48x80()
    inside = np.array([[8, 8, 72, 40], [0, 0, 80, 48], [20, 10, 44, 34], [30, 4, 62, 44]], dtype=np.float32)
    for t, thr in enumerate(THRESHOLDS):
        add(f'anchors-ties-{t}', anchors, inside, **thr)
        add(f'random-{t}', rb(r, 300), rb(r, 7), **thr)
    # integer ground truths placed symmetrically between two anchors: centred at x = 18 between the 32 x 32 stride-4 anchors centred at 16
    # and 20, one inside both (IoU 400 / 1024 each, below pos_iou_thr: only the == step assigns them), one overlapping both alike
    add('symmetric', anchors, [[8, 6, 28, 26], [2, 0, 34, 32], [50, 10, 70, 30]])
    add('no-low-quality', anchors, inside, match_low_quality=False)
    add('below-min-pos', rb(r, 200), np.concatenate((rb(r, 3), [[200, 200, 203, 203]])), min_pos_iou=0.3)
    # two ground truths that claim one box: the later wins
    add('two-claim-one', [[0, 0, 10, 10], [40, 40, 50, 50]], [[0, 0, 20, 10], [0, 0, 10, 20]], min_pos_iou=0.0)
    b = rb(r, 200)
    one = b[5].copy()
    half = np.array([one[0], one[1], one[0] + (one[2] - one[0]) * 0.75, one[3]], dtype=np.float32)     # covers 3/4 of box 5
    for n_ign in (0, 1, 65):
        ign = np.concatenate((half[None], rb(r, 64)))[:n_ign].reshape(-1, 4)
        add(f'ignore{n_ign}', b, rb(r, 6), ignore=ign, ignore_iof_thr=0.5)
    # one box whose iof equals the threshold exactly: [0, 0, 8, 8] against [0, 0, 4, 8] is 32 / 64 = 0.5, not ignored
    add('iof-at-threshold', [[0, 0, 8, 8], [0, 0, 4, 4], [1, 1, 7, 7]], [[0, 0, 8, 8]], ignore=[[0, 0, 4, 8]], ignore_iof_thr=0.5)
    add('all-ignored', rb(r, 70), rb(r, 4), ignore=[[-100, -100, 200, 200]], ignore_iof_thr=0.5)
    add('valid-flags', rb(r, 300), rb(r, 5), present=r.uniform(size=300) < 0.6)
    five = np.concatenate((rb(r, 100), r.uniform(size=(100, 1)).astype(np.float32)), axis=1)
    five[77:] = np.nan
    add('counts-stride5', five, rb(r, 5), present=np.arange(100) < 77)
    odd = rb(r, 70)
    odd[3] = np.nan; odd[4, 2] = np.inf; odd[5] = [-np.inf, 0, np.inf, 10]; odd[6] = [5, 5, 5, 9]; odd[7] = [5, 5, 5, 5]; odd[8, 0] = np.nan
    godd = rb(r, 6)
    godd[1] = np.nan; godd[2] = [3, 3, 3, 3]; godd[3] = [0, 0, np.inf, 20]; godd[4, 3] = np.nan
    add('nan-inf-zero-area', odd, godd)
    return cases


def run_case(case, dtype=np.float32, **kw):
    _, boxes, gts, labels, ignore, present, rule = case
    return assign(boxes, gts, labels, ignore, present, dtype=dtype, **dict(rule, **kw))


def batch_case():
    """N = 3 with different G per image and a G = 0 image in the middle: (boxes (3, 150, 4), [gts], [labels], rule)"""
    r = np.random.default_rng(2101)
    boxes = np.stack([rb(r, 150) for _ in range(3)])
    gts = [rb(r, 5), np.zeros((0, 4), dtype=np.float32), rb(r, 9)]
    return boxes, gts, [r.integers(0, 3, len(g)).astype(np.int64) for g in gts], dict(THRESHOLDS[0])


MARGIN_SEEDS = (102, 105, 107)


def margin_case(seed):
    r = np.random.default_rng(seed)
    g = rb(r, 7)
    b = rb(r, 600)
    return b, g


def margins(b, g):
    """the three fp64 distances of the issue: any IoU to 0.3 / 0.6 / 0.7, each ground truth's best to its second-best box, each box's best to
    its second-best ground truth over the boxes that overlap a ground truth at all (a box whose overlaps are all 0 ties exactly in either
    precision, and the tie rule decides)"""
    ov = overlaps(g, b, dtype=np.float64)
    thr = min(np.abs(ov - t).min() for t in (0.3, 0.6, 0.7))
    by_gt, by_box = np.sort(ov, axis=1), np.sort(ov, axis=0)
    return thr, (by_gt[:, -1] - by_gt[:, -2]).min(), (by_box[-1] - by_box[-2])[by_box[-1] > 0].min()


def delta_cases():
    """(boxes, gts) pairs for the delta bound: random pairs, boxes of 1-px width, ground truths 16x larger and smaller"""
    r = np.random.default_rng(2102)
    p, g = rb(r, 400), rb(r, 400)
    p[:50, 2] = p[:50, 0] + 1                                   # 1 px wide
    c, w = (p[50:100, :2] + p[50:100, 2:]) / 2, (p[50:100, 2:] - p[50:100, :2])
    g[50:100] = np.concatenate((c - w * 8, c + w * 8), axis=1)  # 16x larger
    c, w = (p[100:150, :2] + p[100:150, 2:]) / 2, (p[100:150, 2:] - p[100:150, :2])
    g[100:150] = np.concatenate((c - w / 32, c + w / 32), axis=1)   # 16x smaller
    return p.astype(np.float32), g.astype(np.float32)


RCNN_STDS = (0.1, 0.1, 0.2, 0.2)
