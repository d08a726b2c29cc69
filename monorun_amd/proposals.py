"""The proposal stage's ops: grouped axis-aligned NMS — mmcv's ``nms`` / ``batched_nms`` and mmdet's ``multiclass_nms`` —
and the RPN's fused proposal decode (mmdet's ``delta2bbox`` on the selected candidates), without mmcv, whose NMS is a CUDA extension with
no ROCm build.  :mod:`monorun_amd.rpn_head` builds ``RPNHeadMod.get_bboxes`` on them.

The NMS rule.  Boxes ``[x1, y1, x2, y2]`` in rank order inside a group; box i is kept iff it is valid and no kept box j < i of its group has
``iou(j, i) > thr``, with, every operation rounded to fp32 and no contraction,

    iw = max(min(ax2, bx2) − max(ax1, bx1), 0)   (ih alike),   inter = iw·ih,   area = (x2 − x1)(y2 − y1),
    iou = inter / ((area_a + area_b) − inter)

mmcv's ``offset=0`` arithmetic.  A NaN IoU does not suppress.  Ranks: score descending, TIES TO THE LOWER INPUT INDEX (mmcv leaves them to
``torch.sort``).  ``batched_nms`` runs the rule per distinct ``idxs`` value on the coordinates as they are: mmcv adds ``idx·(max + 1)`` to
them and runs one NMS, which moves fp32 coordinates and can flip a decision at the threshold — the one deliberate deviation.

Hot path: on CUDA fp32 with groups of at most 4096 boxes, :func:`nms_grouped` runs ``mr_nms_grouped`` (two HIP launches, no atomics, no
host synchronisation, bitwise reproducible) and :func:`proposal_decode` ``mr_proposal_decode`` (one launch).  Everything else — CPU
tensors, other dtypes, larger groups — runs the restatements :func:`nms_grouped_torch` and :func:`proposal_decode_torch`.
"""
import ctypes
import functools
import math

import numpy as np
import torch

from . import _lib

MAX_GROUP = 4096        # MR_NMS_MAX_GROUP of include/monorun_proposals.h
MAX_GROUPS = 65535      # MR_NMS_MAX_GROUPS
MAX_LEVELS = 8          # MR_PROPOSAL_MAX_LEVELS
MAX_ANCHORS = 16        # MR_PROPOSAL_MAX_ANCHORS
WH_RATIO_CLIP = 16 / 1000


def host_to_device(values, dtype, device):
    """A small host list as a tensor on ``device`` without a blocking copy (pinned memory, ``non_blocking``): the padded RPN path performs
    no host synchronisation."""
    t = torch.tensor(values, dtype=dtype)
    if torch.device(device).type != 'cuda':
        return t.to(device)
    return t.pin_memory().to(device, non_blocking=True)


@functools.lru_cache(maxsize=64)
def _offsets(sizes, device):
    return host_to_device([0] + list(np.cumsum(sizes, dtype=np.int64)), torch.int32, device)


# ------------------------------------------------------------------------------------------------ grouped NMS
def iou_row_f32(box, others):
    """The rule's IoU of one box (4,) with boxes (m, 4), numpy float32 operation for operation."""
    with np.errstate(all='ignore'):
        iw = np.maximum(np.minimum(box[2], others[:, 2]) - np.maximum(box[0], others[:, 0]), np.float32(0))
        ih = np.maximum(np.minimum(box[3], others[:, 3]) - np.maximum(box[1], others[:, 1]), np.float32(0))
        inter = iw * ih
        area_a = (box[2] - box[0]) * (box[3] - box[1])
        area_b = (others[:, 2] - others[:, 0]) * (others[:, 3] - others[:, 1])
        return inter / ((area_a + area_b) - inter)


def nms_grouped_torch(boxes, valid, sizes, thr):
    """The restatement of ``mr_nms_grouped``: the rule in numpy float32 on the host, any device or floating dtype in (computed in fp32).
    -> keep (T,) uint8, num_keep (G,) int32 on ``boxes``' device."""
    b = boxes.detach().to(torch.float32).cpu().numpy().reshape(-1, 4)
    v = np.ones(b.shape[0], dtype=bool) if valid is None else valid.detach().cpu().numpy().astype(bool)
    thr = np.float32(thr)
    keep = np.zeros(b.shape[0], dtype=np.uint8)
    counts = np.zeros(len(sizes), dtype=np.int32)
    first = 0
    for g, n in enumerate(sizes):
        bg = b[first:first + n]
        removed = ~v[first:first + n]
        for i in range(n):
            if removed[i]:
                continue
            keep[first + i] = 1
            if i + 1 < n:
                removed[i + 1:] |= iou_row_f32(bg[i], bg[i + 1:]) > thr
        counts[g] = keep[first:first + n].sum()
        first += n
    return torch.from_numpy(keep).to(boxes.device), torch.from_numpy(counts).to(boxes.device)


def hip_ok(boxes, sizes):
    """Whether ``mr_nms_grouped`` covers this call: CUDA fp32 boxes (T, 4), at most 65535 groups of at most 4096 boxes."""
    if not isinstance(boxes, torch.Tensor) or boxes.device.type != 'cuda' or boxes.dtype != torch.float32:
        return False
    return boxes.dim() == 2 and boxes.shape[1] == 4 and len(sizes) <= MAX_GROUPS and max(sizes, default=0) <= MAX_GROUP


def nms_workspace_bytes(sizes):
    g = len(sizes)
    return int(_lib.load().mr_nms_workspace_bytes((ctypes.c_int * max(g, 1))(*sizes), g, max(sizes, default=0)))


def nms_grouped(boxes, valid, sizes, thr):
    """Greedy NMS inside each group.  boxes (T, 4) in rank order inside each group, valid (T,) uint8 / bool or None, sizes: the group sizes,
    host integers summing to T (the grid and the workspace are sized from them).  -> keep (T,) uint8, num_keep (G,) int32.  The two HIP
    launches when :func:`hip_ok`, else :func:`nms_grouped_torch`.  No host synchronisation on the HIP path."""
    sizes = tuple(int(s) for s in sizes)
    assert boxes.dim() == 2 and boxes.shape[1] == 4 and sum(sizes) == boxes.shape[0] and min(sizes, default=0) >= 0, 'nms_grouped: sizes'
    if valid is not None:
        valid = valid.to(torch.uint8) if valid.dtype != torch.uint8 else valid
    if not hip_ok(boxes, sizes):
        return nms_grouped_torch(boxes, valid, sizes, thr)
    dev = boxes.device
    keep = torch.zeros(boxes.shape[0], dtype=torch.uint8, device=dev)
    num_keep = torch.zeros(len(sizes), dtype=torch.int32, device=dev)
    if boxes.shape[0] == 0:
        return keep, num_keep
    boxes = boxes.detach().contiguous()
    ws = torch.empty(max(nms_workspace_bytes(sizes) // 8, 1), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        offsets = _offsets(sizes, dev)
        _lib.call('mr_nms_grouped', boxes=boxes.data_ptr(), valid=_lib.ptr(valid.contiguous() if valid is not None else None),
                  offsets=offsets.data_ptr(), groups=len(sizes), max_group=max(sizes), thr=float(thr), keep=keep.data_ptr(),
                  num_keep=num_keep.data_ptr(), workspace=ws.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
    return keep, num_keep


def _dets(boxes, scores, keep):
    return torch.cat((boxes[keep], scores[keep][:, None].to(boxes.dtype)), dim=1), keep


def nms(boxes, scores, iou_threshold):
    """mmcv's ``nms``: boxes (n, 4), scores (n,) -> (dets (k, 5), keep (k,) int64), score descending, ties to the lower input index."""
    assert boxes.dim() == 2 and boxes.shape[1] == 4 and scores.shape == boxes.shape[:1], 'nms: boxes (n, 4), scores (n,)'
    order = torch.sort(scores, descending=True, stable=True)[1]
    flags = nms_grouped(boxes[order], None, (boxes.shape[0],), iou_threshold)[0]
    return _dets(boxes, scores, order[flags.bool()])


def parse_nms_cfg(nms_cfg, class_agnostic=False):
    """(iou threshold, class_agnostic) of an mmcv ``nms_cfg``: ``type='nms'`` only, ``iou_threshold`` or the legacy ``iou_thr``;
    ``split_thr`` is ignored (the grouped kernel has no size at which another method takes over)."""
    cfg = dict(nms_cfg)
    class_agnostic = cfg.pop('class_agnostic', class_agnostic)
    kind = cfg.pop('type', 'nms')
    if kind != 'nms':
        raise NotImplementedError(f"nms_cfg type {kind!r} is not provided ('nms' only)")
    cfg.pop('split_thr', None)
    if 'iou_threshold' in cfg:
        thr = cfg.pop('iou_threshold')
        cfg.pop('iou_thr', None)
    elif 'iou_thr' in cfg:
        thr = cfg.pop('iou_thr')
    else:
        raise KeyError('nms_cfg: iou_threshold')
    if cfg:
        raise TypeError(f'nms_cfg: unknown keys {sorted(cfg)}')
    return float(thr), bool(class_agnostic)


def batched_nms(boxes, scores, idxs, nms_cfg, class_agnostic=False):
    """mmcv's ``batched_nms``: NMS per distinct value of ``idxs`` (n,), on the coordinates as they are.  -> (dets (k, 5), keep (k,) int64)
    in score-descending order, ties to the lower input index.  Synchronises once, to learn the group sizes."""
    thr, class_agnostic = parse_nms_cfg(nms_cfg, class_agnostic)
    if class_agnostic:
        return nms(boxes, scores, thr)
    assert boxes.dim() == 2 and boxes.shape[1] == 4 and scores.shape == boxes.shape[:1] == idxs.shape, 'batched_nms: shapes'
    order1 = torch.sort(scores, descending=True, stable=True)[1]
    order2 = torch.sort(idxs[order1], stable=True)[1]
    perm = order1[order2]
    sizes = torch.unique_consecutive(idxs[perm], return_counts=True)[1].tolist()
    flags = nms_grouped(boxes[perm], None, sizes, thr)[0]
    by_score = torch.empty_like(flags)
    by_score[order2] = flags
    return _dets(boxes, scores, order1[by_score.bool()])


def multiclass_nms(multi_bboxes, multi_scores, score_thr, nms_cfg, max_num=-1, score_factors=None):
    """mmdet's ``multiclass_nms``: multi_bboxes (K, 4) or (K, 4C), multi_scores (K, C + 1) (the last column is the background) ->
    (dets (k, 5), labels (k,) int64).  The candidates are the (box, class) pairs with ``score > score_thr``; ``score_factors`` (K,)
    multiply the scores after that test; NMS per class; score descending, ties to the lower candidate (box-major, class-minor); the first
    ``max_num``.  The groups are the C classes with K boxes each and the threshold a ``valid`` flag: the sizes are static, so the only
    synchronisation is the final count."""
    thr, _ = parse_nms_cfg(nms_cfg)
    K, C = multi_scores.shape[0], multi_scores.shape[1] - 1
    bboxes = multi_bboxes.reshape(K, -1, 4) if multi_bboxes.shape[1] > 4 else multi_bboxes[:, None].expand(K, C, 4)
    assert bboxes.shape == (K, C, 4), 'multiclass_nms: multi_bboxes (K, 4) or (K, 4C)'
    scores = multi_scores[:, :C]
    valid = scores > score_thr
    if score_factors is not None:
        scores = scores * score_factors[:, None]
    if K == 0 or C == 0:
        return multi_bboxes.new_zeros((0, 5)), torch.zeros(0, dtype=torch.int64, device=multi_bboxes.device)
    order = torch.sort(scores.t(), dim=1, descending=True, stable=True)[1]                          # (C, K): each class's ranks
    cls = torch.arange(C, device=order.device)[:, None].expand(C, K)
    ranked = bboxes[order, cls]                                                                     # (C, K, 4)
    flags = nms_grouped(ranked.reshape(-1, 4), valid.t().gather(1, order).reshape(-1), (K,) * C, thr)[0]
    kept = torch.zeros(K * C, dtype=torch.bool, device=order.device)
    kept[(order * C + cls).reshape(-1)] = flags.bool()                                              # in candidate order k C + c
    flat = scores.reshape(-1)
    by_score = torch.sort(flat, descending=True, stable=True)[1]
    sel = by_score[kept[by_score]]
    if max_num > 0:
        sel = sel[:max_num]
    dets = torch.cat((bboxes.reshape(-1, 4)[sel], flat[sel][:, None].to(bboxes.dtype)), dim=1)
    return dets, sel % C


# ------------------------------------------------------------------------------------------------ proposal decode
def max_ratio(wh_ratio_clip=WH_RATIO_CLIP):
    """The clamp of dw, dh: ``|log(wh_ratio_clip)|`` rounded to fp32, as the kernel receives it."""
    return float(np.float32(abs(math.log(wh_ratio_clip))))


def proposal_decode_torch(cls_scores, bbox_preds, index, counts, img_shape, base_anchors, strides, means, stds,
                          wh_ratio_clip=WH_RATIO_CLIP, min_bbox_size=0):
    """The restatement of ``mr_proposal_decode`` in fp32 torch ops on any device: the arguments and results of :func:`proposal_decode`."""
    N = cls_scores[0].shape[0]
    f = dict(dtype=torch.float32, device=cls_scores[0].device)
    logits, deltas, anchors = [], [], []
    first = 0
    for l, (c, r, k) in enumerate(zip(cls_scores, bbox_preds, counts)):
        A, (H, W) = c.shape[1], c.shape[2:]
        t = index[:, first:first + k]
        first += k
        logits.append(c.to(torch.float32).permute(0, 2, 3, 1).reshape(N, -1).gather(1, t))
        d = r.to(torch.float32).permute(0, 2, 3, 1).reshape(N, -1, 4)
        deltas.append(d.gather(1, t[..., None].expand(-1, -1, 4)))
        cell, a = torch.div(t, A, rounding_mode='floor'), t % A
        x, y = (cell % W).to(torch.float32) * float(strides[l]), torch.div(cell, W, rounding_mode='floor').to(torch.float32) * float(strides[l])
        anchors.append(base_anchors[l].to(**f)[a] + torch.stack((x, y, x, y), dim=-1))
    logit, d, an = torch.cat(logits, 1), torch.cat(deltas, 1), torch.cat(anchors, 1)
    d = d * torch.tensor(list(stds), **f) + torch.tensor(list(means), **f)
    m = max_ratio(wh_ratio_clip)
    dw, dh = d[..., 2].clamp(-m, m), d[..., 3].clamp(-m, m)
    px, py = (an[..., 0] + an[..., 2]) * 0.5, (an[..., 1] + an[..., 3]) * 0.5
    pw, ph = an[..., 2] - an[..., 0], an[..., 3] - an[..., 1]
    gw, gh = pw * torch.exp(dw), ph * torch.exp(dh)
    gx, gy = px + pw * d[..., 0], py + ph * d[..., 1]
    shape = img_shape.to(**f)
    zero, img_h, img_w = torch.zeros((), **f), shape[:, 0:1], shape[:, 1:2]
    x1, x2 = torch.minimum(torch.maximum(gx - gw * 0.5, zero), img_w), torch.minimum(torch.maximum(gx + gw * 0.5, zero), img_w)
    y1, y2 = torch.minimum(torch.maximum(gy - gh * 0.5, zero), img_h), torch.minimum(torch.maximum(gy + gh * 0.5, zero), img_h)
    boxes = torch.stack((x1, y1, x2, y2), dim=-1)
    score = 1.0 / (1.0 + torch.exp(-logit))
    valid = torch.ones_like(logit, dtype=torch.uint8)
    if min_bbox_size > 0:
        valid = (~((x2 - x1 < min_bbox_size) | (y2 - y1 < min_bbox_size))).to(torch.uint8)
    return boxes, score, logit, valid


def decode_hip_ok(cls_scores, bbox_preds, index):
    """Whether ``mr_proposal_decode`` covers this call: CUDA fp32 head outputs on one device, at most 8 levels and 16 base anchors."""
    if not cls_scores or len(cls_scores) > MAX_LEVELS or len(cls_scores) != len(bbox_preds):
        return False
    dev, (N, A) = cls_scores[0].device, cls_scores[0].shape[:2]
    if dev.type != 'cuda' or index.device != dev or A > MAX_ANCHORS or N * len(cls_scores) > 65535:
        return False
    for c, r in zip(cls_scores, bbox_preds):
        if c.device != dev or r.device != dev or c.dtype != torch.float32 or r.dtype != torch.float32 or r.numel() > 2 ** 31 - 1:
            return False
    return index.numel() <= 2 ** 31 - 1


def proposal_decode(cls_scores, bbox_preds, index, counts, img_shape, base_anchors, strides, means, stds,
                    wh_ratio_clip=WH_RATIO_CLIP, min_bbox_size=0):
    """Decode the selected candidates of every image and level.  cls_scores[l] (N, A, H_l, W_l), bbox_preds[l] (N, 4A, H_l, W_l): the
    head's outputs; index (N, P) int64, P = sum(counts): per image the counts[l] flat anchor indices ``(y·W_l + x)·A + a`` of each level
    in rank order, level after level; img_shape (N, 2) = [img_h, img_w] on the device; base_anchors[l] (A, 4).  -> boxes (N, P, 4), score
    (N, P), logit (N, P) fp32, valid (N, P) uint8.  ONE HIP launch when :func:`decode_hip_ok` (head outputs that are not contiguous are
    copied first), else :func:`proposal_decode_torch`."""
    cls_scores, bbox_preds, counts = list(cls_scores), list(bbox_preds), [int(k) for k in counts]
    N, P = index.shape
    assert P == sum(counts) and len(counts) == len(cls_scores) == len(bbox_preds) == len(strides), 'proposal_decode: one count per level'
    args = (img_shape, base_anchors, strides, means, stds, wh_ratio_clip, min_bbox_size)
    if not decode_hip_ok(cls_scores, bbox_preds, index):
        return proposal_decode_torch(cls_scores, bbox_preds, index, counts, *args)
    dev, L, A = index.device, len(counts), cls_scores[0].shape[1]
    boxes = torch.empty(N, P, 4, dtype=torch.float32, device=dev)
    score, logit = torch.empty(N, P, dtype=torch.float32, device=dev), torch.empty(N, P, dtype=torch.float32, device=dev)
    valid = torch.empty(N, P, dtype=torch.uint8, device=dev)
    if N * P == 0:
        return boxes, score, logit, valid
    cls_scores = [c.detach().contiguous() for c in cls_scores]
    bbox_preds = [r.detach().contiguous() for r in bbox_preds]
    index = index.contiguous()
    shape = img_shape.to(device=dev, dtype=torch.float32).contiguous()
    base = np.stack([np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b, dtype=np.float32).reshape(A, 4) for b in base_anchors])
    i32, f4 = ctypes.c_int * L, ctypes.c_float * 4
    with torch.cuda.device(dev):
        _lib.call('mr_proposal_decode', cls=(ctypes.c_void_p * L)(*[c.data_ptr() for c in cls_scores]),
                  reg=(ctypes.c_void_p * L)(*[r.data_ptr() for r in bbox_preds]), level_h=i32(*[c.shape[2] for c in cls_scores]),
                  level_w=i32(*[c.shape[3] for c in cls_scores]), level_stride=i32(*[int(s) for s in strides]), level_count=i32(*counts),
                  base_anchors=(ctypes.c_float * base.size)(*base.reshape(-1).tolist()), n_levels=L, n_anchors=A, n_images=N,
                  index=index.data_ptr(), img_shape=shape.data_ptr(), means=f4(*[float(m) for m in means]), stds=f4(*[float(s) for s in stds]),
                  wh_ratio_clip=float(wh_ratio_clip), min_bbox_size=float(min_bbox_size), boxes=boxes.data_ptr(), score=score.data_ptr(),
                  logit=logit.data_ptr(), valid=valid.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
    return boxes, score, logit, valid
