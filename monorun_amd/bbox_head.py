"""The 2-D detection head: mmdet's ``Shared2FCBBoxHead`` as the reference configures it (configs/kitti_multiclass.py:44-62)
and its ``get_bboxes`` — softmax, ``delta2bbox`` per class, the clamp, the rescale and ``multiclass_nms`` — without mmdet or mmcv.  It
stands between :mod:`monorun_amd.roi_extractor` and the 3-D stage in ``MonoRUnRoIHead.simple_test``.

The rule, per RoI r of image n with logits ``x[0..C]`` (background last), every operation rounded to fp32:

    score_c = e_c / s,  e_j = exp(x_j − max_j x_j),  s = e_0 + e_1 + … in index order
    box_c   = §19's delta2bbox of ``rois[r, 1:5]`` and ``bbox_pred[r, 4c:4c+4]`` (columns 0:4 when class-agnostic), clamped to the image's
              ``[0, img_w] × [0, img_h]``; with ``rescale`` each coordinate divided by the matching entry of the image's ``scale_factor``
    valid   = score_c > score_thr and the four RoI coordinates finite (the NaN rows of a padded proposal list give no detection)
    ranks inside group (n, c): score descending, NaN after every number, ties to the lower RoI, over all RoIs of the image
    NMS per group: §19's rule on the ranked (rescaled) boxes with the valid flags
    per image: the kept candidates by score descending, ties to the lower candidate ``r·C + c``, the first ``max_per_img``

Hot path: on CUDA fp32 within the caps (4096 RoIs per image, 16 classes) ``get_bboxes`` with a ``cfg`` is ``mr_bbox_head_detect`` — four
HIP launches (rank, the NMS's two, select), no atomics, bitwise reproducible — and ``padded=True`` performs no host synchronisation.
Everything else runs :func:`bbox_head_rank_torch`, :func:`monorun_amd.proposals.nms_grouped` and :func:`select_torch`: the same rule.

Training: ``get_targets``, ``loss``, ``accuracy``, ``regress_by_class`` and ``refine_bboxes`` are mmdet's ``BBoxHead`` ones
on the sampling results of :mod:`monorun_amd.assigners`, in torch; ``get_targets`` also takes a ``BatchSamplingResult`` and then, like
``loss``, performs no host synchronisation.

Not provided: ``with_avg_pool``, other ``ConvFCBBoxHead`` shapes.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from . import proposals as P
from .assigners import BatchSamplingResult, _ascending, bbox2delta
from .detection_losses import resolve
from .losses import UnbuiltLoss, build_loss

MAX_ROIS = 4096         # MR_BBOX_MAX_ROIS of include/monorun_bbox.h
MAX_CLASSES = 16        # MR_BBOX_MAX_CLASSES
MAX_IMAGES = 4095       # MR_BBOX_MAX_IMAGES


# ------------------------------------------------------------------------------------------------ mmdet's helpers
def bbox2roi(bbox_list):
    """mmdet's ``bbox2roi``: per-image boxes (k_n, 4) or (k_n, 5) -> (sum k_n, 5) ``[image, x1, y1, x2, y2]``, image-major."""
    rois = []
    for n, b in enumerate(bbox_list):
        if b.shape[0] > 0:
            rois.append(torch.cat((b.new_full((b.shape[0], 1), n), b[:, :4]), dim=-1))
        else:
            rois.append(b.new_zeros((0, 5)))
    return torch.cat(rois, 0)


def bbox2result(bboxes, labels, num_classes):
    """mmdet's ``bbox2result``: detections (k, 5) and labels (k,) -> a list of ``num_classes`` numpy arrays (k_c, 5)."""
    if bboxes.shape[0] == 0:
        return [np.zeros((0, 5), dtype=np.float32) for _ in range(num_classes)]
    if isinstance(bboxes, torch.Tensor):
        bboxes, labels = bboxes.detach().cpu().numpy(), labels.detach().cpu().numpy()
    return [bboxes[labels == c, :] for c in range(num_classes)]


def register_with_mmdet():
    """Register ``Shared2FCBBoxHead`` under mmdet's HEADS registry in place of mmdet's own, if mmdet is importable (-> True)."""
    try:
        from mmdet.models.builder import HEADS
    except ImportError:
        return False
    HEADS.register_module(name='Shared2FCBBoxHead', force=True, module=Shared2FCBBoxHead)
    return True


# ------------------------------------------------------------------------------------------------ the rule in torch ops
def softmax_torch(cls_score):
    """The rule's scores (R, C + 1) in fp32 torch ops: the sum in index order."""
    x = cls_score.to(torch.float32)
    e = torch.exp(x - x.max(dim=1, keepdim=True)[0])
    s = e[:, 0]
    for j in range(1, e.shape[1]):
        s = s + e[:, j]
    return e / s[:, None]


def decode_torch(rois, bbox_pred, img_hw, scale, means, stds, wh_ratio_clip=P.WH_RATIO_CLIP):
    """The rule's boxes (R, G, 4), G = bbox_pred's groups of four, in fp32 torch ops.  rois (R, 5); img_hw (R, 2) [img_h, img_w] of each
    row's image; scale (R, 4) or None."""
    f = dict(dtype=torch.float32, device=rois.device)
    R = rois.shape[0]
    d = bbox_pred.to(torch.float32).reshape(R, bbox_pred.shape[-1] // 4, 4)
    d = [d[..., k] * float(stds[k]) + float(means[k]) for k in range(4)]      # scalars: rounded to fp32 by the op, no tensor to copy over
    m = P.max_ratio(wh_ratio_clip)
    dw, dh = d[2].clamp(-m, m), d[3].clamp(-m, m)
    r = rois.to(torch.float32)[:, None, 1:5]
    px, py = (r[..., 0] + r[..., 2]) * 0.5, (r[..., 1] + r[..., 3]) * 0.5
    pw, ph = r[..., 2] - r[..., 0], r[..., 3] - r[..., 1]
    gw, gh = pw * torch.exp(dw), ph * torch.exp(dh)
    gx, gy = px + pw * d[0], py + ph * d[1]
    zero, img_h, img_w = torch.zeros((), **f), img_hw.to(**f)[:, 0:1], img_hw.to(**f)[:, 1:2]
    x1, x2 = torch.minimum(torch.maximum(gx - gw * 0.5, zero), img_w), torch.minimum(torch.maximum(gx + gw * 0.5, zero), img_w)
    y1, y2 = torch.minimum(torch.maximum(gy - gh * 0.5, zero), img_h), torch.minimum(torch.maximum(gy + gh * 0.5, zero), img_h)
    boxes = torch.stack((x1, y1, x2, y2), dim=-1)
    return boxes if scale is None else boxes / scale.to(**f)[:, None, :]


def _per_row(table, counts):
    """A per-image table (N, k) repeated to the rows of the images."""
    index = P.host_to_device(np.repeat(np.arange(len(counts)), list(counts)).tolist(), torch.int64, table.device)
    return table[index]


def bbox_head_rank_torch(rois, cls_score, bbox_pred, counts, img_shape, scale, num_classes, reg_class_agnostic, means, stds, score_thr,
                         wh_ratio_clip=P.WH_RATIO_CLIP):
    """The restatement of ``mr_bbox_head_rank`` in fp32 torch ops on any device: the arguments and results of :func:`rank`."""
    C, dev = num_classes, rois.device
    score_all = softmax_torch(cls_score)[:, :C]
    boxes_all = decode_torch(rois, bbox_pred, _per_row(img_shape, counts), None if scale is None else _per_row(scale, counts), means, stds,
                             wh_ratio_clip)
    if boxes_all.shape[1] == 1:
        boxes_all = boxes_all.expand(-1, C, -1)
    finite = torch.isfinite(rois[:, 1:5].to(torch.float32)).all(dim=1)
    valid_all = (score_all > score_thr) & finite[:, None]
    boxes, score, order, valid = [], [], [], []
    first = 0
    for k in counts:
        sl = slice(first, first + k)
        first += k
        s = score_all[sl].t()                                                                       # (C, k)
        o = torch.sort(torch.where(torch.isnan(s), torch.full_like(s, -1.0), s), dim=1, descending=True, stable=True)[1]
        cls = torch.arange(C, device=dev)[:, None].expand(C, k)
        boxes.append(boxes_all[sl][o, cls].reshape(-1, 4))
        score.append(s.gather(1, o).reshape(-1))
        order.append(o.reshape(-1).to(torch.int32))
        valid.append(valid_all[sl].t().gather(1, o).reshape(-1).to(torch.uint8))
    if not boxes:
        z = torch.zeros(0, dtype=torch.float32, device=dev)
        return z.reshape(0, 4), z, z.to(torch.int32), z.to(torch.uint8)
    return torch.cat(boxes), torch.cat(score), torch.cat(order), torch.cat(valid)


def select_torch(boxes, score, order, keep, counts, num_classes, max_num):
    """The restatement of ``mr_bbox_head_select``: per image the kept candidates of the groups' layout by score descending, ties to the
    lower candidate ``order·C + c``, the first ``max_num`` (all when ``max_num <= 0``).  -> [(dets (k_n, 5), labels (k_n,) int64)]."""
    C, out, first = num_classes, [], 0
    for k in counts:
        sl = slice(first, first + C * k)
        first += C * k
        cls = torch.arange(C, device=boxes.device)[:, None].expand(C, k).reshape(-1)
        cand = order[sl].to(torch.int64) * C + cls
        by_cand = torch.sort(cand, stable=True)[1]
        by_cand = by_cand[keep[sl][by_cand].bool()]
        sel = by_cand[torch.sort(score[sl][by_cand], descending=True, stable=True)[1]]
        if max_num > 0:
            sel = sel[:max_num]
        out.append((torch.cat((boxes[sl][sel], score[sl][sel][:, None]), dim=1), cls[sel]))
    return out


# ------------------------------------------------------------------------------------------------ the HIP launches
def hip_ok(rois, cls_score, bbox_pred, counts, num_classes):
    """Whether the HIP launches cover this call: CUDA fp32 tensors on one device, at most 4096 RoIs per image, 16 classes, 4095 images."""
    for t in (rois, cls_score, bbox_pred):
        if not isinstance(t, torch.Tensor) or t.device.type != 'cuda' or t.dtype != torch.float32 or t.device != rois.device:
            return False
    return (1 <= num_classes <= MAX_CLASSES and len(counts) <= MAX_IMAGES and max(counts, default=0) <= MAX_ROIS
            and 4 * rois.shape[0] * num_classes <= 2 ** 31 - 1)


def _launch_inputs(rois, cls_score, bbox_pred, counts, img_shape, scale):
    """The device inputs of a launch as contiguous tensors, bound to names that live across it (a temporary's block would go back to the
    caching allocator, and to the next copy, before the kernel reads it): rois, cls_score, bbox_pred, row offsets, img_shape, scale."""
    return (rois.detach().contiguous(), cls_score.detach().contiguous(), bbox_pred.detach().contiguous(), P._offsets(tuple(counts), rois.device),
            img_shape.contiguous(), None if scale is None else scale.contiguous())


def _coder_args(means, stds, wh_ratio_clip):
    f4 = ctypes.c_float * 4
    return dict(means=f4(*[float(m) for m in means]), stds=f4(*[float(s) for s in stds]), wh_ratio_clip=float(wh_ratio_clip))


def rank(rois, cls_score, bbox_pred, counts, img_shape, scale, num_classes, reg_class_agnostic, means, stds, score_thr,
         wh_ratio_clip=P.WH_RATIO_CLIP):
    """Score, rank and decode the candidates of every (image, class).  rois (R, 5), cls_score (R, C + 1), bbox_pred (R, 4C) or (R, 4);
    counts: the RoIs of each image, host integers summing to R; img_shape (N, 2) fp32 [img_h, img_w] and scale (N, 4) fp32 or None on the
    device.  -> boxes (T, 4), score (T,), order (T,) int32, valid (T,) uint8 in the groups' layout, T = R·C: group (n, c) holds the
    counts[n] RoIs of image n in rank order for class c, image-major.  ONE HIP launch when :func:`hip_ok`, else
    :func:`bbox_head_rank_torch`."""
    counts = [int(k) for k in counts]
    R, C = rois.shape[0], int(num_classes)
    assert sum(counts) == R and cls_score.shape == (R, C + 1) and bbox_pred.shape == (R, 4 if reg_class_agnostic else 4 * C), 'rank: shapes'
    if not hip_ok(rois, cls_score, bbox_pred, counts, C):
        return bbox_head_rank_torch(rois, cls_score, bbox_pred, counts, img_shape, scale, C, reg_class_agnostic, means, stds, score_thr,
                                    wh_ratio_clip)
    dev, T = rois.device, R * C
    boxes = torch.empty(T, 4, dtype=torch.float32, device=dev)
    score = torch.empty(T, dtype=torch.float32, device=dev)
    order = torch.empty(T, dtype=torch.int32, device=dev)
    valid = torch.empty(T, dtype=torch.uint8, device=dev)
    if T == 0:
        return boxes, score, order, valid
    groups = torch.empty(len(counts) * C + 1, dtype=torch.int32, device=dev)
    rois, cls_score, bbox_pred, offsets, img_shape, scale = _launch_inputs(rois, cls_score, bbox_pred, counts, img_shape, scale)
    with torch.cuda.device(dev):
        _lib.call('mr_bbox_head_rank', _coder_args(means, stds, wh_ratio_clip), cls_score=cls_score.data_ptr(), bbox_pred=bbox_pred.data_ptr(),
                  rois=rois.data_ptr(), row_offsets=offsets.data_ptr(), img_shape=img_shape.data_ptr(), scale_factor=_lib.ptr(scale), n_rois=R,
                  n_images=len(counts), num_classes=C, reg_class_agnostic=int(bool(reg_class_agnostic)), max_rois=max(counts),
                  score_thr=float(score_thr), boxes=boxes.data_ptr(), score=score.data_ptr(), order=order.data_ptr(), valid=valid.data_ptr(),
                  group_offsets=groups.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
    return boxes, score, order, valid


def _empty_padded(N, max_num, dev):
    return (torch.full((N, max_num, 5), float('nan'), dtype=torch.float32, device=dev),
            torch.full((N, max_num), -1, dtype=torch.int64, device=dev), torch.zeros(N, dtype=torch.int32, device=dev))


def detect(rois, cls_score, bbox_pred, counts, img_shape, scale, num_classes, reg_class_agnostic, means, stds, score_thr, iou_thr, max_num,
           wh_ratio_clip=P.WH_RATIO_CLIP):
    """The whole stage, padded: :func:`rank`'s arguments, the NMS threshold and ``max_num`` > 0 -> dets (N, max_num, 5), labels
    (N, max_num) int64, counts (N,) int32; rows past the count are NaN, their labels −1.  ``mr_bbox_head_detect`` (four launches, no host
    synchronisation) when :func:`hip_ok`, else the restatements."""
    counts = [int(k) for k in counts]
    R, C, N, dev = rois.shape[0], int(num_classes), len(counts), rois.device
    assert max_num > 0, 'detect: max_num > 0 (the padded form has max_num rows per image)'
    assert sum(counts) == R and cls_score.shape == (R, C + 1) and bbox_pred.shape == (R, 4 if reg_class_agnostic else 4 * C), 'detect: shapes'
    dets, labels, num = _empty_padded(N, max_num, dev)
    if R == 0 or N == 0:
        return dets, labels, num
    if not hip_ok(rois, cls_score, bbox_pred, counts, C):
        boxes, score, order, valid = bbox_head_rank_torch(rois, cls_score, bbox_pred, counts, img_shape, scale, C, reg_class_agnostic, means,
                                                          stds, score_thr, wh_ratio_clip)
        keep = P.nms_grouped(boxes, valid, [k for k in counts for _ in range(C)], iou_thr)[0]
        for n, (d, l) in enumerate(select_torch(boxes, score, order, keep, counts, C, max_num)):
            dets[n, :len(d)], labels[n, :len(d)], num[n] = d, l, len(d)
        return dets, labels, num
    rois, cls_score, bbox_pred, offsets, img_shape, scale = _launch_inputs(rois, cls_score, bbox_pred, counts, img_shape, scale)
    with torch.cuda.device(dev):
        ws_bytes = int(_lib.load().mr_bbox_head_workspace_bytes(R, N, C, max(counts)))
        ws = torch.empty(ws_bytes // 8 + 1, dtype=torch.int64, device=dev)
        _lib.call('mr_bbox_head_detect', _coder_args(means, stds, wh_ratio_clip), cls_score=cls_score.data_ptr(), bbox_pred=bbox_pred.data_ptr(),
                  rois=rois.data_ptr(), row_offsets=offsets.data_ptr(), img_shape=img_shape.data_ptr(), scale_factor=_lib.ptr(scale), n_rois=R,
                  n_images=N, num_classes=C, reg_class_agnostic=int(bool(reg_class_agnostic)), max_rois=max(counts), score_thr=float(score_thr),
                  iou_thr=float(iou_thr), max_num=int(max_num), dets=dets.data_ptr(), labels=labels.data_ptr(), counts=num.data_ptr(),
                  workspace=ws.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
    return dets, labels, num


# ------------------------------------------------------------------------------------------------ the module
def _cfg_get(cfg, key):
    return cfg[key] if isinstance(cfg, dict) else getattr(cfg, key)


def _is_per_image(value):
    """Whether ``img_shape`` / ``scale_factor`` is a list with one entry per image (its entries are sequences or arrays themselves)."""
    return isinstance(value, (list, tuple)) and len(value) > 0 and isinstance(value[0], (list, tuple, np.ndarray, torch.Tensor))


def _scale_rows(scale_factor, N, dev):
    """(N, 4) fp32 on ``dev`` from a scalar or a 4-vector (array, tensor, sequence of four numbers) for all images, or a list with one
    entry per image whose entries are arrays, tensors or sequences themselves (of one or of four numbers).  A flat sequence of numbers is
    always ONE 4-vector — per-image scalar factors go as ``[[f0], [f1], ...]`` — and any other length raises.  No blocking copy."""
    if isinstance(scale_factor, torch.Tensor):
        t = scale_factor.to(device=dev, dtype=torch.float32)
        return (t.reshape(1, -1) if t.dim() < 2 else t).expand(N, 4)
    if isinstance(scale_factor, (list, tuple)) and not _is_per_image(scale_factor) and len(scale_factor) != 4:
        raise ValueError('scale_factor: a flat sequence is one 4-vector; give per-image factors as one sequence or array per image')
    per_image = scale_factor if _is_per_image(scale_factor) else [scale_factor] * N
    rows = []
    for s in per_image:
        if isinstance(s, torch.Tensor):
            s = s.detach().cpu().numpy()
        s = np.asarray(s, dtype=np.float32).reshape(-1)
        rows.append([float(v) for v in (np.repeat(s, 4) if s.size == 1 else s)])
    assert len(rows) == N and all(len(r) == 4 for r in rows), 'scale_factor: a scalar or four entries, one per image'
    return P.host_to_device(rows, torch.float32, dev)


def _build_loss(cfg):
    """``losses.build_loss``; a form of a known loss that is not restated (the softmax cross entropy of this head's ``loss_cls``) stands
    unbuilt like an unknown one: the head constructs and runs, calling the loss raises."""
    try:
        return build_loss(cfg)
    except NotImplementedError:
        return UnbuiltLoss(cfg)


class Shared2FCBBoxHead(nn.Module):
    """mmdet's ``Shared2FCBBoxHead``: two shared FCs with ReLU on the flattened RoI feature, ``fc_cls`` (``num_classes + 1`` logits, the
    background last) and ``fc_reg`` (``4·num_classes`` deltas, or 4 when class-agnostic); mmdet's parameter names, so a checkpoint's
    ``roi_head.bbox_head.*`` loads with ``strict=True``."""

    def __init__(self, in_channels=256, fc_out_channels=1024, roi_feat_size=7, num_classes=80,
                 bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=(.0, .0, .0, .0), target_stds=(0.1, 0.1, 0.2, 0.2)),
                 reg_class_agnostic=False, loss_cls=None, loss_bbox=None, train_cfg=None, test_cfg=None, **kwargs):
        super().__init__()
        coder = dict(bbox_coder)
        kind = coder.pop('type', 'DeltaXYWHBBoxCoder')
        if kind != 'DeltaXYWHBBoxCoder':
            raise NotImplementedError(f'bbox_coder type {kind!r} is not provided (DeltaXYWHBBoxCoder only)')
        self.in_channels, self.fc_out_channels, self.num_classes = in_channels, fc_out_channels, int(num_classes)
        self.roi_feat_size = (roi_feat_size, roi_feat_size) if isinstance(roi_feat_size, int) else tuple(roi_feat_size)
        self.reg_class_agnostic = bool(reg_class_agnostic)
        self.target_means = tuple(float(m) for m in coder.get('target_means', (0.0,) * 4))
        self.target_stds = tuple(float(s) for s in coder.get('target_stds', (1.0,) * 4))
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.loss_cls, self.loss_bbox = _build_loss(loss_cls), _build_loss(loss_bbox)
        area = self.roi_feat_size[0] * self.roi_feat_size[1]
        self.shared_fcs = nn.ModuleList([nn.Linear(in_channels * area, fc_out_channels), nn.Linear(fc_out_channels, fc_out_channels)])
        self.fc_cls = nn.Linear(fc_out_channels, self.num_classes + 1)
        self.fc_reg = nn.Linear(fc_out_channels, 4 if self.reg_class_agnostic else 4 * self.num_classes)
        self.init_weights()

    def init_weights(self):
        for fc in self.shared_fcs:
            nn.init.xavier_uniform_(fc.weight)
            nn.init.zeros_(fc.bias)
        nn.init.normal_(self.fc_cls.weight, 0, 0.01)
        nn.init.zeros_(self.fc_cls.bias)
        nn.init.normal_(self.fc_reg.weight, 0, 0.001)
        nn.init.zeros_(self.fc_reg.bias)

    def forward(self, x):
        """RoI features (R, in_channels, h, w) -> (cls_score (R, C + 1), bbox_pred (R, 4C) or (R, 4))."""
        x = x.flatten(1)
        for fc in self.shared_fcs:
            x = F.relu(fc(x))
        return self.fc_cls(x), self.fc_reg(x)

    def get_bboxes(self, rois, cls_score, bbox_pred, img_shape, scale_factor, rescale=False, cfg=None, padded=False, roi_counts=None):
        """mmdet's ``get_bboxes`` (the module's text).  rois (R, 5), cls_score (R, C + 1), bbox_pred (R, 4C) or (R, 4); ``img_shape``
        (h, w[, c]) and ``scale_factor`` (a scalar or four entries) of the image.  ``cfg=None`` -> (bboxes (R, 4C), scores (R, C + 1));
        with a ``cfg`` (``score_thr``, ``nms``, ``max_per_img``; a dict or an attribute object) -> (det_bboxes (k, 5), det_labels (k,)
        int64).  Several images: ``img_shape`` / ``scale_factor`` as lists with one entry per image and ``roi_counts``, the RoIs of each
        image in ``bbox2roi`` order, or rois (N, K, 5) (cls_score and bbox_pred with or without the leading N); the results are then
        per-image lists.  ``padded=True`` (``max_per_img`` > 0) -> (dets (N, max_per_img, 5), labels (N, max_per_img) int64, counts (N,)
        int32) with NaN rows and −1 labels past the count, without a host synchronisation."""
        C = self.num_classes
        many = _is_per_image(img_shape) or rois.dim() == 3 or roi_counts is not None
        if rois.dim() == 3:
            assert roi_counts is None, 'get_bboxes: rois (N, K, 5) say the counts themselves'
            roi_counts = [rois.shape[1]] * rois.shape[0]
            rois, cls_score, bbox_pred = rois.reshape(-1, 5), cls_score.reshape(-1, cls_score.shape[-1]), bbox_pred.reshape(-1, bbox_pred.shape[-1])
        counts = [int(k) for k in roi_counts] if roi_counts is not None else [rois.shape[0]]
        N, dev = len(counts), rois.device
        if img_shape is None:
            raise ValueError('get_bboxes: img_shape=None (no clamp) is not provided')
        shapes = list(img_shape) if _is_per_image(img_shape) else [img_shape] * N
        assert len(shapes) == N and sum(counts) == rois.shape[0], 'get_bboxes: one img_shape and one count per image'
        rois, cls_score, bbox_pred = rois.detach(), cls_score.detach(), bbox_pred.detach()           # detections carry no gradient
        img_hw = P.host_to_device([[float(s[0]), float(s[1])] for s in shapes], torch.float32, dev)
        scale = _scale_rows(scale_factor, N, dev) if rescale else None
        if cfg is None:
            assert not padded, 'get_bboxes: padded=True needs a cfg'
            boxes = decode_torch(rois, bbox_pred, _per_row(img_hw, counts), None if scale is None else _per_row(scale, counts),
                                 self.target_means, self.target_stds)
            boxes, scores = boxes.reshape(rois.shape[0], -1), softmax_torch(cls_score)
            if not many:
                return boxes, scores
            return list(torch.split(boxes, counts)), list(torch.split(scores, counts))
        score_thr, max_num = float(_cfg_get(cfg, 'score_thr')), int(_cfg_get(cfg, 'max_per_img'))
        iou_thr = P.parse_nms_cfg(_cfg_get(cfg, 'nms'))[0]
        args = (rois, cls_score, bbox_pred, counts, img_hw, scale, C, self.reg_class_agnostic, self.target_means, self.target_stds, score_thr)
        if padded:
            if max_num <= 0:
                raise ValueError('get_bboxes: padded=True requires max_per_img > 0')
            return detect(*args, iou_thr, max_num)
        if max_num > 0:
            dets, labels, num = detect(*args, iou_thr, max_num)
            out = [(dets[n, :k], labels[n, :k]) for n, k in enumerate(num.tolist())]
        else:                                                                   # every kept candidate: no padded form
            boxes, score, order, valid = bbox_head_rank_torch(*args)
            keep = P.nms_grouped(boxes, valid, [k for k in counts for _ in range(C)], iou_thr)[0]
            out = select_torch(boxes, score, order, keep, counts, C, max_num)
        if not many:
            return out[0]
        return [d for d, _ in out], [l for _, l in out]

    # -------------------------------------------------------------------------------------------- training
    def get_targets(self, sampling_results, gt_bboxes, gt_labels, rcnn_train_cfg, concat=True):
        """mmdet's ``get_targets``: per image the positives, then the negatives -> (labels int64: ``num_classes`` on the negatives,
        label_weights: ``pos_weight`` (1 when <= 0) on the positives and 1 on the negatives, bbox_targets: the coder's deltas of the
        positives against their ground truths, bbox_weights: 1 on the positives), concatenated over the images unless ``concat=False``.
        A :class:`monorun_amd.assigners.BatchSamplingResult` gives the padded form instead, without a host synchronisation: per image
        ``num`` rows, the sampled boxes in ascending index order, then rows of weight 0 — (rois (N·num, 5), labels, label_weights,
        bbox_targets, bbox_weights), whose first entry replaces ``bbox2roi``."""
        pos_weight = float(_cfg_get(rcnn_train_cfg, 'pos_weight')) if _has(rcnn_train_cfg, 'pos_weight') else -1.0
        pos_weight = 1.0 if pos_weight <= 0 else pos_weight
        if isinstance(sampling_results, BatchSamplingResult):
            return self._padded_targets(sampling_results, pos_weight)
        out = []
        for res in sampling_results:
            pos, neg = res.pos_bboxes[:, :4], res.neg_bboxes
            num_pos, num = pos.shape[0], pos.shape[0] + neg.shape[0]
            labels = pos.new_full((num,), self.num_classes, dtype=torch.int64)
            label_weights, bbox_targets, bbox_weights = pos.new_zeros(num), pos.new_zeros(num, 4), pos.new_zeros(num, 4)
            if num_pos > 0:
                labels[:num_pos] = res.pos_gt_labels
                label_weights[:num_pos] = pos_weight
                bbox_targets[:num_pos] = bbox2delta(pos, res.pos_gt_bboxes, self.target_means, self.target_stds)
                bbox_weights[:num_pos] = 1
            label_weights[num_pos:] = 1.0
            out.append((labels, label_weights, bbox_targets, bbox_weights))
        if not concat:
            return tuple(list(t) for t in zip(*out))
        return tuple(torch.cat(t, 0) for t in zip(*out))

    def _padded_targets(self, s, pos_weight):
        N, T = s.gt_inds.shape
        num = s.pos_inds.shape[1]
        rows = _ascending(s.pos_mask | s.neg_mask, num)                                             # (N, num), -1 past the count
        live, at = rows >= 0, rows.clamp(min=0)
        pos = s.pos_mask.gather(1, at) & live
        boxes = s.bboxes.gather(1, at[..., None].expand(N, num, 4))
        own = (s.gt_inds.gather(1, at) - 1).clamp(min=0)                                            # (N, num): each row's ground truth
        Gm = max(max(s.num_gts, default=0), 1)
        gts = torch.stack([torch.cat((g, g.new_zeros(Gm - g.shape[0], 4))) for g in s.gt_bboxes]).to(boxes.dtype)
        mine = gts.gather(1, own.clamp(max=Gm - 1)[..., None].expand(N, num, 4))
        unit = torch.stack([torch.full((), float(k >= 2), dtype=boxes.dtype, device=boxes.device) for k in range(4)])
        safe = lambda b: torch.where(pos[..., None], b, unit)                                      # [0, 0, 1, 1] where no delta is wanted
        w = pos.to(boxes.dtype)
        deltas = bbox2delta(safe(boxes), safe(mine), self.target_means, self.target_stds) * w[..., None]
        labels = torch.where(pos, s.labels.gather(1, at), self.num_classes)
        image = torch.arange(N, device=boxes.device, dtype=boxes.dtype)[:, None, None].expand(N, num, 1)
        rois = torch.cat((image, torch.where(live[..., None], boxes, unit)), dim=-1)
        return (rois.reshape(-1, 5), labels.reshape(-1), (w * pos_weight + (live & ~pos).to(boxes.dtype)).reshape(-1), deltas.reshape(-1, 4),
                w[..., None].expand(N, num, 4).reshape(-1, 4))

    def loss(self, cls_score, bbox_pred, rois, labels, label_weights, bbox_targets, bbox_weights, reduction_override=None):
        """mmdet's ``loss``: -> dict(loss_cls, acc, loss_bbox).  ``loss_cls`` with ``avg_factor = max(sum(label_weights > 0), 1)`` as a
        tensor and ``acc`` over the rows of positive weight; the regression picks each positive's own class columns, is weighted by
        ``bbox_weights`` and has as ``avg_factor`` the number of rows (of positive weight: the padded form's other rows are no samples).
        With no positives it is 0 = ``bbox_pred[pos].sum()``.  No host synchronisation."""
        losses = dict()
        live = label_weights > 0
        rows = live.sum().clamp(min=1).to(torch.float32)
        if cls_score is not None:
            losses['loss_cls'] = resolve(self.loss_cls)(cls_score, labels, label_weights, avg_factor=rows, reduction_override=reduction_override)
            losses['acc'] = accuracy(cls_score, labels, weight=live)
        if bbox_pred is not None:
            R = bbox_pred.shape[0]
            pos = (labels >= 0) & (labels < self.num_classes)
            if self.reg_class_agnostic:
                own = bbox_pred.reshape(R, 4)
            else:
                cls = torch.where(pos, labels, 0)
                own = bbox_pred.reshape(R, -1, 4).gather(1, cls[:, None, None].expand(R, 1, 4)).reshape(R, 4)
            weight = bbox_weights * pos[:, None].to(bbox_weights.dtype)
            losses['loss_bbox'] = resolve(self.loss_bbox)(own, bbox_targets, weight, avg_factor=rows, reduction_override=reduction_override)
        return losses

    def regress_by_class(self, rois, label, bbox_pred, img_meta):
        """mmdet's ``regress_by_class``: rois (n, 4) or (n, 5), label (n,), bbox_pred (n, 4C) or (n, 4) -> the rois moved by their class's
        deltas and clamped to ``img_meta['img_shape']``."""
        assert rois.shape[1] in (4, 5), 'regress_by_class: rois (n, 4) or (n, 5)'
        if not self.reg_class_agnostic:
            groups = bbox_pred.shape[1] // 4                                                        # stated: no rows leave -1 ambiguous
            bbox_pred = bbox_pred.reshape(bbox_pred.shape[0], groups, 4).gather(1, label[:, None, None].expand(-1, 1, 4).long()).reshape(-1, 4)
        rois5 = rois if rois.shape[1] == 5 else torch.cat((rois.new_zeros(rois.shape[0], 1), rois), dim=1)
        hw = rois.new_tensor([float(img_meta['img_shape'][0]), float(img_meta['img_shape'][1])]).expand(rois.shape[0], 2)
        boxes = decode_torch(rois5, bbox_pred, hw, None, self.target_means, self.target_stds)[:, 0].to(rois.dtype)
        return boxes if rois.shape[1] == 4 else torch.cat((rois[:, :1], boxes), dim=1)

    def refine_bboxes(self, rois, labels, bbox_preds, pos_is_gts, img_metas):
        """mmdet's ``refine_bboxes``: per image the rois regressed by their labels' deltas, without the positives that are ground truths."""
        img_ids = rois[:, 0].long().unique(sorted=True)
        assert img_ids.numel() <= len(img_metas)
        out = []
        for i in range(len(img_metas)):
            inds = torch.nonzero(rois[:, 0] == i, as_tuple=False).squeeze(dim=1)
            bboxes = self.regress_by_class(rois[inds, 1:], labels[inds], bbox_preds[inds], img_metas[i])
            keep = pos_is_gts[i].new_ones(inds.numel())
            keep[:len(pos_is_gts[i])] = 1 - pos_is_gts[i]
            out.append(bboxes[keep.bool()])
        return out


def _has(cfg, key):
    return key in cfg if isinstance(cfg, dict) else hasattr(cfg, key)


def accuracy(pred, target, topk=1, thresh=None, weight=None):
    """mmdet's ``accuracy``: the percentage of rows whose ``topk`` highest scores hold the target (above ``thresh``, if given), a tensor
    (1,) — a tuple of them for a tuple of ``topk``.  ``weight`` (R,) bool: the rows that count (default: all)."""
    ks = (topk,) if isinstance(topk, int) else tuple(topk)
    rows = pred.shape[0] if weight is None else weight.sum().clamp(min=1)
    if pred.shape[0] == 0:
        res = [pred.new_zeros(1) for _ in ks]
        return res[0] if isinstance(topk, int) else tuple(res)
    value, label = pred.topk(max(ks), dim=1)
    correct = label.t() == target[None, :]
    if thresh is not None:
        correct = correct & (value > thresh).t()
    if weight is not None:
        correct = correct & weight[None, :]
    res = [correct[:k].reshape(-1).float().sum(0, keepdim=True) * (100.0 / rows) for k in ks]
    return res[0] if isinstance(topk, int) else tuple(res)
