"""The region proposal head: the reference's ``RPNHeadMod`` (monorun/models/dense_heads/rpn_head.py), which is mmdet's
``RPNHead`` on ``feats[starting_level:]``, with mmdet's ``AnchorGenerator`` and ``get_bboxes`` — without mmdet or mmcv.  It produces the
RoIs every later stage (:mod:`monorun_amd.roi_extractor` onwards) consumes.

``get_bboxes`` per image: per level the ``min(nms_pre, H·W·A)`` highest LOGITS (``nms_pre <= 0``: all; ties to the lower anchor index
``(y·W + x)·A + a``; mmdet ranks the sigmoid, which is the same order wherever the sigmoid does not collapse two logits), the decode
(:func:`monorun_amd.proposals.proposal_decode`), NMS with one group per (image, level) (:func:`monorun_amd.proposals.nms_grouped`), the
survivors of all levels by logit descending (ties to their position in the level-concatenated list), the first ``nms_post``.  The
convolutions and the sorts are torch; decode and NMS are three HIP launches for all images and levels.  ``padded=True`` returns
``(N, nms_post, 5)`` with NaN rows past ``counts`` (N,) int32 and performs no host synchronisation; the list form is the padded form plus
one read of ``counts``.

Training: ``get_anchors``, ``get_targets``, ``loss`` and ``forward_train`` are mmdet's ``AnchorHead`` ones on
:mod:`monorun_amd.assigners` — ONE ``assign_batch`` (two HIP launches for all images and levels, the shared anchors are not copied) and one
``sample_batch`` per step; the regression targets are the launch's deltas times the sampled-positive mask.  ``loss`` and ``forward_train``
(with ``padded=True`` in ``proposal_cfg``) perform no host synchronisation.
"""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import proposals as P
from .assigners import build_assigner, build_sampler
from .detection_losses import resolve
from .losses import build_loss


class AnchorGenerator:
    """mmdet's ``AnchorGenerator`` (``scale_major=True``, centre 0): per level ``len(ratios)·len(scales)`` base anchors, ratio-major, in
    fp32 torch ops on the host: ``h_r = sqrt(ratio)``, ``w_r = 1 / h_r``, ``w = stride·w_r·scale``, ``h = stride·h_r·scale``,
    ``[−w/2, −h/2, w/2, h/2]``."""

    def __init__(self, scales, ratios, strides, type='AnchorGenerator'):
        assert type == 'AnchorGenerator', f'anchor generator type {type!r} is not provided'
        self.scales, self.ratios, self.strides = [float(s) for s in scales], [float(r) for r in ratios], [int(s) for s in strides]
        scales_t, ratios_t = torch.tensor(self.scales, dtype=torch.float32), torch.tensor(self.ratios, dtype=torch.float32)
        h_r = torch.sqrt(ratios_t)
        w_r = 1 / h_r
        self.base_anchors = []
        for s in self.strides:
            w = (float(s) * w_r[:, None] * scales_t[None, :]).reshape(-1)
            h = (float(s) * h_r[:, None] * scales_t[None, :]).reshape(-1)
            self.base_anchors.append(torch.stack((-0.5 * w, -0.5 * h, 0.5 * w, 0.5 * h), dim=-1))

    @property
    def num_levels(self):
        return len(self.strides)

    @property
    def num_base_anchors(self):
        return [b.shape[0] for b in self.base_anchors]

    def valid_flags(self, featmap_sizes, pad_shape):
        """mmdet's ``valid_flags`` of one image as a host array (sum H·W·A,) bool: the cells inside ``pad_shape`` (h, w[, c]), each
        repeated for its A anchors."""
        out = []
        for (h, w), s, base in zip(featmap_sizes, self.strides, self.base_anchors):
            valid_h, valid_w = min(int(math.ceil(pad_shape[0] / s)), h), min(int(math.ceil(pad_shape[1] / s)), w)
            cell = (np.arange(h) < valid_h)[:, None] & (np.arange(w) < valid_w)[None, :]
            out.append(np.repeat(cell.reshape(-1), base.shape[0]))
        return np.concatenate(out)

    def grid_anchors(self, featmap_sizes, device='cpu'):
        """mmdet's ``grid_anchors``: per level (H·W·A, 4), anchor ``(y·W + x)·A + a`` = base[a] + (x·s, y·s, x·s, y·s)."""
        out = []
        for (h, w), s, base in zip(featmap_sizes, self.strides, self.base_anchors):
            x = torch.arange(w, dtype=torch.float32) * s
            y = torch.arange(h, dtype=torch.float32) * s
            xx, yy = x.repeat(h), y[:, None].expand(h, w).reshape(-1)
            shifts = torch.stack((xx, yy, xx, yy), dim=-1)
            out.append((shifts[:, None, :] + base[None, :, :]).reshape(-1, 4).to(device))
        return out


def _cfg(cfg, key, *default):
    """An entry of a train / test config given as a dict or as an attribute object."""
    if isinstance(cfg, dict):
        return cfg.get(key, *default) if default else cfg[key]
    return getattr(cfg, key, *default)


def _image_shapes(img_metas, device):
    """(N, 2) fp32 [img_h, img_w] on ``device`` from mmdet's img_metas (dicts with ``img_shape``) or a tensor (N, 2); no blocking copy."""
    if isinstance(img_metas, torch.Tensor):
        return img_metas.to(device=device, dtype=torch.float32).reshape(-1, 2)
    return P.host_to_device([[float(m['img_shape'][0]), float(m['img_shape'][1])] for m in img_metas], torch.float32, device)


class RPNHeadMod(nn.Module):
    """The reference's ``RPNHeadMod``: mmdet's ``RPNHead`` (``rpn_conv`` 3 × 3 + ReLU, ``rpn_cls`` 1 × 1 with A sigmoid channels, ``rpn_reg``
    1 × 1 with 4A channels; mmdet's parameter names, so a checkpoint's ``rpn_head.*`` loads with ``strict=True``) whose ``forward`` takes
    ``feats[starting_level:]``."""

    def __init__(self, in_channels, starting_level=0, feat_channels=256,
                 anchor_generator=dict(type='AnchorGenerator', scales=[8], ratios=[0.5, 1.0, 2.0], strides=[4, 8, 16, 32, 64]),
                 bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=(.0, .0, .0, .0), target_stds=(1.0, 1.0, 1.0, 1.0)),
                 loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
                 loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0), test_cfg=None, train_cfg=None, **kwargs):
        super().__init__()
        coder = dict(bbox_coder)
        assert coder.pop('type', 'DeltaXYWHBBoxCoder') == 'DeltaXYWHBBoxCoder', 'bbox_coder: DeltaXYWHBBoxCoder only'
        self.in_channels, self.feat_channels, self.starting_level = in_channels, feat_channels, starting_level
        self.anchor_generator = anchor_generator if isinstance(anchor_generator, AnchorGenerator) else AnchorGenerator(**anchor_generator)
        self.target_means = tuple(float(m) for m in coder.get('target_means', (0.0,) * 4))
        self.target_stds = tuple(float(s) for s in coder.get('target_stds', (1.0,) * 4))
        self.test_cfg, self.train_cfg = test_cfg, train_cfg
        self.loss_cls, self.loss_bbox = build_loss(loss_cls), build_loss(loss_bbox)      # an UnbuiltLoss without mmdet: `loss` resolves it
        self.assigner = self.sampler = None
        if train_cfg is not None and _cfg(train_cfg, 'assigner', None) is not None:
            self.assigner = build_assigner(_cfg(train_cfg, 'assigner'))
            self.sampler = build_sampler(_cfg(train_cfg, 'sampler', dict(type='RandomSampler', num=256, pos_fraction=0.5,
                                                                           add_gt_as_proposals=False)), context=self)
        self._anchor_cache = {}
        self.num_anchors = self.anchor_generator.num_base_anchors[0]
        self.rpn_conv = nn.Conv2d(in_channels, feat_channels, 3, padding=1)
        self.rpn_cls = nn.Conv2d(feat_channels, self.num_anchors, 1)
        self.rpn_reg = nn.Conv2d(feat_channels, self.num_anchors * 4, 1)
        self.init_weights()

    def init_weights(self):
        for m in (self.rpn_conv, self.rpn_cls, self.rpn_reg):
            nn.init.normal_(m.weight, std=0.01)
            nn.init.zeros_(m.bias)

    def forward_single(self, x):
        x = F.relu(self.rpn_conv(x), inplace=True)
        return self.rpn_cls(x), self.rpn_reg(x)

    def forward(self, feats):
        """-> (cls_scores, bbox_preds): per map of ``feats[starting_level:]`` (N, A, H, W) logits and (N, 4A, H, W) deltas."""
        outs = [self.forward_single(f) for f in list(feats)[self.starting_level:]]
        return [o[0] for o in outs], [o[1] for o in outs]

    def get_bboxes(self, cls_scores, bbox_preds, img_metas, cfg=None, rescale=False, padded=False):
        """The proposals of every image from the head's outputs (the module's text).  cfg: ``nms_pre``, ``nms_post``, ``nms_thr`` (or
        ``nms=dict(type='nms', iou_threshold=...)``), ``min_bbox_size``; ``max_num`` / ``max_per_img``, if present, must equal
        ``nms_post``.  -> a list of (k_n, 5) ``[x1, y1, x2, y2, score]``, or with ``padded=True`` ((N, nms_post, 5) with NaN rows past the
        count, counts (N,) int32) without a host synchronisation.  ``rescale`` is accepted and, as in mmdet's RPN, has no effect."""
        cfg = dict(self.test_cfg if cfg is None else cfg)
        if cfg.get('nms_across_levels', False):
            raise NotImplementedError('RPNHeadMod: nms_across_levels=True is not provided (no reference config uses it)')
        nms_pre, nms_post = int(cfg.get('nms_pre', 0)), int(cfg['nms_post'])
        for key in ('max_num', 'max_per_img'):
            if key in cfg and int(cfg[key]) != nms_post:
                raise ValueError(f'RPNHeadMod: {key}={cfg[key]} differs from nms_post={nms_post}')
        thr = float(cfg['nms_thr']) if 'nms_thr' in cfg else P.parse_nms_cfg(cfg['nms'])[0]
        cls_scores, bbox_preds = [c.detach() for c in cls_scores], [r.detach() for r in bbox_preds]       # proposals carry no gradient
        gen = self.anchor_generator
        assert len(cls_scores) == len(bbox_preds) == gen.num_levels, 'RPNHeadMod: one head output per anchor level'
        N, dev = cls_scores[0].shape[0], cls_scores[0].device
        index, counts = [], []
        for c in cls_scores:
            logits = c.permute(0, 2, 3, 1).reshape(N, -1)
            k = min(nms_pre, logits.shape[1]) if nms_pre > 0 else logits.shape[1]
            index.append(torch.sort(logits, dim=1, descending=True, stable=True)[1][:, :k])
            counts.append(k)
        index = torch.cat(index, dim=1).contiguous()
        boxes, score, logit, valid = P.proposal_decode(cls_scores, bbox_preds, index, counts, _image_shapes(img_metas, dev), gen.base_anchors,
                                                       gen.strides, self.target_means, self.target_stds,
                                                       min_bbox_size=float(cfg.get('min_bbox_size', 0)))
        keep = P.nms_grouped(boxes.reshape(-1, 4), valid.reshape(-1), tuple(counts) * N, thr)[0].reshape(N, -1)
        out, num = merge_levels(boxes, score, logit, keep, nms_post)
        if padded:
            return out, num
        return [out[n, :k] for n, k in enumerate(num.tolist())]

    # -------------------------------------------------------------------------------------------- training
    def get_anchors(self, featmap_sizes, img_metas, device='cuda'):
        """mmdet's ``get_anchors``, dense: (anchors of every level, one set for all images: a list of (H·W·A, 4); valid (N, sum H·W·A)
        bool from each image's ``pad_shape``).  The anchors are cached per sizes and device; no blocking copy."""
        sizes = tuple((int(h), int(w)) for h, w in featmap_sizes)
        key = (sizes, str(device))
        if key not in self._anchor_cache:
            self._anchor_cache[key] = self.anchor_generator.grid_anchors(sizes, device)
        flags = np.stack([self.anchor_generator.valid_flags(sizes, m['pad_shape']) for m in img_metas])
        return self._anchor_cache[key], P.host_to_device(flags.tolist(), torch.bool, device)

    def get_targets(self, anchor_list, valid_flags, gt_bboxes, img_metas, gt_bboxes_ignore=None, generator=None, keys=None):
        """mmdet's ``AnchorHead.get_targets`` for all images at once: ``allowed_border``, one ``assign_batch``, one ``sample_batch``.
        anchor_list, valid_flags: :meth:`get_anchors`' results.  -> (labels (N, B) int64: 0 on the sampled positives, 1 elsewhere;
        label_weights (N, B): ``pos_weight`` (1 when <= 0) on the sampled positives, 1 on the sampled negatives; bbox_targets (N, B, 4):
        the launch's deltas on the sampled positives; bbox_weights (N, B, 4): 1 there; num_total_pos, num_total_neg: device scalars,
        the sum over the images of max(count, 1)).  B runs over the levels in order.  No host synchronisation."""
        if self.assigner is None:
            raise RuntimeError('RPNHeadMod.get_targets: the head was built without a train_cfg')
        if self.sampler.add_gt_as_proposals:
            raise NotImplementedError('RPNHeadMod: a sampler with add_gt_as_proposals=True is not provided (anchors have no row for them)')
        anchors = torch.cat(list(anchor_list)) if not isinstance(anchor_list, torch.Tensor) else anchor_list
        border = _cfg(self.train_cfg, 'allowed_border', -1)
        present = valid_flags
        if border >= 0:
            shape = _image_shapes(img_metas, anchors.device)                     # (N, 2) img_h, img_w
            inside = ((anchors[None, :, 0] >= -border) & (anchors[None, :, 1] >= -border)
                      & (anchors[None, :, 2] < shape[:, 1:2] + border) & (anchors[None, :, 3] < shape[:, 0:1] + border))
            present = present & inside
        result = self.assigner.assign_batch(anchors, gt_bboxes, gt_bboxes_ignore, None, valid=present, means=self.target_means,
                                            stds=self.target_stds)
        sampled = self.sampler.sample_batch(result, anchors, gt_bboxes, generator=generator, keys=keys)
        pos, neg = sampled.pos_mask, sampled.neg_mask
        pos_weight = float(_cfg(self.train_cfg, 'pos_weight', -1))
        labels = torch.where(pos, 0, 1)
        label_weights = pos.to(torch.float32) * (1.0 if pos_weight <= 0 else pos_weight) + neg.to(torch.float32)
        bbox_weights = pos[..., None].to(torch.float32).expand(-1, -1, 4)
        return (labels, label_weights, result.deltas * bbox_weights, bbox_weights, sampled.num_pos.clamp(min=1).sum(),
                sampled.num_neg.clamp(min=1).sum())

    def loss(self, cls_scores, bbox_preds, gt_bboxes, img_metas, gt_bboxes_ignore=None, generator=None, keys=None):
        """mmdet's ``RPNHead.loss``: -> dict(loss_rpn_cls=[per level], loss_rpn_bbox=[per level]).  Per level the NHWC-flattened outputs,
        the sigmoid cross entropy against ``label == 0`` and the regression loss on the deltas, both with
        ``avg_factor = num_total_pos + num_total_neg``.  No host synchronisation."""
        sizes = [tuple(c.shape[-2:]) for c in cls_scores]
        N, dev = cls_scores[0].shape[0], cls_scores[0].device
        anchors, flags = self.get_anchors(sizes, img_metas, dev)
        labels, label_weights, bbox_targets, bbox_weights, num_pos, num_neg = self.get_targets(
            anchors, flags, gt_bboxes, img_metas, gt_bboxes_ignore, generator=generator, keys=keys)
        avg = (num_pos + num_neg).to(torch.float32)
        loss_cls, loss_bbox = resolve(self.loss_cls), resolve(self.loss_bbox)
        out_cls, out_bbox, first = [], [], 0
        for c, r, a in zip(cls_scores, bbox_preds, anchors):
            sl = slice(first, first + a.shape[0])
            first += a.shape[0]
            score = c.permute(0, 2, 3, 1).reshape(-1, 1)
            out_cls.append(loss_cls(score, (labels[:, sl] == 0).reshape(-1, 1), label_weights[:, sl].reshape(-1, 1), avg_factor=avg))
            out_bbox.append(loss_bbox(r.permute(0, 2, 3, 1).reshape(-1, 4), bbox_targets[:, sl].reshape(-1, 4),
                                      bbox_weights[:, sl].reshape(-1, 4), avg_factor=avg))
        return dict(loss_rpn_cls=out_cls, loss_rpn_bbox=out_bbox)

    def forward_train(self, x, img_metas, gt_bboxes, gt_labels=None, gt_bboxes_ignore=None, proposal_cfg=None, **kwargs):
        """mmdet's ``forward_train``: the head on the maps ``x``, :meth:`loss`, and with a ``proposal_cfg`` the proposals of
        :meth:`get_bboxes` -> (losses, proposal_list); with ``padded=True`` in ``proposal_cfg`` the proposals are get_bboxes' padded pair
        and nothing synchronises.  ``gt_labels`` is accepted and, as in mmdet's RPN, unused."""
        outs = self(x)
        losses = self.loss(*outs, gt_bboxes, img_metas, gt_bboxes_ignore, **kwargs)
        if proposal_cfg is None:
            return losses
        cfg = dict(proposal_cfg)
        padded = bool(cfg.pop('padded', False))
        return losses, self.get_bboxes(*outs, img_metas, cfg=cfg, padded=padded)

    def simple_test_rpn(self, x, img_metas, padded=False):
        """mmdet's ``RPNTestMixin.simple_test_rpn``: the head on the maps ``x``, then :meth:`get_bboxes` with ``test_cfg``."""
        return self.get_bboxes(*self(x), img_metas, padded=padded)


def merge_levels(boxes, score, logit, keep, nms_post):
    """The kept candidates of each image by logit descending (ties to the position in the level-concatenated list), the first
    ``nms_post``: boxes (N, P, 4), score, logit (N, P), keep (N, P) uint8 -> ((N, nms_post, 5) with NaN rows past the count, counts (N,)
    int32).  No host synchronisation: a stable sort, a running count and one scatter, whose surplus rows go to a spare row."""
    N, P_ = logit.shape
    order = torch.sort(logit, dim=1, descending=True, stable=True)[1]
    kept = keep.gather(1, order).bool()
    pos = torch.cumsum(kept, dim=1) - 1
    dest = torch.where(kept & (pos < nms_post), pos, torch.full_like(pos, nms_post))
    src = torch.cat((boxes, score[..., None]), dim=-1).gather(1, order[..., None].expand(N, P_, 5))
    out = torch.full((N, nms_post + 1, 5), float('nan'), dtype=boxes.dtype, device=boxes.device)
    out.scatter_(1, dest[..., None].expand(N, P_, 5), src)
    return out[:, :nms_post].contiguous(), kept.sum(dim=1).clamp(max=nms_post).to(torch.int32)
