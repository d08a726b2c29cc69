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

Training targets and the RPN's ``loss`` (anchor assignment, sampling, the two losses) are not provided: they are torch ops.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import proposals as P


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
                 test_cfg=None, train_cfg=None, **kwargs):
        super().__init__()
        coder = dict(bbox_coder)
        assert coder.pop('type', 'DeltaXYWHBBoxCoder') == 'DeltaXYWHBBoxCoder', 'bbox_coder: DeltaXYWHBBoxCoder only'
        self.in_channels, self.feat_channels, self.starting_level = in_channels, feat_channels, starting_level
        self.anchor_generator = anchor_generator if isinstance(anchor_generator, AnchorGenerator) else AnchorGenerator(**anchor_generator)
        self.target_means = tuple(float(m) for m in coder.get('target_means', (0.0,) * 4))
        self.target_stds = tuple(float(s) for s in coder.get('target_stds', (1.0,) * 4))
        self.test_cfg, self.train_cfg = test_cfg, train_cfg
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
