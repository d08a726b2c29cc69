"""``MonoRUnDetector``, inference side: the reference's two-stage detector (monorun/models/detectors/monorun.py over mmdet's
``TwoStageDetector``) as a thin class over this package's modules — image in, ``[dict(bbox_results=…, bbox_3d_results=…)]`` out
(INTEGRATION.md §2).  Sub-modules are given built or as the reference's config dicts (``roi_head.build``); the attribute
names make the checkpoint prefixes ``backbone.`` / ``neck.`` / ``rpn_head.`` / ``roi_head.``.  ``show_result`` is not provided: it
needs mmcv's and OpenCV's drawing.  Training side: ``forward_train``, ``_parse_losses`` and ``train_step`` with the
semantics of mmdet's ``TwoStageDetector`` and ``BaseDetector``."""
from collections import OrderedDict

import torch
import torch.distributed as dist
import torch.nn as nn

from .roi_head import MonoRUnRoIHead, build, cfg_get


class MonoRUnDetector(nn.Module):

    def __init__(self, backbone, neck=None, rpn_head=None, roi_head=None, train_cfg=None, test_cfg=None, pretrained=None):
        super().__init__()
        self.backbone = build(backbone)
        if neck is not None:
            self.neck = build(neck)
        if rpn_head is not None:
            extra = dict(train_cfg=cfg_get(train_cfg, 'rpn'), test_cfg=cfg_get(test_cfg, 'rpn')) if isinstance(rpn_head, dict) else {}
            self.rpn_head = build(rpn_head, **extra)
        if roi_head is not None:
            if isinstance(roi_head, dict):
                cfg = dict(roi_head)
                typ = cfg.pop('type', 'MonoRUnRoIHead')
                if typ != 'MonoRUnRoIHead':
                    raise KeyError(f'{typ}: the detector\'s roi_head is a MonoRUnRoIHead')
                roi_head = MonoRUnRoIHead(**cfg, train_cfg=cfg_get(train_cfg, 'rcnn'), test_cfg=cfg_get(test_cfg, 'rcnn'))
            self.roi_head = roi_head
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.init_weights(pretrained=pretrained)

    with_neck = property(lambda self: getattr(self, 'neck', None) is not None)
    with_rpn = property(lambda self: getattr(self, 'rpn_head', None) is not None)
    with_roi_head = property(lambda self: getattr(self, 'roi_head', None) is not None)
    with_bbox = property(lambda self: self.with_roi_head and self.roi_head.with_bbox)

    def init_weights(self, pretrained=None):
        """mmdet's: the backbone from ``pretrained`` (a LOCAL checkpoint file; a URL raises, nothing is fetched) or its own rule, then
        every other part's own rule."""
        if isinstance(pretrained, str) and '://' in pretrained:
            raise ValueError(f'init_weights: {pretrained!r} would have to be fetched; download the checkpoint and pass its local path')
        self.backbone.init_weights(pretrained=pretrained)
        if self.with_neck:
            self.neck.init_weights()
        if self.with_rpn:
            self.rpn_head.init_weights()
        if self.with_roi_head:
            self.roi_head.init_weights(pretrained)

    def extract_feat(self, img):
        x = self.backbone(img)
        if self.with_neck:
            x = self.neck(x)
        return x

    def simple_test(self, img, img_metas, proposals=None, rescale=False, **kwargs):
        """Test without augmentation (monorun.py:10-23)."""
        assert self.with_bbox, 'Bbox head must be implemented.'
        x = self.extract_feat(img)
        if proposals is None:
            proposal_list = self.rpn_head.simple_test_rpn(x, img_metas)
        else:
            proposal_list = proposals
        return self.roi_head.simple_test(x, proposal_list, img_metas, rescale=rescale, **kwargs)

    def forward_test(self, imgs, img_metas, **kwargs):
        """mmdet's ``BaseDetector.forward_test`` for one augmentation: ``imgs`` and ``img_metas`` are lists with one entry, which is
        unwrapped, as is ``proposals``; the other keywords (``coord_2d``, ``cam_intrinsic``) reach ``simple_test`` as the per-augmentation
        lists they are, and the RoI head takes their first entry."""
        if not isinstance(imgs, (list, tuple)) or not isinstance(img_metas, (list, tuple)):
            raise TypeError('forward_test: imgs and img_metas must be lists (one entry per augmentation)')
        if len(imgs) != 1 or len(img_metas) != 1:
            raise NotImplementedError('aug_test is not provided: one augmentation only')
        if kwargs.get('proposals') is not None:
            kwargs['proposals'] = kwargs['proposals'][0]
        return self.simple_test(imgs[0], img_metas[0], **kwargs)

    def forward_train(self, img, img_metas, gt_bboxes, gt_labels, gt_bboxes_ignore=None, gt_masks=None, proposals=None, rpn_kwargs=None,
                      **kwargs):
        """mmdet's ``TwoStageDetector.forward_train``: ``extract_feat``, the RPN's ``forward_train`` with
        ``proposal_cfg = train_cfg.rpn_proposal`` (``test_cfg.rpn`` without one), whose losses are merged, then the RoI head's
        ``forward_train`` on its proposals (on ``proposals`` without an RPN).  ``kwargs``: what the RoI head takes besides (``gt_bboxes_3d``,
        ``gt_coords_3d``, ``gt_coords_3d_mask``, ``coord_2d``, ``cam_intrinsic``, ``path``, ``generator``, ``keys``); ``rpn_kwargs``: the
        RPN sampler's ``generator`` / ``keys``.  -> the dict of all losses."""
        x = self.extract_feat(img)
        losses = dict()
        if self.with_rpn:
            proposal_cfg = cfg_get(self.train_cfg, 'rpn_proposal', cfg_get(self.test_cfg, 'rpn'))
            rpn_losses, proposal_list = self.rpn_head.forward_train(x, img_metas, gt_bboxes, gt_labels=None, gt_bboxes_ignore=gt_bboxes_ignore,
                                                                    proposal_cfg=proposal_cfg, **(rpn_kwargs or {}))
            losses.update(rpn_losses)
        else:
            proposal_list = proposals
        roi_losses = self.roi_head.forward_train(x, img_metas, proposal_list, gt_bboxes, gt_labels, gt_bboxes_ignore, gt_masks, **kwargs)
        losses.update(roi_losses)
        return losses

    @staticmethod
    def _parse_losses(losses):
        """mmdet's ``BaseDetector._parse_losses``: every entry reduced to a scalar (a tensor by its mean, a list of tensors by the sum of
        their means), ``loss`` the sum of the entries whose key contains ``'loss'``, ``log_vars`` every entry (and ``loss``) as a Python
        float — averaged over the ranks first where ``torch.distributed`` is initialised.  -> (loss, log_vars)."""
        log_vars = OrderedDict()
        for name, value in losses.items():
            if isinstance(value, torch.Tensor):
                log_vars[name] = value.mean()
            elif isinstance(value, (list, tuple)):
                log_vars[name] = sum(v.mean() for v in value)
            else:
                raise TypeError(f'{name} is not a tensor or list of tensors')
        loss = sum(value for key, value in log_vars.items() if 'loss' in key)
        log_vars['loss'] = loss
        for name, value in log_vars.items():
            if dist.is_available() and dist.is_initialized():
                value = value.data.clone()
                dist.all_reduce(value.div_(dist.get_world_size()))
            log_vars[name] = value.item()
        return loss, log_vars

    def train_step(self, data, optimizer=None):
        """mmdet's ``BaseDetector.train_step``: ``data`` the keywords of :meth:`forward` (``img``, ``img_metas`` and the ground truth) ->
        ``dict(loss, log_vars, num_samples)``; the caller runs ``backward()`` and the optimizer, which is not used here."""
        losses = self(**data)
        loss, log_vars = self._parse_losses(losses)
        return dict(loss=loss, log_vars=log_vars, num_samples=len(data['img_metas']))

    def forward(self, img, img_metas, return_loss=True, **kwargs):
        if return_loss:
            if self.train_cfg is None:                  # an inference detector stays what it was: it does not train
                raise NotImplementedError('MonoRUnDetector.forward(return_loss=True): the detector was built without a train_cfg')
            return self.forward_train(img, img_metas, **kwargs)
        with torch.no_grad():
            return self.forward_test(img, img_metas, **kwargs)


def register_with_mmdet(force=False):
    """Put :class:`MonoRUnDetector` into mmdet's ``DETECTORS`` registry; False without mmdet, or (unless ``force``) when the name is taken."""
    try:
        from mmdet.models.builder import DETECTORS
    except Exception:
        return False
    if DETECTORS.get('MonoRUnDetector') is not None and not force:
        return False
    DETECTORS.register_module(name='MonoRUnDetector', force=True, module=MonoRUnDetector)
    return True
