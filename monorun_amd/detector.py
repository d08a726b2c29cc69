"""``MonoRUnDetector``, inference side: the reference's two-stage detector (monorun/models/detectors/monorun.py over mmdet's
``TwoStageDetector``) as a thin class over this package's modules — image in, ``[dict(bbox_results=…, bbox_3d_results=…)]`` out
(INTEGRATION.md §2).  Sub-modules are given built or as the reference's config dicts (``roi_head.build``); the attribute
names make the checkpoint prefixes ``backbone.`` / ``neck.`` / ``rpn_head.`` / ``roi_head.``.  ``show_result`` is not provided: it
needs mmcv's and OpenCV's drawing."""
import torch
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

    def forward(self, img, img_metas, return_loss=True, **kwargs):
        if return_loss:
            raise NotImplementedError('MonoRUnDetector.forward_train follows MonoRUnRoIHead.forward_train')
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
