"""The two losses of the 2-D detector's heads that :mod:`monorun_amd.losses` does not restate: mmdet's ``SmoothL1Loss``
(the ``loss_bbox`` of the RPN and of the box head) and the softmax form of its ``CrossEntropyLoss`` (the box head's ``loss_cls``), in torch.

    SmoothL1Loss:             d = |pred − target|;  0.5·d²/β where d < β, else d − 0.5·β
    SoftmaxCrossEntropyLoss:  −log softmax(cls_score)[label]

both reduced as mmdet's ``weighted_loss`` reduces (:func:`monorun_amd.losses.weight_reduce_loss`) and scaled by ``loss_weight``.

:mod:`monorun_amd.losses` is left as it is: without mmdet ``build_loss(dict(type='SmoothL1Loss'))`` is an ``UnbuiltLoss`` and
``CrossEntropyLoss(use_sigmoid=False)`` raises, and the heads keep those attributes.  The heads' ``loss`` methods go through
:func:`resolve`, which builds the loss such an ``UnbuiltLoss`` names, once.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .losses import UnbuiltLoss, weight_reduce_loss


def smooth_l1_loss(pred, target, beta=1.0):
    """mmdet's element-wise ``smooth_l1_loss``."""
    assert beta > 0 and pred.shape == target.shape, 'smooth_l1_loss: beta > 0 and one shape'
    diff = torch.abs(pred - target)
    return torch.where(diff < beta, 0.5 * diff * diff / beta, diff - 0.5 * beta)


def _reduction(override, own, name):
    if override not in (None, 'none', 'mean', 'sum'):
        raise ValueError(f'{name}: reduction_override {override!r}')
    return override if override else own


class SmoothL1Loss(nn.Module):
    """mmdet's ``SmoothL1Loss``.  An empty target gives ``pred.sum()·0``, as mmdet's does."""

    def __init__(self, beta=1.0, reduction='mean', loss_weight=1.0):
        super().__init__()
        self.beta, self.reduction, self.loss_weight = beta, reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None, **kwargs):
        reduction = _reduction(reduction_override, self.reduction, 'SmoothL1Loss')
        if target.numel() == 0:
            return pred.sum() * 0
        return self.loss_weight * weight_reduce_loss(smooth_l1_loss(pred, target, self.beta), weight, reduction, avg_factor)


class SoftmaxCrossEntropyLoss(nn.Module):
    """The softmax form of mmdet's ``CrossEntropyLoss`` (``use_sigmoid=False``, ``use_mask=False``): cls_score (R, C), label (R,) int64,
    weight (R,) or None."""

    def __init__(self, use_sigmoid=False, use_mask=False, reduction='mean', class_weight=None, loss_weight=1.0):
        super().__init__()
        if use_sigmoid or use_mask:
            raise NotImplementedError('SoftmaxCrossEntropyLoss is the softmax form (monorun_amd.losses.CrossEntropyLoss is the sigmoid form)')
        self.use_sigmoid, self.use_mask, self.reduction, self.class_weight, self.loss_weight = False, False, reduction, class_weight, loss_weight

    def forward(self, cls_score, label, weight=None, avg_factor=None, reduction_override=None, **kwargs):
        reduction = _reduction(reduction_override, self.reduction, 'SoftmaxCrossEntropyLoss')
        class_weight = None if self.class_weight is None else cls_score.new_tensor(self.class_weight)
        loss = F.cross_entropy(cls_score, label, weight=class_weight, reduction='none')
        if weight is not None:
            weight = weight.to(loss.dtype)
        return self.loss_weight * weight_reduce_loss(loss, weight, reduction, avg_factor)


def _names(cfg):
    """The class an unbuilt config names, or None: ``SmoothL1Loss``; ``SoftmaxCrossEntropyLoss`` or mmdet's spelling of it,
    ``CrossEntropyLoss`` with ``use_sigmoid=False``."""
    kind = cfg.get('type')
    if kind == 'SmoothL1Loss':
        return SmoothL1Loss
    if kind == 'SoftmaxCrossEntropyLoss' or (kind == 'CrossEntropyLoss' and not cfg.get('use_sigmoid', False) and not cfg.get('use_mask', False)):
        return SoftmaxCrossEntropyLoss
    return None


def resolve(loss):
    """The callable behind a head's loss attribute: for an ``UnbuiltLoss`` whose config names one of this module's two losses, that loss,
    built once and cached on the ``UnbuiltLoss`` (the attribute itself stays what it was); anything else is returned as it is."""
    if not isinstance(loss, UnbuiltLoss):
        return loss
    cls = _names(loss.cfg)
    if cls is None:
        return loss
    if getattr(loss, '_resolved', None) is None:
        cfg = dict(loss.cfg)
        cfg.pop('type')
        loss._resolved = cls(**cfg)
    return loss._resolved
