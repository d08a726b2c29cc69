"""Training losses of the pose head, in torch so that autograd reaches ``pose_cov``, ``cov_calib_logscale`` and, through
``pnp_uncert(..., differentiable=True)``, the coordinate maps.

``KLLossMV`` is the only pose-head loss a shipped MonoRUn config names (``loss_calib``, installed by ``LossUpdaterHook`` at
iteration 100).  It is the negative log-likelihood of the pose error d under N(0, cov), up to a constant:

    loss = 0.5 * (d^T inv_cov d - logdet(inv_cov)),   0 where logdet(inv_cov) is NaN or +-inf,

reduced as mmdet's ``weighted_loss`` reduces ('none' | 'mean' | 'sum', optional element weight and ``avg_factor``) and scaled by
``loss_weight``.

``build_loss`` builds a loss config dict: with mmdet's registry when mmdet imports and knows the type, else with this module's
registry.  A type neither knows becomes an ``UnbuiltLoss``, which raises, naming the type, only when it is called.
"""
import torch
import torch.nn as nn


def weight_reduce_loss(loss, weight=None, reduction='mean', avg_factor=None):
    """mmdet's element-wise loss reduction: optional weight, then 'none' / 'mean' / 'sum'; with ``avg_factor``, 'mean' is sum / avg_factor."""
    if weight is not None:
        loss = loss * weight
    if avg_factor is None:
        if reduction == 'mean':
            return loss.mean()
        if reduction == 'sum':
            return loss.sum()
        if reduction == 'none':
            return loss
        raise ValueError(f'unknown reduction {reduction!r}')
    if reduction == 'mean':
        return loss.sum() / avg_factor
    if reduction == 'none':
        return loss
    raise ValueError('avg_factor can not be used with reduction="sum"')


def kl_loss_mv(pred, target, inv_cov):
    """Element-wise (*, 1) loss of ``KLLossMV``: pred (*, n), target (*, n) or the integer 0 (pred is then the difference itself),
    inv_cov (*, n, n)."""
    if inv_cov is None or pred.shape[:-1] != inv_cov.shape[:-2]:
        raise ValueError('kl_loss_mv: inv_cov must be given with shape pred.shape[:-1] + (n, n)')
    if isinstance(target, int):
        if target != 0:
            raise ValueError('kl_loss_mv: an integer target must be 0')
        d = pred
    else:
        if pred.shape != target.shape or target.numel() == 0:
            raise ValueError('kl_loss_mv: pred and target must have the same non-empty shape')
        d = pred - target
    logdet = torch.logdet(inv_cov)
    maha = (d.unsqueeze(-2) @ inv_cov @ d.unsqueeze(-1)).flatten()
    loss = (maha - logdet) / 2
    loss = torch.where(torch.isnan(logdet) | torch.isinf(logdet), torch.zeros_like(loss), loss)
    return loss.unsqueeze(-1)


class KLLossMV(nn.Module):
    """Multivariate Gaussian KL / NLL loss of the pose covariance (no parameters, no buffers)."""

    def __init__(self, reduction='mean', loss_weight=1.0):
        super().__init__()
        self.reduction = reduction
        self.loss_weight = loss_weight

    def forward(self, pred, target, inv_cov=None, weight=None, avg_factor=None, reduction_override=None):
        if reduction_override not in (None, 'none', 'mean', 'sum'):
            raise ValueError(f'KLLossMV: reduction_override {reduction_override!r}')
        reduction = reduction_override if reduction_override else self.reduction
        return self.loss_weight * weight_reduce_loss(kl_loss_mv(pred, target, inv_cov), weight, reduction, avg_factor)


LOSSES = {'KLLossMV': KLLossMV}


class UnbuiltLoss:
    """Stands in for a loss config whose type no registry knows: the head still constructs and runs ``forward``; calling the loss
    raises."""

    def __init__(self, cfg):
        self.cfg = dict(cfg)

    def __call__(self, *args, **kwargs):
        raise RuntimeError(f"loss type {self.cfg.get('type')!r} is not available: it is not in monorun_amd.losses and mmdet "
                           'is not importable or does not register it')

    def __repr__(self):
        return f'UnbuiltLoss({self.cfg!r})'


def build_loss(cfg):
    if cfg is None:
        return None
    cfg = dict(cfg)
    typ = cfg.get('type')
    try:
        from mmdet.models.builder import LOSSES as MMDET_LOSSES, build_loss as mmdet_build_loss
    except ImportError:
        MMDET_LOSSES = None
    if MMDET_LOSSES is not None and MMDET_LOSSES.get(typ) is not None:
        return mmdet_build_loss(cfg)
    if typ in LOSSES:
        return LOSSES[cfg.pop('type')](**cfg)
    return UnbuiltLoss(cfg)
