"""Training losses of the pose head, in torch so that autograd reaches ``pose_cov``, ``cov_calib_logscale`` and, through
``pnp_uncert(..., differentiable=True)``, the coordinate maps.

``KLLossMV`` is the only pose-head loss a shipped MonoRUn config names (``loss_calib``, installed by ``LossUpdaterHook`` at
iteration 100).  It is the negative log-likelihood of the pose error d under N(0, cov), up to a constant:

    loss = 0.5 * (d^T inv_cov d - logdet(inv_cov)),   0 where logdet(inv_cov) is NaN or +-inf,

reduced as mmdet's ``weighted_loss`` reduces ('none' | 'mean' | 'sum', optional element weight and ``avg_factor``) and scaled by
``loss_weight``.

``RobustKLLoss`` is the NOC head's projection loss (``loss_proj`` of ``UncertProjectionHead``), the only loss that
trains the NOC head in the shipped configs with ``loss_noc=None``.  Its reduced forms on CUDA run HIP kernels; the rest runs in torch.

``CrossEntropyLoss`` is the sigmoid form of mmdet's loss of that name, the score head's ``loss_score``, in torch.

``SmoothL1LossMod`` is the NOC head's ``loss_noc`` of the LiDAR-supervised configs, the reference's
monorun/models/losses/smooth_l1_loss.py.  Its reduced forms on CUDA run HIP kernels; the rest runs in torch.

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




# ---------------------------------------------------------------------------------------------------------------------------------
# RobustKLLoss: the NOC head's projection loss, the reference's monorun/models/losses/robust_kl_loss.py.

def robust_kl_loss(pred, target, logstd=None, delta=1.414, momentum=1.0, mean_inv_std=None, eps=1e-4, training=True):
    """Element-wise robust KL loss, divided by the running mean of the inverse std; in training mode the running mean (the
    buffer ``mean_inv_std``, 0-dim) is first updated in place.  target: 0 (pred is the error), -1 (pred is the non-negative
    distance) or a tensor."""
    if logstd is None or pred.size() != logstd.size():
        raise ValueError('robust_kl_loss: logstd must be given with the shape of pred')
    if isinstance(target, int):
        if target not in (0, -1):
            raise ValueError(f'robust_kl_loss: an integer target must be 0 or -1, not {target}')
        diff = pred.abs() if target == 0 else pred
    else:
        diff = (pred - target).abs()
    inv_std = torch.exp(-logstd).clamp(max=1 / eps)
    dw = diff * inv_std
    loss = torch.where(dw < delta, 0.5 * dw.square(), delta * (dw - 0.5 * delta)) + logstd
    if training:
        with torch.no_grad():
            mean_inv_std.mul_(1 - momentum)
            mean_inv_std.add_(momentum * inv_std.detach().mean())
    return loss / mean_inv_std.clamp(min=1e-6)


class _RobustKLFunction(torch.autograd.Function):
    """Reduced loss in two HIP launches (``mr_robust_kl_loss``), both gradients in one (``mr_robust_kl_loss_backward``).  pred
    and logstd arrive as contiguous fp32; the buffer is updated on the device, and the divisor c it gave is saved for the
    backward, which therefore never reads the buffer (it may have moved since) and never waits for the host."""

    @staticmethod
    def forward(ctx, pred, logstd, buf, mode, delta, eps, momentum, training, reduction, loss_weight):
        from . import _lib
        lib = _lib.load()
        numel = pred.numel()
        dev = pred.device
        loss = torch.empty((), device=dev, dtype=torch.float32)
        c = torch.empty((), device=dev, dtype=torch.float32)
        ws = torch.empty(int(lib.mr_robust_kl_workspace_bytes(numel)), device=dev, dtype=torch.uint8)
        with torch.cuda.device(dev):
            _lib.call('mr_robust_kl_loss', pred=pred.data_ptr(), logstd=logstd.data_ptr(), numel=numel, target_mode=mode, delta=delta, eps=eps,
                      momentum=momentum, training=int(training), reduction=reduction, loss_weight=loss_weight, mean_inv_std=buf.data_ptr(),
                      loss=loss.data_ptr(), c_out=c.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=ws.numel(),
                      stream=torch.cuda.current_stream(dev).cuda_stream)
        ctx.save_for_backward(pred, logstd, c)
        ctx.args = (mode, delta, eps, reduction, loss_weight)
        return loss

    @staticmethod
    def backward(ctx, grad):
        from . import _lib
        pred, logstd, c = ctx.saved_tensors
        mode, delta, eps, reduction, loss_weight = ctx.args
        grad = grad.to(torch.float32).contiguous()
        gp, gl = torch.empty_like(pred), torch.empty_like(logstd)
        dev = pred.device
        with torch.cuda.device(dev):
            _lib.call('mr_robust_kl_loss_backward', pred=pred.data_ptr(), logstd=logstd.data_ptr(), numel=pred.numel(), target_mode=mode,
                      delta=delta, eps=eps, reduction=reduction, loss_weight=loss_weight, grad_loss=grad.data_ptr(), c=c.data_ptr(),
                      grad_pred=gp.data_ptr(), grad_logstd=gl.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
        return gp, gl, None, None, None, None, None, None, None, None


def _robust_kl_hip_ok(pred, target, logstd, buf, weight, avg_factor, reduction):
    if weight is not None or avg_factor is not None or reduction not in ('mean', 'sum'):
        return False
    if not (isinstance(pred, torch.Tensor) and isinstance(logstd, torch.Tensor)) or pred.device.type != 'cuda':
        return False
    if logstd.device != pred.device or logstd.shape != pred.shape or pred.numel() == 0:
        return False
    if buf.device != pred.device or buf.dtype != torch.float32 or buf.dim() != 0:
        return False
    if isinstance(target, int):
        return target in (0, -1)
    return isinstance(target, torch.Tensor) and target.device == pred.device and target.shape == pred.shape


class RobustKLLoss(nn.Module):
    """The reference's RobustKLLoss: same constructor, buffer ``mean_inv_std`` (0-dim fp32, initially 1, updated in training mode
    only) and call forms.  CUDA inputs without ``weight`` / ``avg_factor`` and with reduction 'mean' or 'sum' run the HIP kernels;
    everything else runs :func:`robust_kl_loss` in torch."""

    def __init__(self, delta=1.414, reduction='mean', loss_weight=1.0, momentum=1.0, eps=1e-4):
        super().__init__()
        self.delta = delta
        self.reduction = reduction
        self.loss_weight = loss_weight
        self.eps = eps
        self.momentum = momentum
        self.register_buffer('mean_inv_std', torch.tensor(1, dtype=torch.float))

    def forward(self, pred, target, logstd=None, weight=None, avg_factor=None, reduction_override=None, **kwargs):
        if reduction_override not in (None, 'none', 'mean', 'sum'):
            raise ValueError(f'RobustKLLoss: reduction_override {reduction_override!r}')
        if kwargs:
            raise TypeError(f'RobustKLLoss: unexpected arguments {sorted(kwargs)}')
        reduction = reduction_override if reduction_override else self.reduction
        if _robust_kl_hip_ok(pred, target, logstd, self.mean_inv_std, weight, avg_factor, reduction):
            if isinstance(target, int):
                x, mode = pred, target
            else:
                x, mode = pred - target, 0
            loss = _RobustKLFunction.apply(x.to(torch.float32).contiguous(), logstd.to(torch.float32).contiguous(), self.mean_inv_std,
                                           mode, float(self.delta), float(self.eps), float(self.momentum), self.training,
                                           0 if reduction == 'mean' else 1, float(self.loss_weight))
            return loss.to(pred.dtype)
        loss = robust_kl_loss(pred, target, logstd=logstd, delta=self.delta, momentum=self.momentum, mean_inv_std=self.mean_inv_std,
                              eps=self.eps, training=self.training)
        return self.loss_weight * weight_reduce_loss(loss, weight, reduction, avg_factor)


# ---------------------------------------------------------------------------------------------------------------------------------
# SmoothL1LossMod: the NOC head's loss_noc, the reference's monorun/models/losses/smooth_l1_loss.py.

def smooth_l1_loss_mod(pred, target, beta=1.0):
    """The per-element loss of ``SmoothL1LossMod``: with the distance d between pred and target, half a parabola 0.5 d d / beta below
    beta and the line d - 0.5 beta from there on.  target: a tensor of pred's shape, or the integer 0 (pred is the signed error) or -1
    (pred is the distance itself, taken as given)."""
    if not beta > 0:
        raise ValueError(f'smooth_l1_loss_mod: beta must be positive, not {beta}')
    if isinstance(target, int):
        if target not in (0, -1):
            raise ValueError(f'smooth_l1_loss_mod: an integer target must be 0 or -1, not {target}')
        distance = pred if target == -1 else pred.abs()
    else:
        if target.shape != pred.shape or target.numel() == 0:
            raise ValueError('smooth_l1_loss_mod: pred and target must have the same non-empty shape')
        distance = (pred - target).abs()
    parabola = 0.5 * distance * distance / beta
    line = distance - 0.5 * beta
    return torch.where(distance < beta, parabola, line)


class _SmoothL1ModFunction(torch.autograd.Function):
    """Reduced loss in two HIP launches (``mr_smooth_l1_mod_loss``), the gradient to pred in one (``mr_smooth_l1_mod_loss_backward``).
    pred, target and weight arrive as contiguous fp32; target and weight get no gradient."""

    @staticmethod
    def forward(ctx, pred, target, weight, weight_mode, channels, hw, beta, reduction, loss_weight):
        from . import _lib
        lib = _lib.load()
        numel = pred.numel()
        dev = pred.device
        loss = torch.empty((), device=dev, dtype=torch.float32)
        ws = torch.empty(int(lib.mr_smooth_l1_mod_workspace_bytes(numel)), device=dev, dtype=torch.uint8)
        ctx.common = dict(pred=pred.data_ptr(), target=target.data_ptr(), weight=_lib.ptr(weight), weight_mode=weight_mode, numel=numel,
                          channels=channels, hw=hw, beta=beta, reduction=reduction, loss_weight=loss_weight)
        with torch.cuda.device(dev):
            _lib.call('mr_smooth_l1_mod_loss', ctx.common, loss=loss.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=ws.numel(),
                      stream=torch.cuda.current_stream(dev).cuda_stream)
        ctx.save_for_backward(pred, target, weight)
        ctx.args = (beta, reduction, loss_weight)
        return loss

    @staticmethod
    def backward(ctx, grad):
        from . import _lib
        pred, target, weight = ctx.saved_tensors
        if torch.is_grad_enabled():
            # create_graph=True: the gradient must carry a graph itself, which the kernel cannot give: torch differentiates the restatement
            beta, reduction, loss_weight = ctx.args
            with torch.enable_grad():
                loss = loss_weight * weight_reduce_loss(smooth_l1_loss_mod(pred, target, beta), weight, 'mean' if reduction == 0 else 'sum')
                gp, = torch.autograd.grad(loss, pred, grad, create_graph=True)
            return (gp,) + (None,) * 8
        grad = grad.to(torch.float32).contiguous()
        gp = torch.empty_like(pred)
        dev = pred.device
        with torch.cuda.device(dev):
            _lib.call('mr_smooth_l1_mod_loss_backward', ctx.common, grad_loss=grad.data_ptr(), grad_pred=gp.data_ptr(),
                      stream=torch.cuda.current_stream(dev).cuda_stream)
        return (gp,) + (None,) * 8


def _smooth_l1_weight_mode(pred, weight):
    """0 no weight, 1 of pred's shape, 2 (n, 1, h, w) against a 4-D pred; None: a form the kernels do not take."""
    if weight is None:
        return 0
    if not isinstance(weight, torch.Tensor) or weight.device != pred.device or weight.dtype != torch.float32:
        return None
    if weight.shape == pred.shape:
        return 1
    if pred.dim() == 4 and weight.shape == (pred.shape[0], 1) + tuple(pred.shape[2:]):
        return 2
    return None


def _smooth_l1_hip_ok(pred, target, weight, avg_factor, reduction):
    if avg_factor is not None or reduction not in ('mean', 'sum'):
        return False
    if not (isinstance(pred, torch.Tensor) and isinstance(target, torch.Tensor)) or pred.device.type != 'cuda':
        return False
    if pred.dtype != torch.float32 or target.dtype != torch.float32 or target.device != pred.device:
        return False
    if target.shape != pred.shape or pred.numel() == 0:
        return False
    return _smooth_l1_weight_mode(pred, weight) is not None


class SmoothL1LossMod(nn.Module):
    """The reference's SmoothL1LossMod: same constructor and call forms.  CUDA fp32 ``pred`` and tensor ``target`` of its shape, with
    reduction 'mean' or 'sum', no ``avg_factor`` and a weight that is None, of pred's shape or (n, 1, h, w), run the HIP kernels (fp64
    sum, bitwise reproducible); everything else — integer targets, 'none', ``avg_factor``, CPU or empty inputs, a backward under
    ``create_graph=True`` — runs :func:`smooth_l1_loss_mod` in torch."""

    def __init__(self, beta=1.0, reduction='mean', loss_weight=1.0):
        super().__init__()
        self.beta = beta
        self.reduction = reduction
        self.loss_weight = loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None, **kwargs):
        if reduction_override not in (None, 'none', 'mean', 'sum'):
            raise ValueError(f'SmoothL1LossMod: reduction_override {reduction_override!r}')
        if kwargs:
            raise TypeError(f'SmoothL1LossMod: unexpected arguments {sorted(kwargs)}')
        reduction = reduction_override if reduction_override else self.reduction
        if _smooth_l1_hip_ok(pred, target, weight, avg_factor, reduction):
            if not self.beta > 0:
                raise ValueError(f'SmoothL1LossMod: beta must be positive, not {self.beta}')
            mode = _smooth_l1_weight_mode(pred, weight)
            channels, hw = (pred.shape[1], pred.shape[2] * pred.shape[3]) if mode == 2 else (1, 1)
            return _SmoothL1ModFunction.apply(pred.contiguous(), target.detach().contiguous(), weight.detach().contiguous() if mode else None,
                                              mode, int(channels), int(hw), float(self.beta), 0 if reduction == 'mean' else 1,
                                              float(self.loss_weight))
        return self.loss_weight * weight_reduce_loss(smooth_l1_loss_mod(pred, target, beta=self.beta), weight, reduction, avg_factor)


class CrossEntropyLoss(nn.Module):
    """The sigmoid form of mmdet's ``CrossEntropyLoss`` (``use_sigmoid=True``), the score head's default ``loss_score``:
    ``binary_cross_entropy_with_logits(pred, target)`` per element, then :func:`weight_reduce_loss`.  ``weight`` is per sample:
    it is reshaped to ``pred``'s shape, so an (N,) weight scales the rows of an (N, 1) loss and never broadcasts to (N, N).
    The softmax and mask forms are not restated: ``use_sigmoid=False`` raises."""

    def __init__(self, use_sigmoid=True, reduction='mean', loss_weight=1.0):
        super().__init__()
        if not use_sigmoid:
            raise NotImplementedError('monorun_amd.losses.CrossEntropyLoss restates the sigmoid form only (use_sigmoid=True)')
        self.use_sigmoid = True
        self.reduction = reduction
        self.loss_weight = loss_weight

    def forward(self, cls_score, label, weight=None, avg_factor=None, reduction_override=None):
        if reduction_override not in (None, 'none', 'mean', 'sum'):
            raise ValueError(f'CrossEntropyLoss: reduction_override {reduction_override!r}')
        reduction = reduction_override if reduction_override else self.reduction
        loss = nn.functional.binary_cross_entropy_with_logits(cls_score, label.to(cls_score.dtype).reshape(cls_score.shape), reduction='none')
        if weight is not None:
            weight = weight.to(loss.dtype).reshape(loss.shape)
        return self.loss_weight * weight_reduce_loss(loss, weight, reduction, avg_factor)


LOSSES = {'KLLossMV': KLLossMV, 'RobustKLLoss': RobustKLLoss, 'CrossEntropyLoss': CrossEntropyLoss, 'SmoothL1LossMod': SmoothL1LossMod}


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
