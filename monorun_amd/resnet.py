"""The backbone (N13): mmdet's ``ResNet`` without mmcv / mmdet, and the op its norms run when they use their running
statistics.  Every shipped config builds ``ResNet(depth=101, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1,
norm_cfg=dict(type='BN', requires_grad=True), norm_eval=True, style='pytorch')``: all 104 batch norms are per-channel affine maps, in
training as at test time, and the four maps it returns are what ``FPNplus`` consumes.

The convolutions are torch's (MIOpen on a HIP device).  What runs after each of them is the op :func:`bn_act`.  ``x`` (N, C, H, W), fp32,
every operation rounded on its own, c the channel:

  ``istd[c] = 1 / sqrt(var[c] + eps)``;  ``xhat = (x − mean[c]) · istd[c]``;  ``t = xhat · weight[c] + bias[c]`` (a missing weight or
  bias skips its operation);  ``u = t + residual`` (when given);  ``y = (u <= 0 ? +0 : u)`` under ``relu``, else ``u``.

Its backward from ``g``: ``gm = (y <= 0 ? +0 : g)`` under ``relu``; ``grad_residual = gm``; ``grad_x = gm · k[c]`` with ``k = istd ·
weight`` rounded once; ``grad_bias[c] = Σ gm``; ``grad_weight[c] = Σ gm · xhat``.  include/monorun_backbone.h states the order of the sums.

Hot path: on CUDA fp32 contiguous maps ONE fused HIP launch forward (``mr_bn_act_forward``: the eager chain is two to three) and one
backward, two when a parameter gradient is asked for (``mr_bn_act_backward``: no atomics, no memset, bitwise reproducible); an output that
is not needed is neither computed nor stored.  The stem's ``bn → relu → max_pool2d(3, 2, 1)`` is one launch that never writes the
full-resolution map (``mr_bn_relu_maxpool_forward``), used when no gradient is required through the stem.  Everything else — CPU, other
dtypes, non-contiguous or channels-last maps, a backward under ``create_graph=True`` — runs the torch restatement, :func:`bn_act_torch`.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib


CHUNK = 4096            # MR_BN_CHUNK of include/monorun_backbone.h


# ------------------------------------------------------------------------------------------------ the op
def _per_channel(t, like):
    return t.to(like.dtype).view(1, -1, 1, 1)


def _istd(var, eps, dtype):
    """``1 / sqrt(var + eps)`` per channel, every operation correctly rounded in `dtype`.  torch's vectorised fp32 ``sqrt`` is not always
    correctly rounded on a CPU; the fp64 root of an fp32 number, rounded to fp32, is (53 >= 2 * 24 + 2 bits)."""
    if dtype == torch.float64:
        return 1.0 / torch.sqrt(var.to(dtype) + eps)
    return 1.0 / torch.sqrt((var.to(torch.float32) + eps).to(torch.float64)).to(torch.float32)


def _forward_torch(x, mean, var, weight, bias, eps, residual, relu):
    """the definition in torch ops, operation for operation; fp16 / bf16 maps are computed in fp32 and returned in their dtype"""
    work = x if x.dtype in (torch.float32, torch.float64) else x.to(torch.float32)
    istd = _istd(var, eps, work.dtype)
    u = (work - _per_channel(mean, work)) * _per_channel(istd, work)
    if weight is not None:
        u = u * _per_channel(weight, work)
    if bias is not None:
        u = u + _per_channel(bias, work)
    if residual is not None:
        u = u + residual.to(work.dtype)
    if relu:
        u = torch.where(u <= 0, torch.zeros((), dtype=work.dtype, device=work.device), u)
    return u.to(x.dtype)


def _backward_torch(g, y, x, mean, var, weight, eps, relu, need_x, need_w, need_b, need_r):
    """the backward of the definition in torch ops (differentiable itself): grad_x, grad_weight, grad_bias, grad_residual or None"""
    work = g if g.dtype in (torch.float32, torch.float64) else g.to(torch.float32)
    gm = torch.where(y.to(work.dtype) <= 0, torch.zeros((), dtype=work.dtype, device=work.device), work) if relu else work
    istd = _istd(var, eps, work.dtype)
    gx = gw = gb = None
    if need_x:
        k = istd * weight.to(work.dtype) if weight is not None else istd
        gx = (gm * _per_channel(k, work)).to(g.dtype)
    if need_w:
        xhat = (x.to(work.dtype) - _per_channel(mean, work)) * _per_channel(istd, work)
        gw = (gm * xhat).sum(dim=(0, 2, 3)).to(weight.dtype)
    if need_b:
        gb = gm.sum(dim=(0, 2, 3))
    return gx, gw, gb, (gm.to(g.dtype) if need_r else None)


def hip_ok(x, running_mean, running_var, weight=None, bias=None, residual=None):
    """Whether the fused HIP launches cover this call: a CUDA fp32 contiguous (N, C, H, W) map of fewer than 2^31 elements, fp32
    contiguous per-channel vectors and a residual of the map's shape on its device, statistics that need no gradient.  (A backward under
    ``create_graph=True`` is the restatement's, decided when it runs.)"""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype is torch.float32 and x.dim() == 4 and x.is_contiguous()
            and 1 <= x.numel() < 2 ** 31):
        return False
    if running_mean is None or running_var is None or running_mean.requires_grad or running_var.requires_grad:
        return False
    dev, shape = x.device, x.shape[1:2]
    for v in (running_mean, running_var, weight, bias):
        if v is not None and not (v.dtype is torch.float32 and v.shape == shape and v.device == dev and v.is_contiguous()):
            return False
    return residual is None or (residual.dtype is torch.float32 and residual.shape == x.shape and residual.device == dev
                                and residual.is_contiguous())


def _launch(fn, dev, **named):
    """`fn` by its header's argument names on the current stream of `dev`; the device is switched only when it is not the current one
    (the host's share of a call is what a single norm costs at the small stages)"""
    stream = torch._C._cuda_getCurrentRawStream(dev.index)
    if torch._C._cuda_getDevice() == dev.index:
        _lib.call(fn, stream=stream, **named)
    else:
        with torch.cuda.device(dev):
            _lib.call(fn, stream=stream, **named)


class _BnActFunction(torch.autograd.Function):
    """``y = bn_act(x)``: ``mr_bn_act_forward`` / ``mr_bn_act_backward`` with ``hip``, the torch restatement of both without.  Saves y
    (under relu) and the per-channel vectors, and x only when a parameter gradient can be asked for."""

    @staticmethod
    def forward(ctx, x, mean, var, weight, bias, residual, eps, relu, hip):
        ctx.eps, ctx.relu, ctx.hip = float(eps), bool(relu), bool(hip)
        ctx.set_materialize_grads(False)
        if hip:
            y = torch.empty_like(x)
            N, C, H, W = x.shape
            _launch('mr_bn_act_forward', x.device, x=x.data_ptr(), mean=mean.data_ptr(), var=var.data_ptr(), weight=_lib.ptr(weight),
                    bias=_lib.ptr(bias), r=_lib.ptr(residual), n_images=N, channels=C, height=H, width=W, eps=ctx.eps, relu=int(ctx.relu),
                    y=y.data_ptr())
        else:
            y = _forward_torch(x, mean, var, weight, bias, ctx.eps, residual, ctx.relu)
        need = ctx.needs_input_grad
        params = (weight is not None and need[3]) or (bias is not None and need[4])
        ctx.has_residual = residual is not None
        if need[0] or params or (ctx.has_residual and need[5]):
            ctx.save_for_backward(y if ctx.relu else None, x if (weight is not None and need[3]) else None, mean, var, weight)
        return y

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return (None,) * 9
        y, x, mean, var, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        need_x, need_w, need_b, need_r = need[0], weight is not None and need[3], need[4], ctx.has_residual and need[5]
        if not ctx.hip or torch.is_grad_enabled() or g.dtype != torch.float32:
            # the restatement, and every backward under create_graph=True: the gradients must carry a graph, which the kernel cannot give
            gx, gw, gb, gr = _backward_torch(g, y, x, mean, var, weight, ctx.eps, ctx.relu, need_x, need_w, need_b, need_r)
            return gx, None, None, gw, gb, gr, None, None, None
        g = g.contiguous()
        dev = g.device
        N, C, H, W = g.shape
        gx = torch.empty_like(g) if need_x else None
        gr = torch.empty_like(g) if need_r else None
        gw = torch.empty(C, device=dev, dtype=torch.float32) if need_w else None
        gb = torch.empty(C, device=dev, dtype=torch.float32) if need_b else None
        ws = None
        if need_w or need_b:            # mr_bn_act_backward_workspace_bytes: a pair of floats per chunk
            ws = torch.empty(2 * N * C * (-(-(H * W) // CHUNK)), device=dev, dtype=torch.float32)
            if x is None:           # only the bias asks: the weight sums are formed from g's own values and dropped
                x = g
        _launch('mr_bn_act_backward', dev, g=g.data_ptr(), y=_lib.ptr(y), x=_lib.ptr(x), mean=mean.data_ptr(), var=var.data_ptr(),
                weight=_lib.ptr(weight), n_images=N, channels=C, height=H, width=W, eps=ctx.eps, relu=int(ctx.relu), grad_x=_lib.ptr(gx),
                grad_r=_lib.ptr(gr), grad_weight=_lib.ptr(gw), grad_bias=_lib.ptr(gb), workspace=_lib.ptr(ws))
        return gx, None, None, gw, gb, gr, None, None, None


def bn_act_torch(x, running_mean, running_var, weight=None, bias=None, eps=1e-5, residual=None, relu=True):
    """The op in torch ops on any device and floating dtype, differentiable (twice): the same operations in the same order, forward and
    backward (``grad_x = gm · (istd · weight)``); only the order of the two per-channel sums is torch's."""
    return _BnActFunction.apply(x, running_mean, running_var, weight, bias, residual, eps, relu, False)


def bn_act(x, running_mean, running_var, weight=None, bias=None, eps=1e-5, residual=None, relu=True):
    """Frozen-statistics batch norm, the residual add and the ReLU: x (N, C, H, W) -> y of its shape, differentiable in x, weight, bias and
    residual.  The fused HIP launches when :func:`hip_ok`, else the restatement."""
    hip = hip_ok(x, running_mean, running_var, weight, bias, residual)
    return _BnActFunction.apply(x, running_mean, running_var, weight, bias, residual, eps, relu, hip)


def bn_relu_maxpool_torch(x, running_mean, running_var, weight=None, bias=None, eps=1e-5):
    """``max_pool2d(bn_act(x, relu=True), kernel 3, stride 2, padding 1)`` by the restatement"""
    return F.max_pool2d(bn_act_torch(x, running_mean, running_var, weight, bias, eps, None, True), kernel_size=3, stride=2, padding=1)


def bn_relu_maxpool(x, running_mean, running_var, weight=None, bias=None, eps=1e-5):
    """The stem: the norm, the ReLU and the 3×3 / stride-2 / padding-1 max pooling.  One fused HIP launch that never writes the
    full-resolution map when :func:`hip_ok` and no gradient is required through it (forward only: the stem is frozen and the image needs
    no gradient in every reference config); else :func:`bn_act` followed by ``F.max_pool2d``."""
    wants_grad = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, weight, bias))
    if wants_grad or not hip_ok(x, running_mean, running_var, weight, bias):
        return F.max_pool2d(bn_act(x, running_mean, running_var, weight, bias, eps, None, True), kernel_size=3, stride=2, padding=1)
    N, C, H, W = x.shape
    p = torch.empty(N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1, device=x.device, dtype=torch.float32)
    _launch('mr_bn_relu_maxpool_forward', x.device, x=x.data_ptr(), mean=running_mean.data_ptr(), var=running_var.data_ptr(),
            weight=_lib.ptr(weight), bias=_lib.ptr(bias), n_images=N, channels=C, height=H, width=W, eps=float(eps), p=p.data_ptr())
    return p


# ------------------------------------------------------------------------------------------------ the modules
def _norm_act(norm, x, residual=None, relu=True):
    """one norm of a block with what follows it: the fused op when the norm uses its running statistics, ``nn.BatchNorm2d.forward`` with a
    separate add and ReLU when it uses the batch's"""
    if not norm.training and norm.track_running_stats:
        return bn_act(x, norm.running_mean, norm.running_var, norm.weight, norm.bias, norm.eps, residual, relu)
    x = norm(x)
    if residual is not None:
        x = x + residual
    return F.relu(x) if relu else x


def _build_norm(norm_cfg, channels):
    norm = nn.BatchNorm2d(channels, eps=norm_cfg.get('eps', 1e-5), momentum=norm_cfg.get('momentum', 0.1))
    for p in norm.parameters():
        p.requires_grad = norm_cfg.get('requires_grad', True)
    return norm


class BasicBlock(nn.Module):
    """mmdet's ``BasicBlock``: two 3×3 convolutions (``conv1``, ``bn1``, ``conv2``, ``bn2``, ``downsample``)"""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, style='pytorch', norm_cfg=dict(type='BN')):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride=stride, padding=dilation, dilation=dilation, bias=False)
        self.bn1 = _build_norm(norm_cfg, planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = _build_norm(norm_cfg, planes)
        self.downsample = downsample
        self.stride, self.dilation = stride, dilation

    @property
    def last_norm(self):
        return self.bn2

    def forward(self, x):
        identity = x if self.downsample is None else _norm_act(self.downsample[1], self.downsample[0](x), None, False)
        out = _norm_act(self.bn1, self.conv1(x))
        return _norm_act(self.bn2, self.conv2(out), identity, True)


class Bottleneck(nn.Module):
    """mmdet's ``Bottleneck``: 1×1, 3×3, 1×1; the stride sits on ``conv2`` with ``style='pytorch'`` and on ``conv1`` with ``'caffe'``"""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, style='pytorch', norm_cfg=dict(type='BN')):
        super().__init__()
        assert style in ('pytorch', 'caffe')
        s1, s2 = (1, stride) if style == 'pytorch' else (stride, 1)
        self.conv1 = nn.Conv2d(inplanes, planes, 1, stride=s1, bias=False)
        self.bn1 = _build_norm(norm_cfg, planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=s2, padding=dilation, dilation=dilation, bias=False)
        self.bn2 = _build_norm(norm_cfg, planes)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, 1, bias=False)
        self.bn3 = _build_norm(norm_cfg, planes * self.expansion)
        self.downsample = downsample
        self.stride, self.dilation, self.style = stride, dilation, style

    @property
    def last_norm(self):
        return self.bn3

    def forward(self, x):
        identity = x if self.downsample is None else _norm_act(self.downsample[1], self.downsample[0](x), None, False)
        out = _norm_act(self.bn1, self.conv1(x))
        out = _norm_act(self.bn2, self.conv2(out))
        return _norm_act(self.bn3, self.conv3(out), identity, True)


class ResNet(nn.Module):
    """mmdet's ``ResNet``: same constructor arguments and defaults, same ``state_dict`` keys as torchvision's and mmdet's (``conv1``,
    ``bn1``, ``layer{s}.{i}.conv{j}``, ``.bn{j}``, ``.downsample.0`` / ``.1``), ``forward(x) -> tuple`` of the ``out_indices`` stages.
    ``deep_stem``, ``avg_down``, ``dcn``, ``plugins``, ``with_cp=True``, ``conv_cfg`` and norm types other than ``'BN'`` raise
    ``NotImplementedError``."""

    arch_settings = {18: (BasicBlock, (2, 2, 2, 2)), 34: (BasicBlock, (3, 4, 6, 3)), 50: (Bottleneck, (3, 4, 6, 3)),
                     101: (Bottleneck, (3, 4, 23, 3)), 152: (Bottleneck, (3, 8, 36, 3))}

    def __init__(self, depth, in_channels=3, stem_channels=None, base_channels=64, num_stages=4, strides=(1, 2, 2, 2), dilations=(1, 1, 1, 1),
                 out_indices=(0, 1, 2, 3), style='pytorch', deep_stem=False, avg_down=False, frozen_stages=-1, conv_cfg=None,
                 norm_cfg=dict(type='BN', requires_grad=True), norm_eval=True, dcn=None, stage_with_dcn=(False, False, False, False),
                 plugins=None, with_cp=False, zero_init_residual=True):
        super().__init__()
        if depth not in self.arch_settings:
            raise KeyError(f'invalid depth {depth} for resnet')
        for name, value in (('deep_stem', deep_stem), ('avg_down', avg_down), ('dcn', dcn), ('plugins', plugins), ('with_cp', with_cp),
                            ('conv_cfg', conv_cfg)):
            if value:
                raise NotImplementedError(f'{type(self).__name__}: {name} is not built here (it needs mmcv / mmdet)')
        if norm_cfg.get('type') != 'BN':
            raise NotImplementedError(f'{type(self).__name__}: norm type {norm_cfg.get("type")!r}; only \'BN\' is built here')
        assert 1 <= num_stages <= 4 and len(strides) == len(dilations) == num_stages
        assert max(out_indices) < num_stages and style in ('pytorch', 'caffe')
        self.depth, self.style = depth, style
        self.stem_channels = stem_channels if stem_channels is not None else base_channels
        self.base_channels, self.num_stages, self.strides, self.dilations = base_channels, num_stages, tuple(strides), tuple(dilations)
        self.out_indices, self.frozen_stages, self.norm_cfg, self.norm_eval = tuple(out_indices), frozen_stages, dict(norm_cfg), norm_eval
        self.zero_init_residual = zero_init_residual
        self.block, stage_blocks = self.arch_settings[depth]
        self.stage_blocks = stage_blocks[:num_stages]
        self.conv1 = nn.Conv2d(in_channels, self.stem_channels, 7, stride=2, padding=3, bias=False)
        self.bn1 = _build_norm(self.norm_cfg, self.stem_channels)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        inplanes = self.stem_channels
        self.res_layers = []
        for i, blocks in enumerate(self.stage_blocks):
            planes = base_channels * 2 ** i
            name = f'layer{i + 1}'
            self.add_module(name, self._make_layer(inplanes, planes, blocks, strides[i], dilations[i]))
            inplanes = planes * self.block.expansion
            self.res_layers.append(name)
        self.feat_dim = inplanes
        self._freeze_stages()

    def _make_layer(self, inplanes, planes, blocks, stride, dilation):
        out = planes * self.block.expansion
        downsample = None
        if stride != 1 or inplanes != out:
            downsample = nn.Sequential(nn.Conv2d(inplanes, out, 1, stride=stride, bias=False), _build_norm(self.norm_cfg, out))
        layers = [self.block(inplanes, planes, stride, dilation, downsample, self.style, self.norm_cfg)]
        layers += [self.block(out, planes, 1, dilation, None, self.style, self.norm_cfg) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    def _freeze_stages(self):
        if self.frozen_stages >= 0:
            self.bn1.eval()
            for m in (self.conv1, self.bn1):
                for p in m.parameters():
                    p.requires_grad = False
        for i in range(1, min(self.frozen_stages, self.num_stages) + 1):
            m = getattr(self, f'layer{i}')
            m.eval()
            for p in m.parameters():
                p.requires_grad = False

    def init_weights(self, pretrained=None):
        """Kaiming-normal (fan_out) convolutions, norms at weight 1 and bias 0, and with ``zero_init_residual`` the last norm of every
        block at weight 0; or a LOCAL checkpoint file through ``torch.load`` (its ``state_dict`` entry when it has one).  Nothing is
        fetched: a URL raises."""
        if isinstance(pretrained, str):
            if '://' in pretrained:
                raise ValueError(f'init_weights: {pretrained!r} would have to be fetched; download the checkpoint and pass its local path')
            state = torch.load(pretrained, map_location='cpu')
            state = state.get('state_dict', state)
            self.load_state_dict(state, strict=False)
            return
        if pretrained is not None:
            raise TypeError('pretrained must be a str or None')
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        if self.zero_init_residual:
            for m in self.modules():
                if isinstance(m, (BasicBlock, Bottleneck)):
                    nn.init.constant_(m.last_norm.weight, 0)

    def forward(self, x):
        x = self.conv1(x)
        if not self.bn1.training:
            x = bn_relu_maxpool(x, self.bn1.running_mean, self.bn1.running_var, self.bn1.weight, self.bn1.bias, self.bn1.eps)
        else:
            x = self.maxpool(self.relu(self.bn1(x)))
        outs = []
        for i, name in enumerate(self.res_layers):
            x = getattr(self, name)(x)
            if i in self.out_indices:
                outs.append(x)
        return tuple(outs)

    def train(self, mode=True):
        super().train(mode)
        self._freeze_stages()
        if mode and self.norm_eval:
            for m in self.modules():
                if isinstance(m, nn.BatchNorm2d):
                    m.eval()
        return self


def register_with_mmdet(force=False):
    """Put ``ResNet`` into mmdet's ``BACKBONES`` registry; False without mmdet.  mmdet registers a ``ResNet`` of its own, so on import
    (``force=False``) a name that is taken is KEPT and a config still builds that class; ``force=True`` replaces it: call it after mmdet
    is imported and before the model is built.  Returns whether the class was registered."""
    try:
        from mmdet.models.builder import BACKBONES
    except Exception:
        return False
    if force or BACKBONES.get(ResNet.__name__) is None:
        BACKBONES.register_module(module=ResNet, force=force)
        return True
    return False


register_with_mmdet()
