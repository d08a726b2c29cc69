"""The feature pyramid (N12): mmdet's ``FPN`` and the reference's ``FPNplus`` (monorun/models/necks/fpn_plus.py), without
mmcv / mmdet.  Every shipped config builds ``FPNplus(in_channels=[256, 512, 1024, 2048], out_channels=256, num_outs=5,
num_lower_outs=1)``: its tuple of six maps (strides 2 .. 64) is what ``RPNHeadMod`` and ``SingleRoIExtractorMod`` consume.

The convolutions are torch's (MIOpen on a HIP device).  What runs between the lateral 1×1 and the output 3×3 convolutions is the op
:func:`fpn_topdown`.  ``lat[l]`` (N, C, H_l, W_l), finest first, fp32, every operation rounded on its own:

  1. ``m[L−1] = lat[L−1]``; for l = L−2 .. 0:  ``m[l][y, x] = lat[l][y, x] + m[l+1][iy(y), ix(x)]`` with
     ``iy(y) = min(int(floorf(y · (float(H_{l+1}) / float(H_l)))), H_{l+1} − 1)``: bit for bit the reference's in-place chain
     ``lat[l] += F.interpolate(lat[l+1], size=lat[l].shape[2:], mode='nearest')``;
  2. with ``lower_scale=2``, ``low`` (N, C, 2 H_0, 2 W_0): the ``align_corners=False`` bilinear ×2 up-sample of ``m[0]``,
     ``src = max((Y + 0.5) · 0.5 − 0.5, 0)``, ``i0 = int(src)``, ``i1 = i0 + (i0 < H_0 − 1)``, ``l1 = src − i0``, ``l0 = 1 − l1``,
     ``low = l0y · (l0x · a + l1x · b) + l1y · (l0x · c + l1x · d)``.  torch's own bilinear kernels differ from this expression in the last
     bit, so the expression defines the op (include/monorun_fpn.h) and torch agrees within ``8 · 2⁻²⁴ · max|m[0]|``.

Hot path: on CUDA fp32, for a pyramid inside the header's rule (``H_{l+1} ≤ H_l ≤ 2 H_{l+1}``, the same for W: every pyramid of
stride-2 convolutions), at most 6 levels and ``lower_scale`` 0 or 2, ONE fused HIP launch forward (``mr_fpn_topdown_forward``: the eager
chain is seven) and ONE backward (``mr_fpn_topdown_backward``: a gather that stores every gradient element once; no atomics, no memset,
bitwise reproducible).  Everything else — CPU, other dtypes, other pyramids, another ``lower_scale`` or ``upsample_cfg``, a backward under
``create_graph=True`` — runs :func:`fpn_topdown_torch`, the torch restatement.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib

MAX_LEVELS = 6          # MR_FPN_MAX_LEVELS of include/monorun_fpn.h


def _bilinear_taps(size, scale, device):
    """i0, i1 (int64) and l0, l1 (fp32) of the 2-tap rule along one axis of `size` pixels up-sampled by `scale`"""
    out = int(np.floor(size * float(scale)))
    rs = float(np.float32(1.0 / float(scale)))
    src = ((torch.arange(out, dtype=torch.float32, device=device) + 0.5) * rs - 0.5).clamp(min=0)
    i0 = src.to(torch.int64).clamp(max=size - 1)
    i1 = i0 + (i0 < size - 1).to(torch.int64)
    l1 = src - i0.to(torch.float32)
    return i0, i1, 1.0 - l1, l1


def bilinear_upsample_torch(m, scale=2):
    """The ``align_corners=False`` bilinear up-sample of m (N, C, H, W) by `scale` in the op's stated order (rule 2), differentiable; fp16 and
    bf16 maps are computed in fp32 and returned in their dtype."""
    work = m if m.dtype in (torch.float32, torch.float64) else m.to(torch.float32)
    i0y, i1y, l0y, l1y = _bilinear_taps(m.shape[2], scale, m.device)
    i0x, i1x, l0x, l1x = _bilinear_taps(m.shape[3], scale, m.device)
    l0y, l1y, l0x, l1x = (w.to(work.dtype) for w in (l0y[:, None], l1y[:, None], l0x, l1x))
    r0, r1 = work.index_select(2, i0y), work.index_select(2, i1y)
    top = l0x * r0.index_select(3, i0x) + l1x * r0.index_select(3, i1x)
    bottom = l0x * r1.index_select(3, i0x) + l1x * r1.index_select(3, i1x)
    return (l0y * top + l1y * bottom).to(m.dtype)


def fpn_topdown_torch(lats, lower_scale=2):
    """The op in torch ops on any device and floating dtype, differentiable: ``(m, low)`` with m the list of the L merged maps (``m[L−1]``
    is ``lats[L−1]`` itself) and low the up-sample of ``m[0]`` by ``lower_scale`` (None for 0)."""
    lats = list(lats)
    m = [None] * len(lats)
    m[-1] = lats[-1]
    for l in range(len(lats) - 2, -1, -1):
        m[l] = lats[l] + F.interpolate(m[l + 1], size=lats[l].shape[2:], mode='nearest')
    return m, (bilinear_upsample_torch(m[0], lower_scale) if lower_scale else None)


def in_pyramid_rule(sizes):
    """The header's pyramid rule on [(H_l, W_l)], finest first: every level between the finer one's size and half of it, rounded up."""
    return all(b <= a <= 2 * b for s, t in zip(sizes[:-1], sizes[1:]) for a, b in zip(s, t))


def hip_ok(lats, lower_scale=2):
    """Whether the fused HIP launches cover this call: CUDA fp32 maps of one (N, C) on one device, at most 6 levels inside the pyramid
    rule, ``lower_scale`` 0 or 2, and 32-bit offsets within every (image, level) slab, that of ``low`` included.  (A backward under
    ``create_graph=True`` is the restatement's, decided when it runs.)"""
    lats = list(lats)
    if not lats or len(lats) > MAX_LEVELS or lower_scale not in (0, 2):
        return False
    if not all(isinstance(t, torch.Tensor) and t.dim() == 4 for t in lats):
        return False
    dev, (N, C) = lats[0].device, lats[0].shape[:2]
    if dev.type != 'cuda':
        return False
    lim = 2 ** 31 - 1
    for t in lats:
        if t.device != dev or t.dtype != torch.float32 or t.shape[:2] != (N, C) or min(t.shape) < 1 or C * t.shape[2] * t.shape[3] > lim:
            return False
    if lower_scale and 4 * C * lats[0].shape[2] * lats[0].shape[3] > lim:
        return False
    return N * C <= lim and in_pyramid_rule([tuple(t.shape[2:]) for t in lats])


def _table(tensors):
    return (ctypes.c_void_p * len(tensors))(*[_lib.ptr(t) for t in tensors])


class _FPNTopDownFunction(torch.autograd.Function):
    """``mr_fpn_topdown_forward`` forward, ``mr_fpn_topdown_backward`` for the gradients to the laterals, which arrive contiguous fp32 on
    one CUDA device.  Returns ``m[0 .. L−2]`` and, with ``lower_scale=2``, ``low``; ``m[L−1]`` is the last lateral and never passes through.
    Nothing is saved: the op is linear."""

    @staticmethod
    def forward(ctx, lower_scale, *lats):
        L, dev = len(lats), lats[0].device
        N, C, H0, W0 = lats[0].shape
        merged = [torch.empty_like(t) for t in lats[:-1]]
        low = torch.empty(N, C, 2 * H0, 2 * W0, device=dev, dtype=torch.float32) if lower_scale else None
        i32 = ctypes.c_int * L
        ctx.common = dict(level_h=i32(*[t.shape[2] for t in lats]), level_w=i32(*[t.shape[3] for t in lats]), n_levels=L, n_images=N, channels=C,
                          lower_scale=int(lower_scale))
        with torch.cuda.device(dev):
            _lib.call('mr_fpn_topdown_forward', ctx.common, lat=_table(lats), merged=_table(merged + [None]), low=_lib.ptr(low),
                      stream=torch.cuda.current_stream(dev).cuda_stream)
        ctx.shapes, ctx.device = [t.shape for t in lats], dev
        ctx.set_materialize_grads(False)            # an unused output arrives as None and travels as a NULL pointer: zeros
        return tuple(merged) + ((low,) if lower_scale else ())

    @staticmethod
    def backward(ctx, *grads):
        L, dev, lower_scale = len(ctx.shapes), ctx.device, ctx.common['lower_scale']
        need = ctx.needs_input_grad[1:]
        if torch.is_grad_enabled():
            # create_graph=True: the gradients must carry a graph themselves, which the kernel cannot give.  The op is linear in the
            # laterals, so torch differentiates the restatement at zero laterals: the result depends on the arriving gradients alone.
            with torch.enable_grad():
                zeros = [torch.zeros(s, device=dev, dtype=torch.float32, requires_grad=True) for s in ctx.shapes]
                m, low = fpn_topdown_torch(zeros, lower_scale)
                outs = m[:-1] + ([low] if lower_scale else [])
                pairs = [(o, g) for o, g in zip(outs, grads) if g is not None]
                got = torch.autograd.grad([o for o, _ in pairs], zeros, [g for _, g in pairs], create_graph=True, allow_unused=True)
            return (None,) + tuple(g if n else None for g, n in zip(got, need))
        gm = [g.to(torch.float32).contiguous() if g is not None else None for g in grads[:L - 1]] + [None]
        gl = grads[L - 1].to(torch.float32).contiguous() if lower_scale and grads[L - 1] is not None else None
        out = [torch.empty(s, device=dev, dtype=torch.float32) if n else None for s, n in zip(ctx.shapes, need)]
        with torch.cuda.device(dev):
            _lib.call('mr_fpn_topdown_backward', ctx.common, grad_merged=_table(gm), grad_low=_lib.ptr(gl), grad_lat=_table(out),
                      stream=torch.cuda.current_stream(dev).cuda_stream)
        return (None,) + tuple(out)


def fpn_topdown(lats, lower_scale=2):
    """The top-down pathway: lats [(N, C, H_l, W_l)], finest first -> ``(m, low)`` as :func:`fpn_topdown_torch`, differentiable in the
    laterals.  The fused HIP launches when :func:`hip_ok`, else the restatement."""
    lats = list(lats)
    if not hip_ok(lats, lower_scale):
        return fpn_topdown_torch(lats, lower_scale)
    if len(lats) == 1 and not lower_scale:
        return [lats[0]], None
    outs = _FPNTopDownFunction.apply(int(lower_scale), *[t.contiguous() for t in lats])
    return list(outs[:len(lats) - 1]) + [lats[-1]], (outs[-1] if lower_scale else None)


class ConvModule(nn.Module):
    """What mmcv's ``ConvModule`` is with ``conv_cfg=None, norm_cfg=None, act_cfg=None``: ``conv`` with bias, under the key ``conv``."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride=stride, padding=padding)

    def forward(self, x):
        return self.conv(x)


class FPN(nn.Module):
    """mmdet's ``FPN``: same constructor arguments and defaults, same ``state_dict`` keys (``lateral_convs.{i}.conv.*``,
    ``fpn_convs.{i}.conv.*``), ``forward(inputs) -> tuple`` of ``num_outs`` maps.  ``conv_cfg``, ``norm_cfg`` and ``act_cfg`` other than
    None raise ``NotImplementedError`` (they need mmcv's builders).  The top-down pathway is :func:`fpn_topdown` when ``upsample_cfg`` is
    the default ``dict(mode='nearest')``; for any other it is the reference's plain ``F.interpolate`` chain, the bilinear map included
    (no bitwise contract applies there)."""

    def __init__(self, in_channels, out_channels, num_outs, start_level=0, end_level=-1, add_extra_convs=False, extra_convs_on_inputs=True,
                 relu_before_extra_convs=False, no_norm_on_lateral=False, conv_cfg=None, norm_cfg=None, act_cfg=None,
                 upsample_cfg=dict(mode='nearest')):
        super().__init__()
        if conv_cfg is not None or norm_cfg is not None or act_cfg is not None:
            raise NotImplementedError(f'{type(self).__name__}: conv_cfg, norm_cfg and act_cfg other than None need mmcv\'s ConvModule builders')
        assert isinstance(in_channels, list)
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.num_ins = len(in_channels)
        self.num_outs = num_outs
        self.relu_before_extra_convs = relu_before_extra_convs
        self.no_norm_on_lateral = no_norm_on_lateral
        self.fp16_enabled = False
        self.upsample_cfg = dict(upsample_cfg)
        if end_level == -1:
            self.backbone_end_level = self.num_ins
            assert num_outs >= self.num_ins - start_level
        else:                                   # no extra level beyond end_level
            self.backbone_end_level = end_level
            assert end_level <= len(in_channels)
            assert num_outs == end_level - start_level
        self.start_level = start_level
        self.end_level = end_level
        assert isinstance(add_extra_convs, (str, bool))
        if isinstance(add_extra_convs, str):
            assert add_extra_convs in ('on_input', 'on_lateral', 'on_output')
        elif add_extra_convs:                   # True: the older flag decides
            add_extra_convs = 'on_input' if extra_convs_on_inputs else 'on_output'
        self.add_extra_convs = add_extra_convs
        self.lateral_convs = nn.ModuleList()
        self.fpn_convs = nn.ModuleList()
        for i in range(self.start_level, self.backbone_end_level):
            self.lateral_convs.append(ConvModule(in_channels[i], out_channels, 1))
            self.fpn_convs.append(ConvModule(out_channels, out_channels, 3, padding=1))
        extra_levels = num_outs - self.backbone_end_level + self.start_level
        if self.add_extra_convs and extra_levels >= 1:
            for i in range(extra_levels):
                first = i == 0 and self.add_extra_convs == 'on_input'
                self.fpn_convs.append(ConvModule(self.in_channels[self.backbone_end_level - 1] if first else out_channels, out_channels, 3,
                                                 stride=2, padding=1))

    def init_weights(self):
        """mmdet's: Xavier-uniform weights and zero biases on every convolution."""
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.xavier_uniform_(m.weight, gain=1)
                nn.init.constant_(m.bias, 0)

    def _laterals(self, inputs):
        assert len(inputs) == len(self.in_channels)
        if self.fp16_enabled:                   # mmdet's auto_fp16: the inputs go to half when the wrapper has enabled it
            inputs = [x.half() if x.is_floating_point() else x for x in inputs]
        return inputs, [conv(inputs[i + self.start_level]) for i, conv in enumerate(self.lateral_convs)]

    def _top_down(self, laterals, lower_scale):
        """the merged laterals and the map up-sampled by `lower_scale` (None for 0)"""
        if self.upsample_cfg == dict(mode='nearest'):
            return fpn_topdown(laterals, lower_scale)
        m = list(laterals)
        for i in range(len(m) - 1, 0, -1):
            if 'scale_factor' in self.upsample_cfg:
                m[i - 1] = m[i - 1] + F.interpolate(m[i], **self.upsample_cfg)
            else:
                m[i - 1] = m[i - 1] + F.interpolate(m[i], size=m[i - 1].shape[2:], **self.upsample_cfg)
        return m, (F.interpolate(m[0], scale_factor=lower_scale, mode='bilinear', align_corners=False) if lower_scale else None)

    def _outputs(self, inputs, laterals):
        used = len(laterals)
        outs = [self.fpn_convs[i](laterals[i]) for i in range(used)]
        if self.num_outs > len(outs):
            if not self.add_extra_convs:        # max pooling on top of the outputs (Faster R-CNN, Mask R-CNN)
                for i in range(self.num_outs - used):
                    outs.append(F.max_pool2d(outs[-1], 1, stride=2))
            else:                               # convolutions on top of the original maps (RetinaNet)
                if self.add_extra_convs == 'on_input':
                    extra_source = inputs[self.backbone_end_level - 1]
                elif self.add_extra_convs == 'on_lateral':
                    extra_source = laterals[-1]
                else:
                    extra_source = outs[-1]
                outs.append(self.fpn_convs[used](extra_source))
                for i in range(used + 1, self.num_outs):
                    outs.append(self.fpn_convs[i](F.relu(outs[-1]) if self.relu_before_extra_convs else outs[-1]))
        return outs

    def forward(self, inputs):
        inputs, laterals = self._laterals(inputs)
        merged, _ = self._top_down(laterals, 0)
        return tuple(self._outputs(inputs, merged))


class FPNplus(FPN):
    """The reference's neck: ``FPN`` with ``num_lower_outs`` maps below the finest level, each a 3×3 convolution
    (``lower_fpn_convs.{i}.conv.*``) of the merged finest lateral up-sampled bilinearly by ``2^(num_lower_outs − i)``.  ``forward`` returns
    the lower outputs first (finest first), then the pyramid, then the extra levels.  The ×2 map comes out of the fused launch; with
    ``num_lower_outs ≥ 2`` the finer ones are ``F.interpolate``'s."""

    def __init__(self, in_channels, out_channels, num_outs, num_lower_outs=1, start_level=0, end_level=-1, add_extra_convs=False,
                 extra_convs_on_inputs=True, relu_before_extra_convs=False, no_norm_on_lateral=False, conv_cfg=None, norm_cfg=None,
                 act_cfg=None, upsample_cfg=dict(mode='nearest')):
        super().__init__(in_channels, out_channels, num_outs, start_level, end_level, add_extra_convs, extra_convs_on_inputs,
                         relu_before_extra_convs, no_norm_on_lateral, conv_cfg, norm_cfg, act_cfg, upsample_cfg)
        self.num_lower_outs = num_lower_outs
        self.lower_fpn_convs = nn.ModuleList([ConvModule(out_channels, out_channels, 3, padding=1) for _ in range(num_lower_outs)])

    def forward(self, inputs):
        inputs, laterals = self._laterals(inputs)
        n = self.num_lower_outs
        merged, low = self._top_down(laterals, 2 if n else 0)
        lower = [F.interpolate(merged[0], scale_factor=2 ** (n - i), mode='bilinear', align_corners=False) for i in range(n - 1)]
        if n:
            lower.append(low)
        outs_lower = [conv(x) for conv, x in zip(self.lower_fpn_convs, lower)]
        return tuple(outs_lower + self._outputs(inputs, merged))


def register_with_mmdet(force=False):
    """Put the two necks into mmdet's ``NECKS`` registry; False without mmdet.  mmdet registers an ``FPN`` of its own and the reference an
    ``FPNplus``, so on import (``force=False``) a name that is taken is KEPT and a config still builds that class.  ``force=True`` replaces
    them: call it after mmdet and the reference's ``monorun`` package are imported and before the model is built, and
    ``neck=dict(type='FPNplus', ...)`` of a config builds the class of this module.  Returns whether a class was registered."""
    try:
        from mmdet.models.builder import NECKS
    except Exception:
        return False
    done = False
    for cls in (FPN, FPNplus):
        if force or NECKS.get(cls.__name__) is None:
            NECKS.register_module(module=cls, force=force)
            done = True
    return done


register_with_mmdet()
