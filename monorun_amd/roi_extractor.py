"""The RoI feature extractors (N11): mmdet's ``SingleRoIExtractor`` and the reference's ``SingleRoIExtractorMod``
(monorun/models/roi_heads/roi_extractors/single_level_roi_extractor.py) over ``mmcv.ops.RoIAlign`` (average pooling), without mmcv, whose
op is a CUDA extension with no ROCm build.  ``MonoRUnRoIHead`` builds two of them, ``bbox_roi_extractor`` (7×7) and ``noc_roi_extractor``
(14×14): every head of the RoI head consumes their output.

The op.  ``feats[l]`` (N, C, H_l, W_l), ``rois`` (K, 5) = [image, x1, y1, x2, y2], strides, ``finest_scale``, output (oh, ow) ->
(K, C, oh, ow):

  1. the level of a RoI: ``v = sqrt((x2 − x1)(y2 − y1)) / finest_scale + 1e−6`` in fp32, level = #{i in 1..L−1 : v ≥ 2^i} (a NaN ``v``:
     level 0).  mmdet's ``floor(log2(v)).clamp(0, L − 1)`` wherever the rounded ``log2`` does not cross an integer: comparing with exact
     powers of two, the level never depends on whose ``log2`` ran;
  2. RoIAlign of ``feats[level][image]`` at ``spatial_scale = 1 / stride``: the arithmetic of ``mr_roi_align_avg`` operation for operation;
  3. a DEGENERATE RoI — a coordinate or image index that is not finite, an image outside [0, N), or at ``sampling_ratio=0`` a sample grid
     ``ceil(roi_h / oh) > H_l + 2`` or ``ceil(roi_w / ow) > W_l + 2`` — gives zeros and no gradient: the one deliberate deviation from
     mmcv, whose sample loops such a RoI leaves unbounded;
  4. the gradient goes to ``feats`` only; levels and images no RoI touches get exact zeros (mmdet's ``feats[i].sum() * 0``).

Hot path: :func:`roi_extract` on CUDA fp32 runs ONE fused HIP launch forward (``mr_roi_extract_forward``: all levels, the level rule in
the kernel, no host synchronisation — mmdet's wrapper runs per level a mask, a blocking ``nonzero``, an index, a launch and an
``index_put``) and ONE backward (``mr_roi_extract_backward``: a gather that stores every gradient element once; no atomics, no memset,
bitwise reproducible).  Everything else — CPU, other dtypes, more than 8 levels, outputs above 32, a backward under
``create_graph=True`` — runs :func:`roi_extract_torch`, the torch restatement.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .noc_targets import roi_align_avg_torch

MAX_LEVELS = 8          # MR_ROI_MAX_LEVELS of include/monorun_roi.h
MAX_OUT = 32            # MR_ROI_MAX_OUT


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else tuple(int(x) for x in v)


def map_roi_levels(rois, num_levels, finest_scale=56):
    """The level of each RoI (K,) int64: rule 1 of the module's text, in fp32 torch ops on the RoIs' device."""
    r = rois.detach().to(torch.float32)
    v = torch.sqrt((r[:, 3] - r[:, 1]) * (r[:, 4] - r[:, 2])) / r.new_tensor(float(finest_scale)) + r.new_tensor(1e-6)
    levels = torch.zeros(r.shape[0], dtype=torch.int64, device=r.device)
    for i in range(1, int(num_levels)):
        levels += (v >= float(2 ** i)).to(torch.int64)
    return levels


def roi_rescale(rois, scale_factor):
    """mmdet's ``BaseRoIExtractor.roi_rescale``: the RoIs about their centres, width and height multiplied by ``scale_factor``."""
    cx = (rois[:, 1] + rois[:, 3]) * 0.5
    cy = (rois[:, 2] + rois[:, 4]) * 0.5
    w = (rois[:, 3] - rois[:, 1]) * scale_factor
    h = (rois[:, 4] - rois[:, 2]) * scale_factor
    return torch.stack((rois[:, 0], cx - w * 0.5, cy - h * 0.5, cx + w * 0.5, cy + h * 0.5), dim=-1)


def _roi_sizes(r32, scale, aligned):
    """roi_w, roi_h of RoIs (K, 5) fp32 numpy on a map of the given spatial scale (per RoI), as the kernels round them."""
    f32 = np.float32
    off = f32(0.5 if aligned else 0.0)
    with np.errstate(all='ignore'):
        rw = (r32[:, 3] * scale - off) - (r32[:, 1] * scale - off)
        rh = (r32[:, 4] * scale - off) - (r32[:, 2] * scale - off)
    if not aligned:
        rw, rh = np.maximum(rw, f32(1.0)), np.maximum(rh, f32(1.0))
    return rw.astype(f32), rh.astype(f32)


def valid_rois(rois, levels, level_sizes, featmap_strides, num_images, output_size, sampling_ratio=0, aligned=True):
    """(K,) bool numpy: the RoIs that are NOT degenerate (rule 3), decided in fp32 as the kernels decide it.  rois (K, 5) and levels (K,)
    as arrays or tensors; level_sizes [(H_l, W_l)]."""
    f32 = np.float32
    oh, ow = _pair(output_size)
    r32 = np.asarray(rois.detach().cpu() if isinstance(rois, torch.Tensor) else rois, dtype=f32).reshape(-1, 5)
    lv = np.asarray(levels.cpu() if isinstance(levels, torch.Tensor) else levels, dtype=np.int64)
    ok = np.isfinite(r32).all(axis=1)
    with np.errstate(all='ignore'):
        ok &= (r32[:, 0] > f32(-1.0)) & (r32[:, 0] < f32(num_images))
        if int(sampling_ratio) <= 0 and r32.shape[0]:
            scale = (f32(1.0) / np.asarray(featmap_strides, dtype=f32))[lv]
            rw, rh = _roi_sizes(r32, scale, aligned)
            hs = np.asarray([s[0] for s in level_sizes], dtype=np.int64)[lv]
            ws = np.asarray([s[1] for s in level_sizes], dtype=np.int64)[lv]
            ok &= ~(np.ceil(rh / f32(oh)) > (hs + 2).astype(f32)) & ~(np.ceil(rw / f32(ow)) > (ws + 2).astype(f32))
    return ok


def _roi_align_avg_general(inp, rois, output_size, sampling_ratio, aligned):
    """:func:`monorun_amd.noc_targets.roi_align_avg_torch` for the other ``sampling_ratio`` / ``aligned`` values (RoIs already on the
    map's scale): the same arithmetic, differentiable in ``inp``."""
    oh, ow = _pair(output_size)
    inp = inp.to(torch.float32)
    N, C, H, W = inp.shape
    f = dict(dtype=torch.float32, device=inp.device)
    f32 = np.float32
    r32 = rois.detach().to(torch.float32).cpu().numpy()
    ph = torch.arange(oh, **f)[:, None]
    pw = torch.arange(ow, **f)[None, :]
    off = f32(0.5 if aligned else 0.0)
    rows = []
    for k in range(r32.shape[0]):
        sw, sh = f32(r32[k, 1] - off), f32(r32[k, 2] - off)
        rw, rh = f32(f32(r32[k, 3] - off) - sw), f32(f32(r32[k, 4] - off) - sh)
        if not aligned:
            rw, rh = max(rw, f32(1.0)), max(rh, f32(1.0))
        bh, bw = f32(rh / f32(oh)), f32(rw / f32(ow))
        gh = int(sampling_ratio) if sampling_ratio > 0 else int(np.ceil(bh))
        gw = int(sampling_ratio) if sampling_ratio > 0 else int(np.ceil(bw))
        count = float(max(gh * gw, 1))
        m = inp[int(r32[k, 0])]
        acc = torch.zeros(C, oh, ow, **f)
        ybase = float(sh) + ph * float(bh)
        xbase = float(sw) + pw * float(bw)
        for iy in range(gh):
            y = (ybase + float(f32(f32(f32(f32(iy) + f32(0.5)) * bh) / f32(gh)))).expand(oh, ow)
            for ix in range(gw):
                x = (xbase + float(f32(f32(f32(f32(ix) + f32(0.5)) * bw) / f32(gw)))).expand(oh, ow)
                dead = (y < -1.0) | (y > H) | (x < -1.0) | (x > W)
                yy = torch.where((y <= 0) | dead, torch.zeros_like(y), y)       # a dead sample is not converted: it may be huge
                xx = torch.where((x <= 0) | dead, torch.zeros_like(x), x)
                yl, xl = yy.to(torch.int64), xx.to(torch.int64)
                top, right = yl >= H - 1, xl >= W - 1
                yl = torch.where(top, torch.full_like(yl, H - 1), yl)
                xl = torch.where(right, torch.full_like(xl, W - 1), xl)
                yh = torch.where(top, yl, yl + 1)
                xh = torch.where(right, xl, xl + 1)
                yy = torch.where(top, yl.to(torch.float32), yy)
                xx = torch.where(right, xl.to(torch.float32), xx)
                ly, lx = yy - yl.to(torch.float32), xx - xl.to(torch.float32)
                hy, hx = 1.0 - ly, 1.0 - lx
                val = (hy * hx) * m[:, yl, xl] + (hy * lx) * m[:, yl, xh] + (ly * hx) * m[:, yh, xl] + (ly * lx) * m[:, yh, xh]
                acc = acc + torch.where(dead, torch.zeros_like(val), val)
        rows.append(acc / count)
    return torch.stack(rows) if rows else torch.zeros(0, C, oh, ow, **f)


def roi_extract_torch(feats, rois, featmap_strides, finest_scale, output_size, sampling_ratio=0, aligned=True, level_rois=None):
    """The op in torch ops on any device and floating dtype (computed in fp32, returned in ``feats[0]``'s dtype), differentiable in
    ``feats``: the level rule, per level one RoIAlign of its RoIs multiplied by ``1 / stride`` (exact for power-of-two strides) and an
    ``index_copy``.  Degenerate RoIs give zeros; a level without RoIs joins the graph with an exact zero.  ``level_rois``: the boxes the
    level rule reads when they are not the pooled ones (``roi_scale_factor``)."""
    oh, ow = _pair(output_size)
    feats = list(feats)
    L, (N, C) = len(feats), feats[0].shape[:2]
    K = rois.shape[0]
    out = torch.zeros(K, C, oh, ow, dtype=torch.float32, device=feats[0].device)
    levels = map_roi_levels(rois if level_rois is None else level_rois, L, finest_scale)
    ok = valid_rois(rois, levels, [f.shape[-2:] for f in feats], featmap_strides, N, (oh, ow), sampling_ratio, aligned)
    ok = torch.from_numpy(ok).to(levels.device)
    r32 = rois.detach().to(torch.float32)
    for l, (f, stride) in enumerate(zip(feats, featmap_strides)):
        idx = torch.nonzero((levels == l) & ok, as_tuple=False).flatten()
        if idx.numel() == 0:
            out = out + f[:0].to(torch.float32).sum()           # an exact zero that carries the level's (zero) gradient
            continue
        r = r32[idx].clone()
        r[:, 1:] = r[:, 1:] * float(np.float32(1.0) / np.float32(stride))
        if int(sampling_ratio) == 0 and aligned:
            pooled = roi_align_avg_torch(f, r, (oh, ow))
        else:
            pooled = _roi_align_avg_general(f, r, (oh, ow), int(sampling_ratio), bool(aligned))
        out = out.index_copy(0, idx.to(out.device), pooled)
    return out.to(feats[0].dtype)


def hip_ok(feats, rois, output_size):
    """Whether the fused HIP launches cover this call: CUDA fp32 tensors on one device, at most 8 levels of one (N, C), an output of at
    most 32 x 32, and 32-bit offsets within every (image, level) slab and within the output.  (A backward under ``create_graph=True`` is
    the restatement's, decided when it runs.)"""
    feats = list(feats)
    oh, ow = _pair(output_size)
    if not feats or len(feats) > MAX_LEVELS or not (1 <= oh <= MAX_OUT and 1 <= ow <= MAX_OUT):
        return False
    if not isinstance(rois, torch.Tensor) or rois.dim() != 2 or rois.shape[1] != 5:
        return False
    dev = feats[0].device
    if dev.type != 'cuda' or rois.device != dev or rois.dtype != torch.float32:
        return False
    if feats[0].dim() != 4:
        return False
    N, C = feats[0].shape[:2]
    lim = 2 ** 31 - 1
    for f in feats:
        if f.dim() != 4 or f.device != dev or f.dtype != torch.float32 or f.shape[:2] != (N, C) or min(f.shape) < 1:
            return False
        if C * f.shape[2] * f.shape[3] > lim:
            return False
    return rois.shape[0] * C * oh * ow <= lim


def _level_args(maps, strides):
    L = len(maps)
    i32 = ctypes.c_int * L
    return dict(level_h=i32(*[m.shape[2] for m in maps]), level_w=i32(*[m.shape[3] for m in maps]), level_stride=i32(*[int(s) for s in strides]),
                n_levels=L, n_images=maps[0].shape[0], channels=maps[0].shape[1])


class _RoIExtractFunction(torch.autograd.Function):
    """``mr_roi_extract_forward`` forward, ``mr_roi_extract_backward`` for the gradients to the maps; the maps and the RoIs arrive
    contiguous fp32 on one CUDA device.  Only the RoIs are saved: the op is linear in the maps."""

    @staticmethod
    def forward(ctx, rois, level_rois, cfg, *feats):
        strides, finest_scale, (oh, ow), sampling_ratio, aligned = cfg
        K, C, dev = rois.shape[0], feats[0].shape[1], rois.device
        out = torch.empty(K, C, oh, ow, device=dev, dtype=torch.float32)
        common = dict(finest_scale=float(finest_scale), out_h=oh, out_w=ow, sampling_ratio=int(sampling_ratio), aligned=int(bool(aligned)),
                      rois=rois.data_ptr(), level_rois=_lib.ptr(level_rois), n_rois=K)
        with torch.cuda.device(dev):
            _lib.call('mr_roi_extract_forward', common, feats=(ctypes.c_void_p * len(feats))(*[f.data_ptr() for f in feats]),
                      out=out.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream, **_level_args(feats, strides))
        ctx.save_for_backward(rois, level_rois)          # level_rois may be None
        ctx.cfg, ctx.common, ctx.shapes = cfg, common, [f.shape for f in feats]
        return out

    @staticmethod
    def backward(ctx, grad_out):
        rois, level_rois = ctx.saved_tensors
        strides, finest_scale, size, sampling_ratio, aligned = ctx.cfg
        need = ctx.needs_input_grad[3:]
        dev = rois.device
        if torch.is_grad_enabled():
            # create_graph=True: the gradients must carry a graph themselves, which the kernel cannot give.  The op is linear in the maps,
            # so torch differentiates the restatement at zero maps: the result depends on grad_out alone.
            with torch.enable_grad():
                zeros = [torch.zeros(s, device=dev, dtype=torch.float32, requires_grad=True) for s in ctx.shapes]
                got = torch.autograd.grad(roi_extract_torch(zeros, rois, strides, finest_scale, size, sampling_ratio, aligned, level_rois),
                                          zeros, grad_out, create_graph=True)
            return (None, None, None) + tuple(g if n else None for g, n in zip(got, need))
        go = grad_out.to(torch.float32).contiguous()
        grads = [torch.empty(s, device=dev, dtype=torch.float32) for s in ctx.shapes]
        with torch.cuda.device(dev):
            _lib.call('mr_roi_extract_backward', ctx.common, grad_out=go.data_ptr(),
                      grad_feats=(ctypes.c_void_p * len(grads))(*[g.data_ptr() for g in grads]),
                      stream=torch.cuda.current_stream(dev).cuda_stream, **_level_args(grads, strides))
        return (None, None, None) + tuple(g if n else None for g, n in zip(grads, need))


def roi_extract(feats, rois, featmap_strides, finest_scale, output_size, sampling_ratio=0, aligned=True, level_rois=None):
    """The multi-level extraction: feats [(N, C, H_l, W_l)], rois (K, 5) -> (K, C, oh, ow), differentiable in ``feats``.  The fused HIP
    launches when :func:`hip_ok`, else :func:`roi_extract_torch`.  No RoIs: an empty tensor, no launch.  ``level_rois`` (K, 5): the
    boxes the level rule reads when they are not ``rois`` (mmdet's ``roi_scale_factor`` rescales the RoIs after the rule)."""
    feats = list(feats)
    size = _pair(output_size)
    assert len(feats) == len(featmap_strides), 'roi_extract: one stride per feature map'
    assert int(sampling_ratio) >= 0, 'roi_extract: sampling_ratio >= 0'
    if rois.shape[0] == 0:
        return feats[0].new_zeros((0, feats[0].shape[1]) + size)
    if level_rois is not None:
        assert level_rois.shape == rois.shape, 'roi_extract: level_rois has the shape of rois'
        level_rois = level_rois.detach().to(device=rois.device, dtype=rois.dtype).contiguous()
    if not hip_ok(feats, rois, size):
        return roi_extract_torch(feats, rois, featmap_strides, finest_scale, size, sampling_ratio, aligned, level_rois)
    cfg = (tuple(int(s) for s in featmap_strides), float(finest_scale), size, int(sampling_ratio), bool(aligned))
    return _RoIExtractFunction.apply(rois.detach().contiguous(), level_rois, cfg, *[f.contiguous() for f in feats])


class RoIAlign(nn.Module):
    """mmcv's ``RoIAlign`` layer with ``pool_mode='avg'``: same constructor arguments.  ``forward``: input (N, C, H, W), rois (K, 5) ->
    (K, C, oh, ow); the single-level case of :func:`roi_extract` when ``1 / spatial_scale`` is an integer stride."""

    def __init__(self, output_size, spatial_scale=1.0, sampling_ratio=0, pool_mode='avg', aligned=True, use_torchvision=False):
        super().__init__()
        assert pool_mode == 'avg', "RoIAlign: pool_mode='max' is not provided"
        self.output_size = _pair(output_size)
        self.spatial_scale = float(spatial_scale)
        self.sampling_ratio = int(sampling_ratio)
        self.pool_mode = pool_mode
        self.aligned = bool(aligned)
        self.use_torchvision = use_torchvision

    def forward(self, input, rois):
        stride = 1.0 / self.spatial_scale
        if stride >= 1.0 and float(round(stride)) == stride:
            return roi_extract([input], rois, [int(round(stride))], 56, self.output_size, self.sampling_ratio, self.aligned)
        r = rois.detach().to(torch.float32).clone()         # another scale: the restatement on the RoIs brought to the map's scale
        r[:, 1:] = r[:, 1:] * self.spatial_scale
        return roi_extract_torch([input], r, [1], 56, self.output_size, self.sampling_ratio, self.aligned)

    def __repr__(self):
        return (f'{self.__class__.__name__}(output_size={self.output_size}, spatial_scale={self.spatial_scale}, '
                f'sampling_ratio={self.sampling_ratio}, pool_mode={self.pool_mode}, aligned={self.aligned})')


class SingleRoIExtractor(nn.Module):
    """mmdet's ``SingleRoIExtractor``: same constructor arguments (``roi_layer`` = dict(type='RoIAlign', output_size=...,
    sampling_ratio=...)), ``num_inputs`` and ``forward(feats, rois, roi_scale_factor=None)``.  It has no parameters."""

    def __init__(self, roi_layer, out_channels, featmap_strides, finest_scale=56):
        super().__init__()
        cfg = dict(roi_layer)
        layer_type = cfg.pop('type', 'RoIAlign')
        assert layer_type == 'RoIAlign', f'SingleRoIExtractor: roi_layer type {layer_type!r} is not provided (RoIAlign only)'
        self.roi_layers = nn.ModuleList([RoIAlign(spatial_scale=1.0 / s, **cfg) for s in featmap_strides])
        self.out_channels = out_channels
        self.featmap_strides = list(featmap_strides)
        self.finest_scale = finest_scale
        self.fp16_enabled = False

    @property
    def num_inputs(self):
        """The number of feature maps ``forward`` takes."""
        return len(self.featmap_strides)

    def init_weights(self):
        pass

    def map_roi_levels(self, rois, num_levels):
        return map_roi_levels(rois, num_levels, self.finest_scale)

    def roi_rescale(self, rois, scale_factor):
        return roi_rescale(rois, scale_factor)

    def forward(self, feats, rois, roi_scale_factor=None):
        """feats: the maps, finest first; rois (K, 5) -> (K, out_channels, oh, ow) in the maps' dtype (maps that are not fp32 are pooled
        in fp32 by the restatement: mmdet's ``force_fp32(apply_to=('feats',), out_fp16=True)``)."""
        layer = self.roi_layers[0]
        feats = list(feats)
        level_rois = None
        if roi_scale_factor is not None:            # mmdet: the level from the RoIs as given, the pooling from the rescaled ones
            level_rois, rois = rois, roi_rescale(rois, roi_scale_factor)
        return roi_extract(feats, rois, self.featmap_strides[:len(feats)], self.finest_scale, layer.output_size, layer.sampling_ratio,
                           layer.aligned, level_rois=level_rois)


class SingleRoIExtractorMod(SingleRoIExtractor):
    """The reference's extractor: ``SingleRoIExtractor`` on ``feats[starting_level:]`` (its FPN hands over one finer map than the
    extractors use)."""

    def __init__(self, roi_layer, out_channels, featmap_strides, finest_scale=56, starting_level=0):
        super().__init__(roi_layer, out_channels, featmap_strides, finest_scale=finest_scale)
        self.starting_level = starting_level

    def forward(self, feats, rois, roi_scale_factor=None):
        return super().forward(list(feats)[self.starting_level:], rois, roi_scale_factor=roi_scale_factor)


def register_with_mmdet(force=False):
    """Put the two extractors into mmdet's ``ROI_EXTRACTORS`` registry; False without mmdet.  mmdet registers a ``SingleRoIExtractor`` of
    its own and the reference a ``SingleRoIExtractorMod``, both over mmcv's op, so on import (``force=False``) a name that is taken is
    KEPT and a config still builds that class.  ``force=True`` replaces them: call it after mmdet and the reference's ``monorun`` package
    are imported and before the model is built, and ``type='SingleRoIExtractorMod'`` of a config builds the class of this module.
    Returns whether a class was registered."""
    try:
        from mmdet.models.builder import ROI_EXTRACTORS
    except Exception:
        return False
    done = False
    for cls in (SingleRoIExtractor, SingleRoIExtractorMod):
        if force or ROI_EXTRACTORS.get(cls.__name__) is None:
            ROI_EXTRACTORS.register_module(module=cls, force=force)
            done = True
    return done


register_with_mmdet()
