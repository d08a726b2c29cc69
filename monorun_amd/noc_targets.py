"""The NOC head's dense targets (N9): what ``FCNNOCDecoder.get_targets`` of the reference computes for its LiDAR-supervised
configs (monorun/models/roi_heads/bbox_3d_heads/dense_decoders/fcn_noc_decoder.py:269-286):

  * ``NOCCoder.encode`` (core/bbox_3d/coord_coder/noc_coder.py:17-48): :func:`noc_encode`,
  * ``masked_dense_target`` (core/bbox_3d/masked_dense_target.py): :func:`masked_dense_target`, the composed path over already-encoded
    maps (RoIAlign by ``mr_roi_align_avg`` on the GPU, by :func:`roi_align_avg_torch` elsewhere),
  * both fused: :func:`noc_targets`, two HIP launches (``mr_noc_dense_target``) that read the raw maps only under the positive RoIs.

The fused and the composed path give the same bits: every operation is an IEEE fp32 ``+ - * /`` in the same order, and bilinear sampling
reads the encoded map at integer pixels only.  The mean of the 0/1 weights is taken as a true division ``sum / numel`` on every device
(what ``torch.mean`` computes on the CPU; its GPU kernel multiplies by ``1 / numel`` instead, which may differ in the last bit).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .pose_head import NOC_MEANS, NOC_STDS, _const, roi_align_avg

MAX_IMAGES = 32            # MR_NOC_TARGET_MAX_IMAGES of include/monorun_targets.h


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else tuple(int(x) for x in v)


def noc_encode(gt_coords_3d, gt_coords_3d_mask, dimensions, flip, target_means=NOC_MEANS, target_stds=NOC_STDS, eps=1e-5):
    """The NOC coder's encode of one image.  gt_coords_3d (G, 3, H, W): object coordinates already multiplied by the mask;
    gt_coords_3d_mask (G, 1, H, W); dimensions (G, 3) [l, h, w]; flip: the image is mirrored.  Returns the normalised part coordinates
    times the kept mask (G, 3, H, W) and the kept mask (G, 1, H, W): the mask with every pixel below eps set to 0.

    Per pixel, each step one rounding (the order the kernel follows): coordinate / max(mask, eps) / max(dimension, eps), the z part
    negated in a mirrored image, minus the mean, divided by the std, times the kept mask."""
    kept = torch.where(gt_coords_3d_mask >= eps, gt_coords_3d_mask, torch.zeros_like(gt_coords_3d_mask))
    extent = dimensions.clamp(min=eps)[:, :, None, None]
    part = gt_coords_3d / gt_coords_3d_mask.clamp(min=eps) / extent
    if flip:
        part = part * part.new_tensor((1.0, 1.0, -1.0))[:, None, None]          # a sign change: exact
    shift = part.new_tensor(target_means)[:, None, None]
    scale = part.new_tensor(target_stds)[:, None, None]
    return (part - shift) / scale * kept, kept


def roi_align_avg_torch(inp, rois, output_size):
    """``mmcv.ops.roi_align(inp, rois, output_size, 1.0, 0, 'avg', True)`` forward in torch ops, on any device: the arithmetic of
    ``mr_roi_align_avg`` operation for operation (fp32; a sample more than a pixel outside contributes 0, else it is clamped into the map).
    inp (N, C, H, W), rois (K, 5) [batch index, x1, y1, x2, y2] -> (K, C, oh, ow).  One small loop per RoI and tap: for the CPU path."""
    oh, ow = _pair(output_size)
    inp = inp.to(torch.float32)
    N, C, H, W = inp.shape
    f = dict(dtype=torch.float32, device=inp.device)
    out = torch.zeros(rois.shape[0], C, oh, ow, **f)
    ph = torch.arange(oh, **f)[:, None]
    pw = torch.arange(ow, **f)[None, :]
    r32 = rois.detach().to(torch.float32).cpu().numpy()
    f32 = np.float32
    for k in range(r32.shape[0]):
        bi = int(r32[k, 0])
        sw, sh = f32(r32[k, 1] - f32(0.5)), f32(r32[k, 2] - f32(0.5))
        rw, rh = f32(f32(r32[k, 3] - f32(0.5)) - sw), f32(f32(r32[k, 4] - f32(0.5)) - sh)
        bh, bw = f32(rh / f32(oh)), f32(rw / f32(ow))
        if not (np.isfinite(bh) and np.isfinite(bw)):
            raise ValueError('roi_align_avg_torch: a RoI coordinate is not finite')
        gh, gw = int(np.ceil(bh)), int(np.ceil(bw))
        count = float(max(gh * gw, 1))
        m = inp[bi]
        acc = torch.zeros(C, oh, ow, **f)
        ybase = float(sh) + ph * float(bh)
        xbase = float(sw) + pw * float(bw)
        for iy in range(gh):
            y = (ybase + float(f32(f32(f32(f32(iy) + f32(0.5)) * bh) / f32(gh)))).expand(oh, ow)
            for ix in range(gw):
                x = (xbase + float(f32(f32(f32(f32(ix) + f32(0.5)) * bw) / f32(gw)))).expand(oh, ow)
                dead = (y < -1.0) | (y > H) | (x < -1.0) | (x > W)
                yy = torch.where(y <= 0, torch.zeros_like(y), y)
                xx = torch.where(x <= 0, torch.zeros_like(x), x)
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
        out[k] = acc / count
    return out


def _roi_align(inp, rois, dense_size):
    if inp.device.type == 'cuda':
        return roi_align_avg(inp, rois, dense_size, 1.0, 0, True)
    return roi_align_avg_torch(inp, rois, dense_size)


def _dense_size(cfg):
    return _pair(cfg['dense_size'] if isinstance(cfg, dict) else cfg.dense_size)


def _image_targets(boxes, gt_inds, encoded, kept_mask, size, eps):
    """One image's share of :func:`masked_dense_target`: the boxes clipped to the map, the three encoded planes and the mask pooled as
    four channels of ONE RoIAlign (per channel the arithmetic of pooling them apart), the mask divided out where it is above eps."""
    if boxes.shape[0] == 0:
        return boxes.new_zeros((0, 3) + size), boxes.new_zeros((0, 1) + size)
    H, W = encoded.shape[-2:]
    inside = torch.minimum(boxes.clamp(min=0), boxes.new_tensor((W, H, W, H)))       # [0, W] x [0, H]: the map's size, not size - 1
    rois = torch.cat([gt_inds.to(boxes.dtype)[:, None], inside], dim=1)
    pooled = _roi_align(torch.cat([encoded, kept_mask], dim=1), rois, size).to(boxes.dtype)
    value, density = pooled[:, :3], pooled[:, 3:]
    seen = density > eps
    return torch.where(seen, value / density, value), seen.to(value.dtype)


def masked_dense_target(pos_proposals_list, pos_assigned_gt_inds_list, gt_dense_list, gt_mask_list, cfg, eps=1e-4):
    """The reference's function of this name, composed of the project's pieces: per image the positive proposals (n_j, 4), their
    ground-truth indices (n_j,), the ENCODED dense maps (G_j, 3, H_j, W_j) and masks (G_j, 1, H_j, W_j); cfg with ``dense_size``.  Returns
    (targets (n, 3, h, w), weights (n, 1, h, w)): the 0/1 weights divided by their mean over the batch (at least eps)."""
    size = _dense_size(cfg)
    per_image = [_image_targets(b, g, e, m, size, eps)
                 for b, g, e, m in zip(pos_proposals_list, pos_assigned_gt_inds_list, gt_dense_list, gt_mask_list)]
    targets = torch.cat([t for t, _ in per_image])
    seen = torch.cat([w for _, w in per_image])
    if seen.numel() == 0:
        return targets, seen
    # the mean as torch.mean forms it on the CPU: the sum (exact for fewer than 2^24 ones, in any order) divided by the count.  The
    # divisor is a tensor: on the GPU torch divides by a Python scalar as a multiplication by its reciprocal, which may differ in the last bit
    share = seen.sum() / seen.new_full((), seen.numel())
    return targets, seen / share.clamp(min=eps)


def _coder_consts(coord_coder):
    if coord_coder is None:
        return NOC_MEANS, NOC_STDS, 1e-5
    return coord_coder.target_means, coord_coder.target_stds, coord_coder.eps


def noc_targets_composed(pos_bboxes_list, pos_assigned_gt_inds_list, gt_coords_3d, gt_coords_3d_mask, dimensions_list, flips, dense_size,
                         coord_coder=None, eps=1e-4):
    """:func:`noc_targets` as the reference composes it: encode every ground truth's whole map, then :func:`masked_dense_target`."""
    means, stds, eps_c = _coder_consts(coord_coder)
    enc = [noc_encode(c, m, d, bool(f), means, stds, eps_c) for c, m, d, f in zip(gt_coords_3d, gt_coords_3d_mask, dimensions_list, flips)]
    t, w = masked_dense_target(pos_bboxes_list, pos_assigned_gt_inds_list, [e[0] for e in enc], [e[1] for e in enc],
                               dict(dense_size=dense_size), eps=eps)
    return t.detach(), w.detach()


def _hip_ok(pos_bboxes_list, gt_coords_3d, gt_coords_3d_mask, dimensions_list):
    L = len(pos_bboxes_list)
    if not (0 < L <= MAX_IMAGES and len(gt_coords_3d) == len(gt_coords_3d_mask) == len(dimensions_list) == L):
        return False
    if sum(int(b.shape[0]) for b in pos_bboxes_list) < 1:
        return False
    dev = pos_bboxes_list[0].device
    if dev.type != 'cuda':
        return False
    for b, c, m, d in zip(pos_bboxes_list, gt_coords_3d, gt_coords_3d_mask, dimensions_list):
        for t in (b, c, m, d):
            if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.float32:
                return False
        if not (c.is_contiguous() and m.is_contiguous()) or c.dim() != 4 or m.dim() != 4:
            return False
        G = c.shape[0]
        if c.shape[1] != 3 or m.shape != (G, 1) + tuple(c.shape[2:]) or (G and (c.shape[2] < 1 or c.shape[3] < 1)):
            return False
        if b.dim() != 2 or b.shape[1] != 4 or d.dim() != 2 or d.shape[0] != G or d.shape[1] < 3 or (G and d.stride(1) != 1):
            return False
    return True


_ROI_IMAGES = {}


def _roi_images(counts, dev):
    """(n,) int32 on the device: the image of every RoI when image j holds counts[j] of them.  Kept per (device, counts) — a sampler gives
    the same few count tuples step after step — so that the steady state copies nothing from the host."""
    key = (str(dev), tuple(counts))
    t = _ROI_IMAGES.get(key)
    if t is None:
        if len(_ROI_IMAGES) > 256:
            _ROI_IMAGES.clear()
        t = _ROI_IMAGES[key] = torch.from_numpy(np.repeat(np.arange(len(counts), dtype=np.int32), counts)).to(dev)
    return t


def noc_targets(pos_bboxes_list, pos_assigned_gt_inds_list, gt_coords_3d, gt_coords_3d_mask, dimensions_list, flips, dense_size,
                coord_coder=None, eps=1e-4):
    """The dense NOC targets from the RAW maps.  Per image j: pos_bboxes (n_j, 4), pos_assigned_gt_inds (n_j,), gt_coords_3d
    (G_j, 3, H_j, W_j) masked coordinates, gt_coords_3d_mask (G_j, 1, H_j, W_j), dimensions (G_j, 3) rows, flip; ``dense_size`` int or (h, w);
    ``coord_coder`` anything with ``target_means``, ``target_stds`` and ``eps`` (default: the NOC coder's).

    Returns (targets (n, 3, h, w), weights (n, 1, h, w)), detached, n = sum n_j; the reference's empty tensors when n = 0.

    CUDA tensors in fp32 with contiguous maps and unit-stride dimension rows, n >= 1 and at most 32 images run two HIP launches (``mr_noc_dense_target``): only the
    pixels under the RoIs are read and encoded.  Anything else runs :func:`noc_targets_composed`.  Both give the same bits, except for
    the RoIs the kernel is specified to zero and the composed path cannot index: a ground-truth index outside its image's range and a
    NaN coordinate."""
    h, w = _pair(dense_size)
    if sum(int(b.shape[0]) for b in pos_bboxes_list) == 0 and len(pos_bboxes_list):
        b = pos_bboxes_list[0]
        return b.new_zeros((0, 3, h, w)), b.new_zeros((0, 1, h, w))
    if not _hip_ok(pos_bboxes_list, gt_coords_3d, gt_coords_3d_mask, dimensions_list):
        return noc_targets_composed(pos_bboxes_list, pos_assigned_gt_inds_list, gt_coords_3d, gt_coords_3d_mask, dimensions_list, flips,
                                    (h, w), coord_coder, eps)
    return _noc_targets_hip(pos_bboxes_list, pos_assigned_gt_inds_list, gt_coords_3d, gt_coords_3d_mask, dimensions_list, flips, (h, w),
                            coord_coder, eps)[:2]


def _noc_targets_hip(pos_bboxes_list, pos_assigned_gt_inds_list, gt_coords_3d, gt_coords_3d_mask, dimensions_list, flips, dense_size,
                     coord_coder=None, eps=1e-4, out=None):
    """The fused path itself (inputs as ``_hip_ok`` admits them): (targets, weights, counts), counts (n,) int32 the positive bins per RoI.
    ``out``: the three output tensors to write into instead of new ones (the tests fill them with NaN first)."""
    h, w = dense_size
    means, stds, eps_c = _coder_consts(coord_coder)
    dev = pos_bboxes_list[0].device
    L = len(pos_bboxes_list)
    counts = [int(b.shape[0]) for b in pos_bboxes_list]
    n = sum(counts)
    rois = torch.cat([b.detach().reshape(-1, 4) for b in pos_bboxes_list], dim=0).contiguous()
    roi_gt = torch.cat([torch.as_tensor(g, device=dev).detach().reshape(-1).to(torch.int64) for g in pos_assigned_gt_inds_list], dim=0).contiguous()
    assert roi_gt.numel() == n, 'one assigned ground-truth index per positive proposal'
    roi_img = _roi_images(counts, dev)
    dims = [d.detach() for d in dimensions_list]
    vp = ctypes.c_void_p * L
    i32 = ctypes.c_int32 * L
    tables = dict(
        coords_3d=vp(*[c.data_ptr() for c in gt_coords_3d]), coords_3d_mask=vp(*[m.data_ptr() for m in gt_coords_3d_mask]),
        dimensions=vp(*[d.data_ptr() for d in dims]),
        dimensions_row_stride=(ctypes.c_int64 * L)(*[d.stride(0) if d.shape[0] > 1 else max(d.shape[1], 3) for d in dims]),
        map_h=i32(*[max(int(c.shape[2]), 1) for c in gt_coords_3d]), map_w=i32(*[max(int(c.shape[3]), 1) for c in gt_coords_3d]),
        num_gt=i32(*[int(c.shape[0]) for c in gt_coords_3d]), flip=(ctypes.c_uint8 * L)(*[1 if bool(f) else 0 for f in flips]))
    if out is None:
        out = (torch.empty(n, 3, h, w, device=dev, dtype=torch.float32), torch.empty(n, 1, h, w, device=dev, dtype=torch.float32),
               torch.empty(n, device=dev, dtype=torch.int32))
    targets, weights, cnt = out
    assert targets.shape == (n, 3, h, w) and weights.shape == (n, 1, h, w) and cnt.shape == (n,) and cnt.dtype == torch.int32
    assert all(t.is_contiguous() and t.device == dev for t in out) and targets.dtype == weights.dtype == torch.float32
    mu, sd = _const(means, dev), _const(stds, dev)
    with torch.cuda.device(dev):
        _lib.call('mr_noc_dense_target', tables, num_images=L, rois=rois.data_ptr(), roi_img=roi_img.data_ptr(), roi_gt=roi_gt.data_ptr(), n=n, h=h,
                  w=w, target_means=mu.data_ptr(), target_stds=sd.data_ptr(), eps_coder=float(eps_c), eps_target=float(eps),
                  targets=targets.data_ptr(), weights=weights.data_ptr(), counts=cnt.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
    return targets, weights, cnt
