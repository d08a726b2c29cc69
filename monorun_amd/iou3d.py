"""Aligned rotated 3-D IoU on the GPU (N5): box i against query box i, as the pose head's training loss computes it
(the reference's monorun/core/bbox_3d/iou_calculators/bbox3d_iou_calculator.py:166-192 ``bbox3d_overlaps_aligned_torch``, whose BEV
step is a numba-CUDA kernel that cannot run on ROCm).  One HIP launch, ``mr_bbox3d_overlaps_aligned``; no CPU fallback: host tensors
are staged through the GPU and the result is returned on the input's device.

Drop-in for the reference's symbol::

    import monorun_amd.iou3d
    sys.modules['monorun.core'].bbox3d_overlaps_aligned_torch = monorun_amd.iou3d.bbox3d_overlaps_aligned_torch
"""
import torch

from . import _lib

HEIGHT_RULES = {'reference': 0, 'geometric': _lib.MR_IOU3D_GEOMETRIC_HEIGHT}


def _rows(t, dev):
    """(N, 7) fp32 on ``dev`` whose rows the kernel can read in place: the 7 values of a row contiguous, any row stride >= 7."""
    t = t.detach()
    if t.dtype != torch.float32 or t.device != dev:
        t = t.to(device=dev, dtype=torch.float32)
    if t.size(0) > 1 and (t.stride(1) != 1 or t.stride(0) < 7):
        t = t.contiguous()
    return t, (t.stride(0) if t.size(0) > 1 else 7)


def bbox3d_overlaps_aligned(boxes, qboxes, criterion=-1, z_axis=1, z_center=1.0, height_rule='reference', return_rinc=False):
    """
    Args:
        boxes (Tensor): (N, 7) [x, y, z, l, h, w, ry] — any device and float dtype (computed in fp32, as the reference does)
        qboxes (Tensor): (N, 7), same layout
        criterion: -1 IoU, 0 over the box volume, 1 over the query volume, 2 intersection volume
        z_axis: the height axis (1 for KITTI camera boxes)
        z_center: 1.0 when the height coordinate is the bottom of the box, 0.0 when it is the top
        height_rule: 'reference' — the lower edge of the height overlap is min(box top, query top), as the reference's torch function
            computes it (bbox3d_iou_calculator.py:145), the value its score head trains against; 'geometric' — max(...), the true
            overlap, as its numpy function (:84)
        return_rinc: also return the BEV intersection areas (N,)

    Returns:
        Tensor: (N, 1) fp32 IoUs on the input device (and the (N,) BEV areas with ``return_rinc``)
    """
    if criterion not in (-1, 0, 1, 2) or z_axis not in (0, 1, 2) or height_rule not in HEIGHT_RULES:
        raise ValueError(f'bbox3d_overlaps_aligned: criterion {criterion!r}, z_axis {z_axis!r}, height_rule {height_rule!r}')
    if boxes.dim() != 2 or boxes.size(1) != 7 or tuple(qboxes.shape) != tuple(boxes.shape):
        raise ValueError(f'bbox3d_overlaps_aligned: boxes {tuple(boxes.shape)} and qboxes {tuple(qboxes.shape)} must both be (N, 7)')
    src = boxes.device
    dev = src if src.type == 'cuda' else (qboxes.device if qboxes.device.type == 'cuda' else None)
    if dev is None:
        if not torch.cuda.is_available():
            raise RuntimeError('bbox3d_overlaps_aligned runs on an MI355X only (no CPU fallback)')
        dev = torch.device('cuda', torch.cuda.current_device())
    n = boxes.size(0)
    with torch.no_grad():
        b, bs = _rows(boxes, dev)
        q, qs = _rows(qboxes, dev)
        iou = torch.empty(n, 1, device=dev, dtype=torch.float32)
        rinc = torch.empty(n, device=dev, dtype=torch.float32) if return_rinc else None
        if n:
            with torch.cuda.device(dev):
                _lib.call('mr_bbox3d_overlaps_aligned', boxes=b.data_ptr(), boxes_row_stride=bs, qboxes=q.data_ptr(), qboxes_row_stride=qs, n=n,
                          criterion=int(criterion), z_axis=int(z_axis), z_center=float(z_center), flags=HEIGHT_RULES[height_rule],
                          iou=iou.data_ptr(), rinc=_lib.ptr(rinc), stream=torch.cuda.current_stream(dev).cuda_stream)
    if src != dev:
        iou = iou.to(src)
        rinc = rinc.to(src) if rinc is not None else None
    return (iou, rinc) if return_rinc else iou


def bbox3d_overlaps_aligned_torch(boxes, qboxes, criterion=-1, z_axis=1, z_center=1.0):
    """The reference's symbol, for aliasing it: same arguments and the shape it actually returns, (N,) — its docstring says
    (N, 1), but its caller unsqueezes the result (uncert_prop_pnp_optimizer.py:118-124)."""
    return bbox3d_overlaps_aligned(boxes, qboxes, criterion, z_axis, z_center).squeeze(1)
