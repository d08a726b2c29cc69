"""The positives of a training step: the hand-over from the 2-D stage to the 3-D heads in
``MonoRUnRoIHead.forward_train`` (the reference's monorun_roi_head.py:168-195 and :374-394).  From the dense sampling of the batch
(:class:`monorun_amd.assigners.BatchSamplingResult`), the bbox head's deltas and the per-image ground truth, for the K sampled positives
image by image and, inside an image, by ascending sampled index:

    pos_bboxes (K, 4), pos_rois (K, 5)      the positive RoI moved by the deltas of its ground-truth label's class and clamped to its image
                                            (``regress_by_class``; positives that are prepended ground truths are moved like any other)
    pos_gt_labels, pos_assigned_gt_inds     (K,) int64
    pos_img (K,) int32, pos_img_long int64  the image of each positive
    pos_bboxes_3d (K, 7), pos_cam_intrinsic (K, 3, 3), img_shapes (K, 2) [H, W], flip (K,) uint8      ``get_properties`` and the flip list
    dim_targets (K, 3)                      ``(dims − mean[label]) / std[label]``: ``global_head.get_targets``

Hot path: on CUDA fp32 within the caps (``assigners.MAX_IMAGES`` images, ``assigners.MAX_GT`` ground truths per image,
``bbox_head.MAX_CLASSES`` classes) :func:`positives` is ``mr_roi_train_positives`` — ONE HIP launch, no atomics, no host synchronisation,
bitwise reproducible.  Everything else runs :func:`positives_torch`: the same rule in torch ops (``regress_by_class``, ``get_properties``,
``global_head.get_targets`` and gathers), bit for bit on inputs whose indices stay inside their tables (the kernel voids a positive whose
index leaves its table, include/monorun_roi_train.h; torch's indexing raises instead).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from . import proposals as P
from .assigners import MAX_GT, MAX_IMAGES
from .bbox_head import MAX_CLASSES, decode_torch
from .pose_head import _const

FIELDS = ('pos_rois', 'pos_bboxes', 'pos_gt_labels', 'pos_assigned_gt_inds', 'pos_img', 'pos_img_long', 'pos_bboxes_3d', 'pos_cam_intrinsic',
          'img_shapes', 'flip', 'dim_targets')


class Positives:
    """The fields of the module's text, ``counts``: the positives of each image, host integers, and ``launched``: whether the HIP path
    made them (False: :func:`positives_torch`)."""

    def __init__(self, counts, launched=False, **fields):
        assert set(fields) == set(FIELDS)
        self.counts = [int(c) for c in counts]
        self.launched = bool(launched)                     # whether mr_roi_train_positives made them (K = 0: its path, without a launch)
        self.__dict__.update(fields)

    def __len__(self):
        return sum(self.counts)

    def per_image(self, field):
        """The rows of one field image by image: views, no copy."""
        return list(torch.split(getattr(self, field), self.counts))


def _gt3d(gt_bboxes_3d, dev):
    return torch.cat([g.detach().reshape(-1, 7).to(device=dev, dtype=torch.float32) for g in gt_bboxes_3d]) if len(gt_bboxes_3d) else \
        torch.zeros(0, 7, dtype=torch.float32, device=dev)


def _image_rows(img_shapes, flips, dev):
    """(N, 2) fp32 [H, W] and (N,) uint8 on ``dev`` from host values, or device tensors as they are: no blocking copy."""
    hw = img_shapes if isinstance(img_shapes, torch.Tensor) else P.host_to_device([[float(s[0]), float(s[1])] for s in img_shapes], torch.float32, dev)
    fl = flips if isinstance(flips, torch.Tensor) else P.host_to_device([1 if bool(f) else 0 for f in flips], torch.uint8, dev)
    return hw.to(device=dev, dtype=torch.float32), fl.to(device=dev, dtype=torch.uint8)


def _cam_rows(cam_intrinsic, N, dev):
    cam = cam_intrinsic if isinstance(cam_intrinsic, torch.Tensor) else torch.stack([k.reshape(3, 3) for k in cam_intrinsic])
    return cam.detach().to(device=dev, dtype=torch.float32).reshape(N, 3, 3)


def _row_index(counts, dev):
    """The image of every positive, (K,) int64 on ``dev`` from the host counts, without a blocking copy."""
    return P.host_to_device(np.repeat(np.arange(len(counts)), list(counts)).tolist(), torch.int64, dev)


def positives_torch(batch, counts, bbox_pred, bbox_row_offsets, gt_bboxes_3d, cam_intrinsic, img_shapes, flips, num_classes,
                    reg_class_agnostic, means, stds, dim_means, dim_stds, wh_ratio_clip=P.WH_RATIO_CLIP):
    """The restatement of ``mr_roi_train_positives`` in fp32 torch ops on any device: the arguments and result of :func:`positives`."""
    counts = [int(c) for c in counts]
    N, K, dev = len(counts), sum(counts), batch.bboxes.device
    f, i64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int64, device=dev)
    if K == 0:
        return Positives(counts, pos_rois=torch.zeros(0, 5, **f), pos_bboxes=torch.zeros(0, 4, **f), pos_gt_labels=torch.zeros(0, **i64),
                         pos_assigned_gt_inds=torch.zeros(0, **i64), pos_img=torch.zeros(0, dtype=torch.int32, device=dev),
                         pos_img_long=torch.zeros(0, **i64), pos_bboxes_3d=torch.zeros(0, 7, **f), pos_cam_intrinsic=torch.zeros(0, 3, 3, **f),
                         img_shapes=torch.zeros(0, 2, **f), flip=torch.zeros(0, dtype=torch.uint8, device=dev), dim_targets=torch.zeros(0, 3, **f))
    img = _row_index(counts, dev)                                                                   # (K,)
    place = torch.cat([torch.arange(c, device=dev) for c in counts])
    t = batch.pos_inds[img, place]
    label, gt = batch.labels[img, t].to(torch.int64), batch.gt_inds[img, t].to(torch.int64) - 1
    boxes = batch.bboxes[img, t].to(torch.float32).reshape(K, 4)
    offs = torch.as_tensor([int(o) for o in bbox_row_offsets], dtype=torch.int64)
    rows = P.host_to_device(np.repeat(offs.numpy()[:N], counts).tolist(), torch.int64, dev) + place
    pred = bbox_pred.detach().to(torch.float32)[rows].reshape(K, -1)
    if not reg_class_agnostic:
        pred = pred.reshape(K, -1, 4).gather(1, label[:, None, None].expand(K, 1, 4)).reshape(K, 4)
    hw, fl = _image_rows(img_shapes, flips, dev)
    rois5 = torch.cat((img.to(torch.float32)[:, None], boxes), dim=1)
    moved = decode_torch(rois5, pred, hw[img], None, means, stds, wh_ratio_clip)[:, 0]
    gt_off = torch.as_tensor([0] + list(np.cumsum([int(g.shape[0]) for g in gt_bboxes_3d])), dtype=torch.int64)
    gt_first = P.host_to_device(np.repeat(gt_off.numpy()[:N], counts).tolist(), torch.int64, dev)
    box3d = _gt3d(gt_bboxes_3d, dev)[gt_first + gt].reshape(K, 7)
    mu, sd = _const(dim_means, dev), _const(dim_stds, dev)
    dim_targets = box3d[:, :3].sub(mu[label]).div(sd[label])
    cam = _cam_rows(cam_intrinsic, N, dev)
    return Positives(counts, pos_rois=torch.cat((img.to(torch.float32)[:, None], moved), dim=1), pos_bboxes=moved, pos_gt_labels=label,
                     pos_assigned_gt_inds=gt, pos_img=img.to(torch.int32), pos_img_long=img, pos_bboxes_3d=box3d, pos_cam_intrinsic=cam[img],
                     img_shapes=hw[img], flip=fl[img], dim_targets=dim_targets)


def hip_ok(batch, counts, bbox_pred, gt_bboxes_3d, cam_intrinsic, num_classes, dim_means):
    """Whether ``mr_roi_train_positives`` covers this call: CUDA fp32 tensors on one device, int64 sampling indices, within the caps of the
    assignment (images, ground truths per image) and of the bbox head (classes), a dimension coder with a row per class."""
    dev = batch.bboxes.device
    if dev.type != 'cuda':
        return False
    floats = [batch.bboxes, bbox_pred] + list(gt_bboxes_3d) + (list(cam_intrinsic) if not isinstance(cam_intrinsic, torch.Tensor) else [cam_intrinsic])
    if any(not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.float32 for t in floats):
        return False
    if any(t.device != dev or t.dtype != torch.int64 for t in (batch.gt_inds, batch.labels, batch.pos_inds)):
        return False
    if len(counts) > MAX_IMAGES or max((int(g.shape[0]) for g in gt_bboxes_3d), default=0) > MAX_GT or not 1 <= num_classes <= MAX_CLASSES:
        return False
    N, T = batch.gt_inds.shape
    return len(dim_means) >= num_classes and N * T <= 2 ** 31 - 1 and 4 * bbox_pred.shape[0] * num_classes <= 2 ** 31 - 1


def positives(batch, counts, bbox_pred, bbox_row_offsets, gt_bboxes_3d, cam_intrinsic, img_shapes, flips, num_classes, reg_class_agnostic,
              means, stds, dim_means, dim_stds, wh_ratio_clip=P.WH_RATIO_CLIP):
    """The positives of the batch.  batch: the :class:`BatchSamplingResult` (``bboxes`` (N, T, 4), ``gt_inds``, ``labels`` (N, T),
    ``pos_inds`` (N, num)); counts: the sampled positives of each image, HOST integers (the one read of ``num_pos`` a step performs);
    bbox_pred (R, 4C) or (R, 4): the bbox head's deltas, image n's positives at rows ``bbox_row_offsets[n] + j`` (host integers: the
    reference orders an image's rows positives first); gt_bboxes_3d: N tensors (G_n, 7); cam_intrinsic: N tensors (3, 3) or (N, 3, 3);
    img_shapes: N host ``(H, W[, c])`` or a device tensor (N, 2); flips: N host bools or a device tensor (N,) uint8; means, stds,
    wh_ratio_clip: the bbox coder's; dim_means, dim_stds: the dimension coder's per-class rows.  -> :class:`Positives`.  ONE HIP launch when
    :func:`hip_ok`, else :func:`positives_torch`."""
    counts = [int(c) for c in counts]
    N, K, C = len(counts), sum(counts), int(num_classes)
    assert batch.gt_inds.shape[0] == N == len(gt_bboxes_3d) and len(bbox_row_offsets) >= N, 'positives: one entry per image'
    assert bbox_pred.dim() == 2 and bbox_pred.shape[1] == (4 if reg_class_agnostic else 4 * C), 'positives: bbox_pred (R, 4C) or (R, 4)'
    assert max(counts, default=0) <= batch.pos_inds.shape[1], 'positives: more positives than the sampler gives an image'
    args = (batch, counts, bbox_pred, bbox_row_offsets, gt_bboxes_3d, cam_intrinsic, img_shapes, flips, C, reg_class_agnostic, means, stds,
            dim_means, dim_stds, wh_ratio_clip)
    if not hip_ok(batch, counts, bbox_pred, gt_bboxes_3d, cam_intrinsic, C, dim_means):
        return positives_torch(*args)
    dev = batch.bboxes.device
    f32, i64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int64, device=dev)
    out = dict(pos_rois=torch.empty(K, 5, **f32), pos_bboxes=torch.empty(K, 4, **f32), pos_gt_labels=torch.empty(K, **i64),
               pos_assigned_gt_inds=torch.empty(K, **i64), pos_img=torch.empty(K, dtype=torch.int32, device=dev), pos_img_long=torch.empty(K, **i64),
               pos_bboxes_3d=torch.empty(K, 7, **f32), pos_cam_intrinsic=torch.empty(K, 3, 3, **f32), img_shapes=torch.empty(K, 2, **f32),
               flip=torch.empty(K, dtype=torch.uint8, device=dev), dim_targets=torch.empty(K, 3, **f32))
    if K == 0:
        return Positives(counts, launched=True, **out)
    # the device inputs, bound to names that live across the launch
    boxes, gt_inds, labels, pos_inds = batch.bboxes.detach().contiguous(), batch.gt_inds.contiguous(), batch.labels.contiguous(), batch.pos_inds.contiguous()
    pred = bbox_pred.detach().contiguous()
    num_gts = [int(g.shape[0]) for g in gt_bboxes_3d]
    gt3d = _gt3d(gt_bboxes_3d, dev).contiguous()
    cam = _cam_rows(cam_intrinsic, N, dev).contiguous()
    hw, fl = _image_rows(img_shapes, flips, dev)
    hw, fl = hw.contiguous(), fl.contiguous()
    assert hw.shape == (N, 2) and fl.shape == (N,) and boxes.shape == (N, gt_inds.shape[1], 4), 'positives: one shape and flag per image'
    pos_off, gt_off = P._offsets(tuple(counts), dev), P._offsets(tuple(num_gts), dev)
    row_off = P.host_to_device([int(o) for o in bbox_row_offsets][:N], torch.int32, dev)
    mu, sd = _const(dim_means, dev), _const(dim_stds, dev)
    assert mu.shape == sd.shape and mu.dim() == 2 and mu.shape[1] == 3 and mu.shape[0] >= C, 'positives: dimension coder rows (>= C, 3)'
    f4 = ctypes.c_float * 4
    with torch.cuda.device(dev):
        _lib.call('mr_roi_train_positives', bboxes=boxes.data_ptr(), gt_inds=gt_inds.data_ptr(), labels=labels.data_ptr(),
                  pos_inds=pos_inds.data_ptr(), pos_offsets=pos_off.data_ptr(), n_images=N, n_boxes=gt_inds.shape[1], num=pos_inds.shape[1],
                  n_pos=K, bbox_pred=pred.data_ptr(), bbox_row_offsets=row_off.data_ptr(), n_rows=pred.shape[0], num_classes=C,
                  reg_class_agnostic=int(bool(reg_class_agnostic)), gt_bboxes_3d=gt3d.data_ptr(), gt_offsets=gt_off.data_ptr(),
                  n_gt=gt3d.shape[0], max_gt=max(num_gts), cam_intrinsic=cam.data_ptr(), img_shape=hw.data_ptr(), flip=fl.data_ptr(),
                  means=f4(*[float(m) for m in means]), stds=f4(*[float(s) for s in stds]), wh_ratio_clip=float(wh_ratio_clip),
                  dim_means=mu.data_ptr(), dim_stds=sd.data_ptr(), pos_rois=out['pos_rois'].data_ptr(), pos_bboxes=out['pos_bboxes'].data_ptr(),
                  pos_gt_labels=out['pos_gt_labels'].data_ptr(), pos_assigned_gt_inds=out['pos_assigned_gt_inds'].data_ptr(),
                  pos_img=out['pos_img'].data_ptr(), pos_img_long=out['pos_img_long'].data_ptr(), pos_bboxes_3d=out['pos_bboxes_3d'].data_ptr(),
                  pos_cam_intrinsic=out['pos_cam_intrinsic'].data_ptr(), pos_img_shapes=out['img_shapes'].data_ptr(),
                  pos_flip=out['flip'].data_ptr(), dim_targets=out['dim_targets'].data_ptr(),
                  stream=torch.cuda.current_stream(dev).cuda_stream)
    return Positives(counts, launched=True, **out)
