"""Consumers of the PnP outputs on the inference tail, forward only:

  * ``score_head_inputs``  — the feature vector MLPScoreHead builds from the pose
    (/root/reference/monorun/models/roi_heads/bbox_3d_heads/score_heads/mlp_score_head.py:101-103)
  * ``get_bbox_3d_result`` / ``xywhr2xyxyr`` / ``multiclass_3d_result_nms`` — same contracts as
    monorun/models/roi_heads/monorun_roi_head.py:606-677, with the rotated-BEV NMS done by this library's
    HIP kernel (``mr_nms_bev_batched``) instead of ``mmdet3d.ops.iou3d.nms_gpu`` (third-party CUDA op).
"""
import numpy as np
import torch

from . import _lib


def score_head_inputs(yaw, t_vec, pose_cov, dimensions):
    """[yaw, t_vec, tril(pose_cov) in torch.tril_indices(4, 4) order, dimensions] -> (n, 17)."""
    r, c = torch.tril_indices(4, 4, device=pose_cov.device)
    return torch.cat([yaw, t_vec, pose_cov[:, r, c], dimensions], dim=1)


def get_bbox_3d_result(dimensions, yaw, t_vec, scores, labels, num_classes, to_np=False):
    """Per-class list of (n_c, 8) rows [l, h, w, x, y, z, ry, score] (monorun_roi_head.py:606-617)."""
    rows = torch.cat((dimensions, t_vec, yaw, scores.unsqueeze(1)), dim=1)
    if to_np:
        rows, labels = rows.cpu().numpy(), labels.cpu().numpy()
    return [rows[labels == c] for c in range(num_classes)]


def xywhr2xyxyr(boxes_xywhr):
    """[cx, cy, w, h, r] -> [x1, y1, x2, y2, r] (monorun_roi_head.py:657-677)."""
    centre, half = boxes_xywhr[:, 0:2], boxes_xywhr[:, 2:4] / 2
    return torch.cat((centre - half, centre + half, boxes_xywhr[:, 4:5]), dim=1)


def nms_bev(boxes_xyxyr_list, scores_list, thr):
    """Batched rotated-BEV NMS: one group per list entry, ONE launch.  Returns a list of int64 tensors of
    kept indices (local to each group, descending score)."""
    _lib.load()
    dev = boxes_xyxyr_list[0].device
    if dev.type != 'cuda':
        raise RuntimeError('monorun_amd.consumers.nms_bev runs on an MI355X only (no CPU fallback)')
    sizes = [int(b.shape[0]) for b in boxes_xyxyr_list]
    total, groups = sum(sizes), len(sizes)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=dev)
    f32 = dict(device=dev, dtype=torch.float32)
    boxes = torch.cat([b.detach().to(**f32).reshape(-1, 5) for b in boxes_xyxyr_list]).contiguous() if total else torch.zeros(0, 5, **f32)
    scores = torch.cat([s.detach().to(**f32).reshape(-1) for s in scores_list]).contiguous() if total else torch.zeros(0, **f32)
    keep = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
    num = torch.zeros(groups, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.call('mr_nms_bev_batched', boxes_xyxyr=boxes.data_ptr(), scores=scores.data_ptr(), offsets=offsets.data_ptr(), groups=groups,
                  max_group=max(sizes) if sizes else 0, thr=float(thr), keep=keep.data_ptr(), num_keep=num.data_ptr(),
                  stream=torch.cuda.current_stream(dev).cuda_stream)
    num_h = num.cpu().tolist()
    off_h = offsets.cpu().tolist()
    return [keep[off_h[g]:off_h[g] + num_h[g]] for g in range(groups)]


def multiclass_3d_result_nms(bbox_3d_result, nms_thr=0.25, to_np=True):
    """Rotated-BEV NMS per class over a list of (n, 8) [l, h, w, x, y, z, ry, score] tensors; returns (kept rows per class,
    kept indices per class), as numpy when to_np — the contract of monorun_roi_head.py:619-655, including its n <= 1 branch
    that returns zeros(n) as indices."""
    big = [i for i, b in enumerate(bbox_3d_result) if b.size(0) > 1]
    kept = {}
    if big:
        ks = nms_bev([xywhr2xyxyr(bbox_3d_result[i][:, [3, 5, 0, 2, 6]]) for i in big], [bbox_3d_result[i][:, 7] for i in big], nms_thr)
        kept = dict(zip(big, ks))
    out, inds = [], []
    for i, b in enumerate(bbox_3d_result):
        n = b.size(0)
        if i in kept:
            k = kept[i]
            out.append(b[k].cpu().numpy() if to_np else b[k])
            inds.append(k.cpu().numpy() if to_np else k)
        else:
            out.append(b.cpu().numpy() if to_np else b)
            inds.append(np.zeros(n, dtype=np.int64) if to_np else b.new_zeros((n, ), dtype=torch.int64))
    return out, inds


# ----------------------------------------------------------------------------------------------------------------------------------
# The same tail in ONE launch (mr_result3d_nms, include/monorun_result3d.h): rows, split by class, xywhr2xyxyr,
# NMS and the gather of the kept 3-D rows and 2-D boxes, into one packed buffer that a single copy brings to the host.
RESULT3D_MAX_N = 512                # MR_RESULT3D_MAX_N
RESULT3D_MAX_CLASSES = 16           # MR_RESULT3D_MAX_CLASSES
RESULT3D_FIELDS = ('out3d', 'out2d', 'keep_local', 'keep_row', 'num_keep', 'num_in_class')


def result_3d_layout(num_classes, n):
    """The packed buffer of `num_classes` classes over `n` rows: {field: (byte offset, numpy dtype, shape)} and its size in bytes.
    The int64 fields come first and out3d starts on a multiple of 16 bytes."""
    c = int(num_classes)
    shapes = (('keep_local', np.int64, (c, n)), ('keep_row', np.int64, (c, n)), ('out3d', np.float32, (c, n, 8)),
              ('out2d', np.float32, (c, n, 5)), ('num_keep', np.int32, (c,)), ('num_in_class', np.int32, (c,)))
    layout, off = {}, 0
    for name, dtype, shape in shapes:
        layout[name] = (off, np.dtype(dtype), shape)
        off += int(np.prod(shape)) * np.dtype(dtype).itemsize
    return layout, off


def _result_3d_fast(dimensions, yaw, t_vec, scores, labels, det_bboxes, num_classes):
    """The one-launch path serves CUDA fp32 inputs (int64 labels) within the caps; everything else takes the composition."""
    n = int(scores.shape[0])
    return (scores.device.type == 'cuda' and n <= RESULT3D_MAX_N and 0 <= num_classes <= RESULT3D_MAX_CLASSES and labels.dtype == torch.int64
            and all(t.dtype == torch.float32 and t.device == scores.device for t in (dimensions, yaw, t_vec, scores, det_bboxes))
            and labels.device == scores.device)


_TORCH_OF = {np.dtype(np.int64): torch.int64, np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32}


def _result_3d_views(buf, num_classes, n):
    layout, _ = result_3d_layout(num_classes, n)
    out = {}
    for name, (off, dtype, shape) in layout.items():
        size = int(np.prod(shape)) * dtype.itemsize
        out[name] = buf[off:off + size].view(_TORCH_OF[dtype]).view(shape)
    return out


def _result_3d_packed(dimensions, yaw, t_vec, scores, labels, det_bboxes, num_classes, nms_thr):
    """(packed uint8 buffer on the inputs' device, its six views).  No host synchronisation on the one-launch path."""
    n, dev = int(scores.shape[0]), scores.device
    _, size = result_3d_layout(num_classes, n)
    if _result_3d_fast(dimensions, yaw, t_vec, scores, labels, det_bboxes, num_classes):
        _lib.load()
        buf = torch.empty(max(size, 16), dtype=torch.uint8, device=dev)
        v = _result_3d_views(buf, num_classes, n)
        ins = [t.detach().contiguous() for t in (dimensions, yaw, t_vec, scores, labels, det_bboxes)]
        with torch.cuda.device(dev):
            _lib.call('mr_result3d_nms', dimensions=ins[0].data_ptr(), yaw=ins[1].data_ptr(), t_vec=ins[2].data_ptr(), scores=ins[3].data_ptr(),
                      labels=ins[4].data_ptr(), det_bboxes=ins[5].data_ptr(), n=n, num_classes=int(num_classes), thr=float(nms_thr),
                      out3d=v['out3d'].data_ptr(), out2d=v['out2d'].data_ptr(), keep_local=v['keep_local'].data_ptr(),
                      keep_row=v['keep_row'].data_ptr(), num_keep=v['num_keep'].data_ptr(), num_in_class=v['num_in_class'].data_ptr(),
                      stream=torch.cuda.current_stream(dev).cuda_stream)
        return buf, v
    # the same rule with more launches: the composition above, written into the same layout
    buf = torch.zeros(max(size, 16), dtype=torch.uint8, device=dev)
    v = _result_3d_views(buf, num_classes, n)
    v['out3d'].fill_(float('nan'))
    v['out2d'].fill_(float('nan'))
    v['keep_local'].fill_(-1)
    v['keep_row'].fill_(-1)
    res = get_bbox_3d_result(dimensions, yaw, t_vec, scores, labels, num_classes)
    out, inds = multiclass_3d_result_nms(res, nms_thr, to_np=False)
    for c in range(num_classes):
        rows = torch.nonzero(labels == c).reshape(-1)[inds[c]]
        k = int(rows.numel())
        v['out3d'][c, :k] = out[c]
        v['out2d'][c, :k] = det_bboxes[rows]
        v['keep_local'][c, :k] = inds[c]
        v['keep_row'][c, :k] = rows
        v['num_keep'][c] = k
        v['num_in_class'][c] = int(res[c].shape[0])
    return buf, v


def result_3d_nms_padded(dimensions, yaw, t_vec, scores, labels, det_bboxes, num_classes, nms_thr):
    """The class-grouped result of the 3-D NMS as six device tensors over n rows and C = num_classes classes:

      out3d (C, n, 8)  [l, h, w, x, y, z, ry, score] of the k-th kept member of class c at [c, k], in the order the NMS keeps them
      out2d (C, n, 5)  the matching rows of det_bboxes
      keep_local (C, n) int64  their indices within the class (what multiclass_3d_result_nms returns), keep_row (C, n) int64 their rows
      num_keep (C,) int32, num_in_class (C,) int32

    Places past num_keep[c] hold NaN (out3d, out2d) and -1 (keep_local, keep_row).  CUDA fp32 inputs with n <= RESULT3D_MAX_N and
    C <= RESULT3D_MAX_CLASSES take one launch and no host synchronisation; anything else takes get_bbox_3d_result +
    multiclass_3d_result_nms, the same rule with more launches (and their synchronisations)."""
    v = _result_3d_packed(dimensions, yaw, t_vec, scores, labels, det_bboxes, num_classes, nms_thr)[1]
    return tuple(v[f] for f in RESULT3D_FIELDS)


def split_packed_result(buf, num_classes, n):
    """The host side of result_3d_nms: a packed buffer as a numpy uint8 array -> (bbox_3d_result, keep_inds_3d, bbox_result, keep_rows),
    lists over the classes of (k, 8) float32, (k,) int64, (k, 5) float32 and (k,) int64 arrays (copies: they do not keep `buf` alive)."""
    layout, size = result_3d_layout(num_classes, n)
    buf = np.ascontiguousarray(buf).reshape(-1)
    assert buf.dtype == np.uint8 and buf.size >= size, (buf.dtype, buf.size, size)
    f = {name: buf[off:off + int(np.prod(shape)) * dtype.itemsize].view(dtype).reshape(shape) for name, (off, dtype, shape) in layout.items()}
    num = [int(k) for k in f['num_keep']]
    assert all(0 <= k <= n for k in num), num
    return ([f['out3d'][c, :k].copy() for c, k in enumerate(num)], [f['keep_local'][c, :k].copy() for c, k in enumerate(num)],
            [f['out2d'][c, :k].copy() for c, k in enumerate(num)], [f['keep_row'][c, :k].copy() for c, k in enumerate(num)])


def result_3d_nms(dimensions, yaw, t_vec, scores, labels, det_bboxes, num_classes, nms_thr=0.25, to_np=True, with_rows=False):
    """(bbox_3d_result, keep_inds_3d, bbox_result): per class the kept (k, 8) rows, their indices within the class and the matching
    (k, 5) rows of det_bboxes — what monorun_roi_head.py:552-565 computes.  to_np: numpy arrays from ONE copy of the packed buffer to
    the host, the call's only synchronisation; otherwise device tensors, sized by one copy of num_keep.  with_rows: a fourth list, the
    kept members' rows in the inputs."""
    n = int(scores.shape[0])
    buf, v = _result_3d_packed(dimensions, yaw, t_vec, scores, labels, det_bboxes, num_classes, nms_thr)
    if to_np:
        out = split_packed_result(buf.cpu().numpy(), num_classes, n)
    else:
        num = v['num_keep'].cpu().tolist()
        out = tuple([v[f][c, :k] for c, k in enumerate(num)] for f in ('out3d', 'keep_local', 'out2d', 'keep_row'))
    return out if with_rows else out[:3]
