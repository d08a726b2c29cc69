"""Target assignment and sampling of the 2-D detector's training step: mmdet 2.x's ``MaxIoUAssigner``, ``RandomSampler``,
``AssignResult``, ``SamplingResult`` and ``bbox_overlaps`` / ``bbox2delta`` — without mmdet.  :mod:`monorun_amd.rpn_head` and
:mod:`monorun_amd.bbox_head` build ``get_targets`` and ``loss`` on them.

The overlap, every operation rounded to fp32 and no contraction (``eps = 1e-6``; min and max return a NaN operand, as torch's do):

    area = (x2 − x1)·(y2 − y1),   w = max(min(ax2, bx2) − max(ax1, bx1), 0)  (h alike),   inter = w·h
    iou = inter / max((area_a + area_b) − inter, eps),   iof = inter / max(area_a, eps)  with the candidate box first

The assignment per image, over the PRESENT boxes (``valid`` flag set and row below ``counts[n]``; an absent box gets ``gt_ind = −1``,
``max_overlap = 0``, ``label = −1``, deltas 0 and takes part in nothing):

1. with ``ignore_iof_thr > 0`` and ignore boxes, a box whose largest ``iof`` over them is ``> ignore_iof_thr`` has all its overlaps set to −1;
2. ``max_overlap[b]`` / ``argmax[b]``: the largest overlap over the ground truths from a running maximum that starts at (−1, 0) and is raised
   by ``>`` only — ties to the LOWER ground truth, a NaN never raises it;
3. ``gt_max[i]``: the largest overlap of ground truth i over the present boxes, −1 if nothing raises it;
4. ``gt_ind = −1``; 0 where ``0 ≤ max_overlap < neg_iou_thr``; ``argmax + 1`` where ``max_overlap ≥ pos_iou_thr``;
5. with ``match_low_quality``, for i ascending, every box with ``overlap(i, b) == gt_max[i]`` gets ``gt_ind = i + 1`` if
   ``gt_max[i] ≥ min_pos_iou``; the last i wins (``gt_max_assign_all=True``);
6. ``label = gt_labels[gt_ind − 1]`` where ``gt_ind > 0`` (0 without labels), else −1;
7. G = 0: ``gt_ind = 0`` and ``max_overlap = 0`` for every present box.

and ``deltas = bbox2delta(box, gt[gt_ind − 1])`` where ``gt_ind > 0``, else 0: the targets of either head are this array times a mask.

Sampling (``RandomSampler``) per image from ``gt_ind`` and ONE UNIFORM KEY PER BOX (``torch.rand`` on the boxes' device from an optional
``generator``): the sampled positives are the ``min(P, int(num·pos_fraction))`` positives with the smallest keys, the sampled negatives the
``min(Q, num − sampled_pos)`` negatives with the smallest keys (with ``neg_pos_ub ≥ 0`` at most ``int(max(1, sampled_pos)·neg_pos_ub)``), ties
to the lower index, indices reported ascending.  Every subset has the probability ``randperm`` gives it, but the draw is not from
``randperm``'s stream: the one deliberate deviation from mmdet.

Hot path: on CUDA fp32 within the caps (256 ground truths and 256 ignore boxes per image), with ``gt_max_assign_all=True``,
``ignore_wrt_candidates=True`` and a float ``neg_iou_thr``, the assignment of ALL images is ``mr_assign_max_iou`` — two HIP launches, no host
synchronisation, bitwise reproducible.  Everything else — CPU tensors, other dtypes, more ground truths, ``gt_max_assign_all=False`` — runs
the fp32 restatement :func:`assign_torch` per image.
"""
import ctypes

import torch

from . import _lib
from . import proposals as P

MAX_GT = 256            # MR_ASSIGN_MAX_GT of include/monorun_assign.h
MAX_IGNORE = 256        # MR_ASSIGN_MAX_IGNORE
MAX_IMAGES = 65535      # MR_ASSIGN_MAX_IMAGES
EPS = 1e-6


# ------------------------------------------------------------------------------------------------ the rule in torch ops
def bbox_overlaps(bboxes1, bboxes2, mode='iou', is_aligned=False, eps=EPS):
    """mmdet's ``bbox_overlaps``: (m, 4) and (n, 4) -> (m, n), or (m,) when aligned, in the boxes' dtype; ``mode`` 'iou' or 'iof' (over
    the area of ``bboxes1``)."""
    assert mode in ('iou', 'iof'), f'bbox_overlaps: mode {mode!r}'
    assert bboxes1.shape[-1] == 4 and bboxes2.shape[-1] == 4, 'bbox_overlaps: boxes (.., 4)'
    a, b = (bboxes1, bboxes2) if is_aligned else (bboxes1[..., :, None, :], bboxes2[..., None, :, :])
    if is_aligned:
        assert bboxes1.shape == bboxes2.shape, 'bbox_overlaps: aligned boxes have one shape'
    area_a = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    area_b = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    w = (torch.min(a[..., 2], b[..., 2]) - torch.max(a[..., 0], b[..., 0])).clamp(min=0)
    h = (torch.min(a[..., 3], b[..., 3]) - torch.max(a[..., 1], b[..., 1])).clamp(min=0)
    inter = w * h
    union = (area_a + area_b) - inter if mode == 'iou' else area_a + torch.zeros_like(inter)
    return inter / torch.max(union, torch.full((), eps, dtype=union.dtype, device=union.device))


def bbox2delta(proposals, gt, means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.)):
    """mmdet's ``bbox2delta``: (.., 4) and (.., 4) -> (.., 4) in the boxes' dtype."""
    px, py = (proposals[..., 0] + proposals[..., 2]) * 0.5, (proposals[..., 1] + proposals[..., 3]) * 0.5
    pw, ph = proposals[..., 2] - proposals[..., 0], proposals[..., 3] - proposals[..., 1]
    gx, gy = (gt[..., 0] + gt[..., 2]) * 0.5, (gt[..., 1] + gt[..., 3]) * 0.5
    gw, gh = gt[..., 2] - gt[..., 0], gt[..., 3] - gt[..., 1]
    d = ((gx - px) / pw, (gy - py) / ph, torch.log(gw / pw), torch.log(gh / ph))
    return torch.stack([(d[k] - float(means[k])) / float(stds[k]) for k in range(4)], dim=-1)      # scalars: no tensor to copy over


def assign_torch(bboxes, gt_bboxes, gt_bboxes_ignore=None, gt_labels=None, present=None, pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.0,
                 ignore_iof_thr=-1.0, match_low_quality=True, gt_max_assign_all=True, means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.)):
    """The restatement of ``mr_assign_max_iou`` for ONE image in fp32 torch ops on any device (the module's text): bboxes (B, 4 or 5),
    gt_bboxes (G, 4), present (B,) bool or None.  -> dict(gt_ind (B,) int64, label (B,) int64, max_overlap (B,), argmax (B,) int64, ignored
    (B,) bool, gt_max (G,), deltas (B, 4)).  ``gt_max_assign_all=False``: step 5 gives each ground truth only its first best box."""
    f = dict(dtype=torch.float32, device=bboxes.device)
    boxes = bboxes[:, :4].to(torch.float32)
    gts = gt_bboxes.reshape(-1, 4).to(**f)
    B, G = boxes.shape[0], gts.shape[0]
    here = torch.ones(B, dtype=torch.bool, device=boxes.device) if present is None else present.to(device=boxes.device, dtype=torch.bool)
    boxes = torch.where(here[:, None], boxes, torch.zeros((), **f))                   # an absent box is never read
    thr = lambda v: torch.full((), float(v), **f)
    minus, zero = torch.full((), -1.0, **f), torch.zeros((), **f)
    ignored = torch.zeros(B, dtype=torch.bool, device=boxes.device)
    if G == 0:
        gt_ind = torch.where(here, 0, -1)
        return dict(gt_ind=gt_ind, label=torch.full_like(gt_ind, -1), max_overlap=torch.zeros(B, **f), argmax=torch.zeros_like(gt_ind),
                    ignored=ignored, gt_max=torch.zeros(0, **f), deltas=torch.zeros(B, 4, **f))
    ov = bbox_overlaps(gts, boxes)                                                     # (G, B)
    if ignore_iof_thr > 0 and gt_bboxes_ignore is not None and gt_bboxes_ignore.shape[0] > 0:
        iof = bbox_overlaps(boxes, gt_bboxes_ignore.reshape(-1, 4).to(**f), mode='iof')            # (B, I)
        worst = torch.where(iof > minus, iof, minus).max(dim=1)[0]
        ignored = here & (worst > thr(ignore_iof_thr))
        ov = torch.where(ignored[None, :], minus, ov)
    raised = torch.where(ov > minus, ov, minus)                                       # a NaN raises nothing
    index = torch.arange(G, device=boxes.device)[:, None]
    mo = raised.max(dim=0)[0]
    arg = torch.where(raised == mo[None, :], index, G).min(dim=0)[0]
    gt_max = torch.where(here[None, :], raised, minus).max(dim=1)[0] if B > 0 else minus.expand(G).clone()
    gt_ind = torch.full((B,), -1, dtype=torch.int64, device=boxes.device)
    gt_ind = torch.where((mo >= zero) & (mo < thr(neg_iou_thr)), 0, gt_ind)
    gt_ind = torch.where(mo >= thr(pos_iou_thr), arg + 1, gt_ind)
    if match_low_quality and B > 0:
        hit = (ov == gt_max[:, None]) & (gt_max >= thr(min_pos_iou))[:, None] & here[None, :]
        if not gt_max_assign_all:                                                      # each ground truth's first best box only
            first = torch.where(hit, torch.arange(B, device=boxes.device)[None, :], B).min(dim=1)[0]
            hit = hit & (torch.arange(B, device=boxes.device)[None, :] == first[:, None])
        last = torch.where(hit, index + 1, 0).max(dim=0)[0]
        gt_ind = torch.where(last > 0, last, gt_ind)
    gt_ind = torch.where(here, gt_ind, -1)
    pos = gt_ind > 0
    own = (gt_ind - 1).clamp(min=0)
    labels = torch.zeros(G, dtype=torch.int64, device=boxes.device) if gt_labels is None else gt_labels.to(device=boxes.device, dtype=torch.int64)
    label = torch.where(pos, labels[own], -1)
    safe = torch.stack([torch.where(pos, boxes[:, k], torch.full((), float(k >= 2), **f)) for k in range(4)], dim=-1)     # [0, 0, 1, 1]
    deltas = torch.where(pos[:, None], bbox2delta(safe, torch.where(pos[:, None], gts[own], safe), means, stds), zero)
    return dict(gt_ind=gt_ind, label=label, max_overlap=torch.where(here, mo, zero), argmax=torch.where(here, arg, 0), ignored=ignored,
                gt_max=gt_max, deltas=deltas)


# ------------------------------------------------------------------------------------------------ results
class AssignResult:
    """mmdet's ``AssignResult``: ``num_gts``, ``gt_inds`` (B,) int64 (−1 ignore, 0 negative, i + 1 ground truth i), ``max_overlaps`` (B,),
    ``labels`` (B,) int64 or None; ``deltas`` (B, 4), the launch's regression targets, rides along."""

    def __init__(self, num_gts, gt_inds, max_overlaps, labels=None, deltas=None):
        self.num_gts, self.gt_inds, self.max_overlaps, self.labels, self.deltas = num_gts, gt_inds, max_overlaps, labels, deltas

    @property
    def num_preds(self):
        return len(self.gt_inds)

    def add_gt_(self, gt_labels):
        """mmdet's ``add_gt_``: the ground truths are prepended as boxes assigned to themselves with overlap 1."""
        self_inds = torch.arange(1, len(gt_labels) + 1, dtype=torch.int64, device=gt_labels.device)
        self.gt_inds = torch.cat([self_inds, self.gt_inds])
        self.max_overlaps = torch.cat([self.max_overlaps.new_ones(len(gt_labels)), self.max_overlaps])
        if self.labels is not None:
            self.labels = torch.cat([gt_labels.to(self.labels.dtype), self.labels])
        if self.deltas is not None:
            self.deltas = torch.cat([self.deltas.new_zeros(len(gt_labels), 4), self.deltas])


class SamplingResult:
    """mmdet's ``SamplingResult``.  ``bboxes`` (positives, then negatives) and ``pos_bboxes`` are plain attributes: the reference's
    ``forward_train`` assigns them."""

    def __init__(self, pos_inds, neg_inds, bboxes, gt_bboxes, assign_result, gt_flags):
        self.pos_inds, self.neg_inds = pos_inds, neg_inds
        self.pos_bboxes, self.neg_bboxes = bboxes[pos_inds], bboxes[neg_inds]
        self.pos_is_gt = gt_flags[pos_inds]
        self.num_gts = gt_bboxes.shape[0]
        self.pos_assigned_gt_inds = assign_result.gt_inds[pos_inds] - 1
        if gt_bboxes.numel() == 0:
            assert self.pos_assigned_gt_inds.numel() == 0
            self.pos_gt_bboxes = torch.empty_like(gt_bboxes).view(-1, 4)
        else:
            self.pos_gt_bboxes = gt_bboxes.view(-1, gt_bboxes.shape[-1])[self.pos_assigned_gt_inds, :]
        self.pos_gt_labels = assign_result.labels[pos_inds] if assign_result.labels is not None else None
        self.bboxes = torch.cat([self.pos_bboxes, self.neg_bboxes])


class BatchAssignResult:
    """Dense (N, B) results of :meth:`MaxIoUAssigner.assign_batch`: ``gt_inds`` and ``labels`` int64, ``max_overlaps`` fp32, ``ignored``
    bool, ``deltas`` (N, B, 4), ``present`` (N, B) bool; ``gt_max``: per image (G_n,) fp32; ``num_gts``: host integers."""

    def __init__(self, gt_inds, labels, max_overlaps, ignored, deltas, present, gt_max, num_gts):
        self.gt_inds, self.labels, self.max_overlaps, self.ignored, self.deltas = gt_inds, labels, max_overlaps, ignored, deltas
        self.present, self.gt_max, self.num_gts = present, gt_max, list(num_gts)

    def image(self, n, count=None, with_labels=True):
        """The :class:`AssignResult` of image n (its first ``count`` boxes)."""
        s = slice(None, count)
        return AssignResult(self.num_gts[n], self.gt_inds[n, s], self.max_overlaps[n, s], self.labels[n, s] if with_labels else None,
                            self.deltas[n, s])


class BatchSamplingResult:
    """Dense results of :meth:`RandomSampler.sample_batch` over T = Gmax + B boxes per image (Gmax rows of prepended ground truths, 0
    without ``add_gt_as_proposals``; the rows past an image's own G are absent): ``bboxes`` (N, T, 4), ``gt_inds``, ``labels`` (N, T) int64,
    ``deltas`` (N, T, 4), ``pos_mask``, ``neg_mask``, ``pos_is_gt`` (N, T) bool, ``pos_inds``, ``neg_inds`` (N, num) int64 ascending and
    −1 past ``num_pos``, ``num_neg`` (N,) int64; ``gt_rows``: Gmax; ``num_gts``: host integers."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


# ------------------------------------------------------------------------------------------------ the assigner
def _is_float(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


class MaxIoUAssigner:
    """mmdet's ``MaxIoUAssigner`` with its constructor arguments.  The tuple form of ``neg_iou_thr`` and ``gpu_assign_thr > 0`` raise
    ``NotImplementedError``; ``iou_calculator`` must be ``BboxOverlaps2D``."""

    def __init__(self, pos_iou_thr, neg_iou_thr, min_pos_iou=.0, gt_max_assign_all=True, ignore_iof_thr=-1, ignore_wrt_candidates=True,
                 match_low_quality=True, gpu_assign_thr=-1, iou_calculator=dict(type='BboxOverlaps2D')):
        if not _is_float(neg_iou_thr):
            raise NotImplementedError('MaxIoUAssigner: the tuple form of neg_iou_thr is not provided')
        if gpu_assign_thr > 0:
            raise NotImplementedError('MaxIoUAssigner: gpu_assign_thr > 0 is not provided (nothing is moved to the CPU)')
        if dict(iou_calculator).get('type', 'BboxOverlaps2D') != 'BboxOverlaps2D':
            raise NotImplementedError(f'MaxIoUAssigner: iou_calculator {iou_calculator!r} is not provided')
        if not ignore_wrt_candidates and ignore_iof_thr > 0:
            raise NotImplementedError('MaxIoUAssigner: ignore_wrt_candidates=False is not provided')
        self.pos_iou_thr, self.neg_iou_thr, self.min_pos_iou = float(pos_iou_thr), float(neg_iou_thr), float(min_pos_iou)
        self.gt_max_assign_all, self.ignore_iof_thr = bool(gt_max_assign_all), float(ignore_iof_thr)
        self.ignore_wrt_candidates, self.match_low_quality, self.gpu_assign_thr = bool(ignore_wrt_candidates), bool(match_low_quality), gpu_assign_thr

    def _rule(self):
        return dict(pos_iou_thr=self.pos_iou_thr, neg_iou_thr=self.neg_iou_thr, min_pos_iou=self.min_pos_iou,
                    ignore_iof_thr=self.ignore_iof_thr, match_low_quality=self.match_low_quality)

    def hip_ok(self, bboxes, gt_bboxes, gt_bboxes_ignore=None):
        """Whether ``mr_assign_max_iou`` covers this call: CUDA fp32 boxes and ground truths on one device, within the caps,
        ``gt_max_assign_all=True``."""
        if not self.gt_max_assign_all or not isinstance(bboxes, torch.Tensor) or bboxes.device.type != 'cuda' or bboxes.dtype != torch.float32:
            return False
        lists = list(gt_bboxes) + [g for g in (gt_bboxes_ignore or []) if g is not None]
        if any(g.device != bboxes.device or g.dtype != torch.float32 for g in lists):
            return False
        if max((g.shape[0] for g in gt_bboxes), default=0) > MAX_GT or len(gt_bboxes) > MAX_IMAGES:
            return False
        return max((g.shape[0] for g in (gt_bboxes_ignore or []) if g is not None), default=0) <= MAX_IGNORE

    def assign_batch(self, bboxes, gt_bboxes, gt_bboxes_ignore=None, gt_labels=None, valid=None, counts=None,
                     means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.)):
        """All images in one call.  bboxes (N, B, 4 or 5), or (B, 4 or 5): one set of boxes for every image (it is not copied);
        gt_bboxes: N tensors (G_n, 4); gt_bboxes_ignore, gt_labels: N tensors (or None entries) or None; valid (N, B) uint8 / bool or None;
        counts (N,) int32 on the device or None (the rows past ``counts[n]``, NaN in a padded proposal list, are absent).  ->
        :class:`BatchAssignResult`.  Two HIP launches and no host synchronisation when :meth:`hip_ok`, else :func:`assign_torch` per image."""
        N = len(gt_bboxes)
        assert bboxes.dim() in (2, 3) and bboxes.shape[-1] in (4, 5), 'assign_batch: bboxes (N, B, 4 or 5) or (B, 4 or 5)'
        assert bboxes.dim() == 2 or bboxes.shape[0] == N, 'assign_batch: one list entry per image'
        shared, B, dev = bboxes.dim() == 2, bboxes.shape[-2], bboxes.device
        ignore = [None] * N if gt_bboxes_ignore is None else list(gt_bboxes_ignore)
        labels = None if gt_labels is None else list(gt_labels)
        assert len(ignore) == N and (labels is None or len(labels) == N), 'assign_batch: one list entry per image'
        assert valid is None or tuple(valid.shape) == (N, B), 'assign_batch: valid (N, B)'
        assert counts is None or tuple(counts.shape) == (N,), 'assign_batch: counts (N,)'
        num_gts = [int(g.shape[0]) for g in gt_bboxes]
        present = torch.ones(N, B, dtype=torch.bool, device=dev)
        if valid is not None:
            present = present & valid.to(dev).bool()
        if counts is not None:
            present = present & (torch.arange(B, device=dev)[None, :] < counts.to(dev)[:, None])
        if not self.hip_ok(bboxes, gt_bboxes, ignore):
            per = [assign_torch(bboxes if shared else bboxes[n], gt_bboxes[n], ignore[n], None if labels is None else labels[n], present[n],
                                gt_max_assign_all=self.gt_max_assign_all, means=means, stds=stds, **self._rule()) for n in range(N)]
            stack = lambda k, dt: torch.stack([p[k] for p in per]) if N else torch.zeros((0, B) + ((4,) if k == 'deltas' else ()), dtype=dt, device=dev)
            return BatchAssignResult(stack('gt_ind', torch.int64), stack('label', torch.int64), stack('max_overlap', torch.float32),
                                     stack('ignored', torch.bool), stack('deltas', torch.float32), present, [p['gt_max'] for p in per], num_gts)
        i32 = dict(dtype=torch.int32, device=dev)
        max_overlap = torch.zeros(N, B, dtype=torch.float32, device=dev)
        argmax, gt_ind, label = torch.zeros(N, B, **i32), torch.full((N, B), -1, **i32), torch.full((N, B), -1, **i32)
        ignored = torch.zeros(N, B, dtype=torch.uint8, device=dev)
        deltas = torch.zeros(N, B, 4, dtype=torch.float32, device=dev)
        gt_max = torch.full((sum(num_gts),), -1.0, dtype=torch.float32, device=dev)
        if N > 0 and B > 0:
            boxes = bboxes.detach().contiguous()
            gts = torch.cat([g.detach().reshape(-1, 4) for g in gt_bboxes]).contiguous()
            gt_lab = None if labels is None else torch.cat([l.reshape(-1) for l in labels]).to(torch.int32).contiguous()
            num_ign = [0 if g is None else int(g.shape[0]) for g in ignore]
            with_ignore = self.ignore_iof_thr > 0 and max(num_ign) > 0
            ign = torch.cat([g.detach().reshape(-1, 4) for g in ignore if g is not None]).contiguous() if with_ignore else None
            valid8 = None if valid is None else valid.to(device=dev, dtype=torch.uint8).contiguous()
            counts32 = None if counts is None else counts.to(device=dev, dtype=torch.int32).contiguous()
            f4 = ctypes.c_float * 4
            with torch.cuda.device(dev):
                max_gt = max(num_gts)
                ws = torch.empty(max(int(_lib.load().mr_assign_workspace_bytes(N, max_gt)) // 4, 1), **i32)
                gt_off = P._offsets(tuple(num_gts), dev)
                ign_off = P._offsets(tuple(num_ign), dev) if with_ignore else None
                _lib.call('mr_assign_max_iou', boxes=boxes.data_ptr(), image_stride=0 if shared else B * boxes.shape[-1],
                          box_stride=boxes.shape[-1], valid=_lib.ptr(valid8), counts=_lib.ptr(counts32), n_images=N, n_boxes=B,
                          gt_bboxes=gts.data_ptr(), gt_offsets=gt_off.data_ptr(), gt_labels=_lib.ptr(gt_lab), max_gt=max_gt,
                          ignore_bboxes=_lib.ptr(ign), ignore_offsets=_lib.ptr(ign_off), max_ignore=max(num_ign) if with_ignore else 0,
                          means=f4(*[float(m) for m in means]), stds=f4(*[float(s) for s in stds]), max_overlap=max_overlap.data_ptr(),
                          argmax=argmax.data_ptr(), ignored=ignored.data_ptr(), gt_max=gt_max.data_ptr(), gt_ind=gt_ind.data_ptr(),
                          label=label.data_ptr(), deltas=deltas.data_ptr(), workspace=ws.data_ptr(),
                          stream=torch.cuda.current_stream(dev).cuda_stream, **self._rule())
        return BatchAssignResult(gt_ind.long(), label.long(), max_overlap, ignored.bool(), deltas, present, list(torch.split(gt_max, num_gts)),
                                 num_gts)

    def assign(self, bboxes, gt_bboxes, gt_bboxes_ignore=None, gt_labels=None):
        """mmdet's ``assign`` for one image: bboxes (n, 4) or (n, 5) -> :class:`AssignResult`."""
        r = self.assign_batch(bboxes[None], [gt_bboxes], [gt_bboxes_ignore], None if gt_labels is None else [gt_labels])
        return r.image(0, with_labels=gt_labels is not None)


# ------------------------------------------------------------------------------------------------ the sampler
def _ascending(mask, width):
    """The indices of each row's set flags in ascending order: (N, T) bool -> (N, width) int64, −1 past the row's count (a row has at most
    ``width`` flags).  A running count and one scatter whose surplus goes to a spare column: no host synchronisation."""
    N, T = mask.shape
    pos = torch.cumsum(mask, dim=1) - 1
    dest = torch.where(mask & (pos < width), pos, torch.full_like(pos, width))
    out = torch.full((N, width + 1), -1, dtype=torch.int64, device=mask.device)
    out.scatter_(1, dest, torch.arange(T, device=mask.device)[None, :].expand(N, T).contiguous())
    out[:, width] = -1
    return out[:, :width].contiguous()


def _smallest(mask, keys, k):
    """Per row the ``k[n]`` flagged entries with the smallest keys, ties to the lower index: -> (N, T) bool."""
    order = torch.sort(torch.where(mask, keys, torch.full_like(keys, 2.0)), dim=1, stable=True)[1]       # keys are in [0, 1)
    rank = torch.empty_like(order)
    rank.scatter_(1, order, torch.arange(mask.shape[1], device=mask.device)[None, :].expand_as(order).contiguous())
    return mask & (rank < k[:, None])


class RandomSampler:
    """mmdet's ``RandomSampler`` with its constructor arguments, drawing by one uniform key per box (the module's text)."""

    def __init__(self, num, pos_fraction, neg_pos_ub=-1, add_gt_as_proposals=True, **kwargs):
        self.num, self.pos_fraction, self.neg_pos_ub, self.add_gt_as_proposals = int(num), float(pos_fraction), neg_pos_ub, bool(add_gt_as_proposals)

    def _choose(self, gt_inds, keys):
        """-> (pos_mask, neg_mask) (N, T) bool from gt_inds (N, T) and keys (N, T)."""
        pos, neg = gt_inds > 0, gt_inds == 0
        n_pos = pos.sum(dim=1).clamp(max=int(self.num * self.pos_fraction))
        n_neg = torch.minimum(neg.sum(dim=1), self.num - n_pos)
        if self.neg_pos_ub >= 0:
            n_neg = torch.minimum(n_neg, torch.floor(n_pos.clamp(min=1).to(torch.float64) * float(self.neg_pos_ub)).to(torch.int64))
        return _smallest(pos, keys, n_pos), _smallest(neg, keys, n_neg)

    def sample_batch(self, assign_result, bboxes, gt_bboxes, gt_labels=None, generator=None, keys=None):
        """All images in one call, without a host synchronisation.  assign_result: a :class:`BatchAssignResult`; bboxes (N, B, 4 or 5) or
        (B, 4 or 5); gt_bboxes: N tensors (G_n, 4); gt_labels: N tensors, needed with ``add_gt_as_proposals`` when the assignment carries
        labels; keys (N, Gmax + B) fp32 in [0, 1) or None: ``torch.rand`` on the boxes' device from ``generator``.  ->
        :class:`BatchSamplingResult`."""
        a, N = assign_result, len(gt_bboxes)
        dev = a.gt_inds.device
        boxes = (bboxes[None].expand(N, -1, -1) if bboxes.dim() == 2 else bboxes)[..., :4]
        B = boxes.shape[1]
        num_gts = [int(g.shape[0]) for g in gt_bboxes]
        Gm = max(num_gts, default=0) if self.add_gt_as_proposals else 0
        gt_inds, labels, deltas, is_gt = a.gt_inds, a.labels, a.deltas, torch.zeros(N, Gm + B, dtype=torch.bool, device=dev)
        if Gm > 0:
            rows = torch.arange(Gm, device=dev)[None, :]
            own = rows < P.host_to_device(num_gts, torch.int64, dev)[:, None]                      # (N, Gm): the image has this ground truth
            pad = lambda t, fill: torch.cat((t, t.new_full((Gm - t.shape[0],) + tuple(t.shape[1:]), fill)))
            gt_rows = torch.stack([pad(g.detach().reshape(-1, 4).to(boxes.dtype), 0) for g in gt_bboxes])
            lab_rows = torch.stack([pad(l.reshape(-1).to(torch.int64), -1) for l in gt_labels]) if gt_labels is not None else torch.where(own, 0, -1)
            boxes = torch.cat((gt_rows, boxes), dim=1)
            gt_inds = torch.cat((torch.where(own, rows + 1, -1), gt_inds), dim=1)
            labels = torch.cat((torch.where(own, lab_rows, -1), labels), dim=1)
            deltas = torch.cat((deltas.new_zeros(N, Gm, 4), deltas), dim=1)
            is_gt[:, :Gm] = own
        if keys is None:
            keys = torch.rand(N, Gm + B, device=dev, generator=generator)
        assert tuple(keys.shape) == (N, Gm + B), 'sample_batch: one key per box, the prepended ground truths first'
        pos_mask, neg_mask = self._choose(gt_inds, keys.to(dev))
        return BatchSamplingResult(bboxes=boxes, gt_inds=gt_inds, labels=labels, deltas=deltas, pos_mask=pos_mask, neg_mask=neg_mask,
                                   pos_is_gt=is_gt, pos_inds=_ascending(pos_mask, self.num), neg_inds=_ascending(neg_mask, self.num),
                                   num_pos=pos_mask.sum(dim=1), num_neg=neg_mask.sum(dim=1), gt_rows=Gm, num_gts=num_gts, keys=keys,
                                   gt_bboxes=[g.detach().reshape(-1, 4) for g in gt_bboxes])

    def sample(self, assign_result, bboxes, gt_bboxes, gt_labels=None, generator=None, keys=None, **kwargs):
        """mmdet's ``sample`` for one image: -> :class:`SamplingResult`.  keys (G + n,) (G = 0 without ``add_gt_as_proposals``) or None."""
        if bboxes.dim() < 2:
            bboxes = bboxes[None, :]
        bboxes = bboxes[:, :4]
        gt_flags = bboxes.new_zeros((bboxes.shape[0],), dtype=torch.uint8)
        if self.add_gt_as_proposals and len(gt_bboxes) > 0:
            if gt_labels is None:
                raise ValueError('gt_labels must be given when add_gt_as_proposals is True')
            bboxes = torch.cat([gt_bboxes.to(bboxes.dtype), bboxes], dim=0)
            assign_result.add_gt_(gt_labels)
            gt_flags = torch.cat([bboxes.new_ones(gt_bboxes.shape[0], dtype=torch.uint8), gt_flags])
        T = bboxes.shape[0]
        if keys is None:
            keys = torch.rand(T, device=bboxes.device, generator=generator)
        assert tuple(keys.shape) == (T,), 'sample: one key per box, the prepended ground truths first'
        pos_mask, neg_mask = self._choose(assign_result.gt_inds[None, :], keys[None, :].to(bboxes.device))
        pos_inds, neg_inds = torch.nonzero(pos_mask[0]).reshape(-1), torch.nonzero(neg_mask[0]).reshape(-1)
        return SamplingResult(pos_inds, neg_inds, bboxes, gt_bboxes, assign_result, gt_flags)


def split_sampling(batch, counts=None):
    """The list form of a :class:`BatchSamplingResult`: one :class:`SamplingResult` per image, as :meth:`RandomSampler.sample` gives it on
    the image's own ``G_n + B_n`` boxes (``counts``: the B_n, host integers; default: all B).  One read of the counts."""
    out, Gm = [], batch.gt_rows
    num_pos, num_neg = batch.num_pos.tolist(), batch.num_neg.tolist()
    for n, G in enumerate(batch.num_gts):
        g = G if Gm > 0 else 0
        k = batch.bboxes.shape[1] - Gm if counts is None else int(counts[n])
        rows = torch.cat((torch.arange(g, device=batch.bboxes.device), torch.arange(Gm, Gm + k, device=batch.bboxes.device)))
        shift = lambda idx: torch.where(idx >= Gm, idx - (Gm - g), idx)
        a = AssignResult(G, batch.gt_inds[n, rows], None, batch.labels[n, rows], batch.deltas[n, rows])
        out.append(SamplingResult(shift(batch.pos_inds[n, :num_pos[n]]), shift(batch.neg_inds[n, :num_neg[n]]), batch.bboxes[n, rows], batch.gt_bboxes[n], a,
                                  batch.pos_is_gt[n, rows].to(torch.uint8)))
    return out


# ------------------------------------------------------------------------------------------------ builders
ASSIGNERS = {'MaxIoUAssigner': MaxIoUAssigner}
SAMPLERS = {'RandomSampler': RandomSampler}


def _build(cfg, table, what, **extra):
    if not isinstance(cfg, dict):
        return cfg
    cfg = dict(cfg)
    kind = cfg.pop('type')
    if kind not in table:
        raise NotImplementedError(f'{what} type {kind!r} is not provided ({sorted(table)} only)')
    return table[kind](**cfg, **extra)


def build_assigner(cfg):
    return _build(cfg, ASSIGNERS, 'assigner')


def build_sampler(cfg, context=None):
    return _build(cfg, SAMPLERS, 'sampler', context=context)
