"""The NOC head's training decode (N8): from the head's raw output ``all_pred`` to ``coords_3d`` and the pixel log-std, as
``MonoRUnRoIHead.forward_train`` of the reference chains them (monorun/models/roi_heads/monorun_roi_head.py:189-217, :374-394):

  * the flip branch and class slice of ``FCNNOCDecoder`` (bbox_3d_heads/dense_decoders/fcn_noc_decoder.py:225-267),
  * ``MultiClassNormDimCoder.decode`` (core/bbox_3d/dim_coder/multiclass_norm_dim_coder.py:28-36),
  * ``NOCCoder.decode`` with ``part_var=None`` (core/bbox_3d/coord_coder/noc_coder.py:50-73),
  * ``DistanceInvarProjErrorCoder.decode_logstd`` with the ground-truth distances
    (core/bbox_3d/proj_error_coder/distance_invar_proj_error_coder.py:39-60).

``pose_head.noc_decode`` (K2) is the inference form of the same chain: no gradients, ``distance=None``, an inverse std instead of the
log-std.  :func:`decode_for_training` is differentiable in ``all_pred``, ``dim`` and ``dim_var``.

Hot path: CUDA inputs run one HIP launch forward (``mr_noc_decode_train``) and one backward (``mr_noc_decode_train_backward``, which
recomputes the forward from the inputs and writes every channel of ``grad_all_pred``).  Everything else — CPU tensors, no objects,
``distances`` that require grad, a backward under ``create_graph=True`` — runs :func:`decode_for_training_torch`, the torch restatement.

:func:`get_targets` and :func:`loss` (N9) are the head's LiDAR supervision, ``FCNNOCDecoder.get_targets`` and ``.loss``
(fcn_noc_decoder.py:269-297): the dense NOC targets by :func:`monorun_amd.noc_targets.noc_targets` and ``loss_noc``.
"""
import torch

from . import _lib
from . import noc_targets as _noc_targets
from .pose_head import DIM_MEANS, DIM_STDS, NOC_MEANS, NOC_STDS, _PRED_DTYPES, _const, _flip_flags
from .projection_head import DistanceInvarProjErrorCoder

OUTPUTS = ('noc_pred', 'proj_logstd', 'coords_3d', 'coords_3d_var', 'proj_logstd_px', 'dims', 'dims_var')


def decode_for_training_torch(all_pred, labels, flip, dim, dim_var=None, distances=None, num_classes=3, class_agnostic=False,
                              dim_means=DIM_MEANS, dim_stds=DIM_STDS, noc_means=NOC_MEANS, noc_stds=NOC_STDS,
                              ref_length=1.6, ref_focal_y=722, target_std=0.15, distance_min=0.1, epistemic_std_gain=1.0):
    """The chain in plain differentiable torch, operation for operation what the reference's four functions do.  Same arguments and
    result as :func:`decode_for_training`; any device, any floating dtype."""
    n, ch, h, w = all_pred.shape
    cn = 1 if class_agnostic else num_classes
    assert ch == 2 * cn * 5, f'all_pred has {ch} channels, expected {2 * cn * 5}'
    labels = torch.as_tensor(labels, device=all_pred.device).long()
    inds = torch.arange(0, n, dtype=torch.long, device=all_pred.device)
    # the flip branch (fcn_noc_decoder.py:225-235)
    pred = all_pred.reshape(n, 2, ch // 2, h, w)
    if isinstance(flip, bool):
        pred = pred[:, 1] if flip else pred[:, 0]
    else:
        pred = pred[inds, torch.as_tensor(flip, device=all_pred.device).reshape(-1).long().expand(n)]
    # slice_pred (fcn_noc_decoder.py:243-267)
    all_noc_pred, all_proj_logstd = pred.split([3 * cn, 2 * cn], dim=1)
    if class_agnostic:
        noc_pred, proj_logstd = all_noc_pred, all_proj_logstd
    else:
        noc_pred = all_noc_pred.reshape(n, num_classes, 3, h, w)[inds, labels]
        proj_logstd = all_proj_logstd.reshape(n, num_classes, 2, h, w)[inds, labels]
    # MultiClassNormDimCoder.decode
    target_means = dim.new_tensor(dim_means)[labels]
    target_stds = dim.new_tensor(dim_stds)[labels]
    dims = dim * target_stds + target_means
    dims_var = dim_var * target_stds.square() if dim_var is not None else None
    # NOCCoder.decode, part_var=None (its `flip` argument is unused)
    part = noc_pred * noc_pred.new_tensor(noc_stds)[:, None, None] + noc_pred.new_tensor(noc_means)[:, None, None]
    coords_3d = part * dims[..., None, None]
    coords_3d_var = dims_var[..., None, None] * part.square() if dims_var is not None else None
    # DistanceInvarProjErrorCoder.decode_logstd
    coder = DistanceInvarProjErrorCoder(ref_length=ref_length, ref_focal_y=ref_focal_y, target_std=target_std, distance_min=distance_min,
                                        epistemic_std_gain=epistemic_std_gain)
    if distances is not None:
        distances = distances.reshape(n, 1)
    proj_logstd_px = coder.decode_logstd(proj_logstd, coords_3d_var, distances)
    return dict(noc_pred=noc_pred, proj_logstd=proj_logstd, coords_3d=coords_3d, coords_3d_var=coords_3d_var,
                proj_logstd_px=proj_logstd_px, dims=dims, dims_var=dims_var)


class _DecodeFunction(torch.autograd.Function):
    """``mr_noc_decode_train`` forward, ``mr_noc_decode_train_backward`` for the gradients to all_pred, dim and dim_var.  all_pred arrives
    contiguous in fp32, fp16 or bf16, dim / dim_var as contiguous fp32, labels int64, flip uint8, distances fp32 (n) or None, the coder
    constants as device tensors.  Outputs whose gradient is None reach the kernel as NULL."""

    @staticmethod
    def forward(ctx, all_pred, dim, dim_var, labels, flip, distances, consts, scalars):
        n, _, h, w = all_pred.shape
        dev = all_pred.device
        f32 = dict(device=dev, dtype=torch.float32)
        maps3 = [torch.empty(n, 3, h, w, **f32) for _ in range(3 if dim_var is not None else 2)]
        maps2 = [torch.empty(n, 2, h, w, **f32) for _ in range(2)]
        dims = torch.empty(n, 3, **f32)
        dims_var = torch.empty(n, 3, **f32) if dim_var is not None else None
        out = dict(noc_pred=maps3[0], proj_logstd=maps2[0], coords_3d=maps3[1], coords_3d_var=maps3[2] if dim_var is not None else None,
                   proj_logstd_px=maps2[1], dims=dims, dims_var=dims_var)
        ctx.common = _common_args(all_pred, labels, flip, dim, dim_var, consts, scalars)
        with torch.cuda.device(dev):
            _lib.call('mr_noc_decode_train', ctx.common, distances=_lib.ptr(distances), distance_min=scalars['distance_min'],
                      **{k: _lib.ptr(v) for k, v in out.items()}, stream=torch.cuda.current_stream(dev).cuda_stream)
        ctx.save_for_backward(all_pred, dim, dim_var, labels, flip, distances, *consts)
        ctx.scalars = scalars
        ctx.set_materialize_grads(False)
        return tuple(out[k] for k in OUTPUTS)

    @staticmethod
    def backward(ctx, *grads):
        all_pred, dim, dim_var, labels, flip, distances = ctx.saved_tensors[:6]
        if torch.is_grad_enabled():
            # create_graph=True: the gradients must carry a graph themselves, which the kernel cannot give: torch differentiates the restatement
            return _torch_backward(ctx, grads) + (None,) * 5
        dev = all_pred.device
        grads = [g.to(torch.float32).contiguous() if g is not None else None for g in grads]
        grad_all_pred = torch.empty_like(all_pred)
        grad_dim = torch.empty_like(dim)
        grad_dim_var = torch.empty_like(dim_var) if dim_var is not None else None
        with torch.cuda.device(dev):
            _lib.call('mr_noc_decode_train_backward', ctx.common, grad_all_pred=grad_all_pred.data_ptr(), grad_dim=grad_dim.data_ptr(),
                      grad_dim_var=_lib.ptr(grad_dim_var), **{'grad_' + k: _lib.ptr(g) for k, g in zip(OUTPUTS, grads)},
                      stream=torch.cuda.current_stream(dev).cuda_stream)
        return grad_all_pred, grad_dim, grad_dim_var, None, None, None, None, None


def _common_args(all_pred, labels, flip, dim, dim_var, consts, scalars):
    """The arguments both entry points share, by the header's names.  Pointers only: the tensors are kept by save_for_backward."""
    n, _, h, w = all_pred.shape
    mu, sd, nm, ns = consts
    return dict(all_pred=all_pred.data_ptr(), pred_dtype=_PRED_DTYPES[all_pred.dtype], labels=labels.data_ptr(), flip=flip.data_ptr(),
                dim=dim.data_ptr(), dim_var=_lib.ptr(dim_var), n=n, num_classes=scalars['num_classes'], class_agnostic=scalars['class_agnostic'],
                h=h, w=w, dim_means=mu.data_ptr(), dim_stds=sd.data_ptr(), noc_means=nm.data_ptr(), noc_stds=ns.data_ptr(),
                proj_scaling_denominator=scalars['proj_scaling_denominator'], ref_focal_y=scalars['ref_focal_y'],
                epistemic_std_gain=scalars['epistemic_std_gain'])


def _torch_backward(ctx, grads):
    """(grad_all_pred, grad_dim, grad_dim_var) by autograd of the torch restatement on the saved inputs, with a graph of their own."""
    all_pred, dim, dim_var, labels, flip, distances = ctx.saved_tensors[:6]
    with torch.enable_grad():
        out = decode_for_training_torch(all_pred.float(), labels, flip.bool(), dim, dim_var, distances, **ctx.scalars['kw'])
        pairs = [(out[k], g) for k, g in zip(OUTPUTS, grads) if g is not None and out[k] is not None]
        ins = [t for t in (all_pred, dim, dim_var) if t is not None and t.requires_grad]
        got = iter(torch.autograd.grad([o for o, _ in pairs], ins, [g for _, g in pairs], create_graph=True, allow_unused=True))
    return tuple(next(got) if t is not None and t.requires_grad else None for t in (all_pred, dim, dim_var))


def _hip_ok(all_pred, dim, dim_var, distances):
    ts = [t for t in (all_pred, dim, dim_var, distances) if t is not None]
    if not all(isinstance(t, torch.Tensor) and t.is_floating_point() for t in ts):
        return False
    dev = all_pred.device
    if dev.type != 'cuda' or any(t.device != dev for t in ts):
        return False
    if all_pred.dim() != 4 or all_pred.numel() == 0:
        return False
    return not (distances is not None and torch.is_grad_enabled() and distances.requires_grad)


def decode_for_training(all_pred, labels, flip, dim, dim_var=None, distances=None, num_classes=3, class_agnostic=False,
                        dim_means=DIM_MEANS, dim_stds=DIM_STDS, noc_means=NOC_MEANS, noc_stds=NOC_STDS,
                        ref_length=1.6, ref_focal_y=722, target_std=0.15, distance_min=0.1, epistemic_std_gain=1.0):
    """Raw NOC-head output of the n positive RoIs -> everything ``forward_train`` decodes from it, differentiably.

    all_pred (n, 2*Cn*5, h, w) with Cn = 1 if class_agnostic else num_classes; labels (n,) int; flip bool | (n,) bool;
    dim (n, 3); dim_var (n, 3) | None; distances (n, 1) | (n,) | None (the ground-truth distances of the projection head's
    ``get_properties``; None: the reference distance, as at inference).

    Returns dict(noc_pred (n,3,h,w), proj_logstd (n,2,h,w) — the selected channels, encoded —, coords_3d (n,3,h,w),
    coords_3d_var (n,3,h,w) | None, proj_logstd_px (n,2,h,w) — the pixel log-std the pose head takes —, dims (n,3), dims_var (n,3) | None).
    Gradients flow to all_pred, dim and dim_var (in their dtypes); the HIP path gives none to distances, labels and flip.  On the HIP
    path the outputs are fp32 (an all_pred of another dtype than fp32 / fp16 / bf16 is cast to fp32 and the outputs back to it).
    """
    kw = dict(num_classes=num_classes, class_agnostic=class_agnostic, dim_means=dim_means, dim_stds=dim_stds, noc_means=noc_means,
              noc_stds=noc_stds, ref_length=ref_length, ref_focal_y=ref_focal_y, target_std=target_std, distance_min=distance_min,
              epistemic_std_gain=epistemic_std_gain)
    if not _hip_ok(all_pred, dim, dim_var, distances):
        if isinstance(all_pred, torch.Tensor) and all_pred.dtype in (torch.float16, torch.bfloat16):
            all_pred = all_pred.float()          # decoded in fp32, as the kernel does
        return decode_for_training_torch(all_pred, labels, flip, dim, dim_var, distances, **kw)
    n, ch, h, w = all_pred.shape
    cn = 1 if class_agnostic else num_classes
    assert ch == 2 * cn * 5, f'all_pred has {ch} channels, expected {2 * cn * 5}'
    dev = all_pred.device
    ap = (all_pred if all_pred.dtype in _PRED_DTYPES else all_pred.to(torch.float32)).contiguous()
    dm = dim.to(torch.float32).contiguous()
    dv = dim_var.to(torch.float32).contiguous() if dim_var is not None else None
    assert dm.shape == (n, 3) and (dv is None or dv.shape == (n, 3)), 'dim and dim_var must be (n, 3)'
    lab = torch.as_tensor(labels, device=dev).detach().to(torch.int64).contiguous()
    assert lab.shape == (n,), 'labels must hold one class per object'
    fl = _flip_flags(flip, n, dev)
    dist = None
    if distances is not None:
        dist = distances.detach().to(torch.float32).reshape(-1).contiguous()
        assert dist.numel() == n, 'distances must hold one distance per object'
    consts = tuple(_const(v, dev) for v in (dim_means, dim_stds, noc_means, noc_stds))
    assert consts[0].shape == consts[1].shape and consts[0].shape[1] == 3 and consts[0].shape[0] >= (1 if class_agnostic else num_classes)
    scalars = dict(num_classes=int(num_classes), class_agnostic=int(bool(class_agnostic)),
                   proj_scaling_denominator=float(ref_length * ref_focal_y * target_std), ref_focal_y=float(ref_focal_y),
                   epistemic_std_gain=float(epistemic_std_gain), distance_min=float(distance_min), kw=kw)
    out = dict(zip(OUTPUTS, _DecodeFunction.apply(ap, dm, dv, lab, fl, dist, consts, scalars)))
    if all_pred.dtype not in _PRED_DTYPES:
        out = {k: v.to(all_pred.dtype) if v is not None else None for k, v in out.items()}
    return out


class NOCCoder:
    """The reference's ``NOCCoder`` (core/bbox_3d/coord_coder/noc_coder.py): ``encode`` of the ground truth's masked coordinate maps into
    the head's targets, ``decode`` of its predictions into object coordinates and their variance."""

    def __init__(self, target_means=NOC_MEANS, target_stds=NOC_STDS, eps=1e-5):
        self.target_means = target_means
        self.target_stds = target_stds
        self.eps = eps

    def encode(self, gt_coords_3d, gt_coords_3d_mask, dimensions, flip):
        return _noc_targets.noc_encode(gt_coords_3d, gt_coords_3d_mask, dimensions, flip, self.target_means, self.target_stds, self.eps)

    def decode(self, part, part_var, dimensions, dimensions_var, flip=None):
        """Encoded parts (n, 3, h, w) and object dimensions (n, 3) -> object coordinates: p = part * std + mean, coords_3d = p * dim.
        With a variance of the parts and / or of the dimensions (either may be None), the variance of that product of two
        independent factors: var_p dim^2 + var_dim p^2 + var_p var_dim, var_p = part_var * std^2; None when neither is given.
        ``flip`` is unused (the reference's decode ignores it too)."""
        scale = part.new_tensor(self.target_stds)[:, None, None]
        p = part * scale + part.new_tensor(self.target_means)[:, None, None]
        extent = dimensions[..., None, None]
        var_p = part_var * scale.square() if part_var is not None else None
        var_d = dimensions_var[..., None, None] if dimensions_var is not None else None
        terms = []
        if var_p is not None:
            terms.append(var_p * extent.square())
        if var_d is not None:
            terms.append(var_d * p.square())
        if var_p is not None and var_d is not None:
            terms.append(var_p * var_d)
        return p * extent, (sum(terms[1:], terms[0]) if terms else None)


def get_targets(sampling_results, gt_coords_3d, gt_coords_3d_mask, gt_bboxes_3d, rcnn_train_cfg, img_metas, coord_coder=None):
    """``FCNNOCDecoder.get_targets``: per image the sampling result (``pos_bboxes``, ``pos_assigned_gt_inds``), the ground truth's masked
    coordinate maps and masks, its 3-D boxes (the first three columns are the dimensions) and the image meta (``flip``);
    ``rcnn_train_cfg.dense_size``.  Returns (noc_targets (n, 3, h, w), noc_weights (n, 1, h, w)) over the positives of the batch."""
    dense_size = rcnn_train_cfg['dense_size'] if isinstance(rcnn_train_cfg, dict) else rcnn_train_cfg.dense_size
    return _noc_targets.noc_targets(
        [res.pos_bboxes for res in sampling_results], [res.pos_assigned_gt_inds for res in sampling_results], gt_coords_3d,
        gt_coords_3d_mask, [b[:, :3] for b in gt_bboxes_3d], [meta['flip'] for meta in img_metas], dense_size,
        coord_coder=coord_coder if coord_coder is not None else NOCCoder())


def loss(noc_pred, noc_targets, noc_weights, loss_noc):
    """``FCNNOCDecoder.loss``: dict(loss_noc=...) or, without a ``loss_noc``, an empty dict.  noc_pred is taken in fp32 (the
    reference's ``force_fp32``); with no positives the loss is ``noc_pred.sum()``, a zero that keeps the graph."""
    if loss_noc is None:
        return dict()
    if noc_pred.dtype in (torch.float16, torch.bfloat16):
        noc_pred = noc_pred.float()
    if noc_pred.size(0) == 0:
        return dict(loss_noc=noc_pred.sum())
    return dict(loss_noc=loss_noc(noc_pred, noc_targets, weight=noc_weights))
