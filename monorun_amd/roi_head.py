"""``MonoRUnRoIHead``, inference side: the reference's ``simple_test`` (monorun/models/roi_heads/monorun_roi_head.py:442-605) assembled
from this package's modules — proposals and feature maps of ONE image in, ``[dict(bbox_results=…, bbox_3d_results=…)]`` out (DESIGN.md
§24).  It needs neither mmcv nor mmdet: every sub-module is given built, or as the reference's config dict, which :func:`build`
resolves through :data:`MODULES`, a table of the classes this package has (a type it does not know raises ``KeyError``).

``simple_test`` has two paths over the same sub-modules, and the docstring of :meth:`MonoRUnRoIHead.simple_test` states which
conditions choose which.  Both start alike — the 2-D detection (``_bbox_forward``, ``get_bboxes``) and the global head
(``_reg_forward``) — and differ from the NOC head on:

  literal   ``_noc_forward`` -> ``coord_coder.decode`` -> ``_projection_decode`` -> RoIAlign of ``coord_2d`` -> ``_pose_forward`` ->
            ``cov_correction`` -> ``_score_forward`` -> ``consumers.get_bbox_3d_result`` + ``multiclass_3d_result_nms``: the
            reference's statements, one for one
  fast      ``noc_head.forward_all_pred`` -> ``pose_head.pose_from_head`` -> ``score_head.score_poses`` ->
            ``consumers.result_3d_nms``: the fused launches, two host synchronisations in all (the detection count, the result copy)

``forward_train`` is the reference's training step (monorun_roi_head.py:99-254) over the same sub-modules, again with two
paths, which differ in the sampling and in the hand-over from the 2-D stage to the 3-D heads:

  literal   per image ``bbox_assigner.assign`` + ``bbox_sampler.sample``; the reference's else-branch (a mask over the RoIs,
            ``regress_by_class``) or its refined-assigner branch; ``get_targets`` / ``get_properties`` of the heads on the list of
            ``SamplingResult``: the reference's statements, one for one, on any device
  fast      one ``assign_batch`` and one ``sample_batch`` for all images, one read of the counts (``split_sampling``), the same bbox
            stage, then ONE launch — ``roi_train.positives`` — whose outputs feed the 3-D heads directly, and
            ``noc_head.forward_all_pred`` -> ``slice_pred`` + ``decode_for_training`` where :meth:`train_decode_reason` is None

``aug_test``, ``async_simple_test`` and ``forward_dummy`` raise ``NotImplementedError``."""
import copy
import types

import numpy as np
import torch
import torch.nn as nn

from . import assigners, consumers, roi_train
from . import proposals as P
from .bbox_head import Shared2FCBBoxHead, bbox2result, bbox2roi
from .fpn import FPN, FPNplus
from .global_head import FCExtractor, FCExtractorMonteCarlo, MultiClassNormDimCoder
from .noc_decoder import FCNNOCDecoder
from .noc_head import NOCCoder, decode_for_training
from .noc_targets import roi_align_avg_torch
from .pose_head import UncertPropPnPOptimizer, pose_from_head, roi_align_avg
from .projection_head import DistanceInvarProjErrorCoder, UncertProjectionHead
from .resnet import ResNet
from .roi_extractor import SingleRoIExtractor, SingleRoIExtractorMod
from .rpn_head import RPNHeadMod
from .score_head import MLPScoreHead, score_poses

# config ``type`` -> class, for the modules this package has (their constructors call the package's own build_* helpers for the coders,
# the losses and the PnP op)
MODULES = {cls.__name__: cls for cls in (
    ResNet, FPN, FPNplus, RPNHeadMod, SingleRoIExtractor, SingleRoIExtractorMod, Shared2FCBBoxHead, FCExtractor, FCExtractorMonteCarlo,
    FCNNOCDecoder, UncertProjectionHead, UncertPropPnPOptimizer, MLPScoreHead)}


def build(cfg, **extra):
    """A built module as it is, None as None, a config dict ``dict(type=…, **kwargs)`` through :data:`MODULES` (``extra``: keywords
    added to the dict, as the reference adds ``train_cfg`` / ``test_cfg``).  ``KeyError`` naming a type the table does not have."""
    if cfg is None or isinstance(cfg, nn.Module):
        return cfg
    cfg = dict(cfg)
    typ = cfg.pop('type')
    if typ not in MODULES:
        raise KeyError(f'{typ}: monorun_amd has no module of this type (it has {sorted(MODULES)})')
    cfg.update(extra)
    return MODULES[typ](**cfg)


def cfg_get(cfg, key, default=None):
    """``cfg[key]`` of a dict or ``cfg.key`` of an attribute object (mmcv's ``Config``); ``default`` when absent or ``cfg`` is None."""
    if cfg is None:
        return default
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


class MonoRUnRoIHead(nn.Module):
    """The reference's RoI head with its constructor keywords and attribute names, so the ``roi_head.*`` slice of a MonoRUn checkpoint
    (``bbox_head.*``, ``noc_head.*``, ``global_head.*``, ``projection_head.*``, ``pose_head.*``, ``score_head.*``) loads with
    ``strict=True``.  The RoI extractors have no parameters."""

    def __init__(self, bbox_roi_extractor=None, bbox_head=None, noc_roi_extractor=None, noc_head=None, global_head=None,
                 projection_head=None, pose_head=None, score_head=None, train_cfg=None, test_cfg=None, debug=False):
        super().__init__()
        self.train_cfg = train_cfg
        self.test_cfg = test_cfg
        if bbox_head is not None:
            self.bbox_roi_extractor = build(bbox_roi_extractor)
            self.bbox_head = build(bbox_head)
        if noc_head is not None:
            assert noc_roi_extractor is not None
            self.noc_roi_extractor = build(noc_roi_extractor)
            self.noc_head = build(noc_head)
        if global_head is not None:
            self.global_head = build(global_head)
        if projection_head is not None:
            self.projection_head = build(projection_head)
        if pose_head is not None:
            self.pose_head = build(pose_head)
        if score_head is not None:
            self.score_head = build(score_head, train_cfg=train_cfg) if isinstance(score_head, dict) else score_head
        self.debug = debug
        self.new_version = True                       # mmdet >= 2.4.0: simple_test returns a list with one dict per image
        self.init_assigner_sampler()

    def init_assigner_sampler(self):
        """The reference's: ``bbox_assigner`` / ``bbox_sampler`` and the optional ``bbox_refined_assigner`` / ``bbox_refined_sampler`` from
        ``train_cfg`` through ``assigners.build_*``; all None without a ``train_cfg``, or with one that lacks either of the first two
        (one that only carries what the sub-heads read, such as ``iou3d_sampler`` or ``dense_size``)."""
        self.bbox_assigner = self.bbox_sampler = None
        self.bbox_refined_assigner = self.bbox_refined_sampler = None
        if cfg_get(self.train_cfg, 'bbox_assigner') is not None and cfg_get(self.train_cfg, 'bbox_sampler') is not None:
            self.bbox_assigner = assigners.build_assigner(cfg_get(self.train_cfg, 'bbox_assigner'))
            self.bbox_sampler = assigners.build_sampler(cfg_get(self.train_cfg, 'bbox_sampler'), context=self)
            if cfg_get(self.train_cfg, 'bbox_refined_assigner') is not None:
                self.bbox_refined_assigner = assigners.build_assigner(cfg_get(self.train_cfg, 'bbox_refined_assigner'))
            if cfg_get(self.train_cfg, 'bbox_refined_sampler') is not None:
                self.bbox_refined_sampler = assigners.build_sampler(cfg_get(self.train_cfg, 'bbox_refined_sampler'), context=self)

    with_bbox = property(lambda self: getattr(self, 'bbox_head', None) is not None)
    with_noc = property(lambda self: getattr(self, 'noc_head', None) is not None)
    with_reg = property(lambda self: getattr(self, 'global_head', None) is not None)
    with_projection = property(lambda self: getattr(self, 'projection_head', None) is not None)
    with_pose = property(lambda self: getattr(self, 'pose_head', None) is not None)
    with_score = property(lambda self: getattr(self, 'score_head', None) is not None)

    def init_weights(self, pretrained=None):
        if self.with_bbox:
            self.bbox_roi_extractor.init_weights()
            self.bbox_head.init_weights()
        if self.with_noc:
            self.noc_head.init_weights()
            self.noc_roi_extractor.init_weights()
        if self.with_reg:
            self.global_head.init_weights()
        if self.with_pose:
            self.pose_head.init_weights()
        if self.with_score:
            self.score_head.init_weights()

    def forward_dummy(self, x, proposals):
        raise NotImplementedError

    # ------------------------------------------------------------------------------------------------ training
    def train_fast_path_reason(self, x, proposal_list=None):
        """None when the fast path serves ``forward_train``, else the condition that sends the call to the literal path (a string)."""
        if not (x[0].device.type == 'cuda' and x[0].dtype == torch.float32):
            return 'the feature maps are not CUDA fp32'
        if self.bbox_refined_assigner is not None and self.bbox_refined_sampler is not None:
            return 'a refined assigner: the proposals are refined and sampled again per image'
        if self.debug:
            return 'debug: the targets replace the predictions per stage'
        if not (isinstance(self.bbox_assigner, assigners.MaxIoUAssigner) and isinstance(self.bbox_sampler, assigners.RandomSampler)):
            return 'an assigner or sampler without the batch form'
        if not (isinstance(self.bbox_head, Shared2FCBBoxHead) and isinstance(self.global_head, FCExtractor)
                and isinstance(self.global_head.dim_coder, MultiClassNormDimCoder) and self.global_head.loss_dim is not None):
            return 'a bbox head, global head or dimension coder the positive stage does not restate'
        if self.with_projection and not isinstance(self.projection_head, UncertProjectionHead):
            return 'a projection head whose get_properties the positive stage does not restate'
        if proposal_list is not None and any(p.device != x[0].device or p.dtype != torch.float32 for p in proposal_list):
            return 'proposals that are not CUDA fp32'
        return None

    def train_decode_reason(self):
        """None when the fast path decodes with ``noc_head.decode_for_training`` (one launch forward, one backward), else the condition
        that keeps the literal decode (``noc_head(...)``, ``coord_coder.decode``, ``_projection_decode``) inside it (a string)."""
        nh, gh = self.noc_head, self.global_head
        if not self.with_projection:
            return 'no projection head: its coder decodes the log-std'
        ph = self.projection_head
        if not ph.train_std_of_encoded_error:
            return 'train_std_of_encoded_error is off: the fused decode always decodes the encoded log-std'
        if not (isinstance(ph.proj_error_coder, DistanceInvarProjErrorCoder) and isinstance(gh.dim_coder, MultiClassNormDimCoder)
                and isinstance(nh, FCNNOCDecoder) and isinstance(nh.coord_coder, NOCCoder)):
            return 'a coder or head the fused decode does not restate'
        if not (nh.flip_correction and nh.noc_channels == 3 and nh.uncert_channels == 2):
            return 'a NOC head layout other than two flip branches of 3 + 2 channels per class'
        return None

    def _pos_distances(self, pos_bboxes_3d):
        """``get_properties``' distances of the positives' ground-truth boxes, (n, 1)."""
        if self.projection_head.distance_mode == 'z-depth':
            return pos_bboxes_3d[:, 5:6]
        return torch.norm(pos_bboxes_3d[:, 3:6], p=2, dim=1, keepdim=True)

    def forward_train(self, x, img_metas, proposal_list, gt_bboxes, gt_labels, gt_bboxes_ignore=None, gt_masks=None, gt_bboxes_3d=None,
                      gt_coords_3d=None, gt_coords_3d_mask=None, coord_2d=None, cam_intrinsic=None, path=None, generator=None, keys=None):
        """The reference's training step (monorun_roi_head.py:99-254): feature maps ``x``, per image the proposals (k_n, 4 or 5), the 2-D
        and 3-D ground truth, the dense coordinate maps and masks; ``coord_2d`` (N, 2, H, W) and ``cam_intrinsic`` (N, 3, 3) (or N
        matrices).  -> the dict of the sub-modules' losses under their own keys.

        ``path=None`` takes the FAST path when :meth:`train_fast_path_reason` is None — CUDA fp32, no refined assigner, no ``debug``, this
        package's assigner, sampler, bbox head, global head and coders — and the LITERAL path otherwise; ``path='literal'`` forces the
        literal path; ``path='fast'`` raises where the fast path does not apply.  The last path taken is kept in ``self.last_train_path``.
        ``generator`` / ``keys``: the sampler's, as ``RPNHeadMod.loss`` has them; ``keys`` (N, Gmax + Bmax) in the batch layout of
        ``RandomSampler.sample_batch`` (Gmax rows of prepended ground truths, then Bmax = the most proposals of an image), from which the
        literal path takes each image's own entries: with the same keys both paths sample the same boxes.  The fast path reads the
        sampled counts once; every tensor after that read is sized from them.  Inside it, ``last_positive_stage`` says whether the
        launch or its torch restatement made the positives, and ``last_train_decode`` whether the fused training decode ran
        (:meth:`train_decode_reason`); what is downstream of that decode agrees with the literal path to fp32 rounding, the rest bit for bit."""
        if self.bbox_assigner is None or self.bbox_sampler is None:
            # an inference head stays what it was: it does not train.  Training needs the train_cfg's bbox_assigner and bbox_sampler
            raise NotImplementedError('MonoRUnRoIHead.forward_train: the head was built without a train_cfg (bbox_assigner, bbox_sampler); '
                                      'an assigner and a sampler chosen by default for such a head are a follow-up: pass the train_cfg')
        assert self.with_bbox and self.with_noc and self.with_reg
        assert path in (None, 'fast', 'literal'), path
        why = self.train_fast_path_reason(x, proposal_list)
        if path == 'fast' and why is not None:
            raise RuntimeError(f'MonoRUnRoIHead.forward_train(path="fast"): {why}')
        fast = why is None and path != 'literal'
        self.last_train_path = 'fast' if fast else 'literal'
        num_imgs = len(img_metas)
        if gt_bboxes_ignore is None:
            gt_bboxes_ignore = [None for _ in range(num_imgs)]
        num_gts = [int(g.shape[0]) for g in gt_bboxes]
        num_props = [int(p.shape[0]) for p in proposal_list]
        Gm = max(num_gts, default=0) if getattr(self.bbox_sampler, 'add_gt_as_proposals', False) else 0

        batch = None
        if fast:
            # one assignment and one sampling for all images: the proposals padded to the longest list, the rows past an image's own absent
            Bm, dev = max(num_props, default=0), x[0].device
            boxes = torch.stack([torch.cat((p[:, :4], p.new_zeros(Bm - p.shape[0], 4))) for p in proposal_list])
            counts = None if min(num_props, default=0) == Bm else P.host_to_device(num_props, torch.int32, dev)
            assigned = self.bbox_assigner.assign_batch(boxes, gt_bboxes, gt_bboxes_ignore, gt_labels, counts=counts)
            batch = self.bbox_sampler.sample_batch(assigned, boxes, gt_bboxes, gt_labels, generator=generator, keys=keys)
            sampling_results = assigners.split_sampling(batch, counts=num_props)          # the one read of the counts
        else:
            sampling_results = []
            for i in range(num_imgs):
                assign_result = self.bbox_assigner.assign(proposal_list[i], gt_bboxes[i], gt_bboxes_ignore[i], gt_labels[i])
                keys_i = None if keys is None else torch.cat((keys[i, :num_gts[i] if Gm else 0], keys[i, Gm:Gm + num_props[i]]))
                sampling_results.append(self.bbox_sampler.sample(assign_result, proposal_list[i], gt_bboxes[i], gt_labels[i], generator=generator,
                                                                 keys=keys_i, feats=[lvl_feat[i][None] for lvl_feat in x]))

        losses = dict()
        # bbox head forward and loss
        bbox_results = self._bbox_forward_train(x, sampling_results, gt_bboxes, gt_labels, img_metas)
        losses.update(bbox_results['loss_bbox'])

        roi_labels = bbox_results['bbox_targets'][0]
        pos = None
        if fast:
            # the positives of the batch in one launch: regress_by_class, get_properties, the dimension targets, the flip flags
            num_pos = [len(res.pos_inds) for res in sampling_results]
            rows = [len(res.pos_inds) + len(res.neg_inds) for res in sampling_results]
            with torch.no_grad():
                pos = roi_train.positives(batch, num_pos, bbox_results['bbox_pred'], np.concatenate(([0], np.cumsum(rows)))[:num_imgs].tolist(),
                                          gt_bboxes_3d, cam_intrinsic, [m['img_shape'] for m in img_metas], [m['flip'] for m in img_metas],
                                          self.bbox_head.num_classes, self.bbox_head.reg_class_agnostic, self.bbox_head.target_means,
                                          self.bbox_head.target_stds, self.global_head.dim_coder.target_means, self.global_head.dim_coder.target_stds)
            self.last_positive_stage = 'launch' if pos.launched else 'torch'
        elif self.bbox_refined_assigner is not None and self.bbox_refined_sampler is not None:
            # refine bboxes like Cascade R-CNN
            pos_is_gts = [res.pos_is_gt for res in sampling_results]
            with torch.no_grad():
                roi_labels = torch.where(roi_labels == self.bbox_head.num_classes, bbox_results['cls_score'][:, :-1].argmax(1), roi_labels)
                proposal_list = self.bbox_head.refine_bboxes(bbox_results['rois'], roi_labels, bbox_results['bbox_pred'], pos_is_gts, img_metas)
            # assign and sample for 3D R-CNN
            sampling_results = []
            for i in range(num_imgs):
                assign_result = self.bbox_refined_assigner.assign(proposal_list[i], gt_bboxes[i], gt_bboxes_ignore[i], gt_labels[i])
                sampling_results.append(self.bbox_refined_sampler.sample(assign_result, proposal_list[i], gt_bboxes[i], gt_labels[i],
                                                                         generator=generator, feats=[lvl_feat[i][None] for lvl_feat in x]))
        else:
            # only refine pos bboxes (without filtering gts) and do not resample
            with torch.no_grad():
                for i, img_meta in enumerate(img_metas):
                    mask = bbox_results['rois'][:, 0] == i
                    roi_labels_i = roi_labels[mask]
                    pos_keep = roi_labels_i < self.bbox_head.num_classes
                    pos_rois = bbox_results['rois'][mask, 1:][pos_keep]
                    pos_bbox_pred = bbox_results['bbox_pred'][mask][pos_keep]
                    pos_label = roi_labels_i[pos_keep]
                    pos_bboxes = self.bbox_head.regress_by_class(pos_rois, pos_label, pos_bbox_pred, img_meta)
                    sampling_results[i].bboxes[pos_keep] = pos_bboxes
                    sampling_results[i].pos_bboxes = pos_bboxes

        # reg head forward and loss
        reg_results = self._reg_forward_train(x, sampling_results, gt_bboxes_3d, gt_labels, positives=pos)
        losses.update(reg_results['loss_reg'])

        # noc head forward and loss
        if pos is not None:
            flip = pos.flip
        else:
            flip = []
            for img_meta, res in zip(img_metas, sampling_results):
                flip += [img_meta['flip']] * len(res.pos_inds)
        fused_decode = pos is not None and self.train_decode_reason() is None
        self.last_train_decode = 'fused' if fused_decode else 'literal'
        noc_results = self._noc_forward_train(x, sampling_results, reg_results['latent_pred'], reg_results['latent_var'], gt_coords_3d,
                                              gt_coords_3d_mask, gt_bboxes_3d, img_metas, flip, positives=pos, fused_decode=fused_decode)
        losses.update(noc_results['loss_noc'])

        # decode coords_3d and get coords_2d
        decoded_logstd = None
        if fused_decode:
            # the fast path: dimensions, object coordinates and the pixel log-std from the raw output in one launch (and one backward)
            kw = self._decode_kw(None)
            kw.pop('coord_2d')
            dec = decode_for_training(noc_results['all_pred'], pos.pos_gt_labels, flip, reg_results['dim_pred'], reg_results['dim_var'],
                                      self._pos_distances(pos.pos_bboxes_3d), distance_min=self.projection_head.proj_error_coder.distance_min, **kw)
            dimensions_pred, coords_3d_pred, coords_3d_var, decoded_logstd = dec['dims'], dec['coords_3d'], dec['coords_3d_var'], dec['proj_logstd_px']
        elif self.with_projection or self.with_pose:
            dimensions_pred, dimensions_var = self.global_head.dim_coder.decode(reg_results['dim_pred'], reg_results['dim_var'],
                                                                                reg_results['pos_gt_labels'])
            coords_3d_pred, coords_3d_var = self.noc_head.coord_coder.decode(noc_results['noc_pred'], noc_results['noc_var'], dimensions_pred,
                                                                             dimensions_var, flip)
        if self.with_projection or self.with_pose:
            size = tuple(noc_results['noc_pred'].shape[-2:])
            if noc_results['rois'].size(0) == 0:
                coords_2d_roi = noc_results['noc_pred'].new_zeros((0, 2) + size)
            elif coord_2d.device.type == 'cuda':
                coords_2d_roi = roi_align_avg(coord_2d, noc_results['rois'], size, 1.0, 0, True).to(noc_results['noc_pred'].dtype)
            else:                                       # the launch's arithmetic in torch ops: the host has no roi_align_avg
                coords_2d_roi = roi_align_avg_torch(coord_2d, noc_results['rois'], size)
        else:
            coords_3d_pred = coords_3d_var = dimensions_pred = coords_2d_roi = None

        # projection head forward and loss
        if self.with_projection:
            projection_results = self._projection_forward_train(coords_3d_pred, noc_results['proj_logstd'], coords_3d_var, sampling_results,
                                                                coords_2d_roi, cam_intrinsic, gt_bboxes_3d, img_metas, positives=pos,
                                                                decoded_logstd=decoded_logstd)
            losses.update(projection_results['loss_proj'])
        else:
            projection_results = dict(proj_logstd=noc_results['proj_logstd'])

        if self.with_pose:
            pose_results = self._pose_forward_train(coords_2d_roi, projection_results['proj_logstd'], coords_3d_pred, dimensions_pred,
                                                    projection_results['img_shapes'], projection_results['pos_bboxes_3d'],
                                                    projection_results['pos_cam_intrinsic'])
            losses.update(pose_results['loss_pose'])
            if self.with_score:
                score_results = self._score_forward_train(
                    reg_results['reg_fc_out'], pose_results['ret_val'], pose_results['yaw_pred'], pose_results['t_vec_pred'],
                    pose_results['pose_cov_calib'] if cfg_get(self.train_cfg, 'calib_scoring', False) else pose_results['pose_cov_pred'],
                    dimensions_pred, pose_results['ious'])
                losses.update(score_results['loss_score'])
        return losses

    def _bbox_forward_train(self, x, sampling_results, gt_bboxes, gt_labels, rcnn_train_cfg):
        """Run forward function and calculate loss for box head in training: an image's rows are its positives, then its negatives."""
        rois = bbox2roi([res.bboxes for res in sampling_results])
        bbox_results = self._bbox_forward(x, rois)
        bbox_targets = self.bbox_head.get_targets(sampling_results, gt_bboxes, gt_labels, self.train_cfg)
        loss_bbox = self.bbox_head.loss(bbox_results['cls_score'], bbox_results['bbox_pred'], rois, *bbox_targets)
        bbox_results.update(loss_bbox=loss_bbox, rois=rois, bbox_targets=bbox_targets)
        return bbox_results

    def _reg_forward_train(self, x, sampling_results, gt_bboxes_3d, gt_labels, positives=None):
        """``positives``: the fast path's launch results, which replace the walks over ``sampling_results`` (here and below)."""
        if positives is not None:
            pos_rois, pos_gt_labels = positives.pos_rois, positives.pos_gt_labels
            reg_targets = (positives.dim_targets, None)
        else:
            pos_rois = bbox2roi([res.pos_bboxes for res in sampling_results])
            pos_gt_labels = torch.cat([res.pos_gt_labels for res in sampling_results], dim=0)
            reg_targets = self.global_head.get_targets(sampling_results, gt_bboxes_3d, gt_labels)
        reg_results = self._reg_forward(x, pos_rois, pos_gt_labels)
        loss_reg = self.global_head.loss(reg_results['dim_pred'], reg_results['distance_pred'], reg_results['distance_logstd'], *reg_targets)
        if reg_results['distance_pred'] is not None and reg_results['distance_pred'].size(1):
            distance_pred, distance_logstd = reg_results['distance_pred'], reg_results['distance_logstd']
            if not self.global_head.reg_decoded_distance:
                distance_pred, distance_logstd = self.global_head.distance_coder.decode(distance_pred, distance_logstd)
        else:
            distance_pred = distance_logstd = None
        reg_results.update(loss_reg=loss_reg, distance_pred=distance_pred, distance_logstd=distance_logstd, pos_gt_labels=pos_gt_labels)
        if self.debug:
            reg_results['dim_pred'] = reg_targets[0]
        return reg_results

    def _noc_forward_train(self, x, sampling_results, latent_pred, latent_var, gt_coords_3d, gt_coords_3d_mask, gt_bboxes_3d, img_metas, flip,
                           positives=None, fused_decode=False):
        if positives is not None:
            pos_rois, pos_labels = positives.pos_rois, positives.pos_gt_labels
            # what get_targets reads of a sampling result, as views of the launch's rows
            sampling_results = [types.SimpleNamespace(pos_bboxes=b, pos_assigned_gt_inds=g) for b, g in
                                zip(positives.per_image('pos_bboxes'), positives.per_image('pos_assigned_gt_inds'))]
        else:
            pos_rois = bbox2roi([res.pos_bboxes for res in sampling_results])
            pos_labels = torch.cat([res.pos_gt_labels for res in sampling_results])
        if fused_decode:
            # the trunk alone: the raw output feeds decode_for_training; the class's channels of the flip branch, which loss_noc and
            # loss_proj read, are the selections the head's own forward makes
            noc_feats = self.noc_roi_extractor(x[:self.noc_roi_extractor.num_inputs], pos_rois)
            all_pred = self.noc_head.forward_all_pred(noc_feats, latent_pred, latent_var)
            n, ch, h, w = all_pred.shape
            branch = all_pred.view(n, 2, ch // 2, h, w)[torch.arange(n, device=all_pred.device), flip.long()]
            noc_pred, noc_var, proj_logstd = self.noc_head.slice_pred(branch, pos_labels)
            noc_results = dict(noc_pred=noc_pred, noc_var=noc_var, proj_logstd=proj_logstd, regular_params=None, rois=pos_rois, all_pred=all_pred)
        else:
            noc_results = self._noc_forward(x, pos_rois, latent_pred, latent_var, pos_labels, flip)
        if self.noc_head.loss_noc is not None:
            noc_targets, noc_weights = self.noc_head.get_targets(sampling_results, gt_coords_3d, gt_coords_3d_mask, gt_bboxes_3d, self.train_cfg,
                                                                 img_metas)
            loss_noc = self.noc_head.loss(noc_results['noc_pred'], noc_targets, noc_weights)
            if self.debug:
                noc_results['noc_pred'] = noc_targets
                noc_results['proj_logstd'] = (1 / noc_weights.clamp(min=1e-6, max=1e6)).log().repeat(1, 2, 1, 1)
        else:
            loss_noc = dict()
        noc_results.update(loss_noc=loss_noc)
        return noc_results

    def _projection_forward_train(self, coords_3d_pred, proj_logstd, coords_3d_var, sampling_results, coords_2d_roi, cam_intrinsic,
                                  gt_bboxes_3d, img_metas, positives=None, decoded_logstd=None):
        """``decoded_logstd``: the pixel log-std ``decode_for_training`` already made of ``proj_logstd`` (the fast path), in place of
        :meth:`_projection_decode`."""
        if positives is not None:
            pos_cam_intrinsic, pos_bboxes_3d, img_shapes = positives.pos_cam_intrinsic, positives.pos_bboxes_3d, positives.img_shapes
            pos_distances = self._pos_distances(pos_bboxes_3d)
        else:
            pos_cam_intrinsic, pos_bboxes_3d, pos_distances, img_shapes = self.projection_head.get_properties(
                sampling_results, cam_intrinsic, gt_bboxes_3d, img_metas)
        coords_2d_proj = self.projection_head(coords_3d_pred, pos_bboxes_3d[:, 3:7], pos_cam_intrinsic, img_shapes)
        loss_proj = self.projection_head.loss(coords_2d_proj, proj_logstd, coords_2d_roi, pos_distances)
        projection_results = dict(loss_proj=loss_proj, img_shapes=img_shapes, pos_bboxes_3d=pos_bboxes_3d, pos_cam_intrinsic=pos_cam_intrinsic,
                                  pos_distances=pos_distances)
        if decoded_logstd is not None:
            projection_results.update(proj_logstd=decoded_logstd)
        else:
            projection_results.update(self._projection_decode(proj_logstd, coords_3d_var, pos_distances))
        return projection_results

    def _pose_forward_train(self, coords_2d, proj_logstd, coords_3d_pred, dimensions_pred, img_shapes, pos_bboxes_3d, pos_cam_intrinsic):
        pose_results = self._pose_forward(coords_2d, proj_logstd, coords_3d_pred, pos_cam_intrinsic, img_shapes)
        yaw_targets, trans_targets = self.pose_head.get_targets(pos_bboxes_3d)
        loss_pose, ious = self.pose_head.loss(pose_results['ret_val'], pose_results['yaw_pred'], pose_results['t_vec_pred'],
                                              pose_results['pose_cov_calib'], dimensions_pred, yaw_targets, trans_targets, pos_bboxes_3d)
        pose_results.update(loss_pose=loss_pose, ious=ious)
        return pose_results

    def _score_forward_train(self, reg_fc_out, ret_val, yaw, t_vec, pose_cov, dimensions, ious):
        score_results = self._score_forward(reg_fc_out[ret_val], yaw[ret_val], t_vec[ret_val], pose_cov[ret_val], dimensions[ret_val])
        loss_score = self.score_head.loss(score_results['scores'], ious[ret_val])
        score_results.update(loss_score=loss_score)
        return score_results

    async def async_simple_test(self, *args, **kwargs):
        raise NotImplementedError

    def aug_test(self, *args, **kwargs):
        raise NotImplementedError

    # ------------------------------------------------------------------------------------------------ the reference's stage methods
    def _bbox_forward(self, x, rois):
        bbox_feats = self.bbox_roi_extractor(x[:self.bbox_roi_extractor.num_inputs], rois)
        cls_score, bbox_pred = self.bbox_head(bbox_feats)
        return dict(cls_score=cls_score, bbox_pred=bbox_pred, bbox_feats=bbox_feats)

    def _reg_forward(self, x, rois, labels):
        reg_feats = self.bbox_roi_extractor(x[:self.bbox_roi_extractor.num_inputs], rois)
        dim_latent_pred, dim_latent_var, distance_pred, distance_logstd, reg_fc_out = self.global_head(reg_feats)
        dim_pred, dim_var, latent_pred, latent_var = self.global_head.slice_pred(dim_latent_pred, dim_latent_var, labels)
        return dict(dim_pred=dim_pred, dim_var=dim_var, latent_pred=latent_pred, latent_var=latent_var, distance_pred=distance_pred,
                    distance_logstd=distance_logstd, roi_feats=reg_feats, reg_fc_out=reg_fc_out)

    def _noc_forward(self, x, rois, latent_pred, latent_var, labels, flip):
        noc_feats = self.noc_roi_extractor(x[:self.noc_roi_extractor.num_inputs], rois)
        noc_pred, noc_var, proj_logstd, regular_params = self.noc_head(noc_feats, latent_pred, latent_var, labels, flip=flip)
        return dict(noc_pred=noc_pred, noc_var=noc_var, proj_logstd=proj_logstd, regular_params=regular_params, rois=rois)

    def _projection_decode(self, proj_logstd, coords_3d_var, distances=None):
        if self.projection_head.train_std_of_encoded_error:
            proj_logstd = self.projection_head.proj_error_coder.decode_logstd(proj_logstd, coords_3d_var, distances)
        return dict(proj_logstd=proj_logstd)

    def _pose_forward(self, coords_2d, proj_logstd, coords_3d_pred, cam_intrinsic, img_shapes):
        ret_val, yaw_pred, t_vec_pred, pose_cov_pred, pose_cov_calib = self.pose_head(coords_2d, proj_logstd, coords_3d_pred, cam_intrinsic, img_shapes)
        return dict(ret_val=ret_val, yaw_pred=yaw_pred, t_vec_pred=t_vec_pred, pose_cov_pred=pose_cov_pred, pose_cov_calib=pose_cov_calib)

    def _score_forward(self, reg_fc_out, yaw, t_vec, pose_cov, dimensions):
        return dict(scores=self.score_head(reg_fc_out, yaw, t_vec, pose_cov, dimensions))

    def get_bbox_3d_result(self, dimensions, yaw, t_vec, scores, labels, to_np=False):
        return consumers.get_bbox_3d_result(dimensions, yaw, t_vec, scores, labels, self.bbox_head.num_classes, to_np=to_np)

    def multiclass_3d_result_nms(self, bbox_3d_result, nms_thr=0.25, to_np=True):
        return consumers.multiclass_3d_result_nms(bbox_3d_result, nms_thr, to_np=to_np)

    xywhr2xyxyr = staticmethod(consumers.xywhr2xyxyr)

    # ------------------------------------------------------------------------------------------------ inference
    def fast_path_reason(self, x, reg_results, n):
        """None when the fast path serves this call, else the condition that sends it to the literal path (a string)."""
        cfg, ph, nh, gh = self.test_cfg, self.projection_head, self.noc_head, self.global_head
        if not (x[0].device.type == 'cuda' and x[0].dtype == torch.float32):
            return 'the feature maps are not CUDA fp32'
        if reg_results['distance_pred'] is not None and reg_results['distance_pred'].size(1):
            return 'the global head has a distance branch'
        if not ph.train_std_of_encoded_error:
            return 'train_std_of_encoded_error is off: the fused decode always decodes the encoded log-std'
        if cfg_get(cfg, 'cov_correction', False) and ph.distance_mode != 'range':
            return "cov_correction with distance_mode 'z-depth': the fused correction divides by the range"
        if not (isinstance(ph.proj_error_coder, DistanceInvarProjErrorCoder) and isinstance(gh.dim_coder, MultiClassNormDimCoder)
                and isinstance(nh, FCNNOCDecoder) and isinstance(nh.coord_coder, NOCCoder) and isinstance(self.pose_head, UncertPropPnPOptimizer)
                and isinstance(self.score_head, MLPScoreHead)):
            return 'a coder or head the fused decode does not restate'
        if ph.proj_error_coder.distance_min > ph.proj_error_coder.scaling_denomitor:
            return 'distance_min above the reference distance'
        if not (nh.flip_correction and nh.noc_channels == 3 and nh.uncert_channels == 2):
            return 'a NOC head layout other than two flip branches of 3 + 2 channels per class'
        if not self.score_head.pre_sigmoid:
            return 'a score head that returns probabilities'
        if n > consumers.RESULT3D_MAX_N or self.bbox_head.num_classes > consumers.RESULT3D_MAX_CLASSES:
            return 'more detections or classes than the one-launch result tail takes'
        return None

    def _decode_kw(self, coord_2d):
        ph, nh, gh = self.projection_head.proj_error_coder, self.noc_head, self.global_head
        return dict(num_classes=nh.num_classes, class_agnostic=nh.class_agnostic, dim_means=gh.dim_coder.target_means, dim_stds=gh.dim_coder.target_stds,
                    noc_means=nh.coord_coder.target_means, noc_stds=nh.coord_coder.target_stds,
                    # the coder keeps the product ref_length ref_focal_y target_std; the decode takes it as one factor again
                    ref_length=ph.scaling_denomitor / ph.ref_focal_y, ref_focal_y=ph.ref_focal_y, target_std=1.0,
                    epistemic_std_gain=ph.epistemic_std_gain, coord_2d=coord_2d)

    def simple_test(self, x, proposal_list, img_metas, proposals=None, coord_2d=None, cam_intrinsic=None, rescale=False, path=None):
        """The reference's contract (monorun_roi_head.py:442-605): one image; ``x`` its feature maps, ``proposal_list`` its proposals,
        ``coord_2d`` / ``cam_intrinsic`` the per-image lists the pipeline collates; ``test_cfg`` gives ``score_thr`` / ``nms`` /
        ``max_per_img`` of the 2-D stage and ``mult_2d_score``, ``calib_scoring``, ``cov_correction``, ``nms_3d_thr``, ``debug``.
        Returns ``[dict(bbox_results, bbox_3d_results[, oc_maps, std_maps, pose_covs, latent_vecs])]``, numpy arrays per class.

        The two paths (module docstring).  ``path=None`` takes the FAST path when all of these hold and the LITERAL path otherwise
        (:meth:`fast_path_reason` names the first that fails): CUDA fp32 feature maps; a global head without a distance branch; a
        projection head with ``train_std_of_encoded_error`` and, under ``cov_correction``, ``distance_mode='range'``; this package's
        coders and heads with the NOC head's two flip branches of 3 + 2 channels per class; at most ``consumers.RESULT3D_MAX_N``
        detections and ``RESULT3D_MAX_CLASSES`` classes.  ``path='literal'`` forces the literal path; ``path='fast'`` raises where
        the fast path does not apply.  The last path taken is kept in ``self.last_path``.  Inside the fast path,
        ``pose_from_head`` picks its own launches from the pose head's ``pnp`` options, as documented there.  The fast path's results
        agree with the literal path's within the tolerances tests/test_gpu_decode_and_head.py states for ``pose_from_head`` against
        the literal chain; scores that land on the other side of ``nms_3d_thr``'s decisions can therefore differ, as between any two
        fp32 evaluation orders.  Two host synchronisations on the fast path: the number of 2-D detections (the reference branches on
        it too, and it sizes every later tensor: NaN-padded rows are not sent through extractors, heads or solver, none of which
        states a contract for them), and the copy of the packed result."""
        assert self.with_bbox and self.with_noc and self.with_pose and self.with_score
        assert len(img_metas) == 1, 'batch inference is not supported yet'
        assert path in (None, 'fast', 'literal'), path
        img_shape, scale_factor, flip = img_metas[0]['img_shape'], img_metas[0]['scale_factor'], img_metas[0]['flip']
        cfg = self.test_cfg
        num_classes = self.bbox_head.num_classes
        coord_2d = coord_2d[0]
        cam_intrinsic = cam_intrinsic[0][0][None, ...]

        rois = bbox2roi(proposal_list)
        bbox_results = self._bbox_forward(x, rois)
        det_bboxes, det_labels = self.bbox_head.get_bboxes(rois, bbox_results['cls_score'], bbox_results['bbox_pred'], img_shape, scale_factor,
                                                           rescale=rescale, cfg=cfg)
        n = det_bboxes.shape[0]
        debug = cfg_get(cfg, 'debug', False)
        if n == 0:
            self.last_path = 'empty'
            results = dict(bbox_results=bbox2result(det_bboxes, det_labels, num_classes),
                           bbox_3d_results=[np.zeros((0, 8), dtype=np.float32) for _ in range(self.noc_head.num_classes)])
            if debug:
                results.update(oc_maps=[np.zeros((0, 3, 0, 0), dtype=np.float32)] * num_classes,
                               std_maps=[np.zeros((0, self.noc_head.uncert_channels, 0, 0), dtype=np.float32)] * num_classes,
                               pose_covs=[np.zeros((0, 4, 4), dtype=np.float32)] * num_classes,
                               latent_vecs=[np.zeros((0, 16), dtype=np.float32)] * num_classes)
            return [results]
        # if det_bboxes is rescaled to the original image size, rescale it back to the testing scale to obtain RoIs
        _bboxes = det_bboxes[:, :4] * det_bboxes.new_tensor(scale_factor) if rescale else det_bboxes
        bbox_3d_rois = bbox2roi([_bboxes])
        reg_results = self._reg_forward(x, bbox_3d_rois, det_labels)
        why = self.fast_path_reason(x, reg_results, n)
        if path == 'fast' and why is not None:
            raise RuntimeError(f'MonoRUnRoIHead.simple_test(path="fast"): {why}')
        fast = why is None and path != 'literal'
        self.last_path = 'fast' if fast else 'literal'
        mult_2d, calib = cfg_get(cfg, 'mult_2d_score'), cfg_get(cfg, 'calib_scoring', False)
        if fast:
            noc_feats = self.noc_roi_extractor(x[:self.noc_roi_extractor.num_inputs], bbox_3d_rois)
            all_pred = self.noc_head.forward_all_pred(noc_feats, reg_results['latent_pred'], reg_results['latent_var'])
            pose_results = pose_from_head(self.pose_head, all_pred, det_labels, flip, reg_results['dim_pred'], reg_results['dim_var'], bbox_3d_rois,
                                          cam_intrinsic, img_shape, apply_cov_correction=bool(cfg_get(cfg, 'cov_correction', False)),
                                          **self._decode_kw(coord_2d))
            scores = score_poses(self.score_head, reg_results['reg_fc_out'], pose_results, det_scores=det_bboxes[:, -1], calib_scoring=bool(calib),
                                 mult_2d_score=bool(mult_2d))
            bbox_3d_result, keep_inds_3d, bbox_result, keep_rows = consumers.result_3d_nms(
                pose_results['dimensions_pred'], pose_results['yaw_pred'], pose_results['t_vec_pred'], scores, det_labels, det_bboxes, num_classes,
                cfg_get(cfg, 'nms_3d_thr'), to_np=True, with_rows=True)
            results = dict(bbox_results=bbox_result, bbox_3d_results=bbox_3d_result)
            if debug:
                results.update(self._debug_maps_fast(all_pred, det_labels, flip, reg_results, bbox_3d_rois, pose_results, coord_2d, keep_rows))
            return [results]

        bbox_result = bbox2result(det_bboxes, det_labels, num_classes)
        # decode distance
        if reg_results['distance_pred'] is not None and reg_results['distance_pred'].size(1):
            distance_pred, distance_logstd = reg_results['distance_pred'], reg_results['distance_logstd']
            if not self.global_head.reg_decoded_distance:
                distance_pred, distance_logstd = self.global_head.distance_coder.decode(distance_pred, distance_logstd)
        else:
            distance_pred = distance_logstd = None
        dimensions_pred, dimensions_var = self.global_head.dim_coder.decode(reg_results['dim_pred'], reg_results['dim_var'], det_labels)
        noc_results = self._noc_forward(x, bbox_3d_rois, reg_results['latent_pred'], reg_results['latent_var'], det_labels, flip)
        coords_3d_pred, coords_3d_var = self.noc_head.coord_coder.decode(noc_results['noc_pred'], noc_results['noc_var'], dimensions_pred,
                                                                         dimensions_var, flip)
        proj_logstd = self._projection_decode(noc_results['proj_logstd'], coords_3d_var, distance_pred)['proj_logstd']
        coords_2d_roi = roi_align_avg(coord_2d, bbox_3d_rois, noc_results['noc_pred'].shape[-2:], 1.0, 0, True)
        pose_results = self._pose_forward(coords_2d_roi, proj_logstd, coords_3d_pred, cam_intrinsic, cam_intrinsic.new_tensor(img_shape[:2])[None, ...])
        if cfg_get(cfg, 'cov_correction', False):
            distance = self.projection_head.get_distance(pose_results['t_vec_pred'])
            pose_results['pose_cov_calib'] = self.projection_head.proj_error_coder.cov_correction(pose_results['pose_cov_calib'], distance)
        score_results = self._score_forward(reg_results['reg_fc_out'], pose_results['yaw_pred'], pose_results['t_vec_pred'],
                                            pose_results['pose_cov_calib'] if calib else pose_results['pose_cov_pred'], dimensions_pred)
        if self.score_head.pre_sigmoid:
            score_results['scores'].sigmoid_()
        score_results['scores'][~pose_results['ret_val']] = 0
        scores = det_bboxes[:, -1] * score_results['scores'] if mult_2d else score_results['scores']
        bbox_3d_result = self.get_bbox_3d_result(dimensions_pred, pose_results['yaw_pred'], pose_results['t_vec_pred'], scores, det_labels, to_np=False)
        bbox_3d_result, keep_inds_3d = self.multiclass_3d_result_nms(bbox_3d_result, cfg_get(cfg, 'nms_3d_thr'), to_np=True)
        bbox_result = [b[k] for b, k in zip(bbox_result, keep_inds_3d)]
        results = dict(bbox_results=bbox_result, bbox_3d_results=bbox_3d_result)
        if debug:
            results.update(debug_maps(coords_3d_pred, proj_logstd, pose_results['pose_cov_calib'], reg_results['latent_pred'], det_labels,
                                      keep_inds_3d, num_classes))
        return [results]

    def _debug_maps_fast(self, all_pred, det_labels, flip, reg_results, rois, pose_results, coord_2d, keep_rows):
        """``oc_maps``, ``std_maps``, ``pose_covs``, ``latent_vecs`` of the fast path: the maps the fused launch never writes out come from
        one extra ``noc_decode`` launch (std = 1 / (std_scale istd)), gathered by the kept members' rows."""
        from .pose_head import noc_decode
        kw = self._decode_kw(coord_2d)
        dec = noc_decode(all_pred, det_labels, flip, reg_results['dim_pred'], reg_results['dim_var'], rois, std_scale=self.pose_head.std_scale,
                         epnp_ransac_thres_ratio=self.pose_head.epnp_ransac_thres_ratio, **kw)
        oc, std = dec['coords_3d'].cpu().numpy(), (1 / (dec['coords_2d_istd'] * self.pose_head.std_scale)).cpu().numpy()
        cov, latent = pose_results['pose_cov_calib'].cpu().numpy(), reg_results['latent_pred'].cpu().numpy()
        return dict(oc_maps=[oc[r] for r in keep_rows], std_maps=[std[r] for r in keep_rows], pose_covs=[cov[r] for r in keep_rows],
                    latent_vecs=[latent[r] for r in keep_rows])


def debug_maps(coords_3d_pred, proj_logstd, pose_cov_calib, latent_pred, det_labels, keep_inds_3d, num_classes):
    """The reference's debug outputs (monorun_roi_head.py:580-601): per class, the kept members' maps."""
    oc_pred, std = coords_3d_pred.cpu().numpy(), torch.exp(proj_logstd).cpu().numpy()
    pose_cov, labels, latent = pose_cov_calib.cpu().numpy(), det_labels.cpu().numpy(), latent_pred.cpu().numpy()
    out = dict(oc_maps=[], std_maps=[], pose_covs=[], latent_vecs=[])
    for i in range(num_classes):
        mask, keep = labels == i, keep_inds_3d[i]
        out['oc_maps'].append(oc_pred[mask][keep])
        out['std_maps'].append(std[mask][keep])
        out['pose_covs'].append(pose_cov[mask][keep])
        out['latent_vecs'].append(latent[mask][keep])
    return out


def register_with_mmdet(force=False):
    """Put :class:`MonoRUnRoIHead` into mmdet's ``HEADS`` registry; False without mmdet, or (unless ``force``) when the name is taken."""
    try:
        from mmdet.models.builder import HEADS
    except Exception:
        return False
    if HEADS.get('MonoRUnRoIHead') is not None and not force:
        return False
    HEADS.register_module(name='MonoRUnRoIHead', force=True, module=MonoRUnRoIHead)
    return True
