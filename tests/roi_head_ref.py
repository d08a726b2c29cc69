"""Shared by tests/test_roi_head_cpu.py and tests/test_gpu_roi_head.py: a reference-shaped config of the detector at reduced widths
(written here; the reference's config files are not copied), the inputs of one 96 x 320 image, and ``simple_test_ref``: a literal
restatement of the reference's ``simple_test`` (monorun/models/roi_heads/monorun_roi_head.py:454-566) that calls the same public
building blocks the head's fast path uses — ``get_bboxes``, ``pose_from_head``, ``score_poses`` — and then the OLD consumers tail
(``get_bbox_3d_result`` + ``multiclass_3d_result_nms`` + the per-class selection of the 2-D boxes).  The fast path must equal it bit for
bit: what differs between them is the result tail alone."""
import copy

import numpy as np
import torch

IMG_H, IMG_W = 96, 320
NUM_CLASSES = 3
TEST_CFG = dict(
    rpn=dict(nms_pre=200, nms_post=20, max_num=20, nms_thr=0.7, min_bbox_size=0),
    rcnn=dict(score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100, mult_2d_score=True, calib_scoring=True,
              cov_correction=True, nms_3d_thr=0.01))


def extractor(size):
    return dict(type='SingleRoIExtractor', roi_layer=dict(type='RoIAlign', output_size=size, sampling_ratio=0), out_channels=16,
                featmap_strides=[2, 4, 8, 16, 32], finest_scale=20)


def roi_head_cfg(pnp=None, mc=True):
    """ResNet-18 at base_channels 8 feeds 16 FPN channels; fc_out_channels 32"""
    pose_head = dict(type='UncertPropPnPOptimizer')
    if pnp is not None:
        pose_head['pnp'] = pnp
    global_head = dict(type='FCExtractorMonteCarlo', num_samples=4, in_channels=16, fc_out_channels=32, num_classes=NUM_CLASSES, roi_feat_size=7,
                       latent_channels=16) if mc else dict(type='FCExtractor', in_channels=16, fc_out_channels=32, num_classes=NUM_CLASSES,
                                                           roi_feat_size=7, latent_channels=16)
    return dict(
        type='MonoRUnRoIHead',
        bbox_roi_extractor=extractor(7),
        bbox_head=dict(type='Shared2FCBBoxHead', in_channels=16, fc_out_channels=32, roi_feat_size=7, num_classes=NUM_CLASSES),
        noc_roi_extractor=extractor(14),
        noc_head=dict(type='FCNNOCDecoder', num_convs=1, in_channels=16, conv_out_channels=16, num_classes=NUM_CLASSES, latent_channels=16,
                      upsample_cfg=dict(type='carafe', scale_factor=2, up_kernel=5, up_group=1, encoder_kernel=3, encoder_dilation=1,
                                        compressed_channels=8)),
        global_head=global_head,
        projection_head=dict(type='UncertProjectionHead'),
        pose_head=pose_head,
        score_head=dict(type='MLPScoreHead', reg_fc_out_channels=32, pose_fc_out_channels=32, fc_out_channels=16))


def model_cfg(**kw):
    return dict(
        backbone=dict(type='ResNet', depth=18, base_channels=8, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1, norm_eval=True,
                      style='pytorch'),
        neck=dict(type='FPNplus', in_channels=[8, 16, 32, 64], out_channels=16, num_outs=5, num_lower_outs=1),
        rpn_head=dict(type='RPNHeadMod', in_channels=16, feat_channels=16, starting_level=1,
                      anchor_generator=dict(type='AnchorGenerator', scales=[8], ratios=[0.5, 1.0, 2.0], strides=[4, 8, 16, 32, 64])),
        roi_head=roi_head_cfg(**kw))


def build_roi_head(seed=0, test_cfg=None, **kw):
    from monorun_amd.roi_head import MonoRUnRoIHead
    torch.manual_seed(seed)
    cfg = roi_head_cfg(**kw)
    cfg.pop('type')
    head = MonoRUnRoIHead(**cfg, test_cfg=copy.deepcopy(TEST_CFG['rcnn'] if test_cfg is None else test_cfg))
    head.init_weights()
    seed_heads(head, seed)
    return head.eval()


def seed_heads(head, seed):
    """init_weights leaves the regression layers near zero; seeded weights of some size spread the classes and the boxes"""
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in (head.bbox_head.fc_cls, head.bbox_head.fc_reg, head.global_head.fc_reg, head.noc_head.conv_final, head.noc_head.latent_decoder):
            size = 0.05 if m is head.bbox_head.fc_reg else 0.5
            m.weight.copy_(torch.randn(m.weight.shape, generator=g) * size)
            m.bias.copy_(torch.randn(m.bias.shape, generator=g) * size)
        head.pose_head.cov_calib_logscale.copy_(torch.tensor([0.3, -0.2, 0.1, 0.5]))


def build_detector(seed=0, **kw):
    from monorun_amd.detector import MonoRUnDetector
    torch.manual_seed(seed)
    det = MonoRUnDetector(**model_cfg(**kw), test_cfg=copy.deepcopy(TEST_CFG))
    seed_heads(det.roi_head, seed)
    return det.eval()


def image_inputs(dev, seed=0, flip=False, n_proposals=20):
    """feature maps of a 96 x 320 image (strides 2 .. 64), about 20 proposals, the image's coordinate map and camera matrix"""
    from monorun_amd.pose_head import gen_coord_2d
    g = torch.Generator().manual_seed(100 + seed)
    feats = [torch.randn(1, 16, -(-IMG_H // s), -(-IMG_W // s), generator=g).to(dev) for s in (2, 4, 8, 16, 32, 64)]
    rng = np.random.default_rng(seed)
    cx, cy = rng.uniform(30, IMG_W - 30, n_proposals), rng.uniform(20, IMG_H - 20, n_proposals)
    w, h = rng.uniform(16, 90, n_proposals), rng.uniform(12, 50, n_proposals)
    props = np.stack([np.clip(cx - w / 2, 0, IMG_W), np.clip(cy - h / 2, 0, IMG_H), np.clip(cx + w / 2, 0, IMG_W), np.clip(cy + h / 2, 0, IMG_H),
                      rng.uniform(0.3, 1, n_proposals)], 1).astype(np.float32)
    metas = [dict(img_shape=(IMG_H, IMG_W, 3), ori_shape=(IMG_H * 2, IMG_W * 2, 3), pad_shape=(IMG_H, IMG_W, 3), scale_factor=np.array([0.5, 0.5, 0.5, 0.5], np.float32),
                  flip=flip)]
    coord = gen_coord_2d(IMG_H, IMG_W, flip=flip, device=dev)                                         # (1, 2, 96, 320)
    K = torch.tensor([[[[360.0, 0.0, 160.0], [0.0, 360.0, 48.0], [0.0, 0.0, 1.0]]]], device=dev)       # [aug][image] -> (3, 3)
    return dict(x=feats, proposal_list=[torch.from_numpy(props).to(dev)], img_metas=metas, coord_2d=[coord], cam_intrinsic=[K[0]])


def with_canned_noc_head(head, inputs, mask_seed, seed=0):
    """Replace ``head.noc_head`` by one whose ``forward_all_pred`` returns a fixed output: for the head's own detections on ``inputs``, object
    coordinates that project EXACTLY onto each RoI's pixel grid under a seeded pose (a smooth surface with 5 % depth relief in front of
    the camera), encoded back through the NOC and dimension coders into the class's channels of the unflipped branch; seeded noise
    elsewhere.  A random trunk's output is no object at all: its PnP problems have posterior deviations of metres to kilometres (measured
    on this model: up to 2.7 km in z), so two evaluation orders of the same maps land centimetres apart.  With this head every
    detection is a well-posed problem, which is what the bars on the pose are stated for."""
    from monorun_amd.bbox_head import bbox2roi
    from monorun_amd.noc_decoder import FCNNOCDecoder
    from monorun_amd.pose_head import roi_align_avg

    class CannedNOCHead(FCNNOCDecoder):
        canned = None

        def forward_all_pred(self, x, latent_pred, latent_var=None):
            assert x.size(0) == self.canned.size(0)
            return self.canned

    metas = inputs['img_metas']
    assert not metas[0]['flip']
    dev = inputs['x'][0].device
    with torch.no_grad():
        torch.manual_seed(mask_seed)
        rois = bbox2roi(inputs['proposal_list'])
        br = head._bbox_forward(inputs['x'], rois)
        det, lab = head.bbox_head.get_bboxes(rois, br['cls_score'], br['bbox_pred'], metas[0]['img_shape'], metas[0]['scale_factor'], rescale=False,
                                             cfg=head.test_cfg)
        r3 = bbox2roi([det])
        reg = head._reg_forward(inputs['x'], r3, lab)
        dims, _ = head.global_head.dim_coder.decode(reg['dim_pred'], reg['dim_var'], lab)
        c2 = roi_align_avg(inputs['coord_2d'][0], r3, (28, 28), 1.0, 0, True)
    n, C = len(lab), head.noc_head.num_classes
    K = inputs['cam_intrinsic'][0][0]
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    g = torch.Generator().manual_seed(500 + seed)
    yaw = ((torch.rand(n, generator=g) * 2 - 1) * np.pi).to(dev)
    z0 = (fy * 1.6 / (det[:, 3] - det[:, 1]).clamp(min=4.0)).clamp(4.0, 60.0)
    ramp = torch.cos(np.pi * torch.arange(28, device=dev) / 27)
    d = z0[:, None, None] * (1 + 0.05 * ramp[None, :, None] * ramp[None, None, :])
    cam = torch.stack((d * (c2[:, 0] - cx) / fx, d * (c2[:, 1] - cy) / fy, d), 1)                       # (n, 3, 28, 28)
    v = cam - cam.mean((2, 3), keepdim=True)
    c, s = torch.cos(yaw)[:, None, None], torch.sin(yaw)[:, None, None]
    obj = torch.stack((c * v[:, 0] - s * v[:, 2], v[:, 1], s * v[:, 0] + c * v[:, 2]), 1)             # R_y(yaw)^T (X_cam - t)
    coder = head.noc_head.coord_coder
    noc = (obj / dims[:, :, None, None] - obj.new_tensor(coder.target_means)[:, None, None]) / obj.new_tensor(coder.target_stds)[:, None, None]
    all_pred = (0.1 * torch.randn(n, 2 * C * 5, 28, 28, generator=g)).to(dev)
    ar = torch.arange(n, device=dev)
    for k in range(3):
        all_pred[ar, lab * 3 + k] = noc[:, k]
    for k in range(2):
        all_pred[ar, C * 3 + lab * 2 + k] = -1.0
    cfg = roi_head_cfg()['noc_head']
    cfg.pop('type')
    canned = CannedNOCHead(**cfg)
    canned.load_state_dict(head.noc_head.state_dict())
    canned.canned = all_pred.contiguous()
    head.noc_head = canned.to(dev).eval()
    return head


def simple_test_ref(head, x, proposal_list, img_metas, coord_2d=None, cam_intrinsic=None, rescale=False):
    """monorun_roi_head.py:454-566 over the package's building blocks, ending in the old consumers tail"""
    from monorun_amd import consumers
    from monorun_amd.bbox_head import bbox2result, bbox2roi
    from monorun_amd.pose_head import pose_from_head
    from monorun_amd.roi_head import cfg_get, debug_maps
    from monorun_amd.score_head import score_poses
    img_shape, scale_factor, flip = img_metas[0]['img_shape'], img_metas[0]['scale_factor'], img_metas[0]['flip']
    cfg = head.test_cfg
    C = head.bbox_head.num_classes
    coord_2d = coord_2d[0]
    cam_intrinsic = cam_intrinsic[0][0][None, ...]
    rois = bbox2roi(proposal_list)
    bbox_results = head._bbox_forward(x, rois)
    det_bboxes, det_labels = head.bbox_head.get_bboxes(rois, bbox_results['cls_score'], bbox_results['bbox_pred'], img_shape, scale_factor,
                                                       rescale=rescale, cfg=cfg)
    bbox_result = bbox2result(det_bboxes, det_labels, C)
    if det_bboxes.shape[0] == 0:
        return [dict(bbox_results=bbox_result, bbox_3d_results=[np.zeros((0, 8), dtype=np.float32) for _ in range(C)])], det_labels
    _bboxes = det_bboxes[:, :4] * det_bboxes.new_tensor(scale_factor) if rescale else det_bboxes
    bbox_3d_rois = bbox2roi([_bboxes])
    reg = head._reg_forward(x, bbox_3d_rois, det_labels)
    noc_feats = head.noc_roi_extractor(x[:head.noc_roi_extractor.num_inputs], bbox_3d_rois)
    all_pred = head.noc_head.forward_all_pred(noc_feats, reg['latent_pred'], reg['latent_var'])
    pose = pose_from_head(head.pose_head, all_pred, det_labels, flip, reg['dim_pred'], reg['dim_var'], bbox_3d_rois, cam_intrinsic, img_shape,
                          apply_cov_correction=bool(cfg_get(cfg, 'cov_correction', False)), **head._decode_kw(coord_2d))
    scores = score_poses(head.score_head, reg['reg_fc_out'], pose, det_scores=det_bboxes[:, -1], calib_scoring=bool(cfg_get(cfg, 'calib_scoring', False)),
                         mult_2d_score=bool(cfg_get(cfg, 'mult_2d_score')))
    res = consumers.get_bbox_3d_result(pose['dimensions_pred'], pose['yaw_pred'], pose['t_vec_pred'], scores, det_labels, C, to_np=False)
    res, keep = consumers.multiclass_3d_result_nms(res, cfg_get(cfg, 'nms_3d_thr'), to_np=True)
    out = dict(bbox_results=[b[k] for b, k in zip(bbox_result, keep)], bbox_3d_results=res)
    if cfg_get(cfg, 'debug', False):
        from monorun_amd.pose_head import noc_decode
        dec = noc_decode(all_pred, det_labels, flip, reg['dim_pred'], reg['dim_var'], bbox_3d_rois, std_scale=head.pose_head.std_scale,
                         epnp_ransac_thres_ratio=head.pose_head.epnp_ransac_thres_ratio, **head._decode_kw(coord_2d))
        logstd = torch.log(1 / (dec['coords_2d_istd'] * head.pose_head.std_scale))
        maps = debug_maps(dec['coords_3d'], logstd, pose['pose_cov_calib'], reg['latent_pred'], det_labels, keep, C)
        maps['std_maps'] = [(1 / (dec['coords_2d_istd'] * head.pose_head.std_scale)).cpu().numpy()[det_labels.cpu().numpy() == i][keep[i]] for i in range(C)]
        out.update(maps)
    return [out], det_labels
