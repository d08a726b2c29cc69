#!/usr/bin/env python3
"""G15: the NOC head's projection head and its loss (uncert_projection_head.py, robust_kl_loss.py, distance_invar_proj_error_coder.py),
from the reference's own code.

Runs only in the authoring container (needs the reference tree, read-only; loaded by file path under the mmcv / mmdet stubs of
make_golden.py, nothing of it is copied).  The fixture is data: seeded inputs and what the reference's functions returned for them.

    python tests/golden/make_golden_projection.py      # rewrites tests/golden/g15_projection_loss.npz

Group A: 24 objects at 28x28 in two images (12 positives each), their properties from the reference's get_properties (range and
z-depth).  Group B: 6 objects at 7x9.  coords_3d, proj_logstd and coords_3d_var hold float16-representable values (stored as
float16, used as float32: lossless, half the size); coords_2d_roi is oracle.roi_grid(rois).  The inputs include points behind z_min,
projections beyond both borders on both axes, logstd < ln(1e-4) (the inverse-std clamp) and encoded errors on both sides of delta.

Recorded with the head's defaults (RobustKLLoss momentum 0.1, target_std 0.15), training mode: forward A; loss 1 (A) with the
gradients to coords_3d and proj_logstd; forward and loss 2 (B) with its gradients; loss 3 (A again); the buffer after each; then
one eval-mode loss (A).  Also decode_logstd with the ground-truth range distances (with and without coords_3d_var, first 6 objects
of A), with distance None, and get_distance in both modes.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as mg  # noqa: E402
from make_golden_pose_loss import _weighted_loss  # noqa: E402
from oracle import oracle as orc  # noqa: E402

OUT = HERE


def load():
    mg.install_stubs()
    for p in ('monorun', 'monorun.core', 'monorun.core.bbox_3d', 'monorun.core.bbox_3d.proj_error_coder', 'monorun.models',
              'monorun.models.losses', 'monorun.models.roi_heads', 'monorun.models.roi_heads.bbox_3d_heads',
              'monorun.models.roi_heads.bbox_3d_heads.reprojection_heads'):
        mg._pkg(p)
    bld = mg._load('monorun.core.bbox_3d.builder', 'core/bbox_3d/builder.py')
    coder = mg._load('monorun.core.bbox_3d.proj_error_coder.distance_invar_proj_error_coder',
                     'core/bbox_3d/proj_error_coder/distance_invar_proj_error_coder.py')
    losses_reg = mg._Registry('losses')
    mdm = sys.modules['mmdet.models']
    mdm.LOSSES, mdm.weighted_loss = losses_reg, _weighted_loss
    mg._load('monorun.models.losses.robust_kl_loss', 'models/losses/robust_kl_loss.py')
    sys.modules['mmdet.models.builder'].build_loss = lambda cfg: mg._build_from_cfg(cfg, losses_reg)
    sys.modules['monorun.core'].build_proj_error_coder = lambda cfg: mg._build_from_cfg(cfg, bld.PROJ_ERROR_CODERS)
    head = mg._load('monorun.models.roi_heads.bbox_3d_heads.reprojection_heads.uncert_projection_head',
                    'models/roi_heads/bbox_3d_heads/reprojection_heads/uncert_projection_head.py')
    return head, coder


def f16(a):
    return np.asarray(a, np.float32).astype(np.float16)


def make_objects(rng, n, h, w, per_image=None):
    """GT boxes [l, h, w, x, y, z, yaw], K, image shapes [H, W], rois, object coordinates, logstd, coords_3d_var (n, ...)."""
    dims = rng.uniform([3.2, 1.4, 1.5], [4.6, 1.8, 1.8], (n, 3))
    t = np.stack([rng.uniform(-12, 12, n), rng.uniform(1.0, 2.0, n), rng.uniform(5, 45, n)], 1)
    t[0] = [0.5, 1.5, 1.0]                  # near the camera: part of the object is behind z_min
    t[1] = [-3.0, 1.2, 0.9]
    t[2] = [9.0, 1.6, 2.0]                  # beyond the right border (u > W + 200), and below (v > H + 200)
    t[3] = [-9.0, -1.4, 2.2]                # beyond the left border (u < -200), and above (v < -200)
    yaw = rng.uniform(-np.pi, np.pi, n)
    gt = np.concatenate([dims, t, yaw[:, None]], 1).astype(np.float32)
    K = np.tile(np.array([[721.5377, 0.0, 609.5593], [0.0, 721.5377, 172.854], [0.0, 0.0, 1.0]]), (n, 1, 1))
    K[:, 0, 0] += rng.normal(0, 5, n); K[:, 1, 1] = K[:, 0, 0]; K[:, :2, 2] += rng.normal(0, 3, (n, 2))
    img = np.where(rng.random(n)[:, None] < 0.5, [375.0, 1242.0], [370.0, 1224.0])
    if per_image:                            # blocks of per_image objects share an image: one camera, one image shape
        first = np.arange(n) // per_image * per_image
        K, img = K[first], img[first]
    # RoI: the box around the projected centre, roughly the object's size
    zc = np.maximum(t[:, 2], 0.5)
    u0 = K[:, 0, 0] * t[:, 0] / zc + K[:, 0, 2]; v0 = K[:, 1, 1] * (t[:, 1] - dims[:, 1] / 2) / zc + K[:, 1, 2]
    half = 0.5 * K[:, 0, 0][:, None] * np.stack([dims[:, 0], dims[:, 1]], 1) / zc[:, None] * rng.uniform(0.8, 1.2, (n, 2))
    rois = np.stack([u0 - half[:, 0], v0 - half[:, 1], u0 + half[:, 0], v0 + half[:, 1]], 1).astype(np.float32)
    # object coordinates: the RoI grid back-projected to a depth inside the box, then noise (~0.15 m) and 5 % gross outliers
    grid = orc.roi_grid(rois, h, w).astype(np.float64)
    depth = t[:, 2, None, None] + rng.uniform(-0.5, 0.5, (n, h, w)) * dims[:, 0, None, None]
    cam = np.stack([(grid[:, 0] - K[:, 0, 2, None, None]) * depth / K[:, 0, 0, None, None],
                    (grid[:, 1] - K[:, 1, 2, None, None]) * depth / K[:, 1, 1, None, None], depth], 1) - t[:, :, None, None]
    c, s = np.cos(yaw)[:, None, None], np.sin(yaw)[:, None, None]
    c3d = np.stack([c * cam[:, 0] - s * cam[:, 2], cam[:, 1], s * cam[:, 0] + c * cam[:, 2]], 1)      # R_y(yaw)^T (X - t)
    c3d += rng.normal(0, 0.15, (n, 3, h, w))
    out = rng.random((n, h, w)) < 0.05
    c3d[:, 0][out] += rng.normal(0, 1.5, out.sum()); c3d[:, 2][out] += rng.normal(0, 1.5, out.sum())
    # logstd around 0 with a tail below ln(1e-4), where the inverse std is clamped
    ls = rng.normal(-0.2, 1.0, (n, 2, h, w))
    low = rng.random((n, 2, h, w)) < 0.005
    ls[low] = rng.uniform(-11.0, -9.4, low.sum())
    var = np.exp(rng.normal(-4.0, 1.0, (n, 3, h, w)))
    return gt, K.astype(np.float32), img.astype(np.float32), rois, f16(c3d), f16(ls), f16(var)


def main():
    href, cref = load()
    rng = np.random.default_rng(1515)
    out = {}
    gtA, KA, imgA, roisA, c3dA, lsA, varA = make_objects(rng, 24, 28, 28, per_image=12)
    gtB, KB, imgB, roisB, c3dB, lsB, varB = make_objects(rng, 6, 7, 9)
    # two images of group A: the reference's get_properties picks the positives' ground truth, camera and image shape
    # per image: one camera, one image shape (as in training), 12 positives assigned to its 12 boxes in a shuffled order
    res = [types.SimpleNamespace(pos_inds=torch.arange(12), pos_assigned_gt_inds=torch.from_numpy(rng.permutation(12))) for _ in range(2)]
    gt_imgs = [torch.from_numpy(gtA[:12]), torch.from_numpy(gtA[12:])]
    k_imgs = torch.from_numpy(np.stack([KA[0], KA[12]]))
    metas = [dict(img_shape=(int(imgA[0, 0]), int(imgA[0, 1]), 3)), dict(img_shape=(int(imgA[12, 0]), int(imgA[12, 1]), 3))]
    for mode in ('range', 'z-depth'):
        h = href.UncertProjectionHead(distance_mode=mode)
        pk, pb, pd, pim = h.get_properties(res, k_imgs, gt_imgs, metas)
        out[f'prop_{mode}_k'], out[f'prop_{mode}_bboxes_3d'] = pk.numpy(), pb.numpy()
        out[f'prop_{mode}_distances'], out[f'prop_{mode}_img_shapes'] = pd.numpy(), pim.numpy()
        out[f'get_distance_{mode}'] = h.get_distance(torch.from_numpy(gtA[:, 3:6])).numpy()
    out.update(A_gt_imgs=gtA, A_k_imgs=k_imgs.numpy(), A_img_shapes_imgs=np.array([m['img_shape'][:2] for m in metas], np.float32),
               A_pos_assigned_gt_inds=np.stack([r.pos_assigned_gt_inds.numpy() for r in res]))
    KA_, poseA_, imgA_, distA = (out['prop_range_k'], out['prop_range_bboxes_3d'], out['prop_range_img_shapes'], out['prop_range_distances'])
    poseA = poseA_[:, 3:7]
    order = np.concatenate([res[0].pos_assigned_gt_inds.numpy(), 12 + res[1].pos_assigned_gt_inds.numpy()])     # positive -> object
    assert np.array_equal(poseA_, gtA[order]) and np.array_equal(KA_, KA[order])
    c3dA, lsA, varA, roisA = c3dA[order], lsA[order], varA[order], roisA[order]

    head = href.UncertProjectionHead()
    head.train()
    assert abs(head.proj_error_coder.scaling_denomitor - 1.6 * 722 * 0.15) < 1e-9

    def run(c3d, ls, pose, K, img, rois, dist, h, w, grads):
        tc = torch.from_numpy(c3d.astype(np.float32)).requires_grad_(grads)
        tl = torch.from_numpy(ls.astype(np.float32)).requires_grad_(grads)
        proj = head(tc, torch.from_numpy(pose), torch.from_numpy(K), torch.from_numpy(img))
        roi = torch.from_numpy(orc.roi_grid(rois, h, w))
        loss = head.loss(proj, tl, roi, torch.from_numpy(dist))['loss_proj']
        g = None
        if grads:
            loss.backward()
            g = (tc.grad.numpy(), tl.grad.numpy())
        return proj.detach().numpy(), float(loss.item()), float(head.loss_proj.mean_inv_std.item()), g

    projA, l1, b1, gA = run(c3dA, lsA, poseA, KA_, imgA_, roisA, distA, 28, 28, True)
    distB = np.linalg.norm(gtB[:, 3:6], axis=1, keepdims=True).astype(np.float32)
    projB, l2, b2, gB = run(c3dB, lsB, gtB[:, 3:7], KB, imgB, roisB, distB, 7, 9, True)
    _, l3, b3, _ = run(c3dA, lsA, poseA, KA_, imgA_, roisA, distA, 28, 28, False)
    head.eval()
    _, le, be, _ = run(c3dA, lsA, poseA, KA_, imgA_, roisA, distA, 28, 28, False)
    assert be == b3
    # what the inputs cover
    z = np.einsum('nij,njhw->nihw', np.stack([np.array([[np.cos(y), 0, np.sin(y)], [0, 1, 0], [-np.sin(y), 0, np.cos(y)]]) for y in poseA[:, 3]]),
                  c3dA.astype(np.float64))[:, 2] + poseA[:, 2, None, None]
    enc = np.abs((projA - orc.roi_grid(roisA, 28, 28)) * distA[:, :, None, None] / (1.6 * 722 * 0.15))
    dw = enc * np.minimum(np.exp(-lsA.astype(np.float64)), 1e4)
    print('behind z_min:', int((z < 0.5).sum()), 'u < -200:', int((projA[:, 0] == -200).sum()), 'u > W+200:',
          int((projA[:, 0] == imgA_[:, 1, None, None] + 200).sum()), 'v < -200:', int((projA[:, 1] == -200).sum()),
          'v > H+200:', int((projA[:, 1] == imgA_[:, 0, None, None] + 200).sum()), 'clamped inv:', int((lsA < np.log(1e-4)).sum()),
          'dw < delta:', int((dw < 1.414).sum()), 'dw >= delta:', int((dw >= 1.414).sum()))
    out.update(A_coords_3d=c3dA, A_proj_logstd=lsA, A_rois=roisA, A_pose=poseA, A_cam_intrinsic=KA_, A_img_shapes=imgA_, A_distances=distA,
               A_coords_2d_proj=projA, A_grad_coords_3d=gA[0], A_grad_proj_logstd=gA[1],
               B_coords_3d=c3dB, B_proj_logstd=lsB, B_rois=roisB, B_pose=gtB[:, 3:7], B_cam_intrinsic=KB, B_img_shapes=imgB, B_distances=distB,
               B_coords_2d_proj=projB, B_grad_coords_3d=gB[0], B_grad_proj_logstd=gB[1],
               train_losses=np.array([l1, l2, l3], np.float32), train_buffers=np.array([b1, b2, b3], np.float32),
               eval_loss=np.float32(le), eval_buffer=np.float32(be))
    # decode_logstd (monorun_roi_head.py:367-372 with the training distances), first 6 objects of A
    c = cref.DistanceInvarProjErrorCoder(target_std=0.15)
    ls6, var6, d6 = (torch.from_numpy(lsA[:6].astype(np.float32)), torch.from_numpy(varA[:6].astype(np.float32)), torch.from_numpy(distA[:6]))
    out.update(dec_coords_3d_var=varA[:6], dec_logstd_var=c.decode_logstd(ls6, var6, d6).numpy(),
               dec_logstd_novar=c.decode_logstd(ls6, None, d6).numpy(), dec_logstd_var_nodist=c.decode_logstd(ls6, var6, None).numpy())
    path = os.path.join(OUT, 'g15_projection_loss.npz')
    np.savez_compressed(path, **out)
    print('G15: losses', [l1, l2, l3], 'buffers', [b1, b2, b3], 'eval', le, be, os.path.getsize(path) // 1024, 'KiB')


if __name__ == '__main__':
    main()
