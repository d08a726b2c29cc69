#!/usr/bin/env python3
"""G14: the pose head's training loss (uncert_prop_pnp_optimizer.py:106-159) and its aligned rotated 3-D IoU
(core/bbox_3d/iou_calculators/bbox3d_iou_calculator.py:66-192), from the reference's own code.

Runs only in the authoring container (needs the reference tree, read-only; loaded by file path under numba / mmcv / mmdet stubs,
nothing of it is copied).  The fixture is data: seeded inputs and what the reference's functions returned for them.

    python tests/golden/make_golden_pose_loss.py      # rewrites tests/golden/g14_pose_loss.npz

Pairs (training layout [x, y, z, l, h, w, ry], boxes = the target, qboxes = the prediction), in 8 groups of 40, one group per
(criterion, z_center) with criterion in (-1, 0, 1, 2) and z_center in (1.0, 0.5); in every group:
   0..3   identical boxes (the numba BEV intersection is degenerate on coincident edges: `coincident`)
   4..9   concentric: same centre, other size / angle          10..13  disjoint in BEV
  14..19  offset vertically, box above the query (y smaller)    20..25  offset vertically, box below the query
  26..27  zero height overlap (touching)                        28..39  random nearby pairs
Per pair: rinc = devRotateIoUEval(box_bev, qbox_bev, 2) (the numba device function, run as Python on float32), iou_torch =
bev_to_box3d_overlaps_aligned_torch(boxes, qboxes, rinc, ...) (the function training uses), iou_numpy =
bev_to_box3d_overlaps_aligned(...) (its numpy sibling).  criterion 2 raises in both reference functions (`ua = 1.0` is a Python
float without .clamp / .clip); those entries are NaN and `ref_raises` is set.

Loss case: the reference's UncertPropPnPOptimizer.loss with loss_calib = KLLossMV(loss_weight=0.01) (its own loss file; mmdet's
weighted_loss restated in the stub) and its 3-D IoU with the BEV step run as above, on 24 synthetic objects of which 6 are
invalid.  Recorded: mean_iou, ious, loss_calib and d loss_calib / d pose_cov (autograd).
"""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def _weighted_loss(f):
    """mmdet.models.losses.utils.weighted_loss: element-wise loss -> optional weight -> reduction / avg_factor."""
    def wrapper(pred, target, weight=None, reduction='mean', avg_factor=None, **kw):
        loss = f(pred, target, **kw)
        if weight is not None:
            loss = loss * weight
        if avg_factor is None:
            return {'mean': loss.mean, 'sum': loss.sum}.get(reduction, lambda: loss)()
        if reduction == 'mean':
            return loss.sum() / avg_factor
        assert reduction == 'none'
        return loss
    return wrapper


def load():
    mg.install_stubs()
    nb = mg._pkg('numba')
    cu = mg._pkg('numba.cuda')

    def _jit(*a, **k):
        if len(a) == 1 and callable(a[0]) and not k:
            return a[0]
        return lambda f: f
    nb.jit = _jit; cu.jit = _jit; nb.cuda = cu
    nb.float32 = np.float32; nb.int32 = np.int32
    cu.local = types.SimpleNamespace(array=lambda shape, dtype: np.zeros(shape, dtype))
    cu.shared = cu.local
    for p in ('monorun', 'monorun.ops', 'monorun.core', 'monorun.core.bbox_3d', 'monorun.core.bbox_3d.iou_calculators',
              'monorun.core.bbox_3d.rotation_coder', 'monorun.models', 'monorun.models.losses', 'monorun.models.roi_heads',
              'monorun.models.roi_heads.bbox_3d_heads', 'monorun.models.roi_heads.bbox_3d_heads.optimizers'):
        mg._pkg(p)
    rk = mg._load('monorun.core.bbox_3d.iou_calculators.rotate_iou_kernel', 'core/bbox_3d/iou_calculators/rotate_iou_kernel.py')
    mg._load('monorun.core.bbox_3d.iou_calculators.rotate_iou_calculator', 'core/bbox_3d/iou_calculators/rotate_iou_calculator.py')
    calc = mg._load('monorun.core.bbox_3d.iou_calculators.bbox3d_iou_calculator', 'core/bbox_3d/iou_calculators/bbox3d_iou_calculator.py')

    def rinc_aligned(boxes, qboxes, criterion=-1):
        """the launch of rotate_iou_kernel_eval_aligned (rotate_iou_calculator.py:68-92), one devRotateIoUEval per pair"""
        b, q = boxes.detach().cpu().numpy().astype(np.float32), qboxes.detach().cpu().numpy().astype(np.float32)
        return torch.tensor([np.float32(rk.devRotateIoUEval(b[i], q[i], criterion)) for i in range(len(b))], dtype=torch.float32)
    calc.bbox_rotate_overlaps_aligned_torch = rinc_aligned

    bld = mg._load('monorun.core.bbox_3d.builder', 'core/bbox_3d/builder.py')
    mg._load('monorun.core.bbox_3d.rotation_coder.vec2d_rotation_coder', 'core/bbox_3d/rotation_coder/vec2d_rotation_coder.py')
    losses_reg = mg._Registry('losses')
    mdm = sys.modules['mmdet.models']
    mdm.LOSSES, mdm.weighted_loss = losses_reg, _weighted_loss
    mg._load('monorun.models.losses.kl_loss_mv', 'models/losses/kl_loss_mv.py')
    sys.modules['mmdet.models.builder'].build_loss = lambda cfg: mg._build_from_cfg(cfg, losses_reg)
    core = sys.modules['monorun.core']
    core.build_rotation_coder = lambda cfg: mg._build_from_cfg(cfg, bld.ROTATION_CODERS)
    core.bbox3d_overlaps_aligned_torch = calc.bbox3d_overlaps_aligned_torch
    sys.modules['monorun.ops'].build_pnp = lambda cfg: torch.nn.Identity()
    opt = mg._load('monorun.models.roi_heads.bbox_3d_heads.optimizers.uncert_prop_pnp_optimizer',
                   'models/roi_heads/bbox_3d_heads/optimizers/uncert_prop_pnp_optimizer.py')
    return rk, calc, opt


def make_pairs(rng, z_center, n=40):
    """boxes / qboxes (n, 7) float32 [x, y, z, l, h, w, ry], camera frame (y down), height coordinate at z_center of the box."""
    b = np.stack([rng.uniform(-10, 10, n), rng.uniform(0.5, 2.5, n), rng.uniform(5, 50, n), rng.uniform(3.0, 4.8, n),
                  rng.uniform(1.3, 1.9, n), rng.uniform(1.4, 1.9, n), rng.uniform(-np.pi, np.pi, n)], 1)
    q = b.copy()
    q[4:10, 3:6] *= rng.uniform(0.7, 1.3, (6, 3)); q[4:10, 6] += rng.normal(0, 0.6, 6)
    q[10:14, 0] += rng.choice([-1, 1], 4) * rng.uniform(8, 15, 4); q[10:14, 3:6] *= rng.uniform(0.8, 1.2, (4, 3))
    q[14:20, 1] = b[14:20, 1] + rng.uniform(0.2, 1.0, 6); q[20:26, 1] = b[20:26, 1] - rng.uniform(0.2, 1.0, 6)
    q[14:26, 0] += rng.normal(0, 0.3, 12); q[14:26, 2] += rng.normal(0, 0.3, 12); q[14:26, 3:6] *= rng.uniform(0.85, 1.15, (12, 3))
    q[14:26, 6] += rng.normal(0, 0.2, 12)
    q[26:28, 0] += rng.normal(0, 0.3, 2)
    q[26, 1] = b[26, 1] + b[26, 4] * z_center + q[26, 4] * (1 - z_center)          # query entirely below the box
    q[27, 1] = b[27, 1] - b[27, 4] * (1 - z_center) - q[27, 4] * z_center          # query entirely above the box
    q[28:] += np.concatenate([rng.normal(0, 0.8, (12, 3)), rng.normal(0, 0.25, (12, 3)) * b[28:, 3:6], rng.normal(0, 0.5, (12, 1))], 1)
    q[28:, 3:6] = np.abs(q[28:, 3:6])
    return b.astype(np.float32), q.astype(np.float32)


def main():
    rk, calc, opt = load()
    rng = np.random.default_rng(1414)
    rows = {k: [] for k in ('boxes', 'qboxes', 'criterion', 'z_center', 'rinc', 'iou_torch', 'iou_numpy', 'coincident', 'ref_raises')}
    for crit in (-1, 0, 1, 2):
        for zc in (1.0, 0.5):
            b, q = make_pairs(rng, zc)
            bev = [0, 2, 3, 5, 6]                    # z_axis = 1: bbox3d_iou_calculator.py:186-188
            rinc = np.array([np.float32(rk.devRotateIoUEval(b[i, bev], q[i, bev], 2)) for i in range(len(b))], np.float32)
            tb, tq, tr = torch.from_numpy(b), torch.from_numpy(q), torch.from_numpy(rinc)
            raises = False
            try:
                it = calc.bev_to_box3d_overlaps_aligned_torch(tb, tq, tr, crit, 1, zc).numpy()
                inp = calc.bev_to_box3d_overlaps_aligned(b, q, rinc, crit, 1, zc)
            except AttributeError:
                assert crit == 2
                raises = True
                it = inp = np.full(len(b), np.nan, np.float32)
            coinc = np.zeros(len(b), bool); coinc[:4] = True
            for k, v in (('boxes', b), ('qboxes', q), ('criterion', np.full(len(b), crit, np.int32)), ('z_center', np.full(len(b), zc, np.float32)),
                         ('rinc', rinc), ('iou_torch', np.asarray(it, np.float32)), ('iou_numpy', np.asarray(inp, np.float32)),
                         ('coincident', coinc), ('ref_raises', np.full(len(b), raises))):
                rows[k].append(v)
    out = {k: np.concatenate(v) for k, v in rows.items()}

    # ---- the loss: 24 objects, 6 invalid
    n = 24
    gt = np.stack([rng.uniform(3.2, 4.6, n), rng.uniform(1.4, 1.8, n), rng.uniform(1.5, 1.8, n), rng.uniform(-12, 12, n),
                   rng.uniform(1.0, 2.2, n), rng.uniform(6, 45, n), rng.uniform(-np.pi, np.pi, n)], 1).astype(np.float32)
    yaw = (gt[:, 6:7] + rng.normal(0, 0.15, (n, 1))).astype(np.float32)
    yaw[:3] += np.float32(2 * np.pi)                                         # wrapped yaw differences
    t = (gt[:, 3:6] + rng.normal(0, 0.3, (n, 3)) * np.array([1, 0.3, 1.5])).astype(np.float32)
    dims = (gt[:, 0:3] * rng.uniform(0.9, 1.1, (n, 3))).astype(np.float32)
    a = rng.normal(0, 1, (n, 4, 4)) * np.array([0.05, 0.3, 0.1, 0.6])[:, None]
    cov = (a @ a.transpose(0, 2, 1) + np.diag([1e-3, 0.02, 0.01, 0.1])).astype(np.float32)
    ret_val = np.ones(n, bool); ret_val[rng.choice(n, 6, replace=False)] = False
    head = opt.UncertPropPnPOptimizer(loss_calib=dict(type='KLLossMV', loss_weight=0.01))
    tcov = torch.from_numpy(cov).requires_grad_(True)
    tgt = torch.from_numpy(gt)
    yt, tt = head.get_targets(tgt)
    loss, ious = head.loss(torch.from_numpy(ret_val), torch.from_numpy(yaw), torch.from_numpy(t), tcov, torch.from_numpy(dims), yt, tt, tgt)
    loss['loss_calib'].backward()
    out.update(loss_pos_bboxes_3d=gt, loss_yaw_pred=yaw, loss_t_vec_pred=t, loss_dims_pred=dims, loss_pose_cov=cov, loss_ret_val=ret_val,
               loss_mean_iou=np.float32(loss['mean_iou'].item()), loss_ious=ious.numpy(), loss_calib=np.float32(loss['loss_calib'].item()),
               loss_calib_grad_pose_cov=tcov.grad.numpy())
    path = os.path.join(OUT, 'g14_pose_loss.npz')
    np.savez_compressed(path, **out)
    v = ~out['ref_raises']
    print('G14:', len(out['rinc']), 'pairs; torch != numpy rule on', int((out['iou_torch'][v] != out['iou_numpy'][v]).sum()),
          'of', int(v.sum()), '; mean_iou', loss['mean_iou'].item(), 'loss_calib', loss['loss_calib'].item(), os.path.getsize(path) // 1024, 'KiB')


if __name__ == '__main__':
    main()
