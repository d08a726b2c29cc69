#!/usr/bin/env python3
"""G18: the NOC head's LiDAR supervision (noc_coder.py encode, masked_dense_target.py, smooth_l1_loss.py), from the reference's own code.

Runs only in the authoring container (needs the reference tree, read-only; loaded by file path under the mmcv / mmdet stubs of
make_golden.py, nothing of it is copied).  The fixture is data: seeded inputs and what the reference's functions returned for them.

    python tests/golden/make_golden_noc_targets.py      # rewrites tests/golden/g18_noc_targets.npz

Stubs beyond make_golden.py's: ``mmcv.ops.roi_align.roi_align`` calls ``oracle.roi_align_avg`` (mmcv is absent: parity with mmcv's own
binary stays unpinned, as in G12), ``mmdet.models.weighted_loss`` is make_golden_pose_loss's, ``SmoothL1Loss`` a minimal base class.

Group a, dense_size 28: image 0 is 40x56, unflipped, 3 ground truths; image 1 is 33x47, flipped, 1 ground truth; image 2 (20x24, 2 ground
truths) has no positives.  Mask pixels are drawn from {0, 5e-6, 1e-5, 0.3, 1} in sparse and dense patches (stored as indices into
``mask_values``); the coordinates are ``raw * mask`` in fp32 with fp16-exact ``raw`` (stored as fp16).  One dimension lies below the coder's
eps.  11 RoIs: interior, sub-pixel bins (one tap), several taps per bin, overhanging every border by more than a pixel, zero area,
entirely over masked-out pixels, x2 == W.  Group b, dense_size (7, 9): one 20x30 image, flipped, 2 ground truths, 4 RoIs.

Recorded per group: targets, weights, a seeded fp16-exact noc_pred, the loss for reduction 'mean' and 'sum' (weight = weights) and
grad_pred of the 'mean' loss for a fixed upstream scalar.  The generator ASSERTS that no pooled mask value lies within 1 % of the
target eps 1e-4 (it tries the next seed otherwise), so that the 0/1 weights compare exactly.
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
MASK_VALUES = np.array([0.0, 5e-6, 1e-5, 0.3, 1.0], np.float32)
EPS_T = 1e-4


class _SmoothL1Loss(torch.nn.Module):
    def __init__(self, beta=1.0, reduction='mean', loss_weight=1.0):
        super().__init__()
        self.beta, self.reduction, self.loss_weight = beta, reduction, loss_weight


def load():
    mg.install_stubs()
    ra = mg._pkg('mmcv.ops.roi_align')

    def roi_align(inp, rois, out_size, spatial_scale, sampling_ratio, mode, aligned):
        assert mode == 'avg'
        return torch.from_numpy(orc.roi_align_avg(inp.numpy(), rois.numpy(), tuple(out_size), spatial_scale, sampling_ratio, aligned))
    ra.roi_align = roi_align
    sys.modules['mmcv.ops'].roi_align = ra
    for p in ('monorun', 'monorun.core', 'monorun.core.bbox_3d', 'monorun.core.bbox_3d.coord_coder', 'monorun.models', 'monorun.models.losses'):
        mg._pkg(p)
    mg._load('monorun.core.bbox_3d.builder', 'core/bbox_3d/builder.py')
    coder = mg._load('monorun.core.bbox_3d.coord_coder.noc_coder', 'core/bbox_3d/coord_coder/noc_coder.py')
    mdt = mg._load('monorun.core.bbox_3d.masked_dense_target', 'core/bbox_3d/masked_dense_target.py')
    mdm = sys.modules['mmdet.models']
    mdm.LOSSES, mdm.weighted_loss, mdm.SmoothL1Loss = mg._Registry('losses'), _weighted_loss, _SmoothL1Loss
    sl1 = mg._load('monorun.models.losses.smooth_l1_loss', 'models/losses/smooth_l1_loss.py')
    return coder, mdt, sl1


def make_image(rng, G, H, W, empty_left=None):
    """raw (G, 3, H, W) fp16-exact unmasked coordinates, mask index (G, 1, H, W) uint8 into MASK_VALUES, dimensions (G, 3)."""
    dims = rng.uniform([3.2, 1.4, 1.5], [4.6, 1.8, 1.8], (G, 3)).astype(np.float32)
    raw = (rng.uniform(-0.5, 0.5, (G, 3, H, W)) * dims[:, :, None, None] * 1.1).astype(np.float16)
    raw[:, 1] = (rng.uniform(-1.0, 0.0, (G, H, W)) * dims[:, 1, None, None]).astype(np.float16)
    idx = np.zeros((G, 1, H, W), np.uint8)
    for g in range(G):
        y0, x0 = rng.integers(0, H // 3), rng.integers(0, W // 3)
        y1, x1 = rng.integers(2 * H // 3, H + 1), rng.integers(2 * W // 3, W + 1)
        dense = rng.choice(5, (y1 - y0, x1 - x0), p=[0.1, 0.05, 0.05, 0.3, 0.5])
        idx[g, 0, y0:y1, x0:x1] = dense
        sparse = rng.random((H, W)) < 0.08                                          # LiDAR-like sparse returns everywhere else
        vals = rng.choice(5, (H, W), p=[0.0, 0.15, 0.15, 0.3, 0.4])
        outside = np.ones((H, W), bool); outside[y0:y1, x0:x1] = False
        idx[g, 0][sparse & outside] = vals[sparse & outside]
        if empty_left is not None and g == G - 1:
            idx[g, 0, :, :empty_left] = 0
    return raw, idx, dims


def maps(raw, idx):
    m = MASK_VALUES[idx]
    return (raw.astype(np.float32) * m).astype(np.float32), m


def run_group(ref, rng, images, rois, gts, dense_size, beta, loss_weight, upstream, tag, out):
    coder_mod, mdt, sl1 = ref
    coder = coder_mod.NOCCoder()
    enc, encm = [], []
    for k, (raw, idx, dims, flip) in enumerate(images):
        c, m = maps(raw, idx)
        e, em = coder.encode(torch.from_numpy(c), torch.from_numpy(m), torch.from_numpy(dims), flip)
        enc.append(e); encm.append(em)
        out[f'{tag}_img{k}_raw'], out[f'{tag}_img{k}_mask_index'], out[f'{tag}_img{k}_dimensions'] = raw, idx, dims
        out[f'{tag}_img{k}_rois'], out[f'{tag}_img{k}_gt_inds'] = rois[k], gts[k]
    out[f'{tag}_flips'] = np.array([f for _, _, _, f in images])
    cfg = types.SimpleNamespace(dense_size=dense_size)
    targets, weights = mdt.masked_dense_target([torch.from_numpy(r) for r in rois], [torch.from_numpy(g) for g in gts], enc, encm, cfg)
    # the condition that makes the 0/1 weights comparable exactly: no pooled mask value near the threshold
    hw = (dense_size, dense_size) if isinstance(dense_size, int) else tuple(dense_size)
    for k, (r, g) in enumerate(zip(rois, gts)):
        if len(r):
            H, W = images[k][0].shape[-2:]
            clip = np.stack([r[:, 0].clip(0, W), r[:, 1].clip(0, H), r[:, 2].clip(0, W), r[:, 3].clip(0, H)], 1).astype(np.float32)
            M = orc.roi_align_avg(encm[k].numpy(), np.concatenate([g[:, None].astype(np.float32), clip], 1), hw)
            if (np.abs(M - np.float32(EPS_T)) <= 0.01 * EPS_T).any():
                return False
    n = targets.shape[0]
    pred = torch.from_numpy(rng.normal(0, 1.5, (n, 3) + hw).astype(np.float16).astype(np.float32)).requires_grad_(True)
    lm = sl1.SmoothL1LossMod(beta=beta, loss_weight=loss_weight)
    loss_mean = lm(pred, targets, weight=weights)
    loss_mean.backward(torch.tensor(upstream, dtype=torch.float32))
    loss_sum = lm(pred.detach(), targets, weight=weights, reduction_override='sum')
    d = (pred.detach() - targets).abs()
    w = (weights > 0).expand_as(d)
    print(f'G18 {tag}: n {n}, positive bins {int((weights > 0).sum())} of {weights.numel()}, |d| < beta {int(((d < beta) & w).sum())}, '
          f'>= beta {int(((d >= beta) & w).sum())}, loss mean {loss_mean.item():.6f} sum {loss_sum.item():.3f}')
    out.update({f'{tag}_targets': targets.numpy(), f'{tag}_weights': weights.numpy(), f'{tag}_noc_pred': pred.detach().numpy().astype(np.float16),
                f'{tag}_loss_mean': np.float32(loss_mean.item()), f'{tag}_loss_sum': np.float32(loss_sum.item()),
                f'{tag}_grad_pred': pred.grad.numpy(), f'{tag}_beta': np.float64(beta), f'{tag}_loss_weight': np.float64(loss_weight),
                f'{tag}_upstream': np.float32(upstream), f'{tag}_dense_size': np.array(hw)})
    return True


def group_a(ref, seed, out):
    rng = np.random.default_rng(seed)
    im0 = make_image(rng, 3, 40, 56, empty_left=20)
    im0[2][2, 1] = 5e-6                                                             # one dimension below the coder's eps
    im1 = make_image(rng, 1, 33, 47)
    im2 = make_image(rng, 2, 20, 24)
    rois0 = np.array([[10.3, 8.2, 38.7, 30.1],          # interior
                      [20.0, 15.0, 30.5, 24.2],         # sub-pixel bins: one tap each
                      [0.5, 0.7, 55.2, 39.4],           # 2 x 2 taps per bin
                      [-5.5, -3.2, 20.1, 18.6],         # beyond the left and the top border by more than a pixel
                      [40.2, 25.3, 62.9, 47.8],         # beyond the right and the bottom border
                      [12.0, 12.0, 12.0, 12.0],         # zero area
                      [2.0, 2.0, 15.0, 30.0],           # over masked-out pixels only (ground truth 2 is empty left of x = 20)
                      [30.0, 5.0, 56.0, 35.0]], np.float32)      # x2 == W
    gts0 = np.array([0, 1, 1, 0, 2, 0, 2, 1], np.int64)
    rois1 = np.array([[3.3, 4.4, 40.2, 30.9], [-2.5, 10.0, 50.0, 36.5], [10.0, 10.0, 20.0, 18.0]], np.float32)
    gts1 = np.array([0, 0, 0], np.int64)
    images = [im0 + (False,), im1 + (True,), im2 + (False,)]
    return run_group(ref, rng, images, [rois0, rois1, np.zeros((0, 4), np.float32)], [gts0, gts1, np.zeros(0, np.int64)], 28, 1.0, 1.0, 0.75,
                     'a', out)


def group_b(ref, seed, out):
    rng = np.random.default_rng(seed)
    im = make_image(rng, 2, 20, 30)
    rois = np.array([[1.2, 0.8, 28.6, 19.1], [-3.0, 5.0, 14.0, 25.0], [8.0, 3.0, 30.0, 12.5], [11.0, 7.0, 13.0, 9.0]], np.float32)
    gts = np.array([1, 0, 0, 1], np.int64)
    return run_group(ref, rng, [im + (True,)], [rois], [gts], (7, 9), 0.7, 1.5, 1.3, 'b', out)


def main():
    ref = load()
    out = dict(mask_values=MASK_VALUES)
    for group, seed0 in ((group_a, 1800), (group_b, 1850)):
        for seed in range(seed0, seed0 + 20):
            trial = {}
            if group(ref, seed, trial):
                out.update(trial)
                print('seed', seed)
                break
        else:
            raise SystemExit('no seed keeps the pooled mask away from the threshold')
    path = os.path.join(OUT, 'g18_noc_targets.npz')
    np.savez_compressed(path, **out)
    print('G18:', os.path.getsize(path) // 1024, 'KiB')


if __name__ == '__main__':
    main()
