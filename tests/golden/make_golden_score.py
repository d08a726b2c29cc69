#!/usr/bin/env python3
"""G16: the score head and its IoU sampler (mlp_score_head.py, iou3d_balanced_sampler.py), from the reference's own code.

Runs only in the authoring container (needs the reference tree, read-only; loaded by file path under the mmcv / mmdet stubs of
make_golden.py, nothing of it is copied).  The fixture is data: seeded inputs and what the reference's classes returned for them.

    python tests/golden/make_golden_score.py      # rewrites tests/golden/g16_score_head.npz

Head: reg_fc_out_channels = pose_fc_out_channels = 96, fc_out_channels = 40 (small on purpose: the fixture holds the weights), seeded
parameters, running statistics away from (0, 1).  24 rows of inputs whose covariances span five orders of magnitude.  Recorded: the
eval-mode logits; logits, running statistics and num_batches_tracked after each of two training-mode calls (24 rows, then 13 other
rows) and after a training-mode call with one row; the state_dict keys and shapes of a head with the DEFAULT sizes; what the head's
``loss`` hands to ``loss_score`` (a recording stand-in: targets for the three modes, and the weight with a sampler); the sampler's
keep rate and mask for three IoU sets (everything kept, too many positives, too many negatives) under a recorded uniform draw
``u`` that stands in for ``torch.rand_like``.
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as mg  # noqa: E402

OUT = HERE
C1, C2 = 96, 40


class _RecordingLoss:
    """Stands in for mmdet's loss module: keeps what the head passes to it."""

    def __init__(self):
        self.calls = []

    def __call__(self, scores, targets, weight=None):
        self.calls.append((scores.detach().clone(), targets.detach().clone(), None if weight is None else weight.detach().clone()))
        return scores.sum() * 0


def load():
    mg.install_stubs()
    for p in ('monorun', 'monorun.core', 'monorun.core.bbox_3d', 'monorun.core.bbox_3d.samplers', 'monorun.models', 'monorun.models.roi_heads',
              'monorun.models.roi_heads.bbox_3d_heads', 'monorun.models.roi_heads.bbox_3d_heads.score_heads'):
        mg._pkg(p)
    bld = mg._load('monorun.core.bbox_3d.builder', 'core/bbox_3d/builder.py')
    smp = mg._load('monorun.core.bbox_3d.samplers.iou3d_balanced_sampler', 'core/bbox_3d/samplers/iou3d_balanced_sampler.py')
    sys.modules['monorun.core'].build_iou3d_sampler = lambda cfg: mg._build_from_cfg(cfg, bld.IOU3D_SAMPLERS)
    sys.modules['mmdet.models.builder'].build_loss = lambda cfg: _RecordingLoss()
    head = mg._load('monorun.models.roi_heads.bbox_3d_heads.score_heads.mlp_score_head',
                    'models/roi_heads/bbox_3d_heads/score_heads/mlp_score_head.py')
    return head, smp


def make_inputs(rng, n):
    yaw = rng.uniform(-np.pi, np.pi, (n, 1))
    t = np.stack([rng.uniform(-12, 12, n), rng.uniform(1.0, 2.0, n), rng.uniform(5, 45, n)], 1)
    a = rng.normal(0, 1, (n, 4, 4))
    cov = a @ a.transpose(0, 2, 1) * 10.0 ** rng.uniform(-4, 2, (n, 1, 1))
    dims = rng.uniform([3.2, 1.4, 1.5], [4.6, 1.8, 1.8], (n, 3))
    reg = rng.normal(0, 1, (n, C1))
    return [torch.from_numpy(np.asarray(v, np.float32)) for v in (reg, yaw, t, cov, dims)]


class _Draw:
    """What the patched torch.rand_like returns: compares like the recorded draw ``u`` and keeps the keep rate it met."""

    def __init__(self, u):
        self.u, self.rate = u, None

    def __lt__(self, rate):
        self.rate = rate
        return self.u < rate


def main():
    href, sref = load()
    rng = np.random.default_rng(1616)
    torch.manual_seed(1616)
    out = {}

    head = href.MLPScoreHead(reg_fc_out_channels=C1, pose_fc_out_channels=C1, fc_out_channels=C2)
    head.init_weights()
    with torch.no_grad():
        for fc in list(head.pose_fcs) + list(head.fused_fcs):
            fc.bias.normal_(0, 0.1)
        head.fc_out.weight.normal_(0, 0.2)
        head.fc_out.bias.fill_(-0.3)
        head.pose_norm.running_mean.copy_(torch.from_numpy(rng.normal(0, 2, 17).astype(np.float32)))
        head.pose_norm.running_var.copy_(torch.from_numpy(rng.uniform(0.3, 30, 17).astype(np.float32)))
        head.pose_norm.weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, 17).astype(np.float32)))
        head.pose_norm.bias.copy_(torch.from_numpy(rng.normal(0, 0.2, 17).astype(np.float32)))
    for k, v in head.state_dict().items():
        out['param.' + k] = v.numpy().copy()

    inA, inB, inC = make_inputs(rng, 24), make_inputs(rng, 13), make_inputs(rng, 1)
    for name, ins in (('A', inA), ('B', inB), ('C', inC)):
        for key, v in zip(('reg_fc_out', 'yaw', 't_vec', 'pose_cov', 'dimensions'), ins):
            out[f'{name}_{key}'] = v.numpy()
    print('covariance scale, orders of magnitude:', float(np.ptp(np.log10(np.abs(out["A_pose_cov"]).reshape(24, -1).max(1)))))

    def buffers(tag):
        out[f'{tag}_running_mean'] = head.pose_norm.running_mean.detach().numpy().copy()
        out[f'{tag}_running_var'] = head.pose_norm.running_var.detach().numpy().copy()
        out[f'{tag}_num_batches_tracked'] = np.int64(head.pose_norm.num_batches_tracked.item())

    head.eval()
    with torch.no_grad():
        out['eval_logits'] = head(*inA).numpy()
    buffers('eval')
    assert np.array_equal(out['eval_running_mean'], out['param.pose_norm.running_mean'])
    head.train()
    for tag, ins in (('train1', inA), ('train2', inB), ('train_one_row', inC)):
        out[f'{tag}_logits'] = head(*ins).detach().numpy()
        buffers(tag)
    assert np.array_equal(out['train_one_row_running_mean'], out['train2_running_mean']) and out['train_one_row_num_batches_tracked'] == 3

    default = href.MLPScoreHead()
    out['default_state_dict'] = np.array(json.dumps([[k, list(v.shape)] for k, v in default.state_dict().items()]))

    # what loss() hands to loss_score: the targets of the three modes
    ious = torch.from_numpy(rng.uniform(0, 1, (24, 1)).astype(np.float32))
    ious[:3, 0] = torch.tensor([0.0, 0.25, 0.75])                     # the ends of the linear map, and on the threshold below
    ious[3, 0] = 0.7
    scores = torch.from_numpy(rng.normal(0, 1, 24).astype(np.float32))
    out['loss_ious'], out['loss_scores'] = ious.numpy(), scores.numpy()
    for mode in ('average', 'thres', 'linear_average'):
        h = href.MLPScoreHead(reg_fc_out_channels=C1, pose_fc_out_channels=C1, fc_out_channels=C2, mode=mode)
        h.loss(scores, ious.clone())
        (s, t, w), = h.loss_score.calls
        assert w is None and s.shape == (24, 1)
        out[f'loss_targets_{mode}'] = t.numpy()

    # the sampler: keep rate and mask under the recorded draw u
    u = torch.from_numpy(rng.uniform(0, 1, (24, 1)).astype(np.float32))
    out['sampler_u'] = u.numpy()
    sets = dict(all_kept=rng.uniform(0, 1, (24, 1)), many_pos=np.concatenate([rng.uniform(0.5, 1, (21, 1)), rng.uniform(0, 0.5, (3, 1))]),
                many_neg=np.concatenate([rng.uniform(0, 0.5, (22, 1)), rng.uniform(0.5, 1, (2, 1))]))
    sets['all_kept'][:12] = rng.uniform(0.5, 1, (12, 1)); sets['all_kept'][12:] = rng.uniform(0, 0.5, (12, 1))
    sets['many_pos'][0], sets['many_pos'][-1] = 0.98, 0.02            # beyond the strong thresholds: the unclamped rate leaves [min, max]
    sets['many_neg'][0], sets['many_neg'][-1] = 0.03, 0.97
    real_rand_like = torch.rand_like
    for smooth in (True, False):
        for name, v in sets.items():
            x = torch.from_numpy(v.astype(np.float32))
            draw = _Draw(u)
            torch.rand_like = lambda t, **k: draw
            try:
                mask = sref.IoU3DBalancedSampler(smooth_keeprate=smooth).sample(x)
                draw_min = _Draw(u)
                torch.rand_like = lambda t, **k: draw_min
                mask_min = sref.IoU3DBalancedSampler(smooth_keeprate=smooth, min_iou=0.2).sample(x)
            finally:
                torch.rand_like = real_rand_like
            tag = f'sampler_{"smooth" if smooth else "step"}_{name}'
            out[f'sampler_ious_{name}'] = x.numpy()
            out[tag + '_kept_all'] = np.bool_(draw.rate is None)
            if draw.rate is not None:
                out[tag + '_keeprate'] = draw.rate.numpy()
            out[tag + '_mask'] = mask.numpy()
            out[tag + '_mask_min_iou'] = mask_min.numpy()
            print(tag, 'kept' if draw.rate is None else (float(draw.rate.min()), float(draw.rate.max())), int(mask.sum()), int(mask_min.sum()))
    assert out['sampler_smooth_all_kept_kept_all'] and not out['sampler_smooth_many_pos_kept_all'] and not out['sampler_smooth_many_neg_kept_all']
    assert out['sampler_smooth_many_pos_keeprate'].max() > 1 and out['sampler_smooth_many_neg_keeprate'].max() > 1

    # loss() with a sampler: the per-sample weight it hands to loss_score
    x = torch.from_numpy(sets['many_pos'].astype(np.float32))
    h = href.MLPScoreHead(reg_fc_out_channels=C1, pose_fc_out_channels=C1, fc_out_channels=C2,
                          train_cfg=types.SimpleNamespace(iou3d_sampler=dict(type='IoU3DBalancedSampler')))
    draw = _Draw(u)
    torch.rand_like = lambda t, **k: draw
    try:
        h.loss(scores, x.clone())
    finally:
        torch.rand_like = real_rand_like
    (s, t, w), = h.loss_score.calls
    out['loss_sampled_targets'], out['loss_sampled_weight'] = t.numpy(), w.numpy()

    path = os.path.join(OUT, 'g16_score_head.npz')
    np.savez_compressed(path, **out)
    print('G16: eval logits', out['eval_logits'][:4], os.path.getsize(path) // 1024, 'KiB')


if __name__ == '__main__':
    main()
