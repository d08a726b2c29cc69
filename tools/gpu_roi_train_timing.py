"""Host time of ``MonoRUnRoIHead.forward_train``, its fast path against its own literal path, forward alone and forward +
backward, at the reference's training shape: 3 KITTI-shaped images (384 x 1248 maps at the reference's widths), 1000 seeded proposals
each, ``RandomSampler(num=512, pos_fraction=0.25)``, 6 ground truths per image.  The weights are random and seeded: the time does not depend
on them except through the number of valid poses, which is reported.  Every call ends in a device synchronisation.

Then the positive stage alone on the sampling of that batch: ``roi_train.positives`` (one launch) against ``roi_train.positives_torch``.

The versions run in one process and ALTERNATE inside every window, after a warm-up of all; a window's figure is the median of its calls,
and the report is the median of the windows with their spread (min .. max), so that a difference can be held against the noise of the
shared host.  Every window runs under its own time limit (an alarm: a window that overruns ends the tool with an error, and nothing is
written).  Python delivers the alarm between bytecodes only: it ends a SLOW window, not one hung inside a device synchronisation, so run
the tool under an outer limit as well (`timeout -k 10 600 python tools/gpu_roi_train_timing.py`).  Before anything is timed the two paths'
losses are compared: the entries upstream of the NOC decode bit for bit, the entries downstream of it (the fast path decodes with
``decode_for_training``) by their difference, which is reported.

Writes profiles/roi_train_timing.json; 'established' says whether the two versions' ranges over the windows are disjoint.
Development aid: python tools/gpu_roi_train_timing.py [--windows 9] [--calls 20] [--stage-calls 200] [--window-limit 120]"""
import argparse
import copy
import json
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from monorun_amd import roi_train

dev = torch.device('cuda:0')
N, C, PROPOSALS, NUM, GTS = 3, 3, 1000, 512, 6
IMG_H, IMG_W = 384, 1248                   # a KITTI image at the training scale, padded to a multiple of 32
TRAIN_CFG = dict(bbox_assigner=dict(type='MaxIoUAssigner', pos_iou_thr=0.6, neg_iou_thr=0.6, min_pos_iou=0.6, match_low_quality=True, ignore_iof_thr=0.6),
                 bbox_sampler=dict(type='RandomSampler', num=NUM, pos_fraction=0.25, neg_pos_ub=-1, add_gt_as_proposals=True),
                 iou3d_sampler=dict(type='IoU3DBalancedSampler', pos_iou_thr=0.5, pos_fraction_min=0.25, pos_fraction_max=0.75, smooth_keeprate=True),
                 dense_size=28, pos_weight=-1, calib_scoring=True, debug=False)


def roi_head_and_batch(seed=0):
    """The RoI head at the reference's widths with the losses of its LiDAR-supervised config and seeded random weights, and a batch: six
    256-channel maps (strides 2 .. 64), per image 1000 seeded proposals (300 of them jittered ground truths), 6 ground truths with 3-D
    boxes behind their 2-D boxes and masked coordinate maps, the coordinate maps, KITTI's camera."""
    from monorun_amd.pose_head import gen_coord_2d
    from monorun_amd.roi_head import MonoRUnRoIHead

    def extractor(size):
        return dict(type='SingleRoIExtractor', roi_layer=dict(type='RoIAlign', output_size=size, sampling_ratio=0), out_channels=256,
                    featmap_strides=[2, 4, 8, 16, 32], finest_scale=20)
    torch.manual_seed(seed)
    head = MonoRUnRoIHead(
        bbox_roi_extractor=extractor(7),
        bbox_head=dict(type='Shared2FCBBoxHead', in_channels=256, fc_out_channels=1024, roi_feat_size=7, num_classes=C,
                       loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0), loss_bbox=dict(type='SmoothL1Loss', beta=1.0, loss_weight=1.0)),
        noc_roi_extractor=extractor(14), noc_head=dict(type='FCNNOCDecoder', num_classes=C, loss_noc=dict(type='SmoothL1LossMod', loss_weight=1.0, beta=1.0)),
        global_head=dict(type='FCExtractorMonteCarlo', num_samples=50, num_classes=C, loss_dim=dict(type='SmoothL1LossMod', loss_weight=1.0, beta=1.0)),
        projection_head=dict(type='UncertProjectionHead'), pose_head=dict(type='UncertPropPnPOptimizer', loss_calib=dict(type='KLLossMV', loss_weight=0.01)),
        score_head=dict(type='MLPScoreHead'), train_cfg=copy.deepcopy(TRAIN_CFG))
    head.init_weights()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m, size in ((head.bbox_head.fc_cls, 0.05), (head.noc_head.conv_final, 0.05), (head.noc_head.latent_decoder, 0.05)):
            m.weight.copy_(torch.randn(m.weight.shape, generator=g) * size)
    head = head.to(dev).train()
    feats = [torch.randn(N, 256, -(-IMG_H // s), -(-IMG_W // s), generator=g).to(dev) for s in (2, 4, 8, 16, 32, 64)]
    rng = np.random.default_rng(seed)
    fx, cx0, cy0 = 721.5377, 609.5593, 172.854
    out = dict(x=feats, img_metas=[], proposal_list=[], gt_bboxes=[], gt_labels=[], gt_bboxes_3d=[], gt_coords_3d=[], gt_coords_3d_mask=[])
    for n in range(N):
        cx, cy = rng.uniform(80, IMG_W - 80, GTS), rng.uniform(150, IMG_H - 60, GTS)
        w, h = rng.uniform(40, 300, GTS), rng.uniform(30, 150, GTS)
        gt = np.stack([np.clip(cx - w / 2, 0, 1242), np.clip(cy - h / 2, 0, 375), np.clip(cx + w / 2, 0, 1242), np.clip(cy + h / 2, 0, 375)], 1)
        lab = rng.choice(C, GTS, p=(0.7, 0.2, 0.1))
        px, py = rng.uniform(40, IMG_W - 40, PROPOSALS), rng.uniform(120, IMG_H - 40, PROPOSALS)
        pw, ph = rng.uniform(24, 300, PROPOSALS), rng.uniform(20, 160, PROPOSALS)
        p = np.stack([px - pw / 2, py - ph / 2, px + pw / 2, py + ph / 2], 1)
        p[:300] = gt[np.arange(300) % GTS] + rng.uniform(-6, 6, (300, 4))
        p[:, 0::2], p[:, 1::2] = np.clip(p[:, 0::2], 0, 1242), np.clip(p[:, 1::2], 0, 375)
        p = np.concatenate([p, rng.uniform(0.3, 1, (PROPOSALS, 1))], 1)
        dims = np.array([[3.9, 1.5, 1.6], [0.8, 1.75, 0.6], [1.8, 1.7, 0.6]])[lab] * rng.uniform(0.9, 1.1, (GTS, 3))
        z = fx * dims[:, 1] / (gt[:, 3] - gt[:, 1])
        b3 = np.concatenate([dims, ((gt[:, 0] + gt[:, 2]) / 2 - cx0)[:, None] / fx * z[:, None], ((gt[:, 1] + gt[:, 3]) / 2 - cy0)[:, None] / fx * z[:, None],
                             z[:, None], rng.uniform(-3, 3, (GTS, 1))], 1)
        m = np.zeros((GTS, 1, IMG_H, IMG_W), np.float32)
        for i, b in enumerate(gt.astype(int)):
            m[i, 0, b[1]:b[3], b[0]:b[2]] = rng.uniform(size=(b[3] - b[1], b[2] - b[0])) < 0.5
        c3 = (rng.uniform(-0.5, 0.5, (GTS, 3, IMG_H, IMG_W)) * dims[:, :, None, None]).astype(np.float32) * m
        t = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(dev)
        out['proposal_list'].append(t(p)); out['gt_bboxes'].append(t(gt)); out['gt_labels'].append(t(lab, np.int64)); out['gt_bboxes_3d'].append(t(b3))
        out['gt_coords_3d'].append(t(c3)); out['gt_coords_3d_mask'].append(t(m))
        out['img_metas'].append(dict(img_shape=(375, 1242, 3), pad_shape=(IMG_H, IMG_W, 3), scale_factor=np.ones(4, np.float32), flip=bool(n % 2)))
    out['coord_2d'] = torch.cat([gen_coord_2d(375, 1242, flip=bool(n % 2), device=dev) for n in range(N)])
    out['cam_intrinsic'] = torch.tensor([[fx, 0.0, cx0], [0.0, fx, cy0], [0.0, 0.0, 1.0]], device=dev).expand(N, 3, 3).contiguous()
    return head, out


def head_call(head, batch, keys, path, backward):
    torch.manual_seed(7)                        # dropout and the score head's sampler: the same draws for both paths
    losses = head.forward_train(**batch, keys=keys, path=path)
    if backward:
        head.zero_grad(set_to_none=True)
        sum(v.sum() for k, v in losses.items() if 'loss' in k).backward()
    torch.cuda.synchronize()
    return losses


class limit:
    """a wall-clock limit on a block: SIGALRM raises when it runs out"""

    def __init__(self, seconds):
        self.seconds = int(seconds)

    def __enter__(self):
        def over(*_):
            raise TimeoutError(f'a timing window ran past its limit of {self.seconds} s')
        self.before = signal.signal(signal.SIGALRM, over)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        signal.signal(signal.SIGALRM, self.before)


def window(fns, calls, seconds):
    """median host time in us of each function over `calls` alternating rounds; every function ends in a device synchronisation"""
    ts = [[] for _ in fns]
    with limit(seconds):
        for _ in range(calls):
            for i, fn in enumerate(fns):
                t0 = time.perf_counter()
                fn()
                ts[i].append(time.perf_counter() - t0)
    return [float(np.median(x)) * 1e6 for x in ts]


def report(per_window):
    a = np.array(per_window)
    return dict(median_us=round(float(np.median(a)), 1), min_us=round(float(a.min()), 1), max_us=round(float(a.max()), 1))


def compare(names, wins):
    out = {name: report([w[i] for w in wins]) for i, name in enumerate(names)}
    a, b = out[names[0]], out[names[1]]
    out['established'] = bool(a['max_us'] < b['min_us'] or b['max_us'] < a['min_us'])      # the windows' ranges do not overlap
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=9)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--stage-calls', type=int, default=200)
    ap.add_argument('--window-limit', type=int, default=120)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'roi_train_timing.json'))
    args = ap.parse_args()
    assert args.windows >= 9, 'at least nine windows'
    head, batch = roi_head_and_batch()
    Gm = GTS
    keys = torch.from_numpy(np.random.default_rng(3).uniform(size=(N, Gm + PROPOSALS)).astype(np.float32)).to(dev)
    assert head.train_fast_path_reason(batch['x'], batch['proposal_list']) is None
    with limit(args.window_limit):
        fast, lit = head_call(copy.deepcopy(head), batch, keys, 'fast', False), head_call(copy.deepcopy(head), batch, keys, 'literal', False)
    upstream = ('loss_cls', 'acc', 'loss_bbox', 'loss_dim', 'loss_noc')
    same = list(fast) == list(lit) and all(torch.equal(fast[k], lit[k]) for k in upstream)
    below = {k: abs(float((fast[k].detach() - lit[k].detach()).sum())) for k in lit if k not in upstream}
    out = dict(device=torch.cuda.get_device_name(0),
               shape=dict(images=N, image=[IMG_H, IMG_W], proposals=PROPOSALS, num=NUM, ground_truths=GTS, classes=C),
               upstream_losses_bitwise_equal=bool(same), downstream_losses_abs_difference=below, losses={k: float(v.detach().sum()) for k, v in fast.items()}, windows=args.windows,
               calls_per_window=args.calls, window_limit_s=args.window_limit)
    for name, backward in (('forward', False), ('forward_backward', True)):
        fns = (lambda: head_call(head, batch, keys, 'literal', backward), lambda: head_call(head, batch, keys, 'fast', backward))
        window(fns, 2, args.window_limit)                                                  # warm-up of both
        out[name] = compare(('literal', 'fast'), [window(fns, args.calls, args.window_limit) for _ in range(args.windows)])
    # the positive stage alone, on this batch's sampling
    boxes = torch.stack([p[:, :4] for p in batch['proposal_list']])
    sampled = head.bbox_sampler.sample_batch(head.bbox_assigner.assign_batch(boxes, batch['gt_bboxes'], None, batch['gt_labels']), boxes,
                                             batch['gt_bboxes'], batch['gt_labels'], keys=keys)
    num_pos, num_neg = sampled.num_pos.tolist(), sampled.num_neg.tolist()
    rows = np.concatenate(([0], np.cumsum(np.add(num_pos, num_neg))))[:N].tolist()
    pred = torch.randn(int(sum(num_pos) + sum(num_neg)), 4 * C, generator=torch.Generator().manual_seed(9)).to(dev)
    stage = (sampled, num_pos, pred, rows, batch['gt_bboxes_3d'], batch['cam_intrinsic'], [m['img_shape'] for m in batch['img_metas']],
             [m['flip'] for m in batch['img_metas']], C, False, head.bbox_head.target_means, head.bbox_head.target_stds,
             head.global_head.dim_coder.target_means, head.global_head.dim_coder.target_stds)

    def stage_call(fn):
        fn(*stage)
        torch.cuda.synchronize()
    a, b = roi_train.positives(*stage), roi_train.positives_torch(*stage)
    fns = (lambda: stage_call(roi_train.positives_torch), lambda: stage_call(roi_train.positives))
    window(fns, 20, args.window_limit)
    out['positive_stage'] = compare(('torch', 'launch'), [window(fns, args.stage_calls, args.window_limit) for _ in range(args.windows)])
    out['positive_stage'].update(positives=int(sum(num_pos)), calls_per_window=args.stage_calls,
                                 outputs_bitwise_equal=bool(all(torch.equal(getattr(a, k), getattr(b, k)) for k in roi_train.FIELDS)))
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
