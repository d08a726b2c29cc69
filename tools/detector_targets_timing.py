#!/usr/bin/env python3
"""Times the 2-D detector's target assignment and sampling against the only alternative the library offers, this change's
own eager restatement, on the same device, at the reference's training shape: 3 images of 384 x 1248, strides 4 .. 64 with 3 anchors
(119 700 anchors, one set for all images), about 10 ground truths and 3 ignore boxes per image (the RPN side: thresholds 0.7 / 0.3 / 0.3,
ignore 0.5, 256 samples), and 3 x 1000 proposals (the R-CNN side: 0.6 / 0.6 / 0.6, 512 samples, the ground truths added).

HIP path: ``MaxIoUAssigner.assign_batch`` (``mr_assign_max_iou``: two launches for all images) and ``RandomSampler.sample_batch``, no host
synchronisation.  Eager: per image ``bbox_overlaps`` in torch, mmdet's assignment with its Python loop over the ground truths (``if
gt_max_overlaps[i] >= min_pos_iou`` on a device tensor: one synchronisation per ground truth), ``bbox2delta`` on the positives and the list
form ``RandomSampler.sample``.

HIP events around single calls after 5 warm-ups, the median of the repeats, a rotating set of inputs; the launches of one call are counted
with torch's profiler where it is available.  Not a test: asserts nothing about speed.

    python tools/detector_targets_timing.py [--repeats 40] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from monorun_amd import assigners as A  # noqa: E402
from monorun_amd.rpn_head import AnchorGenerator  # noqa: E402

IMAGE, STRIDES, N = (384, 1248), (4, 8, 16, 32, 64), 3
SIDES = {'rpn': (dict(pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3, ignore_iof_thr=0.5), dict(num=256, pos_fraction=0.5, add_gt_as_proposals=False),
                 (0.0,) * 4, (1.0,) * 4),
         'rcnn': (dict(pos_iou_thr=0.6, neg_iou_thr=0.6, min_pos_iou=0.6, ignore_iof_thr=0.6), dict(num=512, pos_fraction=0.25, add_gt_as_proposals=True),
                  (0.0,) * 4, (0.1, 0.1, 0.2, 0.2))}


def timed(fn, sets, repeats, warmup=5):
    for i in range(warmup):
        fn(sets[i % len(sets)])
    torch.cuda.synchronize()
    times = []
    for i in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(sets[i % len(sets)])
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return statistics.median(times)


def launches(fn, d):
    """the device kernels and memsets of one call, or None without a working profiler"""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn(d)
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception:
        return None


def eager_assign(boxes, gts, ignore, rule, means, stds):
    """mmdet's MaxIoUAssigner.assign_wrt_overlaps on one image, its loop and its synchronisations as they are, then the coder on the positives"""
    overlaps = A.bbox_overlaps(gts, boxes[:, :4])
    if rule['ignore_iof_thr'] > 0 and ignore is not None and ignore.numel() > 0:
        ignore_max, _ = A.bbox_overlaps(boxes[:, :4], ignore, mode='iof').max(dim=1)
        overlaps[:, ignore_max > rule['ignore_iof_thr']] = -1
    num_gts = overlaps.size(0)
    assigned = overlaps.new_full((overlaps.size(1),), -1, dtype=torch.long)
    max_overlaps, argmax_overlaps = overlaps.max(dim=0)
    gt_max_overlaps, _ = overlaps.max(dim=1)
    assigned[(max_overlaps >= 0) & (max_overlaps < rule['neg_iou_thr'])] = 0
    pos = max_overlaps >= rule['pos_iou_thr']
    assigned[pos] = argmax_overlaps[pos] + 1
    for i in range(num_gts):
        if gt_max_overlaps[i] >= rule['min_pos_iou']:
            assigned[overlaps[i, :] == gt_max_overlaps[i]] = i + 1
    pos_inds = torch.nonzero(assigned > 0, as_tuple=False).squeeze(1)
    deltas = A.bbox2delta(boxes[pos_inds, :4], gts[assigned[pos_inds] - 1], means, stds)
    return A.AssignResult(num_gts, assigned, max_overlaps, assigned.new_zeros(assigned.shape)), deltas


def ground_truths(gen, dev):
    u = torch.rand(10, 4, generator=gen, device=dev)
    centre = u[:, :2] * torch.tensor([float(IMAGE[1]), float(IMAGE[0])], device=dev)
    wh = 24.0 + 200.0 * u[:, 2:] ** 2
    return torch.cat((centre - wh / 2, centre + wh / 2), dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=40)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'detector_targets_timing needs a HIP device'
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(1)
    sizes = [(-(-IMAGE[0] // s), -(-IMAGE[1] // s)) for s in STRIDES]
    anchors = torch.cat(AnchorGenerator([5], [0.4, 0.7, 1.0], list(STRIDES)).grid_anchors(sizes, dev))
    rows = []
    for side, (rule, sampling, means, stds) in SIDES.items():
        assigner, sampler = A.MaxIoUAssigner(**rule), A.RandomSampler(**sampling)
        sets = []
        for _ in range(4):
            gts = [ground_truths(gen, dev) for _ in range(N)]
            labels = [torch.randint(0, 3, (10,), device=dev, generator=gen) for _ in range(N)]
            ignore = [ground_truths(gen, dev)[:3] for _ in range(N)]
            if side == 'rpn':
                boxes, counts = anchors, None
            else:                       # proposals: jittered ground truths and random boxes, (N, 1000, 5) with NaN rows past the count
                jitter = torch.cat([g[torch.randint(0, 10, (300,), device=dev, generator=gen)] + 8.0 * torch.randn(300, 4, device=dev, generator=gen)
                                    for g in gts]).reshape(N, 300, 4)
                rand = torch.stack([torch.cat([ground_truths(gen, dev) for _ in range(70)]) for _ in range(N)])
                boxes = torch.cat((torch.cat((jitter, rand), dim=1), torch.rand(N, 1000, 1, device=dev, generator=gen)), dim=2)
                counts = torch.tensor([1000, 930, 870], dtype=torch.int32).to(dev)
                for n, k in enumerate((1000, 930, 870)):
                    boxes[n, k:] = float('nan')
            sets.append(dict(boxes=boxes, counts=counts, gts=gts, labels=labels, ignore=ignore, host_counts=(1000, 930, 870)))
        assert assigner.hip_ok(sets[0]['boxes'], sets[0]['gts'], sets[0]['ignore'])

        def hip_assign(d):
            return assigner.assign_batch(d['boxes'], d['gts'], d['ignore'], d['labels'], counts=d['counts'], means=means, stds=stds)

        def hip_both(d):
            return sampler.sample_batch(hip_assign(d), d['boxes'], d['gts'], d['labels'])

        def eager_assign_all(d):
            out = []
            for n in range(N):
                b = d['boxes'] if d['boxes'].dim() == 2 else d['boxes'][n, :d['host_counts'][n]]
                out.append(eager_assign(b, d['gts'][n], d['ignore'][n], rule, means, stds))
            return out

        def eager_both(d):
            out = []
            for n, (result, _) in enumerate(eager_assign_all(d)):
                b = d['boxes'] if d['boxes'].dim() == 2 else d['boxes'][n, :d['host_counts'][n]]
                out.append(sampler.sample(result, b, d['gts'][n], d['labels'][n]))
            return out

        torch.cuda.set_sync_debug_mode('error')
        hip_both(sets[0])                                       # the HIP path synchronises nowhere
        torch.cuda.set_sync_debug_mode('default')
        got, want = hip_assign(sets[0]), eager_assign_all(sets[0])
        agree = [bool(torch.equal(got.gt_inds[n, :len(want[n][0].gt_inds)], want[n][0].gt_inds)) for n in range(N)]
        row = dict(side=side, images=N, boxes=int(sets[0]['boxes'].shape[-2]), ground_truths=10, ignore_boxes=3, same_assignment=agree,
                   positives=[int((got.gt_inds[n] > 0).sum()) for n in range(N)])
        for name, fn in (('hip_assign', hip_assign), ('hip_assign_and_sample', hip_both)):
            row[name + '_us'] = timed(fn, sets, args.repeats)
            row[name + '_launches'] = launches(fn, sets[0])
        for name, fn in (('eager_assign', eager_assign_all), ('eager_assign_and_sample', eager_both)):
            row[name + '_us'] = timed(fn, sets, max(args.repeats // 4, 3), warmup=2)
            row[name + '_launches'] = launches(fn, sets[0])
        rows.append(row)
        print(f"{side}: {row['boxes']} boxes x {N} images: assign {row['hip_assign_us']:8.1f} us ({row['hip_assign_launches']} launches) against eager "
              f"{row['eager_assign_us']:9.1f} us ({row['eager_assign_launches']}); with sampling {row['hip_assign_and_sample_us']:8.1f} us "
              f"({row['hip_assign_and_sample_launches']}) against {row['eager_assign_and_sample_us']:9.1f} us "
              f"({row['eager_assign_and_sample_launches']}); same assignment {agree}, positives {row['positives']}", flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
