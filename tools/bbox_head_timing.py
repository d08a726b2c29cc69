#!/usr/bin/env python3
"""Times the detection head's get_bboxes against the only alternative the library offered before it, on the same device in
the same process: ``Shared2FCBBoxHead.get_bboxes(padded=True)`` — ``mr_bbox_head_detect``, four launches, no host synchronisation — against
``F.softmax`` + delta2bbox in torch ops + ``proposals.multiclass_nms`` per image.  The test config (score_thr 0.05, iou_threshold 0.7,
max_per_img 100) at R = 1000 RoIs with C = 1 and C = 3 classes, one image, and at three images of 1000 RoIs; seeded logits such that a few
percent of the candidates pass the threshold, seeded deltas, RoIs in clusters.

HIP events around single calls, after 5 warm-ups; the median of the repeats; four rotating input sets; the two paths alternated in three
rounds.  ``--profile`` runs the fused call alone a few times (for ``rocprofv3 --kernel-trace --stats``).  The assertion at the end is the
requirement: the fused call is not slower than the composition at any shape.  ``--out`` writes ``device``, ``method``, ``config`` and
``shapes``; the ``kernel_us`` of each shape, the benchmark's headline and the test file's wall time in profiles/bbox_head_timing.json come
from runs of their own and were added to that file by hand.

    python tools/bbox_head_timing.py [--repeats 40] [--rounds 3] [--out FILE] [--profile]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from monorun_amd import bbox_head as B  # noqa: E402
from monorun_amd import proposals as P  # noqa: E402

IMAGE = (384, 1248)
SHAPES = ((1, 1000, 1), (1, 1000, 3), (3, 1000, 3))            # images, RoIs per image, classes
CFG = dict(score_thr=0.05, nms=dict(type='nms', iou_threshold=0.7), max_per_img=100)
MEANS, STDS = (0.0, 0.0, 0.0, 0.0), (0.1, 0.1, 0.2, 0.2)
METHOD = ('HIP events around single calls, 5 warm-up calls, the median of the repeats, four rotating input sets, the two paths alternated '
          'round by round in one process')
SCALE = (1.5, 1.25, 1.5, 1.25)


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


def inputs(n, k, c, gen, dev):
    """RoIs in clusters of near-duplicates, as an RPN hands them over; foreground logits about 7 below the background's, so that a few
    percent of the candidates score above 0.05"""
    centre = torch.rand(n * k // 12 + 1, 2, generator=gen, device=dev) * torch.tensor([IMAGE[1], IMAGE[0]], device=dev)
    size = 16 + 104 * torch.rand(len(centre), 2, generator=gen, device=dev)
    which = torch.randint(len(centre), (n * k,), generator=gen, device=dev)
    ctr = centre[which] + 0.12 * torch.randn(n * k, 2, generator=gen, device=dev) * size[which]
    wh = size[which] * torch.exp(0.15 * torch.randn(n * k, 2, generator=gen, device=dev))
    lo = torch.zeros(2, device=dev)
    hi = torch.tensor([IMAGE[1], IMAGE[0]], dtype=torch.float32, device=dev)
    boxes = torch.cat((torch.maximum(ctr - wh / 2, lo), torch.minimum(ctr + wh / 2, hi)), dim=1)
    image = torch.arange(n, device=dev, dtype=torch.float32).repeat_interleave(k)[:, None]
    cls = 1.5 * torch.randn(n * k, c + 1, generator=gen, device=dev)
    cls[:, c] += 7.0
    return dict(rois=torch.cat((image, boxes), dim=1).contiguous(), cls=cls, reg=torch.randn(n * k, 4 * c, generator=gen, device=dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=40)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--profile', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bbox_head_timing needs a HIP device'
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(1)
    rows = []
    for n, k, c in SHAPES:
        head = B.Shared2FCBBoxHead(in_channels=4, fc_out_channels=8, roi_feat_size=7, num_classes=c,
                                   bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=MEANS, target_stds=STDS)).to(dev)
        sets = [inputs(n, k, c, gen, dev) for _ in range(4)]
        shapes, scales, counts = [IMAGE + (3,)] * n, torch.tensor([SCALE] * n, device=dev), [k] * n
        img_hw = torch.tensor([[float(IMAGE[0]), float(IMAGE[1])]] * n, device=dev)
        assert B.hip_ok(sets[0]['rois'], sets[0]['cls'], sets[0]['reg'], counts, c)

        def fused(d):
            return head.get_bboxes(d['rois'], d['cls'], d['reg'], shapes, scales, rescale=True, cfg=CFG, padded=True, roi_counts=counts)

        def composition(d):
            """what the parent offers: softmax, the decode in torch ops, multiclass_nms per image (its count is a host synchronisation)"""
            scores = F.softmax(d['cls'], dim=1)
            boxes = B.decode_torch(d['rois'], d['reg'], img_hw.repeat_interleave(k, dim=0), scales.repeat_interleave(k, dim=0), MEANS, STDS)
            boxes = boxes.reshape(n * k, -1)
            return [P.multiclass_nms(boxes[i * k:(i + 1) * k], scores[i * k:(i + 1) * k], CFG['score_thr'], CFG['nms'], CFG['max_per_img'])
                    for i in range(n)]

        if args.profile:
            for i in range(8):
                fused(sets[i % 4])
            torch.cuda.synchronize()
            continue
        dets, labels, num = fused(sets[0])
        passed = float((F.softmax(sets[0]['cls'], dim=1)[:, :c] > CFG['score_thr']).float().mean())
        got = composition(sets[0])
        same = all(len(g[0]) == int(m) and torch.equal(g[1], labels[i, :int(m)]) for i, (g, m) in enumerate(zip(got, num.tolist())))
        row = dict(images=n, rois_per_image=k, classes=c, candidates_above_thr=round(passed, 4), detections=num.tolist(),
                   same_labels_as_composition=bool(same), fused_us=[], composition_us=[])
        for _ in range(args.rounds):
            row['fused_us'].append(timed(fused, sets, args.repeats))
            row['composition_us'].append(timed(composition, sets, args.repeats))
        row['speedup'] = statistics.median(row['composition_us']) / statistics.median(row['fused_us'])
        rows.append(row)
        print(f"N={n} R={k} C={c}: fused {row['fused_us']} us, composition {row['composition_us']} us, ratio {row['speedup']:.2f}, "
              f"{passed:.1%} above the threshold, detections {row['detections']}, same labels {same}", flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(dict(device=torch.cuda.get_device_name(dev), method=METHOD, config=dict(CFG, rescale=True), shapes=rows), f, indent=1)
    assert all(max(r['fused_us']) <= min(r['composition_us']) for r in rows), 'the fused call must not be slower than the composition'


if __name__ == '__main__':
    main()
