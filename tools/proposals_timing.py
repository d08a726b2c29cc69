#!/usr/bin/env python3
"""Times the proposal stage against the only alternative the library offers, this change's own eager restatement, on the
same device: ``RPNHeadMod.get_bboxes`` (padded: no host synchronisation) on the head outputs of a 384 x 1248 image at strides 4 .. 64 with
3 anchors — N = 1 with nms_pre = nms_post = 1000, nms_thr 0.75 (the test config) and N = 3 with nms_pre = 2000 (training) — with its parts
(the per-level sorts, ``mr_proposal_decode``, ``mr_nms_grouped``, the merge), and ``multiclass_nms`` at K = 1000 boxes, C = 1 and 3 classes,
score_thr 0.05, iou 0.7, max_num 100.  The restatement runs the same plumbing with the decode in torch ops and the NMS rule in numpy on
the host (``proposal_decode_torch``, ``nms_grouped_torch``).

HIP events around single calls, after 5 warm-ups; the median of the repeats (the restatement: 3 repeats after 1); a rotating set of input
buffers.  Not a test: asserts nothing about speed.

    python tools/proposals_timing.py [--repeats 40] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from monorun_amd import proposals as P  # noqa: E402
from monorun_amd.rpn_head import RPNHeadMod, merge_levels  # noqa: E402

IMAGE, STRIDES, A = (384, 1248), (4, 8, 16, 32, 64), 3
SHAPES = ((1, 1000, 1000), (3, 2000, 1000))            # images, nms_pre, nms_post
MULTICLASS = ((1000, 1), (1000, 3))                    # boxes, classes


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


class restated:
    """inside: every call runs the restatement"""

    def __enter__(self):
        self.saved = P.hip_ok, P.decode_hip_ok
        P.hip_ok = P.decode_hip_ok = lambda *a: False

    def __exit__(self, *exc):
        P.hip_ok, P.decode_hip_ok = self.saved


def head_outputs(n, gen, dev):
    """logits N(0, 2) and deltas N(0, 0.3): neighbouring anchors decode to overlapping boxes, as a trained head's do"""
    sizes = [(-(-IMAGE[0] // s), -(-IMAGE[1] // s)) for s in STRIDES]
    return ([2.0 * torch.randn(n, A, h, w, device=dev, generator=gen) for h, w in sizes],
            [0.3 * torch.randn(n, 4 * A, h, w, device=dev, generator=gen) for h, w in sizes])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=40)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'proposals_timing needs a HIP device'
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(1)
    rows = []
    for n, nms_pre, nms_post in SHAPES:
        cfg = dict(nms_across_levels=False, nms_pre=nms_pre, nms_post=nms_post, max_num=nms_post, nms_thr=0.75, min_bbox_size=0)
        head = RPNHeadMod(8, feat_channels=8, test_cfg=cfg,
                          anchor_generator=dict(type='AnchorGenerator', scales=[5], ratios=[0.4, 0.7, 1.0], strides=list(STRIDES)))
        gen_a = head.anchor_generator
        shapes = torch.tensor([[float(IMAGE[0]), float(IMAGE[1])]] * n, device=dev)
        sets = []
        for _ in range(4):
            cls, reg = head_outputs(n, gen, dev)
            index, counts = [], []
            for c in cls:
                logits = c.permute(0, 2, 3, 1).reshape(n, -1)
                k = min(nms_pre, logits.shape[1])
                index.append(torch.sort(logits, dim=1, descending=True, stable=True)[1][:, :k])
                counts.append(k)
            index = torch.cat(index, dim=1).contiguous()
            boxes, score, logit, valid = P.proposal_decode(cls, reg, index, counts, shapes, gen_a.base_anchors, STRIDES, (0.0,) * 4, (1.0,) * 4)
            keep = P.nms_grouped(boxes.reshape(-1, 4), valid.reshape(-1), tuple(counts) * n, 0.75)[0].reshape(n, -1)
            sets.append(dict(cls=cls, reg=reg, index=index, counts=counts, boxes=boxes, score=score, logit=logit, valid=valid, keep=keep))
        counts = sets[0]['counts']
        assert P.decode_hip_ok(sets[0]['cls'], sets[0]['reg'], sets[0]['index']) and P.hip_ok(sets[0]['boxes'].reshape(-1, 4), tuple(counts) * n)

        def whole(d):
            head.get_bboxes(d['cls'], d['reg'], shapes, padded=True)

        def sorts(d):
            for c in d['cls']:
                torch.sort(c.permute(0, 2, 3, 1).reshape(n, -1), dim=1, descending=True, stable=True)

        def decode(d):
            P.proposal_decode(d['cls'], d['reg'], d['index'], d['counts'], shapes, gen_a.base_anchors, STRIDES, (0.0,) * 4, (1.0,) * 4)

        def nms(d):
            P.nms_grouped(d['boxes'].reshape(-1, 4), d['valid'].reshape(-1), tuple(d['counts']) * n, 0.75)

        def merge(d):
            merge_levels(d['boxes'], d['score'], d['logit'], d['keep'], nms_post)

        row = dict(images=n, nms_pre=nms_pre, nms_post=nms_post, candidates_per_level=counts,
                   kept_per_image=[int(k) for k in sets[0]['keep'].sum(1).tolist()])
        for name, fn in (('get_bboxes', whole), ('sorts', sorts), ('decode', decode), ('nms', nms), ('merge', merge)):
            row[name + '_us'] = timed(fn, sets, args.repeats)
        with restated():
            for name, fn in (('get_bboxes', whole), ('decode', decode), ('nms', nms)):
                row['restated_' + name + '_us'] = timed(fn, sets, 3, warmup=1)
        rows.append(row)
        print(f"N={n} nms_pre={nms_pre}: get_bboxes {row['get_bboxes_us']:9.1f} us (restatement {row['restated_get_bboxes_us']:11.1f} us) = sorts "
              f"{row['sorts_us']:7.1f} + decode {row['decode_us']:6.1f} (restatement {row['restated_decode_us']:8.1f}) + nms {row['nms_us']:7.1f} "
              f"(restatement {row['restated_nms_us']:11.1f}) + merge {row['merge_us']:6.1f} + the rest   candidates per level {counts}   kept "
              f"{row['kept_per_image']}", flush=True)
    for k, c in MULTICLASS:
        sets = []
        for _ in range(4):
            u = torch.rand(k, 4, generator=gen, device=dev)
            centre = u[:, :2] * torch.tensor([IMAGE[1], IMAGE[0]], device=dev)
            wh = 20.0 + 180.0 * u[:, 2:]
            boxes = torch.cat((centre - wh / 2, centre + wh / 2), dim=1)
            scores = torch.rand(k, c + 1, generator=gen, device=dev) ** 3
            sets.append(dict(boxes=boxes, scores=scores))

        def multiclass(d):
            P.multiclass_nms(d['boxes'], d['scores'], 0.05, dict(type='nms', iou_threshold=0.7), 100)

        row = dict(boxes=k, classes=c, multiclass_nms_us=timed(multiclass, sets, args.repeats))
        with restated():
            row['restated_multiclass_nms_us'] = timed(multiclass, sets, 3, warmup=1)
        rows.append(row)
        print(f"multiclass_nms K={k} C={c}: {row['multiclass_nms_us']:9.1f} us (restatement {row['restated_multiclass_nms_us']:11.1f} us)", flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
