"""Host time of the per-image result tail, each version ending in its copy to the host, at the workload's shape: 100
detections, 3 classes, nms_3d_thr = 0.01, seeded KITTI-like boxes.

  parent   consumers.get_bbox_3d_result -> consumers.multiclass_3d_result_nms(to_np=True) -> per-class selection of the 2-D boxes
           (bbox2result, then indexing with the kept indices), as monorun_roi_head.py:481-565 does it
  fused    consumers.result_3d_nms(to_np=True): one launch, one copy

Both run in one process and ALTERNATE inside every window, after a warm-up of both; a window's figure is the median of its calls, and
the report is the median of the windows with their spread (min .. max), so that a difference can be held against the noise of the
shared host.  The two versions' outputs are compared bit for bit before anything is timed.

Then, in the same way, ``MonoRUnRoIHead.simple_test``'s fast path against its own literal path on one KITTI-shaped image (384 x 1248
maps at the reference's widths, 100 seeded proposals).  The weights are random and seeded: the time does not depend on them except
through the number of detections, which is reported.  Every call ends on the host (numpy results).

Writes profiles/roi_head_timing.json; 'established' says whether the two versions' ranges over the windows are disjoint.
Development aid: python tools/gpu_roi_head_timing.py [--windows 9] [--calls 200] [--head-calls 20]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from monorun_amd import consumers
from monorun_amd.bbox_head import bbox2result

dev = torch.device('cuda:0')
N, C, THR = 100, 3, 0.01


def detections(seed=0):
    """100 KITTI-like objects in front of the camera: cars, pedestrians and cyclists by size, a road scene's spread (x +-25 m, z 5 .. 60 m)
    dense enough that the NMS removes some; 2-D boxes with scores; a few failed solves (score 0)"""
    rng = np.random.default_rng(seed)
    labels = rng.choice(C, N, p=(0.7, 0.2, 0.1)).astype(np.int64)
    size = np.array([[3.9, 1.5, 1.6], [0.8, 1.75, 0.6], [1.8, 1.7, 0.6]], np.float32)[labels]           # l, h, w
    dims = (size * rng.uniform(0.85, 1.15, (N, 3))).astype(np.float32)
    t = np.stack([rng.uniform(-25, 25, N), rng.uniform(1.0, 2.0, N), rng.uniform(5, 60, N)], 1).astype(np.float32)
    yaw = rng.uniform(-np.pi, np.pi, (N, 1)).astype(np.float32)
    scores = rng.uniform(0.05, 1, N).astype(np.float32)
    scores[rng.permutation(N)[:5]] = 0
    xy = rng.uniform(0, 1000, (N, 2))
    det = np.concatenate([xy, xy + rng.uniform(20, 200, (N, 2)), rng.uniform(0.05, 1, (N, 1))], 1).astype(np.float32)
    return [torch.from_numpy(a).to(dev) for a in (dims, yaw, t, scores, labels, det)]


def parent_tail(dims, yaw, t, scores, labels, det):
    bbox_result = bbox2result(det, labels, C)
    res = consumers.get_bbox_3d_result(dims, yaw, t, scores, labels, C, to_np=False)
    res, keep = consumers.multiclass_3d_result_nms(res, THR, to_np=True)
    return res, keep, [b[k] for b, k in zip(bbox_result, keep)]


def fused_tail(dims, yaw, t, scores, labels, det):
    return consumers.result_3d_nms(dims, yaw, t, scores, labels, det, C, THR, to_np=True)


def window(fns, calls):
    """median host time in us of each function over `calls` alternating rounds; every call ends on the host (its arrays are numpy)"""
    ts = [[] for _ in fns]
    for _ in range(calls):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            ts[i].append(time.perf_counter() - t0)
    return [float(np.median(x)) * 1e6 for x in ts]


def report(name, per_window):
    a = np.array(per_window)
    return {name: dict(median_us=round(float(np.median(a)), 1), min_us=round(float(a.min()), 1), max_us=round(float(a.max()), 1))}


IMG_H, IMG_W = 384, 1248                   # a KITTI image at the testing scale, padded to a multiple of 32


def roi_head_and_image(seed=0):
    """The RoI head at the reference's widths (256 channels, 1024-wide FC layers, 50 Monte-Carlo samples) with seeded random weights, and
    one KITTI-shaped image's inputs: six 256-channel maps (strides 2 .. 64), 100 seeded proposals, the coordinate map, KITTI's camera."""
    from monorun_amd.pose_head import gen_coord_2d
    from monorun_amd.roi_head import MonoRUnRoIHead

    def extractor(size):
        return dict(type='SingleRoIExtractor', roi_layer=dict(type='RoIAlign', output_size=size, sampling_ratio=0), out_channels=256,
                    featmap_strides=[2, 4, 8, 16, 32], finest_scale=20)
    torch.manual_seed(seed)
    head = MonoRUnRoIHead(
        bbox_roi_extractor=extractor(7), bbox_head=dict(type='Shared2FCBBoxHead', in_channels=256, fc_out_channels=1024, roi_feat_size=7, num_classes=C),
        noc_roi_extractor=extractor(14), noc_head=dict(type='FCNNOCDecoder', num_classes=C),
        global_head=dict(type='FCExtractorMonteCarlo', num_samples=50, num_classes=C), projection_head=dict(type='UncertProjectionHead'),
        pose_head=dict(type='UncertPropPnPOptimizer'), score_head=dict(type='MLPScoreHead'),
        test_cfg=dict(score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100, mult_2d_score=True, calib_scoring=True,
                      cov_correction=True, nms_3d_thr=THR))
    head.init_weights()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():                       # init_weights leaves the classifier near zero: seeded weights of some size spread the classes
        for m, size in ((head.bbox_head.fc_cls, 0.05), (head.noc_head.conv_final, 0.05), (head.noc_head.latent_decoder, 0.05)):
            m.weight.copy_(torch.randn(m.weight.shape, generator=g) * size)
    head = head.to(dev).eval()
    feats = [torch.randn(1, 256, -(-IMG_H // s), -(-IMG_W // s), generator=g).to(dev) for s in (2, 4, 8, 16, 32, 64)]
    rng = np.random.default_rng(seed)
    cx, cy = rng.uniform(40, IMG_W - 40, N), rng.uniform(120, IMG_H - 40, N)
    w, h = rng.uniform(24, 300, N), rng.uniform(20, 160, N)
    props = np.stack([np.clip(cx - w / 2, 0, IMG_W), np.clip(cy - h / 2, 0, IMG_H), np.clip(cx + w / 2, 0, IMG_W), np.clip(cy + h / 2, 0, IMG_H),
                      rng.uniform(0.3, 1, N)], 1).astype(np.float32)
    K = torch.tensor([[[721.5377, 0.0, 609.5593], [0.0, 721.5377, 172.854], [0.0, 0.0, 1.0]]], device=dev)
    return head, dict(x=feats, proposal_list=[torch.from_numpy(props).to(dev)],
                      img_metas=[dict(img_shape=(375, 1242, 3), scale_factor=np.ones(4, np.float32), flip=False)],
                      coord_2d=[gen_coord_2d(375, 1242, device=dev)], cam_intrinsic=[K])


def head_call(head, inputs, path):
    torch.manual_seed(7)                        # the Monte-Carlo masks: the same draws for both paths
    with torch.no_grad():
        return head.simple_test(inputs['x'], inputs['proposal_list'], inputs['img_metas'], coord_2d=inputs['coord_2d'],
                                cam_intrinsic=inputs['cam_intrinsic'], path=path)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=9)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--head-calls', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'roi_head_timing.json'))
    args = ap.parse_args()
    ins = detections()
    old, new = parent_tail(*ins), fused_tail(*ins)
    same = all(np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
               for x, y in zip(old, new) for a, b in zip(x, y))
    kept = [int(len(k)) for k in new[1]]
    fns = (lambda: parent_tail(*ins), lambda: fused_tail(*ins))
    window(fns, 50)                                                  # warm-up of both
    torch.cuda.synchronize()
    wins = [window(fns, args.calls) for _ in range(args.windows)]
    out = dict(device=torch.cuda.get_device_name(0), shape=dict(detections=N, classes=C, nms_3d_thr=THR, per_class=[int((ins[4] == c).sum()) for c in range(C)],
                                                                kept=kept),
               outputs_bitwise_equal=bool(same), windows=args.windows, calls_per_window=args.calls, result_tail={})
    out['result_tail'].update(report('parent', [w[0] for w in wins]))
    out['result_tail'].update(report('fused', [w[1] for w in wins]))
    p, f = out['result_tail']['parent'], out['result_tail']['fused']
    out['result_tail']['established'] = bool(f['max_us'] < p['min_us'] or p['max_us'] < f['min_us'])      # the windows' ranges do not overlap
    # MonoRUnRoIHead.simple_test: its fast path against its own literal path on one KITTI-shaped image
    head, image = roi_head_and_image()
    fast, lit = head_call(head, image, 'fast'), head_call(head, image, 'literal')
    hf = (lambda: head_call(head, image, 'literal'), lambda: head_call(head, image, 'fast'))
    window(hf, 3)
    torch.cuda.synchronize()
    hw = [window(hf, args.head_calls) for _ in range(args.windows)]
    out['simple_test'] = dict(image=[IMG_H, IMG_W], proposals=N, calls_per_window=args.head_calls,
                              detections_kept=dict(fast=[int(len(b)) for b in fast['bbox_3d_results']], literal=[int(len(b)) for b in lit['bbox_3d_results']]))
    out['simple_test'].update(report('literal', [w[0] for w in hw]))
    out['simple_test'].update(report('fast', [w[1] for w in hw]))
    p, f = out['simple_test']['literal'], out['simple_test']['fast']
    out['simple_test']['established'] = bool(f['max_us'] < p['min_us'] or p['max_us'] < f['min_us'])
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
