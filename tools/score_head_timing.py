#!/usr/bin/env python3
"""Time the scoring step on the MI355X at the real sizes (reg_fc_out_channels = 1024, fc_out_channels = 256), for
n = 100 (one image's proposals) and n = 1024, three ways:

  eager   the torch ops of this module in eval mode (``score_poses_torch``): the reference's sequence of ops, which is all a user
          has without the fused launch
  fused   ``score_poses``: one launch of mr_score_head_forward, arguments marshalled on every call
  replay  ``ScoreHeadLaunch.replay()``: the prepared launch as a HIP graph

Each sample is the device-event time of a window of ``--calls`` back-to-back calls on one stream, divided by the number of calls, so
it includes whatever the host cannot hide between launches — what a caller of the step sees.  The three paths are sampled in turn
(eager, fused, replay, eager, ...) after a warm-up of every path at every shape, so that drift of the machine hits all alike.  Writes
medians and spreads (min, 10th / 90th percentile, max) in microseconds as JSON.

    python tools/score_head_timing.py [--out profiles/score_head_timing.json] [--samples 30] [--calls 200]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from monorun_amd.score_head import MLPScoreHead, ScoreHeadLaunch, score_poses, score_poses_torch  # noqa: E402

C1, C2 = 1024, 256


def window(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / calls            # microseconds per call


def summary(samples):
    a = np.asarray(samples)
    return dict(median_us=float(np.median(a)), min_us=float(a.min()), p10_us=float(np.percentile(a, 10)), p90_us=float(np.percentile(a, 90)),
                max_us=float(a.max()), samples=len(samples))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'score_head_timing.json'))
    ap.add_argument('--samples', type=int, default=30)
    ap.add_argument('--calls', type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('score_head_timing.py measures on an MI355X: no HIP device here, nothing measured')
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    head = MLPScoreHead(reg_fc_out_channels=C1, pose_fc_out_channels=C1, fc_out_channels=C2)
    head.init_weights()
    head = head.eval().to(dev)
    result = dict(device=torch.cuda.get_device_name(0), c1=C1, c2=C2, calls_per_sample=args.calls, unit='microseconds per call',
                  method='device events around a window of back-to-back calls; paths sampled in turn after warm-up', sizes={})
    for n in (100, 1024):
        g = torch.Generator(device='cpu').manual_seed(n)
        a = torch.randn(n, 4, 4, generator=g)
        res = dict(ret_val=torch.rand(n, generator=g) < 0.95, yaw_pred=torch.randn(n, 1, generator=g), t_vec_pred=torch.randn(n, 3, generator=g) * 10,
                   pose_cov_calib=a @ a.transpose(1, 2), pose_cov_pred=a @ a.transpose(1, 2), dimensions_pred=torch.rand(n, 3, generator=g) + 1.5)
        res = {k: v.to(dev) for k, v in res.items()}
        reg, det = torch.randn(n, C1, generator=g).to(dev), torch.rand(n, generator=g).to(dev)
        launch = ScoreHeadLaunch(head, n, dev)
        for k, v in (('reg_fc_out', reg), ('yaw', res['yaw_pred']), ('t_vec', res['t_vec_pred']), ('pose_cov', res['pose_cov_calib']),
                     ('dimensions', res['dimensions_pred']), ('ret_val', res['ret_val']), ('det_scores', det)):
            launch.inputs[k].copy_(v)
        launch.capture()
        with torch.no_grad():
            paths = dict(eager=lambda: score_poses_torch(head, reg, res, det_scores=det), fused=lambda: score_poses(head, reg, res, det_scores=det),
                         replay=launch.replay)
            # the three paths agree before anything is timed
            e, f, r = paths['eager'](), paths['fused'](), paths['replay']()['scores']
            torch.cuda.synchronize()
            assert torch.equal(f, r) and float((e - f).abs().max()) < 1e-4, 'the paths disagree: nothing measured'
            for fn in paths.values():
                window(fn, args.calls)                       # warm-up of this shape
            samples = {k: [] for k in paths}
            for _ in range(args.samples):
                for k, fn in paths.items():
                    samples[k].append(window(fn, args.calls))
        result['sizes'][str(n)] = {k: summary(v) for k, v in samples.items()}
        print(n, {k: round(v['median_us'], 2) for k, v in result['sizes'][str(n)].items()}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
