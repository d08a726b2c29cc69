#!/usr/bin/env python3
"""Time the global head's Monte-Carlo eval forward on the MI355X at the real sizes (256 x 7 x 7 -> 1024 -> 1024 -> 57,
S = 50), for n = 100 (one image's proposals) and n = 16, two ways on the same masks:

  eager   ``mc_forward_torch``: the reference's sequence of ops (repeat, mask multiplies, three ``Linear`` layers on rocBLAS,
          var_mean), which is all a user has without the kernels
  hip     ``mc_forward_hip``: mr_global_head_mc_forward, the first layer factored over the channel mask

Each sample is the device-event time of a window of ``--calls`` back-to-back calls on one stream, divided by the number of calls, so
it includes whatever the host cannot hide between launches — what a caller of the step sees.  The two paths are sampled in turn
(eager, hip, eager, ...) after a warm-up of both at every size, so that drift of the machine hits both alike.  Drawing the masks is
outside the windows (both paths need them).  Writes medians and spreads (min, 10th / 90th percentile, max) in microseconds as JSON.

    python tools/global_head_timing.py [--out profiles/global_head_timing.json] [--samples 15] [--calls 10]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from monorun_amd.global_head import FCExtractorMonteCarlo  # noqa: E402


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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'global_head_timing.json'))
    ap.add_argument('--samples', type=int, default=15)
    ap.add_argument('--calls', type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('global_head_timing.py measures on an MI355X: no HIP device here, nothing measured')
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    head = FCExtractorMonteCarlo(dim_coder=dict(type='MultiClassNormDimCoder'), loss_dim=None, with_dim=False)      # the configs' sizes are the defaults
    head.init_weights()
    head = head.eval().to(dev)
    result = dict(device=torch.cuda.get_device_name(0), in_channels=head.in_channels, roi_feat_size=list(head.roi_feat_size),
                  fc_out_channels=head.fc_out_channels, out_channels=head.out_channels, num_samples=head.num_samples,
                  calls_per_sample=args.calls, unit='microseconds per call',
                  method='device events around a window of back-to-back calls; paths sampled in turn after warm-up; same masks', sizes={})
    for n in (100, 16):
        g = torch.Generator(device='cpu').manual_seed(n)
        x = torch.randn(n, head.in_channels, *head.roi_feat_size, generator=g).to(dev)
        masks = [m.to(dev) for m in head.draw_masks(n, 'cpu', generator=g)]
        work = torch.empty(head.workspace_numel(n), device=dev)
        with torch.no_grad():
            paths = dict(eager=lambda: head.mc_forward_torch(x, masks), hip=lambda: head.mc_forward_hip(x, masks, workspace=work))
            # the two paths agree before anything is timed
            e, h = paths['eager'](), paths['hip']()
            torch.cuda.synchronize()
            scale = float(e[0].abs().max())
            assert float((e[0] - h[0]).abs().max()) < 1e-4 * max(scale, 1e-3) and float((e[4] - h[4]).abs().max()) < 1e-4 * float(e[4].abs().max()), \
                'the paths disagree: nothing measured'
            for fn in paths.values():
                window(fn, args.calls)                       # warm-up of this size
            samples = {k: [] for k in paths}
            for _ in range(args.samples):
                for k, fn in paths.items():
                    samples[k].append(window(fn, args.calls))
        result['sizes'][str(n)] = {k: summary(v) for k, v in samples.items()}
        print(n, {k: round(v['median_us'], 1) for k, v in result['sizes'][str(n)].items()}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
