#!/usr/bin/env python3
"""Times the fused CARAFE launches against the torch restatement on the same device, at the workload's shape
(256 channels, 14 x 14 -> 28 x 28, k = 5, G = 1, s = 2) for N = 100 RoIs (one image) and N = 384 (a training step's positives).

HIP events around single calls, after warm-up; the median of the repeats; a rotating set of input / output buffers larger than the
256 MiB Infinity Cache, so that no call finds its operands cached by the previous one.  Reports microseconds and the achieved
algorithmic bytes/s — forward: x + m read, out written; backward: x + m + grad_out read, grad_x + grad_m written — as a fraction of the
6.29 TB/s the device copies at.  Not a test: asserts nothing about speed.

    python tools/carafe_timing.py [--repeats 50] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from monorun_amd import carafe  # noqa: E402

COPY_RATE = 6.29e12
C, H, W, K, G, S = 256, 14, 14, 5, 1, 2


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
    return statistics.median(times), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=50)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'carafe_timing needs a HIP device'
    dev = torch.device('cuda:0')
    rows = []
    for n in (100, 384):
        fwd_bytes = 4 * n * (C * H * W + G * K * K * S * S * H * W + C * H * S * W * S)
        bwd_bytes = 4 * n * (2 * C * H * W + 2 * G * K * K * S * S * H * W + C * H * S * W * S)
        nsets = max(2, int(600e6 // fwd_bytes) + 1)
        g = torch.Generator(device=dev).manual_seed(1)
        sets = [dict(x=torch.randn(n, C, H, W, device=dev, generator=g), m=3 * torch.randn(n, G * K * K * S * S, H, W, device=dev, generator=g),
                     go=torch.randn(n, C, H * S, W * S, device=dev, generator=g)) for _ in range(nsets)]
        assert carafe.hip_ok(sets[0]['x'], sets[0]['m'], K, G, S)

        def fwd(fn):
            def run(d):
                with torch.no_grad():
                    fn(d['x'], d['m'], K, G, S)
            return run

        def bwd_sets(fn, count):
            out = []
            for d in sets[:count]:
                x, m = d['x'].clone().requires_grad_(True), d['m'].clone().requires_grad_(True)
                out.append(dict(y=fn(x, m, K, G, S), x=x, m=m, go=d['go']))
            return out

        def bwd(d):
            torch.autograd.grad(d['y'], (d['x'], d['m']), d['go'], retain_graph=True)
        for name, fn, reps in (('fused', carafe.carafe_pack, args.repeats), ('torch', carafe.carafe_pack_torch, max(3, args.repeats // 10))):
            f_med, f_min = timed(fwd(fn), sets, reps)
            bs = bwd_sets(fn, nsets if name == 'fused' else 2)         # the restatement's graph keeps k^2 output-sized tensors per set
            b_med, b_min = timed(bwd, bs, reps)
            del bs
            torch.cuda.empty_cache()
            rows.append(dict(n=n, path=name, forward_us=f_med, forward_min_us=f_min, backward_us=b_med, backward_min_us=b_min,
                             forward_bytes=fwd_bytes, backward_bytes=bwd_bytes, forward_copy_fraction=fwd_bytes / (f_med * 1e-6) / COPY_RATE,
                             backward_copy_fraction=bwd_bytes / (b_med * 1e-6) / COPY_RATE, buffer_sets=nsets))
            r = rows[-1]
            print(f"N={n:4d} {name:5s} forward {r['forward_us']:9.1f} us ({100 * r['forward_copy_fraction']:5.1f}% of the copy rate)   "
                  f"backward {r['backward_us']:9.1f} us ({100 * r['backward_copy_fraction']:5.1f}%)   [{nsets} buffer sets]", flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
