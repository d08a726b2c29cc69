#!/usr/bin/env python3
"""Times the feature pyramid's fused top-down launches against the eager chain on the same device, at the workload's
shape: 256 channels, a 384 x 1248 image, laterals of 96 x 312, 48 x 156, 24 x 78 and 12 x 39, lower_scale 2, for one image (a test image)
and three (a training step).  Three variants, alternated call by call in one process: the fused launches (``fpn_topdown``), the
restatement (``fpn_topdown_torch``: ``F.interpolate`` and an add per level, the bilinear rule in torch ops) and the reference's literal
chain (in place, ``F.interpolate`` for the bilinear map too: seven launches).  Each is timed forward under ``no_grad`` and forward plus
backward (``autograd.grad`` of every output to every lateral).

HIP events around single calls, after warm-ups; a rotating set of buffers larger than the 256 MiB Infinity Cache.  Per variant the median,
the minimum, and the 10th and 90th percentiles: that range is the spread of repeated runs of the same code, which a speed-up has to
exceed (the medians of the even and of the odd rounds are recorded too; they cannot see a distribution with two modes).  Bytes are counted from the shapes — fused forward: every lateral read
once, every merged level and the stride-2 map written once; backward: its mirror image; eager forward: also the up-sampled temporaries
written and re-read and each level read twice and written once by its add.  A single call at one image is bound by the host's share of
it, so the two launches are also timed through the C ABI, queued back to back, and it is those device times that are reported as a share
of the 6.3 TB/s the device copies at.  Not a test: asserts nothing about speed.

    python tools/fpn_timing.py [--repeats 30] [--out profiles/fpn_timing.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from monorun_amd import _lib, fpn  # noqa: E402

COPY_RATE = 6.3e12
C = 256
SIZES = ((96, 312), (48, 156), (24, 78), (12, 39))


def literal_chain(lats, lower_scale):
    """the reference's chain; its in-place add is written out of place (the same bytes: two reads and a write), so the buffers are kept"""
    lats = list(lats)
    for i in range(len(lats) - 1, 0, -1):
        lats[i - 1] = lats[i - 1] + F.interpolate(lats[i], size=lats[i - 1].shape[2:], mode='nearest')
    return lats, F.interpolate(lats[0], scale_factor=lower_scale, mode='bilinear', align_corners=False)


def counted_bytes(n):
    hw = [h * w for h, w in SIZES]
    fused = sum(hw) + sum(hw[:-1]) + 4 * hw[0]
    eager = sum(4 * a + b for a, b in zip(hw[:-1], hw[1:])) + 5 * hw[0]
    return dict(fused_forward=4 * n * C * fused, fused_backward=4 * n * C * fused, eager_forward=4 * n * C * eager)


def kernel_times(sets, n, reps=12):
    """microseconds per launch of the two entry points through the C ABI, `reps` launches queued back to back between two events: the
    device time without the host's share of a call"""
    L, dev = len(SIZES), sets[0]['lats'][0].device
    i32 = ctypes.c_int * L
    common = dict(level_h=i32(*[h for h, _ in SIZES]), level_w=i32(*[w for _, w in SIZES]), n_levels=L, n_images=n, channels=C, lower_scale=2)
    table = lambda ts: (ctypes.c_void_p * L)(*[_lib.ptr(t) for t in ts])
    stream = torch.cuda.current_stream(dev).cuda_stream
    outs = [dict(m=[torch.empty_like(t) for t in d['lats']], low=torch.empty_like(d['gs'][-1])) for d in sets]

    def forward(d, o):
        _lib.call('mr_fpn_topdown_forward', common, lat=table(d['lats']), merged=table(o['m'][:-1] + [None]), low=o['low'].data_ptr(), stream=stream)

    def backward(d, o):
        _lib.call('mr_fpn_topdown_backward', common, grad_merged=table(d['gs'][:L]), grad_low=d['gs'][L].data_ptr(), grad_lat=table(o['m']),
                  stream=stream)

    res = {}
    for name, fn in (('forward', forward), ('backward', backward)):
        for d, o in zip(sets, outs):
            fn(d, o)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(reps):
            fn(sets[i % len(sets)], outs[i % len(sets)])
        b.record()
        b.synchronize()
        res[name] = a.elapsed_time(b) * 1e3 / reps
    return res


def summary(times):
    s = sorted(times)
    pick = lambda q: s[min(len(s) - 1, int(q * len(s)))]
    return dict(median_us=statistics.median(times), min_us=s[0], p10_us=pick(0.1), p90_us=pick(0.9),
                even_rounds_median_us=statistics.median(times[0::2]), odd_rounds_median_us=statistics.median(times[1::2]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'fpn_timing needs a HIP device'
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(1)
    variants = dict(fused=fpn.fpn_topdown, restatement=fpn.fpn_topdown_torch, literal_chain=literal_chain)
    rows = []
    for n in (1, 3):
        rand = lambda *s: torch.randn(*s, device=dev, generator=gen)
        set_bytes = 4 * n * C * (2 * sum(h * w for h, w in SIZES) + 4 * SIZES[0][0] * SIZES[0][1])
        nsets = max(2, int(600e6 // set_bytes) + 1)
        sets = [dict(lats=[rand(n, C, h, w) for h, w in SIZES], gs=[rand(n, C, h, w) for h, w in SIZES] + [rand(n, C, 2 * SIZES[0][0], 2 * SIZES[0][1])])
                for _ in range(nsets)]
        assert fpn.hip_ok(sets[0]['lats'], 2)

        def forward(fn, d):
            with torch.no_grad():
                fn(d['lats'], 2)

        def both(fn, d):
            lats = [t.requires_grad_(True) for t in d['lats']]
            m, low = fn(lats, 2)
            torch.autograd.grad(list(m) + [low], lats, d['gs'])
            for t in lats:
                t.requires_grad_(False)

        times = {(name, what.__name__): [] for name in variants for what in (forward, both)}
        for i in range(args.warmup + args.repeats):
            d = sets[i % nsets]
            for what in (forward, both):
                for name, fn in variants.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    what(fn, d)
                    b.record()
                    b.synchronize()
                    if i >= args.warmup:
                        times[(name, what.__name__)].append(a.elapsed_time(b) * 1e3)
        nbytes = counted_bytes(n)
        row = dict(images=n, channels=C, sizes=SIZES, buffer_sets=nsets, repeats=args.repeats, counted_bytes=nbytes)
        for (name, what), t in times.items():
            row[f'{name}_{what}'] = summary(t)
        kt = kernel_times(sets, n)
        row['fused_forward_kernel_us'], row['fused_backward_kernel_us'] = kt['forward'], kt['backward']
        row['fused_forward_bytes_per_s'] = nbytes['fused_forward'] / (kt['forward'] * 1e-6)
        row['fused_backward_bytes_per_s'] = nbytes['fused_backward'] / (kt['backward'] * 1e-6)
        row['fused_forward_copy_fraction'] = row['fused_forward_bytes_per_s'] / COPY_RATE
        row['fused_backward_copy_fraction'] = row['fused_backward_bytes_per_s'] / COPY_RATE
        rows.append(row)
        for what in ('forward', 'both'):
            line = f'N={n} {what:8s}'
            for name in variants:
                s = row[f'{name}_{what}']
                line += (f'  {name} {s["median_us"]:9.1f} us (min {s["min_us"]:9.1f}, p10 {s["p10_us"]:9.1f}, p90 {s["p90_us"]:9.1f}, even / odd rounds '
                         f'{s["even_rounds_median_us"]:9.1f} / {s["odd_rounds_median_us"]:9.1f})')
            print(line, flush=True)
        print(f'N={n} launches queued back to back: forward {kt["forward"]:.1f} us = {100 * row["fused_forward_copy_fraction"]:.1f}%, backward '
              f'{kt["backward"]:.1f} us = {100 * row["fused_backward_copy_fraction"]:.1f}% of the copy rate by counted bytes  [{nsets} buffer sets]',
              flush=True)
        del sets
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
