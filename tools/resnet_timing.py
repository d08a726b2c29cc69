#!/usr/bin/env python3
"""Times the backbone's fused batch norm against the literal eager chain on the same device, at the workload's shapes: a
1248 x 384 image, the activations of ResNet-101's four stages (256 x 96 x 312, 512 x 48 x 156, 1024 x 24 x 78, 2048 x 12 x 39) and of
its stem (64 x 192 x 624), for one image (a test image) and three (a training step).

  ops      ``bn_act`` against ``F.batch_norm(training=False)``, ``add_``, ``relu_``: with and without the residual; forward under
           ``no_grad``, and forward plus backward with the gradients of x, the residual, the weight and the bias.
  stem     ``bn_relu_maxpool`` against ``F.batch_norm``, ``relu_``, ``F.max_pool2d``, forward.
  network  ResNet-101 whole: forward at N = 1 in eval mode, forward plus backward at N = 3 in training mode with ``frozen_stages=1`` and
           ``norm_eval=True``; the fused module, the same module with the restatement forced, and a literal eager module
           (``nn.BatchNorm2d.forward``, ``+=``, in-place ReLU, ``nn.MaxPool2d``).  The convolutions are MIOpen's in all three.

HIP events around single calls, after warm-ups, the variants alternated call by call in one process; a rotating set of buffers larger
than the 256 MiB Infinity Cache.  Per variant the median, the minimum and the 10th and 90th percentiles: that range is the spread of
repeated runs of the same code, which a difference has to exceed — ``separated`` records whether the two ranges do not meet.  Bytes are
counted from the shapes (forward: x and the residual read, y written; backward with parameter gradients: g, y and x read, grad_x and
grad_r written; the stem: x read, a quarter written), and the launches are also timed through the C ABI, queued back to back: it is those
device times that are reported as a share of the 6.3 TB/s the device copies at.  Not a test: asserts nothing about speed.

    python tools/resnet_timing.py [--repeats 30] [--out profiles/resnet_timing.json] [--skip-network]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from monorun_amd import _lib, resnet  # noqa: E402

COPY_RATE = 6.3e12
IMAGE = (384, 1248)
STAGES = (('layer1', 256, 96, 312), ('layer2', 512, 48, 156), ('layer3', 1024, 24, 78), ('layer4', 2048, 12, 39))
STEM = (64, 192, 624)
EPS = 1e-5


def literal_chain(x, mean, var, weight, bias, eps, residual, relu=True):
    y = F.batch_norm(x, mean, var, weight, bias, False, 0.1, eps)
    if residual is not None:
        y.add_(residual)
    return y.relu_() if relu else y


def summary(times):
    s = sorted(times)
    pick = lambda q: s[min(len(s) - 1, int(q * len(s)))]
    return dict(median_us=statistics.median(times), min_us=s[0], p10_us=pick(0.1), p90_us=pick(0.9))


def compare(row, a, b):
    """whether the 10th - 90th percentile ranges of the variants a and b do not meet, and the ratio of the medians b / a"""
    sa, sb = row[a], row[b]
    row['separated'] = bool(sa['p90_us'] < sb['p10_us'] or sb['p90_us'] < sa['p10_us'])
    row['median_ratio'] = sb['median_us'] / sa['median_us']
    row['verdict'] = (f'{a} faster' if sa['median_us'] < sb['median_us'] else f'{b} faster') if row['separated'] else 'no difference established'


def alternate(variants, sets, repeats, warmup):
    """{name: [us]}: every variant once per round on that round's buffer set, HIP events around each single call"""
    times = {name: [] for name in variants}
    for i in range(warmup + repeats):
        d = sets[i % len(sets)]
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(d)
            b.record()
            b.synchronize()
            if i >= warmup:
                times[name].append(a.elapsed_time(b) * 1e3)
    return times


def queued(fn, sets, reps=12):
    """microseconds per call of `fn`, `reps` calls queued back to back between two events: the device time without the host's share"""
    for d in sets:
        fn(d)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(reps):
        fn(sets[i % len(sets)])
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def op_rows(dev, gen, args):
    rows = []
    stream = torch.cuda.current_stream(dev).cuda_stream
    lib = _lib.load()
    for n in (1, 3):
        for name, C, H, W in STAGES:
            rand = lambda *s: torch.randn(*s, device=dev, generator=gen)
            unit = 4 * n * C * H * W
            nsets = max(2, int(600e6 // (5 * unit)) + 1)
            sets = [dict(x=rand(n, C, H, W), r=rand(n, C, H, W), g=rand(n, C, H, W), y=torch.empty(n, C, H, W, device=dev),
                         gx=torch.empty(n, C, H, W, device=dev), mean=rand(C), var=torch.rand(C, device=dev, generator=gen) + 0.5,
                         weight=rand(C), bias=rand(C)) for _ in range(nsets)]
            ws = torch.empty(lib.mr_bn_act_backward_workspace_bytes(n, C, H, W) // 4, device=dev)
            gw, gb = torch.empty(C, device=dev), torch.empty(C, device=dev)
            for residual in (True, False):
                def forward(fn):
                    def run(d):
                        with torch.no_grad():
                            fn(d['x'], d['mean'], d['var'], d['weight'], d['bias'], EPS, d['r'] if residual else None, True)
                    return run

                def both(fn):
                    def run(d):
                        leaves = [d['x'], d['weight'], d['bias']] + ([d['r']] if residual else [])
                        for t in leaves:
                            t.requires_grad_(True)
                        y = fn(d['x'], d['mean'], d['var'], d['weight'], d['bias'], EPS, d['r'] if residual else None, True)
                        torch.autograd.grad(y, leaves, d['g'])
                        for t in leaves:
                            t.requires_grad_(False)
                    return run

                def c_forward(d):
                    _lib.call('mr_bn_act_forward', x=d['x'].data_ptr(), mean=d['mean'].data_ptr(), var=d['var'].data_ptr(),
                              weight=d['weight'].data_ptr(), bias=d['bias'].data_ptr(), r=d['r'].data_ptr() if residual else None, n_images=n,
                              channels=C, height=H, width=W, eps=EPS, relu=1, y=d['y'].data_ptr(), stream=stream)

                def c_backward(d):
                    _lib.call('mr_bn_act_backward', g=d['g'].data_ptr(), y=d['y'].data_ptr(), x=d['x'].data_ptr(), mean=d['mean'].data_ptr(),
                              var=d['var'].data_ptr(), weight=d['weight'].data_ptr(), n_images=n, channels=C, height=H, width=W, eps=EPS, relu=1,
                              grad_x=d['gx'].data_ptr(), grad_r=d['r'].data_ptr() if residual else None, grad_weight=gw.data_ptr(),
                              grad_bias=gb.data_ptr(), workspace=ws.data_ptr(), stream=stream)

                for what, wrap in (('forward', forward), ('forward_backward', both)):
                    t = alternate(dict(fused=wrap(resnet.bn_act), literal_chain=wrap(literal_chain)), sets, args.repeats, args.warmup)
                    row = dict(op='bn_act', shape=name, images=n, channels=C, height=H, width=W, residual=residual, what=what, buffer_sets=nsets,
                               repeats=args.repeats, fused=summary(t['fused']), literal_chain=summary(t['literal_chain']))
                    compare(row, 'fused', 'literal_chain')
                    units = (3 if residual else 2) if what == 'forward' else (5 if residual else 4)
                    kernel_us = queued(c_forward if what == 'forward' else c_backward, sets)
                    row['counted_bytes'] = units * unit
                    row['kernel_us'] = kernel_us          # forward: its one launch; forward_backward: the backward's two launches alone
                    row['kernel_copy_fraction'] = units * unit / (kernel_us * 1e-6) / COPY_RATE
                    rows.append(row)
                    print(f'{name} N={n} residual={int(residual)} {what:16s} fused {row["fused"]["median_us"]:8.1f} us (p10 {row["fused"]["p10_us"]:8.1f}, '
                          f'p90 {row["fused"]["p90_us"]:8.1f})  literal {row["literal_chain"]["median_us"]:8.1f} us (p10 {row["literal_chain"]["p10_us"]:8.1f}, '
                          f'p90 {row["literal_chain"]["p90_us"]:8.1f})  x{row["median_ratio"]:.2f}  {row["verdict"]};  '
                          f'{"forward" if what == "forward" else "backward"} launches queued: {kernel_us:7.1f} us = '
                          f'{100 * row["kernel_copy_fraction"]:.1f}% of the copy rate', flush=True)
            del sets
            torch.cuda.empty_cache()
    return rows


def stem_rows(dev, gen, args):
    rows = []
    C, H, W = STEM
    stream = torch.cuda.current_stream(dev).cuda_stream
    for n in (1, 3):
        unit = 4 * n * C * H * W
        nsets = max(2, int(600e6 // unit) + 1)
        sets = [dict(x=torch.randn(n, C, H, W, device=dev, generator=gen), mean=torch.randn(C, device=dev, generator=gen),
                     var=torch.rand(C, device=dev, generator=gen) + 0.5, weight=torch.randn(C, device=dev, generator=gen),
                     bias=torch.randn(C, device=dev, generator=gen), p=torch.empty(n, C, H // 2, W // 2, device=dev)) for _ in range(nsets)]

        def fused(d):
            with torch.no_grad():
                resnet.bn_relu_maxpool(d['x'], d['mean'], d['var'], d['weight'], d['bias'], EPS)

        def literal(d):
            with torch.no_grad():
                F.max_pool2d(F.batch_norm(d['x'], d['mean'], d['var'], d['weight'], d['bias'], False, 0.1, EPS).relu_(), 3, 2, 1)

        def c_stem(d):
            _lib.call('mr_bn_relu_maxpool_forward', x=d['x'].data_ptr(), mean=d['mean'].data_ptr(), var=d['var'].data_ptr(),
                      weight=d['weight'].data_ptr(), bias=d['bias'].data_ptr(), n_images=n, channels=C, height=H, width=W, eps=EPS,
                      p=d['p'].data_ptr(), stream=stream)

        t = alternate(dict(fused=fused, literal_chain=literal), sets, args.repeats, args.warmup)
        row = dict(op='bn_relu_maxpool', shape='stem', images=n, channels=C, height=H, width=W, what='forward', buffer_sets=nsets,
                   repeats=args.repeats, fused=summary(t['fused']), literal_chain=summary(t['literal_chain']))
        compare(row, 'fused', 'literal_chain')
        kernel_us = queued(c_stem, sets)
        row['counted_bytes'] = unit + unit // 4
        row['kernel_us'] = kernel_us
        row['kernel_copy_fraction'] = row['counted_bytes'] / (kernel_us * 1e-6) / COPY_RATE
        rows.append(row)
        print(f'stem N={n} fused {row["fused"]["median_us"]:8.1f} us (p10 {row["fused"]["p10_us"]:8.1f}, p90 {row["fused"]["p90_us"]:8.1f})  literal '
              f'{row["literal_chain"]["median_us"]:8.1f} us (p10 {row["literal_chain"]["p10_us"]:8.1f}, p90 {row["literal_chain"]["p90_us"]:8.1f})  '
              f'x{row["median_ratio"]:.2f}  {row["verdict"]};  launch queued: {kernel_us:7.1f} us = {100 * row["kernel_copy_fraction"]:.1f}% of the copy rate',
              flush=True)
        del sets
        torch.cuda.empty_cache()
    return rows


def literal_norm_act(norm, x, residual=None, relu=True):
    x = nn.BatchNorm2d.forward(norm, x)
    if residual is not None:
        x += residual
    return F.relu_(x) if relu else x


def literal_stem(x, mean, var, weight, bias, eps):
    return F.max_pool2d(F.batch_norm(x, mean, var, weight, bias, False, 0.1, eps).relu_(), 3, 2, 1)


def network_rows(dev, gen, args):
    fused_parts = (resnet._norm_act, resnet.bn_relu_maxpool, resnet.hip_ok)

    def mode(which):
        resnet._norm_act, resnet.bn_relu_maxpool, resnet.hip_ok = {
            'fused': fused_parts, 'restatement': (fused_parts[0], fused_parts[1], lambda *a, **k: False),
            'literal_module': (literal_norm_act, literal_stem, fused_parts[2])}[which]

    torch.manual_seed(0)
    net = resnet.ResNet(101, frozen_stages=1, norm_eval=True)
    net.init_weights()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.fill_(0.5)
                m.running_var.fill_(0.9)
    net = net.to(dev)
    rows = []
    for n, training in ((1, False), (3, True)):
        net.train(training)
        sets = [torch.randn(n, 3, *IMAGE, device=dev, generator=gen) for _ in range(4)]

        def run(which):
            def call(x):
                mode(which)
                try:
                    with torch.set_grad_enabled(training):
                        outs = net(x)
                        if training:
                            torch.autograd.backward([o.sum() for o in outs[1:]])
                finally:
                    mode('fused')
                net.zero_grad(set_to_none=True)
            return call
        t = alternate({k: run(k) for k in ('fused', 'restatement', 'literal_module')}, sets, args.repeats, args.warmup)
        row = dict(op='ResNet-101', images=n, image=IMAGE, what='forward_backward' if training else 'forward', training=training, frozen_stages=1,
                   repeats=args.repeats, **{k: summary(v) for k, v in t.items()})
        compare(row, 'fused', 'literal_module')
        rows.append(row)
        print(f'ResNet-101 N={n} {row["what"]:16s} ' + '  '.join(f'{k} {row[k]["median_us"] / 1e3:8.2f} ms (p10 {row[k]["p10_us"] / 1e3:8.2f}, p90 '
              f'{row[k]["p90_us"] / 1e3:8.2f})' for k in t) + f'  fused against literal: x{row["median_ratio"]:.3f}  {row["verdict"]}', flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--skip-network', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'resnet_timing needs a HIP device'
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(1)
    rows = op_rows(dev, gen, args) + stem_rows(dev, gen, args)
    if not args.skip_network:
        rows += network_rows(dev, gen, args)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
