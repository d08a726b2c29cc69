#!/usr/bin/env python3
"""Times the fused RoI extraction launches against the only alternative the library offered before them, on the same
device, at the workload's shapes: 256 channels, a 384 x 1248 image, strides 2 .. 32 (maps of 192 x 624 .. 12 x 39), for
K = 1536 RoIs at 7 x 7 and K = 384 at 14 x 14 over 3 images (a training step), K = 1000 at 7 x 7 and K = 100 at 14 x 14 over one (a test
image).  Forward alternative: the per-level composition of ``roi_align_avg`` with ``nonzero`` and ``index_copy`` (mmdet's structure: one
blocking ``nonzero`` and one launch per level).  Backward alternative: autograd through ``roi_extract_torch``.

HIP events around single calls, after 5 warm-ups; the median of the repeats; a rotating set of map buffers larger than the 256 MiB
Infinity Cache.  Reports microseconds and the achieved algorithmic bytes/s as a fraction of the 6.29 TB/s the device copies at — forward:
the RoIs' footprints read once (taken as the output's size: a bin reads about a pixel's worth per channel at these scales) and the output
written; backward: grad_out read and every grad_feats element written once, the launch's floor.  Not a test: asserts nothing about speed.

    python tools/roi_extract_timing.py [--repeats 40] [--torch-rois 64] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from monorun_amd import roi_extractor as R  # noqa: E402
from monorun_amd.pose_head import roi_align_avg  # noqa: E402

COPY_RATE = 6.29e12
C, IMAGE, STRIDES, FINEST = 256, (384, 1248), (2, 4, 8, 16, 32), 28
SHAPES = ((1536, 7, 3), (384, 14, 3), (1000, 7, 1), (100, 14, 1))          # K, output size, images


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


def make_rois(k, n, gen, dev):
    """proposals of a street scene: scales log-uniform in 16 .. 400 px, aspect ratios in 1/2 .. 2, centres inside the image"""
    u = torch.rand(k, 4, generator=gen, device=dev)
    scale = 16.0 * (400.0 / 16.0) ** u[:, 0]
    aspect = 2.0 ** (2 * u[:, 1] - 1)
    w, h = scale * aspect.sqrt(), scale / aspect.sqrt()
    cx, cy = u[:, 2] * IMAGE[1], u[:, 3] * IMAGE[0]
    img = torch.randint(0, n, (k,), generator=gen, device=dev).float()
    return torch.stack((img, cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2), dim=1)


def composed(feats, rois, size):
    """the per-level composition: levels, then per level nonzero (blocks the host), the single-map kernel, index_copy"""
    levels = R.map_roi_levels(rois, len(feats), FINEST)
    out = feats[0].new_zeros(rois.shape[0], C, size, size)
    for l, f in enumerate(feats):
        idx = torch.nonzero(levels == l, as_tuple=False).flatten()
        if idx.numel():
            out.index_copy_(0, idx, roi_align_avg(f, rois[idx], size, 1.0 / STRIDES[l], 0, True))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=40)
    ap.add_argument('--torch-rois', type=int, default=64, help='RoIs of the autograd-through-the-restatement backward (a python loop per RoI); '
                    'its time is reported as measured and scaled to K')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'roi_extract_timing needs a HIP device'
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(1)
    sizes = [(-(-IMAGE[0] // s), -(-IMAGE[1] // s)) for s in STRIDES]
    rows = []
    for k, size, n in SHAPES:
        map_bytes = 4 * n * C * sum(h * w for h, w in sizes)
        out_bytes = 4 * k * C * size * size
        nsets = max(2, int(600e6 // map_bytes) + 1)
        sets = [dict(feats=[torch.randn(n, C, h, w, device=dev, generator=gen) for h, w in sizes], rois=make_rois(k, n, gen, dev),
                     go=torch.randn(k, C, size, size, device=dev, generator=gen)) for _ in range(nsets)]
        assert R.hip_ok(sets[0]['feats'], sets[0]['rois'], size)
        levels = torch.bincount(R.map_roi_levels(sets[0]['rois'], 5, FINEST), minlength=5).tolist()

        def fused_fwd(d):
            with torch.no_grad():
                R.roi_extract(d['feats'], d['rois'], STRIDES, FINEST, size)

        def composed_fwd(d):
            with torch.no_grad():
                composed(d['feats'], d['rois'], size)

        def fused_bwd_sets():
            out = []
            for d in sets:
                feats = [f.requires_grad_(True) for f in d['feats']]
                out.append(dict(y=R.roi_extract(feats, d['rois'], STRIDES, FINEST, size), feats=feats, go=d['go']))
            return out

        def bwd(d):
            torch.autograd.grad(d['y'], d['feats'], d['go'], retain_graph=True)

        f_med, f_min = timed(fused_fwd, sets, args.repeats)
        c_med, c_min = timed(composed_fwd, sets, args.repeats)
        bs = fused_bwd_sets()
        b_med, b_min = timed(bwd, bs, args.repeats)
        del bs
        kt = min(k, args.torch_rois)
        d = sets[0]
        y = R.roi_extract_torch(d['feats'], d['rois'][:kt], STRIDES, FINEST, size)
        t_med, _ = timed(bwd, [dict(y=y, feats=d['feats'], go=d['go'][:kt])], 3, warmup=1)
        del y
        for s in sets:
            for f in s['feats']:
                f.requires_grad_(False)
        fwd_bytes, bwd_bytes = 2 * out_bytes, out_bytes + map_bytes
        rows.append(dict(k=k, size=size, images=n, rois_per_level=levels, buffer_sets=nsets,
                         forward_us=f_med, forward_min_us=f_min, composed_forward_us=c_med, composed_forward_min_us=c_min,
                         backward_us=b_med, backward_min_us=b_min, torch_backward_rois=kt, torch_backward_us=t_med,
                         torch_backward_scaled_us=t_med * k / kt, forward_bytes=fwd_bytes, backward_bytes=bwd_bytes,
                         forward_copy_fraction=fwd_bytes / (f_med * 1e-6) / COPY_RATE, backward_copy_fraction=bwd_bytes / (b_med * 1e-6) / COPY_RATE))
        r = rows[-1]
        print(f"K={k:5d} {size:2d}x{size:<2d} N={n}  forward {f_med:8.1f} us ({100 * r['forward_copy_fraction']:5.1f}% of the copy rate; per-level "
              f"composition {c_med:8.1f} us)   backward {b_med:9.1f} us ({100 * r['backward_copy_fraction']:5.1f}%; autograd through the "
              f"restatement {t_med:10.1f} us for {kt} RoIs)   RoIs per level {levels}   [{nsets} buffer sets]", flush=True)
        del sets
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
