"""Host time of ``image_pipeline.prepare_batch``, the launch (``mr_image_prepare``) against its own literal path in torch ops on the device
(DESIGN.md §26), from uint8 host arrays to ``img`` and ``coord_2d`` on the device: one and three KITTI-shaped images (375 x 1242, padded
to 384 x 1248), with and without the photometric distortion (drawn by ``draw_augmentation`` from a fixed seed; two of the three images
flipped).  Every call ends in a device synchronisation, so a figure holds the host's packing and staging, the copy and the device work.

The versions run in one process and ALTERNATE inside every window, after a warm-up of both; a window's figure is the median of its calls,
and the report is the median of the windows with their spread (min .. max), so that a difference can be held against the noise of the
shared host.  Every window runs under its own time limit (an alarm: a window that overruns ends the tool with an error, and nothing is
written).  Python delivers the alarm between bytecodes only: it ends a SLOW window, not one hung inside a device synchronisation, so run
the tool under an outer limit as well (`timeout -k 10 600 python tools/gpu_image_prepare_timing.py`).  Before anything is timed the two
paths' outputs are compared bit for bit.

Writes profiles/image_prepare_timing.json; 'established' says whether the two versions' ranges over the windows are disjoint.
Development aid: python tools/gpu_image_prepare_timing.py [--windows 9] [--calls 20] [--window-limit 120]"""
import argparse
import json
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from monorun_amd import image_pipeline as ip

dev = torch.device('cuda:0')
IMG_H, IMG_W = 375, 1242
MEAN, STD = (95.80, 98.72, 93.82), (83.11, 81.65, 80.54)


class limit:
    """a wall-clock limit on a block: SIGALRM raises when it runs out"""

    def __init__(self, seconds):
        self.seconds = int(seconds)

    def __enter__(self):
        def over(*_):
            raise TimeoutError(f'a timing window ran past its limit of {self.seconds} s')
        self.before = signal.signal(signal.SIGALRM, over)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        signal.signal(signal.SIGALRM, self.before)


def window(fns, calls, seconds):
    """median host time in us of each function over `calls` alternating rounds; every function ends in a device synchronisation"""
    ts = [[] for _ in fns]
    with limit(seconds):
        for _ in range(calls):
            for i, fn in enumerate(fns):
                t0 = time.perf_counter()
                fn()
                ts[i].append(time.perf_counter() - t0)
    return [float(np.median(x)) * 1e6 for x in ts]


def report(per_window):
    a = np.array(per_window)
    return dict(median_us=round(float(np.median(a)), 1), min_us=round(float(a.min()), 1), max_us=round(float(a.max()), 1))


def compare(names, wins):
    out = {name: report([w[i] for w in wins]) for i, name in enumerate(names)}
    a, b = out[names[0]], out[names[1]]
    out['established'] = bool(a['max_us'] < b['min_us'] or b['max_us'] < a['min_us'])      # the windows' ranges do not overlap
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=9)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--window-limit', type=int, default=120)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'image_prepare_timing.json'))
    args = ap.parse_args()
    assert args.windows >= 9, 'at least nine windows'
    rng = np.random.RandomState(0)
    images = [rng.randint(0, 256, (IMG_H, IMG_W, 3)).astype(np.uint8) for _ in range(3)]
    drawn = [ip.draw_augmentation(np.random.RandomState(11 + n))[1] for n in range(3)]
    out = dict(device=torch.cuda.get_device_name(0), image=[IMG_H, IMG_W], windows=args.windows, calls_per_window=args.calls,
               window_limit_s=args.window_limit, source_bytes_per_image=IMG_H * IMG_W * 3, output_bytes_per_image=5 * 4 * 384 * 1248)
    for n_images in (1, 3):
        for distort in (False, True):
            kw = dict(images=images[:n_images], mean=MEAN, std=STD, to_rgb=True, size_divisor=32, flips=[False, True, True][:n_images],
                      photometric=drawn[:n_images] if distort else None, device=dev)

            def call(path):
                res = ip.prepare_batch(**kw, path=path)
                torch.cuda.synchronize()
                return res
            with limit(args.window_limit):
                fast, lit = call('fast'), call('literal')
            same = bool(torch.equal(fast[0].view(torch.int32), lit[0].view(torch.int32)) and torch.equal(fast[1].view(torch.int32), lit[1].view(torch.int32)))
            fns = (lambda: call('literal'), lambda: call('fast'))
            window(fns, 3, args.window_limit)                                              # warm-up of both
            key = f'{n_images}_image{"s" if n_images > 1 else ""}_{"distorted" if distort else "plain"}'
            out[key] = compare(('literal', 'fast'), [window(fns, args.calls, args.window_limit) for _ in range(args.windows)])
            out[key]['outputs_bitwise_equal'] = same
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
