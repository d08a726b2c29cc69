"""Forward + backward of the NOC head's training decode at n = 384 (one training step's positives) and n = 4096, 28x28,
3 classes, dim_var and distances given: the HIP path (``noc_head.decode_for_training``: one launch forward, one backward) against the
torch restatement (``decode_for_training_torch``), alternated in one process; prints host wall times (median of synchronised steps,
us).  A step is the decode, a weighted sum of its seven outputs (the same torch ops on both paths) and backward().  Development aid.

Kernel times and launch counts: run it under ``rocprofv3 --kernel-trace --stats -d DIR -- python tools/gpu_noc_decode_train_timing.py``,
then ``python tools/gpu_noc_decode_train_timing.py --count DIR/<...>_results.db`` (or a ``--output-format csv`` kernel_trace.csv).  Before
timing, the script runs COUNT_STEPS steps of each path and size in separate phases, 0.3 s apart; ``--count`` splits the trace at those
gaps and prints the launches per step of each phase (the weighted sum's torch kernels included) and of the two HIP kernels."""
import argparse
import csv
import json
import os
import re
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

COUNT_STEPS = 10
SIZES = (384, 4096)
OURS = ('noc_decode_train_kernel', 'noc_decode_train_backward_kernel')


def _dispatches(path):
    """[(kernel name, start ns, end ns)] of a rocprofv3 kernel trace: its SQLite database (the default output) or kernel_trace.csv"""
    if path.endswith('.db'):
        import sqlite3
        rows = sqlite3.connect(path).execute('select name, start, end from kernels').fetchall()
    else:
        rows = [(r['Kernel_Name'], int(r['Start_Timestamp']), int(r['End_Timestamp'])) for r in csv.DictReader(open(path))]
    return sorted(rows, key=lambda r: r[1])


def count(path):
    phases, last = [], None
    for name, start, end in _dispatches(path):
        if last is None or start - last > 200_000_000:      # ns: the 0.3 s pauses between the phases
            phases.append([])
        phases[-1].append((name, end - start))
        last = end
    names = [f'{p}_n{n}' for n in SIZES for p in ('hip', 'torch')]
    out = {}
    for name, ph in zip(names, phases[-len(names) - 1:-1]):        # the last phase is the timing loop
        ours = {k: [d for kn, d in ph if re.search(r'(^|::|\d)' + k + r'(E|\()', kn)] for k in OURS}     # demangled or mangled
        out[name] = dict(launches_per_step=len(ph) / COUNT_STEPS, hip_kernels_per_step=sum(map(len, ours.values())) / COUNT_STEPS,
                         gpu_busy_us_per_step=round(sum(d for _, d in ph) / COUNT_STEPS / 1e3, 1),
                         kernel_median_us={k: round(float(np.median(v)) / 1e3, 2) for k, v in ours.items() if v})
    print(json.dumps(dict(phases=len(phases), counts=out), indent=1))


def main():
    import torch
    from monorun_amd.noc_head import decode_for_training, decode_for_training_torch
    dev = torch.device('cuda:0')

    def inputs(n, seed):
        rng = np.random.default_rng(seed)
        T = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dev)
        d = dict(all_pred=T(rng.normal(0, 1, (n, 30, 28, 28))), labels=torch.from_numpy(np.arange(n) % 3).to(dev),
                 flip=torch.from_numpy((np.arange(n) // 3) % 2 == 1).to(dev), dim=T(rng.normal(0, 1, (n, 3))),
                 dim_var=T(rng.uniform(0.01, 0.2, (n, 3)) ** 2), dist=T(rng.uniform(3, 80, (n, 1))))
        d['ups'] = [T(rng.normal(0, 1, s)) for s in ((n, 3, 28, 28), (n, 2, 28, 28), (n, 3, 28, 28), (n, 3, 28, 28), (n, 2, 28, 28), (n, 3), (n, 3))]
        return d

    def step(fn, d):
        ap, dim, dv = (d[k].detach().requires_grad_(True) for k in ('all_pred', 'dim', 'dim_var'))
        out = fn(ap, d['labels'], d['flip'], dim, dv, d['dist'])
        sum((o * u).sum() for o, u in zip(out.values(), d['ups'])).backward()

    def hip_step(d):
        step(decode_for_training, d)

    def torch_step(d):
        step(decode_for_training_torch, d)

    data = {n: inputs(n, n) for n in SIZES}
    for d in data.values():                             # warm-up: library load, allocator, torch's kernels
        for _ in range(3):
            hip_step(d); torch_step(d)
    torch.cuda.synchronize()
    time.sleep(0.3)
    for n in SIZES:                                     # launch-count phases, 0.3 s apart
        for fn in (hip_step, torch_step):
            for _ in range(COUNT_STEPS):
                fn(data[n])
            torch.cuda.synchronize()
            time.sleep(0.3)
    out = {}
    for n in SIZES:
        ts = {'hip': [], 'torch': []}
        for _ in range(200):
            for name, fn in (('hip', hip_step), ('torch', torch_step)):
                t0 = time.perf_counter()
                fn(data[n])
                torch.cuda.synchronize()
                ts[name].append(time.perf_counter() - t0)
        out[f'n{n}'] = {f'{k}_fwd_bwd_host_us': round(float(np.median(v)) * 1e6, 1) for k, v in ts.items()}
    print(json.dumps(out))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--count', help='the results.db or kernel_trace.csv of a rocprofv3 --kernel-trace run over this script')
    a = ap.parse_args()
    count(a.count) if a.count else main()
