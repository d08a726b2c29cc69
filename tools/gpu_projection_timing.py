"""Forward + backward of the NOC head's training loss at n = 384 (one training step's positives) and n = 4096, 28x28:
the HIP path (``UncertProjectionHead`` -> encode -> ``RobustKLLoss``, backward) against the torch restatement of the same formulas
(``uncert_projection`` -> encode -> ``robust_kl_loss``), alternated in one process; prints host wall times (median of synchronised
steps, us).  Development aid.

Kernel times and launch counts: run it under ``rocprofv3 --kernel-trace --stats -d DIR -- python tools/gpu_projection_timing.py``,
then ``python tools/gpu_projection_timing.py --count DIR/<...>_results.db`` (or a ``--output-format csv`` kernel_trace.csv).  Before timing, the script runs COUNT_STEPS steps
of each path and size in separate phases, 0.3 s apart; ``--count`` splits the trace at those gaps and prints the launches per step of
each phase (the head's torch encode included) and of the five HIP kernels."""
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
OURS = ('uncert_projection_kernel', 'uncert_projection_backward_kernel', 'robust_kl_partial_kernel', 'robust_kl_fold_kernel',
        'robust_kl_backward_kernel')


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
    from monorun_amd.losses import robust_kl_loss
    from monorun_amd.projection_head import UncertProjectionHead, uncert_projection
    dev = torch.device('cuda:0')

    def inputs(n, seed):
        rng = np.random.default_rng(seed)
        t = np.stack([rng.uniform(-12, 12, n), rng.uniform(1, 2, n), rng.uniform(5, 45, n)], 1)
        T = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dev)
        return dict(c3d=T(rng.normal(0, 1, (n, 3, 28, 28))), ls=T(rng.normal(0, 1, (n, 2, 28, 28))),
                    pose=T(np.concatenate([t, rng.uniform(-3, 3, (n, 1))], 1)),
                    K=T(np.tile([[721.5, 0, 609.6], [0, 721.5, 172.9], [0, 0, 1]], (n, 1, 1))), img=T(np.tile([[375.0, 1242.0]], (n, 1))),
                    roi=T(rng.uniform(0, 1242, (n, 2, 28, 28))), dist=T(np.linalg.norm(t, axis=1, keepdims=True)))

    head = UncertProjectionHead().to(dev)
    buf = torch.ones((), device=dev)

    def hip_step(d):
        c3d, ls = d['c3d'].detach().requires_grad_(True), d['ls'].detach().requires_grad_(True)
        proj = head(c3d, d['pose'], d['K'], d['img'])
        head.loss(proj, ls, d['roi'], d['dist'])['loss_proj'].backward()

    def torch_step(d):
        c3d, ls = d['c3d'].detach().requires_grad_(True), d['ls'].detach().requires_grad_(True)
        proj = uncert_projection(c3d, d['pose'], d['K'], d['img'])
        err = head.proj_error_coder.encode(proj - d['roi'], d['dist'])
        robust_kl_loss(err, 0, logstd=ls, momentum=0.1, mean_inv_std=buf).mean().backward()

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
