"""Time of the aligned 3-D IoU launch (``mr_bbox3d_overlaps_aligned``) at N = 512 (a training batch's positives) and N = 100 000, and
the host time of the pose head's ``loss()`` around it at N = 512.  Kernel times: run under
``rocprofv3 --kernel-trace --stats -- python tools/gpu_iou3d_timing.py`` (``bbox3d_overlaps_aligned_kernel`` in the stats); the script
itself prints host wall times (median of synchronised calls, us).  Development aid."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from monorun_amd.iou3d import bbox3d_overlaps_aligned
from monorun_amd.pose_head import UncertPropPnPOptimizer

dev = torch.device('cuda:0')


def pairs(n, seed):
    rng = np.random.default_rng(seed)
    b = np.stack([rng.uniform(3.0, 4.8, n), rng.uniform(1.3, 1.9, n), rng.uniform(1.4, 1.9, n), rng.uniform(-10, 10, n),
                  rng.uniform(0.5, 2.5, n), rng.uniform(5, 50, n), rng.uniform(-np.pi, np.pi, n)], 1).astype(np.float32)
    return torch.from_numpy(b).to(dev)


def host_us(fn, reps=200):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return round(float(np.median(ts)) * 1e6, 1)


out = {}
head = UncertPropPnPOptimizer(loss_calib=dict(type='KLLossMV', loss_weight=0.01)).to(dev)
for n in (512, 100000):
    gt = pairs(n, n)
    g = torch.Generator().manual_seed(1)
    yaw = gt[:, 6:7] + 0.1 * torch.randn(n, 1, generator=g).to(dev)
    t = gt[:, 3:6] + 0.3 * torch.randn(n, 3, generator=g).to(dev)
    dims = gt[:, :3] * 1.05
    a = torch.randn(n, 4, 4, generator=g).to(dev) * 0.2
    cov = a @ a.transpose(1, 2) + 0.01 * torch.eye(4, device=dev)
    ret = torch.ones(n, dtype=torch.bool, device=dev)
    boxes, qboxes = gt[:, [3, 4, 5, 0, 1, 2, 6]], torch.cat((t, dims, yaw), 1)
    r = dict(iou_op_host_us=host_us(lambda: bbox3d_overlaps_aligned(boxes, qboxes)))
    if n == 512:
        yt, tt = head.get_targets(gt)
        r['loss_host_us'] = host_us(lambda: head.loss(ret, yaw, t, cov, dims, yt, tt, gt))
    out[f'N{n}'] = r
print(json.dumps(out))
