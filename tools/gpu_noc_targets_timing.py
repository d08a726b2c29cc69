"""The dense NOC targets at the training step's shape — 3 images of 384x1248, 6 ground truths each, 384 positives, 28x28
bins — by the fused path (``noc_targets.noc_targets``: two HIP launches over the raw maps) and by the composed path
(``noc_targets.noc_targets_composed``: encode every whole map in torch, ``mr_roi_align_avg`` twice per image, torch), alternated in one
process; prints the host wall medians of synchronised steps (us) and whether the two results are equal bit for bit.  Development aid;
for kernel times and launch counts run it under ``rocprofv3 --kernel-trace --stats -- python tools/gpu_noc_targets_timing.py``."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

IMAGES, H, W, G, N, DENSE, STEPS = 3, 384, 1248, 6, 384, 28, 100


def workload(dev, seed=15):
    import torch
    rng = np.random.default_rng(seed)
    per = [N // IMAGES] * IMAGES
    per[0] += N - sum(per)
    d = dict(pos_bboxes=[], gt_inds=[], coords=[], masks=[], dims=[], flips=[])
    for j, n in enumerate(per):
        # objects of 30 .. 300 pixels, LiDAR-like: a fifth of the pixels inside a box carry a return
        m = np.zeros((G, 1, H, W), np.float32)
        boxes = []
        for g in range(G):
            bw, bh = rng.uniform(30, 300), rng.uniform(30, 150)
            x0, y0 = rng.uniform(0, W - bw), rng.uniform(0, H - bh)
            boxes.append((x0, y0, x0 + bw, y0 + bh))
            ys, xs = slice(int(y0), int(y0 + bh)), slice(int(x0), int(x0 + bw))
            m[g, 0, ys, xs] = (rng.random(m[g, 0, ys, xs].shape) < 0.2)
        c = (rng.uniform(-2, 2, (G, 3, H, W)).astype(np.float32) * m).astype(np.float32)
        gt = rng.integers(0, G, n)
        r = np.array([boxes[g] for g in gt], np.float32) + rng.normal(0, 4, (n, 4)).astype(np.float32)      # jittered proposals
        d['coords'].append(torch.from_numpy(c).to(dev)); d['masks'].append(torch.from_numpy(m).to(dev))
        d['dims'].append(torch.from_numpy(rng.uniform(1.4, 4.6, (G, 7)).astype(np.float32)).to(dev)[:, :3])
        d['pos_bboxes'].append(torch.from_numpy(r).to(dev)); d['gt_inds'].append(torch.from_numpy(gt).to(dev))
        d['flips'].append(bool(j % 2))
    return d


def main():
    import torch
    from monorun_amd import noc_targets as nt
    dev = torch.device('cuda:0')
    d = workload(dev)
    args = (d['pos_bboxes'], d['gt_inds'], d['coords'], d['masks'], d['dims'], d['flips'], DENSE)
    paths = (('fused', nt.noc_targets), ('composed', nt.noc_targets_composed))
    res = {}
    for name, fn in paths:
        for _ in range(3):
            res[name] = fn(*args)
    torch.cuda.synchronize()
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(res['fused'], res['composed']))
    ts = {name: [] for name, _ in paths}
    for _ in range(STEPS):
        for name, fn in paths:
            t0 = time.perf_counter()
            fn(*args)
            torch.cuda.synchronize()
            ts[name].append(time.perf_counter() - t0)
    print(json.dumps(dict(shape=dict(images=IMAGES, H=H, W=W, gt_per_image=G, positives=N, dense_size=DENSE), steps=STEPS, equal_bits=same,
                          positive_bins=int((res['fused'][1] > 0).sum()),
                          **{f'{k}_host_us_median': round(float(np.median(v)) * 1e6, 1) for k, v in ts.items()})))


if __name__ == '__main__':
    main()
