"""G18 (tests/golden/g18_noc_targets.npz, written by make_golden_noc_targets.py) as the NOC-target tests use it: the groups' inputs rebuilt
as torch tensors, the recorded results, and random workloads for the shape sweeps.  No test in here."""
import functools
import os
import types

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
EPS_T = 1e-4


@functools.lru_cache(maxsize=None)
def g18():
    return dict(np.load(os.path.join(GOLDEN, 'g18_noc_targets.npz')))


def group(tag, device='cpu'):
    """The inputs of group 'a' or 'b' as noc_targets takes them, and the recorded results (read-only: shared between tests)."""
    g = g18()
    vals = g['mask_values']
    n_img = len(g[f'{tag}_flips'])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)      # noqa: E731
    ins = dict(pos_bboxes=[], gt_inds=[], coords=[], masks=[], dims=[], flips=[bool(f) for f in g[f'{tag}_flips']],
               dense_size=tuple(int(v) for v in g[f'{tag}_dense_size']))
    for k in range(n_img):
        m = vals[g[f'{tag}_img{k}_mask_index']]
        c = (g[f'{tag}_img{k}_raw'].astype(np.float32) * m).astype(np.float32)
        ins['coords'].append(t(c)); ins['masks'].append(t(m)); ins['dims'].append(t(g[f'{tag}_img{k}_dimensions']))
        ins['pos_bboxes'].append(t(g[f'{tag}_img{k}_rois'])); ins['gt_inds'].append(t(g[f'{tag}_img{k}_gt_inds']))
    rec = types.SimpleNamespace(
        targets=t(g[f'{tag}_targets']), weights=t(g[f'{tag}_weights']), noc_pred=t(g[f'{tag}_noc_pred'].astype(np.float32)),
        loss_mean=float(g[f'{tag}_loss_mean']), loss_sum=float(g[f'{tag}_loss_sum']), grad_pred=t(g[f'{tag}_grad_pred']),
        beta=float(g[f'{tag}_beta']), loss_weight=float(g[f'{tag}_loss_weight']), upstream=float(g[f'{tag}_upstream']))
    return ins, rec


def call_args(ins):
    return (ins['pos_bboxes'], ins['gt_inds'], ins['coords'], ins['masks'], ins['dims'], ins['flips'], ins['dense_size'])


def loss_terms64(rec, reduction):
    """The weighted element losses of the recorded form (weight = weights) as fp32 terms, their fp64 sum reduced, and the deviation of
    torch's fp32 reduction of the same terms from it (relative): the measure the HIP loss's tolerance is taken from."""
    from monorun_amd.losses import smooth_l1_loss_mod
    terms = smooth_l1_loss_mod(rec.noc_pred.cpu(), rec.targets.cpu(), rec.beta) * rec.weights.cpu()
    s64 = terms.double().sum().item()
    s32 = terms.sum().item()
    if reduction == 'mean':
        s64, s32 = s64 / terms.numel(), terms.mean().item()
    return rec.loss_weight * s64, abs(s32 - s64) / abs(s64)


def random_workload(seed, sizes, n_per_image, G=2, device='cpu'):
    """Images of the given (H, W) sizes with G ground truths each and n_per_image[j] positives (0 allowed): masks in {0, 1e-5, 0.3, 1},
    RoIs inside and across the borders.  Pooled mask values near the threshold are not excluded: for fused-against-composed, which
    compute the same numbers."""
    rng = np.random.default_rng(seed)
    out = dict(pos_bboxes=[], gt_inds=[], coords=[], masks=[], dims=[], flips=[])
    for (H, W), n in zip(sizes, n_per_image):
        m = rng.choice(np.array([0.0, 1e-5, 0.3, 1.0], np.float32), (G, 1, H, W), p=[0.3, 0.05, 0.25, 0.4])
        c = (rng.uniform(-2, 2, (G, 3, H, W)).astype(np.float32) * m).astype(np.float32)
        d = rng.uniform(1.4, 4.6, (G, 7)).astype(np.float32)
        cx, cy = rng.uniform(0, W, n), rng.uniform(0, H, n)
        hw_, hh = rng.uniform(0.3, W * 0.7, n), rng.uniform(0.3, H * 0.7, n)
        r = np.stack([cx - hw_, cy - hh, cx + hw_, cy + hh], 1).astype(np.float32)
        out['coords'].append(torch.from_numpy(c).to(device)); out['masks'].append(torch.from_numpy(m).to(device))
        out['dims'].append(torch.from_numpy(d).to(device)[:, :3])                       # a strided view, as gt_bboxes_3d[:, :3] is
        out['pos_bboxes'].append(torch.from_numpy(r).to(device)); out['gt_inds'].append(torch.from_numpy(rng.integers(0, G, n)).to(device))
        out['flips'].append(bool(rng.integers(0, 2)))
    return out
