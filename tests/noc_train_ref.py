"""Shared by the training decode's tests (test_noc_train_decode_cpu.py, test_gpu_noc_train_decode.py): fixture G17's groups as tensors,
the numpy restatement of the pixel log-std with the specified exp / log, and the tolerances."""
import os

import numpy as np
import torch

from oracle import oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
OUTPUTS = ('noc_pred', 'proj_logstd', 'coords_3d', 'coords_3d_var', 'proj_logstd_px', 'dims', 'dims_var')
GROUPS = {'a': dict(num_classes=3, class_agnostic=False), 'b': dict(num_classes=3, class_agnostic=True)}

# library exp / log against the reference's values: the tolerance test_gpu_decode_and_head.py uses against G3
RTOL_EXP_LOG = 3e-6
# Gradients: max |g - ref| <= GRAD_TOL * max |ref| per gradient tensor.  Measured (test_noc_train_decode_cpu.py::
# test_fp32_autograd_against_fp64_on_g17 prints it): fp32 autograd of the restatement deviates from its fp64 autograd on G17's inputs
# by at most 1.237e-7 of the largest element (group a, grad_dim_var; grad_all_pred 1.140e-7, grad_dim 9.55e-8); the bound is 4 x that — fp32 rounding, not a property of the code under test.
GRAD_FP32_DEVIATION = 1.237e-7
GRAD_TOL = 4 * GRAD_FP32_DEVIATION


def load_g17():
    return dict(np.load(os.path.join(GOLDEN, 'g17_noc_train_decode.npz')))


def group(g, tag, dev='cpu', dtype=torch.float32):
    """(inputs, kwargs, upstream gradients, expected outputs and gradients) of one group; the float16-stored arrays as `dtype`."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).to(device=dev, dtype=dtype)
    get = lambda k: g.get(f'{tag}_{k}')
    ins = dict(all_pred=T(get('all_pred')), labels=torch.from_numpy(get('labels')).to(dev), flip=torch.from_numpy(get('flip')).to(dev),
               dim=T(get('dim')), dim_var=T(get('dim_var')) if get('dim_var') is not None else None,
               distances=T(get('distances')) if get('distances') is not None else None)
    ups = {k: T(get('up_' + k)) for k in OUTPUTS if get('up_' + k) is not None}
    want = {k: get(k) for k in OUTPUTS + ('grad_all_pred', 'grad_dim', 'grad_dim_var')}
    return ins, dict(GROUPS[tag]), ups, want


def run(fn, ins, kw, ups=None, leaves=('all_pred', 'dim', 'dim_var')):
    """fn(**ins, **kw) on fresh leaves; with `ups`, backward of sum(output * upstream).  -> (outputs, {name: grad})"""
    ins = dict(ins)
    for k in leaves:
        if ins[k] is not None:
            ins[k] = ins[k].detach().clone().requires_grad_(ups is not None)
    out = fn(ins['all_pred'], ins['labels'], ins['flip'], ins['dim'], ins['dim_var'], ins['distances'], **kw)
    grads = {}
    if ups is not None:
        loss = sum((out[k].to(ups[k].dtype) * ups[k]).sum() for k in ups if out[k] is not None)
        loss.backward()
        grads = {'grad_' + k: ins[k].grad if ins[k].grad is not None else torch.zeros_like(ins[k]) for k in leaves if ins[k] is not None}
    return out, grads


def grad_err(mine, ref):
    """max |mine - ref| / max |ref|"""
    mine = np.asarray(mine.detach().cpu().double() if torch.is_tensor(mine) else mine, np.float64)
    ref = np.asarray(ref.detach().cpu().double() if torch.is_tensor(ref) else ref, np.float64)
    assert mine.shape == ref.shape, (mine.shape, ref.shape)
    return float(np.abs(mine - ref).max() / np.abs(ref).max())


def spec_logstd_px(proj_logstd, coords_3d_var, distances, ref_length=1.6, ref_focal_y=722, target_std=0.15, distance_min=0.1,
                   epistemic_std_gain=1.0):
    """decode_logstd in numpy float32, one IEEE operation at a time in the kernel's order, with oracle.spec_expf / spec_logf.
    proj_logstd (n, 2, h, w), coords_3d_var (n, 3, h, w) | None, distances (n, 1) | None."""
    f = np.float32
    sd = ref_length * ref_focal_y * target_std
    ls = np.asarray(proj_logstd, f)
    n = ls.shape[0]
    if distances is None:
        d = np.full((n, 1, 1, 1), f(sd), f)
    else:
        d = np.asarray(distances, f).reshape(n, 1, 1, 1)
        d = np.where(d < f(distance_min), f(distance_min), d)
    if coords_3d_var is None:
        return ls + orc.spec_logf(f(sd) / d)
    v = np.asarray(coords_3d_var, f)
    v2 = np.stack([f(0.5) * (v[:, 0] + v[:, 2]), v[:, 1]], 1)
    num = v2 * f((ref_focal_y * epistemic_std_gain) ** 2) + orc.spec_expf(f(2.0) * ls) * f(sd ** 2)
    return f(0.5) * orc.spec_logf(num / (d * d))
