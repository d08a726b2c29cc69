#!/usr/bin/env python3
"""G17: the NOC head's training decode chain with its gradients, from the reference's own code.

Runs only in the authoring container (needs the reference tree, read-only; loaded by file path under the mmcv / mmdet stubs of
make_golden.py, nothing of it is copied).  The fixture is data: seeded inputs, what the reference's functions returned for them, and
what torch autograd gave through them.

    python tests/golden/make_golden_noc_train.py      # rewrites tests/golden/g17_noc_train_decode.npz

The chain is make_golden.py's G3 chain — the flip branch of FCNNOCDecoder.forward restated (it is not separable), then the
reference's slice_pred, MultiClassNormDimCoder.decode, NOCCoder.decode and DistanceInvarProjErrorCoder.decode_logstd (target_std
0.15) — with leaves that require grad and, in group A, the ground-truth distances.

Group a: 6 objects at 28x28, 3 classes: labels 0 1 2 0 1 2, flip F T F T F T (all six (label, flip) pairs), dim_var given, distances
given (object 3: 0.05 < distance_min).  Group b: 4 objects at 7x9, class-agnostic
(10 channels, labels 0 2 1 0 pick the dim statistics only), flip T F F T, dim_var None, distances None.

all_pred and the upstream gradients hold float16-representable values (stored as float16, used as float32: lossless, half the
size).  Recorded per group: the inputs, the seven outputs, one fixed random upstream gradient per output, and the gradients of
sum(output * upstream) to all_pred, dim and dim_var.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

OUT = HERE
OUTPUTS = ('noc_pred', 'proj_logstd', 'coords_3d', 'coords_3d_var', 'proj_logstd_px', 'dims', 'dims_var')


def f16(a):
    return np.asarray(a, np.float32).astype(np.float16)


def chain(ref, all_pred, labels, flip, dim, dim_var, distances, num_classes, class_agnostic):
    n, ch, h, w = all_pred.shape
    v = all_pred.view(n, 2, ch // 2, h, w)
    inds = torch.arange(0, n, dtype=torch.long)
    sel = v[inds, inds.new_tensor(flip)]                     # fcn_noc_decoder.py:225-235
    fake = types.SimpleNamespace(class_agnostic=class_agnostic, num_classes=num_classes, noc_channels=3, uncert_channels=2)
    noc_pred, noc_var, proj_logstd = ref['dec'].FCNNOCDecoder.slice_pred(fake, sel, labels)
    assert noc_var is None
    dims, dims_var = ref['dim'].MultiClassNormDimCoder().decode(dim, dim_var, labels)
    c3d, c3d_var = ref['noc'].NOCCoder().decode(noc_pred, None, dims, dims_var, flip)
    coder = ref['prj'].DistanceInvarProjErrorCoder(ref_length=1.6, ref_focal_y=722, target_std=0.15)
    px = coder.decode_logstd(proj_logstd, c3d_var, distances)
    return dict(noc_pred=noc_pred, proj_logstd=proj_logstd, coords_3d=c3d, coords_3d_var=c3d_var, proj_logstd_px=px, dims=dims,
                dims_var=dims_var)


def record(ref, rng, tag, n, h, w, labels, flip, num_classes, class_agnostic, with_var, distances):
    cn = 1 if class_agnostic else num_classes
    all_pred = f16(rng.normal(0, 1, (n, 2 * cn * 5, h, w)))
    dim = rng.normal(0, 1, (n, 3)).astype(np.float32)
    dim_var = (rng.uniform(0.01, 0.2, (n, 3)) ** 2).astype(np.float32) if with_var else None
    ap = torch.tensor(all_pred.astype(np.float32), requires_grad=True)
    dm = torch.tensor(dim, requires_grad=True)
    dv = torch.tensor(dim_var, requires_grad=True) if with_var else None
    dist = torch.tensor(distances) if distances is not None else None
    out = chain(ref, ap, torch.tensor(labels), list(map(bool, flip)), dm, dv, dist, num_classes, class_agnostic)
    rec = {'all_pred': all_pred, 'labels': np.asarray(labels, np.int64), 'flip': np.asarray(flip, bool), 'dim': dim}
    if with_var:
        rec['dim_var'] = dim_var
    if distances is not None:
        rec['distances'] = distances
    loss = 0
    for k in OUTPUTS:
        if out[k] is None:
            continue
        g = f16(rng.normal(0, 1, tuple(out[k].shape)))
        rec['up_' + k] = g
        rec[k] = out[k].detach().numpy()
        loss = loss + (out[k] * torch.tensor(g.astype(np.float32))).sum()
    loss.backward()
    rec['grad_all_pred'] = ap.grad.numpy()
    rec['grad_dim'] = dm.grad.numpy()
    if with_var:
        rec['grad_dim_var'] = dv.grad.numpy()
    print(f'G17 {tag}: n = {n}, {h}x{w}, grad_all_pred non-zero in {int((ap.grad != 0).any(-1).any(-1).sum())} of {n * 2 * cn * 5} channels')
    return {f'{tag}_{k}': v for k, v in rec.items()}


def main():
    ref = mg.load_reference()
    rng = np.random.default_rng(17)
    out = {}
    dist_a = np.array([[12.5], [33.0], [4.2], [0.05], [61.0], [173.28]], np.float32)        # object 3 is clamped to distance_min = 0.1
    out.update(record(ref, rng, 'a', 6, 28, 28, [0, 1, 2, 0, 1, 2], [False, True, False, True, False, True], 3, False, True, dist_a))
    out.update(record(ref, rng, 'b', 4, 7, 9, [0, 2, 1, 0], [True, False, False, True], 3, True, False, None))
    path = os.path.join(OUT, 'g17_noc_train_decode.npz')
    np.savez_compressed(path, **out)
    print('G17:', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
