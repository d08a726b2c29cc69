#!/usr/bin/env python3
"""G21: the CARAFE op as the real ``mmcv.ops.carafe`` computes it.  Runs only where mmcv's compiled op and a device
it supports exist — not in this repository's image, where ``import mmcv`` fails; the fixture is therefore ABSENT until somebody records
it there, and tests/test_carafe_mmcv_golden.py skips by name meanwhile.

    python tests/golden/make_golden_carafe_mmcv.py      # writes tests/golden/g21_carafe_mmcv.npz

Recorded for every shape of tests/carafe_ref.SHAPES but the largest, on that module's seeded inputs: the normalised masks mmcv's
``CARAFEPack.kernel_normalizer`` makes of the raw logits, ``carafe(features, masks, k, G, s)`` on them, and its gradients to the
features and the masks for the seeded grad_out.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import carafe_ref as ref  # noqa: E402


def main():
    from mmcv.ops.carafe import CARAFEPack, carafe
    dev = torch.device('cuda')
    out = {}
    for i, shape in enumerate(ref.SHAPES[:-1]):
        N, C, H, W, k, G, s = shape
        x, m, go = (torch.from_numpy(a).to(dev) for a in ref.make_inputs(shape))
        pack = CARAFEPack(C, s, up_kernel=k, up_group=G, compressed_channels=4).to(dev)
        masks = pack.kernel_normalizer(m).detach().requires_grad_(True)
        x.requires_grad_(True)
        y = carafe(x, masks, k, G, s)
        y.backward(go)
        out[f's{i}_shape'] = np.array(shape)
        out[f's{i}_masks'], out[f's{i}_out'] = masks.detach().cpu().numpy(), y.detach().cpu().numpy()
        out[f's{i}_grad_features'], out[f's{i}_grad_masks'] = x.grad.cpu().numpy(), masks.grad.cpu().numpy()
    path = os.path.join(HERE, 'g21_carafe_mmcv.npz')
    np.savez_compressed(path, **out)
    print('G21:', os.path.getsize(path) // 1024, 'KiB')


if __name__ == '__main__':
    main()
