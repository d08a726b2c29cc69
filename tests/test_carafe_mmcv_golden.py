"""The CARAFE op against the real mmcv.ops.carafe (G21, tests/golden/make_golden_carafe_mmcv.py).  mmcv's op is a CUDA extension that
does not exist in this image, so the fixture is absent here and the test SKIPS BY NAME, saying which command records it."""
import os

import numpy as np
import pytest
import torch

from tests import carafe_ref as ref

G21 = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g21_carafe_mmcv.npz')


def test_g21_mmcv_carafe_against_the_restatement():
    if not os.path.exists(G21):
        pytest.skip('g21_carafe_mmcv.npz is absent: it can only be recorded where mmcv.ops.carafe (a CUDA extension) and its device exist — '
                    'python tests/golden/make_golden_carafe_mmcv.py')
    from monorun_amd.carafe import carafe, normalize_masks
    g = np.load(G21)
    for i, shape in enumerate(ref.SHAPES[:-1]):
        assert tuple(g[f's{i}_shape']) == shape
        N, C, H, W, k, G, s = shape
        x, m, go = ref.make_inputs(shape)
        want, unit = ref.forward(x, m, k, G, s)
        # mmcv's fp32 op against the definition within the same bound as this project's kernels
        assert ref.ratio(g[f's{i}_out'], want, unit) <= ref.C_BOUND
        masks = normalize_masks(torch.from_numpy(m), k, G, s)
        assert np.allclose(masks.numpy(), g[f's{i}_masks'], rtol=1e-5, atol=1e-7)
        xt = torch.from_numpy(x).requires_grad_(True)
        mt = torch.from_numpy(g[f's{i}_masks'].copy()).requires_grad_(True)
        carafe(xt, mt, k, G, s).backward(torch.from_numpy(go))
        assert np.allclose(xt.grad.numpy(), g[f's{i}_grad_features'], rtol=1e-4, atol=1e-5)
        assert np.allclose(mt.grad.numpy(), g[f's{i}_grad_masks'], rtol=1e-4, atol=1e-5)
