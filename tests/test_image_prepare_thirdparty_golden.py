"""Consumer of G24 (tests/golden/make_golden_image_prepare.py): what OpenCV's colour conversions (through mmcv), mmcv's ``imnormalize``,
``imflip`` and ``impad_to_multiple`` and mmdet's ``PhotoMetricDistortion`` return on the seeded test images, recorded where those packages
exist.  None of them imports where this project is developed, so the fixture is absent and the test SKIPS BY NAME, saying which command
records it; the generator has not been run (the colour conversions are this project's definition, unpinned).

With the fixture present: the index operations (flip, padding) are exact; for every arithmetic stage the largest absolute difference is
printed, and the bar is the measured value recorded in ``MEASURED`` below (and in DESIGN.md §26) plus one float32 ulp of the stage's largest
magnitude.  ``MEASURED`` holds None until somebody has recorded the fixture: the test then fails asking for the measurement, it does not
invent a tolerance."""
import os

import numpy as np
import pytest
import torch

from tests import image_prepare_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
NAME = 'g24_image_prepare_thirdparty.npz'
MEASURED = dict(bgr2hsv=None, hsv2bgr=None, imnormalize=None, distort=None)        # largest |this project - third party| per stage


def _load():
    f = os.path.join(GOLDEN, NAME)
    if not os.path.exists(f):
        pytest.skip(f'{NAME} is absent: it can only be recorded where cv2, mmcv and mmdet 2.x import — python tests/golden/make_golden_image_prepare.py')
    return dict(np.load(f, allow_pickle=False))


def _hsv(x):
    """BGR -> HSV of the literal path's chain, stage by stage: -> (hsv, back)"""
    from monorun_amd.image_pipeline import FLT_EPSILON
    b, g, r = torch.from_numpy(x).unbind(-1)
    V = torch.maximum(b, torch.maximum(g, r))
    d = V - torch.minimum(b, torch.minimum(g, r))
    S = d / (V.abs() + FLT_EPSILON)
    k = (60.0 / (d + FLT_EPSILON).double()).float()
    H = torch.where(V == r, (g - b) * k, torch.where(V == g, (b - r) * k + 120.0, (r - g) * k + 240.0))
    H = torch.where(H < 0, H + 360.0, H)
    return torch.stack((H, S, V), -1).numpy()


def test_stages_against_opencv_mmcv_and_mmdet():
    from monorun_amd import image_pipeline as ip
    g = _load()
    worst = dict.fromkeys(MEASURED, 0.0)
    scale = dict.fromkeys(MEASURED, 0.0)

    def note(stage, got, want):
        assert got.shape == want.shape, stage
        worst[stage] = max(worst[stage], float(np.abs(got.astype(np.float64) - want).max()))
        scale[stage] = max(scale[stage], float(np.abs(want).max()))

    n_images = sum(k.startswith('imflip_') for k in g)
    for i in range(n_images):
        im = ref.image(12, 20, i)
        x = im.astype(np.float32)
        note('bgr2hsv', _hsv(x), g[f'bgr2hsv_{i}'])
        kw = dict(mean=(0, 0, 0), std=(1, 1, 1), to_rgb=False, device='cpu')
        back = ip.prepare_batch([im], photometric=[ip.PhotoParams()], **kw)[0][0, :, :12, :20].permute(1, 2, 0).numpy()
        note('hsv2bgr', back, g[f'hsv2bgr_{i}'])
        img, _, _ = ip.prepare_batch([im], ref.MEAN, ref.STD, True, 32, device='cpu')
        note('imnormalize', img[0, :, :12, :20].permute(1, 2, 0).numpy(), g[f'imnormalize_{i}'])
        pad = g[f'impad_{i}']
        assert pad.shape == (32, 32, 3) and float(np.abs(pad[12:]).sum()) == 0 and float(np.abs(pad[:, 20:]).sum()) == 0
        assert float(img[0, :, 12:].abs().sum()) == 0 and float(img[0, :, :, 20:].abs().sum()) == 0                       # exact: zeros where mmcv pads
        flipped = ip.prepare_batch([im], flips=[True], **kw)[0][0, :, :12, :20].permute(1, 2, 0).numpy()
        assert np.array_equal(flipped, g[f'imflip_{i}'].astype(np.float32))                                               # exact: an index operation
    for key in sorted(k for k in g if k.startswith('distort_')):
        seed = int(key.split('_')[1])
        _, p = ip.draw_augmentation(np.random.RandomState(seed))
        got = ip.prepare_batch([ref.image(12, 20, 0)], (0, 0, 0), (1, 1, 1), False, photometric=[p], device='cpu')[0][0, :, :12, :20].permute(1, 2, 0).numpy()
        note('distort', got, g[key])
    for stage in MEASURED:
        print(f'{stage}: largest absolute difference {worst[stage]:.3e} at magnitudes up to {scale[stage]:.3e}')
    for stage, measured in MEASURED.items():
        assert measured is not None, f'{stage}: the fixture exists now: record the printed measurement here and in DESIGN.md section 26'
        assert worst[stage] <= measured + float(np.spacing(np.float32(scale[stage]))), stage
