#!/usr/bin/env python3
"""G24: the image preparation's third-party pins — what OpenCV, mmcv and mmdet compute on the test images.

    python tests/golden/make_golden_image_prepare.py        # writes tests/golden/g24_image_prepare_thirdparty.npz

Runs only where ``cv2``, ``mmcv`` and ``mmdet`` (2.x) import; none of them exists where this project is developed, so the fixture is absent
until somebody records it, and tests/test_image_prepare_thirdparty_golden.py skips by name while it is.  Nothing is restated here: every
array is the return value of the third-party function named by its key, called on the seeded images of tests/image_prepare_ref.py.

  bgr2hsv_<i>, hsv2bgr_<i>     mmcv.bgr2hsv of image i as float32; mmcv.hsv2bgr of THAT result
  imnormalize_<i>              mmcv.imnormalize(float32 image, mean, std, to_rgb=True)
  imflip_<i>                   mmcv.imflip(image, 'horizontal')
  impad_<i>                    mmcv.impad_to_multiple(normalised image, 32, pad_val=0)
  distort_<s>                  mmdet's PhotoMetricDistortion()(dict(img=float32 image 0)) after ``np.random.seed(s); np.random.rand()`` (the
                               one draw RandomFlip 2.3 makes first), so that ``draw_augmentation(RandomState(s))`` holds the same parameters
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
NAME = 'g24_image_prepare_thirdparty.npz'
N_IMAGES, SEEDS = 4, tuple(range(8))


def main():
    import cv2  # noqa: F401  (mmcv's colour conversions are OpenCV's)
    import mmcv
    from mmdet.datasets.pipelines import PhotoMetricDistortion
    from tests import image_prepare_ref as ref
    out = dict(versions=np.array([cv2.__version__, mmcv.__version__, __import__('mmdet').__version__]))
    mean, std = np.array(ref.MEAN, np.float32), np.array(ref.STD, np.float32)
    for i in range(N_IMAGES):
        im = ref.image(12, 20, i)
        x = im.astype(np.float32)
        out[f'bgr2hsv_{i}'] = mmcv.bgr2hsv(x)
        out[f'hsv2bgr_{i}'] = mmcv.hsv2bgr(out[f'bgr2hsv_{i}'])
        out[f'imnormalize_{i}'] = mmcv.imnormalize(x.copy(), mean, std, True)
        out[f'imflip_{i}'] = mmcv.imflip(im, 'horizontal')
        out[f'impad_{i}'] = mmcv.impad_to_multiple(out[f'imnormalize_{i}'], 32, pad_val=0)
    for s in SEEDS:
        np.random.seed(s)
        np.random.rand()
        out[f'distort_{s}'] = PhotoMetricDistortion()(dict(img=ref.image(12, 20, 0).astype(np.float32)))['img']
    np.savez_compressed(os.path.join(HERE, NAME), **out)
    print('wrote', NAME, os.path.getsize(os.path.join(HERE, NAME)), 'bytes')


if __name__ == '__main__':
    main()
