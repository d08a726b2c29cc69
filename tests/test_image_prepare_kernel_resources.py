"""The image preparation's kernel as the compiler reports it (-Rpass-analysis=kernel-resource-usage, as
tools/kernel_resources.sh reads it): it compiles for gfx950, uses no scratch and spills nothing, and its LDS is what
include/monorun_image.h states (none).  Needs hipcc, no GPU."""
import os
import re

import pytest

from tests.kernel_resources import ROOT, have_hipcc, kernel_resources

KERNEL, LDS = 'image_prepare_kernel', 'MR_IMAGE_PREPARE_LDS_BYTES'


def header_constants():
    text = open(os.path.join(ROOT, 'include', 'monorun_image.h')).read()
    return {k: int(v, 0) for k, v in re.findall(r'^#define (MR_IMAGE_\w+) (\w+)', text, flags=re.M)}


def test_header_states_the_launch():
    v = header_constants()
    assert v['MR_IMAGE_THREADS'] % 64 == 0 and v[LDS] == 0
    assert v['MR_IMAGE_MAX_IMAGES'] == 65535, 'the images are the second grid dimension'
    assert v['MR_IMAGE_MAX_PIXELS'] == 2 ** 31 - 1 and v['MR_IMAGE_TABLE_WORDS'] == 16
    words = [v[k] for k in ('MR_IMAGE_OFFSET_LO', 'MR_IMAGE_OFFSET_HI', 'MR_IMAGE_H', 'MR_IMAGE_W', 'MR_IMAGE_STRIDE', 'MR_IMAGE_FLIP', 'MR_IMAGE_SWITCHES',
                            'MR_IMAGE_PERMUTATION', 'MR_IMAGE_BRIGHTNESS_DELTA', 'MR_IMAGE_CONTRAST_ALPHA', 'MR_IMAGE_SATURATION_ALPHA', 'MR_IMAGE_HUE_DELTA')]
    assert words == list(range(12))
    bits = [v[k] for k in ('MR_IMAGE_SW_BRIGHTNESS', 'MR_IMAGE_SW_CONTRAST', 'MR_IMAGE_SW_CONTRAST_FIRST', 'MR_IMAGE_SW_SATURATION', 'MR_IMAGE_SW_HUE',
                           'MR_IMAGE_SW_HSV')]
    assert bits == [1, 2, 4, 8, 16, 32] and v['MR_IMAGE_SW_ALL'] == sum(bits)


@pytest.mark.skipif(not have_hipcc(), reason='hipcc not installed')
def test_image_prepare_kernel_compiles_without_scratch():
    kernels, consts = kernel_resources(), header_constants()
    found = {name: r for name, r in kernels.items() if re.search(r'\d' + KERNEL + 'E', name)}
    assert len(found) == 1, sorted(found)
    (name, r), = found.items()
    assert r['scratch'] == 0 and r['spill'] == 0 and r['sgpr_spill'] == 0, (name, r)
    assert r['lds'] == consts[LDS], (name, r)
    assert r['occ'] >= 8, (name, r)             # a streaming kernel: every wave slot
