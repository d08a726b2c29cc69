"""The RoI extraction kernels as the compiler reports them (-Rpass-analysis=kernel-resource-usage, as
tools/kernel_resources.sh reads them): both compile for gfx950, use no scratch and spill nothing; their LDS is what include/monorun_roi.h
states: the forward's two per-axis tap tables, the backward's separable weights, staged grad_out block and RoI list.  Needs hipcc, no GPU."""
import os
import re

import pytest

from tests.kernel_resources import ROOT, have_hipcc, kernel_resources

KERNELS = {'roi_extract_forward_kernel': 'MR_ROI_FORWARD_LDS_BYTES', 'roi_extract_backward_kernel': 'MR_ROI_BACKWARD_LDS_BYTES'}


def header_constants():
    """the integer #defines of monorun_roi.h, the two LDS sizes evaluated from the others"""
    text = open(os.path.join(ROOT, 'include', 'monorun_roi.h')).read()
    vals = {}
    for name, expr in re.findall(r'^#define (MR_ROI_\w+) (.+?)\s*(?:/\*.*)?$', text, flags=re.M):
        assert re.fullmatch(r'[\w\s()*+]+', expr), (name, expr)
        vals[name] = int(eval(expr, {'__builtins__': {}}, vals))
    return vals


def test_header_states_the_tiling():
    v = header_constants()
    assert v['MR_ROI_FORWARD_LDS_BYTES'] == 2 * 256 * 16 == 8192
    assert v['MR_ROI_BACKWARD_LDS_BYTES'] == 4 * ((8 + 32) * 32 + 32 * 32 * 8 + 256 + 4) == 38928
    assert v['MR_ROI_TILE_H'] * v['MR_ROI_TILE_W'] == 256 and v['MR_ROI_MAX_LEVELS'] == 8 and v['MR_ROI_MAX_OUT'] == 32


@pytest.mark.skipif(not have_hipcc(), reason='hipcc not installed')
def test_roi_extract_kernels_compile_without_scratch():
    kernels, consts = kernel_resources(), header_constants()
    for k, lds in KERNELS.items():
        found = {name: r for name, r in kernels.items() if re.search(r'\d' + k + 'E', name)}
        assert len(found) == 1, (k, sorted(found))
        (name, r), = found.items()
        assert r['scratch'] == 0 and r['spill'] == 0 and r['sgpr_spill'] == 0, (name, r)
        assert r['lds'] == consts[lds], (name, r)
        assert r['occ'] >= 4, (name, r)            # 4 workgroups of the backward fit a CU's LDS: 16 waves per CU
