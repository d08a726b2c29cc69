"""The proposal stage's kernels as the compiler reports them (-Rpass-analysis=kernel-resource-usage, as
tools/kernel_resources.sh reads them): the three compile for gfx950, use no scratch and spill nothing; their LDS is what
include/monorun_proposals.h states: the mask kernel's 64 column boxes, none for the decode and the scan.  Needs hipcc, no GPU."""
import os
import re

import pytest

from tests.kernel_resources import ROOT, have_hipcc, kernel_resources

KERNELS = {'proposal_decode_kernel': 'MR_PROPOSAL_DECODE_LDS_BYTES', 'nms_mask_kernel': 'MR_NMS_MASK_LDS_BYTES',
           'nms_scan_kernel': 'MR_NMS_SCAN_LDS_BYTES'}


def header_constants():
    """the integer #defines of monorun_proposals.h, the LDS sizes evaluated from the others"""
    text = open(os.path.join(ROOT, 'include', 'monorun_proposals.h')).read()
    vals = {}
    for name, expr in re.findall(r'^#define (MR_(?:NMS|PROPOSAL)_\w+) (.+?)\s*(?:/\*.*)?$', text, flags=re.M):
        assert re.fullmatch(r'[\w\s()*+]+', expr), (name, expr)
        vals[name] = int(eval(expr, {'__builtins__': {}}, vals))
    return vals


def test_header_states_the_caps_and_the_tiling():
    v = header_constants()
    assert v['MR_NMS_MAX_GROUP'] == 64 * 64 == 4096 and v['MR_NMS_TILE'] == 64 and 2 * v['MR_NMS_SCAN_ROWS'] == v['MR_NMS_TILE']
    assert v['MR_NMS_MASK_LDS_BYTES'] == 64 * 16 == 1024 and v['MR_NMS_SCAN_LDS_BYTES'] == 0 and v['MR_PROPOSAL_DECODE_LDS_BYTES'] == 0
    assert v['MR_PROPOSAL_MAX_LEVELS'] == 8 and v['MR_PROPOSAL_MAX_ANCHORS'] == 16 and v['MR_NMS_MAX_GROUPS'] == 65535


@pytest.mark.skipif(not have_hipcc(), reason='hipcc not installed')
def test_proposal_kernels_compile_without_scratch():
    kernels, consts = kernel_resources(), header_constants()
    for k, lds in KERNELS.items():
        found = {name: r for name, r in kernels.items() if re.search(r'\d' + k + 'E', name)}
        assert len(found) == 1, (k, sorted(found))
        (name, r), = found.items()
        assert r['scratch'] == 0 and r['spill'] == 0 and r['sgpr_spill'] == 0, (name, r)
        assert r['lds'] == consts[lds], (name, r)
    scan, = (r for name, r in kernels.items() if 'nms_scan_kernel' in name)
    assert scan['vgpr'] + scan['agpr'] <= 256, scan            # two buffers of 32 rows (128 VGPRs) and the rest: at least two waves per SIMD
