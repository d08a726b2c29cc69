"""The assignment's kernels as the compiler reports them (-Rpass-analysis=kernel-resource-usage, as
tools/kernel_resources.sh reads them): the two compile for gfx950, use no scratch and spill nothing; their LDS is what
include/monorun_assign.h states: the staged ground truths and ignore boxes and the block's gt_max keys for the first launch, the ground
truths and gt_max for the second.  Needs hipcc, no GPU."""
import os
import re

import pytest

from tests.kernel_resources import ROOT, have_hipcc, kernel_resources

KERNELS = {'assign_max_kernel': 'MR_ASSIGN_MAX_LDS_BYTES', 'assign_finish_kernel': 'MR_ASSIGN_FINISH_LDS_BYTES'}


def header_constants():
    """the integer #defines of monorun_assign.h, the LDS sizes evaluated from the others"""
    text = open(os.path.join(ROOT, 'include', 'monorun_assign.h')).read()
    vals = {}
    for name, expr in re.findall(r'^#define (MR_ASSIGN_\w+) (.+?)\s*(?:/\*.*)?$', text, flags=re.M):
        assert re.fullmatch(r'[\w\s()*+]+', expr), (name, expr)
        vals[name] = int(eval(expr, {'__builtins__': {}}, vals))
    return vals


def test_header_states_the_caps_and_the_lds():
    v = header_constants()
    assert v['MR_ASSIGN_MAX_GT'] == 256 and v['MR_ASSIGN_MAX_IGNORE'] == 256 and v['MR_ASSIGN_THREADS'] == 256 and v['MR_ASSIGN_MAX_IMAGES'] == 65535
    assert v['MR_ASSIGN_MAX_LDS_BYTES'] == 4096 + 4096 + 1024 and v['MR_ASSIGN_FINISH_LDS_BYTES'] == 4096 + 1024


@pytest.mark.skipif(not have_hipcc(), reason='hipcc not installed')
def test_assign_kernels_compile_without_scratch():
    kernels, consts = kernel_resources(), header_constants()
    for k, lds in KERNELS.items():
        found = {name: r for name, r in kernels.items() if re.search(r'\d' + k + 'E', name)}
        assert len(found) == 1, (k, sorted(found))
        (name, r), = found.items()
        assert r['scratch'] == 0 and r['spill'] == 0 and r['sgpr_spill'] == 0, (name, r)
        assert r['lds'] == consts[lds], (name, r)
        assert r['vgpr'] + r['agpr'] <= 64, (name, r)           # 256 threads, one box each: eight waves per SIMD
