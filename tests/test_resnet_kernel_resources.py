"""The backbone's kernels as the compiler reports them (-Rpass-analysis=kernel-resource-usage, as
tools/kernel_resources.sh reads them): every instantiation compiles for gfx950, uses no scratch and spills nothing; their LDS is what
include/monorun_backbone.h states; every one reaches the occupancy §23 states: 8 waves per SIMD, and 5 for the backward stream with the ReLU and the parameter
gradients, which keeps twelve 16-byte loads per lane in flight.  Needs hipcc, no GPU."""
import os
import re

import pytest

from tests.kernel_resources import ROOT, have_hipcc, kernel_resources

# kernel -> (instantiations, the header's LDS #define per instantiation by its mangled template arguments, waves per SIMD)
KERNELS = {
    'bn_act_forward_kernel': (4, lambda name: 'MR_BN_FORWARD_LDS_BYTES', 8),
    # <RELU, PARAMS>: the pair of sums per wave exists only with the parameter gradients
    'bn_act_backward_kernel': (4, lambda name: 'MR_BN_BACKWARD_LDS_BYTES' if re.search(r'ILb[01]ELb1EE', name) else 'MR_BN_FORWARD_LDS_BYTES',
                               lambda name: 5 if 'ILb1ELb1EE' in name else 8),
    'bn_act_backward_final_kernel': (1, lambda name: 'MR_BN_FINAL_LDS_BYTES', 8),
    'bn_relu_maxpool_forward_kernel': (1, lambda name: 'MR_STEM_LDS_BYTES', 8),
}


def header_constants():
    """the integer #defines of monorun_backbone.h, the LDS sizes evaluated from the others"""
    text = open(os.path.join(ROOT, 'include', 'monorun_backbone.h')).read()
    vals = {}
    for name, expr in re.findall(r'^#define (MR_(?:BN|STEM)_\w+) (.+?)\s*(?:/\*.*)?$', text, flags=re.M):
        assert re.fullmatch(r'[\w\s()*+]+', expr), (name, expr)
        vals[name] = int(eval(expr, {'__builtins__': {}}, vals))
    return vals


def test_header_states_the_tiling():
    v = header_constants()
    assert v['MR_BN_THREADS'] == 64 * v['MR_BN_WAVES'] and v['MR_BN_CHUNK'] % (4 * v['MR_BN_THREADS']) == 0
    assert v['MR_BN_BACKWARD_LDS_BYTES'] == 32 and v['MR_BN_FORWARD_LDS_BYTES'] == 0 and v['MR_BN_FINAL_LDS_BYTES'] == 0
    assert v['MR_STEM_LDS_BYTES'] == 4 * 17 * 129 == 8772
    assert v['MR_STEM_TILE_H'] * v['MR_STEM_TILE_W'] % v['MR_STEM_THREADS'] == 0 and v['MR_BN_MAX_GRID'] == 2048


@pytest.mark.skipif(not have_hipcc(), reason='hipcc not installed')
def test_backbone_kernels_compile_without_scratch():
    kernels, consts = kernel_resources(), header_constants()
    for k, (count, lds, waves) in KERNELS.items():
        found = {name: r for name, r in kernels.items() if re.search(r'\d' + k + '(E|I)', name)}
        assert len(found) == count, (k, sorted(found))
        for name, r in found.items():
            assert r['scratch'] == 0 and r['spill'] == 0 and r['sgpr_spill'] == 0, (name, r)
            assert r['lds'] == consts[lds(name)], (name, r)
            assert r['occ'] >= (waves(name) if callable(waves) else waves), (name, r)
