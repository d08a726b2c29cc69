"""The feature pyramid's two kernels as the compiler reports them (-Rpass-analysis=kernel-resource-usage, as
tools/kernel_resources.sh reads them): both compile for gfx950, use no scratch and spill nothing; their LDS is what include/monorun_fpn.h
states: the forward's tile of m[0] with its halo, the backward's two footprint buffers and its tables.  Needs hipcc, no GPU."""
import os
import re

import pytest

from tests.kernel_resources import ROOT, have_hipcc, kernel_resources

KERNELS = {'fpn_topdown_forward_kernel': ('MR_FPN_FORWARD_LDS_BYTES', 8), 'fpn_topdown_backward_kernel': ('MR_FPN_BACKWARD_LDS_BYTES', 5)}


def header_constants():
    """the integer #defines of monorun_fpn.h, the two LDS sizes evaluated from the others"""
    text = open(os.path.join(ROOT, 'include', 'monorun_fpn.h')).read()
    vals = {}
    for name, expr in re.findall(r'^#define (MR_FPN_\w+) (.+?)\s*(?:/\*.*)?$', text, flags=re.M):
        assert re.fullmatch(r'[\w\s()*+]+', expr), (name, expr)
        vals[name] = int(eval(expr, {'__builtins__': {}}, vals))
    return vals


def footprint_bound(levels, root):
    """the largest extent per axis of a footprint on the levels below a block of `root` coarsest pixels: k parents have at most 2k + 1
    children under the pyramid rule"""
    out = [root]
    for _ in range(levels - 1):
        out.append(2 * out[-1] + 1)
    return out[::-1]            # finest first


def test_header_states_the_tiling_and_the_buffers_hold_every_footprint():
    v = header_constants()
    assert v['MR_FPN_FORWARD_LDS_BYTES'] == 4 * 18 * 66 == 4752
    assert v['MR_FPN_BACKWARD_LDS_BYTES'] == 4 * (6144 + 1536 + 24 + 33 + 49) == 31144
    assert v['MR_FPN_MAX_LEVELS'] >= 6 and v['MR_FPN_TILE_H'] * v['MR_FPN_TILE_W'] == v['MR_FPN_FLAT']
    for L in range(1, v['MR_FPN_MAX_LEVELS'] + 1):
        hs = footprint_bound(L, max(1, v['MR_FPN_TILE_H'] >> (L - 1)))
        ws = footprint_bound(L, max(1, v['MR_FPN_TILE_W'] >> (L - 1)))
        for l, (h, w) in enumerate(zip(hs, ws)):
            assert h * w <= (v['MR_FPN_BWD_ODD'] if l & 1 else v['MR_FPN_BWD_EVEN']), (L, l, h, w)
            assert l == 0 or (h <= v['MR_FPN_BWD_ROWS'] and w <= v['MR_FPN_BWD_COLS']), (L, l, h, w)


@pytest.mark.skipif(not have_hipcc(), reason='hipcc not installed')
def test_fpn_kernels_compile_without_scratch():
    kernels, consts = kernel_resources(), header_constants()
    for k, (lds, waves) in KERNELS.items():
        found = {name: r for name, r in kernels.items() if re.search(r'\d' + k + 'E', name)}
        assert len(found) == 1, (k, sorted(found))
        (name, r), = found.items()
        assert r['scratch'] == 0 and r['spill'] == 0 and r['sgpr_spill'] == 0, (name, r)
        assert r['lds'] == consts[lds], (name, r)
        assert r['occ'] >= waves, (name, r)        # the forward: every wave slot; the backward: 5 workgroups fit a CU's LDS, 20 waves per CU
