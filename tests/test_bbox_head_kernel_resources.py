"""The detection head's two kernels as the compiler reports them (-Rpass-analysis=kernel-resource-usage, as
tools/kernel_resources.sh reads them): they compile for gfx950, use no scratch and spill nothing; their LDS is what include/monorun_bbox.h
states: one 64-bit key per row for the rank launch, the packed kept flags with a count per word for the select launch.  And the record
of tools/isa_diff.sh against the parent: every kernel the parent has is byte-identical.  Needs hipcc, no GPU."""
import os
import re

import pytest

from tests.kernel_resources import ROOT, have_hipcc, kernel_resources

KERNELS = {'bbox_head_rank_kernel': 'MR_BBOX_RANK_LDS_BYTES', 'bbox_head_select_kernel': 'MR_BBOX_SELECT_LDS_BYTES'}


def header_constants():
    """the integer #defines of monorun_bbox.h, the LDS sizes evaluated from the others"""
    text = open(os.path.join(ROOT, 'include', 'monorun_bbox.h')).read()
    vals = {}
    for name, expr in re.findall(r'^#define (MR_BBOX_\w+) (.+?)\s*(?:/\*.*)?$', text, flags=re.M):
        assert re.fullmatch(r'[\w\s()*+/]+', expr), (name, expr)
        vals[name] = int(eval(expr.replace('/', '//'), {'__builtins__': {}}, vals))
    return vals


def test_header_states_the_caps_and_the_lds():
    v = header_constants()
    assert v['MR_BBOX_MAX_ROIS'] == 4096 and v['MR_BBOX_MAX_CLASSES'] >= 8 and v['MR_BBOX_MAX_IMAGES'] * v['MR_BBOX_MAX_CLASSES'] <= 65535
    assert v['MR_BBOX_RANK_LDS_BYTES'] == 8 * 4096 == 32768
    assert v['MR_BBOX_SELECT_LDS_BYTES'] == v['MR_BBOX_MAX_CLASSES'] * 64 * (8 + 4)
    from monorun_amd import bbox_head
    assert (bbox_head.MAX_ROIS, bbox_head.MAX_CLASSES, bbox_head.MAX_IMAGES) == (v['MR_BBOX_MAX_ROIS'], v['MR_BBOX_MAX_CLASSES'], v['MR_BBOX_MAX_IMAGES'])


@pytest.mark.skipif(not have_hipcc(), reason='hipcc not installed')
def test_bbox_head_kernels_compile_without_scratch():
    kernels, consts = kernel_resources(), header_constants()
    for k, lds in KERNELS.items():
        found = {name: r for name, r in kernels.items() if re.search(r'\d' + k + 'E', name)}
        assert len(found) == 1, (k, sorted(found))
        (name, r), = found.items()
        assert r['scratch'] == 0 and r['spill'] == 0 and r['sgpr_spill'] == 0, (name, r)
        assert r['lds'] == consts[lds], (name, r)
        assert r['vgpr'] + r['agpr'] <= 128, (name, r)          # 1024 threads: four waves per SIMD


def test_isa_diff_record_shows_only_new_kernels():
    """profiles/bbox_head_isa_diff.txt, the output of tools/isa_diff.sh against the parent: nothing differs, nothing is gone, and the
    kernels that exist only now are this stage's two"""
    text = open(os.path.join(ROOT, 'profiles', 'bbox_head_isa_diff.txt')).read()
    m = re.search(r'(\d+) kernels at \S+, (\d+) now: (\d+) identical, (\d+) differing', text)
    old, new, same, differ = (int(x) for x in m.groups())
    assert differ == 0 and same == old and new == old + 2 and 'only at' not in text
    only_now = re.findall(r'only now: (\S+)', text)
    assert len(only_now) == 2 and all(any(k in n for k in KERNELS) for n in only_now)
