"""The one-launch result tail's kernel as the compiler reports it (-Rpass-analysis=kernel-resource-usage, as
tools/kernel_resources.sh reads it): it compiles for gfx950, uses no scratch and spills nothing; all its LDS is dynamic (no static
share in front of the 16-byte-aligned carve), sized by the formula of include/monorun_result3d.h, which the entry point's static_asserts
tie to the kernel's carve; the header's caps are the Python constants; LATER_HEADERS names the entry point; and the committed ISA
comparison with the parent says what the issue expects of it.  Needs hipcc, no GPU."""
import os
import re

import pytest

from tests.kernel_resources import ROOT, have_hipcc, kernel_resources

HEADER = os.path.join(ROOT, 'include', 'monorun_result3d.h')


def header_constants():
    """the integer #defines of monorun_result3d.h and its LDS formula as a function of (n, np2)"""
    text = open(HEADER).read()
    vals = {}
    for name, expr in re.findall(r'^#define (MR_RESULT3D_\w+) ([\w\s()*+]+?)\s*(?:/\*.*)?$', text, flags=re.M):
        if name != 'MR_RESULT3D_MAX_LDS_BYTES':
            vals[name] = int(eval(expr, {'__builtins__': {}}, vals))
    m = re.search(r'^#define MR_RESULT3D_LDS_BYTES\(n, np2\) (.+)$', text, flags=re.M)
    assert m and re.fullmatch(r'[\w\s()*+/]+', m.group(1)), m
    formula = m.group(1).replace('/', '//')

    def lds(n, np2):
        return int(eval(formula, {'__builtins__': {}}, dict(vals, n=n, np2=np2)))
    m = re.search(r'^#define MR_RESULT3D_MAX_LDS_BYTES MR_RESULT3D_LDS_BYTES\((\w+), (\d+)\)$', text, flags=re.M)
    assert m, 'MR_RESULT3D_MAX_LDS_BYTES is the formula at the caps'
    vals['MR_RESULT3D_MAX_LDS_BYTES'] = lds(vals[m.group(1)], int(m.group(2)))
    return vals, lds


def test_header_states_the_caps_and_the_lds():
    from monorun_amd import consumers
    v, lds = header_constants()
    assert v['MR_RESULT3D_MAX_N'] == consumers.RESULT3D_MAX_N == 512 and v['MR_RESULT3D_MAX_CLASSES'] == consumers.RESULT3D_MAX_CLASSES == 16
    assert v['MR_RESULT3D_THREADS'] == 256 and v['MR_RESULT3D_BOX_BYTES'] == 44
    # keys and indices of the padded sort, boxes, 16 words of suppression bits per box, the counters, the members' rows
    assert v['MR_RESULT3D_MAX_LDS_BYTES'] == 512 * 8 + 512 * 44 + 512 * 16 * 4 + 16 + 512 * 4 == 61456 <= 64 * 1024
    assert lds(0, 1) == 24 and lds(1, 1) == 8 + 44 + 4 + 16 + 4 and lds(33, 64) == 512 + 33 * 44 + 33 * 2 * 4 + 16 + 33 * 4
    np2 = lambda n: 1 if n <= 1 else 1 << (n - 1).bit_length()  # noqa: E731
    assert np2(33) == 64 and np2(512) == 512 and all(lds(n + 1, np2(n + 1)) > lds(n, np2(n)) for n in range(512))    # a class's share fits the launch's
    abi = open(os.path.join(ROOT, 'monorun_amd', 'csrc', 'result3d_abi.inc')).read()
    for name in ('MR_RESULT3D_MAX_N', 'MR_RESULT3D_MAX_CLASSES', 'MR_RESULT3D_THREADS', 'MR_RESULT3D_BOX_BYTES', 'MR_RESULT3D_MAX_LDS_BYTES',
                 'MR_RESULT3D_LDS_BYTES('):
        assert re.search(r'static_assert\([^;]*' + re.escape(name), abi), name


def test_later_headers_names_the_entry_point():
    from monorun_amd import _lib
    assert _lib.LATER_HEADERS['result3d'] == ('monorun_result3d.h', ('mr_result3d_nms',))
    assert _lib.exported_symbols('result3d') == ('mr_result3d_nms',) and _lib.header_path('result3d') == HEADER
    protos = _lib.header_prototypes(HEADER)
    assert [p[0] for p in protos] == ['mr_result3d_nms'] and protos[0][1] == 'int'
    assert _lib.arg_names('mr_result3d_nms') == ('dimensions', 'yaw', 't_vec', 'scores', 'labels', 'det_bboxes', 'n', 'num_classes', 'thr', 'out3d', 'out2d',
                                                 'keep_local', 'keep_row', 'num_keep', 'num_in_class')
    assert 'result3d' not in _lib.HEADERS and 'result3d' not in _lib.EXTRA_HEADERS        # the two pinned tables stay as they were


@pytest.mark.skipif(not have_hipcc(), reason='hipcc not installed')
def test_result3d_kernel_compiles_without_scratch():
    kernels = kernel_resources()
    found = {name: r for name, r in kernels.items() if re.search(r'\d' + 'result3d_nms_kernel' + 'E', name)}
    assert len(found) == 1, sorted(found)
    (name, r), = found.items()
    assert r['scratch'] == 0 and r['spill'] == 0 and r['sgpr_spill'] == 0, (name, r)
    assert r['lds'] == 0, (name, r)                              # no static LDS: the dynamic carve starts at a 16-byte-aligned base
    assert r['vgpr'] + r['agpr'] <= 256, (name, r)               # a 256-thread block is one wave per SIMD; at most 16 blocks, one per class, run
    old = {n: q for n, q in kernels.items() if re.search(r'\d' + 'nms_bev_kernel' + 'E', n)}
    assert len(old) == 1
    (_, q), = old.items()
    assert q['scratch'] == 0 and q['spill'] == 0 and q['sgpr_spill'] == 0 and q['lds'] == 0, q


def test_isa_diff_record():
    """profiles/result3d_isa_diff.txt: tools/isa_diff.sh against the parent.  Exactly one kernel is new; a parent kernel that differs
    can only be nms_bev_kernel (it now calls the shared routine), and then the record and DESIGN.md §24 say so."""
    text = open(os.path.join(ROOT, 'profiles', 'result3d_isa_diff.txt')).read()
    m = re.search(r'(\d+) kernels at \w+, (\d+) now: (\d+) identical, (\d+) differing', text)
    assert m, text
    old, new, same, differ = map(int, m.groups())
    assert new == old + 1 and same + differ == old
    only_now = re.findall(r'only now: (\S+)', text)
    assert len(only_now) == 1 and 'result3d_nms_kernel' in only_now[0] and not re.search(r'only at ', text)
    differs = re.findall(r'differs: (\S+)', text)
    assert len(differs) == differ <= 1
    if differ:
        assert 'nms_bev_kernel' in differs[0]
        design = open(os.path.join(ROOT, 'DESIGN.md')).read()
        sec = design[design.index('## 24'):]
        assert 'nms_bev_kernel' in sec and 'result3d_isa_diff.txt' in sec
