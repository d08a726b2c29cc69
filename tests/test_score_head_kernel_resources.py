"""The score head's fused kernel as the compiler reports it (-Rpass-analysis=kernel-resource-usage, as
tools/kernel_resources.sh reads it): it compiles for gfx950, uses no scratch, spills no register and keeps its workgroup's LDS at or
under 80 KB, so that two workgroups fit a CU.  Needs hipcc, no GPU."""
import re

import pytest

from tests.kernel_resources import have_hipcc, kernel_resources

KERNEL = 'score_head_forward_kernel'


@pytest.mark.skipif(not have_hipcc(), reason='hipcc not installed')
def test_score_head_kernel_compiles_without_scratch_or_spills():
    kernels = kernel_resources()
    found = {name: r for name, r in kernels.items() if re.search(r'\d' + KERNEL + 'E', name)}              # _ZN12_GLOBAL__N_1<len><name>E...
    assert len(found) == 1, sorted(found)
    (name, r), = found.items()
    assert r['scratch'] == 0 and r['spill'] == 0 and r['sgpr_spill'] == 0, (name, r)
    assert 0 < r['lds'] <= 80 * 1024, (name, r)                 # static: the launch adds no dynamic LDS
