"""The global head's kernels as the compiler reports them (-Rpass-analysis=kernel-resource-usage, as
tools/kernel_resources.sh reads them): all five compile for gfx950, use no scratch and spill nothing, with the LDS §16 states.
Needs hipcc, no GPU."""
import re

import pytest

from monorun_amd import _lib
from tests.kernel_resources import have_hipcc, kernel_resources

# kernel -> LDS bytes per workgroup: the A and the B tile of the MFMA tile routine, 64 rows x (32 + 1) floats each; the output layer
# reduces inside a wave and the statistics kernel in a thread
TILE_LDS = 2 * 64 * 33 * 4
KERNELS = {'gh_p_kernel': TILE_LDS, 'gh_h1_kernel': TILE_LDS, 'gh_h2_kernel': TILE_LDS, 'gh_out_kernel': 0, 'gh_stats_kernel': 0}


@pytest.mark.skipif(not have_hipcc(), reason='hipcc not installed')
def test_global_head_kernels_compile_without_scratch_or_spills():
    assert len(_lib.exported_symbols('global')) == 2 and TILE_LDS == 16896
    kernels = kernel_resources()
    for k, lds in KERNELS.items():
        found = {name: r for name, r in kernels.items() if re.search(r'\d' + k + 'E', name)}          # _ZN12_GLOBAL__N_1<len><name>E...
        assert len(found) == 1, (k, sorted(found))
        (name, r), = found.items()
        assert r['scratch'] == 0 and r['spill'] == 0 and r['sgpr_spill'] == 0, (name, r)
        assert r['lds'] == lds, (name, r)
        assert r['vgpr'] + r.get('agpr', 0) <= 128, (name, r)          # at least four waves per SIMD
