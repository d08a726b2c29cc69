"""The NOC target and loss_noc kernels as the compiler reports them (-Rpass-analysis=kernel-resource-usage, as
tools/kernel_resources.sh reads them): all five compile for gfx950, use no scratch and spill nothing, with the LDS §15 states.
Needs hipcc, no GPU."""
import re

import pytest

from tests.kernel_resources import have_hipcc, kernel_resources

# kernel -> LDS bytes per workgroup: the four waves' partial counts (4 ints) or partial sums (4 doubles); the backward reduces nothing
KERNELS = {'noc_dense_target_kernel': 16, 'noc_target_normalise_kernel': 16, 'smooth_l1_mod_loss_kernel': 32,
           'smooth_l1_mod_finish_kernel': 32, 'smooth_l1_mod_loss_backward_kernel': 0}


@pytest.mark.skipif(not have_hipcc(), reason='hipcc not installed')
def test_noc_target_kernels_compile_without_scratch_or_spills():
    kernels = kernel_resources()
    for k, lds in KERNELS.items():
        found = {name: r for name, r in kernels.items() if re.search(r'\d' + k + 'E', name)}          # _ZN12_GLOBAL__N_1<len><name>E...
        assert len(found) == 1, (k, sorted(found))
        (name, r), = found.items()
        assert r['scratch'] == 0 and r['spill'] == 0 and r['sgpr_spill'] == 0, (name, r)
        assert r['lds'] == lds, (name, r)
        assert r['vgpr'] <= 128, (name, r)                 # at least four waves per SIMD
