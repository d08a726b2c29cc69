"""The NOC head's training kernels as the compiler reports them (-Rpass-analysis=kernel-resource-usage, as
tools/kernel_resources.sh reads them): all five compile for gfx950 and use no scratch.  Needs hipcc, no GPU."""
import re

import pytest

from tests.kernel_resources import have_hipcc, kernel_resources

KERNELS = ('uncert_projection_kernel', 'uncert_projection_backward_kernel', 'robust_kl_partial_kernel', 'robust_kl_fold_kernel',
           'robust_kl_backward_kernel')


@pytest.mark.skipif(not have_hipcc(), reason='hipcc not installed')
def test_projection_loss_kernels_compile_without_scratch():
    kernels = kernel_resources()
    for k in KERNELS:
        found = {name: r for name, r in kernels.items() if re.search(r'\d' + k + 'E', name)}          # _ZN12_GLOBAL__N_1<len><name>E...
        assert len(found) == 1, (k, sorted(found))
        (name, r), = found.items()
        assert r['scratch'] == 0 and r['spill'] == 0, (name, r)
        assert r['lds'] <= 64, (name, r)                  # the reductions' 4 x 2 doubles, nothing else
