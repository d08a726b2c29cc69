"""The training decode's kernels as the compiler reports them (-Rpass-analysis=kernel-resource-usage, as
tools/kernel_resources.sh reads them): both compile for gfx950, use no scratch and spill nothing; the forward has no LDS, the backward
the 4 waves x 6 doubles of its reduction.  Needs hipcc, no GPU."""
import re

import pytest

from tests.kernel_resources import have_hipcc, kernel_resources

KERNELS = {'noc_decode_train_kernel': 0, 'noc_decode_train_backward_kernel': 4 * 6 * 8}


@pytest.mark.skipif(not have_hipcc(), reason='hipcc not installed')
def test_training_decode_kernels_compile_without_scratch():
    kernels = kernel_resources()
    for k, lds in KERNELS.items():
        found = {name: r for name, r in kernels.items() if re.search(r'\d' + k + 'E', name)}          # _ZN12_GLOBAL__N_1<len><name>E...
        assert len(found) == 1, (k, sorted(found))
        (name, r), = found.items()
        assert r['scratch'] == 0 and r['spill'] == 0 and r['sgpr_spill'] == 0, (name, r)
        assert r['lds'] == lds, (name, r)
