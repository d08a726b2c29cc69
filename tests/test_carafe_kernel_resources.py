"""The CARAFE kernels as the compiler reports them (-Rpass-analysis=kernel-resource-usage, as tools/kernel_resources.sh
reads them): every instantiation (up_kernel 1, 3, 5, 7 of the forward and the two backward kernels) compiles for gfx950, uses no scratch
and spills nothing; its LDS is the one staged image of the tiling: 32 channels x (16 + k - 1)^2 source pixels (the tile with its halo) in
fp32.  Needs hipcc, no GPU."""
import re

import pytest

from tests.kernel_resources import have_hipcc, kernel_resources

KERNELS = ('carafe_pack_forward_kernel', 'carafe_pack_backward_mask_kernel', 'carafe_pack_backward_input_kernel')
CHUNK, TILE = 32, 16


@pytest.mark.skipif(not have_hipcc(), reason='hipcc not installed')
def test_carafe_kernels_compile_without_scratch():
    kernels = kernel_resources()
    for k in KERNELS:
        for up_kernel in (1, 3, 5, 7):
            found = {name: r for name, r in kernels.items() if re.search(r'\d' + k + f'ILi{up_kernel}EEE', name)}   # _ZN12_GLOBAL__N_1<len><name>ILi<k>EEE...
            assert len(found) == 1, (k, up_kernel, sorted(found))
            (name, r), = found.items()
            assert r['scratch'] == 0 and r['spill'] == 0 and r['sgpr_spill'] == 0, (name, r)
            assert r['lds'] == CHUNK * (TILE + up_kernel - 1) ** 2 * 4, (name, r)
            assert r['occ'] >= (2 if up_kernel == 7 else 3), (name, r)          # what the LDS image allows: 61952 B at k = 7, 51200 B at k = 5
