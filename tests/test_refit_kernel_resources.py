"""The re-fit's launches as the compiler reports them (-Rpass-analysis=kernel-resource-usage, as tools/kernel_resources.sh reads them):
since round 8 `epnp_refit_betas_kernel` also computes the three candidates' pose and yaw, and the LM launch that carries the re-fit
(`pnp_uncert_refit_kernel`) only their error passes.  The lane-mapped launch must keep two waves per SIMD and no scratch in every
mapping; the LM launch must keep the occupancy, scratch and (up to the 8-register allocation granule) the registers it had before
(profiles/r08_kernel_resources.txt).  Needs hipcc, no GPU."""
import re

import pytest

from tests.kernel_resources import have_hipcc, kernel_resources


# pnp_uncert_refit_kernel<T, WPO> before round 8: (VGPRs, waves per SIMD, scratch bytes per lane)
LM_BEFORE = {('f', 2): (144, 3, 0), ('f', 4): (128, 4, 28), ('f', 8): (128, 4, 20),
             ('6__half', 2): (149, 3, 0), ('6__half', 4): (127, 4, 20), ('6__half', 8): (128, 4, 20),
             ('d', 2): (145, 3, 0), ('d', 4): (139, 3, 0), ('d', 8): (143, 3, 0)}


def _alloc(v):
    return (v + 7) // 8 * 8


@pytest.mark.skipif(not have_hipcc(), reason='hipcc not installed')
def test_refit_launches_keep_their_occupancy_and_no_new_scratch():
    kernels = kernel_resources()
    betas = {k: v for k, v in kernels.items() if 'epnp_refit_betas_kernel' in k}
    assert len(betas) == 3, sorted(kernels)                                # LV = 0 | 2 | 4: quad, row, wave
    for name, r in betas.items():
        assert r['occ'] == 2 and r['scratch'] == 0 and r['spill'] == 0, (name, r)
    lm = {k: v for k, v in kernels.items() if 'pnp_uncert_refit_kernel' in k}
    assert len(lm) == len(LM_BEFORE), sorted(lm)
    for (t, wpo), (vgpr, occ, scratch) in LM_BEFORE.items():
        name = next(k for k in lm if re.search(rf'pnp_uncert_refit_kernelI{re.escape(t)}Li{wpo}E', k))
        r = lm[name]
        assert r['occ'] >= occ and r['scratch'] <= scratch and _alloc(r['vgpr']) <= _alloc(vgpr), (name, r)
