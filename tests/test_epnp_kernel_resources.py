"""The consensus launch's resources as the compiler reports them (-Rpass-analysis=kernel-resource-usage, as tools/kernel_resources.sh
reads them): the occupancy it is compiled for (MR_EP_CONS_WAVES waves per SIMD) and its scratch — none at 4 waves, at most the 7
spilled registers (32 B per lane) of wave 0's control-point block at 5 —, so that a change that makes it spill more or lose a wave
does not go unnoticed.  Needs hipcc, no GPU."""
import os
import re

import pytest

from tests.kernel_resources import have_hipcc, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cons_waves():
    src = open(os.path.join(ROOT, 'monorun_amd', 'csrc', 'epnp_stages.inc')).read()
    return int(re.search(r'#define MR_EP_CONS_WAVES (\d+)', src).group(1))


@pytest.mark.skipif(not have_hipcc(), reason='hipcc not installed')
def test_consensus_kernels_no_scratch_at_their_occupancy():
    kernels = kernel_resources()
    cons = {k: v for k, v in kernels.items() if 'epnp_consensus_kernel' in k and 'Li4E' in k}
    assert len(cons) == 3, sorted(kernels)                                 # fp32, fp16, fp64 storage
    waves = _cons_waves()
    for name, r in cons.items():
        assert (r['scratch'], r['spill']) == (0, 0) if waves <= 4 else (r['scratch'] <= 32 and r['spill'] <= 7), (name, r)
        assert r['occ'] == waves, (name, r)
