"""The consensus launch's resources as the compiler reports them (-Rpass-analysis=kernel-resource-usage, as tools/kernel_resources.sh
reads them): the occupancy it is compiled for (MR_EP_CONS_WAVES waves per SIMD) and its scratch — none at 4 waves, at most the 7
spilled registers (32 B per lane) of wave 0's control-point block at 5 —, so that a change that makes it spill more or lose a wave
does not go unnoticed.  Needs hipcc, no GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


def _cons_waves():
    src = open(os.path.join(ROOT, 'monorun_amd', 'csrc', 'epnp_stages.inc')).read()
    return int(re.search(r'#define MR_EP_CONS_WAVES (\d+)', src).group(1))


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which('hipcc')), reason='hipcc not installed')
def test_consensus_kernels_no_scratch_at_their_occupancy():
    cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-I', os.path.join(ROOT, 'include'), '--cuda-device-only', '-c',
           '-Rpass-analysis=kernel-resource-usage', os.path.join(ROOT, 'monorun_amd', 'csrc', 'monorun_pnp.hip'), '-o', os.devnull]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            cur = m.group(1)
            kernels[cur] = {}
            continue
        for key, pat in (('vgpr', r' VGPRs: (\d+)'), ('spill', r'VGPRs Spill: (\d+)'), ('scratch', r'ScratchSize \[bytes/lane\]: (\d+)'),
                         ('occ', r'Occupancy \[waves/SIMD\]: (\d+)')):
            m = re.search(pat, line)
            if m and cur:
                kernels[cur][key] = int(m.group(1))
    cons = {k: v for k, v in kernels.items() if 'epnp_consensus_kernel' in k and 'Li4E' in k}
    assert len(cons) == 3, sorted(kernels)                                 # fp32, fp16, fp64 storage
    waves = _cons_waves()
    for name, r in cons.items():
        assert (r['scratch'], r['spill']) == (0, 0) if waves <= 4 else (r['scratch'] <= 32 and r['spill'] <= 7), (name, r)
        assert r['occ'] == waves, (name, r)
