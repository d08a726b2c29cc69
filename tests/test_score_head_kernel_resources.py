"""The score head's fused kernel as the compiler reports it (-Rpass-analysis=kernel-resource-usage, as
tools/kernel_resources.sh reads it): it compiles for gfx950, uses no scratch, spills no register and keeps its workgroup's LDS at or
under 80 KB, so that two workgroups fit a CU.  Needs hipcc, no GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
KERNEL = 'score_head_forward_kernel'


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which('hipcc')), reason='hipcc not installed')
def test_score_head_kernel_compiles_without_scratch_or_spills():
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
        for key, pat in (('vgpr', r' VGPRs: (\d+)'), ('spill', r'VGPRs Spill: (\d+)'), ('sgpr_spill', r'SGPRs Spill: (\d+)'),
                         ('scratch', r'ScratchSize \[bytes/lane\]: (\d+)'), ('lds', r'LDS Size \[bytes/block\]: (\d+)')):
            m = re.search(pat, line)
            if m and cur:
                kernels[cur][key] = int(m.group(1))
    found = {name: r for name, r in kernels.items() if re.search(r'\d' + KERNEL + 'E', name)}              # _ZN12_GLOBAL__N_1<len><name>E...
    assert len(found) == 1, sorted(found)
    (name, r), = found.items()
    assert r['scratch'] == 0 and r['spill'] == 0 and r['sgpr_spill'] == 0, (name, r)
    assert 0 < r['lds'] <= 80 * 1024, (name, r)                 # static: the launch adds no dynamic LDS
