"""The NOC head's training kernels as the compiler reports them (-Rpass-analysis=kernel-resource-usage, as
tools/kernel_resources.sh reads them): all five compile for gfx950 and use no scratch.  Needs hipcc, no GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
KERNELS = ('uncert_projection_kernel', 'uncert_projection_backward_kernel', 'robust_kl_partial_kernel', 'robust_kl_fold_kernel',
           'robust_kl_backward_kernel')


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which('hipcc')), reason='hipcc not installed')
def test_projection_loss_kernels_compile_without_scratch():
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
                         ('lds', r'LDS Size \[bytes/block\]: (\d+)')):
            m = re.search(pat, line)
            if m and cur:
                kernels[cur][key] = int(m.group(1))
    for k in KERNELS:
        found = {name: r for name, r in kernels.items() if re.search(r'\d' + k + 'E', name)}          # _ZN12_GLOBAL__N_1<len><name>E...
        assert len(found) == 1, (k, sorted(found))
        (name, r), = found.items()
        assert r['scratch'] == 0 and r['spill'] == 0, (name, r)
        assert r['lds'] <= 64, (name, r)                  # the reductions' 4 x 2 doubles, nothing else
