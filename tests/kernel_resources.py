"""Every kernel's resources as the compiler reports them (-Rpass-analysis=kernel-resource-usage): one device-only compile of the
library per process, shared by the resource tests (test_*_kernel_resources.py) and by tools/kernel_resources.sh, which prints the
table below.  Needs hipcc, no GPU."""
import functools
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
FIELDS = (('vgpr', r' VGPRs: (\d+)'), ('agpr', r'AGPRs: (\d+)'), ('sgpr', r' SGPRs: (\d+)'), ('sgpr_spill', r'SGPRs Spill: (\d+)'),
          ('spill', r'VGPRs Spill: (\d+)'), ('scratch', r'ScratchSize \[bytes/lane\]: (\d+)'), ('occ', r'Occupancy \[waves/SIMD\]: (\d+)'),
          ('lds', r'LDS Size \[bytes/block\]: (\d+)'))


def have_hipcc():
    return bool(os.path.exists(HIPCC) or shutil.which('hipcc'))


def parse(remarks):
    """{mangled kernel name: {field: value}} from the compiler's remarks, in the order of the file"""
    kernels, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            cur = m.group(1)
            kernels[cur] = {}
            continue
        for key, pat in FIELDS:
            m = re.search(pat, line)
            if m and cur:
                kernels[cur][key] = int(m.group(1))
    return kernels


@functools.lru_cache(maxsize=None)
def kernel_resources(extra_flags=()):
    """the library's kernels (compiled once per process and set of flags): {mangled name: {vgpr, agpr, sgpr, sgpr_spill, spill, scratch, occ, lds}}"""
    cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-I', os.path.join(ROOT, 'include'), '--cuda-device-only', '-c', *extra_flags,
           '-Rpass-analysis=kernel-resource-usage', os.path.join(ROOT, 'monorun_amd', 'csrc', 'monorun_pnp.hip'), '-o', os.devnull]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
    assert out.returncode == 0, out.stderr[-2000:]
    return parse(out.stderr)


if __name__ == '__main__':          # tools/kernel_resources.sh: [name-filter-regex] [extra hipcc flags...]
    name_filter = sys.argv[1] if len(sys.argv) > 1 else '.'
    for name, r in kernel_resources(tuple(sys.argv[2:])).items():
        if 'lds' in r and re.search(name_filter, name):
            print(f"{name:<75} VGPRs {r.get('vgpr', 0):3d} AGPRs {r.get('agpr', 0):3d} SGPRs {r.get('sgpr', 0):3d} sgpr-spill {r.get('sgpr_spill', 0):3d} "
                  f"vgpr-spill {r.get('spill', 0):3d} scratch {r.get('scratch', 0):4d} waves/SIMD {r.get('occ', 0)}")
