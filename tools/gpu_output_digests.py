"""sha256 of every output of the reference flow (pose, cov, tr, valid, mask, diag, init_pose, init_mask, init_valid, init_diag) for one build of the library
(MR_PNP_SO selects it, as for tools/gpu_wide_ab.py): one call at a time at B = 100 and B = 1024, at fp32, fp16 and fp64 storage, the LM launch carrying the
re-fit (fused) and behind the complete initialiser; and one launch set of five 1024-object calls.  Run it once per build and diff the outputs: equal lines
mean bit-identical results.  Development aid (profiles/r15_digests.txt)."""
import hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from monorun_amd import synthetic as syn, PnPEpnpLaunch, PnPEpnpGroupLaunch
dev = torch.device('cuda:0')
NAMES = ('valid', 'pose', 'cov', 'tr', 'mask', 'diag', 'init_pose', 'init_mask', 'init_valid', 'init_diag')
DT = {'fp32': torch.float32, 'fp16': torch.float16, 'fp64': torch.float64}


def launch(B, seed, dtype, fused=True):
    b = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in syn.pnp_boundary(syn.make_batch(B=B, seed=seed), planar=True)]
    x = [t.to(DT[dtype]) for t in b[:3]]
    return PnPEpnpLaunch(*x, *b[3:6], z_min=0.5, epnp_istd_thres=0.6, epnp_ransac_thres=b[6], inlier_opt_only=True, with_diag=True, fused=fused)


def digests(label, l):
    torch.cuda.synchronize()
    for name in NAMES:
        t = getattr(l, name).contiguous().cpu().numpy()
        print(f'{label:<40} {name:<10} {hashlib.sha256(t.tobytes()).hexdigest()}')


for B in (100, 1024):
    for dtype in ('fp32', 'fp16', 'fp64'):
        for fused in (True, False):
            l = launch(B, 1234, dtype, fused)
            l.run()
            digests(f'B={B} {dtype} {"fused" if fused else "two entry points"}', l)
five = [launch(1024, 1234 + 7919 * i, 'fp32') for i in range(5)]
PnPEpnpGroupLaunch(five).run()
for i, l in enumerate(five):
    digests(f'launch set of five, call {i}', l)
sys.stdout.flush()
