"""What an object of the LM launch that carries the re-fit (pnp_uncert_refit_kernel) spends before its first useful flop, thread 0 of every object whose
re-fit ran: stamps 0 -> 1 (tile and per-object scalars loaded, first barrier), 1 -> 2 (stage 1: the inlier list in LDS), 2 -> 10 (the re-fit prologue's inputs
— prep_r, the candidate records — have arrived: the wait at the head of the prologue), 10 -> 5 (the candidates' error pass and the choice), against the whole
object (0 -> 7).  One 1024-object call (PnPEpnpLaunch) and one launch set of five such calls (PnPEpnpGroupLaunch), the reference flow as bench.py runs it.
A stamps build:
    tools/build_variant.sh stamps -DMR_DEBUG_STAMPS;  MR_PNP_SO=monorun_amd/variants/libmr_stamps.so python tools/gpu_lm_handover_stamps.py
Development aid (profiles/r15_lm_handover_stamps.txt); compare builds interval by interval, the stamps build's run time is not the release build's."""
import ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from monorun_amd import synthetic as syn, _lib, PnPEpnpLaunch, PnPEpnpGroupLaunch
dev = torch.device('cuda:0')
lib = _lib.load()
lib.mr_pnp_debug_set_stamps.argtypes = [ctypes.c_void_p]
BO = 1024
INTERVALS = [(0, 1, 'tile + scalars, first barrier'), (1, 2, 'stage 1: inlier list in LDS'), (2, 10, 'prologue inputs arrive (wait)'),
             (10, 5, 'error pass + choice'), (2, 5, 'prologue (whole)'), (0, 5, 'before the LM'), (0, 7, 'whole object')]


def dv(a):
    t = torch.from_numpy(np.asarray(a)); d = torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=dev); d.copy_(t); return d


def launches(n):
    out = []
    for i in range(n):
        b = [dv(a) for a in syn.pnp_boundary(syn.make_batch(B=BO, seed=1234 + 7919 * i), planar=True)]
        out.append(PnPEpnpLaunch(*b[:6], z_min=0.5, epnp_istd_thres=0.6, epnp_ransac_thres=b[6], inlier_opt_only=True))
    return out


def measure(label, run, members):
    nobj = BO * len(members)
    st = torch.zeros(max(nobj, 64), 24, dtype=torch.int64, device=dev)       # 24 stamps per object of the LM launch; the initialiser's first 64 workgroups
    for _ in range(4):
        st.zero_()
        lib.mr_pnp_debug_set_stamps(st.data_ptr())
        run()
        torch.cuda.synchronize()
    lib.mr_pnp_debug_set_stamps(None)
    s = st.cpu().numpy()[:nobj].astype(np.float64)
    ok = (torch.cat([m.init_valid for m in members]).cpu().numpy() != 0) & (s[:, 10] > 0)
    s = s[ok]
    ghz = np.median((s[:, 7] - s[:, 0]) / np.maximum((s[:, 9] - s[:, 8]) * 10.0, 1.0))
    print(f'{label}: {int(ok.sum())} objects with a re-fit; shader clock {ghz:.2f} GHz (stamps build)')
    for i, j, name in INTERVALS:
        us = (s[:, j] - s[:, i]) / ghz / 1e3
        print(f'  {i:2d} -> {j:2d} {name:<32} median {np.median(us):6.2f} us  mean {us.mean():6.2f} us  p90 {np.percentile(us, 90):6.2f} us')
    gate = (s[:, 2] - s[:, 1] + s[:, 10] - s[:, 2]) / ghz / 1e3
    print(f'  stage 1 + the wait at the head of the prologue (1 -> 10): median {np.median(gate):6.2f} us  mean {gate.mean():6.2f} us', flush=True)


one = launches(1)
measure(f'one call of {BO} objects', lambda: one[0].run(), one)
five = launches(5)
g = PnPEpnpGroupLaunch(five)
measure(f'one launch set of five calls ({5 * BO} objects)', g.run, five)
