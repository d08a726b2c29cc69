"""How long the re-fit prologue of the LM launch that carries it (pnp_uncert_refit_kernel: stamps 2 -> 5, the candidates' pose and error
passes) takes against the object's whole span in that launch (stamps 0 -> 7), thread 0 of every object whose re-fit ran: one 1024-object
call (PnPEpnpLaunch) and one launch set of five such calls (PnPEpnpGroupLaunch), the reference flow as bench.py runs it.  A stamps build:
    tools/build_variant.sh stamps -DMR_DEBUG_STAMPS;  MR_PNP_SO=monorun_amd/variants/libmr_stamps.so python tools/gpu_refit_prologue_stamps.py
Development aid (profiles/r08_refit_prologue_stamps.txt); read the shares, not the stamps build's run time."""
import ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from monorun_amd import synthetic as syn, _lib, PnPEpnpLaunch, PnPEpnpGroupLaunch
dev = torch.device('cuda:0')
lib = _lib.load()
lib.mr_pnp_debug_set_stamps.argtypes = [ctypes.c_void_p]
BO = 1024


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
    ok = torch.cat([m.init_valid for m in members]).cpu().numpy() != 0
    pro = s[ok, 5] - s[ok, 2]
    tot = s[ok, 7] - s[ok, 0]
    ghz = np.median(tot / np.maximum((s[ok, 9] - s[ok, 8]) * 10.0, 1.0))
    us = lambda c: c / ghz / 1e3
    print(f'{label}: {int(ok.sum())} objects with a re-fit; shader clock {ghz:.2f} GHz (stamps build)')
    print(f'  prologue (stamps 2 -> 5)   median {np.median(pro):8.0f} cycles ({us(np.median(pro)):6.2f} us)  mean {us(pro.mean()):6.2f} us  p90 {us(np.percentile(pro, 90)):6.2f} us')
    print(f'  object     (stamps 0 -> 7)   median {np.median(tot):8.0f} cycles ({us(np.median(tot)):6.2f} us)  mean {us(tot.mean()):6.2f} us  p90 {us(np.percentile(tot, 90)):6.2f} us')
    print(f'  prologue share: of the median object {100 * np.median(pro) / np.median(tot):5.1f} %, of the summed object time {100 * pro.sum() / tot.sum():5.1f} %', flush=True)


one = launches(1)
measure(f'one call of {BO} objects', lambda: one[0].run(), one)
five = launches(5)
g = PnPEpnpGroupLaunch(five)
measure(f'one launch set of five calls ({5 * BO} objects)', g.run, five)
