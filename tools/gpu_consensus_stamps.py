"""Where an object spends its time in the consensus launches (epnp_consensus_body.inc, EPC_STAMP: thread 0 of every object, both rounds): median, mean and p90 per phase
for one 1024-object call (PnPEpnpLaunch: first round of 10, the second round as epnp_round2_kernel) and for one launch set of five such calls (PnPEpnpGroupLaunch: first
round of 3, two compact launches per round), batch 0 of bench.py's data, the reference flow as bench.py runs it.  A stamps build:
    tools/build_variant.sh stamps -DMR_DEBUG_STAMPS;  MR_PNP_SO=monorun_amd/variants/libmr_stamps.so python tools/gpu_consensus_stamps.py
Development aid (profiles/r10_consensus_stamps.txt); compare builds phase by phase, the stamps build's run time is not the release build's."""
import ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from monorun_amd import synthetic as syn, _lib, PnPEpnpLaunch, PnPEpnpGroupLaunch
dev = torch.device('cuda:0')
lib = _lib.load()
lib.mr_pnp_debug_set_consensus_stamps.argtypes = [ctypes.c_void_p]
BO = 1024
PHASES = ['tile loaded', 'counts done', 'loop replayed', 'mask + list done', 'control points done', 'moments done', 'end']


def dv(a):
    t = torch.from_numpy(np.asarray(a)); d = torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=dev); d.copy_(t); return d


def launches(n):
    out = []
    for i in range(n):
        b = [dv(a) for a in syn.pnp_boundary(syn.make_batch(B=BO, seed=1234 + 7919 * i), planar=True)]
        out.append(PnPEpnpLaunch(*b[:6], z_min=0.5, epnp_istd_thres=0.6, epnp_ransac_thres=b[6], inlier_opt_only=True))
    return out


def line(name, us):
    print(f'  {name:<34} n {len(us):5d}  median {np.median(us):6.2f} us  mean {us.mean():6.2f} us  p90 {np.percentile(us, 90):6.2f} us')


def measure(label, run, members):
    nobj = BO * len(members)
    st = torch.zeros(nobj, 2, 12, dtype=torch.int64, device=dev)        # per object and round: stamps 0..7 (cycles), 8, 9 (100 MHz clock)
    for _ in range(4):
        st.zero_()
        lib.mr_pnp_debug_set_consensus_stamps(st.data_ptr())
        run()
        torch.cuda.synchronize()
    lib.mr_pnp_debug_set_consensus_stamps(None)
    s = st.cpu().numpy().astype(np.float64)
    done = [(s[:, r, 7] > 0) & (s[:, r, 6] > 0) for r in (0, 1)]          # the round in which the object went through to its moments
    left = (s[:, 0, 7] > 0) & (s[:, 0, 6] == 0) & (s[:, 0, 3] > 0)       # first round left with the loop pending
    r0 = s[s[:, 0, 7] > 0, 0]
    ghz = np.median((r0[:, 7] - r0[:, 0]) / np.maximum((r0[:, 9] - r0[:, 8]) * 10.0, 1.0))
    print(f'{label}: {int(done[0].sum())} objects finish in the first round, {int(left.sum())} leave it pending, {int(done[1].sum())} finish in the second; shader clock {ghz:.2f} GHz (stamps build)')
    for r in (0, 1):
        if not done[r].any():
            continue
        q = s[done[r], r]
        print(f' objects finishing in round {r}:')
        for i, name in enumerate(PHASES):
            line(f'{i} -> {i + 1} {name}', (q[:, i + 1] - q[:, i]) / ghz / 1e3)
        line('0 -> 7 whole object', (q[:, 7] - q[:, 0]) / ghz / 1e3)
    if left.any():
        q = s[left, 0]
        print(' objects leaving the first round pending:')
        for i, name in enumerate(PHASES[:3]):
            line(f'{i} -> {i + 1} {name}', (q[:, i + 1] - q[:, i]) / ghz / 1e3)
        line('3 -> 7 samples of the next round', (q[:, 7] - q[:, 3]) / ghz / 1e3)
    sys.stdout.flush()


one = launches(1)
measure(f'one call of {BO} objects', lambda: one[0].run(), one)
five = launches(5)
g = PnPEpnpGroupLaunch(five)
measure(f'one launch set of five calls ({5 * BO} objects)', g.run, five)
