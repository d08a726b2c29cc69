"""Time of the pnp_uncert backward launch (``mr_pnp_uncert_backward_batched``) at B = 100 and B = 1024 config-2 objects (P = 784),
after warm-up, with HIP events; the fused forward launch of the same objects (``mr_pnp_uncert_batched``: initialiser, LM,
covariance) alongside for scale.  Loss on pose and covariance (the heavier form).  Development aid:
    python tools/gpu_backward_timing.py"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from monorun_amd import _lib, synthetic as syn
from monorun_amd.ops.least_squares.pnp_uncert import PnPLaunch, _strides

dev = torch.device('cuda:0')
lib = _lib.load()


def timed(fn, reps=50):
    """(median of single launches bracketed by events, mean of `reps` back-to-back launches) in us"""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    single = float(np.median([e0.elapsed_time(e1) for e0, e1 in ev])) * 1e3
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return single, e0.elapsed_time(e1) * 1e3 / reps


out = {}
for B in (100, 1024):
    b = syn.make_batch(B=B, seed=1234)
    x = [torch.from_numpy(np.asarray(a)).to(dev) for a in syn.pnp_boundary(b, planar=True)]
    fwd = PnPLaunch(*x[:6], z_min=0.5, epnp_istd_thres=0.6, epnp_ransac_thres=x[6], inlier_opt_only=True)
    fwd.run()
    torch.cuda.synchronize()
    x2d, istd, x3d = x[:3]
    cam, ur, vr = fwd.keep['cam_mats'], fwd.keep['u_range'], fwd.keep['v_range']
    g = torch.Generator().manual_seed(0)
    gp = torch.randn(B, 4, generator=g).to(dev)
    gc = torch.randn(B, 16, generator=g).to(dev)
    g2 = torch.empty(B, 784, 2, device=dev)
    gw = torch.empty(B, 784, 2, device=dev)
    g3 = torch.empty(B, 784, 3, device=dev)
    st = torch.empty(B, device=dev, dtype=torch.uint8)
    stream = torch.cuda.current_stream(dev).cuda_stream
    args = [x2d.data_ptr(), _strides(x2d), istd.data_ptr(), _strides(istd), x3d.data_ptr(), _strides(x3d), _lib.MR_F32,
            cam.data_ptr(), cam.shape[0], ur.data_ptr(), vr.data_ptr(), ur.shape[0], fwd.pose.data_ptr(), fwd.mask.data_ptr(),
            fwd.valid.data_ptr(), 0, gp.data_ptr(), fwd.cov.data_ptr(), gc.data_ptr(), B, 784, 0.5,
            g2.data_ptr(), gw.data_ptr(), g3.data_ptr(), st.data_ptr(), stream]
    bwd = lambda: lib.mr_pnp_uncert_backward_batched(*args)
    assert bwd() == 0
    torch.cuda.synchronize()
    b1, bn = timed(bwd)
    f1, fn = timed(fwd.run)
    out[f'B{B}'] = dict(backward_us_single=round(b1, 1), backward_us_back_to_back=round(bn, 1), forward_fused_us_single=round(f1, 1),
                        forward_fused_us_back_to_back=round(fn, 1), status_ok=int((st == 0).sum()), valid=int(fwd.valid.sum()))
print(json.dumps(out))
