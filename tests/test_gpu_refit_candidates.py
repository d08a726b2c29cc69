"""The re-fit's candidate poses are solved in `epnp_refit_betas_kernel` (round 8) and only evaluated where the re-fit ends: the initialiser's
hand-over — init_pose, init_valid and its diagnostics — is bit-equal across the three paths that end it: `epnp_refit_kernel` (the
initialiser alone, mr_epnp_ransac_batched), the LM launch that carries the re-fit (one call, MR_EPNP_DEFER_REFIT), and a launch set of
three calls; for fp32, fp16 and fp64 storage and 2, 4 and 8 waves per object in the LM launch (2: one wave evaluates two candidates in
one pass over the inliers)."""
import numpy as np
import pytest
import torch

from monorun_amd import synthetic as syn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _t(dev, a):
    t = torch.from_numpy(np.asarray(a))
    d = torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=dev)
    d.copy_(t)
    return d


def _batch(dev, dtype, seed, rng):
    b = syn.make_batch(B=96, hw=(12 if dtype == np.float16 else 28), seed=seed)
    x = [np.array(a, copy=True) for a in syn.pnp_boundary(b, planar=True)]
    P = x[0].shape[1]
    for i in range(0, 12):                                 # gross outliers: many RANSAC iterations
        bad = rng.random(P) < 0.5
        x[2][i, bad] += rng.normal(0, 0.8, (int(bad.sum()), 3)).astype(np.float32)
    x[6][12:16] = 1e-4                                     # RANSAC fails
    for i in range(16, 20):                                # exactly five candidates
        x[1][i] = 1e-3
        x[1][i, rng.choice(P, 5, replace=False)] = 1.0
    x[2][20] = 0.0; x[0][21, 3] = np.nan; x[2][22, :, 1] = 0.0
    return [_t(dev, np.ascontiguousarray(a.astype(dtype)) if k < 3 else a) for k, a in enumerate(x)]


def test_candidate_poses_agree_across_the_paths_that_end_the_refit(dev):
    from monorun_amd import PnPEpnpLaunch, PnPEpnpGroupLaunch
    from monorun_amd.ops.least_squares.pnp_uncert import epnp_ransac_device
    rng = np.random.default_rng(23)
    kw = dict(z_min=0.5, epnp_istd_thres=0.6, inlier_opt_only=True, with_diag=True)
    for dtype in (np.float32, np.float16, np.float64):
        xs = [_batch(dev, dtype, int(rng.integers(1 << 30)), rng) for _ in range(3)]
        refs = [epnp_ransac_device(x[0], x[1], x[2], x[3], epnp_istd_thres=0.6, epnp_ransac_thres=x[6], with_diag=True) for x in xs]
        torch.cuda.synchronize()
        assert int(refs[0][2].sum()) > 60 and not bool(refs[0][2][12:16].any())
        for w in (2, 4, 8):
            one = PnPEpnpLaunch(*xs[0][:6], epnp_ransac_thres=xs[0][6], flags=w << 8, fused=True, **kw)
            one.run()
            ms = [PnPEpnpLaunch(*x[:6], epnp_ransac_thres=x[6], flags=w << 8, **kw) for x in xs]
            PnPEpnpGroupLaunch(ms, lm='fused').run()
            torch.cuda.synchronize()
            for l, r in [(one, refs[0])] + list(zip(ms, refs)):
                assert torch.equal(l.init_pose, r[0]), (dtype, w)
                assert torch.equal(l.init_valid, r[2]), (dtype, w)
                assert torch.equal(l.init_diag, r[3]), (dtype, w)
