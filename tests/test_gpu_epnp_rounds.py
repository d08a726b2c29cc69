"""The reference flow's two rounds of hypotheses on the GPU: where the first round ends changes the work, never a result.  The front
launch fetches the samples of the first round only; the consensus launch writes those of a pending object's second round from its
geometry tile.  Forcing the first round to 1, 2, 3 and 10 hypotheses makes many objects pending, single calls and launch sets, fp32 /
fp16 / fp64 storage, the one- and the two-launch second round."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from monorun_amd import synthetic as syn
from tests.test_gpu_epnp import _check_stage, _stage_reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRSTS = (1, 2, 3, 10)


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _t(dev, a):
    t = torch.from_numpy(np.asarray(a))
    d = torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=dev)
    d.copy_(t)
    return d


def _batches(seed=2718):
    """a config-2 batch and a low-inlier-ratio one (40 - 70 % gross outliers: the replayed loop runs long)"""
    cfg2 = [np.ascontiguousarray(a) for a in syn.pnp_boundary(syn.make_batch(B=64, seed=seed), planar=True)]
    x2d, istd, x3d, K, ur, vr, thr = [np.ascontiguousarray(a).copy() for a in syn.pnp_boundary(syn.make_batch(B=32, seed=seed + 1), planar=False)]
    rng = np.random.default_rng(seed)
    for i in range(x2d.shape[0]):
        bad = rng.random(x2d.shape[1]) < rng.uniform(0.4, 0.7)
        x3d[i, bad] += rng.normal(0, 0.8, (int(bad.sum()), 3)).astype(np.float32)
    return [cfg2, [x2d, istd, x3d, K, ur, vr, thr]]


@pytest.mark.parametrize('dtype', ['f32', 'f16', 'f64'])
def test_first_round_choices_single_calls(dev, orc, dtype):
    from monorun_amd.ops.least_squares.pnp_uncert import epnp_ransac_device
    for bi, (x2d, istd, x3d, K, ur, vr, thr) in enumerate(_batches()):
        d = [_t(dev, a) for a in (x2d, istd, x3d)]
        if dtype == 'f16':
            d = [a.half() for a in d]
            x2d, istd, x3d = [np.ascontiguousarray(a.float().cpu().numpy()) for a in d]          # the oracle sees the rounded values
        elif dtype == 'f64':
            d = [a.double() for a in d]                                                           # float32 values in fp64 storage
        refs = _stage_reference(orc, x2d, istd, x3d, K, thr)
        if bi == 1:
            assert max(r['iters'] for r in refs) >= 20
        outs = []
        for first in FIRSTS:
            g = epnp_ransac_device(*d, _t(dev, K), epnp_istd_thres=0.6, epnp_ransac_thres=_t(dev, thr), with_diag=True,
                                   debug_hypotheses=True, first_round=first)
            torch.cuda.synchronize()
            _check_stage(g, refs)
            outs.append(g[:4])
        for first, o in zip(FIRSTS[1:], outs[1:]):
            assert all(torch.equal(p, q) for p, q in zip(o, outs[0])), (bi, first)


@pytest.mark.parametrize('B', [192, 1024])
def test_first_round_choices_launch_sets(dev, B):
    """two calls per launch set: 384 objects (one-launch second round) and 2048 (two compact launches); every output of every call
    equal across the first-round choices"""
    from monorun_amd import PnPEpnpLaunch, PnPEpnpGroupLaunch
    kw = dict(z_min=0.5, epnp_istd_thres=0.6, inlier_opt_only=True, with_diag=True)
    bs = [[_t(dev, a) for a in syn.pnp_boundary(syn.make_batch(B=B, seed=31 + i, outlier_frac=(0.15, 0.4)[i]), planar=True)] for i in range(2)]
    res = []
    for first in FIRSTS:
        ls = [PnPEpnpLaunch(*x[:6], epnp_ransac_thres=x[6], first_round=first, **kw) for x in bs]
        PnPEpnpGroupLaunch(ls).run()
        torch.cuda.synchronize()
        res.append([[t.clone() for t in (l.init_pose, l.init_mask, l.init_valid, l.init_diag, l.valid, l.pose, l.cov, l.mask)] for l in ls])
    assert int(res[0][0][2].sum()) > 0.9 * B
    assert any(bool((r[3][:, 0] > 3).any()) for r in res[0])                 # objects whose loop ran past a short first round
    for first, r in zip(FIRSTS[1:], res[1:]):
        for c in range(2):
            assert all(torch.equal(p, q) for p, q in zip(r[c], res[0][c])), (first, c)


def test_56x56_pending_objects(dev):
    """the config-5 shape through the geometry tile with a first round of one hypothesis (most objects pending) against the default"""
    from monorun_amd.ops.least_squares.pnp_uncert import epnp_ransac_device
    b = syn.make_batch(B=24, hw=56, seed=4321, outlier_frac=0.4)
    x2d, istd, x3d, K, ur, vr, thr = [_t(dev, a) for a in syn.pnp_boundary(b, planar=True)]
    for conv in (lambda a: a, lambda a: a.half()):
        d = [conv(a) for a in (x2d, istd, x3d)]
        a = epnp_ransac_device(*d, K, epnp_istd_thres=0.6, epnp_ransac_thres=thr, with_diag=True)
        c = epnp_ransac_device(*d, K, epnp_istd_thres=0.6, epnp_ransac_thres=thr, with_diag=True, first_round=1)
        torch.cuda.synchronize()
        assert all(torch.equal(p, q) for p, q in zip(a[:4], c[:4]))
        assert int(a[2].sum()) >= 20 and bool((a[3][:, 0] > 1).any())


_CHILD = r'''
import hashlib, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch
from monorun_amd import synthetic as syn, PnPEpnpLaunch, PnPEpnpGroupLaunch
dev = torch.device('cuda:0')
def dv(a):
    t = torch.from_numpy(np.asarray(a)); d = torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=dev); d.copy_(t); return d
bs = [[dv(a) for a in syn.pnp_boundary(syn.make_batch(B=256, seed=71 + i, outlier_frac=0.4), planar=True)] for i in range(3)]
ls = [PnPEpnpLaunch(*x[:6], epnp_ransac_thres=x[6], z_min=0.5, epnp_istd_thres=0.6, inlier_opt_only=True, with_diag=True, first_round=2) for x in bs]
outs = lambda l: (l.valid, l.pose, l.cov, l.tr, l.mask, l.init_pose, l.init_mask, l.init_valid, l.diag, l.init_diag)
for l in ls:
    for t in outs(l):
        t.zero_()
PnPEpnpGroupLaunch(ls).run()
torch.cuda.synchronize()
h = hashlib.sha256()
for l in ls:
    for t in outs(l):
        h.update(t.cpu().numpy().tobytes())
print('pending', int(sum(int((l.init_diag[:, 0] > 2).sum()) for l in ls)), 'digest', h.hexdigest())
'''


def test_one_launch_and_two_launch_second_round_agree():
    """a launch set of three calls (768 objects) with MR_EP_ROUND2=1 (two compact launches) against =2 (one launch), each in a fresh
    process: digests over every output, the buffers zero-filled first"""
    lines = []
    for mode in ('1', '2'):
        env = dict(os.environ, MR_EP_ROUND2=mode)
        r = subprocess.run([sys.executable, '-c', _CHILD, ROOT], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(r.stdout.strip().splitlines()[-1])
    assert lines[0] == lines[1], lines
    assert int(lines[0].split()[1]) > 0                                     # objects went through the second round
