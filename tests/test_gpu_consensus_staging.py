"""The consensus launch (csrc/epnp_consensus_body.inc) at the edges of its inlier bookkeeping: inlier sets on both sides of a 64-lane chunk,
of the 256 candidates one pass of the workgroup covers and of the full set (the per-inlier terms are NOT staged through LDS: that part of the
round was not built, the file keeps the name the round gave it); the best model's mask taken from the counting loop's kept ballots (its round has at most 10
hypotheses and found the model) against the mask evaluated again (wider rounds, a model of the first round used in the second); launch sets
with the one- and the two-launch second round; plain solvePnP.  Masks bit-exact and the initial pose within test_gpu_epnp's bars against the
restatement (oracle/epnp.inc), and every output equal across the ways the work can be split."""
import numpy as np
import pytest
import torch

from monorun_amd import synthetic as syn
from tests.test_gpu_epnp import INIT_TOL, POSE_TOL, _check_stage, _stage_reference

pytestmark = pytest.mark.gpu
HW, NOBJ = 18, 24
# (inliers, gross outliers) among the candidates of an object: the counts aimed at lie on both sides of 64, 128, 192 and 256 and at the ends
# (5 = the least a model is accepted with, 324 = every point); the second row has so many outliers that the replayed loop keeps running
# after it has found its best model
TARGETS = [(5, 1), (63, 2), (64, 2), (65, 2), (255, 3), (256, 3), (257, 3), (320, 4), (324, 0), (321, 3), (127, 2), (128, 2), (129, 2), (191, 2), (193, 2), (192, 2),
           (63, 30), (64, 30), (65, 30), (128, 60), (255, 69), (256, 68), (257, 67), (200, 100)]
CLASSES = (5, 63, 64, 65, 255, 256, 257)          # + "320 or more"
FIRSTS = (1, 3, 10, 20, 30)        # 20: the second round has 10 hypotheses and keeps its ballots


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _t(dev, a):
    t = torch.from_numpy(np.asarray(a))
    d = torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=dev)
    d.copy_(t)
    return d


_cache = {}


def _inputs(dtype):
    """24 of the largest objects of a synthetic.make_batch draw at hw = 18 (P = 324).  Per object k inliers and m gross outliers are the
    candidates (istd = 1, every other point's 1e-3): the image point of an inlier is the projection of its 3-D point under the object's
    pose, an outlier's lies 60 ... 120 px off, so a model of five inliers counts exactly the k inliers.  fp16 storage: the 3-D points are
    rounded before they are projected, and the oracle sees the rounded image points."""
    if dtype in _cache:
        return _cache[dtype]
    b = syn.make_batch(B=96, hw=HW, seed=1810, outlier_frac=0.0, noise_3d=0.0)
    x2d, istd, x3d, K, ur, vr, thr = [np.ascontiguousarray(a).copy() for a in syn.pnp_boundary(b, planar=False)]
    pick = np.argsort(-thr)[:NOBJ]
    x2d, istd, x3d, thr = x2d[pick], istd[pick], x3d[pick], thr[pick]
    yaw, t = b['gt_yaw'][pick], b['gt_t'][pick]
    if dtype == 'f16':
        x3d = x3d.astype(np.float16).astype(np.float32)
    rng = np.random.default_rng(7)
    P = x2d.shape[1]
    Xc = syn._to_cam(x3d.astype(np.float64), yaw, t)
    Kd = K.reshape(3, 3).astype(np.float64)
    x2d[..., 0] = (Kd[0, 0] * Xc[..., 0] / Xc[..., 2] + Kd[0, 2]).astype(np.float32)
    x2d[..., 1] = (Kd[1, 1] * Xc[..., 1] / Xc[..., 2] + Kd[1, 2]).astype(np.float32)
    for i, (k, m) in enumerate(TARGETS):
        order = rng.permutation(P)
        out = order[k:k + m]
        ang = rng.uniform(0, 2 * np.pi, m)
        x2d[i, out] += (rng.uniform(60, 120, m)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)).astype(np.float32)
        istd[i] = 1e-3
        istd[i, order[:k + m]] = 1.0
    if dtype == 'f16':
        x2d = x2d.astype(np.float16).astype(np.float32)
    _cache[dtype] = (x2d, istd, x3d, K, ur, vr, thr)
    return _cache[dtype]


def _device(dev, dtype, arrays):
    d = [_t(dev, a) for a in arrays]
    conv = {'f32': lambda a: a, 'f16': lambda a: a.half(), 'f64': lambda a: a.double()}[dtype]      # f16: exact (the values are fp16 values); f64: float32 values in fp64 storage
    return [conv(a) for a in d]


_refs = {}


def _reference(orc, dtype):
    if dtype not in _refs:
        x2d, istd, x3d, K, ur, vr, thr = _inputs(dtype)
        _refs[dtype] = _stage_reference(orc, x2d, istd, x3d, K, thr)
    return _refs[dtype]


def _best_iteration(r):
    """the iteration of the sequential loop that found the best model (strict improvement: the first one with the final count;
    r['mask'] is over the candidates, r['full_mask'] the same bits scattered to point space)"""
    cnt = np.asarray(r['cnt'])
    assert int(r['mask'].sum()) == int(r['full_mask'].sum())
    return int(np.nonzero(cnt == int(r['mask'].sum()))[0][0])


@pytest.mark.parametrize('dtype', ['f32', 'f16', 'f64'])
def test_inlier_counts_at_the_chunk_edges(dev, orc, dtype):
    """inlier counts after RANSAC on both sides of 64, 256 and the full set, 5 at the low end: masks bit-exact, initial pose <= 1e-9; then
    the flow's LM outputs against u2d_pnp_epnp"""
    from monorun_amd.ops.least_squares.pnp_uncert import epnp_ransac_device, pnp_uncert_from_init_device
    x2d, istd, x3d, K, ur, vr, thr = _inputs(dtype)
    refs = _reference(orc, dtype)
    counts = sorted(int(r['mask'].sum()) for r in refs if r['ok'])
    print('inlier counts of the best models:', counts)
    present = sum(c in counts for c in CLASSES) + (max(counts) >= 320)
    assert present >= 6, counts
    d = _device(dev, dtype, (x2d, istd, x3d))
    g = epnp_ransac_device(*d, _t(dev, K), epnp_istd_thres=0.6, epnp_ransac_thres=_t(dev, thr), with_diag=True, debug_hypotheses=True)
    torch.cuda.synchronize()
    _check_stage(g, refs)
    ref = orc.u2d_pnp_epnp(x2d, istd, x3d, K, ur, vr, 0.5, 0.6, thr, True, return_diag=True, return_init=True, num_threads=0)
    r_ret, r_yaw, r_t, r_cov, r_tr, r_mask, r_diag, r_init = ref
    valid, pose, cov, tr, mask, diag = [a.cpu().numpy() for a in pnp_uncert_from_init_device(*d, _t(dev, K), _t(dev, ur), _t(dev, vr), g[0], g[1], g[2], z_min=0.5,
                                                                                           inlier_opt_only=True, with_diag=True)]
    assert np.array_equal(mask.astype(bool), r_mask) and np.array_equal(valid.astype(bool), r_ret)
    assert np.abs(g[0].cpu().numpy() - r_init).max() <= INIT_TOL
    ok = r_ret
    dyaw = np.abs(np.angle(np.exp(1j * (pose[:, 0] - r_yaw[:, 0]))))
    assert dyaw[ok].max() <= POSE_TOL and np.abs(pose[:, 1:] - r_t)[ok].max() <= POSE_TOL


@pytest.mark.parametrize('dtype', ['f32', 'f16', 'f64'])
def test_kept_ballots_against_the_mask_evaluated_again(dev, orc, dtype):
    """first rounds of 1, 3, 10 (the ballots are kept), 20 (kept in the second round, which then has 10 hypotheses) and 30 (they are not): identical initialiser and LM outputs.  Among the objects are
    ones whose best model is found inside a first round that does not end the loop: their second round evaluates the mask again"""
    from monorun_amd import PnPEpnpLaunch
    x2d, istd, x3d, K, ur, vr, thr = _inputs(dtype)
    refs = _reference(orc, dtype)
    carried = [(i, first) for i, r in enumerate(refs) if r['ok'] for first in (1, 3, 10) if _best_iteration(r) < first < r['iters']]
    assert carried, [(_best_iteration(r), r['iters']) for r in refs if r['ok']]
    d = _device(dev, dtype, (x2d, istd, x3d))
    res = []
    for first in FIRSTS:
        l = PnPEpnpLaunch(*d, _t(dev, K), _t(dev, ur), _t(dev, vr), z_min=0.5, epnp_istd_thres=0.6, epnp_ransac_thres=_t(dev, thr), inlier_opt_only=True,
                          with_diag=True, first_round=first)
        l.run()
        torch.cuda.synchronize()
        res.append([t.clone() for t in (l.init_pose, l.init_mask, l.init_valid, l.init_diag, l.valid, l.pose, l.cov, l.mask)])
    for i, r in enumerate(refs):
        assert np.array_equal(res[0][1][i].cpu().numpy().astype(bool), r['full_mask']), i
    for first, r in zip(FIRSTS[1:], res[1:]):
        assert all(torch.equal(p, q) for p, q in zip(r, res[0])), first


@pytest.mark.parametrize('B,hw,members', [(24, HW, 2), (700, 10, 3)])
def test_launch_sets_equal_the_calls_one_by_one(dev, B, hw, members):
    """two members below 2048 objects in all (one-launch second round) and three of 700 objects (2100: two compact launches, first round of 3)"""
    from monorun_amd import PnPEpnpLaunch, PnPEpnpGroupLaunch
    kw = dict(z_min=0.5, epnp_istd_thres=0.6, inlier_opt_only=True, with_diag=True)
    if B == NOBJ:
        a = _inputs('f32')
        bs = [[_t(dev, x) for x in a], [_t(dev, x) for x in (a[0][::-1].copy(), a[1][::-1].copy(), a[2][::-1].copy(), a[3], a[4], a[5], a[6][::-1].copy())]]
    else:
        bs = [[_t(dev, x) for x in syn.pnp_boundary(syn.make_batch(B=B, hw=hw, seed=500 + i, outlier_frac=(0.15, 0.4, 0.3)[i]), planar=True)] for i in range(members)]
    outs = lambda l: [t.clone() for t in (l.init_pose, l.init_mask, l.init_valid, l.init_diag, l.valid, l.pose, l.cov, l.mask)]
    single = []
    for x in bs:
        l = PnPEpnpLaunch(*x[:6], epnp_ransac_thres=x[6], **kw)
        l.run()
        torch.cuda.synchronize()
        single.append(outs(l))
    ls = [PnPEpnpLaunch(*x[:6], epnp_ransac_thres=x[6], **kw) for x in bs]
    PnPEpnpGroupLaunch(ls).run()
    torch.cuda.synchronize()
    assert int(single[0][2].sum()) > 0.8 * B
    if B != NOBJ:
        assert any(bool((s[3][:, 0] > 3).any()) for s in single)                 # objects whose loop ran past the set's first round of 3
    for c, l in enumerate(ls):
        assert all(torch.equal(p, q) for p, q in zip(outs(l), single[c])), c


def test_plain_solvepnp_enters_with_the_candidate_list(dev, orc):
    """no thresholds (EP_MODE_PLAIN): no RANSAC block, the re-fit's list is the candidate list — 5 ... 324 candidates around the chunk edges"""
    from monorun_amd.ops.least_squares.pnp_uncert import epnp_ransac_device
    x2d, istd, x3d, K, ur, vr, thr = _inputs('f32')
    ini, imask, ivalid, _, _ = epnp_ransac_device(_t(dev, x2d), _t(dev, istd), _t(dev, x3d), _t(dev, K), epnp_istd_thres=0.6)
    torch.cuda.synchronize()
    ini, imask, ivalid = ini.cpu().numpy(), imask.cpu().numpy().astype(bool), ivalid.cpu().numpy().astype(bool)
    cand = orc.istd_inlier_mask(istd, np.float32(0.6))
    assert sorted(int(c.sum()) for c in cand) == sorted(k + m for k, m in TARGETS)
    for i in range(NOBJ):
        rvec, tvec, _ = orc.epnp(x3d[i][cand[i]], x2d[i][cand[i]], K)
        assert np.array_equal(imask[i], cand[i]) and ivalid[i]
        assert np.abs(np.array([rvec[1], *tvec]) - ini[i]).max() <= INIT_TOL, i
