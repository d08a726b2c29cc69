"""Solver-free inputs for the shape, layout and edge tests of the ``pnp_uncert`` backward (tests/test_gpu_pnp_grad_shapes.py).

The kernel evaluates its formulas at whatever pose it is given, so a case needs no forward solve: the first P points of a synthetic
32 x 32 batch as (B,P,C) contiguous tensors, pose = ground truth + N(0, 0.02) rounded to f32, a random inlier mask (about 70 % ones, the
first four points in), a random SPD covariance and random output gradients.  ``cam`` / ``ranges`` select a shared or a per-object camera
and clip range; a per-object camera re-images x2d through itself, so the residuals stay those of the shared camera.  Cases and their
fp64 references (tests/pnp_grad_ref.py) are cached: treat both as read-only and ``dict(case, key=...)`` what a test changes."""
import functools
import os
import sys

import numpy as np
import torch
from torch.func import vmap

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_grad_ref as ref  # noqa: E402

Z_MIN = 0.5
COND_MAX = 1e8                       # an object is compared with the reference only if cond(H_F) <= COND_MAX in the reference's own fp64
GRADS = ('grad_x2d', 'grad_istd', 'grad_x3d')


def device():
    return torch.device('cuda:0')


def _cut(vals, lo, hi):
    """A clip bound inside the widest gap of sorted(vals)[lo:hi + 1], as f32, at least 1e-3 px from both neighbours: which rows it clips
    does not depend on the last bits of a projection."""
    s = np.sort(vals)
    j = lo + int(np.argmax(s[lo + 1:hi + 1] - s[lo:hi]))
    cut = np.float32(0.5 * (s[j] + s[j + 1]))
    assert min(float(cut) - s[j], s[j + 1] - float(cut)) > 1e-3, 'no gap wide enough for a clip bound'
    return cut


@functools.lru_cache(maxsize=None)
def make_case(B, P, seed=0, cam='shared', ranges='shared', dtype=torch.float32):
    """cam: 'shared' K (1,3,3) | 'per_object' (B,3,3) focal lengths and principal points | 'general' = per_object with a third row
    near (1e-3, -2e-3, 1.01).  ranges: 'shared' (1,2) | 'per_object' (B,2), where objects b % 3 == 1 get an upper u bound and objects
    b % 3 == 2 a lower v bound that clips about a fifth of their rows: case['clipped'] (B,P,2) bool holds exactly those rows."""
    from monorun_amd import synthetic as syn
    assert 5 <= P <= 1024
    b = syn.make_batch(B=B, hw=32, seed=100 + seed)
    x2d, istd, x3d, K, ur, vr, _ = syn.pnp_boundary(b, planar=False)
    x2d, istd, x3d = (np.asarray(a[:, :P], np.float64) for a in (x2d, istd, x3d))
    rng = np.random.default_rng(seed)
    K0 = np.asarray(K, np.float64)[0]
    Kb = K0[None].astype(np.float32)
    if cam != 'shared':
        Kb = np.repeat(K0[None], B, 0)
        Kb[:, 0, 0] *= rng.uniform(0.8, 1.2, B)
        Kb[:, 1, 1] *= rng.uniform(0.8, 1.2, B)
        Kb[:, 0, 2] += rng.normal(0, 30, B)
        Kb[:, 1, 2] += rng.normal(0, 10, B)
        if cam == 'general':
            Kb[:, 2, 0] = 1e-3 * rng.uniform(0.5, 1.5, B)
            Kb[:, 2, 1] = -2e-3 * rng.uniform(0.5, 1.5, B)
            Kb[:, 2, 2] = 1.01 + 0.02 * rng.uniform(-1, 1, B)
        Kb = Kb.astype(np.float32)
        rays = np.concatenate([x2d, np.ones((B, P, 1))], -1) @ np.linalg.inv(K0).T
        h = np.einsum('bij,bpj->bpi', Kb.astype(np.float64), rays)
        x2d = h[..., :2] / h[..., 2:]
    pose = (np.concatenate([b['gt_yaw'][:, None], b['gt_t']], 1) + rng.normal(0, 0.02, (B, 4))).astype(np.float32)
    mask = rng.uniform(size=(B, P)) < 0.7
    mask[:, :4] = True
    A = rng.normal(size=(B, 4, 4))
    cov = (1e-2 * (A @ A.transpose(0, 2, 1) / 4 + 0.5 * np.eye(4))).astype(np.float32)
    gp, gc = rng.normal(size=(B, 4)).astype(np.float32), rng.normal(size=(B, 4, 4)).astype(np.float32)
    x2d, istd, x3d = (torch.from_numpy(a).to(dtype) for a in (x2d, istd, x3d))      # the storage dtype's rounding comes first
    ur, vr = np.asarray(ur, np.float32), np.asarray(vr, np.float32)
    clipped = np.zeros((B, P, 2), bool)
    if ranges != 'shared':
        assert P >= 32
        ur, vr = np.repeat(ur, B, 0), np.repeat(vr, B, 0)
        ur[:, 1] += np.arange(B, dtype=np.float32)
        vr[:, 0] -= np.arange(B, dtype=np.float32)
        pi, _ = vmap(ref._proj)(torch.from_numpy(pose).double(), x3d.double(), torch.from_numpy(Kb).double().expand(B, 3, 3))
        pi = pi.numpy()
        for o in range(B):
            if o % 3 == 1:
                ur[o, 1] = _cut(pi[o, :, 0], int(0.7 * P), int(0.9 * P))
                clipped[o, :, 0] = pi[o, :, 0] > ur[o, 1]
            elif o % 3 == 2:
                vr[o, 0] = _cut(pi[o, :, 1], int(0.1 * P), int(0.3 * P))
                clipped[o, :, 1] = pi[o, :, 1] < vr[o, 0]
    dev = device()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(x2d=x2d.to(dev), istd=istd.to(dev), x3d=x3d.to(dev), K=t(Kb), ur=t(ur), vr=t(vr), pose=t(pose), mask=t(mask.astype(np.uint8)),
                valid=torch.ones(B, dtype=torch.uint8, device=dev), gp=t(gp), cov=t(cov), gc=t(gc), clipped=t(clipped))


def sub(case, idx):
    """The objects idx (a list or slice) of a case as a batch of their own; a shared camera or range stays shared."""
    pick = lambda k, v: v if v is None or (k in ('K', 'ur', 'vr') and v.shape[0] == 1) else v[idx]
    return {k: pick(k, v) for k, v in case.items()}


def run(case, lm_all, needs=(True, True, True), out=None):
    """The kernel on a case: (grad_x2d, grad_istd, grad_x3d, status)."""
    from monorun_amd.ops.least_squares.pnp_uncert import pnp_uncert_backward_device
    c = case
    return pnp_uncert_backward_device(c['x2d'], c['istd'], c['x3d'], c['K'], c['ur'], c['vr'], c['pose'], c['mask'], c['valid'], c['gp'], c['cov'],
                                      c['gc'], z_min=Z_MIN, lm_all_points=lm_all, needs=needs, with_status=True, out=out)


def same(a, b, objs=None):
    """every tensor of two results bit-identical (on the objects objs, if given)"""
    pick = (lambda t: t) if objs is None else (lambda t: t[objs])
    return all((u is None and v is None) or torch.equal(pick(u), pick(v)) for u, v in zip(a, b))


def all_zero_bits(t):
    """+0.0 everywhere: no -0.0, which torch.equal would take for a zero"""
    return bool((t.contiguous().view(torch.int32) == 0).all())


def _mask(case):
    m = case['mask']
    return (m if m is not None else torch.ones(case['x2d'].shape[:2], dtype=torch.uint8, device=case['x2d'].device)).bool()


def reference(case, lm_all):
    c = case
    return ref.pnp_grad_ref(c['x2d'], c['istd'], c['x3d'], c['K'], c['ur'], c['vr'], Z_MIN, c['pose'], _mask(c), c['valid'].bool(), lm_all,
                            c['gp'], c['cov'], c['gc'])


def row_counts_and_cond(case, lm_all):
    """Per object: the number of rows in S_LM and cond_2(H_F), both from the reference's own fp64 H_F (torch.func autodiff)."""
    c, d = case, dict(dtype=torch.float64)
    B = c['x2d'].shape[0]
    x2d, istd, x3d, pose = c['x2d'].to(**d), c['istd'].to(**d), c['x3d'].to(**d), c['pose'].to(**d)
    K, ur, vr = c['K'].to(**d).expand(B, 3, 3), c['ur'].to(**d).expand(B, 2), c['vr'].to(**d).expand(B, 2)
    m_lm, _ = ref.row_masks(x2d, x3d, K, ur, vr, Z_MIN, pose, _mask(c), lm_all)
    _, H = ref.stationarity(pose, x2d, istd, x3d, K, m_lm)
    sv = torch.linalg.svdvals(H.cpu())
    return m_lm.sum((1, 2)).cpu(), sv[:, 0] / sv[:, -1]


def check(case, lm_all, want=None, skip=(), **kw):
    """The kernel against the reference on one case: status bit-equal, per object and gradient tensor max|g - g_ref| <= TOL max|g_ref|.
    Every valid object outside `skip` must have no row in S_LM or cond(H_F) <= COND_MAX.  Returns (result, worst err / TOL)."""
    from test_gpu_pnp_grad import TOL, _close
    want = reference(case, lm_all) if want is None else want
    rows, cond = row_counts_and_cond(case, lm_all)
    for o in range(rows.shape[0]):
        if o in skip or not bool(case['valid'][o]):
            continue
        assert rows[o] == 0 or cond[o] <= COND_MAX, f'object {o}: cond(H_F) = {float(cond[o]):.3g} with {int(rows[o])} rows: not a fair comparison'
    got = run(case, lm_all, **kw)
    assert torch.equal(got[3], want[3]), ('status differs from the reference', got[3].tolist(), want[3].tolist())
    keep = [o for o in range(rows.shape[0]) if o not in skip]
    errs = [_close(g[keep], r[keep]) for g, r in zip(got[:3], want[:3]) if g is not None]
    assert all(bool(torch.isfinite(g).all()) for g in got[:3] if g is not None)
    assert max(errs) <= TOL, dict(zip(GRADS, errs))
    return got, max(errs) / TOL


@functools.lru_cache(maxsize=None)
def cached_reference(lm_all, *key):
    """reference(make_case(*key), lm_all), computed once per test session"""
    return reference(make_case(*key), lm_all)
