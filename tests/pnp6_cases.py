"""Solver-free inputs and the reference for the shape, layout and edge tests of the 6-DoF refinement (tests/test_pnp6_cases_cpu.py,
tests/test_gpu_pnp6_shapes.py).

``pnp6_refine_device`` takes the 4-DoF result as arguments, so a case needs no forward solve: ``mask``, ``pose4`` and ``valid4`` are
constructed here and a case is a pure function of its key.  ``make_case`` draws object points in a car-sized box, a full angle-axis
ground truth, projects with KITTI-like intrinsics, adds pixel noise (gross noise at the points outside the mask), draws ``istd`` as
monorun_amd.synthetic does, a random inlier mask and pose4 = (ground-truth ry, t) + a perturbation.  Everything lives on the host: the
CPU tests use the cases as they are, ``to_device`` moves one to the GPU.

The yardstick is ``reference``: the oracle's one-object 6-DoF solve (oracle.pnp6_uncert, fp64) on the fp64 widening of the STORED
values at the masked points, object by object — the same for every storage type and layout.  Cases and references are cached: treat
both as read-only and ``dict(case, key=...)`` what a test changes."""
import functools

import numpy as np
import torch

Z_MIN = 0.5
Z_MIN_CLAMP = 6.0                    # the clamp cases' z_min: in front of the objects (t_z in [9.2, 11]) except for three moved points each
UR, VR = (-200.0, 1442.0), (-200.0, 575.0)
POSE_TOL = COV_TOL = 1e-4            # tests/test_pnp6.py's: |pose6 - ref| <= 1e-4, |cov6 - ref| <= 1e-4 max|ref cov of the object|
START = {'near': (0.05, 0.03), 'far': (0.5, 0.30)}          # perturbation of pose4: yaw (rad), translation (fraction of the depth)
WHY = dict(GRADIENT=1, PARAMETER=2, FUNCTION=3, MAXITER=4, MINRADIUS=5, INVALID=6, EVALFAIL=7, NOT_STARTED=8)      # MR_DIAG_WHY
RAGGED_P = (4, 5, 8, 63, 64, 65, 255, 256, 257, 1000)
F32, F16, F64 = torch.float32, torch.float16, torch.float64

# name -> make_case key (B, P, seed, rot, cam, ranges, dtype, start, clamp, noise).  Every case the GPU tests compare with the
# reference is listed here, so that tests/test_pnp6_cases_cpu.py checks each one's claims with the oracle alone.
CASES = {
    'general_near': (16, 300, 1, 'general', 'shared', 'shared', F32, 'near'),
    'general_far': (16, 300, 2, 'general', 'shared', 'shared', F32, 'far'),
    'yaw_near': (16, 300, 1, 'yaw', 'shared', 'shared', F32, 'near'),
    'yaw_far': (16, 300, 2, 'yaw', 'shared', 'shared', F32, 'far'),
    'small_angle': (12, 100, 3, 'small'),
    'f32': (8, 300, 4, 'general', 'shared', 'shared', F32),
    'f16': (8, 300, 4, 'general', 'shared', 'shared', F16),
    'f64': (8, 300, 4, 'general', 'shared', 'shared', F64),
    'cam_both': (9, 100, 5, 'general', 'per_object', 'per_object'),
    'cam_only': (9, 100, 5, 'general', 'per_object', 'shared'),
    'ranges_only': (9, 100, 5, 'general', 'shared', 'per_object'),
    'cam_clamp': (9, 100, 5, 'general', 'per_object', 'per_object', F32, 'near', True),
    'clamp': (12, 200, 6, 'general', 'shared', 'per_object', F32, 'near', True),
    'clamp_f16': (12, 257, 6, 'general', 'shared', 'per_object', F16, 'near', True),
    'maxit': (8, 100, 23, 'general', 'shared', 'shared', F32, 'far'),          # object 4 has three rejected steps
    'exact': (12, 100, 8, 'general', 'shared', 'shared', F64, 'near', False, 0.0),
    'edge': (8, 65, 9),
    'rank': (10, 65, 10),
}
CASES.update({f'ragged_{P}': (6, P, 20 + P) for P in RAGGED_P})
MAXIT = (1, 2, 63)                   # the caps run on CASES['maxit']


def rodrigues(r):
    th = np.linalg.norm(r)
    if th < 1e-12:
        return np.eye(3)
    k = np.asarray(r) / th
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * kx + (1 - np.cos(th)) * kx @ kx


def _cut(vals, lo, hi):
    """A clip bound inside the widest gap of sorted(vals)[lo:hi + 1], as f32 (tests/pnp_grad_cases.py)."""
    s = np.sort(vals)
    j = lo + int(np.argmax(s[lo + 1:hi + 1] - s[lo:hi]))
    cut = np.float32(0.5 * (s[j] + s[j + 1]))
    assert min(float(cut) - s[j], s[j + 1] - float(cut)) > 1e-3, 'no gap wide enough for a clip bound'
    return cut


def _masks(rng, B, P, lo):
    """Inlier masks with between min(lo, P) and P ones.  With lo == 6 the first three objects are the edges of the kernel's list
    compaction: exactly 6 inliers spread over the tile, every point, and a set confined to the last 64-point chunk (to the last six
    points where that chunk holds fewer: the list's tail then crosses a chunk boundary)."""
    mask = np.zeros((B, P), bool)
    for b in range(B):
        n = int(rng.integers(min(lo, P), P + 1))
        idx = rng.permutation(P)[:n]
        if lo == 6 and b == 0:
            idx = rng.permutation(P)[:min(6, P)]
        elif lo == 6 and b == 1:
            idx = np.arange(P)
        elif lo == 6 and b == 2:
            last = np.arange(64 * ((P - 1) // 64), P)
            idx = last if 6 <= last.size <= 12 else (rng.permutation(last)[:6] if last.size > 12 else np.arange(max(P - 6, 0), P))
        mask[b, idx] = True
    return mask


@functools.lru_cache(maxsize=None)
def make_case(B, P, seed=0, rot='general', cam='shared', ranges='shared', dtype=F32, start='near', clamp=False, noise=0.5):
    """rot: 'general' (each of rx, ry, rz of magnitude in [0.15, 0.6], random sign) | 'yaw' (rx = rz = 0: the regime of
    tests/test_pnp6.py) | 'small' (0.2 rad about a general axis and pose4[:, 0] = 0 exactly: the first evaluation takes the
    first-order branch).  cam: 'shared' K (1,3,3) | 'per_object' (B,3,3), each object imaged by its own.  ranges: 'shared' (1,2) |
    'per_object' (B,2) wide, distinct ranges.  clamp=True (per-object ranges, P >= 100): every object gets an upper u bound and a
    lower v bound cut through its inliers' projections (about a tenth of the rows each), z_min = Z_MIN_CLAMP and three inlier
    points moved 0.6 behind it.  start: START.  noise: pixel sigma at the inliers (those outside the mask get 30 px more)."""
    from monorun_amd import synthetic as syn
    assert 4 <= P <= 1024 and (not clamp or (ranges == 'per_object' and P >= 100 and start == 'near'))
    rng = np.random.default_rng(1000 + seed)
    X = rng.uniform(-1, 1, (B, P, 3)) * np.array([2.0, 0.8, 0.9])
    sgn = lambda *s: rng.choice([-1.0, 1.0], s)
    if rot == 'general':
        r = sgn(B, 3) * rng.uniform(0.15, 0.6, (B, 3))
    elif rot == 'yaw':
        r = np.stack([np.zeros(B), rng.uniform(-np.pi, np.pi, B), np.zeros(B)], 1)
    else:
        assert rot == 'small'
        a = sgn(B, 3) * rng.uniform(0.3, 1.0, (B, 3))
        r = 0.2 * a / np.linalg.norm(a, axis=1, keepdims=True)
    t = np.stack([rng.uniform(-4, 4, B), rng.uniform(1, 2, B), rng.uniform(9.2, 11, B) if clamp else rng.uniform(8, 25, B)], 1)
    K0 = np.asarray(syn.KITTI_K, np.float64)
    Kb = K0[None].astype(np.float32)
    if cam != 'shared':
        Kb = np.repeat(K0[None], B, 0)
        Kb[:, 0, 0] *= rng.uniform(0.8, 1.2, B)
        Kb[:, 1, 1] *= rng.uniform(0.8, 1.2, B)
        Kb[:, 0, 2] += rng.normal(0, 30, B)
        Kb[:, 1, 2] += rng.normal(0, 10, B)
        Kb = Kb.astype(np.float32)
    Kd = np.broadcast_to(Kb.astype(np.float64), (B, 3, 3))
    mask = _masks(rng, B, P, 30 if clamp else 6)
    R = np.stack([rodrigues(r[b]) for b in range(B)])
    z_min = Z_MIN_CLAMP if clamp else Z_MIN
    zpts = np.zeros((B, P), bool)
    if clamp:
        for b in range(B):
            for p in rng.permutation(np.flatnonzero(mask[b]))[:3]:
                zc = R[b, 2] @ X[b, p] + t[b, 2]
                X[b, p] += R[b].T @ np.array([0.0, 0.0, (z_min - 0.6) - zc])
                zpts[b, p] = True
    Xc = np.einsum('bij,bpj->bpi', R, X) + t[:, None]
    assert (Xc[..., 2][~zpts] > z_min + 0.6).all() and (not clamp or np.allclose(Xc[..., 2][zpts], z_min - 0.6))
    zu = np.maximum(Xc[..., 2], z_min)
    proj = np.stack([Kd[:, None, 0, 0] * Xc[..., 0] / zu + Kd[:, None, 0, 2], Kd[:, None, 1, 1] * Xc[..., 1] / zu + Kd[:, None, 1, 2]], -1)
    x2d = proj + rng.normal(0, noise, (B, P, 2)) + (~mask)[..., None] * rng.normal(0, 30.0, (B, P, 2))
    istd = np.exp(-rng.normal(np.log(2.0), 0.5, (B, P, 2))) / 10.0
    ur, vr = np.array([UR], np.float32), np.array([VR], np.float32)
    if ranges != 'shared':
        ur, vr = np.repeat(ur, B, 0), np.repeat(vr, B, 0)
        ur[:, 1] += np.arange(B, dtype=np.float32)
        vr[:, 0] -= np.arange(B, dtype=np.float32)
    if clamp:
        for b in range(B):
            u, v = proj[b, mask[b] & ~zpts[b], 0], proj[b, mask[b] & ~zpts[b], 1]
            ur[b, 1] = _cut(u, int(0.85 * u.size), int(0.95 * u.size) - 1)
            vr[b, 0] = _cut(v, int(0.05 * v.size), int(0.15 * v.size))
    ang, frac = START[start]
    d = rng.normal(size=(B, 3))
    pose4 = np.concatenate([r[:, 1:2] + ang * sgn(B, 1), t + frac * t[:, 2:3] * d / np.linalg.norm(d, axis=1, keepdims=True)], 1).astype(np.float32)
    if rot == 'small':
        pose4[:, 0] = 0.0
    tt = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)).to(dt) if dt is not None else torch.from_numpy(np.ascontiguousarray(a))
    return dict(x2d=tt(x2d, dtype), istd=tt(istd, dtype), x3d=tt(X, dtype), K=tt(Kb), ur=tt(ur), vr=tt(vr), mask=tt(mask.astype(np.uint8)),
                pose4=tt(pose4), valid4=torch.ones(B, dtype=torch.uint8), z_min=z_min, gt=np.concatenate([r, t], 1), zpts=zpts)


TENSORS = ('x2d', 'istd', 'x3d', 'K', 'ur', 'vr', 'mask', 'pose4', 'valid4')


def case(name):
    return make_case(*CASES[name])


def sub(c, idx):
    """The objects idx (a list) of a case as a batch of their own; a shared camera or range stays shared."""
    pick = lambda k, v: v[idx] if k in TENSORS and not (k in ('K', 'ur', 'vr') and v.shape[0] == 1) else v
    return {k: pick(k, v) for k, v in c.items()}


def to_device(c, dev=None):
    dev = dev or torch.device('cuda:0')
    return {k: (v.to(dev) if k in TENSORS else v) for k, v in c.items()}


def run(c, flags=0):
    """The kernel on a case whose tensors are on the device: (valid u8 (B,), pose6 (B,6), cov6 (B,6,6), diag (B,2))."""
    from monorun_amd.ops.least_squares.pnp_uncert import pnp6_refine_device
    return pnp6_refine_device(c['x2d'], c['istd'], c['x3d'], c['K'], c['ur'], c['vr'], c['mask'], c['pose4'], c['valid4'], z_min=c['z_min'],
                              flags=flags, with_diag=True)


def same(a, b, objs=None):
    """every tensor of two results bit-identical (on the objects objs, if given); NaN equals NaN of the same bits"""
    pick = (lambda t: t) if objs is None else (lambda t: t[objs])
    bits = lambda t: pick(t).contiguous().view(torch.int32 if t.dtype == torch.float32 else t.dtype)
    return all(torch.equal(bits(u), bits(v)) for u, v in zip(a, b))


def rank_deficient(c):
    """A copy of a case whose objects 0..4 keep only their first 1..5 inliers (2n residuals for 6 parameters: J^T J singular for
    n <= 2, singular or nearly so beyond)."""
    m = c['mask'].clone()
    for b in range(5):
        m[b, torch.nonzero(m[b])[b + 1:, 0]] = 0
    return dict(c, mask=m)


def object_problem(c, b):
    """Object b as the oracle's one-object entry points take it: the fp64 widening of the stored values at the masked points
    (pts2d, pts3d, wgt2d, K9, init pose6 = (0, f32 yaw, 0, f32 t), clips)."""
    m = c['mask'][b].bool()
    f = lambda t: t[b][m].double().numpy()
    kb, rb = (b if c['K'].shape[0] > 1 else 0), (b if c['ur'].shape[0] > 1 else 0)
    p4 = c['pose4'][b].double().numpy()
    clips = np.array([c['z_min'], *c['ur'][rb].double().tolist(), *c['vr'][rb].double().tolist()])
    return f(c['x2d']), f(c['x3d']), f(c['istd']), c['K'][kb].double().numpy().reshape(9), np.array([0.0, p4[0], 0.0, p4[1], p4[2], p4[3]]), clips


def reference(c, max_iter=50, orc=None, stability=True):
    """The oracle on a case, object by object, as orc_pnp6_refine_batch assembles its outputs: dict(valid (B,) bool, pose (B,6) f32,
    cov (B,6,6) f32, diag (B,2) f32 [iters, why; (0, 0) for an object that never started], n_success, n (inliers), started, cond
    (cond_2 of J^T J at the returned pose; inf where not valid) and, with stability, stable (B,) bool: (iters, why) unchanged when the
    start pose is scaled by 1 +- 1e-9 and when the weights are scaled by 1 + 1e-9)."""
    if orc is None:
        from oracle import oracle as orc
    B = c['x2d'].shape[0]
    out = dict(valid=np.zeros(B, bool), pose=np.zeros((B, 6), np.float32), cov=np.tile(np.eye(6, dtype=np.float32), (B, 1, 1)),
               diag=np.zeros((B, 2), np.float32), n_success=np.zeros(B, int), n=c['mask'].sum(1).numpy().astype(int),
               started=np.zeros(B, bool), cond=np.full(B, np.inf), stable=np.ones(B, bool))
    orc.set_lm_options(max_iter=max_iter)
    try:
        for b in range(B):
            if not int(c['valid4'][b]):
                continue
            u, X, w, K9, init, clips = object_problem(c, b)
            out['pose'][b] = init
            if out['n'][b] == 0:
                continue
            out['started'][b] = True
            r = orc.pnp6_uncert(u, X, w, K9, init, clips)
            out['valid'][b], out['pose'][b], out['diag'][b], out['n_success'][b] = bool(r['val']), r['pose'], (r['iters'], r['why']), r['n_success']
            if r['val']:
                out['cov'][b] = r['cov']
                out['cond'][b] = np.linalg.cond(orc.eval6(u, X, w, K9, r['pose'], clips)[3])
            if stability:
                for i2, w2 in ((init * (1 + 1e-9), w), (init * (1 - 1e-9), w), (init, w * (1 + 1e-9))):
                    r2 = orc.pnp6_uncert(u, X, w2, K9, i2, clips)
                    out['stable'][b] &= (r2['iters'], r2['why']) == (r['iters'], r['why'])
    finally:
        orc.set_lm_options()
    return out


@functools.lru_cache(maxsize=None)
def cached_reference(name, max_iter=50):
    """reference(case(name), max_iter), computed once per test session"""
    return reference(case(name), max_iter)


def expected_diag(want):
    """The kernel's diag for the reference's: an object that never started reports (0, NOT_STARTED) where the oracle leaves (0, 0)."""
    d = want['diag'].copy()
    d[~want['started']] = (0.0, WHY['NOT_STARTED'])
    return d


def check(got, want, what=''):
    """A kernel result against the reference: valid equal, |pose6 - ref| <= POSE_TOL on every object (a non-finite reference entry
    must be non-finite in the same way), |cov6 - ref| <= COV_TOL max|ref cov| on the objects valid in the reference and the exact
    identity elsewhere, diag equal on the stable objects.  Returns the worst err / tol."""
    valid, pose, cov, diag = (t.cpu().numpy() for t in got)
    assert np.array_equal(valid.astype(bool), want['valid']), (what, 'valid', valid.tolist(), want['valid'].tolist())
    fin = np.isfinite(want['pose'])
    assert np.array_equal(pose[~fin], want['pose'][~fin], equal_nan=True), (what, 'non-finite pose entries')
    worst = float(np.abs(pose - want['pose'])[fin].max()) / POSE_TOL if fin.any() else 0.0
    v = want['valid']
    assert np.array_equal(cov[~v], np.tile(np.eye(6, dtype=np.float32), (int((~v).sum()), 1, 1))), (what, 'cov of an invalid object is not the identity')
    if v.any():
        sc = np.abs(want['cov'][v]).reshape(int(v.sum()), -1).max(1)[:, None, None]
        worst = max(worst, float((np.abs(cov[v] - want['cov'][v]) / sc).max()) / COV_TOL)
    s = want['stable']
    assert np.array_equal(diag[s], expected_diag(want)[s]), (what, 'diag on stable objects', diag.tolist(), expected_diag(want).tolist(), s.tolist())
    assert worst <= 1.0, (what, 'worst err / tol', worst)
    return worst
