"""Named, seeded cases for exact_hessian_kernel (csrc/hessian_kernel.inc) beyond the one shape of the G8 fixture (B = 10, P = 96): what
tests/test_gpu_exact_hessian_shapes.py runs on the MI355X and what tests/test_exact_hessian_cases_cpu.py pins about them on the CPU.

Inputs follow the recipe of tests/golden/make_golden_hessian.py (G8), restated here with its constants as parameters, and
monorun_amd.synthetic for the two memory layouts.  A case is a dict of fp64 arrays: x2d (B,P,2), istd (B,P,2), x3d (B,P,3), K (B,3,3),
u_range (B,2), v_range (B,2), yaw (B,1), t (B,3), mask (B,P) bool or None, valid_in (B,) u8, z_min.

The reference of every case is orc.exact_hessian / orc.pose_cov_general on the values the kernel is given: camera, ranges and pose
rounded to float32, the correspondences rounded to the storage type (tests/test_exact_hessian.py feeds them the same way)."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(1, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KITTI_K = np.array([[707.0912, 0.0, 601.8873], [0.0, 707.0912, 183.1104], [0.0, 0.0, 1.0]])
DIMS = np.array([3.89, 1.53, 1.62])
Z_MIN = 0.5
SHAPE_P = (1, 5, 96, 255, 256, 257, 600)          # the lane loop `for (p = tid; p < P; p += 256)`: one, two and three trips, full and ragged
SHAPE_B = (1, 3, 10)
MASKS = ('none', 'ones', 'half', 'single', 'zero', 'zclip', 'enters_invalid')
HESS_BOUND = 3e-7                                  # relative to max |H|: the float32 rounding of the output (tests/test_exact_hessian.py)


def cov_bound(H):
    """tests/test_exact_hessian.py's bound on cov against orc.pose_cov_general(H), relative to max |cov|"""
    return 1e-5 * max(1.0, np.linalg.cond(H) * 1e-7)


def recipe(B, P, seed, depth=(6.0, 40.0), focal=707.0912, spread=1.0, noise=1.5, lateral=8.0, vertical=(1.0, 2.0), border=200.0, offset=(0.0, 0.0)):
    """the G8 recipe: B objects of P points each, evaluated near the generating pose.  depth: range of t_z; focal: fx = fy; spread:
    scale of the object's points; noise: pixel residuals (the second-order term of h); lateral / vertical: range of t_x and t_y;
    border: how far past the image the clip ranges reach; offset: added to every (t_x, t_y)."""
    rng = np.random.default_rng(seed)
    K1 = KITTI_K.copy()
    K1[0, 0] = K1[1, 1] = focal
    yaw = rng.uniform(-np.pi, np.pi, (B, 1))
    t = np.stack([rng.uniform(-lateral, lateral, B), rng.uniform(vertical[0], vertical[1], B), rng.uniform(depth[0], depth[1], B)], 1)
    t[:, 0:2] += offset
    x3d = (rng.uniform(-0.5, 0.5, (B, P, 3)) + np.array([0.0, -0.5, 0.0])) * DIMS * spread
    c, s = np.cos(yaw[:, 0]), np.sin(yaw[:, 0])
    R = np.zeros((B, 3, 3))
    R[:, 0, 0], R[:, 0, 2], R[:, 1, 1], R[:, 2, 0], R[:, 2, 2] = c, s, 1, -s, c
    uvz = np.einsum('ij,bpj->bpi', K1, np.einsum('bij,bpj->bpi', R, x3d) + t[:, None])
    x2d = uvz[..., :2] / uvz[..., 2:] + rng.normal(0, noise, (B, P, 2))
    istd = np.exp(-rng.normal(np.log(2.0), 0.5, (B, P, 2))) / 10.0
    mask = rng.random((B, P)) > 0.25
    yaw_e, t_e = yaw + rng.normal(0, 0.05, (B, 1)), t + rng.normal(0, 0.2, (B, 3))
    return dict(x2d=x2d, istd=istd, x3d=x3d, K=np.repeat(K1[None], B, 0), u_range=np.repeat([[-border, 1242.0 + border]], B, 0),
                v_range=np.repeat([[-border, 375.0 + border]], B, 0), yaw=yaw_e, t=t_e, mask=mask, valid_in=np.ones(B, np.uint8), z_min=Z_MIN)


def stack(cases):
    """several cases of one P as one batch"""
    out = {k: np.concatenate([c[k] for c in cases]) for k in ('x2d', 'istd', 'x3d', 'K', 'u_range', 'v_range', 'yaw', 't', 'mask', 'valid_in')}
    out['z_min'] = Z_MIN
    return out


def take(c, idx):
    """objects idx of a case"""
    idx = np.atleast_1d(idx)
    return {k: (v if k == 'z_min' or v is None else v[idx]) for k, v in c.items()}


# ------------------------------------------------------------------------------- shapes and masks
def shape_case(B, P):
    c = recipe(B, P, seed=1000 * B + P)
    if P == 1:
        c['mask'][:] = True                        # one point: an inlier, or nothing is summed (that is mask kind 'zero')
    return c


def mask_case(kind, B=3, P=257):
    """the mask kinds at a shape with two lane trips, the second of one point"""
    c = recipe(B, P, seed=4242)
    rng = np.random.default_rng(17)
    if kind == 'none':
        c['mask'] = None
    elif kind == 'ones':
        c['mask'][:] = True
    elif kind == 'half':
        c['mask'] = rng.random((B, P)) < 0.5
    elif kind == 'single':
        c['mask'][:] = False
        c['mask'][np.arange(B), [0, 255, 256][:B]] = True        # the first lane's first trip, the last lane's, the second trip
    elif kind == 'zero':
        c['mask'][:] = False
    elif kind == 'zclip':
        c['t'][:, 2] = -5.0                        # every point behind z_min: both rows of every point masked
    elif kind == 'enters_invalid':
        c['valid_in'][1] = 0
    else:
        raise KeyError(kind)
    return c


# ------------------------------------------------------------------------------- pivot paths
def pivot_rows(H):
    """Gauss-Jordan with partial pivoting on [H | I], restated in numpy: the row picked for each column (the first of the largest
    |entries| at or below the diagonal), or -1 from the column on where none is non-zero"""
    M = np.concatenate([np.array(H, np.float64), np.eye(4)], 1)
    rows = []
    for col in range(4):
        piv = col + int(np.argmax(np.abs(M[col:, col])))
        if not np.abs(M[piv, col]) > 0:
            return rows + [-1] * (4 - col)
        rows.append(piv)
        M[[col, piv]] = M[[piv, col]]
        M[col] /= M[col, col]
        for r in range(4):
            if r != col:
                M[r] -= M[r, col] * M[col]
    return rows


def pivot_object(seed):
    """one object of 96 points whose depth, focal length, point spread, offset from the optical axis and residual size are drawn from
    the seed: they move the yaw entries of H against the translation entries, and those against each other (an object further off
    the axis than the focal length, |u - cx| > f, has |H[tz][tx]| > |H[tx][tx]|)"""
    rng = np.random.default_rng(seed)
    z = float(np.exp(rng.uniform(np.log(3.0), np.log(60.0))))
    focal = float(np.exp(rng.uniform(np.log(150.0), np.log(1500.0))))
    spread = float(np.exp(rng.uniform(np.log(0.1), np.log(3.0))))
    tx, ty = z * rng.uniform(-2.0, 2.0), z * rng.uniform(-2.0, 2.0)
    noise = float(rng.choice([0.5, 1.5, 40.0]))
    return recipe(1, 96, seed, depth=(z, z), focal=focal, spread=spread, noise=noise, lateral=0.0, vertical=(0.0, 0.0), border=1e5, offset=(tx, ty))


def singular_object():
    """the G8 object-9 construction: so far to the right that every u row is clipped; t_x is unobservable and h exactly singular"""
    c = recipe(1, 96, seed=909)
    c['t'][0] = [30.0, 1.5, 10.0]
    return c


# seeds of pivot_object found by PIVOT_SEARCH below: per (column, 'self' | 'later'), an object whose pivot row for that column is the
# column itself / a later row; INDEFINITE_SEED: an object whose h has a negative eigenvalue and cond(h) < 1e6
PIVOT_SEEDS = {(0, 'later'): [0, 26], (1, 'later'): [0, 1], (2, 'self'): [0, 1], (0, 'self'): [1, 2], (1, 'self'): [3, 5], (2, 'later'): [3, 5]}
INDEFINITE_SEED = 0


def pivot_seeds():
    return list(dict.fromkeys([s for v in PIVOT_SEEDS.values() for s in v] + [INDEFINITE_SEED]))


def pivots_case():
    """the objects of pivot_seeds(), then the singular one; per-object cameras"""
    seeds = pivot_seeds()
    return stack([pivot_object(s) for s in seeds] + [singular_object()])


def strides_case():
    """per-object cameras and ranges that really differ (K_stride 9, r_stride 2): a skewed camera, one with a general third row, other
    focal lengths, a tight range pair (objects 6, 7 and 8 of G8)"""
    c = recipe(5, 257, seed=777)
    c['K'][1, 0, 1] = 3.0
    c['K'][2, 2] = [1e-4, -2e-4, 1.001]
    c['K'][3, 0, 0], c['K'][3, 1, 1] = 500.0, 520.0
    c['u_range'][4], c['v_range'][4] = [550.0, 700.0], [150.0, 220.0]
    c['t'][4] = [0.5, 1.5, 12.0]
    return c


def layout_batch(planar):
    """monorun_amd.synthetic's correspondences (B = 3, P = 17 x 17 = 289) in the reference's planar views (strides (C P, 1, P)) or as
    contiguous (B, P, C) copies, evaluated at the generating pose"""
    from monorun_amd import synthetic as syn
    b = syn.make_batch(B=3, hw=17, seed=99)
    x2d, istd, x3d, K, ur, vr, _ = syn.pnp_boundary(b, planar=planar)
    pose = np.concatenate([b['gt_yaw'][:, None], b['gt_t']], 1).astype(np.float32)
    return x2d, istd, x3d, K, ur, vr, pose, ~b['outlier'].reshape(3, -1)


# ------------------------------------------------------------------------------- the reference
STORAGE = {'f32': np.float32, 'f16': np.float16, 'f64': np.float64}


def reference(c, storage='f32'):
    """(H (B,4,4) fp64, ok (B,) bool, cov (B,4,4) fp64) from the oracle on the values the kernel is given; an object that enters
    invalid: H = 0, not ok, cov = I"""
    from oracle import oracle as orc
    st = STORAGE[storage]
    r32 = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)
    rs = lambda a: np.asarray(a, np.float64).astype(st).astype(np.float64)
    B = len(c['x2d'])
    H, ok, cov = np.zeros((B, 4, 4)), np.zeros(B, bool), np.repeat(np.eye(4)[None], B, 0)
    for b in range(B):
        if not c['valid_in'][b]:
            continue
        H[b] = orc.exact_hessian(r32(c['K'][b]), c['z_min'], r32(c['u_range'][b]), r32(c['v_range'][b]), float(r32(c['yaw'][b])[0]), r32(c['t'][b]),
                                 rs(c['x2d'][b]), rs(c['x3d'][b]), rs(c['istd'][b]), None if c['mask'] is None else c['mask'][b])
        ok[b], cov[b] = orc.pose_cov_general(H[b])
    return H, ok, cov


CASES = {f'shape_B{B}_P{P}': functools.partial(shape_case, B, P) for P in SHAPE_P for B in SHAPE_B}
CASES.update({f'mask_{k}': functools.partial(mask_case, k) for k in MASKS})
CASES.update(pivots=pivots_case, strides=strides_case)
SHAPE_NAMES = tuple(n for n in CASES if n.startswith('shape_'))
MASK_NAMES = tuple(n for n in CASES if n.startswith('mask_'))


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def expected(name, storage='f32'):
    """computed once per run, shared by the tests, never modified"""
    return reference(case(name), storage)


# ------------------------------------------------------------------------------- the seed search
def PIVOT_SEARCH(tries=4000):
    """prints PIVOT_SEEDS and INDEFINITE_SEED: the first seeds of pivot_object with each pivot row class and an indefinite, regular h
    (the first two of each class; all with cond(h) < 1e6, so that the covariance bound stays the plain 1e-5)"""
    found, indef = {}, None
    for seed in range(tries):
        c = pivot_object(seed)
        H, ok, _ = reference(c)
        if not ok[0] or np.linalg.cond(H[0]) >= 1e6:
            continue
        rows = pivot_rows(H[0])
        for col in range(3):
            got = found.setdefault((col, 'self' if rows[col] == col else 'later'), [])
            if len(got) < 2:
                got.append(seed)
        if indef is None and np.linalg.eigvalsh(0.5 * (H[0] + H[0].T)).min() < 0:
            indef = seed
        if len(found) == 6 and all(len(v) == 2 for v in found.values()) and indef is not None:
            break
    print('PIVOT_SEEDS =', found)
    print('INDEFINITE_SEED =', indef)


if __name__ == '__main__':
    PIVOT_SEARCH()
