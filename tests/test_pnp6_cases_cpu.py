"""The cases of tests/pnp6_cases.py do what they claim, shown with the oracle alone (no GPU): general rotations end away from the
yaw-only start, the small-angle start takes the first-order branch, the clamp cases have zeroed Jacobian rows and entries at the
optimum, the exits reached cover FUNCTION, MAXITER and GRADIENT / PARAMETER, a far start has a rejected step, at least 90 % of the
objects of every case are stable, and every reference solve used for parity has enough inliers.  The figures are printed."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp6_cases as pc  # noqa: E402

PARITY = [n for n in pc.CASES if n != 'rank']          # 'rank' is the base of the rank-deficient masks: compared as it stands, too
GENERAL = [n for n, k in pc.CASES.items() if (k[3] if len(k) > 3 else 'general') == 'general']
CLAMP = [n for n, k in pc.CASES.items() if len(k) > 8 and k[8]]


def _refs():
    return [(n, 50) for n in pc.CASES] + [('maxit', m) for m in pc.MAXIT]


def test_reference_equals_the_batch_oracle_on_f32_contiguous_cases(orc):
    """reference() assembles its outputs as orc_pnp6_refine_batch does: exactly equal where that driver applies (fp32, contiguous)."""
    for name in ('general_far', 'cam_clamp', 'ragged_65'):
        c, w = pc.case(name), pc.cached_reference(name)
        assert c['x2d'].dtype == torch.float32 and c['x2d'].is_contiguous()
        n = lambda k: c[k].numpy()
        # (the batch driver takes z_min as an argument and the ranges per object or shared, like the kernel)
        rv, rp, rc, rd = orc.pnp6_refine(n('x2d'), n('istd'), n('x3d'), n('K'), n('ur'), n('vr'), n('mask'), n('pose4'), n('valid4'), z_min=c['z_min'])
        assert np.array_equal(rv, w['valid']) and np.array_equal(rp, w['pose']) and np.array_equal(rc, w['cov']) and np.array_equal(rd, w['diag'])
    # ... also for the objects that do not start: valid4 = 0 (zeros) and an empty mask (the start pose), both with diag (0, 0)
    c = pc.case('edge')
    d = dict(c, mask=c['mask'].clone(), valid4=c['valid4'].clone())
    d['mask'][1] = 0
    d['valid4'][3] = 0
    w = pc.reference(d)
    n = lambda k: d[k].numpy()
    rv, rp, rc, rd = orc.pnp6_refine(n('x2d'), n('istd'), n('x3d'), n('K'), n('ur'), n('vr'), n('mask'), n('pose4'), n('valid4'), z_min=d['z_min'])
    assert np.array_equal(rv, w['valid']) and np.array_equal(rp, w['pose']) and np.array_equal(rc, w['cov']) and np.array_equal(rd, w['diag'])
    p4 = d['pose4'][1].numpy()
    assert not w['valid'][1] and np.array_equal(w['pose'][1], [0, p4[0], 0, p4[1], p4[2], p4[3]]) and not w['pose'][3].any()
    assert w['started'].tolist() == [True, False, True, False] + [True] * 4 and not w['diag'][[1, 3]].any()


def test_general_rotations_leave_the_yaw_only_start(orc):
    for name in GENERAL:
        c, w = pc.case(name), pc.cached_reference(name)
        assert w['valid'].all()
        rxz = np.abs(w['pose'][:, [0, 2]]).min(1)
        start = np.zeros((len(rxz), 3)); start[:, 1] = c['pose4'][:, 0].numpy()
        moved = np.array([np.linalg.norm(pc.rodrigues(a) @ pc.rodrigues(b).T - np.eye(3)) / np.sqrt(2) for a, b in zip(w['pose'][:, :3].astype(float), start)])
        print(f'{name}: min(|rx|, |rz|) at the optimum in [{rxz.min():.3f}, {rxz.max():.3f}], rotation moved by >= {2 * np.arcsin(moved.min() / 2):.3f} rad')
        assert rxz.min() >= 0.1 and 2 * np.arcsin(moved.min() / 2) > 0.1
    w = pc.cached_reference('yaw_near')
    assert np.abs(w['pose'][:, [0, 2]]).max() <= 0.05               # the control: the old regime


def test_small_angle_start_takes_the_first_order_branch(orc):
    c = pc.case('small_angle')
    assert not c['pose4'][:, 0].any() and np.allclose(np.linalg.norm(c['gt'][:, :3], axis=1), 0.2)
    assert np.abs(c['gt'][:, :3]).min() > 0.05                       # a general axis
    for b in range(c['x2d'].shape[0]):
        u, X, w, K9, init, clips = pc.object_problem(c, b)
        assert not init[:3].any()                                    # |r|^2 = 0 <= eps: AngleAxisRotatePoint's first-order branch
        ok, _, _, _, _, jac = orc.eval6(u, X, w, K9, init, clips)
        assert ok
        for k in range(6):
            e = np.zeros(6); e[k] = 1e-6
            fd = (orc.eval6(u, X, w, K9, init + e, clips)[4] - orc.eval6(u, X, w, K9, init - e, clips)[4]) / 2e-6
            assert np.abs(fd - jac[:, :, k]).max() <= 2e-5 * max(1.0, np.abs(jac[:, :, k]).max()), (b, k)
    r = pc.cached_reference('small_angle')
    assert r['valid'].all() and np.abs(r['pose'][:, :3] - c['gt'][:, :3]).max() <= 0.05


def test_clamp_cases_have_zeroed_rows_at_the_optimum(orc):
    for name in CLAMP:
        c, r = pc.case(name), pc.cached_reference(name)
        counts = []
        for b in range(c['x2d'].shape[0]):
            u, X, w, K9, _, clips = pc.object_problem(c, b)
            jac = orc.eval6(u, X, w, K9, r['pose'][b].astype(float), clips)[5]
            urow, vrow = ~jac[:, 0].any(1), ~jac[:, 1].any(1)
            # a z-clamped point keeps its x / y columns and loses the z one (a u- or v-clamped row has lost all six)
            zcol = (jac[:, 0, 5] == 0) & (jac[:, 0, 3] != 0) | (jac[:, 1, 5] == 0) & (jac[:, 1, 4] != 0)
            counts.append((int(urow.sum()), int(vrow.sum()), int(zcol.sum())))
            assert urow.sum() >= 1 and vrow.sum() >= 1 and zcol.sum() >= 1, (name, b, counts[-1])
            assert urow.sum() < 0.3 * len(u) and vrow.sum() < 0.3 * len(u)
        print(f'{name}: (zero u rows, zero v rows, zero z entries) per object = {counts}')


def test_exit_reasons_and_rejected_steps(orc):
    why = {}
    for name, m in _refs():
        r = pc.cached_reference(name, m)
        for v in np.unique(r['diag'][r['started'], 1]).astype(int):
            why.setdefault(int(v), []).append(name if m == 50 else f'{name}@{m}')
    names = {v: k for k, v in pc.WHY.items()}
    print('exit reasons reached:', {names[k]: len(v) for k, v in sorted(why.items())})
    assert pc.WHY['FUNCTION'] in why and pc.WHY['MAXITER'] in why and (pc.WHY['GRADIENT'] in why or pc.WHY['PARAMETER'] in why)
    # the noise-free fp64 case is where GRADIENT comes from
    assert 'exact' in why.get(pc.WHY['GRADIENT'], []) or 'exact' in why.get(pc.WHY['PARAMETER'], [])
    for m in (1, 2):
        r = pc.cached_reference('maxit', m)
        assert (r['diag'][:, 1] == pc.WHY['MAXITER']).all() and (r['diag'][:, 0] == m).all() and r['valid'].all()
    # a rejected step: a pass that neither succeeded nor was the tolerance exit (PARAMETER / FUNCTION leave inside their last pass)
    rej = {}
    for name in ('general_far', 'maxit'):
        r = pc.cached_reference(name)
        rej[name] = (r['diag'][:, 0] - r['n_success'] - np.isin(r['diag'][:, 1], (pc.WHY['PARAMETER'], pc.WHY['FUNCTION']))).astype(int).tolist()
    print('rejected steps per object:', rej)
    assert max(rej['maxit']) >= 1                                    # the far start that has one; general_far is printed for the record


def test_stability_and_conditioning(orc):
    worst_cond, shares = 0.0, {}
    for name, m in _refs():
        r = pc.cached_reference(name, m)
        shares[name if m == 50 else f'{name}@{m}'] = float(r['stable'].mean())
        assert r['stable'].mean() >= 0.9, (name, m, r['stable'].tolist())
        P = pc.case(name)['x2d'].shape[1]
        assert (r['n'] >= min(6, P)).all() and r['started'].all() and r['valid'].all(), name
        worst_cond = max(worst_cond, float(r['cond'].max()))
    print('stable share per case:', {k: round(v, 2) for k, v in shares.items()})
    print(f'largest cond_2(J^T J) of a reference solve: {worst_cond:.3g}')
    assert worst_cond <= 1e8                            # the pose tolerance is not a statement about a direction the data leave open


def test_rank_deficient_masks_are_invalid_in_the_reference_for_one_and_two_inliers(orc):
    d = pc.rank_deficient(pc.case('rank'))
    r = pc.reference(d, stability=False)
    assert r['n'][:5].tolist() == [1, 2, 3, 4, 5] and not r['valid'][:2].any()
    print('rank-deficient inlier sets: reference valid =', r['valid'][:5].tolist(), 'why =', r['diag'][:5, 1].astype(int).tolist())
    for b in range(2):                                              # 2n residuals: rank(J^T J) <= 4 < 6
        u, X, w, K9, _, clips = pc.object_problem(d, b)
        H = orc.eval6(u, X, w, K9, r['pose'][b].astype(float), clips)[3]
        assert np.linalg.matrix_rank(H, tol=1e-9 * np.abs(H).max()) <= 2 * (b + 1)
