"""The backward of ``pnp_uncert`` (``mr_pnp_uncert_backward_batched``) away from the one recipe tests/test_gpu_pnp_grad.py draws from:
ragged point counts, the three input layouts, per-object cameras and clip ranges, a camera with a general third row, every optional
pointer, status 1 / 2 objects and non-finite inputs.  Cases come from tests/pnp_grad_cases.py (no forward solve); the yardstick is the
fp64 autodiff reference tests/pnp_grad_ref.py under the metric and TOL of tests/test_gpu_pnp_grad.py, plus bit-identity between calls
that must not differ.  Each test prints the worst err / TOL it saw."""
import itertools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_grad_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu

LM = [False, True]
NAN = float('nan')
INF = float('inf')


def _sentinel(case, needs=(True, True, True)):
    B, P = case['x2d'].shape[:2]
    return [torch.full((B, P, c), NAN, device=pc.device()) if n else None for n, c in zip(needs, (2, 2, 3))]


@pytest.mark.parametrize('lm_all', LM)
@pytest.mark.parametrize('P', [5, 8, 63, 64, 65, 255, 256, 257, 1000])
def test_ragged_point_counts(P, lm_all):
    """P below, at and above the 256 lanes of a workgroup: parity, every one of the B * P rows written (NaN sentinel in the output
    buffers), exact zeros at the points outside both sets, and two calls bit-identical."""
    key = (9, P, P + 1)
    c = pc.make_case(*key)
    out = _sentinel(c)
    got, worst = pc.check(c, lm_all, want=pc.cached_reference(lm_all, *key), out=out)
    print(f'ragged P={P} lm_all={lm_all}: worst err / TOL = {worst:.3g}')
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got[:3], out))
    assert not any(bool(torch.isnan(g).any()) for g in got[:3]), 'a row of an output buffer was not written'
    assert pc.same(got, pc.run(c, lm_all))                                   # fresh allocations, second call
    if not lm_all:
        outside = c['mask'] == 0
        assert int(outside.sum()) > 0 or P < 8
        assert all(pc.all_zero_bits(g[outside]) for g in got[:3])
    else:                                                                    # every point is in S_LM: nothing is left at zero
        assert bool((got[0].abs().amax(2) > 0).all())


def _planar(t):
    return t.transpose(1, 2).contiguous().transpose(1, 2)                    # strides (C * P, 1, P)


def _strided(t):
    """the same values as rows of a wider tensor: strides (.., 2 (C + 3), 1), a storage offset, NaN in everything the view skips"""
    B, P, C = t.shape
    wide = torch.full((B, 2 * P + 1, C + 3), NAN, dtype=t.dtype, device=t.device)
    v = wide[:, 1::2, 1:1 + C]
    v.copy_(t)
    return v


@pytest.mark.parametrize('lm_all', LM)
@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.float64])
def test_layouts(dtype, lm_all):
    """(B,P,C) contiguous, channel-planar and a generic strided view, uniform and mixed within one call: bit-identical gradients, one
    of them checked against the reference.  f16 storage widens exactly: equal to the f32 run on the f16-rounded values."""
    key = (8, 300, 1, 'shared', 'shared', dtype)
    c = pc.make_case(*key)
    base, worst = pc.check(c, lm_all, want=pc.cached_reference(lm_all, *key))
    print(f'layouts {dtype} lm_all={lm_all}: worst err / TOL = {worst:.3g}')
    forms = {'contiguous': lambda t: t, 'planar': _planar, 'strided': _strided}
    for combo in [('planar',) * 3, ('strided',) * 3, ('contiguous', 'planar', 'strided'), ('strided', 'contiguous', 'planar'),
                  ('planar', 'strided', 'contiguous')]:
        v = dict(c, **{k: forms[f](c[k]) for k, f in zip(('x2d', 'istd', 'x3d'), combo)})
        assert all(torch.equal(v[k], c[k]) for k in ('x2d', 'istd', 'x3d'))
        assert v['x2d'].is_contiguous() == (combo[0] == 'contiguous') and (combo[0] != 'strided' or v['x2d'].storage_offset() > 0)
        assert pc.same(pc.run(v, lm_all), base), combo
    if dtype == torch.float16:
        f32 = dict(c, x2d=c['x2d'].float(), istd=c['istd'].float(), x3d=c['x3d'].float())
        assert pc.same(pc.run(f32, lm_all), base)


@pytest.mark.parametrize('lm_all', LM)
@pytest.mark.parametrize('cam,ranges', [('per_object', 'per_object'), ('shared', 'per_object'), ('per_object', 'shared'),
                                        ('general', 'per_object'), ('general', 'shared')])
def test_per_object_cameras_and_ranges(cam, ranges, lm_all):
    """K (B,3,3) and u / v ranges (B,2), also with a general third row of K: parity, the rows the tightened ranges clip are the ones
    constructed, and object b of the batch is bit-identical to a B = 1 call on object b with its own camera and range."""
    key = (9, 100, 2, cam, ranges)
    c = pc.make_case(*key)
    B = 9
    assert c['K'].shape[0] == (1 if cam == 'shared' else B) and c['ur'].shape[0] == c['vr'].shape[0] == (1 if ranges == 'shared' else B)
    got, worst = pc.check(c, lm_all, want=pc.cached_reference(lm_all, *key))
    print(f'cameras {cam} ranges {ranges} lm_all={lm_all}: worst err / TOL = {worst:.3g}')
    if cam == 'general':
        assert float(c['K'][:, 2, :2].abs().min()) > 0 and float((c['K'][:, 2, 2] - 1).abs().min()) > 0
    if ranges == 'per_object':
        # the reference's frozen row masks are the constructed ones: nothing else is clipped, and only in the tightened objects
        d = dict(dtype=torch.float64)
        m_lm, _ = pc.ref.row_masks(c['x2d'].to(**d), c['x3d'].to(**d), c['K'].to(**d).expand(B, 3, 3), c['ur'].to(**d), c['vr'].to(**d), pc.Z_MIN,
                                   c['pose'].to(**d), c['mask'].bool(), True)
        assert torch.equal(m_lm == 0, c['clipped'])
        n = c['clipped'].sum((1, 2)).tolist()
        assert all((k > 0.05 * 100) == (o % 3 != 0) for o, k in enumerate(n)), n
        # a clipped row is in neither set: its grad_x2d and grad_istd entries are exactly zero, the kept rows' are not
        assert pc.all_zero_bits(got[0][c['clipped']]) and pc.all_zero_bits(got[1][c['clipped']])
        kept = ~c['clipped'] & (c['mask'].bool()[..., None] | lm_all)
        assert bool((got[0][kept] != 0).all())
    for o in range(B):
        one = pc.run(pc.sub(c, [o]), lm_all)
        assert all(torch.equal(a[0], g[o]) for a, g in zip(one, got)), o


@pytest.mark.parametrize('lm_all', LM)
def test_optional_pointers(lm_all):
    """inlier_mask / grad_pose / cov NULL, and each of grad_x2d / grad_istd / grad_x3d on its own."""
    c = pc.make_case(8, 65, 3, 'per_object')
    full, worst = pc.check(c, lm_all)
    # no mask = every point an inlier
    ones = dict(c, mask=torch.ones_like(c['mask']))
    nomask, w = pc.check(dict(c, mask=None), lm_all)
    worst = max(worst, w)
    assert pc.same(nomask, pc.run(ones, lm_all))
    # the 7 non-empty subsets of the outputs
    for needs in itertools.product([False, True], repeat=3):
        if not any(needs):
            continue
        out = _sentinel(c, needs)
        part = pc.run(c, lm_all, needs=needs, out=out)
        for g, f, n in zip(part[:3], full[:3], needs):
            assert (g is None) if not n else torch.equal(g, f), needs
        assert torch.equal(part[3], full[3])
    # no grad_pose with a covariance term = a zero grad_pose
    nogp, w = pc.check(dict(c, gp=None), lm_all)
    worst = max(worst, w)
    assert pc.same(nogp, pc.run(dict(c, gp=torch.zeros_like(c['gp'])), lm_all))
    assert not pc.same(nogp, full)
    # grad_pose only
    nocov, w = pc.check(dict(c, cov=None, gc=None), lm_all)
    worst = max(worst, w)
    assert not pc.same(nocov, full)
    print(f'optional pointers lm_all={lm_all}: worst err / TOL = {worst:.3g}')


@pytest.mark.parametrize('inlier_opt_only', [True, False])
def test_autograd_single_leaf(inlier_opt_only):
    """pnp_uncert(..., differentiable=True) with one leaf requiring grad: that leaf's gradient is the all-leaves run's."""
    from monorun_amd.ops import pnp_uncert
    from test_gpu_pnp_grad import _inputs, _losses
    B = 16
    x2d, istd, x3d, K, ur, vr, thr = _inputs(B, seed=31)
    gp, gc = (g.float() for g in _losses(B, seed=5))

    def grads(req):
        leaves = [a.clone().requires_grad_(r) for a, r in zip((x2d, istd, x3d), req)]
        out = pnp_uncert(*leaves, K, ur, vr, z_min=0.5, epnp_istd_thres=0.6, epnp_ransac_thres=thr, inlier_opt_only=inlier_opt_only,
                         initialiser='k0', differentiable=True)
        L = (out[1] * gp[:, :1]).sum() + (out[2] * gp[:, 1:]).sum() + (out[3] * gc).sum()
        g = torch.autograd.grad(L, [a for a, r in zip(leaves, req) if r])
        it = iter(g)
        return [next(it) if r else None for r in req], out
    every, out = grads((True, True, True))
    assert int(out[0].sum()) >= 12 and all(float(g.abs().max()) > 0 for g in every)
    for i in range(3):
        req = tuple(j == i for j in range(3))
        single, o = grads(req)
        assert all(torch.equal(a, b) for a, b in zip(o, out))
        assert torch.equal(single[i], every[i]) and all(single[j] is None for j in range(3) if j != i)


@pytest.mark.parametrize('lm_all', LM)
@pytest.mark.parametrize('P', [65, 257])
def test_status_and_zero_gradients(P, lm_all):
    """Objects without a solution: an empty inlier set (status 2 when S_LM is the inlier set), every row clipped by depth or by range
    (status 2), not valid on entry (status 1).  All get +0.0 in every gradient; their neighbours do not notice them."""
    c = pc.make_case(10, P, 4, 'shared', 'per_object')
    clean, worst = pc.check(c, lm_all)
    assert clean[3].tolist() == [0] * 10
    d = dict(c, **{k: c[k].clone() for k in ('mask', 'pose', 'ur', 'vr', 'valid')})
    d['mask'][1] = 0                                   # H_F = 0 exactly unless the LM set is every point
    d['pose'][3, 3] = -10.0                            # every point behind z_min
    d['ur'][5] = torch.tensor([1e6, 2e6])              # no u row and
    d['vr'][5] = torch.tensor([-2e6, -1e6])            # no v row in range
    d['valid'][7] = 0
    out = _sentinel(d)
    got, w = pc.check(d, lm_all, out=out)
    worst = max(worst, w)
    print(f'status P={P} lm_all={lm_all}: worst err / TOL = {worst:.3g}')
    assert got[3].tolist() == [0, 0 if lm_all else 2, 0, 2, 0, 2, 0, 1, 0, 0]
    dead = [o for o in range(10) if got[3][o] != 0]
    for g in got[:3]:
        assert torch.equal(g[dead], torch.zeros_like(g[dead])) and pc.all_zero_bits(g[dead])
    near = [0, 2, 4, 6, 8, 9]
    assert pc.same(got, clean, near)
    # ... nor a batch that never held them
    alone = pc.run(pc.sub(c, near), lm_all)
    assert all(torch.equal(a, g[near]) for a, g in zip(alone, clean))
    if lm_all:                                         # the empty inlier set under lm_all: S_cov is empty, the pose term is all there is
        nocov = pc.run(dict(d, cov=None, gc=None), lm_all)
        assert all(torch.equal(a[1], b[1]) for a, b in zip(nocov, got))


def _cpu(case):
    return {k: (v.cpu() if v is not None else None) for k, v in case.items()}


@pytest.mark.parametrize('lm_all', LM)
def test_non_finite_inputs(lm_all):
    """NaN / Inf in an inlier point of object 2, or in its covariance: status 2 and +0.0 gradients for that object (as the reference
    says, run on the host), every other object bit-identical to the clean run.  A NaN at a point in neither set changes nothing."""
    c = pc.make_case(8, 65, 5)
    clean, worst = pc.check(c, lm_all)
    print(f'non-finite lm_all={lm_all}: worst err / TOL (clean run) = {worst:.3g}')
    assert clean[3].tolist() == [0] * 8 and bool(c['mask'][2, 1])
    others = [0, 1, 3, 4, 5, 6, 7]
    poisons = [('x2d', (2, 1, 0), NAN), ('x2d', (2, 1, 1), INF), ('x2d', (2, 1, 0), -INF), ('istd', (2, 1, 1), NAN), ('istd', (2, 1, 0), INF),
               ('x3d', (2, 1, 0), NAN), ('x3d', (2, 1, 2), NAN), ('x3d', (2, 1, 1), INF), ('cov', (2, 1, 2), NAN), ('cov', (2, 0, 0), INF)]
    for name, at, value in poisons:
        d = dict(c, **{name: c[name].clone()})
        d[name][at] = value
        got = pc.run(d, lm_all, out=_sentinel(d))
        want_status = pc.reference(_cpu(d), lm_all)[3]
        assert want_status.tolist() == [0, 0, 2, 0, 0, 0, 0, 0], (name, at, value)
        assert torch.equal(got[3].cpu(), want_status), (name, at, value, got[3].tolist())
        assert all(pc.all_zero_bits(g[2]) for g in got[:3]), (name, at, value)
        assert pc.same(got, clean, others), (name, at, value)
    if not lm_all:
        p = int((c['mask'][2] == 0).nonzero()[0])
        for name in ('x2d', 'istd', 'x3d'):
            d = dict(c, **{name: c[name].clone()})
            d[name][2, p] = NAN
            assert pc.same(pc.run(d, lm_all), clean), name
