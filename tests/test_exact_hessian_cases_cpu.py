"""What the cases of tests/exact_hessian_cases.py claim to exercise, pinned on the CPU against the oracle alone, before
tests/test_gpu_exact_hessian_shapes.py runs them through exact_hessian_kernel."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_hessian_cases as hc  # noqa: E402


def test_shape_cases_cover_the_lane_trips():
    assert hc.SHAPE_P == (1, 5, 96, 255, 256, 257, 600) and hc.SHAPE_B == (1, 3, 10) and len(hc.SHAPE_NAMES) == 21
    assert sorted({-(-P // 256) for P in hc.SHAPE_P}) == [1, 2, 3] and {P % 256 for P in hc.SHAPE_P} >= {0, 1, 255}
    conds = []
    for name in hc.SHAPE_NAMES:
        c = hc.case(name)
        H, ok, cov = hc.expected(name)
        B, P = c['x2d'].shape[:2]
        assert name == f'shape_B{B}_P{P}' and c['mask'].shape == (B, P) and c['mask'].any(1).all()
        # every h is regular, that of a single point too: its two residual rows give J^T J rank 2, the second-order term the rest
        assert ok.all() and np.abs(H).max(axis=(1, 2)).min() > 0, name
        assert not c['mask'].all() or P < 96
        conds.append(max(np.linalg.cond(h) for h in H))
    print('largest cond(h) per shape case:', {n: f'{v:.3g}' for n, v in zip(hc.SHAPE_NAMES, conds)})


def test_mask_cases(orc):
    full = hc.expected('mask_none')
    assert hc.case('mask_none')['mask'] is None and np.array_equal(full[0], hc.expected('mask_ones')[0]) and full[1].all()
    H, ok, _ = hc.expected('mask_half')
    assert ok.all() and not np.array_equal(H, full[0])
    c = hc.case('mask_single')
    assert c['mask'].sum(1).tolist() == [1, 1, 1] and np.nonzero(c['mask'])[1].tolist() == [0, 255, 256]
    H, ok, cov = hc.expected('mask_single')
    assert ok.all() and np.abs(H).max(axis=(1, 2)).min() > 0          # one point: h is summed (and regular: the second-order term)
    print('mask_single cond(h):', [f'{np.linalg.cond(h):.3g}' for h in H])
    for name in ('mask_zero', 'mask_zclip'):                          # nothing summed: h = 0, invalid, cov = I
        H, ok, cov = hc.expected(name)
        assert not H.any() and not ok.any() and np.array_equal(cov, np.repeat(np.eye(4)[None], 3, 0)), name
    c = hc.case('mask_zclip')
    assert c['mask'].any() and np.all(c['t'][:, 2] + np.abs(c['x3d']).sum(-1).max() < hc.Z_MIN)
    H, ok, cov = hc.expected('mask_enters_invalid')
    base = hc.expected('shape_B3_P257')
    assert ok.tolist() == [True, False, True] and not H[1].any() and np.array_equal(cov[1], np.eye(4)) and H[0].any() and H[2].any()
    del base


def test_pivot_census():
    """for each of columns 0, 1 and 2 the case set holds objects whose pivot row is the column itself and objects whose pivot row is a
    later row: the kernel's compare-and-swap pivoting both swaps and does not swap at every column"""
    c = hc.case('pivots')
    H, ok, cov = hc.expected('pivots')
    seeds = hc.pivot_seeds()
    assert len(H) == len(seeds) + 1 and ok[:-1].all() and not ok[-1]
    rows = [hc.pivot_rows(h) for h in H]
    print('pivot rows per object (seeds', seeds, '+ singular):', rows)
    for (col, kind), ss in hc.PIVOT_SEEDS.items():
        for s in ss:
            r = rows[seeds.index(s)][col]
            assert (r == col) if kind == 'self' else (r > col), (col, kind, s, r)
    census = {(col, kind): sum((r[col] == col) if kind == 'self' else (r[col] > col) for r in rows[:-1]) for col in range(3) for kind in ('self', 'later')}
    print('census (objects per column and kind):', census)
    assert min(census.values()) >= 2 and set(hc.PIVOT_SEEDS) == set(census)
    conds = [np.linalg.cond(h) for h in H[:-1]]
    print('cond(h):', [f'{v:.3g}' for v in conds])
    assert max(conds) < 1e6
    # the singular object (G8's object 9): every u row clipped, the t_x row and column exactly zero, no pivot for column 1
    assert not H[-1][1].any() and not H[-1][:, 1].any() and rows[-1][1] == -1 and np.array_equal(cov[-1], np.eye(4))
    # the indefinite, regular one
    hi = H[seeds.index(hc.INDEFINITE_SEED)]
    ev = np.linalg.eigvalsh(0.5 * (hi + hi.T))
    assert ev.min() < 0 < ev.max() and ok[seeds.index(hc.INDEFINITE_SEED)]
    for h, co in zip(H[:-1], cov[:-1]):                                 # the oracle's inverse is one
        assert np.abs(h @ co - np.eye(4)).max() < 1e-8


def test_pivot_rows_restatement():
    assert hc.pivot_rows(np.eye(4)) == [0, 1, 2, 3]
    assert hc.pivot_rows(np.eye(4)[[3, 0, 1, 2]]) == [1, 2, 3, 3]
    assert hc.pivot_rows(np.diag([1.0, 0.0, 1.0, 1.0])) == [0, -1, -1, -1]
    assert hc.pivot_rows([[1, 2, 0, 0], [2, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]) == [1, 1, 2, 3]
    assert hc.pivot_rows([[2, 0, 0, 0], [0, -1, 0, 0], [0, -1, 0, 3], [0, 0, 1, 0]]) == [0, 1, 3, 3]       # ties: the first row


def test_strides_case_differs_per_object():
    c = hc.case('strides')
    assert len(np.unique(c['K'].reshape(5, -1), axis=0)) == 4 and len(np.unique(c['u_range'], axis=0)) == 2
    H, ok, _ = hc.expected('strides')
    assert ok.all()
    shared = dict(c, K=np.repeat(c['K'][:1], 5, 0), u_range=np.repeat(c['u_range'][:1], 5, 0), v_range=np.repeat(c['v_range'][:1], 5, 0))
    Hs = hc.reference(shared)[0]
    assert np.array_equal(H[0], Hs[0]) and all(not np.allclose(H[b], Hs[b], rtol=1e-6) for b in range(1, 5))
    assert np.abs(H[2] - H[2].T).max() > 1e-6 * np.abs(H[2]).max()      # the general third row: h is not symmetric


def test_layouts_hold_the_same_values():
    a, b = hc.layout_batch(True), hc.layout_batch(False)
    for x, y in zip(a[:3], b[:3]):
        assert x.shape == y.shape and x.strides != y.strides and np.array_equal(x, y) and y.flags.c_contiguous and x.dtype == np.float32
    assert a[0].shape == (3, 289, 2) and a[7].shape == (3, 289) and 0 < a[7].sum() < a[7].size


@pytest.mark.parametrize('storage', ['f16', 'f64'])
def test_other_storage_types_change_the_reference(storage):
    H32, H = hc.expected('shape_B3_P257')[0], hc.expected('shape_B3_P257', storage)[0]
    rel = np.abs(H - H32).max() / np.abs(H32).max()
    print(f'{storage} against f32 storage: {rel:.3e}')
    assert 0 < rel < (1e-1 if storage == 'f16' else 1e-4)
