"""CPU side of the wave-count contract (tests/test_gpu_launch_regimes.py is the GPU side): the numpy restatement of the covariance
stage's summation tree against the oracle's, the tree-sensitive corpus whose `valid` flag the wave count decides, and the coverage of
the launch-regime case list."""
import numpy as np

from tests import cov_tree, fuzz_cases
from tests import launch_regimes as lr

WAVES = (1, 2, 3, 4, 8)


def test_numpy_tree_equals_the_oracle_tree():
    rng = np.random.default_rng(3)
    for w in WAVES:
        part = rng.normal(0, 1, (64 * w, 10)) * 10.0 ** rng.integers(-8, 17, (64 * w, 10))
        from oracle import oracle as orc
        assert np.array_equal(cov_tree.tree_sum(part, w).view(np.uint64), orc.tree_sum(part, w).view(np.uint64)), w


def test_numpy_cov_hessian_equals_the_specified_one(orc):
    """cov_tree.cov_hessian (thread q % (64 w), butterfly 32, 16, 1, 2, 4, 8, then wave order) against orc.cov_hessian_spec(waves=w), bit for
    bit, at the oracle's LM pose: tree-sensitive and ordinary objects, P = 300 (every wave count gives a different thread assignment)."""
    from monorun_amd import synthetic as syn
    rng = np.random.default_rng(5)
    tree = fuzz_cases.make_tree_sensitive(rng, 2, 300)
    b = syn.make_batch(B=1, hw=18, seed=9)
    plain = [np.ascontiguousarray(a) for a in syn.pnp_boundary(b, planar=False)]
    plain[:3] = [a[:, :300] for a in plain[:3]]
    for x in (tree, plain):
        with np.errstate(all='ignore'):
            ref = orc.u2d_pnp_epnp(*x[:6], 0.5, 0.6, x[6], True)
        for i in range(x[0].shape[0]):
            yaw, t, inl = float(ref[1][i, 0]), ref[2][i], ref[5][i]
            sn, cs = orc.spec_sincos(yaw)
            K = x[3].reshape(-1, 9)[0]
            for w in WAVES:
                want = orc.cov_hessian_spec(K, 0.5, x[4][0], x[5][0], yaw, t, x[2][i], x[1][i], inl, waves=w)
                got = cov_tree.cov_hessian(K, 0.5, x[4][0], x[5][0], float(sn[0]), float(cs[0]), t, x[2][i], x[1][i], inl, w)
                assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (i, w, got - want)


MIN_TREE_DECIDED = 20        # of 256 tree-sensitive objects (measured: about 45)


def test_corpus_valid_flag_depends_on_the_wave_count(orc):
    """The corpus the GPU regime tests tile (a quarter of their objects): objects whose oracle `valid` flag differs between 1, 2, 4 and 8
    waves per object, with the initialiser succeeding and the LM ending at a finite pose.  Without them a kernel that summed in another
    order than its wave count's would pass the parity tests.  Also counts valid objects whose cov moves by more than 1e-5 relative."""
    rng = np.random.default_rng(2024)
    decided = cov_moved = 0
    for P in (784, 300):
        x = fuzz_cases.make_tree_sensitive(rng, 128, P)
        refs = {}
        for w in (1, 2, 4, 8):
            with np.errstate(all='ignore'):
                refs[w] = orc.u2d_pnp_epnp(*x[:6], 0.5, 0.6, x[6], True, num_threads=0, return_diag=True, cov_waves=w)
        vs = np.array([refs[w][0] for w in (1, 2, 4, 8)])
        d = (vs != vs[:1]).any(0)
        r = refs[4]
        normal = (r[6][:, 2] != 8) & np.isfinite(r[1][:, 0]) & np.isfinite(r[2]).all(1)
        for w in (1, 2, 8):                             # the pose does not depend on the covariance stage
            assert np.array_equal(refs[w][1], r[1]) and np.array_equal(refs[w][2], r[2])
        decided += int((d & normal).sum())
        ok = vs.all(0)
        for w in (1, 2, 8):
            c, c4 = refs[w][3][ok].astype(np.float64), r[3][ok].astype(np.float64)
            sc = np.abs(c4).reshape(int(ok.sum()), -1).max(1)[:, None, None]
            cov_moved += int(((np.abs(c - c4) / sc) > 1e-5).any((1, 2)).sum())
    print(f'tree-decided valid flags: {decided} of 256; valid objects with cov moved > 1e-5: {cov_moved}')
    assert decided >= MIN_TREE_DECIDED, decided


def test_regime_case_list_covers_every_boundary_and_choice():
    cases = lr.cases()
    epnp = [c for c in cases if c[0] == 'epnp']
    Bs = {c[1] for c in epnp if c[2] == 784 and c[3] == 'fp32'}
    for b in lr.B_BOUNDARIES:
        assert b in Bs and b + 1 in Bs, b
        assert lr.regime(b, 1, 784, 'fp32') != lr.regime(b + 1, 1, 784, 'fp32') or b == 4096, b      # 4096 / 4097: P = 300 below
    Ps = {c[2] for c in epnp}
    for p in lr.P_BOUNDARIES:
        assert p in Ps and p + 1 in Ps, p
    for b in (2048, 4096):                                          # the wave count's object boundaries, at P = 300
        assert lr.regime(b, 1, 300, 'fp32', flow='k0') != lr.regime(b + 1, 1, 300, 'fp32', flow='k0')
    seen = {}
    for flow, B, P, dt, layout in cases:
        for k, v in lr.regime(B, 1, P, dt, flow=flow).items():
            for e in (v if isinstance(v, tuple) else (v,)):
                seen.setdefault((flow, k), set()).add(e)
    assert seen[('epnp', 'first')] == {10, 3}
    assert seen[('epnp', 'round2')] == {'one', 'two'}
    assert seen[('epnp', 'lv_h')] == {4, 2, 0} and seen[('epnp', 'lv_b')] == {4, 2, 0}
    assert seen[('epnp', 'wpo')] == {2, 4, 8}                     # the default flow's LM launch has no one-wave form
    assert seen[('k0', 'wpo')] >= {1, 2, 4}
    assert {c[3] for c in cases} == {'fp16', 'fp32', 'fp64'} and {c[4] for c in cases} == {'planar', 'contiguous'}
    assert any(c[2] % 4 for c in epnp)                              # P not a multiple of 4: the byte-store mask path
    # the rule as the issue's table states it (MI355X, 256 CUs)
    assert [lr.lm_waves(B, 300, 'fp32') for B in (2048, 2049, 4096, 4097)] == [4, 2, 2, 2]
    assert [lr.lm_waves(B, 300, 'fp32', after_init=False) for B in (2048, 2049, 4096, 4097)] == [4, 2, 2, 1]
    assert [lr.lm_waves(64, P, 'fp32', after_init=False) for P in (127, 128, 255, 256)] == [1, 2, 2, 4]
    assert lr.lm_waves(64, 3136, 'fp16') == 8 and lr.lm_waves(64, 3136, 'fp32') == 8 and lr.lm_waves(64, 3136, 'fp64') == 4
    assert lr.epnp_regime(2047)['round2'] == 'one' and lr.epnp_regime(2048) == dict(first=3, round2='two', lv_h=(0, 0), lv_b=0)
