"""The LM launch that carries the re-fit (pnp_uncert_refit_kernel) takes the re-fit's point list, its bit row and the prologue's inputs from the
consensus launch's workspace instead of rebuilding the list from init_mask's bytes (csrc/pnp_kernel_body.inc, MR_K1_REFIT; the rows are written in
csrc/epnp_consensus_body.inc).  Every case runs the fused form against the un-fused path (mr_epnp_ransac_batched with its epnp_refit_kernel, then
mr_pnp_uncert_from_init_batched: PnPEpnpLaunch(fused=False)), which must agree bit for bit in every output and hand-over tensor, and against the
oracle at the launch's own wave count under the rules of tests/test_gpu_launch_regimes.check_against_oracle."""
import numpy as np
import pytest
import torch

from tests import test_gpu_launch_regimes as base

pytestmark = pytest.mark.gpu

KW = base.KW
N = base.N_DISTINCT
B_EDGE = 37


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def lib():
    from monorun_amd import _lib
    return _lib.load()


def _run(x, fused, **kw):
    from monorun_amd import PnPEpnpLaunch
    l = PnPEpnpLaunch(*x[:6], epnp_ransac_thres=x[6], with_diag=True, fused=fused, **dict(KW, **kw))
    l.run()
    return base._outputs(l)               # valid, pose, cov, tr, mask, diag, init_pose, init_mask, init_valid, init_diag


def _differing(a, b):
    names = ('valid', 'pose', 'cov', 'tr', 'mask', 'diag', 'init_pose', 'init_mask', 'init_valid', 'init_diag')
    return [n for n, x, y in zip(names, a, b) if not base._bytes_equal([x], [y])]


def _check_oracle(ref, idx, out, what):
    o = [t.numpy() for t in out]
    base.check_against_oracle(ref, idx, o[0], o[1], o[2].reshape(len(idx), 4, 4), o[4], o[5], o[6], o[8], what=what)


def _check_init_mask(out, what):
    """Caller-visible init_mask: for objects with a re-fit, init_mask != 0 is exactly the inlier mask the LM reports (inlier_opt_only)."""
    iv = out[8].numpy().astype(bool)
    assert np.array_equal(out[7].numpy()[iv] != 0, out[4].numpy()[iv] != 0), (what, 'init_mask is the final inlier mask')


# ---- P at the chunk edges -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('P', [5, 63, 64, 65, 127, 128, 129, 784])
def test_p_at_the_chunk_edges(dev, lib, orc, P):
    x, idx = base.inputs(dev, P, 'fp32', B_EDGE, 'planar')
    fused, plain = _run(x, True), _run(x, False)
    assert not _differing(fused, plain), (P, _differing(fused, plain))
    _check_init_mask(fused, P)
    _check_oracle(base.oracle(orc, P, 'fp32', base._query(lib, B_EDGE, P, 'fp32')), idx, fused, ('P', P))


# ---- constructed inlier sets and objects without a re-fit record, inside a batch of ordinary ones ------------------------------------------

P_SET = 130                                # three chunks, the last one of two points
ALL_IN, FIVE, EMPTY_TAIL, FEW_CAND, NO_MODEL = 3, 7, 11, 15, 19
FIVE_AT = (1, 40, 77, 100, 129)
_SETS = {}


def _constructed():
    """B_EDGE objects of P_SET points: ordinary ones of the distinct set, five of them rewritten —
    ALL_IN: uniform weights and a threshold no point misses: every point is a candidate and an inlier (n_fit = P);
    FIVE: five points carry the weight (the others 1 % of it): exactly five candidates, cv2's five-point shortcut, a list of five;
    EMPTY_TAIL: the first 100 points are the candidates and all of them inliers: the last chunk (points 128, 129) has no entry;
    FEW_CAND: three candidates: not more than four, so every point is one (pnp_uncert_cpu.py:23-32) and the list has P entries.  (EP_MODE_FAIL — fewer than
        four candidates AFTER that rule — needs P < 4, which the C ABI rejects: no call reaches it);
    NO_MODEL: image points unrelated to the object and a threshold of 1e-3 px: no model reaches five inliers, no re-fit record."""
    if 'x' not in _SETS:
        d = base.distinct(P_SET, 'fp32')
        x2d, istd, x3d = (np.array(a[:B_EDGE]) for a in d[:3])
        thr = np.array(d[6][:B_EDGE])

        def weights(b, at):
            istd[b] = 0.01
            istd[b, list(at)] = 1.0
        istd[ALL_IN] = 1.0; thr[ALL_IN] = 1e4
        weights(FIVE, FIVE_AT)
        weights(EMPTY_TAIL, range(100)); thr[EMPTY_TAIL] = 1e4
        weights(FEW_CAND, (2, 64, 129))
        rng = np.random.default_rng(515)
        istd[NO_MODEL] = 1.0; thr[NO_MODEL] = 1e-3
        x2d[NO_MODEL] = rng.uniform(0.0, 300.0, size=x2d[NO_MODEL].shape).astype(np.float32)
        _SETS['x'] = [x2d, istd, x3d, d[3], d[4], d[5], thr]
    return _SETS['x']


def _constructed_oracle(orc, waves, thr=True):
    key = ('ref', waves, thr)
    if key not in _SETS:
        x = _constructed()
        with np.errstate(all='ignore'):
            _SETS[key] = orc.u2d_pnp_epnp(*x[:6], 0.5, 0.6, x[6] if thr else None, True, num_threads=0, return_diag=True, return_init=True, cov_waves=waves)
    return _SETS[key]


def _constructed_device(dev, thr=True):
    x = _constructed()
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in x[:6]] + [torch.from_numpy(x[6]).to(dev) if thr else None]


def test_inlier_sets_and_objects_without_a_refit_record(dev, lib, orc):
    x = _constructed_device(dev)
    fused, plain = _run(x, True), _run(x, False)
    assert not _differing(fused, plain), _differing(fused, plain)
    init_mask, init_valid, mask = fused[7].numpy() != 0, fused[8].numpy().astype(bool), fused[4].numpy() != 0
    # the cases are what they claim to be
    assert init_valid[ALL_IN] and init_mask[ALL_IN].all()
    assert init_valid[FIVE] and np.array_equal(np.flatnonzero(init_mask[FIVE]), FIVE_AT)
    assert init_valid[EMPTY_TAIL] and np.array_equal(np.flatnonzero(init_mask[EMPTY_TAIL]), np.arange(100))
    assert fused[9].numpy()[FEW_CAND, 2] == P_SET and not init_valid[NO_MODEL]         # init_diag[:, 2]: the candidates
    assert init_valid.sum() == B_EDGE - 1, 'the ordinary objects around it have a re-fit'
    # the byte path of the object without a record: the mask the LM reports is init_mask's, the pose is the failure's
    assert np.array_equal(mask[NO_MODEL], init_mask[NO_MODEL]) and not fused[0].numpy()[NO_MODEL] and not fused[1].numpy()[NO_MODEL].any()
    _check_init_mask(fused, 'constructed')
    idx = np.arange(B_EDGE)
    _check_oracle(_constructed_oracle(orc, base._query(lib, B_EDGE, P_SET, 'fp32')), idx, fused, 'constructed')


def test_plain_mode(dev, lib, orc):
    """No thresholds: cv2.solvePnP on the candidates — the list is the candidate list, its bit row is built from it."""
    x = _constructed_device(dev, thr=False)
    fused, plain = _run(x, True), _run(x, False)
    assert not _differing(fused, plain), _differing(fused, plain)
    init_mask, init_valid = fused[7].numpy() != 0, fused[8].numpy().astype(bool)
    assert init_mask[FEW_CAND].all() and init_valid[FIVE] and np.array_equal(np.flatnonzero(init_mask[FIVE]), FIVE_AT)
    assert np.array_equal(np.flatnonzero(init_mask[EMPTY_TAIL]), np.arange(100)) and init_mask[ALL_IN].all()
    _check_init_mask(fused, 'plain')
    _check_oracle(_constructed_oracle(orc, base._query(lib, B_EDGE, P_SET, 'fp32'), thr=False), np.arange(B_EDGE), fused, 'plain')


# ---- launch sets ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('ncalls', [2, 5])
def test_launch_sets(dev, lib, orc, ncalls):
    """Sets of two and five calls of 48 objects, every call with tensors and outputs of its own; one call alone holds an object without a
    re-fit record (image points unrelated to the object, a threshold of 1e-3 px: no model).  Each member equals its own un-fused run bit for bit."""
    from monorun_amd import PnPEpnpLaunch, PnPEpnpGroupLaunch
    B, P, bad_call, bad = 48, 300, 1, 17
    xs = []
    for m in range(ncalls):
        x, idx = base.inputs(dev, P, 'fp32', B, 'contiguous', offset=11 * m)
        if m == bad_call:
            x[0], x[1], x[6] = x[0].clone(), x[1].clone(), x[6].clone()
            x[0][bad] = torch.from_numpy(np.random.default_rng(99).uniform(0.0, 300.0, size=(P, 2)).astype(np.float32)).to(dev)
            x[1][bad] = 1.0
            x[6][bad] = 1e-3
        xs.append((x, idx))
    ls = [PnPEpnpLaunch(*x[:6], epnp_ransac_thres=x[6], with_diag=True, **KW) for x, _ in xs]
    PnPEpnpGroupLaunch(ls).run()
    ref = base.oracle(orc, P, 'fp32', base._query(lib, ncalls * B, P, 'fp32'))
    for m, (l, (x, idx)) in enumerate(zip(ls, xs)):
        g = base._outputs(l)
        assert not _differing(g, _run(x, False)), (ncalls, m, _differing(g, _run(x, False)))
        iv = g[8].numpy().astype(bool)
        assert not iv[bad] if m == bad_call else iv.all(), (ncalls, m)
        _check_init_mask(g, (ncalls, m))
        keep = np.arange(B) != bad if m == bad_call else np.ones(B, bool)
        o = [t.numpy()[keep] for t in g]
        base.check_against_oracle(ref, idx[keep], o[0], o[1], o[2].reshape(-1, 4, 4), o[4], o[5], o[6], o[8], what=('set', ncalls, m))


# ---- wave counts and storage types ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', ['fp32', 'fp16', 'fp64'])
@pytest.mark.parametrize('waves', [1, 2, 4, 8])
def test_wave_counts(dev, lib, orc, waves, dtype):
    """1, 2, 4 and 8 waves per object through the flags (the launch behind the initialiser runs one wave as two: mr_debug_launch_waves): the
    one-list instantiations keep the mask as bits, the others as bytes expanded from the bit row.  300 points: five chunks, the last of 44."""
    from monorun_amd import _lib
    fl = waves << _lib.MR_WAVES_SHIFT
    P = 300
    x, idx = base.inputs(dev, P, dtype, B_EDGE, 'planar', offset=80)          # ordinary and tree-sensitive objects
    fused, plain = _run(x, True, flags=fl), _run(x, False, flags=fl)
    assert not _differing(fused, plain), (waves, dtype, _differing(fused, plain))
    _check_init_mask(fused, (waves, dtype))
    _check_oracle(base.oracle(orc, P, dtype, base._query(lib, B_EDGE, P, dtype, flags=fl)), idx, fused, ('waves', waves, dtype))


# ---- second round ------------------------------------------------------------------------------------------------------------------------

def _outlier_objects():
    """B_EDGE ordinary objects of 300 points with 40 % of the image points replaced by points anywhere in the image: RANSAC's loop wants more than
    three iterations for nearly all of them."""
    if 'out' not in _SETS:
        d = base.distinct(300, 'fp32')
        x2d = np.array(d[0][:B_EDGE])
        rng = np.random.default_rng(616)
        for b in range(B_EDGE):
            at = rng.choice(300, size=120, replace=False)
            x2d[b, at] = rng.uniform(0.0, 300.0, size=(120, 2)).astype(np.float32)
        _SETS['out'] = [x2d] + [np.array(a[:B_EDGE]) for a in d[1:3]] + [d[3], d[4], d[5], np.array(d[6][:B_EDGE])]
    return _SETS['out']


@pytest.mark.parametrize('first_round', [1, 3])
def test_second_round_objects_write_the_rows_too(dev, lib, orc, first_round):
    """A first round forced to 1 and to 3 hypotheses on objects with outliers: most of them finish in the second round (epnp_round2_kernel: the
    same consensus body), whose objects write the list and the bit row too."""
    xn = _outlier_objects()
    x = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in xn]
    fused, plain = _run(x, True, first_round=first_round), _run(x, False, first_round=first_round)
    assert not _differing(fused, plain), (first_round, _differing(fused, plain))
    assert not _differing(fused, _run(x, True)), 'the split of the rounds changes no result'
    assert (fused[9].numpy()[:, 0] > first_round).sum() >= B_EDGE // 2, 'objects that needed the second round'
    _check_init_mask(fused, first_round)
    waves = base._query(lib, B_EDGE, 300, 'fp32')
    if ('out', waves) not in _SETS:
        with np.errstate(all='ignore'):
            _SETS[('out', waves)] = orc.u2d_pnp_epnp(*xn[:6], 0.5, 0.6, xn[6], True, num_threads=0, return_diag=True, return_init=True, cov_waves=waves)
    _check_oracle(_SETS[('out', waves)], np.arange(B_EDGE), fused, ('first round', first_round))
