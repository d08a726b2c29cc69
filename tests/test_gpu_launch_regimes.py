"""The default flow at every launch regime the host picks by size (tests/launch_regimes.py): the initialiser's first round, its second
round in one launch or two, the lane mappings of the hypothesis and re-fit launches (and their partial last workgroups), and the waves per
object of the LM / covariance launch, whose summation tree the `valid` flag follows.  Every case runs against the oracle at the wave count
the launch really uses (mr_debug_launch_waves), on objects of which a quarter are tree-sensitive (tests/fuzz_cases.make_tree_sensitive:
their `valid` flag differs between wave counts, tests/test_cov_tree.py)."""
import ctypes

import numpy as np
import pytest
import torch

from monorun_amd import synthetic as syn
from tests import cov_tree, fuzz_cases
from tests import launch_regimes as lr

pytestmark = pytest.mark.gpu

INIT_TOL = 1e-9          # as tests/test_gpu_epnp.py
POSE_TOL = 1e-4
N_DISTINCT = 128         # distinct objects per (P, dtype); larger launches tile them
NP_DTYPE = {'fp16': np.float16, 'fp32': np.float32, 'fp64': np.float64}
T_DTYPE = {'fp16': torch.float16, 'fp32': torch.float32, 'fp64': torch.float64}
KW = dict(z_min=0.5, epnp_istd_thres=0.6, inlier_opt_only=True)


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def lib():
    from monorun_amd import _lib
    return _lib.load()


def _device():
    return dict(lr.MI355X, cus=torch.cuda.get_device_properties(0).multi_processor_count)


def _query(lib, objects, P, dtype, flags=0, after_init=True):
    from monorun_amd.ops.least_squares.pnp_uncert import _DTYPES
    w = lib.mr_debug_launch_waves(objects, P, _DTYPES[T_DTYPE[dtype]], flags, int(after_init))
    assert w in (1, 2, 3, 4, 8), w
    return w


_DISTINCT, _ORACLE = {}, {}


def distinct(P, dtype):
    """N_DISTINCT objects x P points, contiguous float32 as the storage type rounds them: three quarters ordinary synthetic objects, one
    quarter tree-sensitive ones.  [x2d, istd, x3d, K (1,3,3), u_range, v_range, thr (N,)]"""
    key = (P, dtype)
    if key not in _DISTINCT:
        rng = np.random.default_rng(7000 + P)
        n_tree = N_DISTINCT // 4
        b = syn.make_batch(B=N_DISTINCT - n_tree, hw=int(np.ceil(np.sqrt(P))), seed=int(rng.integers(1 << 30)))
        ordinary = [np.ascontiguousarray(a) for a in syn.pnp_boundary(b, planar=False)]
        tree = fuzz_cases.make_tree_sensitive(rng, n_tree, P)
        x = [np.concatenate([ordinary[k][:, :P], tree[k]]) for k in range(3)]
        x = [np.ascontiguousarray(a.astype(NP_DTYPE[dtype]).astype(np.float32)) for a in x]
        _DISTINCT[key] = x + [np.asarray(ordinary[3], np.float32).reshape(1, 3, 3), ordinary[4], ordinary[5],
                              np.concatenate([ordinary[6], tree[6]]).astype(np.float32)]
    return _DISTINCT[key]


def oracle(orc, P, dtype, waves, flow='epnp'):
    key = (P, dtype, waves, flow)
    if key not in _ORACLE:
        x = distinct(P, dtype)
        f = orc.u2d_pnp_epnp if flow == 'epnp' else orc.u2d_pnp
        with np.errstate(all='ignore'):
            _ORACLE[key] = f(*x[:6], 0.5, 0.6, x[6], True, num_threads=0, return_diag=True, return_init=True, cov_waves=waves)
    return _ORACLE[key]


def inputs(dev, P, dtype, B, layout, offset=0):
    """B objects tiled from the distinct set (object i = distinct (i + offset) % N_DISTINCT) as device tensors of the storage type,
    channel-planar strided views ('planar', as the pipeline hands them over) or contiguous (B,P,C); and the tile index."""
    x = distinct(P, dtype)
    idx = (np.arange(B) + offset) % N_DISTINCT
    it = torch.from_numpy(idx).to(dev)
    out = []
    for a in x[:3]:
        d = torch.from_numpy(a).to(dev, T_DTYPE[dtype])
        if layout == 'planar':
            out.append(d.permute(0, 2, 1).contiguous()[it].permute(0, 2, 1))
        else:
            out.append(d[it].contiguous())
    K, ur, vr = (torch.from_numpy(a).to(dev) for a in x[3:6])
    thr = torch.from_numpy(x[6]).to(dev)[it].contiguous()
    return out + [K, ur, vr, thr], idx


def check_against_oracle(ref, idx, valid, pose, cov, mask, diag, init_pose=None, init_valid=None, what=''):
    """Per object against the oracle at the launch's wave count: masks bit-exact, start pose within INIT_TOL, LM iterations / exit reasons
    identical, pose within 1e-4, `valid` bit-exact where the pose equals the oracle's bit for bit, cov within 1e-5 relative on valid
    objects; at most 1 % of the ordinary objects with another pose.  The tree-sensitive objects (the last quarter of the distinct set) are
    singular to rounding by construction, in the LM too at small P: a pose one rounding away moves their cov arbitrarily, so their cov is
    compared where the pose is the oracle's.  So are all objects of P = 4 (8 residuals for 4 unknowns: cov up to 1e13, about 1 % of them
    one rounding away from the oracle's pose, measured)."""
    loose = (idx >= N_DISTINCT - N_DISTINCT // 4) | (mask.shape[1] == 4)
    r_ret, r_yaw, r_t, r_cov, _, r_mask, r_diag, r_init = [a[idx] for a in ref]
    assert np.array_equal(mask.astype(bool), r_mask), (what, 'inlier mask', np.flatnonzero((mask.astype(bool) != r_mask).any(1))[:8])
    r_ok = r_diag[:, 2] != 8                                   # the oracle's initialiser succeeded
    if init_valid is not None:
        assert np.array_equal(init_valid.astype(bool), r_ok), (what, 'initialiser success')
        assert np.abs(init_pose[r_ok] - r_init[r_ok]).max(initial=0.0) <= INIT_TOL, (what, 'start pose')
    assert np.array_equal(diag[:, 0], r_diag[:, 0]) and np.array_equal(diag[:, 2] % 16, r_diag[:, 2]), (what, 'LM iterations / exit reasons')
    rp = np.concatenate([r_yaw, r_t], 1)
    both = np.isnan(pose) & np.isnan(rp)
    same = ((pose == rp) | both).all(1)
    ok = r_ret & valid.astype(bool)
    dyaw = np.abs(np.angle(np.exp(1j * (pose[ok, 0] - rp[ok, 0]))))
    assert dyaw.max(initial=0.0) <= POSE_TOL and np.abs(pose[ok, 1:] - rp[ok, 1:]).max(initial=0.0) <= POSE_TOL, (what, 'pose')
    assert np.array_equal(valid.astype(bool)[same], r_ret[same]), (what, 'valid', np.flatnonzero(same & (valid.astype(bool) != r_ret))[:8])
    assert (~same & ~loose).sum() <= 0.01 * len(same), (what, 'ordinary objects with another pose', int((~same & ~loose).sum()))
    ok &= same | ~loose
    if ok.any():
        scale = np.abs(r_cov[ok]).reshape(int(ok.sum()), -1).max(1)[:, None, None]
        assert (np.abs(cov[ok] - r_cov[ok]) / scale).max() <= 1e-5, (what, 'cov')


# ---- the reduction tree itself -------------------------------------------------------------------------------------------------

def _tree_partials(waves, seed):
    """(64 waves, 10) partials of mixed magnitudes (1e16, 1, -1e16, ...): the bits of a sum depend on its order."""
    rng = np.random.default_rng(seed)
    mag = rng.choice([1e16, 1.0, 3.0, 1e8, 0.5], size=(64 * waves, 10))
    return mag * rng.choice([-1.0, 1.0], size=mag.shape) * (1.0 + rng.integers(0, 7, mag.shape) / 8.0)


@pytest.mark.parametrize('waves', [1, 2, 3, 4, 8])
def test_block_sum_follows_the_specified_tree(dev, lib, orc, waves):
    """block_sum_packed<WPO, 10> (the covariance stage's reduction) on given per-lane partials equals the oracle's tree (orc_tree_sum:
    butterfly strides 32, 16, 1, 2, 4, 8 within a wave, then the waves in order) and the numpy restatement, bit for bit, in every wave;
    the partials are chosen so that other orders give other bits."""
    for seed in range(4):
        part = _tree_partials(waves, 100 * waves + seed)
        want = orc.tree_sum(part, waves)
        assert np.array_equal(want.view(np.uint64), cov_tree.tree_sum(part, waves).view(np.uint64))
        sequential = np.zeros(10)
        for row in part:
            sequential = sequential + row
        others = [sequential, cov_tree.tree_sum(part, waves, strides=(1, 2, 4, 8, 16, 32)), cov_tree.tree_sum(part, waves, strides=(32, 16, 2, 1, 4, 8))]
        assert sum(not np.array_equal(o.view(np.uint64), want.view(np.uint64)) for o in others) >= 2, 'partials do not discriminate the order'
        d_part = torch.from_numpy(part).to(dev)
        out = torch.full((waves, 10), float('nan'), dtype=torch.float64, device=dev)
        assert lib.mr_debug_block_sum(waves, ctypes.c_void_p(d_part.data_ptr()), ctypes.c_void_p(out.data_ptr()), None) == 0
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for w in range(waves):
            assert np.array_equal(got[w].view(np.uint64), want.view(np.uint64)), (waves, seed, w, got[w] - want)
    assert lib.mr_debug_block_sum(5, ctypes.c_void_p(d_part.data_ptr()), ctypes.c_void_p(out.data_ptr()), None) < 0


# ---- the regime table ----------------------------------------------------------------------------------------------------------

def test_wave_query_matches_the_restated_rule(lib):
    """mr_debug_launch_waves (what the LM launch uses) equals tests/launch_regimes.py's restatement over the whole case list, the grouped
    shapes and both flows; the restatement is what the CPU coverage test relies on."""
    d = _device()
    shapes = {(B, P, dt) for _, B, P, dt, _ in lr.cases()} | {(B * n, 784, 'fp32') for n, B in GROUPS} | {(B, 784, 'fp32') for n, B in GROUPS}
    for B, P, dt in sorted(shapes):
        for after_init in (True, False):
            assert _query(lib, B, P, dt, after_init=after_init) == lr.lm_waves(B, P, dt, after_init=after_init, dev=d), (B, P, dt, after_init)
    from monorun_amd import _lib
    for w in (1, 2, 3, 4, 8):                          # explicit waves: honoured (the default flow's launch has 2, 4 and 8)
        assert _query(lib, 100, 784, 'fp32', flags=w << _lib.MR_WAVES_SHIFT, after_init=False) == w
        assert _query(lib, 100, 784, 'fp32', flags=w << _lib.MR_WAVES_SHIFT) == {1: 2, 3: 4}.get(w, w)
    assert lib.mr_debug_launch_waves(0, 784, 0, 0, 1) < 0 and lib.mr_debug_launch_waves(10, 3, 0, 0, 1) < 0


_CASES = lr.cases()


@pytest.mark.parametrize('case', _CASES, ids=['-'.join(str(v) for v in c) for c in _CASES])
def test_default_flow_at_the_regime_boundaries(dev, lib, orc, case):
    """One call per case of tests/launch_regimes.cases() against the oracle at the launch's own wave count; the default flow through
    pnp_uncert_epnp_device and PnPEpnpLaunch (fused and the two entry points), the fast mode through pnp_uncert_device."""
    from monorun_amd import PnPEpnpLaunch
    from monorun_amd.ops.least_squares.pnp_uncert import pnp_uncert_device, pnp_uncert_epnp_device
    flow, B, P, dtype, layout = case
    x, idx = inputs(dev, P, dtype, B, layout)
    waves = _query(lib, B, P, dtype, after_init=(flow == 'epnp'))
    ref = oracle(orc, P, dtype, waves, flow)
    init_pose = init_valid = None
    if flow == 'k0':
        valid, pose, cov, tr, mask, diag = pnp_uncert_device(*x[:6], epnp_ransac_thres=x[6], with_diag=True, **KW)
    else:
        api = _CASES.index(case) % 3
        if api == 0:
            valid, pose, cov, tr, mask, diag, init_pose, init_valid = pnp_uncert_epnp_device(*x[:6], epnp_ransac_thres=x[6], with_diag=True, **KW)
        else:
            l = PnPEpnpLaunch(*x[:6], epnp_ransac_thres=x[6], with_diag=True, fused=(api == 1), **KW)
            l.run()
            valid, pose, cov, mask, diag, init_pose, init_valid = l.valid, l.pose, l.cov, l.mask, l.diag, l.init_pose, l.init_valid
            torch.cuda.synchronize()
            iv = init_valid.cpu().numpy().astype(bool)
            assert np.array_equal(l.init_mask.cpu().numpy()[iv], mask.cpu().numpy()[iv]), 'the hand-over mask is the final inlier mask'
    torch.cuda.synchronize()
    n = lambda t: None if t is None else t.cpu().numpy()
    check_against_oracle(ref, idx, n(valid), n(pose), n(cov).reshape(B, 4, 4), n(mask), n(diag), n(init_pose), n(init_valid), what=(case, waves))


def test_the_wave_count_decides_valid_on_the_corpus(dev, lib, orc):
    """The parity test above can fail: on the distinct objects of P = 784 and 300, the oracle's `valid` differs between the wave counts the
    library launches, and the GPU agrees with the oracle at its own count, not at the other, on objects whose pose is the oracle's."""
    decided = 0
    for P in (784, 300):
        refs = {w: oracle(orc, P, 'fp32', w) for w in (2, 4)}
        assert (refs[2][0] != refs[4][0]).sum() >= 3, P
        for B in (64, 4097):
            w = _query(lib, B, P, 'fp32')
            other = 4 if w == 2 else 2
            x, idx = inputs(dev, P, 'fp32', B, 'planar')
            from monorun_amd.ops.least_squares.pnp_uncert import pnp_uncert_epnp_device
            out = pnp_uncert_epnp_device(*x[:6], epnp_ransac_thres=x[6], **KW)
            torch.cuda.synchronize()
            valid = out[0].cpu().numpy().astype(bool)
            pose = out[1].cpu().numpy()
            rp = np.concatenate([refs[w][1], refs[w][2]], 1)[idx]
            same = (pose == rp).all(1)
            assert np.array_equal(valid[same], refs[w][0][idx][same]), (P, B, w)
            decided += int((valid[same] != refs[other][0][idx][same]).sum())
    assert decided >= 1, 'the other wave count would have passed too'


# ---- results that do not depend on the launch shape --------------------------------------------------------------------------

def _outputs(l):
    torch.cuda.synchronize()
    return [t.cpu() for t in (l.valid, l.pose, l.cov, l.tr, l.mask, l.diag, l.init_pose, l.init_mask, l.init_valid, l.init_diag)]


def _bytes_equal(a, b):
    return all(torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)) for x, y in zip(a, b))


def test_fixed_waves_results_do_not_depend_on_the_initialiser_regime(dev):
    """Explicit, identical waves per object (MR_WAVES = 4): B below and above each of the initialiser's boundaries gives every output
    bit-identical per distinct object — the lane mappings (wave / row / quad form with its partial last workgroup), the first round of 10
    or 3, the second round in one launch or two change the work, never a result."""
    from monorun_amd import PnPEpnpLaunch, _lib
    fl = 4 << _lib.MR_WAVES_SHIFT
    ref = None
    for B in (4097, 102, 103, 409, 410, 512, 513, 2047, 2048, 2049, 1):
        x, idx = inputs(dev, 784, 'fp32', B, 'planar')
        l = PnPEpnpLaunch(*x[:6], epnp_ransac_thres=x[6], with_diag=True, flags=fl, **KW)
        l.run()
        out = _outputs(l)
        if ref is None:
            ref = out                                  # 4097 objects: every distinct object at least 32 times
            first = [o[:N_DISTINCT] for o in ref]
            for k in range(1, 32):
                assert _bytes_equal([o[k * N_DISTINCT:(k + 1) * N_DISTINCT] for o in ref], first), ('tile', k)
            continue
        assert _bytes_equal(out, [o[torch.from_numpy(idx)] for o in first]), B


def test_first_round_does_not_change_a_result(dev):
    """PnPEpnpLaunch(first_round=1, 3, 10, 29, 30) at B = 1000 (one-launch second round) and B = 2100 (two launches): bit-identical."""
    from monorun_amd import PnPEpnpLaunch
    for B in (1000, 2100):
        x, _ = inputs(dev, 784, 'fp32', B, 'contiguous', offset=5)
        outs = []
        for fr in (None, 1, 3, 10, 29, 30):
            l = PnPEpnpLaunch(*x[:6], epnp_ransac_thres=x[6], with_diag=True, first_round=fr, **KW)
            l.run()
            outs.append(_outputs(l))
        for k, o in enumerate(outs[1:]):
            assert _bytes_equal(o, outs[0]), (B, k)


def test_automatic_waves_equal_the_queried_explicit_waves(dev, lib):
    """The automatic launch equals the launch with MR_WAVES = the queried count bit for bit, on the tree-sensitive objects too: the
    query tells the truth."""
    from monorun_amd import PnPEpnpLaunch, _lib
    for B, P, dtype in ((64, 784, 'fp32'), (2049, 784, 'fp32'), (2049, 300, 'fp32'), (4097, 300, 'fp32'), (64, 3136, 'fp16'), (64, 127, 'fp32')):
        x, _ = inputs(dev, P, dtype, B, 'planar')
        w = _query(lib, B, P, dtype)
        for fused in (True, False):
            la = PnPEpnpLaunch(*x[:6], epnp_ransac_thres=x[6], with_diag=True, fused=fused, **KW)
            le = PnPEpnpLaunch(*x[:6], epnp_ransac_thres=x[6], with_diag=True, fused=fused, flags=w << _lib.MR_WAVES_SHIFT, **KW)
            la.run(); le.run()
            assert _bytes_equal(_outputs(la), _outputs(le)), (B, P, dtype, w, fused)


@pytest.mark.parametrize('B', [103, 2049])
def test_every_output_is_written(dev, B):
    """Every output and hand-over tensor of PnPEpnpLaunch (fused and not) prefilled with NaN / 0xA5 bytes and with zeros: identical
    results, so no element is left as the caller's memory had it."""
    from monorun_amd import PnPEpnpLaunch
    x, _ = inputs(dev, 300, 'fp32', B, 'planar', offset=3)
    for fused in (True, False):
        res = []
        for fill in ('garbage', 'zero'):
            l = PnPEpnpLaunch(*x[:6], epnp_ransac_thres=x[6], with_diag=True, fused=fused, **KW)
            for t in (l.valid, l.pose, l.cov, l.tr, l.mask, l.diag, l.init_pose, l.init_mask, l.init_valid, l.init_diag):
                if fill == 'zero':
                    t.zero_()
                elif t.dtype == torch.uint8:
                    t.fill_(0xA5)
                else:
                    t.fill_(float('nan'))
            l.run()
            res.append(_outputs(l))
        assert _bytes_equal(res[0], res[1]), (B, fused, [k for k, (a, b) in enumerate(zip(*res)) if not _bytes_equal([a], [b])])


# ---- grouped calls across 2048 ---------------------------------------------------------------------------------------------------

GROUPS = ((8, 255), (8, 256), (3, 683), (2, 2049))


@pytest.mark.parametrize('group', GROUPS, ids=[f'{n}x{B}' for n, B in GROUPS])
def test_grouped_calls_across_2048_objects(dev, lib, orc, group):
    """PnPEpnpGroupLaunch of equal members whose set crosses the initialiser's 2048-object boundaries, LM launches 'fused' / 'grouped' (one
    over the set) and 'serial' (one per member) — their wave counts differ.  Against the calls one by one: masks, hand-over, pose, LM
    iterations / exit reasons / consensus bit-identical on objects whose pose is, tr and cost within 1e-6; `valid` and cov against the
    oracle at each LM launch's own wave count."""
    from monorun_amd import PnPEpnpLaunch, PnPEpnpGroupLaunch
    n, B = group
    xs = [inputs(dev, 784, 'fp32', B, 'planar', offset=37 * m) for m in range(n)]
    solo = []
    for x, _ in xs:
        l = PnPEpnpLaunch(*x[:6], epnp_ransac_thres=x[6], with_diag=True, **KW)
        l.run()
        solo.append(_outputs(l))
    for lm in ('fused', 'grouped', 'serial'):
        ls = [PnPEpnpLaunch(*x[:6], epnp_ransac_thres=x[6], with_diag=True, **KW) for x, _ in xs]
        PnPEpnpGroupLaunch(ls, lm=lm).run()
        waves = _query(lib, B if lm == 'serial' else n * B, 784, 'fp32')
        ref = oracle(orc, 784, 'fp32', waves)
        for m, (l, (_, idx)) in enumerate(zip(ls, xs)):
            g = _outputs(l)
            s = solo[m]
            for k in (4, 6, 7, 8, 9):                  # mask, init_pose / mask / valid / diag
                assert torch.equal(g[k], s[k]), (group, lm, m, k)
            same = ((g[1] == s[1]) | (torch.isnan(g[1]) & torch.isnan(s[1]))).all(1).numpy()
            assert (~same).sum() <= 0.01 * B, (group, lm, m, int((~same).sum()))
            gd, sd = g[5].numpy(), s[5].numpy()
            assert np.array_equal(gd[same][:, [0, 2, 3]], sd[same][:, [0, 2, 3]]), (group, lm, m, 'iterations / reasons / consensus')
            for a, b in ((g[3].numpy(), s[3].numpy()), (gd[:, 1], sd[:, 1])):
                fin = np.isfinite(b)
                assert np.array_equal(np.isfinite(a), fin) and (np.abs(a[fin] - b[fin]) <= 1e-6 * np.abs(b[fin]) + 1e-30).all(), (group, lm, m)
            check_against_oracle(ref, idx, g[0].numpy(), g[1].numpy(), g[2].numpy(), g[4].numpy(), gd, g[6].numpy(), g[8].numpy(), what=(group, lm, m, waves))
