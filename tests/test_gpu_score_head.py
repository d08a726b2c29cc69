"""The score head's fused launch on the MI355X: parity with tests/score_head_ref.py (numpy float64) within the derived
running-error bound at the real sizes, at the channel tails and on G16; row tiles; the sigmoid bit for bit from the kernel's own
logits; independence of a row from its batch; determinism; failed solves; the 2-D score; strided views; score_poses against the torch
path of the same module; the parameter cache; the HIP graph of ScoreHeadLaunch; the fall-back of a configuration the kernel does not
cover."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_head_ref as ref  # noqa: E402
from oracle import oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g16_score_head.npz')
DEV = torch.device('cuda:0')
KEYS = ('reg_fc_out', 'yaw', 't_vec', 'pose_cov', 'dimensions')
_heads = {}


@pytest.fixture(scope='module')
def g16():
    return dict(np.load(GOLDEN))


def _head(c1, c2, use_pose_norm=True):
    """A seeded eval-mode head on the device (built once per size) with running statistics away from (0, 1)."""
    from monorun_amd.score_head import MLPScoreHead
    key = (c1, c2, use_pose_norm)
    if key not in _heads:
        torch.manual_seed(1000 * c1 + c2)
        h = MLPScoreHead(reg_fc_out_channels=c1, pose_fc_out_channels=c1, fc_out_channels=c2, use_pose_norm=use_pose_norm)
        with torch.no_grad():
            h.fc_out.weight.normal_(0, 0.1)
            h.fc_out.bias.fill_(-0.2)
            if use_pose_norm:
                h.pose_norm.running_mean.normal_(0, 2)
                h.pose_norm.running_var.uniform_(0.3, 30)
                h.pose_norm.weight.uniform_(0.5, 1.5)
                h.pose_norm.bias.normal_(0, 0.2)
        _heads[key] = h.eval().to(DEV)
    return _heads[key]


def _g16_head(g16):
    from monorun_amd.score_head import MLPScoreHead
    h = MLPScoreHead(reg_fc_out_channels=96, pose_fc_out_channels=96, fc_out_channels=40)
    h.load_state_dict({k[len('param.'):]: torch.from_numpy(v) for k, v in g16.items() if k.startswith('param.')}, strict=True)
    return h.eval().to(DEV)


def _inputs(n, c1, seed):
    rng = np.random.default_rng(seed)
    a = rng.normal(0, 1, (n, 4, 4))
    d = dict(reg_fc_out=rng.normal(0, 1, (n, c1)), yaw=rng.uniform(-np.pi, np.pi, (n, 1)),
             t_vec=np.stack([rng.uniform(-12, 12, n), rng.uniform(1, 2, n), rng.uniform(5, 45, n)], 1),
             pose_cov=a @ a.transpose(0, 2, 1) * 10.0 ** rng.uniform(-4, 2, (n, 1, 1)), dimensions=rng.uniform([3.2, 1.4, 1.5], [4.6, 1.8, 1.8], (n, 3)))
    return {k: np.ascontiguousarray(v, np.float32) for k, v in d.items()}


def _dev(d):
    return [torch.from_numpy(d[k]).to(DEV) for k in KEYS]


def _logits(head, d, **kw):
    from monorun_amd.score_head import score_head_forward_fused
    out = score_head_forward_fused(head, *_dev(d), sigmoid=kw.pop('sigmoid', False), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_parity(head, d, c1, c2, what):
    z, A = ref.score_head_ref(ref.params_of(head), *[d[k] for k in KEYS])
    got = _logits(head, d)
    tol = ref.tolerance(A, c1, c2)
    err = np.abs(got.astype(np.float64) - z)
    print(f'{what}: max |z_gpu - z| = {err.max():.3e}, least tolerance = {tol.min():.3e}, worst err / tol = {(err / tol).max():.3e}')
    assert got.dtype == np.float32 and got.shape == z.shape
    assert (err <= tol).all(), (what, float((err / tol).max()))
    return got


@pytest.mark.parametrize('c1,c2,n', [(1024, 256, 100), (70, 33, 5), (1, 1, 5), (2048, 1024, 5)])
def test_parity_with_the_float64_reference(c1, c2, n):
    _check_parity(_head(c1, c2), _inputs(n, c1, seed=c1 + c2 + n), c1, c2, f'({c1}, {c2}) n = {n}')


def test_parity_without_the_norm():
    _check_parity(_head(70, 33, use_pose_norm=False), _inputs(9, 70, seed=4), 70, 33, 'no norm')


def test_parity_on_g16_and_with_the_reference_logits(g16):
    head = _g16_head(g16)
    d = {k: g16['A_' + k] for k in KEYS}
    got = _check_parity(head, d, 96, 40, 'G16')
    # the reference's own fp32 logits carry an error of their own within the same bound: twice the bound between the two
    _, A = ref.score_head_ref(ref.params_of(head), *[d[k] for k in KEYS])
    assert (np.abs(got.astype(np.float64) - g16['eval_logits']) <= 2 * ref.tolerance(A, 96, 40)).all()


def test_row_tiles():
    from monorun_amd.score_head import ROWS_PER_WORKGROUP as R
    head = _head(70, 33)
    for n in (0, 1, R - 1, R, R + 1, 257):
        d = _inputs(n, 70, seed=n)
        if n == 0:
            assert _logits(head, d).shape == (0,)
        else:
            _check_parity(head, d, 70, 33, f'n = {n}')


def test_sigmoid_is_the_specified_exp_bit_for_bit():
    head, d = _head(70, 33), _inputs(100, 70, seed=11)
    d['reg_fc_out'] *= 3                                                     # logits well into both tails
    z = _logits(head, d)
    s = _logits(head, d, sigmoid=True)
    with np.errstate(all='ignore'):
        want = np.float32(1) / (np.float32(1) + orc.spec_expf(-z))
    assert want.dtype == np.float32 and np.array_equal(s, want)
    assert s.min() < 0.2 and s.max() > 0.8


def test_a_row_does_not_depend_on_its_batch():
    head = _head(1024, 256)
    d = _inputs(100, 1024, seed=21)
    one = {k: v[:1].copy() for k, v in _inputs(1, 1024, seed=22).items()}
    alone = _logits(head, one)
    for pos in (0, 37, 99):                                                  # tile slots 0, 1 and 3
        b = {k: v.copy() for k, v in d.items()}
        for k in KEYS:
            b[k][pos] = one[k][0]
        assert _logits(head, b)[pos].tobytes() == alone[0].tobytes(), pos


def test_two_runs_are_bitwise_equal():
    head, d = _head(1024, 256), _inputs(100, 1024, seed=31)
    assert _logits(head, d, sigmoid=True).tobytes() == _logits(head, d, sigmoid=True).tobytes()


def test_failed_solves_score_exactly_zero():
    head, d = _head(70, 33), _inputs(23, 70, seed=41)
    ret_val = np.ones(23, bool)
    bad = [1, 4, 5, 22]
    ret_val[bad] = False
    rv = torch.from_numpy(ret_val).to(DEV)
    clean = _logits(head, d, sigmoid=True, ret_val=rv)
    dirty = {k: v.copy() for k, v in d.items()}
    dirty['pose_cov'][1] = np.nan
    dirty['pose_cov'][4] = np.inf
    dirty['pose_cov'][5, 2, 1] = -np.inf
    dirty['pose_cov'][22, 0, 0] = np.nan
    dirty['t_vec'][4] = np.nan
    for sigmoid in (True, False):
        got = _logits(head, dirty, sigmoid=sigmoid, ret_val=rv)
        assert (got[bad] == 0).all() and not np.signbit(got[bad]).any()
        want = clean if sigmoid else _logits(head, d, ret_val=rv)
        assert got.tobytes() == want.tobytes()
    unmasked = _logits(head, dirty, sigmoid=True)                            # without ret_val the NaN is the row's own, nobody else's
    ok = ret_val.copy()
    assert np.isnan(unmasked[[1, 22]]).all() and np.array_equal(unmasked[ok], clean[ok])


def test_scores_2d_multiplies_and_null_skips():
    head, d = _head(70, 33), _inputs(23, 70, seed=51)
    det = np.random.default_rng(52).uniform(0, 1, 23).astype(np.float32)
    rv = torch.ones(23, dtype=torch.bool, device=DEV)
    rv[3] = False
    base = _logits(head, d, sigmoid=True, ret_val=rv)
    got = _logits(head, d, sigmoid=True, ret_val=rv, scores_2d=torch.from_numpy(det).to(DEV))
    assert np.array_equal(got, base * det) and got[3] == 0 and not np.array_equal(got, base)


def test_strided_views_go_through_the_strides():
    from monorun_amd.score_head import _rows, score_head_forward_fused
    head, n = _head(70, 33), 19
    d = _inputs(n, 70, seed=61)
    want = _logits(head, d)
    rng = np.random.default_rng(62)
    wide = torch.from_numpy(rng.normal(0, 1, (2 * n, 96)).astype(np.float32)).to(DEV)
    pose = torch.from_numpy(rng.normal(0, 1, (n, 4)).astype(np.float32)).to(DEV)
    boxes = torch.from_numpy(rng.normal(0, 1, (n, 8)).astype(np.float32)).to(DEV)
    reg, yaw, t_vec, cov, dims = _dev(d)
    wide[::2, 5:75] = reg
    pose[:, :1], pose[:, 1:] = yaw, t_vec
    boxes[:, :3] = dims
    views = (wide[::2, 5:75], pose[:, :1], pose[:, 1:], cov, boxes[:, :3])
    for v, w in zip(views, (70, 1, 3, None, 3)):
        if w:
            assert not v.is_contiguous() and _rows(v, w).data_ptr() == v.data_ptr()      # read in place, no copy
    got = score_head_forward_fused(head, *views, sigmoid=False)
    torch.cuda.synchronize()
    assert got.cpu().numpy().tobytes() == want.tobytes()
    # a boolean selection of rows, as the RoI head's training path indexes (reg_fc_out[ret_val])
    keep = torch.from_numpy(rng.random(n) < 0.6).to(DEV)
    got = score_head_forward_fused(head, reg[keep], yaw[keep], t_vec[keep], cov[keep], dims[keep], sigmoid=False)
    torch.cuda.synchronize()
    assert got.cpu().numpy().tobytes() == want[keep.cpu().numpy()].tobytes()


def _pose_results(d, ret_val):
    reg, yaw, t_vec, cov, dims = _dev(d)
    return reg, dict(ret_val=ret_val, yaw_pred=yaw, t_vec_pred=t_vec, pose_cov_pred=cov * 0.5, pose_cov_calib=cov, dimensions_pred=dims)


def test_score_poses_fused_against_the_torch_path():
    import copy
    from monorun_amd.score_head import score_poses, score_poses_torch
    for c1, c2, n in ((1024, 256, 100), (70, 33, 7)):
        head, d = _head(c1, c2), _inputs(n, c1, seed=71)
        rv = torch.ones(n, dtype=torch.bool, device=DEV)
        rv[2] = False
        reg, res = _pose_results(d, rv)
        det = torch.from_numpy(np.random.default_rng(72).uniform(0, 1, n).astype(np.float32)).to(DEV)
        assert head.fused_ok() and not head.training
        with torch.no_grad():
            for calib in (True, False):
                scored = d if calib else dict(d, pose_cov=d['pose_cov'] * np.float32(0.5))       # pose_cov_pred of _pose_results
                _, A = ref.score_head_ref(ref.params_of(head), *[scored[k] for k in KEYS])
                tol = ref.tolerance(A, c1, c2) / 4 + 8 * 2.0 ** -24              # the sigmoid is 1/4-Lipschitz; its own roundings
                got = score_poses(head, reg, res, calib_scoring=calib, mult_2d_score=False)
                want = score_poses_torch(head, reg, res, calib_scoring=calib, mult_2d_score=False)
                torch.cuda.synchronize()
                err = (got.double() - want.double()).abs().cpu().numpy()
                print(f'({c1}, {c2}) calib = {calib}: max |fused - torch| = {err.max():.3e}, least tolerance = {tol.min():.3e}')
                assert (err <= tol).all() and float(got[2]) == 0 and got.shape == (n,)
            both = score_poses(head, reg, res, det_scores=det)
            assert torch.equal(both, score_poses(head, reg, res, mult_2d_score=False) * det)
    # training mode takes the torch ops and keeps the graph
    training = copy.deepcopy(_head(70, 33)).train()
    assert score_poses(training, reg, res, mult_2d_score=False).requires_grad


def test_parameter_cache_follows_in_place_updates():
    import copy
    head = copy.deepcopy(_head(70, 33))
    d = _inputs(9, 70, seed=81)
    before = _check_parity(head, d, 70, 33, 'before the step')
    with torch.no_grad():                                                    # what optimizer.step() does: in-place updates
        for p in head.parameters():
            p.add_(0.05 * torch.randn_like(p))
        head.pose_norm.running_mean.mul_(0.9)
    after = _check_parity(head, d, 70, 33, 'after the step')                 # the reference reads the new weights
    assert not np.array_equal(before, after)
    head.load_state_dict(_head(70, 33).state_dict())
    assert np.array_equal(_logits(head, d), before)


def test_prepared_launch_and_its_graph():
    from monorun_amd.score_head import ScoreHeadLaunch
    n = 100
    head = _head(1024, 256)
    launch = ScoreHeadLaunch(head, n, DEV)
    assert set(KEYS) <= set(launch.inputs) and launch.out['scores'].shape == (n,)

    def fill(seed):
        d = _inputs(n, 1024, seed=seed)
        for k, v in zip(KEYS, _dev(d)):
            launch.inputs[k].copy_(v)
        rv = torch.from_numpy(np.random.default_rng(seed).random(n) < 0.9).to(DEV)
        launch.inputs['ret_val'].copy_(rv)
        launch.inputs['det_scores'].copy_(torch.from_numpy(np.random.default_rng(seed + 1).uniform(0, 1, n).astype(np.float32)).to(DEV))
        return d, rv
    d, rv = fill(91)
    ran = launch.run()['scores'].clone()
    torch.cuda.synchronize()
    want = _logits(head, d, sigmoid=True, ret_val=rv, scores_2d=launch.inputs['det_scores'])
    assert ran.cpu().numpy().tobytes() == want.tobytes()
    launch.capture()                                                         # one stream, one kernel node: no parallel branches
    for seed in (92, 93):
        fill(seed)
        launch.out['scores'].zero_()
        replayed = launch.replay()['scores'].clone()
        launch.out['scores'].zero_()
        ran = launch.run()['scores'].clone()
        torch.cuda.synchronize()
        assert replayed.cpu().numpy().tobytes() == ran.cpu().numpy().tobytes() and float(ran.abs().max()) > 0
    with pytest.raises(ValueError):
        from monorun_amd.score_head import MLPScoreHead
        ScoreHeadLaunch(MLPScoreHead(reg_fc_out_channels=8, pose_fc_out_channels=8, fc_out_channels=4, fusion_type='concat').eval(), 4, DEV)


def test_a_configuration_the_kernel_does_not_cover_takes_the_torch_ops():
    from monorun_amd.score_head import MLPScoreHead, score_poses
    torch.manual_seed(5)
    cpu = MLPScoreHead(reg_fc_out_channels=24, pose_fc_out_channels=16, fc_out_channels=8, fusion_type='concat').eval()
    with torch.no_grad():
        cpu.fc_out.weight.normal_(0, 0.3)
    assert not cpu.fused_ok()
    import copy
    head = copy.deepcopy(cpu).to(DEV)
    n = 11
    d = _inputs(n, 24, seed=101)
    rv = torch.ones(n, dtype=torch.bool)
    rv[5] = False
    det = torch.from_numpy(np.random.default_rng(102).uniform(0, 1, n).astype(np.float32))
    cpu_in = [torch.from_numpy(d[k]) for k in KEYS]
    with torch.no_grad():
        res_cpu = dict(ret_val=rv, yaw_pred=cpu_in[1], t_vec_pred=cpu_in[2], pose_cov_pred=cpu_in[3], pose_cov_calib=cpu_in[3], dimensions_pred=cpu_in[4])
        want = score_poses(cpu, cpu_in[0], res_cpu, det_scores=det)
        reg, res = _pose_results(d, rv.to(DEV))
        got = score_poses(head, reg, res, det_scores=det.to(DEV))
        # the same network on absolute values bounds every partial sum: the running-error bound of both fp32 evaluations
        x = ref.inputs_x(*[d[k] for k in KEYS[1:]]).astype(np.float64)
        nrm = cpu.pose_norm
        g = lambda t: t.detach().double().abs().numpy()
        xa = (np.abs(x) + g(nrm.running_mean)) * g(nrm.weight / (nrm.running_var + nrm.eps).sqrt()) + g(nrm.bias)
        h1a = np.concatenate([xa @ g(cpu.pose_fcs[0].weight).T + g(cpu.pose_fcs[0].bias), np.abs(d['reg_fc_out']).astype(np.float64)], 1)
        A = (h1a @ g(cpu.fused_fcs[0].weight).T + g(cpu.fused_fcs[0].bias)) @ g(cpu.fc_out.weight).reshape(-1) + g(cpu.fc_out.bias)
        tol = 2 * (2.0 * (17 + 40 + 8 + 16) * 2.0 ** -24 * A / 4 + 8 * 2.0 ** -24)
    err = (got.cpu().double() - want.double()).abs().numpy()
    print(f'concat head: max |device - cpu| = {err.max():.3e}, least tolerance = {tol.min():.3e}')
    assert (err <= tol).all() and float(got[5]) == 0
