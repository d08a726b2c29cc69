"""The global head's Monte-Carlo eval forward on the GPU: mr_global_head_mc_forward against the numpy fp64 reference
of tests/global_head_ref.py on the same masks.

Bound B per element of ``samples`` and ``reg_fc_out``: 2 (A + C + 2F + 16) 2^-24 Abs, Abs the same network in fp64 on |x|, |W|, |b|
with the same masks and scales (the running-error bound of fp32 sums in any order; relu is 1-Lipschitz; the 16 covers bias adds,
scales and roundings).  ``mean`` and ``var`` are checked against the fp64 mean / two-pass unbiased variance of the kernel's own
returned samples, to 1 fp32 ulp.  The device torch path (``mc_forward_torch``) is another fp32 evaluation: within 2 B."""
import os

import numpy as np
import pytest
import torch

from tests import global_head_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'

# (in_channels, (rh, rw), F, latent, classes, class_agnostic, S, n)
SHAPES = {
    'odd': (5, (3, 3), 70, 3, 2, False, 3, 5),                  # nothing is a multiple of any tile edge
    'one': (1, (1, 1), 1, 1, 1, False, 2, 1),
    'chunks': (16, (7, 7), 64, 16, 3, False, 50, 130),          # 6500 sample rows: many M tiles, three RoI passes
    'real': (256, (7, 7), 1024, 16, 3, False, 50, 3),           # the real layer sizes
}


def _make_head(C, rf, F, lat, classes, agnostic, S, seed=0, **kw):
    from monorun_amd.global_head import FCExtractorMonteCarlo
    head = FCExtractorMonteCarlo(num_samples=S, in_channels=C, roi_feat_size=rf, fc_out_channels=F, latent_channels=lat, num_classes=classes,
                                 latent_class_agnostic=agnostic, loss_dim=dict(type='SmoothL1LossMod'), dim_coder=dict(type='MultiClassNormDimCoder'),
                                 **kw)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in head.parameters():                              # ~unit-variance pre-activations: relu cuts about half
            fan_in = p.size(1) if p.dim() == 2 else 1
            p.copy_(torch.randn(p.shape, generator=g) * (1.5 / fan_in ** 0.5 if p.dim() == 2 else 0.3))
    return head.eval()


class Case:
    def __init__(self, head, x, masks):
        self.head, self.x, self.masks = head.to(DEV), x, masks
        self.params = ref.params_of(head)
        self.p2d, self.p = head.dropout2d_rate, head.dropout_rate
        self.ref = ref.mc_forward_ref(self.params, x.numpy(), [m.numpy() for m in masks], self.p2d, self.p)
        self.B = ref.bound(self.params, x.numpy(), [m.numpy() for m in masks], self.p2d, self.p)
        self._hip = None

    def run(self, x=None, masks=None, **kw):
        x = self.x if x is None else x
        masks = self.masks if masks is None else masks
        with torch.no_grad():
            out = self.head.mc_forward_hip(x.to(DEV), [m.to(DEV) for m in masks], return_samples=True, **kw)
        torch.cuda.synchronize()
        return dict(mean=out[0].cpu().numpy(), var=out[1].cpu().numpy(), reg_fc_out=out[4].cpu().numpy(), samples=out[5].cpu().numpy())

    @property
    def hip(self):
        if self._hip is None:
            self._hip = self.run()
        return self._hip


def _synthetic(name):
    C, rf, F, lat, classes, agnostic, S, n = SHAPES[name]
    head = _make_head(C, rf, F, lat, classes, agnostic, S, seed=len(name))
    g = torch.Generator().manual_seed(100 + n)
    x = torch.randn(n, C, *rf, generator=g)
    return Case(head, x, head.draw_masks(n, 'cpu', generator=g))


def _g19(tag):
    g = dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'g19_global_head.npz')))
    head = _make_head(6, 3, 40, 5, 3 if tag == 'a' else 1, tag == 'b', 7)
    head.load_state_dict({k[len(tag) + 7:]: torch.from_numpy(v) for k, v in g.items() if k.startswith(tag + '_param.')}, strict=True)
    return Case(head, torch.from_numpy(g[tag + '_x']), [torch.from_numpy(g[f'{tag}_keep{k}']) for k in range(3)])


_cases = {}


def case(name):
    """each case and its references are computed once and shared"""
    if name not in _cases:
        _cases[name] = _g19(name[-1]) if name.startswith('g19') else _synthetic(name)
    return _cases[name]


ALL = ['g19a', 'g19b', 'odd', 'one', 'chunks', 'real']


def _check_against_ref(c, got, tag):
    for key in ('samples', 'reg_fc_out'):
        err, B = np.abs(got[key] - c.ref[key]), c.B[key]
        print(f'{tag} {key}: max err {err.max():.3e}, max err / B {np.max(err / np.maximum(B, 1e-300)):.3f}')
        assert got[key].shape == c.ref[key].shape and np.all(err <= B), (tag, key, float(err.max()))
    mean64, var64 = ref.stats_of_samples(got['samples'])
    em, ev = np.abs(got['mean'] - mean64) / ref.ulp32(mean64), np.abs(got['var'] - var64) / ref.ulp32(var64)
    print(f'{tag} mean: {em.max():.3f} ulp, var: {ev.max():.3f} ulp')
    assert em.max() <= 1.0 and ev.max() <= 1.0, (tag, float(em.max()), float(ev.max()))


@pytest.mark.parametrize('name', ALL)
def test_hip_path_matches_the_fp64_reference(name):
    c = case(name)
    with torch.no_grad():                                           # the parameters require grad: covered where no graph is kept
        assert c.head.hip_ok(c.x.to(DEV))
    _check_against_ref(c, c.hip, name)


@pytest.mark.parametrize('name', ALL)
def test_hip_path_against_the_torch_path_on_the_device(name):
    c = case(name)
    with torch.no_grad():
        t = c.head.mc_forward_torch(c.x.to(DEV), [m.to(DEV) for m in c.masks], return_samples=True)
    for key, tv in (('samples', t[5]), ('reg_fc_out', t[4])):
        err = np.abs(c.hip[key] - tv.cpu().numpy())
        print(f'{name} {key}: hip - torch max err / 2B {np.max(err / np.maximum(2 * c.B[key], 1e-300)):.3f}')
        assert np.all(err <= 2 * c.B[key]), (name, key)
    # the statistics of near-equal samples are near-equal: checked loosely here, exactly in the reference test
    np.testing.assert_allclose(c.hip['mean'], t[0].cpu().numpy(), atol=float(2 * c.B['samples'].max()))


@pytest.mark.parametrize('name', ['g19a', 'odd', 'chunks', 'real'])
def test_a_roi_alone_equals_the_roi_in_its_batch_bitwise(name):
    c = case(name)
    n = c.x.size(0)
    for i in sorted({0, n // 2, n - 1, min(n - 1, 64), min(n - 1, 129)}):
        alone = c.run(c.x[i:i + 1].contiguous(), [m[:, i:i + 1].contiguous() for m in c.masks])
        for key in ('mean', 'var', 'reg_fc_out'):
            assert np.array_equal(alone[key][0], c.hip[key][i], equal_nan=True), (name, i, key)
        assert np.array_equal(alone['samples'][:, 0], c.hip['samples'][:, i], equal_nan=True), (name, i)


@pytest.mark.parametrize('name', ['odd', 'chunks'])
def test_two_calls_agree_bitwise_and_nothing_is_read_before_it_is_written(name):
    c = case(name)
    n, S, J, F = c.x.size(0), c.head.num_samples, c.head.out_channels, c.head.fc_out_channels
    f32 = dict(device=DEV, dtype=torch.float32)
    work = torch.full((c.head.workspace_numel(n) + 64,), float('nan'), **f32)
    out = dict(mean=torch.full((n, J), float('nan'), **f32), var=torch.full((n, J), float('nan'), **f32),
               reg_fc_out=torch.full((n, F), float('nan'), **f32), samples=torch.full((S, n, J), float('nan'), **f32))
    again = c.run(workspace=work, out=out)
    for key, v in again.items():
        assert np.all(np.isfinite(v)), (name, key)
        assert np.array_equal(v, c.hip[key]), (name, key)
    assert bool(torch.isnan(work[-64:]).all())                      # nothing beyond the stated size is touched
    if n > 64:
        assert c.head.workspace_numel(n) == c.head.workspace_numel(64)      # the workspace is one pass's


def test_all_true_masks_make_every_sample_identical():
    c = case('odd')
    got = c.run(masks=[torch.ones_like(m) for m in c.masks])
    assert np.all(got['samples'] == got['samples'][:1])
    assert np.all(got['var'] == 0) and np.array_equal(got['mean'], got['samples'][0])


def test_a_roi_with_every_channel_dropped_sees_only_the_bias():
    c = case('odd')
    masks = [m.clone() for m in c.masks]
    masks[0][:, 2] = False
    got = c.run(masks=masks)
    r = ref.mc_forward_ref(c.params, c.x.numpy(), [m.numpy() for m in masks], c.p2d, c.p)
    B = ref.bound(c.params, c.x.numpy(), [m.numpy() for m in masks], c.p2d, c.p)
    b1 = c.params['fcs.0.bias']
    assert np.array_equal(r['h1'][:, 2], np.maximum(b1, 0) * masks[1][:, 2].numpy() / (1 - c.p))      # h1 = keep1 q1 relu(b1)
    assert np.all(np.abs(got['samples'] - r['samples']) <= B['samples'])
    assert np.all(np.abs(got['reg_fc_out'] - r['reg_fc_out']) <= B['reg_fc_out'])


def test_a_nan_stays_in_its_roi():
    c = case('odd')
    x = c.x.clone()
    x[3, 1, 0, 2] = float('nan')
    got = c.run(x)
    others = [i for i in range(x.size(0)) if i != 3]
    for key in ('mean', 'var', 'reg_fc_out'):
        assert np.array_equal(got[key][others], c.hip[key][others]), key
        assert np.isnan(got[key][3]).any(), key
    assert np.array_equal(got['samples'][:, others], c.hip['samples'][:, others])
    assert np.isnan(got['mean'][3]).all()                           # W1 is dense: every first-layer output of the RoI is NaN


def test_dispatch_takes_the_torch_path_where_the_kernels_do_not_apply():
    from monorun_amd.global_head import FCExtractorMonteCarlo
    c = case('odd')
    head, x, masks = c.head, c.x.to(DEV), [m.to(DEV) for m in c.masks]

    def same(a, b):
        # the torch path against itself: rocBLAS may pick another kernel on a second call, so agreement is to fp rounding
        return all((u is None and v is None) or torch.allclose(u, v, rtol=1e-5, atol=1e-6) for u, v in zip(a, b))
    with torch.no_grad():
        # the HIP path is what mc_forward runs on a covered call, and forward draws its own masks
        got = head.mc_forward(x, masks)
        assert np.array_equal(got[0].cpu().numpy(), c.hip['mean']) and got[2] is None and got[3] is None and len(got) == 5
        g1, g2 = torch.Generator(DEV).manual_seed(5), torch.Generator(DEV).manual_seed(5)
        a, b = head.mc_forward(x, generator=g1), head.mc_forward(x, masks=head.draw_masks(x.size(0), DEV, generator=g2))
        assert all(torch.equal(a[k], b[k]) for k in (0, 1, 4))          # the same seed: the same masks, the HIP path's bits
        out = head(x)
        assert out[0].shape == (5, head.out_channels) and out[1].shape == (5, head.out_channels) and out[4].shape == (5, 70)
        assert bool((out[1] >= 0).all()) and out[0].dtype == torch.float32 and out[0].is_contiguous()
        # CPU, fp64, non-contiguous x
        cpu_head = _make_head(*SHAPES['odd'][:7], seed=len('odd'))
        cm = [m.cpu() for m in masks]
        assert not cpu_head.hip_ok(c.x) and same(cpu_head.mc_forward(c.x, cm), cpu_head.mc_forward_torch(c.x, cm))
        d_head = _make_head(*SHAPES['odd'][:7], seed=len('odd')).double().to(DEV)
        assert not d_head.hip_ok(x.double()) and same(d_head.mc_forward(x.double(), masks), d_head.mc_forward_torch(x.double(), masks))
        xt = x.transpose(2, 3)
        assert not xt.is_contiguous() and not head.hip_ok(xt) and same(head.mc_forward(xt, masks), head.mc_forward_torch(xt, masks))
        with pytest.raises(RuntimeError):
            head.mc_forward_hip(xt, masks)                          # the HIP path itself never falls back
        # three FC layers
        h3 = FCExtractorMonteCarlo(num_samples=3, in_channels=5, roi_feat_size=3, fc_out_channels=70, latent_channels=3, num_classes=2, num_fcs=3,
                                   dim_coder=dict(type='MultiClassNormDimCoder')).to(DEV).eval()
        assert not h3.hip_ok(x) and same(h3.mc_forward(x, masks), h3.mc_forward_torch(x, masks))
        # n = 0
        e = head.mc_forward(x[:0], return_samples=True)
        assert e[0].shape == (0, head.out_channels) and e[1].shape == (0, head.out_channels) and e[4].shape == (0, 70) and e[5].shape == (3, 0, head.out_channels)
    # a graph to keep: the torch path, and the gradient arrives
    xg = x.clone().requires_grad_(True)
    assert not head.hip_ok(xg)
    out = head.mc_forward(xg, masks)
    assert out[0].requires_grad
    out[0].sum().backward()
    assert xg.grad is not None and bool(torch.isfinite(xg.grad).all())
    with torch.no_grad():
        assert head.hip_ok(xg)                                      # under no_grad nothing requires a graph
    for p in head.parameters():
        p.requires_grad_(False)
    assert head.hip_ok(x)                                           # nothing requires grad: the HIP path, in grad mode too
    assert np.array_equal(head.mc_forward(x, masks)[0].cpu().numpy(), c.hip['mean'])
    for p in head.parameters():
        p.requires_grad_(True)


def test_outputs_compose_with_the_noc_decode_and_the_score_head():
    """dim / dim_var (after slice_pred) and reg_fc_out of forward go into noc_decode and score_poses as they are."""
    from monorun_amd.pose_head import noc_decode
    from monorun_amd.score_head import MLPScoreHead, score_poses
    n, classes, h, w = 4, 3, 8, 8
    head = _make_head(8, 3, 32, 4, classes, False, 6, seed=9).to(DEV)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(n, 8, 3, 3, generator=g).to(DEV)
    masks = [m.to(DEV) for m in head.draw_masks(n, 'cpu', generator=g)]
    labels = torch.tensor([0, 2, 1, 2], device=DEV)
    all_pred = torch.randn(n, 2 * classes * 5, h, w, generator=g).to(DEV)
    rois = torch.tensor([[10., 20, 90, 80], [100, 50, 180, 120], [300, 100, 340, 160], [500, 120, 620, 200]], device=DEV)
    score_head = MLPScoreHead(reg_fc_out_channels=32, pose_fc_out_channels=32, fc_out_channels=16).to(DEV).eval()
    score_head.init_weights()
    a = torch.randn(n, 4, 4, generator=g)
    pose = dict(ret_val=torch.tensor([True, True, False, True], device=DEV), yaw_pred=torch.randn(n, 1, generator=g).to(DEV),
                t_vec_pred=(torch.randn(n, 3, generator=g) + torch.tensor([0., 1.5, 20.])).to(DEV), pose_cov_calib=(a @ a.transpose(1, 2)).to(DEV))
    det = torch.rand(n, generator=g).to(DEV)
    results = []
    with torch.no_grad():
        for fwd in (head.mc_forward, head.mc_forward_torch):
            mean, var, _, _, reg = fwd(x, masks)
            dim, dim_var, latent, latent_var = head.slice_pred(mean, var, labels)
            for t in (dim, dim_var, reg):
                assert t.dtype == torch.float32 and t.device.type == 'cuda'
            assert dim.shape == (n, 3) and dim_var.shape == (n, 3) and latent.shape == (n, 4) and latent_var.shape == (n, 4) and reg.is_contiguous()
            dec = noc_decode(all_pred, labels, False, dim, dim_var, rois, num_classes=classes)
            dimensions, _ = head.dim_coder.decode(dim, dim_var, labels)
            scores = score_poses(score_head, reg, dict(pose, dimensions_pred=dimensions), det_scores=det)
            results.append((dec, scores))
    (dec_h, s_h), (dec_t, s_t) = results
    # the two paths' dim / dim_var / reg_fc_out differ by fp32 rounding (a few 1e-6 relative); the decode and the score head are smooth
    # in them, so their outputs agree to the tolerance their own tests use against fp32 torch restatements (1e-4 relative)
    for key in ('coords_3d', 'coords_2d_istd', 'dims', 'dims_var', 'coords_2d'):
        torch.testing.assert_close(dec_h[key], dec_t[key], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(s_h, s_t, rtol=1e-4, atol=1e-6)
    assert float(s_h[2]) == 0.0
