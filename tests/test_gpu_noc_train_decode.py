"""The NOC head's training decode on the MI355X: the forward bit for bit against the reference's values (G17, G3), against
K2 and against a numpy restatement with the specified exp / log; the backward against G17's gradients and an fp64 autograd of the torch
restatement; every channel of grad_all_pred written; shapes, dtypes, layouts, NULL upstream gradients, determinism; and one training
step of the NOC head through the projection loss and the differentiable PnP."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import noc_train_ref as ntr  # noqa: E402
from oracle import oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
EXACT = ('noc_pred', 'proj_logstd', 'coords_3d', 'coords_3d_var', 'dims', 'dims_var')


def _api():
    from monorun_amd.noc_head import decode_for_training, decode_for_training_torch
    return decode_for_training, decode_for_training_torch


@pytest.fixture(scope='module')
def g17():
    return ntr.load_g17()


def _np(t):
    return t.detach().cpu().numpy()


def _inputs(n, h, w, agnostic, with_var, with_dist, seed, C=3):
    """labels and flips cycle through every (label, flip) pair; one distance below distance_min"""
    rng = np.random.default_rng(seed)
    cn = 1 if agnostic else C
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    dist = rng.uniform(3, 80, (n, 1)).astype(np.float32)
    dist[n // 2] = 0.03
    return dict(all_pred=T(rng.normal(0, 1, (n, 2 * cn * 5, h, w)).astype(np.float32)), labels=T(np.arange(n) % C),
                flip=T((np.arange(n) // C) % 2 == 1), dim=T(rng.normal(0, 1, (n, 3)).astype(np.float32)),
                dim_var=T((rng.uniform(0.01, 0.2, (n, 3)) ** 2).astype(np.float32)) if with_var else None,
                distances=T(dist) if with_dist else None), dict(num_classes=C, class_agnostic=agnostic)


def _ups(out, seed):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return {k: torch.randn(v.shape, generator=g).to(DEV) for k, v in out.items() if v is not None}


def _f64(ins):
    return {k: v.double() if v is not None and v.is_floating_point() else v for k, v in ins.items()}


def _check_forward(out, ins, kw):
    """the maps and dims bit for bit what torch's unfused fp32 ops give; the pixel log-std bit for bit the numpy restatement"""
    _, torch_fn = _api()
    ref = torch_fn(ins['all_pred'].float(), ins['labels'], ins['flip'], ins['dim'], ins['dim_var'], ins['distances'], **kw)
    for k in EXACT:
        if ref[k] is None:
            assert out[k] is None, k
        else:
            assert out[k].dtype == torch.float32 and out[k].is_contiguous() and torch.equal(out[k], ref[k]), k
    var = _np(out['coords_3d_var']) if out['coords_3d_var'] is not None else None
    dist = _np(ins['distances']) if ins['distances'] is not None else None
    assert np.array_equal(_np(out['proj_logstd_px']), ntr.spec_logstd_px(_np(out['proj_logstd']), var, dist), equal_nan=True)


def _check_backward(ins, kw, seed):
    hip_fn, torch_fn = _api()
    out, grads = ntr.run(hip_fn, ins, kw, None)
    ups = _ups(out, seed)
    _, grads = ntr.run(hip_fn, ins, kw, ups)
    _, ref = ntr.run(torch_fn, _f64(ins), kw, {k: v.double() for k, v in ups.items()})
    for k, g in grads.items():
        assert g.dtype == ins[k[5:]].dtype and g.shape == ins[k[5:]].shape
        err = ntr.grad_err(g, ref[k])
        print(f'{k}: {err:.3g} of the largest element (bound {ntr.GRAD_TOL:.3g})')
        assert err <= ntr.GRAD_TOL, (k, err)
    return grads


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize('tag', ['a', 'b'])
def test_forward_against_g17_and_k2(g17, tag):
    from monorun_amd.pose_head import noc_decode
    hip_fn, _ = _api()
    ins, kw, _, want = ntr.group(g17, tag, DEV)
    out, _ = ntr.run(hip_fn, ins, kw)
    for k in EXACT:
        if want[k] is None:
            assert out[k] is None, k
        else:
            assert np.array_equal(_np(out[k]), want[k]), k
    _check_forward(out, ins, kw)
    np.testing.assert_allclose(_np(out['proj_logstd_px']), want['proj_logstd_px'], rtol=ntr.RTOL_EXP_LOG)
    n = ins['dim'].shape[0]
    rois = torch.tensor([[10.0, 20.0, 90.0, 70.0]], device=DEV).repeat(n, 1)
    k2 = noc_decode(ins['all_pred'], ins['labels'], ins['flip'], ins['dim'], ins['dim_var'], rois, **kw)
    assert torch.equal(out['coords_3d'], k2['coords_3d']) and torch.equal(out['dims'], k2['dims'])
    if ins['dim_var'] is not None:
        assert torch.equal(out['dims_var'], k2['dims_var'])


def test_forward_against_g3_and_k2_istd(g3):
    from monorun_amd.pose_head import noc_decode
    hip_fn, _ = _api()
    T = lambda a: torch.from_numpy(a).to(DEV)
    args = (T(g3['all_pred']), T(g3['labels']), T(g3['flip']), T(g3['dim']))
    out = hip_fn(*args, T(g3['dim_var']), None)
    for mine, theirs in (('coords_3d', 'c3d'), ('coords_3d_var', 'c3d_var'), ('dims', 'dims'), ('dims_var', 'dims_var'), ('noc_pred', 'noc_pred'),
                         ('proj_logstd', 'proj_logstd')):
        assert np.array_equal(_np(out[mine]), g3[theirs]), mine
    rois = torch.tensor([[10.0, 20.0, 90.0, 70.0]], device=DEV).repeat(8, 1)
    k2 = noc_decode(*args, T(g3['dim_var']), rois, std_scale=10)
    assert torch.equal(out['coords_3d'], k2['coords_3d']) and torch.equal(out['dims'], k2['dims']) and torch.equal(out['dims_var'], k2['dims_var'])
    # distances=None with variance: K2's inverse std is exp(-proj_logstd_px) / std_scale, bit for bit
    assert np.array_equal(orc.spec_expf(-_np(out['proj_logstd_px'])) / np.float32(10), _np(k2['coords_2d_istd']))
    np.testing.assert_allclose(np.exp(-_np(out['proj_logstd_px'])), np.exp(-g3['logstd_px']), rtol=ntr.RTOL_EXP_LOG)
    nv = hip_fn(*args, None, None)
    assert nv['coords_3d_var'] is None and nv['dims_var'] is None and np.array_equal(_np(nv['coords_3d']), g3['c3d'])
    assert np.array_equal(_np(nv['proj_logstd_px']), g3['logstd_px_novar'])
    ag = hip_fn(T(g3['all_pred'][:, :10].copy()), *args[1:], None, None, class_agnostic=True)
    assert np.array_equal(_np(ag['noc_pred']), g3['noc_agnostic']) and np.array_equal(_np(ag['proj_logstd']), g3['logstd_agnostic'])


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize('tag', ['a', 'b'])
def test_backward_against_g17(g17, tag):
    hip_fn, _ = _api()
    ins, kw, ups, want = ntr.group(g17, tag, DEV)
    _, grads = ntr.run(hip_fn, ins, kw, ups)
    for k, g in grads.items():
        err = ntr.grad_err(g, want[k])
        print(f'G17 {tag} {k}: {err:.3g} of the largest element (bound {ntr.GRAD_TOL:.3g})')
        assert err <= ntr.GRAD_TOL, (k, err)
    assert np.array_equal(_np(grads['grad_all_pred']) == 0, want['grad_all_pred'] == 0)


@pytest.mark.parametrize('agnostic', [False, True])
@pytest.mark.parametrize('h,w', [(28, 28), (7, 9), (56, 56), (1, 1)])
@pytest.mark.parametrize('n', [1, 3, 65])
def test_shapes(n, h, w, agnostic):
    """28x28 = 3 x 256 + 16 is ragged against the workgroup, 7x9 less than a wave, 56x56 several trips of the backward's loop, 1x1 one lane;
    n = 65 holds every (label, flip) pair; with and without dim_var and distances"""
    hip_fn, _ = _api()
    for i, (with_var, with_dist) in enumerate(((True, True), (True, False), (False, True), (False, False))):
        ins, kw = _inputs(n, h, w, agnostic, with_var, with_dist, seed=100 * n + h + i)
        out, _ = ntr.run(hip_fn, ins, kw)
        _check_forward(out, ins, kw)
        grads = _check_backward(ins, kw, seed=n + i)
        # exactly the selected channels carry a gradient
        cn = 1 if agnostic else 3
        lab = _np(ins['labels']) * (0 if agnostic else 1)
        f = _np(ins['flip']).astype(int)
        sel = np.zeros((n, 10 * cn), bool)
        for b in range(n):
            sel[b, f[b] * 5 * cn + 3 * lab[b]: f[b] * 5 * cn + 3 * lab[b] + 3] = True
            sel[b, f[b] * 5 * cn + 3 * cn + 2 * lab[b]: f[b] * 5 * cn + 3 * cn + 2 * lab[b] + 2] = True
        ga = _np(grads['grad_all_pred'])
        assert np.all(ga[~sel] == 0) and np.all(np.abs(ga[sel]).reshape(n, 5, -1).max(-1) > 0)


def test_unselected_channels_are_written(g17):
    """the raw entry point on a NaN-filled grad_all_pred: every unselected channel exactly 0.0, every selected one finite"""
    from monorun_amd import _lib
    from monorun_amd.pose_head import DIM_MEANS, DIM_STDS, NOC_MEANS, NOC_STDS, _const
    ins, kw, ups, want = ntr.group(g17, 'a', DEV)
    n, ch, h, w = ins['all_pred'].shape
    ga = torch.full_like(ins['all_pred'], float('nan'))
    gd, gv = torch.full((n, 3), float('nan'), device=DEV), torch.full((n, 3), float('nan'), device=DEV)
    flip = ins['flip'].to(torch.uint8)
    consts = [_const(v, DEV) for v in (DIM_MEANS, DIM_STDS, NOC_MEANS, NOC_STDS)]
    args = _lib.pack('mr_noc_decode_train_backward', all_pred=ins['all_pred'].data_ptr(), pred_dtype=_lib.MR_F32, labels=ins['labels'].data_ptr(),
                     flip=flip.data_ptr(), dim=ins['dim'].data_ptr(), dim_var=ins['dim_var'].data_ptr(), n=n, num_classes=3, class_agnostic=0, h=h, w=w,
                     dim_means=consts[0].data_ptr(), dim_stds=consts[1].data_ptr(), noc_means=consts[2].data_ptr(), noc_stds=consts[3].data_ptr(),
                     proj_scaling_denominator=1.6 * 722 * 0.15, ref_focal_y=722.0, epistemic_std_gain=1.0,
                     grad_all_pred=ga.data_ptr(), grad_dim=gd.data_ptr(), grad_dim_var=gv.data_ptr(),
                     **{'grad_' + k: ups[k].data_ptr() for k in ntr.OUTPUTS})
    _lib.check(_lib.load().mr_noc_decode_train_backward(*args, torch.cuda.current_stream(DEV).cuda_stream))
    torch.cuda.synchronize()
    sel = want['grad_all_pred'] != 0
    got = _np(ga)
    assert np.all(got[~sel.any((2, 3))] == 0.0) and not np.signbit(got[~sel.any((2, 3))]).any()
    assert np.isfinite(got[sel.any((2, 3))]).all() and np.isfinite(_np(gd)).all() and np.isfinite(_np(gv)).all()
    assert ntr.grad_err(ga, want['grad_all_pred']) <= ntr.GRAD_TOL and ntr.grad_err(gd, want['grad_dim']) <= ntr.GRAD_TOL
    # argument errors: NULL required output; an unknown dtype
    lib = _lib.load()
    bad = list(args); bad[_lib.arg_names('mr_noc_decode_train_backward').index('grad_dim')] = None
    assert lib.mr_pnp_error_string(lib.mr_noc_decode_train_backward(*bad, None)) == b'bad argument'
    bad = list(args); bad[1] = _lib.MR_F64
    assert lib.mr_noc_decode_train_backward(*bad, None) != 0


# ------------------------------------------------------------------------------------------------ dtypes, layouts, edge cases
@pytest.mark.parametrize('dtype,eps', [(torch.float16, 2.0 ** -11), (torch.bfloat16, 2.0 ** -8)])
def test_half_all_pred(dtype, eps):
    """read as is, decoded in fp32: the forward equals the restatement on the upcast input; grad_all_pred comes back in the input's dtype,
    rounded once (relative eps of the format, half an ulp of its smallest normal below that) from a gradient within the fp32 bound"""
    hip_fn, torch_fn = _api()
    ins, kw = _inputs(5, 28, 28, False, True, True, seed=5)
    ins['all_pred'] = ins['all_pred'].to(dtype)
    out, _ = ntr.run(hip_fn, ins, kw)
    up = dict(ins, all_pred=ins['all_pred'].float())
    _check_forward(out, up, kw)
    ups = _ups(out, 6)
    _, grads = ntr.run(hip_fn, ins, kw, ups)
    _, ref = ntr.run(torch_fn, _f64(up), kw, {k: v.double() for k, v in ups.items()})
    assert grads['grad_all_pred'].dtype == dtype and grads['grad_dim'].dtype == torch.float32
    g, r = grads['grad_all_pred'].double(), ref['grad_all_pred']
    tiny = 2.0 ** -15 if dtype == torch.float16 else 0.0
    assert bool(((g - r).abs() <= ntr.GRAD_TOL * r.abs().max() + eps * r.abs() + eps * tiny).all())
    assert ntr.grad_err(grads['grad_dim'], ref['grad_dim']) <= ntr.GRAD_TOL and ntr.grad_err(grads['grad_dim_var'], ref['grad_dim_var']) <= ntr.GRAD_TOL


def test_other_dtypes_and_layouts():
    hip_fn, torch_fn = _api()
    ins, kw = _inputs(4, 7, 9, False, True, True, seed=9)
    ref_out, _ = ntr.run(hip_fn, ins, kw)
    ups = _ups(ref_out, 10)
    _, ref_g = ntr.run(hip_fn, ins, kw, ups)
    # a non-contiguous all_pred (channels-last memory) and dim (a column slice): copied differentiably
    nc = dict(ins, all_pred=ins['all_pred'].to(memory_format=torch.channels_last))
    nc['dim'] = torch.cat([ins['dim'][:, :1], ins['dim']], 1)[:, 1:]
    assert not nc['all_pred'].is_contiguous() and not nc['dim'].is_contiguous()
    ap = nc['all_pred'].detach().requires_grad_(True)
    out = hip_fn(ap, nc['labels'], nc['flip'], nc['dim'], nc['dim_var'], nc['distances'], **kw)
    assert all(torch.equal(out[k], ref_out[k]) for k in ref_out)
    sum((out[k] * ups[k]).sum() for k in ups).backward()
    assert torch.equal(ap.grad, ref_g['grad_all_pred'])
    # fp64 everywhere: cast to fp32 differentiably, outputs and gradients back in fp64
    d = _f64(ins)
    out64, g64 = ntr.run(hip_fn, d, kw, {k: v.double() for k, v in ups.items()})
    assert all(v.dtype == torch.float64 for v in out64.values()) and all(g.dtype == torch.float64 for g in g64.values())
    assert torch.equal(out64['coords_3d'], ref_out['coords_3d'].double()) and torch.equal(g64['grad_dim'], ref_g['grad_dim'].double())
    # distances that require grad: the torch restatement, which gives them one
    dist = ins['distances'].clone().requires_grad_(True)
    out = hip_fn(ins['all_pred'], ins['labels'], ins['flip'], ins['dim'], ins['dim_var'], dist, **kw)
    out['proj_logstd_px'].sum().backward()
    assert dist.grad is not None and float(dist.grad.abs().max()) > 0
    # a bool flip and a (n,) distance
    one = hip_fn(ins['all_pred'], ins['labels'], True, ins['dim'], ins['dim_var'], ins['distances'].reshape(-1), **kw)
    two = torch_fn(ins['all_pred'], ins['labels'], True, ins['dim'], ins['dim_var'], ins['distances'], **kw)
    assert torch.equal(one['coords_3d'], two['coords_3d']) and torch.equal(one['noc_pred'], two['noc_pred'])


def test_no_objects_no_launch():
    hip_fn, _ = _api()
    ap = torch.zeros(0, 30, 28, 28, device=DEV, requires_grad=True)
    dim = torch.zeros(0, 3, device=DEV, requires_grad=True)
    dv = torch.zeros(0, 3, device=DEV, requires_grad=True)
    out = hip_fn(ap, torch.zeros(0, dtype=torch.long, device=DEV), False, dim, dv, torch.zeros(0, 1, device=DEV))
    assert out['coords_3d'].shape == (0, 3, 28, 28) and out['proj_logstd_px'].shape == (0, 2, 28, 28) and out['dims_var'].shape == (0, 3)
    assert all(v.grad_fn is not None and 'DecodeFunction' not in type(v.grad_fn).__name__ for v in out.values())      # torch ops: no launch of ours
    sum(v.sum() for v in out.values()).backward()
    assert ap.grad.shape == ap.shape and dim.grad.shape == (0, 3) and dv.grad.shape == (0, 3)


@pytest.mark.parametrize('only', ['coords_3d', 'proj_logstd_px'])
def test_null_upstream_gradients(only):
    """a loss that uses one output: the others reach the kernel as NULL"""
    hip_fn, torch_fn = _api()
    ins, kw = _inputs(7, 28, 28, False, True, True, seed=12)
    out, _ = ntr.run(hip_fn, ins, kw)
    ups = {only: _ups(out, 13)[only]}
    _, grads = ntr.run(hip_fn, ins, kw, ups)
    _, ref = ntr.run(torch_fn, _f64(ins), kw, {only: ups[only].double()})
    for k in grads:
        if float(ref[k].abs().max()) == 0:
            assert float(grads[k].abs().max()) == 0, k                 # (coords_3d alone gives dim_var nothing)
        else:
            assert ntr.grad_err(grads[k], ref[k]) <= ntr.GRAD_TOL, k


def test_determinism():
    hip_fn, _ = _api()
    ins, kw = _inputs(65, 28, 28, False, True, True, seed=21)
    runs = []
    for _ in range(2):
        out, _ = ntr.run(hip_fn, ins, kw)
        _, grads = ntr.run(hip_fn, ins, kw, _ups(out, 22))
        runs.append(list(out.values()) + list(grads.values()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_backward_under_create_graph():
    """create_graph=True: the gradients come from the torch restatement and carry a graph"""
    hip_fn, torch_fn = _api()
    ins, kw = _inputs(3, 7, 9, False, True, True, seed=30)
    res = []
    for fn in (hip_fn, torch_fn):
        ap = ins['all_pred'].clone().requires_grad_(True)
        out = fn(ap, ins['labels'], ins['flip'], ins['dim'], ins['dim_var'], ins['distances'], **kw)
        g, = torch.autograd.grad(out['proj_logstd_px'].square().sum(), ap, create_graph=True)
        gg, = torch.autograd.grad(g.square().sum(), ap)
        res.append((g.detach(), gg))
    assert ntr.grad_err(res[0][0], res[1][0]) <= 1e-5 and ntr.grad_err(res[0][1], res[1][1]) <= 1e-5


# ------------------------------------------------------------------------------------------------ one training step
def _training_step(fn, b, seed=0):
    from monorun_amd import synthetic as syn
    from monorun_amd.pose_head import DIM_MEANS, DIM_STDS, NOC_MEANS, NOC_STDS, UncertPropPnPOptimizer, roi_align_avg
    from monorun_amd.projection_head import UncertProjectionHead
    B = len(b['dims'])
    rng = np.random.default_rng(seed)
    labels = np.arange(B) % 3
    flip = (np.arange(B) // 3) % 2 == 1
    dims = np.asarray(b['dims'], np.float32)
    noc = (b['coords_3d'] / dims[:, :, None, None] - np.asarray(NOC_MEANS, np.float32)[:, None, None]) / np.asarray(NOC_STDS, np.float32)[:, None, None]
    all_pred = rng.normal(0, 1, (B, 30, 28, 28)).astype(np.float32)
    sel = np.zeros((B, 30), bool)
    for i in range(B):
        c0, l0 = flip[i] * 15 + 3 * labels[i], flip[i] * 15 + 9 + 2 * labels[i]
        all_pred[i, c0:c0 + 3], all_pred[i, l0:l0 + 2] = noc[i], b['logstd'][i]
        sel[i, c0:c0 + 3] = sel[i, l0:l0 + 2] = True
    dim = (dims - np.asarray(DIM_MEANS, np.float32)[labels]) / np.asarray(DIM_STDS, np.float32)[labels]
    T = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).to(DEV)
    all_pred, dim = T(all_pred).requires_grad_(True), T(dim).requires_grad_(True)
    K1, img1 = T(b['K']), T(b['img_shape'])
    K, img = K1.expand(B, 3, 3).contiguous(), img1.expand(B, 2).contiguous()
    gt = T(np.concatenate([b['dims'], b['gt_t'], b['gt_yaw'][:, None]], 1))
    rois = T(np.concatenate([np.zeros((B, 1)), b['rois']], 1))
    coord_map = torch.stack(torch.meshgrid(torch.arange(syn.IMG_W, device=DEV, dtype=torch.float32),
                                           torch.arange(syn.IMG_H, device=DEV, dtype=torch.float32), indexing='xy'), 0)[None]
    roi_grid = roi_align_avg(coord_map, rois, (28, 28))
    head = UncertProjectionHead().to(DEV)
    dist = torch.norm(gt[:, 3:6], dim=1, keepdim=True)
    dec = fn(all_pred, torch.from_numpy(labels).to(DEV), torch.from_numpy(flip).to(DEV), dim, None, dist)
    proj = head(dec['coords_3d'], gt[:, 3:7], K, img)
    loss_proj = head.loss(proj, dec['proj_logstd'], roi_grid, dist)['loss_proj']
    cfg = dict(type='PnPUncert', z_min=0.5, epnp_istd_thres=0.6, inlier_opt_only=True, forward_exact_hessian=False, differentiable=True)
    pose_head = UncertPropPnPOptimizer(pnp=cfg, loss_calib=dict(type='KLLossMV', loss_weight=0.01)).to(DEV)
    ret, yaw, t, cov, cov_calib = pose_head(roi_grid, dec['proj_logstd_px'], dec['coords_3d'], K1, img1)
    yt, tt = pose_head.get_targets(gt)
    losses, _ = pose_head.loss(ret, yaw, t, cov_calib, dec['dims'], yt, tt, gt)
    (loss_proj + losses['loss_calib']).backward()
    return all_pred.grad, dim.grad, sel, ret


def test_training_step_of_the_noc_head_through_the_decode():
    """The scenario of test_gpu_projection_loss.py::test_training_step_of_the_noc_head from a leaf all_pred of 30 channels with mixed labels
    and flips and a leaf dim: decode_for_training -> UncertProjectionHead + loss_proj with the ground-truth poses on the roi_align_avg grid ->
    proj_logstd_px into the differentiable pose head -> loss_proj + loss_calib backpropagated."""
    from monorun_amd import synthetic as syn
    hip_fn, torch_fn = _api()
    b = syn.make_batch(B=64, seed=41)
    ga, gd, sel, ret = _training_step(hip_fn, b)
    assert int(ret.sum()) >= 32
    assert bool(torch.isfinite(ga).all()) and bool(torch.isfinite(gd).all()) and float(gd.abs().max()) > 0
    g = _np(ga)
    assert np.all(g[~sel] == 0) and np.all(np.abs(g[sel]).reshape(64, 5, -1).max(-1) > 0)
    ta, td, _, _ = _training_step(torch_fn, b)
    ea, ed = ntr.grad_err(ga, ta), ntr.grad_err(gd, td)
    print(f'training step, HIP decode against torch decode: all_pred.grad {ea:.3g}, dim.grad {ed:.3g} of the largest element (bound {ntr.GRAD_TOL:.3g})')
    assert ea <= ntr.GRAD_TOL and ed <= ntr.GRAD_TOL, (ea, ed)
