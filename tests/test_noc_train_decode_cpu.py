"""The training decode without a GPU: the torch restatement against the reference's values and gradients (G17, G3),
its fp64 gradcheck, the edge forms of its arguments, the dispatcher on CPU tensors, and the new entry points in the built library."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import noc_train_ref as ntr  # noqa: E402

from monorun_amd import _lib  # noqa: E402
from monorun_amd.noc_head import decode_for_training, decode_for_training_torch  # noqa: E402

EXACT = ('noc_pred', 'proj_logstd', 'coords_3d', 'coords_3d_var', 'dims', 'dims_var')


@pytest.fixture(scope='module')
def g17():
    return ntr.load_g17()


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_restatement_against_g17(g17, tag):
    ins, kw, ups, want = ntr.group(g17, tag)
    out, grads = ntr.run(decode_for_training_torch, ins, kw, ups)
    for k in EXACT:
        if want[k] is None:
            assert out[k] is None, k
        else:
            assert np.array_equal(out[k].detach().numpy(), want[k]), k                # the same unfused fp32 chain
    np.testing.assert_allclose(out['proj_logstd_px'].detach().numpy(), want['proj_logstd_px'], rtol=ntr.RTOL_EXP_LOG)
    for k, g in grads.items():
        err = ntr.grad_err(g, want[k])
        print(f'G17 {tag} {k}: {err:.3g}')
        assert err <= ntr.GRAD_TOL, (k, err)
    # flip, labels and distances get no gradient; the unselected channels an exact zero
    ga = grads['grad_all_pred'].numpy()
    assert np.array_equal(ga == 0, want['grad_all_pred'] == 0)


def test_fp32_autograd_against_fp64_on_g17(g17):
    """The measurement behind noc_train_ref.GRAD_TOL: fp32 against fp64 autograd of the same restatement."""
    worst = 0.0
    for tag in ('a', 'b'):
        ins, kw, ups, _ = ntr.group(g17, tag)
        _, g32 = ntr.run(decode_for_training_torch, ins, kw, ups)
        ins64, _, ups64, _ = ntr.group(g17, tag, dtype=torch.float64)
        _, g64 = ntr.run(decode_for_training_torch, ins64, kw, ups64)
        for k in g32:
            err = ntr.grad_err(g32[k], g64[k])
            print(f'fp32 vs fp64 autograd, G17 {tag} {k}: {err:.3g}')
            worst = max(worst, err)
    assert 0.5 * ntr.GRAD_FP32_DEVIATION <= worst <= ntr.GRAD_FP32_DEVIATION * 1.001, worst      # the constant is what is measured here


def test_restatement_against_g3(g3):
    T = torch.from_numpy
    args = (T(g3['all_pred']), T(g3['labels']), T(g3['flip']), T(g3['dim']))
    out = decode_for_training_torch(*args, T(g3['dim_var']), None)
    assert np.array_equal(out['coords_3d'].numpy(), g3['c3d']) and np.array_equal(out['coords_3d_var'].numpy(), g3['c3d_var'])
    assert np.array_equal(out['noc_pred'].numpy(), g3['noc_pred']) and np.array_equal(out['proj_logstd'].numpy(), g3['proj_logstd'])
    assert np.array_equal(out['dims'].numpy(), g3['dims']) and np.array_equal(out['dims_var'].numpy(), g3['dims_var'])
    np.testing.assert_allclose(out['proj_logstd_px'].numpy(), g3['logstd_px'], rtol=ntr.RTOL_EXP_LOG)
    nv = decode_for_training_torch(*args, None, None)
    assert nv['coords_3d_var'] is None and nv['dims_var'] is None
    assert np.array_equal(nv['coords_3d'].numpy(), g3['c3d'])
    np.testing.assert_allclose(nv['proj_logstd_px'].numpy(), g3['logstd_px_novar'], rtol=ntr.RTOL_EXP_LOG)
    ag = decode_for_training_torch(T(g3['all_pred'][:, :10].copy()), *args[1:], None, None, class_agnostic=True)
    assert np.array_equal(ag['noc_pred'].numpy(), g3['noc_agnostic']) and np.array_equal(ag['proj_logstd'].numpy(), g3['logstd_agnostic'])


def test_numpy_restatement_of_the_pixel_logstd(g17, g3):
    """tests' own spec_logstd_px (the GPU test's bit-exact reference) agrees with the reference's values to the exp / log tolerance"""
    a = {k[2:]: v for k, v in g17.items() if k.startswith('a_')}
    np.testing.assert_allclose(ntr.spec_logstd_px(a['proj_logstd'], a['coords_3d_var'], a['distances']), a['proj_logstd_px'], rtol=ntr.RTOL_EXP_LOG)
    b = {k[2:]: v for k, v in g17.items() if k.startswith('b_')}
    assert np.array_equal(ntr.spec_logstd_px(b['proj_logstd'], None, None), b['proj_logstd_px'])          # ls + log(1)
    # G3 holds log-stds next to 0, where a relative bound on the logarithm itself means nothing: compared as the inverse std, as G3's own test does
    np.testing.assert_allclose(np.exp(-ntr.spec_logstd_px(g3['proj_logstd'], g3['c3d_var'], None)), np.exp(-g3['logstd_px']), rtol=ntr.RTOL_EXP_LOG)
    np.testing.assert_allclose(ntr.spec_logstd_px(a['proj_logstd'], None, a['distances']),
                               a['proj_logstd'] + np.log(np.float32(173.28) / np.maximum(a['distances'], np.float32(0.1)))[:, :, None, None],
                               rtol=ntr.RTOL_EXP_LOG, atol=1e-6)


@pytest.mark.parametrize('with_var,with_dist', [(True, True), (True, False), (False, True), (False, False)])
def test_gradcheck_fp64(with_var, with_dist):
    rng = np.random.default_rng(3)
    n, h, w = 2, 3, 4
    ap = torch.tensor(rng.normal(0, 1, (n, 30, h, w)), requires_grad=True)
    dim = torch.tensor(rng.normal(0, 1, (n, 3)), requires_grad=True)
    dv = torch.tensor(rng.uniform(0.01, 0.2, (n, 3)) ** 2, requires_grad=True) if with_var else None
    dist = torch.tensor([[7.5], [0.02]], dtype=torch.float64) if with_dist else None
    labels, flip = torch.tensor([2, 0]), torch.tensor([True, False])
    leaves = [t for t in (ap, dim, dv) if t is not None]

    def f(*xs):
        xs = list(xs) + [None]
        out = decode_for_training_torch(xs[0], labels, flip, xs[1], xs[2], dist)
        return tuple(v for v in out.values() if v is not None)

    assert torch.autograd.gradcheck(f, leaves, eps=1e-6, atol=1e-7, rtol=1e-5)


def test_no_objects():
    ap = torch.zeros(0, 30, 28, 28, requires_grad=True)
    dim = torch.zeros(0, 3, requires_grad=True)
    dv = torch.zeros(0, 3, requires_grad=True)
    for fn in (decode_for_training_torch, decode_for_training):
        out = fn(ap, torch.zeros(0, dtype=torch.long), False, dim, dv, torch.zeros(0, 1))
        assert out['coords_3d'].shape == (0, 3, 28, 28) and out['proj_logstd_px'].shape == (0, 2, 28, 28) and out['dims'].shape == (0, 3)
        ap.grad = dim.grad = dv.grad = None
        sum(v.sum() for v in out.values()).backward()
        assert ap.grad.shape == ap.shape and dim.grad.shape == (0, 3) and dv.grad.shape == (0, 3)


def test_flip_forms_and_dispatch_on_cpu(g17):
    ins, kw, _, _ = ntr.group(g17, 'a')
    a = (ins['all_pred'], ins['labels'])
    rest = (ins['dim'], ins['dim_var'], ins['distances'])
    for flag in (False, True):
        one = decode_for_training_torch(*a, flag, *rest, **kw)
        for form in (torch.full((6,), flag), [flag] * 6, np.bool_(flag), torch.tensor(flag)):
            other = decode_for_training_torch(*a, form, *rest, **kw)
            assert all(torch.equal(one[k], other[k]) for k in one), (flag, type(form))
        want = ins['all_pred'].view(6, 2, 15, 28, 28)[torch.arange(6), int(flag)][:, :9].reshape(6, 3, 3, 28, 28)
        assert torch.equal(one['noc_pred'], want[torch.arange(6), ins['labels']])
    # CPU tensors: the dispatcher is the restatement; half inputs are decoded in fp32
    mine = decode_for_training(*a, ins['flip'], *rest, **kw)
    ref = decode_for_training_torch(*a, ins['flip'], *rest, **kw)
    assert all(torch.equal(mine[k], ref[k]) for k in ref)
    half = decode_for_training(ins['all_pred'].half(), ins['labels'], ins['flip'], *rest, **kw)
    assert half['coords_3d'].dtype == torch.float32 and torch.equal(half['coords_3d'], ref['coords_3d'])      # G17's all_pred is fp16-exact
    nv = decode_for_training(*a, ins['flip'], ins['dim'], None, ins['distances'], **kw)
    assert nv['coords_3d_var'] is None and nv['dims_var'] is None


def test_symbols_exported_and_bound_by_name():
    """The training decode's own; test_capi_and_host.py::test_loader_binds_every_header has what holds for every header."""
    lib = _lib.load()
    for fn in ('mr_noc_decode_train', 'mr_noc_decode_train_backward'):
        f = getattr(lib, fn)
        names = _lib.arg_names(fn)
        assert len(f.argtypes) == len(names) + 1                                  # stream last, not among the names
        args = _lib.pack(fn, {k: 0 for k in names})
        assert len(args) == len(names)
        with pytest.raises(TypeError):
            _lib.pack(fn, {k: 0 for k in names}, rois=0)
    assert 'distances' in _lib.arg_names('mr_noc_decode_train') and 'distances' not in _lib.arg_names('mr_noc_decode_train_backward')
    # n = 0: success without a launch, before any pointer is looked at; argument errors need no device either
    fwd = _lib.pack('mr_noc_decode_train', {k: 0 for k in _lib.arg_names('mr_noc_decode_train')}, all_pred=None, num_classes=3, h=28, w=28)
    assert lib.mr_noc_decode_train(*fwd, None) == 0
    bwd = dict({k: 0 for k in _lib.arg_names('mr_noc_decode_train_backward')}, num_classes=3, h=28, w=28)
    assert lib.mr_noc_decode_train_backward(*_lib.pack('mr_noc_decode_train_backward', bwd), None) == 0
    for fn, common in (('mr_noc_decode_train', {k: 0 for k in _lib.arg_names('mr_noc_decode_train')}), ('mr_noc_decode_train_backward', bwd)):
        for bad in (dict(n=1, num_classes=3, h=28, w=28), dict(n=-1, num_classes=3, h=28, w=28), dict(n=1, num_classes=3, h=0, w=28)):      # NULL all_pred; n < 0; h w < 1
            code = getattr(lib, fn)(*_lib.pack(fn, common, **bad), None)
            assert code != 0 and lib.mr_pnp_error_string(code) == b'bad argument', (fn, bad, code)
