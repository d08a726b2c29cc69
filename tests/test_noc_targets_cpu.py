"""The NOC head's LiDAR supervision without a GPU: the torch restatements of NOCCoder.encode, masked_dense_target and
SmoothL1LossMod against G18 (recorded from the reference's own functions), the head's get_targets / loss, and the C ABI's fourth header."""
import types

import numpy as np
import pytest
import torch

from monorun_amd import _lib, noc_head, noc_targets as nt
from monorun_amd.losses import LOSSES, SmoothL1LossMod, build_loss, smooth_l1_loss_mod
from tests import noc_targets_ref as ref


def _bits(a, b):
    a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_encode_then_masked_dense_target_equal_g18_bit_for_bit(tag):
    ins, rec = ref.group(tag)
    enc = [nt.noc_encode(c, m, d, f) for c, m, d, f in zip(ins['coords'], ins['masks'], ins['dims'], ins['flips'])]
    for (e, em), m in zip(enc, ins['masks']):
        assert e.shape[1] == 3 and em.shape == m.shape
        assert torch.equal(em != 0, m >= np.float32(1e-5))               # 5e-6 is below the coder's eps, fp32(1e-5) is not
    t, w = nt.masked_dense_target(ins['pos_bboxes'], ins['gt_inds'], [e for e, _ in enc], [m for _, m in enc],
                                  types.SimpleNamespace(dense_size=ins['dense_size']))
    assert _bits(t, rec.targets)
    assert _bits(w, rec.weights)                                        # the normalised weights, exactly
    pos = w > 0
    assert 0 < int(pos.sum()) < w.numel() and torch.unique(w).numel() == 2


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_noc_targets_on_the_cpu_is_the_composed_path(tag):
    ins, rec = ref.group(tag)
    t, w = nt.noc_targets(*ref.call_args(ins))
    assert _bits(t, rec.targets) and _bits(w, rec.weights)
    assert not t.requires_grad and not w.requires_grad
    coder = noc_head.NOCCoder()
    t2, w2 = nt.noc_targets(*ref.call_args(ins), coord_coder=coder)
    assert _bits(t2, t) and _bits(w2, w)


def test_fixture_covers_what_it_says():
    ins, rec = ref.group('a')
    g = ref.g18()
    assert ins['coords'][0].shape == (3, 3, 40, 56) and ins['coords'][1].shape == (1, 3, 33, 47) and ins['flips'] == [False, True, False]
    assert ins['pos_bboxes'][2].shape == (0, 4) and ins['coords'][2].shape[0] == 2
    assert sorted(np.unique(g['a_img0_mask_index'])) == [0, 1, 2, 3, 4]
    assert (ins['dims'][0] < 1e-5).sum() == 1
    r0 = ins['pos_bboxes'][0]
    assert (r0[:, 2] == 56).any() and (r0[:, 0] < -1).any() and (r0[:, 1] < -1).any() and (r0[:, 2] > 57).any() and (r0[:, 3] > 41).any()
    per_roi = rec.weights.flatten(1).sum(1)
    assert (per_roi == 0).sum() >= 1                                     # the RoI over masked-out pixels
    assert ins['dense_size'] == (28, 28) and ref.group('b')[0]['dense_size'] == (7, 9)


def test_all_empty_batch_gives_the_reference_s_empty_tensors():
    ins, _ = ref.group('a')
    empty = [b[:0] for b in ins['pos_bboxes']]
    t, w = nt.noc_targets(empty, [g[:0] for g in ins['gt_inds']], *ref.call_args(ins)[2:])
    assert t.shape == (0, 3, 28, 28) and w.shape == (0, 1, 28, 28) and t.dtype == torch.float32


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_smooth_l1_mod_in_torch_equals_g18(tag):
    _, rec = ref.group(tag)
    lm = SmoothL1LossMod(beta=rec.beta, loss_weight=rec.loss_weight)
    pred = rec.noc_pred.clone().requires_grad_(True)
    loss = lm(pred, rec.targets, weight=rec.weights)
    assert np.float32(loss.item()) == np.float32(rec.loss_mean)
    loss.backward(torch.tensor(rec.upstream))
    assert _bits(pred.grad, rec.grad_pred)
    assert np.float32(lm(pred.detach(), rec.targets, weight=rec.weights, reduction_override='sum').item()) == np.float32(rec.loss_sum)
    # the deviation of the fp32 reduction from an fp64 one of the same terms: what the HIP loss's tolerance is taken from
    for reduction, recorded in (('mean', rec.loss_mean), ('sum', rec.loss_sum)):
        exact, dev = ref.loss_terms64(rec, reduction)
        print(f'G18 {tag} {reduction}: fp64 {exact!r} recorded {recorded!r} relative deviation of the fp32 reduction {dev:.3e}')
        assert abs(recorded - exact) <= (dev + 2.0 ** -23) * abs(exact)
        assert dev < 1e-5


def test_smooth_l1_mod_gradcheck_fp64():
    rng = np.random.default_rng(5)
    beta = 0.7
    d = rng.uniform(0.05, 2.0, (2, 3, 4, 5)) * rng.choice([-1, 1], (2, 3, 4, 5))
    d[np.abs(np.abs(d) - beta) < 0.02] = 0.3                            # away from the kink at |d| = beta and from d = 0
    target = torch.from_numpy(rng.normal(0, 1, d.shape))
    pred = (target + torch.from_numpy(d)).requires_grad_(True)
    weight = torch.from_numpy(rng.uniform(0, 2, (2, 1, 4, 5)))
    for reduction in ('mean', 'sum', 'none'):
        lm = SmoothL1LossMod(beta=beta, reduction=reduction, loss_weight=1.7)
        assert torch.autograd.gradcheck(lambda p: lm(p, target, weight=weight), (pred,), eps=1e-6, atol=1e-8)
    assert torch.autograd.gradcheck(lambda p: SmoothL1LossMod(beta=beta)(p, 0), (pred,), eps=1e-6, atol=1e-8)


def test_smooth_l1_mod_call_forms():
    rng = np.random.default_rng(6)
    pred = torch.from_numpy(rng.normal(0, 1.5, (3, 3, 4, 4)).astype(np.float32))
    target = torch.from_numpy(rng.normal(0, 1, (3, 3, 4, 4)).astype(np.float32))
    lm = SmoothL1LossMod(beta=0.5, loss_weight=2.0)
    d = (pred - target).abs()
    elem = torch.where(d < 0.5, 0.5 * d * d / 0.5, d - 0.25)
    assert torch.equal(lm(pred, target, reduction_override='none'), 2.0 * elem)
    assert torch.equal(lm(pred, target, avg_factor=7.0), 2.0 * (elem.sum() / 7.0))
    assert torch.equal(lm(pred - target, 0), lm(pred, target))           # target 0: pred is the error
    assert torch.equal(lm(d, -1), lm(pred, target))                      # target -1: pred is the non-negative distance
    with pytest.raises(ValueError):
        lm(pred, 3)
    with pytest.raises(ValueError):
        lm(pred, target, reduction_override='median')
    with pytest.raises(ValueError):
        lm(pred, target, avg_factor=2.0, reduction_override='sum')
    assert torch.equal(smooth_l1_loss_mod(pred, target, 0.5), elem)


def test_build_loss_builds_it():
    built = build_loss(dict(type='SmoothL1LossMod', loss_weight=1.0, beta=1.0))
    assert isinstance(built, SmoothL1LossMod) and LOSSES['SmoothL1LossMod'] is SmoothL1LossMod
    assert (built.beta, built.reduction, built.loss_weight) == (1.0, 'mean', 1.0)
    assert not list(built.parameters()) and not list(built.buffers())


def _sampling(ins):
    return [types.SimpleNamespace(pos_bboxes=b, pos_assigned_gt_inds=g) for b, g in zip(ins['pos_bboxes'], ins['gt_inds'])]


def test_head_get_targets_and_loss():
    ins, rec = ref.group('a')
    boxes = [torch.cat([d, torch.zeros(d.shape[0], 4)], 1) for d in ins['dims']]          # [l, h, w, x, y, z, yaw]
    metas = [dict(flip=f) for f in ins['flips']]
    cfg = types.SimpleNamespace(dense_size=28)
    t, w = noc_head.get_targets(_sampling(ins), ins['coords'], ins['masks'], boxes, cfg, metas, noc_head.NOCCoder())
    assert _bits(t, rec.targets) and _bits(w, rec.weights)
    t2, _ = noc_head.get_targets(_sampling(ins), ins['coords'], ins['masks'], boxes, dict(dense_size=(28, 28)), metas)
    assert _bits(t2, t)
    loss_noc = build_loss(dict(type='SmoothL1LossMod', loss_weight=rec.loss_weight, beta=rec.beta))
    out = noc_head.loss(rec.noc_pred, t, w, loss_noc)
    assert list(out) == ['loss_noc'] and np.float32(out['loss_noc'].item()) == np.float32(rec.loss_mean)
    assert noc_head.loss(rec.noc_pred, t, w, None) == {}


def test_head_all_empty_batch():
    ins, _ = ref.group('a')
    ins = dict(ins, pos_bboxes=[b[:0] for b in ins['pos_bboxes']], gt_inds=[g[:0] for g in ins['gt_inds']])
    boxes = [torch.cat([d, torch.zeros(d.shape[0], 4)], 1) for d in ins['dims']]
    t, w = noc_head.get_targets(_sampling(ins), ins['coords'], ins['masks'], boxes, dict(dense_size=28), [dict(flip=f) for f in ins['flips']])
    assert t.shape == (0, 3, 28, 28) and w.shape == (0, 1, 28, 28)
    pred = torch.zeros(0, 3, 28, 28, requires_grad=True)
    out = noc_head.loss(pred, t, w, SmoothL1LossMod())
    assert out['loss_noc'].item() == 0.0 and out['loss_noc'].requires_grad
    out['loss_noc'].backward()
    assert pred.grad.shape == pred.shape


def test_noc_coder_decode_inverts_encode():
    ins, _ = ref.group('b')
    coder = noc_head.NOCCoder()
    c, m, d = ins['coords'][0].double(), ins['masks'][0].double(), ins['dims'][0].double()
    enc, em = coder.encode(c, m, d, False)
    full = (m == 1.0).expand_as(c)
    dec, var = coder.decode(enc, None, d, None, False)
    assert var is None and torch.allclose(dec[full], c[full], atol=1e-12)


def test_noc_coder_decode_variance_against_the_closed_form():
    """coords_3d = p * dim with p = part * std + mean: var = var_p dim^2 + var_dim p^2 + var_p var_dim, var_p = part_var * std^2, in
    numpy fp64; with dimensions_var alone also the project's training decode (decode_for_training_torch)."""
    from monorun_amd.pose_head import DIM_MEANS, DIM_STDS, NOC_MEANS, NOC_STDS
    rng = np.random.default_rng(11)
    n, h, w = 3, 4, 5
    part, part_var = rng.normal(0, 1, (n, 3, h, w)), rng.uniform(0.01, 0.5, (n, 3, h, w))
    dim, dim_var = rng.uniform(1.4, 4.6, (n, 3)), rng.uniform(0.001, 0.05, (n, 3))
    s, mu = np.asarray(NOC_STDS)[:, None, None], np.asarray(NOC_MEANS)[:, None, None]
    p, vp, D, vd = part * s + mu, part_var * s * s, dim[:, :, None, None], dim_var[:, :, None, None]
    T = torch.from_numpy
    coder = noc_head.NOCCoder()
    for pv, dv, want in ((part_var, None, vp * D * D), (None, dim_var, vd * p * p), (part_var, dim_var, vp * D * D + vd * p * p + vp * vd)):
        c3d, var = coder.decode(T(part), T(pv) if pv is not None else None, T(dim), T(dv) if dv is not None else None, False)
        np.testing.assert_allclose(c3d.numpy(), p * D, rtol=1e-13)
        np.testing.assert_allclose(var.numpy(), want, rtol=1e-13)
    # the same numbers from the training decode: class 0, encoded dimensions that decode to `dim` and `dim_var`
    sd0, mu0 = np.asarray(DIM_STDS[0]), np.asarray(DIM_MEANS[0])
    all_pred = np.zeros((n, 30, h, w)); all_pred[:, :3] = part
    dec = noc_head.decode_for_training_torch(T(all_pred), torch.zeros(n, dtype=torch.long), False, T((dim - mu0) / sd0), T(dim_var / sd0 ** 2))
    c3d, var = coder.decode(T(part), None, T(dim), T(dim_var), False)
    assert torch.allclose(dec['coords_3d'], c3d, rtol=1e-12) and torch.allclose(dec['coords_3d_var'], var, rtol=1e-12)


def test_symbols_exported_and_bound_by_name():
    """The NOC targets' own; test_capi_and_host.py::test_loader_binds_every_header has what holds for every header."""
    names = ('mr_noc_dense_target', 'mr_smooth_l1_mod_workspace_bytes', 'mr_smooth_l1_mod_loss', 'mr_smooth_l1_mod_loss_backward')
    lib = _lib.load()
    for fn in names:
        f = getattr(lib, fn)
        an = _lib.arg_names(fn)
        has_stream = fn != 'mr_smooth_l1_mod_workspace_bytes'
        assert len(f.argtypes) == len(an) + (1 if has_stream else 0)
        args = _lib.pack(fn, {k: 0 for k in an})
        assert len(args) == len(an)
    assert _lib.table_args('mr_noc_dense_target') == ('coords_3d', 'coords_3d_mask', 'dimensions')
    with pytest.raises(TypeError):
        _lib.pack('mr_smooth_l1_mod_loss', {k: 0 for k in _lib.arg_names('mr_smooth_l1_mod_loss')}, logstd=0)
    assert lib.mr_smooth_l1_mod_workspace_bytes(0) == 0 and lib.mr_smooth_l1_mod_workspace_bytes(1) == 256
    assert lib.mr_smooth_l1_mod_workspace_bytes(3 * 28 * 28 * 65) % 256 == 0


def test_argument_checks_need_no_device():
    """The entry points validate before they launch: these calls return without touching a device."""
    lib = _lib.load()
    E = -1                                                               # MR_ERR_BAD_ARGUMENT
    base = {k: 0 for k in _lib.arg_names('mr_noc_dense_target')}
    assert lib.mr_noc_dense_target(*_lib.pack('mr_noc_dense_target', base, n=0, h=1, w=1), None) == 0
    assert lib.mr_noc_dense_target(*_lib.pack('mr_noc_dense_target', base, n=-1, h=1, w=1), None) == E
    assert lib.mr_noc_dense_target(*_lib.pack('mr_noc_dense_target', base, n=0, h=0, w=1), None) == E
    assert lib.mr_noc_dense_target(*_lib.pack('mr_noc_dense_target', base, n=1, h=1, w=1), None) == E          # NULL pointers
    sl = {k: 0 for k in _lib.arg_names('mr_smooth_l1_mod_loss')}
    assert lib.mr_smooth_l1_mod_loss(*_lib.pack('mr_smooth_l1_mod_loss', sl, numel=4, beta=1.0), None) == E
    assert lib.mr_smooth_l1_mod_loss(*_lib.pack('mr_smooth_l1_mod_loss', sl, numel=0, beta=1.0), None) == E
    bw = {k: 0 for k in _lib.arg_names('mr_smooth_l1_mod_loss_backward')}
    assert lib.mr_smooth_l1_mod_loss_backward(*_lib.pack('mr_smooth_l1_mod_loss_backward', bw, numel=4, beta=1.0), None) == E
