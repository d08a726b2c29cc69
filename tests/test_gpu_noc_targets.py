"""The NOC head's LiDAR supervision on the MI355X: the fused dense targets bit for bit against G18 (the reference's values)
and against the composed path (encode the whole maps, mr_roi_align_avg, torch); every output element written; shapes; the RoIs the kernel
is specified to zero; determinism; dispatch.  SmoothL1LossMod's HIP path against G18 and the torch restatement; one training step."""
import types

import numpy as np
import pytest
import torch

from tests import noc_targets_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')


def _nt():
    from monorun_amd import noc_targets
    return noc_targets


def _bits(a, b):
    a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _spy(monkeypatch):
    """counts the calls of the fused path"""
    nt = _nt()
    calls = []
    real = nt._noc_targets_hip
    monkeypatch.setattr(nt, '_noc_targets_hip', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_fused_equals_g18_and_the_composed_path_bit_for_bit(tag, monkeypatch):
    nt = _nt()
    calls = _spy(monkeypatch)
    ins, rec = ref.group(tag, DEV)
    t, w = nt.noc_targets(*ref.call_args(ins))
    assert calls == [1] and t.device.type == 'cuda' and not t.requires_grad
    assert _bits(t, rec.targets), float((t - rec.targets).abs().max())
    assert _bits(w, rec.weights)
    tc, wc = nt.noc_targets_composed(*ref.call_args(ins))
    assert _bits(tc, rec.targets) and _bits(wc, rec.weights)
    assert calls == [1]


def test_raw_entry_point_writes_every_element():
    nt = _nt()
    ins, rec = ref.group('a', DEV)
    n = rec.targets.shape[0]
    out = (torch.full((n, 3, 28, 28), float('nan'), device=DEV), torch.full((n, 1, 28, 28), float('nan'), device=DEV),
           torch.full((n,), -7, device=DEV, dtype=torch.int32))
    t, w, cnt = nt._noc_targets_hip(*ref.call_args(ins), out=out)
    assert t is out[0] and _bits(t, rec.targets) and _bits(w, rec.weights)
    assert torch.equal(cnt.long(), (rec.weights > 0).flatten(1).sum(1))


SWEEP = [(n, ds, sizes) for n in (1, 3, 65) for ds in ((28, 28), (7, 9), (1, 1)) for sizes in (((24, 31),), ((24, 31), (17, 40), (30, 22)))]


@pytest.mark.parametrize('n,dense_size,sizes', SWEEP)
def test_shape_sweep_fused_equals_composed(n, dense_size, sizes, monkeypatch):
    nt = _nt()
    calls = _spy(monkeypatch)
    if len(sizes) == 1:
        per = [n]
    else:
        per = [n - n // 2, 0, n // 2] if n > 1 else [0, 0, 1]          # an image without positives in the middle (or two in front)
    wl = ref.random_workload(100 + n, sizes, per, device=DEV)
    args = (wl['pos_bboxes'], wl['gt_inds'], wl['coords'], wl['masks'], wl['dims'], wl['flips'], dense_size)
    t, w = nt.noc_targets(*args)
    assert calls == [1] and t.shape == (n, 3) + dense_size and w.shape == (n, 1) + dense_size
    tc, wc = nt.noc_targets_composed(*args)
    assert _bits(t, tc) and _bits(w, wc)
    assert bool(torch.isfinite(t).all())


def test_out_of_range_indices_and_nan_rois_give_zeros():
    nt = _nt()
    wl = ref.random_workload(7, ((24, 31), (17, 40)), [5, 4], device=DEV)
    args = lambda d: (d['pos_bboxes'], d['gt_inds'], d['coords'], d['masks'], d['dims'], d['flips'], (7, 9))      # noqa: E731
    t0, w0, c0 = nt._noc_targets_hip(*args(wl))
    bad = dict(wl, gt_inds=[g.clone() for g in wl['gt_inds']], pos_bboxes=[b.clone() for b in wl['pos_bboxes']])
    bad['gt_inds'][0][1] = -1
    bad['gt_inds'][1][0] = 2                                            # == G of its image
    bad['pos_bboxes'][0][3, 2] = float('nan')
    bad['pos_bboxes'][1][2, 1] = float('nan')
    zeroed = [1, 3, 5, 7]
    kept = [i for i in range(9) if i not in zeroed]
    out = (torch.full((9, 3, 7, 9), float('nan'), device=DEV), torch.full((9, 1, 7, 9), float('nan'), device=DEV),
           torch.full((9,), -7, device=DEV, dtype=torch.int32))
    t, w, c = nt._noc_targets_hip(*args(bad), out=out)                  # returns: the call's status was 0
    torch.cuda.synchronize()
    assert bool((t[zeroed] == 0).all()) and bool((w[zeroed] == 0).all()) and bool((c[zeroed] == 0).all())
    assert _bits(t[kept], t0[kept]) and torch.equal(c[kept], c0[kept]) and torch.equal(w[kept] > 0, w0[kept] > 0)
    pos = (w > 0).float()
    assert _bits(w, pos / (pos.sum() / pos.new_full((), pos.numel())).clamp(min=1e-4))
    # +-inf clips to a finite border: not zeroed
    inf = dict(wl, pos_bboxes=[b.clone() for b in wl['pos_bboxes']])
    inf['pos_bboxes'][0][0, 2] = float('inf')
    inf['pos_bboxes'][0][0, 0] = float('-inf')
    ti, wi = nt.noc_targets(*args(inf))
    tc, wc = nt.noc_targets_composed(*args(inf))
    assert _bits(ti, tc) and _bits(wi, wc)


def test_two_calls_give_equal_bytes():
    nt = _nt()
    ins, _ = ref.group('a', DEV)
    a = nt.noc_targets(*ref.call_args(ins))
    b = nt.noc_targets(*ref.call_args(ins))
    assert _bits(a[0], b[0]) and _bits(a[1], b[1])


def test_other_layouts_take_the_composed_path_and_agree(monkeypatch):
    nt = _nt()
    calls = _spy(monkeypatch)
    ins, rec = ref.group('b', DEV)
    nc = dict(ins, coords=[torch.cat([c, c], 3)[..., :c.shape[3]] for c in ins['coords']])       # a view with a longer row stride
    assert not nc['coords'][0].is_contiguous()
    t, w = nt.noc_targets(*ref.call_args(nc))
    assert calls == [] and _bits(t, rec.targets) and _bits(w, rec.weights)
    st = dict(ins, dims=[torch.stack([d, d], 2)[:, :, 0] for d in ins['dims']])                 # dimension rows with an inner stride of 2
    assert st['dims'][0].stride(1) == 2
    t, w = nt.noc_targets(*ref.call_args(st))
    assert calls == [] and _bits(t, rec.targets) and _bits(w, rec.weights)
    # fp64 maps: fp32(1e-5) as a double is below the coder's eps 1e-5, so the pixels at the threshold are a different input in fp64;
    # compare on maps without the sub-threshold values (pooled masks are then 0 or far above eps_t: checked)
    lo = [m < 0.1 for m in ins['masks']]
    cl = dict(ins, masks=[torch.where(z, torch.zeros_like(m), m) for m, z in zip(ins['masks'], lo)],
              coords=[torch.where(z, torch.zeros_like(c), c) for c, z in zip(ins['coords'], lo)])
    t32, w32, c32 = nt._noc_targets_hip(*ref.call_args(cl))
    f64 = dict(cl, coords=[c.double() for c in cl['coords']], masks=[m.double() for m in cl['masks']], dims=[d.double() for d in cl['dims']],
               pos_bboxes=[b.double() for b in cl['pos_bboxes']])
    calls.clear()
    t, w = nt.noc_targets(*ref.call_args(f64))
    assert calls == [] and t.dtype == torch.float64
    # encoded in fp64, pooled in fp32: apart from the fused path's five fp32 roundings of the encode, 2^-24 each of terms up to
    # max(|part|, |mean|) / std <= 1 / 0.23, i.e. 1.3e-6 absolute, and the pooling's own relative roundings
    assert torch.allclose(t.float(), t32, rtol=1e-5, atol=2e-6), float((t.float() - t32).abs().max())
    assert torch.equal(w > 0, w32 > 0) and torch.allclose(w.float(), w32, rtol=1e-6)
    cpu, _ = ref.group('b')
    t, w = nt.noc_targets(*ref.call_args(cpu))
    assert calls == [] and t.device.type == 'cpu' and _bits(t, rec.targets) and _bits(w, rec.weights)


def test_no_positives():
    nt = _nt()
    from monorun_amd import _lib
    ins, _ = ref.group('a', DEV)
    t, w = nt.noc_targets([b[:0] for b in ins['pos_bboxes']], [g[:0] for g in ins['gt_inds']], *ref.call_args(ins)[2:])
    assert t.shape == (0, 3, 28, 28) and w.shape == (0, 1, 28, 28) and t.device.type == 'cuda'
    base = {k: 0 for k in _lib.arg_names('mr_noc_dense_target')}
    assert _lib.load().mr_noc_dense_target(*_lib.pack('mr_noc_dense_target', base, n=0, h=28, w=28), None) == 0


# ------------------------------------------------------------------------------------------------ SmoothL1LossMod
def _loss_module(rec, **kw):
    from monorun_amd.losses import SmoothL1LossMod
    return SmoothL1LossMod(beta=rec.beta, loss_weight=rec.loss_weight, **kw)


def _hip_calls(monkeypatch):
    from monorun_amd import losses
    calls = []
    real = losses._SmoothL1ModFunction.apply
    monkeypatch.setattr(losses._SmoothL1ModFunction, 'apply', staticmethod(lambda *a: (calls.append(1), real(*a))[1]))
    return calls


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_smooth_l1_hip_against_g18(tag, monkeypatch):
    calls = _hip_calls(monkeypatch)
    _, rec = ref.group(tag, DEV)
    lm = _loss_module(rec)
    pred = rec.noc_pred.clone().requires_grad_(True)
    loss = lm(pred, rec.targets, weight=rec.weights)
    loss.backward(torch.tensor(rec.upstream, device=DEV))
    loss_sum = lm(pred.detach(), rec.targets, weight=rec.weights, reduction_override='sum')
    assert calls == [1, 1] and loss.dtype == torch.float32 and loss.dim() == 0
    for reduction, got, recorded in (('mean', loss.item(), rec.loss_mean), ('sum', loss_sum.item(), rec.loss_sum)):
        _, dev = ref.loss_terms64(rec, reduction)
        tol = max(4 * dev, 1e-7)
        err = abs(got - recorded) / abs(recorded)
        print(f'G18 {tag} {reduction}: HIP {got!r} recorded {recorded!r} relative error {err:.3e} (bound {tol:.3e})')
        assert err <= tol
    g, r = pred.grad, rec.grad_pred
    err = float(((g - r).abs() / r.abs().clamp(min=1e-30))[r != 0].max())
    print(f'G18 {tag} grad_pred: largest relative error {err:.3e} (bound 1e-6)')
    assert torch.equal(g == 0, r == 0)
    assert torch.allclose(g, r, rtol=1e-6, atol=0)


@pytest.mark.parametrize('numel', [1, 255, 256, 257, 3 * 28 * 28 * 65])
@pytest.mark.parametrize('weight_form', ['none', 'full', 'per_pixel'])
@pytest.mark.parametrize('reduction', ['mean', 'sum'])
def test_smooth_l1_hip_forms_and_sizes(numel, weight_form, reduction, monkeypatch):
    from monorun_amd.losses import SmoothL1LossMod
    calls = _hip_calls(monkeypatch)
    shape = (65, 3, 28, 28) if numel > 257 else ((1, 1, 1, 1) if numel == 1 else (1, 3, numel // 3, 1) if numel % 3 == 0 else (1, 1, numel, 1))
    if numel == 256:
        shape = (2, 2, 8, 8)
    assert int(np.prod(shape)) == numel
    rng = np.random.default_rng(numel)
    pred = torch.from_numpy(rng.normal(0, 1.5, shape).astype(np.float32)).to(DEV).requires_grad_(True)
    target = torch.from_numpy(rng.normal(0, 1, shape).astype(np.float32)).to(DEV)
    wshape = dict(none=None, full=shape, per_pixel=(shape[0], 1) + shape[2:])[weight_form]
    weight = torch.from_numpy(rng.uniform(0, 2, wshape).astype(np.float32)).to(DEV) if wshape else None
    lm = SmoothL1LossMod(beta=0.7, reduction=reduction, loss_weight=1.5)
    loss = lm(pred, target, weight=weight)
    loss.backward()
    assert calls == [1]
    # the same terms in torch: reduced in fp64 for the loss; the fp32 autograd chain for the gradient
    p64 = pred.detach().cpu().requires_grad_(True)
    w_cpu = weight.cpu() if weight is not None else None
    ref_loss = lm(p64, target.cpu(), weight=w_cpu)
    ref_loss.backward()
    from monorun_amd.losses import smooth_l1_loss_mod
    terms = smooth_l1_loss_mod(p64.detach(), target.cpu(), 0.7)
    terms = (terms * w_cpu if w_cpu is not None else terms).double()
    exact = 1.5 * (terms.mean() if reduction == 'mean' else terms.sum()).item()
    # fp32(loss_weight * fp32(sum)): two roundings of 2^-24 each
    assert abs(loss.item() - exact) <= 2.0 ** -22 * abs(exact)
    assert torch.allclose(pred.grad.cpu(), p64.grad, rtol=1e-6, atol=0)


def test_smooth_l1_fallbacks_run_in_torch(monkeypatch):
    calls = _hip_calls(monkeypatch)
    _, rec = ref.group('b', DEV)
    lm = _loss_module(rec)
    cpu_rec = ref.group('b')[1]
    want = _loss_module(cpu_rec)(cpu_rec.noc_pred - cpu_rec.targets, 0)
    assert torch.allclose(lm(rec.noc_pred - rec.targets, 0).cpu(), want, rtol=1e-6)                     # integer target
    assert lm(rec.noc_pred, rec.targets, weight=rec.weights, reduction_override='none').shape == rec.noc_pred.shape
    lm(rec.noc_pred, rec.targets, weight=rec.weights, avg_factor=10.0)
    _loss_module(cpu_rec)(cpu_rec.noc_pred, cpu_rec.targets, weight=cpu_rec.weights)                    # CPU
    lm(rec.noc_pred.double(), rec.targets.double())                                                     # not fp32
    assert calls == []
    # create_graph=True: the HIP forward, the restatement's backward with a graph of its own
    pred = rec.noc_pred.clone().requires_grad_(True)
    loss = lm(pred, rec.targets, weight=rec.weights)
    g, = torch.autograd.grad(loss, pred, create_graph=True)
    assert calls == [1] and g.requires_grad
    gg, = torch.autograd.grad(g.square().sum(), pred)
    p2 = rec.noc_pred.clone().requires_grad_(True)
    from monorun_amd.losses import smooth_l1_loss_mod, weight_reduce_loss
    l2 = rec.loss_weight * weight_reduce_loss(smooth_l1_loss_mod(p2, rec.targets, rec.beta), rec.weights)
    g2, = torch.autograd.grad(l2, p2, create_graph=True)
    gg2, = torch.autograd.grad(g2.square().sum(), p2)
    assert torch.allclose(g, g2, rtol=1e-5, atol=0) and torch.allclose(gg, gg2, rtol=1e-4, atol=1e-12)


def test_training_step_with_loss_noc_and_loss_proj():
    """noc_pred from decode_for_training on a leaf all_pred; loss_noc (fused targets of G18's group a) + loss_proj of §12; one backward."""
    from monorun_amd import noc_head
    from monorun_amd.losses import build_loss
    from monorun_amd.projection_head import UncertProjectionHead
    ins, rec = ref.group('a', DEV)
    n = rec.targets.shape[0]
    rng = np.random.default_rng(3)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).to(DEV)      # noqa: E731
    labels, flip = np.arange(n) % 3, (np.arange(n) // 3) % 2 == 1
    all_pred = T(rng.normal(0, 0.5, (n, 30, 28, 28))).requires_grad_(True)
    sel = np.zeros((n, 30), bool)
    noc_ch = np.zeros((n, 30), bool)
    for i in range(n):
        c0, l0 = flip[i] * 15 + 3 * labels[i], flip[i] * 15 + 9 + 2 * labels[i]
        sel[i, c0:c0 + 3] = sel[i, l0:l0 + 2] = noc_ch[i, c0:c0 + 3] = True
    dim = T(rng.normal(0, 0.5, (n, 3)))
    pose = T(np.stack([rng.uniform(-8, 8, n), rng.uniform(1, 2, n), rng.uniform(10, 40, n), rng.uniform(-3, 3, n)], 1))
    K = T(np.tile(np.array([[721.5, 0, 609.5], [0, 721.5, 172.8], [0, 0, 1]]), (n, 1, 1)))
    img = T(np.tile([375.0, 1242.0], (n, 1)))
    dist = torch.norm(pose[:, :3], dim=1, keepdim=True)
    dec = noc_head.decode_for_training(all_pred, torch.from_numpy(labels).to(DEV), torch.from_numpy(flip).to(DEV), dim, None, dist)
    head = UncertProjectionHead().to(DEV)
    proj = head(dec['coords_3d'], pose, K, img)
    roi_grid = proj.detach() + T(rng.normal(0, 3.0, tuple(proj.shape)))
    loss_proj = head.loss(proj, dec['proj_logstd'], roi_grid, dist)['loss_proj']
    sampling = [types.SimpleNamespace(pos_bboxes=b, pos_assigned_gt_inds=g) for b, g in zip(ins['pos_bboxes'], ins['gt_inds'])]
    boxes = [torch.cat([d, torch.zeros(d.shape[0], 4, device=DEV)], 1) for d in ins['dims']]
    t, w = noc_head.get_targets(sampling, ins['coords'], ins['masks'], boxes, dict(dense_size=28), [dict(flip=f) for f in ins['flips']])
    assert _bits(t, rec.targets) and _bits(w, rec.weights)
    loss_noc = noc_head.loss(dec['noc_pred'], t, w, build_loss(dict(type='SmoothL1LossMod', loss_weight=1.0, beta=1.0)))['loss_noc']
    g_noc, = torch.autograd.grad(loss_noc, all_pred, retain_graph=True)
    (loss_noc + loss_proj).backward()
    g = all_pred.grad.cpu().numpy()
    assert np.isfinite(g).all() and np.isfinite(loss_noc.item()) and loss_noc.item() > 0
    assert np.all(g[~sel] == 0) and np.all(np.abs(g[sel]).reshape(n, 5, -1).max(-1) > 0)
    gn = g_noc.cpu().numpy()
    has_pos = (rec.weights > 0).flatten(1).any(1).cpu().numpy()
    assert np.all(gn[~noc_ch] == 0)
    assert np.array_equal(np.abs(gn[noc_ch]).reshape(n, 3, -1).max(-1).min(-1) > 0, has_pos)
    assert has_pos.sum() < n                                             # the RoI over masked-out pixels trains nothing through loss_noc
