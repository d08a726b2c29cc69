"""The fused CARAFE launches on the GPU against the fp64 definition (tests/carafe_ref.py), at the smallest shapes that
exercise each way the kernels can be wrong (carafe_ref.SHAPES).  Bound, per element: |got - ref64| <= C_BOUND 2^-23 (sum of the
absolute terms of that element), C_BOUND = 4 x the ratio measured for the fp32 torch restatement on the CPU."""
import functools

import numpy as np
import pytest
import torch

from tests import carafe_ref as ref

pytestmark = pytest.mark.gpu

IDS = ['x'.join(map(str, s)) for s in ref.SHAPES]


@functools.lru_cache(maxsize=None)
def reference(shape):
    """inputs and the fp64 results, computed once per shape and shared"""
    N, C, H, W, k, G, s = shape
    x, m, go = ref.make_inputs(shape)
    out, outa = ref.forward(x, m, k, G, s)
    gx, gxa, gm, gma = ref.backward(x, m, go, k, G, s)
    arrays = dict(x=x, m=m, go=go, out=out, outa=outa, gx=gx, gxa=gxa, gm=gm, gma=gma)
    for a in arrays.values():
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def hip_run(shape):
    """(out, grad_x, grad_m) of the fused path on the whole batch, as CPU tensors"""
    return run(shape, slice(None))


def run(shape, rois, need_m=True, noncontiguous=False):
    from monorun_amd import carafe
    N, C, H, W, k, G, s = shape
    r = reference(shape)
    dev = torch.device('cuda:0')
    x, m, go = (torch.from_numpy(r[n][rois].copy()).to(dev) for n in ('x', 'm', 'go'))
    if noncontiguous:
        x = x.transpose(2, 3).contiguous().transpose(2, 3)
        m = torch.stack([m, m], dim=-1)[..., 0]
        go = go.transpose(2, 3).contiguous().transpose(2, 3)
        assert not m.is_contiguous() and (not x.is_contiguous() or H == 1 or W == 1)
    assert carafe.hip_ok(x, m, k, G, s), 'the test must run the HIP path'
    x.requires_grad_(True)
    m.requires_grad_(need_m)
    out = carafe.carafe_pack(x, m, k, G, s)
    assert out.grad_fn is not None and type(out.grad_fn).__name__.startswith('_CarafePackFunction')
    out.backward(go)
    torch.cuda.synchronize()
    return out.detach().cpu(), x.grad.cpu(), m.grad.cpu() if need_m else m.grad


@pytest.mark.parametrize('shape', ref.SHAPES, ids=IDS)
def test_forward_and_gradients_match_the_fp64_definition(shape):
    r = reference(shape)
    out, gx, gm = hip_run(shape)
    ratios = dict(out=ref.ratio(out.numpy(), r['out'], r['outa']), grad_x=ref.ratio(gx.numpy(), r['gx'], r['gxa']),
                  grad_m=ref.ratio(gm.numpy(), r['gm'], r['gma']))
    print(f'carafe {shape}: error / (2^-23 sum|terms|) = {ratios}, bound {ref.C_BOUND}')
    assert all(np.isfinite(t.numpy()).all() for t in (out, gx, gm))
    assert max(ratios.values()) <= ref.C_BOUND, ratios


@pytest.mark.parametrize('shape', ref.SHAPES, ids=IDS)
def test_a_roi_alone_equals_the_roi_in_the_batch_bitwise(shape):
    out, gx, gm = hip_run(shape)
    i = shape[0] - 1
    o1, gx1, gm1 = run(shape, slice(i, i + 1))
    assert torch.equal(o1[0], out[i]) and torch.equal(gx1[0], gx[i]) and torch.equal(gm1[0], gm[i])


@pytest.mark.parametrize('shape', ref.SHAPES, ids=IDS)
def test_two_runs_are_bitwise_equal(shape):
    first, second = hip_run(shape), run(shape, slice(None))
    assert all(torch.equal(a, b) for a, b in zip(first, second))


@pytest.mark.parametrize('shape', ref.SHAPES, ids=IDS)
def test_noncontiguous_inputs_and_a_mask_without_grad(shape):
    out, gx, gm = hip_run(shape)
    o2, gx2, gm2 = run(shape, slice(None), need_m=False, noncontiguous=True)
    assert gm2 is None
    assert torch.equal(o2, out) and torch.equal(gx2, gx)


def test_only_the_mask_gradient():
    """x without grad: the first backward launch alone, no workspace"""
    from monorun_amd import carafe
    shape = ref.SHAPES[2]
    r = reference(shape)
    dev = torch.device('cuda:0')
    x, m, go = (torch.from_numpy(r[n].copy()).to(dev) for n in ('x', 'm', 'go'))
    m.requires_grad_(True)
    carafe.carafe_pack(x, m, *shape[4:]).backward(go)
    assert torch.equal(m.grad.cpu(), hip_run(shape)[2])


def test_double_backward_runs_the_restatement():
    from monorun_amd import carafe
    shape = ref.SHAPES[1]
    r = reference(shape)
    dev = torch.device('cuda:0')
    x, m, go = (torch.from_numpy(r[n].copy()).to(dev) for n in ('x', 'm', 'go'))
    x.requires_grad_(True)
    m.requires_grad_(True)
    gx, gm = torch.autograd.grad(carafe.carafe_pack(x, m, *shape[4:]), (x, m), go, create_graph=True)
    assert gx.requires_grad and gm.requires_grad
    assert ref.ratio(gx.detach().cpu().numpy(), r['gx'], r['gxa']) <= ref.C_BOUND
    (gx.square().sum() + gm.square().sum()).backward()
    assert x.grad is not None and torch.isfinite(x.grad).all() and torch.isfinite(m.grad).all()


@pytest.mark.parametrize('shape', ref.SHAPES, ids=IDS)
def test_carafe_pack_module_on_the_gpu_equals_the_cpu(shape):
    """CARAFEPack with the same parameters on both devices: the op's bound plus the convolutions' own deviation.  The encoder's weights are
    scaled so that the logits are O(1); the deviation of the GPU's logits from the CPU's, dl, moves a softmax weight by at most
    w_t 2 max|dl| relatively (first order), which the bound takes in through the sum of absolute terms."""
    from monorun_amd.carafe import CARAFEPack
    N, C, H, W, k, G, s = shape
    torch.manual_seed(11)
    mod = CARAFEPack(C, s, up_kernel=k, up_group=G, compressed_channels=4).double()
    with torch.no_grad():
        mod.content_encoder.weight.mul_(1000.0)
    x = torch.from_numpy(reference(shape)['x'].copy())
    with torch.no_grad():
        m64 = mod.encode(x.double())
        want, unit = ref.forward(x.numpy(), m64.numpy(), k, G, s)
        gpu = mod.float().to('cuda:0')
        xg = x.to('cuda:0')
        dl = float((gpu.encode(xg).cpu().double() - m64).abs().max())
        got = gpu(xg).cpu().numpy()
    err = np.abs(got - want)
    bound = (ref.C_BOUND * ref.EPS32 + 2.0 * dl * (1.0 + 2.0 * dl)) * unit
    print(f'CARAFEPack {shape}: max |dl| {dl:.3e}, worst err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}')
    assert dl < 1e-3, 'the convolutions themselves deviate'
    assert np.all(err <= bound)
