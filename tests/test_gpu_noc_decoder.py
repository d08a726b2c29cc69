"""FCNNOCDecoder on the GPU: G20 through the fused CARAFE launches, the training-mode forward and parameter gradients
against the CPU run, and forward_all_pred feeding the fused training decode."""
import numpy as np
import pytest
import torch

from tests import noc_decoder_cases as cases

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-4, atol=1e-4)            # three fp32 convolution layers of MIOpen against the CPU's, on activations of size 1 .. 10


@pytest.fixture(scope='module')
def g20():
    return cases.load()


@pytest.fixture()
def hip_calls(monkeypatch):
    """counts the fused forward launches, so that a test cannot silently run the torch path"""
    from monorun_amd import carafe
    calls = []
    real = carafe._CarafePackFunction.apply
    monkeypatch.setattr(carafe._CarafePackFunction, 'apply', lambda *a: calls.append(a[0].shape) or real(*a))
    return calls


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_eval_forward_matches_g20_through_the_hip_path(g20, tag, hip_calls):
    head = cases.build(g20, tag).eval().to('cuda:0')
    x, latent, labels, flips = cases.inputs(g20, tag, 'cuda:0')
    with torch.no_grad():
        for name, flip in (('list', flips), ('true', True), ('false', False)):
            noc, var, ls, reg = head(x, latent, None, labels, flip=flip)
            assert var is None and reg is None
            assert np.allclose(noc.cpu().numpy(), g20[f'{tag}_eval_{name}_noc'], **TOL)
            assert np.allclose(ls.cpu().numpy(), g20[f'{tag}_eval_{name}_logstd'], **TOL)
        assert len(hip_calls) == 3 and hip_calls[0] == (cases.N, cases.CO, cases.RH, cases.RW)
        empty = head(x[:0], latent[:0], None, labels[:0])
        assert empty[0].shape == (0, 3, 2 * cases.RH, 2 * cases.RW) and len(hip_calls) == 3          # no RoIs: nothing launched


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_training_forward_and_parameter_gradients_match_the_cpu(g20, tag, hip_calls):
    results = {}
    for dev in ('cpu', 'cuda:0'):
        head = cases.with_recorded_masks(cases.build(g20, tag), g20, tag).train().to(dev)
        x, latent, labels, flips = cases.inputs(g20, tag, dev)
        noc, _, ls, _ = head(x, latent, None, labels, flip=flips)
        g = torch.Generator().manual_seed(5)
        wn, wl = torch.randn(noc.shape, generator=g).to(dev), torch.randn(ls.shape, generator=g).to(dev)
        ((noc * wn).sum() + (ls * wl).sum()).backward()
        results[dev] = (noc.detach().cpu().numpy(), ls.detach().cpu().numpy(), {k: p.grad.cpu().numpy() for k, p in head.named_parameters()})
    assert len(hip_calls) == 1
    cpu, gpu = results['cpu'], results['cuda:0']
    assert np.allclose(gpu[0], g20[f'{tag}_train_noc'], **TOL) and np.allclose(gpu[1], g20[f'{tag}_train_logstd'], **TOL)
    assert np.allclose(gpu[0], cpu[0], **TOL) and np.allclose(gpu[1], cpu[1], **TOL)
    for k, want in cpu[2].items():
        scale = float(np.abs(want).max())
        assert scale > 0 or k.startswith('conv_final'), k                                             # unselected classes' rows get none
        assert np.allclose(gpu[2][k], want, rtol=1e-3, atol=1e-4 * max(scale, 1.0)), (k, float(np.abs(gpu[2][k] - want).max()), scale)


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_forward_all_pred_feeds_the_fused_training_decode(g20, tag, hip_calls):
    from monorun_amd import noc_head
    head = cases.build(g20, tag).eval().to('cuda:0')
    x, latent, labels, flips = cases.inputs(g20, tag, 'cuda:0')
    kw = cases.GROUPS[tag]
    dim = torch.tensor([[0.1, -0.2, 0.3]], device='cuda:0').repeat(cases.N, 1).requires_grad_(True)
    all_pred = head.forward_all_pred(x, latent)
    out = noc_head.decode_for_training(all_pred, labels, flips, dim, **kw)
    assert len(hip_calls) == 1 and out['coords_3d'].grad_fn is not None
    assert np.allclose(out['noc_pred'].detach().cpu().numpy(), g20[f'{tag}_eval_list_noc'], **TOL)
    assert np.allclose(out['proj_logstd'].detach().cpu().numpy(), g20[f'{tag}_eval_list_logstd'], **TOL)
    want = noc_head.decode_for_training_torch(all_pred.detach().cpu(), labels.cpu(), flips, dim.detach().cpu(), **kw)
    assert torch.allclose(out['coords_3d'].detach().cpu(), want['coords_3d'], rtol=1e-6, atol=1e-6)
    out['coords_3d'].square().sum().backward()                                                        # through both fused backwards to the trunk
    g = head.upsample.content_encoder.weight.grad
    assert g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0 and dim.grad is not None
