"""The CARAFE op's torch restatement against the fp64 definition (tests/carafe_ref.py), the module's parameters, and the C ABI of the
fused launches (include/monorun_carafe.h) as far as it goes without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

from tests import carafe_ref as ref

IDS = ['x'.join(map(str, s)) for s in ref.SHAPES]


def torch_run(shape, dtype):
    from monorun_amd.carafe import carafe_pack_torch
    N, C, H, W, k, G, s = shape
    x, m, go = ref.make_inputs(shape)
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    mt = torch.from_numpy(m).to(dtype).requires_grad_(True)
    out = carafe_pack_torch(xt, mt, k, G, s)
    out.backward(torch.from_numpy(go).to(dtype))
    want = ref.forward(x, m, k, G, s) + ref.backward(x, m, go, k, G, s)
    got = (out.detach().numpy(), xt.grad.numpy(), mt.grad.numpy())
    return [ref.ratio(g, want[2 * i], want[2 * i + 1]) for i, g in enumerate(got)]


@pytest.mark.parametrize('shape', ref.SHAPES, ids=IDS)
def test_restatement_matches_the_definition_in_fp64(shape):
    """forward, grad_x and grad_m in fp64: errors of fp64 size, 1e-6 of the fp32 unit"""
    assert max(torch_run(shape, torch.float64)) <= 1e-6


def test_the_bound_constant_is_the_measured_one():
    """C_MEASURED of carafe_ref is what the fp32 restatement shows on these inputs (torch's kernels differ a little between builds:
    the recorded figure must cover this build's and be no more than twice it)"""
    worst = np.max([torch_run(shape, torch.float32) for shape in ref.SHAPES], axis=0)
    print('fp32 restatement, error / (2^-23 sum|terms|): forward %.2f grad_x %.2f grad_m %.2f' % tuple(worst))
    assert worst.max() <= ref.C_MEASURED * 1.05 and ref.C_MEASURED <= 2 * worst.max()
    assert ref.C_BOUND == 4 * ref.C_MEASURED


def test_gradcheck():
    from monorun_amd.carafe import carafe, carafe_pack_torch
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 4, 2, 3, dtype=torch.float64, generator=g, requires_grad=True)
    m = torch.randn(2, 2 * 9 * 4, 2, 3, dtype=torch.float64, generator=g, requires_grad=True)
    assert torch.autograd.gradcheck(lambda a, b: carafe_pack_torch(a, b, 3, 2, 2), (x, m))
    w = torch.rand(2, 2 * 9, 4, 6, dtype=torch.float64, generator=g, requires_grad=True)
    assert torch.autograd.gradcheck(lambda a, b: carafe(a, b, 3, 2, 2), (x, w))


def test_plain_op_on_given_masks():
    from monorun_amd.carafe import carafe, normalize_masks
    shape = ref.SHAPES[2]
    N, C, H, W, k, G, s = shape
    x, m, _ = ref.make_inputs(shape)
    w = normalize_masks(torch.from_numpy(m).double(), k, G, s)
    assert w.shape == (N, G * k * k, H * s, W * s)
    assert torch.allclose(w.view(N, G, k * k, H * s, W * s).sum(2), torch.ones(1, dtype=torch.float64))
    assert np.allclose(w.numpy().reshape(N, G, k * k, H * s, W * s), ref.softmax(ref.shuffled_logits(m.astype(np.float64), k, G, s), 2))
    out = carafe(torch.from_numpy(x).double(), w, k, G, s)
    assert ref.ratio(out.numpy(), *ref.forward(x, m, k, G, s)) <= 1e-6


def test_cpu_and_other_dtypes_run_the_restatement():
    from monorun_amd import carafe
    x = torch.randn(2, 4, 3, 3)
    m = torch.randn(2, 25 * 4, 3, 3)
    assert not carafe.hip_ok(x, m, 5, 1, 2)
    out = carafe.carafe_pack(x, m, 5, 1, 2)
    assert out.shape == (2, 4, 6, 6) and torch.equal(out, carafe.carafe_pack_torch(x, m, 5, 1, 2))
    assert carafe.carafe_pack(x.double(), m.double(), 5, 1, 2).dtype == torch.float64
    assert carafe.carafe_pack(x[:0], m[:0], 5, 1, 2).shape == (0, 4, 6, 6)
    assert carafe.carafe_pack(x, torch.randn(2, 9 * 9, 3, 3), 3, 1, 3).shape == (2, 4, 9, 9)       # a scale the kernels do not cover


def test_carafe_pack_module_parameters():
    from monorun_amd.carafe import CARAFEPack
    torch.manual_seed(0)
    mod = CARAFEPack(256, 2)
    shapes = {k: tuple(v.shape) for k, v in mod.state_dict().items()}
    assert shapes == {'channel_compressor.weight': (64, 256, 1, 1), 'channel_compressor.bias': (64,),
                      'content_encoder.weight': (100, 64, 3, 3), 'content_encoder.bias': (100,)}
    assert list(shapes) == ['channel_compressor.weight', 'channel_compressor.bias', 'content_encoder.weight', 'content_encoder.bias']
    assert mod.content_encoder.padding == (1, 1) and float(mod.content_encoder.bias.detach().abs().max()) == 0
    assert 0.0008 < float(mod.content_encoder.weight.detach().std()) < 0.0012
    bound = (6.0 / (256 + 64)) ** 0.5                                                              # Xavier-uniform of the 1 x 1 compressor
    assert float(mod.channel_compressor.weight.detach().abs().max()) <= bound and float(mod.channel_compressor.weight.detach().std()) > 0.5 * bound
    small = CARAFEPack(6, 4, up_kernel=3, up_group=2, encoder_kernel=5, encoder_dilation=2, compressed_channels=4)
    assert small.content_encoder.weight.shape == (9 * 2 * 16, 4, 5, 5) and small.content_encoder.padding == (4, 4)
    x = torch.randn(2, 6, 3, 5)
    assert small(x).shape == (2, 6, 12, 20)
    # near-uniform masks after init: the output is close to a box filter of the input, and exactly differentiable
    x.requires_grad_(True)
    small(x).sum().backward()
    assert x.grad is not None and small.content_encoder.weight.grad is not None


def test_loader_binds_the_carafe_header():
    """What is CARAFE's own; test_capi_and_host.py::test_loader_binds_every_header has what holds for every header."""
    from monorun_amd import _lib, carafe
    lib = _lib.load()
    assert len(lib.mr_carafe_pack_forward.argtypes) == 11 and len(lib.mr_carafe_pack_backward.argtypes) == 15
    src = open(_lib.header_path('carafe')).read()
    assert '#define MR_CARAFE_CHUNK 32' in src and '#define MR_CARAFE_TILE 16' in src and '#define MR_CARAFE_MAX_KERNEL 7' in src
    assert (carafe.CHUNK, carafe.TILE, carafe.MAX_KERNEL) == (32, 16, 7) and ref.CHUNK == carafe.CHUNK


def test_entry_points_check_their_arguments_without_a_gpu():
    """Bad arguments are rejected before any HIP call, so this runs on the CPU."""
    from monorun_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    sizes = dict(n=3, channels=6, h=3, w=5, up_kernel=5, up_group=2, scale_factor=2)

    def nbytes(**kw):
        return lib.mr_carafe_backward_workspace_bytes(*_lib.pack('mr_carafe_backward_workspace_bytes', dict(sizes, **kw)))
    assert nbytes() == 4 * 3 * 2 * 25 * 6 * 10
    assert nbytes(n=100, channels=256, h=14, w=14, up_group=1) == 4 * 100 * 25 * 28 * 28
    assert nbytes(n=0) == 0 and nbytes(n=-1) == 0 and nbytes(up_kernel=4) == 0 and nbytes(scale_factor=3) == 0 and nbytes(up_group=4) == 0

    def fwd(**kw):
        return lib.mr_carafe_pack_forward(*_lib.pack('mr_carafe_pack_forward', {**sizes, **dict(x=p, m=p, out=p), **kw}), None)

    def bwd(**kw):
        a = dict(sizes, x=p, m=p, grad_out=p, workspace=p, grad_x=p, grad_m=p)
        a.update(kw)
        a.setdefault('workspace_bytes', nbytes(**{k: a[k] for k in sizes}))
        return lib.mr_carafe_pack_backward(*_lib.pack('mr_carafe_pack_backward', a), None)
    assert fwd(n=0) == 0 and bwd(n=0) == 0                                                         # launch nothing
    assert bwd(grad_x=None, grad_m=None) == 0                                                      # nothing wanted
    for kw in (dict(n=-1), dict(channels=0), dict(h=0), dict(w=0), dict(up_group=0), dict(up_group=4), dict(channels=7)):
        assert fwd(**kw) == -1 and bwd(**kw) == -1, kw
    for kw in (dict(x=None), dict(m=None), dict(out=None)):
        assert fwd(**kw) == -1, kw
    for kw in (dict(x=None), dict(m=None), dict(grad_out=None), dict(workspace=None), dict(workspace=p + 2), dict(workspace_bytes=nbytes() - 1)):
        assert bwd(**kw) == -1, kw
    for kw in (dict(up_kernel=4), dict(up_kernel=9), dict(up_kernel=0), dict(scale_factor=3), dict(scale_factor=8), dict(scale_factor=0),
               dict(h=40000, w=40000), dict(channels=2 ** 20, up_group=1, h=64, w=64)):
        assert fwd(n=0, **kw) == -2 and bwd(n=0, **kw) == -2, kw
