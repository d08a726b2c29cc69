"""The backbone's fused launches on the GPU against the numpy definition (tests/resnet_ref.py) and the literal eager chain,
on the smallest shapes at which the kernels can go wrong: planes of 1, 3, 35 and 256 elements and an odd one of more than two chunks,
1, 3 and 70 channels, every pointer at every 4-byte alignment, every combination of the optional gradient outputs; the stem kernel across
its tile borders; and ``ResNet`` with every norm on the fused path."""
import copy
import ctypes
import itertools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import resnet_ref as ref
from tests.test_resnet_cpu import OPTIONS, U, check_sums, fp64_forward, literal_chain, run_torch, tensors

pytestmark = pytest.mark.gpu
ids = lambda o: '-'.join(k for k, v in o.items() if v) or 'plain'


def dev():
    return torch.device('cuda:0')


@pytest.mark.parametrize('opts', OPTIONS, ids=ids)
@pytest.mark.parametrize('shape', ref.SHAPES)
def test_random_data_is_bitwise_the_definition(shape, opts):
    from monorun_amd import resnet
    c = ref.case(shape, False, **opts)
    t = tensors(c, device=dev())
    assert resnet.hip_ok(t['x'], t['mean'], t['var'], t['weight'], t['bias'], t['r'])
    y, gx, gr, gw, gb = run_torch(resnet.bn_act, c, device=dev())
    assert np.array_equal(y, c['y']), 'values'
    assert np.array_equal(gx, c['gx']), 'grad_x'
    if opts['residual']:
        assert np.array_equal(gr, c['gr']), 'grad_r'
    check_sums(c, gw, gb, 'kernel')
    if opts['affine']:
        assert np.array_equal(gw, c['gw']) and np.array_equal(gb, c['gb']), 'the sums in the stated order'
    again = run_torch(resnet.bn_act, c, device=dev())
    for a, b in zip((y, gx, gr, gw, gb), again):
        assert (a is None and b is None) or np.array_equal(a, b), 'two runs are bitwise equal'
    # the literal chain on the GPU: within the definition's bound plus the chain's own distance to the fp64 evaluation
    lit = literal_chain(t['x'], t['mean'], t['var'], t['weight'], t['bias'], c['eps'], t['r'], c['relu']).cpu().numpy().astype(np.float64)
    truth, A = fp64_forward(c)
    assert np.all(np.abs(y - truth) <= 6 * U * A)
    assert np.all(np.abs(y - lit) <= 6 * U * A + np.abs(lit - truth))


@pytest.mark.parametrize('opts', OPTIONS, ids=ids)
@pytest.mark.parametrize('shape', ref.SHAPES)
def test_exactness_data_is_bitwise_the_literal_chain_and_its_autograd(shape, opts):
    from monorun_amd import resnet
    c = ref.case(shape, True, **opts)
    got, want = run_torch(resnet.bn_act, c, device=dev()), run_torch(literal_chain, c, device=dev())
    for name, a, b, d in zip(('y', 'grad_x', 'grad_r', 'grad_weight', 'grad_bias'), got, want, (c['y'], c['gx'], c['gr'], c['gw'], c['gb'])):
        if a is None:
            assert b is None
            continue
        assert np.array_equal(a, b), f'{name} against the literal chain'
        assert np.array_equal(a, d), f'{name} against the definition'


SENTINEL = 12345.0


class Guarded:
    """a tensor of the given shape inside a larger buffer filled with a sentinel, `offset` floats in: 4 * (offset % 4) bytes past a 16-byte
    boundary.  `fill`: a number, or the array it holds"""

    def __init__(self, shape, fill, offset):
        self.n = int(np.prod(shape))
        self.offset = offset
        self.buf = torch.full((self.n + offset + 37,), SENTINEL, device=dev(), dtype=torch.float32)
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf[offset:offset + self.n]
        if isinstance(fill, np.ndarray):
            self.view.copy_(torch.from_numpy(np.array(fill)).reshape(-1))
        else:
            self.view.fill_(fill)
        self.shape = shape

    def ptr(self):
        return self.view.data_ptr()

    def check(self):
        b = self.buf.cpu().numpy()
        assert np.all(b[:self.offset] == SENTINEL) and np.all(b[self.offset + self.n:] == SENTINEL), 'a store outside the tensor'
        return b[self.offset:self.offset + self.n].reshape(self.shape)


@pytest.mark.parametrize('offset', [0, 1, 2, 3])
@pytest.mark.parametrize('opts', OPTIONS[:3], ids=ids)
@pytest.mark.parametrize('shape', [(2, 3, 5, 7), (1, 70, 1, 3), (2, 1, 91, 93), (1, 1, 1, 1)])
def test_c_abi_writes_every_element_and_nothing_else(shape, opts, offset):
    """through the C ABI, every input and output inside a sentinel-filled buffer 0, 4, 8 or 12 bytes past a 16-byte boundary (each pointer
    at another one), every output starting as NaN, for every combination of the three optional gradient outputs: afterwards no NaN is left
    in what was asked for, the values are the definition's, the sentinels are intact, and what was not asked for is untouched"""
    from monorun_amd import _lib
    lib = _lib.load()
    c = ref.case(shape, False, **opts)
    N, C, H, W = shape
    nan = float('nan')
    stream = torch.cuda.current_stream(dev()).cuda_stream
    off = lambda k: 4 + (offset + k) % 4
    vec = lambda a, k: None if a is None else Guarded(a.shape, a, off(k))
    x, r, g = vec(c['x'], 0), vec(c['r'], 1), vec(c['g'], 2)
    mean, var, weight, bias = vec(c['mean'], 3), vec(c['var'], 0), vec(c['weight'], 1), vec(c['bias'], 2)
    p = lambda t: None if t is None else t.ptr()
    common = dict(mean=p(mean), var=p(var), weight=p(weight), n_images=N, channels=C, height=H, width=W, eps=c['eps'], relu=int(c['relu']))
    y = Guarded(shape, nan, off(3))
    _lib.call('mr_bn_act_forward', common, x=p(x), bias=p(bias), r=p(r), y=y.ptr(), stream=stream)
    torch.cuda.synchronize()
    assert np.array_equal(y.check(), c['y'])
    ws_bytes = lib.mr_bn_act_backward_workspace_bytes(N, C, H, W)
    assert ws_bytes == 8 * N * C * -(-(H * W) // ref.CHUNK)
    for want_x, want_r, want_p in itertools.product((False, True), repeat=3):
        gx, gr = Guarded(shape, nan, off(1)), Guarded(shape, nan, off(2))
        gw, gb = Guarded((C,), nan, off(3)), Guarded((C,), nan, off(0))
        ws = Guarded((ws_bytes // 4,), nan, off(1))
        _lib.call('mr_bn_act_backward', common, g=p(g), y=y.ptr(), x=p(x), grad_x=gx.ptr() if want_x else None,
                  grad_r=gr.ptr() if want_r else None, grad_weight=gw.ptr() if want_p else None, grad_bias=gb.ptr() if want_p else None,
                  workspace=ws.ptr() if want_p else None, stream=stream)
        torch.cuda.synchronize()
        for buf, asked, want in ((gx, want_x, c['gx']), (gr, want_r, c['gr']), (gw, want_p, c['gw']), (gb, want_p, c['gb'])):
            got = buf.check()
            if asked:
                assert np.array_equal(got, want.reshape(got.shape)), (want_x, want_r, want_p)
            else:
                assert np.all(np.isnan(got)), 'an output that was not asked for was written'
        part = ws.check()
        assert np.all(np.isnan(part)) if not want_p else not np.any(np.isnan(part)), 'one partial pair per chunk, each stored once'
    for buf, a in ((x, c['x']), (g, c['g']), (mean, c['mean']), (var, c['var'])):
        assert np.array_equal(buf.check(), a), 'an input was written'
    # only one of the two parameter gradients
    gw, gb, ws = Guarded((C,), nan, off(0)), Guarded((C,), nan, off(1)), Guarded((ws_bytes // 4,), nan, off(2))
    _lib.call('mr_bn_act_backward', common, g=p(g), y=y.ptr(), x=p(x), grad_x=None, grad_r=None, grad_weight=gw.ptr(), grad_bias=None,
              workspace=ws.ptr(), stream=stream)
    torch.cuda.synchronize()
    assert np.array_equal(gw.check(), c['gw']) and np.all(np.isnan(gb.check()))


def test_edge_values_on_the_gpu():
    """u exactly 0, -0, negative, NaN in x and in r; relu off; no weight; no bias: the bit patterns of the definition"""
    from monorun_amd import resnet
    nan = float('nan')
    x = torch.tensor([0.0, -0.0, -3.0, nan, 2.0, 1.0, -1.0, 5.0, 0.5]).view(1, 1, 3, 3)
    r = torch.tensor([0.0, 0.0, 1.0, 1.0, nan, -1.0, 1.0, -0.0, -0.5]).view(1, 1, 3, 3)
    g = torch.arange(1.0, 10.0).view(1, 1, 3, 3)
    mean, var, one = torch.zeros(1), torch.ones(1), torch.ones(1)
    n = lambda t: None if t is None else t.numpy()
    d = lambda t: None if t is None else t.to(dev())
    for weight, bias, res, relu in ((one, mean, r, True), (one, mean, r, False), (None, None, r, True), (None, None, None, False),
                                    (one, None, None, True), (None, mean, None, False), (-one, None, None, False)):
        xx, rr = d(x).requires_grad_(True), (d(res).requires_grad_(True) if res is not None else None)
        assert resnet.hip_ok(xx, d(mean), d(var), d(weight), d(bias), rr)
        y = resnet.bn_act(xx, d(mean), d(var), d(weight), d(bias), 0.0, rr, relu)
        want = ref.forward(n(x), n(mean), n(var), n(weight), n(bias), 0.0, n(res), relu)
        got = y.detach().cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want)), 'NaN propagates'
        assert np.array_equal(np.nan_to_num(got, nan=7.0).view(np.uint32), np.nan_to_num(want, nan=7.0).view(np.uint32)), 'values, signs of zero'
        grads = torch.autograd.grad(y, [xx] + ([rr] if rr is not None else []), d(g))
        gx, gm, _, _, _ = ref.backward(n(g), want, n(x), n(mean), n(var), n(weight), 0.0, relu, sums=False)
        assert np.array_equal(grads[0].cpu().numpy().view(np.uint32), gx.view(np.uint32))
        if rr is not None:
            assert np.array_equal(grads[1].cpu().numpy().view(np.uint32), gm.view(np.uint32))


# ------------------------------------------------------------------------------------------------ the stem
# the tile of the pooled map is 8 x 64, of the input 16 x 128: heights and widths 1, 2, 3, odd and even across a tile border, and a map
# wider and taller than one tile
STEM_SHAPES = [(1, 1, 1, 1), (1, 2, 1, 2), (2, 3, 2, 1), (1, 1, 2, 2), (1, 3, 3, 3), (2, 3, 5, 7), (1, 2, 15, 127), (1, 2, 16, 128),
               (1, 1, 17, 129), (1, 1, 18, 130), (2, 3, 35, 261)]


def run_stem(c, x=None):
    from monorun_amd import resnet
    t = tensors(c, device=dev())
    if x is not None:
        t['x'] = torch.from_numpy(x).to(dev())
    assert resnet.hip_ok(t['x'], t['mean'], t['var'], t['weight'], t['bias'])
    with torch.no_grad():
        return resnet.bn_relu_maxpool(t['x'], t['mean'], t['var'], t['weight'], t['bias'], c['eps']), t


@pytest.mark.parametrize('shape', STEM_SHAPES)
def test_stem_kernel_is_bitwise_the_definition(shape, monkeypatch):
    from monorun_amd import _lib, resnet
    calls = []
    real = _lib.call
    monkeypatch.setattr(resnet._lib, 'call', lambda fn, *a, **k: calls.append(fn) or real(fn, *a, **k))
    c = ref.stem_case(shape)
    p, _ = run_stem(c)
    assert calls == ['mr_bn_relu_maxpool_forward'], 'one launch, the full-resolution map is never written'
    assert tuple(p.shape) == c['p'].shape and np.array_equal(p.cpu().numpy(), c['p'])
    e = ref.stem_case(shape, True)
    p, t = run_stem(e)
    lit = F.max_pool2d(literal_chain(t['x'], t['mean'], t['var'], t['weight'], t['bias'], e['eps']), 3, 2, 1)
    assert torch.equal(p, lit) and np.array_equal(p.cpu().numpy(), e['p']), 'exactness data: bitwise the literal chain'
    # NaNs: at the corners of the map, and on both sides of every tile border (rows 15 / 16, columns 127 / 128: a tile's halo)
    N, C, H, W = shape
    x = np.array(c['x'])
    for iy, ix in ((0, 0), (H - 1, W - 1), (15, 127), (16, 128), (15, 5), (3, 128), (17, 129)):
        if iy < H and ix < W:
            x[0, 0, iy, ix] = np.nan
    want = ref.maxpool(ref.forward(x, c['mean'], c['var'], c['weight'], c['bias'], c['eps'], None, True))
    p, _ = run_stem(c, x)
    assert np.isnan(want[0, 0, 0, 0]) and np.array_equal(p.cpu().numpy(), want, equal_nan=True)
    # with a gradient required through the stem: bn_act, then F.max_pool2d
    t = tensors(c, device=dev())
    calls.clear()
    q = resnet.bn_relu_maxpool(t['x'].requires_grad_(True), t['mean'], t['var'], t['weight'], t['bias'], c['eps'])
    assert calls == ['mr_bn_act_forward'] and q.requires_grad and np.array_equal(q.detach().cpu().numpy(), c['p'])


@pytest.mark.parametrize('offset', [0, 1, 2, 3])
def test_stem_c_abi_writes_every_element_and_nothing_else(offset):
    from monorun_amd import _lib
    shape = (2, 3, 35, 261)
    c = ref.stem_case(shape)
    N, C, H, W = shape
    g = {k: Guarded(c[k].shape, c[k], 4 + (offset + i) % 4) for i, k in enumerate(('x', 'mean', 'var', 'weight', 'bias'))}
    p = Guarded(c['p'].shape, float('nan'), 4 + (offset + 1) % 4)
    _lib.call('mr_bn_relu_maxpool_forward', x=g['x'].ptr(), mean=g['mean'].ptr(), var=g['var'].ptr(), weight=g['weight'].ptr(),
              bias=g['bias'].ptr(), n_images=N, channels=C, height=H, width=W, eps=c['eps'], p=p.ptr(),
              stream=torch.cuda.current_stream(dev()).cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(p.check(), c['p'])
    assert np.array_equal(g['x'].check(), c['x'])


# ------------------------------------------------------------------------------------------------ autograd
def test_create_graph_runs_the_restatement():
    """a backward under create_graph=True leaves the kernel for the restatement: grad_x and grad_r are the definition's bit for bit (the
    same operations), the sums are within the bound, all carry a graph, and differentiating <grad_x, R> by g gives gm's mask times k"""
    from monorun_amd import resnet
    c = ref.case((2, 3, 5, 7))
    t = tensors(c, device=dev())
    leaves = [t[k].requires_grad_(True) for k in ('x', 'r', 'weight', 'bias')]
    g = t['g'].requires_grad_(True)
    y = resnet.bn_act(t['x'], t['mean'], t['var'], t['weight'], t['bias'], c['eps'], t['r'], True)
    gx, gr, gw, gb = torch.autograd.grad(y, leaves, g, create_graph=True)
    assert all(v.requires_grad for v in (gx, gr, gw, gb))
    assert np.array_equal(gx.detach().cpu().numpy(), c['gx']) and np.array_equal(gr.detach().cpu().numpy(), c['gr'])
    check_sums(c, gw.detach().cpu().numpy(), gb.detach().cpu().numpy(), 'create_graph')
    back, = torch.autograd.grad(gx.sum(), g)
    k = ref.istd_of(c['var'], c['eps']) * c['weight']
    want = np.where(c['y'] <= 0, np.float32(0), np.broadcast_to(ref.per_channel(k), c['y'].shape))
    assert np.array_equal(back.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ the module
def eager_resnet(state, x, stat_stage):
    """an independent eager composition from a state dict (torchvision's keys, style 'pytorch'): F.conv2d, F.batch_norm, +, F.relu,
    F.max_pool2d.  Norms of the stages >= stat_stage (the stem is stage 0) use the batch's statistics"""
    def bn(t, p, stage):
        return F.batch_norm(t, state[f'{p}.running_mean'].clone(), state[f'{p}.running_var'].clone(), state[f'{p}.weight'], state[f'{p}.bias'],
                            stage >= stat_stage, 0.1, 1e-5)
    t = F.max_pool2d(F.relu(bn(F.conv2d(x, state['conv1.weight'], stride=2, padding=3), 'bn1', 0)), 3, 2, 1)
    outs = []
    for s in range(1, 5):
        i = 0
        while f'layer{s}.{i}.conv1.weight' in state:
            p = f'layer{s}.{i}'
            stride = 2 if (s > 1 and i == 0) else 1
            out = F.relu(bn(F.conv2d(t, state[f'{p}.conv1.weight']), f'{p}.bn1', s))
            out = F.relu(bn(F.conv2d(out, state[f'{p}.conv2.weight'], stride=stride, padding=1), f'{p}.bn2', s))
            out = bn(F.conv2d(out, state[f'{p}.conv3.weight']), f'{p}.bn3', s)
            if f'{p}.downsample.0.weight' in state:
                t = bn(F.conv2d(t, state[f'{p}.downsample.0.weight'], stride=stride), f'{p}.downsample.1', s)
            t = F.relu(out + t)
            i += 1
        outs.append(t)
    return outs


def make_net(norm_eval=True):
    from monorun_amd.resnet import ResNet
    torch.manual_seed(11)
    net = ResNet(50, base_channels=8, frozen_stages=1, norm_eval=norm_eval)
    net.init_weights()
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():
        for name, v in net.state_dict().items():
            if 'num_batches' not in name and 'conv' not in name and 'downsample.0' not in name:
                v.copy_(torch.rand(v.shape, generator=g) * 0.5 + 0.75)
    x = torch.randn(2, 3, 40, 72, generator=g)
    return net, x, g


@pytest.mark.parametrize('training', [True, False])
def test_resnet_on_the_gpu_against_the_restatement(training, monkeypatch):
    """ResNet-50 (base 8) with frozen_stages=1 and norm_eval=True: every norm takes the fused path (nn.BatchNorm2d.forward raises), and the
    four outputs and every parameter gradient of stages 2 - 4 lie within four times the forced restatement's own distance to the fp64
    evaluation on the CPU (the margin of DESIGN.md §22 for the same comparison); frozen parameters get no gradient"""
    from monorun_amd import resnet
    net, x, g = make_net()
    gos = None

    def evaluate(module, device, dtype):
        nonlocal gos
        module = module.to(device=device, dtype=dtype).train(training)
        with torch.set_grad_enabled(training):
            outs = module(x.to(device=device, dtype=dtype))
        if gos is None:
            gos = [torch.randn(o.shape, generator=g) for o in outs]
        res = [o.detach().double().cpu() for o in outs]
        if training:
            named = [(n, p) for n, p in module.named_parameters() if p.requires_grad]
            assert named and all(n.startswith(('layer2', 'layer3', 'layer4')) for n, _ in named)
            assert not outs[0].requires_grad and all(o.requires_grad for o in outs[1:]), 'stage 1 is frozen'
            torch.autograd.backward(outs[1:], [t.to(device=device, dtype=dtype) for t in gos[1:]])
            for n, p in module.named_parameters():
                assert (p.grad is not None) == p.requires_grad, n
            res += [p.grad.double().cpu() for _, p in named]
        return res

    truth = evaluate(copy.deepcopy(net), 'cpu', torch.float64)
    calls = []
    real = resnet._lib.call
    monkeypatch.setattr(resnet._lib, 'call', lambda fn, *a, **k: calls.append(fn) or real(fn, *a, **k))

    def no_batch_norm(self, t):
        raise AssertionError('nn.BatchNorm2d.forward ran: a norm left the fused path')
    monkeypatch.setattr(nn.BatchNorm2d, 'forward', no_batch_norm)
    fused = evaluate(copy.deepcopy(net), dev(), torch.float32)
    assert calls.count('mr_bn_relu_maxpool_forward') == 1 and calls.count('mr_bn_act_forward') == 52
    assert calls.count('mr_bn_act_backward') == (52 - 10 if training else 0), 'the frozen stage 1 and its input need no backward'
    n_calls = len(calls)
    monkeypatch.setattr(resnet, 'hip_ok', lambda *a, **k: False)
    restated = evaluate(copy.deepcopy(net), dev(), torch.float32)
    assert len(calls) == n_calls, 'the restatement was forced'
    assert len(truth) == len(fused) == len(restated) and len(truth) == (4 + 3 * 42 if training else 4)
    worst = 0.0
    for k, (t, f, r) in enumerate(zip(truth, fused, restated)):
        ef, er = (f - t).abs().max().item(), (r - t).abs().max().item()
        print(f'tensor {k}: fused {ef:.3e} restatement {er:.3e} against fp64; bitwise equal: {torch.equal(f, r)}')
        worst = max(worst, ef / er if er else 0.0)
        assert ef <= 4 * er, k
    print(f'largest ratio of the fused error to the restatement\'s: {worst:.2f}')


def test_resnet_batch_statistics_path_equals_the_eager_composition():
    """norm_eval=False in training mode: the norms of stages 2 - 4 use the batch's statistics through nn.BatchNorm2d.forward with a
    separate add and ReLU, the frozen stem and stage 1 stay fused.  The two sides run the same torch kernels from stage 2 on and differ
    before it by the definition's rounding (6 u per norm); batch statistics over as few as 12 values per channel can amplify that, so the
    bound is 1e-3 of each map's largest value: four orders of magnitude above u, three below what any wiring error gives"""
    net, x, _ = make_net(norm_eval=False)
    net = net.to(dev()).train()
    assert net.layer2[0].bn1.training and not net.layer1[0].bn1.training and not net.bn1.training
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        outs = net(x.to(dev()))
        want = eager_resnet(state, x.to(dev()), 2)
    assert int(net.layer2[0].bn1.num_batches_tracked) == 1 and int(net.layer1[0].bn1.num_batches_tracked) == 0
    for a, b in zip(outs, want):
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-3 * float(b.abs().max())
