"""The backbone without a GPU: the torch restatement of the fused batch norm against the numpy definition
(tests/resnet_ref.py) and against the literal eager chain, the edge values, the ``ResNet`` module, the loader's row and the argument checks
of the four entry points."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import resnet_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
SHAPES = [(1, 1, 1, 1), (2, 3, 1, 3), (2, 3, 5, 7), (1, 70, 5, 7), (2, 3, 16, 16), (2, 1, 91, 93)]
OPTIONS = [dict(residual=True, relu=True, affine=True), dict(residual=False, relu=True, affine=True),
           dict(residual=True, relu=False, affine=True), dict(residual=False, relu=False, affine=False)]


def tensors(c, dtype=torch.float32, device='cpu'):
    t = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(device=device, dtype=dtype)
    return {k: t(c[k]) for k in ('x', 'g', 'r', 'mean', 'var', 'weight', 'bias')}


def literal_chain(x, mean, var, weight=None, bias=None, eps=1e-5, residual=None, relu=True):
    """what the reference's blocks run with norm_eval=True, as separate ops"""
    if eps > 0:
        y = F.batch_norm(x, mean, var, weight, bias, False, 0.1, eps)
    else:           # the exactness data: F.batch_norm's Python wrapper refuses eps = 0; this is the op it calls
        y = torch.batch_norm(x, weight, bias, mean, var, False, 0.1, eps, torch.backends.cudnn.enabled)
    if residual is not None:
        y = y + residual
    return F.relu(y) if relu else y


def run_torch(fn, c, dtype=torch.float32, device='cpu'):
    """(y, grad_x, grad_r, grad_weight, grad_bias) of a torch implementation on a case of resnet_ref, as numpy"""
    t = tensors(c, dtype, device)
    leaves = [t[k].requires_grad_(True) for k in ('x', 'r', 'weight', 'bias') if t[k] is not None]
    y = fn(t['x'], t['mean'], t['var'], t['weight'], t['bias'], c['eps'], t['r'], c['relu'])
    grads = iter(torch.autograd.grad(y, leaves, t['g']))
    out = {k: (next(grads).detach().cpu().numpy() if t[k] is not None else None) for k in ('x', 'r', 'weight', 'bias')}
    return y.detach().cpu().numpy(), out['x'], out['r'], out['weight'], out['bias']


def fp64_forward(c):
    """the definition evaluated in fp64 from the fp32 inputs, and A of the bound: (|x| + |mean|) |istd weight| + |bias| + |r|"""
    d = lambda a: None if a is None else a.astype(np.float64)
    x, mean, var, w, b, r = (d(c[k]) for k in ('x', 'mean', 'var', 'weight', 'bias', 'r'))
    pc = ref.per_channel
    istd = 1.0 / np.sqrt(var + c['eps'])
    k = istd * (w if w is not None else 1.0)
    u = (x - pc(mean)) * pc(k) + (pc(b) if b is not None else 0.0) + (r if r is not None else 0.0)
    A = (np.abs(x) + np.abs(pc(mean))) * np.abs(pc(k)) + (np.abs(pc(b)) if b is not None else 0.0) + (np.abs(r) if r is not None else 0.0)
    return (np.where(u <= 0, 0.0, u) if c['relu'] else u), A


def sum_bound(c, terms):
    """(D + 1) 2^-24 sum|term| per channel, D = 34 + ceil(P / 64) of include/monorun_backbone.h: a lane's head, 16 group elements and
    tail (18), the butterfly (6), the four waves (4), a finalising lane's ceil(P / 64) partials and its butterfly (6).  torch's own orders
    (a pairwise tree, vectorised) chain fewer additions on these shapes"""
    N, C, H, W = c['shape']
    D = ref.chain_depth(N, H * W)
    assert D == 34 + -(-(N * -(-(H * W) // 4096)) // 64)
    return (D + 1) * U * np.abs(terms.astype(np.float64)).sum(axis=(0, 2, 3))


def check_sums(c, gw, gb, what):
    N, C, H, W = c['shape']
    gm = c['gr'].astype(np.float64)
    for name, got, terms in (('grad_weight', gw, c['terms']), ('grad_bias', gb, c['gr'])):
        if got is None:
            continue
        exact = terms.astype(np.float64).sum(axis=(0, 2, 3))
        err, bound = np.abs(got.astype(np.float64) - exact), sum_bound(c, terms)
        print(f'{what} {c["shape"]} {name}: largest error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}')
        assert np.all(err <= bound), (what, name)
    del gm


@pytest.mark.parametrize('opts', OPTIONS, ids=lambda o: '-'.join(k for k, v in o.items() if v) or 'plain')
@pytest.mark.parametrize('shape', SHAPES)
def test_restatement_matches_the_definition(shape, opts):
    from monorun_amd.resnet import bn_act_torch
    c = ref.case(shape, False, **opts)
    y, gx, gr, gw, gb = run_torch(bn_act_torch, c)
    assert np.array_equal(y, c['y']), 'values'
    assert np.array_equal(gx, c['gx']), 'grad_x'
    if opts['residual']:
        assert np.array_equal(gr, c['gr']), 'grad_r'
    check_sums(c, gw, gb, 'restatement')
    check_sums(c, c['gw'], c['gb'], 'definition')               # the stated order itself is within its own bound


@pytest.mark.parametrize('opts', OPTIONS, ids=lambda o: '-'.join(k for k, v in o.items() if v) or 'plain')
@pytest.mark.parametrize('shape', SHAPES)
def test_exactness_data_is_bitwise_the_literal_chain(shape, opts):
    """integers in [-8, 8], var in {0.25, 1, 4}, eps = 0: every order of these operations is exact, the gradients' sums included"""
    from monorun_amd.resnet import bn_act_torch
    c = ref.case(shape, True, **opts)
    got, want = run_torch(bn_act_torch, c), run_torch(literal_chain, c)
    for name, a, b, d in zip(('y', 'grad_x', 'grad_r', 'grad_weight', 'grad_bias'), got, want, (c['y'], c['gx'], c['gr'], c['gw'], c['gb'])):
        if a is None:
            assert b is None
            continue
        assert np.array_equal(a, b), f'{name} against the literal chain'
        assert np.array_equal(a, d), f'{name} against the definition'


@pytest.mark.parametrize('opts', OPTIONS, ids=lambda o: '-'.join(k for k, v in o.items() if v) or 'plain')
@pytest.mark.parametrize('shape', SHAPES)
def test_random_data_against_fp64_and_the_literal_chain(shape, opts):
    """the definition rounds at most six times on the path of an element (var + eps, sqrt, 1 / ., x - mean, . istd, . weight, + bias,
    + r; the first three belong to istd, which enters A once): |y - fp64| <= 6 u A.  The literal chain may differ from the restatement
    by that plus its own measured distance to fp64, element by element"""
    from monorun_amd.resnet import bn_act_torch
    c = ref.case(shape, False, **opts)
    t = tensors(c)
    y = bn_act_torch(t['x'], t['mean'], t['var'], t['weight'], t['bias'], c['eps'], t['r'], c['relu']).numpy().astype(np.float64)
    lit = literal_chain(t['x'], t['mean'], t['var'], t['weight'], t['bias'], c['eps'], t['r'], c['relu']).numpy().astype(np.float64)
    truth, A = fp64_forward(c)
    bound = 6 * U * A
    err = np.abs(y - truth)
    print(f'{shape}: restatement against fp64: largest error / bound {np.max(err / bound):.3f}')
    assert np.all(err <= bound)
    assert np.all(np.abs(y - lit) <= bound + np.abs(lit - truth))


def test_edge_values():
    """u exactly 0, -0, negative, NaN in x and in r; relu off; no weight; no bias"""
    from monorun_amd.resnet import bn_act_torch
    nan = float('nan')
    x = torch.tensor([0.0, -0.0, -3.0, nan, 2.0, 1.0, -1.0, 5.0]).view(1, 1, 2, 4)
    r = torch.tensor([0.0, 0.0, 1.0, 1.0, nan, -1.0, 1.0, -0.0]).view(1, 1, 2, 4)
    mean, var, one = torch.zeros(1), torch.ones(1), torch.ones(1)
    args = (x.numpy(), mean.numpy(), var.numpy())
    for weight, bias, res, relu in ((one, mean, r, True), (one, mean, r, False), (None, None, r, True), (None, None, None, False),
                                    (one, None, None, True), (None, mean, None, False), (-one, None, None, False)):
        xx, rr = x.clone().requires_grad_(True), (res.clone().requires_grad_(True) if res is not None else None)
        y = bn_act_torch(xx, mean, var, weight, bias, 0.0, rr, relu)
        n = lambda t: None if t is None else t.numpy()
        want = ref.forward(*args, n(weight), n(bias), 0.0, n(res), relu)
        assert np.array_equal(y.detach().numpy().view(np.uint32), want.view(np.uint32)), 'bit patterns: the sign of zero, the NaNs'
        g = torch.arange(1.0, 9.0).view(1, 1, 2, 4)
        grads = torch.autograd.grad(y, [xx] + ([rr] if rr is not None else []), g)
        gx, gm, _, _, _ = ref.backward(g.numpy(), want, *args, n(weight), 0.0, relu, sums=False)
        assert np.array_equal(grads[0].numpy().view(np.uint32), gx.view(np.uint32))
        if rr is not None:
            assert np.array_equal(grads[1].numpy().view(np.uint32), gm.view(np.uint32))
    y = bn_act_torch(x, mean, var, one, mean, 0.0, r, True).view(-1)
    assert y[0].item() == 0 and not np.signbit(y[0].item()) and not np.signbit(y[1].item()), 'relu: +0 from either zero'
    assert y[2].item() == 0 and not np.signbit(y[2].item()) and torch.isnan(y[3]) and torch.isnan(y[4]) and y[5].item() == 0 and y[7].item() == 5
    z = bn_act_torch(x, mean, var, None, None, 0.0, None, False).view(-1)
    assert np.signbit(z[1].item()), 'no relu, no bias: -0 stays'


@pytest.mark.parametrize('shape', [(1, 1, 1, 1), (2, 3, 1, 3), (2, 3, 5, 7), (1, 2, 16, 16), (1, 1, 2, 2)])
def test_stem_restatement(shape):
    from monorun_amd.resnet import bn_relu_maxpool_torch
    for exact in (False, True):
        c = ref.stem_case(shape, exact)
        t = tensors(c)
        p = bn_relu_maxpool_torch(t['x'], t['mean'], t['var'], t['weight'], t['bias'], c['eps'])
        assert tuple(p.shape) == c['p'].shape and np.array_equal(p.numpy(), c['p'])
        if exact:
            lit = F.max_pool2d(literal_chain(t['x'], t['mean'], t['var'], t['weight'], t['bias'], c['eps']), 3, 2, 1)
            assert torch.equal(p, lit)
    y = np.array([[1.0, np.nan, 0.0], [0.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 3.0]], np.float32).reshape(1, 1, 4, 3)
    want = F.max_pool2d(torch.from_numpy(y), 3, 2, 1).numpy()
    assert np.array_equal(ref.maxpool(y), want, equal_nan=True) and np.isnan(want[0, 0, 0, 0]) and want[0, 0, 1, 1] == 3


def test_other_dtypes_layouts_and_create_graph():
    from monorun_amd import resnet
    c = ref.case((2, 3, 5, 7))
    t = tensors(c)
    args = lambda d: (d['x'], d['mean'], d['var'], d['weight'], d['bias'], c['eps'], d['r'], True)
    assert not resnet.hip_ok(t['x'], t['mean'], t['var'], t['weight'], t['bias'], t['r']), 'CPU tensors never take the HIP path'
    y = resnet.bn_act(*args(t))
    assert np.array_equal(y.numpy(), c['y'])
    for dtype, tol in ((torch.float64, 1e-5), (torch.bfloat16, 1e-1), (torch.float16, 2e-2)):
        d = tensors(c, dtype)
        yd = resnet.bn_act(*args(d))
        assert yd.dtype == dtype and torch.allclose(yd.float(), y, atol=tol, rtol=tol)
    cl = dict(t, x=t['x'].contiguous(memory_format=torch.channels_last), r=t['r'].transpose(2, 3).contiguous().transpose(2, 3))
    assert torch.equal(resnet.bn_act(*args(cl)), y)
    d = {k: (v.double().requires_grad_(k in ('x', 'r', 'weight', 'bias')) if v is not None else None) for k, v in t.items()}
    fn = lambda x, w, b, r: resnet.bn_act(x, d['mean'], d['var'], w, b, c['eps'], r, True)
    assert torch.autograd.gradcheck(fn, (d['x'], d['weight'], d['bias'], d['r']), eps=1e-6, atol=1e-5)
    small = {k: (v[:1, :, :2, :2] if v is not None and v.dim() == 4 else v) for k, v in d.items()}
    small = {k: (v.detach().clone().requires_grad_(v.requires_grad) if v is not None else None) for k, v in small.items()}
    fn2 = lambda x, w, b, r: resnet.bn_act(x, small['mean'], small['var'], w, b, c['eps'], r, False)
    assert torch.autograd.gradgradcheck(fn2, (small['x'], small['weight'], small['bias'], small['r']), eps=1e-6, atol=1e-5)


# ------------------------------------------------------------------------------------------------ the module
STAGES = {18: (2, 2, 2, 2), 50: (3, 4, 6, 3), 101: (3, 4, 23, 3)}


def expected_keys(depth, base=64):
    """{key: shape} generated from the stage table: torchvision's and mmdet's names"""
    bottleneck = depth >= 50
    exp = 4 if bottleneck else 1
    keys = {'conv1.weight': (base, 3, 7, 7)}

    def norm(prefix, ch):
        for n in ('weight', 'bias', 'running_mean', 'running_var'):
            keys[f'{prefix}.{n}'] = (ch,)
        keys[f'{prefix}.num_batches_tracked'] = ()
    norm('bn1', base)
    inplanes = base
    for s, blocks in enumerate(STAGES[depth]):
        planes = base * 2 ** s
        for i in range(blocks):
            p = f'layer{s + 1}.{i}'
            if bottleneck:
                convs = [(inplanes, planes, 1), (planes, planes, 3), (planes, planes * 4, 1)]
            else:
                convs = [(inplanes, planes, 3), (planes, planes, 3)]
            for j, (cin, cout, k) in enumerate(convs, 1):
                keys[f'{p}.conv{j}.weight'] = (cout, cin, k, k)
                norm(f'{p}.bn{j}', cout)
            if i == 0 and (s > 0 or inplanes != planes * exp):
                keys[f'{p}.downsample.0.weight'] = (planes * exp, inplanes, 1, 1)
                norm(f'{p}.downsample.1', planes * exp)
            inplanes = planes * exp
    return keys


@pytest.mark.parametrize('depth', [18, 50, 101])
def test_state_dict_keys_are_torchvisions(depth):
    from monorun_amd.resnet import ResNet
    net = ResNet(depth)
    want = expected_keys(depth)
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == want
    assert sum(isinstance(m, nn.BatchNorm2d) for m in net.modules()) == {18: 20, 50: 53, 101: 104}[depth]
    g = torch.Generator().manual_seed(depth)
    state = {k: (torch.rand(s, generator=g) + 0.5 if s else torch.tensor(7)) for k, s in want.items()}
    net.load_state_dict({f'{k}': v for k, v in state.items()}, strict=True)
    assert torch.equal(net.layer2[0].downsample[1].running_var, state['layer2.0.downsample.1.running_var'])


def test_outputs_strides_and_out_indices():
    from monorun_amd.resnet import ResNet
    x = torch.randn(1, 3, 64, 96, generator=torch.Generator().manual_seed(0))
    for depth, chans in ((18, (8, 16, 32, 64)), (50, (32, 64, 128, 256))):
        net = ResNet(depth, base_channels=8).eval()
        with torch.no_grad():
            outs = net(x)
        assert isinstance(outs, tuple)
        assert [tuple(o.shape) for o in outs] == [(1, c, 64 // s, 96 // s) for c, s in zip(chans, (4, 8, 16, 32))]
        assert net.feat_dim == chans[-1]
    net = ResNet(18, base_channels=8, out_indices=(1, 3)).eval()
    with torch.no_grad():
        outs = net(x)
    assert [o.shape[1] for o in outs] == [16, 64]
    three = ResNet(18, base_channels=8, num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,)).eval()
    assert not hasattr(three, 'layer4') and three(x)[0].shape == (1, 32, 4, 6)
    dil = ResNet(50, base_channels=8, strides=(1, 2, 1, 1), dilations=(1, 1, 2, 4), out_indices=(3,)).eval()
    assert dil(x)[0].shape == (1, 256, 8, 12) and dil.layer4[1].conv2.dilation == (4, 4)


def test_style_puts_the_stride():
    from monorun_amd.resnet import ResNet
    py, caffe = ResNet(50, base_channels=8), ResNet(50, base_channels=8, style='caffe')
    assert py.layer2[0].conv1.stride == (1, 1) and py.layer2[0].conv2.stride == (2, 2)
    assert caffe.layer2[0].conv1.stride == (2, 2) and caffe.layer2[0].conv2.stride == (1, 1)
    assert py.layer2[0].downsample[0].stride == (2, 2) and py.layer1[0].downsample[0].stride == (1, 1) and py.layer1[1].downsample is None


@pytest.mark.parametrize('norm_eval', [True, False])
@pytest.mark.parametrize('frozen', [-1, 0, 1, 4])
def test_frozen_stages_and_norm_eval(frozen, norm_eval):
    from monorun_amd.resnet import ResNet
    net = ResNet(18, base_channels=8, frozen_stages=frozen, norm_eval=norm_eval)
    net.train()
    for name, p in net.named_parameters():
        stage = 0 if name.startswith(('conv1', 'bn1')) else int(name[5])
        assert p.requires_grad == (stage > frozen), name
    for name, m in net.named_modules():
        if isinstance(m, nn.BatchNorm2d):
            stage = 0 if name == 'bn1' else int(name[5])
            assert m.training == (not norm_eval and stage > frozen), name
    if frozen >= 1:
        assert not net.layer1.training and not net.layer1[0].conv1.training
    net.eval()
    assert not any(m.training for m in net.modules())
    off = ResNet(18, base_channels=8, norm_cfg=dict(type='BN', requires_grad=False))
    assert not any(p.requires_grad for n, p in off.named_parameters() if '.bn' in n or n.startswith('bn1') or 'downsample.1' in n)
    assert off.layer1[0].conv1.weight.requires_grad


def test_unsupported_arguments_and_pretrained(tmp_path, monkeypatch):
    from monorun_amd import resnet
    val = lambda t: float(t.detach())
    for bad in (dict(deep_stem=True), dict(avg_down=True), dict(dcn=dict(type='DCN')), dict(plugins=[dict(cfg=1)]), dict(with_cp=True),
                dict(conv_cfg=dict(type='ConvWS')), dict(norm_cfg=dict(type='GN', num_groups=32)), dict(norm_cfg=dict(type='SyncBN'))):
        with pytest.raises(NotImplementedError):
            resnet.ResNet(18, **bad)
    with pytest.raises(KeyError):
        resnet.ResNet(20)
    net = resnet.ResNet(18, base_channels=8)
    import socket
    monkeypatch.setattr(socket, 'socket', lambda *a, **k: pytest.fail('init_weights opened a socket'))
    for url in ('torchvision://resnet101', 'https://example.invalid/resnet101.pth', 'open-mmlab://resnet101_caffe'):
        with pytest.raises(ValueError, match='fetched'):
            net.init_weights(pretrained=url)
    net.init_weights()
    assert val(net.layer1[0].bn2.weight.abs().max()) == 0 and val(net.layer1[0].bn1.weight.min()) == 1 and val(net.bn1.bias.abs().max()) == 0
    w = net.layer2[0].conv1.weight
    assert abs(val(w.std()) - (2.0 / (16 * 9)) ** 0.5) < 0.02          # Kaiming, fan_out
    plain = resnet.ResNet(50, base_channels=8, zero_init_residual=False)
    plain.init_weights()
    assert val(plain.layer1[0].bn3.weight.min()) == 1
    zero = resnet.ResNet(50, base_channels=8)
    zero.init_weights()
    assert val(zero.layer1[0].bn3.weight.abs().max()) == 0 and val(zero.layer1[0].bn2.weight.min()) == 1
    other = resnet.ResNet(18, base_channels=8)
    other.init_weights()
    path = tmp_path / 'ckpt.pth'
    torch.save(dict(state_dict=net.state_dict(), meta=dict()), str(path))
    other.layer3[0].conv1.weight.data.zero_()
    other.init_weights(pretrained=str(path))
    assert torch.equal(other.layer3[0].conv1.weight, net.layer3[0].conv1.weight)
    try:
        import mmdet  # noqa: F401
        have = True
    except Exception:
        have = False
    if not have:
        assert resnet.register_with_mmdet() is False and resnet.register_with_mmdet(force=True) is False


def eager_resnet18(state, x, base, train_stats=False):
    """an independent composition of depth 18 from a state dict: F.conv2d, F.batch_norm, +, F.relu, F.max_pool2d"""
    def bn(t, p):
        return F.batch_norm(t, state[f'{p}.running_mean'].clone(), state[f'{p}.running_var'].clone(), state[f'{p}.weight'], state[f'{p}.bias'],
                            train_stats, 0.1, 1e-5)
    t = F.max_pool2d(F.relu(bn(F.conv2d(x, state['conv1.weight'], stride=2, padding=3), 'bn1')), 3, 2, 1)
    outs = []
    for s in range(4):
        for i in range(2):
            p = f'layer{s + 1}.{i}'
            stride = 2 if (s > 0 and i == 0) else 1
            out = F.relu(bn(F.conv2d(t, state[f'{p}.conv1.weight'], stride=stride, padding=1), f'{p}.bn1'))
            out = bn(F.conv2d(out, state[f'{p}.conv2.weight'], padding=1), f'{p}.bn2')
            if f'{p}.downsample.0.weight' in state:
                t = bn(F.conv2d(t, state[f'{p}.downsample.0.weight'], stride=stride), f'{p}.downsample.1')
            t = F.relu(out + t)
        outs.append(t)
    return outs


@pytest.mark.parametrize('norm_eval', [True, False])
def test_module_against_an_independent_eager_composition(norm_eval):
    from monorun_amd.resnet import ResNet
    g = torch.Generator().manual_seed(4)
    net = ResNet(18, base_channels=8, norm_eval=norm_eval).double()
    net.init_weights()
    with torch.no_grad():
        for name, v in net.state_dict().items():
            if 'num_batches' not in name and 'conv' not in name and 'downsample.0' not in name:
                v.copy_(torch.rand(v.shape, generator=g, dtype=torch.float64) + 0.5)
    net.train()
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    x = torch.randn(2, 3, 40, 56, generator=g, dtype=torch.float64)
    outs = net(x)
    want = eager_resnet18(state, x, 8, train_stats=not norm_eval)
    assert len(outs) == 4
    for a, b in zip(outs, want):
        a, b = a.detach(), b.detach()
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    grads = torch.autograd.grad(sum(o.sum() for o in outs), [p for p in net.parameters()])
    leaves = {k: v.clone().requires_grad_(True) for k, v in state.items() if v.dtype == torch.float64 and 'running' not in k}
    want = eager_resnet18({**state, **leaves}, x, 8, train_stats=not norm_eval)
    wg = torch.autograd.grad(sum(o.sum() for o in want), [leaves[n] for n, _ in net.named_parameters()])
    for (n, _), a, b in zip(net.named_parameters(), grads, wg):
        assert float((a - b).abs().max()) <= 1e-10 * max(1.0, float(b.abs().max())), n


# ------------------------------------------------------------------------------------------------ the loader's row
_PINNED = ('mr_bn_act_forward', 'mr_bn_act_backward_workspace_bytes', 'mr_bn_act_backward', 'mr_bn_relu_maxpool_forward')
_SCALAR = {'int': ctypes.c_int, 'float': ctypes.c_float, 'double': ctypes.c_double, 'size_t': ctypes.c_size_t, 'int64_t': ctypes.c_int64}


def _declared_prototypes(path):
    """[(return type, name, [arguments])] of a header, by a regex of this file's own (not `_lib.header_prototypes`)."""
    src = re.sub(r'/\*.*?\*/', ' ', open(path).read(), flags=re.S)
    found = re.findall(r'^((?:const\s+)?\w+[\s\*]+)(\w+)\s*\(([^)]*)\)\s*;', src, flags=re.M)
    return [(' '.join(ret.split()), name, [] if args.strip() in ('', 'void') else [' '.join(a.split()) for a in args.split(',')])
            for ret, name, args in found]


def test_loader_binds_the_backbone_header(monkeypatch):
    """the row of `_lib.LATER_HEADERS` this subsystem owns (nothing is asserted about the table's other rows): the pinned names are what the
    header declares, in order, and no other header's; the library exports each; restype, argtypes and arg_names are the declared ones; the
    header alone makes the library stale"""
    from monorun_amd import _lib
    key = 'backbone'
    assert key in _lib.LATER_HEADERS and key in _lib.all_header_keys() and key not in _lib.header_keys()
    assert not set(_PINNED) & set(_lib.exported_symbols())
    lib, raw = _lib.load(), ctypes.CDLL(_lib.SO)
    assert _lib.exported_symbols(key) == _lib.LATER_HEADERS[key][1] == _PINNED
    assert _lib.header_path(key) == os.path.join(ROOT, 'include', 'monorun_backbone.h')
    assert [n for n, _, _ in _lib.header_prototypes(_lib.header_path(key))] == list(_PINNED)
    declared = _declared_prototypes(_lib.header_path(key))
    assert [name for _, name, _ in declared] == list(_PINNED)
    for other in _lib.all_header_keys():
        if other != key:
            assert not set(_PINNED) & set(_lib.exported_symbols(other)), other
            assert not set(_PINNED) & {n for _, n, _ in _declared_prototypes(_lib.header_path(other))}, other
    for ret, name, args in declared:
        assert hasattr(raw, name), f'{name} declared but not exported'
        f = getattr(lib, name)
        names = [re.search(r'\w+$', a).group() for a in args]
        types = [a.replace('const ', '')[:-len(n)].strip() for a, n in zip(args, names)]
        assert len(set(names)) == len(names)
        has_stream = names[-1] == 'stream'
        assert has_stream == (name != 'mr_bn_act_backward_workspace_bytes')
        assert list(_lib.arg_names(name)) == (names[:-1] if has_stream else names), name
        assert f.restype is _SCALAR[ret], name
        assert list(f.argtypes) == [ctypes.c_void_p if '*' in t else _SCALAR[t] for t in types], name
        assert _lib.table_args(name) == ()
    src = open(_lib.header_path(key)).read()
    assert '#define MR_BN_CHUNK 4096' in src and ref.CHUNK == 4096 and '#define MR_BN_THREADS 256' in src and ref.THREADS == 256
    assert '#define MR_BN_FINAL_THREADS 64' in src and ref.FINAL_THREADS == 64
    assert not _lib._stale()
    so_time, real = os.path.getmtime(_lib.SO), os.path.getmtime
    monkeypatch.setattr(os.path, 'getmtime', lambda f: so_time + 10 if f == _lib.header_path(key) else real(f))
    assert _lib._stale()


def test_argument_checks_without_a_gpu():
    """all four entry points reject bad arguments before any HIP call: the codes of monorun_pnp.h (-1 bad argument, -2 unsupported)"""
    from monorun_amd import _lib
    lib = _lib.load()
    BAD, UNSUPPORTED = -1, -2
    one = ctypes.c_void_p(16)                       # never dereferenced: every call below is rejected before a launch, or launches nothing
    base = dict(n_images=1, channels=2, height=3, width=4, eps=1e-5, relu=1, mean=one, var=one, weight=one, bias=one)

    def fwd(**over):
        a = dict(base, x=one, r=one, y=one)
        a.update(over)
        return lib.mr_bn_act_forward(*_lib.pack('mr_bn_act_forward', a), None)

    def bwd(**over):
        a = dict(base, g=one, y=one, x=one, grad_x=one, grad_r=one, grad_weight=one, grad_bias=one, workspace=one)
        a.pop('bias')
        a.update(over)
        return lib.mr_bn_act_backward(*_lib.pack('mr_bn_act_backward', a), None)

    def stem(**over):
        a = dict(base, x=one, p=one)
        a.pop('relu')
        a.update(over)
        return lib.mr_bn_relu_maxpool_forward(*_lib.pack('mr_bn_relu_maxpool_forward', a), None)

    for call in (fwd, bwd, stem):
        for k in ('n_images', 'channels', 'height', 'width'):
            assert call(**{k: 0}) == BAD and call(**{k: -1}) == BAD, k
        assert call(mean=None) == BAD and call(var=None) == BAD and call(x=None) == BAD
        assert call(eps=-1.0) == BAD and call(eps=float('nan')) == BAD and call(eps=float('inf')) == BAD
        assert call(n_images=1 << 11, channels=1 << 10, height=1 << 5, width=1 << 5) == UNSUPPORTED        # 2^31 elements
        assert call(n_images=1 << 16, channels=1 << 16, height=1, width=1) == UNSUPPORTED
        assert call(n_images=1, channels=1, height=1 << 16, width=1 << 16) == UNSUPPORTED
    assert fwd(relu=2) == BAD and fwd(relu=-1) == BAD and fwd(y=None) == BAD
    assert bwd(relu=2) == BAD and bwd(g=None) == BAD and bwd(y=None) == BAD and bwd(workspace=None) == BAD
    assert bwd(x=None) == BAD
    assert bwd(grad_x=None, grad_r=None, grad_weight=None, grad_bias=None, x=None, workspace=None) == 0        # nothing asked: nothing launched
    assert bwd(grad_x=None, grad_r=None, grad_weight=None, grad_bias=None, relu=0, y=None, x=None, workspace=None) == 0
    assert stem(p=None) == BAD
    ws = lib.mr_bn_act_backward_workspace_bytes
    assert ws(1, 2, 3, 4) == 8 * 2 and ws(2, 3, 91, 93) == 8 * 2 * 3 * 3 and ws(3, 256, 96, 312) == 8 * 3 * 256 * 8
    from monorun_amd import resnet
    assert resnet.CHUNK == ref.CHUNK == 4096 and ws(2, 5, 64, 65) == 4 * 2 * 2 * 5 * -(-(64 * 65) // resnet.CHUNK)
    assert ws(0, 2, 3, 4) == 0 and ws(1 << 11, 1 << 10, 1 << 5, 1 << 5) == 0
