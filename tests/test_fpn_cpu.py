"""The feature pyramid without a GPU: the torch restatement against the numpy definition (tests/fpn_ref.py) and against the
reference's literal ``F.interpolate`` chain, the two modules, the loader's row and the argument checks of the two entry points."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import fpn_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
CASES = [(name, shape) for name in ref.PYRAMIDS for shape in ((2, 5),)] + [('wide', (1, 40)), ('pow2', (1, 1))]


def literal_chain(lats, lower_scale):
    """the reference's forward between its convolutions, as it is written: in place, F.interpolate for both up-samples"""
    lats = [t.clone() for t in lats]
    for i in range(len(lats) - 1, 0, -1):
        lats[i - 1] += F.interpolate(lats[i], size=lats[i - 1].shape[2:], mode='nearest')
    low = F.interpolate(lats[0], scale_factor=lower_scale, mode='bilinear', align_corners=False) if lower_scale else None
    return lats, low


def run_torch(fn, c, lower_scale):
    """outputs and gradients of a torch implementation on a case of fpn_ref"""
    lats = [torch.from_numpy(t.copy()).requires_grad_(True) for t in c['lats']]
    m, low = fn(lats, lower_scale)
    outs = list(m) + ([low] if lower_scale else [])
    gs = [torch.from_numpy(g.copy()) for g in c['g_m']] + ([torch.from_numpy(c['g_low'].copy())] if lower_scale else [])
    grads = torch.autograd.grad(outs, lats, gs)
    return [t.detach().numpy() for t in m], (low.detach().numpy() if lower_scale else None), [g.numpy() for g in grads]


def gradient_bound(c, shape, lower_scale):
    """|a - b| for two fp32 evaluations, in any order, of the sums G[l][p]: a sum of n terms carries at most (n - 1) u sum|terms| in either
    order (the weights, multiples of 1/16, and their products are exact), so 2 n u A with A = the backward of the absolute gradients (the
    weights are not negative) and n = 17 per pixel of the subtree (itself and at most 16 low pixels), counted by the backward of ones."""
    absolute = ref.backward(c['sizes'], shape, lower_scale, [np.abs(g) for g in c['g_m']], np.abs(c['g_low']) if lower_scale else None)
    ones = ref.backward(c['sizes'], shape, 0, [np.ones_like(g) for g in c['g_m']], None)
    return [2 * 17 * n.astype(np.float64) * U * a.astype(np.float64) * 1.01 for n, a in zip(ones, absolute)]


@pytest.mark.parametrize('lower_scale', [0, 2])
@pytest.mark.parametrize('name,shape', CASES)
def test_restatement_matches_the_definition(name, shape, lower_scale):
    from monorun_amd.fpn import fpn_topdown_torch
    c = ref.case(name, shape, lower_scale)
    m, low, grads = run_torch(fpn_topdown_torch, c, lower_scale)
    for l, (a, b) in enumerate(zip(m, c['m'])):
        assert np.array_equal(a, b), f'merged level {l}'
    if lower_scale:
        assert low.shape == c['low'].shape and np.array_equal(low, c['low']), 'low, evaluated in the stated order'
    for l, (a, b, bound) in enumerate(zip(grads, c['grads'], gradient_bound(c, shape, lower_scale))):
        err = np.abs(a.astype(np.float64) - b)
        print(f'{name} level {l}: largest gradient error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}')
        assert np.all(err <= bound), f'gradient of level {l}'


@pytest.mark.parametrize('name,shape', CASES)
def test_restatement_matches_the_literal_chain(name, shape):
    """merged levels bit for bit; low within 8 u max|m[0]|: each side rounds at most four times on the path of any tap of a convex
    combination"""
    from monorun_amd.fpn import fpn_topdown_torch
    c = ref.case(name, shape, 2)
    lats = [torch.from_numpy(t.copy()) for t in c['lats']]
    m, low = fpn_topdown_torch(lats, 2)
    lm, llow = literal_chain(lats, 2)
    for a, b in zip(m, lm):
        assert torch.equal(a, b)
    err, bound = (low - llow).abs().max().item(), 8 * U * m[0].abs().max().item()
    print(f'{name}: low against F.interpolate: {err:.3e} (bound {bound:.3e})')
    assert low.shape == llow.shape and err <= bound


@pytest.mark.parametrize('name,shape', CASES)
def test_integer_data_is_exact_in_every_order(name, shape):
    """integers in [-64, 64]: every value is exact whatever the order, so the restatement, the definition and the literal chain with its
    autograd agree bit for bit, gradients included"""
    from monorun_amd.fpn import fpn_topdown_torch
    c = ref.case(name, shape, 2, True)
    got, want = run_torch(fpn_topdown_torch, c, 2), run_torch(literal_chain, c, 2)
    for a, b, d in zip(got[0] + [got[1]] + got[2], want[0] + [want[1]] + want[2], c['m'] + [c['low']] + c['grads']):
        assert np.array_equal(a, b) and np.array_equal(a, d)


def test_other_scales_and_dtypes_run_the_restatement():
    from monorun_amd import fpn
    g = torch.Generator().manual_seed(3)
    lats = [torch.randn(1, 3, h, w, generator=g) for h, w in ref.PYRAMIDS['ceil_odd']]
    assert not fpn.hip_ok(lats, 2) and not fpn.hip_ok(lats, 4), 'CPU tensors never take the HIP path'
    m, low = fpn.fpn_topdown(lats, 4)
    want = F.interpolate(m[0], scale_factor=4, mode='bilinear', align_corners=False)
    assert low.shape == want.shape and (low - want).abs().max().item() <= 8 * U * m[0].abs().max().item()
    mh, lowh = fpn.fpn_topdown([t.half() for t in lats], 2)
    assert lowh.dtype == torch.float16 and all(t.dtype == torch.float16 for t in mh)
    assert torch.allclose(lowh.float(), fpn.fpn_topdown(lats, 2)[1], atol=5e-2)
    md, lowd = fpn.fpn_topdown([t.double() for t in lats], 2)
    assert lowd.dtype == torch.float64 and torch.allclose(lowd, F.interpolate(md[0], scale_factor=2, mode='bilinear', align_corners=False), atol=1e-12)
    assert fpn.fpn_topdown(lats, 0)[1] is None and fpn.fpn_topdown(lats[:1], 0)[0][0] is lats[0]
    assert fpn.in_pyramid_rule(ref.PYRAMIDS['wide']) and not fpn.in_pyramid_rule(ref.PYRAMIDS['outside_rule'])
    assert all(fpn.in_pyramid_rule(s) == ref.in_rule(s) for s in ref.PYRAMIDS.values())
    assert fpn.in_pyramid_rule([(96, 312), (48, 156), (24, 78), (12, 39)]) and fpn.in_pyramid_rule([(7, 9), (7, 9)])


# ------------------------------------------------------------------------------------------------ the modules
REFERENCE_CFG = dict(in_channels=[256, 512, 1024, 2048], out_channels=256, num_outs=5, num_lower_outs=1)


def test_fpnplus_state_dict_is_mmdets():
    from monorun_amd.fpn import FPNplus
    neck = FPNplus(**REFERENCE_CFG)
    want = {}
    for i, cin in enumerate(REFERENCE_CFG['in_channels']):
        want[f'lateral_convs.{i}.conv.weight'], want[f'lateral_convs.{i}.conv.bias'] = (256, cin, 1, 1), (256,)
        want[f'fpn_convs.{i}.conv.weight'], want[f'fpn_convs.{i}.conv.bias'] = (256, 256, 3, 3), (256,)
    want['lower_fpn_convs.0.conv.weight'], want['lower_fpn_convs.0.conv.bias'] = (256, 256, 3, 3), (256,)
    assert {k: tuple(v.shape) for k, v in neck.state_dict().items()} == want
    neck.init_weights()
    w = neck.lateral_convs[3].conv.weight.detach()
    assert float(w.abs().max()) <= (6.0 / (2048 + 256)) ** 0.5 + 1e-6 and float(w.std()) > 0.02            # Xavier-uniform
    assert all(float(m.bias.abs().max()) == 0 for m in neck.modules() if isinstance(m, torch.nn.Conv2d))
    for bad in (dict(conv_cfg=dict(type='Conv2d')), dict(norm_cfg=dict(type='BN')), dict(act_cfg=dict(type='ReLU'))):
        with pytest.raises(NotImplementedError):
            FPNplus(**REFERENCE_CFG, **bad)


def _inputs(channels, sizes, seed=1, n=2):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, c, h, w, generator=g) for c, (h, w) in zip(channels, sizes)]


def test_fpnplus_outputs_in_the_references_order():
    from monorun_amd.fpn import FPNplus
    chans, sizes = [3, 5, 6, 4], ref.PYRAMIDS['ceil_odd']
    neck = FPNplus(chans, 8, 5, num_lower_outs=1)
    neck.init_weights()
    xs = _inputs(chans, sizes)
    outs = neck(xs)
    assert isinstance(outs, tuple) and len(outs) == 6
    assert [tuple(o.shape) for o in outs] == [(2, 8, 26, 14), (2, 8, 13, 7), (2, 8, 7, 4), (2, 8, 4, 2), (2, 8, 2, 1), (2, 8, 1, 1)]
    # the eager composition, as the reference writes it
    lat = [neck.lateral_convs[i](x) for i, x in enumerate(xs)]
    m, low = literal_chain(lat, 2)
    want = [neck.lower_fpn_convs[0](low)] + [neck.fpn_convs[i](t) for i, t in enumerate(m)]
    want.append(F.max_pool2d(want[-1], 1, stride=2))
    for a, b in zip(outs, want):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-5)
    assert torch.equal(outs[5], F.max_pool2d(outs[4], 1, stride=2))
    # two lower maps: x4 first, then x2; none: mmdet's FPN
    two = FPNplus(chans, 8, 4, num_lower_outs=2)
    o2 = two(xs)
    assert [tuple(o.shape[2:]) for o in o2] == [(52, 28), (26, 14), (13, 7), (7, 4), (4, 2), (2, 1)]
    lat = [two.lateral_convs[i](x) for i, x in enumerate(xs)]
    m, _ = literal_chain(lat, 0)
    assert torch.allclose(o2[0], two.lower_fpn_convs[0](F.interpolate(m[0], scale_factor=4, mode='bilinear', align_corners=False)), rtol=1e-5, atol=1e-5)
    assert len(FPNplus(chans, 8, 4, num_lower_outs=0)(xs)) == 4


@pytest.mark.parametrize('mode', [False, True, 'on_input', 'on_lateral', 'on_output'])
@pytest.mark.parametrize('relu', [False, True])
def test_fpn_extra_levels_follow_mmdet(mode, relu):
    from monorun_amd.fpn import FPN
    chans, sizes = [3, 5, 6, 4], ref.PYRAMIDS['wide']
    neck = FPN(chans, 8, 5, start_level=1, add_extra_convs=mode, relu_before_extra_convs=relu)
    assert neck.add_extra_convs == ('on_input' if mode is True else mode)
    assert len(neck.lateral_convs) == 3 and len(neck.fpn_convs) == (5 if mode else 3)
    if mode:
        assert neck.fpn_convs[3].conv.in_channels == (4 if neck.add_extra_convs == 'on_input' else 8) and neck.fpn_convs[3].conv.stride == (2, 2)
    xs = _inputs(chans, sizes)
    outs = neck(xs)
    lat = [conv(xs[i + 1]) for i, conv in enumerate(neck.lateral_convs)]
    m, _ = literal_chain(lat, 0)
    want = [neck.fpn_convs[i](t) for i, t in enumerate(m)]
    if not mode:
        want += [F.max_pool2d(want[-1], 1, stride=2)]
        want += [F.max_pool2d(want[-1], 1, stride=2)]
    else:
        source = {'on_input': xs[3], 'on_lateral': m[-1], 'on_output': want[-1]}[neck.add_extra_convs]
        want.append(neck.fpn_convs[3](source))
        want.append(neck.fpn_convs[4](F.relu(want[-1]) if relu else want[-1]))
    assert len(outs) == 5
    for a, b in zip(outs, want):
        assert a.shape == b.shape and torch.allclose(a, b, rtol=1e-5, atol=1e-5)


def test_fpn_end_level_another_upsample_and_the_registry():
    from monorun_amd import fpn
    chans, sizes = [3, 5, 6, 4], ref.PYRAMIDS['pow2']
    xs = _inputs(chans, sizes)
    neck = fpn.FPN(chans, 8, 2, start_level=1, end_level=3)
    assert len(neck(xs)) == 2 and len(neck.lateral_convs) == 2
    with pytest.raises(AssertionError):
        fpn.FPN(chans, 8, 3, start_level=1, end_level=3)
    fixed = fpn.FPN(chans, 8, 4, upsample_cfg=dict(mode='nearest', scale_factor=2))
    fixed.load_state_dict(fpn.FPN(chans, 8, 4).state_dict())
    plain = fpn.FPN(chans, 8, 4)
    plain.load_state_dict(fixed.state_dict())
    for a, b in zip(fixed(xs), plain(xs)):
        assert torch.equal(a, b)            # on a power-of-two pyramid the two rules read the same pixels
    bil = fpn.FPN(chans, 8, 4, upsample_cfg=dict(mode='bilinear', align_corners=False))
    assert len(bil(xs)) == 4
    try:
        import mmdet  # noqa: F401
        have = True
    except Exception:
        have = False
    if not have:
        assert fpn.register_with_mmdet() is False and fpn.register_with_mmdet(force=True) is False


# ------------------------------------------------------------------------------------------------ the loader's row
_PINNED = ('mr_fpn_topdown_forward', 'mr_fpn_topdown_backward')
_SCALAR = {'int': ctypes.c_int, 'float': ctypes.c_float, 'double': ctypes.c_double, 'size_t': ctypes.c_size_t, 'int64_t': ctypes.c_int64}


def _declared_prototypes(path):
    """[(return type, name, [arguments])] of a header, by a regex of this file's own (not `_lib.header_prototypes`)."""
    src = re.sub(r'/\*.*?\*/', ' ', open(path).read(), flags=re.S)
    found = re.findall(r'^((?:const\s+)?\w+[\s\*]+)(\w+)\s*\(([^)]*)\)\s*;', src, flags=re.M)
    return [(' '.join(ret.split()), name, [] if args.strip() in ('', 'void') else [' '.join(a.split()) for a in args.split(',')])
            for ret, name, args in found]


def test_loader_binds_the_fpn_header(monkeypatch):
    """the row of `_lib.LATER_HEADERS` this subsystem owns (nothing is asserted about the table's other rows): the pinned names are what the
    header declares, in order, and no other header's; the library exports each; restype, argtypes and arg_names are the declared ones; the
    header alone makes the library stale"""
    from monorun_amd import _lib, fpn
    key = 'fpn'
    assert key in _lib.LATER_HEADERS and key in _lib.all_header_keys() and key not in _lib.header_keys()
    assert not set(_PINNED) & set(_lib.exported_symbols())
    lib, raw = _lib.load(), ctypes.CDLL(_lib.SO)
    assert _lib.exported_symbols(key) == _lib.LATER_HEADERS[key][1] == _PINNED
    assert _lib.header_path(key) == os.path.join(ROOT, 'include', 'monorun_fpn.h')
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
        assert len(set(names)) == len(names) and names[-1] == 'stream'
        assert list(_lib.arg_names(name)) == names[:-1], name
        assert f.restype is _SCALAR[ret], name
        assert list(f.argtypes) == [ctypes.c_void_p if '*' in t else _SCALAR[t] for t in types], name
    assert set(_lib.table_args('mr_fpn_topdown_forward')) == {'lat', 'merged'}
    assert set(_lib.table_args('mr_fpn_topdown_backward')) == {'grad_merged', 'grad_lat'}
    src = open(_lib.header_path(key)).read()
    assert '#define MR_FPN_MAX_LEVELS 6' in src and fpn.MAX_LEVELS == 6
    assert not _lib._stale()
    so_time, real = os.path.getmtime(_lib.SO), os.path.getmtime
    monkeypatch.setattr(os.path, 'getmtime', lambda f: so_time + 10 if f == _lib.header_path(key) else real(f))
    assert _lib._stale()


def test_argument_checks_without_a_gpu():
    """both entry points reject bad arguments before any HIP call: the codes of monorun_pnp.h (-1 bad argument, -2 unsupported)"""
    from monorun_amd import _lib
    lib = _lib.load()
    BAD, UNSUPPORTED = -1, -2
    one = ctypes.c_void_p(16)                       # never dereferenced: every call below is rejected before a launch, or launches nothing

    def tables(sizes, null=()):
        L = len(sizes)
        return dict(level_h=(ctypes.c_int * L)(*[h for h, _ in sizes]), level_w=(ctypes.c_int * L)(*[w for _, w in sizes]), n_levels=L,
                    maps=(ctypes.c_void_p * L)(*[None if l in null else 16 for l in range(L)]))

    def fwd(sizes=((8, 8), (4, 4)), null=(), null_merged=(), **over):
        t = tables(sizes, null)
        a = dict(n_images=1, channels=2, lower_scale=2, low=one, level_h=t['level_h'], level_w=t['level_w'], n_levels=t['n_levels'],
                 lat=t['maps'], merged=tables(sizes, null_merged)['maps'])
        a.update(over)
        return lib.mr_fpn_topdown_forward(*_lib.pack('mr_fpn_topdown_forward', a), None)

    def bwd(sizes=((8, 8), (4, 4)), null=(), **over):
        t = tables(sizes, null)
        a = dict(n_images=1, channels=2, lower_scale=2, grad_low=one, level_h=t['level_h'], level_w=t['level_w'], n_levels=t['n_levels'],
                 grad_merged=t['maps'], grad_lat=t['maps'])
        a.update(over)
        return lib.mr_fpn_topdown_backward(*_lib.pack('mr_fpn_topdown_backward', a), None)

    for call in (fwd, bwd):
        assert call(n_levels=0) == BAD and call(n_images=0) == BAD and call(channels=0) == BAD
        assert call(lower_scale=1) == BAD and call(lower_scale=4) == BAD and call(lower_scale=-2) == BAD
        assert call(sizes=((8, 0), (4, 4))) == BAD and call(sizes=((8, 8), (0, 4))) == BAD
        assert call(level_h=None) == BAD and call(level_w=None) == BAD
        assert call(sizes=((64, 64),) * 3 + ((32, 32),) * 4) == UNSUPPORTED                     # seven levels
        assert call(sizes=ref.PYRAMIDS['outside_rule']) == UNSUPPORTED                          # 7 > 2 * 3
        assert call(sizes=((4, 4), (8, 8))) == UNSUPPORTED and call(sizes=((8, 9), (4, 4))) == UNSUPPORTED
        assert call(sizes=((1 << 15, 1 << 15), (1 << 14, 1 << 14))) == UNSUPPORTED             # a slab beyond 32-bit offsets
        assert call(sizes=((1 << 14, 1 << 14), (1 << 13, 1 << 13)), channels=4) == UNSUPPORTED # low's slab beyond them
        assert call(n_images=1 << 16, channels=1 << 16) == UNSUPPORTED
    assert fwd(lat=None) == BAD and fwd(merged=None) == BAD and fwd(low=None) == BAD and fwd(null=(1,)) == BAD and fwd(null_merged=(0,)) == BAD
    assert bwd(grad_lat=None) == BAD
    assert fwd(sizes=((8, 8),), lower_scale=0, merged=None, low=None) == 0                     # one level, no lower map: nothing is launched
