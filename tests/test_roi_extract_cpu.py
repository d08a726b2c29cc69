"""The RoI extractors without a GPU: the torch restatement against the fp64 definition (tests/roi_extract_ref.py), the
level rule, roi_rescale, the modules, the loader's second header table and the argument checks of the two entry points."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import roi_extract_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def torch_run(name, dtype):
    """the largest error ratios (forward, grad_feats) of the restatement on one case, maps of the given dtype"""
    from monorun_amd.roi_extractor import roi_extract_torch
    case = ref.CASES[ref.IDS.index(name)]
    feats, go = ref.make_inputs(case)
    out, outa, grads, gradsa = ref.extract(case, feats, go)
    ft = [torch.from_numpy(f).to(dtype).requires_grad_(True) for f in feats]
    got = roi_extract_torch(ft, torch.from_numpy(case['rois']), ref.STRIDES[:case['L']], ref.FINEST, case['size'], case['sampling_ratio'],
                            case['aligned'])
    assert got.shape == out.shape and got.dtype == dtype
    if got.numel() == 0:
        return 0.0, 0.0
    got.backward(torch.from_numpy(go).to(dtype))
    assert all(f.grad is not None for f in ft), 'a level without RoIs gets a zero gradient, not None'
    return (ref.ratio(got.detach().numpy(), out, outa),
            max(ref.ratio(f.grad.numpy(), g, ga) for f, g, ga in zip(ft, grads, gradsa)))


@pytest.mark.parametrize('name', ref.IDS)
def test_restatement_matches_the_definition_within_the_bound(name):
    """forward and autograd's grad_feats of the fp32 restatement against the analytic ones, within the bound"""
    fwd, grad = torch_run(name, torch.float32)
    print(f'{name}: error / (2^-23 sum|terms|): forward {fwd:.2f} grad_feats {grad:.2f}')
    assert fwd <= ref.C_BOUND and grad <= ref.C_BOUND


def test_the_bound_constant_is_the_measured_one():
    """C_MEASURED of roi_extract_ref is what the fp32 restatement shows on CASES (torch's kernels differ a little between builds: the
    recorded figure must cover this build's and be no more than twice it)"""
    worst = np.max([torch_run(name, torch.float32) for name in ref.IDS], axis=0)
    print('fp32 restatement, error / (2^-23 sum|terms|): forward %.2f grad_feats %.2f' % tuple(worst))
    assert worst.max() <= ref.C_MEASURED * 1.05 and ref.C_MEASURED <= 2 * worst.max()
    assert ref.C_BOUND == 4 * ref.C_MEASURED


def test_degenerate_rois_give_zeros_and_cases_cover_every_kind():
    from monorun_amd.roi_extractor import map_roi_levels, valid_rois
    case = ref.CASES[0]
    rois, L = case['rois'], case['L']
    levels = ref.roi_levels(rois, L)
    assert torch.equal(map_roi_levels(torch.from_numpy(rois), L, ref.FINEST), torch.from_numpy(levels))
    sizes = ref.level_sizes(L)
    want = np.array([ref.roi_valid(r, sizes[l], ref.STRIDES[l], ref.N_IMAGES, case['size'], 0, True) for r, l in zip(rois, levels)])
    got = valid_rois(rois, levels, sizes, ref.STRIDES[:L], ref.N_IMAGES, case['size'], 0, True)
    assert np.array_equal(got, want)
    bad = ~want
    assert (~np.isfinite(rois[:, 1:]).all(1))[bad].sum() == 2 and np.isnan(rois[bad, 0]).sum() == 1           # NaN, inf, NaN image
    assert (rois[bad, 0] == 2).sum() == 1 and (rois[bad, 0] == -1).sum() == 1 and bad.sum() >= 7              # images outside; huge grids
    feats, _ = ref.make_inputs(case)
    out = ref.extract(case, feats)[0]
    assert np.all(out[bad] == 0) and set(levels[want]) == {0, 1, 2, 3} and set(rois[want, 0]) == {0.0, 1.0}
    one = ref.CASES[ref.IDS.index('c5_L5_7x7_one_image')]
    lv1 = ref.roi_levels(one['rois'], 5)
    assert 4 in set(lv1) and not (one['rois'][:, 0] == 1).any()


def test_level_rule_is_floor_log2_away_from_the_powers_of_two():
    """the rule equals mmdet's floor(log2(v)).clamp(0, L - 1) on every RoI of CASES whose v is not within 1e-4 (relative) of a power of two;
    at least 90 % of all the RoIs of CASES are compared (a NaN v has no floor(log2): such a RoI is not compared and counts as unchecked;
    an infinite v is compared: level L - 1)"""
    from monorun_amd.roi_extractor import map_roi_levels
    total = checked = 0
    for case in ref.CASES:
        rois, L = torch.from_numpy(case['rois']), case['L']
        if rois.shape[0] == 0:
            continue
        got = map_roi_levels(rois, L, ref.FINEST)
        assert np.array_equal(got.numpy(), ref.roi_levels(case['rois'], L))
        scale = torch.sqrt((rois[:, 3] - rois[:, 1]) * (rois[:, 4] - rois[:, 2]))
        v = (scale / ref.FINEST + 1e-6).double()
        near = torch.zeros_like(v, dtype=torch.bool)
        for i in range(-30, 40):
            near |= (v / 2.0 ** i - 1).abs() < 1e-4
        use = ~near & ~torch.isnan(v)
        mmdet = torch.floor(torch.log2(scale / ref.FINEST + 1e-6)).clamp(min=0, max=L - 1).long()
        assert torch.equal(got[use], mmdet[use])
        total += int(rois.shape[0])
        checked += int(use.sum())
    assert checked >= 0.9 * total, (checked, total)


def test_roi_rescale_closed_form():
    from monorun_amd.roi_extractor import roi_rescale
    rois = torch.tensor([[0, 10.0, 20.0, 30.0, 60.0], [1, -4.0, 2.0, 4.0, 3.0]], dtype=torch.float64)
    got = roi_rescale(rois, 1.5)
    want = torch.tensor([[0, 5.0, 10.0, 35.0, 70.0], [1, -6.0, 1.75, 6.0, 3.25]], dtype=torch.float64)
    assert torch.equal(got, want)
    assert torch.equal(roi_rescale(rois, 1.0), rois)


def _maps(C, sizes, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(ref.N_IMAGES, C, h, w, generator=g) for h, w in sizes]


def test_modules_follow_the_reference():
    from monorun_amd import roi_extractor as R
    layer = dict(type='RoIAlign', output_size=7, sampling_ratio=0)
    sizes = [(48, 80)] + ref.level_sizes(5)
    feats = _maps(4, sizes)
    rois = torch.from_numpy(ref.CASES[0]['rois'])
    mod = R.SingleRoIExtractorMod(layer, 4, list(ref.STRIDES), finest_scale=ref.FINEST, starting_level=1)
    plain = R.SingleRoIExtractor(dict(layer), 4, list(ref.STRIDES), finest_scale=ref.FINEST)
    assert mod.num_inputs == plain.num_inputs == 5 and not list(mod.parameters()) and mod.init_weights() is None
    assert layer == dict(type='RoIAlign', output_size=7, sampling_ratio=0), 'the config is not consumed'
    assert [l.spatial_scale for l in plain.roi_layers] == [1 / s for s in ref.STRIDES] and plain.roi_layers[0].output_size == (7, 7)
    a, b = mod(feats, rois), plain(feats[1:], rois)
    assert a.shape == (rois.shape[0], 4, 7, 7) and torch.equal(a, b)
    want = R.roi_extract_torch(feats[1:], rois, ref.STRIDES, ref.FINEST, 7)
    assert torch.equal(a, want)
    # roi_scale_factor: the level from the unscaled RoIs, the pooling from the rescaled ones
    good = rois[torch.isfinite(rois).all(1)]
    c = plain(feats[1:], good, roi_scale_factor=1.25)
    want = R.roi_extract_torch(feats[1:], R.roi_rescale(good, 1.25), ref.STRIDES, ref.FINEST, 7, level_rois=good)
    assert torch.equal(c, want)
    lv, lv_scaled = R.map_roi_levels(good, 5, ref.FINEST), R.map_roi_levels(R.roi_rescale(good, 1.25), 5, ref.FINEST)
    assert not torch.equal(lv, lv_scaled), 'the case must tell the two rules apart'
    # no RoIs; half maps come back half
    assert plain(feats[1:], rois[:0]).shape == (0, 4, 7, 7)
    h = plain([f.half() for f in feats[1:]], good[:3])
    assert h.dtype == torch.float16 and torch.allclose(h.float(), plain(feats[1:], good[:3]), atol=2e-2)
    # a single map: every RoI on level 0, as mmdet's early return
    one = R.SingleRoIExtractor(dict(layer), 4, [4])
    assert torch.equal(one(feats[2:3], good), R.RoIAlign(7, 0.25)(feats[2], good))
    assert torch.equal(R.map_roi_levels(good, 1, 56), torch.zeros(good.shape[0], dtype=torch.int64))


def test_gradient_is_the_transpose_and_differentiable():
    """the op is linear in the maps: its gradient under create_graph=True is differentiable in grad_out, and differentiating
    <grad_feats, R> by grad_out gives the extraction of R (the adjoint identity)"""
    from monorun_amd.roi_extractor import roi_extract
    feats = [f.requires_grad_(True) for f in _maps(2, ref.level_sizes(2))]
    probe = _maps(2, ref.level_sizes(2), seed=6)
    rois = torch.tensor([[0, 3.0, 4.0, 17.0, 15.0], [1, 20.0, 10.0, 50.0, 40.0], [1, 2.0, 2.0, 9.0, 8.0]])
    args = (rois, ref.STRIDES[:2], ref.FINEST, (2, 3))
    out = roi_extract(feats, *args)
    go = torch.randn(out.shape, generator=torch.Generator().manual_seed(7)).requires_grad_(True)
    grads = torch.autograd.grad(out, feats, go, create_graph=True)
    sum((g * p).sum() for g, p in zip(grads, probe)).backward()
    assert torch.allclose(go.grad, roi_extract(probe, *args), rtol=1e-5, atol=1e-6)


_PINNED = {'roi': ('mr_roi_extract_forward', 'mr_roi_extract_backward')}
_SCALAR = {'int': ctypes.c_int, 'float': ctypes.c_float, 'double': ctypes.c_double, 'size_t': ctypes.c_size_t, 'int64_t': ctypes.c_int64}


def _declared_prototypes(path):
    """[(return type, name, [arguments])] of a header, by a regex of this file's own (not `_lib.header_prototypes`)."""
    src = re.sub(r'/\*.*?\*/', ' ', open(path).read(), flags=re.S)
    found = re.findall(r'^((?:const\s+)?\w+[\s\*]+)(\w+)\s*\(([^)]*)\)\s*;', src, flags=re.M)
    return [(' '.join(ret.split()), name, [] if args.strip() in ('', 'void') else [' '.join(a.split()) for a in args.split(',')])
            for ret, name, args in found]


@pytest.mark.parametrize('key', ['roi'])
def test_loader_binds_every_extra_header(key, monkeypatch):
    """`_lib.EXTRA_HEADERS` as tests/test_capi_and_host.py pins `_lib.HEADERS`: the pinned tuple is what the header declares, in order, and
    shares no name with any other header; the library exports every symbol; the loaded function has the declared restype and argtypes and
    `arg_names` the declared names; the header alone makes the library stale; the first table and a bare exported_symbols() are untouched."""
    from monorun_amd import _lib
    assert list(_lib.EXTRA_HEADERS) == ['roi'] and set(_PINNED) == set(_lib.EXTRA_HEADERS)
    assert list(_lib.HEADERS) == ['pnp', 'heads', 'train', 'targets', 'global', 'carafe'] and not set(_lib.HEADERS) & set(_lib.EXTRA_HEADERS)
    assert _lib.header_keys() == tuple(_lib.HEADERS) + tuple(_lib.EXTRA_HEADERS)
    assert _lib.exported_symbols() == tuple(n for k in _lib.HEADERS for n in _lib.exported_symbols(k))
    lib, raw = _lib.load(), ctypes.CDLL(_lib.SO)
    pinned = _lib.exported_symbols(key)
    assert pinned == _lib.EXTRA_HEADERS[key][1] == _PINNED[key]
    assert _lib.header_path(key) == os.path.join(ROOT, 'include', _lib.EXTRA_HEADERS[key][0])
    assert [n for n, _, _ in _lib.header_prototypes(_lib.header_path(key))] == list(pinned)
    declared = _declared_prototypes(_lib.header_path(key))
    assert [name for _, name, _ in declared] == list(pinned) and len(set(pinned)) == len(pinned)
    for other in _lib.header_keys():
        if other != key:
            assert not set(pinned) & set(_lib.exported_symbols(other)), other
            assert not set(pinned) & {n for _, n, _ in _declared_prototypes(_lib.header_path(other))}, other
    for ret, name, args in declared:
        assert hasattr(raw, name), f'{name} declared in {_lib.EXTRA_HEADERS[key][0]} but not exported'
        f = getattr(lib, name)
        names = [re.search(r'\w+$', a).group() for a in args]
        types = [a.replace('const ', '')[:-len(n)].strip() for a, n in zip(args, names)]
        assert len(set(names)) == len(names) and names[-1] == 'stream', name
        assert list(_lib.arg_names(name)) == names[:-1], name
        assert f.restype is _SCALAR[ret], name
        assert list(f.argtypes) == [ctypes.c_void_p if '*' in t else _SCALAR[t] for t in types], name
    assert set(_lib.table_args('mr_roi_extract_forward')) == {'feats'} and set(_lib.table_args('mr_roi_extract_backward')) == {'grad_feats'}
    assert not _lib._stale()
    so_time, real = os.path.getmtime(_lib.SO), os.path.getmtime
    monkeypatch.setattr(os.path, 'getmtime', lambda f: so_time + 10 if f == _lib.header_path(key) else real(f))
    assert _lib._stale()


def test_argument_checks_without_a_gpu():
    """both entry points reject bad arguments before any HIP call: the codes of monorun_pnp.h (-1 bad argument, -2 unsupported)"""
    from monorun_amd import _lib
    lib = _lib.load()
    BAD, UNSUPPORTED = -1, -2
    one = ctypes.c_void_p(16)                       # never dereferenced: every call below is rejected before a launch
    def tables(L, h=4, w=4, s=2, null_map=False):
        return dict(level_h=(ctypes.c_int * L)(*[h] * L), level_w=(ctypes.c_int * L)(*[w] * L), level_stride=(ctypes.c_int * L)(*[s] * L),
                    n_levels=L, maps=(ctypes.c_void_p * L)(*[None if null_map else 16] * L))
    base = dict(n_images=1, channels=2, rois=one, level_rois=None, n_rois=3, finest_scale=56.0, out_h=7, out_w=7, sampling_ratio=0, aligned=1)

    def fwd(L=1, table={}, **over):
        t = tables(L, **table)
        a = dict(base, **{k: v for k, v in t.items() if k != 'maps'}, feats=t['maps'], out=one)
        a.update(over)
        return lib.mr_roi_extract_forward(*_lib.pack('mr_roi_extract_forward', a), None)

    def bwd(L=1, table={}, **over):
        t = tables(L, **table)
        a = dict(base, **{k: v for k, v in t.items() if k != 'maps'}, grad_feats=t['maps'], grad_out=one)
        a.update(over)
        return lib.mr_roi_extract_backward(*_lib.pack('mr_roi_extract_backward', a), None)

    for call in (fwd, bwd):
        assert call(n_levels=0) == BAD and call(n_images=0) == BAD and call(channels=0) == BAD
        assert call(out_h=0) == BAD and call(out_w=0) == BAD and call(n_rois=-1) == BAD and call(sampling_ratio=-1) == BAD
        assert call(finest_scale=0.0) == BAD and call(finest_scale=float('nan')) == BAD
        assert call(table=dict(h=0)) == BAD and call(table=dict(w=0)) == BAD and call(table=dict(s=0)) == BAD
        assert call(table=dict(null_map=True)) == BAD and call(level_h=None) == BAD and call(level_stride=None) == BAD
        assert call(rois=None) == BAD
        assert call(L=9) == UNSUPPORTED and call(out_h=33) == UNSUPPORTED and call(out_w=33) == UNSUPPORTED
        assert call(table=dict(h=1 << 15, w=1 << 15)) == UNSUPPORTED                    # a slab beyond 32-bit offsets
        assert call(n_rois=1 << 25) == UNSUPPORTED                                      # an output beyond 32-bit offsets
    assert fwd(out=None) == BAD and fwd(feats=None) == BAD and bwd(grad_out=None) == BAD and bwd(grad_feats=None) == BAD
    assert fwd(n_rois=0, rois=None, out=None) == 0                                      # no RoIs: nothing is launched
