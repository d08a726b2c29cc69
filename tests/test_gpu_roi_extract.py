"""The fused RoI extraction launches on the GPU: bit for bit against the per-level composition of the existing single-map
kernel, against the fp64 definition (tests/roi_extract_ref.py) within |got - ref64| <= C_BOUND 2^-23 (sum of the absolute terms of that
element), C_BOUND = 4 x the ratio measured for the fp32 torch restatement on the CPU; the backward's completeness and reproducibility;
the modules; the extractor in front of the NOC head's trunk."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import roi_extract_ref as ref

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def case_of(name):
    return ref.CASES[ref.IDS.index(name)]


@functools.lru_cache(maxsize=None)
def reference(name):
    """inputs and the fp64 results, computed once per case and shared"""
    case = case_of(name)
    feats, go = ref.make_inputs(case)
    out, outa, grads, gradsa = ref.extract(case, feats, go)
    for a in [go, out, outa, *feats, *grads, *gradsa]:
        a.setflags(write=False)
    return dict(feats=feats, go=go, out=out, outa=outa, grads=grads, gradsa=gradsa)


def extract_args(case):
    return ref.STRIDES[:case['L']], ref.FINEST, case['size'], case['sampling_ratio'], case['aligned']


def run(name, rows=slice(None), noncontiguous=False):
    """(out, [grad_feats]) of the fused path on the RoIs `rows` of a case, as CPU tensors"""
    from monorun_amd import roi_extractor as R
    case, r = case_of(name), reference(name)
    feats = [torch.from_numpy(f.copy()).to(DEV) for f in r['feats']]
    rois = torch.from_numpy(case['rois'][rows].copy()).to(DEV)
    go = torch.from_numpy(r['go'][rows].copy()).to(DEV)
    if noncontiguous:
        feats = [f.transpose(2, 3).contiguous().transpose(2, 3) for f in feats]
        rois = torch.stack([rois, rois], dim=-1)[..., 0]
        go = go.transpose(2, 3).contiguous().transpose(2, 3)
        assert not rois.is_contiguous() and not feats[0].is_contiguous()
    assert R.hip_ok(feats, rois, case['size']), 'the test must run the HIP path'
    for f in feats:
        f.requires_grad_(True)
    out = R.roi_extract(feats, rois, *extract_args(case))
    if rois.shape[0] == 0:
        return out.detach().cpu(), [torch.zeros(f.shape) for f in feats]
    assert out.grad_fn is not None and type(out.grad_fn).__name__.startswith('_RoIExtractFunction')
    out.backward(go)
    torch.cuda.synchronize()
    return out.detach().cpu(), [f.grad.cpu() for f in feats]


@functools.lru_cache(maxsize=None)
def hip_run(name):
    return run(name)


def composed(case, feats, rois, level_rois=None):
    """the parent's only way to the same tensor: mr_roi_align_avg per level on the level's RoIs, scattered by index; zeros for degenerate RoIs"""
    from monorun_amd.pose_head import roi_align_avg
    from monorun_amd.roi_extractor import map_roi_levels
    L, size, sr, aligned = case['L'], case['size'], case['sampling_ratio'], case['aligned']
    sizes = ref.level_sizes(L)
    levels = map_roi_levels((rois if level_rois is None else level_rois).cpu(), L, ref.FINEST)
    rn = rois.cpu().numpy()
    ok = torch.tensor([ref.roi_valid(r, sizes[l], ref.STRIDES[l], ref.N_IMAGES, size, sr, aligned) for r, l in zip(rn, levels.tolist())],
                      dtype=torch.bool)
    out = torch.zeros((rois.shape[0], feats[0].shape[1]) + tuple(size), device=rois.device)
    for l in range(L):
        idx = torch.nonzero((levels == l) & ok).flatten().to(rois.device)
        if idx.numel():
            out[idx] = roi_align_avg(feats[l], rois[idx], size, 1.0 / ref.STRIDES[l], sr, aligned)
    return out


@pytest.mark.parametrize('name', ref.IDS)
def test_forward_is_bitwise_the_per_level_composition(name):
    from monorun_amd.roi_extractor import map_roi_levels
    case, r = case_of(name), reference(name)
    out, _ = hip_run(name)
    feats = [torch.from_numpy(f.copy()).to(DEV) for f in r['feats']]
    want = composed(case, feats, torch.from_numpy(case['rois'].copy()).to(DEV))
    assert out.shape == want.shape and torch.equal(out, want.cpu())
    on_gpu = map_roi_levels(torch.from_numpy(case['rois'].copy()).to(DEV), case['L'], ref.FINEST)
    assert np.array_equal(on_gpu.cpu().numpy(), ref.roi_levels(case['rois'], case['L'])), 'the level rule in torch ops on the GPU'


@pytest.mark.parametrize('name', ref.IDS)
def test_forward_and_gradient_match_the_fp64_definition(name):
    r = reference(name)
    out, grads = hip_run(name)
    fwd = ref.ratio(out.numpy(), r['out'], r['outa'])
    per_level = [ref.ratio(g.numpy(), want, unit) for g, want, unit in zip(grads, r['grads'], r['gradsa'])]
    print(f'{name}: error / (2^-23 sum|terms|): forward {fwd:.2f} grad_feats {max(per_level):.2f}')
    assert fwd <= ref.C_BOUND
    assert max(per_level) <= ref.C_BOUND, per_level


def test_untouched_levels_and_images_get_exact_zeros():
    _, grads = hip_run('c5_L5_7x7')
    assert float(grads[4].abs().max()) == 0 and all(float(g.abs().max()) > 0 for g in grads[:4])          # level 4 has no RoI
    _, grads = hip_run('c5_L5_7x7_one_image')
    assert all(float(g[1].abs().max()) == 0 for g in grads)                                               # image 1 has none
    assert all(float(g[0].abs().max()) > 0 for g in grads)                                                # image 0 uses every level


@pytest.mark.parametrize('name', ['c5_L5_7x7', 'c33_L2_14x14_sr2_unaligned', 'c5_L5_7x7_no_rois'])
def test_backward_writes_every_element(name):
    """the C ABI on NaN-prefilled gradient buffers (no memset anywhere): no NaN is left, and the result is the Function's"""
    from monorun_amd import _lib
    case, r = case_of(name), reference(name)
    _, want = hip_run(name)
    strides, finest, (oh, ow), sr, aligned = extract_args(case)
    L, K = case['L'], case['rois'].shape[0]
    rois = torch.from_numpy(case['rois'].copy()).to(DEV)
    go = torch.from_numpy(r['go'].copy()).to(DEV)
    grads = [torch.full(f.shape, float('nan'), device=DEV) for f in r['feats']]
    i32 = ctypes.c_int * L
    _lib.call('mr_roi_extract_backward', grad_out=go.data_ptr() if K else None, rois=rois.data_ptr() if K else None, level_rois=None, n_rois=K,
              grad_feats=(ctypes.c_void_p * L)(*[g.data_ptr() for g in grads]), level_h=i32(*[g.shape[2] for g in grads]),
              level_w=i32(*[g.shape[3] for g in grads]), level_stride=i32(*strides), n_levels=L, n_images=ref.N_IMAGES, channels=case['C'],
              finest_scale=finest, out_h=oh, out_w=ow, sampling_ratio=sr, aligned=int(aligned),
              stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for g, w in zip(grads, want):
        assert not torch.isnan(g).any() and torch.equal(g.cpu(), w)


def test_runs_are_bitwise_reproducible_and_accept_strided_inputs():
    name = 'c33_L5_14x14'
    out, grads = hip_run(name)
    for again in (run(name), run(name, noncontiguous=True)):
        assert torch.equal(again[0], out) and all(torch.equal(a, b) for a, b in zip(again[1], grads))


def test_a_roi_alone_equals_the_roi_in_the_batch():
    name = 'c5_L5_7x7'
    out, _ = hip_run(name)
    for k in range(case_of(name)['rois'].shape[0]):
        alone, _ = run(name, slice(k, k + 1))
        assert torch.equal(alone[0], out[k]), k


def test_gradient_of_two_halves_sums_to_the_whole():
    name = 'c33_L5_14x14'
    r = reference(name)
    K = case_of(name)['rois'].shape[0]
    _, whole = hip_run(name)
    _, first = run(name, slice(0, K // 2))
    _, second = run(name, slice(K // 2, K))
    for a, b, w, want, unit in zip(first, second, whole, r['grads'], r['gradsa']):
        assert ref.ratio((a + b).numpy(), want, unit) <= ref.C_BOUND
        assert np.all(np.abs((a + b).double().numpy() - w.double().numpy()) <= 2 * ref.C_BOUND * ref.EPS32 * unit)


def test_level_rois_and_roi_scale_factor():
    """mmdet's roi_scale_factor: the level from the RoIs as given, the pooling from the rescaled ones, still one launch"""
    from monorun_amd import roi_extractor as R
    case, r = case_of('c5_L5_7x7'), reference('c5_L5_7x7')
    feats = [torch.from_numpy(f.copy()).to(DEV) for f in r['feats']]
    rois = torch.from_numpy(case['rois'].copy())
    rois = rois[torch.isfinite(rois).all(1)].to(DEV)
    mod = R.SingleRoIExtractor(dict(type='RoIAlign', output_size=7, sampling_ratio=0), case['C'], list(ref.STRIDES), finest_scale=ref.FINEST)
    got = mod(feats, rois, roi_scale_factor=1.25)
    scaled = R.roi_rescale(rois, 1.25)
    assert torch.equal(got, composed(case, feats, scaled, level_rois=rois))
    assert not torch.equal(got, composed(case, feats, scaled)), 'the case must tell the two rules apart'


def test_mod_with_starting_level_drops_the_finest_map():
    from monorun_amd import roi_extractor as R
    case, r = case_of('c5_L5_7x7'), reference('c5_L5_7x7')
    feats = [torch.from_numpy(f.copy()).to(DEV) for f in r['feats']]
    six = [torch.randn(ref.N_IMAGES, case['C'], *ref.IMAGE, device=DEV)] + feats
    rois = torch.from_numpy(case['rois'].copy()).to(DEV)
    layer = dict(type='RoIAlign', output_size=7, sampling_ratio=0)
    mod = R.SingleRoIExtractorMod(layer, case['C'], list(ref.STRIDES), finest_scale=ref.FINEST, starting_level=1)
    plain = R.SingleRoIExtractor(layer, case['C'], list(ref.STRIDES), finest_scale=ref.FINEST)
    a, b = mod(six, rois), plain(feats, rois)
    assert torch.equal(a, b) and torch.equal(a.cpu(), hip_run('c5_L5_7x7')[0])
    assert plain(feats, rois[:0]).shape == (0, case['C'], 7, 7)


def test_create_graph_backward_is_the_restatement():
    """under create_graph=True the Function's gradient carries a graph: differentiating <grad_feats, R> by grad_out gives the extraction
    of R (the op is linear in the maps)"""
    from monorun_amd import roi_extractor as R
    g = torch.Generator().manual_seed(3)
    sizes = ref.level_sizes(2)
    feats = [torch.randn(ref.N_IMAGES, 2, h, w, generator=g).to(DEV).requires_grad_(True) for h, w in sizes]
    probe = [torch.randn(ref.N_IMAGES, 2, h, w, generator=g).to(DEV) for h, w in sizes]
    rois = torch.tensor([[0, 3.0, 4.0, 17.0, 15.0], [1, 20.0, 10.0, 50.0, 40.0], [1, 2.0, 2.0, 9.0, 8.0]], device=DEV)
    args = (rois, ref.STRIDES[:2], ref.FINEST, (2, 3))
    out = R.roi_extract(feats, *args)
    assert type(out.grad_fn).__name__.startswith('_RoIExtractFunction')
    go = torch.randn(out.shape, generator=g).to(DEV).requires_grad_(True)
    grads = torch.autograd.grad(out, feats, go, create_graph=True)
    plain = torch.autograd.grad(out, feats, go.detach())
    assert all(torch.allclose(a, b, rtol=1e-5, atol=1e-6) for a, b in zip(grads, plain))
    sum((a * p).sum() for a, p in zip(grads, probe)).backward()
    assert torch.allclose(go.grad, R.roi_extract(probe, *args), rtol=1e-5, atol=1e-6)


def test_extractor_feeds_the_noc_trunk_and_gradients_reach_every_level():
    from monorun_amd import roi_extractor as R
    from tests import noc_decoder_cases as cases
    g20 = cases.load()
    head = cases.build(g20, 'a').eval().to(DEV)
    g = torch.Generator().manual_seed(11)
    feats = [torch.randn(ref.N_IMAGES, cases.CIN, h, w, generator=g).to(DEV).requires_grad_(True) for h, w in ref.level_sizes(5)]
    rows = [(0, 20.3, 10.7, 44.9, 30.1), (1, 69.0, 38.5, 81.0, 49.2), (1, 60.0, 30.0, 100.0, 70.0), (0, 0.0, -10.0, 64.0, 54.0),
            (1, -150.0, -150.0, 250.0, 200.0)]                                                          # levels 1, 0, 2, 3, 4
    rois = torch.tensor(rows, device=DEV)
    assert R.map_roi_levels(rois, 5, ref.FINEST).tolist() == [1, 0, 2, 3, 4]
    ext = R.SingleRoIExtractor(dict(type='RoIAlign', output_size=(cases.RH, cases.RW), sampling_ratio=0), cases.CIN, list(ref.STRIDES),
                               finest_scale=ref.FINEST)
    x = ext(feats, rois)
    assert x.shape == (5, cases.CIN, cases.RH, cases.RW) and type(x.grad_fn).__name__.startswith('_RoIExtractFunction')
    latent = torch.randn(5, cases.LAT, generator=g).to(DEV)
    all_pred = head.forward_all_pred(x, latent)
    all_pred.square().sum().backward()
    for l, f in enumerate(feats):
        assert f.grad is not None and torch.isfinite(f.grad).all() and float(f.grad.abs().max()) > 0, l
