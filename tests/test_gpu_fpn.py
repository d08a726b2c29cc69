"""The feature pyramid's fused launches on the GPU against the numpy definition (tests/fpn_ref.py) and the eager torch
chain, on the smallest pyramids at which the kernels can go wrong: odd sizes at every level, wider than one tile, one and two levels, six
levels, and one pyramid outside the header's rule, which must take the restatement and still agree."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import fpn_ref as ref
from tests.test_fpn_cpu import gradient_bound, literal_chain

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
CASES = [(name, shape) for name in ref.PYRAMIDS for shape in ref.SHAPES]


def dev():
    return torch.device('cuda:0')


def to_dev(a):
    return torch.from_numpy(np.array(a)).to(dev())


def run(fn, c, lower_scale, need=None, use=None):
    """merged maps, low and the gradients of the laterals of `fn` on a case of fpn_ref, on the GPU.  need[l]: whether lateral l asks for a
    gradient; use[k]: whether output k (the merged maps, then low) receives one."""
    L = len(c['lats'])
    need = need or [True] * L
    lats = [to_dev(t).requires_grad_(n) for t, n in zip(c['lats'], need)]
    m, low = fn(lats, lower_scale)
    outs = list(m) + ([low] if lower_scale else [])
    gs = [to_dev(g) for g in c['g_m']] + ([to_dev(c['g_low'])] if lower_scale else [])
    use = [u and o.requires_grad for u, o in zip(use or [True] * len(outs), outs)]
    grads = torch.autograd.grad([o for o, u in zip(outs, use) if u], [t for t, n in zip(lats, need) if n], [g for g, u in zip(gs, use) if u],
                                allow_unused=True)
    grads = iter(grads)
    grads = [next(grads) if n else None for n in need]
    torch.cuda.synchronize()
    return ([t.detach().cpu().numpy() for t in m], low.detach().cpu().numpy() if lower_scale else None,
            [g.cpu().numpy() if g is not None else None for g in grads])


@pytest.mark.parametrize('lower_scale', [0, 2])
@pytest.mark.parametrize('name,shape', CASES)
def test_random_data_is_bitwise_the_definition(name, shape, lower_scale):
    from monorun_amd import fpn
    c = ref.case(name, shape, lower_scale)
    lats = [to_dev(t) for t in c['lats']]
    assert fpn.hip_ok(lats, lower_scale) == ref.in_rule(c['sizes'])
    m, low, grads = run(fpn.fpn_topdown, c, lower_scale)
    eager = fpn.fpn_topdown_torch(lats, lower_scale)[0]
    for l, (a, b, e) in enumerate(zip(m, c['m'], eager)):
        assert np.array_equal(a, b), f'merged level {l} against the definition'
        assert np.array_equal(a, e.cpu().numpy()), f'merged level {l} against the eager chain on the GPU'
    if lower_scale:
        assert low.shape == c['low'].shape and np.array_equal(low, c['low']), 'low'
    if ref.in_rule(c['sizes']):
        for l, (a, b) in enumerate(zip(grads, c['grads'])):
            assert a.shape == b.shape and np.array_equal(a, b), f'gradient of lateral {l}'
    else:                                       # the restatement: autograd's order, within the bound of two fp32 orders
        for l, (a, b, bound) in enumerate(zip(grads, c['grads'], gradient_bound(c, shape, lower_scale))):
            assert np.all(np.abs(a.astype(np.float64) - b) <= bound), f'gradient of lateral {l}'


@pytest.mark.parametrize('name,shape', CASES)
def test_integer_data_is_bitwise_the_eager_chain_and_its_autograd(name, shape):
    from monorun_amd import fpn
    c = ref.case(name, shape, 2, True)
    got, want = run(fpn.fpn_topdown, c, 2), run(literal_chain, c, 2)
    for a, b, d in zip(got[0] + [got[1]] + got[2], want[0] + [want[1]] + want[2], c['m'] + [c['low']] + c['grads']):
        assert np.array_equal(a, b) and np.array_equal(a, d)


@pytest.mark.parametrize('name', ['ceil_odd', 'wide', 'tall_six'])
def test_gradient_handling(name):
    """an unused output gives what zeros give; a lateral that needs no gradient gets None; two runs are bitwise identical"""
    from monorun_amd import fpn
    shape = (2, 5)
    c = ref.case(name, shape, 2)
    L = len(c['sizes'])
    full = run(fpn.fpn_topdown, c, 2)
    again = run(fpn.fpn_topdown, c, 2)
    for a, b in zip(full[2], again[2]):
        assert np.array_equal(a, b)
    for skip in ([1], [0, L], [0, 1, 2], list(range(1, L + 1))):           # outputs left out: merged maps by level, L = low
        use = [k not in skip for k in range(L + 1)]
        g_m = [g if use[l] else None for l, g in enumerate(c['g_m'])]
        want = ref.backward(c['sizes'], shape, 2, g_m, c['g_low'] if use[L] else None)
        got = run(fpn.fpn_topdown, c, 2, use=use)[2]
        for l, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(a, b), (skip, l)
    need = [l % 2 == 0 for l in range(L)]
    got = run(fpn.fpn_topdown, c, 2, need=need)[2]
    for l, (a, b) in enumerate(zip(got, c['grads'])):
        assert (a is None) if not need[l] else np.array_equal(a, b), l


SENTINEL = 12345.0


class Guarded:
    """a tensor of the given shape inside a larger buffer filled with a sentinel (the tensor itself with `fill`), `offset` floats in"""

    def __init__(self, shape, fill, offset):
        self.n = int(np.prod(shape))
        self.offset = offset
        self.buf = torch.full((self.n + offset + 37,), SENTINEL, device=dev(), dtype=torch.float32)
        self.view = self.buf[offset:offset + self.n]
        self.view.fill_(fill)
        self.shape = shape

    def ptr(self):
        return self.view.data_ptr()

    def check(self):
        b = self.buf.cpu().numpy()
        assert np.all(b[:self.offset] == SENTINEL) and np.all(b[self.offset + self.n:] == SENTINEL), 'a store outside the tensor'
        return b[self.offset:self.offset + self.n].reshape(self.shape)


@pytest.mark.parametrize('offset', [4, 2, 1])          # low 16-byte aligned, 8-byte aligned, neither: the three store widths
@pytest.mark.parametrize('shape', ref.SHAPES)
@pytest.mark.parametrize('name', ['ceil_odd', 'wide', 'one_level', 'tall_six'])
def test_c_abi_writes_every_element_and_nothing_else(name, shape, offset):
    """through the C ABI, every output inside a sentinel-filled buffer and starting as NaN: afterwards no NaN is left (every element is
    stored: the launches need no memset), the values are the definition's, and the sentinels are intact"""
    from monorun_amd import _lib
    c = ref.case(name, shape, 2)
    sizes, L = c['sizes'], len(c['sizes'])
    nan = float('nan')
    i32 = ctypes.c_int * L
    common = dict(level_h=i32(*[h for h, _ in sizes]), level_w=i32(*[w for _, w in sizes]), n_levels=L, n_images=shape[0], channels=shape[1],
                  lower_scale=2)
    table = lambda ptrs: (ctypes.c_void_p * L)(*ptrs)
    stream = torch.cuda.current_stream(dev()).cuda_stream
    lats = [to_dev(t) for t in c['lats']]
    merged = [Guarded(shape + s, nan, 4 + offset) for s in sizes[:-1]]
    low = Guarded(shape + (2 * sizes[0][0], 2 * sizes[0][1]), nan, offset)
    _lib.call('mr_fpn_topdown_forward', common, lat=table([t.data_ptr() for t in lats]), merged=table([g.ptr() for g in merged] + [None]),
              low=low.ptr(), stream=stream)
    g_m, g_low = [to_dev(g) for g in c['g_m']], to_dev(c['g_low'])
    grads = [Guarded(shape + s, nan, 8 + offset) for s in sizes]
    _lib.call('mr_fpn_topdown_backward', common, grad_merged=table([t.data_ptr() for t in g_m]), grad_low=g_low.data_ptr(),
              grad_lat=table([g.ptr() for g in grads]), stream=stream)
    torch.cuda.synchronize()
    for l, g in enumerate(merged):
        assert np.array_equal(g.check(), c['m'][l]), f'merged level {l}'
    assert np.array_equal(low.check(), c['low'])
    for l, g in enumerate(grads):
        assert np.array_equal(g.check(), c['grads'][l]), f'gradient of lateral {l}'


@pytest.mark.parametrize('training', [False, True])
def test_fpnplus_on_the_gpu_against_the_restatement(training, monkeypatch):
    """FPNplus with the fused launches against the same module with the restatement forced.  The maps entering the 3 x 3 convolutions
    (what `_top_down` returns: the merged levels and `low`) are bit for bit the same, and so are the six outputs: both asserted.  The
    gradients of the parameters and the inputs pass through autograd's order on one side and the gather's on the other and through
    MIOpen's convolutions: each of those 22 tensors may differ from the fp64 evaluation (on the CPU) by at most four times what the fp32
    restatement itself differs by (DESIGN.md §22 records the measured figures)."""
    import copy
    from monorun_amd import fpn
    chans, sizes = [3, 5, 6, 4], ref.PYRAMIDS['wide']
    torch.manual_seed(5)
    neck = fpn.FPNplus(chans, 8, 5, num_lower_outs=1)
    neck.init_weights()
    g = torch.Generator().manual_seed(9)
    xs = [torch.randn(2, ch, h, w, generator=g) for ch, (h, w) in zip(chans, sizes)]
    gos = None
    pathway = []                # what _top_down returned, per evaluation
    real_top_down = fpn.FPN._top_down

    def top_down(self, laterals, lower_scale):
        m, low = real_top_down(self, laterals, lower_scale)
        pathway.append([t.detach().clone() for t in m] + [low.detach().clone()])
        return m, low
    monkeypatch.setattr(fpn.FPN, '_top_down', top_down)

    def evaluate(module, device, dtype):
        nonlocal gos
        module = module.to(device=device, dtype=dtype).train(training)
        ins = [x.to(device=device, dtype=dtype).requires_grad_(training) for x in xs]
        with torch.set_grad_enabled(training):
            outs = module(ins)
        if gos is None:
            gos = [torch.randn(o.shape, generator=g) for o in outs]
        res = [o.detach().double().cpu() for o in outs]
        if training:
            params = list(module.parameters())
            grads = torch.autograd.grad(outs, params + ins, [t.to(device=device, dtype=dtype) for t in gos])
            res += [t.double().cpu() for t in grads]
        return res

    truth = evaluate(copy.deepcopy(neck), 'cpu', torch.float64)
    calls = []
    real = fpn._FPNTopDownFunction.apply
    monkeypatch.setattr(fpn._FPNTopDownFunction, 'apply', lambda *a: calls.append(1) or real(*a))
    fused = evaluate(copy.deepcopy(neck), dev(), torch.float32)
    assert calls == [1], 'the fused launch ran'
    monkeypatch.setattr(fpn, 'hip_ok', lambda *a, **k: False)
    restated = evaluate(copy.deepcopy(neck), dev(), torch.float32)
    assert calls == [1], 'the restatement was forced'
    assert len(truth) == len(fused) == len(restated) == (6 + (18 + 4 if training else 0))
    assert len(pathway) == 3 and len(pathway[1]) == len(pathway[2]) == 5
    for k, (f, r) in enumerate(zip(pathway[1], pathway[2])):
        assert f.shape == r.shape and torch.equal(f, r), f'map {k} entering the 3 x 3 convolutions (merged levels, then low)'
    for k in range(6):
        assert torch.equal(fused[k], restated[k]), f'output {k}'
    worst = 0.0
    for k in range(6, len(truth)):
        t, f, r = truth[k], fused[k], restated[k]
        ef, er = (f - t).abs().max().item(), (r - t).abs().max().item()
        print(f'gradient {k - 6}: fused {ef:.3e} restatement {er:.3e} against fp64; fused == restatement bitwise: {torch.equal(f, r)}')
        worst = max(worst, ef / er if er else 0.0)
        assert ef <= 4 * er, k
    print(f'largest ratio of the fused error to the restatement\'s: {worst:.2f}')


def test_create_graph_runs_the_restatement_and_is_the_transpose():
    """a backward under create_graph=True leaves the kernel for the restatement at zero laterals: its gradients agree with the kernel's
    within the bound of two fp32 orders, they carry a graph, and differentiating <grad_lat, R> by the arriving gradients gives the op
    applied to R (the op is linear: the adjoint identity), compared with the fused forward of R under the forward's rules"""
    from monorun_amd import fpn
    name, shape = 'ceil_odd', (2, 5)
    c = ref.case(name, shape, 2)
    lats = [to_dev(t).requires_grad_(True) for t in c['lats']]
    gs = [to_dev(g).requires_grad_(True) for g in c['g_m']] + [to_dev(c['g_low']).requires_grad_(True)]
    assert fpn.hip_ok(lats, 2)
    m, low = fpn.fpn_topdown(lats, 2)
    grads = torch.autograd.grad(list(m) + [low], lats, gs, create_graph=True)
    assert all(t.requires_grad for t in grads)
    for l, (a, b, bound) in enumerate(zip(grads, c['grads'], gradient_bound(c, shape, 2))):
        assert np.all(np.abs(a.detach().cpu().numpy().astype(np.float64) - b) <= bound), f'gradient of lateral {l}'
    probe = [to_dev(t) for t in ref.case(name, shape, 2, True)['lats']]          # integers: the op applied to them is exact in any order
    back = torch.autograd.grad(sum((a * p).sum() for a, p in zip(grads, probe)), gs)
    pm, plow = fpn.fpn_topdown(probe, 2)
    for l, (a, b) in enumerate(zip(back, list(pm) + [plow])):
        assert torch.equal(a, b), f'the transpose of the transpose, output {l}'
