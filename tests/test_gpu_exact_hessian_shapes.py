"""exact_hessian_kernel on the MI355X at the cases of tests/exact_hessian_cases.py: every lane-trip count of its point loop, every mask
kind, per-object against shared cameras and ranges, both memory layouts, the three storage types and every pivot path of its
Gauss-Jordan inverse (tests/test_exact_hessian_cases_cpu.py pins what each case exercises), through the C ABI into prefilled buffers
with a guard row on each side.

Bounds: those of tests/test_exact_hessian.py.  hess within 3e-7 of the oracle on the same rounded values, relative to max |H|; cov
within 1e-5 max(1, cond(H) 1e-7) of orc.pose_cov_general(H_oracle), relative to max |cov|.  The measured worst ratios are printed."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_hessian_cases as hc  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
TORCH = {'f32': torch.float32, 'f16': torch.float16, 'f64': torch.float64}
I4 = np.eye(4, dtype=np.float32)


def dv(a):
    """to the device with the strides the array has (the planar views keep theirs)"""
    t = torch.from_numpy(np.asarray(a))
    d = torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=DEV)
    d.copy_(t)
    return d


def tensors(c, storage='f32', shared=False):
    """the device tensors of a case: correspondences in the storage type, camera / ranges / pose float32, mask u8"""
    st = TORCH[storage]
    T = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dt)
    n = 1 if shared else None
    return dict(x2d=T(c['x2d'], st), istd=T(c['istd'], st), x3d=T(c['x3d'], st), K=T(c['K'][:n], torch.float32), ur=T(c['u_range'][:n], torch.float32),
                vr=T(c['v_range'][:n], torch.float32), pose=T(np.concatenate([c['yaw'], c['t']], 1), torch.float32),
                mask=None if c['mask'] is None else T(c['mask'], torch.uint8), valid_in=T(c['valid_in'], torch.uint8), z_min=c['z_min'])


def run_abi(t, fill=0xFF, with_hess=True, sel=None):
    """mr_pnp_exact_hessian_batched into buffers prefilled with the byte `fill`, a guard row on each side of hess, cov and valid
    -> hess (B + 2, 16) f32 bits as int32 | None, cov (B + 2, 16) likewise, valid (B + 2,) u8, code.  sel: run object sel alone."""
    from monorun_amd import _lib
    from monorun_amd.ops.least_squares.pnp_uncert import _inputs
    pick = (lambda a, shared_ok=False: a) if sel is None else (lambda a, shared_ok=False: a if (a is None or (shared_ok and a.shape[0] == 1)) else a[sel:sel + 1])
    x2d, istd, x3d = pick(t['x2d']), pick(t['istd']), pick(t['x3d'])
    _, B, P, common, hold = _inputs(x2d, istd, x3d, pick(t['K'], True), pick(t['ur'], True), pick(t['vr'], True))
    pose, mask = pick(t['pose']).contiguous(), pick(t['mask'])
    mask = mask.contiguous() if mask is not None else None
    buf = lambda cols: torch.full(((B + 2) * cols * 4,), fill, dtype=torch.uint8, device=DEV).view(torch.int32).view(B + 2, cols)
    hess, cov = (buf(16) if with_hess else None), buf(16)
    valid = torch.full((B + 2,), fill, dtype=torch.uint8, device=DEV)
    valid[1:-1] = pick(t['valid_in'])
    code = _lib.load().mr_pnp_exact_hessian_batched(*_lib.pack('mr_pnp_exact_hessian_batched', common, pose=pose.data_ptr(), inlier_mask=_lib.ptr(mask),
                                                               B=B, P=P, z_min=float(t['z_min']), valid=valid[1:].data_ptr(),
                                                               hess=None if hess is None else hess[1:].data_ptr(), cov=cov[1:].data_ptr()),
                                                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    del hold
    return (None if hess is None else hess.cpu().numpy()), cov.cpu().numpy(), valid.cpu().numpy(), code


def f32(bits):
    return np.ascontiguousarray(bits).view(np.float32)


def guards_untouched(hess, cov, valid, fill):
    word = np.int32(-1 if fill == 0xFF else 0)
    return (hess is None or (np.all(hess[[0, -1]] == word))) and np.all(cov[[0, -1]] == word) and valid[0] == fill and valid[-1] == fill


def check(name, t, want, alone=True):
    """one case through the ABI: bounds against the oracle, guard rows, a second run bitwise equal, hess = NULL changing nothing, every
    object alone bitwise equal to itself in the batch.  Returns (hess, cov, valid) without the guard rows."""
    Ho, oko, covo = want
    B = len(Ho)
    hess, cov, valid, code = run_abi(t, 0xFF)
    assert code == 0 and guards_untouched(hess, cov, valid, 0xFF)
    h, c, v = f32(hess[1:-1]).reshape(B, 4, 4).astype(np.float64), f32(cov[1:-1]).reshape(B, 4, 4).astype(np.float64), valid[1:-1]
    worst_h = worst_c = 0.0
    for b in range(B):
        assert v[b] == int(oko[b]), (name, b, v[b], oko[b])
        if not Ho[b].any():
            assert not h[b].any(), (name, b)                                           # nothing summed: exactly zero
        else:
            rh = np.abs(h[b] - Ho[b]).max() / np.abs(Ho[b]).max()
            worst_h = max(worst_h, rh / hc.HESS_BOUND)
            assert rh <= hc.HESS_BOUND, (name, b, rh)
        if oko[b]:
            rc = np.abs(c[b] - covo[b]).max() / np.abs(covo[b]).max()
            worst_c = max(worst_c, rc / hc.cov_bound(Ho[b]))
            assert rc <= hc.cov_bound(Ho[b]), (name, b, rc, hc.cov_bound(Ho[b]))
        else:
            assert np.array_equal(f32(cov[1 + b]).reshape(4, 4), I4), (name, b)
    print(f'{name}: B {B}, {int(v.sum())} valid; worst hess error / bound {worst_h:.3f}, worst cov error / bound {worst_c:.3f}')
    hess2, cov2, valid2, code2 = run_abi(t, 0x00)
    assert code2 == 0 and guards_untouched(hess2, cov2, valid2, 0x00)
    assert np.array_equal(hess[1:-1], hess2[1:-1]) and np.array_equal(cov[1:-1], cov2[1:-1]) and np.array_equal(valid[1:-1], valid2[1:-1])
    _, cov3, valid3, code3 = run_abi(t, 0xFF, with_hess=False)
    assert code3 == 0 and np.array_equal(cov3, cov) and np.array_equal(valid3, valid)
    if alone and B > 1:
        for b in range(B):
            h1, c1, v1, code1 = run_abi(t, 0xFF, sel=b)
            assert code1 == 0 and guards_untouched(h1, c1, v1, 0xFF)
            assert np.array_equal(h1[1], hess[1 + b]) and np.array_equal(c1[1], cov[1 + b]) and v1[1] == valid[1 + b], (name, b)
    return hess[1:-1], cov[1:-1], valid[1:-1]


def no_hip_error():
    from monorun_amd import _lib
    return _lib.load().mr_pnp_last_hip_error() == 0


@pytest.mark.parametrize('name', hc.SHAPE_NAMES)
def test_shapes(name):
    check(name, tensors(hc.case(name)), hc.expected(name))
    assert no_hip_error()


@pytest.mark.parametrize('name', hc.MASK_NAMES)
def test_masks(name):
    _, cov, valid = check(name, tensors(hc.case(name)), hc.expected(name))
    if name in ('mask_zero', 'mask_zclip'):
        assert valid.tolist() == [0, 0, 0] and all(np.array_equal(f32(r).reshape(4, 4), I4) for r in cov)
    if name == 'mask_enters_invalid':
        assert valid.tolist() == [1, 0, 1]
    assert no_hip_error()


def test_a_missing_mask_is_a_mask_of_ones():
    a = run_abi(tensors(hc.case('mask_none')))
    b = run_abi(tensors(hc.case('mask_ones')))
    assert a[3] == 0 and b[3] == 0 and all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))


def test_pivot_paths():
    check('pivots', tensors(hc.case('pivots')), hc.expected('pivots'))
    assert no_hip_error()


def test_per_object_cameras_and_ranges():
    """per-object ones that differ against the oracle; per-object ones that hold one value against shared ones (stride 0): bitwise"""
    check('strides', tensors(hc.case('strides')), hc.expected('strides'))
    c = hc.case('shape_B10_P257')
    shared, per = run_abi(tensors(c, shared=True)), run_abi(tensors(c))
    assert shared[3] == 0 and per[3] == 0 and all(np.array_equal(x, y) for x, y in zip(shared[:3], per[:3]))
    check('shape_B10_P257 shared', tensors(c, shared=True), hc.expected('shape_B10_P257'), alone=False)
    assert no_hip_error()


def test_planar_and_interleaved_layouts_agree(orc):
    out = []
    for planar in (True, False):
        x2d, istd, x3d, K, ur, vr, pose, mask = hc.layout_batch(planar)
        t = dict(x2d=dv(x2d), istd=dv(istd), x3d=dv(x3d), K=dv(K), ur=dv(ur), vr=dv(vr), pose=dv(pose), mask=dv(mask.astype(np.uint8)),
                 valid_in=torch.ones(3, dtype=torch.uint8, device=DEV), z_min=hc.Z_MIN)
        assert t['x2d'].is_contiguous() != planar
        out.append(run_abi(t))
        assert out[-1][3] == 0 and guards_untouched(*out[-1][:3], 0xFF)
    assert all(np.array_equal(x, y) for x, y in zip(out[0][:3], out[1][:3]))
    x2d, istd, x3d, K, ur, vr, pose, mask = hc.layout_batch(False)
    c = dict(x2d=x2d, istd=istd, x3d=x3d, K=np.repeat(K, 3, 0), u_range=np.repeat(ur, 3, 0), v_range=np.repeat(vr, 3, 0), yaw=pose[:, :1], t=pose[:, 1:],
             mask=mask, valid_in=np.ones(3, np.uint8), z_min=hc.Z_MIN)
    t = dict(x2d=dv(x2d), istd=dv(istd), x3d=dv(x3d), K=dv(K), ur=dv(ur), vr=dv(vr), pose=dv(pose), mask=dv(mask.astype(np.uint8)),
             valid_in=torch.ones(3, dtype=torch.uint8, device=DEV), z_min=hc.Z_MIN)
    h, _, _ = check('layouts', t, hc.reference(c))
    assert np.array_equal(h, out[0][0][1:-1])
    assert no_hip_error()


@pytest.mark.parametrize('name', ['shape_B3_P257', 'shape_B3_P600'])
def test_storage_types(name):
    c = hc.case(name)
    check(name + ' f64', tensors(c, 'f64'), hc.expected(name, 'f64'), alone=False)
    h16 = check(name + ' f16', tensors(c, 'f16'), hc.expected(name, 'f16'), alone=False)
    # fp16 storage: the kernel widens exactly, so it equals the fp32 run on the fp16-rounded values
    r16 = lambda a: np.asarray(a).astype(np.float16).astype(np.float64)
    h32 = run_abi(tensors(dict(c, x2d=r16(c['x2d']), istd=r16(c['istd']), x3d=r16(c['x3d']))))
    assert all(np.array_equal(x, y[1:-1]) for x, y in zip(h16, h32[:3]))
    assert no_hip_error()
