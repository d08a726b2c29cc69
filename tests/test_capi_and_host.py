"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol that
include/monorun_pnp.h declares; the Python surface mirrors monorun/ops (names, constructor, registry,
empty batch, loud failure without a GPU).  No compute calls — there is no GPU here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_functions():
    src = open(os.path.join(ROOT, 'include', 'monorun_pnp.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(?:int|void|const char \*)\s*\*?\s*([a-z_0-9]+)\s*\(', src)))


def test_header_declares_the_expected_entry_points():
    names = _declared_functions()
    for n in ('mr_pnp_uncert_batched', 'pnp_uncert', 'mr_noc_decode_batched', 'mr_pnp_version',
              'mr_pnp_error_string', 'mr_pnp_last_hip_error', 'mr_pnp_device_count'):
        assert n in names, names


def test_library_loads_and_exports_every_declared_symbol():
    from monorun_amd import _lib
    assert os.path.exists(_lib.SO), 'run __graft_entry__.build() first'
    lib = ctypes.CDLL(_lib.SO)
    for n in _declared_functions():
        assert hasattr(lib, n), f'{n} declared in include/monorun_pnp.h but not exported'
    h = _lib.load()
    assert h.mr_pnp_version() == 100
    assert h.mr_pnp_error_string(0) == b'ok' and b'argument' in h.mr_pnp_error_string(-1)
    for n in _lib.exported_symbols():
        assert hasattr(h, n)


def test_reference_signature_of_legacy_symbol():
    """ext.h:1-13 — 5 double* in, int*, 3 double*, int, double*."""
    from monorun_amd import _lib
    at = _lib.load().pnp_uncert.argtypes
    dp = ctypes.POINTER(ctypes.c_double)
    assert list(at) == [dp, dp, dp, dp, dp, ctypes.POINTER(ctypes.c_int), dp, dp, dp, ctypes.c_int, dp]


def test_ops_surface_mirrors_reference():
    import monorun_amd.ops as ops
    assert set(ops.__all__) >= {'u2d_pnp_cpu', 'build_pnp', 'PnPUncert', 'pnp_uncert'}
    from monorun_amd.ops import build_pnp, PnPUncert, PNP
    m = build_pnp(dict(type='PnPUncert', z_min=0.5, epnp_istd_thres=0.6, inlier_opt_only=True, forward_exact_hessian=False))
    assert isinstance(m, PnPUncert) and isinstance(m, torch.nn.Module)
    assert (m.z_min, m.epnp_istd_thres, m.inlier_opt_only, m.coord_istd_normalize, m.forward_exact_hessian, m.use_6dof, m.eps) == \
           (0.5, 0.6, True, False, False, False, 1e-6)
    assert len(list(m.state_dict())) == 0                       # no parameters or buffers, like the reference
    assert m.initialiser == 'epnp'                              # the reference's config dict builds the REFERENCE's flow
    d = PnPUncert()
    assert (d.z_min, d.epnp_istd_thres, d.inlier_opt_only, d.initialiser) == (0.5, 0.6, True, 'epnp')
    assert build_pnp(dict(type='PnPUncert', initialiser='k0')).initialiser == 'k0'       # the explicit fast mode
    import inspect
    from monorun_amd.ops import pnp_uncert, u2d_pnp_cpu
    from monorun_amd.ops.least_squares.pnp_uncert import DEFAULT_INITIALISER
    assert DEFAULT_INITIALISER == 'epnp'
    assert inspect.signature(pnp_uncert).parameters['initialiser'].default is None and inspect.signature(u2d_pnp_cpu).parameters['initialiser'].default is None
    with pytest.raises(TypeError):                               # the reference's latent default-dict bug is preserved:
        build_pnp(dict(type='PnPUncert', backward_exact_hessian=True))   # pnp_uncert.py:93-99 does not accept it
    with pytest.raises(KeyError):
        build_pnp(dict(type='NoSuchPnP'))


def test_empty_batch_returns_typed_empties_without_a_gpu():
    from monorun_amd.ops import u2d_pnp_cpu
    e = u2d_pnp_cpu(np.zeros((0, 784, 2), np.float32), np.zeros((0, 784, 2), np.float32), np.zeros((0, 784, 3), np.float32),
                    np.eye(3, dtype=np.float32)[None], np.zeros((1, 2), np.float32), np.zeros((1, 2), np.float32))
    assert [a.shape for a in e] == [(0,), (0, 1), (0, 3), (0, 4, 4), (0, 1), (0, 784)]
    assert e[0].dtype == bool and e[5].dtype == bool and e[1].dtype == np.float32


@pytest.mark.skipif(torch.cuda.is_available(), reason='only meaningful without a GPU')
def test_no_cpu_fallback_fails_loudly():
    from monorun_amd.ops import pnp_uncert, u2d_pnp_cpu
    x = torch.zeros(2, 16, 2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pnp_uncert(x, x + 1, torch.zeros(2, 16, 3), torch.eye(3)[None], torch.zeros(1, 2), torch.zeros(1, 2))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        u2d_pnp_cpu(np.zeros((2, 16, 2), np.float32), np.ones((2, 16, 2), np.float32), np.zeros((2, 16, 3), np.float32),
                    np.eye(3, dtype=np.float32)[None], np.zeros((1, 2), np.float32), np.zeros((1, 2), np.float32))


def test_product_never_imports_the_oracle():
    """③: only tests/, smoke() and bench.py's cpu_baseline leg may touch oracle/."""
    pkg = os.path.join(ROOT, 'monorun_amd')
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith(('.py', '.hip', '.h', '.cpp')):
                txt = open(os.path.join(dp, f)).read()
                assert 'oracle' not in txt.replace('the CPU oracle', '').replace('against the CPU oracle', ''), os.path.join(dp, f)
    # tools/ holds product-side utilities (profiling, timing, the KITTI harness): none may import the checker either; the
    # sweeps that DO compare against it live under tests/sweeps/
    import re
    for f in os.listdir(os.path.join(ROOT, 'tools')):
        if f.endswith(('.py', '.sh')):
            txt = open(os.path.join(ROOT, 'tools', f)).read()
            assert not re.search(r'^\s*(from|import)\s+oracle', txt, re.M), f


def test_synthetic_generator_shapes_and_determinism():
    from monorun_amd import synthetic as syn
    a, b = syn.make_batch(B=16, seed=1234), syn.make_batch(B=16, seed=1234)
    for k in a:
        assert np.array_equal(a[k], b[k])
    assert a['coords_2d'].shape == (16, 2, 28, 28) and a['coords_3d'].shape == (16, 3, 28, 28) and a['logstd'].shape == (16, 2, 28, 28)
    x2d, istd, x3d, K, ur, vr, thr = syn.pnp_boundary(a, planar=True)
    assert x2d.strides == (1568 * 4, 4, 784 * 4) and x3d.strides == (2352 * 4, 4, 784 * 4)
    assert np.array_equal(ur, [[-200, 1442]]) and np.array_equal(vr, [[-200, 575]])
    np.testing.assert_allclose(thr, 0.2 * 27 / 28 * (a['rois'][:, 3] - a['rois'][:, 1]), rtol=1e-4)


def test_capi_argument_validation_without_a_gpu():
    """Bad arguments are rejected before any HIP call, so this runs on CPU: error codes of include/monorun_pnp.h."""
    from monorun_amd import _lib
    lib = _lib.load()
    st = (ctypes.c_int64 * 3)(1568, 1, 784)
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)

    def call(B=4, P=784, x2d=p, cam_batch=1, range_batch=1, cov=p, dtype=0, flags=0):
        return lib.mr_pnp_uncert_batched(x2d, st, p, st, p, st, dtype, p, cam_batch, p, p, range_batch, None, None, B, P,
                                         0.5, 0.6, 1, flags, p, p, cov, p, p, None, None)
    assert call(B=0) == 0                                     # empty batch: success, nothing launched
    assert call(B=-1) == -1 and call(P=3) == -1 and call(P=10 ** 6) == -1
    assert call(x2d=None) == -1 and call(cov=None) == -1
    assert call(cov=None, flags=_lib.MR_COV_NONE, B=0) == 0
    assert call(cam_batch=3) == -1 and call(range_batch=2) == -1
    assert call(P=8192) == -2                                 # tile does not fit the 160 KB LDS
    assert call(dtype=7) == -2
    assert lib.mr_pnp_error_string(-2).startswith(b'unsupported') and lib.mr_pnp_error_string(-99) == b'unknown error'
    # the reference's initialiser: workspace sizing is host arithmetic, bad arguments are refused before any HIP call
    assert lib.mr_epnp_workspace_bytes(0, 784) == 0 and lib.mr_epnp_workspace_bytes(8, 3) == 0
    w1, w2 = lib.mr_epnp_workspace_bytes(1024, 784), lib.mr_epnp_workspace_bytes(2048, 784)
    assert 10e6 < w1 < 20e6 and w1 % 256 == 0 and 1.9 * w1 < w2 < 2.1 * w1

    def ecall(B=4, P=784, x2d=p, cam_batch=1, max_iters=30, out=p, work=None, nbytes=0):
        return lib.mr_epnp_ransac_batched(x2d, st, p, st, p, st, 0, p, cam_batch, p, B, P, 0.6, 0, max_iters, out, p, p, None, None, work, nbytes, None)
    assert ecall(B=0) == 0
    assert ecall(B=-1) == -1 and ecall(P=3) == -1 and ecall(max_iters=0) == -1 and ecall(max_iters=31) == -1
    assert ecall(x2d=None) == -1 and ecall(out=None) == -1 and ecall(cam_batch=2) == -1
    # NMS / decode entry points validate too
    assert lib.mr_nms_bev_batched(None, None, None, 0, 0, 0.1, None, None, None) == 0
    assert lib.mr_nms_bev_batched(p, p, p, 1, 4096, 0.1, p, p, None) == -2
    assert lib.mr_nms_bev_batched(p, p, None, 1, 8, 0.1, p, p, None) == -1

    # The other batched entry points: which code each bad argument gets, and which check comes first.  Every call below is refused
    # before a kernel is launched (a workspace is never both large enough and given: nothing here may reach the GPU).
    F32, F64, COV_NONE = _lib.MR_F32, _lib.MR_F64, _lib.MR_COV_NONE
    tables = []

    def calls(*v):                                            # a per-call pointer table of the grouped entry points
        t = (ctypes.c_void_p * len(v))(*v)
        tables.append(t)
        return ctypes.addressof(t)
    full = calls(*[p] * 8)
    big = 0x7fffffff // 30 + 1                                # objects of a launch set are numbered in int arithmetic: too many

    def icall(B=4, P=784, x2d=p, strides=st, init=p, cam_batch=1, range_batch=1, cov=p, dtype=F32, flags=0):
        return lib.mr_pnp_uncert_from_init_batched(x2d, strides, p, st, p, st, dtype, p, cam_batch, p, p, range_batch, init, p, p, B, P,
                                                   0.5, 1, flags, p, p, cov, p, p, None, None)
    assert icall(B=0) == 0 and icall(B=0, init=None, x2d=None) == 0
    assert icall(B=-1) == -1 and icall(B=-1, init=None) == -1 and icall(B=0, P=3) == -1 and icall(P=3) == -1 and icall(P=10 ** 6) == -1
    assert icall(init=None) == -1 and icall(x2d=None) == -1 and icall(strides=None) == -1 and icall(cov=None) == -1
    assert icall(cam_batch=3) == -1 and icall(range_batch=2) == -1 and icall(cam_batch=3, dtype=7) == -1
    assert icall(dtype=7) == -2 and icall(cov=None, flags=COV_NONE, dtype=7) == -2 and icall(cam_batch=4, range_batch=4, dtype=7) == -2
    assert icall(P=8192) == -2

    def gcall(n=2, B=4, P=784, x2d=full, cov=full, mask=None, diag=None, cam_batch=1, range_batch=1, dtype=F32, flags=0):
        return lib.mr_pnp_uncert_from_init_grouped(n, x2d, st, full, st, full, st, dtype, full, cam_batch, full, full, range_batch,
                                                   full, full, full, B, P, 0.5, 1, flags, full, full, cov, full, mask, diag, None)
    assert gcall(B=0) == 0 and gcall(B=0, P=3, x2d=None) == 0                  # an empty set succeeds before P is looked at
    assert gcall(n=0) == -1 and gcall(n=9) == -1 and gcall(n=0, B=0) == -1 and gcall(B=-1) == -1
    assert gcall(x2d=None) == -1 and gcall(x2d=calls(p, None)) == -1 and gcall(cov=None) == -1 and gcall(cov=calls(p, None)) == -1
    assert gcall(B=big, x2d=calls(None, None)) == -2 and gcall(B=big, P=3) == -2    # the set's size before the calls' pointers and P
    assert gcall(mask=calls(p, None)) == -1 and gcall(mask=calls(None, p)) == -1 and gcall(diag=calls(p, None)) == -1
    assert gcall(P=3) == -1 and gcall(P=10 ** 6) == -1 and gcall(cam_batch=3) == -1 and gcall(range_batch=2) == -1
    assert gcall(dtype=7) == -2 and gcall(dtype=7, mask=full, diag=calls(None, None)) == -2 and gcall(P=8192) == -2
    assert gcall(dtype=7, cov=calls(p, None), flags=COV_NONE) == -2

    wb = lib.mr_epnp_workspace_bytes(8, 784)

    def fcall(n=2, B=4, P=784, x2d=full, work=p, nbytes=wb - 1, epdiag=None, logscale=None, calib=None, dtype=F32, flags=0):
        return lib.mr_pnp_uncert_from_epnp_grouped(n, x2d, st, full, st, full, st, dtype, full, 1, full, full, 1, full, full, full, epdiag, B, P,
                                                   0.5, 1, flags, full, full, full, full, None, None, logscale, 0.1, calib, work, nbytes, None)
    assert fcall(B=0) == 0 and fcall(B=0, work=None, x2d=None) == 0
    assert fcall(n=0) == -1 and fcall(n=9) == -1 and fcall(B=-1) == -1 and fcall(P=3) == -1 and fcall(B=0, P=3) == -1
    assert fcall(B=big, work=None) == -2 and fcall(work=None) == -1 and fcall() == -1                    # no / short workspace
    assert fcall(dtype=7) == -1 and fcall(dtype=7, nbytes=wb) == -2                                      # the workspace before the dtype
    assert fcall(nbytes=wb, calib=full) == -1 and fcall(nbytes=wb, calib=full, logscale=p, flags=COV_NONE) == -1
    assert fcall(nbytes=wb, calib=calls(p, None), logscale=p) == -1 and fcall(nbytes=wb, calib=calls(None, p), logscale=p) == -1
    assert fcall(nbytes=wb, x2d=None) == -1 and fcall(nbytes=wb, x2d=calls(p, None)) == -1
    assert fcall(P=10 ** 6, nbytes=lib.mr_epnp_workspace_bytes(8, 10 ** 6)) == -1
    assert fcall(dtype=7, nbytes=wb, epdiag=calls(p, None)) == -2 and fcall(dtype=7, nbytes=wb, calib=full, logscale=p) == -2
    assert fcall(P=8192, nbytes=lib.mr_epnp_workspace_bytes(8, 8192)) == -2

    def rcall(n=2, B=4, P=784, x2d=full, cam_batch=1, thr=full, diag=None, max_iters=30, work=p, dtype=F32, flags=0):
        return lib.mr_epnp_ransac_grouped(n, x2d, st, full, st, full, st, dtype, full, cam_batch, thr, B, P, 0.6, flags, max_iters,
                                          full, full, full, diag, work, 0, None)
    assert rcall(B=0) == 0 and rcall(B=0, x2d=None) == 0
    assert rcall(n=0) == -1 and rcall(n=9) == -1 and rcall(n=0, B=0) == -1 and rcall(B=-1) == -1 and rcall(B=0, P=3) == -1
    assert rcall(P=3) == -1 and rcall(P=10 ** 6) == -1 and rcall(max_iters=0) == -1 and rcall(max_iters=31) == -1
    assert rcall(B=big, x2d=None) == -2 and rcall(x2d=None) == -1 and rcall(x2d=calls(p, None)) == -1 and rcall(cam_batch=3) == -1
    assert rcall(thr=calls(p, None)) == -1 and rcall(thr=calls(None, p)) == -1 and rcall(diag=calls(p, None)) == -1
    assert rcall(work=None, flags=_lib.MR_EPNP_DEFER_REFIT) == -1
    assert rcall(dtype=7) == -2 and rcall(dtype=7, thr=None, diag=calls(None, None)) == -2 and rcall(dtype=7, cam_batch=4) == -2
    assert rcall() == -1                                                                                  # short workspace

    def p6(B=4, P=784, x2d=p, mask=p, cov6=p, cam_batch=1, range_batch=1, dtype=F32):
        return lib.mr_pnp6_refine_batched(x2d, st, p, st, p, st, dtype, p, cam_batch, p, p, range_batch, mask, p, p, B, P, 0.5, 0, p, p, cov6, None, None)
    assert p6(B=0) == 0 and p6(B=0, x2d=None) == 0
    assert p6(B=-1) == -1 and p6(P=3) == -1 and p6(B=0, P=3) == -1 and p6(P=10 ** 6) == -1
    assert p6(x2d=None) == -1 and p6(mask=None) == -1 and p6(cov6=None) == -1 and p6(cam_batch=3) == -1 and p6(range_batch=2) == -1
    assert p6(dtype=7) == -2 and p6(P=8192) == -2 and p6(P=8192, dtype=F64) == -2

    def hs(B=4, P=784, x2d=p, pose=p, mask=p, hess=p, cov=p, cam_batch=1, range_batch=1, dtype=F32):
        return lib.mr_pnp_exact_hessian_batched(x2d, st, p, st, p, st, dtype, p, cam_batch, p, p, range_batch, pose, mask, B, P, 0.5, p, hess, cov, None)
    assert hs(B=0) == 0 and hs(B=0, pose=None) == 0
    assert hs(B=-1) == -1 and hs(P=0) == -1 and hs(B=0, P=0) == -1
    assert hs(x2d=None) == -1 and hs(pose=None) == -1 and hs(cov=None) == -1 and hs(cam_batch=3) == -1 and hs(range_batch=2) == -1
    assert hs(dtype=7) == -2 and hs(dtype=7, P=1, mask=None, hess=None) == -2

    def bw(B=4, P=784, x2d=p, pose=p, valid=p, cov=None, gcov=None, cam_batch=1, range_batch=1, dtype=F32):
        return lib.mr_pnp_uncert_backward_batched(x2d, st, p, st, p, st, dtype, p, cam_batch, p, p, range_batch, pose, p, valid, 1, p, cov, gcov,
                                                  B, P, 0.5, p, p, p, p, None)
    assert bw(B=0) == 0 and bw(B=0, cov=p) == 0 and bw(B=0, x2d=None, pose=None, valid=None) == 0          # an empty batch touches no pointer
    assert bw(B=-1) == -1 and bw(P=0) == -1 and bw(P=-1) == -1 and bw(B=0, P=0) == -1
    assert bw(cam_batch=3) == -1 and bw(cam_batch=0) == -1 and bw(cam_batch=5) == -1 and bw(range_batch=0) == -1
    assert bw(x2d=None) == -1 and bw(pose=None) == -1 and bw(valid=None) == -1 and bw(pose=None, cov=p, gcov=p) == -1
    assert bw(cov=p) == -1 and bw(gcov=p) == -1 and bw(cov=p, gcov=p, cam_batch=3) == -1 and bw(range_batch=2) == -1
    assert bw(dtype=7) == -2 and bw(dtype=7, cov=p, gcov=p) == -2

    def hd(B=4, h=28, w=28, pred=p, pred_dtype=F32, C=3, cam=p, cam_batch=1, range_batch=1, cov=p, flags=0, map2d=None, map_h=0,
           logscale=None, calib=None):
        return lib.mr_pnp_from_head_batched(pred, pred_dtype, p, p, p, None, p, B, C, 0, h, w, p, p, p, p, 1.0, 1.0, 1.0, 1.0, 0.1,
                                            cam, cam_batch, p, p, range_batch, 0.5, 0.6, 1, flags, p, p, cov, p, p, None,
                                            None, None, map2d, map_h, map_h, logscale, 0.1, calib, None)
    assert hd(B=0) == 0 and hd(B=0, pred=None, cam=None) == 0
    assert hd(B=-1) == -1 and hd(h=1, w=3) == -1 and hd(B=0, h=1, w=3) == -1 and hd(h=128, w=128) == -1
    assert hd(map2d=p, map_h=0) == -1 and hd(B=0, map2d=p, map_h=0) == -1
    assert hd(cam=None) == -1 and hd(cov=None) == -1 and hd(cam_batch=3) == -1 and hd(range_batch=2) == -1
    assert hd(C=0) == -1 and hd(pred=None) == -1 and hd(pred_dtype=7) == -2 and hd(pred_dtype=7, cam_batch=3) == -1
    assert hd(calib=p) == -1 and hd(calib=p, logscale=p, flags=COV_NONE) == -1 and hd(calib=p, pred_dtype=7) == -2
    assert hd(h=64, w=128) == -2


def test_img_shape_and_flip_forms_the_pipeline_passes():
    """mmdet hands img_meta['img_shape'] = (H, W, 3) and a per-image bool flip (Python or numpy bool, or a 0-dim tensor):
    the host glue takes the first two entries per image like the reference (uncert_prop_pnp_optimizer.py:75-80) and turns
    every scalar flip form into B flags (one flag per object otherwise; a wrong count is refused, not read out of bounds)."""
    from monorun_amd import pose_head as ph
    cpu = torch.device('cpu')
    for shp in ((375, 1242), (375, 1242, 3), [[375, 1242, 3]], np.array([[375., 1242.]]), torch.tensor([[375., 1242., 3.]])):
        ur, vr = ph._clip_ranges(shp, 200, cpu)
        assert ur.tolist() == [[-200.0, 1442.0]] and vr.tolist() == [[-200.0, 575.0]]
    ur, vr = ph._clip_ranges(((375, 1242, 3), (370, 1224, 3)), 200, cpu)
    assert ur.tolist() == [[-200.0, 1442.0], [-200.0, 1424.0]] and vr.tolist() == [[-200.0, 575.0], [-200.0, 570.0]]
    with pytest.raises(AssertionError):
        ph._clip_ranges((375, 1242, 3, 1), 200, cpu)
    for f in (True, np.bool_(True), torch.tensor(True), np.array(True), np.array([True])):
        fl = ph._flip_flags(f, 5, cpu)
        assert fl.dtype == torch.uint8 and fl.tolist() == [1] * 5
    assert ph._flip_flags([True, False, True], 3, cpu).tolist() == [1, 0, 1]
    assert ph._flip_flags(torch.tensor([False]), 1, cpu).tolist() == [0]
    with pytest.raises(AssertionError):
        ph._flip_flags([True, False], 3, cpu)


def test_pose_stage_dump_hook_on_a_stand_in_roi_head(tmp_path):
    """monorun_amd.integration.PoseStageDump wraps the four call sites of MonoRUnRoIHead.simple_test
    (monorun_roi_head.py:442-547) and writes what tools/kitti_val.py reads.  mmdet is absent, so the hook is exercised on a
    stand-in object with the same attribute structure and call order; the wrapped functions must behave as before."""
    import types
    from monorun_amd.integration import PoseStageDump
    n, C = 5, 3
    conv = torch.nn.Conv2d(4, 2 * C * 5, 1)

    class Head:
        def __init__(self):
            self.noc_head = types.SimpleNamespace(conv_final=conv)
            self.bbox_head = types.SimpleNamespace(get_bboxes=lambda *a, **k: (torch.cat([torch.rand(n, 4) * 100, torch.rand(n, 1)], 1), torch.arange(n) % C))
            self.score_head = types.SimpleNamespace(pre_sigmoid=True)
            self.test_cfg = types.SimpleNamespace(mult_2d_score=True)

        def _reg_forward(self, x, rois, labels):
            return dict(dim_pred=torch.randn(len(rois), 3), dim_var=torch.rand(len(rois), 3))

        def _score_forward(self, *a):
            return dict(scores=torch.randn(n, 1))

        def simple_test(self, x, proposal_list, img_metas, proposals=None, coord_2d=None, cam_intrinsic=None, rescale=False):
            det_bboxes, det_labels = self.bbox_head.get_bboxes()
            rois = torch.cat([torch.zeros(n, 1), det_bboxes[:, :4]], 1)
            self._reg_forward(x, rois, det_labels)
            self.noc_head.conv_final(torch.randn(n, 4, 28, 28))
            self._score_forward()
            return 'results'
    h = Head()
    orig = h.simple_test
    meta = dict(filename='/data/kitti/training/image_2/000123.png', img_shape=(375, 1242, 3), flip=False)
    with PoseStageDump(h, str(tmp_path)) as d:
        assert h.simple_test(None, None, [meta], cam_intrinsic=[[torch.eye(3)]]) == 'results'
    assert h.simple_test.__func__ is orig.__func__ and d.written == [str(tmp_path / '000123.npz')]       # restored on exit
    z = np.load(d.written[0])
    assert z['all_pred'].shape == (n, 30, 28, 28) and z['labels'].dtype == np.int64 and z['rois'].shape == (n, 4)
    assert z['dim'].shape == (n, 3) and z['dim_var'].shape == (n, 3) and z['bboxes'].shape == (n, 4) and z['scores'].shape == (n,)
    assert z['scores_ref'].shape == (n,) and np.all((z['scores_ref'] >= 0) & (z['scores_ref'] <= 1)) and z['img_shape'].tolist() == [375.0, 1242.0]
    assert np.array_equal(z['rois'], z['bboxes']) and z['cam_intrinsic'].shape == (3, 3) and not bool(z['flip'])


def test_integration_md_cffi_block_is_the_generated_prototype_text_and_every_symbol_is_exported():
    """INTEGRATION.md §3 shows the text a maintainer feeds to cffi's `ffi.cdef`.  cffi is absent here, so instead of executing it
    the test checks (a) the block is exactly what tools/gen_cffi_cdef.py derives from include/monorun_pnp.h, (b) it contains only
    what cffi's declaration parser accepts (prototypes over plain C / stdint types and plain-integer #defines: no comments, no
    `extern "C"`, no parenthesised or shifted macro values), (c) every prototype names a symbol the built library exports, with
    the argument count the header declares."""
    import ctypes
    import re
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import gen_cffi_cdef as gen
    md = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    block = md.split('<!-- cffi-cdef:begin -->')[1].split('<!-- cffi-cdef:end -->')[0]
    text = block.split('```c\n')[1].split('```')[0]
    assert text == gen.cdef_text(), 'INTEGRATION.md cffi block is stale: regenerate with tools/gen_cffi_cdef.py'
    allowed = re.compile(r'^(#define MR_\w+ (0x[0-9A-Fa-f]+|\d+)|[A-Za-z_][\w \*]*\([\w \*,]*\);)$')
    protos = []
    for line in text.strip().split('\n'):
        assert allowed.match(line), line
        assert '/*' not in line and '//' not in line and 'extern' not in line and '<<' not in line and '(-' not in line
        if not line.startswith('#define'):
            m = re.match(r'^(.*?)(\w+)\((.*)\);$', line)
            name, args = m.group(2), m.group(3)
            for tok in re.findall(r'[A-Za-z_]\w*', m.group(1) + ' ' + re.sub(r'\b\w+(?=\s*(,|$))', '', args)):
                assert tok in ('const', 'void', 'int', 'float', 'double', 'char', 'uint8_t', 'int8_t', 'int32_t', 'int64_t', 'size_t'), (name, tok)
            protos.append((name, 0 if args.strip() == 'void' else args.count(',') + 1))
    from monorun_amd import _lib
    lib = ctypes.CDLL(_lib.SO)
    hdr = {n: len(a) for n, _, a in gen.header_prototypes()}
    assert set(n for n, _ in protos) == set(hdr) == set(_lib.exported_symbols('pnp'))
    for name, nargs in protos:
        assert hasattr(lib, name) and hdr[name] == nargs, name


# what each header of `_lib.HEADERS` declares, pinned a second time here: a change to the public surface shows up in the header, in the
# loader's table and in this one (`pnp`, the cffi surface: its size, and how many of its symbols are `mr_*`; the names are in INTEGRATION.md)
_PINNED = {
    'pnp': 34,
    'heads': ('mr_score_head_forward',),
    'train': ('mr_noc_decode_train', 'mr_noc_decode_train_backward'),
    'targets': ('mr_noc_dense_target', 'mr_smooth_l1_mod_workspace_bytes', 'mr_smooth_l1_mod_loss', 'mr_smooth_l1_mod_loss_backward'),
    'global': ('mr_global_head_mc_workspace_bytes', 'mr_global_head_mc_forward'),
    'carafe': ('mr_carafe_pack_forward', 'mr_carafe_backward_workspace_bytes', 'mr_carafe_pack_backward'),
}
_SCALAR = {'int': ctypes.c_int, 'float': ctypes.c_float, 'double': ctypes.c_double, 'size_t': ctypes.c_size_t, 'int64_t': ctypes.c_int64}


def _declared_prototypes(path):
    """[(return type, name, [arguments])] of a header, by a regex of this file's own (not `_lib.header_prototypes`)."""
    src = re.sub(r'/\*.*?\*/', ' ', open(path).read(), flags=re.S)
    found = re.findall(r'^((?:const\s+)?\w+[\s\*]+)(\w+)\s*\(([^)]*)\)\s*;', src, flags=re.M)
    return [(' '.join(ret.split()), name, [] if args.strip() in ('', 'void') else [' '.join(a.split()) for a in args.split(',')])
            for ret, name, args in found]


@pytest.mark.parametrize('key', ['pnp', 'heads', 'train', 'targets', 'global', 'carafe'])
def test_loader_binds_every_header(key, monkeypatch):
    """For each header of `_lib.HEADERS`: the pinned tuple is what the header declares, in order, and shares no name with any other
    header; the library exports every symbol; the loaded function has the declared restype and argtypes, and `arg_names` the declared
    names, the expected ones derived here from the header text and not by the loader's own mapping; the header alone makes the
    library stale."""
    from monorun_amd import _lib
    assert list(_lib.HEADERS) == ['pnp', 'heads', 'train', 'targets', 'global', 'carafe'] and set(_PINNED) == set(_lib.HEADERS)
    lib, raw = _lib.load(), ctypes.CDLL(_lib.SO)
    pinned = _lib.exported_symbols(key)
    assert pinned == _lib.HEADERS[key][1] and _lib.header_path(key) == os.path.join(ROOT, 'include', _lib.HEADERS[key][0])
    if key == 'pnp':
        assert len(pinned) == _PINNED[key] and sum(n.startswith('mr_') for n in pinned) == 31
        assert [n for n, _, _ in _lib.header_prototypes()] == list(pinned)                           # the default header is this one
    else:
        assert pinned == _PINNED[key]
    assert len(set(pinned)) == len(pinned)
    assert [n for n, _, _ in _lib.header_prototypes(_lib.header_path(key))] == list(pinned)
    declared = _declared_prototypes(_lib.header_path(key))
    assert [name for _, name, _ in declared] == list(pinned)
    for other in _lib.HEADERS:
        if other != key:
            assert not set(pinned) & set(_lib.exported_symbols(other)), other
            assert not set(pinned) & {n for n, _, _ in _lib.header_prototypes(_lib.header_path(other))}, other
            assert not set(pinned) & {n for _, n, _ in _declared_prototypes(_lib.header_path(other))}, other
    assert _lib.exported_symbols() == tuple(n for k in _lib.HEADERS for n in _lib.exported_symbols(k))
    for ret, name, args in declared:
        assert hasattr(raw, name), f'{name} declared in {_lib.HEADERS[key][0]} but not exported'
        f = getattr(lib, name)
        names = [re.search(r'\w+$', a).group() for a in args]
        types = [a.replace('const ', '')[:-len(n)].strip() for a, n in zip(args, names)]
        assert len(set(names)) == len(names), name
        if name.startswith('mr_'):
            want_ret = ctypes.c_char_p if ret == 'const char *' else _SCALAR[ret]
            want = [ctypes.c_void_p if '*' in t else _SCALAR[t] for t in types]
            assert list(_lib.arg_names(name)) == (names[:-1] if names[-1:] == ['stream'] else names), name
        else:                                                                                        # ext.h's symbols: typed pointers
            want_ret = None if ret == 'void' else _SCALAR[ret]
            want = [ctypes.POINTER(_SCALAR[t.replace('*', '').strip()]) if '*' in t else _SCALAR[t] for t in types]
        assert f.restype is want_ret, name
        assert list(f.argtypes or []) == want, name
    assert not _lib._stale()
    so_time, real = os.path.getmtime(_lib.SO), os.path.getmtime
    monkeypatch.setattr(os.path, 'getmtime', lambda f: so_time + 10 if f == _lib.header_path(key) else real(f))
    assert _lib._stale()


def test_pack_orders_named_arguments_as_the_abi_does():
    from monorun_amd import _lib
    order = ('x2d', 'x2d_strides', 'istd', 'istd_strides', 'x3d', 'x3d_strides', 'in_dtype', 'cam_mats', 'cam_batch', 'ransac_thr', 'B', 'P',
             'istd_thres', 'flags', 'max_iters', 'init_pose', 'init_mask', 'init_valid', 'diag', 'debug_hypotheses', 'workspace', 'workspace_bytes')
    assert _lib.arg_names('mr_epnp_ransac_batched') == order                     # include/monorun_pnp.h, without the trailing stream
    named = {n: k for k, n in enumerate(order)}
    assert _lib.pack('mr_epnp_ransac_batched', **dict(reversed(list(named.items())))) == list(range(len(order)))
    with pytest.raises(TypeError, match='max_iters'):
        _lib.pack('mr_epnp_ransac_batched', **{n: v for n, v in named.items() if n != 'max_iters'})
    with pytest.raises(TypeError, match='u_range'):
        _lib.pack('mr_epnp_ransac_batched', u_range=0, **named)
    assert _lib.table_args('mr_epnp_ransac_grouped') == ('x2d', 'istd', 'x3d', 'cam_mats', 'ransac_thr', 'init_pose', 'init_mask', 'init_valid', 'diag')
    assert _lib.table_args('mr_epnp_ransac_batched') == ()


def test_launch_set_members_must_agree_by_argument_name():
    """What PnPEpnpGroupLaunch refuses, on the members' named arguments alone (the launch classes need a HIP device): one mismatch per
    argument the set passes once, and per pointer that must be given or left out by all members."""
    import importlib
    pu = importlib.import_module('monorun_amd.ops.least_squares.pnp_uncert')      # (the package re-exports the function under this name)
    st = lambda *v: (ctypes.c_int64 * 3)(*v)
    init = dict(x2d=1, x2d_strides=st(1568, 1, 784), istd=2, istd_strides=st(1568, 1, 784), x3d=3, x3d_strides=st(2352, 1, 784), in_dtype=0, cam_mats=4,
                cam_batch=1, ransac_thr=5, B=64, P=784, istd_thres=0.6, flags=0, max_iters=30, init_pose=6, init_mask=7, init_valid=8, diag=None,
                debug_hypotheses=None, workspace=9, workspace_bytes=10)
    lm = dict(range_batch=1, z_min=0.5, inlier_opt_only=1, flags=0, diag=None, valid=11, pose=12)
    other = dict(init, x2d=21, x2d_strides=st(1568, 1, 784), ransac_thr=25, init_pose=26, workspace=29)     # own tensors, equal strides: agrees
    pu._require_agreement([init, other, init], pu._SET_INIT, 'X')
    pu._require_agreement([lm, dict(lm, valid=31, pose=32)], pu._SET_LM, 'X')
    msg = 'the members of a group must share shape, strides, dtype, camera batching, thresholds and flags'
    for change in (dict(x2d_strides=st(1568, 784, 1)), dict(istd_strides=st(2, 1, 784)), dict(x3d_strides=st(2352, 784, 1)), dict(in_dtype=1),
                   dict(cam_batch=64), dict(B=32), dict(P=144), dict(istd_thres=0.7), dict(flags=4), dict(max_iters=20), dict(ransac_thr=None), dict(diag=40)):
        with pytest.raises(ValueError) as e:
            pu._require_agreement([init, dict(init, **change)], pu._SET_INIT, 'shape, strides, dtype, camera batching, thresholds and flags')
        assert str(e.value) == msg, change
    msg = 'the members of a group must share range batching, z_min, inlier_opt_only and flags'
    for change in (dict(range_batch=64), dict(z_min=0.4), dict(inlier_opt_only=0), dict(flags=0x20), dict(diag=41)):
        with pytest.raises(ValueError) as e:
            pu._require_agreement([lm, lm, dict(lm, **change)], pu._SET_LM, 'range batching, z_min, inlier_opt_only and flags')
        assert str(e.value) == msg, change
