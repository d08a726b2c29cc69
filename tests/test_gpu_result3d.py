"""result3d_nms_kernel on the MI355X against the cases of tests/result3d_cases.py: equality with the expectation, index for index and
bit for bit, with no allowance (tests/test_result3d_cases_cpu.py shows that no pair of an oracle-judged class is within KNIFE of a
threshold); bit-equality with the path it replaces (consumers.get_bbox_3d_result + consumers.multiclass_3d_result_nms), also on random
inputs that are not knife-free, since both run one device routine on bit-identical boxes; the padding, written into prefilled, guarded
buffers through the C ABI; reproducibility; and the fallback past the caps."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import result3d_cases as rc  # noqa: E402
from test_consumers import _rand_boxes  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
KEYS = ('dimensions', 'yaw', 't_vec', 'scores', 'labels', 'det_bboxes')
CASE_THRS = [(name, thr) for name in rc.NAMES for thr in rc.THRS]
MR_ERR_BAD_ARGUMENT, MR_ERR_UNSUPPORTED = -1, -2
GUARD = 4                                   # spare elements around every output of run_abi: 16 bytes of floats, so out3d stays aligned


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    """float32 arrays compared bit for bit (NaN payloads included)"""
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def no_hip_error():
    from monorun_amd import _lib
    return _lib.load().mr_pnp_last_hip_error() == 0


def inputs(c):
    return [dev(c[k]) for k in KEYS]


def old_path(ins, C, thr):
    """the path the kernel replaces, on the same device tensors -> per class (rows, local indices, 2-D boxes, rows in the inputs), numpy"""
    from monorun_amd.consumers import get_bbox_3d_result, multiclass_3d_result_nms
    dims, yaw, t, s, lab, det = ins
    res = get_bbox_3d_result(dims, yaw, t, s, lab, C)
    out, inds = multiclass_3d_result_nms(res, thr, to_np=True)
    lab_h, det_h = lab.cpu().numpy(), det.cpu().numpy()
    rows = [np.nonzero(lab_h == c)[0][inds[c]] for c in range(C)]
    return out, inds, [det_h[lab_h == c][inds[c]] for c in range(C)], rows


def check_padded(padded, C, N, want3d, want_local, want2d, want_rows, sizes):
    out3d, out2d, keep_local, keep_row, num_keep, num_in = [t.cpu().numpy() for t in padded]
    assert out3d.shape == (C, N, 8) and out2d.shape == (C, N, 5) and keep_local.shape == keep_row.shape == (C, N)
    assert out3d.dtype == out2d.dtype == np.float32 and keep_local.dtype == keep_row.dtype == np.int64 and num_keep.dtype == num_in.dtype == np.int32
    assert num_in.tolist() == list(sizes)
    wrong = []
    for c in range(C):
        k = int(num_keep[c])
        if k != len(want_local[c]) or not np.array_equal(keep_local[c, :k], want_local[c]) or not np.array_equal(keep_row[c, :k], want_rows[c]):
            wrong.append((c, sizes[c], k, len(want_local[c])))
            continue
        assert np.array_equal(bits(out3d[c, :k]), bits(want3d[c])) and np.array_equal(bits(out2d[c, :k]), bits(want2d[c])), c
        assert np.isnan(out3d[c, k:]).all() and np.isnan(out2d[c, k:]).all() and np.all(keep_local[c, k:] == -1) and np.all(keep_row[c, k:] == -1), c
    assert not wrong, wrong[:8]


@pytest.mark.parametrize('name,thr', CASE_THRS)
def test_case_equals_the_oracle_expectation_and_the_old_path(name, thr):
    from monorun_amd.consumers import result_3d_nms, result_3d_nms_padded
    c, want, cls = rc.case(name), rc.expected(name, thr), rc.class_rows(name)
    C, N, ins = c['C'], len(c['labels']), inputs(c)
    sizes = [len(r) for r, _ in cls]
    padded = result_3d_nms_padded(*ins, C, thr)
    assert all(t.device == DEV for t in padded)
    # the oracle: kept local indices per class; the rows are gathers of the inputs, bit for bit
    check_padded(padded, C, N, [r[k] for (r, _), k in zip(cls, want)], want, [c['det_bboxes'][rows][k] for (_, rows), k in zip(cls, want)],
                 [rows[k] for (_, rows), k in zip(cls, want)], sizes)
    print(f'{name} thr {thr}: {N} rows, {C} classes, kept {[len(k) for k in want]}')
    # the path it replaces, on the same tensors
    o3, oi, o2, orow = old_path(ins, C, thr)
    check_padded(padded, C, N, o3, oi, o2, orow, sizes)
    # the list form: one copy, the reference's three lists
    b3, inds, b2 = result_3d_nms(*ins, C, thr)
    assert len(b3) == len(inds) == len(b2) == C
    for k in range(C):
        assert isinstance(b3[k], np.ndarray) and inds[k].dtype == np.int64 and b3[k].shape == (len(want[k]), 8) and b2[k].shape == (len(want[k]), 5)
        assert np.array_equal(inds[k], oi[k]) and np.array_equal(bits(b3[k]), bits(o3[k])) and np.array_equal(bits(b2[k]), bits(o2[k]))
    t3, ti, t2, trow = result_3d_nms(*ins, C, thr, to_np=False, with_rows=True)
    for k in range(C):
        assert t3[k].device == DEV and ti[k].dtype == torch.int64
        assert np.array_equal(ti[k].cpu().numpy(), oi[k]) and np.array_equal(bits(t3[k]), bits(o3[k])) and np.array_equal(trow[k].cpu().numpy(), orow[k])
    assert no_hip_error()


def random_inputs(seed, N, C, spread):
    """rows that are NOT searched for knife-freeness: dense boxes, tied and zero scores, labels -1 .. C"""
    rng = np.random.default_rng(seed)
    b = _rand_boxes(rng, N, spread=spread)
    s = rng.uniform(0, 1, N).astype(np.float32)
    s[rng.permutation(N)[:N // 4]] = np.float32(0.5)
    s[rng.permutation(N)[:N // 8]] = 0
    r = rc.rows_of(b, s, rng)
    lab = rng.integers(-1, C + 1, N).astype(np.int64)
    det = rng.uniform(0, 600, (N, 5)).astype(np.float32)
    return [dev(a) for a in (r[:, 0:3], r[:, 6:7], r[:, 3:6], r[:, 7], lab, det)], lab


@pytest.mark.parametrize('seed,N,C,spread', [(1, 100, 3, 8.0), (2, 512, 16, 20.0), (3, 300, 1, 12.0), (4, 511, 2, 15.0), (5, 7, 16, 1.0)])
def test_random_rows_equal_the_old_path_bit_for_bit(seed, N, C, spread):
    from monorun_amd.consumers import result_3d_nms_padded
    ins, lab = random_inputs(seed, N, C, spread)
    for thr in rc.THRS:
        padded = result_3d_nms_padded(*ins, C, thr)
        o3, oi, o2, orow = old_path(ins, C, thr)
        check_padded(padded, C, N, o3, oi, o2, orow, [int((lab == c).sum()) for c in range(C)])
        assert sum(len(i) for i in oi) < sum(int((lab == c).sum()) for c in range(C)) or N < 8          # something was suppressed
    assert no_hip_error()


def run_abi(ins, N, C, thr, fill):
    """mr_result3d_nms with every output prefilled with the byte `fill` and GUARD spare elements on both sides of each
    -> {name: numpy array with the guards}, return code"""
    from monorun_amd import _lib
    lib = _lib.load()
    per = dict(out3d=(N * 8, torch.float32), out2d=(N * 5, torch.float32), keep_local=(N, torch.int64), keep_row=(N, torch.int64),
               num_keep=(1, torch.int32), num_in_class=(1, torch.int32))
    bufs, ptrs = {}, {}
    for name, (width, dt) in per.items():
        itemsize = torch.empty(0, dtype=dt).element_size()
        bufs[name] = torch.full(((C * width + 2 * GUARD) * itemsize,), fill, dtype=torch.uint8, device=DEV).view(dt)
        ptrs[name] = bufs[name][GUARD:].data_ptr()
    code = lib.mr_result3d_nms(*_lib.pack('mr_result3d_nms', dimensions=ins[0].data_ptr(), yaw=ins[1].data_ptr(), t_vec=ins[2].data_ptr(),
                                          scores=ins[3].data_ptr(), labels=ins[4].data_ptr(), det_bboxes=ins[5].data_ptr(), n=N, num_classes=C,
                                          thr=float(thr), **ptrs), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in bufs.items()}, code


@pytest.mark.parametrize('name', ['c16_small', 'special_scores', 'c1_all_512'])
def test_abi_stores_every_element_once_and_nothing_else(name):
    c = rc.case(name)
    C, N, ins, thr = c['C'], len(c['labels']), inputs(c), 0.25
    outs = []
    for fill in (0xFF, 0x00):
        got, code = run_abi(ins, N, C, thr, fill)
        assert code == 0
        inner = {}
        for k, a in got.items():
            guard = np.concatenate([a[:GUARD], a[-GUARD:]]).view(np.uint8)
            assert np.all(guard == fill), k                       # the spare elements on both sides
            inner[k] = a[GUARD:-GUARD]
        outs.append(inner)
    a, b = outs
    for k in a:                                                    # whatever the buffers held before: the same bytes, padding included
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    want = rc.expected(name, thr)
    assert a['num_keep'].tolist() == [len(k) for k in want] and a['num_in_class'].tolist() == list(c['sizes']) + [0] * (C - len(c['sizes']))
    o3, kl = a['out3d'].reshape(C, N, 8), a['keep_local'].reshape(C, N)
    for ci, k in enumerate(want):
        assert np.array_equal(kl[ci, :len(k)], k) and np.all(kl[ci, len(k):] == -1) and np.isnan(o3[ci, len(k):]).all() and not np.isnan(o3[ci, :len(k), :7]).any()
    assert no_hip_error()


def test_abi_argument_checks_and_empty_calls():
    c = rc.case('c16_small')
    ins = inputs(c)
    got, code = run_abi(ins, 0, 3, 0.25, 0xFF)                      # no rows: the counts are stored, nothing else
    assert code == 0 and got['num_keep'][GUARD:-GUARD].tolist() == [0, 0, 0] and got['num_in_class'][GUARD:-GUARD].tolist() == [0, 0, 0]
    assert np.all(np.concatenate([got['num_keep'][:GUARD], got['num_keep'][-GUARD:]]) == -1)
    assert np.all(got['out3d'].view(np.uint8) == 0xFF) and np.all(got['keep_row'].view(np.uint8) == 0xFF)
    got, code = run_abi(ins, 100, 0, 0.25, 0xFF)                  # no classes: nothing is launched
    assert code == 0 and all(np.all(a.view(np.uint8) == 0xFF) for a in got.values())
    got, code = run_abi(ins, 100, 17, 0.25, 0xFF)
    assert code == MR_ERR_UNSUPPORTED and all(np.all(a.view(np.uint8) == 0xFF) for a in got.values())
    from monorun_amd import _lib
    lib, p = _lib.load(), ins[0].data_ptr()
    assert lib.mr_result3d_nms(p, p, p, p, p, p, 513, 3, 0.25, p, p, p, p, p, p, None) == MR_ERR_UNSUPPORTED
    assert lib.mr_result3d_nms(p, p, p, p, p, p, -1, 3, 0.25, p, p, p, p, p, p, None) == MR_ERR_BAD_ARGUMENT
    assert lib.mr_result3d_nms(p, p, p, p, p, p, 8, 3, 0.25, None, p, p, p, p, p, None) == MR_ERR_BAD_ARGUMENT
    assert lib.mr_result3d_nms(p, p, p, p, None, p, 8, 3, 0.25, p, p, p, p, p, p, None) == MR_ERR_BAD_ARGUMENT
    assert lib.mr_result3d_nms(p, p, p, p, p, p, 8, 3, 0.25, p + 4, p, p, p, p, p, None) == MR_ERR_BAD_ARGUMENT        # out3d off 16 bytes
    torch.cuda.synchronize()
    assert no_hip_error()


def test_two_runs_are_bitwise_equal():
    from monorun_amd.consumers import _result_3d_packed
    ins, _ = random_inputs(11, 512, 3, 14.0)
    a = _result_3d_packed(*ins, 3, 0.01)[0].cpu().numpy()
    for _ in range(3):
        assert np.array_equal(a, _result_3d_packed(*ins, 3, 0.01)[0].cpu().numpy())
    assert no_hip_error()


def test_513_rows_and_17_classes_take_the_fallback_and_agree():
    from monorun_amd.consumers import result_3d_nms, result_3d_nms_padded
    for seed, N, C in ((21, 513, 3), (22, 120, 17)):
        ins, lab = random_inputs(seed, N, C, 25.0)
        sizes = [int((lab == c).sum()) for c in range(C)]
        o3, oi, o2, orow = old_path(ins, C, 0.25)
        check_padded(result_3d_nms_padded(*ins, C, 0.25), C, N, o3, oi, o2, orow, sizes)
        b3, inds, b2 = result_3d_nms(*ins, C, 0.25)
        for k in range(C):
            assert np.array_equal(inds[k], oi[k]) and np.array_equal(bits(b3[k]), bits(o3[k])) and np.array_equal(bits(b2[k]), bits(o2[k]))
        # the first 512 rows / 16 classes of the same tensors through the kernel: the fallback and the launch follow one rule
        n2, c2 = min(N, 512), min(C, 16)
        cut = [t[:n2] for t in ins]
        p3, pi, p2, prow = old_path(cut, c2, 0.25)
        check_padded(result_3d_nms_padded(*cut, c2, 0.25), c2, n2, p3, pi, p2, prow, [int((lab[:n2] == c).sum()) for c in range(c2)])
    assert no_hip_error()


def test_padded_form_does_not_synchronise():
    """torch's synchronisation debug mode raises on a synchronising call (tests/test_gpu_proposals.py::test_sync_debug_mode_is_implemented
    shows that this build implements it); the list form's one copy is a synchronisation and is not run under it"""
    from monorun_amd.consumers import result_3d_nms_padded
    c = rc.case('c16_small')
    ins = inputs(c)
    want = [t.clone() for t in result_3d_nms_padded(*ins, c['C'], 0.25)]        # warm: the library is loaded
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = result_3d_nms_padded(*ins, c['C'], 0.25)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    for a, b in zip(got, want):
        assert np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8))
    assert no_hip_error()
