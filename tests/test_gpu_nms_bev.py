"""nms_bev_kernel on the MI355X against the cases of tests/nms_bev_cases.py: equality with the expectation, index for index, with no
allowance (tests/test_nms_bev_cases_cpu.py shows that no pair of an oracle-judged group is within KNIFE of a threshold), through the
C ABI into prefilled, guarded buffers and through monorun_amd.consumers.

The NaN-score cases (special_scores) are safe to run because the sort's order is the one of csrc/nms_order.inc, which
tests/test_nms_order_cpu.py proves never to let a padding index among the first n places; the comparator before it did."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nms_bev_cases as nc  # noqa: E402
from test_consumers import _rand_boxes  # noqa: E402
from test_rotated_overlap_cases_cpu import NMS_THRS  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
MR_ERR_UNSUPPORTED = -2
CASE_THRS = [(name, thr) for name in nc.NAMES for thr in NMS_THRS]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_abi(groups, scores, thr, fill, max_group=None):
    """mr_nms_bev_batched with prefilled outputs and a spare element on both sides of keep and of num_keep
    -> keep (T + 2,) int64, num_keep (G + 2,) int32, return code"""
    from monorun_amd import _lib
    sizes = [len(g) for g in groups]
    T, G = sum(sizes), len(sizes)
    boxes = dev(np.concatenate(groups).astype(np.float32).reshape(-1, 5))
    sc = dev(np.concatenate(scores).astype(np.float32))
    offsets = dev(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32))
    keep = torch.full(((T + 2) * 8,), fill, dtype=torch.uint8, device=DEV).view(torch.int64)
    num = torch.full(((G + 2) * 4,), fill, dtype=torch.uint8, device=DEV).view(torch.int32)
    lib = _lib.load()
    code = lib.mr_nms_bev_batched(*_lib.pack('mr_nms_bev_batched', boxes_xyxyr=boxes.data_ptr(), scores=sc.data_ptr(), offsets=offsets.data_ptr(),
                                             groups=G, max_group=max(sizes, default=0) if max_group is None else max_group, thr=float(thr),
                                             keep=keep[1:].data_ptr(), num_keep=num[1:].data_ptr()), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return keep.cpu().numpy(), num.cpu().numpy(), code


def no_hip_error():
    from monorun_amd import _lib
    return _lib.load().mr_pnp_last_hip_error() == 0


@pytest.mark.parametrize('name,thr', CASE_THRS)
def test_abi_equals_the_expectation_and_writes_nothing_else(name, thr):
    c, want = nc.case(name), nc.expected(name, thr)
    sizes = [len(g) for g in c['groups']]
    keep, num, code = run_abi(c['groups'], c['scores'], thr, 0xFF)
    assert code == 0
    assert keep[0] == -1 and keep[-1] == -1 and num[0] == -1 and num[-1] == -1              # the spare elements
    off = np.concatenate([[0], np.cumsum(sizes)]) + 1
    wrong = []
    for g, (n, w) in enumerate(zip(sizes, want)):
        k = int(num[1 + g])
        if not (0 <= k <= n) or not np.array_equal(keep[off[g]:off[g] + k], w):
            wrong.append((g, n, k))
            continue
        assert np.all(keep[off[g] + k:off[g] + n] == -1), (g, n, k)                         # beyond num_keep inside the slot: untouched
    print(f'{name} thr {thr}: {len(sizes)} groups, {sum(sizes)} boxes, {int(num[1:-1].sum())} kept, {len(wrong)} groups differ')
    assert not wrong, wrong[:8]
    assert [int(num[1 + g]) for g, n in enumerate(sizes) if n == 0] == [0] * sizes.count(0)  # empty groups
    keep2, num2, code2 = run_abi(c['groups'], c['scores'], thr, 0x00)
    assert code2 == 0 and np.array_equal(num[1:-1], num2[1:-1]) and keep2[0] == 0 and keep2[-1] == 0 and num2[0] == 0 and num2[-1] == 0
    for g, n in enumerate(sizes):
        k = int(num[1 + g])
        assert np.array_equal(keep[off[g]:off[g] + k], keep2[off[g]:off[g] + k]) and np.all(keep2[off[g] + k:off[g] + n] == 0)
    assert no_hip_error()


def test_a_group_of_513_is_unsupported_and_touches_nothing():
    from monorun_amd.consumers import nms_bev
    rng = np.random.default_rng(5)
    g = _rand_boxes(rng, 513, spread=40.0)
    s = rng.uniform(0, 1, 513).astype(np.float32)
    small = nc.case('chains')
    keep, num, code = run_abi([small['groups'][0], g], [small['scores'][0], s], 0.25, 0xFF)
    assert code == MR_ERR_UNSUPPORTED and np.all(keep == -1) and np.all(num == -1)
    keep, num, code = run_abi([small['groups'][0]], [small['scores'][0]], 0.25, 0xFF, max_group=513)   # the argument alone decides
    assert code == MR_ERR_UNSUPPORTED and np.all(keep == -1) and np.all(num == -1)
    with pytest.raises(RuntimeError):
        nms_bev([dev(g)], [dev(s)], 0.25)
    k, = nms_bev([dev(g[:512])], [dev(s[:512])], 0.25)                                     # 512 is the limit, not beyond it
    assert 1 < len(k) <= 512
    assert no_hip_error()


@pytest.mark.parametrize('thr', NMS_THRS)
@pytest.mark.parametrize('name', ['every_n', 'special_scores'])
def test_consumers_nms_bev_in_a_batch_and_alone(name, thr):
    from monorun_amd.consumers import nms_bev
    c, want = nc.case(name), nc.expected(name, thr)
    out = nms_bev([dev(g) for g in c['groups']], [dev(s) for s in c['scores']], thr)
    assert len(out) == len(want)
    for g, (k, w) in enumerate(zip(out, want)):
        assert k.dtype == torch.int64 and np.array_equal(k.cpu().numpy(), w), (g, len(c['groups'][g]))
    alone = range(len(want)) if name == 'special_scores' else (0, 1, 31, 32, 63, 64, 99, 129)
    for g in alone:
        k, = nms_bev([dev(c['groups'][g])], [dev(c['scores'][g])], thr)
        assert np.array_equal(k.cpu().numpy(), out[g].cpu().numpy()), g
    assert no_hip_error()


@pytest.mark.parametrize('to_np', [True, False])
def test_multiclass_result_nms_with_nan_scores(orc, to_np):
    """classes: the special_scores groups of 33 and 100 (NaN and infinite scores), its group of 3 (one finite score, two NaN), a class
    of one NaN-scored box and an empty class (the reference's n <= 1 branch), as rows [l, h, w, x, y, z, ry, score]"""
    from monorun_amd.consumers import multiclass_3d_result_nms
    c = nc.case('special_scores')

    def rows(b, s):
        r = np.zeros((len(b), 8), np.float32)
        r[:, 0], r[:, 2] = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]                              # l, w
        r[:, 1], r[:, 4] = 1.5, 1.0                                                          # h, y
        r[:, 3], r[:, 5] = (b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2                  # x, z
        r[:, 6], r[:, 7] = b[:, 4], s
        return r
    res = [rows(c['groups'][i], c['scores'][i]) for i in (2, 3, 0)]
    res += [rows(c['groups'][0][2:3], c['scores'][0][2:3]), np.zeros((0, 8), np.float32)]
    assert np.isnan(res[3][0, 7]) and all(np.isnan(r[:, 7]).any() for r in res[:4])
    for thr in NMS_THRS:
        out, inds = multiclass_3d_result_nms([dev(r) for r in res], thr, to_np=to_np)
        if not to_np:
            assert all(torch.is_tensor(o) and o.device.type == 'cuda' for o in out) and all(i.dtype == torch.int64 for i in inds)
            out, inds = [o.cpu().numpy() for o in out], [i.cpu().numpy() for i in inds]
        for ci, r in enumerate(res[:3]):
            # the class's boxes as the consumer rebuilds them from the rows: within an ulp of the case's, whose pairs are all
            # further than KNIFE from the thresholds
            ref = orc.nms_bev(orc.xywhr2xyxyr(r[:, [3, 5, 0, 2, 6]]), r[:, 7], thr)
            assert np.array_equal(ref, nc.expected('special_scores', thr)[(2, 3, 0)[ci]])
            assert np.array_equal(inds[ci], ref) and np.array_equal(out[ci], r[ref], equal_nan=True), ci
            assert inds[ci].max() < len(r)
        assert inds[2].tolist() == [0, 2]
        assert inds[3].tolist() == [0] and np.array_equal(out[3], res[3], equal_nan=True) and inds[4].shape == (0,) and out[4].shape == (0, 8)
    assert no_hip_error()
