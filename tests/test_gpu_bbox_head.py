"""The detection head's HIP launches on the GPU: the rank launch through the C ABI (scores and boxes within C_SCORE /
C_BOX units of the float64 definition of tests/bbox_head_ref.py — 4 x the ratios measured for the fp32 torch restatement on the CPU —,
ranks and flags exact given its own scores), the select launch exact against select_ref on hand-made flags, get_bboxes by composition
in its three forms, the padded path without a host synchronisation, one fully independent case, the caps, and the chain from the RPN head
through the RoI extractor and this head back into the RoI extractor."""
import functools

import numpy as np
import pytest
import torch

from tests import bbox_head_ref as ref
from tests.proposals_ref import nms_ref32
from tests.test_bbox_head_cpu import check_end_to_end, check_groups, detect_forms, head, metas, rank_args

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
UNSUPPORTED = -2


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def guarded(rows, width, dtype, fill):
    """a buffer of rows + 2 rows, every byte `fill`: the launch gets the rows in the middle"""
    t = torch.empty((rows + 2) * width, dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(fill)
    return t


def untouched(t, width, fill):
    b = t.view(torch.uint8).cpu().numpy()
    n = width * t.element_size()
    return bool((b[:n] == fill).all() and (b[-n:] == fill).all())


def rank_abi(c, fill, max_rois=None):
    """mr_bbox_head_rank on a case into prefilled, guarded outputs -> code, (boxes, score, order, valid, group_offsets) as numpy, guards ok"""
    import ctypes
    from monorun_amd import _lib
    R, N, C = sum(c['counts']), len(c['counts']), c['C']
    T = R * C
    rois, cls, reg = dev(c['rois']), dev(c['cls']), dev(c['reg'])
    offsets = dev(np.concatenate([[0], np.cumsum(c['counts'])]).astype(np.int32))
    shapes = dev(c['img_shapes'])
    scale = None if c['scales'] is None else dev(c['scales'])
    out = dict(boxes=guarded(T, 4, torch.float32, fill), score=guarded(T, 1, torch.float32, fill), order=guarded(T, 1, torch.int32, fill),
               valid=guarded(T, 1, torch.uint8, fill), group_offsets=guarded(N * C + 1, 1, torch.int32, fill))
    width = dict(boxes=4, score=1, order=1, valid=1, group_offsets=1)
    f4 = ctypes.c_float * 4
    lib = _lib.load()
    code = lib.mr_bbox_head_rank(*_lib.pack(
        'mr_bbox_head_rank', cls_score=cls.data_ptr(), bbox_pred=reg.data_ptr(), rois=rois.data_ptr(), row_offsets=offsets.data_ptr(),
        img_shape=shapes.data_ptr(), scale_factor=_lib.ptr(scale), n_rois=R, n_images=N, num_classes=C, reg_class_agnostic=int(c['agnostic']),
        max_rois=max(c['counts']) if max_rois is None else max_rois, means=f4(*c['means']), stds=f4(*c['stds']), wh_ratio_clip=ref.WH_RATIO_CLIP,
        score_thr=c['score_thr'], **{k: t.data_ptr() + width[k] * t.element_size() for k, t in out.items()}),
        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ok = all(untouched(t, width[k], fill) for k, t in out.items())
    res = {k: t[width[k]:-width[k]].cpu().numpy() for k, t in out.items()}
    return code, (res['boxes'].reshape(-1, 4), res['score'], res['order'], res['valid'], res['group_offsets']), ok


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ------------------------------------------------------------------------------------------------ the rank launch
@pytest.mark.parametrize('name', ref.RANK_IDS)
def test_rank_launch_through_the_abi(name):
    """scores and boxes within the bounds of the float64 definition; order and valid exact given the launch's own scores; outputs into
    0xFF-prefilled buffers with guard rows; a second run into zeroed buffers bitwise equal"""
    c = ref.rank_case(name)
    code, (boxes, score, order, valid, groups), guards = rank_abi(c, 0xFF)
    assert code == 0 and guards
    C, T = c['C'], sum(c['counts']) * c['C']
    if T == 0:
        assert (raw(groups) == 0xFF).all()                  # no RoIs: nothing is launched, nothing written
        return
    sizes = ref.group_sizes(c['counts'], C)
    assert groups.tolist() == [0] + np.cumsum(sizes).tolist()
    s_rc = check_groups(c, boxes, score, order, valid)
    b_rc, = ref.ungroup(c['counts'], C, order, boxes)
    if c['agnostic']:
        assert all(np.array_equal(b_rc[:, 0], b_rc[:, k], equal_nan=True) for k in range(1, C))
        b_rc = b_rc[:, :1]
    rb, rs = ref.ratios(name, s_rc, b_rc)
    print(f'{name}: error in units: box {rb:.2f} (bound {ref.C_BOX:.2f}) score {rs:.2f} (bound {ref.C_SCORE:.2f})')
    assert rb <= ref.C_BOX and rs <= ref.C_SCORE
    code2, again, guards2 = rank_abi(c, 0x00)
    assert code2 == 0 and guards2
    assert all(np.array_equal(raw(a), raw(b)) for a, b in zip((boxes, score, order, valid, groups), again))


def test_rank_launch_cuts_an_image_to_max_rois():
    """a host bound below an image's row count: every kernel reads the image's first max_rois rows, the rest takes no part and nothing
    is written outside the buffers"""
    c = ref.rank_case('n3_65_0_129_c3')
    code, (boxes, score, order, valid, groups), guards = rank_abi(c, 0xFF, max_rois=100)
    assert code == 0 and guards
    C = 3
    assert groups.tolist() == [0, 65, 130, 195, 195, 195, 195, 295, 395, 582]
    cut = dict(c, rois=np.concatenate([c['rois'][:65], c['rois'][65:165]]), cls=np.concatenate([c['cls'][:65], c['cls'][65:165]]),
               reg=np.concatenate([c['reg'][:65], c['reg'][65:165]]), counts=(65, 0, 100))
    _, (b2, s2, o2, v2, _), _ = rank_abi(cut, 0xFF)
    assert np.array_equal(raw(boxes[:495]), raw(b2)) and np.array_equal(raw(score[:495]), raw(s2))
    assert np.array_equal(order[:495], o2) and np.array_equal(valid[:495], v2)
    assert (raw(score[495:]) == 0xFF).all() and (raw(valid[495:]) == 0xFF).all()


def test_non_contiguous_inputs_equal_the_contiguous_call():
    """cls_score and bbox_pred as column slices of ONE fused output (class-agnostic, C = 3: both contiguous copies have the same size, so a
    copy freed before the launch would hand its block to the next), rois as a slice of a wider table, scale_factor as an expanded tensor:
    the launches read copies that live across them; rank and get_bboxes equal the contiguous call bitwise"""
    from monorun_amd.bbox_head import hip_ok, rank
    c = ref.rank_case('k1025_c3_agnostic')
    c = dict(c, scales=np.tile(np.asarray(ref.SCALES[0], np.float32), (1, 1)))
    args = rank_args(c, DEV)
    R = sum(c['counts'])
    fused = torch.cat([args[1], args[2]], dim=1).contiguous()                  # (R, 4 + 4)
    cls_v, reg_v = fused[:, :4], fused[:, 4:]
    rois_v = torch.cat([args[0], torch.full((R, 1), 7.0, device=DEV)], dim=1)[:, :5]
    scale_v = dev(np.asarray(ref.SCALES[0], np.float32)).reshape(1, 4).expand(1, 4).t().contiguous().t()       # (1, 4), strides (1, 1)
    assert not cls_v.is_contiguous() and not reg_v.is_contiguous() and not rois_v.is_contiguous()
    assert torch.equal(cls_v, args[1]) and torch.equal(reg_v, args[2]) and torch.equal(rois_v, args[0]) and hip_ok(rois_v, cls_v, reg_v, c['counts'], 3)
    want = rank(*args)
    for _ in range(2):                                                          # the second call finds the first one's blocks in the cache
        got = rank(rois_v, cls_v, reg_v, c['counts'], args[4], scale_v, *args[6:])
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(got, want))
    h = head(3, True).to(DEV)
    shapes, scales = metas(c)
    cfg = dict(score_thr=c['score_thr'], nms=dict(type='nms', iou_threshold=0.5), max_per_img=100)
    want = h.get_bboxes(args[0], args[1], args[2], shapes[0], scales[0], rescale=True, cfg=cfg, padded=True)
    for _ in range(2):
        got = h.get_bboxes(rois_v, cls_v, reg_v, shapes[0], dev(np.asarray(ref.SCALES[0], np.float32)), rescale=True, cfg=cfg, padded=True)
        assert all(torch.equal(a.nan_to_num(-7.0), b.nan_to_num(-7.0)) for a, b in zip(got, want)) and 0 < int(want[2][0]) <= 100


def detect_abi(c, max_rois, max_num, iou_thr=0.5):
    """mr_bbox_head_detect on a case with a host bound of its own -> code, dets (N, max_num, 5), labels, counts as numpy"""
    import ctypes
    from monorun_amd import _lib
    R, N, C = sum(c['counts']), len(c['counts']), c['C']
    rois, cls, reg = dev(c['rois']), dev(c['cls']), dev(c['reg'])
    offsets = dev(np.concatenate([[0], np.cumsum(c['counts'])]).astype(np.int32))
    shapes, scale = dev(c['img_shapes']), None if c['scales'] is None else dev(c['scales'])
    dets, labels, num = guarded(N * max_num, 5, torch.float32, 0xFF), guarded(N * max_num, 1, torch.int64, 0xFF), guarded(N, 1, torch.int32, 0xFF)
    lib = _lib.load()
    ws = torch.full((lib.mr_bbox_head_workspace_bytes(R, N, C, max_rois) // 8 + 2,), -1, dtype=torch.int64, device=DEV)
    f4 = ctypes.c_float * 4
    code = lib.mr_bbox_head_detect(*_lib.pack(
        'mr_bbox_head_detect', cls_score=cls.data_ptr(), bbox_pred=reg.data_ptr(), rois=rois.data_ptr(), row_offsets=offsets.data_ptr(),
        img_shape=shapes.data_ptr(), scale_factor=_lib.ptr(scale), n_rois=R, n_images=N, num_classes=C, reg_class_agnostic=int(c['agnostic']),
        max_rois=max_rois, means=f4(*c['means']), stds=f4(*c['stds']), wh_ratio_clip=ref.WH_RATIO_CLIP, score_thr=c['score_thr'], iou_thr=iou_thr,
        max_num=max_num, dets=dets.data_ptr() + 20, labels=labels.data_ptr() + 8, counts=num.data_ptr() + 4, workspace=ws.data_ptr()),
        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert untouched(dets, 5, 0xFF) and untouched(labels, 1, 0xFF) and untouched(num, 1, 0xFF) and int(ws[-1]) == -1
    return code, dets[5:-5].cpu().numpy().reshape(N, max_num, 5), labels[1:-1].cpu().numpy().reshape(N, max_num), num[1:-1].cpu().numpy()


def cut_case():
    """n3_65_0_129_c3 and the same case with its third image cut to its first 100 rows"""
    c = ref.rank_case('n3_65_0_129_c3')
    return c, dict(c, rois=c['rois'][:165], cls=c['cls'][:165], reg=c['reg'][:165], counts=(65, 0, 100))


@pytest.mark.parametrize('max_num', [10, 400])
def test_detect_cuts_an_image_to_max_rois(max_num):
    """all four launches with a host bound below an image's row count: the result is that of the image's first max_rois rows, the
    workspace's spare word and the guards stay untouched"""
    c, cut = cut_case()
    code, dets, labels, num = detect_abi(c, 100, max_num)
    code2, dets2, labels2, num2 = detect_abi(cut, 100, max_num)
    assert code == 0 and code2 == 0 and num.tolist() == num2.tolist() and num[1] == 0 and num[2] > 0
    assert np.array_equal(raw(dets), raw(dets2)) and np.array_equal(labels, labels2)
    boxes, score, order, valid, keep = composed('n3_65_0_129_c3', 0.5)
    assert np.array_equal(dets[0, :num[0]], ref.select_ref(boxes, score, order, keep, c['counts'], 3, max_num)[0][0])    # image 0 is not cut
    _, _, _, full = detect_abi(c, 129, max_num)
    assert max_num < 400 or full[2] != num[2]                  # the cut does change the third image's result


def test_select_launch_cuts_an_image_to_max_rois():
    """mr_bbox_head_select alone on the rank launch's cut groups: equal to select_ref on the cut case's groups"""
    from monorun_amd import _lib
    c, cut = cut_case()
    _, (boxes, score, order, valid, _), _ = rank_abi(c, 0x00, max_rois=100)
    _, (b2, s2, o2, v2, _), _ = rank_abi(cut, 0x00)
    keep = np.zeros(len(score), np.uint8)
    keep[:495] = nms_ref32(b2, v2, ref.group_sizes(cut['counts'], 3), 0.5)
    keep[495:] = 1                                              # places behind the cut groups: never read
    want = ref.select_ref(b2, s2, o2, keep[:495], cut['counts'], 3, 50)
    N, R = 3, sum(c['counts'])
    offsets = dev(np.concatenate([[0], np.cumsum(c['counts'])]).astype(np.int32))
    dets, labels, num = guarded(N * 50, 5, torch.float32, 0xFF), guarded(N * 50, 1, torch.int64, 0xFF), guarded(N, 1, torch.int32, 0xFF)
    b, s_, o, k = dev(boxes), dev(score), dev(order), dev(keep)
    code = _lib.load().mr_bbox_head_select(*_lib.pack(
        'mr_bbox_head_select', boxes=b.data_ptr(), score=s_.data_ptr(), order=o.data_ptr(), keep=k.data_ptr(), row_offsets=offsets.data_ptr(),
        n_rois=R, n_images=N, num_classes=3, max_rois=100, max_num=50, dets=dets.data_ptr() + 20, labels=labels.data_ptr() + 8,
        counts=num.data_ptr() + 4), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert code == 0 and untouched(dets, 5, 0xFF) and untouched(labels, 1, 0xFF) and untouched(num, 1, 0xFF)
    dets, labels, num = dets[5:-5].cpu().numpy().reshape(N, 50, 5), labels[1:-1].cpu().numpy().reshape(N, 50), num[1:-1].cpu().numpy()
    assert num.tolist() == [len(d) for d, _ in want]
    for n, (wd, wl) in enumerate(want):
        assert np.array_equal(dets[n, :len(wd)], wd) and np.array_equal(labels[n, :len(wd)], wl) and np.isnan(dets[n, len(wd):]).all()


# ------------------------------------------------------------------------------------------------ the select launch
def select_inputs(seed, counts, C, levels):
    """hand-made groups: scores on a few levels (ties inside a class and across classes), ranked by rank_ref"""
    rng = np.random.RandomState(seed)
    R = sum(counts)
    s_rc = (rng.randint(1, levels + 1, size=(R, C)) / np.float32(levels)).astype(np.float32)
    b_rc = rng.uniform(0, 100, size=(R, C, 4)).astype(np.float32)
    boxes, score, order, _ = ref.groups_ref(b_rc, s_rc, np.ones((R, C), bool), counts)
    return boxes, score, order


SELECT_TABLE = {                # counts, C, score levels
    'k130_c3_ties': ((130,), 3, 5),
    'n3_65_0_1000_c3': ((65, 0, 1000), 3, 40),
    'k4096_c1': ((4096,), 1, 300),
    'n2_70_3_c16': ((70, 3), 16, 7),
    'k64_c2': ((64,), 2, 3),
}
KEEP_PATTERNS = ('random', 'all', 'none', 'last_class')


def select_abi(boxes, score, order, keep, counts, C, max_num, fill):
    from monorun_amd import _lib
    N, R = len(counts), sum(counts)
    offsets = dev(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32))
    dets, labels, num = guarded(N * max_num, 5, torch.float32, fill), guarded(N * max_num, 1, torch.int64, fill), guarded(N, 1, torch.int32, fill)
    b, s, o, k = dev(boxes), dev(score), dev(order), dev(keep)
    code = _lib.load().mr_bbox_head_select(*_lib.pack(
        'mr_bbox_head_select', boxes=b.data_ptr(), score=s.data_ptr(), order=o.data_ptr(), keep=k.data_ptr(), row_offsets=offsets.data_ptr(),
        n_rois=R, n_images=N, num_classes=C, max_rois=max(counts), max_num=max_num, dets=dets.data_ptr() + 20, labels=labels.data_ptr() + 8,
        counts=num.data_ptr() + 4), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert untouched(dets, 5, fill) and untouched(labels, 1, fill) and untouched(num, 1, fill)
    return code, dets[5:-5].cpu().numpy().reshape(N, max_num, 5), labels[1:-1].cpu().numpy().reshape(N, max_num), num[1:-1].cpu().numpy()


@pytest.mark.parametrize('name', list(SELECT_TABLE))
@pytest.mark.parametrize('pattern', KEEP_PATTERNS)
def test_select_launch_through_the_abi(name, pattern):
    """exact against select_ref on hand-made keep flags: max_num 1, 100 and more than is kept; cross-class ties to the lower r C + c"""
    counts, C, levels = SELECT_TABLE[name]
    boxes, score, order = select_inputs(31, counts, C, levels)
    T = len(score)
    rng = np.random.RandomState(5)
    keep = dict(random=(rng.uniform(size=T) < 0.3), all=np.ones(T, bool), none=np.zeros(T, bool))[pattern] if pattern != 'last_class' else \
        np.concatenate([np.repeat(np.arange(C) == C - 1, k) for k in counts])
    keep = keep.astype(np.uint8)
    for max_num in (1, 100, int(keep.sum()) + 3):
        want = ref.select_ref(boxes, score, order, keep, counts, C, max_num)
        code, dets, labels, num = select_abi(boxes, score, order, keep, counts, C, max_num, 0xFF)
        assert code == 0 and num.tolist() == [len(d) for d, _ in want]
        for n, (wd, wl) in enumerate(want):
            k = len(wd)
            assert np.array_equal(dets[n, :k], wd) and np.array_equal(labels[n, :k], wl)
            assert np.isnan(dets[n, k:]).all() and (labels[n, k:] == -1).all()
        again = select_abi(boxes, score, order, keep, counts, C, max_num, 0x00)
        assert all(np.array_equal(raw(a), raw(b)) for a, b in zip((dets, labels, num), again[1:]))
    if pattern == 'all' and levels <= 7:
        d = ref.select_ref(boxes, score, order, keep, counts, C, 0)[0][0]
        assert (np.diff(d[:, 4]) == 0).mean() > 0.5           # the case does hold ties, inside and across classes


# ------------------------------------------------------------------------------------------------ get_bboxes
@functools.lru_cache(maxsize=None)
def composed(name, iou_thr):
    """the rank launch's own public output on a case and nms_ref32 on it, computed once and shared"""
    from monorun_amd.bbox_head import hip_ok, rank
    c = ref.rank_case(name)
    args = rank_args(c, DEV)
    assert hip_ok(*args[:4], c['C']), 'the test must run the HIP path'
    boxes, score, order, valid = (x.cpu().numpy() for x in rank(*args))
    keep = nms_ref32(boxes, valid, ref.group_sizes(c['counts'], c['C']), iou_thr)
    return boxes, score, order, valid, keep


@pytest.mark.parametrize('name,max_num', [('n3_65_0_129_c3', 20), ('n3_65_0_129_c3', 400), ('k1000_c3', 100), ('special_c3', 50),
                                          ('k129_c1_agnostic', 30), ('special_n3_c1_agnostic', 200), ('k1025_c3_agnostic', 100)])
def test_get_bboxes_by_composition(name, max_num):
    """get_bboxes equals, bitwise, nms_ref32 plus select_ref applied to the rank launch's own public output, in the list, the padded and
    the per-image forms (detect_forms asserts them equal to each other)"""
    c = ref.rank_case(name)
    boxes, score, order, valid, keep = composed(name, 0.5)
    want = ref.select_ref(boxes, score, order, keep, c['counts'], c['C'], max_num)
    dets, labels, num = detect_forms(c, head(c['C'], c['agnostic']).to(DEV), DEV, max_num)
    assert dets.device.type == 'cuda' and num.tolist() == [len(d) for d, _ in want]
    for n, (wd, wl) in enumerate(want):
        assert np.array_equal(dets[n, :len(wd)].cpu().numpy(), wd) and np.array_equal(labels[n, :len(wd)].cpu().numpy(), wl)
    assert 0 < keep.sum() < valid.sum()


def test_get_bboxes_equal_counts_as_a_batch():
    c = ref.make_case(77, (40, 40), 3, False, True)
    detect_forms(c, head(3).to(DEV), DEV, 30)


def test_padded_path_performs_no_host_synchronisation():
    c = ref.rank_case('n3_65_0_129_c3')
    h = head(3).to(DEV)
    shapes, scales = metas(c)
    cfg = dict(score_thr=c['score_thr'], nms=dict(type='nms', iou_threshold=0.5), max_per_img=40)
    rois, cls, reg, scale_rows = dev(c['rois']), dev(c['cls']), dev(c['reg']), dev(c['scales'])         # copied before the mode is set
    want = h.get_bboxes(rois, cls, reg, shapes, scales, rescale=True, cfg=cfg, padded=True, roi_counts=c['counts'])      # warm
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = h.get_bboxes(rois, cls, reg, shapes, scales, rescale=True, cfg=cfg, padded=True, roi_counts=c['counts'])
        got2 = h.get_bboxes(rois, cls, reg, shapes, scale_rows, rescale=True, cfg=cfg, padded=True, roi_counts=c['counts'])
    finally:
        torch.cuda.set_sync_debug_mode('default')
    for g in (got, got2):
        assert all(torch.equal(a.nan_to_num(-7.0), b.nan_to_num(-7.0)) for a, b in zip(g, want))
    assert want[2].tolist()[1] == 0 and want[2].sum() > 0


def test_get_bboxes_end_to_end_against_the_float64_definition():
    check_end_to_end(DEV)


def test_4097_rows_are_unsupported_and_run_the_restatement():
    from monorun_amd import _lib
    from monorun_amd.bbox_head import hip_ok, rank
    c = ref.make_case(21, (4097,), 1, False, False)
    code, (boxes, score, order, valid, groups), guards = rank_abi(c, 0xFF)
    assert code == UNSUPPORTED and guards and (raw(score) == 0xFF).all() and (raw(groups) == 0xFF).all()      # before any launch
    args = rank_args(c, DEV)
    assert not hip_ok(*args[:4], 1) and hip_ok(args[0][:4096], args[1][:4096], args[2][:4096], (4096,), 1)
    b, s, o, v = (x.cpu().numpy() for x in rank(*args))
    s_rc, b_rc = ref.ungroup(c['counts'], 1, o, s, b)
    want = ref.detect_ref32(c, 0.5, 100, scores=s_rc, boxes=b_rc)
    assert np.array_equal(o, want['order']) and np.array_equal(v.astype(bool), want['valid'])
    shapes, scales = metas(c)
    cfg = dict(score_thr=c['score_thr'], nms=dict(type='nms', iou_threshold=0.5), max_per_img=100)
    dets, labels = head(1).to(DEV).get_bboxes(args[0], args[1], args[2], shapes[0], scales[0], cfg=cfg)
    assert dets.device.type == 'cuda' and np.array_equal(dets.cpu().numpy(), want['dets'][0][0])
    assert np.array_equal(labels.cpu().numpy(), want['dets'][0][1]) and len(dets) == 100
    assert _lib.load().mr_pnp_last_hip_error() == 0


# ------------------------------------------------------------------------------------------------ the chain
def test_the_chain_from_the_rpn_to_the_second_extraction():
    """simple_test_rpn(padded) -> SingleRoIExtractor -> Shared2FCBBoxHead -> get_bboxes(padded) -> rescaled bbox2roi -> SingleRoIExtractor,
    every step on its HIP path and none synchronising with the host before the final read; padded proposal rows yield no detection: the
    result is that of the real proposals alone"""
    from monorun_amd import roi_extractor as R
    from monorun_amd.bbox_head import Shared2FCBBoxHead, bbox2roi, hip_ok
    from tests import proposals_ref as pref
    from tests.test_proposals_cpu import head as rpn_head, metas as rpn_metas
    rpn = rpn_head(nms_post=200, max_num=200).to(DEV)       # more rows than candidates: every image has padded rows
    g = torch.Generator().manual_seed(13)
    N = pref.N_IMAGES
    feats = [torch.randn(N, 8, 2 * pref.MAPS[0][0], 2 * pref.MAPS[0][1], generator=g).to(DEV)] + \
            [torch.randn(N, 8, hh, ww, generator=g).to(DEV) for hh, ww in pref.MAPS]
    ext = R.SingleRoIExtractorMod(dict(type='RoIAlign', output_size=7, sampling_ratio=0), 8, list(pref.STRIDES), finest_scale=16, starting_level=1)
    box_head = Shared2FCBBoxHead(in_channels=8, fc_out_channels=32, roi_feat_size=7, num_classes=3,
                                 bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=ref.MEANS, target_stds=ref.STDS)).to(DEV)
    cfg = dict(score_thr=0.4, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100)
    shapes = [(int(h), int(w), 3) for h, w in pref.IMG_SHAPES]
    scales = [np.asarray([1.5, 1.25, 1.5, 1.25], np.float32), np.asarray([0.8, 0.8, 0.8, 0.8], np.float32)]
    scale_rows = dev(np.stack(scales))
    image = torch.arange(N, device=DEV, dtype=torch.float32)[:, None, None]
    with torch.no_grad():
        for p in list(rpn.parameters()) + list(box_head.parameters()):
            p.copy_((torch.randn(p.shape, generator=g) * 0.15).to(DEV))
        box_head.fc_cls.weight.mul_(4.0)

        def run(sync_free):
            if sync_free:
                torch.cuda.set_sync_debug_mode('error')
            try:
                props, counts = rpn.simple_test_rpn(feats, rpn_metas(), padded=True)
                P = props.shape[1]
                rois = torch.cat([image.expand(N, P, 1), props[..., :4]], dim=-1)
                x = ext(feats, rois.reshape(N * P, 5))
                cls, reg = box_head(x)
                assert R.hip_ok(feats[1:], rois.reshape(N * P, 5), (7, 7)) and hip_ok(rois.reshape(-1, 5), cls, reg, [P] * N, 3)
                dets, labels, num = box_head.get_bboxes(rois, cls, reg, shapes, scales, rescale=True, cfg=cfg, padded=True)
                rois2 = torch.cat([image.expand(N, dets.shape[1], 1), dets[..., :4] * scale_rows[:, None, :]], dim=-1).reshape(-1, 5)
                x2 = ext(feats, rois2)
            finally:
                torch.cuda.set_sync_debug_mode('default')
            return props, counts, cls, reg, dets, labels, num, rois2, x2

        run(False)                                          # warm: the library is loaded, the tables are cached
        torch.cuda.synchronize()
        props, counts, cls, reg, dets, labels, num, rois2, x2 = run(True)
        P, M = props.shape[1], dets.shape[1]
        assert all(0 < k < P for k in counts.tolist()) and all(0 < k < M for k in num.tolist())
        from monorun_amd.bbox_head import softmax_torch
        assert (softmax_torch(cls[-1:])[:, :3] > cfg['score_thr']).any()                # a padded row's score alone would pass the threshold
        real = [props[n, :k] for n, k in enumerate(counts.tolist())]                  # the real proposals alone, in mmdet's list form
        pick = torch.cat([torch.arange(n * P, n * P + k) for n, k in enumerate(counts.tolist())]).to(DEV)
        dl, ll = box_head.get_bboxes(bbox2roi(real), cls[pick], reg[pick], shapes, scales, rescale=True, cfg=cfg, roi_counts=counts.tolist())
        x2 = x2.reshape(N, M, 8, 7, 7)
        for n, k in enumerate(num.tolist()):
            assert torch.equal(dets[n, :k], dl[n]) and torch.equal(labels[n, :k], ll[n]) and len(dl[n]) == k
            assert torch.isnan(dets[n, k:]).all() and (labels[n, k:] == -1).all() and (x2[n, k:] == 0).all()
            assert torch.isfinite(x2[n, :k]).all() and x2[n, :k].abs().max() > 0
            again = ext(feats, bbox2roi([dl[0][:0]] * n + [dl[n][:, :4] * scale_rows[n]]))
            assert torch.equal(again, x2[n, :k])
