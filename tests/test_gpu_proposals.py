"""The proposal stage's HIP launches on the GPU: the grouped NMS exact against the float32 definition of
tests/proposals_ref.py through the C ABI and through nms / batched_nms / multiclass_nms, the decode against the float64 definition within
C_BOX / C_SCORE 2^-23 magnitudes (4 x the ratios measured for the fp32 torch restatement on the CPU), get_bboxes by composition and on
one fully independent case, the padded path without a host synchronisation, and the head in front of the RoI extractor."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import proposals_ref as ref
from tests.test_proposals_cpu import MULTICLASS, SCORED, check_end_to_end, head, metas, multiclass_inputs

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CASES = {c['name']: c for c in ref.nms_cases()}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def want32(name):
    """the float32 definition on a case, computed once and shared"""
    c = CASES[name]
    keep = ref.nms_ref32(c['boxes'], c['valid'], c['sizes'], c['thr'])
    keep.setflags(write=False)
    return keep


def run_abi(c, fill):
    """mr_nms_grouped on a case with prefilled outputs and spare elements on both sides of keep -> keep (T + 2,), num_keep (G,), code"""
    from monorun_amd import _lib
    from monorun_amd.proposals import nms_workspace_bytes
    T, G = len(c['boxes']), len(c['sizes'])
    boxes = dev(c['boxes'])
    valid = None if c['valid'] is None else dev(c['valid'])
    offsets = dev(np.concatenate([[0], np.cumsum(c['sizes'])]).astype(np.int32))
    keep = torch.full((T + 2,), fill, dtype=torch.uint8, device=DEV)
    num = torch.full((max(G, 1),), -7, dtype=torch.int32, device=DEV)
    ws = torch.full((nms_workspace_bytes(c['sizes']) // 8 + 1,), -1, dtype=torch.int64, device=DEV)      # all ones where nobody writes
    lib = _lib.load()
    code = lib.mr_nms_grouped(*_lib.pack('mr_nms_grouped', boxes=boxes.data_ptr(), valid=_lib.ptr(valid), offsets=offsets.data_ptr(), groups=G,
                                         max_group=max(c['sizes'], default=0), thr=c['thr'], keep=keep[1:].data_ptr(), num_keep=num.data_ptr(),
                                         workspace=ws.data_ptr()), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return keep.cpu().numpy(), num.cpu().numpy()[:G], code, int(ws[-1].item())


@pytest.mark.parametrize('name', ref.NMS_IDS)
def test_nms_grouped_abi_equals_the_definition(name):
    """exact, into 0xFF-prefilled buffers (and the spare elements around keep and after the workspace untouched), twice bitwise equal"""
    c, want = CASES[name], want32(name)
    keep, num, code, guard = run_abi(c, 0xFF)
    assert code == 0 and guard == -1 and keep[0] == 0xFF and keep[-1] == 0xFF
    if max(c['sizes'], default=0) == 0:
        assert (keep == 0xFF).all() and (num == -7).all()              # no boxes: nothing is launched, nothing written
        return
    assert set(np.unique(keep[1:-1])) <= {0, 1} and np.array_equal(keep[1:-1].astype(bool), want)
    ends = np.cumsum(c['sizes'])
    assert num.tolist() == [int(want[e - n:e].sum()) for e, n in zip(ends, c['sizes'])]
    keep2, num2, _, _ = run_abi(c, 0x00)
    assert np.array_equal(keep[1:-1], keep2[1:-1]) and np.array_equal(num, num2)


def test_a_group_of_4097_is_unsupported_and_runs_the_restatement():
    from monorun_amd import _lib
    from monorun_amd.proposals import hip_ok, nms_grouped
    boxes = np.concatenate([ref._far(4097, [(0, 4096), (5, 70)]), ref._grid(3)])
    c = dict(boxes=boxes, valid=None, sizes=(4097, 3), thr=0.5)
    keep, num, code, _ = run_abi(c, 0xFF)
    assert code == -2 and (keep == 0xFF).all() and (num == -7).all()        # MR_ERR_UNSUPPORTED before any launch
    assert not hip_ok(dev(boxes), c['sizes']) and hip_ok(dev(boxes), (4096, 4))
    got, n = nms_grouped(dev(boxes), None, c['sizes'], 0.5)
    want = ref.nms_ref32(boxes, None, c['sizes'], 0.5)
    assert got.device.type == 'cuda' and np.array_equal(got.cpu().numpy().astype(bool), want) and n.tolist() == [4095, 3]
    assert _lib.load().mr_pnp_last_hip_error() == 0


@pytest.mark.parametrize('name', ref.NMS_IDS)
def test_nms_grouped_python_entry(name):
    from monorun_amd.proposals import hip_ok, nms_grouped
    c, want = CASES[name], want32(name)
    boxes = dev(c['boxes'])
    assert hip_ok(boxes, c['sizes']), 'the test must run the HIP path'
    keep, num = nms_grouped(boxes, None if c['valid'] is None else dev(c['valid']).bool(), c['sizes'], c['thr'])
    assert keep.dtype == torch.uint8 and num.dtype == torch.int32 and np.array_equal(keep.cpu().numpy().astype(bool), want)
    assert int(num.sum()) == int(want.sum())


@pytest.mark.parametrize('name', SCORED)
def test_nms_and_batched_nms(name):
    """shuffled inputs with tied scores: score-descending order, ties to the lower input index; non-contiguous boxes"""
    from monorun_amd.proposals import batched_nms, nms
    c = CASES[name]
    boxes, scores, idxs = ref.scored(c)
    want = ref.batched_nms_ref(boxes, scores, idxs, c['thr'])
    wide = dev(np.concatenate([boxes, boxes], axis=1))[:, :4]
    assert not wide.is_contiguous() or len(boxes) < 2
    dets, keep = batched_nms(wide, dev(scores), dev(idxs), dict(type='nms', iou_threshold=c['thr'], split_thr=10))
    assert keep.dtype == torch.int64 and np.array_equal(keep.cpu().numpy(), want)
    assert np.array_equal(dets.cpu().numpy(), np.concatenate([boxes[want], scores[want, None]], axis=1), equal_nan=True)
    want = ref.batched_nms_ref(boxes, scores, np.zeros_like(idxs), c['thr'])
    dets, keep = nms(dev(boxes), dev(scores), c['thr'])
    assert np.array_equal(keep.cpu().numpy(), want) and dets.shape == (len(want), 5)


@pytest.mark.parametrize('C,per_class,score_thr,max_num,factors', MULTICLASS)
def test_multiclass_nms(C, per_class, score_thr, max_num, factors):
    from monorun_amd.proposals import multiclass_nms
    boxes, scores, fac = multiclass_inputs(C, per_class)
    fac = fac if factors else None
    want_d, want_l = ref.multiclass_nms_ref(boxes, scores, score_thr, 0.5, max_num, fac)
    dets, labels = multiclass_nms(dev(boxes), dev(scores), score_thr, dict(type='nms', iou_threshold=0.5), max_num, None if fac is None else dev(fac))
    assert dets.device.type == 'cuda' and dets.shape == want_d.shape and labels.shape == want_l.shape
    assert np.array_equal(dets.cpu().numpy(), want_d) and np.array_equal(labels.cpu().numpy(), want_l)


# ------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize('name', list(ref.DECODE_CASES))
@pytest.mark.parametrize('noncontiguous', [False, True])
def test_decode_within_the_bounds(name, noncontiguous):
    """against decode_ref64: two image shapes, three levels, both sides of the wh clamp, all four borders, min_bbox_size 0 and 8"""
    from monorun_amd.proposals import decode_hip_ok, proposal_decode
    m = ref.DECODE_CASES[name]
    c = ref.decode_case(m)
    b64, s64, lg, v, mag = ref.decode_ref64(c['cls'], c['reg'], c['index'], c['counts'], c['img_shape'], c['base'], ref.STRIDES, ref.MEANS,
                                            ref.STDS, min_bbox_size=m)
    cls, reg = [dev(x) for x in c['cls']], [dev(x) for x in c['reg']]
    if noncontiguous:
        cls = [x.transpose(2, 3).contiguous().transpose(2, 3) for x in cls]
        reg = [x.transpose(2, 3).contiguous().transpose(2, 3) for x in reg]
        assert not cls[0].is_contiguous() and not reg[0].is_contiguous()
    index = dev(c['index'])
    assert decode_hip_ok(cls, reg, index), 'the test must run the HIP path'
    boxes, score, logit, valid = proposal_decode(cls, reg, index, c['counts'], dev(c['img_shape']), [torch.from_numpy(x) for x in c['base']],
                                                 ref.STRIDES, ref.MEANS, ref.STDS, min_bbox_size=m)
    boxes, score, logit, valid = boxes.cpu().numpy(), score.cpu().numpy(), logit.cpu().numpy(), valid.cpu().numpy()
    rb = float((np.abs(boxes.astype(np.float64) - b64) / (ref.EPS * mag)).max())
    rs = float((np.abs(score.astype(np.float64) - s64) / (ref.EPS * s64)).max())
    print(f'{name}: error / (2^-23 magnitude): box {rb:.2f} (bound {ref.C_BOX}) score {rs:.2f} (bound {ref.C_SCORE})')
    assert rb <= ref.C_BOX and rs <= ref.C_SCORE
    assert np.array_equal(logit, lg) and set(np.unique(valid)) <= {0, 1}
    sides = np.stack([b64[..., 2] - b64[..., 0], b64[..., 3] - b64[..., 1]])
    clear = (np.abs(sides - m) > 1e-3).all(axis=0) | (m == 0)
    assert np.array_equal(valid.astype(bool)[clear], v[clear])


# ------------------------------------------------------------------------------------------------ get_bboxes
@pytest.mark.parametrize('nms_pre', [0, 100, 10 ** 6])
def test_get_bboxes_by_composition(nms_pre):
    """get_bboxes equals, bitwise, nms_ref32 plus the merge rule on the decode launch's own public output for the same selection: that
    pins selection, grouping, merge, nms_post, the padded form (counts, NaN tail) and the list form; starting_level 1, four input maps"""
    from monorun_amd.proposals import proposal_decode
    nms_post = 250          # between the survivors of nms_pre 100 (about 200 per image) and of all anchors (about 700)
    h = head(nms_pre=nms_pre, nms_post=nms_post, max_num=nms_post, nms_thr=0.7, min_bbox_size=3.0).to(DEV)
    g = torch.Generator().manual_seed(9)
    feats = [torch.randn(ref.N_IMAGES, 8, 2 * ref.MAPS[0][0], 2 * ref.MAPS[0][1], generator=g)] + \
            [torch.randn(ref.N_IMAGES, 8, hh, ww, generator=g) for hh, ww in ref.MAPS]
    with torch.no_grad():
        for p in h.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.15)
        cls, reg = h([f.to(DEV) for f in feats])
    assert len(cls) == 3 and cls[0].shape == (ref.N_IMAGES, 3) + ref.MAPS[0]
    out, counts = h.get_bboxes(cls, reg, metas(), padded=True)
    lst = h.get_bboxes(cls, reg, metas())
    index, level_counts = ref.select_ref([x.cpu().numpy() for x in cls], nms_pre)
    assert level_counts == [min(nms_pre, 3 * hh * ww) if nms_pre > 0 else 3 * hh * ww for hh, ww in ref.MAPS]
    boxes, score, logit, valid = proposal_decode(cls, reg, dev(index), level_counts, dev(np.asarray(ref.IMG_SHAPES, ref.F32)),
                                                 h.anchor_generator.base_anchors, ref.STRIDES, ref.MEANS, ref.STDS, min_bbox_size=3.0)
    boxes, score, logit, valid = boxes.cpu().numpy(), score.cpu().numpy(), logit.cpu().numpy(), valid.cpu().numpy()
    keep = ref.nms_ref32(boxes.reshape(-1, 4), valid.reshape(-1), tuple(level_counts) * ref.N_IMAGES, 0.7).reshape(ref.N_IMAGES, -1)
    want = ref.merge_ref(boxes, score, logit, keep, nms_post)
    assert (valid == 0).any() and (keep.sum(1) < valid.sum(1)).all()
    assert out.shape == (ref.N_IMAGES, nms_post, 5) and counts.dtype == torch.int32 and counts.tolist() == [len(w) for w in want]
    for n, w in enumerate(want):
        assert np.array_equal(lst[n].cpu().numpy(), w) and np.array_equal(out[n, :len(w)].cpu().numpy(), w)
        assert torch.isnan(out[n, len(w):]).all()
    if nms_pre == 100:
        assert all(0 < len(w) < nms_post for w in want)
    else:
        assert all(len(w) == nms_post for w in want)


def test_get_bboxes_end_to_end_against_the_float64_definition():
    check_end_to_end(DEV)


def test_padded_path_performs_no_host_synchronisation():
    c = ref.e2e_case()
    h = head().to(DEV)
    cls, reg = [dev(x) for x in c['cls']], [dev(x) for x in c['reg']]
    want = h.get_bboxes(cls, reg, metas())                              # warm: the library is loaded, the offsets are cached
    shapes = dev(c['img_shape'])                                        # the image shapes as a device tensor: copied before the mode is set
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        out, counts = h.get_bboxes(cls, reg, metas(), padded=True)
        out2, counts2 = h.get_bboxes(cls, reg, shapes, padded=True)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.equal(counts, counts2) and torch.equal(out.nan_to_num(-1.0), out2.nan_to_num(-1.0))
    for n, k in enumerate(counts.tolist()):
        assert torch.equal(out[n, :k], want[n])


def test_sync_debug_mode_is_implemented():
    """the test above proves something only if this build raises on a synchronising call"""
    x = torch.ones(3, device=DEV)
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            x.sum().item()
    finally:
        torch.cuda.set_sync_debug_mode('default')


def test_the_chain_to_the_roi_extractor():
    """simple_test_rpn -> bbox2roi-style (K, 5) RoIs -> SingleRoIExtractor, both on their HIP paths; the padded form flattened gives zeros
    for the padded rows"""
    from monorun_amd import roi_extractor as R
    from monorun_amd.proposals import decode_hip_ok
    h = head(nms_post=200, max_num=200).to(DEV)             # more rows than candidates: every image has padded rows
    g = torch.Generator().manual_seed(13)
    feats = [torch.randn(ref.N_IMAGES, 8, 2 * ref.MAPS[0][0], 2 * ref.MAPS[0][1], generator=g).to(DEV)] + \
            [torch.randn(ref.N_IMAGES, 8, hh, ww, generator=g).to(DEV) for hh, ww in ref.MAPS]
    with torch.no_grad():
        for p in h.parameters():
            p.copy_((torch.randn(p.shape, generator=g) * 0.15).to(DEV))
        cls, reg = h(feats)
        assert decode_hip_ok(cls, reg, torch.zeros(1, 1, dtype=torch.int64, device=DEV))
        props = h.simple_test_rpn(feats, metas())
        rois = torch.cat([torch.cat([p.new_full((len(p), 1), float(n)), p[:, :4]], dim=1) for n, p in enumerate(props)])
        ext = R.SingleRoIExtractorMod(dict(type='RoIAlign', output_size=7, sampling_ratio=0), 8, list(ref.STRIDES), finest_scale=16, starting_level=1)
        assert R.hip_ok(feats[1:], rois, (7, 7)) and len(rois) > 10
        out = ext(feats, rois)
        assert out.shape == (len(rois), 8, 7, 7) and torch.isfinite(out).all() and out.abs().max() > 0
        padded, counts = h.simple_test_rpn(feats, metas(), padded=True)
        N, P = padded.shape[:2]
        image = torch.arange(N, device=DEV, dtype=torch.float32)[:, None, None].expand(N, P, 1)
        flat = torch.cat([image, padded[..., :4]], dim=-1).reshape(N * P, 5)
        out2 = ext(feats, flat).reshape(N, P, 8, 7, 7)
        first = 0
        for n, k in enumerate(counts.tolist()):
            assert k < P and torch.equal(out2[n, :k], out[first:first + k]) and (out2[n, k:] == 0).all()
            first += k
