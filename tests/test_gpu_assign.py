"""The 2-D detector's training side on the GPU: ``mr_assign_max_iou`` through the C ABI and through ``assign`` /
``assign_batch`` bitwise against the float32 rule of tests/detector_train_ref.py, its deltas against float64 within DELTA_C 2^-23 magnitudes,
both heads' training steps without a host synchronisation against the composition of the rule, and the chain from ``forward_train`` to the
box head's loss and the 3-D heads' targets."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import detector_train_ref as ref
from tests.test_assign_cpu import (DELTA_C, GT_LABELS, GTS, IMG, RCNN_TRAIN, bbox_reference, bbox_reference_losses, bits_equal,
                                   make_bbox_head, make_rpn, rcnn_sampling, rpn_reference_losses)
from monorun_amd import assigners as A

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CASES = ref.exact_cases()
GUARD = 3


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def want32(index):
    """the float32 rule on a case, computed once and shared"""
    out = ref.run_case(CASES[index])
    for v in out.values():
        v.setflags(write=False)
    return out


def guarded(shape, dtype, fill):
    """a buffer of `fill` bytes with GUARD spare elements on both sides -> (whole, the view to hand over)"""
    n = int(np.prod(shape))
    whole = torch.empty(n + 2 * GUARD, dtype=dtype, device=DEV)
    whole.view(torch.uint8).fill_(fill)
    return whole, whole[GUARD:GUARD + n]


def run_abi(boxes, gts, labels, ignore, rule, valid=None, counts=None, image_stride=None, fill=0xFF, means=(0, 0, 0, 0), stds=(1, 1, 1, 1),
            max_gt=None):
    """mr_assign_max_iou on N images: boxes (N, B, 4 or 5) or (B, 4 or 5) with image stride 0; gts, labels, ignore: lists of N arrays ->
    (code, dict of host arrays, guards untouched)"""
    from monorun_amd import _lib
    N = len(gts)
    B, stride = boxes.shape[-2], boxes.shape[-1]
    sizes = [len(g) for g in gts]
    off = lambda s: dev(np.concatenate([[0], np.cumsum(s)]).astype(np.int32))
    d_boxes = dev(boxes.astype(np.float32))
    d_gt = dev(np.concatenate(gts).reshape(-1, 4).astype(np.float32)) if sum(sizes) else torch.zeros(1, 4, device=DEV)
    d_lab = dev(np.concatenate(labels).astype(np.int32)) if labels is not None and sum(sizes) else None
    n_ign = [0 if i is None else len(i) for i in ignore] if ignore is not None else [0] * N
    with_ign = sum(n_ign) > 0
    d_ign = dev(np.concatenate([i for i in ignore if i is not None]).reshape(-1, 4).astype(np.float32)) if with_ign else None
    gt_off, ign_off = off(sizes), off(n_ign) if with_ign else None
    mg = max(sizes, default=0) if max_gt is None else max_gt
    f4 = ctypes.c_float * 4
    bufs = dict(max_overlap=guarded((N, B), torch.float32, fill), argmax=guarded((N, B), torch.int32, fill),
                ignored=guarded((N, B), torch.uint8, fill), gt_max=guarded((max(sum(sizes), 1),), torch.float32, fill),
                gt_ind=guarded((N, B), torch.int32, fill), label=guarded((N, B), torch.int32, fill), deltas=guarded((N, B, 4), torch.float32, fill))
    ws_whole, ws = guarded((max(N * mg, 1),), torch.int32, fill)
    lib = _lib.load()
    code = lib.mr_assign_max_iou(*_lib.pack(
        'mr_assign_max_iou', boxes=d_boxes.data_ptr(), image_stride=(0 if boxes.ndim == 2 else B * stride) if image_stride is None else image_stride,
        box_stride=stride, valid=_lib.ptr(dev(valid)), counts=_lib.ptr(dev(counts)), n_images=N, n_boxes=B, gt_bboxes=d_gt.data_ptr(),
        gt_offsets=gt_off.data_ptr(), gt_labels=_lib.ptr(d_lab), max_gt=mg, ignore_bboxes=_lib.ptr(d_ign), ignore_offsets=_lib.ptr(ign_off),
        max_ignore=max(n_ign), pos_iou_thr=rule['pos_iou_thr'], neg_iou_thr=rule['neg_iou_thr'], min_pos_iou=rule['min_pos_iou'],
        ignore_iof_thr=rule.get('ignore_iof_thr', -1.0), match_low_quality=int(rule.get('match_low_quality', True)),
        means=f4(*means), stds=f4(*stds), workspace=ws.data_ptr(), **{k: v[1].data_ptr() for k, v in bufs.items()}),
        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    byte = lambda t: t.view(torch.uint8).cpu().numpy()
    edge = lambda whole, n: np.concatenate((byte(whole[:GUARD]), byte(whole[GUARD + n:])))
    clean = all((edge(whole, view.numel()) == fill).all() for whole, view in list(bufs.values()) + [(ws_whole, ws)])
    out = {k: view.cpu().numpy() for k, (whole, view) in bufs.items()}
    shape = lambda k, s: out[k].reshape(s)
    return code, dict(max_overlap=shape('max_overlap', (N, B)), argmax=shape('argmax', (N, B)), ignored=shape('ignored', (N, B)),
                      gt_max=out['gt_max'][:sum(sizes)], gt_ind=shape('gt_ind', (N, B)), label=shape('label', (N, B)),
                      deltas=shape('deltas', (N, B, 4))), clean


def abi_inputs(case):
    """a one-image case as run_abi's arguments: `present` goes in as counts where it is a prefix (the stride-5 case), else as valid flags"""
    name, boxes, gts, labels, ignore, present, rule = case
    kw = {}
    if present is not None:
        k = int(present.sum())
        if present[:k].all():
            kw['counts'] = np.array([k], dtype=np.int32)
        else:
            kw['valid'] = present.astype(np.uint8)[None]
    return (boxes[None], [gts], [labels], [ignore], rule), kw


def check(got, want, n=None):
    sel = (lambda a: a) if n is None else (lambda a: a[n])
    assert bits_equal(sel(got['gt_ind']).astype(np.int64), want['gt_ind'])
    assert bits_equal(sel(got['label']).astype(np.int64), want['label'])
    assert bits_equal(sel(got['max_overlap']), want['max_overlap'])
    assert bits_equal(sel(got['argmax']).astype(np.int64), want['argmax']) and bits_equal(sel(got['ignored']).astype(bool), want['ignored'])


@pytest.mark.parametrize('index', range(len(CASES)), ids=[c[0] for c in CASES])
def test_abi_equals_the_fp32_rule_bitwise(index):
    """exact, into 0xFF-prefilled buffers with the spare elements around every output and the workspace untouched, twice bitwise equal"""
    case, want = CASES[index], want32(index)
    args, kw = abi_inputs(case)
    code, got, clean = run_abi(*args, **kw)
    assert code == 0 and clean
    if case[1].shape[0] == 0:
        return                                                      # no boxes: nothing is launched
    check(got, want, 0)
    assert bits_equal(got['gt_max'], want['gt_max'])
    pos = want['gt_ind'] > 0
    assert (got['deltas'][0][~pos] == 0).all()
    pairs = case[1][pos, :4], case[2][want['gt_ind'][pos] - 1]
    with np.errstate(all='ignore'):
        want64, terms = ref.bbox2delta(*pairs, dtype=np.float64), ref.delta_bound_terms(*pairs)
    fine = np.isfinite(want64) & np.isfinite(terms)
    assert (np.abs(got['deltas'][0][pos] - want64)[fine] <= DELTA_C * 2.0 ** -23 * terms[fine]).all()
    code2, again, _ = run_abi(*args, fill=0x00, **kw)
    assert code2 == 0 and all(np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)) for k in got)


@pytest.mark.parametrize('index', range(len(CASES)), ids=[c[0] for c in CASES])
def test_assign_and_assign_batch_equal_the_fp32_rule_bitwise(index):
    name, boxes, gts, labels, ignore, present, rule = CASES[index]
    want = want32(index)
    assigner = A.MaxIoUAssigner(**rule)
    assert assigner.hip_ok(dev(boxes), [dev(gts)], [dev(ignore)])
    kw = {}
    if present is not None and present[:int(present.sum())].all():
        kw['counts'] = dev(np.array([present.sum()], dtype=np.int32))
    elif present is not None:
        kw['valid'] = dev(present)[None]
    batch = assigner.assign_batch(dev(boxes)[None], [dev(gts)], [dev(ignore)], [dev(labels)], **kw)
    assert batch.gt_inds.device.type == 'cuda' and batch.gt_inds.dtype == torch.int64
    assert bits_equal(batch.gt_inds[0].cpu().numpy(), want['gt_ind']) and bits_equal(batch.labels[0].cpu().numpy(), want['label'])
    assert bits_equal(batch.max_overlaps[0].cpu().numpy(), want['max_overlap']) and bits_equal(batch.gt_max[0].cpu().numpy(), want['gt_max'])
    if present is None:
        one = assigner.assign(dev(boxes), dev(gts), dev(ignore), dev(labels))
        assert bits_equal(one.gt_inds.cpu().numpy(), want['gt_ind']) and bits_equal(one.labels.cpu().numpy(), want['label'])
        assert bits_equal(one.max_overlaps.cpu().numpy(), want['max_overlap'])


def test_three_images_one_anchor_set_and_an_empty_image():
    """N = 3 with different G per image and a G = 0 image in the middle; the 945 anchors with image stride 0"""
    boxes, gts, labels, rule = ref.batch_case()
    code, got, clean = run_abi(boxes, gts, labels, None, rule)
    assert code == 0 and clean
    first = 0
    for n in range(3):
        want = ref.assign(boxes[n], gts[n], labels[n], **rule)
        check(got, want, n)
        assert bits_equal(got['gt_max'][first:first + len(gts[n])], want['gt_max'])
        first += len(gts[n])
    anchors = ref.anchors_48x80()
    many = [CASES[[c[0] for c in CASES].index('anchors-ties-0')][2], np.zeros((0, 4), dtype=np.float32), GTS[0]]
    code, got, clean = run_abi(anchors, many, None, None, rule)
    assert code == 0 and clean
    via = A.MaxIoUAssigner(**rule).assign_batch(dev(anchors), [dev(g) for g in many])
    for n in range(3):
        want = ref.assign(anchors, many[n], None, **rule)
        check(got, want, n)
        assert bits_equal(via.gt_inds[n].cpu().numpy(), want['gt_ind']) and bits_equal(via.max_overlaps[n].cpu().numpy(), want['max_overlap'])
    # a wrong host bound cuts the image in both kernels alike: the first two ground truths only
    code, cut, clean = run_abi(boxes[:1], gts[:1], labels[:1], None, rule, max_gt=2)
    assert code == 0 and clean
    check(cut, ref.assign(boxes[0], gts[0][:2], labels[0][:2], **rule), 0)


def test_257_ground_truths_are_unsupported_and_run_the_restatement():
    from monorun_amd import _lib
    r = np.random.default_rng(8)
    boxes, gts = ref.rb(r, 50), ref.rb(r, 257)
    rule = dict(ref.THRESHOLDS[0])
    code, got, clean = run_abi(boxes[None], [gts], None, None, rule)
    assert code == -2 and clean and (got['gt_ind'].view(np.uint8) == 0xFF).all()           # MR_ERR_UNSUPPORTED before any launch
    assigner = A.MaxIoUAssigner(**rule)
    assert not assigner.hip_ok(dev(boxes), [dev(gts)]) and assigner.hip_ok(dev(boxes), [dev(gts[:256])])
    res = assigner.assign(dev(boxes), dev(gts))
    assert res.gt_inds.device.type == 'cuda' and bits_equal(res.gt_inds.cpu().numpy(), ref.assign(boxes, gts, **rule)['gt_ind'])
    assert _lib.load().mr_pnp_last_hip_error() == 0


def test_deltas_within_the_bound():
    """|kernel − fp64| <= DELTA_C 2^-23 (sum of the magnitudes of the terms): 400 images of one box and one ground truth each, every pair
    assigned (pos_iou_thr 0), boxes of 1-px width and ground truths 16x larger and smaller among them"""
    p, g = ref.delta_cases()
    worst = 0.0
    for means, stds in (((0, 0, 0, 0), (1, 1, 1, 1)), ((0, 0, 0, 0), ref.RCNN_STDS), ((0.1, -0.2, 0.3, 0.05), ref.RCNN_STDS)):
        code, got, clean = run_abi(p[:, None, :], [x[None] for x in g], None, None, dict(pos_iou_thr=0.0, neg_iou_thr=0.0, min_pos_iou=0.0),
                                   means=means, stds=stds)
        assert code == 0 and clean and (got['gt_ind'] == 1).all()
        want, terms = ref.bbox2delta(p, g, means, stds, dtype=np.float64), ref.delta_bound_terms(p, g, means, stds)
        ratio = np.abs(got['deltas'][:, 0].astype(np.float64) - want) / (2.0 ** -23 * terms)
        worst = max(worst, float(ratio.max()))
    print(f'delta ratio of the kernel: {worst:.3f} (bound {DELTA_C})')
    assert worst <= DELTA_C


# ------------------------------------------------------------------------------------------------ the heads
class no_sync:
    def __enter__(self):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode('error')

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode('default')


def rpn_step():
    head = make_rpn(DEV)
    metas = [dict(IMG), dict(IMG, img_shape=(40, 70, 3))]
    feats = [torch.randn(2, 8, 48 // s, 80 // s, generator=torch.Generator().manual_seed(s)).to(DEV) for s in (4, 8, 16)]
    keys = np.random.default_rng(11).uniform(size=(2, 945)).astype(np.float32)
    ignore = [np.array([[0, 0, 16, 16]], dtype=np.float32), np.zeros((0, 4), dtype=np.float32)]
    return head, metas, feats, keys, ignore


def test_rpn_forward_train_without_a_synchronisation_equals_the_composition():
    head, metas, feats, keys, ignore = rpn_step()
    gts, ign, k = [dev(g) for g in GTS], [dev(i) for i in ignore], dev(keys)
    head.forward_train(feats, metas, gts, gt_bboxes_ignore=ign, proposal_cfg=dict(head.test_cfg, padded=True), keys=k)      # warm-up: caches, pinned buffers
    with no_sync():
        losses, (proposals, counts) = head.forward_train(feats, metas, gts, gt_bboxes_ignore=ign, proposal_cfg=dict(head.test_cfg, padded=True), keys=k)
        total = sum(losses['loss_rpn_cls'] + losses['loss_rpn_bbox'])
        total.backward()
    assert proposals.shape == (2, 50, 5) and counts.shape == (2,) and int(counts.min()) > 0
    cls_scores, bbox_preds = head(feats)
    want_cls, want_bbox, _ = rpn_reference_losses([c.cpu() for c in cls_scores], [b.cpu() for b in bbox_preds], GTS, metas, keys, ignore)
    for l in range(3):
        # sums of at most 945 · 2 fp32 terms of magnitude <= the loss: 1e-5 relative is a thousand roundings
        assert abs(losses['loss_rpn_cls'][l].item() - want_cls[l]) <= 1e-5 * abs(want_cls[l]) + 1e-7, l
        assert abs(losses['loss_rpn_bbox'][l].item() - want_bbox[l]) <= 1e-5 * abs(want_bbox[l]) + 1e-7, l
    assert sum(want_bbox) > 0
    for m in (head.rpn_conv, head.rpn_cls, head.rpn_reg):
        assert torch.isfinite(m.weight.grad).all() and m.weight.grad.abs().sum() > 0


def test_bbox_head_targets_and_loss_without_a_synchronisation_equal_the_composition():
    head = make_bbox_head(DEV)
    props, keys, result, sampled, tg, tl = rcnn_sampling(DEV)
    assert A.build_assigner(RCNN_TRAIN['bbox_assigner']).hip_ok(dev(props), tg)
    rois, labels, lw, bt, bw, terms = bbox_reference(props, keys)
    torch.manual_seed(5)
    feat = torch.randn(128, 8, 7, 7).to(DEV)
    head.loss(*head(feat), None, *head.get_targets(sampled, tg, tl, RCNN_TRAIN)[1:])                # warm-up
    d_props, d_keys = dev(props), dev(keys)
    assigner, sampler = A.build_assigner(RCNN_TRAIN['bbox_assigner']), A.build_sampler(RCNN_TRAIN['bbox_sampler'])
    with no_sync():
        result = assigner.assign_batch(d_props, tg, None, tl, means=(0, 0, 0, 0), stds=ref.RCNN_STDS)
        sampled = sampler.sample_batch(result, d_props, tg, tl, keys=d_keys)
        prois, plabels, plw, pbt, pbw = head.get_targets(sampled, tg, tl, RCNN_TRAIN)
        cls_score, bbox_pred = head(feat)
        losses = head.loss(cls_score, bbox_pred, prois, plabels, plw, pbt, pbw)
        (losses['loss_cls'] + losses['loss_bbox']).backward()
    live = (plw > 0).cpu().numpy()
    assert live.sum() == len(rois)
    # the padded rows of positive weight are the composition's rows (there: positives first; here: ascending box order)
    key = lambda r: tuple(np.round(r, 3))
    assert sorted(map(key, prois.cpu().numpy()[live])) == sorted(map(key, rois))
    match = {key(r): i for i, r in enumerate(rois)}
    idx = np.array([match[key(r)] for r in prois.cpu().numpy()[live]])
    assert np.array_equal(plabels.cpu().numpy()[live], labels[idx]) and np.array_equal(pbw.cpu().numpy()[live][:, 0], bw[idx])
    assert (np.abs(pbt.cpu().numpy()[live] - bt[idx]) <= DELTA_C * 2.0 ** -23 * terms[idx]).all()
    full = lambda a, fill: np.concatenate((a, np.full((128 - len(a),) + a.shape[1:], fill, dtype=a.dtype)))
    pad = np.concatenate((np.nonzero(live)[0], np.nonzero(~live)[0]))
    want_cls, want_bbox, want_acc = bbox_reference_losses(cls_score.cpu()[pad], bbox_pred.cpu()[pad], full(labels[idx], 3), full(lw[idx], 0.0),
                                                          full(bt[idx], 0.0), full(bw[idx], 0.0))
    assert abs(losses['loss_cls'].item() - want_cls) <= 1e-5 * want_cls and abs(losses['loss_bbox'].item() - want_bbox) <= 1e-5 * want_bbox + 1e-7
    assert abs(losses['acc'].item() - want_acc) <= 1e-4 and want_bbox > 0
    for m in (head.fc_cls, head.fc_reg):
        assert torch.isfinite(m.weight.grad).all() and m.weight.grad.abs().sum() > 0


def test_chain_from_forward_train_to_the_box_head_loss_and_the_3d_targets():
    """forward_train -> padded proposals -> assign_batch with counts and stride 5 -> sample_batch -> RoIs -> SingleRoIExtractorMod -> box
    head -> loss; the sampling results then drive global_head.get_targets and noc_head.get_targets as they are"""
    from monorun_amd import noc_head
    from monorun_amd.bbox_head import bbox2roi
    from monorun_amd.global_head import FCExtractor
    from monorun_amd.roi_extractor import SingleRoIExtractorMod
    head, metas, feats, keys, ignore = rpn_step()
    box_head = make_bbox_head(DEV)
    extractor = SingleRoIExtractorMod(dict(type='RoIAlign', output_size=7, sampling_ratio=0), 8, [4, 8, 16], finest_scale=8)
    gts, labels = [dev(g) for g in GTS], [dev(l) for l in GT_LABELS]
    assigner, sampler = A.build_assigner(RCNN_TRAIN['bbox_assigner']), A.build_sampler(RCNN_TRAIN['bbox_sampler'])
    losses, (proposals, counts) = head.forward_train(feats, metas, gts, proposal_cfg=dict(head.test_cfg, padded=True), keys=dev(keys))
    assert torch.isnan(proposals[0, int(counts[0]):]).all()
    rcnn_keys = dev(np.random.default_rng(4).uniform(size=(2, 52)).astype(np.float32))
    with no_sync():
        result = assigner.assign_batch(proposals, gts, None, labels, counts=counts, means=box_head.target_means, stds=box_head.target_stds)
        sampled = sampler.sample_batch(result, proposals, gts, labels, keys=rcnn_keys)
        rois, *targets = box_head.get_targets(sampled, gts, labels, RCNN_TRAIN)
        cls_score, bbox_pred = box_head(extractor(feats, rois))
        out = box_head.loss(cls_score, bbox_pred, rois, *targets)
        (out['loss_cls'] + out['loss_bbox'] + sum(losses['loss_rpn_cls'] + losses['loss_rpn_bbox'])).backward()
    assert torch.isfinite(out['loss_cls']) and torch.isfinite(out['loss_bbox']) and out['loss_bbox'] > 0 and torch.isfinite(rois).all()
    assert box_head.fc_reg.weight.grad.abs().sum() > 0 and head.rpn_conv.weight.grad.abs().sum() > 0
    for n in range(2):                                              # the rows past the count took part in nothing
        k = int(counts[n])
        want = ref.assign(proposals[n, :k].cpu().numpy(), GTS[n], GT_LABELS[n], ignore_iof_thr=0.6, **ref.THRESHOLDS[1])
        assert bits_equal(result.gt_inds[n, :k].cpu().numpy(), want['gt_ind']) and (result.gt_inds[n, k:] == -1).all()
        assert not sampled.pos_mask[n, 2 + k:].any() and not sampled.neg_mask[n, 2 + k:].any()
    results = A.split_sampling(sampled, counts.tolist())
    assert torch.equal(bbox2roi([r.bboxes for r in results])[:, 1:].sort(0)[0], rois[targets[1] > 0][:, 1:].sort(0)[0])
    npos = sum(len(r.pos_inds) for r in results)
    assert npos >= 3
    dims = [torch.rand(len(g), 7, device=DEV) + 1.0 for g in GTS]
    dim_targets = FCExtractor(in_channels=8, fc_out_channels=16).get_targets(results, dims, labels)
    first = dim_targets[0] if isinstance(dim_targets, (tuple, list)) else dim_targets
    assert first.shape[0] == npos
    coords = [torch.rand(len(g), 3, 48, 80, device=DEV) for g in GTS]
    masks = [torch.ones(len(g), 1, 48, 80, device=DEV) for g in GTS]
    noc_t, noc_w = noc_head.get_targets(results, coords, masks, dims, dict(dense_size=14), [dict(flip=False)] * 2)
    assert noc_t.shape == (npos, 3, 14, 14) and noc_w.shape == (npos, 1, 14, 14) and torch.isfinite(noc_t).all()
