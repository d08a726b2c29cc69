"""The 2-D detector's training side without a GPU: the restatements against the numpy rule (tests/detector_train_ref.py),
the margins the rule claims, the delta bound's constant, the sampler on recorded keys, the two losses' closed forms, ``resolve``, the heads'
keys, ``get_targets`` / ``loss`` of both heads against a plain composition of the rule, the loader's row and the argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import detector_train_ref as ref
from monorun_amd import assigners as A
from monorun_amd import detection_losses as DL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ref.exact_cases()
DELTA_RATIO = 1.01          # measured on the CPU: max |fp32 restatement − fp64| / (2^-23 · terms) over delta_cases() and three coders
DELTA_C = 4 * DELTA_RATIO   # the bound of every implementation: another log, another division, another order


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def bits_equal(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if want.dtype == np.float32:
        return got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    return got.shape == want.shape and np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ the assignment
@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_restatement_equals_the_fp32_rule_bitwise(case):
    name, boxes, gts, labels, ignore, present, rule = case
    want = ref.run_case(case)
    got = A.assign_torch(_t(boxes), _t(gts), _t(ignore), _t(labels), _t(present), **rule)
    for k in ('gt_ind', 'label', 'max_overlap', 'gt_max', 'argmax', 'ignored'):
        assert bits_equal(got[k].numpy(), want[k]), (name, k)
    # through the public entries: on CPU tensors they run the restatement
    assigner = A.MaxIoUAssigner(**rule)
    batch = assigner.assign_batch(_t(boxes)[None], [_t(gts)], [_t(ignore)], [_t(labels)], valid=None if present is None else _t(present)[None])
    assert bits_equal(batch.gt_inds[0].numpy(), want['gt_ind']) and bits_equal(batch.labels[0].numpy(), want['label'])
    assert bits_equal(batch.max_overlaps[0].numpy(), want['max_overlap']) and bits_equal(batch.gt_max[0].numpy(), want['gt_max'])
    if present is None:
        one = assigner.assign(_t(boxes), _t(gts), _t(ignore), _t(labels))
        assert one.num_gts == len(gts) and bits_equal(one.gt_inds.numpy(), want['gt_ind']) and bits_equal(one.labels.numpy(), want['label'])
        assert assigner.assign(_t(boxes), _t(gts), _t(ignore)).labels is None


def test_cases_give_what_they_are_built_for():
    """the rule itself on the built cases"""
    out = {c[0]: ref.run_case(c) for c in CASES}
    ties = out['anchors-ties-0']
    boxes, gts = ref.anchors_48x80(), CASES[[c[0] for c in CASES].index('anchors-ties-0')][2]
    ov = ref.overlaps(gts, boxes)
    assert boxes.shape == (945, 4) and max(int((ov[i] == ties['gt_max'][i]).sum()) for i in range(len(gts))) > 1      # gt_max ties: the == step
    assert out['two-claim-one']['gt_ind'].tolist() == [2, 0]                                  # both claim box 0: the later wins
    assert out['iof-at-threshold']['ignored'].tolist() == [False, True, False] and out['iof-at-threshold']['gt_ind'][0] == 1
    assert out['all-ignored']['ignored'].all() and (out['all-ignored']['gt_ind'] == -1).all() and (out['all-ignored']['gt_max'] == -1).all()
    assert (out['below-min-pos']['gt_ind'] != 4).all() and 0 <= out['below-min-pos']['gt_max'][3] < 0.3
    assert (out['G0']['gt_ind'] == 0).all() and (out['G0']['max_overlap'] == 0).all()
    assert (out['counts-stride5']['gt_ind'][77:] == -1).all() and (out['counts-stride5']['max_overlap'][77:] == 0).all()
    assert (out['no-low-quality']['gt_ind'] > 0).sum() < (out['anchors-ties-0']['gt_ind'] > 0).sum()
    odd = out['nan-inf-zero-area']
    assert odd['gt_ind'][3] == -1 and odd['max_overlap'][3] == -1 and not np.isnan(odd['max_overlap']).any() and odd['gt_max'][1] == -1
    assert out['ignore1']['ignored'].sum() == 1 and out['ignore65']['ignored'].sum() > 1 and not out['ignore0']['ignored'].any()
    sym = out['symmetric']
    assert (sym['gt_ind'] == 1).sum() >= 2 and (sym['gt_ind'] == 2).sum() >= 2 and sym['gt_max'][0] == np.float32(400) / np.float32(1024)     # both anchors


@pytest.mark.parametrize('seed', ref.MARGIN_SEEDS)
def test_fp32_rule_equals_fp64_rule_where_the_margins_hold(seed):
    """an fp32 IoU carries about eight roundings, under 1e-6: where every fp64 IoU is farther than 1e-5 from the thresholds, and every best
    from its second best, both precisions decide alike; the margins are asserted on the reference itself"""
    b, g = ref.margin_case(seed)
    m = ref.margins(b, g)
    print(f'seed {seed}: margins {m[0]:.3g} / {m[1]:.3g} / {m[2]:.3g}')
    assert min(m) > 1e-5
    for thr in ref.THRESHOLDS:
        a32, a64 = ref.assign(b, g, **thr), ref.assign(b, g, dtype=np.float64, **thr)
        assert np.array_equal(a32['gt_ind'], a64['gt_ind']) and np.array_equal(a32['argmax'], a64['argmax'])
        got = A.assign_torch(_t(b), _t(g), **thr)
        assert np.array_equal(got['gt_ind'].numpy(), a64['gt_ind'])


def test_gt_max_assign_all_false_gives_each_ground_truth_its_first_best_box():
    case = CASES[[c[0] for c in CASES].index('anchors-ties-0')]
    _, boxes, gts, labels, _, _, rule = case
    every = A.assign_torch(_t(boxes), _t(gts), **rule)['gt_ind'].numpy()
    first = A.assign_torch(_t(boxes), _t(gts), gt_max_assign_all=False, **rule)['gt_ind'].numpy()
    want = ref.run_case(case, match_low_quality=False)['gt_ind'].copy()
    ov, full = ref.overlaps(gts, boxes), ref.run_case(case)
    for i in range(len(gts)):
        if full['gt_max'][i] >= np.float32(rule['min_pos_iou']):
            want[np.nonzero(ov[i] == full['gt_max'][i])[0][0]] = i + 1
    assert np.array_equal(first, want) and (first > 0).sum() < (every > 0).sum()
    got = A.MaxIoUAssigner(gt_max_assign_all=False, **rule).assign(_t(boxes), _t(gts))
    assert np.array_equal(got.gt_inds.numpy(), want)


def test_bbox_overlaps_and_bbox2delta_equal_the_rule():
    r = np.random.default_rng(5)
    a, b = ref.rb(r, 40), ref.rb(r, 30)
    for mode in ('iou', 'iof'):
        assert bits_equal(A.bbox_overlaps(_t(a), _t(b), mode=mode).numpy(), ref.overlaps(a, b, mode=mode))
        assert bits_equal(A.bbox_overlaps(_t(a[:30]), _t(b), mode=mode, is_aligned=True).numpy(),
                          np.ascontiguousarray(np.diagonal(ref.overlaps(a[:30], b, mode=mode))))
        got64 = A.bbox_overlaps(_t(a.astype(np.float64)), _t(b.astype(np.float64)), mode=mode).numpy()
        assert got64.dtype == np.float64 and np.array_equal(got64, ref.overlaps(a, b, mode=mode, dtype=np.float64))
    assert A.bbox_overlaps(_t(a), _t(b[:0])).shape == (40, 0)
    tiny = np.array([[1, 1, 1, 1]], dtype=np.float32)
    assert A.bbox_overlaps(_t(tiny), _t(tiny)).item() == 0.0                                   # eps keeps 0 / 0 away
    with pytest.raises(AssertionError):
        A.bbox_overlaps(_t(a), _t(b), mode='giou')


def test_delta_bound_constant():
    """|fp32 − fp64| <= c 2^-23 (sum of the magnitudes of the terms): the ratio of the fp32 torch restatement is recomputed here, c is four
    times the recorded one"""
    p, g = ref.delta_cases()
    assert ((p[:50, 2] - p[:50, 0]) == 1).all() and np.allclose((g[50:100, 2] - g[50:100, 0]) / (p[50:100, 2] - p[50:100, 0]), 16, rtol=1e-4)
    assert np.allclose((g[100:150, 2] - g[100:150, 0]) / (p[100:150, 2] - p[100:150, 0]), 1 / 16, rtol=1e-3)
    worst = 0.0
    for means, stds in (((0, 0, 0, 0), (1, 1, 1, 1)), ((0, 0, 0, 0), ref.RCNN_STDS), ((0.1, -0.2, 0.3, 0.05), ref.RCNN_STDS)):
        want, terms = ref.bbox2delta(p, g, means, stds, dtype=np.float64), ref.delta_bound_terms(p, g, means, stds)
        got = A.bbox2delta(_t(p), _t(g), means, stds).numpy()
        assert got.dtype == np.float32
        worst = max(worst, float((np.abs(got.astype(np.float64) - want) / (2.0 ** -23 * terms)).max()))
    print(f'delta ratio of the fp32 restatement: {worst:.3f} (recorded {DELTA_RATIO}, c = {DELTA_C})')
    assert worst <= DELTA_C
    # the deltas the assignment writes are the coder's on the positives, 0 elsewhere
    case = CASES[[c[0] for c in CASES].index('random-0')]
    got = A.assign_torch(_t(case[1]), _t(case[2]), means=(0, 0, 0, 0), stds=ref.RCNN_STDS, **case[6])
    want = ref.run_case(case, stds=ref.RCNN_STDS, dtype=np.float64)
    pos = want['gt_ind'] > 0
    terms = ref.delta_bound_terms(case[1][pos], case[2][want['gt_ind'][pos] - 1], stds=ref.RCNN_STDS)
    assert pos.any() and (np.abs(got['deltas'].numpy()[pos] - want['deltas'][pos]) <= DELTA_C * 2.0 ** -23 * terms).all()
    assert (got['deltas'].numpy()[~pos] == 0).all()


def test_assigner_arguments():
    with pytest.raises(NotImplementedError):
        A.MaxIoUAssigner(0.7, (0.1, 0.3))
    with pytest.raises(NotImplementedError):
        A.MaxIoUAssigner(0.7, 0.3, gpu_assign_thr=100)
    with pytest.raises(NotImplementedError):
        A.MaxIoUAssigner(0.7, 0.3, iou_calculator=dict(type='BboxOverlaps3D'))
    with pytest.raises(NotImplementedError):
        A.build_assigner(dict(type='ATSSAssigner', topk=9))
    with pytest.raises(NotImplementedError):
        A.build_sampler(dict(type='OHEMSampler', num=4, pos_fraction=0.5))
    a = A.build_assigner(dict(type='MaxIoUAssigner', pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3, match_low_quality=True, ignore_iof_thr=0.5))
    assert isinstance(a, A.MaxIoUAssigner) and a.gt_max_assign_all and a.ignore_iof_thr == 0.5 and A.build_assigner(a) is a
    s = A.build_sampler(dict(type='RandomSampler', num=256, pos_fraction=0.5, neg_pos_ub=-1, add_gt_as_proposals=False), context=object())
    assert isinstance(s, A.RandomSampler) and s.num == 256 and not s.add_gt_as_proposals
    boxes = torch.zeros(4, 4)
    assert not a.hip_ok(boxes, [boxes]) and not a.hip_ok(boxes.double(), [boxes])              # CPU tensors: the restatement
    with pytest.raises(AssertionError):
        a.assign_batch(torch.zeros(2, 4, 3), [boxes, boxes])
    with pytest.raises(AssertionError):
        a.assign_batch(torch.zeros(2, 4, 4), [boxes])
    with pytest.raises(AssertionError):
        a.assign_batch(torch.zeros(2, 4, 4), [boxes, boxes], valid=torch.ones(2, 5))
    big = a.assign(_t(ref.rb(np.random.default_rng(1), 20)), _t(ref.rb(np.random.default_rng(2), 257)))     # above the cap: the restatement
    assert big.num_gts == 257 and big.gt_inds.shape == (20,)


def test_batch_of_three_images_with_an_empty_one():
    boxes, gts, labels, rule = ref.batch_case()
    got = A.MaxIoUAssigner(**rule).assign_batch(_t(boxes), [_t(g) for g in gts], None, [_t(l) for l in labels])
    shared = A.MaxIoUAssigner(**rule).assign_batch(_t(boxes[0]), [_t(g) for g in gts], None, [_t(l) for l in labels])
    assert got.num_gts == [5, 0, 9] and got.gt_inds.shape == (3, 150)
    for n in range(3):
        want = ref.assign(boxes[n], gts[n], labels[n], **rule)
        for k, v in (('gt_ind', got.gt_inds), ('label', got.labels), ('max_overlap', got.max_overlaps), ('gt_max', got.gt_max)):
            assert bits_equal(v[n].numpy(), want[k]), (n, k)
        assert bits_equal(shared.gt_inds[n].numpy(), ref.assign(boxes[0], gts[n], labels[n], **rule)['gt_ind'])
    assert (got.gt_inds[1] == 0).all()


# ------------------------------------------------------------------------------------------------ the sampler
def _sampler_case(seed, B=60, G=4, pos=10, tie=False):
    r = np.random.default_rng(seed)
    gt_ind = np.zeros(B, dtype=np.int64)
    gt_ind[r.permutation(B)[:pos]] = r.integers(1, G + 1, pos) if G else 0
    gt_ind[r.permutation(B)[:5]] = -1
    keys = r.uniform(size=G + B).astype(np.float32)
    if tie:
        keys = (np.floor(keys * 4) / 4).astype(np.float32)
    return gt_ind, keys


@pytest.mark.parametrize('pos', [3, 8, 9, 20])                                 # int(16 · 0.5) = 8: below, at and above
@pytest.mark.parametrize('ub', [-1, 0, 3])
@pytest.mark.parametrize('tie', [False, True])
def test_sampler_equals_the_rule_on_recorded_keys(pos, ub, tie):
    gt_ind, keys = _sampler_case(100 + pos, pos=pos, tie=tie)
    sampler = A.RandomSampler(num=16, pos_fraction=0.5, neg_pos_ub=ub, add_gt_as_proposals=False)
    want_pos, want_neg = ref.sample(gt_ind, keys[4:], 16, 0.5, ub)
    boxes = _t(ref.rb(np.random.default_rng(3), 60))
    gts = _t(ref.rb(np.random.default_rng(4), 4))
    res = sampler.sample(A.AssignResult(4, _t(gt_ind), torch.zeros(60), _t(np.maximum(gt_ind - 1, -1))), boxes, gts, keys=_t(keys[4:]))
    assert np.array_equal(res.pos_inds.numpy(), want_pos) and np.array_equal(res.neg_inds.numpy(), want_neg)
    assert len(want_pos) == min((gt_ind > 0).sum(), 8) and (ub != 0 or len(want_neg) == 0) and (ub != 3 or len(want_neg) <= 3 * max(1, len(want_pos)))
    assert torch.equal(res.pos_bboxes, boxes[res.pos_inds]) and torch.equal(res.bboxes, torch.cat((boxes[res.pos_inds], boxes[res.neg_inds])))
    assert torch.equal(res.pos_assigned_gt_inds, _t(gt_ind)[res.pos_inds] - 1) and torch.equal(res.pos_gt_bboxes, gts[res.pos_assigned_gt_inds])
    assert not res.pos_is_gt.any() and res.num_gts == 4
    res.bboxes, res.pos_bboxes = res.bboxes[:1], res.pos_bboxes[:1]            # assignable, as the reference's forward_train assigns them


def test_sampler_short_of_negatives_and_added_ground_truths():
    gt_ind, keys = _sampler_case(7, B=12, pos=9)
    want_pos, want_neg = ref.sample(gt_ind, keys[4:], 16, 0.5)
    assert len(want_pos) <= 8 and len(want_neg) == (gt_ind == 0).sum() < 16 - len(want_pos)          # every negative, still short
    boxes, gts, labels = _t(ref.rb(np.random.default_rng(3), 12)), _t(ref.rb(np.random.default_rng(4), 4)), torch.tensor([2, 0, 1, 1])
    plain = A.RandomSampler(16, 0.5, add_gt_as_proposals=False).sample(A.AssignResult(4, _t(gt_ind), torch.zeros(12)), boxes, gts, keys=_t(keys[4:]))
    assert np.array_equal(plain.pos_inds.numpy(), want_pos) and np.array_equal(plain.neg_inds.numpy(), want_neg) and plain.pos_gt_labels is None
    # with the ground truths prepended: gt_ind 1..G, overlap 1, their labels, pos_is_gt
    full = np.concatenate((np.arange(1, 5), gt_ind))
    want_pos, want_neg = ref.sample(full, keys, 16, 0.5)
    a = A.AssignResult(4, _t(gt_ind), torch.zeros(12), torch.zeros(12, dtype=torch.int64))
    res = A.RandomSampler(16, 0.5, add_gt_as_proposals=True).sample(a, boxes, gts, labels, keys=_t(keys))
    assert np.array_equal(res.pos_inds.numpy(), want_pos) and np.array_equal(res.neg_inds.numpy(), want_neg)
    assert a.gt_inds[:4].tolist() == [1, 2, 3, 4] and a.max_overlaps[:4].tolist() == [1.0] * 4 and a.labels[:4].tolist() == [2, 0, 1, 1]
    assert res.pos_is_gt.tolist() == [int(i < 4) for i in want_pos] and torch.equal(res.pos_bboxes, torch.cat((gts, boxes))[res.pos_inds])
    with pytest.raises(ValueError):
        A.RandomSampler(16, 0.5).sample(A.AssignResult(4, _t(gt_ind), torch.zeros(12)), boxes, gts)
    # G = 0: nothing is prepended
    none = A.RandomSampler(16, 0.5, add_gt_as_proposals=True).sample(A.AssignResult(0, torch.zeros(12, dtype=torch.int64), torch.zeros(12)), boxes,
                                                                     gts[:0], labels[:0], keys=_t(keys[4:]))
    assert none.pos_inds.numel() == 0 and none.neg_inds.numel() == 12 and none.pos_gt_bboxes.shape == (0, 4)


@pytest.mark.parametrize('add_gt', [False, True])
def test_batch_sampler_equals_the_rule_and_the_list_form(add_gt):
    """N = 3, a G = 0 image in the middle: the masks and the padded ascending index lists against the rule per image; the list form is the
    padded form cut at its counts"""
    boxes, gts, labels, rule = ref.batch_case()
    tb, tg, tl = _t(boxes), [_t(g) for g in gts], [_t(l) for l in labels]
    result = A.MaxIoUAssigner(**dict(ref.THRESHOLDS[1], min_pos_iou=0.2, neg_iou_thr=0.2)).assign_batch(tb, tg, None, tl)
    sampler = A.RandomSampler(num=32, pos_fraction=0.25, add_gt_as_proposals=add_gt)
    Gm = 9 if add_gt else 0
    keys = np.random.default_rng(9).uniform(size=(3, Gm + 150)).astype(np.float32)
    keys[0, 20:40] = keys[0, 20]                                               # tied keys
    s = sampler.sample_batch(result, tb, tg, tl, keys=_t(keys))
    per_image = A.split_sampling(s)
    for n in range(3):
        G = len(gts[n]) if add_gt else 0
        ind = np.concatenate((np.arange(1, G + 1), result.gt_inds[n].numpy()))
        k = np.concatenate((keys[n, :G], keys[n, Gm:]))
        want_pos, want_neg = ref.sample(ind, k, 32, 0.25)
        back = lambda idx: np.where(idx >= G, idx + (Gm - G), idx)             # the image's own rows in the padded layout
        npos, nneg = int(s.num_pos[n]), int(s.num_neg[n])
        assert np.array_equal(s.pos_inds[n, :npos].numpy(), back(want_pos)) and (s.pos_inds[n, npos:] == -1).all()
        assert np.array_equal(s.neg_inds[n, :nneg].numpy(), back(want_neg)) and (s.neg_inds[n, nneg:] == -1).all()
        assert np.array_equal(np.nonzero(s.pos_mask[n].numpy())[0], back(want_pos))
        res = per_image[n]
        assert np.array_equal(res.pos_inds.numpy(), want_pos) and np.array_equal(res.neg_inds.numpy(), want_neg)
        assert res.num_gts == len(gts[n]) and torch.equal(res.pos_gt_bboxes, tg[n][res.pos_assigned_gt_inds])
        assert torch.equal(res.pos_gt_labels, tl[n][res.pos_assigned_gt_inds])
        assert res.pos_is_gt.tolist() == [int(i < G) for i in want_pos]
        own = A.RandomSampler(num=32, pos_fraction=0.25, add_gt_as_proposals=add_gt).sample(
            result.image(n), tb[n], tg[n], tl[n], keys=_t(k))
        assert torch.equal(own.pos_inds, res.pos_inds) and torch.equal(own.neg_inds, res.neg_inds) and torch.equal(own.bboxes, res.bboxes)
    g = torch.Generator().manual_seed(3)
    drawn = sampler.sample_batch(result, tb, tg, tl, generator=g)
    again = sampler.sample_batch(result, tb, tg, tl, generator=torch.Generator().manual_seed(3))
    assert torch.equal(drawn.pos_inds, again.pos_inds) and torch.equal(drawn.keys, again.keys) and drawn.keys.shape == (3, Gm + 150)


# ------------------------------------------------------------------------------------------------ the losses
def test_loss_closed_forms():
    loss = DL.SmoothL1Loss(beta=0.5, loss_weight=2.0)
    pred, target = torch.tensor([[0.0, 0.25, 0.5, 3.0]]), torch.zeros(1, 4)
    assert torch.allclose(DL.smooth_l1_loss(pred, target, 0.5), torch.tensor([[0.0, 0.0625, 0.25, 2.75]]))       # 0.5 d² / β below β, d − 0.5 β above
    assert torch.allclose(loss(pred, target), torch.tensor(2.0 * (0.0625 + 0.25 + 2.75) / 4))
    w = torch.tensor([[1.0, 0.0, 1.0, 2.0]])
    assert torch.allclose(loss(pred, target, w, avg_factor=torch.tensor(5.0)), torch.tensor(2.0 * (0.25 + 5.5) / 5))
    assert torch.allclose(loss(pred, target, reduction_override='sum'), torch.tensor(2.0 * 3.0625))
    assert loss(pred[:0], target[:0]).item() == 0.0
    with pytest.raises(ValueError):
        loss(pred, target, reduction_override='median')
    ce = DL.SoftmaxCrossEntropyLoss(loss_weight=0.5)
    x, y = torch.tensor([[0.0, 0.0, 0.0], [2.0, 0.0, -1.0]]), torch.tensor([1, 0])
    want = torch.stack((torch.log(torch.tensor(3.0)), -(2.0 - torch.log(torch.exp(torch.tensor([2.0, 0.0, -1.0])).sum()))))
    assert torch.allclose(ce(x, y, reduction_override='none'), 0.5 * want)
    assert torch.allclose(ce(x, y, torch.tensor([1.0, 0.0]), avg_factor=2.0), 0.5 * want[0] / 2)
    with pytest.raises(NotImplementedError):
        DL.SoftmaxCrossEntropyLoss(use_sigmoid=True)


def test_resolve_builds_what_an_unbuilt_loss_names_and_leaves_the_rest():
    from monorun_amd import losses
    try:
        import mmdet  # noqa: F401
        pytest.skip('with mmdet build_loss builds these itself')
    except ImportError:
        pass
    unbuilt = losses.build_loss(dict(type='SmoothL1Loss', beta=0.25, loss_weight=3.0))
    assert isinstance(unbuilt, losses.UnbuiltLoss)                             # losses.py is what it was
    with pytest.raises(RuntimeError):
        unbuilt(torch.zeros(1), torch.zeros(1))
    with pytest.raises(NotImplementedError):
        losses.CrossEntropyLoss(use_sigmoid=False)
    got = DL.resolve(unbuilt)
    assert isinstance(got, DL.SmoothL1Loss) and got.beta == 0.25 and got.loss_weight == 3.0 and DL.resolve(unbuilt) is got
    assert isinstance(unbuilt, losses.UnbuiltLoss) and unbuilt.cfg['type'] == 'SmoothL1Loss'
    soft = DL.resolve(losses.UnbuiltLoss(dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0)))
    assert isinstance(soft, DL.SoftmaxCrossEntropyLoss)
    other = losses.UnbuiltLoss(dict(type='NoSuchLoss'))
    assert DL.resolve(other) is other and DL.resolve(None) is None
    sig = losses.CrossEntropyLoss()
    assert DL.resolve(sig) is sig


# ------------------------------------------------------------------------------------------------ the heads
IMG = dict(img_shape=(48, 80, 3), pad_shape=(48, 80, 3), scale_factor=1.0)
RPN_TRAIN = dict(assigner=dict(type='MaxIoUAssigner', pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3, match_low_quality=True, ignore_iof_thr=0.5),
                 sampler=dict(type='RandomSampler', num=64, pos_fraction=0.5, neg_pos_ub=-1, add_gt_as_proposals=False),
                 allowed_border=-1, pos_weight=-1, debug=False)
RCNN_TRAIN = dict(bbox_assigner=dict(type='MaxIoUAssigner', pos_iou_thr=0.6, neg_iou_thr=0.6, min_pos_iou=0.6, match_low_quality=True,
                                     ignore_iof_thr=0.6),
                  bbox_sampler=dict(type='RandomSampler', num=64, pos_fraction=0.25, neg_pos_ub=-1, add_gt_as_proposals=True), pos_weight=-1)
GTS = [np.array([[8, 8, 72, 40], [20, 10, 44, 34]], dtype=np.float32), np.array([[30, 4, 62, 44]], dtype=np.float32)]
GT_LABELS = [np.array([1, 0]), np.array([2])]


def make_rpn(device='cpu', **train):
    from monorun_amd.rpn_head import RPNHeadMod
    torch.manual_seed(0)
    head = RPNHeadMod(8, feat_channels=8, anchor_generator=dict(type='AnchorGenerator', scales=[8], ratios=[0.5, 1.0, 2.0], strides=[4, 8, 16]),
                      train_cfg=dict(RPN_TRAIN, **train), test_cfg=dict(nms_pre=200, nms_post=50, nms_thr=0.75, min_bbox_size=0))
    for m in (head.rpn_conv, head.rpn_cls, head.rpn_reg):
        torch.nn.init.normal_(m.weight, std=0.1)
    return head.to(device)


def make_bbox_head(device='cpu'):
    from monorun_amd.bbox_head import Shared2FCBBoxHead
    torch.manual_seed(1)
    head = Shared2FCBBoxHead(in_channels=8, fc_out_channels=16, roi_feat_size=7, num_classes=3,
                             loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0),
                             loss_bbox=dict(type='SmoothL1Loss', beta=1.0, loss_weight=1.0))
    torch.nn.init.normal_(head.fc_reg.weight, std=0.05)
    torch.nn.init.normal_(head.fc_cls.weight, std=0.05)
    return head.to(device)


def rpn_reference_losses(cls_scores, bbox_preds, gts, metas, keys, ignore=None, border=-1):
    """RPNHead.loss composed plainly from the numpy rule, image by image and level by level, in float64 from the fp32 outputs"""
    anchors = ref.anchors_48x80()
    N, B = len(gts), len(anchors)
    labels, lw, bt, bw = np.ones((N, B), dtype=np.int64), np.zeros((N, B)), np.zeros((N, B, 4)), np.zeros((N, B, 4))
    terms = np.zeros((N, B, 4))
    total = 0
    for n in range(N):
        present = None
        if border >= 0:
            h, w = metas[n]['img_shape'][:2]
            present = (anchors[:, 0] >= -border) & (anchors[:, 1] >= -border) & (anchors[:, 2] < w + border) & (anchors[:, 3] < h + border)
        a = ref.assign(anchors, gts[n], None, None if ignore is None else ignore[n], present, ignore_iof_thr=0.5, **ref.THRESHOLDS[0])
        pos, neg = ref.sample(a['gt_ind'], keys[n], 64, 0.5)
        labels[n, pos] = 0
        lw[n, pos], lw[n, neg] = 1, 1
        bt[n, pos] = ref.bbox2delta(anchors[pos], gts[n][a['gt_ind'][pos] - 1], dtype=np.float64)
        terms[n, pos] = ref.delta_bound_terms(anchors[pos], gts[n][a['gt_ind'][pos] - 1])
        bw[n, pos] = 1
        total += max(len(pos), 1) + max(len(neg), 1)
    out_cls, out_bbox, first = [], [], 0
    for c, r in zip(cls_scores, bbox_preds):
        x = c.detach().double().permute(0, 2, 3, 1).reshape(N, -1).numpy()
        d = r.detach().double().permute(0, 2, 3, 1).reshape(N, -1, 4).numpy()
        sl = slice(first, first + x.shape[1])
        first += x.shape[1]
        t = (labels[:, sl] == 0).astype(np.float64)
        bce = np.maximum(x, 0) - x * t + np.log1p(np.exp(-np.abs(x)))
        out_cls.append((bce * lw[:, sl]).sum() / total)
        diff = np.abs(d - bt[:, sl])
        beta = 1.0 / 9.0
        out_bbox.append((np.where(diff < beta, 0.5 * diff * diff / beta, diff - 0.5 * beta) * bw[:, sl]).sum() / total)
    return out_cls, out_bbox, (labels, lw, bt, bw, terms)


@pytest.mark.parametrize('border', [-1, 0])
def test_rpn_get_targets_and_loss_equal_the_composition(border):
    head = make_rpn(allowed_border=border)
    metas = [dict(IMG), dict(IMG, pad_shape=(40, 72, 3), img_shape=(40, 70, 3))]
    feats = [torch.randn(2, 8, 48 // s, 80 // s, generator=torch.Generator().manual_seed(s)) for s in (4, 8, 16)]
    cls_scores, bbox_preds = head(feats)
    keys = np.random.default_rng(11).uniform(size=(2, 945)).astype(np.float32)
    ignore = [np.array([[0, 0, 16, 16]], dtype=np.float32), np.zeros((0, 4), dtype=np.float32)]
    anchors, flags = head.get_anchors([c.shape[-2:] for c in cls_scores], metas, 'cpu')
    assert bits_equal(torch.cat(anchors).numpy(), ref.anchors_48x80()) and flags.shape == (2, 945) and flags[0].all()
    grid = flags[1, :720].reshape(12, 20, 3)
    assert grid[:10, :18].all() and not grid[10:].any() and not grid[:, 18:].any()                  # pad_shape (40, 72) at stride 4
    # the composition knows no pad_shape: compare on the image whose pad_shape is the whole map, both images for the rest
    metas[1] = dict(IMG, img_shape=(40, 70, 3))
    want_cls, want_bbox, (labels, lw, bt, bw, terms) = rpn_reference_losses(cls_scores, bbox_preds, GTS, metas, keys, ignore, border)
    anchors, flags = head.get_anchors([c.shape[-2:] for c in cls_scores], metas, 'cpu')
    got = head.get_targets(anchors, flags, [_t(g) for g in GTS], metas, [_t(i) for i in ignore], keys=_t(keys))
    assert np.array_equal(got[0].numpy(), labels) and np.array_equal(got[1].numpy(), lw) and np.array_equal(got[3].numpy(), bw)
    assert (np.abs(got[2].numpy() - bt) <= DELTA_C * 2.0 ** -23 * terms).all() and (bw.sum() > 0)           # 0 bound, so 0, off the positives
    pos_total = sum(max(int((labels[n] == 0).sum()), 1) for n in range(2))
    assert int(got[4]) == pos_total and int(got[4] + got[5]) == sum(max(int((lw[n] > 0).sum()) - int((labels[n] == 0).sum()), 1) for n in range(2)) + pos_total
    if border == 0:
        outside = (ref.anchors_48x80()[:, 0] < 0) | (ref.anchors_48x80()[:, 3] >= 48)
        assert outside.any() and (lw[0][outside] == 0).all()
    losses = head.loss(cls_scores, bbox_preds, [_t(g) for g in GTS], metas, [_t(i) for i in ignore], keys=_t(keys))
    assert set(losses) == {'loss_rpn_cls', 'loss_rpn_bbox'} and len(losses['loss_rpn_cls']) == len(losses['loss_rpn_bbox']) == 3
    for l in range(3):
        # sums of at most 945 · 2 fp32 terms of magnitude <= the loss: 1e-5 relative is a thousand roundings
        assert abs(losses['loss_rpn_cls'][l].item() - want_cls[l]) <= 1e-5 * abs(want_cls[l]) + 1e-7, l
        assert abs(losses['loss_rpn_bbox'][l].item() - want_bbox[l]) <= 1e-5 * abs(want_bbox[l]) + 1e-7, l
    assert sum(want_bbox) > 0 and sum(want_cls) > 0
    both, proposals = head.forward_train(feats, metas, [_t(g) for g in GTS], proposal_cfg=dict(head.test_cfg), keys=_t(keys))
    assert torch.equal(both['loss_rpn_cls'][0], losses['loss_rpn_cls'][0]) and len(proposals) == 2 and proposals[0].shape[1] == 5
    padded = head.forward_train(feats, metas, [_t(g) for g in GTS], proposal_cfg=dict(head.test_cfg, padded=True), keys=_t(keys))[1]
    assert padded[0].shape == (2, 50, 5) and padded[1].tolist() == [len(p) for p in proposals]
    sum(both['loss_rpn_cls'] + both['loss_rpn_bbox']).backward()
    for m in (head.rpn_conv, head.rpn_cls, head.rpn_reg):
        assert torch.isfinite(m.weight.grad).all() and m.weight.grad.abs().sum() > 0


def rcnn_sampling(device='cpu'):
    """the R-CNN side's assignment and sampling on recorded proposals and keys: (proposals (2, 100, 4), batch result, sampled)"""
    r = np.random.default_rng(21)
    props = np.stack([np.concatenate((ref.rb(r, 90), GTS[n][r.integers(0, len(GTS[n]), 10)] + r.uniform(-2, 2, (10, 4)).astype(np.float32)))
                      for n in range(2)]).astype(np.float32)
    keys = r.uniform(size=(2, 2 + 100)).astype(np.float32)
    assigner, sampler = A.build_assigner(RCNN_TRAIN['bbox_assigner']), A.build_sampler(RCNN_TRAIN['bbox_sampler'])
    tg, tl = [_t(g).to(device) for g in GTS], [_t(l).to(device) for l in GT_LABELS]
    result = assigner.assign_batch(_t(props).to(device), tg, None, tl, means=(0, 0, 0, 0), stds=ref.RCNN_STDS)
    return props, keys, result, sampler.sample_batch(result, _t(props).to(device), tg, tl, keys=_t(keys).to(device)), tg, tl


def bbox_reference(props, keys):
    """Shared2FCBBoxHead.get_targets + loss composed plainly from the numpy rule in float64 -> (targets, losses)"""
    rows = []
    for n in range(2):
        a = ref.assign(props[n], GTS[n], GT_LABELS[n], ignore_iof_thr=0.6, **ref.THRESHOLDS[1])
        G = len(GTS[n])
        ind = np.concatenate((np.arange(1, G + 1), a['gt_ind']))
        boxes = np.concatenate((GTS[n], props[n]))
        pos, neg = ref.sample(ind, np.concatenate((keys[n, :G], keys[n, 2:])), 64, 0.25)
        for i in pos:
            rows.append((n, boxes[i], GT_LABELS[n][ind[i] - 1], 1.0, ref.bbox2delta(boxes[i], GTS[n][ind[i] - 1], stds=ref.RCNN_STDS, dtype=np.float64), 1.0,
                         ref.delta_bound_terms(boxes[i], GTS[n][ind[i] - 1], stds=ref.RCNN_STDS)))
        for i in neg:
            rows.append((n, boxes[i], 3, 1.0, np.zeros(4), 0.0, np.zeros(4)))
    rois = np.array([[n, *b] for n, b, *_ in rows], dtype=np.float32)
    labels, lw = np.array([r[2] for r in rows]), np.array([r[3] for r in rows])
    bt, bw = np.array([r[4] for r in rows]), np.array([r[5] for r in rows])
    return rois, labels, lw, bt, bw, np.array([r[6] for r in rows])


def bbox_reference_losses(cls_score, bbox_pred, labels, lw, bt, bw):
    x, d = cls_score.detach().double().numpy(), bbox_pred.detach().double().numpy()
    lse = np.log(np.exp(x - x.max(1, keepdims=True)).sum(1)) + x.max(1)
    ce = lse - x[np.arange(len(x)), labels]
    rows = max((lw > 0).sum(), 1)
    pos = labels < 3
    own = d.reshape(len(d), 3, 4)[np.arange(len(d)), np.where(pos, labels, 0)]
    diff = np.abs(own - bt)
    l1 = np.where(diff < 1.0, 0.5 * diff * diff, diff - 0.5) * (bw * pos)[:, None]
    acc = 100.0 * ((x.argmax(1) == labels) & (lw > 0)).sum() / rows
    return (ce * lw).sum() / rows, l1.sum() / rows, acc


def test_bbox_head_get_targets_and_loss_equal_the_composition():
    head = make_bbox_head()
    props, keys, result, sampled, tg, tl = rcnn_sampling()
    rois, labels, lw, bt, bw, terms = bbox_reference(props, keys)
    results = A.split_sampling(sampled)
    got = head.get_targets(results, tg, tl, RCNN_TRAIN)
    assert np.array_equal(got[0].numpy(), labels) and np.array_equal(got[1].numpy(), lw) and np.array_equal(got[3].numpy(), np.repeat(bw[:, None], 4, 1))
    pos = bw > 0
    assert pos.sum() >= 3 and (labels == 3).sum() > 0
    assert (np.abs(got[2].numpy() - bt) <= DELTA_C * 2.0 ** -23 * terms).all()                             # 0 bound, so 0, off the positives
    split = head.get_targets(results, tg, tl, RCNN_TRAIN, concat=False)
    assert len(split[0]) == 2 and torch.equal(torch.cat(split[0]), got[0])
    from monorun_amd.bbox_head import bbox2roi
    assert np.array_equal(bbox2roi([r.bboxes for r in results]).numpy(), rois)
    weighted = head.get_targets(results, tg, tl, dict(pos_weight=2.5))
    assert (weighted[1].numpy()[pos] == 2.5).all() and (weighted[1].numpy()[~pos] == 1).all()
    # the padded form: per image `num` rows in ascending index order, weight 0 past the count; the same sums
    prois, plabels, plw, pbt, pbw = head.get_targets(sampled, tg, tl, RCNN_TRAIN)
    assert prois.shape == (128, 5) and int((plw > 0).sum()) == len(rois) and (plabels[plw == 0] == 3).all() and (pbw[plw == 0] == 0).all()
    key = lambda r: tuple(np.round(r, 3))
    assert sorted(map(key, prois[plw > 0].numpy())) == sorted(map(key, rois))
    torch.manual_seed(5)
    feat = torch.randn(len(rois), 8, 7, 7)
    cls_score, bbox_pred = head(feat)
    losses = head.loss(cls_score, bbox_pred, _t(rois), *got)
    want_cls, want_bbox, want_acc = bbox_reference_losses(cls_score, bbox_pred, labels, lw, bt, bw)
    assert set(losses) == {'loss_cls', 'acc', 'loss_bbox'}
    assert abs(losses['loss_cls'].item() - want_cls) <= 1e-5 * want_cls and abs(losses['loss_bbox'].item() - want_bbox) <= 1e-5 * want_bbox + 1e-7
    assert abs(losses['acc'].item() - want_acc) <= 1e-4 and want_bbox > 0
    (losses['loss_cls'] + losses['loss_bbox']).backward()
    assert head.fc_cls.weight.grad.abs().sum() > 0 and head.fc_reg.weight.grad.abs().sum() > 0
    # no positives: loss_bbox is 0 = bbox_pred[pos].sum() and carries no gradient into the sums
    none = head.loss(cls_score, bbox_pred, _t(rois), torch.full_like(got[0], 3), got[1], torch.zeros_like(got[2]), torch.zeros_like(got[3]))
    assert none['loss_bbox'].item() == 0.0
    # the unbuilt attributes are what they were
    from monorun_amd.losses import UnbuiltLoss
    assert isinstance(head.loss_cls, UnbuiltLoss) and isinstance(head.loss_bbox, UnbuiltLoss)


def test_regress_by_class_refine_bboxes_and_accuracy():
    from monorun_amd.bbox_head import accuracy, decode_torch
    head = make_bbox_head()
    rois = torch.tensor([[0, 10.0, 10, 30, 30], [0, 5, 5, 25, 45], [1, 40, 8, 70, 40]])
    pred = torch.randn(3, 12, generator=torch.Generator().manual_seed(2))
    label = torch.tensor([2, 0, 1])
    got = head.regress_by_class(rois, label, pred, IMG)
    own = torch.stack([pred[i, 4 * int(label[i]):4 * int(label[i]) + 4] for i in range(3)])
    want = decode_torch(rois, own, torch.tensor([[48.0, 80.0]] * 3), None, head.target_means, head.target_stds)[:, 0]
    assert torch.equal(got[:, 0], rois[:, 0]) and torch.equal(got[:, 1:], want)
    assert torch.equal(head.regress_by_class(rois[:, 1:], label, pred, IMG), want)
    refined = head.refine_bboxes(rois, label, pred, [torch.tensor([1], dtype=torch.uint8), torch.tensor([0], dtype=torch.uint8)], [IMG, IMG])
    assert refined[0].shape == (1, 4) and torch.equal(refined[0][0], want[1]) and torch.equal(refined[1][0], want[2])
    score = torch.tensor([[3.0, 1, 0], [0, 2, 1], [0, 1, 2], [5, 0, 1]])
    assert accuracy(score, torch.tensor([0, 1, 1, 2])).item() == 50.0
    assert [a.item() for a in accuracy(score, torch.tensor([0, 1, 1, 2]), topk=(1, 2))] == [50.0, 100.0]
    assert accuracy(score, torch.tensor([0, 1, 1, 2]), weight=torch.tensor([True, True, False, False])).item() == 100.0


def test_heads_still_load_mmdet_state_dicts():
    rpn, box = make_rpn(), make_bbox_head()
    assert set(rpn.state_dict()) == {'rpn_conv.weight', 'rpn_conv.bias', 'rpn_cls.weight', 'rpn_cls.bias', 'rpn_reg.weight', 'rpn_reg.bias'}
    assert set(box.state_dict()) == {'shared_fcs.0.weight', 'shared_fcs.0.bias', 'shared_fcs.1.weight', 'shared_fcs.1.bias', 'fc_cls.weight',
                                     'fc_cls.bias', 'fc_reg.weight', 'fc_reg.bias'}
    for h in (rpn, box):
        h.load_state_dict({k: torch.zeros_like(v) for k, v in h.state_dict().items()}, strict=True)
    from monorun_amd.rpn_head import RPNHeadMod
    bare = RPNHeadMod(8, feat_channels=8)
    assert bare.assigner is None
    with pytest.raises(RuntimeError):
        bare.get_targets([torch.zeros(3, 4)], torch.ones(1, 3, dtype=torch.bool), [torch.zeros(0, 4)], [IMG])


# ------------------------------------------------------------------------------------------------ the loader's row
_PINNED = ('mr_assign_workspace_bytes', 'mr_assign_max_iou')
_SCALAR = {'int': ctypes.c_int, 'float': ctypes.c_float, 'double': ctypes.c_double, 'size_t': ctypes.c_size_t, 'int64_t': ctypes.c_int64}


def _declared_prototypes(path):
    """[(return type, name, [arguments])] of a header, by a regex of this file's own (not `_lib.header_prototypes`)."""
    src = re.sub(r'/\*.*?\*/', ' ', open(path).read(), flags=re.S)
    found = re.findall(r'^((?:const\s+)?\w+[\s\*]+)(\w+)\s*\(([^)]*)\)\s*;', src, flags=re.M)
    return [(' '.join(ret.split()), name, [] if args.strip() in ('', 'void') else [' '.join(a.split()) for a in args.split(',')])
            for ret, name, args in found]


def test_loader_binds_the_assign_header(monkeypatch):
    """the row of `_lib.LATER_HEADERS` this subsystem owns (nothing is asserted about the table's other rows): the pinned names are what the
    header declares, in order, and no other header's; the library exports each; restype, argtypes and arg_names are the declared ones; the
    header alone makes the library stale"""
    from monorun_amd import _lib
    key = 'assign'
    assert key in _lib.LATER_HEADERS and key in _lib.all_header_keys() and key not in _lib.header_keys()
    assert not set(_PINNED) & set(_lib.exported_symbols())
    lib, raw = _lib.load(), ctypes.CDLL(_lib.SO)
    assert _lib.exported_symbols(key) == _lib.LATER_HEADERS[key][1] == _PINNED
    assert _lib.header_path(key) == os.path.join(ROOT, 'include', 'monorun_assign.h')
    assert [n for n, _, _ in _lib.header_prototypes(_lib.header_path(key))] == list(_PINNED)
    declared = _declared_prototypes(_lib.header_path(key))
    assert [name for _, name, _ in declared] == list(_PINNED)
    for other in _lib.all_header_keys():
        if other != key:
            assert not set(_PINNED) & set(_lib.exported_symbols(other)), other
            assert not set(_PINNED) & {n for _, n, _ in _declared_prototypes(_lib.header_path(other))}, other
    for ret, name, args in declared:
        assert hasattr(raw, name), f'{name} declared but not exported'
        f = getattr(lib, name)
        names = [re.search(r'\w+$', a).group() for a in args]
        types = [a.replace('const ', '')[:-len(n)].strip() for a, n in zip(args, names)]
        assert len(set(names)) == len(names)
        assert list(_lib.arg_names(name)) == (names[:-1] if names[-1] == 'stream' else names), name
        assert f.restype is _SCALAR[ret], name
        assert list(f.argtypes) == [ctypes.c_void_p if '*' in t else _SCALAR[t] for t in types], name
    assert _lib.arg_names('mr_assign_workspace_bytes') == ('n_images', 'max_gt') and _lib.table_args('mr_assign_max_iou') == ()
    assert len(lib.mr_assign_max_iou.argtypes) == 30
    src = open(_lib.header_path(key)).read()
    assert '#define MR_ASSIGN_MAX_GT 256' in src and '#define MR_ASSIGN_MAX_IGNORE 256' in src
    assert (A.MAX_GT, A.MAX_IGNORE, A.MAX_IMAGES) == (256, 256, 65535)
    assert not _lib._stale()
    so_time, real = os.path.getmtime(_lib.SO), os.path.getmtime
    monkeypatch.setattr(os.path, 'getmtime', lambda f: so_time + 10 if f == _lib.header_path(key) else real(f))
    assert _lib._stale()


def test_workspace_bytes_and_argument_checks_without_a_gpu():
    """every check comes before any HIP call: the codes of monorun_pnp.h (-1 bad argument, -2 unsupported); no boxes: no launch"""
    from monorun_amd import _lib
    lib = _lib.load()
    BAD, UNSUPPORTED = -1, -2
    assert lib.mr_assign_workspace_bytes(3, 256) == 3 * 256 * 4 and lib.mr_assign_workspace_bytes(-1, 4) == 0 and lib.mr_assign_workspace_bytes(2, 0) == 0
    one, f4 = ctypes.c_void_p(16), (ctypes.c_float * 4)(1, 1, 1, 1)      # never dereferenced: every call below is rejected before a launch
    base = dict(boxes=one, image_stride=0, box_stride=4, valid=None, counts=None, n_images=2, n_boxes=10, gt_bboxes=one, gt_offsets=one,
                gt_labels=None, max_gt=4, ignore_bboxes=None, ignore_offsets=None, max_ignore=0, pos_iou_thr=0.7, neg_iou_thr=0.3,
                min_pos_iou=0.3, ignore_iof_thr=-1.0, match_low_quality=1, means=f4, stds=f4, max_overlap=one, argmax=one, ignored=one,
                gt_max=None, gt_ind=one, label=None, deltas=None, workspace=one)

    def call(**over):
        return lib.mr_assign_max_iou(*_lib.pack('mr_assign_max_iou', dict(base, **over)), None)

    assert call(n_images=-1) == BAD and call(n_boxes=-1) == BAD and call(max_gt=-1) == BAD and call(max_ignore=-1) == BAD
    assert call(box_stride=3) == BAD and call(box_stride=6) == BAD and call(image_stride=-1) == BAD and call(image_stride=39) == BAD
    assert call(means=None) == BAD and call(stds=None) == BAD
    for name in ('boxes', 'gt_offsets', 'max_overlap', 'argmax', 'ignored', 'gt_ind', 'gt_bboxes', 'workspace'):
        assert call(**{name: None}) == BAD, name
    assert call(max_ignore=3, ignore_bboxes=one) == BAD and call(max_ignore=3, ignore_offsets=one) == BAD
    assert call(max_gt=257) == UNSUPPORTED and call(max_ignore=257, ignore_bboxes=one, ignore_offsets=one) == UNSUPPORTED
    assert call(n_images=65536) == UNSUPPORTED and call(n_images=65535, n_boxes=1 << 16) == UNSUPPORTED
    assert call(n_images=0, boxes=None, gt_offsets=None) == 0 and call(n_boxes=0, boxes=None, gt_ind=None) == 0
    with pytest.raises(TypeError):
        _lib.pack('mr_assign_max_iou', dict(base), no_such_argument=1)
