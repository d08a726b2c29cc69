"""The rotated-rectangle intersection (edge_inside_area_t, csrc/kitti_eval_kernel.inc) on coincident, touching and nearly coincident
edges, through each of its three consumers on the MI355X: the KITTI evaluator's overlaps and curves, the aligned 3-D IoU and the
rotated-BEV NMS.  The pairs and their expected areas are tests/rotated_overlap_cases.py's (pinned on the CPU by
tests/test_rotated_overlap_cases_cpu.py); every class runs in both argument orders."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iou3d_ref  # noqa: E402
import rotated_overlap_cases as roc  # noqa: E402
from test_consumers import _rand_boxes  # noqa: E402
from test_rotated_overlap_cases_cpu import KNIFE, NMS_SKIPPED, NMS_THRS  # noqa: E402

from monorun_amd import synthetic as syn  # noqa: E402
from oracle import kitti_eval as ke  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------- evaluator -----
@pytest.mark.parametrize('name', roc.NAMES)
def test_evaluator_overlaps(name):
    """One image per pair: the label is the routine's first box, the detection its second.  Equal heights and bottoms, so metric 2
    is the BEV area composed as the oracle's overlaps_one_image composes it."""
    from monorun_amd import evaluation as ev
    c = roc.classes()[name]
    gts, dts = roc.annos(c.a), roc.annos(c.b)
    for metric in (1, 2):
        blocks, _, n_rows, n_cols = ev.calculate_iou_partly(dts, gts, metric)
        assert [b.shape for b in blocks] == [(1, 1)] * roc.SIZE and n_rows.tolist() == [1] * roc.SIZE and n_cols.tolist() == [1] * roc.SIZE
        got = np.array([b[0, 0] for b in blocks])
        orc = np.array([ke.overlaps_one_image(dts[i], gts[i], metric)[0, 0] for i in range(roc.SIZE)])
        print(f'{name} metric {metric}: max |kernel - oracle| {np.abs(got - orc).max():.3e}, kernel in [{got.min():.9g}, {got.max():.9g}]')
        assert np.abs(got - orc).max() <= 1e-6, (metric, np.abs(got - orc).max(), int(np.abs(got - orc).argmax()))
        if c.kind == 'identical':
            assert np.abs(got - 1).max() <= 1e-6, (metric, got.min(), got.max())
        elif c.kind == 'touching':
            assert np.array_equal(got, np.zeros(roc.SIZE)), (metric, got.max())


def test_evaluator_curves_on_perfect_detections():
    """The labels themselves as detections (the construction of test_kitti_eval.py::test_perfect_detections_have_unit_precision): every
    matched pair is a pair of identical boxes.  The curves equal the oracle's and have its unit-precision properties."""
    from monorun_amd import evaluation as ev
    gts, _ = syn.make_kitti_annos(n_img=12, seed=3)
    dts = []
    for g in gts:
        keep = np.array([n in ('Car', 'Pedestrian', 'Cyclist') for n in g['name']], bool)
        d = {k: (v[keep].copy() if isinstance(v, np.ndarray) else v) for k, v in g.items()}
        d['score'] = np.linspace(0.9, 0.5, keep.sum()).astype(np.float32)
        dts.append(d)
    mo = ke.KITTI_MIN_OVERLAPS[:, :, [0, 1, 2]]
    for metric in (0, 1, 2):
        r = ev.eval_class(gts, dts, [0, 1, 2], [0, 1, 2], metric, mo, compute_aos=(metric == 0))
        want = ke.eval_class(gts, dts, [0, 1, 2], [0, 1, 2], metric, mo, compute_aos=(metric == 0))
        p = r['precision']
        print(f'metric {metric}: precision == 1 at {(p == 1).sum()} samples (oracle {(want["precision"] == 1).sum()}), max recall {np.nanmax(r["recall"])}')
        for k in ('precision', 'recall', 'orientation'):
            np.testing.assert_allclose(r[k], want[k], rtol=0, atol=1e-12, equal_nan=True, err_msg=f'{metric} {k}')
        assert np.all((p == 0) | (p == 1) | np.isnan(p)) and (p == 1).sum() > 20
        assert np.nanmax(r['recall']) == 1.0
        if metric == 0:
            o = r['orientation']
            assert np.all((o == 0) | (np.abs(o - 1) < 1e-12) | np.isnan(o))


# ------------------------------------------------------------------------------- 3-D IoU -------
@pytest.mark.parametrize('name', roc.NAMES)
def test_iou3d_bev_area(name):
    from monorun_amd.iou3d import bbox3d_overlaps_aligned
    c = roc.classes()[name]
    b, q = roc.rows7(c.a), roc.rows7(c.b)
    iou, rinc = bbox3d_overlaps_aligned(torch.from_numpy(b).to(_dev()), torch.from_numpy(q).to(_dev()), return_rinc=True)
    iou, rinc = iou.cpu().numpy()[:, 0], rinc.cpu().numpy()
    amin = np.minimum(roc.box_area(c.a), roc.box_area(c.b))
    err = np.abs(rinc - c.area) / np.maximum(1.0, c.area)
    print(f'{name}: max |rinc - area| / max(1, area) {err.max():.3e}, max rinc / min area {(rinc / np.maximum(amin, 1e-30)).max():.3e}')
    if c.kind == 'loose':
        assert np.all(rinc <= roc.LOOSE * amin), (rinc / amin).max()
    else:
        assert err.max() <= 2e-5, (err.max(), int(err.argmax()))
    if c.kind == 'touching':
        assert np.array_equal(rinc, np.zeros(roc.SIZE, np.float32)), rinc.max()
    elif c.kind == 'identical':
        np.testing.assert_allclose(rinc, c.area, rtol=1e-6)
    assert np.array_equal(iou, iou3d_ref.compose(b, q, rinc, -1, 1.0))


# ------------------------------------------------------------------------------- NMS -----------
@pytest.mark.parametrize('thr', NMS_THRS)
@pytest.mark.parametrize('name', roc.NAMES)
def test_nms_pairs(name, thr):
    """Every pair as a group of two, the routine's first box with the higher score; the whole class in one launch.  A pair whose
    expected IoU lies within KNIFE of thr is not judged: tests/test_rotated_overlap_cases_cpu.py counts them per class (NMS_SKIPPED:
    none with these seeds)."""
    from monorun_amd.consumers import nms_bev
    c = roc.classes()[name]
    iou = roc.expected_iou(c)
    xa, xb = roc.xyxyr(c.a), roc.xyxyr(c.b)
    groups = [torch.from_numpy(np.stack([xa[i], xb[i]])).to(_dev()) for i in range(roc.SIZE)]
    scores = [torch.tensor([0.9, 0.4], device=_dev())] * roc.SIZE
    out = [k.cpu().tolist() for k in nms_bev(groups, scores, thr)]
    judged = np.abs(iou - thr) >= KNIFE
    assert int((~judged).sum()) <= NMS_SKIPPED.get(name, 0)
    wrong = [i for i in range(roc.SIZE) if judged[i] and out[i] != ([0] if iou[i] > thr else [0, 1])]
    print(f'{name} thr {thr}: {len(wrong)} of {int(judged.sum())} judged pairs wrong, {int((~judged).sum())} skipped')
    assert not wrong, [(i, out[i], float(iou[i])) for i in wrong[:8]]
    if c.kind == 'identical':
        assert out == [[0]] * roc.SIZE
    elif c.kind in ('touching', 'loose'):
        assert out == [[0, 1]] * roc.SIZE


@pytest.mark.parametrize('thr', NMS_THRS)
def test_nms_full_group_of_identical_pairs(thr):
    """kNmsMax = 512 boxes in one group: 256 positions far apart, two identical boxes at a random angle on each, distinct random
    scores.  The higher-scored box of every pair survives, in score order: all 16 words of the suppression mask are in use."""
    from monorun_amd.consumers import nms_bev
    rng = np.random.default_rng(41)
    one = roc._boxes(rng, 256, spread=0.0)
    gx, gy = np.meshgrid(np.arange(16), np.arange(16))
    one[:, 0], one[:, 1] = 8.0 * gx.reshape(-1) - 60, 8.0 * gy.reshape(-1) - 60           # 8 apart: the diagonals reach 3.2 at most
    boxes = roc.xyxyr(np.concatenate([one, one]).astype(np.float32))[rng.permutation(512)]
    scores = rng.permutation(512).astype(np.float32) / 512
    keep, = nms_bev([torch.from_numpy(boxes).to(_dev())], [torch.from_numpy(scores).to(_dev())], thr)
    keep = keep.cpu().numpy()
    pos = {}
    for i in np.argsort(-scores, kind='stable'):
        pos.setdefault(boxes[i].tobytes(), i)
    want = np.array(sorted(pos.values(), key=lambda i: -scores[i]))
    assert len(want) == 256
    print(f'thr {thr}: {len(keep)} kept')
    assert np.array_equal(keep, want)


NMS_BOUNDARY_SEED = 43


def nms_boundary_groups(seed=None):
    """the groups of test_nms_group_sizes_at_word_and_padding_boundaries.  No pair of them has an fp64 IoU within KNIFE of a threshold
    of NMS_THRS (tests/test_nms_bev_cases_cpu.py asserts it for this seed)."""
    rng = np.random.default_rng(NMS_BOUNDARY_SEED if seed is None else seed)
    groups = [_rand_boxes(rng, 33, spread=5.0), _rand_boxes(rng, 257, spread=30.0)]
    scores = [rng.uniform(0, 1, len(g)).astype(np.float32) for g in groups]
    return groups, scores


@pytest.mark.parametrize('thr', NMS_THRS)
def test_nms_group_sizes_at_word_and_padding_boundaries(orc, thr):
    """33 boxes (one bit into the second mask word, padded to 64 for the sort) and 257 (padded to 512), against the oracle's NMS as
    test_consumers.py::test_gpu_nms_matches_oracle checks its groups."""
    from monorun_amd.consumers import nms_bev
    groups, scores = nms_boundary_groups()
    out = nms_bev([torch.from_numpy(g).to(_dev()) for g in groups], [torch.from_numpy(s).to(_dev()) for s in scores], thr)
    for g, s, k in zip(groups, scores, out):
        ref = orc.nms_bev(g, s, thr)
        assert 1 < len(ref) < len(g)
        assert np.array_equal(k.cpu().numpy(), ref)                               # no knife edge in these groups: equality
