"""The proposal stage without a GPU: the restatements against the numpy definitions (tests/proposals_ref.py), the margins
the definitions claim, the decode tolerance constants, the anchors, the head's keys, the loader's row and the argument checks."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import proposals_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c['name']: c for c in ref.nms_cases()}
SCORED = [n for n in ref.NMS_IDS if '4096' not in n and CASES[n]['valid'] is None]      # the Python entries take no valid flags


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize('name', ref.NMS_IDS)
def test_grouped_restatement_equals_the_definition(name):
    from monorun_amd.proposals import nms_grouped, nms_grouped_torch
    c = CASES[name]
    want = ref.nms_ref32(c['boxes'], c['valid'], c['sizes'], c['thr'])
    valid = None if c['valid'] is None else _t(c['valid'])
    for fn in (nms_grouped, nms_grouped_torch):             # on CPU tensors the entry runs the restatement
        keep, num = fn(_t(c['boxes']), valid, c['sizes'], c['thr'])
        assert keep.dtype == torch.uint8 and num.dtype == torch.int32
        assert np.array_equal(keep.numpy().astype(bool), want)
        ends = np.cumsum(c['sizes'])
        assert num.tolist() == [int(want[e - n:e].sum()) for e, n in zip(ends, c['sizes'])]


def test_patterns_give_what_they_are_built_for():
    """the definition itself on the built patterns: every second box of a chain, one of identical boxes, all of disjoint ones, the far
    victims, NaN boxes kept and suppressing nothing, an invalid box suppressing nothing"""
    k = {n: ref.nms_ref32(c['boxes'], c['valid'], c['sizes'], c['thr']) for n, c in CASES.items() if n in
         ('chain_129_65_2', 'identical_65_1_64', 'disjoint_63_0_1025', 'far_4096', 'special_values', 'identical_valid_interleaved', 'none_valid')}
    assert np.array_equal(k['chain_129_65_2'][:129], np.arange(129) % 2 == 0) and k['chain_129_65_2'].sum() == 65 + 33 + 1
    assert k['identical_65_1_64'].sum() == 3 and k['identical_65_1_64'][[0, 65, 66]].all()
    assert k['disjoint_63_0_1025'].all()
    assert sorted(np.nonzero(~k['far_4096'])[0]) == sorted([64, 4095, 4096 - 64 + 3, 4032, 64 + 63, 129, 4000])
    sp = k['special_values'][:15]
    assert sp.tolist() == [True, True, False, True, True, True, True, False, True, True, True, False, True, True, False]
    assert np.array_equal(np.nonzero(k['identical_valid_interleaved'])[0], [1, 65]) and not k['none_valid'].any()


@pytest.mark.parametrize('name', ref.MARGIN_CASES)
def test_fp32_rule_equals_fp64_rule_where_the_margin_holds(name):
    """the fp32 IoU of exact fp32 boxes carries about eight roundings (< 1e-6 relative): a case whose float64 IoUs all lie farther than 1e-5
    from the threshold gives the same kept set in both precisions; the margin is asserted on the reference itself"""
    c = CASES[name]
    margin = ref.nms_margin64(c['boxes'], c['sizes'], c['thr'])
    print(f'{name}: smallest |iou64 - thr| = {margin:.3g}')
    assert margin > 1e-5
    assert np.array_equal(ref.nms_ref32(c['boxes'], None, c['sizes'], c['thr']), ref.nms_ref64(c['boxes'], None, c['sizes'], c['thr']))


@pytest.mark.parametrize('name', SCORED)
def test_nms_and_batched_nms_restatements(name):
    """mmcv's contracts on shuffled inputs with tied scores: dets (k, 5), keep (k,) in score-descending order, ties to the lower index"""
    from monorun_amd.proposals import batched_nms, nms
    c = CASES[name]
    boxes, scores, idxs = ref.scored(c)
    want = ref.batched_nms_ref(boxes, scores, idxs, c['thr'])
    dets, keep = batched_nms(_t(boxes), _t(scores), _t(idxs), dict(type='nms', iou_threshold=c['thr'], split_thr=10))
    assert keep.dtype == torch.int64 and np.array_equal(keep.numpy(), want)
    assert np.array_equal(dets.numpy(), np.concatenate([boxes[want], scores[want, None]], axis=1), equal_nan=True)
    one = np.zeros_like(idxs)
    want = ref.batched_nms_ref(boxes, scores, one, c['thr'])
    for got in (nms(_t(boxes), _t(scores), c['thr'])[1], batched_nms(_t(boxes), _t(scores), _t(idxs), dict(iou_thr=c['thr']), class_agnostic=True)[1],
                batched_nms(_t(boxes), _t(scores), _t(idxs), dict(type='nms', iou_threshold=c['thr'], class_agnostic=True))[1]):
        assert np.array_equal(got.numpy(), want)


def test_nms_cfg_rules():
    from monorun_amd.proposals import parse_nms_cfg
    assert parse_nms_cfg(dict(type='nms', iou_threshold=0.7)) == (0.7, False) and parse_nms_cfg(dict(iou_thr=0.5, split_thr=3)) == (0.5, False)
    with pytest.raises(NotImplementedError):
        parse_nms_cfg(dict(type='soft_nms', iou_threshold=0.5))
    with pytest.raises(KeyError):
        parse_nms_cfg(dict(type='nms'))


def multiclass_inputs(C, per_class, seed=2, K=90):
    rng = np.random.RandomState(seed)
    boxes = ref.clustered(seed, K, 200.0, 100.0)
    if per_class:
        boxes = np.concatenate([boxes + ref.F32(3 * c) for c in range(C)], axis=1)
    scores = rng.uniform(0, 1, size=(K, C + 1)).astype(ref.F32)
    scores[::7, 0] = scores[0, 0]                                       # ties
    return boxes, scores, rng.uniform(0.5, 1.0, size=K).astype(ref.F32)


MULTICLASS = [(C, per_class, thr, max_num, factors) for C in (1, 3) for per_class in (False, True)
              for thr, max_num, factors in ((0.3, -1, False), (0.3, 5, True), (0.3, 1000, True), (2.0, 10, False))]


@pytest.mark.parametrize('C,per_class,score_thr,max_num,factors', MULTICLASS)
def test_multiclass_nms_restatement(C, per_class, score_thr, max_num, factors):
    from monorun_amd.proposals import multiclass_nms
    boxes, scores, fac = multiclass_inputs(C, per_class)
    fac = fac if factors else None
    want_d, want_l = ref.multiclass_nms_ref(boxes, scores, score_thr, 0.5, max_num, fac)
    dets, labels = multiclass_nms(_t(boxes), _t(scores), score_thr, dict(type='nms', iou_threshold=0.5), max_num,
                                  None if fac is None else _t(fac))
    assert dets.shape == want_d.shape and labels.dtype == torch.int64
    assert np.array_equal(dets.numpy(), want_d) and np.array_equal(labels.numpy(), want_l)
    if score_thr > 1:
        assert dets.shape == (0, 5) and labels.shape == (0,)
    elif max_num == 5:
        assert len(want_d) == 5
    else:
        assert 5 < len(want_d) < 1000


# ------------------------------------------------------------------------------------------------ decode
@functools.lru_cache(maxsize=None)
def decode_run(name):
    """(box ratio, score ratio) of the fp32 torch restatement on a decode case, after the exact checks"""
    from monorun_amd.proposals import proposal_decode, proposal_decode_torch
    m = ref.DECODE_CASES[name]
    c = ref.decode_case(m)
    b64, s64, lg, v, mag = ref.decode_ref64(c['cls'], c['reg'], c['index'], c['counts'], c['img_shape'], c['base'], ref.STRIDES, ref.MEANS,
                                            ref.STDS, min_bbox_size=m)
    args = ([_t(x) for x in c['cls']], [_t(x) for x in c['reg']], _t(c['index']), c['counts'], _t(c['img_shape']), [_t(x) for x in c['base']],
            ref.STRIDES, ref.MEANS, ref.STDS)
    boxes, score, logit, valid = proposal_decode_torch(*args, min_bbox_size=m)
    again = proposal_decode(*args, min_bbox_size=m)                     # CPU tensors: the entry runs the restatement
    assert all(torch.equal(a, b) for a, b in zip((boxes, score, logit, valid), again))
    assert np.array_equal(logit.numpy(), lg) and valid.dtype == torch.uint8
    sides = np.stack([b64[..., 2] - b64[..., 0], b64[..., 3] - b64[..., 1]])
    clear = (np.abs(sides - m) > 1e-3).all(axis=0) | (m == 0)           # the flag is compared where fp32 cannot flip it
    assert np.array_equal(valid.numpy().astype(bool)[clear], v[clear]) and clear.mean() > 0.99
    return (float((np.abs(boxes.numpy().astype(np.float64) - b64) / (ref.EPS * mag)).max()),
            float((np.abs(score.numpy().astype(np.float64) - s64) / (ref.EPS * s64)).max()))


def test_decode_cases_cover_the_clamps_and_the_borders():
    c = ref.decode_case(8.0)
    b64, _, _, v, _ = ref.decode_ref64(c['cls'], c['reg'], c['index'], c['counts'], c['img_shape'], c['base'], ref.STRIDES, ref.MEANS, ref.STDS,
                                       min_bbox_size=8.0)
    m = float(ref.F32(abs(np.log(ref.WH_RATIO_CLIP))))
    dw = np.concatenate([r[:, 2::4].ravel() for r in c['reg']])
    assert (dw > m).any() and (dw < -m).any() and (np.abs(dw) < m).any()
    shape = c['img_shape'].astype(np.float64)
    for n in range(ref.N_IMAGES):
        assert (b64[n, :, 0] == 0).any() and (b64[n, :, 1] == 0).any()
        assert (b64[n, :, 2] == shape[n, 1]).any() and (b64[n, :, 3] == shape[n, 0]).any()
    assert v.any() and (~v).any() and shape[0].tolist() != shape[1].tolist()


@pytest.mark.parametrize('name', list(ref.DECODE_CASES))
def test_decode_restatement_within_the_bounds(name):
    box, score = decode_run(name)
    print(f'{name}: error / (2^-23 magnitude): box {box:.2f} score {score:.2f}')
    assert box <= ref.C_BOX and score <= ref.C_SCORE


def test_the_decode_constants_are_the_measured_ones():
    """C_*_MEASURED of proposals_ref are what the fp32 restatement shows (torch's kernels differ a little between builds: the recorded
    figure must cover this build's and be no more than twice it); the bounds are 4 x"""
    box, score = np.max([decode_run(n) for n in ref.DECODE_CASES], axis=0)
    print(f'fp32 restatement, error / (2^-23 magnitude): box {box:.3f} score {score:.3f}')
    assert box <= ref.C_BOX_MEASURED * 1.05 and ref.C_BOX_MEASURED <= 2 * box
    assert score <= ref.C_SCORE_MEASURED * 1.05 and ref.C_SCORE_MEASURED <= 2 * score
    assert ref.C_BOX == 4 * ref.C_BOX_MEASURED and ref.C_SCORE == 4 * ref.C_SCORE_MEASURED


def e2e_reference():
    c = ref.e2e_case()
    index, counts = ref.select_ref(c['cls'], ref.E2E_NMS_PRE)
    out = ref.decode_ref64(c['cls'], c['reg'], index, counts, c['img_shape'], c['base'], ref.STRIDES, ref.MEANS, ref.STDS,
                           min_bbox_size=ref.E2E_MIN_SIZE)
    return c, index, counts, out


def test_end_to_end_case_has_the_margins_it_claims():
    """the fixed seed: no pair's float64 IoU within 5e-3 of the threshold, no two logits of a level equal, no side within 1e-2 of
    min_bbox_size — decoded coordinates move by about 1e-3 px at most, which moves an IoU of boxes with sides >= 4 px by about 2e-3"""
    c, index, counts, (b64, s64, lg, v, mag) = e2e_reference()
    assert ref.nms_margin64(b64.reshape(-1, 4), tuple(counts) * ref.N_IMAGES, ref.E2E_THR) > 5e-3
    assert all(np.unique(x[n]).size == x[n].size for x in c['cls'] for n in range(ref.N_IMAGES))
    sides = np.stack([b64[..., 2] - b64[..., 0], b64[..., 3] - b64[..., 1]])
    assert np.abs(sides - ref.E2E_MIN_SIZE).min() > 1e-2 and v.any() and (~v).any()
    keep = ref.nms_ref64(b64.reshape(-1, 4), v.reshape(-1), tuple(counts) * ref.N_IMAGES, ref.E2E_THR)
    assert 0.5 * v.sum() < keep.sum() < v.sum()                         # the NMS removes something and keeps most


def head(**kw):
    from monorun_amd.rpn_head import RPNHeadMod
    cfg = dict(nms_across_levels=False, nms_pre=ref.E2E_NMS_PRE, nms_post=ref.E2E_NMS_POST, max_num=ref.E2E_NMS_POST, nms_thr=ref.E2E_THR,
               min_bbox_size=ref.E2E_MIN_SIZE)
    cfg.update(kw)
    return RPNHeadMod(8, starting_level=1, feat_channels=8, test_cfg=cfg,
                      anchor_generator=dict(type='AnchorGenerator', scales=[2], ratios=[0.4, 0.7, 1.0], strides=list(ref.STRIDES)),
                      bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=ref.MEANS, target_stds=ref.STDS))


def metas():
    return [dict(img_shape=(int(h), int(w), 3)) for h, w in ref.IMG_SHAPES]


def check_end_to_end(device):
    """get_bboxes on the end-to-end case against nms_ref64 on decode_ref64: equal kept sets, boxes and scores within the decode bounds"""
    c, index, counts, (b64, s64, lg, v, mag) = e2e_reference()
    keep = ref.nms_ref64(b64.reshape(-1, 4), v.reshape(-1), tuple(counts) * ref.N_IMAGES, ref.E2E_THR).reshape(ref.N_IMAGES, -1)
    want = ref.merge_ref(b64, s64, lg, keep, ref.E2E_NMS_POST)
    tol = ref.merge_ref(ref.C_BOX * ref.EPS * mag, ref.C_SCORE * ref.EPS * s64, lg, keep, ref.E2E_NMS_POST)
    h = head().to(device)
    got = h.get_bboxes([_t(x).to(device) for x in c['cls']], [_t(x).to(device) for x in c['reg']], metas())
    assert len(got) == ref.N_IMAGES
    for g, w, t in zip(got, want, tol):
        assert g.shape == w.shape and g.dtype == torch.float32 and 0 < len(w) <= ref.E2E_NMS_POST
        assert (np.abs(g.cpu().numpy().astype(np.float64) - w) <= t).all()


def test_get_bboxes_end_to_end_restatement():
    check_end_to_end('cpu')


def test_get_bboxes_rules():
    c = ref.e2e_case()
    cls, reg = [_t(x) for x in c['cls']], [_t(x) for x in c['reg']]
    h = head()
    out, counts = h.get_bboxes(cls, reg, metas(), padded=True)
    lst = h.get_bboxes(cls, reg, _t(c['img_shape']))                    # the image shapes as a tensor (N, 2)
    assert out.shape == (ref.N_IMAGES, ref.E2E_NMS_POST, 5) and counts.dtype == torch.int32
    for n, k in enumerate(counts.tolist()):
        assert torch.equal(out[n, :k], lst[n]) and torch.isnan(out[n, k:]).all() and not torch.isnan(out[n, :k]).any()
    with pytest.raises(NotImplementedError):
        h.get_bboxes(cls, reg, metas(), cfg=dict(h.test_cfg, nms_across_levels=True))
    with pytest.raises(ValueError):
        h.get_bboxes(cls, reg, metas(), cfg=dict(h.test_cfg, max_num=7))
    with pytest.raises(ValueError):
        h.get_bboxes(cls, reg, metas(), cfg=dict(h.test_cfg, max_per_img=7))
    few = h.get_bboxes(cls, reg, metas(), cfg=dict(nms_pre=0, nms_post=3, nms=dict(type='nms', iou_threshold=0.5)))
    assert [len(f) for f in few] == [3, 3] and all((f[:-1, 4] >= f[1:, 4]).all() for f in few)
    feats = [torch.randn(ref.N_IMAGES, 8, 2 * hh, 2 * ww) for hh, ww in ref.MAPS[:1]] + [torch.randn(ref.N_IMAGES, 8, hh, ww) for hh, ww in ref.MAPS]
    cls2, reg2 = h(feats)
    assert [tuple(x.shape) for x in cls2] == [(ref.N_IMAGES, 3) + m for m in ref.MAPS]
    assert [tuple(x.shape) for x in reg2] == [(ref.N_IMAGES, 12) + m for m in ref.MAPS]
    props = h.simple_test_rpn(feats, metas())
    assert len(props) == ref.N_IMAGES and all(p.shape[1] == 5 and not p.requires_grad for p in props)


def test_head_has_mmdets_keys():
    from monorun_amd.rpn_head import RPNHeadMod
    h = RPNHeadMod(256, starting_level=1, feat_channels=256,
                   anchor_generator=dict(type='AnchorGenerator', scales=[5], ratios=[0.4, 0.7, 1.0], strides=[4, 8, 16, 32, 64]),
                   bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=[.0, .0, .0, .0], target_stds=[1.0, 1.0, 1.0, 1.0]))
    shapes = {k: tuple(v.shape) for k, v in h.state_dict().items()}
    assert shapes == {'rpn_conv.weight': (256, 256, 3, 3), 'rpn_conv.bias': (256,), 'rpn_cls.weight': (3, 256, 1, 1), 'rpn_cls.bias': (3,),
                      'rpn_reg.weight': (12, 256, 1, 1), 'rpn_reg.bias': (12,)}
    h.load_state_dict({k: torch.zeros(s) for k, s in shapes.items()}, strict=True)


def test_anchor_generator_for_the_reference_config():
    from monorun_amd.rpn_head import AnchorGenerator
    scales, ratios, strides = [5], [0.4, 0.7, 1.0], [4, 8, 16, 32, 64]
    gen = AnchorGenerator(scales, ratios, strides)
    want = ref.base_anchors64(scales, ratios, strides)
    assert gen.num_levels == 5 and gen.num_base_anchors == [3] * 5
    for got, w in zip(gen.base_anchors, want):
        assert got.shape == (3, 4) and got.dtype == torch.float32
        assert np.abs(got.numpy().astype(np.float64) - w).max() <= 4 * ref.EPS * np.abs(w).max()      # sqrt, reciprocal, two products, a half
    assert np.allclose(want[0][2], [-10, -10, 10, 10]) and want[2][0][2] > want[2][0][3]           # ratio 1: a square of stride x scale
    grid = gen.grid_anchors([(2, 3)] * 5)
    assert grid[1].shape == (18, 4) and torch.equal(grid[1][(1 * 3 + 2) * 3 + 1], gen.base_anchors[1][1] + torch.tensor([16.0, 8.0, 16.0, 8.0]))


# ------------------------------------------------------------------------------------------------ the loader's row
_PINNED = ('mr_proposal_decode', 'mr_nms_workspace_bytes', 'mr_nms_grouped')
_SCALAR = {'int': ctypes.c_int, 'float': ctypes.c_float, 'double': ctypes.c_double, 'size_t': ctypes.c_size_t, 'int64_t': ctypes.c_int64}


def _declared_prototypes(path):
    """[(return type, name, [arguments])] of a header, by a regex of this file's own (not `_lib.header_prototypes`)."""
    src = re.sub(r'/\*.*?\*/', ' ', open(path).read(), flags=re.S)
    found = re.findall(r'^((?:const\s+)?\w+[\s\*]+)(\w+)\s*\(([^)]*)\)\s*;', src, flags=re.M)
    return [(' '.join(ret.split()), name, [] if args.strip() in ('', 'void') else [' '.join(a.split()) for a in args.split(',')])
            for ret, name, args in found]


def test_loader_binds_the_proposals_header(monkeypatch):
    """the row of `_lib.LATER_HEADERS` this subsystem owns (nothing is asserted about the table's other rows): the pinned names are what the
    header declares, in order, and no other header's; the library exports each; restype, argtypes and arg_names are the declared ones; the
    header alone makes the library stale"""
    from monorun_amd import _lib
    key = 'proposals'
    assert key in _lib.LATER_HEADERS and key in _lib.all_header_keys() and key not in _lib.header_keys()
    assert _lib.all_header_keys()[:len(_lib.header_keys())] == _lib.header_keys()
    assert not set(_PINNED) & set(_lib.exported_symbols())
    lib, raw = _lib.load(), ctypes.CDLL(_lib.SO)
    assert _lib.exported_symbols(key) == _lib.LATER_HEADERS[key][1] == _PINNED
    assert _lib.header_path(key) == os.path.join(ROOT, 'include', 'monorun_proposals.h')
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
    assert _lib.arg_names('mr_nms_workspace_bytes') == ('group_sizes', 'groups', 'max_group')
    assert set(_lib.table_args('mr_proposal_decode')) == {'cls', 'reg'} and _lib.table_args('mr_nms_grouped') == ()
    assert not _lib._stale()
    so_time, real = os.path.getmtime(_lib.SO), os.path.getmtime
    monkeypatch.setattr(os.path, 'getmtime', lambda f: so_time + 10 if f == _lib.header_path(key) else real(f))
    assert _lib._stale()


def test_workspace_bytes_and_argument_checks_without_a_gpu():
    """every check comes before any HIP call: the codes of monorun_pnp.h (-1 bad argument, -2 unsupported); no boxes: no launch"""
    from monorun_amd import _lib
    from monorun_amd.proposals import nms_workspace_bytes
    lib = _lib.load()
    BAD, UNSUPPORTED = -1, -2
    assert nms_workspace_bytes((0, 1, 64, 65, 4096)) == 8 * (1 + 64 + 65 * 2 + 4096 * 64) and nms_workspace_bytes(()) == 0
    sizes = (ctypes.c_int * 3)(5, 100, 4097)
    assert lib.mr_nms_workspace_bytes(sizes, 3, 64) == 8 * (5 + 64 + 64) and lib.mr_nms_workspace_bytes(None, 3, 64) == 0
    one = ctypes.c_void_p(16)                       # never dereferenced: every call below is rejected before a launch
    base = dict(boxes=one, valid=None, offsets=one, groups=2, max_group=10, thr=0.5, keep=one, num_keep=one, workspace=one)

    def nms(**over):
        return lib.mr_nms_grouped(*_lib.pack('mr_nms_grouped', dict(base, **over)), None)

    assert nms(groups=-1) == BAD and nms(max_group=-1) == BAD
    assert nms(boxes=None) == BAD and nms(offsets=None) == BAD and nms(keep=None) == BAD and nms(num_keep=None) == BAD and nms(workspace=None) == BAD
    assert nms(max_group=4097) == UNSUPPORTED and nms(groups=65536) == UNSUPPORTED
    assert nms(groups=0, boxes=None, offsets=None) == 0 and nms(max_group=0, boxes=None, keep=None, workspace=None) == 0

    L = 2
    def tables(L=L, h=4, w=4, s=4, count=3, null=False):
        i = ctypes.c_int * L
        return dict(cls=(ctypes.c_void_p * L)(*[None if null else 16] * L), reg=(ctypes.c_void_p * L)(*[16] * L), level_h=i(*[h] * L),
                    level_w=i(*[w] * L), level_stride=i(*[s] * L), level_count=i(*[count] * L), base_anchors=(ctypes.c_float * (L * 16 * 4))(),
                    n_levels=L)
    f4 = (ctypes.c_float * 4)()
    dbase = dict(n_anchors=3, n_images=1, index=one, img_shape=one, means=f4, stds=f4, wh_ratio_clip=0.016, min_bbox_size=0.0, boxes=one,
                 score=one, logit=one, valid=one)

    def dec(table={}, **over):
        a = dict(dbase, **tables(**table))
        a.update(over)
        return lib.mr_proposal_decode(*_lib.pack('mr_proposal_decode', a), None)

    assert dec(n_levels=0) == BAD and dec(n_images=0) == BAD and dec(n_anchors=0) == BAD
    assert dec(table=dict(h=0)) == BAD and dec(table=dict(w=0)) == BAD and dec(table=dict(s=0)) == BAD and dec(table=dict(count=-1)) == BAD
    assert dec(table=dict(null=True)) == BAD and dec(cls=None) == BAD and dec(level_count=None) == BAD and dec(means=None) == BAD
    assert dec(wh_ratio_clip=0.0) == BAD and dec(wh_ratio_clip=float('nan')) == BAD
    assert dec(index=None) == BAD and dec(img_shape=None) == BAD and dec(boxes=None) == BAD and dec(valid=None) == BAD
    assert dec(table=dict(L=9)) == UNSUPPORTED and dec(n_anchors=17) == UNSUPPORTED and dec(n_images=40000) == UNSUPPORTED
    assert dec(table=dict(h=1 << 14, w=1 << 14)) == UNSUPPORTED
    assert dec(table=dict(count=0), index=None, boxes=None) == 0                      # no candidates: nothing is launched
