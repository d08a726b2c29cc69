"""The training step's assembly on the GPU: ``mr_roi_train_positives`` bitwise against ``positives_torch`` on the device
without a host synchronisation, the fast path of ``MonoRUnRoIHead.forward_train`` bitwise against the literal path — every loss, every
parameter gradient, the gradients of the feature maps —, the paths' choice, a batch without positives, and ``MonoRUnDetector``'s
``forward_train`` / ``train_step``."""
import copy

import pytest
import torch

from tests import roi_train_ref as tr
from monorun_amd import roi_train as RT

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CASES = ('three-images', 'one-image', 'empty', 'agnostic', 'many')


class no_sync:
    def __enter__(self):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode('error')

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode('default')


def same_bits(a, b):
    bits = lambda t: t.detach().contiguous().reshape(-1).view(torch.uint8)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize('name', CASES)
def test_positives_launch_equals_the_restatement_bitwise_without_a_synchronisation(name):
    case = tr.positives_case(name)
    args = tr.case_call(case, DEV)
    assert RT.hip_ok(args[0], args[1], args[2], args[4], args[5], args[8], args[12])
    RT.positives(*args), RT.positives_torch(*args)                               # warm-up: the constants' and offsets' caches
    with no_sync():
        got = RT.positives(*args)
        want = RT.positives_torch(*args)
        again = RT.positives(*args)
    assert len(got) == sum(case['counts'])
    for k in RT.FIELDS:
        assert same_bits(getattr(got, k), getattr(want, k)), (name, k)
        assert same_bits(getattr(got, k), getattr(again, k)), (name, k, 'repeated call')
    if name == 'three-images':
        h, w = case['shapes'][1][:2]
        assert got.pos_bboxes[0].tolist() == [0, 0, w, h] and got.flip.tolist() == [1] * 6 and got.pos_assigned_gt_inds[:2].tolist() == [0, 1]


def test_positives_over_the_caps_run_the_restatement():
    case = tr.positives_case('one-image')
    args = list(tr.case_call(case, DEV))
    assert not RT.hip_ok(args[0], args[1], args[2], [torch.zeros(257, 7, device=DEV)], args[5], args[8], args[12])
    assert not RT.hip_ok(args[0], args[1], args[2].double(), args[4], args[5], args[8], args[12])
    assert not RT.hip_ok(args[0], args[1], args[2], args[4], args[5], 17, args[12])


# ------------------------------------------------------------------------------------------------ the head
UPSTREAM = ('loss_cls', 'acc', 'loss_bbox', 'loss_dim', 'loss_noc')           # what does not pass through the NOC decode
DOWNSTREAM = ('loss_proj', 'mean_iou', 'loss_calib', 'loss_score')            # what does


def run_path(head, inputs, keys, path, seed=7, backward=None):
    """one forward + backward (of the entries ``backward``; default: every loss) of a copy of ``head`` on ``path``: (losses, parameter
    gradients by name, feature-map gradients, the copy)"""
    head = copy.deepcopy(head)
    x = [f.detach().clone().requires_grad_(True) for f in inputs['x']]
    torch.manual_seed(seed)
    losses = head.forward_train(**dict(inputs, x=x), keys=keys, path=path)
    assert head.last_train_path == path
    total = sum(v.sum() for k, v in losses.items() if 'loss' in k and (backward is None or k in backward))
    total.backward()
    grads = {n: p.grad for n, p in head.named_parameters()}
    return losses, grads, [f.grad for f in x], head


@pytest.fixture
def deterministic_convolutions():
    """MIOpen's weight-gradient kernels of the NOC head's convolutions sum in an order that changes from run to run (measured: the
    literal path against ITSELF differs in five conv weights' gradients by up to 4e-7, and in nothing else); with this switch torch asks
    for the deterministic ones, and two runs of one path agree in every bit"""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = before


def assert_same_gradients(fast, lit):
    (_, fast_grads, fast_x, _), (_, lit_grads, lit_x, _) = fast, lit
    reached = 0
    for n, g in lit_grads.items():
        assert (g is None) == (fast_grads[n] is None), n
        if g is not None:
            assert same_bits(fast_grads[n], g), n
            reached += int(g.abs().sum() > 0)
    assert reached > 10
    for a, b in zip(fast_x, lit_x):
        assert (a is None) == (b is None) and (a is None or same_bits(a, b))
    assert sum(g is not None and float(g.abs().sum()) > 0 for g in lit_x) >= 2


@pytest.mark.parametrize('agnostic', [False, True])
def test_fast_path_with_the_literal_decode_equals_the_literal_path_bitwise(agnostic, deterministic_convolutions):
    """a projection head that does not train the std of the encoded error: ``train_decode_reason`` keeps the literal decode inside the fast
    path, and then EVERY entry and every gradient is the literal path's, bit for bit"""
    head = tr.build_roi_head(agnostic=agnostic).to(DEV)
    head.projection_head.train_std_of_encoded_error = False
    inputs = tr.batch_inputs(DEV)
    keys = tr.sampler_keys(inputs, DEV)
    assert head.train_fast_path_reason(inputs['x'], inputs['proposal_list']) is None and head.train_decode_reason().startswith('train_std')
    fast, lit = run_path(head, inputs, keys, 'fast'), run_path(head, inputs, keys, 'literal')
    assert fast[3].last_positive_stage == 'launch' and fast[3].last_train_decode == 'literal'
    assert list(fast[0]) == list(lit[0]) and set(fast[0]) == set(tr.LOSS_KEYS)
    for k in lit[0]:
        assert torch.isfinite(lit[0][k]).all(), k
        assert same_bits(fast[0][k], lit[0][k]), (k, fast[0][k], lit[0][k])
    assert_same_gradients(fast, lit)


@pytest.mark.parametrize('agnostic', [False, True])
def test_fast_path_equals_the_literal_path_bitwise_upstream_of_the_decode(agnostic, deterministic_convolutions):
    """the reference configs' structure: the fast path decodes with ``decode_for_training``.  Everything that does not pass through the
    decode — the 2-D losses, the dimension loss, the NOC loss, and the gradients of their sum to every parameter and to the feature
    maps — is the literal path's bit for bit; the entries downstream are held against float64 below"""
    head = tr.build_roi_head(agnostic=agnostic).to(DEV)
    inputs = tr.batch_inputs(DEV)
    keys = tr.sampler_keys(inputs, DEV)
    assert head.train_fast_path_reason(inputs['x'], inputs['proposal_list']) is None and head.train_decode_reason() is None
    fast, lit = run_path(head, inputs, keys, 'fast', backward=UPSTREAM), run_path(head, inputs, keys, 'literal', backward=UPSTREAM)
    assert fast[3].last_positive_stage == 'launch' and fast[3].last_train_decode == 'fused' and lit[3].last_train_decode == 'literal'
    assert list(fast[0]) == list(lit[0]) and set(fast[0]) == set(tr.LOSS_KEYS) == set(UPSTREAM) | set(DOWNSTREAM)
    print({k: float(v.detach().sum()) for k, v in fast[0].items()})
    for k in UPSTREAM:
        assert same_bits(fast[0][k], lit[0][k]), (k, fast[0][k], lit[0][k])
    for k in DOWNSTREAM:
        assert torch.isfinite(fast[0][k]).all() and torch.isfinite(lit[0][k]).all(), k
    assert float(lit[0]['loss_bbox']) > 0 and float(lit[0]['loss_dim']) > 0 and float(lit[0]['loss_noc']) > 0
    assert_same_gradients(fast, lit)


class float32_dropout_masks:
    """torch's fused dropout consumes its generator in a pattern that depends on the element size, so a float64 run would drop OTHER
    units than a float32 run of the same seed.  Inside this block ``dropout`` and ``dropout2d`` draw one float32 uniform per unit (per
    channel) from the same generator whatever the input's dtype: the three runs of the comparison below see the same masks."""

    @staticmethod
    def dropout(input, p=0.5, training=True, inplace=False):
        if not training or p == 0:
            return input
        keep = torch.rand(input.shape, dtype=torch.float32, device=input.device) >= p
        return input * keep.to(input.dtype) / (1 - p)

    @staticmethod
    def dropout2d(input, p=0.5, training=True, inplace=False):
        if not training or p == 0:
            return input
        keep = torch.rand(input.shape[:2] + (1, 1), dtype=torch.float32, device=input.device) >= p
        return input * keep.to(input.dtype) / (1 - p)

    def __enter__(self):
        F = torch.nn.functional
        self.before = (F.dropout, F.dropout2d)
        F.dropout, F.dropout2d = self.dropout, self.dropout2d

    def __exit__(self, *exc):
        torch.nn.functional.dropout, torch.nn.functional.dropout2d = self.before


def to_float64(inputs):
    cast = lambda v: v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v
    return {k: [cast(t) for t in v] if isinstance(v, list) else cast(v) for k, v in inputs.items()}


def forward_only(head, inputs, keys, path, seed=7):
    head = copy.deepcopy(head)
    torch.manual_seed(seed)
    with torch.no_grad(), float32_dropout_masks():
        losses = head.forward_train(**inputs, keys=keys, path=path)
    return {k: v.detach().double().sum() for k, v in losses.items()}, head


def test_entries_downstream_of_the_fused_decode_against_float64():
    """The fused training decode uses the library's specified exp and log, so the entries downstream of it cannot equal the literal
    path's bit for bit.  For those entries each fp32 path is held against a float64 run of the literal path (same weights, same keys, same
    seeds, same dropout masks): the fast path may deviate at most twice as far as the literal fp32 path itself does.  The upstream
    entries of the three runs are printed too: they say how far the float64 run is from an fp32 one before the decode."""
    head = tr.build_roi_head().to(DEV)
    inputs = tr.batch_inputs(DEV)
    keys = tr.sampler_keys(inputs, DEV)
    fast, fast_head = forward_only(head, inputs, keys, 'fast')
    lit, _ = forward_only(head, inputs, keys, 'literal')
    ref, _ = forward_only(copy.deepcopy(head).double(), to_float64(inputs), keys, 'literal')
    assert fast_head.last_train_decode == 'fused' and fast_head.last_positive_stage == 'launch'
    dev_fast = {k: abs(float(fast[k] - ref[k])) for k in ref}
    dev_lit = {k: abs(float(lit[k] - ref[k])) for k in ref}
    for k in ref:
        print(f'{k}: float64 {float(ref[k]):.9g}  literal fp32 {float(lit[k]):.9g} (|d| {dev_lit[k]:.3g})  fast fp32 {float(fast[k]):.9g} (|d| {dev_fast[k]:.3g})')
    for k in UPSTREAM:
        assert float(fast[k]) == float(lit[k]), k
    for k in DOWNSTREAM:
        assert dev_fast[k] <= 2 * dev_lit[k], (k, dev_fast[k], dev_lit[k])


def test_path_choice():
    inputs = tr.batch_inputs(DEV, n_images=2, n_proposals=(12, 9))
    refined = tr.build_roi_head(refined=True).to(DEV)
    why = refined.train_fast_path_reason(inputs['x'], inputs['proposal_list'])
    assert why is not None and why.startswith('a refined assigner')
    with pytest.raises(RuntimeError, match='a refined assigner'):
        refined.forward_train(**inputs, path='fast')
    torch.manual_seed(3)
    losses = refined.forward_train(**inputs, generator=torch.Generator(device=DEV).manual_seed(5))
    assert refined.last_train_path == 'literal' and set(losses) == set(tr.LOSS_KEYS)
    assert all(torch.isfinite(v).all() for v in losses.values())
    debug = tr.build_roi_head(debug=True).to(DEV)
    assert debug.train_fast_path_reason(inputs['x'], inputs['proposal_list']).startswith('debug')
    plain = tr.build_roi_head().to(DEV)
    plain.forward_train(**inputs, generator=torch.Generator(device=DEV).manual_seed(5))
    assert plain.last_train_path == 'fast'
    assert plain.train_fast_path_reason([f.double() for f in inputs['x']]) == 'the feature maps are not CUDA fp32'


@pytest.mark.parametrize('path', ['fast', 'literal'])
def test_a_batch_without_positives_gives_finite_losses_and_gradients(path):
    head = tr.build_roi_head().to(DEV)
    inputs = tr.batch_inputs(DEV, n_images=2, n_proposals=(7, 5), empty=True)
    torch.manual_seed(1)
    losses = head.forward_train(**inputs, keys=tr.sampler_keys(inputs, DEV), path=path)
    assert set(losses) == set(tr.LOSS_KEYS) and all(torch.isfinite(v).all() for v in losses.values())
    assert float(losses['loss_cls']) > 0 and all(float(losses[k].sum()) == 0 for k in ('loss_bbox', 'loss_dim', 'loss_noc', 'loss_proj', 'loss_score'))
    sum(v.sum() for k, v in losses.items() if 'loss' in k).backward()
    grads = [p.grad for p in head.bbox_head.parameters()]
    assert all(g is not None and torch.isfinite(g).all() for g in grads) and float(head.bbox_head.fc_cls.weight.grad.abs().sum()) > 0


# ------------------------------------------------------------------------------------------------ the detector
def detector_data(n_images=2):
    inputs = tr.batch_inputs(DEV, n_images=n_images, n_proposals=(4, 4, 4)[:n_images])
    img = torch.randn(n_images, 3, tr.IMG_H, tr.IMG_W, generator=torch.Generator().manual_seed(4)).to(DEV)
    return dict(img=img, **{k: v for k, v in inputs.items() if k not in ('x', 'proposal_list')})


def test_detector_forward_train_is_the_composition_of_its_parts():
    det = tr.build_detector().to(DEV)
    data = detector_data()
    gen = lambda s: torch.Generator(device=DEV).manual_seed(s)
    torch.manual_seed(11)
    got = copy.deepcopy(det)(**data, return_loss=True, rpn_kwargs=dict(generator=gen(1)), generator=gen(2))
    ref = copy.deepcopy(det)
    torch.manual_seed(11)
    x = ref.extract_feat(data['img'])
    want, proposals = ref.rpn_head.forward_train(x, data['img_metas'], data['gt_bboxes'], gt_labels=None, gt_bboxes_ignore=None,
                                                 proposal_cfg=tr.TRAIN_CFG['rpn_proposal'], generator=gen(1))
    assert len(proposals) == 2 and all(p.shape[1] == 5 and 0 < p.shape[0] <= 24 for p in proposals)
    rest = {k: v for k, v in data.items() if k not in ('img', 'img_metas', 'gt_bboxes', 'gt_labels')}
    want.update(ref.roi_head.forward_train(x, data['img_metas'], proposals, data['gt_bboxes'], data['gt_labels'], None, None, **rest, generator=gen(2)))
    assert list(got) == list(want) and set(got) == set(tr.LOSS_KEYS) | {'loss_rpn_cls', 'loss_rpn_bbox'}
    for k, v in want.items():
        for a, b in zip(got[k] if isinstance(v, list) else [got[k]], v if isinstance(v, list) else [v]):
            assert same_bits(a, b), k


def test_one_train_step_moves_every_trained_part():
    det = tr.build_detector(iou3d_sampler=False).to(DEV)
    data = detector_data(n_images=3)
    before = {n: p.detach().clone() for n, p in det.named_parameters()}
    opt = torch.optim.SGD([p for p in det.parameters() if p.requires_grad], lr=0.01)
    torch.manual_seed(5)
    out = det.train_step(dict(data, generator=torch.Generator(device=DEV).manual_seed(2)), opt)
    assert set(out) == {'loss', 'log_vars', 'num_samples'} and out['num_samples'] == 3
    assert torch.isfinite(out['loss']) and set(out['log_vars']) == set(tr.LOSS_KEYS) | {'loss_rpn_cls', 'loss_rpn_bbox', 'loss'}
    assert abs(out['log_vars']['loss'] - sum(v for k, v in out['log_vars'].items() if 'loss' in k and k != 'loss')) <= 1e-4 * abs(out['log_vars']['loss'])
    print(out['log_vars'])
    opt.zero_grad()
    out['loss'].backward()
    opt.step()
    moved = {n for n, p in det.named_parameters() if not torch.equal(p.detach(), before[n])}
    assert all(torch.isfinite(p).all() for p in det.parameters())
    for part in ('backbone.layer2', 'backbone.layer4', 'neck', 'rpn_head', 'roi_head.bbox_head', 'roi_head.global_head', 'roi_head.noc_head',
                 'roi_head.pose_head', 'roi_head.score_head'):
        assert any(n.startswith(part + '.') for n in moved), part
    assert not any(n.startswith('backbone.conv1') or n.startswith('backbone.layer1.') for n in moved)      # frozen_stages=1
