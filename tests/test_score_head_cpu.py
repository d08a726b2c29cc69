"""The score head on the CPU: MLPScoreHead, BatchNormSmooth1D, IoU3DBalancedSampler and the sigmoid CrossEntropyLoss
against G16 (tests/golden/g16_score_head.npz: what the reference's own classes returned, tests/golden/make_golden_score.py), the
loader's binding of include/monorun_heads.h, the entry point's argument checks, and score_poses against the step-by-step torch
restatement of monorun_roi_head.py:536-550.  No GPU."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C1, C2 = 96, 40


@pytest.fixture(scope='module')
def g16():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'g16_score_head.npz')))


def _head(g16, **kw):
    from monorun_amd.score_head import MLPScoreHead
    head = MLPScoreHead(reg_fc_out_channels=C1, pose_fc_out_channels=C1, fc_out_channels=C2, **kw)
    head.load_state_dict({k[len('param.'):]: torch.from_numpy(v) for k, v in g16.items() if k.startswith('param.')}, strict=True)
    return head


def _inputs(g16, name):
    return [torch.from_numpy(g16[f'{name}_{k}']) for k in ('reg_fc_out', 'yaw', 't_vec', 'pose_cov', 'dimensions')]


def test_state_dict_has_the_reference_keys_and_round_trips(g16):
    from monorun_amd.score_head import MLPScoreHead
    head = MLPScoreHead()
    want = json.loads(str(g16['default_state_dict']))
    assert [[k, list(v.shape)] for k, v in head.state_dict().items()] == want
    assert any(k.startswith('pose_norm.') for k, _ in want) and any(k.startswith('pose_fcs.0.') for k, _ in want)
    assert any(k.startswith('fused_fcs.0.') for k, _ in want) and any(k.startswith('fc_out.') for k, _ in want)
    torch.manual_seed(3)
    src = MLPScoreHead()
    src.init_weights()
    with torch.no_grad():
        src.pose_norm.running_mean.normal_()
    head.load_state_dict(src.state_dict(), strict=True)
    for (ka, a), (kb, b) in zip(head.state_dict().items(), src.state_dict().items()):
        assert ka == kb and torch.equal(a, b)
    assert head.pre_sigmoid is True
    # the reference's init rules: zero biases, xavier-uniform hidden weights (|w| <= sqrt(6 / (fan_in + fan_out))), N(0, 0.01) output
    for fc in list(src.pose_fcs) + list(src.fused_fcs):
        assert float(fc.bias.detach().abs().max()) == 0
        assert float(fc.weight.detach().abs().max()) <= (6.0 / (fc.in_features + fc.out_features)) ** 0.5
    assert float(src.fc_out.bias.detach().abs().max()) == 0 and 0.005 < float(src.fc_out.weight.detach().std()) < 0.02


def test_eval_logits_match_g16(g16):
    head = _head(g16).eval()
    with torch.no_grad():
        got = head(*_inputs(g16, 'A')).numpy()
    ref = g16['eval_logits']
    assert got.shape == (24,)
    assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max()
    assert int(head.pose_norm.num_batches_tracked) == 0                    # eval mode touches no buffer
    assert np.array_equal(head.pose_norm.running_mean.numpy(), g16['param.pose_norm.running_mean'])


def test_training_calls_update_the_buffers_as_g16(g16):
    head = _head(g16).train()
    for k, (tag, name) in enumerate((('train1', 'A'), ('train2', 'B'), ('train_one_row', 'C')), start=1):
        got = head(*_inputs(g16, name))
        ref = g16[f'{tag}_logits']
        assert np.abs(got.detach().numpy() - ref).max() <= 1e-5 * max(np.abs(ref).max(), 1.0), tag
        np.testing.assert_allclose(head.pose_norm.running_mean.numpy(), g16[f'{tag}_running_mean'], rtol=1e-6, atol=1e-7, err_msg=tag)
        np.testing.assert_allclose(head.pose_norm.running_var.numpy(), g16[f'{tag}_running_var'], rtol=1e-6, atol=1e-7, err_msg=tag)
        assert int(head.pose_norm.num_batches_tracked) == int(g16[f'{tag}_num_batches_tracked']) == k
        assert not head.pose_norm.running_mean.requires_grad and got.requires_grad
    # one row: counted, statistics untouched
    assert np.array_equal(g16['train_one_row_running_var'], g16['train2_running_var'])


def test_batch_norm_smooth_normalises_with_the_running_statistics():
    from monorun_amd.score_head import BatchNormSmooth1D
    bn = BatchNormSmooth1D(5, momentum=0.1)
    ref = torch.nn.BatchNorm1d(5)
    assert [(k, v.shape) for k, v in bn.state_dict().items()] == [(k, v.shape) for k, v in ref.state_dict().items()]
    x = torch.randn(7, 5, generator=torch.Generator().manual_seed(0)) * 3 + 1
    bn.train()
    y = bn(x)
    var, mean = torch.var_mean(x, dim=0)
    torch.testing.assert_close(bn.running_mean, 0.1 * mean)
    torch.testing.assert_close(bn.running_var, 0.9 + 0.1 * var)
    torch.testing.assert_close(y, (x - bn.running_mean) / (bn.running_var + bn.eps).sqrt())      # not the batch's statistics
    with pytest.raises(ValueError):
        bn(torch.zeros(3))


def test_loss_targets_of_the_three_modes_match_g16(g16):
    ious, scores = torch.from_numpy(g16['loss_ious']), torch.from_numpy(g16['loss_scores'])
    for mode in ('average', 'thres', 'linear_average'):
        head = _head(g16, mode=mode)
        want = torch.from_numpy(g16[f'loss_targets_{mode}'])
        got = head.get_targets(ious.clone())
        assert torch.equal(got, want), mode
        loss = head.loss(scores, ious.clone())['loss_score']
        torch.testing.assert_close(loss, F.binary_cross_entropy_with_logits(scores.unsqueeze(1), want))
    assert _head(g16, loss_score=None).loss(scores, ious) == dict()


def test_loss_with_a_sampler_weights_per_sample(g16, monkeypatch):
    head = _head(g16, train_cfg=dict(iou3d_sampler=dict(type='IoU3DBalancedSampler')))
    head2 = _head(g16, train_cfg=type('Cfg', (), dict(iou3d_sampler=dict(type='IoU3DBalancedSampler')))())
    assert head.iou3d_sampler is not None and head2.iou3d_sampler is not None and _head(g16).iou3d_sampler is None
    u = torch.from_numpy(g16['sampler_u'])
    monkeypatch.setattr(torch, 'rand_like', lambda t, **k: u.clone())
    ious, scores = torch.from_numpy(g16['sampler_ious_many_pos']), torch.from_numpy(g16['loss_scores'])
    want_w, want_t = torch.from_numpy(g16['loss_sampled_weight']), torch.from_numpy(g16['loss_sampled_targets'])
    mask = head.iou3d_sampler.sample(ious).to(ious.dtype)
    torch.testing.assert_close(mask / mask.mean().clamp(min=1e-2), want_w)
    loss = head.loss(scores, ious.clone())['loss_score']
    torch.testing.assert_close(loss, (F.binary_cross_entropy_with_logits(scores.unsqueeze(1), want_t, reduction='none') * want_w).mean())


def test_empty_loss_is_a_zero_with_a_graph(g16):
    head = _head(g16)
    scores = torch.zeros(0, requires_grad=True)
    loss = head.loss(scores, torch.zeros(0, 1))['loss_score']
    assert float(loss.detach()) == 0.0 and loss.requires_grad
    loss.backward()
    assert scores.grad is not None and scores.grad.shape == (0,)


def test_sampler_keeprate_and_masks_match_g16(g16, monkeypatch):
    from monorun_amd.score_head import IoU3DBalancedSampler, build_iou3d_sampler
    u = torch.from_numpy(g16['sampler_u'])
    monkeypatch.setattr(torch, 'rand_like', lambda t, **k: u.clone())
    for smooth in (True, False):
        for name in ('all_kept', 'many_pos', 'many_neg'):
            tag = f'sampler_{"smooth" if smooth else "step"}_{name}'
            ious = torch.from_numpy(g16[f'sampler_ious_{name}'])
            s = build_iou3d_sampler(dict(type='IoU3DBalancedSampler', smooth_keeprate=smooth))
            assert isinstance(s, IoU3DBalancedSampler)
            rate = s.keeprate(ious)
            if bool(g16[tag + '_kept_all']):
                assert rate is None, tag
            else:
                np.testing.assert_allclose(rate.numpy(), g16[tag + '_keeprate'], rtol=1e-6, atol=1e-7, err_msg=tag)
            assert np.array_equal(s.sample(ious).numpy(), g16[tag + '_mask']), tag
            s_min = IoU3DBalancedSampler(smooth_keeprate=smooth, min_iou=0.2)
            assert np.array_equal(s_min.sample(ious).numpy(), g16[tag + '_mask_min_iou']), tag
    assert bool(g16['sampler_smooth_all_kept_kept_all']) and bool(g16['sampler_smooth_all_kept_mask'].all())
    with pytest.raises(ValueError):
        build_iou3d_sampler(dict(type='NoSuchSampler'))


def test_smooth_keeprate_is_not_clamped(g16):
    """The reference computes a clamp of the smooth rate and discards it: a G16 case has rates outside [min, max] of the two
    classes' rates, and this implementation reproduces them."""
    from monorun_amd.score_head import IoU3DBalancedSampler
    ious = torch.from_numpy(g16['sampler_ious_many_pos'])
    ref = g16['sampler_smooth_many_pos_keeprate']
    step = g16['sampler_step_many_pos_keeprate']                      # the two classes' rates themselves
    lo, hi = step.min(), step.max()
    assert ref.max() > hi + 1e-3 and ref.min() < lo - 1e-3
    rate = IoU3DBalancedSampler().keeprate(ious).numpy()
    assert rate.max() > hi + 1e-3 and rate.min() < lo - 1e-3


def test_cross_entropy_loss_is_bce_with_logits():
    from monorun_amd.losses import CrossEntropyLoss, build_loss, LOSSES
    g = torch.Generator().manual_seed(5)
    pred, target, w = torch.randn(9, 1, generator=g), torch.rand(9, 1, generator=g), torch.rand(9, generator=g)
    raw = F.binary_cross_entropy_with_logits(pred, target, reduction='none')
    loss = CrossEntropyLoss(use_sigmoid=True, loss_weight=2.0)
    torch.testing.assert_close(loss(pred, target), 2.0 * raw.mean())
    torch.testing.assert_close(loss(pred, target, weight=w), 2.0 * (raw * w[:, None]).mean())             # per sample: (9,) against (9, 1)
    torch.testing.assert_close(loss(pred, target, weight=w[:, None]), 2.0 * (raw * w[:, None]).mean())
    torch.testing.assert_close(loss(pred, target, weight=w, avg_factor=4.0), 2.0 * (raw * w[:, None]).sum() / 4.0)
    torch.testing.assert_close(loss(pred, target, avg_factor=3.0), 2.0 * raw.sum() / 3.0)
    torch.testing.assert_close(loss(pred, target, reduction_override='sum'), 2.0 * raw.sum())
    assert loss(pred, target, weight=w, reduction_override='none').shape == (9, 1)
    with pytest.raises(NotImplementedError):
        CrossEntropyLoss(use_sigmoid=False)
    built = build_loss(dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0))                  # the reference's loss_score dict
    assert isinstance(built, CrossEntropyLoss) and LOSSES['CrossEntropyLoss'] is CrossEntropyLoss
    torch.testing.assert_close(built(pred, target), raw.mean())


def test_loader_binds_the_heads_header():
    """What is the score head's own; test_capi_and_host.py::test_loader_binds_every_header has what holds for every header."""
    from monorun_amd import _lib
    names = _lib.arg_names('mr_score_head_forward')
    assert len(_lib.load().mr_score_head_forward.argtypes) == 19 and len(names) == 18                # stream last, not among the names
    assert _lib.pack('mr_score_head_forward', **{n: k for k, n in enumerate(names)}) == list(range(18))
    assert _lib.arg_names('mr_uncert_projection')[0] == 'coords_3d'                                  # both headers answer by name
    assert '#define MR_SCORE_SIGMOID 0x1' in open(_lib.header_path('heads')).read() and _lib.MR_SCORE_SIGMOID == 1


def test_entry_point_rejects_bad_arguments_without_a_gpu():
    """Bad arguments are rejected before any HIP call, so this runs on the CPU."""
    from monorun_amd import _lib
    from monorun_amd.score_head import packed_numel
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    good = dict(reg_fc_out=p, reg_fc_out_row_stride=96, yaw=p, yaw_row_stride=1, t_vec=p, t_vec_row_stride=3, pose_cov=p, dimensions=p,
                dimensions_row_stride=3, ret_val=None, scores_2d=None, params=p, params_numel=packed_numel(96, 40), n=4, c1=96, c2=40,
                flags=1, scores=p)

    def call(**kw):
        a = dict(good, **kw)
        if 'params_numel' not in kw:
            a['params_numel'] = packed_numel(max(a['c1'], 0), max(a['c2'], 0))
        return lib.mr_score_head_forward(*_lib.pack('mr_score_head_forward', **a), None)
    assert call(n=0) == 0                                                                            # launches nothing
    assert call(n=0, reg_fc_out=None, scores=None) == 0
    bad = [dict(n=-1), dict(c1=0), dict(c1=2049), dict(c2=0), dict(c2=1025), dict(reg_fc_out_row_stride=95), dict(yaw_row_stride=0),
           dict(t_vec_row_stride=2), dict(dimensions_row_stride=2), dict(flags=2), dict(flags=3), dict(flags=-1), dict(params_numel=packed_numel(96, 40) - 1),
           dict(params=p + 4)]
    bad += [{k: None} for k in ('reg_fc_out', 'yaw', 't_vec', 'pose_cov', 'dimensions', 'params', 'scores')]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert call(c1=2048, c2=1024, reg_fc_out_row_stride=2048, n=0) == 0                              # the limits themselves are in range
    assert b'argument' in lib.mr_pnp_error_string(-1)


def test_packed_parameters_follow_the_header_layout(g16):
    from monorun_amd.score_head import pack_params, packed_numel, ROWS_PER_WORKGROUP
    assert ROWS_PER_WORKGROUP == 4
    head = _head(g16).eval()
    buf = head.packed_params('cpu')
    assert buf.dtype == torch.float32 and buf.numel() == packed_numel(C1, C2) == 64 + 17 * 96 + 96 + 96 * 40 + 2 * 40 + 4
    assert packed_numel(1, 1) == 64 + 20 + 4 + 4 + 8 + 4 and packed_numel(70, 33) == 64 + 1192 + 72 + 70 * 36 + 72 + 4
    n = head.pose_norm
    assert torch.equal(buf[:17], n.running_mean) and torch.equal(buf[34:51], n.bias) and float(buf[51:64].abs().max()) == 0
    torch.testing.assert_close(buf[17:34], n.weight / (n.running_var + n.eps).sqrt())
    assert torch.equal(buf[64:64 + 17 * 96].view(17, 96), head.pose_fcs[0].weight.t())
    o = 64 + 17 * 96 + 96
    assert torch.equal(buf[o:o + 96 * 40].view(96, 40), head.fused_fcs[0].weight.t())
    assert float(buf[-4]) == float(head.fc_out.bias.detach()) and torch.equal(buf[-4 - 40:-4], head.fc_out.weight.reshape(-1))
    assert head.packed_params('cpu') is buf                                                          # cached
    with torch.no_grad():
        head.fc_out.bias.add_(1.0)                                                                   # an optimizer step bumps _version
    new = head.packed_params('cpu')
    assert new is not buf and float(new[-4]) == float(head.fc_out.bias.detach())
    with torch.no_grad():
        head.pose_norm.running_var.mul_(2.0)                                                         # so does a buffer update
    assert head.packed_params('cpu') is not new
    plain = _head_without_norm()
    b = pack_params(plain, 'cpu')
    assert float(b[:17].abs().max()) == 0 and bool((b[17:34] == 1).all()) and float(b[34:64].abs().max()) == 0
    from monorun_amd.score_head import MLPScoreHead
    for kw in (dict(fusion_type='concat'), dict(num_pose_fcs=2), dict(num_fused_fcs=2)):
        h = MLPScoreHead(reg_fc_out_channels=8, pose_fc_out_channels=8, fc_out_channels=4, **kw)
        assert not h.fused_ok()
        with pytest.raises(ValueError):
            pack_params(h, 'cpu')
    assert MLPScoreHead().fused_ok() and plain.fused_ok()


def _head_without_norm():
    from monorun_amd.score_head import MLPScoreHead
    return MLPScoreHead(reg_fc_out_channels=8, pose_fc_out_channels=8, fc_out_channels=4, use_pose_norm=False)


def test_score_poses_on_cpu_is_the_roi_head_sequence(g16):
    from monorun_amd.score_head import score_poses
    head = _head(g16).eval()
    reg, yaw, t_vec, cov, dims = _inputs(g16, 'A')
    ret_val = torch.ones(24, dtype=torch.bool)
    ret_val[[2, 7]] = False
    cov_pred = cov * 0.5
    det = torch.rand(24, generator=torch.Generator().manual_seed(1))
    res = dict(ret_val=ret_val, yaw_pred=yaw, t_vec_pred=t_vec, pose_cov_pred=cov_pred, pose_cov_calib=cov, dimensions_pred=dims)
    with torch.no_grad():
        for calib in (True, False):
            for mult in (True, False):
                # monorun_roi_head.py:536-550, step by step
                scores = head(reg, yaw, t_vec, cov if calib else cov_pred, dims)
                scores.sigmoid_()
                scores[~ret_val] = 0
                want = det * scores if mult else scores
                got = score_poses(head, reg, res, det_scores=det, calib_scoring=calib, mult_2d_score=mult)
                assert got.shape == (24,) and torch.equal(got, want), (calib, mult)
                assert float(got[2]) == 0 and float(got[7]) == 0
        assert torch.equal(score_poses(head, reg, res, dimensions=dims * 1.1, det_scores=det),
                           det * head(reg, yaw, t_vec, cov, dims * 1.1).sigmoid().masked_fill(~ret_val, 0))
    with pytest.raises(ValueError):
        score_poses(head, reg, res)                                                                  # mult_2d_score without det_scores


@pytest.mark.skipif(torch.cuda.is_available(), reason='only meaningful without a GPU')
def test_fused_launch_has_no_cpu_fallback(g16):
    from monorun_amd.score_head import ScoreHeadLaunch, score_head_forward_fused
    head = _head(g16).eval()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        score_head_forward_fused(head, *_inputs(g16, 'A'))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ScoreHeadLaunch(head, 4, 'cpu')
