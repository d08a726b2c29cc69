"""The global head on the CPU: FCExtractorMonteCarlo, FCExtractor and MultiClassNormDimCoder against G19
(tests/golden/g19_global_head.npz: what the reference's own classes returned under recorded dropout masks,
tests/golden/make_golden_global_head.py), the numpy reference the GPU tests use against G19, the mask draws, the loader's binding of
include/monorun_global.h and the entry point's argument checks.  No GPU."""
import ctypes
import json
import os
import types

import numpy as np
import pytest
import torch

from tests import global_head_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, RH, F, LAT, S, N = 6, 3, 40, 5, 7, 5
GROUPS = {'a': dict(num_classes=3, latent_class_agnostic=False), 'b': dict(num_classes=1, latent_class_agnostic=True)}
KEYS = ['fcs.0.weight', 'fcs.0.bias', 'fcs.1.weight', 'fcs.1.bias', 'fc_reg.weight', 'fc_reg.bias']


@pytest.fixture(scope='module')
def g19():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'g19_global_head.npz')))


def _head(g19, tag, **kw):
    from monorun_amd.global_head import FCExtractorMonteCarlo
    head = FCExtractorMonteCarlo(num_samples=S, in_channels=C, roi_feat_size=RH, fc_out_channels=F, latent_channels=LAT,
                                 loss_dim=dict(type='SmoothL1LossMod', loss_weight=1.0, beta=1.0), dim_coder=dict(type='MultiClassNormDimCoder'),
                                 **GROUPS[tag], **kw)
    sd = {k[len(tag) + 7:]: torch.from_numpy(v) for k, v in g19.items() if k.startswith(tag + '_param.')}
    assert list(sd) == KEYS                                          # the fixture holds the reference's keys in its order
    head.load_state_dict(sd, strict=True)
    return head


def _masks(g19, tag):
    return [torch.from_numpy(g19[f'{tag}_keep{k}']) for k in range(3)]


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_state_dict_has_the_reference_keys_shapes_and_order(g19, tag):
    head = _head(g19, tag)
    want = json.loads(str(g19[f'{tag}_state_dict']))
    assert [[k, list(v.shape)] for k, v in head.state_dict().items()] == want and [k for k, _ in want] == KEYS
    from monorun_amd.global_head import FCExtractor, FCExtractorMonteCarlo
    default = FCExtractorMonteCarlo()                                # the reference's defaults: 256 x 7 x 7 -> 1024 -> 1024 -> 19 * 3
    assert [(k, tuple(v.shape)) for k, v in default.state_dict().items()] == [
        ('fcs.0.weight', (1024, 12544)), ('fcs.0.bias', (1024,)), ('fcs.1.weight', (1024, 1024)), ('fcs.1.bias', (1024,)),
        ('fc_reg.weight', (57, 1024)), ('fc_reg.bias', (57,))]
    assert default.num_samples == 50 and default.dropout_rate == 0.5 and default.dropout2d_rate == 0.2 and default.num_dropout_layers == 2
    assert list(FCExtractor(in_channels=2, roi_feat_size=2, fc_out_channels=4).state_dict()) == KEYS
    default.init_weights()
    assert float(default.fc_reg.bias.detach().abs().max()) == 0 and 0.0005 < float(default.fc_reg.weight.detach().std()) < 0.002
    assert float(default.fcs[1].weight.detach().abs().max()) <= 0.33 * (6.0 / 2048) ** 0.5 and 0.01 < float(default.fcs[0].bias.detach().mean()) < 0.03


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_mc_forward_torch_on_the_recorded_masks_matches_g19(g19, tag):
    """both sides are fp32 sums in some order, possibly on different CPUs: within twice the bound B"""
    head = _head(g19, tag).eval()
    x, masks = torch.from_numpy(g19[tag + '_x']), _masks(g19, tag)
    with torch.no_grad():
        mean, var, d1, d2, reg, samples = head.mc_forward(x, masks, return_samples=True)
        assert not head.hip_ok(x) and d1 is None and d2 is None
    B = ref.bound(ref.params_of(head), x.numpy(), [m.numpy() for m in masks], 0.2, 0.5)
    Bm = B['samples'].max(0)                                         # a mean's or a centred sample's error is at most the samples' largest
    assert np.all(np.abs(reg.numpy() - g19[tag + '_reg_fc_out']) <= 2 * B['reg_fc_out'])
    assert np.all(np.abs(mean.numpy() - g19[tag + '_mean']) <= 2 * Bm)
    # var = sum d^2 / (S - 1), d = y - mean: |delta var| <= sum 2 |d| |delta d| / (S - 1) with |delta d| <= 2 * (2 Bm)
    y = samples.double().numpy()
    dev = np.abs(y - y.mean(0)).sum(0)
    assert np.all(np.abs(var.numpy() - g19[tag + '_var']) <= 2 * dev * 4 * Bm / (S - 1) + 1e-6 * g19[tag + '_var'])
    out = head(x)                                                    # eval forward: fresh masks, the 5-tuple
    assert len(out) == 5 and out[0].shape == (N, head.out_channels) and out[4].shape == (N, F) and out[2] is None and out[3] is None


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_numpy_reference_agrees_with_g19(g19, tag):
    head = _head(g19, tag)
    r = ref.mc_forward_ref(ref.params_of(head), g19[tag + '_x'], [g19[f'{tag}_keep{k}'] for k in range(3)], 0.2, 0.5)
    for key in ('mean', 'var', 'reg_fc_out'):
        want = g19[f'{tag}_{key}']
        assert np.abs(r[key] - want).max() <= 1e-5 * max(np.abs(want).max(), 1.0), key


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_slice_pred_get_targets_and_loss_match_g19(g19, tag):
    from monorun_amd.losses import SmoothL1LossMod, smooth_l1_loss_mod
    head = _head(g19, tag)
    mean, var, labels = torch.from_numpy(g19[tag + '_mean']), torch.from_numpy(g19[tag + '_var']), torch.from_numpy(g19[tag + '_labels'])
    head.eval()
    got = head.slice_pred(mean, var, labels)
    for name, v in zip(('dim_pred', 'dim_var', 'latent_pred', 'latent_var'), got):
        assert np.array_equal(v.numpy(), g19[f'{tag}_eval_slice_{name}']), name
    head.train()
    dim_pred, dim_var, latent, latent_var = head.slice_pred(mean, None, labels)
    assert dim_var is None and latent_var is None
    assert np.array_equal(dim_pred.numpy(), g19[tag + '_train_slice_dim_pred']) and np.array_equal(latent.numpy(), g19[tag + '_train_slice_latent_pred'])
    sampling = [types.SimpleNamespace(pos_assigned_gt_inds=torch.from_numpy(g19[f'{tag}_pos_inds{j}'])) for j in range(2)]
    boxes = [torch.from_numpy(g19[f'{tag}_gt_boxes{j}']) for j in range(2)]
    gt_labels = [torch.from_numpy(g19[f'{tag}_gt_labels{j}']) for j in range(2)]
    targets, dist = head.get_targets(sampling, boxes, gt_labels)
    assert dist is None and np.array_equal(targets.numpy(), g19[tag + '_dim_targets'])
    per_image, _ = head.get_targets(sampling, boxes, gt_labels, concat=False)
    assert [t.shape[0] for t in per_image] == [3, 2] and torch.equal(torch.cat(per_image), targets)
    assert isinstance(head.loss_dim, SmoothL1LossMod)
    loss = head.loss(dim_pred, None, None, targets, None)
    assert set(loss) == {'loss_dim'}
    torch.testing.assert_close(loss['loss_dim'], smooth_l1_loss_mod(dim_pred, targets, beta=1.0).mean())
    p0 = torch.zeros(0, 3, requires_grad=True)
    empty = head.loss(p0, None, None, targets[:0], None)['loss_dim']
    assert float(empty.detach()) == 0.0 and empty.requires_grad
    assert _head(g19, tag, with_dim=False).loss(dim_pred, None, None, targets, None) == dict()


def test_training_forward_is_the_plain_extractor(g19):
    head = _head(g19, 'a').train()
    x = torch.from_numpy(g19['a_x']).requires_grad_(True)
    torch.manual_seed(3)
    pred, var, d1, d2, feat = head(x)
    assert pred.shape == (N, 24) and var is None and d1 is None and d2 is None and feat.shape == (N, F) and pred.requires_grad
    torch.manual_seed(3)                                             # the same torch dropout draws: dropout2d, then one dropout per layer
    h = torch.nn.functional.dropout2d(x, 0.2, True).flatten(1)
    for fc in head.fcs:
        h = torch.nn.functional.dropout(torch.relu(fc(h)), 0.5, True)
    torch.testing.assert_close(pred, head.fc_reg(h))
    pred.sum().backward()
    assert x.grad is not None and head.fcs[0].weight.grad is not None


def test_dim_coder_matches_g19(g19):
    from monorun_amd.global_head import MultiClassNormDimCoder, build_dim_coder
    cd = build_dim_coder(dict(type='MultiClassNormDimCoder'))
    assert isinstance(cd, MultiClassNormDimCoder)
    dims, lab = torch.from_numpy(g19['coder_dims']), torch.from_numpy(g19['coder_labels'])
    enc = cd.encode(dims, lab)
    assert np.array_equal(enc.numpy(), g19['coder_encoded'])
    dec, dec_var = cd.decode(enc, torch.from_numpy(g19['coder_var']), lab)
    assert np.array_equal(dec.numpy(), g19['coder_decoded']) and np.array_equal(dec_var.numpy(), g19['coder_decoded_var'])
    assert cd.decode(enc, None, lab)[1] is None
    with pytest.raises(ValueError):
        build_dim_coder(dict(type='NoSuchCoder'))


def test_empty_batch_returns_the_reference_shapes(g19):
    head = _head(g19, 'a').eval()
    x = torch.zeros(0, C, RH, RH)
    mean, var, d1, d2, reg = head(x)
    assert mean.shape == (0, 24) and var.shape == (0, 24) and reg.shape == (0, F) and d1 is None and d2 is None
    assert head.mc_forward(x, return_samples=True)[5].shape == (S, 0, 24)
    t = head.mc_forward_torch(x, head.draw_masks(0, 'cpu'))
    assert t[0].shape == (0, 24) and t[1].shape == (0, 24) and t[4].shape == (0, F)


def test_draw_masks_shapes_seeds_and_rates():
    from monorun_amd.global_head import FCExtractorMonteCarlo
    head = FCExtractorMonteCarlo(num_samples=50, in_channels=32, roi_feat_size=2, fc_out_channels=128, dropout_rate=0.5, dropout2d_rate=0.2)
    n = 20
    masks = head.draw_masks(n, 'cpu', generator=torch.Generator().manual_seed(11))
    again = head.draw_masks(n, 'cpu', generator=torch.Generator().manual_seed(11))
    other = head.draw_masks(n, 'cpu', generator=torch.Generator().manual_seed(12))
    assert [tuple(m.shape) for m in masks] == [(50, n, 32), (50, n, 128), (50, n, 128)]
    assert all(m.dtype == torch.bool for m in masks)
    assert all(torch.equal(a, b) for a, b in zip(masks, again)) and not any(torch.equal(a, b) for a, b in zip(masks, other))
    assert not torch.equal(masks[1], masks[2])
    for m, rate in zip(masks, (0.8, 0.5, 0.5)):                      # the kept fraction within 5 binomial standard deviations of its rate
        sd = (rate * (1 - rate) / m.numel()) ** 0.5
        assert abs(float(m.float().mean()) - rate) <= 5 * sd, (rate, float(m.float().mean()))


def test_loader_binds_the_global_header():
    """What is the global head's own; test_capi_and_host.py::test_loader_binds_every_header has what holds for every header."""
    from monorun_amd import _lib, global_head
    assert len(_lib.load().mr_global_head_mc_forward.argtypes) == 25
    src = open(_lib.header_path('global')).read()
    assert '#define MR_GLOBAL_CHUNK 64' in src and '#define MR_GLOBAL_MAX_CHANNELS 8192' in src
    assert (global_head.CHUNK, global_head.MAX_CHANNELS, global_head.MAX_OUT, global_head.MAX_SAMPLES) == (64, 8192, 4096, 4096)


def test_entry_points_check_their_arguments_without_a_gpu():
    """Bad arguments are rejected before any HIP call, so this runs on the CPU."""
    from monorun_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    sizes = dict(n=4, in_channels=6, area=9, fc_channels=40, out_channels=24, num_samples=7)

    def nbytes(**kw):
        return lib.mr_global_head_mc_workspace_bytes(*_lib.pack('mr_global_head_mc_workspace_bytes', dict(sizes, **kw)))
    assert nbytes() == 4 * 4 * (6 * 40 + 2 * 7 * 40 + 7 * 24)
    assert nbytes(n=64) == nbytes(n=65) == nbytes(n=100000) == 16 * nbytes()            # one pass of 64 RoIs bounds it
    assert nbytes(n=0) == 0 and nbytes(n=-1) == 0 and nbytes(num_samples=1) == 0 and nbytes(in_channels=8193) == 0
    real = dict(n=1024, in_channels=256, area=49, fc_channels=1024, out_channels=57, num_samples=50)        # the real head at n = 1024
    assert nbytes(**real) == 4 * 64 * (256 * 1024 + 2 * 50 * 1024 + 50 * 57)
    ptrs = ('x', 'w1', 'b1', 'w2', 'b2', 'w_reg', 'b_reg', 'keep0', 'keep1', 'keep2', 'workspace', 'mean', 'var', 'reg_fc_out')
    good = dict(sizes, q0=1.25, q1=2.0, workspace_bytes=nbytes(), samples=None, **{k: p for k in ptrs})

    def call(**kw):
        a = dict(good, **kw)
        if 'workspace_bytes' not in kw:
            a['workspace_bytes'] = max(nbytes(**{k: a[k] for k in sizes}), 4)
        return lib.mr_global_head_mc_forward(*_lib.pack('mr_global_head_mc_forward', a), None)
    assert call(n=0) == 0                                                               # launches nothing
    assert call(n=0, x=None, mean=None, workspace=None, workspace_bytes=0) == 0
    bad = [dict(n=-1), dict(in_channels=0), dict(area=0), dict(fc_channels=0), dict(out_channels=0), dict(num_samples=1), dict(num_samples=0),
           dict(num_samples=-3), dict(workspace_bytes=nbytes() - 1), dict(workspace_bytes=0), dict(workspace=p + 2)]
    bad += [{k: None} for k in ptrs]
    for kw in bad:
        assert call(**kw) == -1, kw
    unsupported = [dict(in_channels=8193), dict(area=8193), dict(fc_channels=8193), dict(out_channels=4097), dict(num_samples=4097),
                   dict(n=2 ** 31 - 1), dict(in_channels=8192, area=8192, fc_channels=64), dict(n=20000, num_samples=4096, fc_channels=64)]
    for kw in unsupported:
        code = call(n=0, **kw) if 'n' not in kw else call(**kw)
        assert code == -2, kw
    assert call(**dict(real, n=0)) == 0 and call(n=0, in_channels=8192, area=1, fc_channels=8192, out_channels=4096, num_samples=4096) == 0
    assert b'unsupported' in lib.mr_pnp_error_string(-2)
