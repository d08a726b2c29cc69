#!/usr/bin/env python3
"""G19: the global head (fc_extractor.py, fc_extractor_monte_carlo.py) and its dimension coder (multiclass_norm_dim_coder.py), from
the reference's own code.

Runs only in the authoring container (needs the reference tree, read-only; loaded by file path under the mmcv / mmdet stubs of
make_golden.py, nothing of it is copied).  The fixture is data: seeded inputs and what the reference's classes returned for them.

    python tests/golden/make_golden_global_head.py      # rewrites tests/golden/g19_global_head.npz

The ``F.dropout`` / ``F.dropout2d`` the reference module sees are a recording version: it draws ``torch.bernoulli(1 - p)`` (per
channel for dropout2d), stores the mask and returns ``input * (mask / (1 - p))``, so the fixture holds the masks its outputs belong
to.  Sizes: in_channels 6, RoI 3 x 3, F = 40, latent_channels 5, S = 7, n = 5.  Group a: 3 classes, not class-agnostic, labels
covering all three; group b: num_classes = 1, class-agnostic.  Recorded per group: the seeded parameters under the reference's
state_dict keys, x, the three masks, the eval 5-tuple, slice_pred in both modes, a training-mode get_targets / loss case (what the
head hands to a recording loss), and the coder's encode / decode.
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as mg  # noqa: E402

OUT = HERE
C, RH, F, LAT, S, N = 6, 3, 40, 5, 7, 5
P, P2D = 0.5, 0.2


class _RecordingLoss:
    def __init__(self):
        self.calls = []

    def __call__(self, pred, target):
        self.calls.append((pred.detach().clone(), target.detach().clone()))
        return (pred - target).abs().sum()


class _RecordingDropout:
    """Stands in for torch.nn.functional inside the reference module: dropout / dropout2d draw a Bernoulli keep mask, keep it and
    scale the kept elements."""

    def __init__(self):
        self.masks = []

    def dropout(self, input, p, training, inplace):
        assert training
        mask = torch.bernoulli(torch.full_like(input, 1 - p))
        self.masks.append(mask.bool())
        return input * (mask / (1 - p))

    def dropout2d(self, input, p, training, inplace):
        assert training and input.dim() == 4
        mask = torch.bernoulli(torch.full((input.size(0), input.size(1), 1, 1), 1 - p, dtype=input.dtype))
        self.masks.append(mask.bool()[:, :, 0, 0])
        return input * (mask / (1 - p))


def load():
    mg.install_stubs()
    for p in ('monorun', 'monorun.core', 'monorun.core.bbox_3d', 'monorun.core.bbox_3d.dim_coder', 'monorun.models', 'monorun.models.roi_heads',
              'monorun.models.roi_heads.bbox_3d_heads', 'monorun.models.roi_heads.bbox_3d_heads.global_extractors'):
        mg._pkg(p)
    bld = mg._load('monorun.core.bbox_3d.builder', 'core/bbox_3d/builder.py')
    coder = mg._load('monorun.core.bbox_3d.dim_coder.multiclass_norm_dim_coder', 'core/bbox_3d/dim_coder/multiclass_norm_dim_coder.py')
    sys.modules['monorun.core'].build_dim_coder = lambda cfg: mg._build_from_cfg(cfg, bld.DIM_CODERS)
    sys.modules['mmdet.models.builder'].build_loss = lambda cfg: _RecordingLoss()
    base = 'monorun.models.roi_heads.bbox_3d_heads.global_extractors.'
    mg._load(base + 'fc_extractor', 'models/roi_heads/bbox_3d_heads/global_extractors/fc_extractor.py')
    mc = mg._load(base + 'fc_extractor_monte_carlo', 'models/roi_heads/bbox_3d_heads/global_extractors/fc_extractor_monte_carlo.py')
    return mc, coder


def main():
    mc, coder_mod = load()
    rng = np.random.default_rng(1919)
    torch.manual_seed(1919)
    out = {}
    rec = _RecordingDropout()
    mc.F = rec                                                      # the module's `F.dropout` / `F.dropout2d`

    for tag, kw in (('a', dict(num_classes=3, latent_class_agnostic=False)), ('b', dict(num_classes=1, latent_class_agnostic=True))):
        head = mc.FCExtractorMonteCarlo(num_samples=S, dropout_rate=P, dropout2d_rate=P2D, in_channels=C, roi_feat_size=RH,
                                        fc_out_channels=F, latent_channels=LAT, loss_dim=dict(type='SmoothL1LossMod', loss_weight=1.0, beta=1.0),
                                        dim_coder=dict(type='MultiClassNormDimCoder'), **kw)
        head.init_weights()
        with torch.no_grad():                                       # the init's weights are small: scale them so that relu cuts about half
            for fc in head.fcs:
                fc.weight.mul_(6.0)
                fc.bias.normal_(0, 0.3)
            head.fc_reg.weight.normal_(0, 0.3)
            head.fc_reg.bias.normal_(0, 0.2)
        out[f'{tag}_state_dict'] = np.array(json.dumps([[k, list(v.shape)] for k, v in head.state_dict().items()]))
        for k, v in head.state_dict().items():
            out[f'{tag}_param.{k}'] = v.numpy().copy()
        x = torch.from_numpy(rng.normal(0, 1, (N, C, RH, RH)).astype(np.float32))
        labels = torch.tensor([0, 1, 2, 1, 0]) if tag == 'a' else torch.zeros(N, dtype=torch.long)
        out[f'{tag}_x'], out[f'{tag}_labels'] = x.numpy(), labels.numpy()

        head.eval()
        rec.masks.clear()
        with torch.no_grad():
            mean, var, d1, d2, reg = head(x)
        assert d1 is None and d2 is None and len(rec.masks) == 3
        out[f'{tag}_keep0'] = rec.masks[0].reshape(S, N, C).numpy()
        out[f'{tag}_keep1'] = rec.masks[1].reshape(S, N, F).numpy()
        out[f'{tag}_keep2'] = rec.masks[2].reshape(S, N, F).numpy()
        out[f'{tag}_mean'], out[f'{tag}_var'], out[f'{tag}_reg_fc_out'] = mean.numpy(), var.numpy(), reg.numpy()
        sl = head.slice_pred(mean, var, labels)
        for name, v in zip(('dim_pred', 'dim_var', 'latent_pred', 'latent_var'), sl):
            out[f'{tag}_eval_slice_{name}'] = v.numpy()

        head.train()
        sl = head.slice_pred(mean, None, labels)
        assert sl[1] is None and sl[3] is None
        out[f'{tag}_train_slice_dim_pred'], out[f'{tag}_train_slice_latent_pred'] = sl[0].numpy(), sl[2].numpy()

        # a training-mode get_targets / loss case: two images, 3 + 2 positives
        gt_boxes = [torch.from_numpy(rng.uniform([1.0, 1.2, 0.5, -10, 1, 5, -3], [4.5, 1.9, 1.8, 10, 2, 40, 3], (4, 7)).astype(np.float32)),
                    torch.from_numpy(rng.uniform([1.0, 1.2, 0.5, -10, 1, 5, -3], [4.5, 1.9, 1.8, 10, 2, 40, 3], (3, 7)).astype(np.float32))]
        ncls = kw['num_classes']
        gt_labels = [torch.from_numpy(rng.integers(0, ncls, 4)), torch.from_numpy(rng.integers(0, ncls, 3))]
        inds = [torch.tensor([2, 0, 3]), torch.tensor([1, 1])]
        sampling = [types.SimpleNamespace(pos_assigned_gt_inds=i) for i in inds]
        targets, dist = head.get_targets(sampling, gt_boxes, gt_labels)
        assert dist is None
        for j in range(2):
            out[f'{tag}_gt_boxes{j}'], out[f'{tag}_gt_labels{j}'], out[f'{tag}_pos_inds{j}'] = gt_boxes[j].numpy(), gt_labels[j].numpy(), inds[j].numpy()
        out[f'{tag}_dim_targets'] = targets.numpy()
        loss = head.loss(sl[0], None, None, targets, None)
        (lp, lt), = head.loss_dim.calls
        assert torch.equal(lp, sl[0]) and torch.equal(lt, targets) and set(loss) == {'loss_dim'}
        empty = head.loss(sl[0][:0], None, None, targets[:0], None)['loss_dim']
        assert float(empty) == 0 and len(head.loss_dim.calls) == 1

    # the coder
    cd = coder_mod.MultiClassNormDimCoder()
    dims = torch.from_numpy(rng.uniform(0.5, 4.5, (6, 3)).astype(np.float32))
    lab = torch.tensor([0, 1, 2, 2, 1, 0])
    enc = cd.encode(dims, lab)
    dv = torch.from_numpy(rng.uniform(0.01, 2, (6, 3)).astype(np.float32))
    dec, dec_var = cd.decode(enc, dv, lab)
    assert cd.decode(enc, None, lab)[1] is None
    out['coder_dims'], out['coder_labels'], out['coder_encoded'] = dims.numpy(), lab.numpy(), enc.numpy()
    out['coder_var'], out['coder_decoded'], out['coder_decoded_var'] = dv.numpy(), dec.numpy(), dec_var.numpy()

    path = os.path.join(OUT, 'g19_global_head.npz')
    np.savez_compressed(path, **out)
    print('G19: mean', out['a_mean'][0, :4], 'var', out['a_var'][0, :4], 'kept', [float(out[f'a_keep{k}'].mean()) for k in range(3)],
          os.path.getsize(path) // 1024, 'KiB')


if __name__ == '__main__':
    main()
