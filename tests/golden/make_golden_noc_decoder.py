#!/usr/bin/env python3
"""G20: the NOC head's trunk (fcn_noc_decoder.py), from the reference's own ``FCNNOCDecoder``.

Runs only in the authoring container (needs the reference tree, read-only; loaded by file path under the mmcv / mmdet stubs of
make_golden.py, nothing of it is copied).  The fixture is data: seeded parameters and inputs and what the reference's class returned.

    python tests/golden/make_golden_noc_decoder.py      # rewrites tests/golden/g20_noc_decoder.npz

mmcv does not import here, so the three mmcv names the reference module uses are this maker's own: ``ConvModule`` is a conv + ReLU with
a ``.conv`` attribute, ``build_upsample_layer`` builds ``nn.Upsample`` or the ``CARAFEPack`` stand-in below, and ``mmcv.ops.Conv2d`` is
``nn.Conv2d``.  THE CARAFE ARITHMETIC INSIDE THIS FIXTURE THEREFORE COMES FROM THE STAND-IN (two convolutions, pixel shuffle, softmax
over the taps, an unfold-based reassembly written from the op's definition), NOT FROM mmcv's CUDA op.  What G20 pins is the reference
class's wiring: dropout order, latent deformation, the n = 0 branch, flip / class selection and the state-dict keys.  The op itself is
pinned against mmcv by make_golden_carafe_mmcv.py where that binary exists.

``nn.Dropout2d`` inside the reference module is a recording version (as G19's): it draws a Bernoulli keep mask per (RoI, channel), stores
it and returns ``input * (mask / (1 - p))``.  Sizes: in_channels 6, conv_out 8, compressed 4, RoI 5 x 4, latent 5, n = 5, 2 convs (a
dropout after the first as well: num_dropout2d_layers = 2), 1 upsampled conv.  Group a: 3 classes, labels covering all three; group b:
class-agnostic.  Recorded per group: the parameters under the reference's keys (scaled so that the ReLUs cut about half and the softmax is
not near-uniform), x, latent, labels, a per-RoI flip list and a bool flip, the eval 4-tuple for both, one training-mode forward with its
masks, and the n = 0 result shapes.
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as mg  # noqa: E402

OUT = HERE
CIN, CO, CC, RH, RW, LAT, N = 6, 8, 4, 5, 4, 5, 5
P2D = 0.2


class ConvModule(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, padding=0, conv_cfg=None, norm_cfg=None):
        super().__init__()
        assert conv_cfg is None and norm_cfg is None
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, padding=padding)

    def forward(self, x):
        return F.relu(self.conv(x))


class CARAFEPack(nn.Module):
    """The stand-in: mmcv's constructor arguments and parameter names; the op from its definition, by unfold."""

    def __init__(self, channels, scale_factor, up_kernel=5, up_group=1, encoder_kernel=3, encoder_dilation=1, compressed_channels=64):
        super().__init__()
        self.channels, self.scale_factor, self.up_kernel, self.up_group = channels, scale_factor, up_kernel, up_group
        self.channel_compressor = nn.Conv2d(channels, compressed_channels, 1)
        self.content_encoder = nn.Conv2d(compressed_channels, up_kernel * up_kernel * up_group * scale_factor * scale_factor, encoder_kernel,
                                         padding=int((encoder_kernel - 1) * encoder_dilation / 2), dilation=encoder_dilation)

    def init_weights(self):
        for m in (self.channel_compressor, self.content_encoder):
            nn.init.xavier_uniform_(m.weight)
            nn.init.constant_(m.bias, 0)
        nn.init.normal_(self.content_encoder.weight, 0, 0.001)

    def forward(self, x):
        k, G, s = self.up_kernel, self.up_group, self.scale_factor
        n, c, h, w = x.shape
        mask = F.pixel_shuffle(self.content_encoder(self.channel_compressor(x)), s)
        mask = F.softmax(mask.view(n, G, k * k, h * s, w * s), dim=2)
        cols = F.unfold(x, k, padding=(k - 1) // 2).view(n, c * k * k, h, w)                       # (n, c k^2, h, w): channel c, tap t
        cols = F.interpolate(cols, scale_factor=s, mode='nearest').view(n, G, c // G, k * k, h * s, w * s)
        return (cols * mask[:, :, None]).sum(3).view(n, c, h * s, w * s)


def build_upsample_layer(cfg):
    cfg = dict(cfg)
    typ = cfg.pop('type')
    if typ == 'carafe':
        return CARAFEPack(**cfg)
    assert typ in ('nearest', 'bilinear')
    return nn.Upsample(**cfg)


class RecordingDropout2d(nn.Module):
    masks = []

    def __init__(self, p):
        super().__init__()
        self.p = p

    def forward(self, x):
        if not self.training:
            return x
        mask = torch.bernoulli(torch.full((x.size(0), x.size(1), 1, 1), 1 - self.p, dtype=x.dtype))
        RecordingDropout2d.masks.append(mask.bool()[:, :, 0, 0])
        return x * (mask / (1 - self.p))


def load():
    mg.load_reference()
    sys.modules['mmcv.cnn'].ConvModule = ConvModule
    sys.modules['mmcv.cnn'].build_upsample_layer = build_upsample_layer
    sys.modules['mmcv.ops'].Conv2d = nn.Conv2d
    sys.modules['mmcv.ops.carafe'].CARAFEPack = CARAFEPack
    return mg._load('monorun.models.roi_heads.bbox_3d_heads.dense_decoders.fcn_noc_decoder_g20',
                    'models/roi_heads/bbox_3d_heads/dense_decoders/fcn_noc_decoder.py')


def main():
    mod = load()
    mod.nn = type('nn', (), dict(vars(nn), Dropout2d=RecordingDropout2d))            # the module's `nn.Dropout2d`
    rng = np.random.default_rng(2020)
    torch.manual_seed(2020)
    out = {}
    for tag, kw in (('a', dict(num_classes=3, class_agnostic=False)), ('b', dict(num_classes=3, class_agnostic=True))):
        head = mod.FCNNOCDecoder(num_convs=2, roi_feat_size=(RH, RW), in_channels=CIN, conv_out_channels=CO, num_convs_upsampled=1,
                                 upsample_cfg=dict(type='carafe', scale_factor=2, up_kernel=5, up_group=1, encoder_kernel=3, encoder_dilation=1,
                                                   compressed_channels=CC),
                                 dropout2d_rate=P2D, num_dropout2d_layers=2, latent_channels=LAT, **kw)
        head.init_weights()
        with torch.no_grad():           # the inits leave the deformation at zero and the masks near-uniform: give every parameter a size that matters
            for p in head.parameters():
                p.normal_(0, 0.35)
            head.upsample.content_encoder.weight.mul_(2.0)
        out[f'{tag}_state_dict'] = np.array(json.dumps([[k, list(v.shape)] for k, v in head.state_dict().items()]))
        for k, v in head.state_dict().items():
            out[f'{tag}_param.{k}'] = v.numpy().copy()
        x = torch.from_numpy(rng.normal(0, 1, (N, CIN, RH, RW)).astype(np.float32))
        latent = torch.from_numpy(rng.normal(0, 1, (N, LAT)).astype(np.float32))
        labels = torch.tensor([0, 1, 2, 1, 0])
        flips = [False, True, True, False, True]
        out[f'{tag}_x'], out[f'{tag}_latent'], out[f'{tag}_labels'], out[f'{tag}_flips'] = x.numpy(), latent.numpy(), labels.numpy(), np.array(flips)

        head.eval()
        with torch.no_grad():
            for name, flip in (('list', flips), ('true', True), ('false', False)):
                noc, var, ls, reg = head(x, latent, None, labels, flip=flip)
                assert var is None and reg is None
                out[f'{tag}_eval_{name}_noc'], out[f'{tag}_eval_{name}_logstd'] = noc.numpy(), ls.numpy()
            # how much the ReLUs cut and how peaked the softmax is, for the record
            h1 = head.convs[0].conv(x)
            print(f'G20 {tag}: relu keeps {float((h1 > 0).float().mean()):.2f} of conv 0')
            e = head(x[:0], latent[:0], None, labels[:0], flip=False)
            out[f'{tag}_empty_shapes'] = np.array([list(e[0].shape), list(e[2].shape)])
        head.train()
        RecordingDropout2d.masks.clear()
        with torch.no_grad():
            noc, var, ls, reg = head(x, latent, None, labels, flip=flips)
        assert len(RecordingDropout2d.masks) == 2
        out[f'{tag}_train_keep0'], out[f'{tag}_train_keep1'] = (m.numpy() for m in RecordingDropout2d.masks)
        out[f'{tag}_train_noc'], out[f'{tag}_train_logstd'] = noc.numpy(), ls.numpy()

    path = os.path.join(OUT, 'g20_noc_decoder.npz')
    np.savez_compressed(path, **out)
    print('G20:', out['a_eval_list_noc'][0, :, 0, 0], os.path.getsize(path) // 1024, 'KiB')


if __name__ == '__main__':
    main()
