"""G20 (tests/golden/g20_noc_decoder.npz, made by tests/golden/make_golden_noc_decoder.py from the reference's FCNNOCDecoder) and the
decoder built for it, shared by test_noc_decoder_cpu.py and test_gpu_noc_decoder.py."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g20_noc_decoder.npz')
CIN, CO, CC, RH, RW, LAT, N = 6, 8, 4, 5, 4, 5, 5
GROUPS = {'a': dict(num_classes=3, class_agnostic=False), 'b': dict(num_classes=3, class_agnostic=True)}


def load():
    return np.load(GOLDEN)


def state_dict(g, tag):
    keys = [k for k, _ in json.loads(str(g[f'{tag}_state_dict']))]
    return {k: torch.from_numpy(g[f'{tag}_param.{k}'].copy()) for k in keys}


def build(g, tag, **over):
    """The decoder of group `tag` with the fixture's parameters, loaded strictly"""
    from monorun_amd.noc_decoder import FCNNOCDecoder
    kw = dict(num_convs=2, roi_feat_size=(RH, RW), in_channels=CIN, conv_out_channels=CO, num_convs_upsampled=1,
              upsample_cfg=dict(type='carafe', scale_factor=2, up_kernel=5, up_group=1, encoder_kernel=3, encoder_dilation=1, compressed_channels=CC),
              dropout2d_rate=0.2, num_dropout2d_layers=2, latent_channels=LAT, **GROUPS[tag])
    kw.update(over)
    head = FCNNOCDecoder(**kw)
    head.load_state_dict(state_dict(g, tag), strict=True)
    return head


def inputs(g, tag, device='cpu'):
    x, latent, labels = (torch.from_numpy(g[f'{tag}_{n}'].copy()).to(device) for n in ('x', 'latent', 'labels'))
    return x, latent, labels, [bool(f) for f in g[f'{tag}_flips']]


class FixedDropout2d(torch.nn.Module):
    """Dropout2d on recorded keep masks (n, channels), one per call in order: input * (keep / (1 - p)) in training mode"""

    def __init__(self, p, masks):
        super().__init__()
        self.p, self.masks, self.calls = p, masks, 0

    def forward(self, x):
        if not self.training:
            return x
        keep = self.masks[self.calls].to(device=x.device, dtype=x.dtype)[:, :, None, None]
        self.calls += 1
        return x * (keep / (1 - self.p))


def with_recorded_masks(head, g, tag):
    head.dropout2d = FixedDropout2d(0.2, [torch.from_numpy(g[f'{tag}_train_keep{i}'].copy()) for i in range(2)])
    return head
