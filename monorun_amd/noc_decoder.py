"""The NOC head's trunk (N10): ``FCNNOCDecoder`` of the reference
(monorun/models/roi_heads/bbox_3d_heads/dense_decoders/fcn_noc_decoder.py), without mmcv / mmdet.  It produces ``all_pred``, the raw
output that ``pose_head.noc_decode`` (inference) and ``noc_head.decode_for_training`` (training) decode.

The convolutions are torch's (MIOpen on a HIP device); the upsampler every shipped config selects, CARAFE, is
:class:`monorun_amd.carafe.CARAFEPack`, whose normaliser and reassembly are one fused HIP launch (``mr_carafe_pack_forward``).
``upsample_cfg['type']`` may also be ``'nearest'``, ``'bilinear'`` or ``None``; ``'deconv'`` and ``plugins`` raise
``NotImplementedError`` (both need mmcv's builders, and the reference's deconv branch calls a ``self.relu`` it never defines).

State-dict keys are the reference's (``convs.{i}.conv.*``, ``latent_decoder.*``, ``upsample.channel_compressor.*``,
``upsample.content_encoder.*``, ``convs_upsampled.{i}.conv.*``, ``conv_final.*``), so the ``noc_head.*`` slice of a MonoRUn checkpoint
loads with ``strict=True``.
"""
import torch
import torch.nn as nn
from torch.nn.modules.utils import _pair

from . import noc_head as _noc_head
from .carafe import CARAFEPack, carafe_pack_torch
from .losses import build_loss
from .pose_head import NOC_MEANS, NOC_STDS

UPSAMPLE_TYPES = (None, 'deconv', 'nearest', 'bilinear', 'carafe')


class ConvReLU(nn.Module):
    """What mmcv's ``ConvModule`` is with ``conv_cfg=None, norm_cfg=None`` and its default activation: ``conv`` (with bias), then ReLU."""

    def __init__(self, in_channels, out_channels, kernel_size, padding=0):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, padding=padding)
        self.activate = nn.ReLU(inplace=True)
        nn.init.kaiming_normal_(self.conv.weight, a=0, mode='fan_out', nonlinearity='relu')        # ConvModule.init_weights
        nn.init.constant_(self.conv.bias, 0)

    def forward(self, x):
        return self.activate(self.conv(x))


def build_coord_coder(cfg):
    cfg = dict(cfg)
    typ = cfg.pop('type')
    if typ != 'NOCCoder':
        raise ValueError(f'unknown coord coder {typ!r}')
    return _noc_head.NOCCoder(**cfg)


class FCNNOCDecoder(nn.Module):
    """The reference's NOC head: same constructor arguments and defaults, same ``state_dict`` keys.  ``forward(x, latent_pred,
    latent_var, labels, flip=False)``: x (n, in_channels, rh, rw) RoI features, latent_pred (n, latent_channels) -> the reference's
    4-tuple ``(noc_pred (n, 3, rh s, rw s), None, proj_logstd (n, 2, rh s, rw s), None)``.  :meth:`forward_all_pred` stops at the raw
    ``all_pred`` (n, 2 Cn 5, rh s, rw s) the fused decodes take."""

    def __init__(self,
                 num_convs=3,
                 roi_feat_size=14,
                 in_channels=256,
                 conv_kernel_size=3,
                 conv_out_channels=256,
                 num_classes=3,
                 class_agnostic=False,
                 upsample_cfg=dict(type='carafe', scale_factor=2, up_kernel=5, up_group=1, encoder_kernel=3, encoder_dilation=1,
                                   compressed_channels=64),
                 num_convs_upsampled=1,
                 conv_cfg=None,
                 norm_cfg=None,
                 loss_noc=None,
                 noc_channels=3,
                 uncert_channels=2,
                 dropout2d_rate=0.2,
                 num_dropout2d_layers=1,
                 flip_correction=True,
                 plugins=None,
                 coord_coder=dict(type='NOCCoder', target_means=NOC_MEANS, target_stds=NOC_STDS, eps=1e-5),
                 use_latent_vec=True,
                 latent_activation=None,
                 latent_channels=16):
        super().__init__()
        self.upsample_cfg = dict(upsample_cfg)
        if self.upsample_cfg['type'] not in UPSAMPLE_TYPES:
            raise ValueError(f'Invalid upsample method {self.upsample_cfg["type"]}, accepted methods are "deconv", "nearest", "bilinear", "carafe"')
        if conv_cfg is not None or norm_cfg is not None:
            raise NotImplementedError('FCNNOCDecoder: conv_cfg and norm_cfg other than None need mmcv\'s ConvModule builders')
        if plugins is not None:
            raise NotImplementedError('FCNNOCDecoder: plugins need mmcv\'s build_plugin_layer')
        if self.upsample_cfg['type'] == 'deconv':
            raise NotImplementedError('FCNNOCDecoder: the deconv upsampler needs mmcv\'s build_upsample_layer (and the reference\'s forward '
                                      'calls a self.relu it never defines on that branch)')
        assert num_convs > 0
        self.num_convs = num_convs
        self.roi_feat_size = _pair(roi_feat_size)           # reserved and not used, as in the reference
        self.in_channels = in_channels
        self.conv_kernel_size = conv_kernel_size
        self.conv_out_channels = conv_out_channels
        self.upsample_method = self.upsample_cfg.get('type')
        self.scale_factor = self.upsample_cfg.pop('scale_factor', None)
        self.num_convs_upsampled = num_convs_upsampled
        self.num_classes = num_classes
        self.class_agnostic = class_agnostic
        self.conv_cfg = conv_cfg
        self.norm_cfg = norm_cfg
        self.fp16_enabled = False
        self.loss_noc = build_loss(loss_noc) if loss_noc is not None else None
        self.flip_correction = flip_correction
        self.with_plugins = False
        self.noc_channels = noc_channels
        self.uncert_channels = uncert_channels
        self.channel_per_class = noc_channels + uncert_channels
        self.coord_coder = build_coord_coder(coord_coder)
        self.use_latent_vec = use_latent_vec
        self.latent_activation = nn.ReLU() if latent_activation == 'ReLU' else nn.LeakyReLU() if latent_activation == 'LeakyReLU' else None
        if self.use_latent_vec:
            self.latent_decoder = nn.Linear(latent_channels, conv_out_channels)

        padding = (conv_kernel_size - 1) // 2
        self.convs = nn.ModuleList(ConvReLU(in_channels if i == 0 else conv_out_channels, conv_out_channels, conv_kernel_size, padding=padding)
                                   for i in range(num_convs))
        cfg = {k: v for k, v in self.upsample_cfg.items() if k != 'type'}
        if self.upsample_method is None:
            self.upsample = None
        elif self.upsample_method == 'carafe':
            self.upsample = CARAFEPack(channels=conv_out_channels, scale_factor=self.scale_factor, **cfg)
        else:
            self.upsample = nn.Upsample(scale_factor=self.scale_factor, mode=self.upsample_method,
                                        align_corners=None if self.upsample_method == 'nearest' else False, **cfg)
        self.convs_upsampled = nn.ModuleList(ConvReLU(conv_out_channels, conv_out_channels, conv_kernel_size, padding=padding)
                                             for _ in range(num_convs_upsampled))
        final_out_channels = self.channel_per_class if class_agnostic else self.channel_per_class * num_classes
        if flip_correction:
            final_out_channels *= 2
        self.conv_final = nn.Conv2d(conv_out_channels, final_out_channels, 1)
        self.use_dropout2d = dropout2d_rate > 0
        if self.use_dropout2d:
            self.dropout2d = nn.Dropout2d(dropout2d_rate)
        self.num_dropout2d_layers = num_dropout2d_layers

    def init_weights(self):
        for m in (self.upsample, self.conv_final):
            if m is None or isinstance(m, nn.Upsample):
                continue
            if isinstance(m, CARAFEPack):
                m.init_weights()
            else:
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
                nn.init.constant_(m.bias, 0)
        if self.use_latent_vec:
            nn.init.constant_(self.latent_decoder.weight, 0)
            nn.init.constant_(self.latent_decoder.bias, 0)

    def forward_all_pred(self, x, latent_pred, latent_var=None):
        """The trunk alone: the raw ``all_pred`` (n, [2] Cn 5, rh s, rw s) of ``conv_final``, before the flip branch and the class
        slice — what ``pose_head.noc_decode`` / ``pose_from_head`` and ``noc_head.decode_for_training`` take.  With no RoIs the
        reference's branch: the upsampler sees one all-zero RoI (plus ``x.sum()``, a zero that keeps the graph to the parameters) and
        its result is sliced empty again; the HIP path launches nothing (the dummy RoI runs the torch restatement)."""
        if self.use_dropout2d and self.num_dropout2d_layers > 0:
            x = self.dropout2d(x)
        for i, conv in enumerate(self.convs):
            x = conv(x)
            if self.use_dropout2d and i + 1 < self.num_dropout2d_layers:
                x = self.dropout2d(x)
        if self.use_latent_vec:
            if self.latent_activation is not None:
                latent_pred = self.latent_activation(latent_pred)
            x = x + self.latent_decoder(latent_pred)[..., None, None]
        n, c, h, w = x.size()
        if n == 0:
            x = x.new_zeros((1, c, h, w)) + x.sum()
        if self.upsample is not None:
            if n == 0 and isinstance(self.upsample, CARAFEPack):
                up = self.upsample
                x = carafe_pack_torch(x, up.encode(x), up.up_kernel, up.up_group, up.scale_factor)
            else:
                x = self.upsample(x)
        if n == 0:
            x = x[:0]
        for conv_upsampled in self.convs_upsampled:
            x = conv_upsampled(x)
        return self.conv_final(x)

    def forward(self, x, latent_pred, latent_var, labels, flip=False):
        all_pred = self.forward_all_pred(x, latent_pred, latent_var)
        if self.flip_correction:
            all_pred = all_pred.view(all_pred.size(0), 2, all_pred.size(1) // 2, all_pred.size(2), all_pred.size(3))
            if isinstance(flip, bool):
                all_pred = all_pred[:, 0] if not flip else all_pred[:, 1]
            else:
                inds = torch.arange(0, all_pred.size(0), dtype=torch.long, device=all_pred.device)
                all_pred = all_pred[inds, torch.as_tensor(flip, device=all_pred.device).long()]
        noc_pred, noc_var, proj_logstd = self.slice_pred(all_pred, labels)
        return noc_pred, noc_var, proj_logstd, None

    def slice_pred(self, all_pred, labels):
        """The class's channels of a flip-selected prediction (n, Cn 5, h, w): (noc_pred (n, 3, h, w), None, proj_logstd (n, 2, h, w))."""
        cn = 1 if self.class_agnostic else self.num_classes
        all_noc_pred, all_proj_logstd = all_pred.split([self.noc_channels * cn, self.uncert_channels * cn], dim=1)
        if self.class_agnostic:
            return all_noc_pred, None, all_proj_logstd
        n, _, h, w = all_noc_pred.size()
        inds = torch.arange(0, n, dtype=torch.long, device=all_noc_pred.device)
        noc_pred = all_noc_pred.view(n, self.num_classes, 3, h, w)[inds, labels]
        proj_logstd = all_proj_logstd.view(n, self.num_classes, self.uncert_channels, h, w)[inds, labels]
        return noc_pred, None, proj_logstd

    def get_targets(self, sampling_results, gt_coords_3d, gt_coords_3d_mask, gt_bboxes_3d, rcnn_train_cfg, img_metas):
        return _noc_head.get_targets(sampling_results, gt_coords_3d, gt_coords_3d_mask, gt_bboxes_3d, rcnn_train_cfg, img_metas,
                                     coord_coder=self.coord_coder)

    def loss(self, noc_pred, noc_targets, noc_weights):
        return _noc_head.loss(noc_pred, noc_targets, noc_weights, self.loss_noc)


def register_with_mmdet():
    """Put :class:`FCNNOCDecoder` into mmdet's ``HEADS`` registry, so that ``noc_head=dict(type='FCNNOCDecoder', ...)`` of a config
    resolves here; False without mmdet, or when a class of that name (the reference's) is registered already."""
    try:
        from mmdet.models.builder import HEADS
    except Exception:
        return False
    if HEADS.get('FCNNOCDecoder') is not None:
        return False
    HEADS.register_module(module=FCNNOCDecoder)
    return True


register_with_mmdet()
