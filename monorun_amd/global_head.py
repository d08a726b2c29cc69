"""The global head (N9): ``FCExtractor`` and ``FCExtractorMonteCarlo`` of the reference
(monorun/models/roi_heads/bbox_3d_heads/global_extractors/fc_extractor.py, fc_extractor_monte_carlo.py) with its
``MultiClassNormDimCoder`` (monorun/core/bbox_3d/dim_coder/multiclass_norm_dim_coder.py), without mmdet.  It is the first stage of
the RoI head's tail: its ``dim`` / ``dim_var`` feed ``noc_decode`` / ``pose_from_head`` and its ``reg_fc_out`` feeds ``score_poses``.

Training mode is torch ops (``nn.Dropout2d`` / ``nn.Dropout``; there is no HIP backward).  In eval mode the Monte-Carlo head draws
``num_samples`` dropout masks per RoI, explicitly (``draw_masks``), and ``mc_forward`` evaluates the samples: on a HIP device in the
configuration every shipped config uses, through ``mr_global_head_mc_forward`` (include/monorun_global.h), which factors the first
layer over the channel mask so that the 50 samples of a RoI share one product with W1; otherwise through ``mc_forward_torch``,
the reference's sequence of ops with the same masks.
"""
import torch
import torch.nn as nn
from torch.nn.modules.utils import _pair

from . import _lib
from .losses import build_loss

MAX_CHANNELS, MAX_OUT, MAX_SAMPLES = 8192, 4096, 4096       # MR_GLOBAL_MAX_* of include/monorun_global.h
CHUNK = 64                                                   # MR_GLOBAL_CHUNK: RoIs per pass of the HIP path

DIM_MEANS = [(3.89, 1.53, 1.62), (0.82, 1.78, 0.63), (1.77, 1.72, 0.57)]        # car, pedestrian, cyclist
DIM_STDS = [(0.44, 0.14, 0.11), (0.25, 0.13, 0.12), (0.15, 0.10, 0.14)]


class MultiClassNormDimCoder:
    """Dimensions <-> per-class normalised dimensions: ``(dimensions - mean[label]) / std[label]`` and back; a variance scales by
    ``std[label]**2``."""

    def __init__(self, target_means=DIM_MEANS, target_stds=DIM_STDS):
        assert len(target_means) == len(target_stds)
        self.target_means = target_means
        self.target_stds = target_stds

    def encode(self, dimensions, labels):
        target_means = dimensions.new_tensor(self.target_means)
        target_stds = dimensions.new_tensor(self.target_stds)
        return dimensions.sub(target_means[labels]).div(target_stds[labels])

    def decode(self, dim, dim_var, labels):
        target_means = dim.new_tensor(self.target_means)[labels]
        target_stds = dim.new_tensor(self.target_stds)[labels]
        dimensions = dim * target_stds + target_means
        dimensions_var = dim_var * target_stds.square() if dim_var is not None else None
        return dimensions, dimensions_var


# 'MultiClassNormCoder' is the name in the reference's constructor default (no registry of the reference knows it; every config file
# passes 'MultiClassNormDimCoder'): here the default builds the same coder
DIM_CODERS = {'MultiClassNormDimCoder': MultiClassNormDimCoder, 'MultiClassNormCoder': MultiClassNormDimCoder}


def build_dim_coder(cfg):
    cfg = dict(cfg)
    typ = cfg.pop('type')
    if typ not in DIM_CODERS:
        raise ValueError(f'unknown dim coder {typ!r}')
    return DIM_CODERS[typ](**cfg)


class FCExtractor(nn.Module):
    """The reference's global extractor: same constructor arguments and defaults, same ``state_dict`` keys, shapes and order
    (``fcs.N.weight``, ``fcs.N.bias``, ``fc_reg.weight``, ``fc_reg.bias``), so ``roi_head.global_head.*`` of a MonoRUn checkpoint loads
    with ``strict=True``.  ``forward(x)``: x (n, in_channels, rh, rw) -> (dim_latent_pred (n, out), None, None, None, the last
    hidden layer (n, fc_out_channels))."""

    def __init__(self,
                 with_dim=True,
                 with_latent_vec=True,
                 latent_channels=16,
                 num_fcs=2,
                 in_channels=256,
                 fc_out_channels=1024,
                 num_classes=3,
                 roi_feat_size=7,
                 latent_class_agnostic=False,
                 loss_dim=dict(type='SmoothL1Loss', loss_weight=1.0, beta=1.0),
                 dim_coder=dict(type='MultiClassNormCoder', target_means=DIM_MEANS, target_stds=DIM_STDS),
                 dropout_rate=0.5,
                 dropout2d_rate=0.2,
                 num_dropout_layers=2):
        super().__init__()
        self.with_dim = with_dim
        self.with_latent_vec = with_latent_vec
        self.dim_dim = 3
        self.latent_channels = latent_channels if self.with_latent_vec else 0
        self.roi_feat_size = _pair(roi_feat_size)
        self.roi_feat_area = self.roi_feat_size[0] * self.roi_feat_size[1]
        self.in_channels = in_channels
        self.fc_out_channels = fc_out_channels
        self.num_classes = num_classes
        self.latent_class_agnostic = latent_class_agnostic
        self.loss_dim = build_loss(loss_dim) if self.with_dim else None
        self.dim_coder = build_dim_coder(dim_coder)
        self.relu = nn.ReLU(inplace=True)
        self.fp16_enabled = False
        self.dropout_rate = dropout_rate
        self.dropout2d_rate = dropout2d_rate
        self.use_dropout = dropout_rate > 0
        self.use_dropout2d = dropout2d_rate > 0
        self.num_dropout_layers = num_dropout_layers

        assert num_fcs > 0
        self.num_fcs = num_fcs
        self.fcs = nn.ModuleList(nn.Linear(self.in_channels * self.roi_feat_area if i == 0 else self.fc_out_channels, self.fc_out_channels)
                                 for i in range(num_fcs))
        out_dim_reg = self.dim_dim + self.latent_channels
        if not self.latent_class_agnostic:
            out_dim_reg *= self.num_classes
        self.out_channels = out_dim_reg
        self.fc_reg = nn.Linear(self.fc_out_channels, out_dim_reg)
        if self.use_dropout:
            self.dropout = nn.Dropout(dropout_rate)
        if self.use_dropout2d:
            self.dropout2d = nn.Dropout2d(dropout2d_rate)

    def init_weights(self):
        for m in self.fcs.modules():
            if isinstance(m, nn.Linear):
                nn.init.xavier_uniform_(m.weight, gain=0.33)
                nn.init.normal_(m.bias, mean=0.02, std=0.04)
        nn.init.normal_(self.fc_reg.weight, 0, 0.001)
        nn.init.constant_(self.fc_reg.bias, 0)

    def forward(self, x):
        if self.use_dropout2d:
            x = self.dropout2d(x)
        x = x.flatten(1)
        for i, fc in enumerate(self.fcs):
            x = self.relu(fc(x))
            if self.use_dropout and i < self.num_dropout_layers:
                x = self.dropout(x)
        return self.fc_reg(x), None, None, None, x

    def _get_dim_target_single(self, pos_assigned_gt_inds, gt_bboxes_3d, gt_labels):
        dimensions = gt_bboxes_3d[pos_assigned_gt_inds, :3]
        labels = gt_labels[pos_assigned_gt_inds]
        return self.dim_coder.encode(dimensions, labels)

    def get_targets(self, sampling_results, gt_bboxes_3d, gt_labels, concat=True):
        """(dim_targets, None): the encoded dimensions of every sampled positive's ground-truth box, per image, concatenated with
        ``concat``.  ``sampling_results``: objects with ``pos_assigned_gt_inds``."""
        pos_assigned_gt_inds = [res.pos_assigned_gt_inds for res in sampling_results]
        if self.loss_dim is not None:
            dim_targets = [self._get_dim_target_single(*args) for args in zip(pos_assigned_gt_inds, gt_bboxes_3d, gt_labels)]
            if concat:
                dim_targets = torch.cat(dim_targets, dim=0)
        else:
            dim_targets = None
        return dim_targets, None

    def _slice(self, t, labels):
        if self.latent_class_agnostic:
            return t
        inds = torch.arange(len(labels), device=labels.device)
        width = self.dim_dim + self.latent_channels
        return t.view(t.size(0), t.size(1) // width, width)[inds, labels]          # stated: with no rows a -1 is ambiguous

    def slice_pred(self, dim_latent_pred, dim_latent_var, labels):
        """-> (dim_pred (n, 3), None, latent_pred (n, latent_channels), None): the class's slice of the prediction."""
        dim_pred, latent_pred = self._slice(dim_latent_pred, labels).split([self.dim_dim, self.latent_channels], dim=1)
        return dim_pred, None, latent_pred, None

    def loss(self, dim_pred, distance_pred, distance_logstd, dim_targets, distance_targets):
        losses = dict()
        if self.loss_dim is not None:
            if dim_pred.size(0) == 0:
                losses['loss_dim'] = dim_pred.sum()
            else:
                losses['loss_dim'] = self.loss_dim(dim_pred.float(), dim_targets)
        return losses


class _McDropout2d(nn.Dropout2d):
    def forward(self, input):
        return nn.functional.dropout2d(input, self.p, True, self.inplace)


class _McDropout(nn.Dropout):
    def forward(self, input):
        return nn.functional.dropout(input, self.p, True, self.inplace)


class FCExtractorMonteCarlo(FCExtractor):
    """The reference's Monte-Carlo dropout head.  Training mode is :class:`FCExtractor`'s forward.  Eval mode evaluates ``num_samples``
    dropout samples of every RoI (sample row ``s * n + i``) and returns ``(mean over s of dim_latent_pred, its unbiased variance,
    None, None, mean over s of the last hidden layer after dropout)``; ``forward`` draws the masks with torch's generator
    (``draw_masks``) and calls ``mc_forward``."""

    def __init__(self, num_samples=50, dropout_rate=0.5, dropout2d_rate=0.2, **kwargs):
        super().__init__(dropout_rate=dropout_rate, dropout2d_rate=dropout2d_rate, **kwargs)
        self.num_samples = num_samples
        assert self.use_dropout
        self.dropout = _McDropout(dropout_rate)
        assert self.use_dropout2d
        self.dropout2d = _McDropout2d(dropout2d_rate)

    def forward(self, x):
        if self.training:
            return super().forward(x)
        return self.mc_forward(x)

    def slice_pred(self, dim_latent_pred, dim_latent_var, labels):
        """Eval mode: (dim_pred, dim_var, latent_pred, latent_var), the class's slice of the mean and of the variance."""
        if self.training:
            return super().slice_pred(dim_latent_pred, dim_latent_var, labels)
        sizes = [self.dim_dim, self.latent_channels]
        dim_pred, latent_pred = self._slice(dim_latent_pred, labels).split(sizes, dim=1)
        dim_var, latent_var = self._slice(dim_latent_var, labels).split(sizes, dim=1)
        return dim_pred, dim_var, latent_pred, latent_var

    # --------------------------------------------------------------------------------------------- the Monte-Carlo samples
    def draw_masks(self, n, device, generator=None):
        """The dropout draws of ``num_samples`` samples of ``n`` RoIs, True = kept: ``keep0 (S, n, in_channels)`` with probability
        ``1 - dropout2d_rate`` (dropout2d: a whole channel), ``keep1 (S, n, F)`` and ``keep2 (S, n, F)`` with ``1 - dropout_rate``,
        from torch's generator (``generator`` or the device's default).  The same seed gives the same masks; they are not the
        draws ``F.dropout`` would make from that seed (the distribution is the same)."""
        S, F = self.num_samples, self.fc_out_channels

        def keep(width, rate):
            return torch.rand(S, n, width, device=device, generator=generator) >= rate
        return keep(self.in_channels, self.dropout2d_rate), keep(F, self.dropout_rate), keep(F, self.dropout_rate)

    def mc_forward_torch(self, x, masks, return_samples=False):
        """The reference's eval-mode sequence of ops with ``input * (keep / (1 - p))`` in place of each dropout: any device and
        dtype, any ``num_fcs`` (``masks``: keep0 and one mask per dropout layer), differentiable."""
        S = self.num_samples
        n = x.size(0)
        x = x.repeat(S, 1, 1, 1)
        x = x * (masks[0].reshape(S * n, self.in_channels, 1, 1).to(x.dtype) / (1 - self.dropout2d_rate))
        x = x.flatten(1)
        for i, fc in enumerate(self.fcs):
            x = self.relu(fc(x))
            if i < self.num_dropout_layers:
                x = x * (masks[1 + i].reshape(S * n, x.size(1)).to(x.dtype) / (1 - self.dropout_rate))
        pred = self.fc_reg(x).view(S, -1, self.out_channels)
        var, mean = torch.var_mean(pred, dim=0)
        out = (mean, var, None, None, torch.mean(x.view(S, -1, x.size(1)), dim=0))
        return out + (pred,) if return_samples else out

    def hip_ok(self, x):
        """Whether ``mr_global_head_mc_forward`` covers this call: CUDA fp32 contiguous (n, in_channels, rh, rw), two FC layers with
        a dropout each, rates in (0, 1), sizes within include/monorun_global.h, and no graph to keep."""
        if not (x.device.type == 'cuda' and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()):
            return False
        if x.size(1) != self.in_channels or x.size(2) * x.size(3) != self.roi_feat_area:
            return False
        if not (self.num_fcs == 2 and self.num_dropout_layers == 2 and 0 < self.dropout_rate < 1 and 0 < self.dropout2d_rate < 1):
            return False
        params = list(self.parameters())
        if any(p.device != x.device or p.dtype != torch.float32 for p in params):
            return False
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
            return False
        n, S, C, A, F, J = x.size(0), self.num_samples, self.in_channels, self.roi_feat_area, self.fc_out_channels, self.out_channels
        lim = 2 ** 31 - 1
        return (2 <= S <= MAX_SAMPLES and max(C, A, F) <= MAX_CHANNELS and J <= MAX_OUT
                and max(n * C * A, F * C * A, S * n * F, S * n * C, S * n * J) <= lim)

    def workspace_numel(self, n):
        """fp32 elements of workspace the HIP path needs for ``n`` RoIs (``mr_global_head_mc_workspace_bytes`` / 4): one pass of
        ``min(n, CHUNK)`` RoIs, so it stops growing at ``CHUNK``."""
        lib = _lib.load()
        sizes = dict(n=n, in_channels=self.in_channels, area=self.roi_feat_area, fc_channels=self.fc_out_channels,
                     out_channels=self.out_channels, num_samples=self.num_samples)
        return lib.mr_global_head_mc_workspace_bytes(*_lib.pack('mr_global_head_mc_workspace_bytes', sizes)) // 4

    def mc_forward(self, x, masks=None, generator=None, return_samples=False):
        """The eval-mode forward on given masks (``draw_masks`` when None): the reference's 5-tuple, and with ``return_samples`` a sixth
        element, the samples ``(S, n, out)`` the mean and variance are taken over.  Runs the HIP path when ``hip_ok(x)``, else
        :meth:`mc_forward_torch`.  n = 0 returns the empties ``(0, out)``, ``(0, out)``, ``(0, F)`` without a launch."""
        n = x.size(0)
        if n == 0:
            out = (x.new_empty(0, self.out_channels), x.new_empty(0, self.out_channels), None, None, x.new_empty(0, self.fc_out_channels))
            return out + (x.new_empty(self.num_samples, 0, self.out_channels),) if return_samples else out
        if masks is None:
            masks = self.draw_masks(n, x.device, generator)
        if self.hip_ok(x):
            return self.mc_forward_hip(x, masks, return_samples)
        return self.mc_forward_torch(x, masks, return_samples)

    def mc_forward_hip(self, x, masks, return_samples=False, workspace=None, out=None):
        """The HIP path itself; a call it does not cover (``hip_ok``) is an error, never a fall-back.  ``workspace``: an fp32 tensor
        of at least ``workspace_numel(n)`` elements on ``x``'s device (allocated when None); ``out``: a dict of preallocated
        contiguous fp32 ``mean``, ``var``, ``reg_fc_out`` and, with ``return_samples``, ``samples`` to write into."""
        if x.size(0) == 0 or not self.hip_ok(x):
            raise RuntimeError('mc_forward_hip: mr_global_head_mc_forward does not cover this call (hip_ok() is False, or n = 0)')
        lib = _lib.load()
        dev = x.device
        n, S, C, A, F, J = x.size(0), self.num_samples, self.in_channels, self.roi_feat_area, self.fc_out_channels, self.out_channels
        keep = []
        for m, width in zip(masks, (C, F, F)):
            if m.shape != (S, n, width):
                raise ValueError(f'mc_forward: a mask of shape {tuple(m.shape)}, expected {(S, n, width)}')
            keep.append(m.to(device=dev, dtype=torch.bool).contiguous().view(torch.uint8))
        f32 = dict(device=dev, dtype=torch.float32)
        w = [t.detach().contiguous() for t in (self.fcs[0].weight, self.fcs[0].bias, self.fcs[1].weight, self.fcs[1].bias,
                                               self.fc_reg.weight, self.fc_reg.bias)]
        out = dict(out or {})
        shapes = dict(mean=(n, J), var=(n, J), reg_fc_out=(n, F), samples=(S, n, J))
        for k in ('mean', 'var', 'reg_fc_out') + (('samples',) if return_samples else ()):
            t = out.setdefault(k, torch.empty(shapes[k], **f32))
            if t.shape != shapes[k] or t.dtype != torch.float32 or t.device != dev or not t.is_contiguous():
                raise ValueError(f'mc_forward_hip: out[{k!r}] must be a contiguous fp32 {shapes[k]} tensor on {dev}')
        mean, var, reg, samples = out['mean'], out['var'], out['reg_fc_out'], out['samples'] if return_samples else None
        sizes = dict(n=n, in_channels=C, area=A, fc_channels=F, out_channels=J, num_samples=S)
        nbytes = 4 * self.workspace_numel(n)
        work = workspace if workspace is not None else torch.empty(nbytes // 4, **f32)
        if work.dtype != torch.float32 or work.device != dev or not work.is_contiguous() or work.numel() * 4 < nbytes:
            raise ValueError(f'mc_forward_hip: the workspace must be a contiguous fp32 tensor of at least {nbytes // 4} elements on {dev}')
        with torch.cuda.device(dev):
            _lib.call('mr_global_head_mc_forward', sizes, x=x.detach().data_ptr(), w1=w[0].data_ptr(), b1=w[1].data_ptr(), w2=w[2].data_ptr(),
                      b2=w[3].data_ptr(), w_reg=w[4].data_ptr(), b_reg=w[5].data_ptr(), keep0=keep[0].data_ptr(), keep1=keep[1].data_ptr(),
                      keep2=keep[2].data_ptr(), q0=1.0 / (1.0 - self.dropout2d_rate), q1=1.0 / (1.0 - self.dropout_rate), workspace=work.data_ptr(),
                      workspace_bytes=nbytes, mean=mean.data_ptr(), var=var.data_ptr(), reg_fc_out=reg.data_ptr(), samples=_lib.ptr(samples),
                      stream=torch.cuda.current_stream(dev).cuda_stream)
        out = (mean, var, None, None, reg)
        return out + (samples,) if return_samples else out
